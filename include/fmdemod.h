/* fmdemod.h — C ABI of the MI355X-native batched broadcast-FM demodulator (libfmdemod.so).
 *
 * Drop-in boundary for the demodulator API of williamyang98/FM-Radio (reference src/fm_demod):
 * one fmd_handle is C independent `Broadcast_FM_Demod` instances (reference
 * src/fm_demod/broadcast_fm_demod.h:91-299) advanced in lock-step on one GPU.  Every entry point
 * names the reference member it replaces.  Plain pointers and sizes only; no C++ / torch types.
 *
 * Threading (same contract as the reference): one caller thread per handle.
 *
 * Output lifetime — ONE rule for every output view and getter (fmd_audio_dev, fmd_rds_dev, fmd_get_*): the outputs of a
 * block stay valid while at most FMD_OUTPUT_LIFETIME_BLOCKS (= 5) further fmd_process_* calls have been made on the handle;
 * the call after that reuses the block's buffers.  (The reference keeps one block: "valid until the next Process",
 * broadcast_fm_demod.h:242-256.)  A consumer that may fall further behind tells the library so with
 * fmd_release_outputs(): the library then orders the reuse behind the consumer's stream.
 *
 * Data layouts (channel-major, time contiguous per channel):
 *   IQ in      cf32 [C][N][2] float  (or u8 [C][N][2], RTL-SDR style, converted as `(float)u8 - 127`,
 *              reference src/app.cpp:56-62)
 *   audio out  f32  [C][N_audio][2]  interleaved L,R   (reference Frame<float>, src/audio/frame.h:6-8)
 *   RDS syms   f32  [C][N_rds]  first counts[c] entries valid (reference GetRDSPredSymbols(), .h:253)
 */
#ifndef FMDEMOD_H
#define FMDEMOD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMD_API_VERSION 3
/* further fmd_process_* calls during which a block's outputs stay valid (see the lifetime rule above) */
#define FMD_OUTPUT_LIFETIME_BLOCKS 5

typedef struct fmd_handle_s* fmd_handle;

enum {
    FMD_OK = 0,
    FMD_ERR_ARG = -1,        /* bad argument / unsupported configuration */
    FMD_ERR_SIZE = -2,       /* n_samples != block_size or n_channels mismatch: block dropped, nothing emitted
                                (reference Process(): silent return, broadcast_fm_demod.cpp:311-313) */
    FMD_ERR_DEVICE = -3,     /* HIP runtime error, see fmd_last_error */
    FMD_ERR_NO_DEVICE = -4,  /* no usable MI355X: the library has NO CPU fallback */
    FMD_ERR_NAME = -5,       /* unknown stream name */
    FMD_ERR_STATE = -6       /* an earlier fmd_process_* call failed part-way (or the pilot-PLL hand-over watchdog fired): the
                                per-channel state is no longer the state after a whole number of blocks; call fmd_reset */
};

/* reference Broadcast_FM_Demod_Controls::AudioOut (broadcast_fm_demod.h:80) */
enum { FMD_AUDIO_LPR = 0, FMD_AUDIO_LMR = 1, FMD_AUDIO_STEREO = 2 };

/* reference Broadcast_FM_Demod(int block_size) (broadcast_fm_demod.h:229) + the hard-wired
 * Fs_baseband (broadcast_fm_demod.cpp:68), made a parameter. */
typedef struct {
    int n_channels;    /* independent stations on this GPU */
    int block_size;    /* baseband samples per channel per fmd_process call; multiple of 1024*(fs_baseband/256000) */
    int fs_baseband;   /* 256000 (no first decimator), 1024000 (reference), 2048000 */
    int device;        /* HIP device ordinal, -1 = current */
    unsigned flags;    /* FMD_FLAG_* */
} fmd_config;

#define FMD_FLAG_KEEP_TAPS   1u  /* keep the intermediate streams readable through fmd_get_stream */
#define FMD_FLAG_NO_PIPELINE 2u  /* run every stage on the caller's stream, one after the other (debugging / profiling) */
#define FMD_FLAG_PLL_TIME_PARALLEL 4u  /* force the time-parallel pilot-PLL kernel (default: batches <= 7168 stations — the station count itself at every rate, not the effective batch of FMD_FLAG_PLL_K8 — and larger ones while stations are out of pilot lock) */
#define FMD_FLAG_PLL_K8           16u  /* time-parallel kernel with 8 (not 16) lanes per channel whatever the batch size (default: effective batches (stations, x 1.5 at 1.024 and 2.048 MSa/s) > 3584; up to 4096 stations 16 lanes all the same while stations are out of pilot lock) */
#define FMD_FLAG_PLL_STREAM_ORDER  32u  /* consecutive blocks' pilot-PLL launches ordered by the stream (kernel boundary) instead of handing over per wavefront while both run (A/B and debugging; same results) */
#define FMD_FLAG_PLL_LOW_WORK      8u  /* force the low-work pilot-PLL kernel (default: larger batches); same results either way */
/* Tolerance mode.  Default (flag clear): every output is bit-identical to the CPU restatement of the reference (oracle/) — the
 * reference's operation order, libm's atan2f, a pilot PLL advanced sample by sample.  That contract has a price the caller should
 * know: a station WITHOUT a lockable pilot (mono station, empty channel, dead input) cannot be advanced under the locked loop's
 * "the frequency word stays put" speculation; its wavefront speculates on the SEQUENCE of words instead (round 6; the serial
 * 78-operation iteration before, ~4x), at about 1.4x a locked wavefront's time, and one such wavefront sets the kernel's duration:
 * 0.89 -> 1.06-1.20 ms per 4096-station block from 1 % unlocked stations on (small batches, where that
 * kernel's latency is the step, pay ~1.5x): a band scan,
 * where most channels are empty, still wants the tolerance mode, whose cost does not depend on lock at all.
 * With the flag the chain keeps the reference's signal flow and state variables but uses cheaper arithmetic: minimax arctangent,
 * hardware sine/cosine, the FIRs as bf16 x 3 products on the matrix cores (fp32 accumulation, ~1e-6 relative), the pilot peak filter
 * as the complex one-pole low-pass of the down-mixed signal that it is, decimated by 16, the pilot PLL advanced 128 samples at a time
 * from the phase at 8 points of the span (the NCO frequency held over the span, the feedback inside it solved exactly on the host),
 * the optional de-emphasis inside the front-end tile (time constants up to ~79 us), and (round 5) the 38 / 57 kHz mixers BEHIND their
 * decimating FIRs: the carrier part of the NCO phase and the Hilbert FIR folded into one complex band-pass FIR per rail, the loop's
 * slow deviation applied once per OUTPUT at the FIR window's centre (the RDS rails with a first-order term in its slope; the L-R rail
 * without: 4e-6 per Hz of NCO offset, i.e. < 1e-5 for a pilot within +-2 Hz of 19 kHz and < 1e-3 for a loop on its +-100 Hz rail).
 * Parity, as tests/test_gpu_fast.py, test_gpu_long.py and test_gpu_realistic.py assert it and profiles/round5/parity_metrics.json records it:
 *   audio, L-R   every block within 1e-4 RMS of the oracle except right behind a sign decision of the reference's L-R phase tracker that
 *                falls on the other side (the allowance is the measured offset difference).  In lock, 64 stations x 30 s: whole-run RMS
 *                <= 2.7e-5 (audio) / 1.4e-5 (L-R) on every station, ONE station-block of 30 016 above 1e-4 (2.7e-4, behind such a decision:
 *                102 of them, 0.053 per station-second; two builds of the reference itself: 0.008-0.042, profiles/round4/reference_flip_evidence.json).
 *                ACQUISITION: over a station's first 0.77 s the whole-run figures are 1.6e-4 (L-R) / 3.1e-4 (audio) on captures whose first
 *                phase estimates flip (4 on 5 stations) — inside the allowance, not inside 1e-4; without flips 1.1e-5 / 2.3e-5.
 *                REALISTIC CAPTURES (noise-like pre-emphasised programme to 15 kHz, L != R, 32 stations x 10 s per condition, u8): CNR 40 /
 *                25 dB, 50 us, carrier +-30 kHz, 110 kHz deviation, pilot +2 Hz, Rician fading, an adjacent station at -20 dB (1.024 MSa/s):
 *                L-R <= 1.2e-5, audio <= 2.9e-5 whole-run in lock on the worst station, L+R <= 2.3e-6; CNR 15 dB: 5.3e-5 / 1.1e-4 (noise moves
 *                single phase estimates in both evaluations).
 *   u8 captures  in a deep fade (a few LSB of signal) consecutive samples fall in exactly opposite directions and the reference's wrap of
 *                a phase difference of exactly pi turns on the last bit of glibc's atan2f — a click of one full turn either way.  The mode
 *                takes the reference's decision from a table made with the exact atan2f (256 kSa/s captures; behind the first decimator
 *                the samples are no longer integers).  Found by the fading condition: L+R 3.4e-3 before, 5.9e-7 with the table.
 *   RDS bits     identical once the synchroniser is in lock (fmd_get_rds_bytes), every station — also on every realistic condition where the
 *                subcarrier stays above the noise; at CNR 15 dB and through fades single symbols are the noise's in either evaluation: the
 *                same groups decode (>= 96 % of the oracle's count on the worst station) and >= 97 % of the bits agree chunk by chunk.
 *   RDS symbols  (fmd_get_rds_symbols, the reference's OnRDSOut payload) the typical symbol within 1.2e-5 and the typical station within
 *                2.6e-5 RMS of the oracle; 0.14 % of the symbols move by 0.1-0.3 where a zero-crossing / clock-wrap decision of the
 *                synchroniser tips (the sign, i.e. the bit, stays) - the reference's own two builds move 1.4 % of theirs; the symbols that
 *                do not move: p99 3.0e-3 on the worst station.  A consumer that needs the soft values inside 1e-4 on EVERY symbol wants
 *                the exact mode.
 * The cost of a block does not depend on the signals: there is no data-dependent path (a station's first 64 ms after a reset also run
 * round 3's per-sample pilot kernel, for the reference's start-up transient; the u8 tie table is consulted on a rare branch).  The
 * FMD_FLAG_PLL_* selectors are ignored.  fmd_default_config() selects this mode. */
#define FMD_FLAG_FAST_MATH        64u

/* reference Broadcast_FM_Demod_Controls (broadcast_fm_demod.h:64-89); defaults in fmd_default_controls */
typedef struct {
    int   audio_out;               /* FMD_AUDIO_* */
    float audio_stereo_mix_factor;
    int   use_deemphasis;
    int   deemphasis_tus;          /* microseconds */
    int   lpr_cutoff_hz;
    int   lmr_cutoff_hz;
} fmd_controls;

/* reference GetBasebandSampleRate() .. GetAudioSampleRate() (broadcast_fm_demod.h:284-288) + block sizes */
typedef struct {
    int fs_baseband, fs_fm_in, fs_fm_out, fs_rds, fs_audio;
    int n_baseband, n_fm_in, n_fm_out, n_rds, n_audio;
} fmd_rates;

/* Every designed coefficient the chain uses (reference filter objects, broadcast_fm_demod.cpp:127-291,
 * bpsk_synchroniser.cpp:26-48).  Same layout as oracle/fm_oracle.h:fmo_coeffs so tests can hand the
 * library's coefficients to the CPU oracle. */
typedef struct {
    int   fs_baseband, m_fm_in;
    float b_fm_in[64], b_fm_out[64], b_hilbert[65];
    float pilot_b[3], pilot_a[3];
    float pll_lpf_b[2], pll_lpf_a[2];
    float deemph_b[2], deemph_a[2];
    float b_lpr[128], b_lmr[128], b_rds[128];
    float ted_lpf_b[2], ted_lpf_a[2];
    float bpsk_lpf_b[2], bpsk_lpf_a[2];
    float fm_gain;
} fmd_coeffs;

int         fmd_api_version(void);
/* == FMD_OUTPUT_LIFETIME_BLOCKS of the library that was loaded */
int         fmd_output_lifetime_blocks(void);
const char* fmd_status_string(int status);
/* number of usable gfx950 devices; <= 0 means every other call fails with FMD_ERR_NO_DEVICE */
int         fmd_device_count(void);

void fmd_default_controls(fmd_controls* c);
/* A configuration for `n_channels` stations of `fs_baseband` with 64 ms blocks (the reference's 65536 samples at 1.024 MSa/s,
 * broadcast_fm_demod.cpp:62-77, scaled to the rate), on the current device, in the mode a many-station deployment wants:
 * FMD_FLAG_FAST_MATH (the tolerance mode above).  `flags = 0`, the bit-exact mode, is what a parity harness asks for explicitly —
 * it costs ~3x per block, and ~13x as soon as 1 % of the stations have no lockable pilot (a band scan: most channels are empty).
 * Returns FMD_ERR_ARG for an unsupported rate. */
int  fmd_default_config(fmd_config* cfg, int n_channels, int fs_baseband);

/* Broadcast_FM_Demod::Broadcast_FM_Demod (broadcast_fm_demod.cpp:59-305) x n_channels */
int fmd_create(const fmd_config* cfg, fmd_handle* out);
/* ~Broadcast_FM_Demod */
int fmd_destroy(fmd_handle h);
/* back to the freshly constructed state (zero histories, AGC gain 0.1, PLLs at rest) */
int fmd_reset(fmd_handle h);

/* GetControls() (broadcast_fm_demod.h:294): channel >= 0 addresses one station, -1 all of them.
 * Takes effect at the next block boundary, like UpdateFilters() (broadcast_fm_demod.cpp:330-389). */
int fmd_set_controls(fmd_handle h, int channel, const fmd_controls* c);
int fmd_get_controls(fmd_handle h, int channel, fmd_controls* c);
int fmd_get_rates(fmd_handle h, fmd_rates* r);
/* the configuration the handle was created with (device resolved to the ordinal in use) */
int fmd_get_config(fmd_handle h, fmd_config* cfg);
int fmd_get_coeffs(fmd_handle h, int channel, fmd_coeffs* k);

/* Broadcast_FM_Demod::Process (broadcast_fm_demod.cpp:309-328) for all channels.
 * *_dev: `d_iq` is a DEVICE pointer.  The call returns without synchronising.  The block is read after everything
 * already queued on `stream` (hipStream_t, NULL = default stream), and work queued on `stream` AFTER the call is
 * ordered behind the library's last read of `d_iq`, so the buffer may be refilled in stream order.  The stages of
 * the block run on the library's own streams and overlap with the neighbouring blocks' stages (up to six blocks in
 * flight); outputs become readable after fmd_synchronize / fmd_wait_outputs and stay valid as the lifetime rule at the
 * top of this header says.  *_host: `iq` is a host pointer; copies, runs, synchronises.
 * `d_iq` may start at any sample (8 / 2 bytes) of an allocation, as the reference's span may; blocks that start on a 16-byte
 * boundary are read fastest (16 bytes per lane).
 * A call that fails with FMD_ERR_DEVICE after some of its kernels were queued leaves the handle in FMD_ERR_STATE. */
int fmd_process_cf32_dev(fmd_handle h, const float* d_iq, int n_channels, int n_samples, void* stream);
int fmd_process_u8_dev(fmd_handle h, const uint8_t* d_iq, int n_channels, int n_samples, void* stream);
int fmd_process_cf32_host(fmd_handle h, const float* iq, int n_channels, int n_samples);
int fmd_process_u8_host(fmd_handle h, const uint8_t* iq, int n_channels, int n_samples);
/* The same blocks submitted WITHOUT touching the caller's streams (API v3) — for hosts that rotate several input buffers, as the
 * reference's device thread does with its USB buffers (src/device/device.cpp:107-119) and fm-radio_amd/host/station_ring.hpp does
 * with its staging blocks.  The block is read after everything already queued on `ready_stream` (NULL: the data is in place
 * now); nothing is queued on `ready_stream` or any other stream of the caller, so the caller's streams never wait for the
 * demodulator and consecutive blocks' first stages run back to back (fmd_process_*_dev orders the caller's stream behind the
 * library's read of every block, which also orders the next block's submission behind it: two cross-queue hand-overs, ~0.1 ms,
 * between consecutive front-end launches).  The buffer may be rewritten once fmd_wait_input() says so. */
int fmd_submit_cf32_dev(fmd_handle h, const float* d_iq, int n_channels, int n_samples, void* ready_stream);
int fmd_submit_u8_dev(fmd_handle h, const uint8_t* d_iq, int n_channels, int n_samples, void* ready_stream);
/* make `stream` wait (on the device, no host block) until the library has finished reading the input buffer of the newest
 * block submitted with fmd_submit_*_dev / fmd_process_*_dev */
int fmd_wait_input(fmd_handle h, void* stream);
int fmd_synchronize(fmd_handle h);
/* make `stream` wait (on the device, no host block) until the newest block's outputs are complete */
int fmd_wait_outputs(fmd_handle h, void* stream);
/* Which outputs the device-side calls (fmd_wait_outputs, fmd_release_outputs, fmd_audio_dev, fmd_audio_pcm16_dev, fmd_rds_dev,
 * fmd_rds_bytes_dev) refer to behind fmd_submit_*_dev in the tolerance mode.
 * Background: there, with 1024 stations' worth of 256 kSa/s blocks or more, a block's extract and RDS stages are queued when the NEXT
 * block is submitted — behind that block's front end, on the same hardware queue: the two large kernels take turns instead of sharing
 * the CUs (6 % on the step, DESIGN.md "Schedule") — or as soon as somebody needs them.
 *   on = 0 (default): the NEWEST block's outputs.  A device-side call that wants them while they are still put off queues them at
 *       once, and from then on the handle queues every block's stages at submission (a consumer that asks after every block would
 *       otherwise stall the front end's queue each time).
 *   on = 1: the newest QUEUED outputs, never forcing anything: after fmd_submit_*_dev of block k those are block k - 1's where the
 *       stages are put off, block k's otherwise — fmd_outputs_block says which (nothing before the second block at most: fmd_wait_outputs / fmd_release_outputs do nothing then, fmd_audio_pcm16_dev fails with FMD_ERR_ARG).
 *       A consumer that takes every block's outputs one submission later (bench.py's per-step gather does) keeps the faster schedule.
 * fmd_synchronize, the host getters and fmd_process_* always complete the newest block.  Synchronises; call it between blocks. */
int fmd_set_output_lag(fmd_handle h, int on);
/* which block the device-side output calls refer to right now: 0 = the first block since fmd_create / fmd_reset, -1 = none yet.
 * (Under fmd_set_output_lag(h, 1) a consumer needs it to tell k from k - 1: batches below the size named above, and the exact mode,
 * queue every block's stages at submission.) */
int fmd_outputs_block(fmd_handle h, long* block);
/* how often the handle's block numbering has restarted (fmd_create counts as the first start; every fmd_reset restarts it): a consumer
 * that follows fmd_outputs_block across resets — the multi-GPU gather does — tells a restart from a repeated or skipped block by it */
int fmd_outputs_epoch(fmd_handle h, long* epoch);
/* The consumer's side of the lifetime rule: everything queued on `stream` so far (the kernels / copies that read the newest
 * block's output views) must finish before the library overwrites those views, however many blocks are submitted meanwhile.
 * Records an event on `stream`; the library's writers of that buffer slot wait for it on the device.  Never blocks the host. */
int fmd_release_outputs(fmd_handle h, void* stream);

/* OnAudioOut() / GetAudioOut() (broadcast_fm_demod.h:256,297): device views of the current block */
int fmd_audio_dev(fmd_handle h, const float** d_audio /* [C][n_audio][2] */);
/* The newest block's audio as the 16-bit PCM frames the reference's headless scraper writes to its WAV files
 * (fm_scraper.cpp:79-82: sample * (32767 * 0.95f), truncated toward zero): d_pcm [C][n_audio][2] int16 on the device,
 * converted on `stream` once the block's outputs are complete.  Half the bytes of the f32 block: the payload of the
 * multi-GPU audio gather. */
int fmd_audio_pcm16_dev(fmd_handle h, int16_t* d_pcm /* [C][n_audio][2] */, void* stream);
/* OnRDSOut() / GetRDSPredSymbols() (broadcast_fm_demod.h:253,298) */
int fmd_rds_dev(fmd_handle h, const float** d_syms /* [C][n_rds] */, const int** d_counts /* [C] */);
/* host copies (synchronise first) */
int fmd_get_audio(fmd_handle h, float* audio /* [C][n_audio][2] */);
int fmd_get_rds_symbols(fmd_handle h, float* syms /* [C][n_rds] */, int* counts /* [C] */);

/* Parity / GUI taps, the reference's buffer getters (broadcast_fm_demod.h:242-256, :291):
 *   "fm_out_iq" GetFMOutIQ [C][n_fm_out][2] | "pll_dt" [C][n_fm_out] | "lpr" GetLPRAudioOutput [C][n_audio]
 *   "lmr" GetLMRAudioOutput [C][n_audio] | "rds" GetRDSOutput (post-AGC) [C][n_rds][2]
 *   "rds_raw_sym" GetRDSRawSymbols [C][n_rds][2] | "lmr_phase" GetAudioLMRPhaseError [C]
 *   "agc_pilot_gain" [C] | "agc_rds_gain" [C]
 *   exact mode with FMD_FLAG_KEEP_TAPS, the two loops' per-sample traces (broadcast_fm_demod.h:245-248, bpsk_synchroniser.h:78-85):
 *   "pilot" GetPilotOutput (after its AGC) [C][n_fm_out][2] | "pll" GetPLLOutput (cos, sin) [C][n_fm_out][2]
 *   "pll_raw_err" Get_PLL_Raw_Phase_Error_Output [C][n_fm_out] | "pll_pi_err" Get_PLL_LPF_Phase_Error_Output [C][n_fm_out]
 *   "bpsk_pll_sym" GetPLLSymbols [C][n_rds][2] | "bpsk_intdump" GetIntDumpFilter [C][n_rds][2] | "bpsk_ted_raw" GetTEDRawPhaseError,
 *   "bpsk_ted_pi" GetTEDPIPhaseError, "bpsk_pll_raw" GetPLLRawPhaseError, "bpsk_pll_pi" GetPLLPIPhaseError, "bpsk_zcd" GetZeroCrossings and
 *   "bpsk_trig" GetIntDumpTriggers (the two bool traces as 0 / 1) [C][n_rds] — bit-identical
 *   to the oracle's; the tolerance mode evaluates its loops at eight points per span / on groups of four samples and has no such trace
 *   (FMD_ERR_NAME)
 *   FMD_FLAG_FAST_MATH keeps fm_out alone (the kernels that need the Hilbert rail make it for themselves) and the NCO phase as one
 *   cubic per 128 samples: "fm_out_iq" and "pll_dt" then need FMD_FLAG_KEEP_TAPS too; "pll_poly" [C][1 + n_fm_out / 128][4] (tolerance mode only) is always there
 * Copies the current block's values to `out` (host); *n_floats receives the float count.  Needs
 * FMD_FLAG_KEEP_TAPS for the streams a fused pipeline would not otherwise materialise. */
int fmd_get_stream(fmd_handle h, const char* name, float* out, size_t cap_floats, size_t* n_floats);

const char* fmd_last_error(fmd_handle h);

/* Per-channel state snapshot / restore (SURVEY.md §5 "checkpoint / resume"; what moving a station between handles or GPUs
 * needs): every filter history, AGC gain, loop integrator, NCO phase, BPSK synchroniser and Manchester decoder variable of ONE
 * channel — the member variables of one reference Broadcast_FM_Demod (broadcast_fm_demod.h:94-227) — as an opaque,
 * self-describing blob of fmd_state_size() bytes.  Both calls synchronise the handle first.  A blob can be restored into any
 * channel of any handle with the same fs_baseband; the restored channel then continues bit-identically.  Controls are not
 * part of the blob (fmd_get_controls / fmd_set_controls).  With FMD_FLAG_RDS_DECODE the blob also holds the channel's RDS decoder
 * (synchroniser, group under way, A/B memories, database): 168 bytes more, and only handles with the flag take it. */
size_t fmd_state_size(fmd_handle h);
int    fmd_get_state(fmd_handle h, int channel, void* blob, size_t cap_bytes);
int    fmd_set_state(fmd_handle h, int channel, const void* blob, size_t n_bytes);

/* Differential Manchester decode of the RDS symbol stream on the GPU, one decoder per channel
 * (reference src/rds_decoder/differential_manchester_decoder.h:25-60; the 16-byte buffer size is the
 * one src/app.cpp:13-20 uses).  bytes: [C][cap_bytes]; counts[c] = bytes appended for channel c this
 * block (multiples of 16). */
int fmd_get_rds_bytes(fmd_handle h, uint8_t* bytes, int cap_bytes_per_channel, int* counts);
/* ... and as device views of the newest block (same lifetime rule as fmd_audio_dev): d_bytes [C][*cap_bytes_per_channel],
 * d_counts [C] — for hosts that fetch the outputs with their own asynchronous copies (fm-radio_amd/host/station_ring.hpp). */
int fmd_rds_bytes_dev(fmd_handle h, const uint8_t** d_bytes, const int** d_counts, int* cap_bytes_per_channel);

/* ------------------------------------------------------------------------------------------------------------------
 * RDS decoding chain on the GPU (reference src/rds_decoder/rds_decoding_chain.h: RDS_Group_Sync -> RDS_Decoder ->
 * RDS_Database_Decoder_Handler -> RDS_Database), one decoder per channel, fed with the Manchester decoder's bytes.
 * Bit-identical to the reference: group sync on the CRC-10 offset words with single-bit correction
 * (rds_group_sync.cpp:29-127, crc10.cpp:28-60), the group decoder (rds_decoder.cpp:82-540) and the database handler
 * (rds_database_decoder_handler.cpp).  Kernel k_rds_decode (fmd_kernels_rds.inc).
 * ------------------------------------------------------------------------------------------------------------------ */
/* opt-in: the handle runs k_rds_decode behind its RDS stage (fmd_get_rds_db, fmd_get_rds_groups).  Without it nothing changes:
 * no allocation, no launch, the same fmd_state_size. */
#define FMD_FLAG_RDS_DECODE      128u

/* reference enum TrafficAnnouncement (rds_database.h:20-25), in its order: the 0A group's TP << 1 | TA */
enum { FMD_RDS_TA_NONE = 0, FMD_RDS_TA_EON_INFO = 1, FMD_RDS_TA_AWAIT_EON_ANNOUNCE = 2, FMD_RDS_TA_NOW_EON_ANNOUNCE = 3 };

/* reference RDS_Database (rds_database.h:27-79) as a fixed-layout record (120 bytes); alt_freqs is left out because the
 * reference's handler never fills it (OnAlternativeFrequencyCode is a TODO).  The last three fields are beyond the reference:
 * the synchroniser's status. */
typedef struct {
    char     service_name[8];          /* PS, '\r' stored as 0 */
    char     programme_type_name[8];   /* PTYN */
    char     radio_text[64];           /* RT */
    uint16_t PI_code;
    uint8_t  programme_type;
    uint8_t  is_stereo, is_music, is_artificial_head, is_compressed, is_dynamic_program_type;
    struct { int32_t day, month, year; uint8_t hour, minute, pad_[2]; } datetime;
    int8_t   local_time_offset;
    uint8_t  traffic_announcement;     /* FMD_RDS_TA_* */
    uint8_t  pad_[2];
    int32_t  in_sync;                  /* 1: the group synchroniser is reading groups (READ_BLOCK), 0: it is hunting for block A */
    uint32_t groups;                   /* groups delivered to the decoder since the decoder's reset */
    uint32_t sync_acquisitions;        /* times the synchroniser locked onto a block A since the decoder's reset */
} fmd_rds_db;

/* reference rds_block_t / rds_group_t (rds_constants.h:30-39): block_type 0 A, 1 B, 2 C, 3 C' (C1), 4 D.  An invalid block keeps
 * its uncorrected data and the type of the last offset word tried, as in the reference. */
typedef struct { uint16_t data; uint8_t block_type; uint8_t is_valid; } fmd_rds_block;
typedef struct { fmd_rds_block blocks[4]; } fmd_rds_group;

/* App::GetRDSDatabase() (reference src/app.cpp:33-35, app.h:42) per channel, after the newest block: db [C] (host copy) / a device
 * view [C] (same lifetime rule as fmd_rds_bytes_dev).  FMD_ERR_ARG without FMD_FLAG_RDS_DECODE. */
int fmd_get_rds_db(fmd_handle h, fmd_rds_db* db);
int fmd_rds_db_dev(fmd_handle h, const fmd_rds_db** d_db);
/* the groups RDS_Group_Sync::OnGroup() delivered in the newest block (rds_group_sync.cpp:95): groups [C][cap_groups_per_channel],
 * counts [C].  A channel delivers at most fmd_rds_groups_dev's *cap_groups_per_channel groups a block; a smaller cap truncates (counts
 * stay the true numbers). */
int fmd_get_rds_groups(fmd_handle h, fmd_rds_group* groups, int cap_groups_per_channel, int* counts);
int fmd_rds_groups_dev(fmd_handle h, const fmd_rds_group** d_groups, const int** d_counts, int* cap_groups_per_channel);
/* RDS_Database::Reset() (rds_database.h:58-79; the GUI's reset button, src/gui/render_rds_database.cpp:46) for one channel, or all
 * with -1: clears the database only.  The synchroniser and the handler's A/B flag memories keep their state, as in the reference.
 * Synchronises the handle; the next block's snapshot shows the cleared record. */
int fmd_reset_rds_db(fmd_handle h, int channel);

/* Standalone batched decoder: RDS_Decoding_Chain::Process (rds_decoding_chain.h:24-26) for n_channels independent byte streams,
 * the counterpart of the reference's rds_decode tool (src/rds_decode.cpp).  Decodes bytes from any source (e.g. the scraper's
 * _rds.bin files) with the same kernel.  State carries over from call to call; counts need not be multiples of 16. */
typedef struct fmd_rdsdec_s* fmd_rdsdec;
int fmd_rdsdec_create(int n_channels, int device, fmd_rdsdec* out);
int fmd_rdsdec_destroy(fmd_rdsdec d);
/* every channel back to the freshly constructed chain */
int fmd_rdsdec_reset(fmd_rdsdec d);
/* RDS_Database::Reset() for one channel (-1: all); see fmd_reset_rds_db */
int fmd_rdsdec_reset_db(fmd_rdsdec d, int channel);
/* d_bytes [C][cap_bytes_per_channel] on the device, d_counts [C] on the device (0 <= counts[c] <= cap).  Asynchronous on `stream`;
 * the outputs (database after the call, groups delivered during it) are readable once the stream has reached this point.
 * The group records of a call hold up to fmd_rdsdec_groups_cap(cap) groups per channel: enough for any count. */
int fmd_rdsdec_process_dev(fmd_rdsdec d, const uint8_t* d_bytes, const int* d_counts, int cap_bytes_per_channel, void* stream);
/* host buffers: copies, runs, synchronises */
int fmd_rdsdec_process_host(fmd_rdsdec d, const uint8_t* bytes, const int* counts, int cap_bytes_per_channel);
/* most groups one channel can deliver from cap_bytes new bytes (one group needs >= 79 new bits: 78 behind a re-lock) */
int fmd_rdsdec_groups_cap(int cap_bytes_per_channel);
/* host copies after the last process call (synchronise its stream first): db [C]; groups [C][cap_groups_per_channel], counts [C] */
int fmd_rdsdec_get_db(fmd_rdsdec d, fmd_rds_db* db);
int fmd_rdsdec_get_groups(fmd_rdsdec d, fmd_rds_group* groups, int cap_groups_per_channel, int* counts);
const char* fmd_rdsdec_last_error(fmd_rdsdec d);

/* ------------------------------------------------------------------------------------------------------------------
 * Wideband channeliser (SURVEY.md §8f row 3 / BASELINE configs[4]; NOT part of the reference, which tunes one station in
 * the RTL-SDR hardware): splits one wideband capture — cf32, or a receiver's interleaved u8 (RTL-SDR), s8 (HackRF) or s16
 * (Airspy, SDRplay, USRP sc16) — into n_stations channels at fs_out, laid out [C][n_out] cf32 — the input layout of fmd_process_cf32_dev.  Per station: mix the centre frequency to 0, then a rational polyphase
 * decimator L/M = fs_out/fs_in (256 k / 10 M = 16 / 625) built from one Kaiser-windowed prototype (cut-off fs_out / 2,
 * 60 dB).  Streaming: histories and the mixers' phases carry over from call to call.
 * The input and output sample indices are counted since create / reset in unsigned 64-bit integers and the mixer's phase n inc is
 * taken modulo 2^64, which is its definition; the first product to overflow is o M (o the output index, in the window start
 * floor(o M / L) and the branch (o M) mod L) at o M = 2^64, i.e. after 2^64 / L >= 2^58 input samples (L <= 64): 101 806 days at
 * 32.768 MSa/s, the highest rate accepted at fs_out = 256 kSa/s.  (A station's mixer runs at inc 2^-64 fs_in with inc the double
 * frac(f / fs_in) rounded to 2^-63: within 2^-54 fs_in, 1.8e-9 Hz at that rate, of f.  Against the exact f that is a phase difference
 * of up to 3.5e-16 rad per sample, 1.5e-6 rad at sample 2^32.)
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_channelizer_s* fmd_channelizer;
typedef struct {
    double        fs_in;             /* wideband sample rate, integer Hz */
    double        fs_out;            /* per-station rate handed to the demodulator, integer Hz (256000) */
    int           n_stations;
    const double* center_hz;         /* [n_stations] station centres relative to the capture's centre, |f| < fs_in / 2 */
    int           taps_per_phase;    /* 0 = default (fmd_chan_default_taps_per_phase), else a multiple of 4 */
    long long     max_input_samples; /* largest n_in of a process call */
    int           device;            /* HIP device ordinal, -1 = current */
} fmd_chan_config;

/* host-only filter design (no GPU needed): L/M and, if taps != NULL, the prototype stored [t][p] (t = tap within phase p) */
int fmd_chan_design(double fs_in, double fs_out, int taps_per_phase, float* taps, int* L, int* M);
/* host-only (no GPU needed): the taps per phase fmd_chan_create uses when taps_per_phase == 0.  640 for every pair with
 * 128 M / L + 642 <= 7168 (all of them up to 12.8 MSa/s -> 256 kSa/s); above, 4 ceil(16.384 (M / L) / 4), which keeps the 64 us of
 * capture 640 taps per phase span at 10 MSa/s (20.48 MSa/s -> 1312, 32.768 MSa/s -> 2100).  FMD_ERR_ARG for rates fmd_chan_design refuses.
 * fmd_chan_create accepts every pair with M / L <= 128 and L <= 64, with 4 to 4096 taps per phase. */
int fmd_chan_default_taps_per_phase(double fs_in, double fs_out);
int fmd_chan_create(const fmd_chan_config* cfg, fmd_channelizer* out);
int fmd_chan_destroy(fmd_channelizer h);
int fmd_chan_reset(fmd_channelizer h);
int fmd_chan_info(fmd_channelizer h, int* L, int* M, int* taps_per_phase, int* n_stations);
int fmd_chan_get_taps(fmd_channelizer h, float* taps, size_t cap_floats);
/* host-only: which kernel serves this handle's process calls (fixed at create by the rate pair and the taps per phase) and how many
 * consecutive outputs one of its workgroups takes per tile (128; 64, 32 or 16 for the general kernel at the whole-band rates; 16 G for
 * the band form's G = 8, 4 or 2 groups).  Either pointer may be NULL.  Diagnostic: results do not depend on the caller knowing it. */
enum {
    FMD_CHAN_FORM_GENERAL = 0,       /* k_channelize: one output per thread, any L <= 64 */
    FMD_CHAN_FORM_VALU16 = 1,        /* k_channelize16: L = 16 on the vector ALUs, taps per phase a multiple of 64 up to 1024 that the next form cannot hold */
    FMD_CHAN_FORM_MFMA16 = 2,        /* k_channelize16_mfma: L = 16 on the matrix cores, floor(15 M / 16) + taps per phase <= 1232 */
    FMD_CHAN_FORM_BAND = 3           /* k_channelize_band_mfma: the whole-band pairs with L dividing 16 */
};
int fmd_chan_kernel_form(fmd_channelizer h, int* form, int* tile_outputs);
/* d_wide: [n_in][2] cf32 on the device; n_in * L must be a multiple of M (625 input samples per 16 outputs at 10 M -> 256 k).
 * d_out: [n_stations][out_capacity_per_station][2] cf32 on the device — station k's *n_out samples start at row k (row
 * stride = out_capacity_per_station; pass the exact n_out to get the dense [C][n_out] layout fmd_process_cf32_dev takes).
 * Asynchronous on `stream`; consecutive calls may use different streams (the library orders them).  d_wide is read IN PLACE by the call's
 * kernel (no staging copy): like d_out it belongs to the call until its work on `stream` has completed. */
int fmd_chan_process_cf32_dev(fmd_channelizer h, const float* d_wide, size_t n_in, float* d_out, size_t out_capacity_per_station,
                              size_t* n_out, void* stream);
/* The same call on a receiver's integer capture, d_wide [n_in][2] interleaved I, Q on the device, read without a conversion pass.
 * Each pair becomes a float exactly: u8 as (float)v - 127 (the reference's and fmd_process_u8_*'s convention), s8 and s16 as (float)v,
 * unscaled (the discriminator and the RDS AGC do not depend on level).  A call on integer samples writes exactly the bits that
 * fmd_chan_process_cf32_dev writes when given the converted samples, for every rate pair, kernel and split of the input into calls.
 * The history holds converted samples, so consecutive calls on one handle may use different formats; arguments, errors, streams
 * and fmd_chan_reset are those of fmd_chan_process_cf32_dev. */
int fmd_chan_process_u8_dev(fmd_channelizer h, const uint8_t* d_wide, size_t n_in, float* d_out, size_t out_capacity_per_station,
                            size_t* n_out, void* stream);
int fmd_chan_process_s8_dev(fmd_channelizer h, const int8_t* d_wide, size_t n_in, float* d_out, size_t out_capacity_per_station,
                            size_t* n_out, void* stream);
int fmd_chan_process_s16_dev(fmd_channelizer h, const int16_t* d_wide, size_t n_in, float* d_out, size_t out_capacity_per_station,
                             size_t* n_out, void* stream);
const char* fmd_chan_last_error(fmd_channelizer h);

/* ------------------------------------------------------------------------------------------------------------------
 * Band scan (NOT part of the reference, whose RTL-SDR hardware tunes one known station): finds the occupied channels of a
 * wideband capture, whose offsets configure fmd_chan_create (fmd_chan_config.center_hz) directly.  Two steps:
 *  1. an averaged periodogram on the GPU.  N = nfft (power of two, 256 ... 16384), hop H = N / 2; frame f covers the absolute input
 *     samples [f H, f H + N) counted since create / reset (no zero padding at the start) and counts once its last sample has arrived.
 *     w[n] = 0.5 - 0.5 cos(2 pi n / N) (periodic Hann, computed in double, stored as fp32); P_f[k] = |sum_n w[n] x[f H + n] e^{-j 2 pi k n / N}|^2
 *     (fp32 FFT); S[k] = sum_f P_f[k] accumulated in fp64 in frame order, so S does not depend, bit for bit, on how the capture is split
 *     into calls.  Reported: PSD[i] = S[k] / (F fs_in sum w^2), i = (k + N / 2) mod N: bin i is at (i - N / 2) fs_in / N Hz, low to
 *     high (F frames; sum w^2 over the fp32 window values, in double; before the first frame the PSD is all zero).
 *     A non-finite sample makes the frames that hold it non-finite, and the PSD stays non-finite until fmd_scan_reset.
 *     No kernel computes with the absolute index: a call's frames are indexed within its window [history][block] (below 2^32 + N), and
 *     the host counts samples in an unsigned and frames in a signed 64-bit integer, so the limit is 2^64 input samples (F = 2^57 at
 *     N = 256): 6.5 million days at 32.768 MSa/s, the highest rate the channeliser accepts at 256 kSa/s (the scanner takes any rate);
 *     F enters the PSD's scale as a double, exact up to 2^53 frames.
 *  2. detection on the host, a pure function of the PSD in double (fmd_scan_detect): channel power over a raster, SNR against a noise
 *     quantile of the usable band, one detection per station (rules: fmd_scan_params below).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_scanner_s* fmd_scanner;
typedef struct {
    double    fs_in;             /* capture rate, Hz (> 0) */
    int       nfft;              /* N, a power of two in 256 ... 16384; 0 = fmd_scan_default_nfft(fs_in) */
    long long max_input_samples; /* largest n_in of a process call */
    int       device;            /* HIP device ordinal, -1 = current */
} fmd_scan_config;
/* Detection rules, with D = fs_in / N the bin width and f_i = (i - N / 2) D:
 *   usable bins     |f_i| <= usable_fraction fs_in / 2; noise floor v = the value at 0-based rank floor(noise_quantile (m - 1)) of the
 *                   m usable bins sorted ascending
 *   raster points   f_c = raster_origin_hz + j raster_hz for every integer j with |f_c| + channel_bw_hz / 2 <= usable_fraction fs_in / 2
 *                   (at most 1000000 raster points: a finer raster is refused)
 *   channel         bins max(0, ceil((f_c - bw / 2) / D) + N / 2) ... min(N - 1, floor((f_c + bw / 2) / D) + N / 2), n_c of them (the
 *                   clip matters only where usable_fraction = 1 lets a channel end exactly at +fs_in / 2, which is no bin of its own);
 *                   P_c = D sum PSD over them;
 *                   snr_db = 10 log10(P_c / (v D n_c)) (+inf where v = 0); a channel with P_c = 0 is never reported
 *   candidates      snr_db >= min_snr_db, taken by descending P_c (ties: lower offset first); one is accepted unless an accepted
 *                   station lies closer than min_spacing_hz (the +-raster neighbours of a strong station are not reported)
 *   output          { offset_hz = f_c, power_db = 10 log10 P_c, snr_db }, ascending by offset */
typedef struct {
    double raster_hz;         /* 100e3 (200e3 in the Americas; 50e3 allowed): > 0 */
    double raster_origin_hz;  /* 0: the offset of one raster point from the capture's centre */
    double channel_bw_hz;     /* 100e3: > 0 */
    double min_snr_db;        /* 10 */
    double usable_fraction;   /* 0.8: in (0, 1] */
    double noise_quantile;    /* 0.1: in [0, 1] */
    double min_spacing_hz;    /* 150e3: >= 0 */
} fmd_scan_params;
typedef struct {
    double offset_hz;         /* from the capture's centre: pass straight to fmd_chan_config.center_hz */
    double power_db;          /* 10 log10 P_c, P_c in the capture's units squared */
    double snr_db;
} fmd_scan_station;

/* host-only (no GPU needed): the smallest power of two N with fs_in / N <= 5 kHz, clamped to [256, 16384]; FMD_ERR_ARG for fs_in <= 0 */
int fmd_scan_default_nfft(double fs_in);
void fmd_scan_default_params(fmd_scan_params* p);
/* host-only (no GPU needed): the detection rules on psd [nfft] (fmd_scan_get_psd's layout).  Writes min(cap, n) stations to out and
 * always sets *n_found = n.  FMD_ERR_ARG with a message (fmd_scan_last_error(NULL)) for a non-finite or negative PSD and invalid
 * parameters. */
int fmd_scan_detect(const double* psd, int nfft, double fs_in, const fmd_scan_params* p,
                    fmd_scan_station* out, int cap, int* n_found);
int fmd_scan_create(const fmd_scan_config* cfg, fmd_scanner* out);
int fmd_scan_destroy(fmd_scanner h);
/* back to the freshly created scanner: no history, no frames (waits for the scanner's earlier work) */
int fmd_scan_reset(fmd_scanner h);
/* d_wide: [n_in][2] on the device, read IN PLACE, 0 < n_in <= max_input_samples.  The integer forms convert each pair exactly as
 * fmd_chan_process_u8_dev / _s8_dev / _s16_dev do (u8: v - 127; s8, s16: v) and give the bits the cf32 call gives on the converted
 * samples; formats may change from call to call.  The scanner keeps up to N - 1 converted samples between calls.  Asynchronous on
 * `stream`; consecutive calls may use different streams (the library orders them); d_wide belongs to the call until its work on
 * `stream` has completed.  A channeliser may read the same block on another stream. */
int fmd_scan_process_cf32_dev(fmd_scanner h, const float* d_wide, size_t n_in, void* stream);
int fmd_scan_process_u8_dev(fmd_scanner h, const uint8_t* d_wide, size_t n_in, void* stream);
int fmd_scan_process_s8_dev(fmd_scanner h, const int8_t* d_wide, size_t n_in, void* stream);
int fmd_scan_process_s16_dev(fmd_scanner h, const int16_t* d_wide, size_t n_in, void* stream);
/* the averaged PSD of every frame so far into psd [cap >= nfft] (layout above) and the frame count F; synchronises with the
 * scanner's work */
int fmd_scan_get_psd(fmd_scanner h, double* psd, int cap, long long* n_frames);
/* fmd_scan_get_psd, then fmd_scan_detect with p (NULL = fmd_scan_default_params) */
int fmd_scan_stations(fmd_scanner h, const fmd_scan_params* p, fmd_scan_station* out, int cap, int* n_found);
const char* fmd_scan_last_error(fmd_scanner h);

/* ------------------------------------------------------------------------------------------------------------------
 * Batched audio resampler: the stage between OnAudioOut and the listener (reference Resampled_PCM_Player,
 * src/audio/resampled_pcm_player.cpp:15-54, fed every OnAudioOut block at src/fm_demod_tuner.cpp:145-165).  C stations'
 * stereo f32 frames at fs_in (fmd_rates.fs_audio) in, [C][n_out][2] at fs_out out, on the GPU.  Standalone: it reads the
 * demodulator's audio views (fmd_audio_dev) and changes nothing in the demodulator.  Two methods:
 *   FMD_RESAMPLE_REFERENCE  Resample() (resampled_pcm_player.cpp:37-54): each call is one ConsumeBuffer of n_in frames,
 *                           block-local linear interpolation, bit-identical to the reference's build; nothing carries over.
 *                           n_out = (int)((float)fs_out / (float)fs_in * (float)n_in).  Where the reference's running
 *                           single-precision index walks past the block's last frame (long calls: n_in = 16384 at 48 kHz) its
 *                           span indexing would abort: such a call returns FMD_ERR_ARG and writes nothing.
 *   FMD_RESAMPLE_POLYPHASE  (beyond the reference) streaming rational L / M = fs_out / fs_in in lowest terms, anti-aliased:
 *                           y[n] = sum_{t<T} h[p + t L] x[floor(n M / L) - t], p = n M mod L, n counted since the last reset;
 *                           output n is emitted by the call that delivers input frame floor(n M / L).  h: one Kaiser-windowed
 *                           sinc (>= 60 dB from min(fs_in, fs_out) / 2 up, every phase's DC gain 1).  Each channel keeps its
 *                           last T - 1 input frames (zero after a reset); the frame counters are 64-bit, on the host and shared by
 *                           all channels, so fmd_resampler_output_frames is exact.  Fixed fp32 FMA order: a station's outputs do
 *                           not depend on how its input was split into calls, on the batch size or on its row.  The counters and
 *                           every product of them are signed 64-bit; the first to overflow is (frames in) L + M - 1 of the output
 *                           count (with it n M of the window start and branch) at 2^63, i.e. after 2^63 / L >= 2^51 input frames
 *                           (L <= 4096): 26 062 days at fs_in = 1 MHz, the highest rate accepted.
 * fs_in == fs_out: either method passes the input through unchanged (ConsumeBuffer, resampled_pcm_player.cpp:17-20).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_resampler_s* fmd_resampler;
enum { FMD_RESAMPLE_REFERENCE = 0, FMD_RESAMPLE_POLYPHASE = 1 };
typedef struct {
    int       n_channels;
    int       fs_in;             /* input rate, Hz: 32000 = fmd_rates.fs_audio */
    int       fs_out;            /* output rate, Hz: 48000, 44100, 22050, 16000, 8000, ... (the player's device rate) */
    int       method;            /* FMD_RESAMPLE_* */
    int       taps_per_phase;    /* polyphase only: T, multiple of 4 in 8 ... 256; 0 = default: 32 x ceil(M / L) */
    long long max_input_frames;  /* largest n_in of a call */
    int       device;            /* HIP device ordinal, -1 = current */
} fmd_resampler_config;

/* host-only polyphase design (no GPU needed): L / M and, if taps != NULL, the prototype h stored [t][p] = h[p + t L]
 * (taps_per_phase 0 = the default) */
int fmd_resampler_design(int fs_in, int fs_out, int taps_per_phase, float* taps, int* L, int* M);
/* Resampled_PCM_Player::Resampled_PCM_Player (resampled_pcm_player.cpp:5-11) x n_channels */
int fmd_resampler_create(const fmd_resampler_config* cfg, fmd_resampler* out);
int fmd_resampler_destroy(fmd_resampler r);
/* polyphase: channel >= 0 clears that channel's history; -1 clears every history and restarts the frame counters.  Waits for
 * the resampler's earlier calls.  (The reference method has no state: nothing to do.) */
int fmd_resampler_reset(fmd_resampler r, int channel);
/* Resampled_PCM_Player::SetInputSampleRate (resampled_pcm_player.cpp:29-33): returns 1 if the rate changed (polyphase: the
 * filter is re-designed and every history and counter reset), 0 if not, < 0 on error */
int fmd_resampler_set_input_rate(fmd_resampler r, int fs_in);
/* the frame count the next process call with n_in input frames emits per channel */
int fmd_resampler_output_frames(fmd_resampler r, long long n_in, long long* n_out);
/* Resampled_PCM_Player::ConsumeBuffer (resampled_pcm_player.cpp:15-27) for every channel.
 * d_in [C][in_stride][2] f32 on the device (fmd_audio_dev's view: in_stride = n_audio), n_in <= in_stride and <= max_input_frames;
 * d_out [C][out_stride][2] on the device, out_stride >= the call's *n_out.  Asynchronous on `stream`; consecutive calls may use
 * different streams (the library orders them).  A call on a new n_in (reference method) uploads that length's index table once.
 * The pcm16 form writes the scraper's frames (fm_scraper.cpp:79-82: sample * (32767 * 0.95f), truncated toward zero): exactly
 * that conversion of the f32 form's output.  The product t is one fp32 multiply; for |t| < 2^31 the frame holds the low 16 bits
 * of (int32_t)t, so it wraps past +-32768 as the reference's conversion does (no saturation: clamp before the call if wanted).
 * NaN gives 0; +inf and t >= 2^31 give -1 and -inf and t <= -2^31 give 0 (the device's float-to-int conversion saturates to
 * 0x7fffffff / 0x80000000 and the low 16 bits are kept). */
int fmd_resampler_process_f32_dev(fmd_resampler r, const float* d_in, long long in_stride, long long n_in,
                                  float* d_out, long long out_stride, long long* n_out, void* stream);
int fmd_resampler_process_pcm16_dev(fmd_resampler r, const float* d_in, long long in_stride, long long n_in,
                                    int16_t* d_out, long long out_stride, long long* n_out, void* stream);
/* the same with a HOST destination out [C][out_stride][2] f32: resamples on `stream` and synchronises it (for hosts that write
 * files, fm-radio_amd/host/resampled_pcm_player_gpu.hpp) */
int fmd_resampler_process_f32_host(fmd_resampler r, const float* d_in, long long in_stride, long long n_in,
                                   float* out, long long out_stride, long long* n_out, void* stream);
const char* fmd_resampler_last_error(fmd_resampler r);

/* ------------------------------------------------------------------------------------------------------------------
 * Batched audio mixer: the stage between the listener's ring buffers and PortAudio (reference AudioMixer::UpdateMixer,
 * src/audio/audio_mixer.cpp:33-79; src/audio/portaudio_output.cpp:84).  B independent buses, each one reference AudioMixer; every bus
 * reads the same device array of station audio [C][in_stride][2] (fmd_audio_dev's view at 32 kHz, or a resampler's output at the
 * playback rate) and changes nothing in the stage that wrote it.  Per call and bus, bit-identical to the reference's build:
 *   k      = the bus's sources whose station delivered (d_active[row] != 0; a row listed twice counts twice)
 *   k == 0 : every output is +0
 *   scale  = gain / log10f((float)k * 10.0f)   (host libm's log10f, on the host; denormal gain or scale -> zero of its sign)
 *   acc    = +0; for each delivering source in registration order: acc = fmaf(x, scale, acc), denormal inputs and results
 *            flushed to zeros of their sign (the reference links crtfastmath: FTZ + DAZ)
 *   out    = t < 1 ? t : 1 with t = (-1 > acc) ? -1 : acc   (x86 vmaxss / vminss order: NaN -> +1, +-inf -> +-1)
 * No state carries over between calls, so a bus's output does not depend on how its frames are split into calls, on the batch or on
 * the bus's row.  Splitting frames into ring-buffer blocks is the caller's business.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_mixer_s* fmd_mixer;
typedef struct {
    int          n_channels;    /* C: station rows of the input */
    int          n_buses;       /* B */
    const int*   bus_offsets;   /* [B + 1]: bus b's sources are bus_sources[bus_offsets[b] .. bus_offsets[b + 1]) */
    const int*   bus_sources;   /* station rows in registration (CreateManagedBuffer) order; a row may appear in many buses */
    const float* gains;         /* [B] AudioMixer::GetOutputGain, NULL = 1.0f each */
    int          device;        /* HIP device ordinal, -1 = current */
} fmd_mixer_config;
/* AudioMixer::AudioMixer + CreateManagedBuffer per source, for every bus */
int fmd_mixer_create(const fmd_mixer_config* cfg, fmd_mixer* out);
int fmd_mixer_destroy(fmd_mixer m);
/* replace bus `bus`'s sources (registration order); takes effect at the next process call */
int fmd_mixer_set_sources(fmd_mixer m, int bus, const int* sources, int n_sources);
/* AudioMixer::GetOutputGain() = gain for bus `bus` (-1 = every bus); takes effect at the next process call */
int fmd_mixer_set_gain(fmd_mixer m, int bus, float gain);
int fmd_mixer_get_gain(fmd_mixer m, int bus, float* gain);
/* AudioMixer::UpdateMixer for every bus on n frames.  d_in [C][in_stride][2] f32 on the device; d_active: [C] uint8 on the device,
 * non-zero = the station delivered a block this call (the reference's non-empty ring buffer), NULL = all; d_out [B][out_stride][2] on
 * the device.  n < 0, n > in_stride or out_stride < n return FMD_ERR_ARG and write nothing; n == 0 and empty buses are valid.
 * Asynchronous on `stream`; consecutive calls may use different streams (the library orders them). */
int fmd_mixer_process_f32_dev(fmd_mixer m, const float* d_in, long long in_stride, long long n, const uint8_t* d_active,
                              float* d_out, long long out_stride, void* stream);
/* the same, delivered to HOST memory out [B][out_stride][2] after `stream` has finished (what a PortAudio-style callback consumes) */
int fmd_mixer_process_f32_host(fmd_mixer m, const float* d_in, long long in_stride, long long n, const uint8_t* d_active,
                               float* out, long long out_stride, void* stream);
const char* fmd_mixer_last_error(fmd_mixer m);

/* ------------------------------------------------------------------------------------------------------------------
 * DC offset and IQ imbalance correction of a wideband capture (NOT part of the reference, whose RTL-SDR hardware is low-IF and tunes
 * one station): one pass over the capture, ahead of the band scanner and the channeliser.  A zero-IF front end leaves a DC term (the
 * scanner sees a carrier at offset 0; u8 read as v - 127 has one of 0.5) and a gain / phase imbalance between I and Q, which mirrors
 * every station to the negated offset 25 - 40 dB down.  The corrector measures both from second-order moments and removes them with
 * y = z + w conj(z), z = x - dc.  Arithmetic, restated in C by tests/cpp/iqcorr_ref.c:
 *   conversion  as fmd_chan_process_*_dev: cf32 as is; u8 v - 127; s8, s16 (float)v.  All exact.
 *   moments     n, sum i, sum q, sum i^2, sum q^2, sum i q over the raw (uncorrected) converted samples since create / reset, in fp64.
 *               Every term is formed in double from the converted floats (a product of two floats is exact in double: only the
 *               additions round), and added in a fixed order that does not depend on how the capture is split into calls, on streams
 *               or on the formats:
 *                 - samples are counted absolutely since reset, in chunks of 4096;
 *                 - within a chunk, 256 partial sums p_j = sum_k term[j + 256 k], k ascending, starting from +0;
 *                 - the partials are combined by the halving tree: p_j += p_{j + 128} for j < 128, then 64, ... 1; the chunk's sum is p_0;
 *                 - chunk sums are added to the running total in chunk order;
 *                 - an unfinished chunk carries its 256 partials per moment to the next call; fmd_iqcorr_get_moments reports
 *                   total + tree(open chunk) and leaves the chunk open.
 *               No floating-point atomics.  For the integer formats every sum is an exact integer while it stays below 2^53: for s16
 *               that is at least 2^23 samples (|v|^2 <= 2^30), for u8 and s8 at least 2^39.  A non-finite sample makes its moments
 *               non-finite until fmd_iqcorr_reset / _reset_moments.  The sample index is an unsigned 64-bit count on the host and a
 *               signed one in the kernel, whose largest expression is the end of a chunk, (floor(a / 4096) + 1) 4096 <= a + 4096
 *               (a: the index of a call's first sample): it overflows at 2^63 samples, 3.26 million days at 32.768 MSa/s (the
 *               corrector takes any rate; this is the highest the channeliser accepts at 256 kSa/s); n is reported as a double,
 *               exact up to 2^53 samples (3181 days at that rate).
 *   solve       host, double, a pure function of the moments (fmd_iqcorr_solve):
 *                 m = (sum i, sum q) / n;  vii = sum i^2 / n - m_i^2;  vqq = sum q^2 / n - m_q^2;  viq = sum i q / n - m_i m_q
 *                 p = vii + vqq;  c = (vii - vqq) + 2j viq;  s = sqrt(max(0, p^2 - |c|^2));  w = -c / (p + s), w = 0 where p + s <= 0
 *                 (p = 0: a constant capture)
 *               { dc_i, dc_q, w_re, w_im } = (m_i, m_q, Re w, Im w) rounded to fp32.  This w is the exact root of
 *               E[(z + w conj(z))^2] = 0 (the circularity condition), not the first-order -c / 2p.
 *   apply       fp32, every FMA an explicit fmaf:
 *                 zi = i - dc_i;  zq = q - dc_q
 *                 yi = fmaf(w_re, zi, fmaf(w_im, zq, zi));  yq = fmaf(w_im, zi, fmaf(-w_re, zq, zq))
 *               No gain normalisation.  The identity correction (all zero: the state after create and reset) reproduces the conversion
 *               in value.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_iqcorr_s* fmd_iqcorr;
typedef struct {
    long long max_input_samples; /* largest n_in of a process call, in (0, 2^32] */
    int       device;            /* HIP device ordinal, -1 = current */
} fmd_iqcorr_config;
typedef struct { double n, sum_i, sum_q, sum_ii, sum_qq, sum_iq; } fmd_iq_moments;
typedef struct { float dc_i, dc_q, w_re, w_im; } fmd_iq_correction;

int fmd_iqcorr_create(const fmd_iqcorr_config* cfg, fmd_iqcorr* out);
int fmd_iqcorr_destroy(fmd_iqcorr h);
/* moments to zero and the correction to identity (waits for the corrector's earlier work) */
int fmd_iqcorr_reset(fmd_iqcorr h);
/* moments to zero; the correction stays */
int fmd_iqcorr_reset_moments(fmd_iqcorr h);
/* d_in: [n_in][2] on the device, starting at any sample (aligned to one I / Q pair of its format), 0 < n_in <= max_input_samples.  One
 * fused kernel reads each raw sample once, adds it to the moments and writes d_out [n_in][2] cf32 (8-byte aligned) corrected with the
 * correction in force when the call was made.  d_out == NULL measures only; d_out == d_in is allowed for cf32 (each thread writes only
 * what it read).  Formats may change from call to call.  An n_in outside its range or a misaligned pointer returns FMD_ERR_ARG, and
 * nothing is written or counted.  Asynchronous on `stream`; consecutive calls may use different streams (the library orders them). */
int fmd_iqcorr_process_cf32_dev(fmd_iqcorr h, const float* d_in, long long n_in, float* d_out, void* stream);
int fmd_iqcorr_process_u8_dev(fmd_iqcorr h, const uint8_t* d_in, long long n_in, float* d_out, void* stream);
int fmd_iqcorr_process_s8_dev(fmd_iqcorr h, const int8_t* d_in, long long n_in, float* d_out, void* stream);
int fmd_iqcorr_process_s16_dev(fmd_iqcorr h, const int16_t* d_in, long long n_in, float* d_out, void* stream);
/* the moments of every sample so far (an open chunk included, and left open); synchronises with the corrector's work */
int fmd_iqcorr_get_moments(fmd_iqcorr h, fmd_iq_moments* out);
/* host-only (no GPU needed): the solve step.  FMD_ERR_ARG (message: fmd_iqcorr_last_error(NULL)) for n <= 0, a non-finite moment or a
 * result that is not finite in fp32 */
int fmd_iqcorr_solve(const fmd_iq_moments* m, fmd_iq_correction* out);
/* takes effect at the next process call; non-finite values are refused (FMD_ERR_ARG) */
int fmd_iqcorr_set_correction(fmd_iqcorr h, const fmd_iq_correction* c);
int fmd_iqcorr_get_correction(fmd_iqcorr h, fmd_iq_correction* c);
/* fmd_iqcorr_get_moments, fmd_iqcorr_solve, fmd_iqcorr_set_correction; the moments are kept.  out may be NULL */
int fmd_iqcorr_calibrate(fmd_iqcorr h, fmd_iq_correction* out);
const char* fmd_iqcorr_last_error(fmd_iqcorr h);

/* ------------------------------------------------------------------------------------------------------------------
 * Batched loudness meter (NOT part of the reference): ITU-R BS.1770 / EBU R 128 programme loudness and sample peak of every station's
 * audio, measured where the audio already is.  It reads the same device array [C][in_stride][2] as the resampler and the mixer
 * (fmd_audio_dev's view, or a resampler's output), changes nothing in the stage that wrote it, and keeps one fmd_meter_status record and
 * a 1000-bin histogram per station.  It measures the audio, not the RF signal.  Maximum true-peak level (BS.1770 Annex 2) and loudness
 * range (EBU Tech 3342) are features chosen at create (fmd_meter_create_ex, "True peak and loudness range" below); channel weights are
 * 1.0 for L and R.  Arithmetic, restated in C by tests/cpp/meter_ref.c:
 *   design      host, double, host libm (fmd_meter_design); pi = 3.14159265358979323846:
 *                 pre-filter (high shelf): f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196
 *                   K = tan(pi * f0 / fs);  Vh = pow(10, G / 20);  Vb = pow(Vh, 0.4996667741545416);  a0 = 1 + K / Q + K * K
 *                   pre_b = { (Vh + Vb * K / Q + K * K) / a0, 2 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0 }
 *                   pre_a = { 1, 2 * (K * K - 1) / a0, (1 - K / Q + K * K) / a0 }
 *                 RLB high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, K and a0 by the same two formulas
 *                   rlb_b = { 1, -2, 1 };  rlb_a = { 1, 2 * (K * K - 1) / a0, (1 - K / Q + K * K) / a0 }
 *                 frames_per_subblock Nsb = fs / 10 (100 ms)
 *                 edge[j]   = pow(10, ((-70 + 0.1 * j) + 0.691) / 10),          j = 0 ... 1000   (-70 LUFS ... +30 LUFS in 0.1 LU steps)
 *                 centre[j] = pow(10, (((-70 + 0.1 * j) + 0.05) + 0.691) / 10), j = 0 ... 999
 *               At 48 kHz the formulas give BS.1770's printed coefficients to better than 1e-14.
 *   filter      per (station, rail), all state in fp64 (denormals kept), direct form II transposed, every multiply-add an explicit fma.
 *               With v = (double)x, pb = pre_b, pa = pre_a, rb = rlb_b, ra = rlb_a:
 *                 o1 = fma(pb0, v, s1);   s1 = fma(-pa1, o1, fma(pb1, v, s2));   s2 = fma(-pa2, o1, pb2 * v)
 *                 o2 = fma(rb0, o1, t1);  t1 = fma(-ra1, o2, fma(rb1, o1, t2));  t2 = fma(-ra2, o2, rb2 * o1)
 *                 acc = fma(o2, o2, acc)              frame order, from +0 at each sub-block start
 *                 peak = fmaxf(peak, fabsf(x))        fp32, on the raw sample (a NaN sample leaves peak as it is)
 *               peak_call starts at 0 in every process call that meters the station; peak_hold only at create, reset and reset_peaks.
 *   sub-blocks  frames are counted per station, absolutely since the station's reset; sub-block g is frames [g Nsb, (g + 1) Nsb).  An
 *               unfinished sub-block carries acc of both rails and the filter states to the next call, so no result depends, bit for bit,
 *               on how the frames are split into calls, on streams, on the batch or on the station's row.  When sub-block g completes:
 *                 E_g = (accL + accR) / (double)Nsb, stored at energy_ring[g % 30]
 *                 if g >= 3: B = (((E_{g-3} + E_{g-2}) + E_{g-1}) + E_g) * 0.25   (a 400 ms gating block, 75 % overlap)
 *                   B not finite -> nonfinite++;  else B < edge[0] -> below_gate++;  else hist[j]++ for the j with
 *                   edge[j] <= B < edge[j + 1] (B >= edge[1000] -> j = 999)
 *               Only comparisons run on the device: no logarithm there.  No floating-point atomics.
 *   read-out    host, double, pure functions:
 *                 fmd_meter_lufs(e)  = -0.691 + 10 * log10(e);  e == 0 -> -inf
 *                 momentary          = lufs((((E_{G-4} + E_{G-3}) + E_{G-2}) + E_{G-1}) / 4), G = subblocks
 *                 short-term         = lufs(s / 30), s = +0, s += E_g for g = G - 30 ... G - 1
 *                 integrated         : n = sum of hist; n == 0 -> -inf.  Gamma = (sum over j ascending, from +0, of (double)hist[j] * centre[j])
 *                                      / (double)n.  Keep the bins with centre[j] >= 0.1 * Gamma (the -10 LU relative gate); with the same
 *                                      two sums over the kept bins, I = lufs(sum hist[j] centre[j] / (double)(sum hist[j])).
 *               The histogram quantises a gating block's loudness to its bin's centre, at most 0.05 LU away: inside the +-0.1 LU of EBU
 *               Tech 3341, and what makes the memory per station fixed.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_meter_s* fmd_meter;
typedef struct {
    int       n_channels;         /* C: station rows of the input */
    int       fs;                 /* the audio's rate: a multiple of 10 in 8000 ... 192000 */
    long long max_input_frames;   /* largest n of a process call, in (0, 2^30] */
    int       device;             /* HIP device ordinal, -1 = current */
} fmd_meter_config;
typedef struct {
    double pre_b[3], pre_a[3], rlb_b[3], rlb_a[3];   /* a[0] == 1 */
    int    frames_per_subblock;                      /* fs / 10 */
    double edge[1001], centre[1000];
} fmd_meter_design_t;
/* one per station, 280 bytes: frames at byte 0, subblocks 8, energy_ring 16, peak_call 256, peak_hold 264, below_gate 272, nonfinite 276 */
typedef struct {
    unsigned long long frames;        /* frames metered since reset */
    unsigned long long subblocks;     /* completed 100 ms sub-blocks G */
    double   energy_ring[30];         /* E_g of sub-block g at [g % 30] */
    float    peak_call[2], peak_hold[2];   /* L, R: of the last call that metered the station / since reset or reset_peaks */
    unsigned below_gate, nonfinite;   /* gating blocks under -70 LUFS / non-finite */
} fmd_meter_status;

/* host-only (no GPU needed).  FMD_ERR_ARG unless fs is a multiple of 10 in 8000 ... 192000 */
int fmd_meter_design(int fs, fmd_meter_design_t* out);
double fmd_meter_lufs(double energy);
/* hist [1000]: one station's histogram */
int fmd_meter_integrated(const unsigned* hist, const fmd_meter_design_t* d, double* lufs);
/* FMD_ERR_STATE before 4 (momentary) and 30 (short-term) completed sub-blocks */
int fmd_meter_momentary(const fmd_meter_status* s, double* lufs);
int fmd_meter_short_term(const fmd_meter_status* s, double* lufs);

int fmd_meter_create(const fmd_meter_config* cfg, fmd_meter* out);
int fmd_meter_destroy(fmd_meter m);
/* everything of station `channel` (-1 = every station) as after create: counters, ring, filter states, histogram, peaks, and with the
 * features the r128 record, the true-peak history and the range histogram.  Waits for the meter's earlier work */
int fmd_meter_reset(fmd_meter m, int channel);
/* peak_call and peak_hold (and tp_call, tp_hold) of station `channel` (-1 = every station) to 0; nothing else: the true-peak history stays */
int fmd_meter_reset_peaks(fmd_meter m, int channel);
/* meters n frames of every station.  d_in [C][in_stride][2] f32 on the device, 8-byte aligned; d_active: [C] uint8 on the device,
 * NULL = all: a station whose byte is 0 is skipped whole (no state, counter or peak of it changes).  n < 0, n > in_stride or
 * n > max_input_frames return FMD_ERR_ARG and change nothing; n == 0 is valid (it sets the metered stations' peak_call to 0).
 * Asynchronous on `stream`; consecutive calls may use different streams (the library orders them). */
int fmd_meter_process_f32_dev(fmd_meter m, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, void* stream);
/* out [C]; synchronises with the meter's work */
int fmd_meter_get_status(fmd_meter m, fmd_meter_status* out);
/* hist [C][1000]; synchronises with the meter's work */
int fmd_meter_get_histogram(fmd_meter m, unsigned* hist);
/* the device's own [C] records, for a consumer on the device: ordered behind the meter's work on the stream of its last process call,
 * valid until the next process call */
int fmd_meter_status_dev(fmd_meter m, const fmd_meter_status** d_status);
const char* fmd_meter_last_error(fmd_meter m);

/* True peak and loudness range: the two other figures of EBU R 128, opt-in per meter.  Nothing above changes with them: fmd_meter_status,
 * the histogram and every entry point keep their layout, meaning and values.  Arithmetic, restated in C by tests/cpp/meter_r128_ref.c:
 *   tp design   host, double, host libm (fmd_meter_tp_design); pi as above, beta = 5.0:
 *                 L = 4 for fs < 88200, 2 for 88200 <= fs < 176400, 1 otherwise;  T = 12 taps per phase;  N = L * T;  c = N / 2
 *                 h[i] = sinc((i - c) / L) * I0(beta * sqrt(1 - ((i - c) / c)^2)) / I0(beta),  i = 0 ... N - 1
 *                   sinc(0) = 1, sinc(x) = sin(pi * x) / (pi * x);  I0(x) = 1 + sum over k >= 1 of prod_{m <= k} (x / (2 m))^2, summed
 *                   in k order until a term falls under 1e-18 of the sum
 *                 phase 0 of h is the identity: the raw sample stands for it.  For p = 1 ... L - 1:
 *                   g_p[k] = h[k * L + p], k = 0 ... 11, divided by (sum over k ascending, from +0, of g_p[k]), rounded to float
 *   true peak   per (station, rail), fp32 (denormals kept), every multiply-add an explicit fmaf:
 *                 y_p[n] = fmaf(g_p[11], x[n-11], ... fmaf(g_p[1], x[n-1], fmaf(g_p[0], x[n], +0.0f)))     k ascending, from +0
 *                 tp = fmaxf(tp, fabsf(x[n]));  for p = 1 ... L - 1: tp = fmaxf(tp, fabsf(y_p[n]))        (a NaN leaves tp as it is)
 *               x[n] for n < 0 is the station's history: zeros after create and reset, otherwise the last 11 frames metered.  tp_call
 *               starts at 0 in every process call that meters the station; tp_hold = fmaxf(tp_hold, tp_call), cleared at create, reset and
 *               reset_peaks (which leaves the history alone).  A maximum that never keeps a NaN does not depend on order, so tp_hold is
 *               bit-identical however the frames are split into calls, and tp_hold >= peak_hold.  At L = 1 tp_* equal peak_*.
 *   range       when sub-block g >= 29 completes, after E_g is stored (one short-term value per 100 ms):
 *                 s = +0;  s += energy_ring[i % 30] for i = g - 29 ... g;  S = s / 30.0
 *                 S not finite -> st_nonfinite++;  else S < edge[0] -> st_below++;  else range_hist[j]++ for the j with
 *                 edge[j] <= S < edge[j + 1] (S >= edge[1000] -> j = 999).  Comparisons only; ordinary stores.
 *   read-out    host, double, pure:
 *                 fmd_meter_dbtp(peak) = 20 * log10((double)peak);  0 -> -inf
 *                 fmd_meter_range    : n0 = sum of hist; n0 == 0 -> FMD_ERR_STATE.  Gamma = (sum over j ascending, from +0, of
 *                                      (double)hist[j] * centre[j]) / (double)n0.  Keep the bins with centre[j] >= 0.01 * Gamma (the -20 LU
 *                                      relative gate); n = their count.  Zero-based ranks r10 = floor(0.10 * (n - 1) + 0.5) and
 *                                      r95 = floor(0.95 * (n - 1) + 0.5) over the kept values in ascending order fall in bins j10 and j95
 *                                      (by cumulative count):  low = -70 + 0.1 * j10 + 0.05, high likewise, lra = (j95 - j10) / 10.0.
 *               The bins quantise the range to 0.1 LU, against the +-1 LU of EBU Tech 3342. */
#define FMD_METER_TRUE_PEAK 1u
#define FMD_METER_RANGE     2u
/* fmd_meter_create(cfg, out) == fmd_meter_create_ex(cfg, 0, out).  Unknown feature bits: FMD_ERR_ARG */
int fmd_meter_create_ex(const fmd_meter_config* cfg, unsigned features, fmd_meter* out);
int fmd_meter_features(fmd_meter m, unsigned* features);

typedef struct {
    int   L, taps_per_phase;          /* 4, 2 or 1; 12 */
    float taps[3][12];                /* taps[p - 1][k] = g_p[k], phases p = 1 ... L - 1; unused rows are 0 */
} fmd_meter_tp_design_t;
/* host only; the fs rule of fmd_meter_design */
int fmd_meter_tp_design(int fs, fmd_meter_tp_design_t* out);
double fmd_meter_dbtp(float peak);

/* one per station, 24 bytes: tp_call at byte 0, tp_hold 8, st_below 16, st_nonfinite 20.  The fields of a feature that is off stay 0 */
typedef struct {
    float    tp_call[2], tp_hold[2];  /* L, R: true peak of the last call that metered the station / since reset or reset_peaks */
    unsigned st_below, st_nonfinite;  /* short-term values under -70 LUFS / non-finite */
} fmd_meter_r128_status;
/* out [C]; synchronises with the meter's work.  FMD_ERR_STATE on a meter that has neither feature */
int fmd_meter_get_r128_status(fmd_meter m, fmd_meter_r128_status* out);
/* as fmd_meter_status_dev */
int fmd_meter_r128_status_dev(fmd_meter m, const fmd_meter_r128_status** d_out);
/* hist [C][1000]: the short-term values' counts per 0.1 LU bin; FMD_ERR_STATE on a meter without FMD_METER_RANGE */
int fmd_meter_get_range_histogram(fmd_meter m, unsigned* hist);
/* host only, pure: one station's [1000] range histogram -> lra in LU, low / high = the 10th / 95th percentile in LUFS.  FMD_ERR_STATE
 * when no bin survives the gates */
int fmd_meter_range(const unsigned* hist, const fmd_meter_design_t* d, double* lra, double* low, double* high);

/* ------------------------------------------------------------------------------------------------------------------
 * FM modulation monitor (NOT part of the reference): peak deviation (ITU-R SM.1268: peak hold over 50 ms intervals and the distribution
 * of those peaks), multiplex power (ITU-R BS.412), carrier frequency offset and pilot deviation of every station, measured where the
 * station's baseband already is.  It reads the device array [C][in_stride][2] (cf32 or u8) that the demodulator takes and the channeliser
 * writes, changes nothing in it, and keeps one fmd_modmon_status record and a 300-bin histogram per station.  It measures the RF signal,
 * not the audio.  Arithmetic, restated in C by tests/cpp/modmon_ref.c; T = 33 taps, NP = 64 partials, NB = 300 bins, RING = 60:
 *   input       u8 converts as (float)v - 127 (fmd_process_u8_*); everything below sees floats i, q.
 *   design      host, double, host libm (fmd_modmon_design); pi = 3.14159265358979323846; fs a multiple of 1000 in 192000 ... 384000:
 *                 M = fs / 20 (samples of a 50 ms interval);  P = fs / gcd(fs, 19000) (the pilot table's period, at most 384)
 *                 hz_per_rad = (double)fs / (2 * pi)
 *                 MPX low-pass, fc = 76000: w = 2 * fc / fs;  x = w * (i - 16);  r = (i - 16) / 16.0
 *                   g[i] = ((w * sinc(x)) * I0(5.0 * sqrt(1 - r * r))) / I0(5.0), i = 0 ... 32, sinc and I0 as in the true-peak design above
 *                   h[i] = (float)(g[i] / (sum over i ascending, from +0, of g[i]))
 *                 pilot_cos[k] = cos((2 * pi * (double)m) / (double)fs), pilot_sin[k] = sin(the same), m = (19000 * k) mod fs, k = 0 ... P - 1
 *                 pilot_gain = sqrt(re * re + im * im) * sinc(19000.0 / fs), with a_i = (2 * pi * (double)(19000 * i)) / (double)fs,
 *                   re = sum over i ascending, from +0, of (double)h[i] * cos(a_i), im likewise with sin
 *                   (the second factor is the difference discriminator's own response to a 19 kHz line)
 *                 edge[j] = 500.0 * j, j = 0 ... 300
 *   discriminator  fp32 (denormals kept), per station, n counted absolutely since the station's reset:
 *                 theta[n] = atan2f(q, i)                                          (the host libm's, fmd_math.h's fmd_atan2f on the device)
 *                 d[n] = wrap(theta[n] - theta[n-1]);  wrap(x) = x >= (float)pi ? x - 2 (float)pi : x <= -(float)pi ? x + 2 (float)pi : x
 *                 d[n] = +0.0f for n <= 0 (the first sample after a reset has no predecessor)
 *                 y[n] = fmaf(h[32], d[n-32], ... fmaf(h[1], d[n-1], fmaf(h[0], d[n], +0.0f)))      t ascending, from +0
 *               The 33 samples before a call's first are the station's history; a masked call and reset_peaks keep it.
 *   per sample  hi = fmaxf(hi, y), lo = fminf(lo, y) from -inf and +inf at each interval's start (a NaN leaves both as they are); the same
 *               two updates go into hold_hi and hold_lo (-inf and +inf at create, reset and reset_peaks).
 *                 fd = (double)y * hz_per_rad
 *               Interval g is the samples [g M, (g + 1) M), r = n - g M.  Partial j = r mod 64 takes its terms in ascending r, from +0:
 *                 s1_j = s1_j + fd;  s2_j = fma(fd, fd, s2_j);  sc_j = fma(fd, pilot_cos[n mod P], sc_j);  ss_j = fma(fd, pilot_sin[n mod P], ss_j)
 *               An open interval carries hi, lo and its 4 x 64 partials to the next call (2 KB per station).
 *   interval end  per sum the halving tree p_j += p_{j+w} for j < w, w = 32, 16, ... 1;  S = p_0.
 *                 D = 0.5 * ((double)hi - (double)lo) * hz_per_rad    (half the peak-to-peak swing: a mistuned carrier is not deviation)
 *                 last_hi, last_lo, last_s1, last_s2, last_sc, last_ss = hi, lo, S1, S2, Sc, Ss;  intervals++
 *                 D or S2 not finite -> nonfinite++ (the interval enters neither the histogram nor the second's sums)
 *                 else: D >= edge[300] -> over++, else hist[j]++ for the j with edge[j] <= D < edge[j + 1] (comparisons only); and
 *                       open_e += S2;  open_f += S1;  open_q += fma(Sc, Sc, Ss * Ss);  open_n += 1
 *                 every 20th interval completes a second: open_e, open_f, open_q, open_n go to sec_e, sec_f, sec_q, sec_n at index
 *                 [seconds % 60], seconds++, and the open sums return to +0.
 *               No floating-point atomics; ordinary stores.  Nothing depends, bit for bit, on how the samples are split into calls, on
 *               streams, on the format, on the batch or on the station's row.
 *   read-out    host, double, pure functions; FMD_ERR_STATE where there is nothing to read yet:
 *                 deviation_hz = D of the newest interval, from last_hi and last_lo          (intervals == 0 -> FMD_ERR_STATE)
 *                 offset_hz    = last_s1 / (double)M;   pilot_hz = 2 * sqrt(fma(sc, sc, ss * ss)) / (double)M / pilot_gain
 *                 mpx_power_dbr(window_s), 1 <= window_s <= 60: over the newest window_s completed seconds, oldest first, from +0:
 *                   e += sec_e, f += sec_f, k += sec_n;  N = (double)M * (double)k;  v = e / N - (f / N) * (f / N)
 *                   10 * log10(2 * v / (19000.0 * 19000.0)), -inf for v <= 0;  FMD_ERR_STATE while seconds < window_s or k == 0
 *                 exceedance(limit_hz), a multiple of 500 in 0 ... 150000: count = over + the bins from limit_hz / 500 up;
 *                   fraction = (double)count / (double)(over + all bins)
 *                 percentile(q), 0 <= q <= 1: n = over + all bins; the zero-based rank floor(q * (n - 1) + 0.5) by cumulative count falls
 *                   in bin j: 500.0 * j + 250.0 (the bin's centre), or 150000.0 where it falls among the `over` intervals
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_modmon_s* fmd_modmon;
typedef struct {
    int       n_channels;         /* C: station rows of the input */
    int       fs;                 /* the baseband's rate: a multiple of 1000 in 192000 ... 384000 */
    long long max_input_samples;  /* largest n of a process call, in (0, 2^30] */
    int       device;             /* HIP device ordinal, -1 = current */
} fmd_modmon_config;
typedef struct {
    int    fs, M, P, reserved;
    double hz_per_rad, pilot_gain;
    float  h[33], reserved_f;
    double pilot_cos[384], pilot_sin[384];           /* [0, P) used, the rest 0 */
    double edge[301];
} fmd_modmon_design_t;
/* one per station, 1792 bytes: samples at byte 0, intervals 8, seconds 16, last_hi 24, last_lo 28, hold_hi 32, hold_lo 36, last_s1 40,
 * last_s2 48, last_sc 56, last_ss 64, sec_e 72, sec_f 552, sec_q 1032, sec_n 1512, open_e 1752, open_f 1760, open_q 1768, open_n 1776,
 * over 1780, nonfinite 1784, reserved 1788 */
typedef struct {
    unsigned long long samples;       /* samples monitored since reset */
    unsigned long long intervals;     /* completed 50 ms intervals */
    unsigned long long seconds;       /* completed groups of 20 intervals */
    float    last_hi, last_lo;        /* extremes of y over the newest interval, in rad per sample */
    float    hold_hi, hold_lo;        /* extremes of y since reset or reset_peaks (-inf, +inf before the first sample) */
    double   last_s1, last_s2, last_sc, last_ss;   /* the newest interval's sums, in Hz and Hz^2 */
    double   sec_e[60], sec_f[60], sec_q[60];      /* second s at [s % 60]: sums of S2, S1 and Sc^2 + Ss^2 over its classified intervals */
    unsigned sec_n[60];               /* ... and their count */
    double   open_e, open_f, open_q;  /* the open second's sums */
    unsigned open_n;
    unsigned over, nonfinite;         /* intervals with D >= 150 kHz / with a non-finite D or S2 */
    unsigned reserved;
} fmd_modmon_status;

/* host-only (no GPU needed).  FMD_ERR_ARG unless fs is a multiple of 1000 in 192000 ... 384000 */
int fmd_modmon_design(int fs, fmd_modmon_design_t* out);
int fmd_modmon_deviation_hz(const fmd_modmon_status* s, const fmd_modmon_design_t* d, double* hz);
int fmd_modmon_offset_hz(const fmd_modmon_status* s, const fmd_modmon_design_t* d, double* hz);
int fmd_modmon_pilot_hz(const fmd_modmon_status* s, const fmd_modmon_design_t* d, double* hz);
int fmd_modmon_mpx_power_dbr(const fmd_modmon_status* s, const fmd_modmon_design_t* d, int window_s, double* dbr);
/* hist [300]: one station's histogram; over: its status record's counter */
int fmd_modmon_exceedance(const unsigned* hist, unsigned over, int limit_hz, double* fraction, unsigned long long* count);
int fmd_modmon_percentile(const unsigned* hist, unsigned over, double q, double* hz);

int fmd_modmon_create(const fmd_modmon_config* cfg, fmd_modmon* out);
int fmd_modmon_destroy(fmd_modmon m);
/* everything of station `channel` (-1 = every station) as after create: counters, sums, histogram, extremes and the 33-sample history.
 * Waits for the monitor's earlier work */
int fmd_modmon_reset(fmd_modmon m, int channel);
/* hold_hi and hold_lo of station `channel` (-1 = every station) to -inf and +inf; nothing else */
int fmd_modmon_reset_peaks(fmd_modmon m, int channel);
/* monitors n samples of every station.  d_in [C][in_stride][2] on the device, cf32 (8-byte aligned) or u8 (2-byte aligned); d_active:
 * [C] uint8 on the device, NULL = all: a station whose byte is 0 is skipped whole.  n < 0, n > in_stride, n > max_input_samples or a
 * misaligned d_in return FMD_ERR_ARG and change nothing; n == 0 is valid.  Asynchronous on `stream`; consecutive calls may use different
 * streams (the library orders them). */
int fmd_modmon_process_cf32_dev(fmd_modmon m, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, void* stream);
int fmd_modmon_process_u8_dev(fmd_modmon m, const uint8_t* d_in, long long in_stride, long long n, const uint8_t* d_active, void* stream);
/* out [C]; synchronises with the monitor's work */
int fmd_modmon_get_status(fmd_modmon m, fmd_modmon_status* out);
/* hist [C][300]: intervals per 500 Hz bin of D; synchronises with the monitor's work */
int fmd_modmon_get_histogram(fmd_modmon m, unsigned* hist);
/* the device's own [C] records, for a consumer on the device: ordered behind the monitor's work on the stream of its last process call,
 * valid until the next process call */
int fmd_modmon_status_dev(fmd_modmon m, const fmd_modmon_status** d_status);
const char* fmd_modmon_last_error(fmd_modmon m);

/* ------------------------------------------------------------------------------------------------------------------
 * Carrier squelch (NOT part of the reference, which tunes one station in hardware): whether there is a station in a channel at all,
 * and how clean it is.  It reads the device array [C][in_stride][2] (cf32 or u8) that the demodulator takes and the channeliser writes,
 * changes nothing in it, keeps per station and per 50 ms interval the two power moments S2 = sum |z|^2 and S4 = sum |z|^4, runs a
 * hysteresis gate on the device and writes the [C] uint8 mask that the mixer, the loudness meter and the modulation monitor take as
 * d_active, with no host round trip.
 *   The estimator: an FM carrier has a constant envelope A, channel noise is complex Gaussian of variance s^2.  Then E|z|^2 = A^2 + s^2
 *   and E|z|^4 = A^4 + 4 A^2 s^2 + 2 s^4, so 2 (E|z|^2)^2 - E|z|^4 = A^4: over M samples the carrier power is sqrt(2 S2^2 - M S4) / M and
 *   the noise power what remains of S2 / M.  With k = 10^(dB / 10), "CNR > dB" is (2 S2^2 - M S4) > (k^2 / (1 + k)^2) S2^2: no square
 *   root, division or logarithm on the device.  The figure is an ENVELOPE-CONSTANCY carrier-to-noise ratio, not a calibrated one:
 *   multipath, fading, adjacent-channel leakage and a clipping converter all break the constant envelope and read as a lower ratio (a u8
 *   input whose peak reaches the rails reads wrong: last_peak and hold_peak exist to flag that).  That is what a squelch wants.
 * Arithmetic, restated in C by tests/cpp/squelch_ref.c; NP = 256 partials, RING = 20 intervals (one second):
 *   input       u8 converts as (float)v - 127 (fmd_process_u8_*); everything below sees floats i, q.  fp32 and fp64 denormals are kept.
 *   design      host, double, host libm; fs a multiple of 1000 in 192000 ... 384000 (the modulation monitor's range: at 1.024 and
 *               2.048 MSa/s a station's feed holds its neighbours and the envelope is not constant):
 *                 M = fs / 20 (samples of a 50 ms interval)
 *                 threshold(db) = (k * k) / ((1 + k) * (1 + k)), k = pow(10, db / 10);  c_open = threshold(open_db), c_close likewise
 *                 min_s2 = pow(10, min_level_db / 10) * M, and +0 for min_level_db = -inf
 *   per sample  n counted absolutely in 64 bits since the station's reset; interval g = n / M, r = n - g M.
 *                 I = (double)i, Q = (double)q;  p = fma(I, I, Q * Q)          (the product is exact in double)
 *               Partial j = r mod 256 takes its terms in ascending r, from +0 at the interval's start:
 *                 s2_j = s2_j + p;  s4_j = fma(p, p, s4_j)
 *                 pk = fmaxf(pk, fmaxf(fabsf(i), fabsf(q))) from +0 at the interval's start (a NaN is dropped); the same update goes into
 *                 hold_peak (+0 at create, reset and reset_peaks).
 *               An open interval carries pk and its 2 x 256 partials to the next call (4 KB per station).
 *   interval end  per sum the halving tree p_j += p_{j+w} for j < w, w = 128, 64, ... 1;  S = p_0.
 *                 ring_s2[g % 20] = S2, ring_s4[g % 20] = S4, last_peak = pk, intervals++
 *                 finite = isfinite(S2) && isfinite(S4);  not finite -> nonfinite++
 *                 a = S2 * S2;  d = fma(-(double)M, S4, 2.0 * a)
 *                 good_open = finite && S2 >= min_s2 && d > c_open * a;  good_close the same with c_close.  The comparisons are strict:
 *                 an all-zero interval is not good, and a NaN compares false.
 *   gate        closed: run = good_open ? run + 1 : 0;  run >= open_intervals -> the gate opens, run = 0, transitions++
 *               open:   run = good_close ? 0 : run + 1; run >= close_intervals -> the gate closes, run = 0, transitions++
 *               intervals_open++ where the gate is open after the update.
 *               mask byte = mode == FMD_SQUELCH_AUTO ? open : (mode == FMD_SQUELCH_FORCE_OPEN).  The state machine runs in every mode.
 *               No atomics; ordinary stores.  Nothing depends, bit for bit, on how the samples are split into calls, on streams, on the
 *               format, on the batch or on the station's row.
 *   read-out    host, double, pure functions; fs as in the design (else FMD_ERR_ARG); FMD_ERR_STATE while intervals < window:
 *                 level_db = 10 * log10(ring_s2[newest] / (double)M)                      (window = 1)
 *                 cnr_db(window), 1 <= window <= 20: over the newest `window` intervals, oldest first, from +0: e2 += ring_s2, e4 += ring_s4;
 *                   N = (double)M * (double)window;  d = fma(-N, e4, 2 * e2 * e2);  d <= 0 -> -inf
 *                   c = sqrt(d) / N;  nz = e2 / N - c;  nz <= 0 -> +inf;  else 10 * log10(c / nz)
 *                   (a NaN or infinite ring entry in the window makes d a NaN, and the result is a NaN)
 *                 powers(window): c and nz of the same sums (d <= 0: c = 0 and nz = e2 / N)
 * ------------------------------------------------------------------------------------------------------------------ */
#define FMD_SQUELCH_AUTO         0   /* the mask byte follows the gate */
#define FMD_SQUELCH_FORCE_OPEN   1   /* the mask byte is 1 */
#define FMD_SQUELCH_FORCE_CLOSED 2   /* the mask byte is 0 */
typedef struct fmd_squelch_s* fmd_squelch;
typedef struct {
    int       n_channels;         /* C: station rows of the input */
    int       fs;                 /* the baseband's rate: a multiple of 1000 in 192000 ... 384000 */
    long long max_input_samples;  /* largest n of a process call, in (0, 2^30] */
    int       device;             /* HIP device ordinal, -1 = current */
} fmd_squelch_config;
/* defaults: 10.0, 7.0, -inf, 2, 10, FMD_SQUELCH_AUTO.  Valid: 0 <= close_db <= open_db <= 60; min_level_db = -inf or finite;
 * open_intervals and close_intervals in 1 ... 1000; mode one of FMD_SQUELCH_* */
typedef struct {
    double open_db, close_db;     /* the gate opens above open_db and stays open above close_db, in dB of envelope-constancy CNR */
    double min_level_db;          /* an interval below this mean power, 10 log10(S2 / M) in the input's own units, is never good */
    int    open_intervals;        /* good intervals in a row that open the gate */
    int    close_intervals;       /* bad intervals in a row that close it (the hold) */
    int    mode;
} fmd_squelch_params;
/* one per station, 368 bytes: samples at byte 0, intervals 8, intervals_open 16, ring_s2 24, ring_s4 184, last_peak 344, hold_peak 348,
 * run 352, transitions 356, nonfinite 360, open 364, mode 365, reserved 366 */
typedef struct {
    unsigned long long samples;        /* samples seen since reset */
    unsigned long long intervals;      /* completed 50 ms intervals */
    unsigned long long intervals_open; /* ... of them with the gate open after their update */
    double   ring_s2[20], ring_s4[20]; /* interval g at [g % 20]: sum |z|^2 and sum |z|^4 */
    float    last_peak;                /* max(|i|, |q|) over the newest interval */
    float    hold_peak;                /* ... since reset or reset_peaks */
    unsigned run;                      /* the gate's run of good (closed) or bad (open) intervals */
    unsigned transitions;              /* openings and closings since reset */
    unsigned nonfinite;                /* intervals with a non-finite S2 or S4 */
    unsigned char open;                /* the gate: 1 open, 0 closed */
    unsigned char mode;                /* the station's FMD_SQUELCH_* mode */
    unsigned char reserved[2];
} fmd_squelch_status;

/* host-only (no GPU needed) */
void fmd_squelch_default_params(fmd_squelch_params* p);
/* (k * k) / ((1 + k) * (1 + k)), k = pow(10, db / 10): what d / S2^2 is compared with */
double fmd_squelch_threshold(double db);
int fmd_squelch_level_db(const fmd_squelch_status* s, int fs, double* db);
int fmd_squelch_cnr_db(const fmd_squelch_status* s, int fs, int window, double* db);
int fmd_squelch_powers(const fmd_squelch_status* s, int fs, int window, double* carrier, double* noise);

int fmd_squelch_create(const fmd_squelch_config* cfg, fmd_squelch* out);
int fmd_squelch_destroy(fmd_squelch q);
/* everything of station `channel` (-1 = every station) as after create: counters, ring, peaks, the open interval and the gate (closed);
 * its parameters are kept.  Waits for the squelch's earlier work */
int fmd_squelch_reset(fmd_squelch q, int channel);
/* hold_peak of station `channel` (-1 = every station) to +0; nothing else */
int fmd_squelch_reset_peaks(fmd_squelch q, int channel);
/* the parameters of station `channel` (-1 = every station): ordered behind the squelch's earlier work, they apply from the next interval
 * that ends.  FMD_ERR_ARG for values outside the ranges above, and nothing changes */
int fmd_squelch_set_params(fmd_squelch q, int channel, const fmd_squelch_params* p);
int fmd_squelch_get_params(fmd_squelch q, int channel, fmd_squelch_params* p);
/* takes n samples of every station.  d_in [C][in_stride][2] on the device, cf32 (8-byte aligned) or u8 (2-byte aligned); d_active: [C]
 * uint8 on the device, NULL = all: a station whose byte is 0 is skipped whole, and its mask byte is left as it is.  d_mask: [C] uint8 on
 * the device, caller-owned, may be NULL: behind its work on `stream` the call writes every other station's byte, 1 or 0, also when
 * n == 0 and for a station whose gate did not move.  n < 0, n > in_stride, n > max_input_samples or a misaligned d_in return FMD_ERR_ARG
 * and change nothing.  Asynchronous on `stream`; consecutive calls may use different streams (the library orders them). */
int fmd_squelch_process_cf32_dev(fmd_squelch q, const float* d_in, long long in_stride, long long n, const uint8_t* d_active,
                                 uint8_t* d_mask, void* stream);
int fmd_squelch_process_u8_dev(fmd_squelch q, const uint8_t* d_in, long long in_stride, long long n, const uint8_t* d_active,
                               uint8_t* d_mask, void* stream);
/* out [C]; synchronises with the squelch's work */
int fmd_squelch_get_status(fmd_squelch q, fmd_squelch_status* out);
/* the device's own [C] records, for a consumer on the device: ordered behind the squelch's work on the stream of its last process call,
 * valid until the next process call */
int fmd_squelch_status_dev(fmd_squelch q, const fmd_squelch_status** d_status);
const char* fmd_squelch_last_error(fmd_squelch q);

/* ------------------------------------------------------------------------------------------------------------------
 * Audio fault monitor (NOT part of the reference): the faults of the demodulated programme that a broadcast monitor alarms on first --
 * dead air (the carrier is up, the programme is silent), a lost rail (one of L / R is gone), antiphase (L and R cancel in every mono
 * receiver and in a bus that sums stations) and a mono programme on a station that should be stereo.  It reads the device array
 * [C][in_stride][2] f32 (interleaved L, R) that the resampler, the mixer and the loudness meter read -- fmd_audio_dev's view or a
 * resampler's output -- changes nothing in it, keeps per station and per 100 ms interval the sums LL = sum L^2, RR = sum R^2,
 * LR = sum L R and the two rail peaks, runs five hysteresis detectors on the device with comparisons only, and writes a [C] uint8 flags
 * byte and a [C] uint8 ok byte per station.  The ok bytes are what the mixer takes as d_active: a dead or antiphase station leaves a
 * bus with no host round trip.  (The loudness meter does not answer these questions: its energies are K-weighted, summed over both
 * rails, and it keeps no cross term.)
 * Arithmetic, restated in C by tests/cpp/audmon_ref.c; NP = 64 partials, RING = 30 intervals (three seconds), five detectors:
 *   design      host, double, host libm; fs a multiple of 10 in 8000 ... 192000 (the loudness meter's range):
 *                 M = fs / 10 (frames of a 100 ms interval)
 *                 min_e  = pow(10, silence_db / 10) * (2.0 * (double)M), and +0 for silence_db = -inf
 *                 c_loss = pow(10, -loss_db / 10);  c_anti = antiphase_corr * antiphase_corr;  c_mono = pow(10, -mono_db / 10)
 *   per frame   n counted absolutely in 64 bits since the station's reset; interval g = n / M, r = n - g M.
 *                 l = (double)L, r_ = (double)R                                  (every product below is exact in double)
 *               Partial j = (r >> 2) & 63 takes its terms in ascending r, from +0 at the interval's start:
 *                 ll_j = fma(l, l, ll_j);  rr_j = fma(r_, r_, rr_j);  lr_j = fma(l, r_, lr_j)
 *                 pkL = fmaxf(pkL, fabsf(L)), pkR = fmaxf(pkR, fabsf(R)) from +0 at the interval's start (a NaN is dropped); the same
 *                 updates go into hold_peak[0], hold_peak[1] (+0 at create, reset and reset_peaks).
 *               fp32 and fp64 denormals are kept.  An open interval carries its two peaks and its 3 x 64 partials (1.5 KB per station)
 *               to the next call.
 *   interval end  per sum the halving tree p_j += p_{j+w} for j < w, w = 32, 16, ... 1;  S = p_0: LL, RR, LR.
 *                 ring_ll[g % 30] = LL, ring_rr[g % 30] = RR, ring_lr[g % 30] = LR, last_peak = {pkL, pkR}, intervals++
 *                 finite = isfinite(LL) && isfinite(RR) && isfinite(LR);  not finite -> nonfinite++
 *                 E = LL + RR
 *                 bad[0] = !(finite && E > min_e)        strict: digital silence is silent at any threshold, also at -inf, and an
 *                                                        interval that is not finite counts as no usable programme
 *                 only where bad[0] is false:
 *                   bad[1] = LL < c_loss * RR
 *                   bad[2] = RR < c_loss * LL
 *                   bad[3] = LR < 0 && LR * LR > c_anti * (LL * RR)
 *                   S = fma(-2.0, LR, E);  Md = fma(2.0, LR, E);  bad[4] = S < c_mono * Md        (S = sum (L - R)^2, Md = sum (L + R)^2)
 *                 where bad[0] is true, detectors 1 ... 4 HOLD: their flag and their run do not change (silence says nothing about
 *                 phase or balance).
 *   detector k  (bit k of flags; k = 0 always runs, k = 1 ... 4 unless held)
 *               flag clear: run = bad ? run + 1 : 0;  run >= raise_intervals[k] -> the flag is set, run = 0, transitions[k]++
 *               flag set:   run = bad ? 0 : run + 1;  run >= clear_intervals[k] -> the flag is cleared, run = 0, transitions[k]++
 *               intervals_flagged[k]++ where the flag is set after the interval, held or not.
 *   bytes       flags = the five bits;  ok = (flags & alarm_mask) == 0, with the station's alarm_mask as it is when the bytes are written
 *               (a process call, set_params, reset).  No atomics; ordinary stores.  Nothing depends, bit for bit, on how the frames are
 *               split into calls, on streams, on the batch or on the station's row.
 *   read-out    host, double, pure functions over one record; fs as in the design and 1 <= window <= 30 (else FMD_ERR_ARG);
 *               FMD_ERR_STATE while intervals < window.  Over the newest `window` intervals, oldest first, from +0:
 *                 ll += ring_ll, rr += ring_rr, lr += ring_lr;  N = (double)M * (double)window
 *                 level_db(rail): 0 (L) 10 * log10(ll / N);  1 (R) 10 * log10(rr / N);  2 (both) 10 * log10((ll + rr) / (2.0 * N))
 *                 balance_db     10 * log10(ll / rr)
 *                 correlation    lr / sqrt(ll * rr)
 *                 side_mid_db    10 * log10(fma(-2.0, lr, ll + rr) / fma(2.0, lr, ll + rr))
 *               Nothing is special-cased: where a division is 0 / 0 (silence: balance, correlation and side / mid) or a ring entry is
 *               not finite, the IEEE result is returned as it comes -- a NaN, or -inf for the level of silence and for the side / mid
 *               ratio of R == L.
 * ------------------------------------------------------------------------------------------------------------------ */
#define FMD_AUDMON_SILENCE    1u    /* detector 0: the interval's energy is not above the silence threshold */
#define FMD_AUDMON_LEFT_LOST  2u    /* detector 1: L is loss_db or more below R */
#define FMD_AUDMON_RIGHT_LOST 4u    /* detector 2: R is loss_db or more below L */
#define FMD_AUDMON_ANTIPHASE  8u    /* detector 3: the correlation of L and R is below -antiphase_corr */
#define FMD_AUDMON_MONO       16u   /* detector 4: the side signal is mono_db or more below the mid signal */
typedef struct fmd_audmon_s* fmd_audmon;
typedef struct {
    int       n_channels;         /* C: station rows of the input */
    int       fs;                 /* the audio's rate: a multiple of 10 in 8000 ... 192000 */
    long long max_input_frames;   /* largest n of a process call, in (0, 2^30] */
    int       device;             /* HIP device ordinal, -1 = current */
} fmd_audmon_config;
/* defaults: -60.0, 30.0, 0.5, 40.0, {100, 100, 100, 50, 100}, {10, 10, 10, 10, 10}, 15 (MONO is an indication, not an alarm).
 * Valid: silence_db = -inf or finite; loss_db and mono_db in (0, 120]; antiphase_corr in (0, 1); every raise_intervals and
 * clear_intervals in 1 ... 36000 (an hour); alarm_mask with no bit above bit 4.  80 bytes */
typedef struct {
    double   silence_db;          /* an interval whose mean power over both rails, 10 log10(E / 2M), is not above this is silent */
    double   loss_db;             /* a rail this far below the other is lost */
    double   antiphase_corr;      /* L and R are in antiphase where their correlation is below minus this */
    double   mono_db;             /* the programme is mono where side is this far below mid */
    int      raise_intervals[5];  /* bad intervals in a row that set detector k's flag */
    int      clear_intervals[5];  /* good intervals in a row that clear it */
    unsigned alarm_mask;          /* the FMD_AUDMON_* flags that take the station's ok byte to 0 */
} fmd_audmon_params;
/* one per station, 840 bytes: frames at byte 0, intervals 8, intervals_flagged 16, ring_ll 56, ring_rr 296, ring_lr 536, last_peak 776,
 * hold_peak 784, run 792, transitions 812, nonfinite 832, flags 836, ok 837, reserved 838 */
typedef struct {
    unsigned long long frames;               /* frames seen since reset */
    unsigned long long intervals;            /* completed 100 ms intervals */
    unsigned long long intervals_flagged[5]; /* ... of them with detector k's flag set after the interval */
    double   ring_ll[30], ring_rr[30], ring_lr[30]; /* interval g at [g % 30]: sum L^2, sum R^2, sum L R */
    float    last_peak[2];                   /* max |L|, max |R| over the newest interval */
    float    hold_peak[2];                   /* ... since reset or reset_peaks */
    unsigned run[5];                         /* detector k's run of bad (flag clear) or good (flag set) intervals */
    unsigned transitions[5];                 /* raises and clears of detector k since reset */
    unsigned nonfinite;                      /* intervals with a non-finite LL, RR or LR */
    unsigned char flags;                     /* FMD_AUDMON_* */
    unsigned char ok;                        /* (flags & alarm_mask) == 0 */
    unsigned char reserved[2];
} fmd_audmon_status;

/* host-only (no GPU needed) */
void fmd_audmon_default_params(fmd_audmon_params* p);
/* rail: 0 L, 1 R, 2 both */
int fmd_audmon_level_db(const fmd_audmon_status* s, int fs, int rail, int window, double* db);
int fmd_audmon_balance_db(const fmd_audmon_status* s, int fs, int window, double* db);
int fmd_audmon_correlation(const fmd_audmon_status* s, int fs, int window, double* corr);
int fmd_audmon_side_mid_db(const fmd_audmon_status* s, int fs, int window, double* db);

int fmd_audmon_create(const fmd_audmon_config* cfg, fmd_audmon* out);
int fmd_audmon_destroy(fmd_audmon a);
/* everything of station `channel` (-1 = every station) as after create: counters, ring, peaks, the open interval, the detectors (every
 * flag clear, ok = 1); its parameters are kept.  Waits for the monitor's earlier work */
int fmd_audmon_reset(fmd_audmon a, int channel);
/* hold_peak of station `channel` (-1 = every station) to +0; nothing else */
int fmd_audmon_reset_peaks(fmd_audmon a, int channel);
/* the parameters of station `channel` (-1 = every station): ordered behind the monitor's earlier work, they apply from the next interval
 * that ends (alarm_mask: from the next bytes written, the record's ok at once).  FMD_ERR_ARG for values outside the ranges above, and
 * nothing changes */
int fmd_audmon_set_params(fmd_audmon a, int channel, const fmd_audmon_params* p);
int fmd_audmon_get_params(fmd_audmon a, int channel, fmd_audmon_params* p);
/* takes n frames of every station.  d_in [C][in_stride][2] f32 on the device, 8-byte aligned; d_active: [C] uint8 on the device,
 * NULL = all: a station whose byte is 0 is skipped whole, and its two output bytes are left as they are.  d_flags, d_ok: [C] uint8 on
 * the device, caller-owned, each may be NULL: behind its work on `stream` the call writes every other station's byte, also when n == 0
 * and for a station whose detectors did not move.  n < 0, n > in_stride, n > max_input_frames or a misaligned d_in return FMD_ERR_ARG
 * and change nothing.  Asynchronous on `stream`; consecutive calls may use different streams (the library orders them). */
int fmd_audmon_process_f32_dev(fmd_audmon a, const float* d_in, long long in_stride, long long n, const uint8_t* d_active,
                               uint8_t* d_flags, uint8_t* d_ok, void* stream);
/* out [C]; synchronises with the monitor's work */
int fmd_audmon_get_status(fmd_audmon a, fmd_audmon_status* out);
/* the device's own [C] records, for a consumer on the device: ordered behind the monitor's work on the stream of its last process call,
 * valid until the next process call */
int fmd_audmon_status_dev(fmd_audmon a, const fmd_audmon_status** d_status);
const char* fmd_audmon_last_error(fmd_audmon a);

/* ------------------------------------------------------------------------------------------------------------------
 * Audio tone detector (NOT part of the reference): what is on the air when the programme has been replaced by a steady tone -- a line-up
 * tone left on a transmitter (1 kHz, 440 Hz, 400 Hz), the two-tone EAS attention signal (853 Hz + 960 Hz), the 1050 Hz weather-radio
 * alert.  A -12 dBFS sine is neither silent nor mono and measures as healthy loudness, so neither the fault monitor nor the loudness
 * meter sees it.  It reads the device array [C][in_stride][2] f32 (interleaved L, R) that the mixer, the meter and the fault monitor
 * read, changes nothing in it, measures per station and per 100 ms interval up to eight tone slots -- the power of the mid signal
 * m = L + R at the slot's frequency (a Goertzel / single-bin DFT sum against a table) over the mid signal's total power -- runs one
 * hysteresis detector per slot on the device with comparisons only, and writes a [C] uint8 flags byte (bit k: slot k's tone is present)
 * and a [C] uint8 ok byte per station, which the mixer takes as d_active.
 * Arithmetic, restated in C by tests/cpp/tonedet_ref.c; NP = 64 partials, RING = 30 intervals (three seconds), NS = 8 slots:
 *   design      host, double, host libm; fs a multiple of 10 in 8000 ... 48000:
 *                 M = fs / 10 (frames of a 100 ms interval)
 *                 tc[j] = cos(2.0 * M_PI * (double)j / (double)fs), ts[j] = sin(2.0 * M_PI * (double)j / (double)fs), j = 0 ... fs - 1:
 *                 one table per handle, uploaded once (16 bytes an entry, 768 KB at most)
 *                 min_e = pow(10, floor_db / 10) * (double)M, and +0 for floor_db = -inf
 *                 c_k   = pow(10, -share_db[k] / 10)
 *   slot k      an integer frequency f_k in Hz (the resolution is 1 Hz: 853 is no multiple of 10); 0 = unused, else 1 <= f_k and
 *               2 f_k < fs.  The phase restarts at every interval's start (the power does not depend on it).
 *   per frame   n counted absolutely in 64 bits since the station's reset; interval g = n / M, r = n - g M.
 *                 m = (double)L + (double)R                                      (one rounding)
 *                 idx_k = (f_k * r) mod fs                                       (the product is below 2^31)
 *               Partial j = (r >> 2) & 63 takes its terms in ascending r, from +0 at the interval's start:
 *                 mm_j = fma(m, m, mm_j)
 *                 for every used slot:  re_kj = fma(m, tc[idx_k], re_kj);  im_kj = fma(m, ts[idx_k], im_kj)
 *               fp32 and fp64 denormals are kept.  An open interval carries its 17 x 64 partials (8.5 KB per station) to the next call.
 *   interval end  per sum the halving tree p_j += p_{j+w} for j < w, w = 32, 16, ... 1;  S = p_0: MM, RE_k, IM_k.
 *                 PW_k = fma(RE_k, RE_k, IM_k * IM_k);  an unused slot has PW_k = +0
 *                 ring_mm[g % 30] = MM, ring_pw[k][g % 30] = PW_k, intervals++
 *                 MM not finite -> nonfinite++;  usable = isfinite(MM) && MM > min_e
 *                 present[k] = usable && isfinite(PW_k) && 2.0 * PW_k > c_k * ((double)M * MM)
 *                 (a pure sine at f_k has 2 PW_k = M MM; an unused slot is never present; an unusable interval carries no tone)
 *   detector k  (bit k of flags; every detector runs at every interval's end: there is no hold)
 *               flag clear: run = present ? run + 1 : 0;  run >= raise_intervals[k] -> the flag is set, run = 0, transitions[k]++
 *               flag set:   run = present ? 0 : run + 1;  run >= clear_intervals[k] -> the flag is cleared, run = 0, transitions[k]++
 *               intervals_flagged[k]++ where the flag is set after the interval.
 *   frequencies the record's freq_hz is what the open interval is measured with.  set_params' frequencies are pending: they come into
 *               force when an interval ends (for the next one), at a reset, and at set_params itself where no interval is open
 *               (frames == intervals * M).  The open interval finishes on the old frequencies.
 *   bytes       flags = the eight bits;  ok = (flags & alarm_mask) == 0, with the station's alarm_mask as it is when the bytes are written
 *               (a process call, set_params, reset).  No atomics; ordinary stores.  Nothing depends, bit for bit, on how the frames are
 *               split into calls, on streams, on the batch or on the station's row.
 *   read-out    host, double, pure functions over one record; fs as in the design, 0 <= slot < 8 and 1 <= window <= 30 (else
 *               FMD_ERR_ARG); FMD_ERR_STATE while intervals < window.  Over the newest `window` intervals, oldest first, from +0:
 *                 pw += ring_pw[slot], mm += ring_mm
 *                 share_db  10.0 * log10(2.0 * pw / ((double)M * mm))                       the tone's share of the mid signal's power
 *                 level_db  10.0 * log10(2.0 * pw / ((double)M * (double)M * (double)window)) the mean square of the tone's part of m
 *               Nothing is special-cased: IEEE results are returned as they come (NaN for 0 / 0, -inf for no power in the slot).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_tonedet_s* fmd_tonedet;
typedef struct {
    int       n_channels;         /* C: station rows of the input */
    int       fs;                 /* the audio's rate: a multiple of 10 in 8000 ... 48000 */
    long long max_input_frames;   /* largest n of a process call, in (0, 2^30] */
    int       device;             /* HIP device ordinal, -1 = current */
} fmd_tonedet_config;
/* defaults: {1000, 440, 400, 853, 960, 1050, 0, 0}, {3, 3, 3, 6, 6, 3, 3, 3}, -50.0, 20 for all, 5 for all, 0 (a tone is an indication
 * until the user makes it an alarm).  Valid: every freq_hz 0 or 1 <= f and 2 f < fs; every share_db in [0, 60]; floor_db = -inf or
 * finite; every raise_intervals and clear_intervals in 1 ... 36000 (an hour); alarm_mask with no bit above bit 7.  176 bytes */
typedef struct {
    int      freq_hz[8];          /* slot k's frequency in Hz, 0 = unused */
    double   share_db[8];         /* slot k's tone is present where its power is no more than this far below the mid signal's */
    double   floor_db;            /* an interval whose mid signal's mean square, 10 log10(MM / M), is not above this carries no tone */
    int      raise_intervals[8];  /* intervals with the tone in a row that set slot k's flag */
    int      clear_intervals[8];  /* intervals without it in a row that clear it */
    unsigned alarm_mask;          /* the slots (bit k) whose flag takes the station's ok byte to 0 */
} fmd_tonedet_params;
/* one per station, 2344 bytes: frames at byte 0, intervals 8, intervals_flagged 16, ring_mm 80, ring_pw 320, run 2240, transitions 2272,
 * nonfinite 2304, freq_hz 2308, flags 2340, ok 2341, reserved 2342 */
typedef struct {
    unsigned long long frames;               /* frames seen since reset */
    unsigned long long intervals;            /* completed 100 ms intervals */
    unsigned long long intervals_flagged[8]; /* ... of them with slot k's flag set after the interval */
    double   ring_mm[30];                    /* interval g at [g % 30]: sum m^2 */
    double   ring_pw[8][30];                 /* ... and slot k's RE^2 + IM^2 */
    unsigned run[8];                         /* slot k's run of intervals with (flag clear) or without (flag set) its tone */
    unsigned transitions[8];                 /* raises and clears of slot k since reset */
    unsigned nonfinite;                      /* intervals with a non-finite MM */
    int      freq_hz[8];                     /* the frequencies in force: what the open interval is measured with */
    unsigned char flags;                     /* bit k: slot k's tone is present */
    unsigned char ok;                        /* (flags & alarm_mask) == 0 */
    unsigned char reserved[2];
} fmd_tonedet_status;

/* host-only (no GPU needed) */
void fmd_tonedet_default_params(fmd_tonedet_params* p);
int fmd_tonedet_share_db(const fmd_tonedet_status* s, int fs, int slot, int window, double* db);
int fmd_tonedet_level_db(const fmd_tonedet_status* s, int fs, int slot, int window, double* db);

int fmd_tonedet_create(const fmd_tonedet_config* cfg, fmd_tonedet* out);
int fmd_tonedet_destroy(fmd_tonedet t);
/* everything of station `channel` (-1 = every station) as after create: counters, ring, the open interval, the detectors (every flag
 * clear, ok = 1); its parameters are kept and its frequencies come into force.  Waits for the detector's earlier work */
int fmd_tonedet_reset(fmd_tonedet t, int channel);
/* the parameters of station `channel` (-1 = every station): ordered behind the detector's earlier work.  Frequencies apply from the next
 * interval that starts; every other field from the next interval that ends (alarm_mask: from the next bytes written, the record's ok
 * at once).  FMD_ERR_ARG for values outside the ranges above, and nothing changes */
int fmd_tonedet_set_params(fmd_tonedet t, int channel, const fmd_tonedet_params* p);
int fmd_tonedet_get_params(fmd_tonedet t, int channel, fmd_tonedet_params* p);
/* takes n frames of every station.  d_in [C][in_stride][2] f32 on the device, 8-byte aligned; d_active: [C] uint8 on the device,
 * NULL = all: a station whose byte is 0 is skipped whole, and its two output bytes are left as they are.  d_flags, d_ok: [C] uint8 on
 * the device, caller-owned, each may be NULL: behind its work on `stream` the call writes every other station's byte, also when n == 0
 * and for a station whose detectors did not move.  n < 0, n > in_stride, n > max_input_frames or a misaligned d_in return FMD_ERR_ARG
 * and change nothing.  Asynchronous on `stream`; consecutive calls may use different streams (the library orders them). */
int fmd_tonedet_process_f32_dev(fmd_tonedet t, const float* d_in, long long in_stride, long long n, const uint8_t* d_active,
                                uint8_t* d_flags, uint8_t* d_ok, void* stream);
/* out [C]; synchronises with the detector's work */
int fmd_tonedet_get_status(fmd_tonedet t, fmd_tonedet_status* out);
/* the device's own [C] records, for a consumer on the device: ordered behind the detector's work on the stream of its last process
 * call, valid until the next process call */
int fmd_tonedet_status_dev(fmd_tonedet t, const fmd_tonedet_status** d_status);
const char* fmd_tonedet_last_error(fmd_tonedet t);

/* ------------------------------------------------------------------------------------------------------------------
 * ADPCM audio encoder (NOT part of the reference): station recordings at a quarter of the 16-bit PCM bytes, as block IMA / DVI ADPCM, the
 * WAV format tag 0x0011 that ordinary players and tools open.  The first side object that is a sink: it reads the device array
 * [C][in_stride][2] f32 (interleaved L, R) that the mixer and the monitors read, changes nothing in it, and writes every station's
 * completed blocks to a caller-owned device array: 32 KB/s per station at 32 kHz, where 16-bit PCM is 128 KB/s.  Stereo only.
 * Arithmetic, restated in C by tests/cpp/adpcm_ref.c; all integer behind one fp32 multiply:
 *   sample      t = x * (32767.0f * 0.95f)                      one fp32 multiply, round to nearest: the scraper's scale (fmd_audio_pcm16_dev)
 *               t NaN or +-inf:  q = 0, the station's nonfinite++ (per sample)
 *               otherwise        v = (int)t, truncated toward zero;  v > 32767 -> q = 32767, v < -32768 -> q = -32768, each with the
 *                                rail's clipped++;  else q = v.  For every in-range sample q is fmd_audio_pcm16_dev's value.
 *   step        the IMA / DVI reference quantiser over (pred, index) per rail, with the 89-entry step table and the index table
 *               {-1, -1, -1, -1, 2, 4, 6, 8}:
 *                 step = table[index];  diff = q - pred;  code = 8 where diff < 0, and diff = -diff then;  vpdiff = step >> 3
 *                 diff >= step      -> code |= 4, diff -= step,      vpdiff += step
 *                 diff >= step >> 1 -> code |= 2, diff -= step >> 1, vpdiff += step >> 1
 *                 diff >= step >> 2 -> code |= 1,                    vpdiff += step >> 2
 *                 pred = pred -+ vpdiff by the sign, clamped to int16;  index += index table[code & 7], clamped to 0 ... 88
 *               (what Python's audioop.lin2adpcm(..., 2, (pred, index)) computes.)
 *   block       S = block_frames frames, S = 1 (mod 8), 9 <= S <= 8185, default 1017;  block_align = 8 * ((S - 1) / 8 + 1) bytes
 *               (1024 for the default, 31.8 ms at 32 kHz).
 *                 bytes 0-1  q(L) of the block's first frame, int16 little-endian;  byte 2  L's index as it stands (0 after a reset,
 *                 else what the previous block's last frame left: the index is carried from block to block);  byte 3  0
 *                 bytes 4-7  the same for R
 *               At the block's first frame each rail's pred is set to the header sample itself and no code is emitted.  Then per further
 *               eight frames four bytes of L codes and four bytes of R codes, the earlier frame in the low nibble.
 *   streaming   frames are counted per station since its reset.  The open block's bytes, its fill count, each rail's pred and index
 *               live in the encoder and carry to the next call.  A call of n frames completes (fill + n) / S blocks for the station,
 *               writes them back to back at d_out + c * out_stride and their number to d_nblocks[c]; bytes of d_out behind them are left
 *               as they are.  Stations may stand at different places in their blocks.  Nothing depends, bit for bit, on how the frames
 *               are split into calls, on streams, on the batch or on the station's row.  Ordinary stores, no atomics.
 *   flush       closes the station's open block: repeats of the last real frame's (q(L), q(R)) are encoded until the block is full,
 *               the block is written at d_out + c * out_stride and 1 to d_nblocks[c];  padded += S - fill, blocks++, fill = 0, pred and
 *               index carried on.  With fill == 0 nothing of the station changes and d_nblocks[c] = 0.
 *   decoder     per block and rail from the header's (pred, index):  vpdiff = step >> 3, + step, + step >> 1, + step >> 2 by the code's
 *               bits 2, 1, 0;  pred and index move as in the encoder.  (audioop.adpcm2lin.)
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_adpcm_s* fmd_adpcm;
typedef struct {
    int       n_channels;         /* C: station rows of the input */
    int       block_frames;       /* S: frames of a block, 1 (mod 8) in 9 ... 8185; 0 = 1017 */
    long long max_input_frames;   /* largest n of a process call, in (0, 2^30] */
    int       device;             /* HIP device ordinal, -1 = current */
} fmd_adpcm_config;
/* one per station, 64 bytes: frames at byte 0, blocks 8, padded 16, clipped 24, nonfinite 40, fill 48, pred 52, index 56, reserved 58 */
typedef struct {
    unsigned long long frames;        /* frames taken since reset */
    unsigned long long blocks;        /* blocks completed since reset, the flushed ones among them */
    unsigned long long padded;        /* frames that flushes repeated to fill their blocks: frames + padded = blocks * S + fill */
    unsigned long long clipped[2];    /* samples of L, R clamped to the 16-bit range */
    unsigned long long nonfinite;     /* samples (of either rail) that were NaN or +-inf after the scale: encoded as 0 */
    unsigned           fill;          /* frames in the open block, 0 ... S - 1 */
    short              pred[2];       /* each rail's predictor */
    unsigned char      index[2];      /* each rail's step index, 0 ... 88 */
    unsigned char      reserved[6];
} fmd_adpcm_status;
#define FMD_ADPCM_WAV_HEADER_BYTES 60

/* host-only (no GPU needed); block_frames as in the configuration (0 = 1017), FMD_ERR_ARG for any other value that is no valid S */
/* bytes of a block */
int fmd_adpcm_block_align(int block_frames);
/* (S - 1 + n) / S: the most blocks a process call of n frames completes for a station, whatever its fill */
long long fmd_adpcm_max_blocks(int block_frames, long long n);
/* the matching decoder: blocks [n_blocks][block_align] -> pcm_out [n_blocks * S][2] int16, interleaved.  FMD_ERR_ARG, with nothing
 * written, where a header's index byte is above 88 */
int fmd_adpcm_decode_blocks(const uint8_t* blocks, int block_frames, long long n_blocks, int16_t* pcm_out);
/* the FMD_ADPCM_WAV_HEADER_BYTES bytes in front of n_blocks blocks in a RIFF / WAVE file, *len = their number: a `fmt ` chunk of 20
 * bytes (tag 0x0011, 2 channels, fs, nAvgBytesPerSec = fs * block_align / S in integers, nBlockAlign, wBitsPerSample = 4, cbSize = 2,
 * wSamplesPerBlock = S), a `fact` chunk with n_frames, the true length (frames - what flushes padded), and the `data` chunk's header.
 * FMD_ERR_ARG for fs outside 1 ... 1000000 or n_frames outside [0, n_blocks * S]; FMD_ERR_SIZE where the file would pass 4 GiB */
int fmd_adpcm_wav_header(int fs, int block_frames, long long n_blocks, long long n_frames, uint8_t* out, int* len);

int fmd_adpcm_create(const fmd_adpcm_config* cfg, fmd_adpcm* out);
int fmd_adpcm_destroy(fmd_adpcm e);
/* station `channel` (-1 = every station) as after create: counters 0, no open block, pred and index 0.  Waits for the encoder's
 * earlier work */
int fmd_adpcm_reset(fmd_adpcm e, int channel);
/* takes n frames of every station.  d_in [C][in_stride][2] f32 on the device, 8-byte aligned; d_active: [C] uint8 on the device,
 * NULL = all: a station whose byte is 0 is skipped whole, its row of d_out is left as it is and d_nblocks[c] = 0.  d_out: caller-owned
 * bytes on the device, 4-byte aligned, station c's completed blocks from d_out + c * out_stride on; out_stride in bytes, a multiple of
 * 4 and at least fmd_adpcm_max_blocks(S, n) * block_align.  d_nblocks: [C] int32 on the device, may be NULL.  n < 0, n > in_stride,
 * n > max_input_frames, a misaligned or null d_in or d_out or an out_stride that is too small or no multiple of 4 return FMD_ERR_ARG and
 * change nothing.  Asynchronous on `stream`; consecutive calls may use different streams (the library orders them). */
int fmd_adpcm_process_f32_dev(fmd_adpcm e, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, uint8_t* d_out,
                              long long out_stride, int* d_nblocks, void* stream);
/* closes the open block of station `channel` (-1 = of every station) as `flush` above says: 0 or 1 block at d_out + c * out_stride and
 * its number in d_nblocks[c] (may be NULL); other stations' rows and counts are left as they are.  d_out 4-byte aligned, out_stride a
 * multiple of 4 and at least block_align, else FMD_ERR_ARG.  Asynchronous on `stream`, ordered like a process call */
int fmd_adpcm_flush(fmd_adpcm e, int channel, uint8_t* d_out, long long out_stride, int* d_nblocks, void* stream);
/* out [C]; synchronises with the encoder's work */
int fmd_adpcm_get_status(fmd_adpcm e, fmd_adpcm_status* out);
/* the device's own [C] records, for a consumer on the device: ordered behind the encoder's work on the stream of its last call, valid
 * until the next call */
int fmd_adpcm_status_dev(fmd_adpcm e, const fmd_adpcm_status** d_status);
const char* fmd_adpcm_last_error(fmd_adpcm e);

/* ------------------------------------------------------------------------------------------------------------------
 * FLAC audio encoder (NOT part of the reference): lossless station recordings.  16-bit PCM is 128 KB/s per station at 32 kHz and the
 * ADPCM encoder a quarter of that but lossy; this one writes, per station, a FLAC stream (RFC 9639, streamable subset, fixed block size)
 * that decodes to exactly the PCM fmd_audio_pcm16_dev writes, in fewer bytes.  It reads the device array [C][in_stride][2] f32
 * (interleaved L, R) that the mixer and the monitors read, changes nothing in it, and writes every station's completed FLAC frames,
 * byte-packed, to a caller-owned device array.  Stereo only, 16 bits, fs 8000 ... 48000 Hz.
 * The rules, restated in C by tests/cpp/flac_ref.c; all integer behind one fp32 multiply:
 *   sample      q exactly as the ADPCM encoder's: t = x * (32767.0f * 0.95f), one fp32 multiply;  t NaN or +-inf: q = 0, nonfinite++;
 *               otherwise (int)t truncated toward zero and clamped to int16, each clamp counting in the rail's clipped.
 *   block       S = block_frames, a multiple of 64 in 64 ... 4608, default 4096.  A fixed-blocksize stream: blocking-strategy bit 0,
 *               the frame number coded.  Per station the open block's q, its fill, the stream's next frame number and the counters live
 *               in the encoder.  Stations may stand at different places in their blocks.
 *   candidates  of a frame of n frames: L, R (16 bits), M = (L + R) >> 1 with an arithmetic shift (16 bits), Sd = L - R (17 bits).
 *   subframe    of a candidate X with b bits a sample: all n samples equal -> CONSTANT, 8 + b bits.  Otherwise the fixed predictors'
 *               residuals for the orders o = 0 ... omax = min(4, n - 1):  x[i];  x[i] - x[i-1];  x[i] - 2 x[i-1] + x[i-2];
 *               x[i] - 3 x[i-1] + 3 x[i-2] - x[i-3];  x[i] - 4 x[i-1] + 6 x[i-2] - 4 x[i-3] + x[i-4].  A_o = sum over i >= omax of
 *               |r_o[i]| in 64 bits; the order with the smallest A_o, ties to the lower order.  Rice coding method 00, parameters
 *               0 ... 14, no escape partitions:  u = 2 r (r >= 0), -2 r - 1 (r < 0);  a sample costs (u >> k) + 1 + k bits.  Partition
 *               orders p = 0 ... P, P the largest p <= 6 with 2^p dividing n and (n >> p) > o;  partition 0 holds (n >> p) - o
 *               residuals;  each partition takes the k with the fewest bits, ties to the lower k;  the order p with the smallest
 *               2 + 4 + sum(4 + bits), ties to the lower p.  FIXED costs 8 + o b + that, and is used only where strictly smaller than
 *               VERBATIM's 8 + n b.  No wasted-bits detection, no LPC subframes.
 *   stereo      the totals of the channel assignments 0001 (L, R), 1000 (L, Sd), 1001 (Sd, R), 1010 (M, Sd): the smallest, ties in
 *               that order.
 *   frame       FF F8;  block-size code: the table's where n has one, else 0110 (8 bits of n - 1) for n <= 256, else 0111 (16 bits);
 *               sample-rate code: the table's where fs has one, else 1101 (16 bits of Hz);  the assignment;  sample size 100, reserved
 *               0;  the frame number, UTF-8-like, 1 - 6 bytes;  the block size's and rate's extra bytes;  CRC-8 (polynomial 0x07, init
 *               0);  the subframes, most significant bit first;  zero bits to a byte;  CRC-16 (polynomial 0x8005, init 0, not
 *               reflected, big-endian).  Over "123456789" the CRC-8 is 0xF4 and the CRC-16 0xFEE8.
 *   bound       fmd_flac_frame_bound(S) = 16 + 2 (1 + 2 S) + 2 bytes: no frame exceeds it, (L, R) as two VERBATIM subframes being
 *               always a candidate.
 *   streaming   a call of n frames completes (fill + n) / S FLAC frames for the station, writes them back to back from
 *               d_out + c * out_stride on, their bytes to d_nbytes[c] and their number to d_nframes[c];  bytes of d_out behind them
 *               are left as they are.  Nothing depends, bit for bit, on how the frames are split into calls, on streams, on the batch
 *               or on the station's row.  Ordinary stores, no global atomics, no workgroup waits on another.
 *   flush       ends the station's stream: with fill > 0 one short frame of exactly `fill` frames (the format allows a short last
 *               frame: nothing is padded), then frame number 0, streams++, the stream's samples, bytes, min and max frame bytes 0;
 *               the lifetime counters stay.  With fill = 0 only the new stream.  A station whose frame number would reach 2^31 starts
 *               a new stream by itself, behind the frame numbered 2^31 - 1, and sets `wrapped` for good; a flush whose short frame is
 *               that frame starts one stream, not two.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_flac_s* fmd_flac;
typedef struct {
    int       n_channels;         /* C: station rows of the input */
    int       block_frames;       /* S: frames of a block, a multiple of 64 in 64 ... 4608; 0 = 4096 */
    int       sample_rate;        /* fs in Hz, 8000 ... 48000: goes into every frame's header */
    long long max_input_frames;   /* largest n of a process call, in (0, 2^30] */
    int       device;             /* HIP device ordinal, -1 = current */
} fmd_flac_config;
/* one per station, 80 bytes: frames at byte 0, blocks 8, stream_samples 16, stream_bytes 24, clipped 32, nonfinite 48, streams 56,
 * frame_number 60, min_frame_bytes 64, max_frame_bytes 68, fill 72, wrapped 76 */
typedef struct {
    unsigned long long frames;           /* audio frames taken since reset */
    unsigned long long blocks;           /* FLAC frames written since reset, the short ones of flushes among them */
    unsigned long long stream_samples;   /* audio frames in the current stream's FLAC frames (the open block's are not among them) */
    unsigned long long stream_bytes;     /* bytes of the current stream's FLAC frames */
    unsigned long long clipped[2];       /* samples of L, R clamped to the 16-bit range */
    unsigned long long nonfinite;        /* samples (of either rail) that were NaN or +-inf after the scale: encoded as 0 */
    unsigned           streams;          /* streams ended since reset, by a flush or by the frame number's wrap */
    unsigned           frame_number;     /* FLAC frames of the current stream: the next frame's number, below 2^31 */
    unsigned           min_frame_bytes;  /* of the current stream's FLAC frames; 0 while it has none */
    unsigned           max_frame_bytes;
    unsigned           fill;             /* frames in the open block, 0 ... S - 1 */
    unsigned           wrapped;          /* 1 once a stream has ended because its frame number would have reached 2^31 */
} fmd_flac_status;
#define FMD_FLAC_STREAM_HEADER_BYTES 42

/* host-only (no GPU needed); block_frames as in the configuration (0 = 4096), FMD_ERR_ARG for any other value that is no valid S */
/* the most bytes of a FLAC frame */
int fmd_flac_frame_bound(int block_frames);
/* ((S - 1 + n) / S) * fmd_flac_frame_bound(S), rounded up to 4: the most bytes a process call of n frames writes for a station,
 * whatever its fill.  n in [0, 2^40] */
long long fmd_flac_max_bytes(int block_frames, long long n);
/* the FMD_FLAC_STREAM_HEADER_BYTES bytes in front of a stream's frames in a .flac file, *len = their number: `fLaC` and a last
 * metadata block STREAMINFO with min = max block size = S, the frame sizes (0 = unknown), fs, 2 channels, 16 bits, total_samples
 * (0 = unknown) and an MD5 signature of all zero, which the format reads as "not computed": a verifying decoder skips the check.
 * FMD_ERR_ARG for fs outside 8000 ... 48000, total_samples outside [0, 2^36), frame bytes outside [0, 2^24) or min above max */
int fmd_flac_stream_header(int fs, int block_frames, long long total_samples, int min_frame_bytes, int max_frame_bytes, uint8_t* out, int* len);
/* the matching decoder of one stream's frames (no stream header), for this encoder's own subset: CONSTANT / VERBATIM / FIXED subframes,
 * method 00, 16-bit stereo, every frame of S frames but a last shorter one.  pcm_out [cap][2] int16, interleaved; NULL with cap 0 only
 * checks and counts.  *n_frames_out = the audio frames decoded.  Sync code, reserved bits, both CRCs, the frame numbers' sequence from
 * 0, the codes' shortest forms and the decoded samples' range are checked: FMD_ERR_ARG on anything else, FMD_ERR_SIZE where pcm_out is
 * too small; pcm_out may then hold the frames in front of the failure */
int fmd_flac_decode(const uint8_t* bytes, long long len, int fs, int block_frames, int16_t* pcm_out, long long cap, long long* n_frames_out);

int fmd_flac_create(const fmd_flac_config* cfg, fmd_flac* out);
int fmd_flac_destroy(fmd_flac e);
/* station `channel` (-1 = every station) as after create: counters 0, no open block, stream 0, frame number 0.  Waits for the
 * encoder's earlier work */
int fmd_flac_reset(fmd_flac e, int channel);
/* takes n frames of every station.  d_in [C][in_stride][2] f32 on the device, 8-byte aligned; d_active: [C] uint8 on the device,
 * NULL = all: a station whose byte is 0 is skipped whole, its row of d_out is left as it is and its counts are 0.  d_out: caller-owned
 * bytes on the device, 4-byte aligned, station c's completed FLAC frames from d_out + c * out_stride on; out_stride in bytes, a
 * multiple of 4 and at least fmd_flac_max_bytes(S, n).  d_nbytes, d_nframes: [C] int32 on the device, either may be NULL.  n < 0,
 * n > in_stride, n > max_input_frames, a misaligned or null d_in or d_out or an out_stride that is too small or no multiple of 4
 * return FMD_ERR_ARG and change nothing.  Asynchronous on `stream`; consecutive calls may use different streams (the library orders
 * them). */
int fmd_flac_process_f32_dev(fmd_flac e, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, uint8_t* d_out,
                             long long out_stride, int* d_nbytes, int* d_nframes, void* stream);
/* ends the stream of station `channel` (-1 = of every station) as `flush` above says: 0 or 1 FLAC frame at d_out + c * out_stride, its
 * bytes in d_nbytes[c] and 0 or 1 in d_nframes[c] (either may be NULL); other stations' rows and counts are left as they are.  d_out
 * 4-byte aligned, out_stride a multiple of 4 and at least fmd_flac_max_bytes(S, 1), else FMD_ERR_ARG.  Asynchronous on `stream`,
 * ordered like a process call */
int fmd_flac_flush(fmd_flac e, int channel, uint8_t* d_out, long long out_stride, int* d_nbytes, int* d_nframes, void* stream);
/* out [C]; synchronises with the encoder's work */
int fmd_flac_get_status(fmd_flac e, fmd_flac_status* out);
/* the device's own [C] records, for a consumer on the device: ordered behind the encoder's work on the stream of its last call, valid
 * until the next call */
int fmd_flac_status_dev(fmd_flac e, const fmd_flac_status** d_status);
const char* fmd_flac_last_error(fmd_flac e);

/* ------------------------------------------------------------------------------------------------------------------
 * Log-mel front end (NOT part of the reference): station audio as the features a model takes.  Transcription, speech / music / advert
 * segmentation and fingerprinting models all start from a log-mel spectrogram: 25 ms Hann window, 10 ms hop, 80 mel bands from 0 to
 * 8 kHz.  This object reads the device array [C][in_stride][2] f32 (interleaved L, R) that the mixer and the monitors read, changes
 * nothing in it, keeps every station's window overlap across calls, and writes the completed spectral frames as rows of n_mels f32 to a
 * caller-owned device array.  It is no spectrum display: its output is a tensor for a model (DESIGN.md §7 keeps the reference's GUI
 * spectra out of scope, and that stays).
 * The rules, restated in C by tests/cpp/logmel_ref.c.  N = win, every fused multiply-add is one fmaf, fp32 denormals are kept:
 *   design      host, double, host libm (fmd_logmel_design):  w[n] = (float)(0.5 - 0.5 cos(2 pi n / N)), the periodic Hann window;
 *               tc[j] = (float)cos(2 pi j / N), ts[j] = (float)sin(2 pi j / N), j = 0 ... N - 1;  K = min(N / 2, floor(f_max N / fs)) + 1
 *               bins at f_k = k fs / N.  Mel scale 0 (Slaney): mel(f) = f / (200 / 3) below 1000 Hz, 15 + ln(f / 1000) / (ln(6.4) / 27)
 *               from there, and its inverse;  1 (HTK): mel(f) = 2595 log10(1 + f / 700), inverse 700 (10^(m / 2595) - 1).  Edges
 *               mu_i = mel(f_min) + i (mel(f_max) - mel(f_min)) / (n_mels + 1), F_i = mel^-1(mu_i), i = 0 ... n_mels + 1.  Weights
 *               fb[j][k] = (float)(max(0, min((f_k - F_j) / (F_j+1 - F_j), (F_j+2 - f_k) / (F_j+2 - F_j+1))) s_j), s_j = 2 / (F_j+2 - F_j)
 *               for Slaney (area normalisation) and 1 for HTK.  empty_bands counts the bands whose weights are all zero; create accepts
 *               such a design.
 *   sample      the sample index counts absolutely, in 64 bits, from the station's reset.  m = 0.5f * (L + R) in fp32: one rounding (the
 *               halving is exact except into denormals, which are kept).
 *   frame t     covers m[t hop ... t hop + N - 1]: no centring, no padding; its centre lies at (t hop + N / 2) / fs seconds, and it exists
 *               once frames >= t hop + N.  xw[n] = w[n] * m[t hop + n], one fp32 rounding.  For every bin k < K, from +0 in ascending n:
 *               re_k = fmaf(xw[n], tc[(k n) mod N], re_k),  im_k = fmaf(xw[n], ts[(k n) mod N], im_k).  P_k = fmaf(re_k, re_k, im_k * im_k).
 *               For every band j, from +0 in ascending k over ALL k < K, zero weights included: mel_j = fmaf(fb[j][k], P_k, mel_j).
 *               A non-finite sample makes the frame's bands non-finite as these chains give them: nothing is special-cased.
 *   output      mode 0 writes mel_j; mode 1 writes flog10(v), v = mel_j > log_floor ? mel_j : (mel_j != mel_j ? mel_j : log_floor).  A NaN
 *               is written as the quiet NaN 0x7fc00000 in both modes, whatever sign or payload the chains gave it.
 *   flog10      a fixed algorithm (fm-radio_amd/csrc/fmd_logmel_math.h), no libm:  u = bits(x) - 0x3f3504f3;  e = (int)u >> 23;
 *               f = bits((u & 0x7fffff) + 0x3f3504f3) - 1.0f (exact; 1 + f in [sqrt(1/2), sqrt(2)));  r = c11, then r = fmaf(f, r, c_i) for
 *               i = 10 ... 1;  t = fmaf(f, r, C0lo);  lm = fmaf(f, C0hi, f * t);  y = fmaf(e, L2hi, fmaf(e, L2lo, lm)).  C0hi, C0lo, L2hi,
 *               L2lo = 0x3ede5bd9, 0xb22d91af, 0x3e9a2000, 0x369a84fc;  c1 ... c11 = 0xbe5e5bd9, 0x3e143d3a, 0xbdde5bb4, 0x3db1e377,
 *               0xbd9445b2, 0x3d7e1719, 0xbd5cc607, 0x3d446f9a, 0xbd41dcff, 0x3d3d35d2, 0xbccff948.  +inf gives +inf and NaN the argument.
 *               Its argument is never below FLT_MIN.  Within 8 fp32 ulp of float64 log10 over every finite float >= FLT_MIN (measured
 *               worst case: DESIGN.md §6n).
 *   streaming   per station the object keeps the mono samples from the next uncompleted frame's start onward (at most N - 1) and the
 *               32-byte record below.  A call of n frames completes T(frames + n) - T(frames) spectral frames of the station,
 *               T(f) = f < N ? 0 : (f - N) / hop + 1, and writes them oldest first as rows of n_mels f32 from d_out + c * out_stride on
 *               and their number to d_nframes[c]; floats behind the rows are left alone.  Nothing depends, bit for bit, on how the
 *               frames are split into calls, on streams, on the batch or on the station's row.  Stations may stand at different places
 *               in their windows.  Ordinary stores, no global atomics, no workgroup waits on another.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_logmel_s* fmd_logmel;
typedef struct {
    int       n_channels;         /* C: station rows of the input */
    int       fs;                 /* the audio's rate in Hz, 8000 ... 48000 */
    int       win;                /* N: frames of a window, a multiple of 16 in 64 ... 2048 */
    int       hop;                /* frames from one window's start to the next, 16 ... win */
    int       n_mels;             /* mel bands, 1 ... 128 */
    double    f_min_hz;           /* 0 <= f_min_hz < f_max_hz <= fs / 2 */
    double    f_max_hz;
    int       mel_scale;          /* 0 = Slaney with area normalisation, 1 = HTK, unnormalised */
    int       out_mode;           /* 0 = mel power, 1 = log10 */
    float     log_floor;          /* finite and >= FLT_MIN */
    long long max_input_frames;   /* largest n of a process call, in (0, 2^30] */
    int       device;             /* HIP device ordinal, -1 = current */
} fmd_logmel_config;
typedef struct {
    int n_bins;                   /* K */
    int empty_bands;              /* bands whose weights are all zero */
} fmd_logmel_design_t;
/* one per station, 32 bytes: frames at byte 0, spectra 8, nonfinite 16, fill 24, reserved 28 */
typedef struct {
    unsigned long long frames;    /* audio frames taken since reset */
    unsigned long long spectra;   /* spectral frames written since reset: T(frames) */
    unsigned long long nonfinite; /* spectral frames with a band that was +-inf or NaN */
    unsigned           fill;      /* mono samples kept for the next frame: frames - spectra * hop, 0 ... N - 1 */
    unsigned           reserved;
} fmd_logmel_status;

/* host-only (no GPU needed) */
/* the usual geometry at the audio's own rate: win = fs / 40 rounded up to a multiple of 16, hop = fs / 100, 80 bands from 0 Hz to
 * min(8000, fs / 2), Slaney, log10, floor 1e-10f, one station, max_input_frames 65536, the current device.  At 32 kHz win = 800 and
 * hop = 320: the 201 bins of an 800-point DFT up to 8 kHz are the bin frequencies and the 25 ms window of 16 kHz / 400 / 160, with no
 * resampler in front.  FMD_ERR_ARG for fs outside 8000 ... 48000 */
int fmd_logmel_default_config(int fs, fmd_logmel_config* cfg);
/* the design of a valid configuration: w [win], tc [win], ts [win], fb [n_mels][K] with K = fmd_logmel_bins(cfg); any of the four may be
 * NULL and is then not written; *out (may be NULL) K and empty_bands.  FMD_ERR_ARG for an invalid configuration */
int fmd_logmel_design(const fmd_logmel_config* cfg, float* w, float* tc, float* ts, float* fb, fmd_logmel_design_t* out);
/* K of a valid configuration, FMD_ERR_ARG otherwise */
int fmd_logmel_bins(const fmd_logmel_config* cfg);
/* (n + hop - 1) / hop: the most spectral frames a process call of n frames completes for a station, wherever it stands in its window.
 * FMD_ERR_ARG for hop outside 16 ... 2048 or n outside [0, 2^40] */
long long fmd_logmel_max_frames(int hop, long long n);
/* flog10 above, evaluated on the host */
float fmd_logmel_flog10(float x);

int fmd_logmel_create(const fmd_logmel_config* cfg, fmd_logmel* out);
int fmd_logmel_destroy(fmd_logmel h);
/* station `channel` (-1 = every station) as after create: counters 0, no samples kept; the configuration stays.  Waits for the
 * object's earlier work */
int fmd_logmel_reset(fmd_logmel h, int channel);
/* takes n frames of every station.  d_in [C][in_stride][2] f32 on the device, 8-byte aligned; d_active: [C] uint8 on the device,
 * NULL = all: a station whose byte is 0 is skipped whole, its rows and its count are left as they are.  d_out: caller-owned floats on
 * the device, 4-byte aligned; out_stride in floats, at least fmd_logmel_max_frames(hop, n) * n_mels.  d_nframes: [C] int32 on the
 * device, may be NULL.  n = 0 is valid.  n < 0, n > in_stride, n > max_input_frames, a null or misaligned d_in or d_out or a short
 * out_stride return FMD_ERR_ARG and change nothing.  Asynchronous on `stream`; consecutive calls may use different streams (the library
 * orders them). */
int fmd_logmel_process_f32_dev(fmd_logmel h, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, float* d_out,
                               long long out_stride, int* d_nframes, void* stream);
/* out [C]; synchronises with the object's work */
int fmd_logmel_get_status(fmd_logmel h, fmd_logmel_status* out);
/* the device's own [C] records, for a consumer on the device: ordered behind the object's work on the stream of its last call, valid
 * until the next call */
int fmd_logmel_status_dev(fmd_logmel h, const fmd_logmel_status** d_status);
const char* fmd_logmel_last_error(fmd_logmel h);

/* ------------------------------------------------------------------------------------------------------------------
 * EAS SAME decoder (NOT part of the reference): which alert is on the air.  The tone detector says that the 853 + 960 Hz attention
 * signal is on a station; the machine-readable part in front of it -- three bursts of a SAME header (47 CFR 11.31), 520.83 bit/s AFSK
 * of `ZCZC-ORG-EEE-PSSCCC...+TTTT-JJJHHMM-LLLLLLLL-`, and three `NNNN` bursts at the alert's end -- says which.  It reads the device
 * array [C][in_stride][2] f32 (interleaved L, R) that the mixer and the monitors read, changes nothing in it, keeps one record per
 * station with the newest eight accepted messages, and writes a [C] uint8 flags byte and a [C] uint8 ok byte per station.
 * Arithmetic, restated in C by tests/cpp/same_ref.c:
 *   design      host, double, host libm; fs a multiple of 10 in 8000 ... 48000:
 *                 g = gcd(3125, 6 fs), P = 6 fs / g (at most 57600);  tc[j] = cos(2.0 * M_PI * (double)j / (double)P), ts[j] likewise sin
 *                 mark step = (4 * 3125 / g) mod P (2083.33 Hz, four cycles a bit), space step = (3 * 3125 / g) mod P (1562.5 Hz, three)
 *   per frame   i counted absolutely in 64 bits since the station's reset:  m = (double)L + (double)R
 *                 the table index of frame i is (i * step) mod P per tone, moved on by an add and a conditional subtract
 *   tick        eight a nominal bit: tick k covers frames [B(k), B(k + 1)), B(k) = ceil(k * 3 fs / 12500) -- with k = 12500 q + r,
 *               B(k) = q * 3 fs + (r * 3 fs + 12499) / 12500 in integers.  Four sums a tick, each from +0 in ascending frame order:
 *                 mre = fma(m, tc[im], mre); mim = fma(m, ts[im], mim); sre = fma(m, tc[is], sre); sim = fma(m, ts[is], sim)
 *               The open tick's sums carry to the next call; fp32 and fp64 denormals are kept.
 *   decision    at a tick's end each of the four window sums is ((((((((+0 + t[k-7]) + t[k-6]) + ...) + t[k]) over this tick and the
 *               seven before it (ticks before the reset read +0);  E1 = fma(mre, mre, mim * mim), E0 = fma(sre, sre, sim * sim);
 *               s = E1 > E0 (a NaN gives 0).  No normalisation, no threshold.
 *   bit clock   integers, ph in 1 / 256 bit, run = ticks since s last changed (counted up to 255).  Where s differs from the previous
 *               tick's s, the run that ends was nb = (run + 4) >> 3 bits long and its middle stood at ph - 16 run, which in lock is 0 for
 *               an odd nb and 128 for an even one.  With nb >= 1 and run <= 96:  err = (ph - 16 run - (nb odd ? 0 : 128)) & 255;
 *               err < 128 -> ph = (ph - min(pull, err)) & 255, else ph = (ph + min(pull, 256 - err)) & 255.  Then run = 0.  In every
 *               tick run++ (up to 255), then ph += 32; at ph >= 256: ph -= 256 and s is a bit (bits++).  (A clock pulled by the
 *               transitions themselves has a second stable state, half a bit off, once the mark tone is louder or softer than the space
 *               tone, because rising and falling edges then move in opposite directions; a run's middle does not move: DESIGN.md §6l.)
 *   framer      sh = (sh >> 1) | (s << 15), 16 bits.  Unsynchronised: sh == 0xABAB synchronises (syncs++, the message in progress starts
 *               empty, sync_tick = this tick's number).  Synchronised: every eighth bit delivers b = sh >> 8.  b == 0xAB with the message
 *               still empty is skipped; b in 0x20 ... 0x7E, 0x0D or 0x0A is appended, and the 268th byte ends the message; any other b ends
 *               it as it stands.  An ended message whose first four bytes are ZCZC or NNNN is accepted: it goes to ring[accepted % 8]
 *               (bytes behind its length 0), accepted++, last_accept_tick = this tick's number; any other is counted in `rejected`.
 *               Either way the framer is unsynchronised again.
 *   flags       bit 0 (FMD_SAME_SYNCED): synchronised at the call's end.  Bit 1 (FMD_SAME_ALERT_OPEN): set by an accepted ZCZC message,
 *               cleared by an accepted NNNN message, and cleared at the end of tick k where k - last_accept_tick >= hold_ticks.
 *               ok = (flags & alarm_mask) == 0.  Parameters apply from the next tick that ends; the record's ok follows alarm_mask at once.
 *   Nothing depends, bit for bit, on how the frames are split into calls, on streams, on the batch or on the station's row.  No atomics;
 *   ordinary stores.  (A NaN's sign and payload in the carried sums are not part of the contract.)
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_same_s* fmd_same;
#define FMD_SAME_SYNCED        1u
#define FMD_SAME_ALERT_OPEN    2u
#define FMD_SAME_MAX_BYTES     268
#define FMD_SAME_RING          8
#define FMD_SAME_KIND_HEADER   1      /* ZCZC */
#define FMD_SAME_KIND_EOM      2      /* NNNN */
#define FMD_SAME_MAX_LOCATIONS 31
typedef struct {
    int       n_channels;         /* C: station rows of the input */
    int       fs;                 /* the audio's rate: a multiple of 10 in 8000 ... 48000 */
    long long max_input_frames;   /* largest n of a process call, in (0, 2^30] */
    int       device;             /* HIP device ordinal, -1 = current */
} fmd_same_config;
/* defaults: 16, 750000 (180 s of ticks: 12500 / 3 a second), 0.  Valid: pull in 0 ... 128; hold_ticks in 1 ... 2^31 - 1; alarm_mask
 * with no bit above bit 1.  16 bytes */
typedef struct {
    int      pull;                /* the most the bit clock moves at a transition, in 1 / 256 bit */
    unsigned hold_ticks;          /* ticks behind the last accepted message after which an open alert is closed */
    unsigned alarm_mask;          /* the flags whose being set takes the station's ok byte to 0 */
    unsigned reserved;            /* 0 */
} fmd_same_params;
/* 280 bytes: sync_tick at byte 0, len 8, kind 10, reserved 11, bytes 12 */
typedef struct {
    unsigned long long sync_tick;         /* the tick at whose end the framer synchronised on this message */
    unsigned short     len;               /* bytes of the message, 4 ... 268 */
    unsigned char      kind;              /* FMD_SAME_KIND_HEADER or FMD_SAME_KIND_EOM */
    unsigned char      reserved;
    unsigned char      bytes[FMD_SAME_MAX_BYTES];   /* the message from its ZCZC or NNNN on, 0 behind len */
} fmd_same_message;
/* one per station, 2856 bytes: frames at byte 0, ticks 8, bits 16, syncs 24, accepted 32, rejected 40, sync_tick 48, last_accept_tick 56,
 * open 64, hist 96, ph 320, sh 324, nbit 328, msg_len 332, run 336, synced 340, prev_s 341, flags 342, ok 343, msg 344, reserved 612, ring 616 */
typedef struct {
    unsigned long long frames;            /* frames seen since reset */
    unsigned long long ticks;             /* completed ticks: the open tick's number */
    unsigned long long bits;              /* bits the clock has taken */
    unsigned long long syncs;             /* times the framer has synchronised */
    unsigned long long accepted;          /* messages accepted: the newest is ring[(accepted - 1) % 8] */
    unsigned long long rejected;          /* messages that ended without ZCZC or NNNN in front */
    unsigned long long sync_tick;         /* of the message in progress */
    unsigned long long last_accept_tick;
    double   open[4];                     /* the open tick's sums: mark re, mark im, space re, space im */
    double   hist[7][4];                  /* the last seven completed ticks' sums, oldest first */
    unsigned ph;                          /* the bit clock, 0 ... 255 */
    unsigned sh;                          /* the framer's 16-bit register */
    unsigned nbit;                        /* bits since the last byte, 0 ... 7 (synchronised) */
    unsigned msg_len;                     /* bytes of the message in progress */
    unsigned run;                         /* ticks since the decision last changed, up to 255 */
    unsigned char synced, prev_s, flags, ok;
    unsigned char msg[FMD_SAME_MAX_BYTES];    /* the message in progress (bytes behind msg_len are stale) */
    unsigned char reserved[4];
    fmd_same_message ring[FMD_SAME_RING];
} fmd_same_status;
/* what fmd_same_encode makes */
typedef struct {
    int       fs;                 /* a multiple of 10 in 8000 ... 48000 */
    int       repeats;            /* bursts, 1 ... 16 (a transmission has three) */
    long long gap_frames;         /* silent frames behind every burst; negative = one second */
    double    clock_ratio;        /* the sender's clock over nominal, in [0.9, 1.1]: bit rate and both tones move with it */
    double    amplitude;          /* of the space tone in each rail, finite and >= 0 (the mid signal carries twice that) */
    double    mark_db;            /* the mark tone's level against the space tone's, in [-40, 40] */
} fmd_same_encode_config;
#define FMD_SAME_VALID_ORG       1u
#define FMD_SAME_VALID_EVENT     2u
#define FMD_SAME_VALID_LOCATIONS 4u
#define FMD_SAME_VALID_DURATION  8u
#define FMD_SAME_VALID_TIME      16u
#define FMD_SAME_VALID_CALLSIGN  32u
typedef struct {
    int      kind;                /* FMD_SAME_KIND_HEADER or FMD_SAME_KIND_EOM (then every other field is 0) */
    unsigned valid;               /* FMD_SAME_VALID_* per field */
    char     org[4], event[4];    /* NUL-terminated */
    int      n_locations;
    char     locations[FMD_SAME_MAX_LOCATIONS][8];   /* PSSCCC, NUL-terminated */
    int      duration_min;        /* +TTTT as hours and minutes, in minutes */
    int      day, hour, minute;   /* JJJHHMM: day of the year 1 ... 366, UTC */
    char     callsign[12];        /* LLLLLLLL, NUL-terminated */
} fmd_same_header;

/* host-only (no GPU needed) */
void fmd_same_default_params(fmd_same_params* p);
/* `text` (len bytes in 1 ... 268, e.g. "ZCZC-WXR-TOR-039173+0030-1051700-KCLE/NWS-") as audio: per burst 16 bytes 0xAB and the text, least
 * significant bit first, one bit per 6 fs / (3125 clock_ratio) frames; frame i of a burst stands u = i * clock_ratio * 3125 / (6 fs) bits
 * in, and both rails carry (float)(a * sin(2 pi cyc frac(u))), cyc = 4 and a = amplitude * 10^(mark_db / 20) in a 1 bit, cyc = 3 and
 * a = amplitude in a 0 bit.  Returns the number of frames of the whole (bursts and gaps); writes out [frames][2] where out is not NULL
 * and cap (in frames) suffices, else FMD_ERR_SIZE; FMD_ERR_ARG for values outside the ranges above */
long long fmd_same_encode(const fmd_same_encode_config* cfg, const char* text, int len, float* out, long long cap);
/* one message's bytes -> its fields.  FMD_ERR_ARG unless it starts with ZCZC or NNNN; else FMD_OK with `valid` telling which fields
 * were well formed (a malformed field is zeroed).  Whatever stands behind the call sign's closing `-` is ignored */
int fmd_same_parse(const unsigned char* bytes, int len, fmd_same_header* out);
/* n = 1 ... 3 messages of one kind in ascending sync_tick, each no more than 2.5 s (10416 ticks) plus its predecessor's own length
 * (64 ticks a byte) behind its predecessor (else FMD_ERR_STATE): byte by byte two out of three.  out: the voted message with the first
 * one's sync_tick; *corrected: bytes at which one copy was outvoted; *unresolved: bytes without a majority, where the first copy's
 * stands (with two copies: every byte at which they differ).  The length is voted the same way */
int fmd_same_vote(const fmd_same_message* msgs, int n, fmd_same_message* out, int* corrected, int* unresolved);

int fmd_same_create(const fmd_same_config* cfg, fmd_same* out);
int fmd_same_destroy(fmd_same d);
/* everything of station `channel` (-1 = every station) as after create: counters, clock, framer, sums, ring, flags clear, ok = 1; its
 * parameters are kept.  Waits for the decoder's earlier work */
int fmd_same_reset(fmd_same d, int channel);
/* the parameters of station `channel` (-1 = every station): ordered behind the decoder's earlier work; they apply from the next tick
 * that ends (the record's ok at once).  FMD_ERR_ARG for values outside the ranges above, and nothing changes */
int fmd_same_set_params(fmd_same d, int channel, const fmd_same_params* p);
int fmd_same_get_params(fmd_same d, int channel, fmd_same_params* p);
/* takes n frames of every station.  d_in [C][in_stride][2] f32 on the device, 8-byte aligned; d_active: [C] uint8 on the device,
 * NULL = all: a station whose byte is 0 is skipped whole, and its two output bytes are left as they are.  d_flags, d_ok: [C] uint8 on
 * the device, caller-owned, each may be NULL: behind its work on `stream` the call writes every other station's byte, also when n == 0.
 * n < 0, n > in_stride, n > max_input_frames or a misaligned d_in return FMD_ERR_ARG and change nothing.  Asynchronous on `stream`;
 * consecutive calls may use different streams (the library orders them). */
int fmd_same_process_f32_dev(fmd_same d, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, uint8_t* d_flags,
                             uint8_t* d_ok, void* stream);
/* out [C]; synchronises with the decoder's work */
int fmd_same_get_status(fmd_same d, fmd_same_status* out);
/* the device's own [C] records, for a consumer on the device: ordered behind the decoder's work on the stream of its last process
 * call, valid until the next process call */
int fmd_same_status_dev(fmd_same d, const fmd_same_status** d_status);
const char* fmd_same_last_error(fmd_same d);

/* ------------------------------------------------------------------------------------------------------------------
 * Audio fingerprinter (NOT part of the reference): which programme is on a station.  The robust hash of Haitsma and Kalker ("A Highly
 * Robust Audio Fingerprinting System", ISMIR 2002): one 32-bit word per hop of 11.5 ms, each bit the sign of an energy difference across
 * neighbouring bands and neighbouring frames, compared by bit error rate (BER) over a few hundred words: 344 bytes a second and station.
 * This object reads the device array [C][in_stride][2] f32 (interleaved L, R) that the mixer and the monitors read, changes nothing in
 * it, keeps every station's state across calls, and writes the completed words as uint32 rows to a caller-owned device array.  The
 * window is R = n_sub hops long, so every hop-sized sub-block is transformed ONCE and a frame is assembled from R kept sub-block spectra.
 * The rules, restated in C by tests/cpp/fprint_ref.c.  H = hop, R = n_sub, N = R H, B = n_bands; every fused multiply-add is one fmaf,
 * fp32 denormals are kept:
 *   design      host, double, host libm (fmd_fprint_design), each value rounded once to f32.  Band edges f_b = f_min (f_max / f_min)^(b / B),
 *               b = 0 ... B (pow);  bin edges k_b = floor(f_b N / fs + 0.5);  band b is the bins [k_b, k_b+1).  Valid: every band non-empty
 *               (k_b < k_b+1), k_0 >= 1 and k_B <= N / 2 - 1; else FMD_ERR_ARG with the reason.  K = k_B - k_0 + 2 bins are transformed,
 *               k_0 - 1 ... k_B: one more on each side for the window.  Sub-block basis for n < H and those bins:
 *               bc[n][k] = (float)cos(phi), bs[n][k] = (float)(-sin(phi)), phi = 2 pi ((k n) mod N) / N.  Frame twiddles for q < R:
 *               wc[q] = (float)cos(2 pi q / R), ws[q] = (float)sin(2 pi q / R), but at the multiples of R / 4 exactly 1, 0, -1, 0 and
 *               0, 1, 0, -1.
 *   sample      the sample index counts absolutely, in 64 bits, from the station's reset.  m = 0.5f * (L + R): one rounding.
 *   sub-block g covers m[g H ... g H + H - 1].  Per bin, from +0 in ascending n:  Sr = fmaf(m[g H + n], bc[n][k], Sr),
 *               Si = fmaf(m[g H + n], bs[n][k], Si).
 *   frame t     covers sub-blocks t ... t + R - 1 (no centring, no padding).  Per bin, from +0 in ascending j = 0 ... R - 1, with
 *               q = (k j) mod R and S = S of sub-block t + j:  re = fmaf(Sr, wc[q], re);  re = fmaf(Si, ws[q], re);
 *               im = fmaf(Si, wc[q], im);  im = fmaf(-Sr, ws[q], im).  That is X = sum_j e^(-2 pi i k j / R) S_j, the N-point DFT.
 *   window      the periodic Hann window as three taps, for k = k_0 ... k_B - 1 and for re and im alike:
 *               Xw = fmaf(-0.25f, X[k-1] + X[k+1], 0.5f * X[k]);  P_k = fmaf(Xw_re, Xw_re, Xw_im * Xw_im).
 *   band        E_t[b], from +0 in ascending k over [k_b, k_b+1):  E = E + P_k.
 *   word        for t >= 1 and b < B - 1:  d = (E_t[b] - E_t[b+1]) - (E_t-1[b] - E_t-1[b+1]), every operation rounded to f32.  Bit b of
 *               word t is d > 0 (a NaN compares false), stored at position 31 - b; the unused low bits are 0.  `nonfinite` counts
 *               the words one of whose 2 B energies E_t[.], E_t-1[.] is +-inf or NaN.  In d_energy a NaN is written as the quiet NaN
 *               0x7fc00000, whatever sign or payload the chains gave it; nothing else is special-cased.
 *   streaming   after f frames a station has s = f / H sub-blocks and prints = max(0, s - R) words: word i compares frames i + 1 and
 *               i and starts at sample (i + 1) H; the first word exists once f = (R + 1) H.  Per station the object keeps the carried
 *               mono samples (fewer than H), the last R - 1 sub-block spectra, E of the last frame and the 32-byte record below.
 *               A call of n frames writes the newly completed words, oldest first, from d_out + c * out_stride on and their number
 *               to d_nprints[c]: at most fmd_fprint_max_prints(hop, n); the slots behind them are left alone.  d_energy (optional)
 *               receives E_t of the same frames as rows of B f32.  Nothing depends, bit for bit, on how the frames are split into
 *               calls, on streams, on the batch or on the station's row.  Ordinary stores, no global atomics, no workgroup waits on
 *               another.
 *   memory      the kept spectra take (R - 1) * 2 * Kp * 4 bytes a station, Kp = K rounded up to a multiple of 16: at the default
 *               geometry at 32 kHz (K = 628) 158 720 bytes, 0.65 GB for 4096 stations; a per-call scratch of up to 64 KB a station comes
 *               on top (0.13 GB for 4096 stations at max_input_frames 2048).  fmd_fprint_state_bytes reports the whole.  A call longer
 *               than the scratch holds is cut into pieces inside the library, which by the rule above changes nothing.
 * Not built: the paper's reliability ordering of bits, a database or search on the device, resampling to 5 kHz, per-station
 * configurations, overlapping or weighted bands.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_fprint_s* fmd_fprint;
typedef struct {
    int       n_channels;         /* C: station rows of the input */
    int       fs;                 /* the audio's rate in Hz, 8000 ... 48000 */
    int       hop;                /* H: frames of a sub-block and between words, a multiple of 16 in 16 ... 1024 */
    int       n_sub;              /* R: sub-blocks of a window, one of 4, 8, 16, 32 */
    int       n_bands;            /* B: 2 ... 33; a word has B - 1 bits */
    double    f_min_hz;           /* 0 < f_min_hz < f_max_hz */
    double    f_max_hz;
    long long max_input_frames;   /* largest n of a process call, in (0, 2^30] */
    int       device;             /* HIP device ordinal, -1 = current */
} fmd_fprint_config;
typedef struct {
    int n_bins;                   /* K = k_B - k_0 + 2 */
    int first_bin;                /* k_0 - 1: the DFT bin of column 0 of bc and bs */
} fmd_fprint_design_t;
/* one per station, 32 bytes: frames at byte 0, prints 8, nonfinite 16, fill 24, reserved 28 */
typedef struct {
    unsigned long long frames;    /* audio frames taken since reset */
    unsigned long long prints;    /* words written since reset: max(0, frames / H - R) */
    unsigned long long nonfinite; /* words with an energy that was +-inf or NaN */
    unsigned           fill;      /* mono samples carried to the next sub-block: frames mod H */
    unsigned           reserved;
} fmd_fprint_status;

/* host-only (no GPU needed) */
/* the paper's geometry at the audio's own rate, with no resampler in front: hop = fs * 0.0115 rounded to a multiple of 16 (368 at
 * 32 kHz), n_sub = 32 (a window of 0.368 s), 33 bands from 300 to 2000 Hz, one station, max_input_frames 65536, the current device.
 * FMD_ERR_ARG for fs outside 8000 ... 48000 */
int fmd_fprint_default_config(int fs, fmd_fprint_config* cfg);
/* the design of a valid configuration: bc, bs [hop][K], wc, ws [n_sub], edges [n_bands + 1] (the DFT bins k_b) with
 * K = fmd_fprint_bins(cfg); any of the five may be NULL and is then not written; *out may be NULL.  FMD_ERR_ARG for an invalid
 * configuration or design, and then nothing is written */
int fmd_fprint_design(const fmd_fprint_config* cfg, float* bc, float* bs, float* wc, float* ws, int* edges, fmd_fprint_design_t* out);
/* K of a valid configuration, FMD_ERR_ARG otherwise */
int fmd_fprint_bins(const fmd_fprint_config* cfg);
/* (n + hop - 1) / hop: the most words a process call of n frames completes for a station, wherever it stands in its sub-block.
 * FMD_ERR_ARG for hop outside 16 ... 1024 or n outside [0, 2^40] */
long long fmd_fprint_max_prints(int hop, long long n);
/* the bytes of device memory an object of `channels` stations holds (kept spectra, scratch, carries, energies, records, design);
 * FMD_ERR_ARG for an invalid configuration or channels <= 0 */
long long fmd_fprint_state_bytes(const fmd_fprint_config* cfg, int channels);

/* FMD_ERR_DEVICE where the device memory (fmd_fprint_state_bytes) cannot be had */
int fmd_fprint_create(const fmd_fprint_config* cfg, fmd_fprint* out);
int fmd_fprint_destroy(fmd_fprint h);
/* station `channel` (-1 = every station) as after create: counters 0, nothing kept; the configuration stays.  Waits for the object's
 * earlier work */
int fmd_fprint_reset(fmd_fprint h, int channel);
/* takes n frames of every station.  d_in [C][in_stride][2] f32 on the device, 8-byte aligned; d_active: [C] uint8 on the device,
 * NULL = all: a station whose byte is 0 is skipped whole: its state, its words, its energies and its count are left as they are.
 * d_out: caller-owned uint32 on the device, 4-byte aligned; out_stride in words, at least fmd_fprint_max_prints(hop, n).  d_nprints:
 * [C] int32 on the device, may be NULL.  d_energy: caller-owned f32 on the device, 4-byte aligned, may be NULL; energy_stride in
 * floats, at least fmd_fprint_max_prints(hop, n) * n_bands.  n = 0 is valid.  n < 0, n > in_stride, n > max_input_frames, a null or
 * misaligned d_in or d_out, a misaligned d_energy or a short stride return FMD_ERR_ARG and change nothing.  Asynchronous on `stream`;
 * consecutive calls may use different streams (the library orders them). */
int fmd_fprint_process_f32_dev(fmd_fprint h, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, uint32_t* d_out,
                               long long out_stride, int* d_nprints, float* d_energy, long long energy_stride, void* stream);
/* out [C]; synchronises with the object's work */
int fmd_fprint_get_status(fmd_fprint h, fmd_fprint_status* out);
/* the device's own [C] records, for a consumer on the device: ordered behind the object's work on the stream of its last call, valid
 * until the next call */
int fmd_fprint_status_dev(fmd_fprint h, const fmd_fprint_status** d_status);
const char* fmd_fprint_last_error(fmd_fprint h);

/* ------------------------------------------------------------------------------------------------------------------
 * Fingerprint matcher (NOT part of the reference): which recording is on a station.  The object holds a catalogue of reference
 * fingerprints on the device, T tracks stored as runs of uint32 words, and per station a ring of the station's newest W words.  It
 * takes the fingerprinter's device outputs as they are (the d_out rows and d_nprints), and whenever a station's word count crosses a
 * multiple of the search interval it searches the WHOLE catalogue for the station's newest W words, by brute force: exact integer
 * arithmetic (XOR, population count, minimum), so every result is the same in every call split and tiling.  The rules, restated in
 * numpy by tests/fpmatch_ref.py.  W = block, I = interval, mask = 0xffffffff << (32 - n_bits):
 *   catalogue   D = starts[T] words; track t is the words starts[t] ... starts[t + 1] - 1 and is at least W words long.  A position p is
 *               valid iff the W words p ... p + W - 1 lie inside one track.  fmd_fpmatch_load replaces the whole catalogue from host
 *               memory, waits for the object's earlier work, clears every station's detector (track = -1, misses = 0, bit 0 of
 *               flags) and keeps every station's ring and counters; n_tracks = 0 empties the catalogue.  FMD_ERR_ARG, and nothing
 *               changed, for a track shorter than W, starts[0] != 0, T above max_tracks, D above max_catalogue_words, a starts array
 *               that does not ascend or null words with D > 0.
 *   push        a call hands station c  k = d_nwords[c] clamped into [0, n]  new words (a clamp adds 1 to `clamped`), k = n where
 *               d_nwords is NULL: d_words[c * words_stride + 0 ... k - 1], oldest first, the layout the fingerprinter writes.  The
 *               station's word index counts absolutely, in 64 bits, from its reset.
 *   query       one for every e with e = 0 (mod I), e >= W and words_before < e <= words_before + k, in ascending e; its window q is the
 *               station's words e - W ... e - 1.  For every valid p, errs(p) = sum_j popcount((q[j] ^ cat[p + j]) & mask); the result is
 *               the smallest errs, on a tie the smallest p, reported as track, offset = p - starts[track] and errs.  With an empty
 *               catalogue track = -1, offset = 0, errs = 0xffffffff.
 *   detector    per query, comparisons only.  hit = track >= 0 and errs <= max_errs.  On a hit: where the record's track differs, track
 *               and since = e are set; offset is set, misses = 0.  On a miss with the record's track >= 0: misses + 1, and at
 *               misses == hold the station is released: track = -1, misses = 0.
 *   event       24 bytes, 8-byte aligned, one per query: end (e) u64 at byte 0, track i32 at 8, offset i32 at 12, errs u32 at 16,
 *               flags u32 at 20 (bit 0 = hit).  A call writes a station's events, oldest first, from d_events + c * events_stride
 *               (in events) and their number to d_nevents[c]: at most fmd_fpmatch_max_events(interval, n); the slots behind them are
 *               left alone.
 *   bytes       d_flags[c]: bit 0 = identified (the record's track >= 0 after the call's last query), bit 1 = the station's last
 *               query ever was a hit; d_ok[c] = bit 0.  Written for every active station on every call, from the record, even when no
 *               query fired.  The record's flags hold the same two bits.
 *   inactive    a station whose d_active byte is 0 is skipped whole: ring, record, events, count and bytes are left as they are.
 * Nothing depends on how a station's words are split into calls, on streams, on the batch, on the station's row or on any tile size.
 * Ordinary vector stores, no global atomics, no workgroup waits on another.
 *   memory      the catalogue (4 bytes a word), a ring of W words a station, the call's query windows (W words a query) and the
 *               partial minima of the search (8 bytes a query and column group, at most 256 groups): fmd_fpmatch_state_bytes reports
 *               the whole for max_words, max_catalogue_words and max_tracks.
 *   index       a second search method for the same object, chosen at create (fmd_fpmatch_create_ex with an fmd_fpmatch_index_config):
 *               the paper's hash-index prefilter.  K = max_bucket, d = follow.  It is NOT exact: a query whose window shares no exact
 *               masked word with the right position misses.  Restated in numpy by tests/fpmatch_index_ref.py.  W, I, mask, D, starts,
 *               position validity, push, the query schedule, the detector, events, records, bytes and `inactive` are as above.  occ(k) is
 *               the set of catalogue word positions p' with cat[p'] & mask == k.  The candidate set S of a query with window q of
 *               station c:
 *                 look-ups   for j = 0 ... W - 1 and k = q[j] & mask: where |occ(k)| > K the word is skipped (a common word, such as
 *                            silence's, carries no information); otherwise every p' in occ(k) proposes p = p' - j.
 *                 follow     where d > 0 and the station's record is identified at the time of this query (track >= 0 after the
 *                            detector step of the station's previous query, also inside one call), p_exp = starts[track] + offset +
 *                            I * (misses + 1), and p_exp - d ... p_exp + d are proposed.
 *                 validity   S is the valid positions among those proposed (negative ones, ones above D - W and windows straddling two
 *                            tracks are dropped); duplicates count once.
 *               The result is the smallest errs(p) over S, on a tie the smallest p, reported as track, offset and errs as above; with S
 *               empty track = -1, offset = 0, errs = 0xffffffff, a miss.  Nothing depends on the call split, on tiling or on how
 *               repeated proposals are dropped.  fmd_fpmatch_load builds the index from the new catalogue on the host (a stable LSD
 *               radix sort of (masked word, position) pairs and a directory over the keys' top dir_bits); a refused catalogue keeps
 *               the old index, n_tracks = 0 empties it.
 *   index stats a 32-byte record per station (fmd_fpmatch_get_index_status), cleared by reset, kept by load, left alone for an
 *               inactive station: candidates = the sum over queries and j of |occ| for the words not skipped, skipped = the
 *               (query, j) pairs skipped, followed = the queries the follow rule applied to, empty = the queries with S empty.
 * Not built: soft or reliability-weighted bits, flipping unreliable bits to widen the look-up, building the index on the device, a
 * fall-back to the brute-force search on an indexed miss, station-against-station comparison, catalogues loaded from device memory or
 * appended to, several catalogues, per-station configurations.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_fpmatch_s* fmd_fpmatch;
typedef struct {
    int       n_channels;          /* C: station rows */
    int       n_bits;              /* 1 ... 32: the top n_bits of a word count */
    int       block;               /* W: words of a query, a multiple of 16 in 16 ... 1024 */
    int       interval;            /* I: words between searches, 1 ... 1024 */
    int       max_errs;            /* a query hits at errs <= max_errs: 0 ... W * n_bits */
    int       hold;                /* misses in a row that release a station, >= 1 */
    int       max_words;           /* largest n of a process call, in (0, 65536] */
    int       max_tracks;          /* in [1, 2^20] */
    long long max_catalogue_words; /* in [W, 2^28] */
    int       device;              /* HIP device ordinal, -1 = current */
} fmd_fpmatch_config;
/* the index of an indexed object (see "index" above) */
typedef struct {
    int       max_bucket;          /* K, 1 ... 64: a window word whose masked value the catalogue holds more than K times is skipped */
    int       follow;              /* d, 0 ... 8: an identified station's expected position +- d is proposed too; 0 = off */
} fmd_fpmatch_index_config;
/* what the kernels are built on, from the constants they use */
typedef struct {
    unsigned  mask;                /* 0xffffffff << (32 - n_bits) */
    int       tile;                /* catalogue positions of a column tile of the search */
    int       query_block;         /* queries a workgroup of the search holds in registers */
    int       groups;              /* column groups of the search at max_catalogue_words: the partial minima a query has, at most 256 */
    int       lds_bytes;           /* the search's LDS image: (tile + W - 1) words */
    long long max_events;          /* fmd_fpmatch_max_events(interval, max_words) */
    long long max_queries;         /* n_channels * max_events */
} fmd_fpmatch_design_t;
/* what the index and k_fpmatch_probe are built on */
typedef struct {
    int       dir_bits;            /* the directory is over the keys' top dir_bits: min(n_bits, ceil(log2(max_catalogue_words)) - 4) in 1 ... 24 */
    int       chunk;               /* candidates the probe's LDS list holds at most */
    int       chunk_words;         /* window words whose runs a chunk takes: min(256, chunk / K) */
    int       table;               /* slots of the LDS set that drops repeated proposals */
    long long dir_entries;         /* 2^dir_bits + 1 */
    long long index_bytes;         /* 8 * max_catalogue_words (keys and positions) + 4 * dir_entries */
} fmd_fpmatch_index_design_t;
/* one per station of an indexed object, 32 bytes.  After create and reset: all 0 */
typedef struct {
    unsigned long long candidates; /* the sum over queries and window words j of |occ| for the words not skipped */
    unsigned long long skipped;    /* (query, j) pairs skipped */
    unsigned long long followed;   /* queries to which the follow rule applied */
    unsigned long long empty;      /* queries with S empty */
} fmd_fpmatch_index_status;
/* one per query, 24 bytes */
typedef struct {
    unsigned long long end;        /* e: the station's word count at the window's end */
    int                track;      /* -1 with an empty catalogue */
    int                offset;     /* p - starts[track] */
    unsigned           errs;
    unsigned           flags;      /* bit 0 = hit */
} fmd_fpmatch_event;
/* one per station, 64 bytes: words at byte 0, queries 8, hits 16, clamped 24, since 32, track 40, offset 44, errs 48, misses 52,
 * fill 56, flags 60.  After create and reset: all 0 but track = -1 */
typedef struct {
    unsigned long long words;      /* words taken since reset */
    unsigned long long queries;    /* searches since reset */
    unsigned long long hits;       /* of them hits */
    unsigned long long clamped;    /* calls whose d_nwords entry lay outside [0, n] */
    unsigned long long since;      /* e of the query that identified the current track */
    int                track;      /* the identified track, -1 = none */
    int                offset;     /* of the last hit */
    unsigned           errs;       /* the last query's */
    unsigned           misses;     /* misses in a row while identified */
    unsigned           fill;       /* min(words, W) */
    unsigned           flags;      /* bit 0 = identified, bit 1 = the last query was a hit */
} fmd_fpmatch_status;

/* host-only (no GPU needed) */
/* one station, n_bits 32, block 256 (the paper's), interval 64, max_errs (35 * 256 * 32) / 100, hold 3, max_words 64,
 * max_tracks 4096, max_catalogue_words 2^22, the current device */
int fmd_fpmatch_default_config(fmd_fpmatch_config* cfg);
/* (n + interval - 1) / interval: the most events a call of n words writes for a station.  FMD_ERR_ARG for interval outside
 * 1 ... 1024 or n outside [0, 65536] */
long long fmd_fpmatch_max_events(int interval, long long n);
/* (ber_percent * block * n_bits) / 100 in integers: the threshold for a bit error rate in per cent.  FMD_ERR_ARG for ber_percent
 * outside 0 ... 100, block no multiple of 16 in 16 ... 1024 or n_bits outside 1 ... 32 */
long long fmd_fpmatch_max_errs(int ber_percent, int block, int n_bits);
/* FMD_OK for a valid configuration and then *out (may be NULL) written; FMD_ERR_ARG otherwise and nothing written */
int fmd_fpmatch_design(const fmd_fpmatch_config* cfg, fmd_fpmatch_design_t* out);
/* FMD_OK where fmd_fpmatch_load would take starts [n_tracks + 1] (NULL allowed for n_tracks = 0) under cfg, FMD_ERR_ARG otherwise */
int fmd_fpmatch_check_catalogue(const fmd_fpmatch_config* cfg, const long long* starts, int n_tracks);
/* the bytes of device memory an object of cfg holds; FMD_ERR_ARG for an invalid configuration */
long long fmd_fpmatch_state_bytes(const fmd_fpmatch_config* cfg);
/* max_bucket 8, follow 2 */
int fmd_fpmatch_index_default_config(fmd_fpmatch_index_config* idx);
/* FMD_OK for a valid pair of configurations and then *out (may be NULL) written; FMD_ERR_ARG otherwise and nothing written */
int fmd_fpmatch_index_design(const fmd_fpmatch_config* cfg, const fmd_fpmatch_index_config* idx, fmd_fpmatch_index_design_t* out);
/* the bytes of device memory an indexed object holds: the brute-force object's with one partial minimum a query instead of one a
 * column group, a (candidates, skipped) pair a query, the index records and the index; FMD_ERR_ARG for an invalid pair */
long long fmd_fpmatch_index_state_bytes(const fmd_fpmatch_config* cfg, const fmd_fpmatch_index_config* idx);
/* the index fmd_fpmatch_load builds, into host memory: keys [n_words] the masked words ascending, pos [n_words] their positions (equal
 * keys in ascending position), dir [dir_entries]: dir[b] = the first i with keys[i] >> (32 - dir_bits) >= b.  FMD_ERR_ARG, and nothing
 * written, for an invalid pair, n_words outside [0, max_catalogue_words] or a null array (keys, pos and words may be NULL at n_words 0) */
int fmd_fpmatch_index_build(const fmd_fpmatch_config* cfg, const fmd_fpmatch_index_config* idx, const uint32_t* words, long long n_words, uint32_t* keys, int* pos,
                            int* dir);

/* FMD_ERR_DEVICE where the device memory (fmd_fpmatch_state_bytes) cannot be had */
int fmd_fpmatch_create(const fmd_fpmatch_config* cfg, fmd_fpmatch* out);
/* idx == NULL is fmd_fpmatch_create exactly; otherwise an indexed object (see "index" above; its memory is fmd_fpmatch_index_state_bytes) */
int fmd_fpmatch_create_ex(const fmd_fpmatch_config* cfg, const fmd_fpmatch_index_config* idx, fmd_fpmatch* out);
int fmd_fpmatch_destroy(fmd_fpmatch h);
/* station `channel` (-1 = every station) as after create: ring emptied, counters 0, track -1; the catalogue stays.  Waits for the
 * object's earlier work */
int fmd_fpmatch_reset(fmd_fpmatch h, int channel);
/* replaces the catalogue: words [starts[n_tracks]] and starts [n_tracks + 1] in host memory (see "catalogue" above) */
int fmd_fpmatch_load(fmd_fpmatch h, const uint32_t* words, const long long* starts, int n_tracks);
/* takes up to n words of every station.  d_words [C][words_stride] uint32 on the device, 4-byte aligned; d_nwords: [C] int32 on the
 * device or NULL; d_active: [C] uint8 on the device or NULL = all; d_events: caller-owned fmd_fpmatch_event rows on the device, 8-byte
 * aligned, events_stride in events, at least fmd_fpmatch_max_events(interval, n); d_nevents [C] int32, d_flags [C] uint8 and d_ok [C]
 * uint8 on the device, each may be NULL.  n = 0 is valid.  n < 0, n > max_words, n > words_stride, a short events_stride, or a null or
 * misaligned d_words or d_events return FMD_ERR_ARG and change nothing.  Asynchronous on `stream`; consecutive calls may use different
 * streams (the library orders them). */
int fmd_fpmatch_process_dev(fmd_fpmatch h, const uint32_t* d_words, long long words_stride, const int* d_nwords, int n, const uint8_t* d_active,
                            fmd_fpmatch_event* d_events, long long events_stride, int* d_nevents, uint8_t* d_flags, uint8_t* d_ok, void* stream);
/* out [C]; synchronises with the object's work */
int fmd_fpmatch_get_status(fmd_fpmatch h, fmd_fpmatch_status* out);
/* the device's own [C] records, for a consumer on the device: ordered behind the object's work on the stream of its last call, valid
 * until the next call */
int fmd_fpmatch_status_dev(fmd_fpmatch h, const fmd_fpmatch_status** d_status);
/* out [C]; synchronises with the object's work.  FMD_ERR_STATE on an object created without an index */
int fmd_fpmatch_get_index_status(fmd_fpmatch h, fmd_fpmatch_index_status* out);
const char* fmd_fpmatch_last_error(fmd_fpmatch h);

/* ------------------------------------------------------------------------------------------------------------------
 * Look-ahead peak limiter (NOT part of the reference): the stage that acts on a level.  A make-up gain per station and a brick-wall
 * look-ahead limiter with a ceiling, behind the loudness measurement as EBU R 128 practice has it.  It reads the device array
 * [C][in_stride][2] f32 (interleaved L, R) that the mixer, the monitors and the encoders read (station audio or a mixer's bus output),
 * changes nothing in it, and writes a caller-owned [C][out_stride][2] f32 array: the same audio, delayed by D frames, times the
 * station's gain, limited to the ceiling T.  Stereo only, fs 8000 ... 192000 Hz.  Sample peaks, not true peaks.
 * Arithmetic, restated in C by tests/cpp/limiter_ref.c.  Per station the frame index n counts from the station's reset or flush;
 * ONE = 2^30;  W = D + 1;  everything from before index 0 counts as silence at unity gain: u = 0, rq = mq = eq = ONE.
 *   gain        u[n] = x[n] * gain                              one fp32 multiply per rail, round to nearest, with the station's gain as it
 *               stands when the call is made.  A rail value that is NaN or +-inf after the multiply becomes +0, nonfinite++ (per sample)
 *   peak        p[n] = max(|uL[n]|, |uR[n]|)                    linked: both rails get one gain, the stereo image holds still
 *   required    rq[n] = ONE where p[n] <= T, else (uint32)((T / p[n]) * 2^30f): the correctly rounded fp32 division (no reciprocal
 *               approximation), an exact multiply, a truncating conversion.  fp32 denormals are kept
 *   look-ahead  mq[n] = min(rq[n - W + 1 ... n])
 *   release     eq[n] = min(mq[n], eq[n - 1] + step), in integers, eq[-1] = ONE: a gain that recovers on a straight line, step per
 *               frame.  Closed form, exact in int64, with eq_in the eq just before the span's first frame (index 0 of the span):
 *                 eq[n] = min(eq_in + (n + 1) * step, min over j <= n of (mq[j] + (n - j) * step))
 *   attack      S[n] = sum of eq[n - W + 1 ... n], exact in uint64;  g[n] = (float)S[n] / (float)(W * 2^30): the conversion rounds to
 *               nearest, the division is the correctly rounded fp32 division.  g[n] = 1.0f exactly where nothing in reach is over T
 *   output      y[n] = u[n - D] * g[n] per rail, one fp32 multiply;  then y > T -> T and y < -T -> -T, each with the rail's clamped++
 *               (the roundings of T / p and of g can leave a product one ulp over).  limited++ where S[n] < W * ONE
 *   ceiling     |y| <= T always: every eq under the sum is at most rq[n - D], so g[n] <= rq[n - D] / ONE before rounding
 *   transparent where no frame in [n - 2D, n] exceeds T after the gain and the release has returned to ONE, y[n] is u[n - D] bit for bit
 *   streaming   eq, the last D values of rq and of eq and the last D frames of u live in the limiter and carry to the next call.  Every
 *               scan is in integers: nothing depends, bit for bit, on how the frames are split into calls, on streams, on the batch or
 *               on the station's row.  Ordinary stores, no atomics.
 *   flush       writes the D frames that D frames of silence would push out, and D to d_nout[c];  they count in limited, clamped and
 *               min_gain, not in frames.  Then the station's signal state is as after reset; counters and gain stay.  A whole
 *               stream's output is therefore D zero frames followed by the limited input, frames + D in all.
 *   design      host, double, host libm (fmd_limiter_design):  D = llround(lookahead_ms * fs / 1000), in [0, 255];
 *               step = clamp(llround(2^30 / (release_ms * fs / 1000)), 1, 2^30), release_ms = 0 gives 2^30 (an instant release):
 *               release_ms is the time the gain needs from 0 to 1;  T = (float)pow(10, ceiling_db / 20), ceiling_db in [-40, 0].
 *               The defaults (1.5 ms, 500 ms, -1 dBFS: a 3 dB reduction recovers in about 150 ms) are conventional values; nobody
 *               has tuned them by listening.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fmd_limiter_s* fmd_limiter;
typedef struct {
    int       n_channels;         /* C: station rows of the input and the output */
    int       fs;                 /* Hz, 8000 ... 192000 */
    double    lookahead_ms;       /* D = llround(lookahead_ms * fs / 1000) frames, at most 255 */
    double    release_ms;         /* the time the gain needs from 0 to 1; 0 = instant */
    double    ceiling_db;         /* dBFS, -40 ... 0 */
    long long max_input_frames;   /* largest n of a process call, in (0, 2^30] */
    int       device;             /* HIP device ordinal, -1 = current */
} fmd_limiter_config;
typedef struct {
    int      lookahead_frames;    /* D */
    unsigned step;                /* Q30 per frame, 1 ... 2^30 */
    float    ceiling;             /* T */
    int      latency_frames;      /* D */
} fmd_limiter_design_t;
/* one per station, 64 bytes: frames at byte 0, limited 8, clamped 16, nonfinite 32, min_gain 40, gain 44, eq 48, reserved 52 */
typedef struct {
    unsigned long long frames;        /* frames taken since reset */
    unsigned long long limited;       /* output frames with S < W * ONE */
    unsigned long long clamped[2];    /* output samples of L, R moved back to +-T */
    unsigned long long nonfinite;     /* samples (of either rail) that were NaN or +-inf after the gain: taken as +0 */
    float              min_gain;      /* the smallest g since reset; 1 after a reset */
    float              gain;          /* the station's gain, as set */
    unsigned           eq;            /* the release state, Q30 */
    unsigned char      reserved[12];
} fmd_limiter_status;

/* host-only (no GPU needed) */
/* D, step, T and the latency as `design` above says; FMD_ERR_ARG for fs outside 8000 ... 192000, a look-ahead above 255 frames, a
 * negative time or ceiling_db outside [-40, 0] */
int fmd_limiter_design(int fs, double lookahead_ms, double release_ms, double ceiling_db, fmd_limiter_design_t* out);
/* one station, 1.5 ms look-ahead, 500 ms release, -1 dBFS ceiling, max_input_frames 65536, the current device */
int fmd_limiter_default_config(int fs, fmd_limiter_config* cfg);
/* 10^((target_lufs - lufs) / 20) as a float: what takes fmd_meter_integrated's result to fmd_limiter_set_gain */
float fmd_limiter_gain_for_loudness(double lufs, double target_lufs);

int fmd_limiter_create(const fmd_limiter_config* cfg, fmd_limiter* out);
int fmd_limiter_destroy(fmd_limiter l);
/* station `channel` (-1 = every station) as after create, except that its gain stays.  Waits for the limiter's earlier work */
int fmd_limiter_reset(fmd_limiter l, int channel);
/* the gain of station `channel` (-1 = of every station): finite and >= 0, else FMD_ERR_ARG; 1 after create.  It holds for the frames
 * that later calls take; waits for the limiter's earlier work */
int fmd_limiter_set_gain(fmd_limiter l, int channel, float gain);
int fmd_limiter_get_gain(fmd_limiter l, int channel, float* gain);
/* takes n frames of every station and writes n output frames at d_out + c * out_stride.  d_in [C][in_stride][2] f32 and d_out
 * [C][out_stride][2] f32 on the device, 8-byte aligned, strides in frames; frames of d_out behind n are left as they are.  d_active:
 * [C] uint8 on the device, NULL = all: a station whose byte is 0 is skipped whole, its state, its row of d_out and its d_gr are left
 * as they are.  d_gr: [C] f32 on the device, may be NULL: the smallest g among the call's output frames, 1.0f for n = 0.  n < 0,
 * n > in_stride, n > out_stride, n > max_input_frames, a null or misaligned d_in or d_out, or an output range (d_out up to row C - 1's
 * frame n) that overlaps the input's range return FMD_ERR_ARG and change nothing.  Asynchronous on `stream`; consecutive calls may use different streams (the library orders
 * them). */
int fmd_limiter_process_f32_dev(fmd_limiter l, const float* d_in, long long in_stride, long long n, const uint8_t* d_active, float* d_out,
                                long long out_stride, float* d_gr, void* stream);
/* station `channel` (-1 = every station) as `flush` above says: D frames at d_out + c * out_stride and D in d_nout[c] ([C] int32 on
 * the device, may be NULL); other stations' rows and counts are left as they are.  d_out 8-byte aligned and out_stride at least D, else
 * FMD_ERR_ARG.  Asynchronous on `stream`, ordered like a process call */
int fmd_limiter_flush(fmd_limiter l, int channel, float* d_out, long long out_stride, int* d_nout, void* stream);
/* out [C]; synchronises with the limiter's work */
int fmd_limiter_get_status(fmd_limiter l, fmd_limiter_status* out);
/* the device's own [C] records, for a consumer on the device: ordered behind the limiter's work on the stream of its last call, valid
 * until the next call */
int fmd_limiter_status_dev(fmd_limiter l, const fmd_limiter_status** d_status);
const char* fmd_limiter_last_error(fmd_limiter l);

#ifdef __cplusplus
}
#endif
#endif
