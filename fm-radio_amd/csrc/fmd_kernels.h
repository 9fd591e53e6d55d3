// Device-side data model and kernel launch interface of the batched FM demodulator.
// See DESIGN.md for the pipeline; each kernel's header comment cites the reference code it replaces.
// The tolerance mode's tables (PilotFastTab, PllSpanTab, PllSparseTab) and the layout constants the host's designers share with the
// kernels are in fmd_tables.h, which has no HIP in it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>

#include "fmd_plan.h"
#include "fmd_schedule.h"
#include "fmd_tables.h"
#include "fmdemod.h"

namespace fmd {

// Development switches (A/B timing, bounding experiments: tools/) are read from the environment only in builds with -DFMD_DEV_HOOKS
// (`make -C fm-radio_amd/csrc dev`); the shipping library reads GPU_MAX_HW_QUEUES and FMD_QUIET and nothing else.
#ifdef FMD_DEV_HOOKS
inline const char* dev_env(const char* name) { return std::getenv(name); }
#else
inline const char* dev_env(const char*) { return nullptr; }
#endif

// Coefficients shared by every channel, passed to kernels by value (kernarg -> scalar loads).
struct FrontTaps {
    float b_fm_in[64];
    float b_fm_out[64];
    float b_hilbert_odd[32];  // the 32 non-zero Hilbert taps, b[1], b[3], ..., b[63]
    float fm_gain;
};

struct RdsTaps { float b[128]; };

struct LoopCoeffs {
    float pilot_k, pilot_a0, pilot_a1;       // y = fma(a0, y[n-2], k*x[n-2]) + a1*y[n-1]
    float pll_b0, pll_b1, pll_a0;            // 1-pole loop filter, newest-last arrays: b=[b0,b1], a=[a0,1]
    float ted_b0, ted_b1, ted_a0;
    float bpsk_b0, bpsk_b1, bpsk_a0;
};

// Per-channel serial state, structure-of-arrays ([field][C]) so a wavefront's 64 lanes (64 adjacent
// channels) load and store it coalesced.  Field list = SURVEY.md A.8 / reference member variables.
enum StateField : int {
    // pilot peak IIR
    SA_X1R, SA_X1I, SA_X2R, SA_X2I, SA_Y1R, SA_Y1I, SA_Y2R, SA_Y2I,
    S_PILOT_POWER0, S_PILOT_POWER1, S_PILOT_POWER2, S_PILOT_POWER3, S_PILOT_POWER4, S_PILOT_POWER5, S_PILOT_POWER6, S_PILOT_POWER7, // sum |pilot|^2 of the block in pipeline slot 0..7 (power pass -> PLL pass)
    S_AGC_PILOT_GAIN,
    S_PLL_X1, S_PLL_Y1, S_PLL_INT, S_PLL_ERR, S_PLL_T,
    S_LMR_PHASE_CUR, S_LMR_PHASE_PREV,
    S_AGC_RDS_GAIN,
    // BPSK synchroniser (reference bpsk_synchroniser.h:40-59)
    S_B_PLL_X1, S_B_PLL_Y1, S_B_PLL_INT, S_B_PLL_ERR, S_B_MIX_T,
    S_B_ZCD_XN, S_B_COOLDOWN, S_B_TED_ERR, S_B_TED_X1, S_B_TED_Y1, S_B_TED_INT, S_B_CLOCK,
    S_B_DUMP_R, S_B_DUMP_I,
    // de-emphasis IIR
    S_DE_X1, S_DE_Y1,
    // Manchester decoder (bit-packed ints stored as float bit patterns)
    S_M_FLAGS, S_M_BUF0, S_M_BUF1, S_M_BUF2, S_M_BUF3,
    S_NUM_FIELDS
};

struct Dims {
    int C;          // channels
    int N;          // baseband samples per block
    int m;          // stage-1 decimation (1, 4, 8)
    int n_fm_in, n_fm_out, n_rds, n_audio, n_est;
    int tail_base;  // fm_in samples of history k_front keeps per channel
};

// Stream buffers are indexed by pipeline slot (= block index % kSlots, fmd_schedule.h)
static_assert(kSlots <= 8, "one S_PILOT_POWER state field per slot");
// buf = block % kSlots (stream buffers), par = block & 1 (history tails); t0/t1: optional events that receive the stage's
// first kernel's start and last kernel's end timestamps (attached to the dispatch packets themselves: no extra queue packets)
// done: optional event that is to fire when the stage's last kernel has completed, carried by that kernel's own dispatch
// packet (a separate hipEventRecord is one more queue packet between two dependent kernels, ~25 us on the PLL stream)
// seq: 1-based number of the block when consecutive blocks' k_pilot_pll launches hand over per wavefront (Buffers::pll_chain),
// 0: plain stream order
// warm: tolerance mode, a block inside some station's first kPllWarmSamples after a reset / a restored start-up state: k_pll_span runs
// beside k_pll_sparse and each station takes the result of the one in charge of it
// FMD_FLAG_KEEP_TAPS in the exact mode: the traces behind the reference's GetPilotOutput / GetPLLOutput / Get_PLL_Raw_Phase_Error_Output /
// Get_PLL_LPF_Phase_Error_Output (broadcast_fm_demod.h:245-248) and BPSK_Synchroniser's Get* views (bpsk_synchroniser.h:78-85); all null otherwise
struct TapPtrs {
    float2* pilot; float2* pll; float* pll_raw; float* pll_pi;                                     // [C][n_fm_out]
    float2* b_pll_sym; float2* b_intdump; float* b_ted_raw; float* b_ted_pi; float* b_pll_raw; float* b_pll_pi; float* b_zcd; float* b_trig;   // [C][n_rds]
};
struct SlotRef { int buf; int par; hipEvent_t t0 = nullptr; hipEvent_t t1 = nullptr; hipEvent_t done = nullptr; unsigned seq = 0; int warm = 0; };
struct Buffers {
    // history tails: stage of block b reads [par], writes [par^1] (producer and consumer are the same stage, same stream)
    float2* base_tail[2];   // [C][tail_base]  fm_in history of k_front
    float2* pre_tail[2];    // [C][64]         baseband history of k_predecim (m > 1)
    float2* fm_in[kSlots];  // [C][n_fm_in]    the first decimator's output (m > 1)
    float2* iq_tail[2];     // [C][128]   last fm_out_iq samples of the previous block
    float*  dt_tail[2];     // [C][128]   last pll_dt samples of the previous block
    float*  fo_tail[2];     // [C][64]    last fm_out samples (Hilbert FIR history, de-emphasis path)
    // intermediate streams
    float2* fm_out_iq[kSlots];   // [C][n_fm_out]
    float*  fm_out[kSlots];      // [C][n_fm_out]  (de-emphasis path only)
    float2* pilot[kSlots];       // [C][n_fm_out]  pilot peak IIR output before AGC (k_pilot_power -> k_pilot_pll)
    float*  pll_dt[kSlots];      // [C][n_fm_out]
    float2* rds[kSlots];    // [C][n_rds]      (extract -> rds_sync, which runs on its own stream)
    float*  lmr_est[2];     // [C][n_est], by block parity (the next block's k_extract integrates them)
    float*  lmr_peek;       // [C] scratch row of the "lmr_phase" getter
    // outputs
    float*  audio[kSlots];       // [C][n_audio][2]
    float*  rds_sym[kSlots];     // [C][n_rds]
    float2* rds_raw_sym[kSlots]; // [C][n_rds]      (KEEP_TAPS)
    float*  taps[kSlots];        // exact mode + KEEP_TAPS: the loops' per-sample traces, one allocation per slot (tap_ptrs() for the layout)
    int*    rds_count[kSlots];   // [C]
    float*  lpr[kSlots];         // [C][n_audio]    (KEEP_TAPS)
    float*  lmr[kSlots];         // [C][n_audio]    (KEEP_TAPS)
    uint8_t* rds_bytes[kSlots];  // [C][bytes_cap]
    int*    rds_bytes_count[kSlots]; // [C]
    // FMD_FLAG_RDS_DECODE only (null otherwise): k_rds_decode's outputs
    fmd_rds_db*    rds_db[kSlots];            // [C]   database after the block
    fmd_rds_group* rds_groups[kSlots];        // [C][rds_groups_cap(bytes_cap)]
    int*           rds_groups_count[kSlots];  // [C]
    // per-channel controls
    float*  b_lpr;          // [C][128]
    float*  b_lmr;          // [C][128]
    float*  deemph;         // [C][4]  b0,b1,a0,flag
    float*  mix;            // [C][2]  audio mode (as float), stereo mix factor
    float*  state;          // [S_NUM_FIELDS][C]
    // FMD_FLAG_FAST_MATH (round 3): planar analytic signal and the PLL's span polynomials
    float*  fo_pl[kSlots];           // [C][kFoPad + n_fm_out]  fm_out (the analytic signal's real rail is this delayed by 32)
    float4* pll_poly[kSlots];        // [C][1 + n_fm_out / kSpan]  NCO phase of a span: c0 + c1 u + c2 u^2 + c3 u^3 - frac(19 (u + 1) / 128), u = sample in span
    float*  rds_pow[kSlots];         // [C][2 n_audio / 256]  partial sums of |rds|^2 (k_extract_bp -> k_rds_sync's AGC)
    PllSpanTab* span_tab;
    PllSparseTab* sparse_tab;
    float4* pv_pl[kSlots];           // [C][n_fm_out / 16] per 16-sample column of fm_out: (new.re, new.im, old.re, old.im), the two half sums of the pilot points' inputs
    float4* pv_hist[2];              // [C][4] the previous block's last four columns, by block parity (k_pll_sparse reads [par], writes [par ^ 1])
    PilotFastTab* pilot_tab;         // FMD_FLAG_FAST_MATH only
    int2*   aud_idx;                 // [C] slots of a station's L+R and L-R images
    uint4*  bp_tab;                  // k_extract_bp: per distinct cut-off the zero-padded tap tables of the L+R FIR and of the L-R composite band-pass FIR's two rails (12 tables a slot, fmd_kernels_bp.inc)
    uint4*  rds_bp_tab;              // ... of the RDS composite band-pass FIR (4 tables) and of its first-order term (2)
    uint4*  bp_edge;                 // ... per cut-off slot [31 outputs][8 lanes][6] (fp16 pairs): the matrix of the block's first outputs' sums over the previous block's samples
    uint4*  front_mfma;              // FMD_FLAG_FAST_MATH only: Toeplitz operand images of k_front_mfma's two FIRs, [fir][k-step][hi/lo][lane]; m > 1: then k_predecim_mfma's
    unsigned int* pll_chain;         // [wavefronts of k_pilot_pll + 1] last block number each wavefront completed; [last] = watchdog flag
    unsigned int* pll_hint;          // [C] 1: the station's wavefront left the previous block out of lock (it runs the kernel's sequence-capable body); [C]: the newest launch (LaunchCtx::pll_launch_no) in which a wavefront spent a quarter of the block or more out of lock, [C + 1]: the newest launch that has run
    unsigned long long* spec_stats;  // [8] speculation counters: pll {chunks, general, replayed, -}, rds {chunks, general, replayed, -}
};

// RDS decoding chain (k_rds_decode, fmd_kernels_rds.inc): per-channel state.  The synchroniser's scalars are planar [RDS_F_NUM][C]
// (one coalesced load / store per field and launch); the group being assembled and the database are one record per channel.
enum RdsDecField { RDS_F_WIN, RDS_F_SYN, RDS_F_HUNT, RDS_F_BITS, RDS_F_BLOCK, RDS_F_ERRORS, RDS_F_DESYNC, RDS_F_AB, RDS_F_NUM };
// window (26 bits), its syndrome, 1 = FINDING_SYNC, bits into the block, curr_data_block, block errors in the group,
// consecutive groups with errors, the handler's A/B memories (radio text | programme type name << 8; both start at 0b100)
struct RdsDecBufs {
    uint32_t* f;              // [RDS_F_NUM][C]
    fmd_rds_group* group;     // [C]
    fmd_rds_db* db;           // [C]
};
inline size_t rds_dec_state_bytes(int C) { return (size_t)C * (RDS_F_NUM * sizeof(uint32_t) + sizeof(fmd_rds_group) + sizeof(fmd_rds_db)); }
// the three arrays inside one allocation of rds_dec_state_bytes(C)
inline RdsDecBufs rds_dec_bufs(void* base, int C) {
    RdsDecBufs s;
    s.f = static_cast<uint32_t*>(base);
    s.group = reinterpret_cast<fmd_rds_group*>(s.f + (size_t)RDS_F_NUM * C);
    s.db = reinterpret_cast<fmd_rds_db*>(s.group + C);
    return s;
}
// one channel's state as the fields of a freshly constructed RDS_Decoding_Chain
inline void rds_dec_initial(uint32_t f[RDS_F_NUM], fmd_rds_group* group, fmd_rds_db* db) {
    for (int i = 0; i < RDS_F_NUM; i++) f[i] = 0;
    f[RDS_F_HUNT] = 1;
    f[RDS_F_AB] = 0x4u | (0x4u << 8);
    *group = fmd_rds_group{};
    *db = fmd_rds_db{};
}
static_assert(sizeof(fmd_rds_db) == 120 && sizeof(fmd_rds_group) == 16, "fixed layouts of include/fmdemod.h");
struct RdsDecArgs {
    int C;
    const uint8_t* bytes;     // [C][cap]
    const int* counts;        // [C]
    int cap;
    RdsDecBufs st;
    fmd_rds_db* db_out;       // [C]   snapshot after this launch's bytes
    fmd_rds_group* groups_out;   // [C][groups_cap]
    int* groups_count;        // [C]
    int groups_cap;
};
inline int rds_groups_cap(int cap_bytes) { return cap_bytes * 8 / 79 + 2; }
// t1: optional event that receives the kernel's end timestamp / completion (as FMD_LAUNCH's last-kernel event)
hipError_t launch_rds_decode(const RdsDecArgs& a, hipStream_t s, hipEvent_t t1 = nullptr);

struct LaunchCtx {
    Dims d;
    Buffers b;
    FrontTaps front;
    RdsTaps rds_taps;
    LoopCoeffs loops;
    int keep_taps;
    int fast;                             // FMD_FLAG_FAST_MATH: the tolerance-mode kernels
    int bytes_cap;
    int rds_decode;                       // FMD_FLAG_RDS_DECODE: k_rds_decode behind k_rds_sync (state in rds_dec)
    RdsDecBufs rds_dec;
    Plan plan;                            // which kernels this batch gets (fmd_plan.h): made once, by fmd_create
    PlanFacts facts;                      // what the controls and the debug hooks have set; whoever changes one calls refresh_block_plan
    BlockPlan block;                      // each stage's kernel form and launch geometry, from plan and facts: the launchers read it and decide nothing
    Dims d_front;                         // the block as k_front / k_front_mfma see it: a 256 kSa/s batch (behind the first decimator: N = n_fm_in, m = 1)
    unsigned pll_launch_no;               // 1-based number of the pilot-PLL launch being queued (exact mode)
    bool pll_unlocked_now;                // wavefronts ran out of lock in the last blocks the host has seen (fmd_api.cpp): pll_kernel()'s second argument
};

// After fmd_create, a control upload or a debug hook (everything idle): ctx.plan or ctx.facts may have changed
inline void refresh_block_plan(LaunchCtx& ctx) {
    ctx.block = make_block_plan(ctx.plan, ctx.facts);
    ctx.d_front = ctx.d;
    if (ctx.d.m > 1) { ctx.d_front.N = ctx.d.n_fm_in; ctx.d_front.m = 1; }
}

// where a slot's traces lie inside Buffers::taps[buf] (null pointers when the handle keeps none)
inline TapPtrs tap_ptrs(const LaunchCtx& ctx, int buf) {
    TapPtrs t{};
    float* p = ctx.b.taps[buf];
    if (!p) return t;
    const size_t nf = (size_t)ctx.d.C * ctx.d.n_fm_out, nr = (size_t)ctx.d.C * ctx.d.n_rds;
    t.pilot = reinterpret_cast<float2*>(p); p += 2 * nf;
    t.pll = reinterpret_cast<float2*>(p); p += 2 * nf;
    t.pll_raw = p; p += nf;
    t.pll_pi = p; p += nf;
    t.b_pll_sym = reinterpret_cast<float2*>(p); p += 2 * nr;
    t.b_intdump = reinterpret_cast<float2*>(p); p += 2 * nr;
    t.b_ted_raw = p; p += nr;
    t.b_ted_pi = p; p += nr;
    t.b_pll_raw = p; p += nr;
    t.b_pll_pi = p; p += nr;
    t.b_zcd = p; p += nr;
    t.b_trig = p;
    return t;
}
inline size_t tap_floats(const Dims& d) { return (size_t)d.C * (6 * (size_t)d.n_fm_out + 10 * (size_t)d.n_rds); }

// One launcher per pipeline stage of one block.  The host (fmd_api.cpp) places the stages on
// streams and orders them with events.
hipError_t launch_stage_predecim(const LaunchCtx& ctx, SlotRef r, const void* d_iq, bool u8, hipStream_t s);   // k_predecim (m > 1)
// pll != NULL (tolerance mode only): the pilot stage of the block in slot pll->buf rides in the same launch (k_front_mfma<..., FUSED>)
hipError_t launch_stage_front(const LaunchCtx& ctx, SlotRef r, const void* d_iq, bool u8, hipStream_t s, const SlotRef* pll = nullptr);   // k_front
// (m > 1, BlockPlan::front == FrontPreMfma: the first decimator runs inside launch_stage_front's kernel and the block has no predecim stage)
hipError_t launch_stage_deemph(const LaunchCtx& ctx, SlotRef r, hipStream_t s);                            // k_deemphasis + k_hilbert
hipError_t launch_stage_power(const LaunchCtx& ctx, SlotRef r, hipStream_t s);                             // k_pilot_power
hipError_t launch_stage_pll(const LaunchCtx& ctx, SlotRef r, hipStream_t s);                               // k_pilot_pll
hipError_t launch_stage_extract(const LaunchCtx& ctx, SlotRef r, hipStream_t s);                           // k_extract
hipError_t launch_stage_rds(const LaunchCtx& ctx, SlotRef r, hipStream_t s);                               // k_rds_sync
hipError_t launch_lmr_phase_peek(const LaunchCtx& ctx, int par, float* out_row, hipStream_t s);            // k_lmr_phase into a scratch row
hipError_t launch_reset_state(const LaunchCtx& ctx, hipStream_t stream);
hipError_t selftest_atan2(const float* d_y, const float* d_x, float* d_out, unsigned char* d_ok, size_t n, int table_form, hipStream_t s);
hipError_t launch_audio_pcm16(const float* d_audio, int16_t* d_pcm, size_t n_values, hipStream_t s);   // k_audio_pcm16
hipError_t prepare_kernels();          // one-time function attributes (dynamic LDS sizes)
int front_tail_len(int m, bool fast);  // input-history samples k_front keeps per channel

}  // namespace fmd
