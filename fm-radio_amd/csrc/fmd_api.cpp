// C ABI of libfmdemod.so (include/fmdemod.h): handle management, per-channel controls, device buffers and
// the HIP side of the per-block kernel launch sequence.  Host side only; the kernels are in fmd_kernels.hip, the coefficient
// design in fmd_design.cpp, the design of the tolerance mode's tables in fmd_tables.cpp and the block schedule — which stage goes on
// which queue behind which events — in fmd_schedule.cpp (all three without HIP).
// There is no CPU fallback: without a gfx950 device every call fails loudly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "fmd_design.h"
#include "fmd_kernels.h"
#include "fmd_plan.h"
#include "fmd_schedule.h"
#include "fmd_tables.h"
#include "fmdemod.h"
#include "fmdemod_debug.h"

using namespace fmd;

struct ProfiledBlock { hipEvent_t t0[ST_COUNT], t1[ST_COUNT]; bool used[ST_COUNT]; };

struct fmd_handle_s {
    fmd_config cfg{};
    LaunchCtx ctx{};
    fmd_coeffs base{};                       // coefficients common to all channels (+ channel-0 control designs)
    std::vector<fmd_controls> controls;      // per channel
    bool controls_dirty = true;
    bool deemph_on = false;                  // some channel uses the de-emphasis IIR
    bool deemph_linger = false;              // keep that path one more block after the last channel leaves it, so the
                                             // Hilbert FIR sees the de-emphasised history the reference would hold
    std::vector<void*> allocs;
    void* d_in = nullptr;                    // staging for the host-pointer entry points
    size_t d_in_bytes = 0;
    hipStream_t own_stream = nullptr;        // host-pointer entry points, uploads, resets
    hipStream_t last_stream = nullptr;       // the caller's stream of the newest block (unpipelined: where its stages ran)
    hipStream_t sF = nullptr, sA = nullptr, sB = nullptr, sX = nullptr, sR = nullptr, sD = nullptr;   // the schedule's queues F A B X R D (Q_OWN is own_stream); sD: the optional de-emphasis stage
    Schedule sched;                          // which stage goes on which queue behind which events (fmd_schedule.h); HipBackend below makes the calls
    // exact mode, Plan::pll_k_adaptive (above kPllK16MaxEff, up to kPllK16UnlockedMaxEff effective stations): the pilot-PLL kernel's lane count follows what is out of lock — 8 lanes a station while every
    // loop holds lock (fewest instructions beside the FIR kernels), 16 while some do not (a loop out of lock costs its wavefront ~1.8x, and
    // the kernel lasts as long as its slowest wavefront: 1.55 -> 1.12 ms a block with 16).  The kernel counts the wavefronts that ran out
    // of lock (Buffers::pll_hint[C]); a 4-byte copy of the counter comes back every other block, and the host looks at it without waiting.
    // The host may be queueing many blocks ahead of the GPU: what it goes by is the pair that came back — the newest launch that had wavefronts out
    // of lock and the newest launch that has run: out of lock "now" while the two are fewer than 8 launches apart; no news, no change.
    unsigned* pll_unl_host = nullptr;        // pinned: [0] newest launch with wavefronts out of lock, [1] newest launch that has run
    hipEvent_t ev_in = nullptr, ev_P[kSlots] = {}, ev_F[kSlots] = {}, ev_A[kSlots] = {}, ev_B[kSlots] = {}, ev_E[kSlots] = {}, ev_X[kSlots] = {};
    hipEvent_t ev_D[kSlots] = {};            // k_front done, de-emphasis stage may start
    hipEvent_t ev_C[kSlots] = {};            // fmd_release_outputs: the consumer of a slot's outputs has finished with them
    bool poisoned = false;                   // a block failed part-way: state is not the state after a whole number of blocks
    bool pipelined = true;
    long epoch = 0;                          // how often the block numbering restarted (fmd_reset, fmd_set_config ...): fmd_outputs_epoch
    int device = 0;
    int bytes_cap = 0;
    std::string err;
    std::map<int, std::vector<float>> lpf_cache;  // cut-off Hz -> 128 taps
    std::map<int, int> img_slot;                  // FMD_FLAG_FAST_MATH: cut-off Hz -> slot of its operand image in aud_img (k_extract_bp)
    size_t img_capacity = 0;                      // slots allocated in aud_img
    std::vector<ProfiledBlock*> marks;       // one per profiled block, drained by fmd_profile_read
};

namespace {

// The pipeline keeps six streams busy beside the caller's; ROCm maps streams onto GPU_MAX_HW_QUEUES hardware queues (default
// 4) and dependent stages sharing a queue block each other.  The library does not touch the process environment (the host
// application owns it); fmd_create warns once on stderr (and in fmd_last_error(NULL)) when the streams have
// to share queues.  FMD_QUIET=1 silences the warning.
void warn_hw_queues_once() {
    static bool done = false;
    if (done) return;
    done = true;
    const char* v = getenv("GPU_MAX_HW_QUEUES");
    const int n = v ? atoi(v) : 4;
    if (n >= 7) return;
    const char* q = getenv("FMD_QUIET");
    if (q && *q && *q != '0') return;
    fprintf(stderr, "libfmdemod: GPU_MAX_HW_QUEUES=%s: the pipelined demodulator uses up to 7 streams and loses part of its overlap on fewer "
                    "hardware queues (see INTEGRATION.md)\n", v ? v : "(unset, default 4)");
}

thread_local std::string g_create_error;

int fail(fmd_handle h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

#define HIP_TRY(h, expr)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return fail((h), FMD_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

template <typename T>
int dev_alloc(fmd_handle h, T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    HIP_TRY(h, hipMalloc(&q, bytes));
    // on the handle's own stream: a null-stream hipMemset is not ordered against the (non-blocking) own_stream, and
    // could land after the k_reset / control uploads that follow
    HIP_TRY(h, hipMemsetAsync(q, 0, bytes, h->own_stream));
    h->allocs.push_back(q);
    *p = static_cast<T*>(q);
    return FMD_OK;
}

constexpr unsigned kKnownFlags = FMD_FLAG_KEEP_TAPS | FMD_FLAG_NO_PIPELINE | FMD_FLAG_PLL_TIME_PARALLEL | FMD_FLAG_PLL_LOW_WORK | FMD_FLAG_PLL_K8 |
                                 FMD_FLAG_PLL_STREAM_ORDER | FMD_FLAG_FAST_MATH | FMD_FLAG_RDS_DECODE;

bool config_ok(const fmd_config* c, int* m) {
    if (!c || c->n_channels <= 0) return false;
    if (c->flags & ~kKnownFlags) return false;        // a flag this build does not implement must not be silently ignored
    if (c->fs_baseband != 256000 && c->fs_baseband != 1024000 && c->fs_baseband != 2048000) return false;
    *m = c->fs_baseband / 256000;
    if (c->block_size <= 0 || (c->block_size % (1024 * *m)) != 0) return false;
    return true;
}

// the block's lengths along the pipeline (m from config_ok)
Dims dims_of(const fmd_config& c, int m) {
    Dims d{};
    d.C = c.n_channels; d.N = c.block_size; d.m = m;
    d.n_fm_in = d.N / m; d.n_fm_out = d.n_fm_in / 2; d.n_rds = d.n_fm_out / 8; d.n_audio = d.n_fm_out / 4;
    d.n_est = (d.n_audio + 9) / 10;
    d.tail_base = front_tail_len(m, (c.flags & FMD_FLAG_FAST_MATH) != 0);
    return d;
}

const std::vector<float>& lpf_taps(fmd_handle h, int hz) {
    auto it = h->lpf_cache.find(hz);
    if (it != h->lpf_cache.end()) return it->second;
    fmd_controls c;
    fmd_default_controls(&c);
    c.lpr_cutoff_hz = hz;
    fmd_coeffs k{};
    design_controls(&k, &c);
    return h->lpf_cache.emplace(hz, std::vector<float>(k.b_lpr, k.b_lpr + 128)).first->second;
}

// reference UpdateFilters() (broadcast_fm_demod.cpp:330-389), for every channel whose controls changed
int upload_controls(fmd_handle h, hipStream_t s) {
    const int C = h->cfg.n_channels;
    std::vector<float> lpr((size_t)C * 128), lmr((size_t)C * 128), de((size_t)C * 4), mix((size_t)C * 2);
    int any = 0;
    bool slow_pole = false;   // a de-emphasis time constant beyond what k_front's in-tile form covers (fmd_kernels.hip kDeemphWarmup)
    for (int c = 0; c < C; c++) {
        const fmd_controls& k = h->controls[c];
        const auto& a = lpf_taps(h, k.lpr_cutoff_hz);
        const auto& b = lpf_taps(h, k.lmr_cutoff_hz);
        std::copy(a.begin(), a.end(), lpr.begin() + (size_t)c * 128);
        std::copy(b.begin(), b.end(), lmr.begin() + (size_t)c * 128);
        fmd_coeffs kk{};
        design_controls(&kk, &k);  // cheap: two cached-size designs would be overkill to cache for the 1-pole
        de[4 * c + 0] = kk.deemph_b[0]; de[4 * c + 1] = kk.deemph_b[1]; de[4 * c + 2] = kk.deemph_a[0];
        de[4 * c + 3] = k.use_deemphasis ? 1.0f : 0.0f;
        any |= k.use_deemphasis ? 1 : 0;
        if (k.use_deemphasis && !(kk.deemph_a[0] >= 0.0f && kk.deemph_a[0] <= 0.905f)) slow_pole = true;
        mix[2 * c] = (float)k.audio_out; mix[2 * c + 1] = k.audio_stereo_mix_factor;
    }
    Buffers& b = h->ctx.b;
    if (h->ctx.fast) {
        // k_extract_bp: one set of tap tables per distinct audio cut-off, and which two each station uses
        std::vector<int> idx((size_t)C * 2);
        bool grew = false;
        for (int c = 0; c < C; c++)
            for (int which = 0; which < 2; which++) {
                const int hz = which ? h->controls[c].lmr_cutoff_hz : h->controls[c].lpr_cutoff_hz;
                auto it = h->img_slot.find(hz);
                if (it == h->img_slot.end()) { it = h->img_slot.emplace(hz, (int)h->img_slot.size()).first; grew = true; }
                idx[(size_t)c * 2 + which] = it->second;
            }
        if (grew) {
            const size_t n_slots = h->img_slot.size();
            if (n_slots > h->img_capacity) {   // (everything is idle here: upload_controls runs behind sync_all)
                const size_t cap = std::max<size_t>(2 * n_slots, 8);
                uint4* q4 = nullptr;
                int rc = dev_alloc(h, &q4, cap * kBpTabSlotU16 * 2 / sizeof(uint4));
                if (rc) return rc;
                b.bp_tab = q4;       // the old table stays on the handle's allocation list until fmd_destroy
                uint4* q3 = nullptr;
                rc = dev_alloc(h, &q3, cap * kBpEdgeHalves * 2 / sizeof(uint4));
                if (rc) return rc;
                b.bp_edge = q3;
                h->img_capacity = cap;
            }
            // per cut-off the tap tables of the L+R FIR and of the L-R composite (mixer + Hilbert FIR folded into the taps)
            std::vector<uint16_t> tabsv(n_slots * kBpTabSlotU16);
            for (const auto& kv : h->img_slot) bp_slot_tap_tables(lpf_taps(h, kv.first).data(), h->base.b_hilbert, tabsv.data() + (size_t)kv.second * kBpTabSlotU16);
            HIP_TRY(h, hipMemcpyAsync(b.bp_tab, tabsv.data(), tabsv.size() * 2, hipMemcpyHostToDevice, s));
            std::vector<uint16_t> edges(n_slots * kBpEdgeHalves);
            for (const auto& kv : h->img_slot) bp_edge_matrix(lpf_taps(h, kv.first).data(), h->base.b_hilbert, edges.data() + (size_t)kv.second * kBpEdgeHalves);
            HIP_TRY(h, hipMemcpyAsync(b.bp_edge, edges.data(), edges.size() * 2, hipMemcpyHostToDevice, s));
            HIP_TRY(h, hipStreamSynchronize(s));
        }
        HIP_TRY(h, hipMemcpyAsync(b.aud_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        h->ctx.facts.uniform_cutoffs = true;
        for (int c = 1; c < C; c++) if (idx[(size_t)c * 2] != idx[0] || idx[(size_t)c * 2 + 1] != idx[1]) { h->ctx.facts.uniform_cutoffs = false; break; }
    }
    HIP_TRY(h, hipMemcpyAsync(b.b_lpr, lpr.data(), lpr.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.b_lmr, lmr.data(), lmr.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.deemph, de.data(), de.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.mix, mix.data(), mix.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipStreamSynchronize(s));  // the host vectors die here
    // FMD_FLAG_FAST_MATH: the IIR runs inside k_front's tile (no state, no extra stage) unless a channel's time constant is too long
    // for its warm-up.  The in-tile form leaves each block's last sample where the serial stage keeps its state (k_front_mfma), so a
    // handle that falls back to the serial stage continues the filter; the in-tile form itself has no state (zero, 128 samples early), so
    // where the reference's IIR resumes from a frozen state, or from another time constant's, the two differ for about a millisecond
    PlanFacts& f = h->ctx.facts;
    f.deemph_in_tile = h->ctx.fast && any && !slow_pole;
    if (f.deemph_in_tile) { f.any_deemph = false; h->deemph_linger = false; h->deemph_on = false; }
    else {
        if (any) { f.any_deemph = true; h->deemph_linger = false; }
        else if (h->deemph_on) { f.any_deemph = true; h->deemph_linger = true; }
        else if (!h->deemph_linger) f.any_deemph = false;
        h->deemph_on = any != 0;
    }
    h->controls_dirty = false;
    refresh_block_plan(h->ctx);
    return FMD_OK;
}

void fill_ctx_coeffs(fmd_handle h) {
    const fmd_coeffs& k = h->base;
    LaunchCtx& x = h->ctx;
    std::memcpy(x.front.b_fm_in, k.b_fm_in, sizeof(k.b_fm_in));
    std::memcpy(x.front.b_fm_out, k.b_fm_out, sizeof(k.b_fm_out));
    for (int i = 0; i < 32; i++) x.front.b_hilbert_odd[i] = k.b_hilbert[2 * i + 1];
    x.front.fm_gain = k.fm_gain;
    std::memcpy(x.rds_taps.b, k.b_rds, sizeof(k.b_rds));
    x.loops.pilot_k = k.pilot_b[0]; x.loops.pilot_a0 = k.pilot_a[0]; x.loops.pilot_a1 = k.pilot_a[1];
    x.loops.pll_b0 = k.pll_lpf_b[0]; x.loops.pll_b1 = k.pll_lpf_b[1]; x.loops.pll_a0 = k.pll_lpf_a[0];
    x.loops.ted_b0 = k.ted_lpf_b[0]; x.loops.ted_b1 = k.ted_lpf_b[1]; x.loops.ted_a0 = k.ted_lpf_a[0];
    x.loops.bpsk_b0 = k.bpsk_lpf_b[0]; x.loops.bpsk_b1 = k.bpsk_lpf_b[1]; x.loops.bpsk_a0 = k.bpsk_lpf_a[0];
}

// every channel's RDS decoder (k_rds_decode) as a freshly constructed RDS_Decoding_Chain; synchronises `s`
hipError_t rds_dec_upload_initial(void* state, int C, hipStream_t s) {
    std::vector<uint8_t> img(rds_dec_state_bytes(C));
    const RdsDecBufs hs = rds_dec_bufs(img.data(), C);
    for (int c = 0; c < C; c++) {
        uint32_t f[RDS_F_NUM];
        rds_dec_initial(f, hs.group + c, hs.db + c);
        for (int i = 0; i < RDS_F_NUM; i++) hs.f[(size_t)i * C + c] = f[i];
    }
    hipError_t e = hipMemcpyAsync(state, img.data(), img.size(), hipMemcpyHostToDevice, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
}

// RDS_Database::Reset() (reference rds_database.h:58-79) of one channel or all (-1), the decoder idle: the database's fields only (the
// synchroniser's status behind them and the handler's A/B memories stay)
hipError_t rds_dec_reset_db(fmd_rds_db* d_db, int C, int channel) {
    const int c0 = channel < 0 ? 0 : channel, n = channel < 0 ? C : 1;
    std::vector<fmd_rds_db> v((size_t)n);
    hipError_t e = hipMemcpy(v.data(), d_db + c0, sizeof(fmd_rds_db) * (size_t)n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (fmd_rds_db& r : v) {
        fmd_rds_db z{};
        z.in_sync = r.in_sync; z.groups = r.groups; z.sync_acquisitions = r.sync_acquisitions;
        r = z;
    }
    return hipMemcpy(d_db + c0, v.data(), sizeof(fmd_rds_db) * (size_t)n, hipMemcpyHostToDevice);
}

int zero_history(fmd_handle h, hipStream_t s) {
    const Dims& d = h->ctx.d;
    Buffers& b = h->ctx.b;
    for (int p = 0; p < 2; p++) {
        HIP_TRY(h, hipMemsetAsync(b.base_tail[p], 0, sizeof(float2) * (size_t)d.C * d.tail_base, s));
        if (b.pre_tail[p]) HIP_TRY(h, hipMemsetAsync(b.pre_tail[p], 0, sizeof(float2) * (size_t)d.C * 64, s));
        HIP_TRY(h, hipMemsetAsync(b.iq_tail[p], 0, sizeof(float2) * (size_t)d.C * 128, s));
        HIP_TRY(h, hipMemsetAsync(b.dt_tail[p], 0, sizeof(float) * (size_t)d.C * 128, s));
        HIP_TRY(h, hipMemsetAsync(b.fo_tail[p], 0, sizeof(float) * (size_t)d.C * 64, s));
        HIP_TRY(h, hipMemsetAsync(b.lmr_est[p], 0, sizeof(float) * (size_t)d.C * d.n_est, s));
        if (b.pv_hist[p]) HIP_TRY(h, hipMemsetAsync(b.pv_hist[p], 0, sizeof(float4) * (size_t)d.C * 4, s));
    }
    for (int p = 0; p < kSlots; p++) {
        if (b.fo_pl[p]) {   // the history in front of the planes' rows (and the rows themselves)
            HIP_TRY(h, hipMemsetAsync(b.fo_pl[p], 0, sizeof(float) * (size_t)d.C * ((size_t)kFoPad + d.n_fm_out), s));
            HIP_TRY(h, hipMemsetAsync(b.pll_poly[p], 0, sizeof(float4) * (size_t)d.C * ((size_t)1 + d.n_fm_out / kSpan), s));
        }
        HIP_TRY(h, hipMemsetAsync(b.rds_count[p], 0, sizeof(int) * (size_t)d.C, s));
        HIP_TRY(h, hipMemsetAsync(b.rds_bytes_count[p], 0, sizeof(int) * (size_t)d.C, s));
        if (b.rds_groups_count[p]) HIP_TRY(h, hipMemsetAsync(b.rds_groups_count[p], 0, sizeof(int) * (size_t)d.C, s));
    }
    if (h->ctx.rds_decode) HIP_TRY(h, rds_dec_upload_initial(h->ctx.rds_dec.f, d.C, s));
    HIP_TRY(h, launch_reset_state(h->ctx, s));
    // everything is idle here (callers synchronise first): restart the per-wavefront PLL hand-over chain, watchdog flag included
    if (b.pll_chain) HIP_TRY(h, hipMemsetAsync(b.pll_chain, 0, sizeof(unsigned) * ((size_t)h->ctx.plan.pll_waves + 1 + (size_t)d.C + 2), s));      // (and the body hints behind it)
    if (h->pll_unl_host) h->pll_unl_host[0] = h->pll_unl_host[1] = 0u;
    h->ctx.pll_unlocked_now = false; h->ctx.pll_launch_no = 0;
    h->sched.reset();
    h->epoch++;
    h->poisoned = false;
    return FMD_OK;
}

// The schedule's names as this handle's streams and events, and its four calls as the HIP runtime's.  caller: the stream the entry point was given
// (Q_CALLER); d_iq / u8: the block the front end or the first decimator reads.
struct HipBackend final : ScheduleBackend {
    fmd_handle h;
    hipStream_t caller;
    const void* d_iq;
    bool u8;
    explicit HipBackend(fmd_handle h_, hipStream_t caller_ = nullptr, const void* d_iq_ = nullptr, bool u8_ = false) : h(h_), caller(caller_), d_iq(d_iq_), u8(u8_) {}
    hipStream_t stream(Queue q) const {
        switch (q) {
            case Q_OWN: return h->own_stream;
            case Q_F: return h->sF;
            case Q_D: return h->sD;
            case Q_A: return h->sA;
            case Q_B: return h->sB;
            case Q_X: return h->sX;
            case Q_R: return h->sR;
            default: return caller;
        }
    }
    hipEvent_t event(Event e) const {
        switch (e.kind) {
            case EV_IN: return h->ev_in;
            case EV_P: return h->ev_P[e.slot];
            case EV_F: return h->ev_F[e.slot];
            case EV_D: return h->ev_D[e.slot];
            case EV_A: return h->ev_A[e.slot];
            case EV_B: return h->ev_B[e.slot];
            case EV_E: return h->ev_E[e.slot];
            case EV_X: return h->ev_X[e.slot];
            case EV_C: return h->ev_C[e.slot];
            case EV_T0: return h->marks[(size_t)e.slot]->t0[e.stage];
            case EV_T1: h->marks[(size_t)e.slot]->used[e.stage] = true; return h->marks[(size_t)e.slot]->t1[e.stage];   // (a stop event is only ever looked up for a stage that is being timed)
            default: return nullptr;
        }
    }
    SlotRef ref(const Launch& l) const { return SlotRef{l.buf, l.par, event(l.t0), event(l.t1), event(l.done), l.seq, l.warm}; }
    int wait(Queue q, Event e) override { return (int)hipStreamWaitEvent(stream(q), event(e), 0); }
    int record(Event e, Queue q) override { return (int)hipEventRecord(event(e), stream(q)); }
    int launch(Stage st, Queue q, const Launch& l, const Launch* ride) override {
        const SlotRef r = ref(l);
        hipStream_t s = stream(q);
        switch (st) {
            case ST_PREDECIM: return (int)launch_stage_predecim(h->ctx, r, d_iq, u8, s);
            case ST_FRONT: {
                const SlotRef rider = ride ? ref(*ride) : SlotRef{};
                return (int)launch_stage_front(h->ctx, r, d_iq, u8, s, ride ? &rider : nullptr);
            }
            case ST_DEEMPH: return (int)launch_stage_deemph(h->ctx, r, s);
            case ST_POWER: return (int)launch_stage_power(h->ctx, r, s);
            case ST_PLL: return (int)launch_stage_pll(h->ctx, r, s);
            case ST_EXTRACT: return (int)launch_stage_extract(h->ctx, r, s);
            case ST_RDS: return (int)launch_stage_rds(h->ctx, r, s);
            default: return (int)hipErrorInvalidValue;
        }
    }
    int copy_pll_hint(Queue q) override {
        return (int)hipMemcpyAsync(h->pll_unl_host, h->ctx.b.pll_hint + h->ctx.d.C, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, stream(q));
    }
};

// what a call into the schedule returned: a runtime error leaves stages half queued
int sched_rc(fmd_handle h, int e) {
    if (!e) return FMD_OK;
    h->poisoned = true;
    return fail(h, FMD_ERR_DEVICE, "%s: %s", h->sched.failed_what(), hipGetErrorString((hipError_t)e));
}

// A caller is about to use the device views of the newest outputs (fmd_wait_outputs, fmd_release_outputs, the *_dev getters): Schedule::outputs_wanted
int outputs_wanted(fmd_handle h) {
    if (!h->sched.outputs_put_off()) return FMD_OK;
    HIP_TRY(h, hipSetDevice(h->device));        // (the *_dev getters reach this without one: launches follow)
    HipBackend be(h);
    return sched_rc(h, h->sched.outputs_wanted(be));
}

int sync_all(fmd_handle h) {
    HIP_TRY(h, hipSetDevice(h->device));
    { HipBackend be(h); int rc = sched_rc(h, h->sched.flush(true, be)); if (rc) return rc; }    // (everything drains: the front end's queue is as good as any)
    for (hipStream_t st : {h->sF, h->sD, h->sA, h->sB, h->sX, h->sR, h->own_stream}) if (st) HIP_TRY(h, hipStreamSynchronize(st));
    h->sched.drained();
    if (!h->pipelined && h->sched.n_blocks() > 0) HIP_TRY(h, hipStreamSynchronize(h->last_stream));
    if (h->ctx.plan.pll_chained && h->sched.pll_seq()) {   // the hand-over watchdog of k_pilot_pll
        unsigned timed_out = 0;
        HIP_TRY(h, hipMemcpy(&timed_out, h->ctx.b.pll_chain + h->ctx.plan.pll_waves, sizeof(unsigned), hipMemcpyDeviceToHost));
        if (timed_out) {
            // reported once; the flag is cleared so that later calls do not fail for good, and the handle asks for a reset
            (void)hipMemset(h->ctx.b.pll_chain + h->ctx.plan.pll_waves, 0, sizeof(unsigned));
            h->poisoned = true;
            return fail(h, FMD_ERR_DEVICE, "k_pilot_pll: a wavefront's predecessor never published its state (call fmd_reset)");
        }
    }
    return FMD_OK;
}

// ordered: fmd_process_*_dev (the caller's stream is ordered behind the library's read of the block); otherwise fmd_submit_*_dev
// (`stream` only says when the input is ready, NULL = now; nothing is queued on it)
template <typename InT>
int process_dev(fmd_handle h, const InT* d_iq, int n_channels, int n_samples, void* stream, bool ordered = true) {
    if (!h) return FMD_ERR_ARG;
    if (!d_iq) return fail(h, FMD_ERR_ARG, "null input pointer");
    if (n_channels != h->cfg.n_channels || n_samples != h->cfg.block_size)
        return fail(h, FMD_ERR_SIZE, "block dropped: got %d x %d, handle is %d x %d", n_channels, n_samples, h->cfg.n_channels, h->cfg.block_size);
    if (h->poisoned) return fail(h, FMD_ERR_STATE, "an earlier block failed part-way: call fmd_reset");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->controls_dirty) {
        int rc = sync_all(h);          // control tables are read by in-flight stages: drain before rewriting them
        if (!rc) rc = upload_controls(h, h->own_stream);
        if (rc) return rc;
    }
    BlockFacts f;
    f.ordered = ordered; f.have_stream = s != nullptr;
    f.any_deemph = h->ctx.facts.any_deemph; f.deemph_in_tile = h->ctx.facts.deemph_in_tile; f.split_front = h->ctx.facts.split_front;
    if (h->sched.profiling()) {
        ProfiledBlock* pm = new ProfiledBlock();
        for (int i = 0; i < ST_COUNT; i++) { pm->used[i] = false; HIP_TRY(h, hipEventCreate(&pm->t0[i])); HIP_TRY(h, hipEventCreate(&pm->t1[i])); }
        h->marks.push_back(pm);
        f.prof_block = (int)h->marks.size() - 1;
    }
    // from here on kernels are queued and host-side counters advance: a failure leaves the state between two blocks
    struct Poison { fmd_handle h; bool armed = true; ~Poison() { if (armed) h->poisoned = true; } } poison{h};
    if (h->ctx.plan.pll_k_adaptive) {      // (the copy that brings the two words back: Schedule::submit, every other block)
        const unsigned done = reinterpret_cast<volatile unsigned*>(h->pll_unl_host)[1], heavy = reinterpret_cast<volatile unsigned*>(h->pll_unl_host)[0];
        h->ctx.pll_unlocked_now = heavy != 0u && (heavy > done || done - heavy < 8u);      // (heavy > done: the launch that is still running has such wavefronts)
        h->ctx.pll_launch_no++;
    }
    HipBackend be(h, s, d_iq, sizeof(InT) == 2);
    { int rc = sched_rc(h, h->sched.submit(f, be)); if (rc) return rc; }
    if (h->deemph_linger) { h->deemph_linger = false; h->ctx.facts.any_deemph = false; refresh_block_plan(h->ctx); }      // (launches only read the plan while they are queued)
    h->last_stream = s;
    poison.armed = false;
    return FMD_OK;
}

template <typename InT>
int process_host(fmd_handle h, const InT* iq, int n_channels, int n_samples) {
    if (!h) return FMD_ERR_ARG;
    if (!iq) return fail(h, FMD_ERR_ARG, "null input pointer");
    if (n_channels != h->cfg.n_channels || n_samples != h->cfg.block_size)
        return fail(h, FMD_ERR_SIZE, "block dropped: got %d x %d, handle is %d x %d", n_channels, n_samples, h->cfg.n_channels, h->cfg.block_size);
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t bytes = sizeof(InT) * (size_t)n_channels * n_samples;
    if (h->d_in_bytes < bytes) {
        if (h->d_in) HIP_TRY(h, hipFree(h->d_in));
        h->d_in = nullptr; h->d_in_bytes = 0;
        HIP_TRY(h, hipMalloc(&h->d_in, bytes));
        h->d_in_bytes = bytes;
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_in, iq, bytes, hipMemcpyHostToDevice, h->own_stream));
    int rc = process_dev<InT>(h, static_cast<const InT*>(h->d_in), n_channels, n_samples, h->own_stream);
    if (rc) return rc;
    return sync_all(h);
}

void free_marks(fmd_handle h) {
    for (ProfiledBlock* pm : h->marks) {
        for (int i = 0; i < ST_COUNT; i++) { (void)hipEventDestroy(pm->t0[i]); (void)hipEventDestroy(pm->t1[i]); }
        delete pm;
    }
    h->marks.clear();
}

}  // namespace

extern "C" {

int fmd_api_version(void) { return FMD_API_VERSION; }
int fmd_output_lifetime_blocks(void) { static_assert(FMD_OUTPUT_LIFETIME_BLOCKS == kSlots - 1, "one contract"); return kSlots - 1; }

const char* fmd_status_string(int s) {
    switch (s) {
        case FMD_OK: return "ok";
        case FMD_ERR_ARG: return "bad argument";
        case FMD_ERR_SIZE: return "block size mismatch (block dropped)";
        case FMD_ERR_DEVICE: return "HIP runtime error";
        case FMD_ERR_NO_DEVICE: return "no gfx950 device (no CPU fallback)";
        case FMD_ERR_NAME: return "unknown stream name";
        case FMD_ERR_STATE: return "a block failed part-way: call fmd_reset";
        default: return "unknown status";
    }
}

int fmd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ok++;
    }
    return ok;
}

int fmd_default_config(fmd_config* cfg, int n_channels, int fs_baseband) {
    if (!cfg || n_channels <= 0 || (fs_baseband != 256000 && fs_baseband != 1024000 && fs_baseband != 2048000)) return FMD_ERR_ARG;
    cfg->n_channels = n_channels;
    cfg->block_size = 16384 * (fs_baseband / 256000);     // 64 ms: the reference's 65536 samples at 1.024 MSa/s
    cfg->fs_baseband = fs_baseband;
    cfg->device = -1;
    cfg->flags = FMD_FLAG_FAST_MATH;
    return FMD_OK;
}

int fmd_create(const fmd_config* cfg, fmd_handle* out) {
    if (!out) return FMD_ERR_ARG;
    *out = nullptr;
    int m = 0;
    if (!config_ok(cfg, &m)) return fail(nullptr, FMD_ERR_ARG, "unsupported configuration");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, FMD_ERR_NO_DEVICE, "no HIP device");
    int dev = cfg->device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) return fail(nullptr, FMD_ERR_NO_DEVICE, "hipGetDevice failed"); }
    if (dev >= ndev) return fail(nullptr, FMD_ERR_ARG, "device %d out of range", dev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, FMD_ERR_NO_DEVICE, "device %d is not gfx950", dev);

    fmd_handle h = new (std::nothrow) fmd_handle_s();
    if (!h) return FMD_ERR_ARG;
    h->cfg = *cfg;
    h->cfg.device = dev;
    h->device = dev;
    auto bail = [&](int rc) { g_create_error = h->err; fmd_destroy(h); return rc; };
    if (hipSetDevice(dev) != hipSuccess) return bail(fail(h, FMD_ERR_DEVICE, "hipSetDevice failed"));
    { hipError_t e = prepare_kernels(); if (e != hipSuccess) return bail(fail(h, FMD_ERR_DEVICE, "prepare_kernels: %s", hipGetErrorString(e))); }
    // (A CU-mask split between the serial and the FIR streams was measured: it shields the PLL wave from FIR waves
    //  sharing its SIMD — 3.06 -> 2.75 ms — but CU-masked streams did not overlap with each other on this runtime, so
    //  the step got slower overall.  Plain streams + s_setprio in the serial kernels it is.)
    // (the second PLL stream is own_stream: one more stream would be the ninth on the device with the caller's and would share a
    //  hardware queue with another stage; everything else own_stream does is preceded by a full synchronisation)
    for (hipStream_t* st : {&h->own_stream, &h->sF, &h->sD, &h->sA, &h->sB, &h->sX, &h->sR}) {
        hipError_t e = hipStreamCreateWithFlags(st, hipStreamNonBlocking);
        if (e != hipSuccess) return bail(fail(h, FMD_ERR_DEVICE, "stream: %s", hipGetErrorString(e)));
    }

    h->pipelined = (cfg->flags & FMD_FLAG_NO_PIPELINE) == 0;
    if (h->pipelined) warn_hw_queues_once();
    {
        std::vector<hipEvent_t*> evs = {&h->ev_in};
        for (int i = 0; i < kSlots; i++) { evs.push_back(&h->ev_P[i]); evs.push_back(&h->ev_F[i]); evs.push_back(&h->ev_A[i]); evs.push_back(&h->ev_B[i]); evs.push_back(&h->ev_E[i]); evs.push_back(&h->ev_X[i]); evs.push_back(&h->ev_C[i]); evs.push_back(&h->ev_D[i]); }
        for (hipEvent_t* ev : evs) {
            hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
            if (e != hipSuccess) return bail(fail(h, FMD_ERR_DEVICE, "event: %s", hipGetErrorString(e)));
        }
    }
    h->ctx.d = dims_of(*cfg, m);
    const Dims& d = h->ctx.d;
    h->ctx.plan = make_plan(d.C, d.m, d.n_fm_out, d.n_est, cfg->flags);
    refresh_block_plan(h->ctx);
    h->ctx.pll_unlocked_now = false; h->ctx.pll_launch_no = 0;
    h->bytes_cap = 16 * (d.n_rds / 256 + 1);
    h->ctx.bytes_cap = h->bytes_cap;
    h->ctx.keep_taps = (cfg->flags & FMD_FLAG_KEEP_TAPS) ? 1 : 0;
    h->ctx.rds_decode = (cfg->flags & FMD_FLAG_RDS_DECODE) ? 1 : 0;
    h->ctx.fast = (cfg->flags & FMD_FLAG_FAST_MATH) ? 1 : 0;

    fmd_controls def;
    fmd_default_controls(&def);
    h->controls.assign((size_t)d.C, def);
    design_all(&h->base, cfg->fs_baseband, &def);
    fill_ctx_coeffs(h);

    Buffers& b = h->ctx.b;
    const size_t C = (size_t)d.C;
    int rc = FMD_OK;
    for (int p = 0; p < 2 && !rc; p++) {
        rc = dev_alloc(h, &b.base_tail[p], C * d.tail_base);
        if (!rc && m > 1) rc = dev_alloc(h, &b.pre_tail[p], C * 64);
        if (!rc) rc = dev_alloc(h, &b.iq_tail[p], C * 128);
        if (!rc) rc = dev_alloc(h, &b.dt_tail[p], C * 128);
        if (!rc) rc = dev_alloc(h, &b.fo_tail[p], C * 64);
    }
    // Tolerance mode: fm_out as a plane (rows with the previous block's tail in front) and the NCO phase as span polynomials; the interleaved / per-sample streams
    // only for FMD_FLAG_KEEP_TAPS (the getters) and for block lengths that run k_extract<128> (BlockPlan::iq_streams: no fact changes it)
    const bool fast = h->ctx.fast != 0;
    const bool streams = h->ctx.block.iq_streams;
    for (int p = 0; p < kSlots && !rc; p++) {
        if (streams) rc = dev_alloc(h, &b.fm_out_iq[p], C * d.n_fm_out);
        if (!rc && m > 1) rc = dev_alloc(h, &b.fm_in[p], C * d.n_fm_in);
        if (!rc && !fast) rc = dev_alloc(h, &b.fm_out[p], C * d.n_fm_out);
        if (!rc && !fast) rc = dev_alloc(h, &b.pilot[p], C * d.n_fm_out);   // (fast mode never materialises the pilot stream)
        if (!rc && streams) rc = dev_alloc(h, &b.pll_dt[p], C * d.n_fm_out);
        if (!rc && fast) rc = dev_alloc(h, &b.fo_pl[p], C * ((size_t)kFoPad + d.n_fm_out));
        if (!rc && fast) rc = dev_alloc(h, &b.pll_poly[p], C * ((size_t)1 + d.n_fm_out / kSpan));
        if (!rc && fast) rc = dev_alloc(h, &b.pv_pl[p], C * (size_t)(d.n_fm_out / 16));
        if (!rc && fast) rc = dev_alloc(h, &b.rds_pow[p], C * (size_t)(2 * (d.n_audio / 256) + 2));
        if (!rc) rc = dev_alloc(h, &b.audio[p], C * d.n_audio * 2);
        if (!rc) rc = dev_alloc(h, &b.rds_sym[p], C * d.n_rds);
        if (!rc) rc = dev_alloc(h, &b.rds_raw_sym[p], h->ctx.keep_taps ? C * d.n_rds : 4);
        if (!rc && !fast && h->ctx.keep_taps) rc = dev_alloc(h, &b.taps[p], tap_floats(d));
        if (!rc) rc = dev_alloc(h, &b.rds_count[p], C);
        if (!rc) rc = dev_alloc(h, &b.lpr[p], h->ctx.keep_taps ? C * d.n_audio : 4);
        if (!rc) rc = dev_alloc(h, &b.lmr[p], h->ctx.keep_taps ? C * d.n_audio : 4);
        if (!rc) rc = dev_alloc(h, &b.rds_bytes[p], C * h->bytes_cap);
        if (!rc) rc = dev_alloc(h, &b.rds_bytes_count[p], C);
        if (!rc) rc = dev_alloc(h, &b.rds[p], C * d.n_rds);
        if (!rc && h->ctx.rds_decode) rc = dev_alloc(h, &b.rds_db[p], C);
        if (!rc && h->ctx.rds_decode) rc = dev_alloc(h, &b.rds_groups[p], C * (size_t)rds_groups_cap(h->bytes_cap));
        if (!rc && h->ctx.rds_decode) rc = dev_alloc(h, &b.rds_groups_count[p], C);
    }
    if (!rc && h->ctx.rds_decode) {
        uint8_t* st = nullptr;
        rc = dev_alloc(h, &st, rds_dec_state_bytes(d.C));
        if (!rc) h->ctx.rds_dec = rds_dec_bufs(st, d.C);
    }
    for (int p = 0; p < 2 && !rc; p++) rc = dev_alloc(h, &b.lmr_est[p], C * d.n_est);
    for (int p = 0; p < 2 && !rc && fast; p++) rc = dev_alloc(h, &b.pv_hist[p], C * 4);
    if (!rc) rc = dev_alloc(h, &b.lmr_peek, C);
    if (!rc) rc = dev_alloc(h, &b.b_lpr, C * 128);
    if (!rc) rc = dev_alloc(h, &b.b_lmr, C * 128);
    if (!rc) rc = dev_alloc(h, &b.deemph, C * 4);
    if (!rc) rc = dev_alloc(h, &b.mix, C * 2);
    if (!rc) rc = dev_alloc(h, &b.state, (size_t)S_NUM_FIELDS * C);
    if (!rc) rc = dev_alloc(h, &b.spec_stats, 8);
    if (!rc && h->ctx.fast) {
        rc = dev_alloc(h, &b.pilot_tab, 1);
        if (!rc) {
            std::vector<uint16_t> img;
            design_front_mfma(h->base, m, img);
            rc = dev_alloc(h, &b.front_mfma, img.size() * 2 / sizeof(uint4));
            if (!rc && (hipMemcpyAsync(b.front_mfma, img.data(), img.size() * 2, hipMemcpyHostToDevice, h->own_stream) != hipSuccess ||
                        hipStreamSynchronize(h->own_stream) != hipSuccess)) rc = fail(h, FMD_ERR_DEVICE, "operand table upload failed");
            if (!rc) rc = dev_alloc(h, &b.aud_idx, C);
            if (!rc) rc = dev_alloc(h, &b.rds_bp_tab, kBpRdsTabU16 * 2 / sizeof(uint4));
            if (!rc) {
                std::vector<uint16_t> rt(kBpRdsTabU16);
                bp_rds_tap_tables(h->base.b_rds, h->base.b_hilbert, rt.data());
                if (hipMemcpyAsync(b.rds_bp_tab, rt.data(), rt.size() * 2, hipMemcpyHostToDevice, h->own_stream) != hipSuccess ||
                    hipStreamSynchronize(h->own_stream) != hipSuccess) rc = fail(h, FMD_ERR_DEVICE, "operand table upload failed");
            }
            if (!rc) rc = dev_alloc(h, &b.span_tab, 1);
            if (!rc) {
                PllSpanTab st_;
                design_pll_span(h->base, &st_);
                if (hipMemcpyAsync(b.span_tab, &st_, sizeof(st_), hipMemcpyHostToDevice, h->own_stream) != hipSuccess ||
                    hipStreamSynchronize(h->own_stream) != hipSuccess) rc = fail(h, FMD_ERR_DEVICE, "span table upload failed");
            }
            if (!rc) rc = dev_alloc(h, &b.sparse_tab, 1);
            if (!rc) {
                PllSparseTab sp_;
                design_pll_sparse(h->base, &sp_);
                design_wrap_tie(sp_.wrap_tie);
                if (hipMemcpyAsync(b.sparse_tab, &sp_, sizeof(sp_), hipMemcpyHostToDevice, h->own_stream) != hipSuccess ||
                    hipStreamSynchronize(h->own_stream) != hipSuccess) rc = fail(h, FMD_ERR_DEVICE, "sparse table upload failed");
            }
            PilotFastTab tab;
            design_pilot_fast(h->base, &tab);
            if (hipMemcpyAsync(b.pilot_tab, &tab, sizeof(tab), hipMemcpyHostToDevice, h->own_stream) != hipSuccess ||
                hipStreamSynchronize(h->own_stream) != hipSuccess) rc = fail(h, FMD_ERR_DEVICE, "pilot table upload failed");
        }
    }
    const int pll_waves = h->ctx.plan.pll_waves;      // per-wavefront hand-over between consecutive k_pilot_pll launches (Plan::pll_chained)
    if (!rc) rc = dev_alloc(h, &b.pll_chain, (size_t)pll_waves + 1 + (size_t)d.C + 2);
    if (!rc) b.pll_hint = b.pll_chain + pll_waves + 1;
    if (!rc && !h->ctx.fast) {
        if (hipHostMalloc(reinterpret_cast<void**>(&h->pll_unl_host), 64, hipHostMallocDefault) != hipSuccess) rc = fail(h, FMD_ERR_DEVICE, "pinned allocation failed");
        else h->pll_unl_host[0] = h->pll_unl_host[1] = 0u;
    }
    if (rc) return bail(rc);
    {
        ScheduleConfig sc;
        sc.fast = fast; sc.pipelined = h->pipelined; sc.iq_streams = streams; sc.m = d.m; sc.n_fm_out = d.n_fm_out;
        sc.warm_forever = dev_env("FMD_DEBUG_PLL_DENSE") != nullptr;   // development knob: k_pll_span for every block (A/B against round 3's pilot stage)
        if (const char* e = dev_env("FMD_DEBUG_SKIP_STAGES")) sc.debug_skip = (unsigned)strtoul(e, nullptr, 0);   // development knob
        h->sched.init(sc, &h->ctx.plan);
    }
    rc = zero_history(h, h->own_stream);
    if (!rc) rc = upload_controls(h, h->own_stream);
    if (rc) return bail(rc);
    if (hipStreamSynchronize(h->own_stream) != hipSuccess) return bail(fail(h, FMD_ERR_DEVICE, "sync failed"));
    *out = h;
    return FMD_OK;
}

int fmd_destroy(fmd_handle h) {
    if (!h) return FMD_ERR_ARG;
    (void)hipSetDevice(h->device);
    (void)sync_all(h);
    free_marks(h);
    for (hipStream_t st : {h->sF, h->sD, h->sA, h->sB, h->sX, h->sR}) if (st) (void)hipStreamDestroy(st);
    {
        std::vector<hipEvent_t> evs = {h->ev_in};
        for (int i = 0; i < kSlots; i++) { evs.push_back(h->ev_P[i]); evs.push_back(h->ev_F[i]); evs.push_back(h->ev_A[i]); evs.push_back(h->ev_B[i]); evs.push_back(h->ev_E[i]); evs.push_back(h->ev_X[i]); evs.push_back(h->ev_C[i]); evs.push_back(h->ev_D[i]); }
        for (hipEvent_t ev : evs) if (ev) (void)hipEventDestroy(ev);
    }
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->d_in) (void)hipFree(h->d_in);
    if (h->pll_unl_host) (void)hipHostFree(h->pll_unl_host);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return FMD_OK;
}

int fmd_reset(fmd_handle h) {
    if (!h) return FMD_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    { int rc0 = sync_all(h); if (rc0 && !h->poisoned) return rc0; }   // a poisoned handle is reset whatever the last error was
    int rc = zero_history(h, h->own_stream);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->own_stream));
    h->deemph_on = false; h->deemph_linger = false; h->ctx.facts.any_deemph = false;
    h->controls_dirty = true;
    return FMD_OK;
}

int fmd_set_controls(fmd_handle h, int channel, const fmd_controls* c) {
    if (!h || !c) return FMD_ERR_ARG;
    if (channel >= h->cfg.n_channels) return fail(h, FMD_ERR_ARG, "channel %d out of range", channel);
    if (c->audio_out < FMD_AUDIO_LPR || c->audio_out > FMD_AUDIO_STEREO || c->deemphasis_tus <= 0)
        return fail(h, FMD_ERR_ARG, "bad controls");
    if (channel < 0) std::fill(h->controls.begin(), h->controls.end(), *c);
    else h->controls[(size_t)channel] = *c;
    h->controls_dirty = true;
    return FMD_OK;
}

int fmd_get_controls(fmd_handle h, int channel, fmd_controls* c) {
    if (!h || !c) return FMD_ERR_ARG;
    if (channel >= h->cfg.n_channels) return fail(h, FMD_ERR_ARG, "channel %d out of range", channel);
    *c = h->controls[(size_t)std::max(channel, 0)];
    return FMD_OK;
}

int fmd_get_rates(fmd_handle h, fmd_rates* r) {
    if (!h || !r) return FMD_ERR_ARG;
    const Dims& d = h->ctx.d;
    r->fs_baseband = h->cfg.fs_baseband; r->fs_fm_in = 256000; r->fs_fm_out = 128000; r->fs_rds = 16000; r->fs_audio = 32000;
    r->n_baseband = d.N; r->n_fm_in = d.n_fm_in; r->n_fm_out = d.n_fm_out; r->n_rds = d.n_rds; r->n_audio = d.n_audio;
    return FMD_OK;
}

int fmd_get_config(fmd_handle h, fmd_config* cfg) {
    if (!h || !cfg) return FMD_ERR_ARG;
    *cfg = h->cfg;
    return FMD_OK;
}

int fmd_get_coeffs(fmd_handle h, int channel, fmd_coeffs* k) {
    if (!h || !k) return FMD_ERR_ARG;
    if (channel >= h->cfg.n_channels) return fail(h, FMD_ERR_ARG, "channel %d out of range", channel);
    *k = h->base;
    design_controls(k, &h->controls[(size_t)std::max(channel, 0)]);
    return FMD_OK;
}

int fmd_process_cf32_dev(fmd_handle h, const float* d_iq, int n_channels, int n_samples, void* stream) {
    return process_dev<float2>(h, reinterpret_cast<const float2*>(d_iq), n_channels, n_samples, stream);
}
int fmd_process_u8_dev(fmd_handle h, const uint8_t* d_iq, int n_channels, int n_samples, void* stream) {
    return process_dev<uchar2>(h, reinterpret_cast<const uchar2*>(d_iq), n_channels, n_samples, stream);
}
int fmd_submit_cf32_dev(fmd_handle h, const float* d_iq, int n_channels, int n_samples, void* ready_stream) {
    return process_dev<float2>(h, reinterpret_cast<const float2*>(d_iq), n_channels, n_samples, ready_stream, false);
}
int fmd_submit_u8_dev(fmd_handle h, const uint8_t* d_iq, int n_channels, int n_samples, void* ready_stream) {
    return process_dev<uchar2>(h, reinterpret_cast<const uchar2*>(d_iq), n_channels, n_samples, ready_stream, false);
}
int fmd_wait_input(fmd_handle h, void* stream) {
    if (!h) return FMD_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HipBackend be(h, static_cast<hipStream_t>(stream));
    return sched_rc(h, h->sched.wait_input(be));
}
int fmd_process_cf32_host(fmd_handle h, const float* iq, int n_channels, int n_samples) {
    return process_host<float2>(h, reinterpret_cast<const float2*>(iq), n_channels, n_samples);
}
int fmd_process_u8_host(fmd_handle h, const uint8_t* iq, int n_channels, int n_samples) {
    return process_host<uchar2>(h, reinterpret_cast<const uchar2*>(iq), n_channels, n_samples);
}

int fmd_set_output_lag(fmd_handle h, int on) {
    if (!h) return FMD_ERR_ARG;
    int rc = sync_all(h);
    if (rc) return rc;
    h->sched.set_output_lag(on != 0);
    return FMD_OK;
}

int fmd_outputs_block(fmd_handle h, long* block) {
    if (!h || !block) return FMD_ERR_ARG;
    int rc = outputs_wanted(h);
    if (rc) return rc;
    *block = h->sched.have_out() ? h->sched.out_block() : -1;
    return FMD_OK;
}

int fmd_outputs_epoch(fmd_handle h, long* epoch) {
    if (!h || !epoch) return FMD_ERR_ARG;
    *epoch = h->epoch;
    return FMD_OK;
}

int fmd_synchronize(fmd_handle h) {
    if (!h) return FMD_ERR_ARG;
    return sync_all(h);
}

int fmd_wait_outputs(fmd_handle h, void* stream) {
    if (!h) return FMD_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HipBackend be(h, static_cast<hipStream_t>(stream));
    return sched_rc(h, h->sched.wait_outputs(be));
}

int fmd_release_outputs(fmd_handle h, void* stream) {
    if (!h) return FMD_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HipBackend be(h, static_cast<hipStream_t>(stream));
    return sched_rc(h, h->sched.release_outputs(be));
}

int fmd_audio_dev(fmd_handle h, const float** d_audio) {
    if (!h || !d_audio) return FMD_ERR_ARG;
    { int rc = outputs_wanted(h); if (rc) return rc; }
    *d_audio = h->ctx.b.audio[h->sched.out_slot()];
    return FMD_OK;
}

int fmd_audio_pcm16_dev(fmd_handle h, int16_t* d_pcm, void* stream) {
    if (!h || !d_pcm) return FMD_ERR_ARG;
    if (h->sched.n_blocks() == 0) return fail(h, FMD_ERR_ARG, "no block has been processed");
    int rc = fmd_wait_outputs(h, stream);
    if (!rc && !h->sched.have_out()) return fail(h, FMD_ERR_ARG, "no block's outputs are queued yet (fmd_set_output_lag: from the second fmd_submit_* on)");
    if (rc) return rc;
    const Dims& d = h->ctx.d;
    hipError_t e = launch_audio_pcm16(h->ctx.b.audio[h->sched.out_slot()], d_pcm, (size_t)d.C * d.n_audio * 2, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, FMD_ERR_DEVICE, "k_audio_pcm16 launch: %s", hipGetErrorString(e));
    return FMD_OK;
}

int fmd_rds_dev(fmd_handle h, const float** d_syms, const int** d_counts) {
    if (!h || !d_syms || !d_counts) return FMD_ERR_ARG;
    { int rc = outputs_wanted(h); if (rc) return rc; }
    *d_syms = h->ctx.b.rds_sym[h->sched.out_slot()];
    *d_counts = h->ctx.b.rds_count[h->sched.out_slot()];
    return FMD_OK;
}

int fmd_get_audio(fmd_handle h, float* audio) {
    if (!h || !audio) return FMD_ERR_ARG;
    int rc = fmd_synchronize(h);
    if (rc) return rc;
    const Dims& d = h->ctx.d;
    HIP_TRY(h, hipMemcpy(audio, h->ctx.b.audio[h->sched.out_slot()], sizeof(float) * 2 * (size_t)d.C * d.n_audio, hipMemcpyDeviceToHost));
    return FMD_OK;
}

int fmd_get_rds_symbols(fmd_handle h, float* syms, int* counts) {
    if (!h || !syms || !counts) return FMD_ERR_ARG;
    int rc = fmd_synchronize(h);
    if (rc) return rc;
    const Dims& d = h->ctx.d;
    HIP_TRY(h, hipMemcpy(syms, h->ctx.b.rds_sym[h->sched.out_slot()], sizeof(float) * (size_t)d.C * d.n_rds, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(counts, h->ctx.b.rds_count[h->sched.out_slot()], sizeof(int) * (size_t)d.C, hipMemcpyDeviceToHost));
    return FMD_OK;
}

int fmd_get_rds_bytes(fmd_handle h, uint8_t* bytes, int cap_bytes_per_channel, int* counts) {
    if (!h || !bytes || !counts || cap_bytes_per_channel < 0) return FMD_ERR_ARG;
    int rc = fmd_synchronize(h);
    if (rc) return rc;
    const Dims& d = h->ctx.d;
    std::vector<uint8_t> tmp((size_t)d.C * h->bytes_cap);
    HIP_TRY(h, hipMemcpy(tmp.data(), h->ctx.b.rds_bytes[h->sched.out_slot()], tmp.size(), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(counts, h->ctx.b.rds_bytes_count[h->sched.out_slot()], sizeof(int) * (size_t)d.C, hipMemcpyDeviceToHost));
    for (int c = 0; c < d.C; c++) {
        counts[c] = std::min(counts[c], std::min(cap_bytes_per_channel, h->bytes_cap));
        std::memcpy(bytes + (size_t)c * cap_bytes_per_channel, tmp.data() + (size_t)c * h->bytes_cap, (size_t)counts[c]);
    }
    return FMD_OK;
}

int fmd_rds_bytes_dev(fmd_handle h, const uint8_t** d_bytes, const int** d_counts, int* cap_bytes_per_channel) {
    if (!h || !d_bytes || !d_counts || !cap_bytes_per_channel) return FMD_ERR_ARG;
    { int rc = outputs_wanted(h); if (rc) return rc; }
    *d_bytes = h->ctx.b.rds_bytes[h->sched.out_slot()];
    *d_counts = h->ctx.b.rds_bytes_count[h->sched.out_slot()];
    *cap_bytes_per_channel = h->bytes_cap;
    return FMD_OK;
}

int fmd_get_rds_db(fmd_handle h, fmd_rds_db* db) {
    if (!h || !db || !h->ctx.rds_decode) return FMD_ERR_ARG;
    int rc = fmd_synchronize(h);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpy(db, h->ctx.b.rds_db[h->sched.out_slot()], sizeof(fmd_rds_db) * (size_t)h->ctx.d.C, hipMemcpyDeviceToHost));
    return FMD_OK;
}

int fmd_rds_db_dev(fmd_handle h, const fmd_rds_db** d_db) {
    if (!h || !d_db || !h->ctx.rds_decode) return FMD_ERR_ARG;
    { int rc = outputs_wanted(h); if (rc) return rc; }
    *d_db = h->ctx.b.rds_db[h->sched.out_slot()];
    return FMD_OK;
}

int fmd_get_rds_groups(fmd_handle h, fmd_rds_group* groups, int cap_groups_per_channel, int* counts) {
    if (!h || !groups || !counts || cap_groups_per_channel < 0 || !h->ctx.rds_decode) return FMD_ERR_ARG;
    int rc = fmd_synchronize(h);
    if (rc) return rc;
    const int C = h->ctx.d.C, gcap = rds_groups_cap(h->bytes_cap);
    std::vector<fmd_rds_group> tmp((size_t)C * gcap);
    HIP_TRY(h, hipMemcpy(tmp.data(), h->ctx.b.rds_groups[h->sched.out_slot()], sizeof(fmd_rds_group) * tmp.size(), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(counts, h->ctx.b.rds_groups_count[h->sched.out_slot()], sizeof(int) * (size_t)C, hipMemcpyDeviceToHost));
    for (int c = 0; c < C; c++) {
        const int n = std::min(counts[c], std::min(cap_groups_per_channel, gcap));
        std::memcpy(groups + (size_t)c * cap_groups_per_channel, tmp.data() + (size_t)c * gcap, sizeof(fmd_rds_group) * (size_t)n);
    }
    return FMD_OK;
}

int fmd_rds_groups_dev(fmd_handle h, const fmd_rds_group** d_groups, const int** d_counts, int* cap_groups_per_channel) {
    if (!h || !d_groups || !d_counts || !cap_groups_per_channel || !h->ctx.rds_decode) return FMD_ERR_ARG;
    { int rc = outputs_wanted(h); if (rc) return rc; }
    *d_groups = h->ctx.b.rds_groups[h->sched.out_slot()];
    *d_counts = h->ctx.b.rds_groups_count[h->sched.out_slot()];
    *cap_groups_per_channel = rds_groups_cap(h->bytes_cap);
    return FMD_OK;
}

int fmd_reset_rds_db(fmd_handle h, int channel) {
    if (!h || !h->ctx.rds_decode || channel < -1 || channel >= h->cfg.n_channels) return FMD_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = sync_all(h);
    if (rc) return rc;
    HIP_TRY(h, rds_dec_reset_db(h->ctx.rds_dec.db, h->ctx.d.C, channel));
    return FMD_OK;
}

int fmd_get_stream(fmd_handle h, const char* name, float* out, size_t cap_floats, size_t* n_floats) {
    if (!h || !name) return FMD_ERR_ARG;
    const Dims& d = h->ctx.d;
    const Buffers& b = h->ctx.b;
    const size_t C = (size_t)d.C;
    const bool keep = h->ctx.keep_taps != 0;
    const int o = h->sched.out_slot();
    const void* p = nullptr;
    size_t n = 0;
    bool from_state = false, lmr_peek = false;
    int field = 0;
    const std::string s(name);
    if (s == "fm_out_iq" && b.fm_out_iq[o]) { p = b.fm_out_iq[o]; n = 2 * C * d.n_fm_out; }
    else if (s == "pll_dt" && b.pll_dt[o]) { p = b.pll_dt[o]; n = C * d.n_fm_out; }
    else if (s == "fm_out_iq" || s == "pll_dt") return fail(h, FMD_ERR_NAME, "stream '%s' needs FMD_FLAG_KEEP_TAPS in the tolerance mode (it is not materialised otherwise)", name);
    else if (s == "pll_poly" && b.pll_poly[o]) { p = b.pll_poly[o]; n = 4 * C * ((size_t)1 + d.n_fm_out / kSpan); }   // tolerance mode: [C][1 + spans][4], entry 0 = the previous block's last span
    else if (s == "audio") { p = b.audio[o]; n = 2 * C * d.n_audio; }
    else if (s == "rds_sym") { p = b.rds_sym[o]; n = C * d.n_rds; }
    else if (s == "lmr_est") { p = b.lmr_est[(h->sched.n_blocks() + 1) & 1]; n = C * d.n_est; }
    else if (s == "rds" ) { p = b.rds[o]; n = 2 * C * d.n_rds; }
    else if (s == "lpr" && keep) { p = b.lpr[o]; n = C * d.n_audio; }
    else if (s == "lmr" && keep) { p = b.lmr[o]; n = C * d.n_audio; }
    else if (s == "rds_raw_sym" && keep) { p = b.rds_raw_sym[o]; n = 2 * C * d.n_rds; }
    else if (s == "pilot" || s == "pll" || s == "pll_raw_err" || s == "pll_pi_err" || s.rfind("bpsk_", 0) == 0) {
        // reference GetPilotOutput / GetPLLOutput / Get_PLL_Raw_Phase_Error_Output / Get_PLL_LPF_Phase_Error_Output (broadcast_fm_demod.h:245-248),
        // BPSK_Synchroniser::Get* (bpsk_synchroniser.h:78-85): per-sample traces of the two loops, kept by the exact mode's kernels on request
        const TapPtrs t = tap_ptrs(h->ctx, o);
        if (!t.pilot) return fail(h, FMD_ERR_NAME, "stream '%s' needs FMD_FLAG_KEEP_TAPS in the exact mode (the tolerance mode's loops run at eight points per span / on "
                                                   "groups of four samples: they have no per-sample trace)", name);
        const size_t nf = C * d.n_fm_out, nr = C * d.n_rds;
        if (s == "pilot") { p = t.pilot; n = 2 * nf; }
        else if (s == "pll") { p = t.pll; n = 2 * nf; }
        else if (s == "pll_raw_err") { p = t.pll_raw; n = nf; }
        else if (s == "pll_pi_err") { p = t.pll_pi; n = nf; }
        else if (s == "bpsk_pll_sym") { p = t.b_pll_sym; n = 2 * nr; }
        else if (s == "bpsk_intdump") { p = t.b_intdump; n = 2 * nr; }
        else if (s == "bpsk_ted_raw") { p = t.b_ted_raw; n = nr; }
        else if (s == "bpsk_ted_pi") { p = t.b_ted_pi; n = nr; }
        else if (s == "bpsk_pll_raw") { p = t.b_pll_raw; n = nr; }
        else if (s == "bpsk_pll_pi") { p = t.b_pll_pi; n = nr; }
        else if (s == "bpsk_zcd") { p = t.b_zcd; n = nr; }
        else if (s == "bpsk_trig") { p = t.b_trig; n = nr; }
        else return fail(h, FMD_ERR_NAME, "unknown stream '%s'", name);
    }
    else if (s == "lmr_phase") { lmr_peek = true; p = b.lmr_peek; n = C; }
    else if (s == "agc_pilot_gain") { from_state = true; field = S_AGC_PILOT_GAIN; }
    else if (s == "agc_rds_gain") { from_state = true; field = S_AGC_RDS_GAIN; }
    else if (s == "lpr" || s == "lmr" || s == "rds_raw_sym") return fail(h, FMD_ERR_NAME, "stream '%s' needs FMD_FLAG_KEEP_TAPS", name);
    else return fail(h, FMD_ERR_NAME, "unknown stream '%s'", name);
    if (from_state) { p = b.state + (size_t)field * C; n = C; }
    if (n_floats) *n_floats = n;
    if (!out || cap_floats < n) return fail(h, FMD_ERR_ARG, "stream '%s' needs %zu floats", name, n);  // size query: out may be NULL
    int rc = fmd_synchronize(h);
    if (rc) return rc;
    if (lmr_peek) {   // reference GetAudioLMRPhaseError(): the offset after the newest block's update (the next block's k_extract computes it for itself)
        HIP_TRY(h, launch_lmr_phase_peek(h->ctx, (int)((h->sched.n_blocks() + 1) & 1), b.lmr_peek, h->own_stream));
        HIP_TRY(h, hipStreamSynchronize(h->own_stream));
    }
    HIP_TRY(h, hipMemcpy(out, p, sizeof(float) * n, hipMemcpyDeviceToHost));
    return FMD_OK;
}

// ---- per-channel state snapshot (include/fmdemod.h: fmd_state_size / fmd_get_state / fmd_set_state) ----
extern "C++" {
namespace {
struct StateHeader { uint32_t magic, version; int32_t fs_baseband, m, n_fields, tail_base; uint32_t reserved[2]; };
constexpr uint32_t kStateMagic = 0x53444d46u;   // "FMDS"
struct StatePart { float* base; size_t floats; size_t stride; };   // the channel's `floats` floats at base + channel * stride

// the histories the NEXT block reads (parity / slot of block number n_blocks)
std::vector<StatePart> state_parts(fmd_handle h) {
    const Dims& d = h->ctx.d;
    Buffers& b = h->ctx.b;
    const int par = (int)(h->sched.n_blocks() & 1), slot = (int)(h->sched.n_blocks() % kSlots);
    std::vector<StatePart> v;
    auto by_par = [&](void* const* base, size_t floats, int flip) { v.push_back({static_cast<float*>(base[par ^ flip]), floats, floats}); };
    { void* p[2] = {b.base_tail[0], b.base_tail[1]}; by_par(p, (size_t)d.tail_base * 2, 0); }
    if (d.m > 1) { void* p[2] = {b.pre_tail[0], b.pre_tail[1]}; by_par(p, 64 * 2, 0); }
    if (b.fm_out_iq[0]) {   // the interleaved streams' consumers keep their own tails (exact mode; tolerance mode with k_extract<128>)
        { void* p[2] = {b.iq_tail[0], b.iq_tail[1]}; by_par(p, 128 * 2, 0); }
        { void* p[2] = {b.dt_tail[0], b.dt_tail[1]}; by_par(p, 128, 0); }
    }
    { void* p[2] = {b.fo_tail[0], b.fo_tail[1]}; by_par(p, 64, 0); }
    { void* p[2] = {b.lmr_est[0], b.lmr_est[1]}; by_par(p, (size_t)d.n_est, 1); }   // the newest block's L-R phase estimates (the next k_extract integrates them)
    if (b.pv_hist[0]) { void* p[2] = {b.pv_hist[0], b.pv_hist[1]}; by_par(p, 16, 0); }   // tolerance mode: the last four columns' pilot sums (k_pll_sparse)
    if (b.fo_pl[0]) {       // tolerance mode: the previous block's tails in front of the next slot's rows (k_pll_span)
        v.push_back({b.fo_pl[slot], (size_t)kFoPad, (size_t)kFoPad + d.n_fm_out});
        v.push_back({reinterpret_cast<float*>(b.pll_poly[slot]), 4, 4 * ((size_t)1 + d.n_fm_out / kSpan)});
    }
    return v;
}
uint32_t state_version(fmd_handle h) { return h->ctx.fast ? 4u : 3u; }
size_t state_floats(fmd_handle h) {
    size_t n = S_NUM_FIELDS;
    for (const StatePart& p : state_parts(h)) n += p.floats;
    return n;
}
}  // namespace
}  // extern "C++"

// FMD_FLAG_RDS_DECODE: the channel's RDS decoder behind the float state — its RDS_F_NUM synchroniser fields, the group being assembled, the database
static constexpr size_t kRdsDecBlobBytes = RDS_F_NUM * sizeof(uint32_t) + sizeof(fmd_rds_group) + sizeof(fmd_rds_db);
size_t fmd_state_size(fmd_handle h) { return h ? sizeof(StateHeader) + sizeof(float) * state_floats(h) + (h->ctx.rds_decode ? kRdsDecBlobBytes : 0) : 0; }

int fmd_get_state(fmd_handle h, int channel, void* blob, size_t cap_bytes) {
    if (!h || !blob) return FMD_ERR_ARG;
    if (channel < 0 || channel >= h->cfg.n_channels) return fail(h, FMD_ERR_ARG, "channel %d out of range", channel);
    if (cap_bytes < fmd_state_size(h)) return fail(h, FMD_ERR_ARG, "state blob needs %zu bytes", fmd_state_size(h));
    if (h->poisoned) return fail(h, FMD_ERR_STATE, "an earlier block failed part-way: call fmd_reset");
    int rc = sync_all(h);
    if (rc) return rc;
    const Dims& d = h->ctx.d;
    StateHeader hd{kStateMagic, state_version(h), h->cfg.fs_baseband, d.m, (int32_t)S_NUM_FIELDS, d.tail_base, {0u, 0u}};
    std::memcpy(blob, &hd, sizeof(hd));
    float* out = reinterpret_cast<float*>(static_cast<char*>(blob) + sizeof(hd));
    // SoA fields [field][C] -> one float per field
    HIP_TRY(h, hipMemcpy2D(out, sizeof(float), h->ctx.b.state + channel, sizeof(float) * (size_t)d.C, sizeof(float), S_NUM_FIELDS, hipMemcpyDeviceToHost));
    const int par = (int)(h->sched.n_blocks() & 1);   // the histories the NEXT block reads
    // the two L-R phase fields hold P_k by k & 1 (fmd_kernels.hip: lmr_field); in the blob: PREV = the newest block's offset
    if (par == 1) std::swap(out[S_LMR_PHASE_CUR], out[S_LMR_PHASE_PREV]);
    // CUR = P_b, the offset the NEXT block is mixed with.  Where the next block's k_extract derives it itself (tolerance mode, small
    // batches) nothing has written it behind the newest block: materialise it here, so that a blob means the same whichever path
    // produced it and can be restored into a handle on the other side of that switch
    if (h->sched.n_blocks() > 0) {
        HIP_TRY(h, launch_lmr_phase_peek(h->ctx, (int)((h->sched.n_blocks() + 1) & 1), h->ctx.b.lmr_peek, h->own_stream));
        HIP_TRY(h, hipStreamSynchronize(h->own_stream));
        HIP_TRY(h, hipMemcpy(&out[S_LMR_PHASE_CUR], h->ctx.b.lmr_peek + channel, sizeof(float), hipMemcpyDeviceToHost));
    }
    out += S_NUM_FIELDS;
    for (const StatePart& p : state_parts(h)) {
        HIP_TRY(h, hipMemcpy(out, p.base + (size_t)channel * p.stride, sizeof(float) * p.floats, hipMemcpyDeviceToHost));
        out += p.floats;
    }
    if (h->ctx.rds_decode) {
        const RdsDecBufs& r = h->ctx.rds_dec;
        uint8_t* o = reinterpret_cast<uint8_t*>(out);
        HIP_TRY(h, hipMemcpy2D(o, sizeof(uint32_t), r.f + channel, sizeof(uint32_t) * (size_t)d.C, sizeof(uint32_t), RDS_F_NUM, hipMemcpyDeviceToHost));
        o += RDS_F_NUM * sizeof(uint32_t);
        HIP_TRY(h, hipMemcpy(o, r.group + channel, sizeof(fmd_rds_group), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(o + sizeof(fmd_rds_group), r.db + channel, sizeof(fmd_rds_db), hipMemcpyDeviceToHost));
    }
    return FMD_OK;
}

int fmd_set_state(fmd_handle h, int channel, const void* blob, size_t n_bytes) {
    if (!h || !blob) return FMD_ERR_ARG;
    if (channel < 0 || channel >= h->cfg.n_channels) return fail(h, FMD_ERR_ARG, "channel %d out of range", channel);
    if (h->poisoned) return fail(h, FMD_ERR_STATE, "an earlier block failed part-way: call fmd_reset");
    const Dims& d = h->ctx.d;
    StateHeader hd;
    if (n_bytes < sizeof(hd)) return fail(h, FMD_ERR_ARG, "state blob too short");
    std::memcpy(&hd, blob, sizeof(hd));
    if (hd.magic != kStateMagic) return fail(h, FMD_ERR_ARG, "not a state blob");
    // exact mode: the layout has not changed since version 2; tolerance mode: version 4 (round 4: the pilot stage's decimated filter state and
    // its last four column sums) — older tolerance-mode blobs lack what k_pll_sparse continues from
    if (h->ctx.fast ? hd.version != 4u : (hd.version < 2u || hd.version > 4u))
        return fail(h, FMD_ERR_ARG, "state blob version %u, this handle takes %s", hd.version, h->ctx.fast ? "4" : "2-4");
    if (hd.fs_baseband != h->cfg.fs_baseband || hd.m != d.m || hd.n_fields != (int32_t)S_NUM_FIELDS || hd.tail_base != d.tail_base || n_bytes != fmd_state_size(h))
        return fail(h, FMD_ERR_ARG, "state blob does not match this handle (rate %d vs %d, %d vs %d fields, %zu vs %zu bytes: the mode or the flags differ)", hd.fs_baseband,
                    h->cfg.fs_baseband, hd.n_fields, (int)S_NUM_FIELDS, n_bytes, fmd_state_size(h));
    int rc = sync_all(h);
    if (rc) return rc;
    const float* in = reinterpret_cast<const float*>(static_cast<const char*>(blob) + sizeof(hd));
    const int par = (int)(h->sched.n_blocks() & 1);
    std::vector<float> fields(in, in + S_NUM_FIELDS);
    if (par == 1) std::swap(fields[S_LMR_PHASE_CUR], fields[S_LMR_PHASE_PREV]);   // see fmd_get_state
    HIP_TRY(h, hipMemcpy2D(h->ctx.b.state + channel, sizeof(float) * (size_t)d.C, fields.data(), sizeof(float), sizeof(float), S_NUM_FIELDS, hipMemcpyHostToDevice));
    // a station restored inside its start-up transient (tolerance mode: SA_X1I counts its samples since the reset) keeps k_pll_span for the rest of it
    if (h->ctx.fast && fields[SA_X1I] < kPllWarmSamples)
        h->sched.keep_warm((int)((kPllWarmSamples - fields[SA_X1I] + (float)d.n_fm_out - 1.0f) / (float)d.n_fm_out));
    in += S_NUM_FIELDS;
    for (const StatePart& p : state_parts(h)) {
        HIP_TRY(h, hipMemcpy(p.base + (size_t)channel * p.stride, in, sizeof(float) * p.floats, hipMemcpyHostToDevice));
        in += p.floats;
    }
    if (h->ctx.rds_decode) {
        const RdsDecBufs& r = h->ctx.rds_dec;
        const uint8_t* i8 = reinterpret_cast<const uint8_t*>(in);
        HIP_TRY(h, hipMemcpy2D(r.f + channel, sizeof(uint32_t) * (size_t)d.C, i8, sizeof(uint32_t), sizeof(uint32_t), RDS_F_NUM, hipMemcpyHostToDevice));
        i8 += RDS_F_NUM * sizeof(uint32_t);
        HIP_TRY(h, hipMemcpy(r.group + channel, i8, sizeof(fmd_rds_group), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(r.db + channel, i8 + sizeof(fmd_rds_group), sizeof(fmd_rds_db), hipMemcpyHostToDevice));
    }
    return FMD_OK;
}

static int selftest_atan2_host(const float* y, const float* x, float* out, uint8_t* ok, size_t n, int table_form = 0) {
    if (!y || !x || !out) return FMD_ERR_ARG;
    if (fmd_device_count() <= 0) return fail(nullptr, FMD_ERR_NO_DEVICE, "no gfx950 device");
    float *dy = nullptr, *dx = nullptr, *dout = nullptr;
    unsigned char* dok = nullptr;
    const size_t bytes = n * sizeof(float);
    int rc = FMD_OK;
    if (hipMalloc(&dy, bytes) != hipSuccess || hipMalloc(&dx, bytes) != hipSuccess || hipMalloc(&dout, bytes) != hipSuccess) rc = FMD_ERR_DEVICE;
    if (!rc && ok && hipMalloc(&dok, n) != hipSuccess) rc = FMD_ERR_DEVICE;
    if (!rc && (hipMemcpy(dy, y, bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice) != hipSuccess)) rc = FMD_ERR_DEVICE;
    if (!rc && selftest_atan2(dy, dx, dout, dok, n, table_form, nullptr) != hipSuccess) rc = FMD_ERR_DEVICE;
    if (!rc && hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = FMD_ERR_DEVICE;
    if (!rc && ok && hipMemcpy(ok, dok, n, hipMemcpyDeviceToHost) != hipSuccess) rc = FMD_ERR_DEVICE;
    if (dy) (void)hipFree(dy);
    if (dx) (void)hipFree(dx);
    if (dout) (void)hipFree(dout);
    if (dok) (void)hipFree(dok);
    return rc ? fail(nullptr, rc, "selftest_atan2 failed") : FMD_OK;
}

int fmd_selftest_atan2(const float* y, const float* x, float* out, size_t n) { return selftest_atan2_host(y, x, out, nullptr, n); }

int fmd_selftest_atan2_table(const float* y, const float* x, float* out, size_t n) { return selftest_atan2_host(y, x, out, nullptr, n, 1); }
int fmd_selftest_atan2_table_u8(const float* y, const float* x, float* out, size_t n) { return selftest_atan2_host(y, x, out, nullptr, n, 2); }

int fmd_selftest_fast_math(int kind, const float* a, const float* b, float* out, size_t n) {
    if (kind < 0 || kind > 3) return FMD_ERR_ARG;
    return selftest_atan2_host(a, b ? b : a, out, nullptr, n, 10 + kind);
}

int fmd_selftest_atan2_small(const float* y, const float* x, float* out, uint8_t* ok, size_t n) {
    if (!ok) return FMD_ERR_ARG;
    return selftest_atan2_host(y, x, out, ok, n);
}

int fmd_get_spec_stats(fmd_handle h, uint64_t* out8, int reset) {
    if (!h || !out8) return FMD_ERR_ARG;
    int rc = fmd_synchronize(h);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpy(out8, h->ctx.b.spec_stats, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(h, hipMemset(h->ctx.b.spec_stats, 0, 8 * sizeof(uint64_t)));
    return FMD_OK;
}

int fmd_debug_split_front(fmd_handle h, int on) {
    if (!h) return FMD_ERR_ARG;
    int rc = fmd_synchronize(h);
    if (rc) return rc;
    h->ctx.facts.split_front = on != 0;
    refresh_block_plan(h->ctx);
    return FMD_OK;
}

int fmd_debug_pll_adaptive(fmd_handle h, int k16_max_channels, int time_parallel_max_channels) {
    if (!h || k16_max_channels < 0 || time_parallel_max_channels < 0) return FMD_ERR_ARG;
    if (h->ctx.fast || !h->pll_unl_host || h->ctx.plan.effective > kPllK16UnlockedMaxEff) return fail(h, FMD_ERR_ARG, "the exact mode, up to 4096 stations");
    int rc = fmd_synchronize(h);
    if (rc) return rc;
    const Dims& d = h->ctx.d;
    const PllThresholds moved{k16_max_channels, time_parallel_max_channels};
    h->ctx.plan = make_plan(d.C, d.m, d.n_fm_out, d.n_est, h->cfg.flags, &moved);
    refresh_block_plan(h->ctx);
    h->ctx.pll_unlocked_now = false;
    return FMD_OK;
}

int fmd_debug_plan(const fmd_config* cfg, int k16_max_channels, int time_parallel_max_channels, int unlocked_now, fmd_plan_info* out) {
    int m = 0;
    if (!out || !config_ok(cfg, &m) || (k16_max_channels < 0) != (time_parallel_max_channels < 0)) return FMD_ERR_ARG;
    const Dims d = dims_of(*cfg, m);
    const PllThresholds moved{k16_max_channels, time_parallel_max_channels};
    const bool is_moved = k16_max_channels >= 0;
    if (is_moved && ((cfg->flags & FMD_FLAG_FAST_MATH) || effective_channels(d.C, d.m) > kPllK16UnlockedMaxEff)) return FMD_ERR_ARG;   // (as fmd_debug_pll_adaptive)
    const Plan p = make_plan(d.C, d.m, d.n_fm_out, d.n_est, cfg->flags, is_moved ? &moved : nullptr);
    *out = fmd_plan_info{p.effective, p.power_rows, p.pll_k_adaptive, p.pll_chained, p.pll_waves, p.lmr_inline, p.lazy_capable, p.front_lds_pad,
                         p.front_big_tile, p.extract_auto_pair, (int)pll_kernel(p, unlocked_now != 0)};
    return FMD_OK;
}

int fmd_debug_block_plan(const fmd_config* cfg, const fmd_plan_facts* facts, int u8, fmd_block_plan_info* out) {
    int m = 0;
    if (!out || !facts || !config_ok(cfg, &m) || facts->extract_pairing < 0 || facts->extract_pairing > 2) return FMD_ERR_ARG;
    const Dims d = dims_of(*cfg, m);
    const Plan p = make_plan(d.C, d.m, d.n_fm_out, d.n_est, cfg->flags);
    PlanFacts f;
    f.any_deemph = facts->any_deemph != 0; f.deemph_in_tile = facts->deemph_in_tile != 0; f.split_front = facts->split_front != 0;
    f.uniform_cutoffs = facts->uniform_cutoffs != 0; f.extract_pairing = facts->extract_pairing;
    const BlockPlan b = make_block_plan(p, f);
    const BlockPlan::Input& in = b.in[u8 != 0];
    *out = fmd_block_plan_info{b.iq_streams, (int)b.front, (int)in.front_input, in.front_tile, b.front_warmup, in.front_workgroups, b.front_lds_pad,
                               (int)in.predecim, in.predecim_tile, in.predecim_workgroups, b.deemph_pilot_sums, b.deemph_workgroups, p.power_rows,
                               (int)b.lmr_phase, b.extract_tile, b.extract_bp, b.extract_nt, b.extract_pair, b.extract_grid_x, (int)b.rds, b.rds_partials};
    return FMD_OK;
}

int fmd_debug_extract_pairing(fmd_handle h, int mode) {
    if (!h || mode < 0 || mode > 2) return FMD_ERR_ARG;
    int rc = fmd_synchronize(h);
    if (rc) return rc;
    h->ctx.facts.extract_pairing = mode;
    refresh_block_plan(h->ctx);
    return FMD_OK;
}

int fmd_profile_enable(fmd_handle h, int on) {
    if (!h) return FMD_ERR_ARG;
    h->sched.set_profiling(on < 0 ? 0 : (on > 3 ? 3 : on));
    return FMD_OK;
}

int fmd_profile_read(fmd_handle h, fmd_kernel_time* out, int cap, int* n_out) {
    if (!h || !out || !n_out || cap <= 0) return FMD_ERR_ARG;
    int rc = fmd_synchronize(h);
    if (rc) return rc;
    int n = 0;
    for (ProfiledBlock* pm : h->marks) {
        for (int i = 0; i < ST_COUNT; i++) {
            if (!pm->used[i]) continue;
            float ms = 0.0f;
            HIP_TRY(h, hipEventElapsedTime(&ms, pm->t0[i], pm->t1[i]));
            int slot = -1;
            const char* nm = h->ctx.block.stage_name[i];
            for (int j = 0; j < n; j++) if (std::strncmp(out[j].name, nm, sizeof(out[j].name)) == 0) { slot = j; break; }
            if (slot < 0) {
                if (n >= cap) continue;
                slot = n++;
                std::memset(&out[slot], 0, sizeof(out[slot]));
                std::strncpy(out[slot].name, nm, sizeof(out[slot].name) - 1);
            }
            out[slot].total_ms += ms;
            out[slot].launches += 1;
        }
    }
    // hand-over on the PLL stream: end of one block's k_pilot_pll to the start of the next block's (the chain that bounds
    // the pipelined step at moderate batch sizes)
    if (n < cap) {
        double gap = 0.0; int cnt = 0;
        for (size_t b = 1; b < h->marks.size(); b++) {
            if (!h->marks[b - 1]->used[ST_PLL] || !h->marks[b]->used[ST_PLL]) continue;
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, h->marks[b - 1]->t1[ST_PLL], h->marks[b]->t0[ST_PLL]) == hipSuccess) { gap += ms; cnt++; }
        }
        if (cnt) {
            std::memset(&out[n], 0, sizeof(out[n]));
            std::strncpy(out[n].name, "gap:k_pilot_pll", sizeof(out[n].name) - 1);
            out[n].total_ms = gap; out[n].launches = cnt;
            n++;
        }
    }
    free_marks(h);
    *n_out = n;
    return FMD_OK;
}

const char* fmd_last_error(fmd_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// ---------------------------------------------------------------------------------------------------------------------------------
// Standalone batched RDS decoder (RDS_Decoding_Chain::Process for C byte streams): the handle's k_rds_decode on the caller's bytes.
struct fmd_rdsdec_s {
    int C = 0, device = 0;
    hipStream_t own = nullptr;
    hipEvent_t done = nullptr;            // behind the newest launch: the next call (whatever its stream) and the getters wait for it
    uint8_t* state = nullptr;
    RdsDecBufs st{};
    fmd_rds_db* db = nullptr;             // [C] snapshot after the newest call
    fmd_rds_group* groups = nullptr;      // [C][gcap] groups of the newest call
    int* counts = nullptr;                // [C]
    size_t groups_alloc = 0;              // groups allocated
    int gcap = 0;                         // groups per channel of the newest call
    uint8_t* stage = nullptr; size_t stage_bytes = 0;   // device staging of the host entry point: the bytes, then the counts
    std::string err;
};

static int rdsdec_fail(fmd_rdsdec d, int code, const char* what, hipError_t e) {
    d->err = std::string(what) + ": " + hipGetErrorString(e);
    return code;
}
#define RDSDEC_TRY(d, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return rdsdec_fail((d), FMD_ERR_DEVICE, #expr, e_); } while (0)

int fmd_rdsdec_groups_cap(int cap_bytes_per_channel) { return cap_bytes_per_channel < 0 ? 0 : rds_groups_cap(cap_bytes_per_channel); }

int fmd_rdsdec_create(int n_channels, int device, fmd_rdsdec* out) {
    if (!out || n_channels <= 0) return FMD_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FMD_ERR_NO_DEVICE;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return FMD_ERR_NO_DEVICE;
    if (device >= ndev) return FMD_ERR_ARG;
    fmd_rdsdec d = new (std::nothrow) fmd_rdsdec_s;
    if (!d) return FMD_ERR_ARG;
    d->C = n_channels;
    d->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->own, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->state), rds_dec_state_bytes(n_channels));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->db), sizeof(fmd_rds_db) * (size_t)n_channels);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->counts), sizeof(int) * (size_t)n_channels);
    if (e == hipSuccess) e = hipMemsetAsync(d->counts, 0, sizeof(int) * (size_t)n_channels, d->own);
    if (e == hipSuccess) { d->st = rds_dec_bufs(d->state, n_channels); e = rds_dec_upload_initial(d->state, n_channels, d->own); }
    if (e == hipSuccess) e = hipMemcpyAsync(d->db, d->st.db, sizeof(fmd_rds_db) * (size_t)n_channels, hipMemcpyDeviceToDevice, d->own);
    if (e == hipSuccess) e = hipEventRecord(d->done, d->own);
    if (e == hipSuccess) e = hipStreamSynchronize(d->own);
    if (e != hipSuccess) {
        g_create_error = std::string("fmd_rdsdec_create: ") + hipGetErrorString(e);
        fmd_rdsdec_destroy(d);
        return FMD_ERR_DEVICE;
    }
    *out = d;
    return FMD_OK;
}

int fmd_rdsdec_destroy(fmd_rdsdec d) {
    if (!d) return FMD_ERR_ARG;
    (void)hipSetDevice(d->device);
    if (d->done) (void)hipEventSynchronize(d->done);
    for (void* p : {(void*)d->state, (void*)d->db, (void*)d->groups, (void*)d->counts}) if (p) (void)hipFree(p);
    if (d->stage) (void)hipFree(d->stage);
    if (d->done) (void)hipEventDestroy(d->done);
    if (d->own) (void)hipStreamDestroy(d->own);
    delete d;
    return FMD_OK;
}

int fmd_rdsdec_reset(fmd_rdsdec d) {
    if (!d) return FMD_ERR_ARG;
    RDSDEC_TRY(d, hipSetDevice(d->device));
    RDSDEC_TRY(d, hipEventSynchronize(d->done));
    RDSDEC_TRY(d, rds_dec_upload_initial(d->state, d->C, d->own));
    return FMD_OK;
}

int fmd_rdsdec_reset_db(fmd_rdsdec d, int channel) {
    if (!d || channel < -1 || channel >= d->C) return FMD_ERR_ARG;
    RDSDEC_TRY(d, hipSetDevice(d->device));
    RDSDEC_TRY(d, hipEventSynchronize(d->done));
    RDSDEC_TRY(d, rds_dec_reset_db(d->st.db, d->C, channel));
    return FMD_OK;
}

int fmd_rdsdec_process_dev(fmd_rdsdec d, const uint8_t* d_bytes, const int* d_counts, int cap_bytes_per_channel, void* stream) {
    if (!d || !d_bytes || !d_counts || cap_bytes_per_channel < 0) return FMD_ERR_ARG;
    RDSDEC_TRY(d, hipSetDevice(d->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int gcap = rds_groups_cap(cap_bytes_per_channel);
    const size_t need = (size_t)d->C * gcap;
    if (need > d->groups_alloc) {       // the previous call's kernel may still write the old records: wait for it before freeing them
        RDSDEC_TRY(d, hipEventSynchronize(d->done));
        if (d->groups) RDSDEC_TRY(d, hipFree(d->groups));
        d->groups = nullptr;
        d->groups_alloc = 0;
        RDSDEC_TRY(d, hipMalloc(reinterpret_cast<void**>(&d->groups), sizeof(fmd_rds_group) * need));
        d->groups_alloc = need;
    }
    RDSDEC_TRY(d, hipStreamWaitEvent(s, d->done, 0));   // consecutive calls update the state in place: one after the other
    RdsDecArgs a{d->C, d_bytes, d_counts, cap_bytes_per_channel, d->st, d->db, d->groups, d->counts, gcap};
    RDSDEC_TRY(d, launch_rds_decode(a, s));
    RDSDEC_TRY(d, hipEventRecord(d->done, s));
    d->gcap = gcap;
    return FMD_OK;
}

int fmd_rdsdec_process_host(fmd_rdsdec d, const uint8_t* bytes, const int* counts, int cap_bytes_per_channel) {
    if (!d || !bytes || !counts || cap_bytes_per_channel < 0) return FMD_ERR_ARG;
    RDSDEC_TRY(d, hipSetDevice(d->device));
    RDSDEC_TRY(d, hipEventSynchronize(d->done));
    const size_t nb = (size_t)d->C * cap_bytes_per_channel, off = (nb + 15) & ~(size_t)15, total = off + sizeof(int) * (size_t)d->C;
    if (total > d->stage_bytes) {
        if (d->stage) RDSDEC_TRY(d, hipFree(d->stage));
        d->stage = nullptr;
        d->stage_bytes = 0;
        RDSDEC_TRY(d, hipMalloc(reinterpret_cast<void**>(&d->stage), total));
        d->stage_bytes = total;
    }
    int* dc = reinterpret_cast<int*>(d->stage + off);
    RDSDEC_TRY(d, hipMemcpyAsync(d->stage, bytes, nb, hipMemcpyHostToDevice, d->own));
    RDSDEC_TRY(d, hipMemcpyAsync(dc, counts, sizeof(int) * (size_t)d->C, hipMemcpyHostToDevice, d->own));
    int rc = fmd_rdsdec_process_dev(d, d->stage, dc, cap_bytes_per_channel, d->own);
    if (rc) return rc;
    RDSDEC_TRY(d, hipStreamSynchronize(d->own));
    return FMD_OK;
}

int fmd_rdsdec_get_db(fmd_rdsdec d, fmd_rds_db* db) {
    if (!d || !db) return FMD_ERR_ARG;
    RDSDEC_TRY(d, hipSetDevice(d->device));
    RDSDEC_TRY(d, hipEventSynchronize(d->done));
    RDSDEC_TRY(d, hipMemcpy(db, d->db, sizeof(fmd_rds_db) * (size_t)d->C, hipMemcpyDeviceToHost));
    return FMD_OK;
}

int fmd_rdsdec_get_groups(fmd_rdsdec d, fmd_rds_group* groups, int cap_groups_per_channel, int* counts) {
    if (!d || !counts || cap_groups_per_channel < 0 || (!groups && cap_groups_per_channel > 0)) return FMD_ERR_ARG;
    RDSDEC_TRY(d, hipSetDevice(d->device));
    RDSDEC_TRY(d, hipEventSynchronize(d->done));
    RDSDEC_TRY(d, hipMemcpy(counts, d->counts, sizeof(int) * (size_t)d->C, hipMemcpyDeviceToHost));
    if (!d->groups) return FMD_OK;
    std::vector<fmd_rds_group> tmp((size_t)d->C * d->gcap);
    RDSDEC_TRY(d, hipMemcpy(tmp.data(), d->groups, sizeof(fmd_rds_group) * tmp.size(), hipMemcpyDeviceToHost));
    for (int c = 0; c < d->C; c++) {
        const int n = std::min(counts[c], std::min(cap_groups_per_channel, d->gcap));
        if (n > 0) std::memcpy(groups + (size_t)c * cap_groups_per_channel, tmp.data() + (size_t)c * d->gcap, sizeof(fmd_rds_group) * (size_t)n);
    }
    return FMD_OK;
}

const char* fmd_rdsdec_last_error(fmd_rdsdec d) { return d ? d->err.c_str() : g_create_error.c_str(); }

}  // extern "C"
