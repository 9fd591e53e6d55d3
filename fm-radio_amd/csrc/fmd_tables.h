// Tables of the tolerance mode's kernels (FMD_FLAG_FAST_MATH): their layouts, the constants host and kernels share, and the host-side
// designers (fmd_tables.cpp).  No HIP here: the kernels see this header through fmd_kernels.h, the designers are built as plain C++ and
// run under the CPU sanitizers on their own (tests/cpp/tables_main.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "fmdemod.h"

namespace fmd {

// FMD_FLAG_FAST_MATH: the pilot peak filter y[n] = K x[n-2] + a1 y[n-1] + a0 y[n-2] evaluated as a parallel scan inside k_pll_span:
// each of a channel's 16 lanes runs kPilotSeg samples from a zero state, the segment end states are combined across the lanes
// with powers of the transition matrix A = [[a1, a0], [1, 0]], and the homogeneous solution is added back.  Designed on the
// host in double precision (fmd_tables.cpp design_pilot_fast).
static constexpr int kPilotSeg = 8;       // samples per lane (16 lanes per station)
struct PilotFastTab {
    float h1[kPilotSeg], h2[kPilotSeg];   // y[k] += h1[k] y[-1] + h2[k] y[-2]: first row of A^(k+1)
    float m[4][4];                        // M^(2^s), M = A^kPilotSeg, as (m00, m01, m10, m11): steps of the cross-lane scan within a row of 16 lanes
    float mlane[33][4];                   // M^j, j = 0..32: what the chunk's initial state contributes to the start state of lane j
    float k, a0, a1;
};

// FMD_FLAG_FAST_MATH, round 3: the pilot PLL advanced one span of kSpan samples at a time (k_pll_span).  Behind the pilot peak
// filter the phase detector's input is a line a few Hz wide, and everything between the detector and the NCO (loop filter,
// integrator, NCO phase) is linear: with the NCO frequency word of the span's first sample HELD, the error sequence
//   eh[n] = wrap(arg pilot[n] + t_prev + (n + 1) F0 Ts)                       (turns; one arctangent per sample, independent of the loop)
// determines the loop state after the span and the NCO phase at any sample as fixed weight vectors applied to eh — the feedback
// of the phase deviation from the hold into the later errors included exactly (a triangular solve, done on the host in double).
// Rows: 0 loop filter output after the span, 1 integrator after the span, 2..4 phase deviation from the hold at samples
// kSpanN1, kSpanN2, kSpan - 1.  v = (lpf, I, e1, e2, r0): the state the span starts from (e1 = newest error, radians) and
// r0 = F0 (as rounded to float, like the reference's frequency word) - its unrounded value.
static constexpr int kSpan = 128;
static constexpr int kSpanN1 = 41, kSpanN2 = 84;
static constexpr int kSpanRows = 5;
struct PllSpanTab {
    float w[kSpanRows][kSpan];       // weights of eh[n] (eh in TURNS: the 2 pi is folded in)
    float s[kSpanRows][8];           // weights of (lpf, I, e1, e2, r0), padded
    float minv[3][4];                // (alpha, beta, gamma) of dev(n) = alpha n + beta n^2 + gamma n^3 from the three deviation rows
    float quad;                      // quadrature of the filtered pilot's real rail P: im[n] = quad (P[n-1] - P[n+1]) (Hilbert FIR gain at 19 kHz / (2 sin w0))
    float kappa;                     // -19000 Ts + 19/128 with Ts = (float)(1 / 128000) as the reference's NCO has it: 7e-9 turns per sample, 9e-4 Hz
    float pad[2];
    float hil[32];                   // the Hilbert FIR's non-zero taps b[1], b[3], ... (a station's warm-up makes that rail for itself)
};
// Round 4: k_pll_sparse.  Behind the peak filter the pilot is a line a few Hz wide, and the filter itself is a complex one-pole low-pass
// of the down-mixed input:  P[m] = K x[m-2] + a1 P[m-1] + a0 P[m-2] = (K / sin wp) Im{ e^{j wp} e^{j w0 m} Z[m] },
// Z[m] = rho Z[m-1] + e^{-j w0 m} x[m-2],  rho = r e^{j (wp - w0)}  (r e^{+-j wp}: the poles the float coefficients really have;
// w0 = 2 pi 19 / 128: the mixer is periodic in the span).  Z decimates exactly (Z[m] = rho^16 Z[m-16] + 16 weighted inputs), so the
// loop's phase detector is evaluated at kSparsePts points per span instead of at every sample: one arctangent of Z per point, and
// the span's five weight rows applied to the straight line through the eight errors (the held-frequency error of a narrow line is
// a straight line in the span; what the reference's per-sample detector adds — the ellipse of its Hilbert rail, programme content
// >= 4 kHz away — its rows average out).  A 17-tap boxcar in front of the decimation (zeros every 8 kHz from the pilot: exactly what
// would alias onto it) is folded into the 32 input weights of a point.  tools/proto/sparse_pll.py is the float64 model of this
// against the oracle; tests/test_span_design.py checks the tables.  The filter has TWO poles: by partial fractions its output's analytic
// signal is e^{j wp} (x filtered by 1 / (1 - p z^-1)) - e^{-j wp} (x filtered by 1 / (1 - p* z^-1)); the second branch is not resonant at
// +19 kHz (gain 1 / (1 - r e^{-j (wp + w0)}) ~ 0.6 against 1 / (1 - r) = 10^4) and answers within a sample, so at a point it is the
// point's own input sum times a constant (kap2): 6e-5 rad of pilot phase in lock, 1e-3 rad for a pilot 35 Hz off.  A station's first 8192 samples after a reset stay with
// k_pll_span (the reference's start-up transient, see its warm-up rail).
static constexpr int kSparsePts = 8, kSparseDec = kSpan / kSparsePts;      // points per span, samples between them
static constexpr float kPllWarmSamples = 8192.0f;
struct PllSparseTab {
    // points sit at n_k = 16 k + 9 of a span: a point's 32 inputs fm_out[span + 16 k - 48 + t] are then two whole 16-sample columns of the
    // front end's tiles, (k - 3) its "old" half (taps 0..15) and (k - 2) its "new" half (taps 16..31): k_front_mfma sums both halves of every
    // column from its fp32 accumulators (front_from_phases) and k_pll_sparse reads 16 bytes per column instead of the 64 bytes of fm_out
    float wre[2 * kSparseDec], wim[2 * kSparseDec];
    float rot[kSparsePts][2];        // e^{-j w0 16 k}
    float scan[3][2];                // rho^16, rho^32, rho^64
    float carry[kSparsePts][2];      // rho^(16 (k + 1))
    float ck[kSparsePts];            // n_k - nbar, n_k = 16 k + 9
    float nk1[kSparsePts];           // n_k + 1
    float phi0;                      // arg(-j (K / sin wp) e^{j wp}) / 2 pi - 19 * 33 / 128: arg Z -> the phase the reference's detector sees, minus frac(19 (n + 1) / 128)
    float inv_s2, nbar, kappa, pw_scale;
    float kap2[2], pad_;             // the filter's second, non-resonant pole branch (see below): Z_eff = Z + kap2 V, V = the point's own 32-sample sum
    // rows: 0 loop filter output after the span, 1 integrator after the span (as PllSpanTab), 2..4 the coefficients alpha, beta, gamma of the
    // phase deviation's cubic directly (PllSpanTab's three deviation rows times its minv)
    float wsum[8], wmom[8];          // sum_n w[r][n], sum_n w[r][n] (n - nbar): the rows applied to a + b (n - nbar)
    float s[kSpanRows][8];           // weights of (lpf, I, e1, e2, r0)
    float sw[kSpanRows][kSpan + 4];  // sw[r][n] = sum_{n' >= n} w[r][n'] (the rare span in which the error crosses half a turn)
    // (carried here for the front end, which has this table's pointer) u8 captures: the reference's wrap of a phase difference of exactly pi
    // between two samples in opposite directions, one bit per first sample (y_raw << 8 | x_raw): 1 = the wrapped difference is +pi
    // (fmd_kernels.hip wrap_tie_u8)
    uint32_t wrap_tie[2048];
};
// Toeplitz operand images (v_mfma_f32_16x16x32_bf16's A operand): per K-step [hi / lo][lane] uint4s of 8 bf16
static constexpr int kImgKStepU4 = 2 * 64;
static constexpr int kFrontImgU4 = 2 * 3 * kImgKStepU4;   // uint4s of k_front_mfma's two operand images in Buffers::front_mfma; k_predecim_mfma's image follows them
// the first decimator (k_predecim_mfma, k_front_pre_mfma; m = 4, 8): its staged window starts this many samples early, on a multiple of
// 8 samples (16-byte loads of u8 captures), A[row][t] = b[t - shift - m row] ...
constexpr int predecim_shift(int m) { return 8 - m; }
// ... and t < 64 + shift + 15 m: 4 / 6 K-steps of 32
constexpr int predecim_ksteps(int m) { return (64 + predecim_shift(m) + 15 * m + 31) / 32; }
// rows of the fast-mode planes carry the previous block's last samples in front (written by k_pll_span of that block), so the
// consumers address history and block uniformly
static constexpr int kFoPad = 192;   // fm_out: k_extract_bp reaches back 124 + 64 samples (its Hilbert FIR), k_pll_span 33 (65 while a station warms up)

// k_extract_bp (fmd_kernels_bp.inc): the composite band-pass FIRs (harmonic mixer's carrier and Hilbert FIR folded into the decimating
// FIR's 128 taps) have kBpTaps taps.  Its tap tables are kBpTL bf16 each, zero padded, tap i at element kBpPadL + i (+ 4 for a "copy 4"
// table): kBpSlotTabs tables per distinct audio cut-off (Buffers::bp_tab), kBpRdsTabs for the RDS rails (Buffers::rds_bp_tab).
static constexpr int kBpTaps = 192;
static constexpr int kBpPadL = 96, kBpTL = 448;
static constexpr int kBpSlotTabs = 12, kBpRdsTabs = 6;
static constexpr size_t kBpTabSlotU16 = (size_t)kBpSlotTabs * kBpTL, kBpRdsTabU16 = (size_t)kBpRdsTabs * kBpTL;
// ... and the block-edge matrix (Buffers::bp_edge) per cut-off: [31 outputs][8 lanes] rows of 24 columns x (re, im) fp16 = kBpEdgeU4 uint4s
static constexpr int kBpEdgeRows = 31 * 8, kBpEdgeU4 = 6;
static constexpr size_t kBpEdgeHalves = (size_t)kBpEdgeRows * kBpEdgeU4 * 8;

// The designers (fmd_tables.cpp), all in double on the host; k: fmd_design.h design_all
void design_pilot_fast(const fmd_coeffs& k, PilotFastTab* t);
void design_pll_span(const fmd_coeffs& k, PllSpanTab* t);
void design_pll_sparse(const fmd_coeffs& k, PllSparseTab* t);             // (all but wrap_tie)
void design_wrap_tie(uint32_t* bits2048);                                 // PllSparseTab::wrap_tie
// the operand images of k_front_mfma's two FIRs, kFrontImgU4 uint4s, and behind them (m > 1) predecim_ksteps(m) K-steps of the first decimator's
void design_front_mfma(const fmd_coeffs& k, int m, std::vector<uint16_t>& img);
void bp_slot_tap_tables(const float* taps, const float* b_hil, uint16_t* dst);     // dst [kBpTabSlotU16]: a cut-off's L+R, L-R re, L-R im blocks
void bp_rds_tap_tables(const float* b_rds, const float* b_hil, uint16_t* dst);     // dst [kBpRdsTabU16]
void bp_edge_matrix(const float* taps, const float* b_hil, uint16_t* dst);         // dst [kBpEdgeHalves]

}  // namespace fmd
