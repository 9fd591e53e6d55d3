// Host-side design of every table the tolerance mode's kernels read (fmd_tables.h): operand images, band-pass tap tables, the block-edge
// matrix, the pilot loop's tables and the u8 wrap ties — and the fmd_design_* entry points of include/fmdemod_debug.h that show them to the
// tests.  Plain C++ (no HIP); -ffp-contract=off -fno-fast-math are part of the arithmetic.
#include "fmd_tables.h"

#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "fmd_design.h"
#include "fmd_math.h"
#include "fmdemod_debug.h"

namespace fmd {

// Operand images of k_front_mfma's FIRs (fmd_kernels.hip FrontGeomM): v_mfma_f32_16x16x32_bf16's A operand, lane l = row l % 16,
// k = 8 (l / 16) + 0..7; A[m][t] = taps[t - stride m] inside the band, 0 outside; every fp32 tap as two bf16 (round to nearest even).
static uint16_t bf16_rne(float x) {
    uint32_t u; std::memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static float bf16_to_f32(uint16_t h) { const uint32_t u = (uint32_t)h << 16; float x; std::memcpy(&x, &u, 4); return x; }
// one FIR's image: A[m][t] = taps[t - shift - stride m], t < 32 ksteps; [k-step][hi / lo][lane][8]
static void toeplitz_image(const float* taps, int n_taps, int stride, int ksteps, uint16_t* img, int shift = 0) {
    for (int sK = 0; sK < ksteps; sK++)
        for (int l = 0; l < 64; l++)
            for (int i = 0; i < 8; i++) {
                const int t = 32 * sK + 8 * (l / 16) + i, idx = t - shift - stride * (l % 16);
                const float v = (idx >= 0 && idx < n_taps) ? taps[idx] : 0.0f;
                const uint16_t hi = bf16_rne(v), lo = bf16_rne(v - bf16_to_f32(hi));
                img[(((size_t)sK * 2 + 0) * 64 + l) * 8 + i] = hi;
                img[(((size_t)sK * 2 + 1) * 64 + l) * 8 + i] = lo;
            }
}

// k_extract_bp (fmd_kernels_bp.inc): the harmonic mixer folded into the decimating FIR.  The reference's L-R / RDS rails are
//   sum_tau h[tau] a[t0 + tau] e^{j 2 pi H dt[t0 + tau]},  a[t] = x[t - 32] + j sum_n b_hil[n] x[t - 64 + n]   (broadcast_fm_demod.cpp:463-536)
// and the NCO's carrier part e^{-j 2 pi H 19 (t + 1) / 128} with the Hilbert FIR is ONE complex FIR of 192 taps on the real signal x:
//   G[u] = sum_tau h[tau] e^{-j 2 pi H 19 tau / 128} (delta[u - tau - 32] + j b_hil[u - tau]),     S[m] = sum_u G[u] x[M m - 188 + 4 (M / 8) + u]
// (in double; the phase of the carrier through its exact period of 128 samples)
static void bandpass_taps(const float* h, const float* b_hil, int H, float* g_re, float* g_im) {
    double re[kBpTaps] = {0.0}, im[kBpTaps] = {0.0};
    const double two_pi = 6.283185307179586476925;
    for (int tau = 0; tau < 128; tau++) {
        const int k = (H * 19 * tau) % 128;
        const double cr = std::cos(two_pi * k / 128.0), ci = -std::sin(two_pi * k / 128.0), hv = h[tau];
        re[tau + 32] += hv * cr; im[tau + 32] += hv * ci;
        for (int n = 0; n < 65; n++) {
            const double b = b_hil[n];
            if (b == 0.0) continue;
            re[tau + n] += hv * (-ci) * b;        // j (cr + j ci) = -ci + j cr
            im[tau + n] += hv * cr * b;
        }
    }
    for (int u = 0; u < kBpTaps; u++) { g_re[u] = (float)re[u]; g_im[u] = (float)im[u]; }
}
// Tap tables of k_extract_bp (fmd_kernels_bp.inc): kBpTL bf16 each, tap i at element kBpPadL + i (+ 4 for a "copy 4" table)
static void bp_tap_table(const float* taps, int n_taps, int move, uint16_t* hi, uint16_t* lo) {
    for (int i = 0; i < kBpTL; i++) { hi[i] = 0; if (lo) lo[i] = 0; }
    for (int i = 0; i < n_taps; i++) {
        const uint16_t h = bf16_rne(taps[i]);
        hi[kBpPadL + move + i] = h;
        if (lo) lo[kBpPadL + move + i] = bf16_rne(taps[i] - bf16_to_f32(h));
    }
}
// a stride-4 family's block: [hi, copy 0][hi, copy 4][lo, copy 0][lo, copy 4]
static void bp_family_block(const float* taps, int n_taps, uint16_t* dst) {
    bp_tap_table(taps, n_taps, 0, dst, dst + 2 * kBpTL);
    bp_tap_table(taps, n_taps, 4, dst + kBpTL, dst + 3 * kBpTL);
}
void bp_slot_tap_tables(const float* taps, const float* b_hil, uint16_t* dst) {
    bp_family_block(taps, 128, dst);
    float gr[kBpTaps], gi[kBpTaps];
    bandpass_taps(taps, b_hil, 2, gr, gi);
    bp_family_block(gr, kBpTaps, dst + 4 * kBpTL);
    bp_family_block(gi, kBpTaps, dst + 8 * kBpTL);
}
// RDS (rows (o, rail), band offset 4 + 8 o: every table moved on by four): S0 [re hi][im hi][re lo][im lo], S1 [re hi][im hi]
void bp_rds_tap_tables(const float* b_rds, const float* b_hil, uint16_t* dst) {
    float gr[kBpTaps], gi[kBpTaps], h1[128];
    bandpass_taps(b_rds, b_hil, 3, gr, gi);
    bp_tap_table(gr, kBpTaps, 4, dst, dst + 2 * kBpTL);
    bp_tap_table(gi, kBpTaps, 4, dst + kBpTL, dst + 3 * kBpTL);
    for (int i = 0; i < 128; i++) h1[i] = (float)(((double)i - 63.5) * (double)b_rds[i]);
    bandpass_taps(h1, b_hil, 3, gr, gi);
    bp_tap_table(gr, kBpTaps, 4, dst + 4 * kBpTL, nullptr);
    bp_tap_table(gi, kBpTaps, 4, dst + 5 * kBpTL, nullptr);
}

// The block's first 31 L-R outputs, the part of their sums that lies in the PREVIOUS block (mixed with its L-R offset, reference
// broadcast_fm_demod.cpp:485-517): S_old[m] = sum_{tau < 124 - 4 m} h[tau] e^{-j 2 pi 38 tau / 128} a[4 m - 124 + tau] = sum_u K_m[u] W[u],
// W[u] = fm_out[u - 188], K_m[u] = (composite of the TRUNCATED taps)[u - 4 m].  Layout [m][lane p of 8][24 columns][re, im], fp16.
static uint16_t f32_to_f16_rne(float x) {       // IEEE binary16, round to nearest even (the matrix entries are < 1: no overflow; denormals kept)
    uint32_t u; std::memcpy(&u, &x, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const int e = (int)((u >> 23) & 0xffu) - 127 + 15;
    uint32_t m = u & 0x7fffffu;
    if (e >= 31) return (uint16_t)(sign | 0x7c00u);
    if (e <= 0) {
        if (e < -10) return (uint16_t)sign;
        m |= 0x800000u;
        const int sh = 14 - e;
        const uint32_t r = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
        return (uint16_t)(sign | (r + ((rem > half || (rem == half && (r & 1u))) ? 1u : 0u)));
    }
    const uint32_t r = ((uint32_t)e << 10) | (m >> 13), rem = m & 0x1fffu;
    return (uint16_t)(sign | (r + ((rem > 0x1000u || (rem == 0x1000u && (r & 1u))) ? 1u : 0u)));
}
void bp_edge_matrix(const float* taps, const float* b_hil, uint16_t* dst) {
    constexpr int NM = kBpEdgeRows / 8, NC = kBpEdgeU4 * 4;       // outputs; columns per lane
    static_assert(8 * NC == kBpTaps, "eight lanes share an output's taps");
    std::memset(dst, 0, sizeof(uint16_t) * kBpEdgeHalves);
    for (int m = 0; m < NM; m++) {
        float ht[128], gr[kBpTaps], gi[kBpTaps];
        for (int i = 0; i < 128; i++) ht[i] = i < 124 - 4 * m ? taps[i] : 0.0f;
        bandpass_taps(ht, b_hil, 2, gr, gi);
        for (int u = 0; u < kBpTaps; u++) {
            const int idx = u - 4 * m;
            if (idx < 0 || idx >= kBpTaps) continue;
            uint16_t* e = dst + (((size_t)m * 8 + u / NC) * NC + u % NC) * 2;
            e[0] = f32_to_f16_rne(gr[idx]); e[1] = f32_to_f16_rne(gi[idx]);
        }
    }
}

// Tables of the parallel form of the pilot peak filter (fmd_tables.h PilotFastTab), in double precision.
void design_pilot_fast(const fmd_coeffs& k, PilotFastTab* t) {
    const double a0 = k.pilot_a[0], a1 = k.pilot_a[1];
    struct M2 { double a, b, c, d; };
    auto mul = [](const M2& x, const M2& y) { return M2{x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d}; };
    const M2 A{a1, a0, 1.0, 0.0};
    M2 P = A;                                   // A^(k+1)
    for (int i = 0; i < kPilotSeg; i++) { t->h1[i] = (float)P.a; t->h2[i] = (float)P.b; if (i + 1 < kPilotSeg) P = mul(A, P); }
    M2 S = P;                                   // M = A^kPilotSeg
    for (int s = 0; s < 4; s++) { t->m[s][0] = (float)S.a; t->m[s][1] = (float)S.b; t->m[s][2] = (float)S.c; t->m[s][3] = (float)S.d; S = mul(S, S); }
    M2 L{1.0, 0.0, 0.0, 1.0};
    for (int l = 0; l <= 32; l++) { t->mlane[l][0] = (float)L.a; t->mlane[l][1] = (float)L.b; t->mlane[l][2] = (float)L.c; t->mlane[l][3] = (float)L.d; L = mul(P, L); }
    t->k = k.pilot_b[0]; t->a0 = k.pilot_a[0]; t->a1 = k.pilot_a[1];
}

// Tables of k_pll_span (fmd_tables.h PllSpanTab): the pilot PLL's loop filter, integrator and NCO over one span as a linear map,
// in double.  Unknowns v = (lpf, I, e1, e2, r0, eh[0..L-1]); conventions of the reference loop (broadcast_fm_demod.cpp:430-456):
// at sample n it uses the previous sample's error, lpf[n] = b0 e[n-2] + b1 e[n-1] + a0 lpf[n-1], I[n] = I[n-1] + 0.1 Ts e[n-1],
// f[n] = -19000 - 100 (0.01 lpf[n] + I[n]), t[n] = t[n-1] + Ts f[n]; with the hold at F0 = f[0] + r0 the error is
// e[n] = 2 pi (eh[n] + dev[n]), dev[n] = Ts sum_{j <= n} (f[j] - F0): substituting sample by sample is the triangular solve.
// rows[r][i]: coefficient of unknown i = (lpf, I, e1, e2, r0, eh[0..L-1]) in row r, in double
static void span_rows(const fmd_coeffs& k, std::vector<double> (&rows)[kSpanRows]) {
    constexpr int L = kSpan, NV = 5 + L;
    const double b0 = k.pll_lpf_b[0], b1 = k.pll_lpf_b[1], a0 = k.pll_lpf_a[0];
    const float Ts32 = 1.0f / 128000.0f;                       // the reference's PLL_Mixer KTs (broadcast_fm_demod.cpp:226-235), a float
    const double Ts = (double)Ts32, ktsi = (double)(0.1f * Ts32), two_pi = 6.283185307179586476925;
    using Vec = std::vector<double>;
    auto unit = [&](int i) { Vec v(NV, 0.0); v[(size_t)i] = 1.0; return v; };
    Vec lpf = unit(0), I = unit(1), e1 = unit(2), e2 = unit(3), dev(NV, 0.0), g0;
    for (int n = 0; n < L; n++) {
        Vec g(NV), e(NV);
        for (int i = 0; i < NV; i++) {
            lpf[i] = b0 * e2[i] + b1 * e1[i] + a0 * lpf[i];
            I[i] += ktsi * e1[i];
            g[i] = -100.0 * (0.01 * lpf[i] + I[i]);
        }
        if (n == 0) g0 = g;
        for (int i = 0; i < NV; i++) dev[i] += Ts * (g[i] - g0[i]);
        dev[4] -= Ts;                                           // the hold runs r0 faster than f[0]
        for (int i = 0; i < NV; i++) e[i] = two_pi * dev[i];
        e[5 + n] += two_pi;
        if (n == kSpanN1) rows[2] = dev;
        if (n == kSpanN2) rows[3] = dev;
        if (n == L - 1) { rows[0] = lpf; rows[1] = I; rows[4] = dev; }
        e2 = e1; e1 = e;
    }
}

// (alpha, beta, gamma) of dev(n) ~ alpha n + beta n^2 + gamma n^3 through the three deviation rows
static void span_cubic_inverse(float (&minv)[3][4]) {
    constexpr int L = kSpan;
    const double x[3] = {(double)kSpanN1, (double)kSpanN2, (double)(L - 1)};
    double A[3][3], inv[3][3];
    for (int i = 0; i < 3; i++) { A[i][0] = x[i]; A[i][1] = x[i] * x[i]; A[i][2] = x[i] * x[i] * x[i]; }
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            inv[j][i] = (A[i1][j1] * A[i2][j2] - A[i1][j2] * A[i2][j1]) / det;     // cofactor (cyclic indices carry the sign), transposed
        }
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) minv[i][j] = (float)inv[i][j]; minv[i][3] = 0.0f; }
}

void design_pll_span(const fmd_coeffs& k, PllSpanTab* t) {
    constexpr int L = kSpan;
    const float Ts32 = 1.0f / 128000.0f;
    const double Ts = (double)Ts32, two_pi = 6.283185307179586476925;
    std::vector<double> rows[kSpanRows];
    span_rows(k, rows);
    std::memset(t, 0, sizeof(*t));
    for (int r = 0; r < kSpanRows; r++) {
        for (int n = 0; n < L; n++) t->w[r][n] = (float)rows[r][(size_t)(5 + n)];
        for (int i = 0; i < 5; i++) t->s[r][i] = (float)rows[r][(size_t)i];
    }
    span_cubic_inverse(t->minv);
    // quadrature of the filtered pilot's real rail.  The reference's Hilbert rail is im[n] = sum_k b[k] s[n - 64 + k] beside
    // re[n] = s[n - 32] (hilbert_fir_filter.h:26-46); for s = cos(w0 n) that is |H(w0)| sin(w0 (n - 32)), and
    // re[n-1] - re[n+1] = 2 sin(w0) sin(w0 (n - 32)): im[n] = quad (re[n-1] - re[n+1]), quad = |H(w0)| / (2 sin w0)
    const double w0 = two_pi * 19000.0 / 128000.0;
    double hr = 0.0, hi = 0.0;
    for (int i = 0; i < 65; i++) { hr += k.b_hilbert[i] * std::cos(w0 * i); hi += k.b_hilbert[i] * std::sin(w0 * i); }
    t->quad = (float)(std::sqrt(hr * hr + hi * hi) / (2.0 * std::sin(w0)));
    t->kappa = (float)(-19000.0 * Ts + 19.0 / 128.0);
    for (int i = 0; i < 32; i++) t->hil[i] = k.b_hilbert[2 * i + 1];
}

// Tables of k_pll_sparse (fmd_tables.h PllSparseTab; float64 model: tools/proto/sparse_pll.py design_sparse)
void design_pll_sparse(const fmd_coeffs& k, PllSparseTab* t) {
    using cd = std::complex<double>;
    constexpr int L = kSpan, D = kSparseDec, KP = kSparsePts;
    const double two_pi = 6.283185307179586476925, w0 = two_pi * 19.0 / 128.0;
    const float Ts32 = 1.0f / 128000.0f;
    std::memset(t, 0, sizeof(*t));
    // the poles of the peak filter as its float coefficients have them: y[n] = K x[n-2] + a1 y[n-1] + a0 y[n-2], a0 = -r^2, a1 = 2 r cos wp
    const double r = std::sqrt(-(double)k.pilot_a[0]), wp = std::acos((double)k.pilot_a[1] / (2.0 * r));
    const cd rho = std::polar(r, wp - w0);
    // W[q], q = -8 .. 23: the 17-tap boxcar (centred) in front of the exact decimation by 16, sum_i rho^i over the i it covers
    cd W[2 * D];
    for (int q = -8; q < 24; q++) {
        cd acc = 0.0;
        for (int i = 0; i < D; i++) if (std::abs(q - i) <= 8) acc += std::pow(rho, i);
        W[q + 8] = acc / 17.0;
    }
    cd wcd[2 * D];
    for (int tt = 0; tt < 2 * D; tt++) {                        // tap tt multiplies x[m' - 25 + tt], q = 23 - tt; the mixer relative to the point (m' = span + 16 k - 23)
        wcd[tt] = W[(23 - tt) + 8] * std::polar(1.0, -w0 * (double)(tt - 46));
        t->wre[tt] = (float)wcd[tt].real(); t->wim[tt] = (float)wcd[tt].imag();
    }
    const cd rho16 = std::pow(rho, D);
    for (int kk = 0; kk < KP; kk++) {
        const cd ro = std::polar(1.0, -w0 * (double)(D * kk)), ca = std::pow(rho16, kk + 1);
        t->rot[kk][0] = (float)ro.real(); t->rot[kk][1] = (float)ro.imag();
        t->carry[kk][0] = (float)ca.real(); t->carry[kk][1] = (float)ca.imag();
        t->nk1[kk] = (float)(D * kk + 10);
    }
    double nbar = 0.0, s2 = 0.0;
    for (int kk = 0; kk < KP; kk++) nbar += (double)(D * kk + 9) / KP;
    for (int kk = 0; kk < KP; kk++) { const double c = (double)(D * kk + 9) - nbar; t->ck[kk] = (float)c; s2 += c * c; }
    for (int s_ = 0; s_ < 3; s_++) { const cd p = std::pow(rho16, 1 << s_); t->scan[s_][0] = (float)p.real(); t->scan[s_][1] = (float)p.imag(); }
    const cd cA = cd(0.0, -1.0) * ((double)k.pilot_b[0] / std::sin(wp)) * std::polar(1.0, wp);
    double phi0 = std::arg(cA) / two_pi - 19.0 * 33.0 / 128.0;
    phi0 -= std::nearbyint(phi0);
    t->phi0 = (float)phi0; t->inv_s2 = (float)(1.0 / s2); t->nbar = (float)nbar;
    t->kappa = (float)(-19000.0 * (double)Ts32 + 19.0 / 128.0);
    double hr = 0.0, hi = 0.0;
    for (int i = 0; i < 65; i++) { hr += k.b_hilbert[i] * std::cos(w0 * i); hi += k.b_hilbert[i] * std::sin(w0 * i); }
    const double g2 = hr * hr + hi * hi;                        // |H_hilbert(w0)|^2: the reference's imaginary rail carries it
    t->pw_scale = (float)(std::norm(cA) * (1.0 + g2) * 0.5 * (double)D);
    // the non-resonant branch: Z_eff = Z - e^{-2 j wp} u_slow / (1 - rho2), rho2 = r e^{-j (wp + w0)}, u_slow = V / (DC gain of a point's 32 weights)
    cd wdc = 0.0;
    for (int q = 0; q < 2 * D; q++) wdc += W[q];
    const cd kap2 = -std::polar(1.0, -2.0 * wp) / (wdc * (1.0 - std::polar(r, -(wp + w0))));
    t->kap2[0] = (float)kap2.real(); t->kap2[1] = (float)kap2.imag();
    std::vector<double> rows[kSpanRows];
    span_rows(k, rows);
    {   // rows 2..4 -> (alpha, beta, gamma) of the deviation's cubic
        float mi[3][4];
        span_cubic_inverse(mi);
        const std::vector<double> d1 = rows[2], d2 = rows[3], d3 = rows[4];
        for (int i = 0; i < 3; i++)
            for (size_t j = 0; j < d1.size(); j++) rows[2 + i][j] = (double)mi[i][0] * d1[j] + (double)mi[i][1] * d2[j] + (double)mi[i][2] * d3[j];
    }
    for (int rr = 0; rr < kSpanRows; rr++) {
        double ws = 0.0, wm = 0.0, suf = 0.0;
        for (int n = L - 1; n >= 0; n--) {
            const double w = rows[rr][(size_t)(5 + n)];
            ws += w; wm += w * ((double)n - nbar); suf += w;
            t->sw[rr][n] = (float)suf;
        }
        t->wsum[rr] = (float)ws; t->wmom[rr] = (float)wm;
        for (int i = 0; i < 5; i++) t->s[rr][i] = (float)rows[rr][(size_t)i];
    }
}

// PllSparseTab::wrap_tie (fmd_kernels.hip wrap_tie_u8): for every u8 sample (x, y) the sign of the reference's wrapped phase difference to a
// sample in exactly the opposite direction — fm_demod.cpp:36-43 on glibc's atan2f, restated bit for bit (fmd_math.h fmd_atan2f_full)
void design_wrap_tie(uint32_t* bits2048) {
    std::memset(bits2048, 0, sizeof(uint32_t) * 2048);
    const float pi = fmd::bits_f32(fmd::kPiBits), two_pi = fmd::bits_f32(fmd::kTwoPiBits);
    for (int yr = 0; yr < 256; yr++)
        for (int xr = 0; xr < 256; xr++) {
            const float x = (float)xr - 127.0f, y = (float)yr - 127.0f;
            if (x == 0.0f && y == 0.0f) continue;
            float dl = fmd::fmd_atan2f_full(0.0f - y, 0.0f - x) - fmd::fmd_atan2f_full(y, x);       // (0 - v: the opposite sample is (float)u8 - 127 too, never -0)
            if (dl >= pi) dl = dl - two_pi;
            else if (dl <= -pi) dl = dl + two_pi;
            const unsigned key = ((unsigned)yr << 8) | (unsigned)xr;
            if (dl > 0.0f) bits2048[key >> 5] |= 1u << (key & 31u);
        }
}

void design_front_mfma(const fmd_coeffs& k, int m, std::vector<uint16_t>& img) {
    const int ks_pre = m > 1 ? predecim_ksteps(m) : 0;                     // k_predecim_mfma (PredecimGeomM::KS, ::SH)
    img.assign(((size_t)kFrontImgU4 + (size_t)ks_pre * kImgKStepU4) * 8, 0);
    toeplitz_image(k.b_fm_out, 64, 2, 3, img.data());
    toeplitz_image(k.b_hilbert, 65, 1, 3, img.data() + (size_t)kFrontImgU4 / 2 * 8);
    if (m > 1) toeplitz_image(k.b_fm_in, 64, m, ks_pre, img.data() + (size_t)kFrontImgU4 * 8, predecim_shift(m));
}

}  // namespace fmd

using namespace fmd;

int fmd_design_pll_span(int fs_baseband, float* w, float* s, float* minv, float* misc2) {
    if (!w || !s || !minv || !misc2) return FMD_ERR_ARG;
    if (fs_baseband != 256000 && fs_baseband != 1024000 && fs_baseband != 2048000) return FMD_ERR_ARG;
    fmd_controls def;
    fmd_default_controls(&def);
    fmd_coeffs k{};
    design_all(&k, fs_baseband, &def);
    PllSpanTab t;
    design_pll_span(k, &t);
    std::memcpy(w, t.w, sizeof(t.w)); std::memcpy(s, t.s, sizeof(t.s)); std::memcpy(minv, t.minv, sizeof(t.minv));
    misc2[0] = t.quad; misc2[1] = t.kappa;
    return FMD_OK;
}

int fmd_design_pll_sparse(int fs_baseband, float* taps, float* cplx, float* rows, float* sw, float* misc8) {
    if (!taps || !cplx || !rows || !sw || !misc8) return FMD_ERR_ARG;
    if (fs_baseband != 256000 && fs_baseband != 1024000 && fs_baseband != 2048000) return FMD_ERR_ARG;
    fmd_controls def;
    fmd_default_controls(&def);
    fmd_coeffs k{};
    design_all(&k, fs_baseband, &def);
    PllSparseTab t;
    design_pll_sparse(k, &t);
    std::memcpy(taps, t.wre, sizeof(t.wre)); std::memcpy(taps + 2 * kSparseDec, t.wim, sizeof(t.wim));
    std::memcpy(cplx, t.rot, sizeof(t.rot)); std::memcpy(cplx + 16, t.scan, sizeof(t.scan)); std::memcpy(cplx + 22, t.carry, sizeof(t.carry));
    std::memcpy(rows, t.wsum, sizeof(t.wsum)); std::memcpy(rows + 8, t.wmom, sizeof(t.wmom));
    std::memcpy(sw, t.sw, sizeof(t.sw));
    const float m[8] = {t.phi0, t.inv_s2, t.nbar, t.kappa, t.pw_scale, t.kap2[0], t.kap2[1], 0.f};
    std::memcpy(misc8, m, sizeof(m));
    return FMD_OK;
}

int fmd_design_wrap_tie(uint32_t* bits2048) {
    if (!bits2048) return FMD_ERR_ARG;
    design_wrap_tie(bits2048);
    return FMD_OK;
}

int fmd_design_extract_bp(int fs_baseband, int cutoff_hz, float* g2, float* g3) {
    if (!g2 || !g3) return FMD_ERR_ARG;
    fmd_controls c;
    fmd_default_controls(&c);
    c.lmr_cutoff_hz = cutoff_hz;
    fmd_coeffs k{};
    design_all(&k, fs_baseband, &c);
    bandpass_taps(k.b_lmr, k.b_hilbert, 2, g2, g2 + kBpTaps);
    bandpass_taps(k.b_rds, k.b_hilbert, 3, g3, g3 + kBpTaps);
    return FMD_OK;
}
