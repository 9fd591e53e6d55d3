/* The loudness meter's true peak and loudness range (include/fmdemod.h, "True peak and loudness range") restated in plain C on top of
 * meter_ref.c, which this file compiles in: one station at a time and one frame after the other, what the tests compare the
 * fmd_meter_* r128 entry points with, bit for bit.  Built with -ffp-contract=off -fno-fast-math: every operation is the one written, and
 * every multiply-add of the interpolator is an explicit fmaf(). */
#include "meter_ref.c"

#define TP_T 12
#define TP_H (TP_T - 1)

typedef struct { int L, taps_per_phase; float taps[3][TP_T]; } meter_r128_tp_design_t;   /* the layout of fmd_meter_tp_design_t */

typedef struct {                       /* the layout of fmd_meter_r128_status */
    float    tp_call[2], tp_hold[2];
    unsigned st_below, st_nonfinite;
} meter_r128_status;

typedef struct {
    meter_ref_chan    base;
    meter_r128_status st;
    float    hist[2][TP_H];            /* per rail, oldest first: x[-11] ... x[-1] */
    unsigned range_hist[BINS];
} meter_r128_chan;

static double r128_i0(double x) {
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 64; k++) { term *= (x / (2.0 * k)) * (x / (2.0 * k)); sum += term; if (term < 1e-18 * sum) break; }
    return sum;
}

int meter_r128_tp_design(int fs, meter_r128_tp_design_t* d) {
    const double pi = 3.14159265358979323846, beta = 5.0;
    if (fs < 8000 || fs > 192000 || fs % 10 != 0) return -1;
    const int L = fs < 88200 ? 4 : fs < 176400 ? 2 : 1, N = L * TP_T;
    const double c = (double)(N / 2), i0b = r128_i0(beta);
    memset(d, 0, sizeof(*d));
    d->L = L;
    d->taps_per_phase = TP_T;
    for (int p = 1; p < L; p++) {
        double g[TP_T], sum = 0.0;
        for (int k = 0; k < TP_T; k++) {
            const double t = (double)(k * L + p) - c, x = t / (double)L, r = t / c;
            const double s = x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
            g[k] = s * r128_i0(beta * sqrt(1.0 - r * r)) / i0b;
            sum += g[k];
        }
        for (int k = 0; k < TP_T; k++) d->taps[p - 1][k] = (float)(g[k] / sum);
    }
    return 0;
}

void meter_r128_reset(meter_r128_chan* c) { memset(c, 0, sizeof(*c)); }

void meter_r128_reset_peaks(meter_r128_chan* c) {
    meter_ref_reset_peaks(&c->base);
    for (int r = 0; r < 2; r++) c->st.tp_call[r] = c->st.tp_hold[r] = 0.0f;
}

/* sub-block g has just completed and E_g is in the ring */
static void short_term_value(const meter_ref_design_t* d, meter_r128_chan* c, unsigned long long g) {
    double s = 0.0;
    if (g < RING - 1) return;
    for (unsigned long long i = g - (RING - 1); i <= g; i++) s += c->base.st.energy_ring[i % RING];
    const double S = s / 30.0;
    if (!isfinite(S)) c->st.st_nonfinite++;
    else if (S < d->edge[0]) c->st.st_below++;
    else {
        int j = BINS - 1;
        while (j > 0 && !(d->edge[j] <= S)) j--;
        c->range_hist[j]++;
    }
}

/* x [n][2]: the station's next n frames.  features: bit 0 true peak, bit 1 range; the fields of a feature that is off stay as they are */
void meter_r128_process(const meter_ref_design_t* d, const meter_r128_tp_design_t* tp, unsigned features, meter_r128_chan* c, const float* x,
                        long long n) {
    /* the meter proper, fed up to each sub-block end so that the short-term value is taken where the device takes it; peak_call is per
     * call, so the pieces' maxima are folded (no peak is ever a NaN) */
    float pc[2] = {0.0f, 0.0f};
    long long f = 0;
    do {
        const long long to_end = (long long)d->nsb - (long long)(c->base.st.frames % (unsigned long long)d->nsb);
        const long long m = n - f < to_end ? n - f : to_end;
        const unsigned long long g = c->base.st.subblocks;
        meter_ref_process(d, &c->base, x + 2 * f, m);
        for (int r = 0; r < 2; r++) pc[r] = fmaxf(pc[r], c->base.st.peak_call[r]);
        if (c->base.st.subblocks != g && (features & 2u)) short_term_value(d, c, g);
        f += m;
    } while (f < n);
    for (int r = 0; r < 2; r++) c->base.st.peak_call[r] = pc[r];

    if (!(features & 1u)) return;
    for (int r = 0; r < 2; r++) {
        float w[TP_T];                 /* w[k] = x[i - k] */
        float tpc = 0.0f;
        for (int k = 1; k < TP_T; k++) w[k] = c->hist[r][TP_H - k];
        for (long long i = 0; i < n; i++) {
            w[0] = x[2 * i + r];
            tpc = fmaxf(tpc, fabsf(w[0]));
            for (int p = 1; p < tp->L; p++) {
                float y = 0.0f;
                for (int k = 0; k < TP_T; k++) y = fmaf(tp->taps[p - 1][k], w[k], y);
                tpc = fmaxf(tpc, fabsf(y));
            }
            for (int k = TP_T - 1; k >= 1; k--) w[k] = w[k - 1];
        }
        for (int k = 1; k < TP_T; k++) c->hist[r][TP_H - k] = w[k];
        c->st.tp_call[r] = tpc;
        c->st.tp_hold[r] = fmaxf(c->st.tp_hold[r], tpc);
    }
}

double meter_r128_dbtp(float peak) { return peak == 0.0f ? -INFINITY : 20.0 * log10((double)peak); }

/* 0, or -6 when no bin survives the gates */
int meter_r128_range(const unsigned* hist, const meter_ref_design_t* d, double* lra, double* low, double* high) {
    unsigned long long n0 = 0, n = 0, cum = 0;
    double s = 0.0, gate;
    int j10 = -1, j95 = -1;
    for (int j = 0; j < BINS; j++) { n0 += hist[j]; s += (double)hist[j] * d->centre[j]; }
    if (n0 == 0) return -6;
    gate = 0.01 * (s / (double)n0);
    for (int j = 0; j < BINS; j++)
        if (d->centre[j] >= gate) n += hist[j];
    if (n == 0) return -6;
    const unsigned long long r10 = (unsigned long long)floor(0.10 * (double)(n - 1) + 0.5);
    const unsigned long long r95 = (unsigned long long)floor(0.95 * (double)(n - 1) + 0.5);
    for (int j = 0; j < BINS; j++) {
        if (!(d->centre[j] >= gate)) continue;
        cum += hist[j];
        if (j10 < 0 && cum > r10) j10 = j;
        if (j95 < 0 && cum > r95) j95 = j;
    }
    *low = -70.0 + 0.1 * (double)j10 + 0.05;
    *high = -70.0 + 0.1 * (double)j95 + 0.05;
    *lra = (double)(j95 - j10) / 10.0;
    return 0;
}
