/* The loudness meter's arithmetic (include/fmdemod.h, "Batched loudness meter") restated in plain C, one station at a time and one frame
 * after the other: what the tests compare fmd_meter_* with, bit for bit.  Built with -ffp-contract=off -fno-fast-math: every operation
 * is the one written, and every multiply-add of the filters is an explicit fma(). */
#include <math.h>
#include <string.h>

#define BINS 1000
#define RING 30

typedef struct {
    double pre_b[3], pre_a[3], rlb_b[3], rlb_a[3];
    int    nsb;
    double edge[BINS + 1], centre[BINS];
} meter_ref_design_t;

typedef struct {                       /* the layout of fmd_meter_status */
    unsigned long long frames, subblocks;
    double   energy_ring[RING];
    float    peak_call[2], peak_hold[2];
    unsigned below_gate, nonfinite;
} meter_ref_status;

typedef struct {
    meter_ref_status st;
    double   s1[2], s2[2], t1[2], t2[2], acc[2];   /* per rail */
    unsigned hist[BINS];
} meter_ref_chan;

int meter_ref_design(int fs, meter_ref_design_t* d) {
    const double pi = 3.14159265358979323846;
    volatile double ten = 10.0;        /* read at run time: libm's pow, not a constant the compiler folded */
    if (fs < 8000 || fs > 192000 || fs % 10 != 0) return -1;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(pi * f0 / (double)fs);
        const double Vh = pow(ten, G / 20.0);
        const double Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        d->pre_b[0] = (Vh + Vb * K / Q + K * K) / a0;
        d->pre_b[1] = 2.0 * (K * K - Vh) / a0;
        d->pre_b[2] = (Vh - Vb * K / Q + K * K) / a0;
        d->pre_a[0] = 1.0;
        d->pre_a[1] = 2.0 * (K * K - 1.0) / a0;
        d->pre_a[2] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(pi * f0 / (double)fs);
        const double a0 = 1.0 + K / Q + K * K;
        d->rlb_b[0] = 1.0; d->rlb_b[1] = -2.0; d->rlb_b[2] = 1.0;
        d->rlb_a[0] = 1.0;
        d->rlb_a[1] = 2.0 * (K * K - 1.0) / a0;
        d->rlb_a[2] = (1.0 - K / Q + K * K) / a0;
    }
    d->nsb = fs / 10;
    for (int j = 0; j <= BINS; j++) d->edge[j] = pow(ten, ((-70.0 + 0.1 * (double)j) + 0.691) / 10.0);
    for (int j = 0; j < BINS; j++) d->centre[j] = pow(ten, (((-70.0 + 0.1 * (double)j) + 0.05) + 0.691) / 10.0);
    return 0;
}

void meter_ref_reset(meter_ref_chan* c) { memset(c, 0, sizeof(*c)); }

void meter_ref_reset_peaks(meter_ref_chan* c) {
    for (int r = 0; r < 2; r++) c->st.peak_call[r] = c->st.peak_hold[r] = 0.0f;
}

static void end_of_subblock(const meter_ref_design_t* d, meter_ref_chan* c) {
    const unsigned long long g = c->st.subblocks;
    const double E = (c->acc[0] + c->acc[1]) / (double)d->nsb;
    double* ring = c->st.energy_ring;
    ring[g % RING] = E;
    if (g >= 3) {
        const double B = (((ring[(g - 3) % RING] + ring[(g - 2) % RING]) + ring[(g - 1) % RING]) + E) * 0.25;
        if (!isfinite(B)) c->st.nonfinite++;
        else if (B < d->edge[0]) c->st.below_gate++;
        else {
            int j = BINS - 1;
            while (j > 0 && !(d->edge[j] <= B)) j--;      /* the j with edge[j] <= B < edge[j + 1]; B >= edge[1000] -> 999 */
            c->hist[j]++;
        }
    }
    c->st.subblocks = g + 1;
    c->acc[0] = c->acc[1] = 0.0;
}

/* x [n][2]: the station's next n frames */
void meter_ref_process(const meter_ref_design_t* d, meter_ref_chan* c, const float* x, long long n) {
    const double pb0 = d->pre_b[0], pb1 = d->pre_b[1], pb2 = d->pre_b[2], pa1 = d->pre_a[1], pa2 = d->pre_a[2];
    const double rb0 = d->rlb_b[0], rb1 = d->rlb_b[1], rb2 = d->rlb_b[2], ra1 = d->rlb_a[1], ra2 = d->rlb_a[2];
    c->st.peak_call[0] = c->st.peak_call[1] = 0.0f;
    for (long long f = 0; f < n; f++) {
        for (int r = 0; r < 2; r++) {
            const float xf = x[2 * f + r];
            const double v = (double)xf;
            const double o1 = fma(pb0, v, c->s1[r]);
            c->s1[r] = fma(-pa1, o1, fma(pb1, v, c->s2[r]));
            c->s2[r] = fma(-pa2, o1, pb2 * v);
            const double o2 = fma(rb0, o1, c->t1[r]);
            c->t1[r] = fma(-ra1, o2, fma(rb1, o1, c->t2[r]));
            c->t2[r] = fma(-ra2, o2, rb2 * o1);
            c->acc[r] = fma(o2, o2, c->acc[r]);
            c->st.peak_call[r] = fmaxf(c->st.peak_call[r], fabsf(xf));
            c->st.peak_hold[r] = fmaxf(c->st.peak_hold[r], fabsf(xf));
        }
        c->st.frames++;
        if (c->st.frames % (unsigned long long)d->nsb == 0) end_of_subblock(d, c);
    }
}

double meter_ref_lufs(double e) { return e == 0.0 ? -INFINITY : -0.691 + 10.0 * log10(e); }

int meter_ref_momentary(const meter_ref_status* s, double* lufs) {
    const unsigned long long G = s->subblocks;
    const double* e = s->energy_ring;
    if (G < 4) return -6;
    *lufs = meter_ref_lufs((((e[(G - 4) % RING] + e[(G - 3) % RING]) + e[(G - 2) % RING]) + e[(G - 1) % RING]) / 4.0);
    return 0;
}

int meter_ref_short_term(const meter_ref_status* s, double* lufs) {
    double sum = 0.0;
    if (s->subblocks < RING) return -6;
    for (unsigned long long g = s->subblocks - RING; g < s->subblocks; g++) sum += s->energy_ring[g % RING];
    *lufs = meter_ref_lufs(sum / 30.0);
    return 0;
}

double meter_ref_integrated(const unsigned* hist, const meter_ref_design_t* d) {
    unsigned long long n = 0, nk = 0;
    double s = 0.0, sk = 0.0, gate;
    for (int j = 0; j < BINS; j++) { n += hist[j]; s += (double)hist[j] * d->centre[j]; }
    if (n == 0) return -INFINITY;
    gate = 0.1 * (s / (double)n);
    for (int j = 0; j < BINS; j++)
        if (d->centre[j] >= gate) { nk += hist[j]; sk += (double)hist[j] * d->centre[j]; }
    return nk == 0 ? -INFINITY : meter_ref_lufs(sk / (double)nk);
}
