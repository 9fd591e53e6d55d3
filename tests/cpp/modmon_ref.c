/* The FM modulation monitor's arithmetic (include/fmdemod.h, "FM modulation monitor") restated in plain C, one station at a time and one
 * sample after the other: what the tests compare fmd_modmon_* with, bit for bit.  Built with -ffp-contract=off -fno-fast-math: every
 * operation is the one written, and every multiply-add is an explicit fma() or fmaf(). */
#include <math.h>
#include <string.h>

#define TAPS 33
#define NP 64
#define BINS 300
#define RING 60
#define MAXP 384

typedef struct {                       /* the layout of fmd_modmon_design_t */
    int    fs, M, P, reserved;
    double hz_per_rad, pilot_gain;
    float  h[TAPS], reserved_f;
    double pilot_cos[MAXP], pilot_sin[MAXP];
    double edge[BINS + 1];
} modmon_ref_design_t;

typedef struct {                       /* the layout of fmd_modmon_status */
    unsigned long long samples, intervals, seconds;
    float    last_hi, last_lo, hold_hi, hold_lo;
    double   last_s1, last_s2, last_sc, last_ss;
    double   sec_e[RING], sec_f[RING], sec_q[RING];
    unsigned sec_n[RING];
    double   open_e, open_f, open_q;
    unsigned open_n, over, nonfinite, reserved;
} modmon_ref_status;

typedef struct {
    modmon_ref_status st;
    float    theta;                    /* theta[n - 1] */
    float    d[TAPS];                  /* d[n - k] at [k] */
    float    hi, lo;                   /* the open interval's */
    double   p[4][NP];                 /* s1, s2, sc, ss partials of the open interval */
    unsigned hist[BINS];
} modmon_ref_chan;

static double i0(double x) {
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 64; k++) { term *= (x / (2.0 * k)) * (x / (2.0 * k)); sum += term; if (term < 1e-18 * sum) break; }
    return sum;
}

static double sinc(double x) {
    const double pi = 3.14159265358979323846;
    return x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
}

int modmon_ref_design(int fs, modmon_ref_design_t* d) {
    const double pi = 3.14159265358979323846;
    if (fs < 192000 || fs > 384000 || fs % 1000 != 0) return -1;
    memset(d, 0, sizeof(*d));
    int a = fs, b = 19000;
    while (b) { const int t = a % b; a = b; b = t; }
    d->fs = fs;
    d->M = fs / 20;
    d->P = fs / a;
    d->hz_per_rad = (double)fs / (2.0 * pi);
    {
        const double w = 2.0 * 76000.0 / (double)fs, i0b = i0(5.0);
        double g[TAPS], sum = 0.0;
        for (int i = 0; i < TAPS; i++) {
            const double x = w * (double)(i - 16), r = (double)(i - 16) / 16.0;
            g[i] = ((w * sinc(x)) * i0(5.0 * sqrt(1.0 - r * r))) / i0b;
            sum += g[i];
        }
        for (int i = 0; i < TAPS; i++) d->h[i] = (float)(g[i] / sum);
    }
    for (int k = 0; k < d->P; k++) {
        const long long m = (19000LL * k) % fs;
        const double ang = (2.0 * pi * (double)m) / (double)fs;
        d->pilot_cos[k] = cos(ang);
        d->pilot_sin[k] = sin(ang);
    }
    {
        double re = 0.0, im = 0.0;
        for (int i = 0; i < TAPS; i++) {
            const double ang = (2.0 * pi * (double)(19000 * i)) / (double)fs;
            re += (double)d->h[i] * cos(ang);
            im += (double)d->h[i] * sin(ang);
        }
        d->pilot_gain = sqrt(re * re + im * im) * sinc(19000.0 / (double)fs);
    }
    for (int j = 0; j <= BINS; j++) d->edge[j] = 500.0 * (double)j;
    return 0;
}

static void open_interval(modmon_ref_chan* c) {
    c->hi = -INFINITY;
    c->lo = INFINITY;
    memset(c->p, 0, sizeof(c->p));
}

void modmon_ref_reset(modmon_ref_chan* c) {
    memset(c, 0, sizeof(*c));
    c->st.hold_hi = -INFINITY;
    c->st.hold_lo = INFINITY;
    open_interval(c);
}

void modmon_ref_reset_peaks(modmon_ref_chan* c) {
    c->st.hold_hi = -INFINITY;
    c->st.hold_lo = INFINITY;
}

static float wrapf(float x) {
    const float pi = (float)3.14159265358979323846;
    if (x >= pi) return x - 2.0f * pi;
    if (x <= -pi) return x + 2.0f * pi;
    return x;
}

static void close_interval(const modmon_ref_design_t* d, modmon_ref_chan* c) {
    modmon_ref_status* st = &c->st;
    double S[4];
    for (int k = 0; k < 4; k++) {
        double* p = c->p[k];
        for (int w = NP / 2; w >= 1; w >>= 1)
            for (int j = 0; j < w; j++) p[j] += p[j + w];
        S[k] = p[0];
    }
    const double D = 0.5 * ((double)c->hi - (double)c->lo) * d->hz_per_rad;
    st->last_hi = c->hi; st->last_lo = c->lo;
    st->last_s1 = S[0]; st->last_s2 = S[1]; st->last_sc = S[2]; st->last_ss = S[3];
    st->intervals++;
    if (!(fabs(D) <= 1.7976931348623157e308) || !(fabs(S[1]) <= 1.7976931348623157e308)) st->nonfinite++;
    else {
        if (D >= d->edge[BINS]) st->over++;
        else {
            int j = 0;
            while (!(D < d->edge[j + 1])) j++;
            c->hist[j]++;
        }
        st->open_e += S[1];
        st->open_f += S[0];
        st->open_q += fma(S[2], S[2], S[3] * S[3]);
        st->open_n += 1;
    }
    if (st->intervals % 20 == 0) {
        const int s = (int)(st->seconds % RING);
        st->sec_e[s] = st->open_e; st->sec_f[s] = st->open_f; st->sec_q[s] = st->open_q; st->sec_n[s] = st->open_n;
        st->seconds++;
        st->open_e = 0.0; st->open_f = 0.0; st->open_q = 0.0; st->open_n = 0;
    }
    open_interval(c);
}

/* iq [n][2] floats */
void modmon_ref_process_cf32(const modmon_ref_design_t* d, modmon_ref_chan* c, const float* iq, long long n) {
    modmon_ref_status* st = &c->st;
    for (long long s = 0; s < n; s++) {
        const unsigned long long na = st->samples;
        const float theta = atan2f(iq[2 * s + 1], iq[2 * s]);
        const float dn = na == 0 ? 0.0f : wrapf(theta - c->theta);
        c->theta = theta;
        for (int k = TAPS - 1; k >= 1; k--) c->d[k] = c->d[k - 1];
        c->d[0] = dn;
        float y = 0.0f;
        for (int t = 0; t < TAPS; t++) y = fmaf(d->h[t], c->d[t], y);
        c->hi = fmaxf(c->hi, y);
        c->lo = fminf(c->lo, y);
        st->hold_hi = fmaxf(st->hold_hi, y);
        st->hold_lo = fminf(st->hold_lo, y);
        const double fd = (double)y * d->hz_per_rad;
        const unsigned long long r = na - st->intervals * (unsigned long long)d->M;
        const int j = (int)(r % NP), k = (int)(na % (unsigned long long)d->P);
        c->p[0][j] = c->p[0][j] + fd;
        c->p[1][j] = fma(fd, fd, c->p[1][j]);
        c->p[2][j] = fma(fd, d->pilot_cos[k], c->p[2][j]);
        c->p[3][j] = fma(fd, d->pilot_sin[k], c->p[3][j]);
        st->samples = na + 1;
        if (r + 1 == (unsigned long long)d->M) close_interval(d, c);
    }
}

/* iq [n][2] bytes: (float)v - 127 */
void modmon_ref_process_u8(const modmon_ref_design_t* d, modmon_ref_chan* c, const unsigned char* iq, long long n) {
    for (long long s = 0; s < n; s++) {
        const float v[2] = {(float)iq[2 * s] - 127.0f, (float)iq[2 * s + 1] - 127.0f};
        modmon_ref_process_cf32(d, c, v, 1);
    }
}

int modmon_ref_deviation_hz(const modmon_ref_status* s, const modmon_ref_design_t* d, double* hz) {
    if (s->intervals == 0) return -6;
    *hz = 0.5 * ((double)s->last_hi - (double)s->last_lo) * d->hz_per_rad;
    return 0;
}

int modmon_ref_offset_hz(const modmon_ref_status* s, const modmon_ref_design_t* d, double* hz) {
    if (s->intervals == 0) return -6;
    *hz = s->last_s1 / (double)d->M;
    return 0;
}

int modmon_ref_pilot_hz(const modmon_ref_status* s, const modmon_ref_design_t* d, double* hz) {
    if (s->intervals == 0) return -6;
    *hz = 2.0 * sqrt(fma(s->last_sc, s->last_sc, s->last_ss * s->last_ss)) / (double)d->M / d->pilot_gain;
    return 0;
}

int modmon_ref_mpx_power_dbr(const modmon_ref_status* s, const modmon_ref_design_t* d, int window_s, double* dbr) {
    if (window_s < 1 || window_s > RING) return -1;
    if (s->seconds < (unsigned long long)window_s) return -6;
    double e = 0.0, f = 0.0;
    unsigned long long k = 0;
    for (unsigned long long t = s->seconds - (unsigned long long)window_s; t < s->seconds; t++) {
        e += s->sec_e[t % RING];
        f += s->sec_f[t % RING];
        k += s->sec_n[t % RING];
    }
    if (k == 0) return -6;
    const double N = (double)d->M * (double)k;
    const double v = e / N - (f / N) * (f / N);
    *dbr = v <= 0.0 ? -INFINITY : 10.0 * log10(2.0 * v / (19000.0 * 19000.0));
    return 0;
}

int modmon_ref_exceedance(const unsigned* hist, unsigned over, int limit_hz, double* fraction, unsigned long long* count) {
    if (limit_hz < 0 || limit_hz > 150000 || limit_hz % 500 != 0) return -1;
    unsigned long long n = over, c = over;
    for (int j = 0; j < BINS; j++) {
        n += hist[j];
        if (j >= limit_hz / 500) c += hist[j];
    }
    if (n == 0) return -6;
    *count = c;
    *fraction = (double)c / (double)n;
    return 0;
}

int modmon_ref_percentile(const unsigned* hist, unsigned over, double q, double* hz) {
    if (!(q >= 0.0 && q <= 1.0)) return -1;
    unsigned long long n = over;
    for (int j = 0; j < BINS; j++) n += hist[j];
    if (n == 0) return -6;
    const unsigned long long rank = (unsigned long long)floor(q * (double)(n - 1) + 0.5);
    unsigned long long cum = 0;
    for (int j = 0; j < BINS; j++) {
        cum += hist[j];
        if (cum > rank) { *hz = 500.0 * (double)j + 250.0; return 0; }
    }
    *hz = 150000.0;
    return 0;
}
