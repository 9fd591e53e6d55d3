/* The carrier squelch's arithmetic (include/fmdemod.h, "Carrier squelch") restated in plain C, one station at a time and one sample
 * after the other: what the tests compare fmd_squelch_* with, bit for bit.  Built with -ffp-contract=off -fno-fast-math: every operation
 * is the one written, and every multiply-add is an explicit fma(). */
#include <math.h>
#include <string.h>

#define NP 256
#define RING 20
#define MODE_AUTO 0
#define MODE_FORCE_OPEN 1
#define MODE_FORCE_CLOSED 2

typedef struct {                       /* the layout of fmd_squelch_params */
    double open_db, close_db, min_level_db;
    int    open_intervals, close_intervals, mode;
} squelch_ref_params;

typedef struct {                       /* the layout of fmd_squelch_status */
    unsigned long long samples, intervals, intervals_open;
    double   ring_s2[RING], ring_s4[RING];
    float    last_peak, hold_peak;
    unsigned run, transitions, nonfinite;
    unsigned char open, mode, reserved[2];
} squelch_ref_status;

typedef struct {
    squelch_ref_status st;
    squelch_ref_params prm;
    int      M;
    double   c_open, c_close, min_s2;
    float    pk;                       /* the open interval's */
    double   p[2][NP];                 /* s2, s4 partials of the open interval */
    unsigned char mask;                /* the station's mask byte as of the last call */
} squelch_ref_chan;

static int interval_of(int fs) { return fs < 192000 || fs > 384000 || fs % 1000 != 0 ? 0 : fs / 20; }

void squelch_ref_default_params(squelch_ref_params* p) {
    p->open_db = 10.0; p->close_db = 7.0; p->min_level_db = -INFINITY;
    p->open_intervals = 2; p->close_intervals = 10; p->mode = MODE_AUTO;
}

double squelch_ref_threshold(double db) {
    const double k = pow(10.0, db / 10.0);
    return (k * k) / ((1.0 + k) * (1.0 + k));
}

/* 0, or -1 for parameters outside their ranges (nothing changes then) */
int squelch_ref_set_params(squelch_ref_chan* c, const squelch_ref_params* p) {
    if (!(p->close_db >= 0.0 && p->close_db <= p->open_db && p->open_db <= 60.0)) return -1;
    if (!(p->min_level_db < INFINITY)) return -1;
    if (p->open_intervals < 1 || p->open_intervals > 1000 || p->close_intervals < 1 || p->close_intervals > 1000) return -1;
    if (p->mode != MODE_AUTO && p->mode != MODE_FORCE_OPEN && p->mode != MODE_FORCE_CLOSED) return -1;
    c->prm = *p;
    c->c_open = squelch_ref_threshold(p->open_db);
    c->c_close = squelch_ref_threshold(p->close_db);
    c->min_s2 = p->min_level_db == -INFINITY ? 0.0 : pow(10.0, p->min_level_db / 10.0) * (double)c->M;
    c->st.mode = (unsigned char)p->mode;
    return 0;
}

/* everything as after create; the parameters are kept */
void squelch_ref_reset(squelch_ref_chan* c) {
    memset(&c->st, 0, sizeof(c->st));
    memset(c->p, 0, sizeof(c->p));
    c->pk = 0.0f;
    c->st.mode = (unsigned char)c->prm.mode;
}

void squelch_ref_reset_peaks(squelch_ref_chan* c) { c->st.hold_peak = 0.0f; }

int squelch_ref_create(squelch_ref_chan* c, int fs) {
    memset(c, 0, sizeof(*c));
    c->M = interval_of(fs);
    if (c->M == 0) return -1;
    squelch_ref_params p;
    squelch_ref_default_params(&p);
    squelch_ref_set_params(c, &p);
    squelch_ref_reset(c);
    c->mask = 0xAA;                    /* no call has written it yet */
    return 0;
}

static void close_interval(squelch_ref_chan* c) {
    squelch_ref_status* st = &c->st;
    double S[2];
    for (int k = 0; k < 2; k++) {
        double* p = c->p[k];
        for (int w = NP / 2; w >= 1; w >>= 1)
            for (int j = 0; j < w; j++) p[j] += p[j + w];
        S[k] = p[0];
    }
    const double S2 = S[0], S4 = S[1];
    const int g = (int)(st->intervals % RING);
    st->ring_s2[g] = S2; st->ring_s4[g] = S4; st->last_peak = c->pk;
    st->intervals++;
    const int finite = isfinite(S2) && isfinite(S4);
    if (!finite) st->nonfinite++;
    const double a = S2 * S2;
    const double d = fma(-(double)c->M, S4, 2.0 * a);
    const int good_open = finite && S2 >= c->min_s2 && d > c->c_open * a;
    const int good_close = finite && S2 >= c->min_s2 && d > c->c_close * a;
    if (!st->open) {
        st->run = good_open ? st->run + 1 : 0;
        if (st->run >= (unsigned)c->prm.open_intervals) { st->open = 1; st->run = 0; st->transitions++; }
    } else {
        st->run = good_close ? 0 : st->run + 1;
        if (st->run >= (unsigned)c->prm.close_intervals) { st->open = 0; st->run = 0; st->transitions++; }
    }
    if (st->open) st->intervals_open++;
    memset(c->p, 0, sizeof(c->p));
    c->pk = 0.0f;
}

static void one_sample(squelch_ref_chan* c, float i, float q) {
    squelch_ref_status* st = &c->st;
    const unsigned long long na = st->samples;
    const unsigned long long r = na - st->intervals * (unsigned long long)c->M;
    const int j = (int)(r % NP);
    const double I = (double)i, Q = (double)q;
    const double p = fma(I, I, Q * Q);
    c->p[0][j] = c->p[0][j] + p;
    c->p[1][j] = fma(p, p, c->p[1][j]);
    const float m = fmaxf(fabsf(i), fabsf(q));
    c->pk = fmaxf(c->pk, m);
    st->hold_peak = fmaxf(st->hold_peak, m);
    st->samples = na + 1;
    if (r + 1 == (unsigned long long)c->M) close_interval(c);
}

static void write_mask(squelch_ref_chan* c) {
    c->mask = (unsigned char)(c->prm.mode == MODE_AUTO ? c->st.open : c->prm.mode == MODE_FORCE_OPEN);
}

/* iq [n][2] floats; n == 0 still writes the mask byte */
void squelch_ref_process_cf32(squelch_ref_chan* c, const float* iq, long long n) {
    for (long long s = 0; s < n; s++) one_sample(c, iq[2 * s], iq[2 * s + 1]);
    write_mask(c);
}

/* iq [n][2] bytes: (float)v - 127 */
void squelch_ref_process_u8(squelch_ref_chan* c, const unsigned char* iq, long long n) {
    for (long long s = 0; s < n; s++) one_sample(c, (float)iq[2 * s] - 127.0f, (float)iq[2 * s + 1] - 127.0f);
    write_mask(c);
}

/* e2, e4 over the newest `window` intervals, oldest first */
static int window_sums(const squelch_ref_status* s, int fs, int window, double* e2, double* e4, double* N) {
    const int M = interval_of(fs);
    if (M == 0 || window < 1 || window > RING) return -1;
    if (s->intervals < (unsigned long long)window) return -6;
    double a = 0.0, b = 0.0;
    for (unsigned long long g = s->intervals - (unsigned long long)window; g < s->intervals; g++) { a += s->ring_s2[g % RING]; b += s->ring_s4[g % RING]; }
    *e2 = a; *e4 = b; *N = (double)M * (double)window;
    return 0;
}

int squelch_ref_level_db(const squelch_ref_status* s, int fs, double* db) {
    double e2, e4, N;
    const int rc = window_sums(s, fs, 1, &e2, &e4, &N);
    if (rc) return rc;
    *db = 10.0 * log10(s->ring_s2[(s->intervals - 1) % RING] / N);
    return 0;
}

int squelch_ref_powers(const squelch_ref_status* s, int fs, int window, double* carrier, double* noise) {
    double e2, e4, N;
    const int rc = window_sums(s, fs, window, &e2, &e4, &N);
    if (rc) return rc;
    const double d = fma(-N, e4, 2.0 * e2 * e2);
    if (d <= 0.0) { *carrier = 0.0; *noise = e2 / N; return 0; }
    const double c = sqrt(d) / N;
    *carrier = c;
    *noise = e2 / N - c;
    return 0;
}

int squelch_ref_cnr_db(const squelch_ref_status* s, int fs, int window, double* db) {
    double e2, e4, N;
    const int rc = window_sums(s, fs, window, &e2, &e4, &N);
    if (rc) return rc;
    const double d = fma(-N, e4, 2.0 * e2 * e2);
    if (d <= 0.0) { *db = -INFINITY; return 0; }
    const double c = sqrt(d) / N;
    const double nz = e2 / N - c;
    *db = nz <= 0.0 ? INFINITY : 10.0 * log10(c / nz);
    return 0;
}
