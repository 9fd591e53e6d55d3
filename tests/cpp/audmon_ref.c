/* The audio fault monitor's arithmetic (include/fmdemod.h, "Audio fault monitor") restated in plain C, one station at a time and one
 * frame after the other: what the tests compare fmd_audmon_* with, bit for bit.  Built with -ffp-contract=off -fno-fast-math: every
 * operation is the one written, and every multiply-add is an explicit fma(). */
#include <math.h>
#include <string.h>

#define NP 64
#define RING 30
#define ND 5

typedef struct {                       /* the layout of fmd_audmon_params */
    double   silence_db, loss_db, antiphase_corr, mono_db;
    int      raise_intervals[ND], clear_intervals[ND];
    unsigned alarm_mask;
} audmon_ref_params;

typedef struct {                       /* the layout of fmd_audmon_status */
    unsigned long long frames, intervals, intervals_flagged[ND];
    double   ring_ll[RING], ring_rr[RING], ring_lr[RING];
    float    last_peak[2], hold_peak[2];
    unsigned run[ND], transitions[ND], nonfinite;
    unsigned char flags, ok, reserved[2];
} audmon_ref_status;

typedef struct {
    audmon_ref_status st;
    audmon_ref_params prm;
    int      M;
    double   min_e, c_loss, c_anti, c_mono;
    float    pk[2];                    /* the open interval's */
    double   p[3][NP];                 /* ll, rr, lr partials of the open interval */
    unsigned char out_flags, out_ok;   /* the station's two bytes as of the last call */
} audmon_ref_chan;

static int interval_of(int fs) { return fs < 8000 || fs > 192000 || fs % 10 != 0 ? 0 : fs / 10; }

void audmon_ref_default_params(audmon_ref_params* p) {
    static const int raise[ND] = {100, 100, 100, 50, 100};
    memset(p, 0, sizeof(*p));
    p->silence_db = -60.0; p->loss_db = 30.0; p->antiphase_corr = 0.5; p->mono_db = 40.0;
    for (int k = 0; k < ND; k++) { p->raise_intervals[k] = raise[k]; p->clear_intervals[k] = 10; }
    p->alarm_mask = 15u;
}

/* 0, or -1 for parameters outside their ranges (nothing changes then) */
int audmon_ref_set_params(audmon_ref_chan* c, const audmon_ref_params* p) {
    if (!(p->silence_db < INFINITY)) return -1;
    if (!(p->loss_db > 0.0 && p->loss_db <= 120.0)) return -1;
    if (!(p->antiphase_corr > 0.0 && p->antiphase_corr < 1.0)) return -1;
    if (!(p->mono_db > 0.0 && p->mono_db <= 120.0)) return -1;
    for (int k = 0; k < ND; k++)
        if (p->raise_intervals[k] < 1 || p->raise_intervals[k] > 36000 || p->clear_intervals[k] < 1 || p->clear_intervals[k] > 36000) return -1;
    if (p->alarm_mask > 31u) return -1;
    c->prm = *p;
    c->min_e = p->silence_db == -INFINITY ? 0.0 : pow(10.0, p->silence_db / 10.0) * (2.0 * (double)c->M);
    c->c_loss = pow(10.0, -p->loss_db / 10.0);
    c->c_anti = p->antiphase_corr * p->antiphase_corr;
    c->c_mono = pow(10.0, -p->mono_db / 10.0);
    c->st.ok = (unsigned char)((c->st.flags & p->alarm_mask) == 0);
    return 0;
}

/* everything as after create; the parameters are kept */
void audmon_ref_reset(audmon_ref_chan* c) {
    memset(&c->st, 0, sizeof(c->st));
    memset(c->p, 0, sizeof(c->p));
    c->pk[0] = c->pk[1] = 0.0f;
    c->st.ok = 1;
}

void audmon_ref_reset_peaks(audmon_ref_chan* c) { c->st.hold_peak[0] = c->st.hold_peak[1] = 0.0f; }

int audmon_ref_create(audmon_ref_chan* c, int fs) {
    memset(c, 0, sizeof(*c));
    c->M = interval_of(fs);
    if (c->M == 0) return -1;
    audmon_ref_params p;
    audmon_ref_default_params(&p);
    audmon_ref_reset(c);
    audmon_ref_set_params(c, &p);
    c->out_flags = c->out_ok = 0xAA;   /* no call has written them yet */
    return 0;
}

static void detector(audmon_ref_chan* c, int k, int bad) {
    audmon_ref_status* st = &c->st;
    const unsigned char bit = (unsigned char)(1u << k);
    if (!(st->flags & bit)) {
        st->run[k] = bad ? st->run[k] + 1 : 0;
        if (st->run[k] >= (unsigned)c->prm.raise_intervals[k]) { st->flags |= bit; st->run[k] = 0; st->transitions[k]++; }
    } else {
        st->run[k] = bad ? 0 : st->run[k] + 1;
        if (st->run[k] >= (unsigned)c->prm.clear_intervals[k]) { st->flags &= (unsigned char)~bit; st->run[k] = 0; st->transitions[k]++; }
    }
}

static void close_interval(audmon_ref_chan* c) {
    audmon_ref_status* st = &c->st;
    double S[3];
    for (int k = 0; k < 3; k++) {
        double* p = c->p[k];
        for (int w = NP / 2; w >= 1; w >>= 1)
            for (int j = 0; j < w; j++) p[j] += p[j + w];
        S[k] = p[0];
    }
    const double LL = S[0], RR = S[1], LR = S[2];
    const int g = (int)(st->intervals % RING);
    st->ring_ll[g] = LL; st->ring_rr[g] = RR; st->ring_lr[g] = LR;
    st->last_peak[0] = c->pk[0]; st->last_peak[1] = c->pk[1];
    st->intervals++;
    const int finite = isfinite(LL) && isfinite(RR) && isfinite(LR);
    if (!finite) st->nonfinite++;
    const double E = LL + RR;
    const int silent = !(finite && E > c->min_e);
    detector(c, 0, silent);
    if (!silent) {                     /* silent: detectors 1 ... 4 hold */
        const double Sd = fma(-2.0, LR, E), Md = fma(2.0, LR, E);
        detector(c, 1, LL < c->c_loss * RR);
        detector(c, 2, RR < c->c_loss * LL);
        detector(c, 3, LR < 0.0 && LR * LR > c->c_anti * (LL * RR));
        detector(c, 4, Sd < c->c_mono * Md);
    }
    for (int k = 0; k < ND; k++)
        if (st->flags & (1u << k)) st->intervals_flagged[k]++;
    memset(c->p, 0, sizeof(c->p));
    c->pk[0] = c->pk[1] = 0.0f;
}

static void one_frame(audmon_ref_chan* c, float L, float R) {
    audmon_ref_status* st = &c->st;
    const unsigned long long na = st->frames;
    const unsigned long long r = na - st->intervals * (unsigned long long)c->M;
    const int j = (int)((r >> 2) & 63);
    const double l = (double)L, r_ = (double)R;
    c->p[0][j] = fma(l, l, c->p[0][j]);
    c->p[1][j] = fma(r_, r_, c->p[1][j]);
    c->p[2][j] = fma(l, r_, c->p[2][j]);
    c->pk[0] = fmaxf(c->pk[0], fabsf(L));
    c->pk[1] = fmaxf(c->pk[1], fabsf(R));
    st->hold_peak[0] = fmaxf(st->hold_peak[0], fabsf(L));
    st->hold_peak[1] = fmaxf(st->hold_peak[1], fabsf(R));
    st->frames = na + 1;
    if (r + 1 == (unsigned long long)c->M) close_interval(c);
}

/* x [n][2] floats (L, R); n == 0 still writes the two bytes */
void audmon_ref_process(audmon_ref_chan* c, const float* x, long long n) {
    for (long long s = 0; s < n; s++) one_frame(c, x[2 * s], x[2 * s + 1]);
    c->st.ok = (unsigned char)((c->st.flags & c->prm.alarm_mask) == 0);
    c->out_flags = c->st.flags;
    c->out_ok = c->st.ok;
}

/* ll, rr, lr over the newest `window` intervals, oldest first */
static int window_sums(const audmon_ref_status* s, int fs, int window, double* ll, double* rr, double* lr, double* N) {
    const int M = interval_of(fs);
    if (M == 0 || window < 1 || window > RING) return -1;
    if (s->intervals < (unsigned long long)window) return -6;
    double a = 0.0, b = 0.0, d = 0.0;
    for (unsigned long long g = s->intervals - (unsigned long long)window; g < s->intervals; g++) {
        a += s->ring_ll[g % RING]; b += s->ring_rr[g % RING]; d += s->ring_lr[g % RING];
    }
    *ll = a; *rr = b; *lr = d; *N = (double)M * (double)window;
    return 0;
}

int audmon_ref_level_db(const audmon_ref_status* s, int fs, int rail, int window, double* db) {
    double ll, rr, lr, N;
    if (rail < 0 || rail > 2) return -1;
    const int rc = window_sums(s, fs, window, &ll, &rr, &lr, &N);
    if (rc) return rc;
    *db = rail == 0 ? 10.0 * log10(ll / N) : rail == 1 ? 10.0 * log10(rr / N) : 10.0 * log10((ll + rr) / (2.0 * N));
    return 0;
}

int audmon_ref_balance_db(const audmon_ref_status* s, int fs, int window, double* db) {
    double ll, rr, lr, N;
    const int rc = window_sums(s, fs, window, &ll, &rr, &lr, &N);
    if (rc) return rc;
    *db = 10.0 * log10(ll / rr);
    return 0;
}

int audmon_ref_correlation(const audmon_ref_status* s, int fs, int window, double* corr) {
    double ll, rr, lr, N;
    const int rc = window_sums(s, fs, window, &ll, &rr, &lr, &N);
    if (rc) return rc;
    *corr = lr / sqrt(ll * rr);
    return 0;
}

int audmon_ref_side_mid_db(const audmon_ref_status* s, int fs, int window, double* db) {
    double ll, rr, lr, N;
    const int rc = window_sums(s, fs, window, &ll, &rr, &lr, &N);
    if (rc) return rc;
    *db = 10.0 * log10(fma(-2.0, lr, ll + rr) / fma(2.0, lr, ll + rr));
    return 0;
}
