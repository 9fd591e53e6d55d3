/* The audio tone detector's arithmetic (include/fmdemod.h, "Audio tone detector") restated in plain C, one station at a time and one
 * frame after the other: what the tests compare fmd_tonedet_* with, bit for bit.  Built with -ffp-contract=off -fno-fast-math: every
 * operation is the one written, and every multiply-add is an explicit fma(). */
#define _DEFAULT_SOURCE                /* M_PI under -std=c99 */
#include <math.h>
#include <string.h>

#define NP 64
#define RING 30
#define NS 8
#define NSUM (1 + 2 * NS)

typedef struct {                       /* the layout of fmd_tonedet_params */
    int      freq_hz[NS];
    double   share_db[NS], floor_db;
    int      raise_intervals[NS], clear_intervals[NS];
    unsigned alarm_mask;
} tonedet_ref_params;

typedef struct {                       /* the layout of fmd_tonedet_status */
    unsigned long long frames, intervals, intervals_flagged[NS];
    double   ring_mm[RING], ring_pw[NS][RING];
    unsigned run[NS], transitions[NS], nonfinite;
    int      freq_hz[NS];              /* in force */
    unsigned char flags, ok, reserved[2];
} tonedet_ref_status;

typedef struct {
    tonedet_ref_status st;
    tonedet_ref_params prm;            /* prm.freq_hz is pending until an interval starts */
    int      fs, M;
    const double* tab;                 /* [fs][2]: tc, ts (the caller's, from tonedet_ref_table) */
    double   min_e, c[NS];
    double   p[NSUM][NP];              /* the open interval's partials: mm, then re and im of slot 0, 1, ... */
    unsigned char out_flags, out_ok;   /* the station's two bytes as of the last call */
} tonedet_ref_chan;

static int interval_of(int fs) { return fs < 8000 || fs > 48000 || fs % 10 != 0 ? 0 : fs / 10; }

/* libm's cos and libm's sin, each called on its own: a compiler that sees both on one argument makes them one sincos(), whose results
 * are not everywhere the bits of the two */
__attribute__((noinline)) static double table_cos(double a) { return cos(a); }
__attribute__((noinline)) static double table_sin(double a) { return sin(a); }

/* tab [fs][2] */
void tonedet_ref_table(int fs, double* tab) {
    for (int j = 0; j < fs; j++) {
        tab[2 * j] = table_cos(2.0 * M_PI * (double)j / (double)fs);
        tab[2 * j + 1] = table_sin(2.0 * M_PI * (double)j / (double)fs);
    }
}

void tonedet_ref_default_params(tonedet_ref_params* p) {
    static const int freq[NS] = {1000, 440, 400, 853, 960, 1050, 0, 0};
    static const double share[NS] = {3.0, 3.0, 3.0, 6.0, 6.0, 3.0, 3.0, 3.0};
    memset(p, 0, sizeof(*p));
    for (int k = 0; k < NS; k++) { p->freq_hz[k] = freq[k]; p->share_db[k] = share[k]; p->raise_intervals[k] = 20; p->clear_intervals[k] = 5; }
    p->floor_db = -50.0;
    p->alarm_mask = 0u;
}

/* 0, or -1 for parameters outside their ranges (nothing changes then) */
int tonedet_ref_set_params(tonedet_ref_chan* c, const tonedet_ref_params* p) {
    for (int k = 0; k < NS; k++) {
        const int f = p->freq_hz[k];
        if (f != 0 && (f < 1 || 2LL * f >= (long long)c->fs)) return -1;
        if (!(p->share_db[k] >= 0.0 && p->share_db[k] <= 60.0)) return -1;
        if (p->raise_intervals[k] < 1 || p->raise_intervals[k] > 36000 || p->clear_intervals[k] < 1 || p->clear_intervals[k] > 36000) return -1;
    }
    if (!(p->floor_db < INFINITY)) return -1;
    if (p->alarm_mask > 255u) return -1;
    c->prm = *p;
    c->min_e = p->floor_db == -INFINITY ? 0.0 : pow(10.0, p->floor_db / 10.0) * (double)c->M;
    for (int k = 0; k < NS; k++) c->c[k] = pow(10.0, -p->share_db[k] / 10.0);
    if (c->st.frames == c->st.intervals * (unsigned long long)c->M)        /* no interval is open: the next one starts on these */
        for (int k = 0; k < NS; k++) c->st.freq_hz[k] = p->freq_hz[k];
    c->st.ok = (unsigned char)((c->st.flags & p->alarm_mask) == 0);
    return 0;
}

/* everything as after create; the parameters are kept, and their frequencies come into force */
void tonedet_ref_reset(tonedet_ref_chan* c) {
    memset(&c->st, 0, sizeof(c->st));
    memset(c->p, 0, sizeof(c->p));
    for (int k = 0; k < NS; k++) c->st.freq_hz[k] = c->prm.freq_hz[k];
    c->st.ok = 1;
}

int tonedet_ref_create(tonedet_ref_chan* c, int fs, const double* tab) {
    memset(c, 0, sizeof(*c));
    c->fs = fs;
    c->M = interval_of(fs);
    c->tab = tab;
    if (c->M == 0) return -1;
    tonedet_ref_params p;
    tonedet_ref_default_params(&p);
    tonedet_ref_reset(c);
    tonedet_ref_set_params(c, &p);
    c->out_flags = c->out_ok = 0xAA;   /* no call has written them yet */
    return 0;
}

static void detector(tonedet_ref_chan* c, int k, int present) {
    tonedet_ref_status* st = &c->st;
    const unsigned char bit = (unsigned char)(1u << k);
    if (!(st->flags & bit)) {
        st->run[k] = present ? st->run[k] + 1 : 0;
        if (st->run[k] >= (unsigned)c->prm.raise_intervals[k]) { st->flags |= bit; st->run[k] = 0; st->transitions[k]++; }
    } else {
        st->run[k] = present ? 0 : st->run[k] + 1;
        if (st->run[k] >= (unsigned)c->prm.clear_intervals[k]) { st->flags &= (unsigned char)~bit; st->run[k] = 0; st->transitions[k]++; }
    }
}

static void close_interval(tonedet_ref_chan* c) {
    tonedet_ref_status* st = &c->st;
    double S[NSUM];
    for (int q = 0; q < NSUM; q++) {
        double* p = c->p[q];
        for (int w = NP / 2; w >= 1; w >>= 1)
            for (int j = 0; j < w; j++) p[j] += p[j + w];
        S[q] = p[0];
    }
    const double MM = S[0];
    const int g = (int)(st->intervals % RING);
    st->ring_mm[g] = MM;
    st->intervals++;
    if (!isfinite(MM)) st->nonfinite++;
    const int usable = isfinite(MM) && MM > c->min_e;
    for (int k = 0; k < NS; k++) {
        const double RE = S[1 + 2 * k], IM = S[2 + 2 * k];
        const double PW = st->freq_hz[k] != 0 ? fma(RE, RE, IM * IM) : 0.0;
        st->ring_pw[k][g] = PW;
        const int present = st->freq_hz[k] != 0 && usable && isfinite(PW) && 2.0 * PW > c->c[k] * ((double)c->M * MM);
        detector(c, k, present);
    }
    for (int k = 0; k < NS; k++)
        if (st->flags & (1u << k)) st->intervals_flagged[k]++;
    memset(c->p, 0, sizeof(c->p));
    for (int k = 0; k < NS; k++) st->freq_hz[k] = c->prm.freq_hz[k];      /* the next interval starts on the pending frequencies */
}

static void one_frame(tonedet_ref_chan* c, float L, float R) {
    tonedet_ref_status* st = &c->st;
    const unsigned long long na = st->frames;
    const unsigned long long r = na - st->intervals * (unsigned long long)c->M;
    const int j = (int)((r >> 2) & 63);
    const double m = (double)L + (double)R;
    c->p[0][j] = fma(m, m, c->p[0][j]);
    for (int k = 0; k < NS; k++) {
        const int f = st->freq_hz[k];
        if (f == 0) continue;
        const int idx = (int)(((long long)f * (long long)r) % (long long)c->fs);
        c->p[1 + 2 * k][j] = fma(m, c->tab[2 * idx], c->p[1 + 2 * k][j]);
        c->p[2 + 2 * k][j] = fma(m, c->tab[2 * idx + 1], c->p[2 + 2 * k][j]);
    }
    st->frames = na + 1;
    if (r + 1 == (unsigned long long)c->M) close_interval(c);
}

/* x [n][2] floats (L, R); n == 0 still writes the two bytes */
void tonedet_ref_process(tonedet_ref_chan* c, const float* x, long long n) {
    for (long long s = 0; s < n; s++) one_frame(c, x[2 * s], x[2 * s + 1]);
    c->st.ok = (unsigned char)((c->st.flags & c->prm.alarm_mask) == 0);
    c->out_flags = c->st.flags;
    c->out_ok = c->st.ok;
}

/* pw of `slot` and mm over the newest `window` intervals, oldest first */
static int window_sums(const tonedet_ref_status* s, int fs, int slot, int window, double* pw, double* mm, double* M) {
    const int Mi = interval_of(fs);
    if (Mi == 0 || slot < 0 || slot >= NS || window < 1 || window > RING) return -1;
    if (s->intervals < (unsigned long long)window) return -6;
    double a = 0.0, b = 0.0;
    for (unsigned long long g = s->intervals - (unsigned long long)window; g < s->intervals; g++) {
        a += s->ring_pw[slot][g % RING]; b += s->ring_mm[g % RING];
    }
    *pw = a; *mm = b; *M = (double)Mi;
    return 0;
}

int tonedet_ref_share_db(const tonedet_ref_status* s, int fs, int slot, int window, double* db) {
    double pw, mm, M;
    const int rc = window_sums(s, fs, slot, window, &pw, &mm, &M);
    if (rc) return rc;
    *db = 10.0 * log10(2.0 * pw / (M * mm));
    return 0;
}

int tonedet_ref_level_db(const tonedet_ref_status* s, int fs, int slot, int window, double* db) {
    double pw, mm, M;
    const int rc = window_sums(s, fs, slot, window, &pw, &mm, &M);
    if (rc) return rc;
    *db = 10.0 * log10(2.0 * pw / (M * M * (double)window));
    return 0;
}
