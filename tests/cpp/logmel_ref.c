/* The log-mel front end's arithmetic contract (include/fmdemod.h, "Log-mel front end") restated in plain C, sample by sample, with
 * nothing of the library's code: the design in double with the host libm, the window, the two DFT chains per bin in ascending n, the
 * powers, the mel chains in ascending k over all bins, the clamp and flog10, and the streaming rule T(f).  The GPU's rows, counts and
 * records must equal this program's bit for bit (tests/test_gpu_logmel.py); tests/test_logmel_cpu.py holds it to a float64 model.
 *
 * Built by tests/logmel_ref.py with gcc -O2 -std=c99 -ffp-contract=off -fno-fast-math: every operation is the one written. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

typedef struct {
    int n_channels, fs, win, hop, n_mels;
    double f_min_hz, f_max_hz;
    int mel_scale, out_mode;
    float log_floor;
    long long max_input_frames;
    int device;
} logmel_ref_config;

typedef struct {
    unsigned long long frames, spectra, nonfinite;
    unsigned fill, reserved;
} logmel_ref_status;

typedef struct {
    logmel_ref_config cfg;
    int K;
    float *w, *tc, *ts, *fb;   /* [N], [N], [N], [n_mels][K] */
    float* buf;                /* the open window's mono samples, [N] */
    float *P, *mel;            /* scratch: [K], [n_mels] */
    logmel_ref_status st;
} logmel_ref_chan;

int logmel_ref_check(const logmel_ref_config* c) {
    if (!c) return -1;
    if (c->n_channels <= 0 || c->max_input_frames <= 0 || c->max_input_frames > (1LL << 30)) return -1;
    if (c->fs < 8000 || c->fs > 48000) return -1;
    if (c->win < 64 || c->win > 2048 || c->win % 16 != 0) return -1;
    if (c->hop < 16 || c->hop > c->win) return -1;
    if (c->n_mels < 1 || c->n_mels > 128) return -1;
    if (!(c->f_min_hz >= 0.0 && c->f_min_hz < c->f_max_hz && c->f_max_hz <= 0.5 * (double)c->fs)) return -1;
    if (c->mel_scale != 0 && c->mel_scale != 1) return -1;
    if (c->out_mode != 0 && c->out_mode != 1) return -1;
    if (!(c->log_floor >= FLT_MIN && c->log_floor <= FLT_MAX)) return -1;
    return 0;
}

int logmel_ref_default_config(int fs, logmel_ref_config* c) {
    if (!c || fs < 8000 || fs > 48000) return -1;
    c->n_channels = 1; c->fs = fs;
    c->win = (fs / 40 + 15) / 16 * 16;
    c->hop = fs / 100;
    c->n_mels = 80;
    c->f_min_hz = 0.0;
    c->f_max_hz = 0.5 * (double)fs < 8000.0 ? 0.5 * (double)fs : 8000.0;
    c->mel_scale = 0; c->out_mode = 1; c->log_floor = 1e-10f;
    c->max_input_frames = 65536; c->device = -1;
    return 0;
}

int logmel_ref_bins(const logmel_ref_config* c) {
    if (logmel_ref_check(c) != 0) return -1;
    {
        const int half = c->win / 2;
        const double top = floor(c->f_max_hz * (double)c->win / (double)c->fs);
        return (top < (double)half ? (int)top : half) + 1;
    }
}

long long logmel_ref_max_frames(int hop, long long n) {
    if (hop < 16 || hop > 2048 || n < 0 || n > (1LL << 40)) return -1;
    return (n + hop - 1) / hop;
}

unsigned long long logmel_ref_T(unsigned long long f, int win, int hop) {
    return f < (unsigned long long)win ? 0ull : (f - (unsigned long long)win) / (unsigned long long)hop + 1ull;
}

/* libm's cos and libm's sin, each called on its own: a compiler that sees both on one argument makes them one sincos(), whose results
 * are not everywhere the bits of the two */
__attribute__((noinline)) static double table_cos(double a) { return cos(a); }
__attribute__((noinline)) static double table_sin(double a) { return sin(a); }

double logmel_ref_mel(double f, int scale) {
    if (scale == 1) return 2595.0 * log10(1.0 + f / 700.0);
    return f < 1000.0 ? f / (200.0 / 3.0) : 15.0 + log(f / 1000.0) / (log(6.4) / 27.0);
}
double logmel_ref_mel_inv(double m, int scale) {
    if (scale == 1) return 700.0 * (pow(10.0, m / 2595.0) - 1.0);
    return m < 15.0 ? m * (200.0 / 3.0) : 1000.0 * exp((m - 15.0) * (log(6.4) / 27.0));
}

/* w, tc, ts [N]; fb [n_mels][K]; any may be null */
int logmel_ref_design(const logmel_ref_config* c, float* w, float* tc, float* ts, float* fb, int* K_out, int* empty_out) {
    int N, K, nm, n, i, j, k, empty = 0;
    double *F, m0, m1;
    if (logmel_ref_check(c) != 0) return -1;
    N = c->win; K = logmel_ref_bins(c); nm = c->n_mels;
    for (n = 0; n < N; n++) {
        const double a = 2.0 * M_PI * (double)n / (double)N;
        if (w) w[n] = (float)(0.5 - 0.5 * table_cos(a));
        if (tc) tc[n] = (float)table_cos(a);
        if (ts) ts[n] = (float)table_sin(a);
    }
    F = (double*)malloc(sizeof(double) * (size_t)(nm + 2));
    m0 = logmel_ref_mel(c->f_min_hz, c->mel_scale); m1 = logmel_ref_mel(c->f_max_hz, c->mel_scale);
    for (i = 0; i < nm + 2; i++) F[i] = logmel_ref_mel_inv(m0 + (double)i * (m1 - m0) / (double)(nm + 1), c->mel_scale);
    for (j = 0; j < nm; j++) {
        const double Fa = F[j], Fb = F[j + 1], Fc = F[j + 2];
        const double s = c->mel_scale == 0 ? 2.0 / (Fc - Fa) : 1.0;
        int any = 0;
        for (k = 0; k < K; k++) {
            const double fk = (double)k * (double)c->fs / (double)N;
            const double up = (fk - Fa) / (Fb - Fa), down = (Fc - fk) / (Fc - Fb);
            const double t = up < down ? up : down;
            const float v = (float)((t > 0.0 ? t : 0.0) * s);
            if (fb) fb[(size_t)j * (size_t)K + (size_t)k] = v;
            if (v != 0.0f) any = 1;
        }
        if (!any) empty++;
    }
    free(F);
    if (K_out) *K_out = K;
    if (empty_out) *empty_out = empty;
    return 0;
}

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

float logmel_ref_flog10(float x) {
    static const uint32_t c[11] = {0xbe5e5bd9u, 0x3e143d3au, 0xbdde5bb4u, 0x3db1e377u, 0xbd9445b2u, 0x3d7e1719u,
                                   0xbd5cc607u, 0x3d446f9au, 0xbd41dcffu, 0x3d3d35d2u, 0xbccff948u};
    const uint32_t ix = to_bits(x), u = ix - 0x3f3504f3u;
    const float ef = (float)((int32_t)u >> 23);
    const float f = from_bits((u & 0x007fffffu) + 0x3f3504f3u) - 1.0f;
    float r = from_bits(c[10]), t, lm, y;
    int i;
    for (i = 9; i >= 0; i--) r = fmaf(f, r, from_bits(c[i]));
    t = fmaf(f, r, from_bits(0xb22d91afu));
    lm = fmaf(f, from_bits(0x3ede5bd9u), f * t);
    y = fmaf(ef, from_bits(0x3e9a2000u), fmaf(ef, from_bits(0x369a84fcu), lm));
    return (ix & 0x7fffffffu) >= 0x7f800000u ? x : y;
}

float logmel_ref_clamp(float mel, float floor_) { return mel > floor_ ? mel : (mel != mel ? mel : floor_); }

float logmel_ref_out(float mel, int out_mode, float floor_) {
    const float v = out_mode ? logmel_ref_flog10(logmel_ref_clamp(mel, floor_)) : mel;
    return v != v ? from_bits(0x7fc00000u) : v;
}

logmel_ref_chan* logmel_ref_create(const logmel_ref_config* c) {
    logmel_ref_chan* h;
    if (logmel_ref_check(c) != 0) return NULL;
    h = (logmel_ref_chan*)calloc(1, sizeof(*h));
    h->cfg = *c;
    h->K = logmel_ref_bins(c);
    h->w = (float*)calloc((size_t)c->win, 4); h->tc = (float*)calloc((size_t)c->win, 4); h->ts = (float*)calloc((size_t)c->win, 4);
    h->fb = (float*)calloc((size_t)c->n_mels * (size_t)h->K, 4);
    h->buf = (float*)calloc((size_t)c->win, 4);
    h->P = (float*)calloc((size_t)h->K, 4); h->mel = (float*)calloc((size_t)c->n_mels, 4);
    logmel_ref_design(c, h->w, h->tc, h->ts, h->fb, NULL, NULL);
    return h;
}

void logmel_ref_destroy(logmel_ref_chan* h) {
    if (!h) return;
    free(h->w); free(h->tc); free(h->ts); free(h->fb); free(h->buf); free(h->P); free(h->mel);
    free(h);
}

void logmel_ref_reset(logmel_ref_chan* h) { memset(&h->st, 0, sizeof(h->st)); }

void logmel_ref_get_status(const logmel_ref_chan* h, logmel_ref_status* out) { *out = h->st; }

/* one spectral frame of the N samples in h->buf into row [n_mels]; returns 1 where a band is not finite */
static int frame(logmel_ref_chan* h, float* row) {
    const int N = h->cfg.win, K = h->K, nm = h->cfg.n_mels;
    int k, n, j, bad = 0;
    for (k = 0; k < K; k++) {
        float re = 0.0f, im = 0.0f;
        int idx = 0;
        for (n = 0; n < N; n++) {
            const float xw = h->w[n] * h->buf[n];
            re = fmaf(xw, h->tc[idx], re);
            im = fmaf(xw, h->ts[idx], im);
            idx += k; if (idx >= N) idx -= N;                   /* (k n) mod N */
        }
        h->P[k] = fmaf(re, re, im * im);
    }
    for (j = 0; j < nm; j++) {
        float mel = 0.0f, v;
        for (k = 0; k < K; k++) mel = fmaf(h->fb[(size_t)j * (size_t)K + (size_t)k], h->P[k], mel);
        v = logmel_ref_out(mel, h->cfg.out_mode, h->cfg.log_floor);
        row[j] = v;
        if ((to_bits(v) & 0x7f800000u) == 0x7f800000u) bad = 1;
    }
    return bad;
}

/* takes n frames x [n][2]; writes the completed spectral frames as rows of n_mels from out on (cap_rows of them at most: -1 is returned
 * if there would be more) and returns their number */
int logmel_ref_process(logmel_ref_chan* h, const float* x, long long n, float* out, int cap_rows) {
    const int N = h->cfg.win, hop = h->cfg.hop, nm = h->cfg.n_mels;
    long long i;
    int rows = 0;
    for (i = 0; i < n; i++) {
        h->buf[h->st.fill++] = 0.5f * (x[2 * i] + x[2 * i + 1]);
        h->st.frames++;
        if ((int)h->st.fill == N) {
            if (rows >= cap_rows) return -1;
            h->st.nonfinite += (unsigned long long)frame(h, out + (size_t)rows * (size_t)nm);
            rows++;
            h->st.spectra++;
            memmove(h->buf, h->buf + hop, sizeof(float) * (size_t)(N - hop));
            h->st.fill = (unsigned)(N - hop);
        }
    }
    return rows;
}

/* the kept samples, for the tests that look at the state */
const float* logmel_ref_kept(const logmel_ref_chan* h) { return h->buf; }

/* drivers around logmel_ref_flog10, so that the sweep of the 2^24 floats in [0.5, 2) runs in C */
void logmel_ref_flog10_array(const float* x, float* y, long long n) {
    long long i;
    for (i = 0; i < n; i++) y[i] = logmel_ref_flog10(x[i]);
}

/* the worst error in fp32 ulp of the exact value against the host's float64 log10 over the bit patterns first, first + stride ... last */
double logmel_ref_flog10_sweep(unsigned first, unsigned last, unsigned stride, unsigned* at, unsigned long long* count) {
    double worst = 0.0;
    unsigned long long b, c = 0;
    for (b = first; b <= last; b += stride) {
        const float x = from_bits((uint32_t)b);
        const double ref = log10((double)x), a = fabs(ref) < 1.17549435e-38 ? 1.17549435e-38 : ref;
        int e;
        double err;
        (void)frexp(a, &e);
        err = fabs((double)logmel_ref_flog10(x) - ref) / ldexp(1.0, e - 24);
        c++;
        if (err > worst) { worst = err; *at = (unsigned)b; }
    }
    *count = c;
    return worst;
}
