/* The audio fingerprinter's arithmetic contract (include/fmdemod.h, "Audio fingerprinter") restated in plain C, sample by sample, with
 * nothing of the library's code: the design in double with the host libm, the sub-block chains in ascending n, the frame chains in
 * ascending j, the three-tap window, the powers, the band sums in ascending k, the differences and the words, and the streaming rule.
 * The GPU's words, counts, energies and records must equal this program's bit for bit (tests/test_gpu_fprint.py);
 * tests/test_fprint_cpu.py holds it to a float64 definition.
 *
 * Built by tests/fprint_ref.py with gcc -O2 -std=c99 -ffp-contract=off -fno-fast-math: every operation is the one written. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

#define MAX_BANDS 33

typedef struct {
    int n_channels, fs, hop, n_sub, n_bands;
    double f_min_hz, f_max_hz;
    long long max_input_frames;
    int device;
} fprint_ref_config;

typedef struct {
    unsigned long long frames, prints, nonfinite;
    unsigned fill, reserved;
} fprint_ref_status;

typedef struct {
    fprint_ref_config cfg;
    int K, first, edges[MAX_BANDS + 1];
    float *bc, *bs;            /* [H][K] */
    float wc[32], ws[32];
    float* carry;              /* the open sub-block's mono samples, [H] */
    float *Sr, *Si;            /* the last R sub-block spectra, oldest first, [R][K] */
    int have;                  /* how many of them are there, up to R */
    float *Xr, *Xi;            /* scratch [K] */
    float E[MAX_BANDS];        /* of the last frame */
    int frames_done;           /* 0 until the first frame (saturates at 1) */
    fprint_ref_status st;
} fprint_ref_chan;

int fprint_ref_check(const fprint_ref_config* c) {
    if (!c) return -1;
    if (c->n_channels <= 0 || c->max_input_frames <= 0 || c->max_input_frames > (1LL << 30)) return -1;
    if (c->fs < 8000 || c->fs > 48000) return -1;
    if (c->hop < 16 || c->hop > 1024 || c->hop % 16 != 0) return -1;
    if (c->n_sub != 4 && c->n_sub != 8 && c->n_sub != 16 && c->n_sub != 32) return -1;
    if (c->n_bands < 2 || c->n_bands > MAX_BANDS) return -1;
    if (!(c->f_min_hz > 0.0 && c->f_min_hz < c->f_max_hz && c->f_max_hz <= 1e9)) return -1;
    return 0;
}

int fprint_ref_default_config(int fs, fprint_ref_config* c) {
    if (!c || fs < 8000 || fs > 48000) return -1;
    c->n_channels = 1; c->fs = fs;
    c->hop = 16 * ((fs * 23 + 16000) / 32000);
    c->n_sub = 32; c->n_bands = 33;
    c->f_min_hz = 300.0; c->f_max_hz = 2000.0;
    c->max_input_frames = 65536; c->device = -1;
    return 0;
}

/* the bin edges k_b [B + 1]; -1 for an invalid configuration or design */
int fprint_ref_edges(const fprint_ref_config* c, int* edges) {
    int b, N;
    if (fprint_ref_check(c) != 0) return -1;
    N = c->n_sub * c->hop;
    for (b = 0; b <= c->n_bands; b++) {
        const double f = c->f_min_hz * pow(c->f_max_hz / c->f_min_hz, (double)b / (double)c->n_bands);
        const double k = floor(f * (double)N / (double)c->fs + 0.5);
        if (!(k <= (double)(N / 2 - 1))) return -1;
        edges[b] = (int)k;
    }
    if (edges[0] < 1) return -1;
    for (b = 0; b < c->n_bands; b++)
        if (edges[b] >= edges[b + 1]) return -1;
    return 0;
}

int fprint_ref_bins(const fprint_ref_config* c) {
    int e[MAX_BANDS + 1];
    if (fprint_ref_edges(c, e) != 0) return -1;
    return e[c->n_bands] - e[0] + 2;
}

long long fprint_ref_max_prints(int hop, long long n) {
    if (hop < 16 || hop > 1024 || n < 0 || n > (1LL << 40)) return -1;
    return (n + hop - 1) / hop;
}

unsigned long long fprint_ref_prints(unsigned long long f, int hop, int n_sub) {
    const unsigned long long s = f / (unsigned long long)hop;
    return s > (unsigned long long)n_sub ? s - (unsigned long long)n_sub : 0ull;
}

__attribute__((noinline)) static double table_cos(double a) { return cos(a); }
__attribute__((noinline)) static double table_sin(double a) { return sin(a); }

/* bc, bs [H][K]; wc, ws [R]; edges [B + 1]; any may be null */
int fprint_ref_design(const fprint_ref_config* c, float* bc, float* bs, float* wc, float* ws, int* edges, int* K_out, int* first_out) {
    int e[MAX_BANDS + 1], H, R, N, K, first, n, k, q, b;
    if (fprint_ref_edges(c, e) != 0) return -1;
    H = c->hop; R = c->n_sub; N = R * H; first = e[0] - 1; K = e[c->n_bands] - e[0] + 2;
    for (n = 0; n < H; n++)
        for (k = 0; k < K; k++) {
            const long long idx = ((long long)(first + k) * (long long)n) % (long long)N;
            const double phi = 2.0 * M_PI * (double)idx / (double)N;
            if (bc) bc[(size_t)n * (size_t)K + (size_t)k] = (float)table_cos(phi);
            if (bs) bs[(size_t)n * (size_t)K + (size_t)k] = (float)(-table_sin(phi));
        }
    for (q = 0; q < R; q++) {
        const double a = 2.0 * M_PI * (double)q / (double)R;
        float cq = (float)table_cos(a), sq = (float)table_sin(a);
        if (q % (R / 4) == 0) {
            const int t = q / (R / 4);
            cq = t == 0 ? 1.0f : (t == 2 ? -1.0f : 0.0f);
            sq = t == 1 ? 1.0f : (t == 3 ? -1.0f : 0.0f);
        }
        if (wc) wc[q] = cq;
        if (ws) ws[q] = sq;
    }
    if (edges) for (b = 0; b <= c->n_bands; b++) edges[b] = e[b];
    if (K_out) *K_out = K;
    if (first_out) *first_out = first;
    return 0;
}

static uint32_t to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static int nonfinite(float f) { return (to_bits(f) & 0x7f800000u) == 0x7f800000u; }

fprint_ref_chan* fprint_ref_create(const fprint_ref_config* c) {
    fprint_ref_chan* h;
    size_t HK, RK;
    if (fprint_ref_bins(c) < 0) return NULL;
    h = (fprint_ref_chan*)calloc(1, sizeof(*h));
    h->cfg = *c;
    h->K = fprint_ref_bins(c);
    HK = (size_t)c->hop * (size_t)h->K; RK = (size_t)c->n_sub * (size_t)h->K;
    h->bc = (float*)calloc(HK, 4); h->bs = (float*)calloc(HK, 4);
    h->carry = (float*)calloc((size_t)c->hop, 4);
    h->Sr = (float*)calloc(RK, 4); h->Si = (float*)calloc(RK, 4);
    h->Xr = (float*)calloc((size_t)h->K, 4); h->Xi = (float*)calloc((size_t)h->K, 4);
    fprint_ref_design(c, h->bc, h->bs, h->wc, h->ws, h->edges, NULL, &h->first);
    return h;
}

void fprint_ref_destroy(fprint_ref_chan* h) {
    if (!h) return;
    free(h->bc); free(h->bs); free(h->carry); free(h->Sr); free(h->Si); free(h->Xr); free(h->Xi);
    free(h);
}

void fprint_ref_reset(fprint_ref_chan* h) {
    memset(&h->st, 0, sizeof(h->st));
    h->have = 0;
    h->frames_done = 0;
}

void fprint_ref_get_status(const fprint_ref_chan* h, fprint_ref_status* out) { *out = h->st; }

/* the sub-block in h->carry is complete: its spectrum joins the kept ones; with R of them a frame, and behind the first frame a word.
 * Returns 1 where a word was written to *word (and its frame's energies to erow [B], where erow is not null) */
static int sub_block(fprint_ref_chan* h, uint32_t* word, float* erow) {
    const int H = h->cfg.hop, R = h->cfg.n_sub, B = h->cfg.n_bands, K = h->K;
    float E[MAX_BANDS];
    int k, n, j, b, wrote = 0;
    if (h->have == R) {                                                   /* the oldest leaves */
        memmove(h->Sr, h->Sr + K, sizeof(float) * (size_t)(R - 1) * (size_t)K);
        memmove(h->Si, h->Si + K, sizeof(float) * (size_t)(R - 1) * (size_t)K);
        h->have = R - 1;
    }
    for (k = 0; k < K; k++) {
        float sr = 0.0f, si = 0.0f;
        for (n = 0; n < H; n++) {
            sr = fmaf(h->carry[n], h->bc[(size_t)n * (size_t)K + (size_t)k], sr);
            si = fmaf(h->carry[n], h->bs[(size_t)n * (size_t)K + (size_t)k], si);
        }
        h->Sr[(size_t)h->have * (size_t)K + (size_t)k] = sr;
        h->Si[(size_t)h->have * (size_t)K + (size_t)k] = si;
    }
    h->have++;
    if (h->have < R) return 0;
    for (k = 0; k < K; k++) {
        float re = 0.0f, im = 0.0f;
        for (j = 0; j < R; j++) {
            const int q = (int)(((long long)(h->first + k) * (long long)j) % (long long)R);
            const float sr = h->Sr[(size_t)j * (size_t)K + (size_t)k], si = h->Si[(size_t)j * (size_t)K + (size_t)k];
            re = fmaf(sr, h->wc[q], re); re = fmaf(si, h->ws[q], re);
            im = fmaf(si, h->wc[q], im); im = fmaf(-sr, h->ws[q], im);
        }
        h->Xr[k] = re; h->Xi[k] = im;
    }
    for (b = 0; b < B; b++) {
        float e = 0.0f;
        for (k = h->edges[b] - h->first; k < h->edges[b + 1] - h->first; k++) {          /* columns 1 ... K - 2 */
            const float xr = fmaf(-0.25f, h->Xr[k - 1] + h->Xr[k + 1], 0.5f * h->Xr[k]);
            const float xi = fmaf(-0.25f, h->Xi[k - 1] + h->Xi[k + 1], 0.5f * h->Xi[k]);
            e = e + fmaf(xr, xr, xi * xi);
        }
        E[b] = e;
    }
    if (h->frames_done) {
        uint32_t w = 0;
        int bad = 0;
        for (b = 0; b < B - 1; b++) {
            const float d0 = E[b] - E[b + 1], d1 = h->E[b] - h->E[b + 1];
            const float d = d0 - d1;
            if (d > 0.0f) w |= 1u << (31 - b);
        }
        for (b = 0; b < B; b++) bad |= nonfinite(E[b]) | nonfinite(h->E[b]);
        *word = w;
        if (erow) for (b = 0; b < B; b++) erow[b] = E[b] != E[b] ? from_bits(0x7fc00000u) : E[b];
        h->st.nonfinite += (unsigned long long)bad;
        h->st.prints++;
        wrote = 1;
    }
    memcpy(h->E, E, sizeof(float) * (size_t)B);
    h->frames_done = 1;
    return wrote;
}

/* takes n frames x [n][2]; writes the completed words from out on (cap of them at most: -1 is returned if there would be more), their
 * frames' energies as rows of B from energy on where it is not null, and returns the number of words */
int fprint_ref_process(fprint_ref_chan* h, const float* x, long long n, uint32_t* out, float* energy, int cap) {
    const int H = h->cfg.hop, B = h->cfg.n_bands;
    long long i;
    int words = 0;
    for (i = 0; i < n; i++) {
        h->carry[h->st.fill++] = 0.5f * (x[2 * i] + x[2 * i + 1]);
        h->st.frames++;
        if ((int)h->st.fill == H) {
            uint32_t w;
            float e[MAX_BANDS];
            h->st.fill = 0;
            if (sub_block(h, &w, e)) {
                if (words >= cap) return -1;
                out[words] = w;
                if (energy) memcpy(energy + (size_t)words * (size_t)B, e, sizeof(float) * (size_t)B);
                words++;
            }
        }
    }
    return words;
}
