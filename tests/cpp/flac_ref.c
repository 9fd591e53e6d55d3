/* The FLAC audio encoder's contract (include/fmdemod.h, "FLAC audio encoder") restated in plain C, one station at a time, sample by
 * sample and bit by bit: what the GPU tests compare the device's bytes, counts and records with, and what tests/test_flac_cpu.py
 * decodes with a decoder written from RFC 9639 (tests/flac_ref.py).  Written from the contract's description and the RFC; shares no
 * code with the library. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define MAXS 4608

/* include/fmdemod.h fmd_flac_status */
typedef struct {
    unsigned long long frames, blocks, stream_samples, stream_bytes, clipped[2], nonfinite;
    unsigned streams, frame_number, min_frame_bytes, max_frame_bytes, fill, wrapped;
} flac_ref_status;

typedef struct {
    flac_ref_status st;
    int S, fs;
    int open[MAXS][2]; /* the open block's q */
} flac_ref_chan;

int flac_ref_block_frames(int S) { return S == 0 ? 4096 : (S >= 64 && S <= MAXS && S % 64 == 0 ? S : 0); }
int flac_ref_frame_bound(int S) { return 16 + 2 * (1 + 2 * S) + 2; }
long long flac_ref_max_bytes(int S, long long n) { return (((long long)S - 1 + n) / S * flac_ref_frame_bound(S) + 3) / 4 * 4; }

/* the sample: *flag = 0 in range, 1 clamped, 2 not finite */
int flac_ref_sample(float x, int* flag) {
    volatile float t = x * (32767.0f * 0.95f);
    *flag = 0;
    if (isnan(t) || isinf(t)) { *flag = 2; return 0; }
    if (t >= 2147483648.0f || t <= -2147483648.0f) { *flag = 1; return t > 0.0f ? 32767 : -32768; }   /* (int)t would not be defined */
    int v = (int)t;
    if (v > 32767) { *flag = 1; return 32767; }
    if (v < -32768) { *flag = 1; return -32768; }
    return v;
}

unsigned flac_ref_crc8(const unsigned char* p, long long n) {
    unsigned c = 0;
    for (long long i = 0; i < n; i++) {
        c ^= p[i];
        for (int b = 0; b < 8; b++) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xffu : (c << 1) & 0xffu;
    }
    return c;
}

unsigned flac_ref_crc16(const unsigned char* p, long long n) {
    unsigned c = 0;
    for (long long i = 0; i < n; i++) {
        c ^= (unsigned)p[i] << 8;
        for (int b = 0; b < 8; b++) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xffffu : (c << 1) & 0xffffu;
    }
    return c;
}

/* the UTF-8-like coding of v < 2^31; returns the bytes written */
int flac_ref_coded_number(unsigned v, unsigned char* out) {
    if (v < 0x80u) { out[0] = (unsigned char)v; return 1; }
    int extra = v < 0x800u ? 1 : v < 0x10000u ? 2 : v < 0x200000u ? 3 : v < 0x4000000u ? 4 : 5;
    out[0] = (unsigned char)((0xff00u >> (extra + 1)) | (v >> (6 * extra)));
    for (int i = 1; i <= extra; i++) out[i] = (unsigned char)(0x80u | ((v >> (6 * (extra - i))) & 0x3fu));
    return extra + 1;
}

/* ---- bits, MSB first ---- */
typedef struct { unsigned char* p; long long pos; } bitw;
static void put(bitw* w, unsigned long long v, int len) {
    for (int i = len - 1; i >= 0; i--) {
        if ((v >> i) & 1u) w->p[w->pos >> 3] |= (unsigned char)(0x80u >> (w->pos & 7));
        else w->p[w->pos >> 3] &= (unsigned char)~(0x80u >> (w->pos & 7));
        w->pos++;
    }
}

/* ---- a subframe ---- */
typedef struct { int type, order, porder, k[64]; long long bits; } plan; /* type 0 CONSTANT, 1 VERBATIM, 2 FIXED */

static void residuals(const int* x, int n, int o, long long* r) {
    for (int i = o; i < n; i++) {
        long long v = x[i];
        if (o == 1) v = (long long)x[i] - x[i - 1];
        if (o == 2) v = (long long)x[i] - 2LL * x[i - 1] + x[i - 2];
        if (o == 3) v = (long long)x[i] - 3LL * x[i - 1] + 3LL * x[i - 2] - x[i - 3];
        if (o == 4) v = (long long)x[i] - 4LL * x[i - 1] + 6LL * x[i - 2] - 4LL * x[i - 3] + x[i - 4];
        r[i] = v;
    }
}

static unsigned long long zigzag(long long r) { return r >= 0 ? 2ULL * (unsigned long long)r : 2ULL * (unsigned long long)(-r) - 1ULL; }

static void plan_subframe(const int* x, int n, int b, plan* pl) {
    static long long r[MAXS];
    int same = 1;
    for (int i = 1; i < n; i++) same &= x[i] == x[0];
    memset(pl, 0, sizeof(*pl));
    if (same) { pl->type = 0; pl->bits = 8 + b; return; }
    const int omax = n - 1 < 4 ? n - 1 : 4;
    unsigned long long best_a = 0;
    int o = 0;
    for (int t = 0; t <= omax; t++) {
        residuals(x, n, t, r);
        unsigned long long a = 0;
        for (int i = omax; i < n; i++) a += (unsigned long long)(r[i] < 0 ? -r[i] : r[i]);
        if (t == 0 || a < best_a) { best_a = a; o = t; }
    }
    residuals(x, n, o, r);
    int P = 0;
    for (int p = 1; p <= 6; p++)
        if (n % (1 << p) == 0 && (n >> p) > o) P = p;
    unsigned long long best = 0;
    for (int p = 0; p <= P; p++) {
        unsigned long long cost = 2 + 4;
        int ks[64];
        for (int j = 0; j < (1 << p); j++) {
            const int a0 = j == 0 ? o : j * (n >> p), a1 = (j + 1) * (n >> p);
            unsigned long long bj = 0;
            for (int k = 0; k <= 14; k++) {
                unsigned long long s = 0;
                for (int i = a0; i < a1; i++) s += (zigzag(r[i]) >> k) + 1ULL + (unsigned long long)k;
                if (k == 0 || s < bj) { bj = s; ks[j] = k; }
            }
            cost += 4 + bj;
        }
        if (p == 0 || cost < best) {
            best = cost; pl->porder = p;
            memcpy(pl->k, ks, sizeof(ks));
        }
    }
    const unsigned long long fixed = 8ULL + (unsigned long long)o * b + best, verbatim = 8ULL + (unsigned long long)n * b;
    if (fixed < verbatim) { pl->type = 2; pl->order = o; pl->bits = (long long)fixed; }
    else { pl->type = 1; pl->bits = (long long)verbatim; }
}

static void write_subframe(bitw* w, const int* x, int n, int b, const plan* pl) {
    static long long r[MAXS];
    const unsigned long long mask = (1ULL << b) - 1ULL;
    if (pl->type == 0) { put(w, 0x00, 8); put(w, (unsigned long long)(long long)x[0] & mask, b); return; }
    if (pl->type == 1) {
        put(w, 0x02, 8);
        for (int i = 0; i < n; i++) put(w, (unsigned long long)(long long)x[i] & mask, b);
        return;
    }
    const int o = pl->order, p = pl->porder;
    put(w, (unsigned long long)((8 | o) << 1), 8);
    for (int i = 0; i < o; i++) put(w, (unsigned long long)(long long)x[i] & mask, b);
    put(w, 0, 2);
    put(w, (unsigned long long)p, 4);
    residuals(x, n, o, r);
    for (int j = 0; j < (1 << p); j++) {
        const int a0 = j == 0 ? o : j * (n >> p), a1 = (j + 1) * (n >> p), k = pl->k[j];
        put(w, (unsigned long long)k, 4);
        for (int i = a0; i < a1; i++) {
            const unsigned long long u = zigzag(r[i]);
            for (unsigned long long z = u >> k; z > 0; z--) put(w, 0, 1);
            put(w, 1, 1);
            put(w, u & ((1ULL << k) - 1ULL), k);
        }
    }
}

/* one frame of n frames of (l, r) with frame number `number`; returns its bytes */
int flac_ref_encode_frame(const int* l, const int* r, int n, int fs, unsigned number, unsigned char* out) {
    static int m[MAXS], s[MAXS];
    plan pl[4];
    for (int i = 0; i < n; i++) { m[i] = (l[i] + r[i]) >> 1; s[i] = l[i] - r[i]; }
    plan_subframe(l, n, 16, &pl[0]);
    plan_subframe(r, n, 16, &pl[1]);
    plan_subframe(m, n, 16, &pl[2]);
    plan_subframe(s, n, 17, &pl[3]);
    const long long tot[4] = {pl[0].bits + pl[1].bits, pl[0].bits + pl[3].bits, pl[3].bits + pl[1].bits, pl[2].bits + pl[3].bits};
    static const int code[4] = {1, 8, 9, 10};
    int mode = 0;
    for (int t = 1; t < 4; t++)
        if (tot[t] < tot[mode]) mode = t;
    unsigned char* h = out;
    int len = 0;
    h[len++] = 0xff; h[len++] = 0xf8;
    int bs_code = n <= 256 ? 6 : 7;
    for (int c = 2; c <= 5; c++)
        if (n == 576 << (c - 2)) bs_code = c;
    for (int c = 8; c <= 15; c++)
        if (n == 256 << (c - 8)) bs_code = c;
    if (n == 192) bs_code = 1;
    int sr_code = 13;
    static const int rates[11] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000};
    for (int c = 1; c <= 10; c++)
        if (fs == rates[c]) sr_code = c;
    h[len++] = (unsigned char)((bs_code << 4) | sr_code);
    h[len++] = (unsigned char)((code[mode] << 4) | (4 << 1));
    len += flac_ref_coded_number(number, h + len);
    if (bs_code == 6) h[len++] = (unsigned char)(n - 1);
    if (bs_code == 7) { h[len++] = (unsigned char)((n - 1) >> 8); h[len++] = (unsigned char)((n - 1) & 255); }
    if (sr_code == 13) { h[len++] = (unsigned char)(fs >> 8); h[len++] = (unsigned char)(fs & 255); }
    h[len] = (unsigned char)flac_ref_crc8(h, len);
    len++;
    bitw w = {out, 8LL * len};
    const int* c0 = mode == 2 ? s : mode == 3 ? m : l;
    const int* c1 = mode == 1 || mode == 3 ? s : r;
    const plan* p0 = mode == 2 ? &pl[3] : mode == 3 ? &pl[2] : &pl[0];
    const plan* p1 = mode == 1 || mode == 3 ? &pl[3] : &pl[1];
    write_subframe(&w, c0, n, mode == 2 ? 17 : 16, p0);
    write_subframe(&w, c1, n, mode == 1 || mode == 3 ? 17 : 16, p1);
    while (w.pos & 7) put(&w, 0, 1);
    len = (int)(w.pos >> 3);
    const unsigned crc = flac_ref_crc16(out, len);
    out[len++] = (unsigned char)(crc >> 8);
    out[len++] = (unsigned char)(crc & 255);
    return len;
}

/* ---- the stream ---- */
static void new_stream(flac_ref_chan* ch) {
    ch->st.streams++;
    ch->st.frame_number = 0;
    ch->st.stream_samples = ch->st.stream_bytes = 0;
    ch->st.min_frame_bytes = ch->st.max_frame_bytes = 0;
}

/* the open block's first n frames as one FLAC frame at out; returns its bytes; *wrap = 1 where the stream ended behind it by itself */
static int emit(flac_ref_chan* ch, int n, unsigned char* out, int* wrap) {
    static int l[MAXS], r[MAXS];
    for (int i = 0; i < n; i++) { l[i] = ch->open[i][0]; r[i] = ch->open[i][1]; }
    const int len = flac_ref_encode_frame(l, r, n, ch->fs, ch->st.frame_number, out);
    ch->st.blocks++;
    ch->st.stream_samples += (unsigned long long)n;
    ch->st.stream_bytes += (unsigned long long)len;
    if (ch->st.min_frame_bytes == 0 || (unsigned)len < ch->st.min_frame_bytes) ch->st.min_frame_bytes = (unsigned)len;
    if ((unsigned)len > ch->st.max_frame_bytes) ch->st.max_frame_bytes = (unsigned)len;
    ch->st.fill = 0;
    *wrap = ch->st.frame_number == 0x7fffffffu;                              /* the number would reach 2^31 */
    if (*wrap) { new_stream(ch); ch->st.wrapped = 1; }
    else ch->st.frame_number++;
    return len;
}

void flac_ref_reset(flac_ref_chan* ch) {
    memset(&ch->st, 0, sizeof(ch->st));
    memset(ch->open, 0, sizeof(ch->open));
}

int flac_ref_create(flac_ref_chan* ch, int S, int fs) {
    memset(ch, 0, sizeof(*ch));
    ch->S = flac_ref_block_frames(S);
    if (ch->S == 0 || fs < 8000 || fs > 48000) return -1;
    ch->fs = fs;
    return 0;
}

/* n frames x [n][2]; the completed FLAC frames back to back into out; *nframes their number; returns their bytes */
long long flac_ref_process(flac_ref_chan* ch, const float* x, long long n, unsigned char* out, int* nframes) {
    long long bytes = 0;
    int wrap;
    *nframes = 0;
    for (long long i = 0; i < n; i++) {
        for (int rail = 0; rail < 2; rail++) {
            int flag;
            ch->open[ch->st.fill][rail] = flac_ref_sample(x[2 * i + rail], &flag);
            if (flag == 1) ch->st.clipped[rail]++;
            if (flag == 2) ch->st.nonfinite++;
        }
        ch->st.frames++;
        if ((int)++ch->st.fill == ch->S) { bytes += emit(ch, ch->S, out + bytes, &wrap); (*nframes)++; }
    }
    return bytes;
}

/* ends the stream: a short last frame where the open block holds frames; returns its bytes (0 at fill 0) and *nframes 0 or 1 */
int flac_ref_flush(flac_ref_chan* ch, unsigned char* out, int* nframes) {
    int len = 0, wrap = 0;
    *nframes = 0;
    if (ch->st.fill > 0) { len = emit(ch, (int)ch->st.fill, out, &wrap); *nframes = 1; }
    if (!wrap) new_stream(ch);                                               /* (a frame numbered 2^31 - 1 has ended the stream already) */
    return len;
}

void flac_ref_set_frame_number(flac_ref_chan* ch, unsigned v) { ch->st.frame_number = v; }
