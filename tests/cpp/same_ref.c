/* The EAS SAME decoder's arithmetic (include/fmdemod.h, "EAS SAME decoder") restated in plain C, one station at a time and one frame
 * after the other: what the tests compare fmd_same_* with, bit for bit.  Built with -ffp-contract=off -fno-fast-math: every operation
 * is the one written, and every multiply-add is an explicit fma(). */
#ifndef _DEFAULT_SOURCE
#define _DEFAULT_SOURCE                /* M_PI under -std=c99 */
#endif
#include <math.h>
#include <string.h>

#define MAXB 268
#define RING 8
#define HIST 7
#define PERIOD 12500ull

typedef struct {                       /* the layout of fmd_same_params */
    int      pull;
    unsigned hold_ticks, alarm_mask, reserved;
} same_ref_params;

typedef struct {                       /* the layout of fmd_same_message */
    unsigned long long sync_tick;
    unsigned short len;
    unsigned char kind, reserved, bytes[MAXB];
} same_ref_message;

typedef struct {                       /* the layout of fmd_same_status */
    unsigned long long frames, ticks, bits, syncs, accepted, rejected, sync_tick, last_accept_tick;
    double   open[4], hist[HIST][4];
    unsigned ph, sh, nbit, msg_len, run;
    unsigned char synced, prev_s, flags, ok, msg[MAXB], reserved[4];
    same_ref_message ring[RING];
} same_ref_status;

typedef struct {
    same_ref_status st;
    same_ref_params prm;
    int      fs, P, mark_step, space_step;
    const double* tab;                 /* [P][2]: tc, ts (the caller's, from same_ref_table) */
    unsigned char out_flags, out_ok;   /* the station's two bytes as of the last call */
} same_ref_chan;

typedef struct {                       /* the layout of fmd_same_encode_config */
    int       fs, repeats;
    long long gap_frames;
    double    clock_ratio, amplitude, mark_db;
} same_ref_encode_config;

static int gcd_of(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

int same_ref_geometry(int fs, int* P, int* mark_step, int* space_step) {
    if (fs < 8000 || fs > 48000 || fs % 10 != 0) return -1;
    const int g = gcd_of(3125, 6 * fs);
    *P = 6 * fs / g;
    *mark_step = (4 * 3125 / g) % *P;
    *space_step = (3 * 3125 / g) % *P;
    return 0;
}

/* libm's cos and libm's sin, each called on its own: a compiler that sees both on one argument makes them one sincos(), whose results
 * are not everywhere the bits of the two */
__attribute__((noinline)) static double table_cos(double a) { return cos(a); }
__attribute__((noinline)) static double table_sin(double a) { return sin(a); }

/* tab [P][2] */
void same_ref_table(int P, double* tab) {
    for (int j = 0; j < P; j++) {
        tab[2 * j] = table_cos(2.0 * M_PI * (double)j / (double)P);
        tab[2 * j + 1] = table_sin(2.0 * M_PI * (double)j / (double)P);
    }
}

/* B(r) - B(0) for r = 0 ... 12500 */
unsigned same_ref_tick_start(int fs, unsigned r) { return (r * 3u * (unsigned)fs + 12499u) / 12500u; }

/* B(k): the first frame of tick k */
static unsigned long long tick_start(int fs, unsigned long long k) {
    return (k / PERIOD) * 3ull * (unsigned long long)fs + (unsigned long long)same_ref_tick_start(fs, (unsigned)(k % PERIOD));
}

void same_ref_default_params(same_ref_params* p) {
    p->pull = 16;
    p->hold_ticks = 750000u;
    p->alarm_mask = 0u;
    p->reserved = 0u;
}

static int params_ok(const same_ref_params* p) {
    return p->pull >= 0 && p->pull <= 128 && p->hold_ticks >= 1u && p->hold_ticks <= 0x7fffffffu && p->alarm_mask <= 3u && p->reserved == 0u;
}

void same_ref_reset(same_ref_chan* c) {
    memset(&c->st, 0, sizeof(c->st));
    c->st.ok = 1;
}

int same_ref_create(same_ref_chan* c, int fs, const double* tab) {
    memset(c, 0, sizeof(*c));
    if (same_ref_geometry(fs, &c->P, &c->mark_step, &c->space_step) != 0) return -1;
    c->fs = fs;
    c->tab = tab;
    same_ref_default_params(&c->prm);
    same_ref_reset(c);
    c->out_flags = 0xAA; c->out_ok = 0xAA;
    return 0;
}

int same_ref_set_params(same_ref_chan* c, const same_ref_params* p) {
    if (!params_ok(p)) return -1;
    c->prm = *p;
    c->st.ok = (unsigned char)((c->st.flags & p->alarm_mask) == 0);
    return 0;
}

static void message_end(same_ref_chan* c, unsigned long long k) {
    same_ref_status* s = &c->st;
    unsigned kind = 0;
    if (s->msg_len >= 4) kind = memcmp(s->msg, "ZCZC", 4) == 0 ? 1u : (memcmp(s->msg, "NNNN", 4) == 0 ? 2u : 0u);
    if (kind) {
        same_ref_message* r = &s->ring[s->accepted % RING];
        memset(r, 0, sizeof(*r));
        r->sync_tick = s->sync_tick;
        r->len = (unsigned short)s->msg_len;
        r->kind = (unsigned char)kind;
        memcpy(r->bytes, s->msg, s->msg_len);
        s->accepted++;
        s->last_accept_tick = k;
        s->flags = (unsigned char)(kind == 1u ? (s->flags | 2u) : (s->flags & ~2u));
    } else {
        s->rejected++;
    }
    s->synced = 0;
    s->msg_len = 0;
}

static void tick_end(same_ref_chan* c) {
    same_ref_status* s = &c->st;
    const unsigned long long k = s->ticks;
    double w[4];
    for (int q = 0; q < 4; q++) {
        w[q] = 0.0;
        for (int h = 0; h < HIST; h++) w[q] += s->hist[h][q];
        w[q] += s->open[q];
    }
    const double e1 = fma(w[0], w[0], w[1] * w[1]), e0 = fma(w[2], w[2], w[3] * w[3]);
    const unsigned bit = e1 > e0 ? 1u : 0u;
    const unsigned pull = (unsigned)c->prm.pull;
    if (bit != s->prev_s) {
        /* the run that ends here was L ticks, n bits long; its middle stood at ph - 16 L, which in lock is 0 for an odd n and 128 for an even n */
        const unsigned L = s->run, nb = (L + 4u) >> 3;
        if (nb >= 1u && L <= 96u) {
            const unsigned err = (s->ph - 16u * L - ((nb & 1u) ? 0u : 128u)) & 255u;    /* 1 ... 127: the clock is ahead; 128 ... 255: behind */
            if (err < 128u) s->ph = (s->ph - (pull < err ? pull : err)) & 255u;
            else s->ph = (s->ph + (pull < 256u - err ? pull : 256u - err)) & 255u;
        }
        s->run = 0;
    }
    if (s->run < 255u) s->run++;
    s->prev_s = (unsigned char)bit;
    s->ph += 32u;
    if (s->ph >= 256u) {
        s->ph -= 256u;
        s->bits++;
        s->sh = (s->sh >> 1) | (bit << 15);
        if (!s->synced) {
            if (s->sh == 0xABABu) { s->synced = 1; s->syncs++; s->nbit = 0; s->msg_len = 0; s->sync_tick = k; }
        } else if (++s->nbit == 8u) {
            s->nbit = 0;
            const unsigned b = s->sh >> 8;
            if (!(b == 0xABu && s->msg_len == 0)) {
                const int valid = (b >= 0x20u && b <= 0x7Eu) || b == 0x0Du || b == 0x0Au;
                if (valid) s->msg[s->msg_len++] = (unsigned char)b;
                if (!valid || s->msg_len == MAXB) message_end(c, k);
            }
        }
    }
    if ((s->flags & 2u) && k - s->last_accept_tick >= (unsigned long long)c->prm.hold_ticks) s->flags = (unsigned char)(s->flags & ~2u);
    for (int h = 0; h + 1 < HIST; h++)
        for (int q = 0; q < 4; q++) s->hist[h][q] = s->hist[h + 1][q];
    for (int q = 0; q < 4; q++) { s->hist[HIST - 1][q] = s->open[q]; s->open[q] = 0.0; }
    s->ticks = k + 1;
}

/* x [n][2] */
void same_ref_process(same_ref_chan* c, const float* x, long long n) {
    same_ref_status* s = &c->st;
    const unsigned P = (unsigned)c->P;
    unsigned im = (unsigned)(((s->frames % P) * (unsigned long long)c->mark_step) % P);
    unsigned is = (unsigned)(((s->frames % P) * (unsigned long long)c->space_step) % P);
    unsigned long long next = tick_start(c->fs, s->ticks + 1);
    for (long long i = 0; i < n; i++) {
        const double m = (double)x[2 * i] + (double)x[2 * i + 1];
        s->open[0] = fma(m, c->tab[2 * im], s->open[0]);
        s->open[1] = fma(m, c->tab[2 * im + 1], s->open[1]);
        s->open[2] = fma(m, c->tab[2 * is], s->open[2]);
        s->open[3] = fma(m, c->tab[2 * is + 1], s->open[3]);
        im += (unsigned)c->mark_step; if (im >= P) im -= P;
        is += (unsigned)c->space_step; if (is >= P) is -= P;
        s->frames++;
        if (s->frames == next) {
            tick_end(c);
            next = tick_start(c->fs, s->ticks + 1);
        }
    }
    s->flags = (unsigned char)((s->flags & ~1u) | (s->synced ? 1u : 0u));
    s->ok = (unsigned char)((s->flags & c->prm.alarm_mask) == 0);
    c->out_flags = s->flags;
    c->out_ok = s->ok;
}

/* ---- the encoder ---- */

static double bits_in(long long i, double ratio, int fs) { return ((double)i * ratio * 3125.0) / (6.0 * (double)fs); }

/* the frames of the whole; out [frames][2] where out is not null (the caller's, large enough); -1 for values outside the ranges */
long long same_ref_encode(const same_ref_encode_config* cfg, const char* text, int len, float* out) {
    int P, a, b;
    if (same_ref_geometry(cfg->fs, &P, &a, &b) != 0 || len < 1 || len > MAXB || cfg->repeats < 1 || cfg->repeats > 16) return -1;
    if (!(cfg->clock_ratio >= 0.9 && cfg->clock_ratio <= 1.1) || !(cfg->amplitude >= 0.0 && cfg->amplitude < INFINITY)) return -1;
    if (!(cfg->mark_db >= -40.0 && cfg->mark_db <= 40.0) || cfg->gap_frames > (1LL << 30)) return -1;
    const int fs = cfg->fs;
    const double ratio = cfg->clock_ratio;
    const long long gap = cfg->gap_frames < 0 ? (long long)fs : cfg->gap_frames;
    const long long nbits = 8LL * (16 + len);
    long long nb = (long long)((double)nbits * 6.0 * (double)fs / (3125.0 * ratio)) - 2;
    if (nb < 0) nb = 0;
    while (bits_in(nb, ratio, fs) < (double)nbits) nb++;
    const long long total = (long long)cfg->repeats * (nb + gap);
    if (!out) return total;
    const double a_space = cfg->amplitude, a_mark = cfg->amplitude * pow(10.0, cfg->mark_db / 20.0);
    float* o = out;
    for (int r = 0; r < cfg->repeats; r++) {
        for (long long i = 0; i < nb; i++) {
            const double u = bits_in(i, ratio, fs);
            long long bi = (long long)u;
            if (bi >= nbits) bi = nbits - 1;
            const double frac = u - (double)bi;
            const long long byte = bi >> 3;
            const unsigned v = byte < 16 ? 0xABu : (unsigned)(unsigned char)text[byte - 16];
            const int bit = (int)((v >> (bi & 7)) & 1u);
            const double cyc = bit ? 4.0 : 3.0, amp = bit ? a_mark : a_space;
            const float s = (float)(amp * table_sin(2.0 * M_PI * cyc * frac));
            *o++ = s; *o++ = s;
        }
        for (long long i = 0; i < 2 * gap; i++) *o++ = 0.0f;
    }
    return total;
}
