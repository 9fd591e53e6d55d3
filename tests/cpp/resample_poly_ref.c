/* Restatement of the audio resampler's polyphase method from its definition (DESIGN.md "Audio resampler", include/fmdemod.h
 * FMD_RESAMPLE_POLYPHASE), not from the kernel: a streaming object that takes one input frame at a time into a delay line of T
 * frames per channel (the frame itself and the T - 1 before it) and emits every output n whose newest frame floor(n M / L) it
 * is,
 *     acc = 0.0f;  for t = 0 .. T - 1:  acc = fmaf(h[p + t L], x[floor(n M / L) - t], acc),   p = n M mod L,
 * with x zero before frame 0 and after a reset.  The two 64-bit counters are shared by all channels.
 * Build with -ffp-contract=off -fno-fast-math so that every operation is the one written. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int C, L, M, T;
    float* taps;              /* [T][L]: taps[t L + p] = h[p + t L] */
    float* line;              /* [C][T][2]: frame m of a channel sits in slot m mod T */
    long long n_abs, o_abs;   /* input frames taken / output frames emitted since the last reset(-1) */
} poly_ref;

poly_ref* poly_ref_create(int C, int L, int M, int T, const float* taps) {
    poly_ref* r = (poly_ref*)calloc(1, sizeof(poly_ref));
    r->C = C; r->L = L; r->M = M; r->T = T;
    r->taps = (float*)malloc(sizeof(float) * (size_t)T * (size_t)L);
    memcpy(r->taps, taps, sizeof(float) * (size_t)T * (size_t)L);
    r->line = (float*)calloc((size_t)C * (size_t)T * 2, sizeof(float));
    return r;
}

void poly_ref_destroy(poly_ref* r) {
    free(r->taps);
    free(r->line);
    free(r);
}

/* channel >= 0: that channel's past becomes zero, the counters stay; -1: every channel's, and the counters restart */
void poly_ref_reset(poly_ref* r, int channel) {
    const size_t row = (size_t)r->T * 2;
    if (channel < 0) {
        memset(r->line, 0, sizeof(float) * row * (size_t)r->C);
        r->n_abs = 0; r->o_abs = 0;
    } else {
        memset(r->line + row * (size_t)channel, 0, sizeof(float) * row);
    }
}

/* outputs n with floor(n M / L) < n_abs + n_in that are not emitted yet */
long long poly_ref_output_frames(const poly_ref* r, long long n_in) {
    const long long end = ((r->n_abs + n_in) * r->L + r->M - 1) / r->M;
    return end - r->o_abs;
}

/* x [C][in_stride][2], y [C][out_stride][2].  Returns the frames emitted per channel, -1 (nothing done) if y is too narrow. */
long long poly_ref_process(poly_ref* r, const float* x, long long in_stride, long long n_in, float* y, long long out_stride) {
    const long long want = poly_ref_output_frames(r, n_in);
    if (want > out_stride) return -1;
    long long emitted = 0;
    for (long long i = 0; i < n_in; i++) {
        const long long m = r->n_abs;
        const int slot = (int)(m % r->T);
        for (int c = 0; c < r->C; c++) {
            float* f = r->line + ((size_t)c * (size_t)r->T + (size_t)slot) * 2;
            f[0] = x[((size_t)c * (size_t)in_stride + (size_t)i) * 2];
            f[1] = x[((size_t)c * (size_t)in_stride + (size_t)i) * 2 + 1];
        }
        while ((r->o_abs * r->M) / r->L == m) {
            const int p = (int)((r->o_abs * r->M) % r->L);
            for (int c = 0; c < r->C; c++) {
                const float* ln = r->line + (size_t)c * (size_t)r->T * 2;
                float al = 0.0f, ar = 0.0f;
                for (int t = 0; t < r->T; t++) {
                    const float h = r->taps[(size_t)t * (size_t)r->L + (size_t)p];
                    const int s = (slot - t) < 0 ? slot - t + r->T : slot - t;      /* (m - t) mod T */
                    al = fmaf(h, ln[2 * s], al);
                    ar = fmaf(h, ln[2 * s + 1], ar);
                }
                y[((size_t)c * (size_t)out_stride + (size_t)emitted) * 2] = al;
                y[((size_t)c * (size_t)out_stride + (size_t)emitted) * 2 + 1] = ar;
            }
            emitted++;
            r->o_abs++;
        }
        r->n_abs++;
    }
    return emitted;
}

void poly_ref_counters(const poly_ref* r, long long* n_abs, long long* o_abs) {
    *n_abs = r->n_abs;
    *o_abs = r->o_abs;
}

/* The pcm16 form of n values: t = y * (32767.0f * 0.95f), one fp32 multiply; for finite |t| < 2^31 the low 16 bits of
 * (int32_t)t (modular, not saturating).  NaN, +-inf and |t| >= 2^31: unspecified[i] = 1 and out[i] = 0. */
void poly_ref_pcm16(const float* y, long long n, int16_t* out, unsigned char* unspecified) {
    const float scale = 32767.0f * 0.95f;
    for (long long i = 0; i < n; i++) {
        const float t = y[i] * scale;
        if (!(fabsf(t) < 2147483648.0f)) {
            unspecified[i] = 1;
            out[i] = 0;
        } else {
            unspecified[i] = 0;
            out[i] = (int16_t)(uint16_t)((uint32_t)(int32_t)t & 0xffffu);
        }
    }
}
