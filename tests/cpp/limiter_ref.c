/* The look-ahead peak limiter's arithmetic contract (include/fmdemod.h, "Look-ahead peak limiter"), restated sequentially: one frame at
 * a time, rings of W = D + 1 entries, every window walked in full.  Build with -O2 -ffp-contract=off and no fast-math: every float
 * operation is the one written. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define LIM_ONE 1073741824u
#define LIM_MAX_W 256

/* include/fmdemod.h fmd_limiter_status */
typedef struct {
    unsigned long long frames, limited, clamped[2], nonfinite;
    float min_gain, gain;
    unsigned eq;
    unsigned char reserved[12];
} lim_status;

typedef struct {
    lim_status st;
    int D;
    unsigned step;
    float T;
    unsigned long long pos;              /* frames since the reset or flush */
    unsigned rq[LIM_MAX_W], eq[LIM_MAX_W];
    float u[LIM_MAX_W][2];
} lim_chan;

static void lim_signal_reset(lim_chan* c) {
    int i;
    c->pos = 0;
    c->st.eq = LIM_ONE;
    for (i = 0; i < LIM_MAX_W; i++) { c->rq[i] = LIM_ONE; c->eq[i] = LIM_ONE; c->u[i][0] = 0.0f; c->u[i][1] = 0.0f; }
}

void limiter_ref_reset(lim_chan* c) {
    const float gain = c->st.gain;
    memset(&c->st, 0, sizeof(c->st));
    c->st.gain = gain;
    c->st.min_gain = 1.0f;
    lim_signal_reset(c);
}

int limiter_ref_create(lim_chan* c, int D, unsigned step, float T) {
    if (D < 0 || D >= LIM_MAX_W || step < 1u || step > LIM_ONE || !(T > 0.0f) || !(T <= 1.0f)) return -1;
    memset(c, 0, sizeof(*c));
    c->D = D; c->step = step; c->T = T;
    c->st.gain = 1.0f;
    limiter_ref_reset(c);
    return 0;
}

void limiter_ref_set_gain(lim_chan* c, float gain) { c->st.gain = gain; }

/* the gain the ceiling requires of a frame, Q30 */
unsigned limiter_ref_rq(float ul, float ur, float T) {
    const float al = fabsf(ul), ar = fabsf(ur), p = al > ar ? al : ar;
    if (p <= T) return LIM_ONE;
    return (unsigned)((T / p) * 1073741824.0f);
}

/* one frame in (already times the gain, finite), one frame out; returns g */
static float lim_frame(lim_chan* c, const float u[2], float y[2]) {
    const int W = c->D + 1;
    const int slot = (int)(c->pos % (unsigned long long)W), old = (int)((c->pos + 1u) % (unsigned long long)W);
    unsigned mq = LIM_ONE, eq;
    unsigned long long S = 0, next;
    float g;
    int i, r;
    c->rq[slot] = limiter_ref_rq(u[0], u[1], c->T);
    c->u[slot][0] = u[0]; c->u[slot][1] = u[1];
    for (i = 0; i < W; i++) mq = c->rq[i] < mq ? c->rq[i] : mq;             /* the look-ahead */
    next = (unsigned long long)c->st.eq + c->step;                           /* the release */
    eq = next < mq ? (unsigned)next : mq;
    c->st.eq = eq;
    c->eq[slot] = eq;
    for (i = 0; i < W; i++) S += c->eq[i];                                   /* the attack */
    g = (float)S / (float)((unsigned long long)W << 30);
    if (S < ((unsigned long long)W << 30)) c->st.limited++;
    if (g < c->st.min_gain) c->st.min_gain = g;
    for (r = 0; r < 2; r++) {                                                /* u[n - D] sits in the slot that frame n + 1 takes */
        float v = c->u[old][r] * g;
        if (v > c->T) { v = c->T; c->st.clamped[r]++; }
        else if (v < -c->T) { v = -c->T; c->st.clamped[r]++; }
        y[r] = v;
    }
    c->pos++;
    return g;
}

/* x [n][2] -> y [n][2]; returns the smallest g of the call's frames (1 for n = 0) */
float limiter_ref_process(lim_chan* c, const float* x, long long n, float* y) {
    float gmin = 1.0f;
    long long k;
    int r;
    for (k = 0; k < n; k++) {
        float u[2], g;
        for (r = 0; r < 2; r++) {
            u[r] = x[2 * k + r] * c->st.gain;
            if (!(fabsf(u[r]) <= 3.402823466e38f)) { u[r] = 0.0f; c->st.nonfinite++; }
        }
        g = lim_frame(c, u, y + 2 * k);
        gmin = g < gmin ? g : gmin;
    }
    c->st.frames += (unsigned long long)n;
    return gmin;
}

/* the D frames that D frames of silence push out -> y [D][2]; returns D */
int limiter_ref_flush(lim_chan* c, float* y) {
    const float zero[2] = {0.0f, 0.0f};
    int k;
    for (k = 0; k < c->D; k++) (void)lim_frame(c, zero, y + 2 * k);
    lim_signal_reset(c);
    return c->D;
}
