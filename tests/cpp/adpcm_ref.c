/* The ADPCM audio encoder's arithmetic contract (include/fmdemod.h, "ADPCM audio encoder") restated in plain C, one station at a time,
 * frame by frame and nibble by nibble: what the GPU tests compare the device's bytes and records with, and what
 * tests/test_adpcm_cpu.py compares with Python's audioop.  Written from the contract's description and the published IMA / DVI tables;
 * shares no code with the library. */
#include <math.h>
#include <stdint.h>
#include <string.h>

static const int STEP[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157, 173, 190, 209, 230,
    253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327,
    3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};
static const int ADJUST[8] = {-1, -1, -1, -1, 2, 4, 6, 8};

/* include/fmdemod.h fmd_adpcm_status */
typedef struct {
    unsigned long long frames, blocks, padded, clipped[2], nonfinite;
    unsigned fill;
    short pred[2];
    unsigned char index[2], reserved[6];
} adpcm_ref_status;

typedef struct {
    adpcm_ref_status st;
    int S, align;
    int last_q[2];             /* the last real frame's samples */
    unsigned char open[8192];  /* the open block's bytes */
} adpcm_ref_chan;

int adpcm_ref_block_frames(int S) { return S == 0 ? 1017 : (S >= 9 && S <= 8185 && S % 8 == 1 ? S : 0); }
int adpcm_ref_block_align(int S) { return 8 * ((S - 1) / 8 + 1); }
long long adpcm_ref_max_blocks(int S, long long n) { return ((long long)S - 1 + n) / S; }

/* the sample: *flag = 0 in range, 1 clamped, 2 not finite */
int adpcm_ref_sample(float x, int* flag) {
    volatile float t = x * (32767.0f * 0.95f);
    *flag = 0;
    if (isnan(t) || isinf(t)) { *flag = 2; return 0; }
    if (t >= 2147483648.0f || t <= -2147483648.0f) { *flag = 1; return t > 0.0f ? 32767 : -32768; }   /* (int)t would not be defined */
    int v = (int)t;
    if (v > 32767) { *flag = 1; return 32767; }
    if (v < -32768) { *flag = 1; return -32768; }
    return v;
}

/* the quantiser's step on one rail: the 4-bit code */
int adpcm_ref_step(int q, int* pred, int* index) {
    int step = STEP[*index];
    int diff = q - *pred, code = 0;
    if (diff < 0) { code = 8; diff = -diff; }
    int vpdiff = step >> 3;
    if (diff >= step) { code |= 4; diff -= step; vpdiff += step; }
    step >>= 1;
    if (diff >= step) { code |= 2; diff -= step; vpdiff += step; }
    step >>= 1;
    if (diff >= step) { code |= 1; vpdiff += step; }
    int p = (code & 8) ? *pred - vpdiff : *pred + vpdiff;
    if (p > 32767) p = 32767;
    if (p < -32768) p = -32768;
    *pred = p;
    int i = *index + ADJUST[code & 7];
    if (i < 0) i = 0;
    if (i > 88) i = 88;
    *index = i;
    return code;
}

void adpcm_ref_reset(adpcm_ref_chan* ch) {
    memset(&ch->st, 0, sizeof(ch->st));
    memset(ch->open, 0, sizeof(ch->open));
    ch->last_q[0] = ch->last_q[1] = 0;
}

int adpcm_ref_create(adpcm_ref_chan* ch, int S) {
    memset(ch, 0, sizeof(*ch));
    ch->S = adpcm_ref_block_frames(S);
    if (ch->S == 0) return -1;
    ch->align = adpcm_ref_block_align(ch->S);
    return 0;
}

/* one frame (qL, qR) into the open block; 1 where it completed the block, which is then copied to out */
static int frame(adpcm_ref_chan* ch, const int* q, unsigned char* out) {
    const int fill = (int)ch->st.fill;
    for (int rail = 0; rail < 2; rail++) {
        int pred = ch->st.pred[rail], index = ch->st.index[rail];
        if (fill == 0) {
            unsigned char* h = ch->open + 4 * rail;
            pred = q[rail];
            h[0] = (unsigned char)(q[rail] & 255); h[1] = (unsigned char)((q[rail] >> 8) & 255); h[2] = (unsigned char)index; h[3] = 0;
        } else {
            const int code = adpcm_ref_step(q[rail], &pred, &index), k = fill - 1;
            unsigned char* b = ch->open + 8 + 8 * (k / 8) + 4 * rail + (k % 8) / 2;
            if (k % 2 == 0) *b = (unsigned char)code;
            else *b = (unsigned char)(*b | (code << 4));
        }
        ch->st.pred[rail] = (short)pred;
        ch->st.index[rail] = (unsigned char)index;
    }
    ch->st.fill++;
    if ((int)ch->st.fill < ch->S) return 0;
    memcpy(out, ch->open, (size_t)ch->align);
    ch->st.fill = 0;
    ch->st.blocks++;
    return 1;
}

/* n frames x [n][2]; the completed blocks back to back into out; returns their number */
long long adpcm_ref_process(adpcm_ref_chan* ch, const float* x, long long n, unsigned char* out) {
    long long nb = 0;
    for (long long i = 0; i < n; i++) {
        int q[2];
        for (int rail = 0; rail < 2; rail++) {
            int flag;
            q[rail] = adpcm_ref_sample(x[2 * i + rail], &flag);
            if (flag == 1) ch->st.clipped[rail]++;
            if (flag == 2) ch->st.nonfinite++;
        }
        ch->last_q[0] = q[0]; ch->last_q[1] = q[1];
        ch->st.frames++;
        nb += frame(ch, q, out + nb * ch->align);
    }
    return nb;
}

/* closes the open block with repeats of the last real frame; returns 0 or 1 */
int adpcm_ref_flush(adpcm_ref_chan* ch, unsigned char* out) {
    if (ch->st.fill == 0) return 0;
    for (;;) {
        ch->st.padded++;
        if (frame(ch, ch->last_q, out)) return 1;
    }
}

/* blocks [nblocks][align] -> pcm [nblocks * S][2]; -1 for a header index above 88 */
int adpcm_ref_decode(const unsigned char* blocks, int S, long long nblocks, short* pcm) {
    const int align = adpcm_ref_block_align(S);
    for (long long b = 0; b < nblocks; b++) {
        const unsigned char* blk = blocks + b * align;
        for (int rail = 0; rail < 2; rail++) {
            int pred = (short)(blk[4 * rail] | (blk[4 * rail + 1] << 8)), index = blk[4 * rail + 2];
            if (index > 88) return -1;
            pcm[(b * S) * 2 + rail] = (short)pred;
            for (int i = 1; i < S; i++) {
                const int k = i - 1;
                const unsigned char byte = blk[8 + 8 * (k / 8) + 4 * rail + (k % 8) / 2];
                const int code = (k % 2) ? byte >> 4 : byte & 15;
                const int step = STEP[index];
                int vpdiff = step >> 3;
                if (code & 4) vpdiff += step;
                if (code & 2) vpdiff += step >> 1;
                if (code & 1) vpdiff += step >> 2;
                pred = (code & 8) ? pred - vpdiff : pred + vpdiff;
                if (pred > 32767) pred = 32767;
                if (pred < -32768) pred = -32768;
                index += ADJUST[code & 7];
                if (index < 0) index = 0;
                if (index > 88) index = 88;
                pcm[(b * S + i) * 2 + rail] = (short)pred;
            }
        }
    }
    return 0;
}
