/* Restatement of the reference's Resampled_PCM_Player::ConsumeBuffer + Resample (reference
 * src/audio/resampled_pcm_player.cpp:15-54) as its -O2 -ffast-math build evaluates it (DESIGN.md "Audio resampler"):
 * one scalar loop, the running index j a chain of single-precision adds, w0 = (1 - j) + jf, out = fmaf(f1, k, f0 * w0).
 * Build with -ffp-contract=off -fno-fast-math so that every operation is the one written. */
#include <math.h>

/* in, out: [n][2] interleaved frames.  Returns n_out; -1 where the running index leaves the input (the reference's span
 * indexing would abort there) — nothing is written then; -2 if cap is too small. */
int resample_ref(const float* in, int n_in, int fs_in, int fs_out, float* out, int cap) {
    if (fs_in == fs_out) {
        if (n_in > cap) return -2;
        for (int i = 0; i < 2 * n_in; i++) out[i] = in[i];
        return n_in;
    }
    const float Lf = (float)fs_out / (float)fs_in;
    const int n_out = (int)(Lf * (float)n_in);
    if (n_out > cap) return -2;
    const float step = (float)n_in / (float)n_out;
    float j = 0.0f;
    for (int i = 0; i < n_out; i++) {
        if ((int)j >= n_in) return -1;
        j += step;
    }
    j = 0.0f;
    for (int i = 0; i < n_out; i++) {
        const int j0 = (int)j;
        const int j1 = (j0 + 1 < n_in) ? j0 + 1 : j0;
        const float jf = (float)j0;
        const float w0 = (1.0f - j) + jf;
        const float k = j - jf;
        out[2 * i] = fmaf(in[2 * j1], k, in[2 * j0] * w0);
        out[2 * i + 1] = fmaf(in[2 * j1 + 1], k, in[2 * j0 + 1] * w0);
        j += step;
    }
    return n_out;
}
