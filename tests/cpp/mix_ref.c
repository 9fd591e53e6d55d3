/* Restatement of the reference's AudioMixer::UpdateMixer (reference src/audio/audio_mixer.cpp:33-79) as its -O2 -ffast-math
 * build evaluates it: n = the sources that delivered a block, scale = gain / log10f((float)n * 10.0f),
 * acc = fmaf(x, scale, acc) in registration order from +0, then the clamp in x86's vmaxss / vminss operand order.  The build links
 * crtfastmath (FTZ + DAZ): denormal inputs act as zeros of their sign, denormal results become zeros of their sign.
 * Build with -ffp-contract=off -fno-fast-math so that every operation is the one written and the flushing is explicit.
 * Limitation: scale uses this host's libm log10f; the fixture pins glibc 2.35's, which is not correctly rounded. */
#include <math.h>
#include <stdint.h>

static float ftz(float v) { return (v != 0.0f && fabsf(v) < 1.17549435e-38f) ? copysignf(0.0f, v) : v; }

/* the scale for k delivering sources (k >= 1); f64_log: log10 in float64 rounded to float instead of log10f */
float mix_ref_scale(float gain, int k, int f64_log) {
    const float l = f64_log ? (float)log10((double)((float)k * 10.0f)) : log10f((float)k * 10.0f);
    return ftz(ftz(gain) / l);
}

/* x: [C][stride][2] station frames; sources: n_src station rows in registration order; active: [C], NULL = all deliver.
 * out: [n][2].  Returns the number of delivering sources. */
int mix_ref(const float* x, long long stride, int n, const int* sources, int n_src, const uint8_t* active, float gain, int f64_log,
            float* out) {
    int k = 0;
    for (int s = 0; s < n_src; s++) k += !active || active[sources[s]];
    const float scale = k > 0 ? mix_ref_scale(gain, k, f64_log) : 0.0f;
    for (int i = 0; i < 2 * n; i++) {
        float acc = 0.0f;
        if (k > 0) {
            for (int s = 0; s < n_src; s++) {
                if (active && !active[sources[s]]) continue;
                acc = ftz(fmaf(ftz(x[(long long)sources[s] * stride * 2 + i]), scale, acc));
            }
            const float t = (-1.0f > acc) ? -1.0f : acc;          /* vmaxss: the second operand (acc) when unordered */
            acc = (t < 1.0f) ? t : 1.0f;                          /* vminss: the second operand (1) when unordered */
        }
        out[i] = acc;
    }
    return k;
}
