// Host-side tables of the batched audio resampler (fmd_resample.hip).  Compiled with the library's -ffp-contract=off
// -fno-fast-math: every float operation below is the one written, in the order written.
//
// Reference method.  g++ 11.4 -O2 -ffast-math -march=x86-64-v3 (the reference's build, oracle/Makefile REF_CXXFLAGS) compiles
// Resample() (reference src/audio/resampled_pcm_player.cpp:37-54) to a scalar loop that evaluates
//     step = (float)N / (float)n_out;  j = 0, then j += step after each output (sequential single-precision adds)
//     j0 = (int)j;  jf = (float)j0;  w0 = (1.0f - j) + jf  (Frame * (1 - k) reassociated);  k = j - jf
//     out = fmaf(f1, k, f0 * w0)   per channel (vfmadd231ss / vfmadd132ss over a vmulss)
// The chain depends on (N, n_out) alone, so it is evaluated here once per input length and the kernel is a gather and two
// operations per value (DESIGN.md "Audio resampler").
#include "fmd_resample_design.h"

#include "fmd_bessel.h"

#include <math.h>

#include <algorithm>
#include <numeric>

namespace fmd {

int resample_ref_frames(int fs_in, int fs_out, long long n_in) {
    const float Lf = (float)fs_out / (float)fs_in;
    return (int)(Lf * (float)n_in);
}

bool resample_ref_table(int n_in, int n_out, std::vector<ResampleRefTap>* tab) {
    std::vector<ResampleRefTap> t((size_t)(n_out > 0 ? n_out : 0));
    const float step = (float)n_in / (float)n_out;
    float j = 0.0f;
    for (int i = 0; i < n_out; i++) {
        const int j0 = (int)j;
        if (j0 < 0 || j0 >= n_in) return false;        // the reference's span indexing would abort here
        const float jf = (float)j0;
        t[(size_t)i] = ResampleRefTap{j0, (1.0f - j) + jf, j - jf, 0};
        j += step;
    }
    tab->swap(t);
    return true;
}

// Kaiser-windowed sinc at the up-sampled rate L fs_in (Kaiser's estimates for the window: beta = 0.1102 (A - 8.7) and
// transition width (A - 7.95) / (14.36 (N - 1)) of the rate), its stopband starting at min(fs_in, fs_out) / 2: the image
// band of an interpolator, the alias band of a decimator.  A = 70 dB keeps >= 60 dB after the per-phase normalisation below.
bool resample_poly_design(int fs_in, int fs_out, int T, std::vector<float>* taps, int* L_out, int* M_out) {
    if (fs_in <= 0 || fs_out <= 0 || fs_in > 1000000 || fs_out > 1000000 || T < 8 || T > 256) return false;
    const int g = std::gcd(fs_in, fs_out);
    const int L = fs_out / g, M = fs_in / g;
    if (L > 4096 || M > 4096 || (long long)L * T > (1 << 20)) return false;
    if (L_out) *L_out = L;
    if (M_out) *M_out = M;
    if (!taps) return true;
    const int N = L * T;
    std::vector<double> h((size_t)N, 0.0);
    if (L == 1 && M == 1) {
        h[0] = 1.0;                                               // (a call passes the input through; the identity filter)
    } else {
        const double A = 70.0, beta = 0.1102 * (A - 8.7);
        const double F = (double)L * (double)fs_in;
        const double f_stop = 0.5 * (double)std::min(fs_in, fs_out);
        const double df = (A - 7.95) / (14.36 * (double)(N - 1)) * F;
        const double fc = f_stop - 0.5 * df;
        if (!(fc > 0.25 * f_stop)) return false;                  // too few taps for this ratio
        const double wc = 2.0 * fc / F;                            // cut-off, cycles per up-sampled sample x 2
        const double mid = 0.5 * (double)(N - 1), i0b = bessel_i0(beta);
        for (int n = 0; n < N; n++) {
            const double x = (double)n - mid, r = x / mid;
            const double s = (x == 0.0) ? wc : sin(M_PI * wc * x) / (M_PI * x);
            h[(size_t)n] = s * bessel_i0(beta * sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
        }
        // every phase passes DC with gain 1 (the prototype's gain is L)
        for (int p = 0; p < L; p++) {
            double sum = 0.0;
            for (int t = 0; t < T; t++) sum += h[(size_t)p + (size_t)t * L];
            for (int t = 0; t < T; t++) h[(size_t)p + (size_t)t * L] /= sum;
        }
    }
    taps->assign((size_t)N, 0.0f);
    for (int n = 0; n < N; n++) (*taps)[(size_t)n] = (float)h[(size_t)n];   // n = p + t L: [t][p]
    return true;
}

}  // namespace fmd
