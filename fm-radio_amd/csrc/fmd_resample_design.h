// Host-side tables of the batched audio resampler (see fmd_resample_design.cpp).
#pragma once

#include <vector>

namespace fmd {

// one output frame of the reference method: out = fmaf(f1, k, f0 * w0), f0 = in[j0], f1 = in[min(j0 + 1, N - 1)]
struct ResampleRefTap { int j0; float w0; float k; int pad; };

// the reference's n_out for an n_in-frame ConsumeBuffer (resampled_pcm_player.cpp:22-24)
int resample_ref_frames(int fs_in, int fs_out, long long n_in);
// Resample()'s index chain for (n_in, n_out); false (nothing written) where the running index leaves the input
bool resample_ref_table(int n_in, int n_out, std::vector<ResampleRefTap>* tab);
// polyphase prototype, [t][p] = h[p + t L]; false for unsupported rates or T
bool resample_poly_design(int fs_in, int fs_out, int T, std::vector<float>* taps, int* L, int* M);

}  // namespace fmd
