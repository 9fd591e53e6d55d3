// Host-side arithmetic of the batched audio mixer (fmd_mix.hip): the reference's per-call scale, evaluated once per (gain, source count).
#pragma once

namespace fmd {

// AudioMixer::UpdateMixer's scale for k >= 1 delivering sources (audio_mixer.cpp:61-64): gain / log10f((float)k * 10.0f) with the
// host libm's log10f, the gain read and the quotient written the way the reference's FTZ + DAZ build does (denormal -> zero of its sign)
float mix_scale(float gain, int k);

}  // namespace fmd
