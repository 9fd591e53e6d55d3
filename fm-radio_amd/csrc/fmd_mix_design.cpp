// Built with -ffp-contract=off -fno-fast-math (Makefile): every float operation is the one written, and the flushing the reference's
// MXCSR does in hardware is done here explicitly.
#include "fmd_mix_design.h"

#include <cfloat>
#include <cmath>

namespace fmd {

static float flush(float v) { return (v != 0.0f && std::fabs(v) < FLT_MIN) ? std::copysign(0.0f, v) : v; }

float mix_scale(float gain, int k) {
    const float l = ::log10f((float)k * 10.0f);   // vcvtsi2ss, vmulss by 10, glibc's log10f (not correctly rounded)
    return flush(flush(gain) / l);                 // vdivss under DAZ + FTZ
}

}  // namespace fmd
