// Host-side half of the EAS SAME decoder (fmd_same.hip): the cos / sin table and the two tones' steps, the tick boundaries, the
// parameters' validation, and the header's encoder, parser and vote (include/fmdemod.h, "EAS SAME decoder"), in double.  Needs no GPU.
#pragma once
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kSameTickPeriod = 12500;  // ticks after which the tick boundaries repeat: 12500 ticks are exactly 3 fs frames
constexpr int kSameHist = 7;            // completed ticks whose sums a decision needs besides its own

// the table's length and the two tones' steps through it
struct SameGeometry {
    int P, mark_step, space_step;
};

// the message of the last failing call that has no decoder handle (fmd_same_create, the host functions)
std::string& same_global_error();
// false unless fs is a multiple of 10 in 8000 ... 48000
bool same_geometry(int fs, SameGeometry* g);
// tab [P][2]: cos and sin of 2 pi j / P
void same_table(int P, double* tab);
// B(r) - B(0) for r = 0 ... 12500: (r * 3 fs + 12499) / 12500
unsigned same_tick_start(int fs, unsigned r);
// FMD_OK for valid parameters; FMD_ERR_ARG and the reason in *err otherwise
int same_check_params(const fmd_same_params* p, std::string* err);

}  // namespace fmd
