// Stand-alone check of the meter's host-only design and read-out (fm-radio_amd/csrc/fmd_meter_design.cpp, compiled in) for a sanitizer
// build: the true-peak design at every rate class, fmd_meter_dbtp, and fmd_meter_range over its edge cases (empty histogram, one bin,
// everything in bin 999, counts near 2^32, a population under the relative gate, null arguments).  Prints "ok" and returns 0, or says
// which check failed and returns 1.
#include <cmath>
#include <cstdio>
#include <vector>

#include "fmdemod.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

int main() {
    for (int fs : {8000, 32000, 44100, 48000, 96000, 192000}) {
        fmd_meter_tp_design_t tp;
        CHECK(fmd_meter_tp_design(fs, &tp) == FMD_OK);
        CHECK(tp.taps_per_phase == 12 && tp.L == (fs < 88200 ? 4 : fs < 176400 ? 2 : 1));
        for (int p = 1; p <= 3; p++) {
            double sum = 0.0;
            for (int k = 0; k < 12; k++) sum += (double)tp.taps[p - 1][k];
            if (p < tp.L) CHECK(std::fabs(sum - 1.0) <= 1e-6); else CHECK(sum == 0.0);
        }
    }
    fmd_meter_tp_design_t tp;
    CHECK(fmd_meter_tp_design(44101, &tp) == FMD_ERR_ARG && fmd_meter_tp_design(7990, &tp) == FMD_ERR_ARG);
    CHECK(fmd_meter_tp_design(48000, nullptr) == FMD_ERR_ARG);
    CHECK(fmd_meter_dbtp(1.0f) == 0.0 && std::isinf(fmd_meter_dbtp(0.0f)) && fmd_meter_dbtp(0.0f) < 0.0);
    CHECK(std::fabs(fmd_meter_dbtp(0.5f) + 6.0206) < 1e-4);

    auto* d = new fmd_meter_design_t;
    CHECK(fmd_meter_design(48000, d) == FMD_OK);
    std::vector<unsigned> h(1000, 0u);
    double lra = -1.0, low = 0.0, high = 0.0;
    CHECK(fmd_meter_range(h.data(), d, &lra, &low, &high) == FMD_ERR_STATE);             // empty
    CHECK(fmd_meter_range(nullptr, d, &lra, &low, &high) == FMD_ERR_ARG && fmd_meter_range(h.data(), nullptr, &lra, &low, &high) == FMD_ERR_ARG);
    CHECK(fmd_meter_range(h.data(), d, nullptr, &low, &high) == FMD_ERR_ARG);
    h[470] = 7;                                                                          // one bin
    CHECK(fmd_meter_range(h.data(), d, &lra, &low, &high) == FMD_OK && lra == 0.0 && low == high && std::fabs(low + 22.95) < 1e-9);
    h.assign(1000, 0u);
    h[999] = 0xffffffffu;                                                                // everything in the last bin, a count near 2^32
    CHECK(fmd_meter_range(h.data(), d, &lra, &low, &high) == FMD_OK && lra == 0.0 && std::fabs(high - 29.95) < 1e-9);
    h.assign(1000, 0xfffffff0u);                                                         // every bin near 2^32: the gate drops the low ones
    CHECK(fmd_meter_range(h.data(), d, &lra, &low, &high) == FMD_OK && lra > 0.0 && lra <= 99.9 && low < high && high <= 29.95 + 1e-9);
    h.assign(1000, 0u);
    h[400] = h[500] = 100;                                                               // two plateaus 10 LU apart
    CHECK(fmd_meter_range(h.data(), d, &lra, &low, &high) == FMD_OK && lra == 10.0);
    h[100] = 100;                                                                        // 40 LU under: dropped by the -20 LU gate
    CHECK(fmd_meter_range(h.data(), d, &lra, &low, &high) == FMD_OK && lra == 10.0 && std::fabs(low + 29.95) < 1e-9);
    h.assign(1000, 0u);
    h[0] = 1;
    CHECK(fmd_meter_range(h.data(), d, &lra, &low, &high) == FMD_OK && lra == 0.0 && std::fabs(low + 69.95) < 1e-9);
    delete d;
    if (failures == 0) printf("ok\n");
    return failures == 0 ? 0 : 1;
}
