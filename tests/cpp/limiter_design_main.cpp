// The limiter's host-only unit (fm-radio_amd/csrc/fmd_limiter_design.cpp) as a stand-alone program, for a build under sanitizers: the
// design at its bounds, the defaults, the loudness helper, and the process call's checks with each bound held from both sides.  Prints
// "ok"; the exit status names the first check that failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "fmd_limiter_design.h"

#define CHECK(k, cond) do { if (!(cond)) { fprintf(stderr, "check %d failed: %s\n", k, #cond); return k; } } while (0)

int main() {
    fmd_limiter_design_t d;
    CHECK(1, fmd_limiter_design(32000, 1.5, 500.0, -1.0, &d) == FMD_OK && d.lookahead_frames == 48 && d.latency_frames == 48 && d.step == 67109u);
    CHECK(2, d.ceiling == (float)std::pow(10.0, -1.0 / 20.0));
    CHECK(3, fmd_limiter_design(32000, 0.0, 0.0, 0.0, &d) == FMD_OK && d.lookahead_frames == 0 && d.step == fmd::kLimiterOne && d.ceiling == 1.0f);
    CHECK(4, fmd_limiter_design(32000, 255.0 / 32.0, 1e11, -40.0, &d) == FMD_OK && d.lookahead_frames == 255 && d.step == 1u && d.ceiling == 0.01f);
    CHECK(5, fmd_limiter_design(32000, 256.0 / 32.0, 500.0, -1.0, &d) == FMD_ERR_ARG && !fmd::limiter_global_error().empty());
    CHECK(6, fmd_limiter_design(7999, 1.5, 500.0, -1.0, &d) == FMD_ERR_ARG && fmd_limiter_design(192001, 1.5, 500.0, -1.0, &d) == FMD_ERR_ARG);
    CHECK(7, fmd_limiter_design(32000, -1.0, 500.0, -1.0, &d) == FMD_ERR_ARG && fmd_limiter_design(32000, 1.5, -1.0, -1.0, &d) == FMD_ERR_ARG);
    CHECK(8, fmd_limiter_design(32000, 1.5, 500.0, 0.5, &d) == FMD_ERR_ARG && fmd_limiter_design(32000, 1.5, 500.0, NAN, &d) == FMD_ERR_ARG);
    CHECK(9, fmd_limiter_design(32000, 1.5, 500.0, -1.0, nullptr) == FMD_ERR_ARG);
    fmd_limiter_config cfg;
    CHECK(10, fmd_limiter_default_config(48000, &cfg) == FMD_OK && cfg.fs == 48000 && cfg.lookahead_ms == 1.5 && cfg.release_ms == 500.0 && cfg.ceiling_db == -1.0);
    CHECK(11, fmd_limiter_default_config(48000, nullptr) == FMD_ERR_ARG && fmd_limiter_default_config(100, &cfg) == FMD_ERR_ARG);
    CHECK(12, fmd_limiter_gain_for_loudness(-23.0, -23.0) == 1.0f && fmd_limiter_gain_for_loudness(-17.0, -23.0) == (float)std::pow(10.0, -6.0 / 20.0));

    // the call's checks: three rows of 100 frames, 16 taken; addresses only, nothing is dereferenced
    std::string err;
    const uintptr_t base = 1u << 20;
    auto at = [&](long long frame) { return reinterpret_cast<const void*>(base + 8u * (uintptr_t)frame); };
    auto call = [&](const void* in, long long is, long long n, const void* out, long long os) { return fmd::limiter_check_call(3, 64, in, is, n, out, os, &err); };
    CHECK(20, call(at(0), 100, 16, at(1000), 100) == FMD_OK);
    CHECK(21, call(nullptr, 100, 16, at(1000), 100) == FMD_ERR_ARG && call(at(0), 100, 16, nullptr, 100) == FMD_ERR_ARG);
    CHECK(22, call(reinterpret_cast<const void*>(base + 4), 100, 16, at(1000), 100) == FMD_ERR_ARG && call(at(0), 100, 16, reinterpret_cast<const void*>(base + 8004), 100) == FMD_ERR_ARG);
    CHECK(23, call(at(0), 100, -1, at(1000), 100) == FMD_ERR_ARG && call(at(0), 100, 0, at(1000), 100) == FMD_OK);
    CHECK(24, call(at(0), 15, 16, at(1000), 100) == FMD_ERR_ARG && call(at(0), 16, 16, at(1000), 100) == FMD_OK);
    CHECK(25, call(at(0), 100, 16, at(1000), 15) == FMD_ERR_ARG && call(at(0), 100, 16, at(1000), 16) == FMD_OK);
    CHECK(26, call(at(0), 100, 65, at(1000), 100) == FMD_ERR_ARG && call(at(0), 100, 64, at(1000), 100) == FMD_OK && !err.empty());
    // the input's bytes are frames 0 ... 215: an output from 215 on overlaps, from 216 on does not; the same from the other side
    CHECK(27, call(at(0), 100, 16, at(0), 100) == FMD_ERR_ARG && call(at(0), 100, 16, at(215), 100) == FMD_ERR_ARG && call(at(0), 100, 16, at(216), 100) == FMD_OK);
    CHECK(28, call(at(215), 100, 16, at(0), 100) == FMD_ERR_ARG && call(at(216), 100, 16, at(0), 100) == FMD_OK);
    CHECK(29, call(at(0), 100, 0, at(0), 100) == FMD_OK);                    // nothing is read or written
    printf("ok\n");
    return 0;
}
