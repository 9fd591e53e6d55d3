// The log-mel front end's host-only unit (fmd_logmel_design.cpp) as a stand-alone program, for tests/test_logmel_cpu.py: built from source
// under -fsanitize=address,undefined, and linked against libfmdemod.so as built.  Every array has exactly the size the header states, on the
// heap, so that a write past an end is seen.
//
//   logmel_design_main OUTDIR [fs win hop n_mels f_min f_max mel_scale]...
//
// Per geometry it writes OUTDIR/logmel_<i>.f32 = w [N], tc [N], ts [N], fb [n_mels][K] and prints "K empty_bands"; then it runs the
// smallest and the largest valid designs, invalid ones (which must write nothing), the default configurations, fmd_logmel_max_frames and
// fmd_logmel_flog10's special values, and prints "ok".
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "fmdemod.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static fmd_logmel_config geometry(int fs, int win, int hop, int n_mels, double f_min, double f_max, int scale) {
    fmd_logmel_config c;
    std::memset(&c, 0, sizeof(c));
    c.n_channels = 1; c.fs = fs; c.win = win; c.hop = hop; c.n_mels = n_mels; c.f_min_hz = f_min; c.f_max_hz = f_max; c.mel_scale = scale;
    c.out_mode = 1; c.log_floor = 1e-10f; c.max_input_frames = 65536; c.device = -1;
    return c;
}

// designs `c` into exact-size arrays; K and empty_bands out; the arrays into `path` if given
static int design(const fmd_logmel_config& c, int* K_out, int* empty_out, const char* path) {
    const int K = fmd_logmel_bins(&c);
    if (K <= 0) return 1;
    const size_t N = (size_t)c.win, F = (size_t)c.n_mels * (size_t)K;
    std::unique_ptr<float[]> w(new float[N]), tc(new float[N]), ts(new float[N]), fb(new float[F]);
    fmd_logmel_design_t d;
    if (fmd_logmel_design(&c, w.get(), tc.get(), ts.get(), fb.get(), &d) != FMD_OK || d.n_bins != K) return 1;
    // each array alone, the others null
    std::unique_ptr<float[]> w2(new float[N]), fb2(new float[F]);
    if (fmd_logmel_design(&c, w2.get(), nullptr, nullptr, nullptr, nullptr) != FMD_OK || std::memcmp(w.get(), w2.get(), 4 * N) != 0) return 1;
    if (fmd_logmel_design(&c, nullptr, nullptr, nullptr, fb2.get(), nullptr) != FMD_OK || std::memcmp(fb.get(), fb2.get(), 4 * F) != 0) return 1;
    if (fmd_logmel_design(&c, nullptr, nullptr, nullptr, nullptr, nullptr) != FMD_OK) return 1;
    if (path) {
        FILE* f = std::fopen(path, "wb");
        if (!f) return 1;
        std::fwrite(w.get(), 4, N, f); std::fwrite(tc.get(), 4, N, f); std::fwrite(ts.get(), 4, N, f); std::fwrite(fb.get(), 4, F, f);
        std::fclose(f);
    }
    *K_out = K; *empty_out = d.empty_bands;
    return 0;
}

int main(int argc, char** argv) {
    CHECK(argc >= 2 && (argc - 2) % 7 == 0);
    const std::string dir = argv[1];
    int K = 0, empty = 0;
    for (int i = 0; 2 + 7 * i < argc; i++) {
        char** a = argv + 2 + 7 * i;
        const fmd_logmel_config c = geometry(std::atoi(a[0]), std::atoi(a[1]), std::atoi(a[2]), std::atoi(a[3]), std::atof(a[4]), std::atof(a[5]), std::atoi(a[6]));
        CHECK(design(c, &K, &empty, (dir + "/logmel_" + std::to_string(i) + ".f32").c_str()) == 0);
        std::printf("%d %d\n", K, empty);
    }
    // the smallest design: one bin, one band; and the largest: 2048 / 1025 bins / 128 bands
    CHECK(design(geometry(48000, 64, 16, 1, 0.0, 1.0, 0), &K, &empty, nullptr) == 0 && K == 1);
    CHECK(design(geometry(8000, 2048, 2048, 128, 0.0, 4000.0, 1), &K, &empty, nullptr) == 0 && K == 1025);
    CHECK(design(geometry(8000, 64, 16, 40, 0.0, 4000.0, 0), &K, &empty, nullptr) == 0 && K == 33 && empty > 0);
    // invalid ones write nothing: one-float arrays stay as they are
    {
        const fmd_logmel_config bad[] = {geometry(7999, 64, 16, 8, 0, 3000, 0), geometry(48001, 64, 16, 8, 0, 3000, 0), geometry(8000, 48, 16, 8, 0, 3000, 0),
                                         geometry(8000, 72, 16, 8, 0, 3000, 0), geometry(8000, 2064, 16, 8, 0, 3000, 0), geometry(8000, 64, 15, 8, 0, 3000, 0),
                                         geometry(8000, 64, 65, 8, 0, 3000, 0), geometry(8000, 64, 16, 0, 0, 3000, 0), geometry(8000, 64, 16, 129, 0, 3000, 0),
                                         geometry(8000, 64, 16, 8, -1.0, 3000, 0), geometry(8000, 64, 16, 8, 3000, 3000, 0), geometry(8000, 64, 16, 8, 0, 4000.5, 0),
                                         geometry(8000, 64, 16, 8, 0, NAN, 0), geometry(8000, 64, 16, 8, 0, 3000, 2), geometry(8000, 64, 16, 8, 0, 3000, -1)};
        for (const fmd_logmel_config& c : bad) {
            std::unique_ptr<float[]> one(new float[1]);
            one[0] = 42.0f;
            fmd_logmel_design_t d = {-7, -7};
            CHECK(fmd_logmel_design(&c, one.get(), one.get(), one.get(), one.get(), &d) == FMD_ERR_ARG);
            CHECK(one[0] == 42.0f && d.n_bins == -7 && d.empty_bands == -7);
            CHECK(fmd_logmel_bins(&c) == FMD_ERR_ARG);
        }
        fmd_logmel_config c = geometry(8000, 64, 16, 8, 0, 3000, 0);
        c.out_mode = 2; CHECK(fmd_logmel_bins(&c) == FMD_ERR_ARG); c.out_mode = 0; CHECK(fmd_logmel_bins(&c) == 25);
        c.log_floor = 0.0f; CHECK(fmd_logmel_bins(&c) == FMD_ERR_ARG); c.log_floor = FLT_MIN; CHECK(fmd_logmel_bins(&c) == 25);
        c.log_floor = INFINITY; CHECK(fmd_logmel_bins(&c) == FMD_ERR_ARG); c.log_floor = NAN; CHECK(fmd_logmel_bins(&c) == FMD_ERR_ARG);
        c.log_floor = FLT_MAX; CHECK(fmd_logmel_bins(&c) == 25);
        c.n_channels = 0; CHECK(fmd_logmel_bins(&c) == FMD_ERR_ARG); c.n_channels = 1;
        c.max_input_frames = 0; CHECK(fmd_logmel_bins(&c) == FMD_ERR_ARG);
        c.max_input_frames = (1LL << 30) + 1; CHECK(fmd_logmel_bins(&c) == FMD_ERR_ARG);
        c.max_input_frames = 1LL << 30; CHECK(fmd_logmel_bins(&c) == 25);
        CHECK(fmd_logmel_design(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == FMD_ERR_ARG);
    }
    // the default configurations
    for (int fs : {8000, 16000, 22050, 32000, 44100, 48000}) {
        fmd_logmel_config c;
        CHECK(fmd_logmel_default_config(fs, &c) == FMD_OK && c.win % 16 == 0 && c.win >= fs / 40 && c.win < fs / 40 + 16 && c.hop == fs / 100);
        CHECK(design(c, &K, &empty, nullptr) == 0);
        std::printf("default %d %d %d %d %d\n", fs, c.win, c.hop, K, empty);
    }
    {
        fmd_logmel_config c;
        CHECK(fmd_logmel_default_config(7999, &c) == FMD_ERR_ARG && fmd_logmel_default_config(48001, &c) == FMD_ERR_ARG);
        CHECK(fmd_logmel_default_config(8000, nullptr) == FMD_ERR_ARG);
    }
    CHECK(fmd_logmel_max_frames(16, 0) == 0 && fmd_logmel_max_frames(16, 1) == 1 && fmd_logmel_max_frames(16, 16) == 1 && fmd_logmel_max_frames(16, 17) == 2);
    CHECK(fmd_logmel_max_frames(2048, 1LL << 40) == (1LL << 29) && fmd_logmel_max_frames(320, 2048) == 7);
    CHECK(fmd_logmel_max_frames(15, 1) == FMD_ERR_ARG && fmd_logmel_max_frames(2049, 1) == FMD_ERR_ARG && fmd_logmel_max_frames(16, -1) == FMD_ERR_ARG);
    CHECK(fmd_logmel_max_frames(16, (1LL << 40) + 1) == FMD_ERR_ARG);
    CHECK(fmd_logmel_flog10(1.0f) == 0.0f && fmd_logmel_flog10(INFINITY) == INFINITY && std::isnan(fmd_logmel_flog10(NAN)));
    CHECK(std::fabs(fmd_logmel_flog10(FLT_MIN) - std::log10((double)FLT_MIN)) < 1e-5 && std::fabs(fmd_logmel_flog10(FLT_MAX) - std::log10((double)FLT_MAX)) < 1e-5);
    std::printf("ok\n");
    return 0;
}
