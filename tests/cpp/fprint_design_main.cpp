// The audio fingerprinter's host-only unit (fmd_fprint_design.cpp) as a stand-alone program, for tests/test_fprint_cpu.py: built from
// source under -fsanitize=address,undefined, and linked against libfmdemod.so as built.  Every array has exactly the size the header
// states, on the heap, so that a write past an end is seen.
//
//   fprint_design_main OUTDIR [fs hop n_sub n_bands f_min f_max]...
//
// Per geometry it writes OUTDIR/fprint_<i>.f32 = bc [H][K], bs [H][K], wc [R], ws [R] and prints "K first_bin edges..."; then it runs the
// smallest and the largest valid designs, invalid ones (which must write nothing), the default configurations, fmd_fprint_max_prints and
// fmd_fprint_state_bytes, and prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "fmdemod.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static fmd_fprint_config geometry(int fs, int hop, int n_sub, int n_bands, double f_min, double f_max) {
    fmd_fprint_config c;
    std::memset(&c, 0, sizeof(c));
    c.n_channels = 1; c.fs = fs; c.hop = hop; c.n_sub = n_sub; c.n_bands = n_bands; c.f_min_hz = f_min; c.f_max_hz = f_max;
    c.max_input_frames = 65536; c.device = -1;
    return c;
}

// designs `c` into exact-size arrays; K and first_bin out; the arrays into `path` if given; the edges printed if `print`
static int design(const fmd_fprint_config& c, int* K_out, int* first_out, const char* path, bool print) {
    const int K = fmd_fprint_bins(&c);
    if (K <= 0) return 1;
    const size_t F = (size_t)c.hop * (size_t)K, R = (size_t)c.n_sub, E = (size_t)c.n_bands + 1;
    std::unique_ptr<float[]> bc(new float[F]), bs(new float[F]), wc(new float[R]), ws(new float[R]);
    std::unique_ptr<int[]> edges(new int[E]);
    fmd_fprint_design_t d;
    if (fmd_fprint_design(&c, bc.get(), bs.get(), wc.get(), ws.get(), edges.get(), &d) != FMD_OK || d.n_bins != K) return 1;
    // each array alone, the others null
    std::unique_ptr<float[]> bc2(new float[F]), ws2(new float[R]);
    std::unique_ptr<int[]> e2(new int[E]);
    if (fmd_fprint_design(&c, bc2.get(), nullptr, nullptr, nullptr, nullptr, nullptr) != FMD_OK || std::memcmp(bc.get(), bc2.get(), 4 * F) != 0) return 1;
    if (fmd_fprint_design(&c, nullptr, nullptr, nullptr, ws2.get(), nullptr, nullptr) != FMD_OK || std::memcmp(ws.get(), ws2.get(), 4 * R) != 0) return 1;
    if (fmd_fprint_design(&c, nullptr, nullptr, nullptr, nullptr, e2.get(), nullptr) != FMD_OK || std::memcmp(edges.get(), e2.get(), 4 * E) != 0) return 1;
    if (fmd_fprint_design(&c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != FMD_OK) return 1;
    if (edges[0] - 1 != d.first_bin || edges[c.n_bands] - edges[0] + 2 != K) return 1;
    if (path) {
        FILE* f = std::fopen(path, "wb");
        if (!f) return 1;
        std::fwrite(bc.get(), 4, F, f); std::fwrite(bs.get(), 4, F, f); std::fwrite(wc.get(), 4, R, f); std::fwrite(ws.get(), 4, R, f);
        std::fclose(f);
    }
    if (print) {
        std::printf("%d %d", K, d.first_bin);
        for (size_t b = 0; b < E; b++) std::printf(" %d", edges[b]);
        std::printf("\n");
    }
    *K_out = K; *first_out = d.first_bin;
    return 0;
}

int main(int argc, char** argv) {
    CHECK(argc >= 2 && (argc - 2) % 6 == 0);
    const std::string dir = argv[1];
    int K = 0, first = 0;
    for (int i = 0; 2 + 6 * i < argc; i++) {
        char** a = argv + 2 + 6 * i;
        const fmd_fprint_config c = geometry(std::atoi(a[0]), std::atoi(a[1]), std::atoi(a[2]), std::atoi(a[3]), std::atof(a[4]), std::atof(a[5]));
        CHECK(design(c, &K, &first, (dir + "/fprint_" + std::to_string(i) + ".f32").c_str(), true) == 0);
    }
    // the smallest design: two bands of one bin each at N = 64 (K = 4); and the largest: N = 32768, 33 bands up to bin N / 2 - 1
    CHECK(design(geometry(8000, 16, 4, 2, 125.0, 375.0), &K, &first, nullptr, false) == 0 && K == 4 && first == 0);
    CHECK(design(geometry(48000, 1024, 32, 33, 20.0, 16383.0 * 48000.0 / 32768.0), &K, &first, nullptr, false) == 0 && first + K - 1 == 16383);
    // invalid ones write nothing: one-element arrays stay as they are
    {
        const fmd_fprint_config bad[] = {geometry(7999, 16, 4, 9, 250, 3500), geometry(48001, 16, 4, 9, 250, 3500), geometry(8000, 15, 4, 9, 250, 3500),
                                         geometry(8000, 24, 4, 9, 250, 3500), geometry(8000, 1040, 4, 9, 250, 3500), geometry(8000, 0, 4, 9, 250, 3500),
                                         geometry(8000, 16, 2, 9, 250, 3500), geometry(8000, 16, 5, 9, 250, 3500), geometry(8000, 16, 64, 9, 250, 3500),
                                         geometry(8000, 16, 4, 1, 250, 3500), geometry(8000, 16, 4, 34, 250, 3500), geometry(8000, 16, 4, 9, 0.0, 3500),
                                         geometry(8000, 16, 4, 9, 3500, 3500), geometry(8000, 16, 4, 9, 250, NAN), geometry(8000, 16, 4, 9, NAN, 3500),
                                         geometry(8000, 16, 4, 9, 250, 2000),      // an empty band: edges 2, 3, 3, ...
                                         geometry(8000, 16, 4, 9, 60, 3500),       // k_0 = 0
                                         geometry(8000, 16, 4, 9, 250, 4000)};     // k_B = N / 2 > N / 2 - 1
        for (const fmd_fprint_config& c : bad) {
            std::unique_ptr<float[]> one(new float[1]);
            std::unique_ptr<int[]> ione(new int[1]);
            one[0] = 42.0f; ione[0] = 42;
            fmd_fprint_design_t d = {-7, -7};
            CHECK(fmd_fprint_design(&c, one.get(), one.get(), one.get(), one.get(), ione.get(), &d) == FMD_ERR_ARG);
            CHECK(one[0] == 42.0f && ione[0] == 42 && d.n_bins == -7 && d.first_bin == -7);
            CHECK(fmd_fprint_bins(&c) == FMD_ERR_ARG && fmd_fprint_state_bytes(&c, 1) == FMD_ERR_ARG);
        }
        fmd_fprint_config c = geometry(8000, 16, 4, 9, 250, 3500);
        CHECK(fmd_fprint_bins(&c) == 28);
        c.n_channels = 0; CHECK(fmd_fprint_bins(&c) == FMD_ERR_ARG); c.n_channels = 1;
        c.max_input_frames = 0; CHECK(fmd_fprint_bins(&c) == FMD_ERR_ARG);
        c.max_input_frames = (1LL << 30) + 1; CHECK(fmd_fprint_bins(&c) == FMD_ERR_ARG);
        c.max_input_frames = 1LL << 30; CHECK(fmd_fprint_bins(&c) == 28);
        CHECK(fmd_fprint_design(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == FMD_ERR_ARG);
        CHECK(fmd_fprint_state_bytes(&c, 0) == FMD_ERR_ARG && fmd_fprint_state_bytes(&c, 1) > 3 * 2 * 32 * 4);
    }
    // the default configurations
    for (int fs : {8000, 16000, 22050, 32000, 44100, 48000}) {
        fmd_fprint_config c;
        CHECK(fmd_fprint_default_config(fs, &c) == FMD_OK && c.hop % 16 == 0 && std::fabs(c.hop - fs * 0.0115) <= 8.0 && c.n_sub == 32 && c.n_bands == 33);
        CHECK(design(c, &K, &first, nullptr, false) == 0);
        std::printf("default %d %d %d %d\n", fs, c.hop, K, first);
    }
    {
        fmd_fprint_config c;
        CHECK(fmd_fprint_default_config(7999, &c) == FMD_ERR_ARG && fmd_fprint_default_config(48001, &c) == FMD_ERR_ARG);
        CHECK(fmd_fprint_default_config(8000, nullptr) == FMD_ERR_ARG);
        CHECK(fmd_fprint_default_config(32000, &c) == FMD_OK && c.hop == 368);
        // the kept spectra: 31 * 2 * 640 * 4 bytes a station
        c.max_input_frames = 2048;
        const long long b1 = fmd_fprint_state_bytes(&c, 1), b4096 = fmd_fprint_state_bytes(&c, 4096);
        CHECK(b1 > 158720 && b4096 > 4096LL * 158720 && b4096 < 4096LL * 200000 + (4LL << 20));
    }
    CHECK(fmd_fprint_max_prints(16, 0) == 0 && fmd_fprint_max_prints(16, 1) == 1 && fmd_fprint_max_prints(16, 16) == 1 && fmd_fprint_max_prints(16, 17) == 2);
    CHECK(fmd_fprint_max_prints(1024, 1LL << 40) == (1LL << 30) && fmd_fprint_max_prints(368, 2048) == 6);
    CHECK(fmd_fprint_max_prints(15, 1) == FMD_ERR_ARG && fmd_fprint_max_prints(1025, 1) == FMD_ERR_ARG && fmd_fprint_max_prints(16, -1) == FMD_ERR_ARG);
    CHECK(fmd_fprint_max_prints(16, (1LL << 40) + 1) == FMD_ERR_ARG);
    std::printf("ok\n");
    return 0;
}
