// The fingerprint matcher's host-only unit (fmd_fpmatch_design.cpp) as a stand-alone program, for tests/test_fpmatch_cpu.py: built from
// source under -fsanitize=address,undefined.  Every array has exactly the size the header states, on the heap, so that a read or a write
// past an end is seen.
//
//   fpmatch_design_main [n_channels n_bits block interval max_words max_tracks max_catalogue_words]...
//
// Per configuration it prints "mask tile query_block groups lds_bytes max_events max_queries state_bytes"; then it runs the smallest and
// the largest designs, invalid ones (which must write nothing), catalogues with exact-size starts arrays, the default configuration,
// fmd_fpmatch_max_events and fmd_fpmatch_max_errs, and prints "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "fmdemod.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static fmd_fpmatch_config config(int C, int bits, int W, int I, int max_words, int max_tracks, long long max_cat) {
    fmd_fpmatch_config c;
    std::memset(&c, 0, sizeof(c));
    c.n_channels = C; c.n_bits = bits; c.block = W; c.interval = I; c.max_errs = (35 * W * bits) / 100; c.hold = 3; c.max_words = max_words;
    c.max_tracks = max_tracks; c.max_catalogue_words = max_cat; c.device = -1;
    return c;
}

// an invalid configuration writes nothing into an exact-size design
static int refused(const fmd_fpmatch_config& c) {
    std::unique_ptr<fmd_fpmatch_design_t> d(new fmd_fpmatch_design_t);
    std::memset(d.get(), 0x5a, sizeof(*d));
    fmd_fpmatch_design_t before = *d;
    if (fmd_fpmatch_design(&c, d.get()) != FMD_ERR_ARG || std::memcmp(d.get(), &before, sizeof(before)) != 0) return 1;
    if (fmd_fpmatch_state_bytes(&c) != FMD_ERR_ARG) return 1;
    const long long st[2] = {0, 4096};
    return fmd_fpmatch_check_catalogue(&c, st, 1) == FMD_ERR_ARG ? 0 : 1;
}

// starts of n_tracks tracks of `len` words each, exactly n_tracks + 1 entries on the heap
static std::unique_ptr<long long[]> even(int n_tracks, long long len) {
    std::unique_ptr<long long[]> s(new long long[(size_t)n_tracks + 1]);
    for (int t = 0; t <= n_tracks; t++) s[(size_t)t] = (long long)t * len;
    return s;
}

int main(int argc, char** argv) {
    for (int a = 1; a + 6 < argc; a += 7) {
        const fmd_fpmatch_config c = config(atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]), atoi(argv[a + 4]), atoi(argv[a + 5]), atoll(argv[a + 6]));
        std::unique_ptr<fmd_fpmatch_design_t> d(new fmd_fpmatch_design_t);
        CHECK(fmd_fpmatch_design(&c, d.get()) == FMD_OK && fmd_fpmatch_design(&c, nullptr) == FMD_OK);
        std::printf("%u %d %d %d %d %lld %lld %lld\n", d->mask, d->tile, d->query_block, d->groups, d->lds_bytes, d->max_events, d->max_queries, fmd_fpmatch_state_bytes(&c));
    }
    // the smallest and the largest designs
    {
        fmd_fpmatch_design_t d;
        fmd_fpmatch_config c = config(1, 1, 16, 1, 1, 1, 16);
        CHECK(fmd_fpmatch_design(&c, &d) == FMD_OK && d.mask == 0x80000000u && d.groups == 1 && d.max_events == 1 && d.max_queries == 1 && d.lds_bytes == 4 * (d.tile + 15));
        CHECK(fmd_fpmatch_state_bytes(&c) > 0);
        c = config(256, 32, 1024, 1, 65536, 1 << 20, 1LL << 28);
        CHECK(fmd_fpmatch_design(&c, &d) == FMD_OK && d.mask == 0xffffffffu && d.groups == 256 && d.max_events == 65536 && d.max_queries == (1LL << 24));
        CHECK(fmd_fpmatch_state_bytes(&c) > (1LL << 36));
        // the catalogue's bounds at exact-size arrays
        c = config(3, 32, 16, 4, 64, 4, 100);
        auto s = even(4, 25);
        CHECK(fmd_fpmatch_check_catalogue(&c, s.get(), 4) == FMD_OK);
        CHECK(fmd_fpmatch_check_catalogue(&c, s.get(), 3) == FMD_OK && fmd_fpmatch_check_catalogue(&c, s.get(), 0) == FMD_OK);
        CHECK(fmd_fpmatch_check_catalogue(&c, nullptr, 0) == FMD_OK && fmd_fpmatch_check_catalogue(&c, nullptr, 1) == FMD_ERR_ARG);
        auto five = even(5, 20);
        CHECK(fmd_fpmatch_check_catalogue(&c, five.get(), 5) == FMD_ERR_ARG);                    // above max_tracks (nothing behind [0] need be read)
        auto longer = even(4, 26);
        CHECK(fmd_fpmatch_check_catalogue(&c, longer.get(), 4) == FMD_ERR_ARG && fmd_fpmatch_check_catalogue(&c, longer.get(), 3) == FMD_OK);   // 104 > 100 words
        auto shorter = even(4, 15);
        CHECK(fmd_fpmatch_check_catalogue(&c, shorter.get(), 1) == FMD_ERR_ARG);                 // a track of 15 < 16 words
        s[2] = 40;                                                                               // 0 25 40 75 100: track 1 has 15 words
        CHECK(fmd_fpmatch_check_catalogue(&c, s.get(), 4) == FMD_ERR_ARG);
        s[2] = 20;                                                                               // does not ascend
        CHECK(fmd_fpmatch_check_catalogue(&c, s.get(), 4) == FMD_ERR_ARG);
        s[2] = 50; s[0] = 1;
        CHECK(fmd_fpmatch_check_catalogue(&c, s.get(), 4) == FMD_ERR_ARG && fmd_fpmatch_check_catalogue(&c, s.get(), 0) == FMD_ERR_ARG);
        s[0] = 0; s[4] = 0x7fffffffffffffffLL;                                                   // no overflow on the way to the refusal
        CHECK(fmd_fpmatch_check_catalogue(&c, s.get(), 4) == FMD_ERR_ARG);
        s[1] = -0x7fffffffffffffffLL;
        CHECK(fmd_fpmatch_check_catalogue(&c, s.get(), 4) == FMD_ERR_ARG);
    }
    // invalid configurations write nothing
    {
        const fmd_fpmatch_config good = config(3, 32, 16, 4, 64, 4, 100);
        fmd_fpmatch_config c;
        c = good; c.n_channels = 0; CHECK(refused(c) == 0);
        c = good; c.n_bits = 0; CHECK(refused(c) == 0);
        c = good; c.n_bits = 33; CHECK(refused(c) == 0);
        c = good; c.block = 24; CHECK(refused(c) == 0);
        c = good; c.block = 0; CHECK(refused(c) == 0);
        c = good; c.block = 1040; c.max_catalogue_words = 4096; CHECK(refused(c) == 0);
        c = good; c.interval = 0; CHECK(refused(c) == 0);
        c = good; c.interval = 1025; CHECK(refused(c) == 0);
        c = good; c.max_errs = -1; CHECK(refused(c) == 0);
        c = good; c.max_errs = 16 * 32 + 1; CHECK(refused(c) == 0);
        c = good; c.hold = 0; CHECK(refused(c) == 0);
        c = good; c.max_words = 0; CHECK(refused(c) == 0);
        c = good; c.max_words = 65537; CHECK(refused(c) == 0);
        c = good; c.max_tracks = 0; CHECK(refused(c) == 0);
        c = good; c.max_tracks = (1 << 20) + 1; CHECK(refused(c) == 0);
        c = good; c.max_catalogue_words = 15; CHECK(refused(c) == 0);
        c = good; c.max_catalogue_words = (1LL << 28) + 1; CHECK(refused(c) == 0);
        c = good; c.n_channels = 257; c.interval = 1; c.max_words = 65536; CHECK(refused(c) == 0);   // above 2^24 queries a call
        CHECK(fmd_fpmatch_design(nullptr, nullptr) == FMD_ERR_ARG && fmd_fpmatch_state_bytes(nullptr) == FMD_ERR_ARG);
    }
    fmd_fpmatch_config d;
    CHECK(fmd_fpmatch_default_config(&d) == FMD_OK && fmd_fpmatch_default_config(nullptr) == FMD_ERR_ARG);
    CHECK(d.n_channels == 1 && d.n_bits == 32 && d.block == 256 && d.interval == 64 && d.max_errs == 2867 && d.hold == 3 && d.device == -1);
    CHECK(fmd_fpmatch_design(&d, nullptr) == FMD_OK && fmd_fpmatch_state_bytes(&d) > 4 * d.max_catalogue_words);
    std::printf("default %d %d %d %d %d %d %d %d %lld\n", d.n_channels, d.n_bits, d.block, d.interval, d.max_errs, d.hold, d.max_words, d.max_tracks, d.max_catalogue_words);
    CHECK(fmd_fpmatch_max_events(64, 0) == 0 && fmd_fpmatch_max_events(64, 1) == 1 && fmd_fpmatch_max_events(64, 64) == 1 && fmd_fpmatch_max_events(64, 65) == 2);
    CHECK(fmd_fpmatch_max_events(1, 65536) == 65536 && fmd_fpmatch_max_events(1024, 65536) == 64);
    CHECK(fmd_fpmatch_max_events(0, 1) == FMD_ERR_ARG && fmd_fpmatch_max_events(1025, 1) == FMD_ERR_ARG && fmd_fpmatch_max_events(4, -1) == FMD_ERR_ARG &&
          fmd_fpmatch_max_events(4, 65537) == FMD_ERR_ARG);
    CHECK(fmd_fpmatch_max_errs(35, 256, 32) == 2867 && fmd_fpmatch_max_errs(0, 16, 1) == 0 && fmd_fpmatch_max_errs(100, 1024, 32) == 32768 && fmd_fpmatch_max_errs(35, 16, 9) == 50);
    CHECK(fmd_fpmatch_max_errs(-1, 16, 1) == FMD_ERR_ARG && fmd_fpmatch_max_errs(101, 16, 1) == FMD_ERR_ARG && fmd_fpmatch_max_errs(35, 24, 1) == FMD_ERR_ARG &&
          fmd_fpmatch_max_errs(35, 16, 0) == FMD_ERR_ARG && fmd_fpmatch_max_errs(35, 16, 33) == FMD_ERR_ARG);
    std::printf("ok\n");
    return 0;
}
