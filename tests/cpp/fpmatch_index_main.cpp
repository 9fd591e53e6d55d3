// The fingerprint matcher's index unit (fmd_fpmatch_index.cpp, with fmd_fpmatch_design.cpp) as a stand-alone program, for
// tests/test_fpmatch_index_cpu.py: built from source under -fsanitize=address,undefined.  Every array has exactly the size the header
// states, on the heap, so that a read or a write past an end is seen.
//
//   fpmatch_index_main [n_bits block max_catalogue_words max_bucket n_words seed]...
//
// Per set it builds the index of n_words seeded words (an LCG, so that the test can make the same words) and prints
// "dir_bits chunk chunk_words table dir_entries index_bytes state_bytes fnv(keys) fnv(pos) fnv(dir)"; then it runs D = W, D = 0, the
// largest dir_bits, invalid configurations and arguments (which must write nothing), the default configuration, and prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "fmdemod.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static fmd_fpmatch_config config(int bits, int W, long long max_cat) {
    fmd_fpmatch_config c;
    std::memset(&c, 0, sizeof(c));
    c.n_channels = 2; c.n_bits = bits; c.block = W; c.interval = 4; c.max_errs = (35 * W * bits) / 100; c.hold = 3; c.max_words = 64;
    c.max_tracks = 4; c.max_catalogue_words = max_cat; c.device = -1;
    return c;
}

static unsigned long long fnv(const void* p, size_t bytes) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; i++) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
    return h;
}

// n words of the LCG x <- x * 1664525 + 1013904223 from `seed`, each word the state after its step; exactly n entries on the heap
static std::unique_ptr<uint32_t[]> lcg(size_t n, uint32_t seed) {
    std::unique_ptr<uint32_t[]> w(new uint32_t[n ? n : 1]);
    uint32_t x = seed;
    for (size_t i = 0; i < n; i++) { x = x * 1664525u + 1013904223u; w[i] = x; }
    return w;
}

// builds into exact-size arrays and checks the index's own invariants: keys ascend, equal keys in ascending position, keys[i] is the
// masked word at pos[i], pos is a permutation, dir[b] is the first key of slice b
static int build_checked(const fmd_fpmatch_config& c, const fmd_fpmatch_index_config& x, const uint32_t* words, long long D, bool print) {
    fmd_fpmatch_index_design_t d;
    fmd_fpmatch_design_t fd;
    CHECK(fmd_fpmatch_index_design(&c, &x, &d) == FMD_OK && fmd_fpmatch_design(&c, &fd) == FMD_OK);
    const size_t n = (size_t)D, ne = (size_t)d.dir_entries;
    std::unique_ptr<uint32_t[]> keys(n ? new uint32_t[n] : nullptr);
    std::unique_ptr<int[]> pos(n ? new int[n] : nullptr), dir(new int[ne]);
    std::unique_ptr<unsigned char[]> seen(new unsigned char[n ? n : 1]());
    CHECK(fmd_fpmatch_index_build(&c, &x, words, D, keys.get(), pos.get(), dir.get()) == FMD_OK);
    for (size_t i = 0; i < n; i++) {
        CHECK(pos[i] >= 0 && (size_t)pos[i] < n && !seen[(size_t)pos[i]]);
        seen[(size_t)pos[i]] = 1;
        CHECK(keys[i] == (words[(size_t)pos[i]] & fd.mask));
        CHECK(i == 0 || keys[i - 1] < keys[i] || (keys[i - 1] == keys[i] && pos[i - 1] < pos[i]));
    }
    CHECK(dir[0] == 0 && (long long)dir[ne - 1] == D);
    for (size_t b = 0; b + 1 < ne; b++) {
        CHECK(dir[b] <= dir[b + 1]);
        for (int i = dir[b]; i < dir[b + 1]; i++) CHECK((size_t)(keys[(size_t)i] >> (32 - d.dir_bits)) == b);
    }
    if (print)
        std::printf("%d %d %d %d %lld %lld %lld %llu %llu %llu\n", d.dir_bits, d.chunk, d.chunk_words, d.table, d.dir_entries, d.index_bytes,
                    fmd_fpmatch_index_state_bytes(&c, &x), fnv(keys.get(), 4 * n), fnv(pos.get(), 4 * n), fnv(dir.get(), 4 * ne));
    return 0;
}

// an invalid pair writes nothing into an exact-size design or into exact-size index arrays
static int refused(const fmd_fpmatch_config& c, const fmd_fpmatch_index_config& x) {
    std::unique_ptr<fmd_fpmatch_index_design_t> d(new fmd_fpmatch_index_design_t);
    std::memset(d.get(), 0x5a, sizeof(*d));
    const fmd_fpmatch_index_design_t before = *d;
    if (fmd_fpmatch_index_design(&c, &x, d.get()) != FMD_ERR_ARG || std::memcmp(d.get(), &before, sizeof(before)) != 0) return 1;
    if (fmd_fpmatch_index_state_bytes(&c, &x) != FMD_ERR_ARG) return 1;
    std::unique_ptr<uint32_t[]> w(new uint32_t[1]), k(new uint32_t[1]);
    std::unique_ptr<int[]> p(new int[1]), dir(new int[1]);
    w[0] = 7u; k[0] = 0x5a5a5a5au; p[0] = 0x5a5a5a5a; dir[0] = 0x5a5a5a5a;
    if (fmd_fpmatch_index_build(&c, &x, w.get(), 1, k.get(), p.get(), dir.get()) != FMD_ERR_ARG) return 1;
    return k[0] == 0x5a5a5a5au && p[0] == 0x5a5a5a5a && dir[0] == 0x5a5a5a5a ? 0 : 1;
}

int main(int argc, char** argv) {
    for (int a = 1; a + 5 < argc; a += 6) {
        const fmd_fpmatch_config c = config(atoi(argv[a]), atoi(argv[a + 1]), atoll(argv[a + 2]));
        const fmd_fpmatch_index_config x = {atoi(argv[a + 3]), 2};
        const long long D = atoll(argv[a + 4]);
        auto w = lcg((size_t)D, (uint32_t)strtoul(argv[a + 5], nullptr, 10));
        CHECK(build_checked(c, x, w.get(), D, true) == 0);
    }
    fmd_fpmatch_index_config x;
    CHECK(fmd_fpmatch_index_default_config(&x) == FMD_OK && fmd_fpmatch_index_default_config(nullptr) == FMD_ERR_ARG && x.max_bucket == 8 && x.follow == 2);
    {
        // D = W, the smallest catalogue an object takes, and D = 0 (keys, pos and words may be NULL)
        fmd_fpmatch_config c = config(32, 16, 16);
        auto w = lcg(16, 5u);
        CHECK(build_checked(c, x, w.get(), 16, false) == 0);
        CHECK(build_checked(c, x, nullptr, 0, false) == 0);
        fmd_fpmatch_index_design_t d;
        CHECK(fmd_fpmatch_index_design(&c, &x, &d) == FMD_OK && d.dir_bits == 1 && d.dir_entries == 3 && d.index_bytes == 8 * 16 + 12 && d.chunk_words == 256);
        // every word the same, 0 and 0xffffffff: one run, in ascending position
        std::unique_ptr<uint32_t[]> same(new uint32_t[16]);
        for (int i = 0; i < 16; i++) same[i] = 0xffffffffu;
        CHECK(build_checked(c, x, same.get(), 16, false) == 0);
        for (int i = 0; i < 16; i++) same[i] = 0u;
        CHECK(build_checked(c, x, same.get(), 16, false) == 0);
        // the largest dir_bits: 2^24 + 1 entries, at 32 and at 24 bits; fewer bits than that cap it
        c = config(32, 16, 1LL << 28);
        auto w2 = lcg(1000, 9u);
        CHECK(fmd_fpmatch_index_design(&c, &x, &d) == FMD_OK && d.dir_bits == 24 && d.dir_entries == (1LL << 24) + 1 && d.index_bytes == (8LL << 28) + 4 * d.dir_entries);
        CHECK(build_checked(c, x, w2.get(), 1000, false) == 0);
        c = config(9, 16, 1LL << 28);
        CHECK(fmd_fpmatch_index_design(&c, &x, &d) == FMD_OK && d.dir_bits == 9);
        CHECK(build_checked(c, x, w2.get(), 1000, false) == 0);
        x.max_bucket = 64;
        CHECK(fmd_fpmatch_index_design(&c, &x, &d) == FMD_OK && d.chunk_words == 64 && d.chunk_words * 64 <= d.chunk && 2 * d.chunk == d.table);
        x.max_bucket = 8;
    }
    {
        // invalid pairs and arguments write nothing
        const fmd_fpmatch_config good = config(32, 16, 100);
        fmd_fpmatch_config c = good;
        fmd_fpmatch_index_config b = x;
        b.max_bucket = 0; CHECK(refused(good, b) == 0);
        b.max_bucket = 65; CHECK(refused(good, b) == 0);
        b = x; b.follow = -1; CHECK(refused(good, b) == 0);
        b.follow = 9; CHECK(refused(good, b) == 0);
        c.block = 24; CHECK(refused(c, x) == 0);
        c = good; c.n_bits = 0; CHECK(refused(c, x) == 0);
        CHECK(fmd_fpmatch_index_design(&good, nullptr, nullptr) == FMD_ERR_ARG && fmd_fpmatch_index_design(nullptr, &x, nullptr) == FMD_ERR_ARG);
        CHECK(fmd_fpmatch_index_state_bytes(&good, nullptr) == FMD_ERR_ARG && fmd_fpmatch_index_state_bytes(nullptr, &x) == FMD_ERR_ARG);
        CHECK(fmd_fpmatch_index_design(&good, &x, nullptr) == FMD_OK && fmd_fpmatch_index_state_bytes(&good, &x) > 0);
        std::unique_ptr<uint32_t[]> w(new uint32_t[1]), k(new uint32_t[1]);
        std::unique_ptr<int[]> p(new int[1]), dir(new int[1]);
        w[0] = 1u; k[0] = 0x5a5a5a5au; p[0] = 0x5a5a5a5a; dir[0] = 0x5a5a5a5a;
        CHECK(fmd_fpmatch_index_build(&good, &x, w.get(), 101, k.get(), p.get(), dir.get()) == FMD_ERR_ARG);    // above max_catalogue_words
        CHECK(fmd_fpmatch_index_build(&good, &x, w.get(), -1, k.get(), p.get(), dir.get()) == FMD_ERR_ARG);
        CHECK(fmd_fpmatch_index_build(&good, &x, nullptr, 1, k.get(), p.get(), dir.get()) == FMD_ERR_ARG);
        CHECK(fmd_fpmatch_index_build(&good, &x, w.get(), 1, nullptr, p.get(), dir.get()) == FMD_ERR_ARG);
        CHECK(fmd_fpmatch_index_build(&good, &x, w.get(), 1, k.get(), nullptr, dir.get()) == FMD_ERR_ARG);
        CHECK(fmd_fpmatch_index_build(&good, &x, w.get(), 1, k.get(), p.get(), nullptr) == FMD_ERR_ARG);
        CHECK(k[0] == 0x5a5a5a5au && p[0] == 0x5a5a5a5a && dir[0] == 0x5a5a5a5a);
    }
    std::printf("ok\n");
    return 0;
}
