// The fingerprint matcher's index, host-only: every value is an integer, so there is nothing here a compiler flag could change.
#include "fmd_fpmatch_index.h"

#include <cstring>
#include <vector>

#include "fmd_fpmatch_design.h"

namespace fmd {

int fpmatch_index_check(const fmd_fpmatch_index_config* x, std::string* err) {
    if (!x) { *err = "null index configuration"; return FMD_ERR_ARG; }
    if (x->max_bucket < 1 || x->max_bucket > 64) { *err = "max_bucket outside 1 ... 64"; return FMD_ERR_ARG; }
    if (x->follow < 0 || x->follow > 8) { *err = "follow outside 0 ... 8"; return FMD_ERR_ARG; }
    return FMD_OK;
}

FpmIndexLayout fpmatch_index_layout(const fmd_fpmatch_config* c, const fmd_fpmatch_index_config* x) {
    FpmIndexLayout l{};
    int lg = 0;                                                              // ceil(log2(max_catalogue_words))
    while ((1LL << lg) < c->max_catalogue_words) lg++;
    int b = lg - 4;                                                          // about 16 keys a directory slice at capacity
    b = b < 1 ? 1 : (b > kFpmIndexMaxDirBits ? kFpmIndexMaxDirBits : b);
    l.dir_bits = b < c->n_bits ? b : c->n_bits;
    l.chunk_words = kFpmIndexChunk / x->max_bucket < kFpmIndexThreads ? kFpmIndexChunk / x->max_bucket : kFpmIndexThreads;
    l.dir_entries = (1LL << l.dir_bits) + 1;
    l.index_bytes = 8 * c->max_catalogue_words + 4 * l.dir_entries;
    const FpmatchLayout f = fpmatch_layout(c);
    const long long C = c->n_channels, W = c->block;
    // records and rings, catalogue, starts, row map, windows, one partial and one (candidates, skipped) pair a query, the index records, the index
    l.bytes = C * (64 + 4 * W) + 4 * c->max_catalogue_words + 4 * ((long long)c->max_tracks + 1) + 4 * (C + 1) + f.max_queries * W * 4 + f.max_queries * 8 +
              f.max_queries * 8 + C * 32 + l.index_bytes;
    return l;
}

void fpmatch_index_build(const uint32_t* words, long long D, unsigned mask, int dir_bits, uint32_t* keys, int32_t* pos, int32_t* dir) {
    const size_t n = (size_t)D;
    for (size_t i = 0; i < n; i++) { keys[i] = words[i] & mask; pos[i] = (int32_t)i; }
    // LSD radix sort, a byte a pass, stable; a byte the mask clears is the same in every key and needs no pass
    std::vector<uint32_t> tk(n);
    std::vector<int32_t> tp(n);
    uint32_t *ka = keys, *kb = tk.data();
    int32_t *pa = pos, *pb = tp.data();
    for (int shift = 0; shift < 32 && n > 0; shift += 8) {
        if (((mask >> shift) & 0xffu) == 0u) continue;
        size_t count[257] = {0};
        for (size_t i = 0; i < n; i++) count[((ka[i] >> shift) & 0xffu) + 1]++;
        for (int d = 0; d < 256; d++) count[d + 1] += count[d];
        for (size_t i = 0; i < n; i++) {
            const size_t at = count[(ka[i] >> shift) & 0xffu]++;
            kb[at] = ka[i];
            pb[at] = pa[i];
        }
        uint32_t* k = ka; ka = kb; kb = k;
        int32_t* p = pa; pa = pb; pb = p;
    }
    if (ka != keys && n > 0) {
        memcpy(keys, ka, sizeof(uint32_t) * n);
        memcpy(pos, pa, sizeof(int32_t) * n);
    }
    const long long slices = 1LL << dir_bits;
    size_t i = 0;
    for (long long b = 0; b <= slices; b++) {
        while (i < n && (long long)(keys[i] >> (32 - dir_bits)) < b) i++;
        dir[b] = (int32_t)i;
    }
}

}  // namespace fmd

static int fpm_fail(int code, const std::string& msg) {
    fmd::fpmatch_global_error() = msg;
    return code;
}

// FMD_OK for a valid pair of configurations, the reason in the global error otherwise
static int check_pair(const fmd_fpmatch_config* cfg, const fmd_fpmatch_index_config* idx) {
    std::string err;
    if (fmd::fpmatch_check(cfg, &err) != FMD_OK || fmd::fpmatch_index_check(idx, &err) != FMD_OK) return fpm_fail(FMD_ERR_ARG, err);
    return FMD_OK;
}

extern "C" {

int fmd_fpmatch_index_default_config(fmd_fpmatch_index_config* idx) {
    if (!idx) return fpm_fail(FMD_ERR_ARG, "null index configuration");
    idx->max_bucket = 8;
    idx->follow = 2;
    return FMD_OK;
}

int fmd_fpmatch_index_design(const fmd_fpmatch_config* cfg, const fmd_fpmatch_index_config* idx, fmd_fpmatch_index_design_t* out) {
    if (check_pair(cfg, idx) != FMD_OK) return FMD_ERR_ARG;
    if (out) {
        const fmd::FpmIndexLayout l = fmd::fpmatch_index_layout(cfg, idx);
        out->dir_bits = l.dir_bits;
        out->chunk = fmd::kFpmIndexChunk;
        out->chunk_words = l.chunk_words;
        out->table = fmd::kFpmIndexTable;
        out->dir_entries = l.dir_entries;
        out->index_bytes = l.index_bytes;
    }
    return FMD_OK;
}

long long fmd_fpmatch_index_state_bytes(const fmd_fpmatch_config* cfg, const fmd_fpmatch_index_config* idx) {
    if (check_pair(cfg, idx) != FMD_OK) return FMD_ERR_ARG;
    return fmd::fpmatch_index_layout(cfg, idx).bytes;
}

int fmd_fpmatch_index_build(const fmd_fpmatch_config* cfg, const fmd_fpmatch_index_config* idx, const uint32_t* words, long long n_words, uint32_t* keys, int* pos,
                            int* dir) {
    if (check_pair(cfg, idx) != FMD_OK) return FMD_ERR_ARG;
    if (n_words < 0 || n_words > cfg->max_catalogue_words) return fpm_fail(FMD_ERR_ARG, "n_words outside [0, max_catalogue_words]");
    if (!dir || (n_words > 0 && (!words || !keys || !pos))) return fpm_fail(FMD_ERR_ARG, "null words, keys, pos or dir");
    fmd::fpmatch_index_build(words, n_words, fmd::fpmatch_layout(cfg).mask, fmd::fpmatch_index_layout(cfg, idx).dir_bits, keys, pos, dir);
    return FMD_OK;
}

}  // extern "C"
