// Host-side half of the fingerprint matcher's index (fmd_fpmatch.hip, k_fpmatch_probe): the index configuration's validation, the sizes
// the probe kernel shares with the host, and the index itself, built at load as a stable LSD radix sort of (masked word, position) pairs
// (include/fmdemod.h, "Fingerprint matcher", "index").  All integer.  Needs no GPU.
#pragma once
#include <cstdint>
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kFpmIndexThreads = 256;           // a workgroup of k_fpmatch_probe: four wavefronts, a lane a window word in a pass
constexpr int kFpmIndexChunk = 4096;            // candidates of a chunk at most: the LDS list k_fpmatch_probe counts from
constexpr int kFpmIndexTable = 8192;            // slots of the LDS set that drops repeated proposals (a power of two, 2 * kFpmIndexChunk)
constexpr int kFpmIndexMaxDirBits = 24;         // the directory has at most 2^24 + 1 entries
static_assert(kFpmIndexChunk >= 64 * 64 && kFpmIndexTable == 2 * kFpmIndexChunk, "a chunk holds 64 words' runs at K = 64");

// the sizes of a checked, valid pair of configurations
struct FpmIndexLayout {
    int dir_bits;              // the directory is over the keys' top dir_bits: min(n_bits, ceil(log2(max_catalogue_words)) - 4) in 1 ... 24
    int chunk_words;           // window words whose runs one chunk takes: min(kFpmIndexThreads, kFpmIndexChunk / K)
    long long dir_entries;     // 2^dir_bits + 1
    long long index_bytes;     // keys and positions (4 + 4 bytes a catalogue word) and the directory (4 bytes an entry)
    long long bytes;           // the indexed object's whole device memory
};

// FMD_OK for a valid index configuration; FMD_ERR_ARG and the reason in *err otherwise
int fpmatch_index_check(const fmd_fpmatch_index_config* idx, std::string* err);
// the sizes of a checked pair
FpmIndexLayout fpmatch_index_layout(const fmd_fpmatch_config* cfg, const fmd_fpmatch_index_config* idx);
// the index of words [D]: keys [D] = the masked words ascending, pos [D] their positions (equal keys in ascending position: the sort is
// stable), dir [2^dir_bits + 1]: dir[b] = the first i with keys[i] >> (32 - dir_bits) >= b, dir[2^dir_bits] = D.  D = 0 is valid.
void fpmatch_index_build(const uint32_t* words, long long D, unsigned mask, int dir_bits, uint32_t* keys, int32_t* pos, int32_t* dir);

}  // namespace fmd
