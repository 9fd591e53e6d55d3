// Host-side half of the fingerprint matcher (fmd_fpmatch.hip): the configuration's and the catalogue's validation, and the sizes, the LDS
// image and the scratch the kernels share with the host (include/fmdemod.h, "Fingerprint matcher").  All integer.  Needs no GPU.
#pragma once
#include <string>

#include "fmdemod.h"

namespace fmd {

constexpr int kFpmatchThreads = 256;            // a workgroup of k_fpmatch_search: four wavefronts
constexpr int kFpmatchTile = 1024;              // catalogue positions of a column tile: four passes of a workgroup's 256 lanes
constexpr int kFpmatchQueries = 8;              // queries a lane accumulates at once (the register block; a workgroup's row tile)
constexpr int kFpmatchMaxGroups = 256;          // column groups at most: the partial minima a query has in the scratch
constexpr long long kFpmatchMaxQueries = 1LL << 24;   // n_channels * max_events at most

// the sizes of a checked, valid configuration
struct FpmatchLayout {
    unsigned mask;
    long long max_events;      // a station's events of a call of max_words
    long long max_queries;     // C * max_events: rows of the query windows and of the scratch
    int groups;                // min(column tiles of max_catalogue_words, kFpmatchMaxGroups)
    int lds_words;             // kFpmatchTile + W - 1
    long long bytes;           // the object's device memory
};

// the message of the last failing call that has no handle (fmd_fpmatch_create and the host-only functions)
std::string& fpmatch_global_error();
// FMD_OK for a valid configuration; FMD_ERR_ARG and the reason in *err otherwise
int fpmatch_check(const fmd_fpmatch_config* cfg, std::string* err);
// the sizes of a checked configuration
FpmatchLayout fpmatch_layout(const fmd_fpmatch_config* cfg);
// column tiles of a catalogue of D >= W words: ceil((D - W + 1) / kFpmatchTile); 0 for D = 0
long long fpmatch_tiles(long long D, int W);
// FMD_OK where starts [n_tracks + 1] is a catalogue cfg takes; FMD_ERR_ARG and the reason otherwise
int fpmatch_check_catalogue(const fmd_fpmatch_config* cfg, const long long* starts, int n_tracks, std::string* err);

}  // namespace fmd
