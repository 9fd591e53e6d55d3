// The fingerprint matcher's host-only unit: every value is an integer, so there is nothing here a compiler flag could change.
#include "fmd_fpmatch_design.h"

#include <cstdio>

namespace fmd {

std::string& fpmatch_global_error() {
    thread_local std::string e;
    return e;
}

static bool block_ok(int W) { return W >= 16 && W <= 1024 && W % 16 == 0; }

int fpmatch_check(const fmd_fpmatch_config* c, std::string* err) {
    if (!c) { *err = "null configuration"; return FMD_ERR_ARG; }
    if (c->n_channels <= 0) { *err = "n_channels is not positive"; return FMD_ERR_ARG; }
    if (c->n_bits < 1 || c->n_bits > 32) { *err = "n_bits outside 1 ... 32"; return FMD_ERR_ARG; }
    if (!block_ok(c->block)) { *err = "block is not a multiple of 16 in 16 ... 1024"; return FMD_ERR_ARG; }
    if (c->interval < 1 || c->interval > 1024) { *err = "interval outside 1 ... 1024"; return FMD_ERR_ARG; }
    if (c->max_errs < 0 || c->max_errs > c->block * c->n_bits) { *err = "max_errs outside 0 ... block * n_bits"; return FMD_ERR_ARG; }
    if (c->hold < 1) { *err = "hold below 1"; return FMD_ERR_ARG; }
    if (c->max_words <= 0 || c->max_words > 65536) { *err = "max_words outside (0, 65536]"; return FMD_ERR_ARG; }
    if (c->max_tracks < 1 || c->max_tracks > (1 << 20)) { *err = "max_tracks outside [1, 2^20]"; return FMD_ERR_ARG; }
    if (c->max_catalogue_words < c->block || c->max_catalogue_words > (1LL << 28)) { *err = "max_catalogue_words outside [block, 2^28]"; return FMD_ERR_ARG; }
    const long long ev = ((long long)c->max_words + c->interval - 1) / c->interval;
    if ((long long)c->n_channels * ev > kFpmatchMaxQueries) { *err = "n_channels * max_events above 2^24 queries a call"; return FMD_ERR_ARG; }
    return FMD_OK;
}

long long fpmatch_tiles(long long D, int W) { return D < W ? 0 : (D - W + 1 + kFpmatchTile - 1) / kFpmatchTile; }

FpmatchLayout fpmatch_layout(const fmd_fpmatch_config* c) {
    FpmatchLayout l{};
    const long long C = c->n_channels, W = c->block;
    l.mask = 0xffffffffu << (32 - c->n_bits);
    l.max_events = ((long long)c->max_words + c->interval - 1) / c->interval;
    l.max_queries = C * l.max_events;
    const long long tiles = fpmatch_tiles(c->max_catalogue_words, c->block);
    l.groups = (int)(tiles < kFpmatchMaxGroups ? tiles : kFpmatchMaxGroups);
    l.lds_words = kFpmatchTile + c->block - 1;
    l.bytes = C * (64 + 4 * W) + 4 * c->max_catalogue_words + 4 * ((long long)c->max_tracks + 1) + 4 * (C + 1) + l.max_queries * W * 4 +
              l.max_queries * l.groups * 8;
    return l;
}

int fpmatch_check_catalogue(const fmd_fpmatch_config* c, const long long* starts, int n_tracks, std::string* err) {
    if (n_tracks < 0 || n_tracks > c->max_tracks) { *err = "n_tracks outside [0, max_tracks]"; return FMD_ERR_ARG; }
    if (n_tracks == 0) {
        if (starts && starts[0] != 0) { *err = "starts[0] is not 0"; return FMD_ERR_ARG; }
        return FMD_OK;
    }
    if (!starts) { *err = "null starts"; return FMD_ERR_ARG; }
    if (starts[0] != 0) { *err = "starts[0] is not 0"; return FMD_ERR_ARG; }
    for (int t = 0; t < n_tracks; t++) {
        // (in this order nothing overflows: starts[t] <= max_catalogue_words holds before starts[t + 1] is compared with it)
        if (starts[t + 1] < starts[t] || starts[t + 1] - starts[t] < c->block) {
            char buf[96];
            snprintf(buf, sizeof(buf), "track %d is shorter than block, or starts does not ascend", t);
            *err = buf;
            return FMD_ERR_ARG;
        }
        if (starts[t + 1] > c->max_catalogue_words) { *err = "the catalogue is longer than max_catalogue_words"; return FMD_ERR_ARG; }
    }
    return FMD_OK;
}

}  // namespace fmd

static int fpm_fail(int code, const std::string& msg) {
    fmd::fpmatch_global_error() = msg;
    return code;
}

extern "C" {

int fmd_fpmatch_default_config(fmd_fpmatch_config* cfg) {
    if (!cfg) return fpm_fail(FMD_ERR_ARG, "null configuration");
    cfg->n_channels = 1;
    cfg->n_bits = 32;
    cfg->block = 256;
    cfg->interval = 64;
    cfg->max_errs = (35 * 256 * 32) / 100;
    cfg->hold = 3;
    cfg->max_words = 64;
    cfg->max_tracks = 4096;
    cfg->max_catalogue_words = 1LL << 22;
    cfg->device = -1;
    return FMD_OK;
}

long long fmd_fpmatch_max_events(int interval, long long n) {
    if (interval < 1 || interval > 1024 || n < 0 || n > 65536) return fpm_fail(FMD_ERR_ARG, "interval outside 1 ... 1024 or n outside [0, 65536]");
    return (n + (long long)interval - 1) / (long long)interval;
}

long long fmd_fpmatch_max_errs(int ber_percent, int block, int n_bits) {
    if (ber_percent < 0 || ber_percent > 100 || !fmd::block_ok(block) || n_bits < 1 || n_bits > 32)
        return fpm_fail(FMD_ERR_ARG, "ber_percent outside 0 ... 100, block no multiple of 16 in 16 ... 1024 or n_bits outside 1 ... 32");
    return ((long long)ber_percent * block * n_bits) / 100;
}

int fmd_fpmatch_design(const fmd_fpmatch_config* cfg, fmd_fpmatch_design_t* out) {
    std::string err;
    if (fmd::fpmatch_check(cfg, &err) != FMD_OK) return fpm_fail(FMD_ERR_ARG, err);
    if (out) {
        const fmd::FpmatchLayout l = fmd::fpmatch_layout(cfg);
        out->mask = l.mask;
        out->tile = fmd::kFpmatchTile;
        out->query_block = fmd::kFpmatchQueries;
        out->groups = l.groups;
        out->lds_bytes = 4 * l.lds_words;
        out->max_events = l.max_events;
        out->max_queries = l.max_queries;
    }
    return FMD_OK;
}

int fmd_fpmatch_check_catalogue(const fmd_fpmatch_config* cfg, const long long* starts, int n_tracks) {
    std::string err;
    if (fmd::fpmatch_check(cfg, &err) != FMD_OK || fmd::fpmatch_check_catalogue(cfg, starts, n_tracks, &err) != FMD_OK) return fpm_fail(FMD_ERR_ARG, err);
    return FMD_OK;
}

long long fmd_fpmatch_state_bytes(const fmd_fpmatch_config* cfg) {
    std::string err;
    if (fmd::fpmatch_check(cfg, &err) != FMD_OK) return fpm_fail(FMD_ERR_ARG, err);
    return fmd::fpmatch_layout(cfg).bytes;
}

}  // extern "C"
