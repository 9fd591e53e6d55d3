// fm-radio_amd/csrc/fmd_tables.cpp (the tolerance mode's table designers) with fmd_design.cpp, on their own (no HIP, no library): built
// with -fsanitize=address,undefined by `make -C oracle asan`.  Writes every table the library uploads as raw bytes to the file given —
// for fs = 256000, 1024000, 2048000 with both audio cut-offs at 15000, 12000, 9000 Hz (the other controls at their defaults), in the order
// main() makes them, case after case — and prints one line per (case, table): fs, table, offset and length in the file.
// tests/test_sanitizers_cpu.py hashes each piece against tests/golden/design_tables.json.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fmd_design.h"
#include "fmd_tables.h"

using namespace fmd;

static std::FILE* g_out;
static long g_off;

static bool put(int fs, const char* table, const void* p, size_t bytes) {
    if (std::fwrite(p, 1, bytes, g_out) != bytes) return false;
    std::printf("%d %s %ld %zu\n", fs, table, g_off, bytes);
    g_off += (long)bytes;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: tables_main out.bin\n"); return 2; }
    g_out = std::fopen(argv[1], "wb");
    if (!g_out) { std::perror(argv[1]); return 2; }
    const int rates[3] = {256000, 1024000, 2048000}, cutoffs[3] = {15000, 12000, 9000};
    bool ok = true;
    for (int i = 0; i < 3 && ok; i++) {
        const int fs = rates[i];
        fmd_controls c;
        fmd_default_controls(&c);
        c.lpr_cutoff_hz = c.lmr_cutoff_hz = cutoffs[i];
        fmd_coeffs k{};
        design_all(&k, fs, &c);

        PilotFastTab pilot;
        design_pilot_fast(k, &pilot);
        ok = ok && put(fs, "pilot_fast", &pilot, sizeof(pilot));
        PllSpanTab span;
        design_pll_span(k, &span);
        ok = ok && put(fs, "pll_span", &span, sizeof(span));
        PllSparseTab sparse;
        design_pll_sparse(k, &sparse);
        design_wrap_tie(sparse.wrap_tie);
        ok = ok && put(fs, "pll_sparse", &sparse, sizeof(sparse));
        std::vector<uint16_t> img;
        design_front_mfma(k, fs / 256000, img);
        ok = ok && put(fs, "front_mfma", img.data(), img.size() * 2);
        std::vector<uint16_t> slot(kBpTabSlotU16), rds(kBpRdsTabU16), edge(kBpEdgeHalves);
        bp_slot_tap_tables(k.b_lmr, k.b_hilbert, slot.data());
        ok = ok && put(fs, "bp_slot_tap_tables", slot.data(), slot.size() * 2);
        bp_rds_tap_tables(k.b_rds, k.b_hilbert, rds.data());
        ok = ok && put(fs, "bp_rds_tap_tables", rds.data(), rds.size() * 2);
        bp_edge_matrix(k.b_lmr, k.b_hilbert, edge.data());
        ok = ok && put(fs, "bp_edge_matrix", edge.data(), edge.size() * 2);
    }
    if (std::fclose(g_out) != 0) ok = false;
    return ok ? 0 : 1;
}
