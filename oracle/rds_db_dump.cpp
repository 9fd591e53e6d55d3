// TEST INFRASTRUCTURE — dump harness around the *unmodified* reference RDS decoding chain.
//
// Ours; compiled together with the reference's src/rds_decoder/*.cpp (oracle/Makefile, target `ref`) into oracle/_ref/fm_rds_db_dump.
// Feeds a byte stream to one RDS_Decoding_Chain (src/rds_decoder/rds_decoding_chain.h) in the chunks a list names and, after every
// chunk, writes what the chain delivered and holds:
//
//   fm_rds_db_dump <bytes.bin> <chunks.txt> <out.bin> [reset_db_after_chunk ...]
//
//   chunks.txt   chunk sizes in bytes, whitespace separated (their sum is the stream's length)
//   out.bin      per chunk: int32 n_groups, n_groups x 16-byte group records, one 120-byte database record — the layouts of
//                include/fmdemod.h's fmd_rds_group and fmd_rds_db (status fields: in_sync, groups, sync_acquisitions)
//   reset_db_after_chunk   chunk indices after which RDS_Database::Reset() is called (the GUI's reset button,
//                src/gui/render_rds_database.cpp:46), after that chunk's record is written
//
// The reference's decoder logs every group on stderr; the harness sends that to <out.bin>.log (removed at the end) and counts the
// synchroniser's lock lines in it.  in_sync is written as 0 (the synchroniser's state is private).
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "rds_decoder/rds_decoding_chain.h"

namespace {

#pragma pack(push, 1)
struct BlockRec { uint16_t data; uint8_t block_type; uint8_t is_valid; };
struct DbRec {
    char service_name[8], programme_type_name[8], radio_text[64];
    uint16_t PI_code;
    uint8_t programme_type;
    uint8_t is_stereo, is_music, is_artificial_head, is_compressed, is_dynamic_program_type;
    int32_t day, month, year;
    uint8_t hour, minute, pad0[2];
    int8_t local_time_offset;
    uint8_t traffic_announcement;
    uint8_t pad1[2];
    int32_t in_sync;
    uint32_t groups, sync_acquisitions;
};
#pragma pack(pop)
static_assert(sizeof(BlockRec) == 4 && sizeof(DbRec) == 120, "fmdemod.h layouts");

std::vector<uint8_t> read_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(1); }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s bytes.bin chunks.txt out.bin [reset_db_after_chunk ...]\n", argv[0]); return 2; }
    const std::vector<uint8_t> bytes = read_file(argv[1]);
    std::vector<long> chunks;
    {
        FILE* f = fopen(argv[2], "r");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
        long v;
        while (fscanf(f, "%ld", &v) == 1) chunks.push_back(v);
        fclose(f);
    }
    std::set<long> resets;
    for (int i = 4; i < argc; i++) resets.insert(atol(argv[i]));
    FILE* out = fopen(argv[3], "wb");
    if (!out) { fprintf(stderr, "cannot open %s\n", argv[3]); return 1; }

    auto chain = std::make_unique<RDS_Decoding_Chain>();
    std::vector<BlockRec> groups;
    uint32_t n_groups_total = 0, n_locks = 0;
    // the synchroniser's state is private: its lock acquisitions are counted from its own log line (rds_group_sync.cpp:64), which
    // goes to stderr — redirected into <out.bin>.log and read back behind the chain
    const std::string log_path = std::string(argv[3]) + ".log";
    if (!freopen(log_path.c_str(), "w", stderr)) return 1;
    setvbuf(stderr, nullptr, _IONBF, 0);
    FILE* log = fopen(log_path.c_str(), "r");
    if (!log) return 1;
    // a second observer of the synchroniser's groups, behind the decoder's (rds_decoding_chain.h:17-19)
    chain->group_sync.OnGroup().Attach([&](rds_group_t g) {
        for (int i = 0; i < 4; i++) groups.push_back({g[i].data, (uint8_t)g[i].block_type, (uint8_t)g[i].is_valid});
        n_groups_total++;
    });

    size_t pos = 0;
    for (size_t k = 0; k < chunks.size(); k++) {
        const size_t n = (size_t)chunks[k];
        if (pos + n > bytes.size()) { fprintf(stderr, "chunk list longer than the stream\n"); return 1; }
        groups.clear();
        chain->Process(tcb::span<const uint8_t>(bytes.data() + pos, n));
        pos += n;
        fflush(stderr);
        char line[4096];
        while (fgets(line, sizeof(line), log)) if (strstr(line, "[rds_sync] Locked onto block A")) n_locks++;
        clearerr(log);
        const int32_t ng = (int32_t)(groups.size() / 4);
        fwrite(&ng, 4, 1, out);
        if (!groups.empty()) fwrite(groups.data(), sizeof(BlockRec), groups.size(), out);
        const RDS_Database& db = chain->db;
        DbRec r;
        memset(&r, 0, sizeof(r));
        memcpy(r.service_name, db.service_name, 8);
        memcpy(r.programme_type_name, db.programme_type_name, 8);
        memcpy(r.radio_text, db.radio_text, 64);
        r.PI_code = db.PI_code;
        r.programme_type = db.programme_type;
        r.is_stereo = db.is_stereo; r.is_music = db.is_music; r.is_artificial_head = db.is_artificial_head;
        r.is_compressed = db.is_compressed; r.is_dynamic_program_type = db.is_dynamic_program_type;
        r.day = db.datetime.day; r.month = db.datetime.month; r.year = db.datetime.year;
        r.hour = db.datetime.hour; r.minute = db.datetime.minute;
        r.local_time_offset = db.local_time_offset;
        r.traffic_announcement = (uint8_t)db.traffic_announcement;
        r.groups = n_groups_total;
        r.sync_acquisitions = n_locks;      // in_sync stays 0: not observable from outside the reference's synchroniser
        fwrite(&r, sizeof(r), 1, out);
        if (resets.count((long)k)) chain->db.Reset();
    }
    fclose(out);
    fclose(log);
    remove(log_path.c_str());
    return 0;
}
