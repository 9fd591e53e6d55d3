// Test driver for the adaptor's RDS surface, written the way the reference's GUI reads App (reference src/gui/render_rds_database.cpp:27-46):
// feed a u8 capture in odd-sized pieces, then print the database App_GPU::GetRDSDatabase() holds, press "Reset Database", feed
// one more block and print it again.  Also reads the newest block's GetRDSRawSymbols() next to GetRDSPredSymbols().
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "broadcast_fm_demod_gpu.hpp"

// texts printed whole, an empty (0) character as '.'
static std::string text(const char* s, size_t n) {
    std::string t(s, n);
    for (char& ch : t) if (ch == 0) ch = '.';
    return t;
}

static void print_db(const fmd_host::RDS_Database_GPU& db) {
    printf("PI=%04X PTY=%u PS='%s' RT='%s' date=%02d/%02d/%04d time=%02u:%02u LTO=%d TA=%d music=%d stereo=%d af=%zu\n", db.PI_code,
           db.programme_type, text(db.service_name, 8).c_str(), text(db.radio_text, 64).c_str(), db.datetime.day,
           db.datetime.month, db.datetime.year, db.datetime.hour, db.datetime.minute, (int)db.local_time_offset, (int)db.traffic_announcement,
           (int)db.is_music, (int)db.is_stereo, db.alt_freqs.size());
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: rds_app_main <capture.u8> <block_size>\n"); return 1; }
    const int block_size = atoi(argv[2]);
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    fseek(fp, 0, SEEK_END); long bytes = ftell(fp); fseek(fp, 0, SEEK_SET);
    std::vector<uint8_t> data((size_t)bytes);
    if (fread(data.data(), 1, data.size(), fp) != data.size()) return 2;
    fclose(fp);
    const size_t n = data.size() / 2, last = n - (size_t)block_size;
    fmd_host::App_GPU app(block_size);
    size_t pos = 0, piece = 777;
    while (pos < last) {
        const size_t take = std::min(piece, last - pos);
        app.Process(data.data() + 2 * pos, take);
        pos += take;
        piece = piece * 3 % 40009 + 1;
    }
    auto& db = app.GetRDSDatabase();
    print_db(db);
    auto raw = app.GetFMDemod().GetRDSRawSymbols();
    auto pred = app.GetFMDemod().GetRDSPredSymbols();
    int same_sign = 0;
    for (size_t i = 0; i < raw.size(); i++) same_sign += ((raw.data()[i].real() > 0.0f) == (pred.data()[i] > 0.0f));
    printf("raw_symbols=%zu pred_symbols=%zu same_sign=%d\n", raw.size(), pred.size(), same_sign);
    db.Reset();
    print_db(db);
    app.Process(data.data() + 2 * pos, n - pos);
    print_db(app.GetRDSDatabase());
    return 0;
}
