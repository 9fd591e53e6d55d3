// The EAS SAME decoder's host unit as a stand-alone program: same_design_main OUTDIR FS...  Per rate it prints "FS P mark_step space_step"
// and writes same_table_FS.f64 ([P][2]), same_ticks_FS.u32 (the 12501 tick starts) and same_audio_FS.f32 (fmd_same_encode of kText, two
// bursts at clock ratio 1.01, amplitude 0.3, mark -3 dB, an eighth of a second of gap); then the default parameters' bytes in hex, what the parser
// and the vote make of a set of well- and ill-formed messages, and "ok".  Linked either with fmd_same_design.cpp itself (the sanitizer
// build, -DSAME_WITH_REF: tests/cpp/same_ref.c is compiled in and decodes the audio in uneven pieces) or with libfmdemod.so (the library
// as it is built).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fmd_same_design.h"
#include "fmdemod.h"

#ifdef SAME_WITH_REF
extern "C" {
#include "same_ref.c"
}
#endif

static const char kText[] = "ZCZC-CIV-EVI-006037-006059+0100-2931415-KABC/FM -";

static void put(const std::string& path, const void* p, size_t bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) { perror(path.c_str()); exit(2); }
    fclose(f);
}

static void show(const char* text) {
    fmd_same_header h;
    const int rc = fmd_same_parse(reinterpret_cast<const unsigned char*>(text), (int)strlen(text), &h);
    printf("parse %d %d %u %s %s %d", rc, h.kind, h.valid, h.org[0] ? h.org : "-", h.event[0] ? h.event : "-", h.n_locations);
    for (int i = 0; i < h.n_locations; i++) printf(" %s", h.locations[i]);
    printf(" %d %d %d %d %s\n", h.duration_min, h.day, h.hour, h.minute, h.callsign[0] ? h.callsign : "-");
}

static fmd_same_message msg(unsigned long long tick, const char* text) {
    fmd_same_message m;
    memset(&m, 0, sizeof(m));
    m.sync_tick = tick; m.len = (unsigned short)strlen(text); m.kind = FMD_SAME_KIND_HEADER;
    memcpy(m.bytes, text, m.len);
    return m;
}

int main(int argc, char** argv) {
    if (argc < 3) return 1;
    const std::string dir = argv[1];
    for (int a = 2; a < argc; a++) {
        const int fs = atoi(argv[a]);
        fmd::SameGeometry g;
        if (!fmd::same_geometry(fs, &g)) return 3;
        printf("%d %d %d %d\n", fs, g.P, g.mark_step, g.space_step);
        std::vector<double> tab(2 * (size_t)g.P);
        fmd::same_table(g.P, tab.data());
        put(dir + "/same_table_" + argv[a] + ".f64", tab.data(), tab.size() * sizeof(double));
        std::vector<unsigned> ticks(12501);
        for (unsigned r = 0; r <= 12500u; r++) ticks[r] = fmd::same_tick_start(fs, r);
        put(dir + "/same_ticks_" + argv[a] + ".u32", ticks.data(), ticks.size() * sizeof(unsigned));
        fmd_same_encode_config cfg{fs, 2, fs / 8, 1.01, 0.3, -3.0};
        const long long n = fmd_same_encode(&cfg, kText, (int)strlen(kText), nullptr, 0);
        if (n <= 0) return 4;
        std::vector<float> audio(2 * (size_t)n);
        if (fmd_same_encode(&cfg, kText, (int)strlen(kText), audio.data(), n - 1) != FMD_ERR_SIZE) return 5;
        if (fmd_same_encode(&cfg, kText, (int)strlen(kText), audio.data(), n) != n) return 6;
        put(dir + "/same_audio_" + argv[a] + ".f32", audio.data(), audio.size() * sizeof(float));
#ifdef SAME_WITH_REF
        same_ref_chan ch;
        std::vector<double> rtab(2 * (size_t)g.P);
        same_ref_table(g.P, rtab.data());
        if (same_ref_create(&ch, fs, rtab.data()) != 0) return 7;
        long long at = 0, step = 1;
        while (at < n) {                                         // pieces of 1, 2, 3 ... frames
            const long long k = at + step > n ? n - at : step;
            same_ref_process(&ch, audio.data() + 2 * at, k);
            at += k; step = step % 97 + 1;
        }
        printf("decoded %llu %llu", ch.st.accepted, ch.st.rejected);
        for (unsigned long long i = 0; i < ch.st.accepted && i < 8; i++) printf(" %.*s|", (int)ch.st.ring[i].len, (const char*)ch.st.ring[i].bytes);
        printf("\n");
#endif
    }
    fmd_same_params p;
    memset(&p, 0xEE, sizeof(p));
    fmd_same_default_params(&p);
    for (size_t i = 0; i < sizeof(p); i++) printf("%02x", reinterpret_cast<const unsigned char*>(&p)[i]);
    printf("\n");
    std::string err;
    fmd_same_params bad = p;
    bad.pull = 129;
    if (fmd::same_check_params(&p, &err) != FMD_OK || fmd::same_check_params(&bad, &err) != FMD_ERR_ARG) return 8;

    show(kText);
    show("NNNN");
    show("ZCZC-WXR-TOR-039173+0030-1051700-KCLE/NWS-\x7f garbage");
    show("ZCZC-WXR-TOR-039173+0030-1051700-KCLE/NWS");          // no closing '-': no call sign
    show("ZCZC-WXR-TOR-039173-03905+0030-1051700-KCLE/NWS-");   // a location of five digits
    show("ZCZC-wxr-T0R-039173+0075-3671700-TOOLONGCALL-");
    show("ZCZC-WXR-TOR-039173");                                 // cut off
    show("ZCZC");
    show("ZCZC-");
    show("ZCZC+");
    {
        std::string many = "ZCZC-EAS-RMT";
        for (int i = 0; i < 32; i++) many += "-0010" + std::to_string(10 + i);   // 32 locations: one too many
        many += "+0015-0010000-WXYZ-";
        show(many.c_str());
        std::string full(268, 'Z');
        memcpy(&full[0], "ZCZC-", 5);
        show(full.c_str());
    }
    fmd_same_message three[3] = {msg(100, kText), msg(100 + 9000, kText), msg(100 + 18000, kText)}, out;
    three[1].bytes[9] = 'X'; three[2].bytes[20] = '?'; three[2].len--;
    int fixed = -1, open = -1;
    int rc = fmd_same_vote(three, 3, &out, &fixed, &open);
    printf("vote %d %d %d %.*s\n", rc, fixed, open, (int)out.len, (const char*)out.bytes);
    three[0].bytes[9] = 'Y';
    rc = fmd_same_vote(three, 3, &out, &fixed, &open);
    printf("vote %d %d %d %.*s\n", rc, fixed, open, (int)out.len, (const char*)out.bytes);
    rc = fmd_same_vote(three, 2, &out, &fixed, &open);
    printf("vote %d %d %d %.*s\n", rc, fixed, open, (int)out.len, (const char*)out.bytes);
    three[2].sync_tick = 1000000;
    printf("vote %d\n", fmd_same_vote(three, 3, &out, &fixed, &open));
    printf("vote %d\n", fmd_same_vote(three, 4, &out, &fixed, &open));
    printf("ok\n");
    return 0;
}
