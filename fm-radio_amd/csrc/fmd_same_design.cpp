// Built with -ffp-contract=off -fno-fast-math (Makefile): every double operation is the one written, so the table, the tick boundaries
// and the encoder's audio are the pure functions that tests/cpp/same_ref.c restates.
#include "fmd_same_design.h"

#include <cmath>
#include <cstring>

namespace fmd {

std::string& same_global_error() {
    thread_local std::string e;
    return e;
}

static int same_gcd(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

bool same_geometry(int fs, SameGeometry* g) {
    if (fs < 8000 || fs > 48000 || fs % 10 != 0) return false;
    const int d = same_gcd(3125, 6 * fs);
    g->P = 6 * fs / d;
    g->mark_step = (4 * 3125 / d) % g->P;
    g->space_step = (3 * 3125 / d) % g->P;
    return true;
}

// libm's cos and libm's sin, each called on its own (one sincos() is not everywhere the bits of the two)
__attribute__((noinline)) static double sd_cos(double a) { return std::cos(a); }
__attribute__((noinline)) static double sd_sin(double a) { return std::sin(a); }

void same_table(int P, double* tab) {
    for (int j = 0; j < P; j++) {
        tab[2 * j] = sd_cos(2.0 * M_PI * (double)j / (double)P);
        tab[2 * j + 1] = sd_sin(2.0 * M_PI * (double)j / (double)P);
    }
}

unsigned same_tick_start(int fs, unsigned r) { return (r * 3u * (unsigned)fs + 12499u) / 12500u; }   // (r <= 12500: below 2^31)

int same_check_params(const fmd_same_params* p, std::string* err) {
    if (!p) { *err = "null parameters"; return FMD_ERR_ARG; }
    if (p->pull < 0 || p->pull > 128) { *err = "pull outside 0 ... 128"; return FMD_ERR_ARG; }
    if (p->hold_ticks < 1u || p->hold_ticks > 0x7fffffffu) { *err = "hold_ticks outside 1 ... 2^31 - 1"; return FMD_ERR_ARG; }
    if (p->alarm_mask > 3u) { *err = "alarm_mask has a bit above bit 1"; return FMD_ERR_ARG; }
    if (p->reserved != 0u) { *err = "reserved is not 0"; return FMD_ERR_ARG; }
    return FMD_OK;
}

}  // namespace fmd

static int sd_fail(int code, const char* msg) {
    fmd::same_global_error() = msg;
    return code;
}

// how far into its burst frame i stands, in bits
static double sd_bits_in(long long i, double ratio, int fs) { return ((double)i * ratio * 3125.0) / (6.0 * (double)fs); }

static bool sd_digits(const unsigned char* s, int n) {
    for (int i = 0; i < n; i++)
        if (s[i] < '0' || s[i] > '9') return false;
    return true;
}
static int sd_num(const unsigned char* s, int n) {
    int v = 0;
    for (int i = 0; i < n; i++) v = 10 * v + (s[i] - '0');
    return v;
}

extern "C" {

void fmd_same_default_params(fmd_same_params* p) {
    if (!p) return;
    p->pull = 16;
    p->hold_ticks = 750000u;
    p->alarm_mask = 0u;
    p->reserved = 0u;
}

long long fmd_same_encode(const fmd_same_encode_config* cfg, const char* text, int len, float* out, long long cap) {
    fmd::SameGeometry geo;
    if (!cfg || !text) return sd_fail(FMD_ERR_ARG, "null configuration or text");
    if (!fmd::same_geometry(cfg->fs, &geo)) return sd_fail(FMD_ERR_ARG, "fs is not a multiple of 10 in 8000 ... 48000");
    if (len < 1 || len > FMD_SAME_MAX_BYTES) return sd_fail(FMD_ERR_ARG, "len outside 1 ... 268");
    if (cfg->repeats < 1 || cfg->repeats > 16) return sd_fail(FMD_ERR_ARG, "repeats outside 1 ... 16");
    if (!(cfg->clock_ratio >= 0.9 && cfg->clock_ratio <= 1.1)) return sd_fail(FMD_ERR_ARG, "clock_ratio outside [0.9, 1.1]");
    if (!(cfg->amplitude >= 0.0 && cfg->amplitude < INFINITY)) return sd_fail(FMD_ERR_ARG, "amplitude is negative or not finite");
    if (!(cfg->mark_db >= -40.0 && cfg->mark_db <= 40.0)) return sd_fail(FMD_ERR_ARG, "mark_db outside [-40, 40]");
    if (cfg->gap_frames > (1LL << 30)) return sd_fail(FMD_ERR_ARG, "gap_frames above 2^30");
    const int fs = cfg->fs;
    const double ratio = cfg->clock_ratio;
    const long long gap = cfg->gap_frames < 0 ? (long long)fs : cfg->gap_frames;
    const long long nbits = 8LL * (16 + len);
    // the burst's frames: every i whose place is in front of the last bit's end
    long long nb = (long long)((double)nbits * 6.0 * (double)fs / (3125.0 * ratio)) - 2;
    if (nb < 0) nb = 0;
    while (sd_bits_in(nb, ratio, fs) < (double)nbits) nb++;
    const long long total = (long long)cfg->repeats * (nb + gap);
    if (!out) return total;
    if (cap < total) return sd_fail(FMD_ERR_SIZE, "cap is below the frames of the whole");
    const double a_space = cfg->amplitude, a_mark = cfg->amplitude * std::pow(10.0, cfg->mark_db / 20.0);
    float* o = out;
    for (int r = 0; r < cfg->repeats; r++) {
        for (long long i = 0; i < nb; i++) {
            const double u = sd_bits_in(i, ratio, fs);
            long long b = (long long)u;
            if (b >= nbits) b = nbits - 1;
            const double frac = u - (double)b;
            const long long byte = b >> 3;
            const unsigned v = byte < 16 ? 0xABu : (unsigned)(unsigned char)text[byte - 16];
            const int bit = (int)((v >> (b & 7)) & 1u);
            const double cyc = bit ? 4.0 : 3.0, a = bit ? a_mark : a_space;
            const float s = (float)(a * fmd::sd_sin(2.0 * M_PI * cyc * frac));
            *o++ = s; *o++ = s;
        }
        for (long long i = 0; i < 2 * gap; i++) *o++ = 0.0f;
    }
    return total;
}

int fmd_same_parse(const unsigned char* bytes, int len, fmd_same_header* out) {
    if (!bytes || !out) return sd_fail(FMD_ERR_ARG, "null message or output");
    std::memset(out, 0, sizeof(*out));
    if (len < 4 || len > FMD_SAME_MAX_BYTES) return sd_fail(FMD_ERR_ARG, "len outside 4 ... 268");
    if (std::memcmp(bytes, "NNNN", 4) == 0) { out->kind = FMD_SAME_KIND_EOM; return FMD_OK; }
    if (std::memcmp(bytes, "ZCZC", 4) != 0) return sd_fail(FMD_ERR_ARG, "the message starts with neither ZCZC nor NNNN");
    out->kind = FMD_SAME_KIND_HEADER;
    int pos = 4;
    // the next field: behind a '-', up to the next '-' or '+' (which *delim names) or the message's end (*delim = 0)
    auto field = [&](const unsigned char** f, int* n, char* delim) {
        if (pos >= len || bytes[pos] != '-') return false;
        const int a = ++pos;
        while (pos < len && bytes[pos] != '-' && bytes[pos] != '+') pos++;
        *f = bytes + a; *n = pos - a; *delim = pos < len ? (char)bytes[pos] : 0;
        return true;
    };
    auto upper3 = [](const unsigned char* f, int n) { return n == 3 && f[0] >= 'A' && f[0] <= 'Z' && f[1] >= 'A' && f[1] <= 'Z' && f[2] >= 'A' && f[2] <= 'Z'; };
    const unsigned char* f; int n; char d;
    if (!field(&f, &n, &d) || d != '-') return FMD_OK;
    if (upper3(f, n)) { std::memcpy(out->org, f, 3); out->valid |= FMD_SAME_VALID_ORG; }
    if (!field(&f, &n, &d) || d != '-') return FMD_OK;
    if (upper3(f, n)) { std::memcpy(out->event, f, 3); out->valid |= FMD_SAME_VALID_EVENT; }
    // locations up to the '+'
    bool loc_ok = true;
    int nl = 0;
    for (;;) {
        if (!field(&f, &n, &d) || d == 0) return FMD_OK;         // no '+' in the message: nothing behind is to be trusted
        if (n == 6 && sd_digits(f, 6) && nl < FMD_SAME_MAX_LOCATIONS) std::memcpy(out->locations[nl++], f, 6);
        else loc_ok = false;
        if (d == '+') break;
    }
    if (loc_ok) { out->n_locations = nl; out->valid |= FMD_SAME_VALID_LOCATIONS; }
    else std::memset(out->locations, 0, sizeof(out->locations));
    // +TTTT: the '+' stands where the other fields have their '-'
    {
        const int a = ++pos;
        while (pos < len && bytes[pos] != '-' && bytes[pos] != '+') pos++;
        if (pos >= len || bytes[pos] != '-') return FMD_OK;
        f = bytes + a; n = pos - a;
        if (n == 4 && sd_digits(f, 4) && sd_num(f + 2, 2) < 60) { out->duration_min = 60 * sd_num(f, 2) + sd_num(f + 2, 2); out->valid |= FMD_SAME_VALID_DURATION; }
    }
    if (!field(&f, &n, &d) || d != '-') return FMD_OK;
    if (n == 7 && sd_digits(f, 7) && sd_num(f, 3) >= 1 && sd_num(f, 3) <= 366 && sd_num(f + 3, 2) < 24 && sd_num(f + 5, 2) < 60) {
        out->day = sd_num(f, 3); out->hour = sd_num(f + 3, 2); out->minute = sd_num(f + 5, 2);
        out->valid |= FMD_SAME_VALID_TIME;
    }
    if (!field(&f, &n, &d) || d != '-') return FMD_OK;            // the call sign counts only with its closing '-'
    if (n >= 1 && n <= 8) { std::memcpy(out->callsign, f, (size_t)n); out->valid |= FMD_SAME_VALID_CALLSIGN; }
    return FMD_OK;
}

int fmd_same_vote(const fmd_same_message* msgs, int n, fmd_same_message* out, int* corrected, int* unresolved) {
    if (!msgs || !out) return sd_fail(FMD_ERR_ARG, "null messages or output");
    if (n < 1 || n > 3) return sd_fail(FMD_ERR_ARG, "n outside 1 ... 3");
    for (int i = 0; i < n; i++) {
        if (msgs[i].len > FMD_SAME_MAX_BYTES || msgs[i].kind != msgs[0].kind) return sd_fail(FMD_ERR_ARG, "a message is too long, or the messages are not of one kind");
        if (i > 0) {
            if (msgs[i].sync_tick < msgs[i - 1].sync_tick) return sd_fail(FMD_ERR_ARG, "the messages are not in ascending sync_tick");
            if (msgs[i].sync_tick - msgs[i - 1].sync_tick > 10416ull + 64ull * msgs[i - 1].len) return sd_fail(FMD_ERR_STATE, "the messages are no bursts of one transmission");
        }
    }
    int fixed = 0, open = 0;
    // of three values: the majority's and whether all agreed; without a majority the first
    auto vote = [&](unsigned a, unsigned b, unsigned c) {
        if (a == b && b == c) return a;
        if (a == b || a == c) { fixed++; return a; }
        if (b == c) { fixed++; return b; }
        open++;
        return a;
    };
    fmd_same_message r;
    std::memset(&r, 0, sizeof(r));
    r.sync_tick = msgs[0].sync_tick;
    r.kind = msgs[0].kind;
    if (n == 1) {
        r.len = msgs[0].len;
        std::memcpy(r.bytes, msgs[0].bytes, r.len);
    } else if (n == 2) {
        r.len = msgs[0].len;
        const unsigned m = msgs[0].len > msgs[1].len ? msgs[0].len : msgs[1].len;
        for (unsigned i = 0; i < m; i++) {
            const int a = i < msgs[0].len ? msgs[0].bytes[i] : -1, b = i < msgs[1].len ? msgs[1].bytes[i] : -1;
            if (a != b) open++;
            if (a >= 0) r.bytes[i] = (unsigned char)a;
        }
    } else {
        const int f0 = fixed, o0 = open;
        r.len = (unsigned short)vote(msgs[0].len, msgs[1].len, msgs[2].len);
        fixed = f0; open = o0;                                    // (the bytes past a shorter copy's end tell of the lengths)
        unsigned m = r.len;
        for (int i = 0; i < 3; i++) m = msgs[i].len > m ? msgs[i].len : m;
        for (unsigned i = 0; i < m; i++) {
            // a copy that has ended reads as 256: no byte
            const unsigned v = vote(i < msgs[0].len ? msgs[0].bytes[i] : 256u, i < msgs[1].len ? msgs[1].bytes[i] : 256u, i < msgs[2].len ? msgs[2].bytes[i] : 256u);
            if (i < r.len) r.bytes[i] = (unsigned char)(v & 255u);
        }
    }
    *out = r;
    if (corrected) *corrected = fixed;
    if (unresolved) *unresolved = open;
    return FMD_OK;
}

}  // extern "C"
