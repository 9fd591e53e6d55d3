// k_rds_decode: the reference's RDS decoding chain (src/rds_decoder/rds_decoding_chain.h) on the GPU, one lane per station.
// Included from fmd_kernels.hip inside namespace fmd.
//
//   group sync     RDS_Group_Sync (rds_group_sync.cpp:29-127): FINDING_SYNC on offset word A with a zero syndrome, READ_BLOCK with
//                  the offset words A, B, C then C' if C fails, D; single-bit correction from the syndrome table (crc10.cpp:28-60);
//                  back to FINDING_SYNC after 3 consecutive groups with errors; a group is delivered every 4 blocks, valid or not.
//   group decoder  RDS_Decoder::ProcessGroup / OnGroup* (rds_decoder.cpp:82-540), only the calls that reach the database handler
//   database       RDS_Database_Decoder_Handler (rds_database_decoder_handler.cpp) writing RDS_Database (rds_database.h)
//
// The sliding 26-bit window's syndrome is kept incrementally: CalculateCRC10 (crc10.cpp:9-25) is the remainder of the window
// modulo g(x), which is linear, so shifting in bit b and dropping bit d gives s' = (x s + b) mod g + d (x^26 mod g).  The syndrome
// of the window under an offset word is s ^ offset (offsets are < x^10).  A syndrome table hit always corrects (the code is
// linear: the corrected word's syndrome is 0), so the reference's re-check is implied.  The 26 single-bit syndromes are distinct.
//
// Persistent state (RdsDecBufs) is read at the start of a launch and written back at its end, in place: consecutive blocks'
// launches are ordered on one stream (the handle's RDS stream sR, behind that block's k_rds_sync; the standalone decoder's
// caller stream), so no two launches touch a channel's state at once.

namespace rdsdec {

constexpr uint32_t kPoly = 0x5B9;                 // g(x) = x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1 (rds_constants.h:12-14)
constexpr uint32_t kOffsets[5] = {0x0FC, 0x198, 0x168, 0x350, 0x1B4};   // A, B, C, C', D (rds_constants.h:18-27)

constexpr uint32_t crc10(uint32_t x) {
    uint32_t reg = 0;
    for (int i = 0; i < 26; i++) {
        reg = (reg << 1) | ((x >> 25) & 1u);
        x <<= 1;
        if (reg & 0x400u) reg ^= kPoly;
    }
    return reg & 0x3FFu;
}
constexpr uint32_t kX26 = ((crc10(1u << 25) << 1) & 0x400u) ? (((crc10(1u << 25) << 1)) ^ kPoly) : (crc10(1u << 25) << 1);   // x^26 mod g
struct SynTable { uint16_t s[26]; };
constexpr SynTable make_syn() { SynTable t{}; for (int i = 0; i < 26; i++) t.s[i] = (uint16_t)crc10(1u << i); return t; }
constexpr SynTable kSyn = make_syn();
static_assert(kX26 == 0x0EE, "x^26 mod g(x)");

// error pattern of a syndrome, 0 = no entry (GetCRCErrorFromSyndrome, crc10.cpp:54-60)
__device__ __forceinline__ uint32_t error_pattern(uint32_t s) {
    uint32_t p = 0;
#pragma unroll
    for (int i = 0; i < 26; i++) p |= (s == kSyn.s[i]) ? (1u << i) : 0u;
    return p;
}

// packed block: data | type << 16 | valid << 24 (fmd_rds_block's little-endian layout)
__device__ __forceinline__ uint32_t attempt(uint32_t win, uint32_t syn, int type, bool& valid) {
    const uint32_t s = syn ^ kOffsets[type];
    const uint32_t p = s ? error_pattern(s) : 0u;
    valid = (s == 0) || (p != 0);
    return (((win ^ p) >> 10) & 0xFFFFu) | ((uint32_t)type << 16) | ((uint32_t)valid << 24);
}

__device__ __forceinline__ char rds_char(uint32_t v) { const char c = (char)(v & 0xFF); return c == '\r' ? (char)0 : c; }

// mjd_to_ymd (modified_julian_date.h): 64-bit, 4000 * (J + 1) does not fit 32 bits
__device__ __forceinline__ void mjd_to_ymd(int64_t mjd, int& year, int& month, int& day) {
    int64_t J = mjd + 2400001 + 68569;
    const int64_t C = 4 * J / 146097;
    J = J - (146097 * C + 3) / 4;
    const int64_t Y = 4000 * (J + 1) / 1461001;
    J = J - 1461 * Y / 4 + 31;
    const int64_t M = 80 * J / 2447;
    day = (int)(J - 2447 * M / 80);
    J = M / 11;
    month = (int)(M + 2 - (12 * J));
    year = (int)(100 * (C - 49) + Y + J);
}

// RDS_Decoder::ProcessGroup (rds_decoder.cpp:82-128) and the OnGroup* handlers that reach RDS_Database_Decoder_Handler
__device__ void decode_group(uint32_t gA, uint32_t gB, uint32_t gC, uint32_t gD, fmd_rds_db* db, uint32_t& ab) {
    if (gA >> 24) db->PI_code = (uint16_t)(gA & 0xFFFF);
    if (!(gB >> 24)) return;
    const uint32_t B = gB & 0xFFFF, Cw = gC & 0xFFFF, D = gD & 0xFFFF;
    db->programme_type = (uint8_t)((B >> 5) & 31);
    if ((B >> 11) & 1) return;                             // version B: "Unsupported_Code"
    const bool hasC = (gC >> 24) && ((gC >> 16) & 0xFF) == 2;   // type C, not C'
    const bool hasD = (gD >> 24) && ((gD >> 16) & 0xFF) == 4;
    switch (B >> 12) {
    case 0: {                                              // OnGroup0A (rds_decoder.cpp:159-244)
        const uint32_t seg = B & 3, di = (B >> 2) & 1;
        db->is_music = (uint8_t)((B >> 3) & 1);
        db->traffic_announcement = (uint8_t)((((B >> 10) & 1) << 1) | ((B >> 4) & 1));
        if (hasD) { db->service_name[2 * seg] = rds_char(D >> 8); db->service_name[2 * seg + 1] = rds_char(D); }
        if (seg == 0) db->is_dynamic_program_type = (uint8_t)di;
        else if (seg == 1) db->is_compressed = (uint8_t)di;
        else if (seg == 2) db->is_artificial_head = (uint8_t)di;
        else db->is_stereo = (uint8_t)di;
        break;
    }
    case 2: {                                              // OnGroup2A (rds_decoder.cpp:302-337), OnRadioTextChange
        const uint32_t flag = (B >> 4) & 1, seg = B & 15;
        if (flag != (ab & 0xFF)) { uint32_t* rt = reinterpret_cast<uint32_t*>(db->radio_text); for (int i = 0; i < 16; i++) rt[i] = 0; }
        ab = (ab & ~0xFFu) | flag;
        if (hasC) { db->radio_text[4 * seg] = rds_char(Cw >> 8); db->radio_text[4 * seg + 1] = rds_char(Cw); }
        if (hasD) { db->radio_text[4 * seg + 2] = rds_char(D >> 8); db->radio_text[4 * seg + 3] = rds_char(D); }
        break;
    }
    case 4: {                                              // OnGroup4A (rds_decoder.cpp:363-405)
        const uint32_t mjd = ((B & 3) << 15) | ((Cw & 0xFFFE) >> 1);
        const uint32_t hour = ((Cw & 1) << 4) | ((D >> 12) & 0xF), minute = (D >> 6) & 0x3F;
        const int lto_val = (int)(D & 31);
        const int8_t lto = (int8_t)(lto_val * (((D >> 5) & 1) ? -1 : +1));
        if (hasC) { int y, m, d; mjd_to_ymd((int64_t)mjd, y, m, d); db->datetime.day = d; db->datetime.month = m; db->datetime.year = y; }
        if (hasC && hasD) { db->datetime.hour = (uint8_t)hour; db->datetime.minute = (uint8_t)minute; }
        if (hasD) db->local_time_offset = lto;
        break;
    }
    case 10: {                                             // OnGroup10A (rds_decoder.cpp:407-443), OnProgrammeTypeNameChange
        const uint32_t flag = (B >> 4) & 1, seg = B & 1;
        if (flag != (ab >> 8)) { uint32_t* pt = reinterpret_cast<uint32_t*>(db->programme_type_name); pt[0] = 0; pt[1] = 0; }
        ab = (ab & 0xFFu) | (flag << 8);
        if (hasC) { db->programme_type_name[4 * seg] = rds_char(Cw >> 8); db->programme_type_name[4 * seg + 1] = rds_char(Cw); }
        if (hasD) { db->programme_type_name[4 * seg + 2] = rds_char(D >> 8); db->programme_type_name[4 * seg + 3] = rds_char(D); }
        break;
    }
    default: break;                                        // 1A, 3A, 11A, 14A: no database effect; others unsupported
    }
}

}  // namespace rdsdec

__global__ void __launch_bounds__(kWave) k_rds_decode(RdsDecArgs a) {
    const int c = blockIdx.x * kWave + threadIdx.x;
    if (c >= a.C) return;
    const size_t C = (size_t)a.C;
    uint32_t* f = a.st.f;
    uint32_t win = f[RDS_F_WIN * C + c], syn = f[RDS_F_SYN * C + c], hunt = f[RDS_F_HUNT * C + c];
    uint32_t block_bits = f[RDS_F_BITS * C + c], cur = f[RDS_F_BLOCK * C + c], errs = f[RDS_F_ERRORS * C + c];
    uint32_t desync = f[RDS_F_DESYNC * C + c], ab = f[RDS_F_AB * C + c];
    const uint4 g = reinterpret_cast<const uint4*>(a.st.group)[c];
    uint32_t g0 = g.x, g1 = g.y, g2 = g.z, g3 = g.w;
    fmd_rds_db* db = a.st.db + c;
    uint32_t n_groups = 0, acquisitions = 0;
    fmd_rds_group* gout = a.groups_out + (size_t)c * a.groups_cap;

    int n = a.counts[c];
    n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
    const uint8_t* __restrict__ row = a.bytes + (size_t)c * a.cap;
    // the bytes come in 16-byte chunks held in registers, the next chunk's load issued before the current one is decoded: one memory
    // round trip per chunk instead of one per byte (the database's byte stores below would otherwise order every byte load behind them)
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    auto load16 = [&](int i0) {
        if (vec && i0 + 16 <= n) return *reinterpret_cast<const uint4*>(row + i0);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; k++) if (i0 + k < n) w[k >> 2] |= (uint32_t)row[i0 + k] << (8 * (k & 3));
        return make_uint4(w[0], w[1], w[2], w[3]);
    };
    uint4 next = n > 0 ? load16(0) : make_uint4(0u, 0u, 0u, 0u);
    for (int i0 = 0; i0 < n; i0 += 16) {
        const uint4 chunk = next;
        if (i0 + 16 < n) next = load16(i0 + 16);
        const int nb = n - i0 < 16 ? n - i0 : 16;
        for (int i = 0; i < nb; i++) {
            const uint32_t word = i < 8 ? (i < 4 ? chunk.x : chunk.y) : (i < 12 ? chunk.z : chunk.w);
            const uint32_t byte = (word >> (8 * (i & 3))) & 0xFFu;
            for (int k = 7; k >= 0; k--) {             // bit_reader_t: MSB first (rds_group_sync.h:23-28)
                const uint32_t bit = (byte >> k) & 1u, dropped = (win >> 25) & 1u;
                win = ((win << 1) | bit) & 0x3FFFFFFu;
                syn = (syn << 1) | bit;
                if (syn & 0x400u) syn ^= rdsdec::kPoly;
                if (dropped) syn ^= rdsdec::kX26;
                // FindingSync (rds_group_sync.cpp:46-74): a block A lock starts READ_BLOCK with the window as its first block;
                // ReadingGroup (:76-127): a block every 26 bits.  Written as selects: the one branch per bit is the (rare) block boundary
                const bool lock = hunt && syn == rdsdec::kOffsets[0];
                const uint32_t bb = hunt ? 0u : block_bits + 1u;
                const bool boundary = lock || bb == 26u;
                block_bits = bb == 26u ? 0u : bb;
                acquisitions += lock ? 1u : 0u;
                hunt = lock ? 0u : hunt;
                if (!boundary) continue;
                // PushBlock (rds_group_sync.cpp:222-253): curr_data_block < 4 here
                bool valid;
                if (cur == 0) g0 = rdsdec::attempt(win, syn, 0, valid);
                else if (cur == 1) g1 = rdsdec::attempt(win, syn, 1, valid);
                else if (cur == 2) { g2 = rdsdec::attempt(win, syn, 2, valid); if (!valid) g2 = rdsdec::attempt(win, syn, 3, valid); }
                else g3 = rdsdec::attempt(win, syn, 4, valid);
                cur++;
                errs += valid ? 0u : 1u;
                if (cur < 4) continue;
                if (n_groups < (uint32_t)a.groups_cap) reinterpret_cast<uint4*>(gout)[n_groups] = make_uint4(g0, g1, g2, g3);
                n_groups++;
                rdsdec::decode_group(g0, g1, g2, g3, db, ab);
                const uint32_t e = errs;
                cur = 0;
                errs = 0;
                if (e == 0) { desync = 0; continue; }
                if (++desync >= 3) { hunt = 1; desync = 0; }
            }
        }
    }

    f[RDS_F_WIN * C + c] = win; f[RDS_F_SYN * C + c] = syn; f[RDS_F_HUNT * C + c] = hunt;
    f[RDS_F_BITS * C + c] = block_bits; f[RDS_F_BLOCK * C + c] = cur; f[RDS_F_ERRORS * C + c] = errs;
    f[RDS_F_DESYNC * C + c] = desync; f[RDS_F_AB * C + c] = ab;
    reinterpret_cast<uint4*>(a.st.group)[c] = make_uint4(g0, g1, g2, g3);
    db->in_sync = hunt ? 0 : 1;
    db->groups += n_groups;
    db->sync_acquisitions += acquisitions;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(db);
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.db_out + c);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(fmd_rds_db) / 4); i++) dst[i] = src[i];
    a.groups_count[c] = (int)n_groups;
}

hipError_t launch_rds_decode(const RdsDecArgs& a, hipStream_t s, hipEvent_t t1) {
    const dim3 grid((unsigned)((a.C + kWave - 1) / kWave));
    if (t1) hipExtLaunchKernelGGL(k_rds_decode, grid, dim3(kWave), 0, s, nullptr, t1, 0, a);
    else hipLaunchKernelGGL(k_rds_decode, grid, dim3(kWave), 0, s, a);
    return hipGetLastError();
}
