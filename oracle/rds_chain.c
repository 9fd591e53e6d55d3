/* rds_chain.c — TEST INFRASTRUCTURE: the reference's RDS_Decoding_Chain restated in C, line by line with citations (reference
 * src/rds_decoder/).  The tests check it against the reference's own chain (oracle/rds_db_dump.cpp) and the GPU kernel against it. */
#include <string.h>

#include "rds_chain.h"

/* ==========================================================================================================================
 * RDS decoding chain — reference src/rds_decoder/rds_decoding_chain.h:11-31
 * ========================================================================================================================== */
static const uint16_t kRdsOffsets[5] = {0x0FC, 0x198, 0x168, 0x350, 0x1B4};   /* A, B, C, C1, D: rds_constants.h:18-27 */

/* CalculateCRC10, crc10.cpp:9-25 (RDS_CRC10_POLY = 0b0110111001, rds_constants.h:13) */
static uint16_t rds_crc10(uint32_t x) {
    uint16_t reg = 0;
    for (int i = 0; i < 26; i++) {
        const uint16_t bit = (uint16_t)((x & (1u << 25)) >> 25);
        x = x << 1;
        reg = (uint16_t)((reg << 1) | bit);
        if (reg & (1u << 10)) reg = reg ^ 0x1B9;
    }
    return reg & 0x3FF;
}

/* CRC10_ERROR_PATTERNS + GetCRCErrorFromSyndrome, crc10.cpp:28-60: the 16 data-bit patterns, then the 10 checksum-bit patterns
 * (a later insertion overwrites an earlier one with the same syndrome); 0 = no entry */
static uint32_t rds_error_pattern(uint16_t syndrome) {
    uint32_t found = 0;
    for (int i = 10; i < 26; i++) if (rds_crc10(1u << i) == syndrome) found = 1u << i;
    for (int i = 0; i < 10; i++) if (rds_crc10(1u << i) == syndrome) found = 1u << i;
    return found;
}

/* AttemptDecode + ValidateCRCCodeword, rds_group_sync.cpp:145-220 */
static int rds_attempt(uint32_t x, int id, fmo_rds_block* b) {
    x = x ^ kRdsOffsets[id];
    uint32_t corrected = x;
    int valid = 0;
    const uint16_t syndrome = rds_crc10(x);
    if (syndrome == 0) valid = 1;
    else {
        const uint32_t pattern = rds_error_pattern(syndrome);
        if (pattern != 0 && rds_crc10(x ^ pattern) == 0) { corrected = x ^ pattern; valid = 1; }
    }
    b->block_type = (uint8_t)id;
    b->data = (uint16_t)((corrected & (0xFFFFu << 10)) >> 10);
    b->is_valid = (uint8_t)valid;
    return valid;
}

/* PushBlock, rds_group_sync.cpp:222-253 */
static void rds_push_block(fmo_rds_chain* ch, uint32_t x) {
    fmo_rds_block* b = &ch->group.blocks[ch->curr_block];
    b->is_valid = 0;
    switch (ch->curr_block) {
    case 0: rds_attempt(x, 0, b); break;
    case 1: rds_attempt(x, 1, b); break;
    case 2: if (!rds_attempt(x, 2, b)) rds_attempt(x, 3, b); break;
    case 3: rds_attempt(x, 4, b); break;
    default: break;
    }
    ch->curr_block++;
    if (!b->is_valid) ch->block_errors++;
}

static char rds_char(int v) { const char c = (char)(v & 0xFF); return c == '\r' ? 0 : c; }   /* OnServiceName etc.: '\r' -> 0 */

/* mjd_to_ymd, modified_julian_date.h:9-22 (long: 64 bits here, as on the reference's Linux build) */
static void rds_mjd_to_ymd(long mjd, int* year, int* month, int* day) {
    long J, Cc, Y, M;
    J = mjd + 2400001 + 68569;
    Cc = 4 * J / 146097;
    J = J - (146097 * Cc + 3) / 4;
    Y = 4000 * (J + 1) / 1461001;
    J = J - 1461 * Y / 4 + 31;
    M = 80 * J / 2447;
    *day = (int)(J - 2447 * M / 80);
    J = M / 11;
    *month = (int)(M + 2 - (12 * J));
    *year = (int)(100 * (Cc - 49) + Y + J);
}

/* RDS_Decoder::ProcessGroup (rds_decoder.cpp:82-128) -> OnGroupType (:128-157) -> the handlers with a database effect;
 * RDS_Database_Decoder_Handler (rds_database_decoder_handler.cpp) inlined */
static void rds_process_group(fmo_rds_chain* ch) {
    const fmo_rds_block* A = &ch->group.blocks[0];
    const fmo_rds_block* B = &ch->group.blocks[1];
    const fmo_rds_block* Cb = &ch->group.blocks[2];
    const fmo_rds_block* D = &ch->group.blocks[3];
    fmo_rds_db* db = &ch->db;
    const uint16_t descriptor = B->data;
    const int group_code = (descriptor & 0xF000) >> 12, version = (descriptor & 0x0800) >> 11;
    if (A->is_valid) db->PI_code = A->data;                                  /* OnProgrammeIdentifier */
    if (!B->is_valid) return;
    db->programme_type = (uint8_t)((descriptor & 0x03E0) >> 5);             /* OnProgrammeType */
    if (version) return;                                                     /* version B: Unsupported_Code */
    const int has_C = Cb->is_valid && Cb->block_type == 2, has_D = D->is_valid && D->block_type == 4;
    switch (group_code) {
    case 0: {   /* OnGroup0A, rds_decoder.cpp:159-244 */
        const int tp = (B->data & 0x0400) >> 10, ta = (B->data & 0x10) >> 4, ms = (B->data & 0x08) >> 3, di = (B->data & 0x04) >> 2, seg = B->data & 3;
        db->is_music = (uint8_t)ms;                                          /* OnMusicSpeech */
        db->traffic_announcement = (uint8_t)(((tp & 1) << 1) | (ta & 1));   /* OnTrafficAnnouncement, handler.cpp:55-75 */
        if (has_D) { db->service_name[2 * seg] = rds_char(D->data >> 8); db->service_name[2 * seg + 1] = rds_char(D->data & 0xFF); }
        switch (seg) {
        case 0: db->is_dynamic_program_type = (uint8_t)di; break;
        case 1: db->is_compressed = (uint8_t)di; break;
        case 2: db->is_artificial_head = (uint8_t)di; break;
        default: db->is_stereo = (uint8_t)di; break;
        }
        break;
    }
    case 2: {   /* OnGroup2A, rds_decoder.cpp:302-337; OnRadioTextChange, handler.cpp:40-45 */
        const uint8_t ab = (uint8_t)((B->data & 0x10) >> 4);
        const int index = (B->data & 0x0F) * 4;
        if (ab != ch->ab_radio_text) memset(db->radio_text, 0, sizeof(db->radio_text));
        ch->ab_radio_text = ab;
        if (has_C) { db->radio_text[index] = rds_char(Cb->data >> 8); db->radio_text[index + 1] = rds_char(Cb->data & 0xFF); }
        if (has_D) { db->radio_text[index + 2] = rds_char(D->data >> 8); db->radio_text[index + 3] = rds_char(D->data & 0xFF); }
        break;
    }
    case 4: {   /* OnGroup4A, rds_decoder.cpp:363-405 */
        const uint32_t mjd = ((uint32_t)(B->data & 0x3) << 15) | ((uint32_t)(Cb->data & 0xFFFE) >> 1);
        const uint8_t hour = (uint8_t)(((Cb->data & 0x1) << 4) | ((D->data & 0xF000) >> 12));
        const uint8_t minute = (uint8_t)((D->data & 0x0FC0) >> 6);
        const uint8_t lto_sign = (uint8_t)((D->data & 0x20) >> 5), lto_val = (uint8_t)(D->data & 0x1F);
        const int8_t lto = (int8_t)((int8_t)lto_val * (lto_sign ? -1 : +1));
        int year, month, day;
        rds_mjd_to_ymd((long)mjd, &year, &month, &day);
        if (has_C) { db->datetime.day = day; db->datetime.month = month; db->datetime.year = year; }
        if (has_C && has_D) { db->datetime.hour = hour; db->datetime.minute = minute; }
        if (has_D) db->local_time_offset = lto;
        break;
    }
    case 10: {  /* OnGroup10A, rds_decoder.cpp:407-443; OnProgrammeTypeNameChange, handler.cpp:28-33 */
        const uint8_t ab = (uint8_t)((B->data & 0x10) >> 4);
        const int index = 4 * (B->data & 0x1);
        if (ab != ch->ab_programme_type_name) memset(db->programme_type_name, 0, sizeof(db->programme_type_name));
        ch->ab_programme_type_name = ab;
        if (has_C) { db->programme_type_name[index] = rds_char(Cb->data >> 8); db->programme_type_name[index + 1] = rds_char(Cb->data & 0xFF); }
        if (has_D) { db->programme_type_name[index + 2] = rds_char(D->data >> 8); db->programme_type_name[index + 3] = rds_char(D->data & 0xFF); }
        break;
    }
    default: break;   /* 1A, 3A, 11A, 14A log only; the rest is Unsupported_Code */
    }
}

void fmo_rds_chain_init(fmo_rds_chain* ch) {
    memset(ch, 0, sizeof(*ch));
    ch->finding_sync = 1;                                        /* State::FINDING_SYNC, rds_group_sync.cpp:14-27 */
    ch->ab_radio_text = ch->ab_programme_type_name = 0x4;        /* rds_database_decoder_handler.h:11-12 */
}

size_t fmo_rds_chain_size(void) { return sizeof(fmo_rds_chain); }
void fmo_rds_chain_get_db(const fmo_rds_chain* ch, fmo_rds_db* db) { *db = ch->db; }

void fmo_rds_chain_reset_db(fmo_rds_chain* ch) {                 /* RDS_Database::Reset, rds_database.h:58-79 */
    const int32_t in_sync = ch->db.in_sync;
    const uint32_t groups = ch->db.groups, acq = ch->db.sync_acquisitions;
    memset(&ch->db, 0, sizeof(ch->db));
    ch->db.in_sync = in_sync; ch->db.groups = groups; ch->db.sync_acquisitions = acq;
}

/* RDS_Group_Sync::Process / FindingSync / ReadingGroup, rds_group_sync.cpp:29-127, bit by bit */
long fmo_rds_chain_process(fmo_rds_chain* ch, const uint8_t* x, long n, fmo_rds_group* out, long cap) {
    long n_groups = 0;
    for (long i = 0; i < 8 * n; i++) {
        const uint32_t bit = (x[i / 8] >> (7 - (i % 8))) & 1u;                       /* bit_reader_t: MSB first */
        ch->block_buf = ((ch->block_buf << 1) | bit) & 0x3FFFFFFu;                    /* PushBit */
        if (ch->finding_sync) {
            if (rds_crc10(ch->block_buf ^ kRdsOffsets[0]) != 0) continue;
            ch->finding_sync = 0;
            ch->block_bits = 0;
            ch->db.sync_acquisitions++;
            rds_push_block(ch, ch->block_buf);
            continue;
        }
        if (++ch->block_bits != 26) continue;
        ch->block_bits = 0;
        rds_push_block(ch, ch->block_buf);
        if (ch->curr_block < 4) continue;
        if (n_groups < cap) out[n_groups] = ch->group;                               /* obs_on_group.Notify */
        n_groups++;
        ch->db.groups++;
        rds_process_group(ch);
        const int errors = ch->block_errors;
        ch->curr_block = 0;
        ch->block_errors = 0;
        if (errors == 0) { ch->groups_desync = 0; continue; }
        if (++ch->groups_desync >= 3) { ch->finding_sync = 1; ch->groups_desync = 0; }
    }
    ch->db.in_sync = ch->finding_sync ? 0 : 1;
    return n_groups;
}
