/* rds_chain.h — TEST INFRASTRUCTURE: C restatement of the reference's RDS decoding chain (liboracle_rds.so, oracle/rds_chain.mk).
 * A file of its own beside fm_oracle.{c,h}: the demodulator's oracle stays as it is. */
#ifndef RDS_CHAIN_H
#define RDS_CHAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* RDS decoding chain — reference src/rds_decoder/rds_decoding_chain.h: RDS_Group_Sync (rds_group_sync.cpp) -> RDS_Decoder
 * (rds_decoder.cpp) -> RDS_Database_Decoder_Handler (rds_database_decoder_handler.cpp) -> RDS_Database (rds_database.h).
 * Records laid out as include/fmdemod.h's fmd_rds_block / fmd_rds_group / fmd_rds_db (tests compare them byte for byte). */
typedef struct { uint16_t data; uint8_t block_type; uint8_t is_valid; } fmo_rds_block;   /* block_type: 0 A, 1 B, 2 C, 3 C', 4 D */
typedef struct { fmo_rds_block blocks[4]; } fmo_rds_group;
typedef struct {
    char     service_name[8], programme_type_name[8], radio_text[64];
    uint16_t PI_code;
    uint8_t  programme_type;
    uint8_t  is_stereo, is_music, is_artificial_head, is_compressed, is_dynamic_program_type;
    struct { int32_t day, month, year; uint8_t hour, minute, pad_[2]; } datetime;
    int8_t   local_time_offset;
    uint8_t  traffic_announcement;
    uint8_t  pad_[2];
    int32_t  in_sync;                 /* beyond the reference: READ_BLOCK state, groups delivered, locks onto block A */
    uint32_t groups, sync_acquisitions;
} fmo_rds_db;
typedef struct {
    uint32_t block_buf;               /* rd_block_buf */
    int block_bits, curr_block, block_errors, groups_desync, finding_sync;
    fmo_rds_group group;
    uint8_t ab_radio_text, ab_programme_type_name;
    fmo_rds_db db;
} fmo_rds_chain;
size_t fmo_rds_chain_size(void);
void fmo_rds_chain_init(fmo_rds_chain* ch);
void fmo_rds_chain_get_db(const fmo_rds_chain* ch, fmo_rds_db* db);
/* RDS_Database::Reset(): the database only (sync state, A/B memories and the status fields stay) */
void fmo_rds_chain_reset_db(fmo_rds_chain* ch);
/* RDS_Decoding_Chain::Process(x[0..n)): returns the number of groups delivered; the first `cap` of them go to out */
long fmo_rds_chain_process(fmo_rds_chain* ch, const uint8_t* x, long n, fmo_rds_group* out, long cap);

#ifdef __cplusplus
}
#endif
#endif
