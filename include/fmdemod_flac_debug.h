/* fmdemod_flac_debug.h — the FLAC audio encoder's test hook (include/fmdemod.h, "FLAC audio encoder").
 *
 * NOT part of the drop-in boundary (include/fmdemod.h), and a header of its own beside fmdemod_debug.h, whose set of hooks
 * tests/test_capi_cpu.py holds fixed.  An encoder's output never depends on this call unless a test makes it.
 */
#ifndef FMDEMOD_FLAC_DEBUG_H
#define FMDEMOD_FLAC_DEBUG_H

#include "fmdemod.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The next FLAC frame's number of station `channel` (below 2^31), so that tests reach the lengths of the coded number and its wrap
 * without running for days.  Waits for the encoder's earlier work.  FMD_ERR_ARG for a channel outside [0, C) or a value of 2^31 and
 * above. */
int fmd_debug_flac_set_frame_number(fmd_flac e, int channel, unsigned value);

#ifdef __cplusplus
}
#endif
#endif
