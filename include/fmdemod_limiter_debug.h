/* fmdemod_limiter_debug.h — the look-ahead peak limiter's test hook (include/fmdemod.h, "Look-ahead peak limiter").
 *
 * NOT part of the drop-in boundary (include/fmdemod.h), and a header of its own beside fmdemod_debug.h, whose set of hooks
 * tests/test_capi_cpu.py holds fixed.  A limiter's output never depends on this call.
 */
#ifndef FMDEMOD_LIMITER_DEBUG_H
#define FMDEMOD_LIMITER_DEBUG_H

#include "fmdemod.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The frame count of station `channel`'s status record, so that tests reach counts past 2^32 without running for days.  Waits for the
 * limiter's earlier work.  FMD_ERR_ARG for a channel outside [0, C). */
int fmd_limiter_debug_set_frames(fmd_limiter l, int channel, unsigned long long frames);

#ifdef __cplusplus
}
#endif
#endif
