#!/usr/bin/env python3
"""k_rds_decode alone (the standalone decoder, fmd_rdsdec_process_dev): every channel gets 16 new bytes a launch — the most one 64 ms block
brings (one Manchester chunk, 128 bit steps) — from a stream that is either LOCKED (the synthesiser's clean 0A / 2A / 4A mix: group sync
in READ_BLOCK, a group decoded every 104 bits) or HUNTING (random bytes: FINDING_SYNC, a false lock now and then).  Run under
`rocprofv3 --kernel-trace --stats` for the kernel's time (tools/rds_decode_evidence.sh); prints the host's view as one JSON line.

    python tools/rds_decode_probe.py --channels 4096 --state locked --launches 200
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "oracle")]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--state", choices=["locked", "hunting"], default="locked")
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    import torch
    import fmradio_loader
    import rds_synth
    pkg = fmradio_loader.load()
    C, L = args.channels, args.launches
    n = 16 * L
    if args.state == "hunting":
        data = np.random.default_rng(5).integers(0, 256, (C, n), dtype=np.uint8)
    else:   # 64 distinct stations (PI / PS), each offset by a channel-dependent number of bits so that the lanes of a wavefront are at different places of a group
        base = []
        for s in range(64):
            base.append(rds_synth.mixed_bits(8 * n + 104, 0x4000 + s, f"PROBE{s:03d}", f"probe station {s:03d}".ljust(64)))
        data = np.stack([rds_synth.pack_bits(base[c % 64][c % 104:c % 104 + 8 * n]) for c in range(C)])
    d = torch.from_numpy(np.ascontiguousarray(data.reshape(C, L, 16).transpose(1, 0, 2))).cuda()     # [launch][C][16]
    counts = torch.full((C,), 16, dtype=torch.int32, device="cuda")
    dec = pkg.RDSDecoder(C)
    for k in range(4):                     # warm-up (and the first lock in the locked case)
        dec.process_tensor(d[k], counts)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for k in range(4, L):
        dec.process_tensor(d[k], counts)
    torch.cuda.synchronize()
    el = time.perf_counter() - t
    db = dec.db()
    print(json.dumps({"channels": C, "state": args.state, "launches_timed": L - 4, "host_us_per_launch": el / (L - 4) * 1e6,
                      "in_sync_frac": float(db["in_sync"].mean()), "groups_per_channel": float(db["groups"].mean()),
                      "locks_per_channel": float(db["sync_acquisitions"].mean())}))
    dec.close()


if __name__ == "__main__":
    main()
