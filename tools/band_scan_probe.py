"""Band scanner timings: ms per 64 ms block of capture (k_scan_frames + k_scan_accumulate, and the carry-over) at 10, 20.48 and
32.768 MSa/s, cf32 and u8, at the default N (fmd_scan_default_nfft) and at N = 16384.  Each configuration: a warm-up, then `--reps`
rounds of `--steps` back-to-back blocks between device events; probe.json keeps every round's ms per block, the median, the real-time
factor and the fraction of the byte bound (input read twice for the 50 % overlap, the frame powers written and read back once, at
6.3 TB/s).  Before timing, the u8 call's PSD is checked against the cf32 call's on its conversion (bit for bit).

    python tools/band_scan_probe.py [--out DIR]                                                           (wall clock: DIR/probe.json)
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/band_scan_probe.py --reps 2 --out DIR     (kernel times)
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests", ROOT / "oracle"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

RATES = [10e6, 20.48e6, 32.768e6]
HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "band_scan"))
    args = ap.parse_args()
    import torch

    import fmradio_loader
    pkg = fmradio_loader.load()
    dev = torch.device("cuda:0")
    res = {}
    g = torch.Generator(device=dev).manual_seed(5)
    for fs_in in RATES:
        n_in = int(round(fs_in * 0.064))
        u8 = torch.randint(0, 256, (2, n_in, 2), dtype=torch.uint8, device=dev, generator=g)
        caps = {"u8": u8, "cf32": u8.to(torch.float32) - 127.0}
        for nfft in (pkg.scan_default_nfft(fs_in), 16384):
            for fmt in ("cf32", "u8"):
                key = f"{fs_in / 1e6:g}MSa_N{nfft}_{fmt}"
                sc = pkg.BandScanner(fs_in, nfft=nfft, max_input_samples=n_in)
                check = None
                if fmt == "u8":
                    sc.process(caps["u8"][0])
                    a = sc.psd()[1]
                    ref = pkg.BandScanner(fs_in, nfft=nfft, max_input_samples=n_in)
                    ref.process(caps["cf32"][0])
                    check = bool(np.array_equal(a.view(np.uint64), ref.psd()[1].view(np.uint64)))
                    ref.close()
                    sc.reset()
                for i in range(args.warmup):
                    sc.process(caps[fmt][i & 1])
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                rounds = []
                for _ in range(args.reps):
                    e0.record()
                    for i in range(args.steps):
                        sc.process(caps[fmt][i & 1])
                    e1.record()
                    torch.cuda.synchronize()
                    rounds.append(e0.elapsed_time(e1) / args.steps)
                med = float(np.median(rounds))
                frames = n_in // (nfft // 2)
                in_bytes = n_in * (8 if fmt == "cf32" else 2)
                bound_bytes = 2 * in_bytes + 2 * 4 * frames * nfft
                res[key] = {
                    "fs_in": fs_in, "nfft": nfft, "format": fmt, "samples_per_block": n_in, "frames_per_block": frames,
                    "ms_per_block_median": med, "ms_per_block_min": float(np.min(rounds)), "ms_per_block_max": float(np.max(rounds)),
                    "ms_per_block_rounds": rounds, "x_real_time": 64.0 / med,
                    "byte_bound_ms": bound_bytes / HBM_BYTES_PER_S * 1e3, "fraction_of_byte_bound": bound_bytes / HBM_BYTES_PER_S * 1e3 / med,
                    "u8_bit_identical_to_cf32_on_conversion": check,
                }
                print(key, json.dumps({k: res[key][k] for k in ("ms_per_block_median", "x_real_time", "fraction_of_byte_bound",
                                                                   "u8_bit_identical_to_cf32_on_conversion")}), flush=True)
                sc.close()
        del caps, u8
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "probe.json").write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
