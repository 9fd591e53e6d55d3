"""IQ corrector timings: ms per 64 ms block of a 20.48 MSa/s capture (k_iqcorr + k_iqcorr_fold) for s16 and cf32 input, writing the
corrected cf32 block and measuring only.  Each configuration: a warm-up, then `--reps` rounds of `--steps` back-to-back blocks (two
buffers alternating) between device events; probe.json keeps every round's ms per block, the median and the fraction of the bytes moved
(input read once, cf32 output written once) over the copy roof of 6.33 TB/s (tools/hbm_roof_probe.hip).  Before timing, the s16 call's
moments are checked against exact integer sums and its output against the cf32 call's on the converted samples (bit for bit).

    python tools/iqcorr_probe.py [--out DIR]                                                             (wall clock: DIR/probe.json)
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/iqcorr_probe.py --reps 2 --out DIR     (kernel times)
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

FS_IN = 20.48e6
HBM_BYTES_PER_S = 6.33e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "iqcorr"))
    args = ap.parse_args()
    import torch

    import fmradio_loader
    pkg = fmradio_loader.load()
    dev = torch.device("cuda:0")
    n_in = int(round(FS_IN * 0.064))
    g = torch.Generator(device=dev).manual_seed(5)
    s16 = torch.randint(-32768, 32768, (2, n_in, 2), dtype=torch.int16, device=dev, generator=g)
    caps = {"s16": s16, "cf32": s16.to(torch.float32)}
    corr = (0.37, -1.21, 0.031, -0.047)

    # correctness at the timed size
    a, b = pkg.IqCorrector(max_input_samples=n_in), pkg.IqCorrector(max_input_samples=n_in)
    a.correction = corr
    b.correction = corr
    ya, yb = a.process(caps["s16"][0]), b.process(caps["cf32"][0])
    v = s16[0].cpu().numpy().astype(np.int64)
    exact = [float(w) for w in (n_in, v[:, 0].sum(), v[:, 1].sum(), (v[:, 0] ** 2).sum(), (v[:, 1] ** 2).sum(), (v[:, 0] * v[:, 1]).sum())]
    checks = {"s16_moments_exact": list(a.moments()) == exact, "cf32_moments_exact": list(b.moments()) == exact,
              "s16_output_equals_cf32_output": bool(torch.equal(ya.view(torch.int32), yb.view(torch.int32)))}
    print(json.dumps(checks), flush=True)
    assert all(checks.values()), checks
    a.close(); b.close()

    res = {"checks": checks}
    for fmt in ("s16", "cf32"):
        for write in (True, False):
            key = f"{fmt}_{'process' if write else 'measure'}"
            co = pkg.IqCorrector(max_input_samples=n_in)
            co.correction = corr
            outs = [torch.empty((n_in, 2), dtype=torch.float32, device=dev) for _ in range(2)] if write else [False, False]
            for i in range(args.warmup):
                co.process(caps[fmt][i & 1], out=outs[i & 1])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            rounds = []
            for _ in range(args.reps):
                co.reset_moments()
                e0.record()
                for i in range(args.steps):
                    co.process(caps[fmt][i & 1], out=outs[i & 1])
                e1.record()
                torch.cuda.synchronize()
                rounds.append(e0.elapsed_time(e1) / args.steps)
            med = float(np.median(rounds))
            nbytes = n_in * ((8 if fmt == "cf32" else 4) + (8 if write else 0))
            res[key] = {"fs_in": FS_IN, "format": fmt, "writes_output": write, "samples_per_block": n_in, "bytes_moved": nbytes,
                        "ms_per_block_median": med, "ms_per_block_min": float(np.min(rounds)), "ms_per_block_max": float(np.max(rounds)),
                        "ms_per_block_rounds": rounds, "x_real_time": 64.0 / med,
                        "byte_bound_ms": nbytes / HBM_BYTES_PER_S * 1e3, "fraction_of_copy_roof": nbytes / HBM_BYTES_PER_S * 1e3 / med}
            print(key, json.dumps({k: res[key][k] for k in ("ms_per_block_median", "byte_bound_ms", "fraction_of_copy_roof")}), flush=True)
            co.close()
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "probe.json").write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
