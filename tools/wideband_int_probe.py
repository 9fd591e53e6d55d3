"""Integer-capture channeliser timings: the same capture as cf32, u8, s8 and s16, and as "convert, then cf32" (a device-side integer -> cf32
conversion, one elementwise pass, then fmd_chan_process_cf32_dev: what a caller had to do before the integer entry points), 64 ms blocks
(16384 outputs per station), at three configurations:
    40 stations at 10 MSa/s (k_channelize16_mfma), 100 stations at 20.48 MSa/s (k_channelize_band_mfma), 12 stations at 2.4 MSa/s
    (k_channelize, the RTL-SDR rate).
Per configuration the variants are timed in turn, `--reps` rounds with the order rotated from round to round, each round `--steps` back-to-back
blocks between device events after a warm-up; probe.json keeps every round's ms per block, the median and the spread.  Before timing, each
integer form's output is checked against the cf32 form's on its conversion (torch.equal) at the timed size.

    python tools/wideband_int_probe.py [--out DIR]                                          (wall clock: DIR/probe.json)
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/wideband_int_probe.py --reps 2 --out DIR     (kernel times)

The capture is bench.synth_wideband_device's (8 stations' worth of FM within +-100), quantised: u8 = 127 + x, s8 = x, s16 = 256 x."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests", ROOT / "oracle"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

# (key, fs_in, stations, raster)
CONFIGS = [("10MSa_40", 10e6, 40, 250e3), ("20.48MSa_100", 20.48e6, 100, 200e3), ("2.4MSa_12", 2.4e6, 12, 200e3)]
VARIANTS = ["cf32", "u8", "s8", "s16", "u8+convert", "s8+convert", "s16+convert"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wideband_int"))
    args = ap.parse_args()
    import torch

    import fmradio_loader
    from bench import synth_wideband_device
    pkg = fmradio_loader.load()
    dev = torch.device("cuda:0")
    fs, bs, n_res = 256_000, 16384, 4
    res = {}
    for key, fs_in, C, raster in CONFIGS:
        n_in = bs * int(fs_in) // fs
        centers = (np.arange(C) - (C - 1) / 2.0) * raster
        x = synth_wideband_device(torch, centers[:8], n_res * n_in, fs_in, 99, dev).view(n_res, n_in, 2)
        caps = {"u8": torch.clamp(torch.round(x + 127.0), 0, 255).to(torch.uint8),
                "s8": torch.clamp(torch.round(x), -128, 127).to(torch.int8),
                "s16": torch.clamp(torch.round(x * 256.0), -32768, 32767).to(torch.int16)}
        caps["cf32"] = caps["u8"].to(torch.float32) - 127.0
        del x
        ch = pkg.Channelizer(fs_in, centers, float(fs), max_input_samples=n_in)
        outs = [torch.empty((C, bs, 2), dtype=torch.float32, device=dev) for _ in range(2)]
        conv = torch.empty((n_in, 2), dtype=torch.float32, device=dev)

        def convert(fmt, i):
            if fmt == "u8":
                return torch.sub(caps["u8"][i], 127.0, out=conv)      # one pass: (float)v - 127
            return conv.copy_(caps[fmt][i])

        def step(v, i):
            fmt = v.split("+")[0]
            wide = convert(fmt, i % n_res) if v.endswith("+convert") else caps[fmt][i % n_res]
            ch.process(wide, out=outs[i & 1])

        # the contract at the timed size: integer form == cf32 form on the conversion, bit for bit
        checks = {}
        for fmt in ("u8", "s8", "s16"):
            ch.reset()
            a = ch.process(caps[fmt][0]).clone()
            ch.reset()
            b = ch.process(convert(fmt, 0)).clone()
            checks[fmt] = bool(torch.equal(a, b))
        ch.reset()
        for v in VARIANTS:
            for i in range(args.warmup):
                step(v, i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        rounds = {v: [] for v in VARIANTS}
        for r in range(args.reps):
            order = VARIANTS[r % len(VARIANTS):] + VARIANTS[:r % len(VARIANTS)]
            for v in order:
                e0.record()
                for i in range(args.steps):
                    step(v, i)
                e1.record()
                torch.cuda.synchronize()
                rounds[v].append(e0.elapsed_time(e1) / args.steps)
        med = {v: float(np.median(rounds[v])) for v in VARIANTS}
        res[key] = {
            "fs_in": fs_in, "stations": C, "taps_per_phase": ch.taps_per_phase, "L": ch.interp, "M": ch.decim,
            "bit_identical_to_cf32_on_conversion": checks,
            "ms_per_block_median": med,
            "ms_per_block_min": {v: float(np.min(rounds[v])) for v in VARIANTS},
            "ms_per_block_max": {v: float(np.max(rounds[v])) for v in VARIANTS},
            "ms_per_block_rounds": rounds,
            "vs_cf32": {v: med[v] / med["cf32"] for v in ("u8", "s8", "s16")},
            "vs_convert_then_cf32": {f: med[f] / med[f + "+convert"] for f in ("u8", "s8", "s16")},
        }
        print(key, json.dumps({k: res[key][k] for k in ("bit_identical_to_cf32_on_conversion", "ms_per_block_median", "vs_cf32", "vs_convert_then_cf32")}),
              flush=True)
        ch.close()
        del caps, outs, conv
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "probe.json").write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
