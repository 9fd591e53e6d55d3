"""Whole-band channeliser timings: 100 stations on the 200 kHz raster out of one 20.48 MSa/s capture, and out of one 32.768 MSa/s capture,
64 ms blocks (16384 outputs per station) -> k_channelize_band_mfma; then channeliser + tolerance-mode demodulator end to end.

    rocprofv3 --kernel-trace --stats -d profiles/wideband_band -o trace -- python tools/wideband_band_probe.py

gives the kernel times; the script itself prints (and writes to profiles/wideband_band/probe.json) the wall-clock figures per block,
measured with device events around back-to-back blocks.  The capture is bench.synth_wideband_device's."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests", ROOT / "oracle"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def main():
    import torch

    import fmradio_loader
    from bench import synth_wideband_device
    pkg = fmradio_loader.load()
    dev = torch.device("cuda:0")
    fs, bs, C, steps, warm = 256_000, 16384, 100, 40, 8
    centers = (np.arange(C) - (C - 1) / 2.0) * 200e3
    res = {}
    for fs_in in (20.48e6, 32.768e6):
        n_in = bs * int(fs_in) // fs
        n_res = 4
        wide = synth_wideband_device(torch, centers[:8], n_res * n_in, fs_in, 99, dev).view(n_res, n_in, 2)   # 8 stations' worth of signal
        ch = pkg.Channelizer(fs_in, centers, float(fs), max_input_samples=n_in)
        outs = [torch.empty((C, bs, 2), dtype=torch.float32, device=dev) for _ in range(2)]
        for i in range(warm):
            ch.process(wide[i % n_res], out=outs[i & 1])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(steps):
            ch.process(wide[i % n_res], out=outs[i & 1])
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        dm = pkg.BatchDemod(C, bs, fs, device=0, fast_math=True)
        for i in range(warm):
            dm.process(ch.process(wide[i % n_res], out=outs[i & 1]))
        torch.cuda.synchronize()
        e0.record()
        for i in range(steps):
            dm.process(ch.process(wide[i % n_res], out=outs[i & 1]))
        e1.record()
        torch.cuda.synchronize()
        ms_e2e = e0.elapsed_time(e1) / steps
        key = f"{fs_in / 1e6:g}MSa"
        res[key] = {"stations": C, "taps_per_phase": ch.taps_per_phase, "L": ch.interp, "M": ch.decim,
                    "channeliser_ms_per_block": ms, "channeliser_x_realtime": 64.0 / ms,
                    "with_demodulator_ms_per_block": ms_e2e, "with_demodulator_x_realtime": 64.0 / ms_e2e}
        print(key, json.dumps(res[key]), flush=True)
        dm.close(); ch.close()
        del wide, outs
    out = ROOT / "profiles" / "wideband_band"
    out.mkdir(parents=True, exist_ok=True)
    (out / "probe.json").write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
