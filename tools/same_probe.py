"""Times the EAS SAME decoder's call (fmd_same_*, k_same) beside fmd_tonedet_process_f32_dev with two slots in use, over the same bytes in
the same process: 4096 stations x 2048 frames at 32 kHz by default (one 64 ms demodulator block).  The calls are timed in alternating
rounds with device events around `--iters` back-to-back calls each; the median, minimum and maximum over the rounds are printed with what
each call does per frame: both read 8 bytes, add 4 fp64 multiply-adds to their sums (the detector a fifth for the mid signal's power) and
gather two 16-byte table entries.  Every fourth station carries the first frames of a SAME burst, its preamble, so that the framer synchronises in every call.  Needs a GPU.  `--out FILE`
also writes the report to a file (profiles/same/)."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fmradio_loader  # noqa: E402

TEXT = b"ZCZC-WXR-TOR-039173-039051-039035+0030-1051700-KCLE/NWS-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stations", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--fs", type=int, default=32000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    C, n = a.stations, a.frames
    # a noise-like stereo programme at -20 dB a rail; every fourth station carries the start of a SAME burst instead
    n1 = torch.randn(C, n, device="cuda")
    x = torch.stack([0.1 * n1, 0.1 * (0.6 * n1 + 0.8 * torch.randn(C, n, device="cuda"))], dim=2).contiguous()
    del n1
    burst = pkg.same_encode(TEXT, a.fs, repeats=1, gap_frames=0)
    reps = -(-n // burst.shape[0])
    x[3::4] = torch.from_numpy(np.tile(burst, (reps, 1))[:n]).cuda()[None]
    dec = pkg.SameDecoder(C, a.fs, max_input_frames=n)
    det = pkg.ToneDetector(C, a.fs, max_input_frames=n)
    det.set_params(freq_hz=(853, 960, 0, 0, 0, 0, 0, 0), raise_intervals=2)
    flags = torch.zeros(C, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(C, dtype=torch.uint8, device="cuda")
    fs_ = torch.zeros(C, dtype=torch.uint8, device="cuda")
    calls = {"same": lambda: dec.process(x, flags=fs_, ok=ok), "tonedet_2": lambda: det.process(x, flags=flags, ok=ok)}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) / a.iters * 1e3)
    lines = [f"{C} stations x {n} frames at {a.fs} Hz, {a.rounds} alternating rounds of {a.iters} calls, device events (us per call)"]
    med = {k: statistics.median(v) for k, v in times.items()}
    fma = {"same": 4, "tonedet_2": 5}
    for k, v in times.items():
        lines.append(f"{k:10s} median {med[k]:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   {C * n * 8 / med[k] / 1e6:5.2f} TB/s of samples; {fma[k]} fp64 fma and 2 gathers a "
                     f"frame: {C * n * fma[k] / med[k] / 1e6:5.2f} Tfma/s, {C * n * 2 / med[k] / 1e3:6.1f} G gathers/s")
    ticks = n * 12500 / (3 * a.fs)
    lines.append(f"same: {med['same'] / med['tonedet_2']:.2f} x the tone detector's time with two slots; {ticks:.0f} ticks a station and call walked by the clock and the "
                 f"framer; {C * n / med['same'] * 1e6 / a.fs / C:.0f} x real time for each of {C} stations")
    st = dec.status()
    lines.append(f"check: station 3 has {int(st[3]['frames'])} frames, {int(st[3]['ticks'])} ticks, {int(st[3]['bits'])} bits, {int(st[3]['syncs'])} syncs, "
                 f"{int(st[3]['accepted'])} accepted; station 0 (noise) {int(st[0]['syncs'])} syncs, {int(st[0]['accepted'])} accepted; "
                 f"alert open on {int(((fs_ & 2) != 0).sum())} of {C}, accepted over all noise stations {int(st['accepted'][np.arange(C) % 4 != 3].sum())}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
