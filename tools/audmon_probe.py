"""Times the audio fault monitor's call (fmd_audmon_*, k_audmon) beside fmd_meter_process_f32_dev, the loudness meter, over the same
bytes in the same process: 4096 stations x 2048 frames at 32 kHz by default (one 64 ms demodulator block), and the same with calls
`--long` (4) blocks long, which separates a call's fixed part from its rows.  The calls are timed in alternating rounds with device
events around `--iters` back-to-back calls each; the median, minimum and maximum over the rounds are printed with the bytes each call
moves: the samples read plus, for the monitor, the state read and written per station and call (the open interval's 1.5 KB of partials
both ways, the 840-byte record and the 80-byte thresholds).  The meter's bytes are the samples alone.  Needs a GPU.  `--out FILE` also
writes the report to a file (profiles/audmon/)."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import fmradio_loader  # noqa: E402

STATE_BYTES = 2 * 3 * 64 * 8 + 840 + 80 + 16     # per station and call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stations", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--long", type=int, default=4)
    ap.add_argument("--fs", type=int, default=32000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--roof", type=float, default=7.07)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    C, n, nl = a.stations, a.frames, a.frames * a.long
    # stereo programme at -20 dB a rail with a correlation of 0.6; every fourth station is mono, every eighth silent
    n1 = torch.randn(C, nl, device="cuda")
    x = torch.stack([0.1 * n1, 0.1 * (0.6 * n1 + 0.8 * torch.randn(C, nl, device="cuda"))], dim=2).contiguous()
    del n1
    x[3::4, :, 1] = x[3::4, :, 0]
    x[7::8] = 0.0
    xs = x[:, :n].contiguous()
    mon = {k: pkg.AudioMonitor(C, a.fs, max_input_frames=nl) for k in ("audmon", "audmon_long")}
    met = {k: pkg.LoudnessMeter(C, a.fs, max_input_frames=nl) for k in ("meter", "meter_long")}
    flags = torch.zeros(C, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(C, dtype=torch.uint8, device="cuda")
    calls = {"audmon": lambda: mon["audmon"].process(xs, flags=flags, ok=ok), "meter": lambda: met["meter"].process(xs),
             "audmon_long": lambda: mon["audmon_long"].process(x, flags=flags, ok=ok), "meter_long": lambda: met["meter_long"].process(x)}
    frames = {"audmon": n, "meter": n, "audmon_long": nl, "meter_long": nl}
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
    lines = [f"{C} stations x {n} frames (and x {nl}: '_long') at {a.fs} Hz, {a.rounds} alternating rounds of {a.iters} calls, device events (us per call)"]
    med = {}
    for k, v in times.items():
        nbytes = C * frames[k] * 8 + (C * STATE_BYTES if k.startswith("audmon") else 0)
        med[k] = statistics.median(v)
        lines.append(f"{k:11s} median {med[k]:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   {nbytes / 1e6:6.1f} MB per call, {nbytes / med[k] / 1e6:5.2f} TB/s"
                     f" = {100.0 * nbytes / med[k] / 1e6 / a.roof:4.1f} % of the {a.roof} TB/s read roof")
    for k in ("audmon", "meter"):
        per_block = (med[k + "_long"] - med[k]) / (a.long - 1)
        fixed = med[k] - per_block
        lines.append(f"{k}: {per_block:.1f} us per further block of {n} frames, so {fixed:.1f} us = {100.0 * fixed / med[k]:.0f} % of a one-block call are fixed")
    lines.append(f"audmon: {C * n / med['audmon']:.0f} frames per us = {C * n / med['audmon'] * 1e6 / a.fs / C:.0f} x real time for each of {C} stations; "
                 f"{med['audmon'] * 1e3 / (n / 256):.1f} ns per 256-frame row of a station's wavefront; {med['meter'] / med['audmon']:.2f} x the meter's speed "
                 f"({med['meter_long'] / med['audmon_long']:.2f} x in the long calls)")
    st = mon["audmon"].status()
    lines.append(f"check: station 0 has {int(st[0]['frames'])} frames, {int(st[0]['intervals'])} intervals, correlation {pkg.audmon_correlation(st[0], a.fs, 10):.3f}, "
                 f"level {pkg.audmon_level_db(st[0], a.fs, 2, 10):.2f} dB; flags of stations 0, 3, 7: {[int(st[c]['flags']) for c in (0, 3, 7)]}; "
                 f"ok {int(ok.sum())} of {C}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
