"""Times the loudness meter's call (fmd_meter_*, k_meter and with FMD_METER_TRUE_PEAK k_meter_tp) beside an audio mixer call of the same
shape in the same process: 4096 stations x 2048 frames (one 64 ms demodulator block at 32 kHz) by default, the mixer as 4096 one-station
buses.  `--features` is a comma-separated list of feature sets (0 none, 1 true peak, 2 range, 3 both): one meter of each is created and all
of them and the mixer are timed in alternating rounds with device events around `--iters` calls each; the median, minimum and maximum
over the rounds are printed, with the bytes each call reads and the frames per second the meter sustains, and for a meter with true
peak the difference to the features-0 (or features-2) meter of the same run, which is k_meter_tp alone.  Needs a GPU.  `--out FILE` also
writes the report to a file (profiles/meter/)."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import fmradio_loader  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stations", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--fs", type=int, default=32000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--features", type=str, default="0", help="comma-separated feature sets to time, e.g. 0,1,2,3")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    C, n = a.stations, a.frames
    x = 0.3 * torch.randn(C, n, 2, device="cuda")
    feats = [int(f) for f in a.features.split(",")]
    meters = {f: (pkg.LoudnessMeter(C, a.fs, max_input_frames=n, features=f) if f else pkg.LoudnessMeter(C, a.fs, max_input_frames=n)) for f in feats}
    meter = meters[feats[0]]
    mixer = pkg.AudioMixer(C, [[c] for c in range(C)])
    out = torch.empty(C, n, 2, device="cuda")
    name = {f: "meter" if f == 0 else f"meter{f}" for f in feats}
    calls = {name[f]: (lambda m=meters[f]: m.process(x)) for f in feats}
    calls["mixer"] = lambda: mixer.process(x, out=out)
    for f in calls.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, f in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                f()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) / a.iters * 1e3)
    lines = [f"{C} stations x {n} frames at {a.fs} Hz, {a.rounds} alternating rounds of {a.iters} calls, device events (us per call)"]
    for k, v in times.items():
        nbytes = C * n * 8 * (2 if k == "mixer" else 1)
        med = statistics.median(v)
        lines.append(f"{k:6s} median {med:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   {nbytes / 1e6:6.1f} MB per call, {nbytes / med / 1e6:5.2f} TB/s")
    for f in feats:
        if f & 1 and (f & 2) in feats:                                       # the same meter without true peak was timed too
            tp = statistics.median(times[name[f]]) - statistics.median(times[name[f & 2]])
            lines.append(f"k_meter_tp alone ({name[f]} - {name[f & 2]}): {tp:8.1f} us, {C * n * 8 / 1e6:6.1f} MB read, {C * n * 8 / tp / 1e6:5.2f} TB/s")
    med = statistics.median(times[name[feats[0]]])
    lines.append(f"meter: {C * n / med:.0f} frames per us = {C * n / med * 1e6 / a.fs / C:.0f} x real time for each of {C} stations; "
                 f"{med / n * 1e3:.1f} ns per frame step of a wavefront")
    st = meter.status()
    lines.append(f"check: station 0 has {int(st[0]['frames'])} frames, {int(st[0]['subblocks'])} sub-blocks, momentary "
                 f"{pkg.meter_momentary(st[0]):.2f} LUFS")
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
