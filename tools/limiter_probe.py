"""Times the look-ahead peak limiter's call (fmd_limiter_*, k_limiter) at its two shapes: 4096 stations x 2048 frames, the 64 ms
demodulator block at 32 kHz, and 8 buses x 4800 frames, 100 ms of a 48 kHz mixer.  Each shape is timed in `--rounds` rounds of `--iters`
back-to-back calls between device events, after warm-up; the median, minimum and maximum over the rounds are printed beside the time
the 16 bytes a frame (8 read, 8 written) take at the copy roof tools/hbm_roof_probe.hip measured, 6.33 TB/s.  The first shape is timed
on a quiet programme (nothing over the ceiling) and on a loud one (a quarter of the stations 12 dB up): the arithmetic is the same, the
counts differ.  Needs a GPU.  `--out FILE` also writes the report to a file (profiles/limiter/)."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import fmradio_loader  # noqa: E402

ROOF_TBS = 6.33


def programme(C, n, fs, loud):
    """a noise-like stereo programme at -20 dB a rail; with `loud` every fourth station is 12 dB up and crosses the ceiling"""
    n1 = torch.randn(C, n, device="cuda")
    x = torch.stack([0.1 * n1, 0.1 * (0.6 * n1 + 0.8 * torch.randn(C, n, device="cuda"))], dim=2).contiguous()
    if loud:
        x[1::4] *= 4.0
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    shapes = [("stations, quiet", 4096, 2048, 32000, False), ("stations, loud", 4096, 2048, 32000, True), ("buses, loud", 8, 4800, 48000, True)]
    calls, lims = {}, {}
    for name, C, n, fs, loud in shapes:
        lim = pkg.Limiter(C, fs, max_input_frames=n)
        x = programme(C, n, fs, loud)
        out = torch.zeros_like(x)
        gr = torch.ones(C, device="cuda")
        lims[name] = (lim, C, n, fs)
        calls[name] = (lambda lim=lim, x=x, out=out, gr=gr: lim.process(x, out=out, gr=gr))
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
    lines = [f"default limiter (1.5 ms, 500 ms, -1 dBFS), {a.rounds} alternating rounds of {a.iters} calls, device events (us per call); "
             f"roof: 16 bytes a frame at {ROOF_TBS} TB/s"]
    for k, v in times.items():
        lim, C, n, fs = lims[k]
        med, roof = statistics.median(v), C * n * 16 / ROOF_TBS / 1e6
        st = lim.status()
        lines.append(f"{k:16s} {C:5d} x {n} frames at {fs} Hz, D = {lim.latency}: median {med:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   roof {roof:6.2f} us, {med / roof:5.1f} x the roof, "
                     f"{C * n * 16 / med / 1e6:5.2f} TB/s;  {med / (n / fs * 1e6) * 100:.3f} % of the {n / fs * 1e3:.0f} ms the frames last;  "
                     f"limited {int(st['limited'].sum())} of {int(st['frames'].sum())} frames, smallest gain {float(st['min_gain'].min()):.3f}")
    lines.append("configuration: one workgroup of 256 threads a station, tiles of 1024 frames, five positions a thread in the scans; no other tile length, "
                 "workgroup size or station grouping was built or measured")
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
