"""Times the modulation monitor's call (fmd_modmon_*, k_modmon) for cf32 and u8 station baseband beside a one-pass reader of a capture
of the same total size in the same process, fmd_iqcorr_process_cf32_dev with d_out = NULL: 4096 stations x 16384 samples at 256 kSa/s by
default (one 64 ms demodulator block).  The three are timed in alternating rounds with device events around `--iters` back-to-back
calls each; the median, minimum and maximum over the rounds are printed with the bytes each call reads.  Needs a GPU.  `--out FILE`
also writes the report to a file (profiles/modmon/)."""
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
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--fs", type=int, default=256000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    C, n = a.stations, a.samples
    # unit carriers frequency-modulated by noise, about 50 kHz peak: every range of atan2f is visited
    f = torch.randn(C, n, device="cuda") * (15000.0 / a.fs * 6.283185307179586)
    ph = torch.cumsum(f, dim=1)
    x = torch.stack([torch.cos(ph), torch.sin(ph)], dim=2).contiguous()
    del f, ph
    b = torch.clamp(torch.round(x * 120.0 + 127.0), 0, 255).to(torch.uint8).contiguous()
    mon_f = pkg.ModulationMonitor(C, a.fs, max_input_samples=n)
    mon_b = pkg.ModulationMonitor(C, a.fs, max_input_samples=n)
    reader = pkg.IqCorrector(max_input_samples=C * n)
    wide = x.view(C * n, 2)
    calls = {"cf32": lambda: mon_f.process(x), "u8": lambda: mon_b.process(b), "reader": lambda: reader.process(wide, out=False)}
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
    lines = [f"{C} stations x {n} samples at {a.fs} Sa/s, {a.rounds} alternating rounds of {a.iters} calls, device events (us per call)"]
    for k, v in times.items():
        nbytes = C * n * (2 if k == "u8" else 8)
        med = statistics.median(v)
        lines.append(f"{k:6s} median {med:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   {nbytes / 1e6:6.1f} MB per call, {nbytes / med / 1e6:5.2f} TB/s")
    med = statistics.median(times["cf32"])
    lines.append(f"cf32: {C * n / med:.0f} samples per us = {C * n / med * 1e6 / a.fs / C:.0f} x real time for each of {C} stations; "
                 f"{med * 1e3 / (n / 64):.1f} ns per 64-sample row of a station's wavefront")
    st = mon_f.status()
    lines.append(f"check: station 0 has {int(st[0]['samples'])} samples, {int(st[0]['intervals'])} intervals, deviation "
                 f"{pkg.modmon_deviation_hz(st[0], mon_f.design):.0f} Hz, u8 station 0 {pkg.modmon_deviation_hz(mon_b.status()[0], mon_b.design):.0f} Hz")
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
