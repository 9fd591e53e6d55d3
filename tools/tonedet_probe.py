"""Times the audio tone detector's call (fmd_tonedet_*, k_tonedet) with eight slots in use and with two, beside fmd_audmon_process_f32_dev,
the audio fault monitor, over the same bytes in the same process: 4096 stations x 2048 frames at 32 kHz by default (one 64 ms
demodulator block).  The calls are timed in alternating rounds with device events around `--iters` back-to-back calls each; the median,
minimum and maximum over the rounds are printed with what each call does per frame: the detector's fp64 multiply-adds (1 + 2 per used
slot) and 16-byte table gathers (one per used slot).  Needs a GPU.  `--out FILE` also writes the report to a file (profiles/tonedet/)."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import fmradio_loader  # noqa: E402

SETS = {"tonedet_8": (1000, 440, 400, 853, 960, 1050, 1, 15999), "tonedet_2": (853, 960, 0, 0, 0, 0, 0, 0)}


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
    # a noise-like stereo programme at -20 dB a rail; every fourth station carries a 1000 Hz line-up tone at -12 dBFS instead
    n1 = torch.randn(C, n, device="cuda")
    x = torch.stack([0.1 * n1, 0.1 * (0.6 * n1 + 0.8 * torch.randn(C, n, device="cuda"))], dim=2).contiguous()
    del n1
    t = torch.arange(n, device="cuda", dtype=torch.float64) / a.fs
    x[3::4] = (0.25 * torch.sin(2.0 * torch.pi * 1000.0 * t)).float()[None, :, None]
    det = {k: pkg.ToneDetector(C, a.fs, max_input_frames=n) for k in SETS}
    for k, f in SETS.items():
        det[k].set_params(freq_hz=f, raise_intervals=2)
    mon = pkg.AudioMonitor(C, a.fs, max_input_frames=n)
    flags = torch.zeros(C, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(C, dtype=torch.uint8, device="cuda")
    f8 = torch.zeros(C, dtype=torch.uint8, device="cuda")
    calls = {"tonedet_8": lambda: det["tonedet_8"].process(x, flags=f8, ok=ok), "tonedet_2": lambda: det["tonedet_2"].process(x, flags=flags, ok=ok),
             "audmon": lambda: mon.process(x, flags=flags, ok=ok)}
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
    for k, v in times.items():
        slots = sum(1 for f in SETS[k] if f) if k in SETS else 0
        work = f"{1 + 2 * slots} fp64 fma and {slots} gathers a frame: {C * n * (1 + 2 * slots) / med[k] / 1e6:5.2f} Tfma/s, {C * n * slots / med[k] / 1e3:6.1f} G gathers/s" if k in SETS \
            else "3 fp64 fma a frame"
        lines.append(f"{k:10s} median {med[k]:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   {C * n * 8 / med[k] / 1e6:5.2f} TB/s of samples; {work}")
    lines.append(f"tonedet: {med['tonedet_8'] / med['audmon']:.1f} x k_audmon's time with eight slots, {med['tonedet_2'] / med['audmon']:.1f} x with two; "
                 f"{(med['tonedet_8'] - med['tonedet_2']) / 6.0:.1f} us a slot; with eight slots {C * n / med['tonedet_8'] * 1e6 / a.fs / C:.0f} x real time for each of {C} stations")
    st = det["tonedet_8"].status()
    lines.append(f"check: station 3 has {int(st[3]['frames'])} frames, {int(st[3]['intervals'])} intervals, share of 1000 Hz {pkg.tonedet_share_db(st[3], a.fs, 0, 10):.3f} dB, "
                 f"of station 0 {pkg.tonedet_share_db(st[0], a.fs, 0, 10):.1f} dB; flags of stations 0, 3: {[int(st[c]['flags']) for c in (0, 3)]}; "
                 f"flagged {int((f8 != 0).sum())} of {C}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
