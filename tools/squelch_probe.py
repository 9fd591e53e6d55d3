"""Times the carrier squelch's call (fmd_squelch_*, k_squelch) for cf32 and u8 station baseband beside two neighbours that read the same
bytes in the same process: fmd_iqcorr_process_cf32_dev with d_out = NULL (a one-pass measuring reader) and fmd_modmon_process_cf32_dev
(the modulation monitor): 4096 stations x 16384 samples at 256 kSa/s by default (one 64 ms demodulator block).  The four are timed in
alternating rounds with device events around `--iters` back-to-back calls each; the median, minimum and maximum over the rounds are
printed with the bytes each call reads and the share of the read roof (`--roof`, TB/s: profiles/round6/hbm_roof_probe.txt).  Needs a
GPU.  `--out FILE` also writes the report to a file (profiles/squelch/)."""
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
    ap.add_argument("--roof", type=float, default=7.07)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    C, n = a.stations, a.samples
    # carriers of amplitude 100 frequency-modulated by noise, about 50 kHz peak, 20 dB over complex Gaussian noise; every fourth station
    # is noise alone
    f = torch.randn(C, n, device="cuda") * (15000.0 / a.fs * 6.283185307179586)
    ph = torch.cumsum(f, dim=1)
    x = torch.stack([torch.cos(ph), torch.sin(ph)], dim=2)
    x[3::4] = 0.0
    x = (100.0 * x + 7.07 * torch.randn(C, n, 2, device="cuda")).contiguous()
    del f, ph
    b = torch.clamp(torch.round(x * 0.4 + 127.0), 0, 255).to(torch.uint8).contiguous()
    sq_f = pkg.Squelch(C, a.fs, max_input_samples=n)
    sq_b = pkg.Squelch(C, a.fs, max_input_samples=n)
    mon = pkg.ModulationMonitor(C, a.fs, max_input_samples=n)
    reader = pkg.IqCorrector(max_input_samples=C * n)
    mask_f = torch.zeros(C, dtype=torch.uint8, device="cuda")
    mask_b = torch.zeros(C, dtype=torch.uint8, device="cuda")
    wide = x.view(C * n, 2)
    calls = {"cf32": lambda: sq_f.process(x, mask=mask_f), "u8": lambda: sq_b.process(b, mask=mask_b),
             "reader": lambda: reader.process(wide, out=False), "modmon": lambda: mon.process(x)}
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
        # the squelch also reads and writes the open interval's 4 KB of partials per station and call
        nbytes = C * n * (2 if k == "u8" else 8) + (C * 8192 if k in ("cf32", "u8") else 0)
        med = statistics.median(v)
        lines.append(f"{k:6s} median {med:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   {nbytes / 1e6:6.1f} MB per call, {nbytes / med / 1e6:5.2f} TB/s"
                     f" = {100.0 * nbytes / med / 1e6 / a.roof:4.1f} % of the {a.roof} TB/s read roof")
    med = statistics.median(times["cf32"])
    lines.append(f"cf32: {C * n / med:.0f} samples per us = {C * n / med * 1e6 / a.fs / C:.0f} x real time for each of {C} stations; "
                 f"{med * 1e3 / (n / 256):.1f} ns per 256-sample row of a station's wavefront; "
                 f"{statistics.median(times['reader']) / med:.2f} x the reader's and {statistics.median(times['modmon']) / med:.2f} x the monitor's speed")
    st, sb = sq_f.status(), sq_b.status()
    lines.append(f"check: station 0 has {int(st[0]['samples'])} samples, {int(st[0]['intervals'])} intervals, cnr {pkg.squelch_cnr_db(st[0], a.fs, 1):.2f} dB "
                 f"(u8 {pkg.squelch_cnr_db(sb[0], a.fs, 1):.2f} dB), station 3 {pkg.squelch_cnr_db(st[3], a.fs, 1):.2f} dB; "
                 f"open {int(mask_f.sum())} of {C} (u8 {int(mask_b.sum())})")
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
