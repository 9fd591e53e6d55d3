"""Times the ADPCM encoder's call (fmd_adpcm_*, k_adpcm) beside fmd_audmon_process_f32_dev, the audio fault monitor, over the same bytes
in the same process: 4096 stations x 2048 frames at 32 kHz by default (one 64 ms demodulator block), default blocks of 1017 frames.  The
calls are timed in alternating rounds with device events around `--iters` back-to-back calls each; the median, minimum and maximum over
the rounds are printed with frames per second and the ratio.  The encoder is timed twice: on a noise-like programme and on the same
programme with every fourth station driven past full scale (the counting path).  Needs a GPU.  `--out FILE` also writes the report to a
file (profiles/adpcm/)."""
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
    ap.add_argument("--block-frames", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    C, n = a.stations, a.frames
    # a noise-like stereo programme at -20 dB a rail; every fourth station carries a 1000 Hz tone at -12 dBFS instead
    n1 = torch.randn(C, n, device="cuda")
    x = torch.stack([0.1 * n1, 0.1 * (0.6 * n1 + 0.8 * torch.randn(C, n, device="cuda"))], dim=2).contiguous()
    del n1
    t = torch.arange(n, device="cuda", dtype=torch.float64) / a.fs
    x[3::4] = (0.25 * torch.sin(2.0 * torch.pi * 1000.0 * t)).float()[None, :, None]
    loud = x.clone()
    loud[1::4] *= 20.0                                            # past full scale most of the time: clamped and counted
    enc = {k: pkg.AdpcmEncoder(C, a.block_frames, max_input_frames=n) for k in ("adpcm", "adpcm_clipping")}
    S, align = enc["adpcm"].block_frames, enc["adpcm"].block_align
    mon = pkg.AudioMonitor(C, a.fs, max_input_frames=n)
    out = torch.zeros((C, pkg.adpcm_max_blocks(S, n) * align), dtype=torch.uint8, device="cuda")
    nb = torch.zeros(C, dtype=torch.int32, device="cuda")
    flags = torch.zeros(C, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(C, dtype=torch.uint8, device="cuda")
    calls = {"adpcm": lambda: enc["adpcm"].process(x, out=out, nblocks=nb), "adpcm_clipping": lambda: enc["adpcm_clipping"].process(loud, out=out, nblocks=nb),
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
    lines = [f"{C} stations x {n} frames at {a.fs} Hz, blocks of {S} frames ({align} bytes), {a.rounds} alternating rounds of {a.iters} calls, device events (us per call)"]
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        lines.append(f"{k:15s} median {med[k]:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   {C * n / med[k] / 1e3:7.2f} G frames/s, {C * n * 8 / med[k] / 1e6:5.2f} TB/s of samples read"
                     + (f", {C * n / S * align / med[k] / 1e3:6.1f} GB/s of blocks written" if k != "audmon" else ""))
    lines.append(f"adpcm: {med['adpcm'] / med['audmon']:.1f} x k_audmon's time ({med['adpcm_clipping'] / med['audmon']:.1f} x with a quarter of the stations clipping); "
                 f"{med['adpcm'] / (n / a.fs * 1e6) * 100:.2f} % of the {n / a.fs * 1e3:.0f} ms the frames last; "
                 f"{C * n / med['adpcm'] * 1e6 / a.fs / C:.0f} x real time for each of {C} stations")
    lines.append(f"configuration: one wavefront per 32 stations ({(C + 31) // 32} wavefronts), tiles of 128 frames, code words stored directly; "
                 "no other tile length, station grouping or output path was built or measured")
    enc["adpcm"].flush(out=out, nblocks=nb)
    st, sl = enc["adpcm"].status(), enc["adpcm_clipping"].status()
    pcm = pkg.adpcm_decode(out[3, :align].cpu().numpy(), S)
    lines.append(f"check: station 3 has {int(st[3]['frames'])} frames, {int(st[3]['blocks'])} blocks, {int(st[3]['padded'])} padded, fill {int(st[3]['fill'])}; "
                 f"its flushed block decodes to a peak of {int(abs(pcm.astype(int)).max())} (a -12 dBFS sine: 7782); "
                 f"clipped samples of stations 0, 1 in the loud set: {[int(sl[c]['clipped'].sum()) for c in (0, 1)]}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
