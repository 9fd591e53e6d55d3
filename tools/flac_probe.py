"""Times the FLAC encoder's call (fmd_flac_*, k_flac) beside fmd_adpcm_process_f32_dev, the ADPCM encoder, over the same bytes in the
same process: 4096 stations x 2048 frames at 32 kHz by default (one 64 ms demodulator block), FLAC blocks of 4096 frames, on the ADPCM
probe's programme (noise-like stereo at -20 dB a rail, every fourth station a 1 kHz tone at -12 dBFS).  The calls are timed in
alternating rounds with device events around `--iters` back-to-back calls each, after a warm-up; the median, minimum and maximum over
the rounds are printed with the bytes written per second and the compression ratio on that programme.  With S = 4096 and calls of 2048
frames a station completes a block in every other call, so a round of 20 calls holds 10 blocks per station.  Needs a GPU.  `--out FILE`
also writes the report to a file (profiles/flac/)."""
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
    # the ADPCM probe's programme
    n1 = torch.randn(C, n, device="cuda")
    x = torch.stack([0.1 * n1, 0.1 * (0.6 * n1 + 0.8 * torch.randn(C, n, device="cuda"))], dim=2).contiguous()
    del n1
    t = torch.arange(n, device="cuda", dtype=torch.float64) / a.fs
    x[3::4] = (0.25 * torch.sin(2.0 * torch.pi * 1000.0 * t)).float()[None, :, None]
    flac = pkg.FlacEncoder(C, a.block_frames, a.fs, max_input_frames=n)
    adpcm = pkg.AdpcmEncoder(C, max_input_frames=n)
    S = flac.block_frames
    out_f = torch.zeros((C, pkg.flac_max_bytes(S, n)), dtype=torch.uint8, device="cuda")
    nby, nfr = torch.zeros(C, dtype=torch.int32, device="cuda"), torch.zeros(C, dtype=torch.int32, device="cuda")
    out_a = torch.zeros((C, pkg.adpcm_max_blocks(adpcm.block_frames, n) * adpcm.block_align), dtype=torch.uint8, device="cuda")
    nb = torch.zeros(C, dtype=torch.int32, device="cuda")
    calls = {"flac": lambda: flac.process(x, out=out_f, nbytes=nby, nframes=nfr), "adpcm": lambda: adpcm.process(x, out=out_a, nblocks=nb)}
    for fn in calls.values():
        for _ in range(4):
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
    st = flac.status()
    frames, written = int(st["frames"].sum()), int(st["stream_bytes"].sum())
    coded = int(st["stream_samples"].sum())
    ratio = written / (coded * 4) if coded else float("nan")
    per = [int(st[c]["stream_bytes"]) / (int(st[c]["stream_samples"]) * 4) for c in (0, 3) if int(st[c]["stream_samples"])]
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"{C} stations x {n} frames at {a.fs} Hz, FLAC blocks of {S} frames, ADPCM blocks of {adpcm.block_frames}, {a.rounds} alternating rounds of {a.iters} calls "
             f"after 4 warm-up calls each, device events (us per call)"]
    for k, v in times.items():
        lines.append(f"{k:6s} median {med[k]:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   {C * n / med[k] / 1e3:7.2f} G frames/s, {C * n * 8 / med[k] / 1e6:5.2f} TB/s of samples read")
    lines.append(f"flac: {med['flac'] / med['adpcm']:.2f} x the ADPCM call's time; {med['flac'] / (n / a.fs * 1e6) * 100:.2f} % of the {n / a.fs * 1e3:.0f} ms the frames last")
    lines.append(f"flac wrote {written} bytes for {coded} coded frames of {frames} taken: {ratio:.4f} of the PCM16 bytes ({ratio * 16:.2f} bits a sample; "
                 f"a noise station {per[0]:.4f}, a tone station {per[1]:.4f}), {C * n * 4 * ratio / med['flac'] / 1e3:.1f} GB/s of FLAC frames written at the median "
                 f"against {C * n / adpcm.block_frames * adpcm.block_align / med['adpcm'] / 1e3:.1f} GB/s of ADPCM blocks")
    lines.append(f"check: station 3 has {int(st[3]['frames'])} frames, {int(st[3]['blocks'])} FLAC frames, fill {int(st[3]['fill'])}, "
                 f"frame bytes {int(st[3]['min_frame_bytes'])} ... {int(st[3]['max_frame_bytes'])}; nonfinite {int(st['nonfinite'].sum())}, clipped {int(st['clipped'].sum())}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
