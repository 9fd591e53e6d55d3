"""Times the audio fingerprinter's call (fmd_fprint_*: k_fprint_map, k_fprint_sub, k_fprint_frame) beside fmd_logmel_process_f32_dev, the
log-mel front end, over the same audio in the same process: 4096 stations x 2048 frames at 32 kHz by default (one 64 ms demodulator
block), the default geometry 368 / 32 / 33 bands, on the log-mel probe's programme (noise-like stereo at -20 dB a rail, every fourth
station a 1 kHz tone at -12 dBFS).  The calls are timed in alternating rounds with device events around `--iters` back-to-back calls
each, after a warm-up; the median, minimum and maximum over the rounds are printed with the share of the block's real time and the
fraction of the fp32 MFMA rate (`--peak-tflops`, 155 by default: what the kernel guide measures for v_mfma_f32_16x16x4_f32) that the
sub-block GEMM's 2 * 2 Kp * H flop a row would reach were the whole call the GEMM.  How the call divides between its kernels is read
from a kernel trace of this script (profiles/fprint/kernels.txt), not timed here.  Needs a GPU.  `--out FILE` also writes the report to a file (profiles/fprint/)."""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--peak-tflops", type=float, default=155.0)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    C, n = a.stations, a.frames
    n1 = torch.randn(C, n, device="cuda")
    x = torch.stack([0.1 * n1, 0.1 * (0.6 * n1 + 0.8 * torch.randn(C, n, device="cuda"))], dim=2).contiguous()
    del n1
    t = torch.arange(n, device="cuda", dtype=torch.float64) / a.fs
    x[3::4] = (0.25 * torch.sin(2.0 * torch.pi * 1000.0 * t)).float()[None, :, None]
    fp = pkg.Fingerprinter(C, a.fs, max_input_frames=n)
    mel = pkg.LogMel(C, a.fs, max_input_frames=n)
    rows = pkg.fprint_max_prints(fp.hop, n)
    out_w = torch.zeros((C, rows), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(C, dtype=torch.int32, device="cuda")
    out_m = torch.zeros((C, pkg.logmel_max_frames(mel.hop, n), mel.n_mels), device="cuda")
    cntm = torch.zeros(C, dtype=torch.int32, device="cuda")
    calls = {"fprint": lambda: fp.process(x, out=out_w, nprints=cnt),
             "logmel": lambda: mel.process(x, out=out_m, nframes=cntm)}
    warm = max(4, 2 * fp.n_sub * fp.hop // n + 2)                 # until every station writes words: the steady state
    for fn in calls.values():
        for _ in range(warm):
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
    st = fp.status()
    calls_made = warm + a.rounds * a.iters
    sub = int((st["frames"] // fp.hop).sum()) / calls_made         # sub-blocks (rows of the GEMM) a call
    Kp = (fp.n_bins + 15) // 16 * 16
    flop = 2.0 * 2.0 * Kp * fp.hop * sub                           # re and im, a multiply and an add each
    block_us = n / a.fs * 1e6
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"{C} stations x {n} frames at {a.fs} Hz, hop {fp.hop}, {fp.n_sub} sub-blocks a window, {fp.n_bands} bands, {fp.n_bins} bins (Kp {Kp}); state "
             f"{fp.state_bytes / 1e9:.3f} GB; {a.rounds} alternating rounds of {a.iters} calls after {warm} warm-up calls each, device events (us per call)"]
    for k, v in times.items():
        lines.append(f"{k:8s} median {med[k]:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   {med[k] / block_us * 100:6.3f} % of the {block_us / 1e3:.0f} ms the frames last")
    k = "fprint"
    lines.append(f"{k}: {sub:.0f} sub-blocks a call, {flop / 1e9:.2f} GFLOP of GEMM; were the whole call the GEMM: {flop / med[k] / 1e6:.1f} TFLOP/s, "
                 f"{flop / med[k] / 1e6 / a.peak_tflops * 100:.1f} % of {a.peak_tflops:.0f} TFLOP/s; {med[k] / med['logmel']:.2f} x the log-mel call's time")
    lines.append(f"check: station 3 has {int(st[3]['frames'])} frames, {int(st[3]['prints'])} words, fill {int(st[3]['fill'])}, its last call wrote "
                 f"{int(cnt[3])} words; nonfinite {int(st['nonfinite'].sum())}; under a tenth of the block's time: {'yes' if med['fprint'] < block_us / 10 else 'NO'}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
