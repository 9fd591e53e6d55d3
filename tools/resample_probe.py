"""Times the batched audio resampler's kernels (fmd_resampler_*): 4096 stations x 2048 frames at 32 kHz -> fs_out, both methods, f32 and
pcm16 outputs.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/resample_probe.py`; it also prints its own event times and the
bytes each call moves (input read once, output written once)."""
import argparse
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
    ap.add_argument("--fs-out", type=int, default=48000)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    x = 0.3 * torch.randn(a.stations, a.frames, 2, device="cuda")
    for method in ("reference", "polyphase"):
        rs = pkg.AudioResampler(a.stations, a.fs_out, method=method, max_input_frames=a.frames)
        for form in ("f32", "pcm16"):
            fn = rs.process if form == "f32" else rs.process_pcm16
            n_out = rs.output_frames(a.frames)
            out = torch.empty(a.stations, n_out + 1, 2, device="cuda", dtype=torch.float32 if form == "f32" else torch.int16)
            for _ in range(5):
                fn(x, out=out)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn(x, out=out)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / a.iters
            nbytes = x.numel() * 4 + a.stations * n_out * 2 * (4 if form == "f32" else 2)
            print(f"{method:9s} {form:5s} {a.stations} x {a.frames} -> {n_out} @ {a.fs_out}: {ms * 1e3:8.1f} us  {nbytes / ms / 1e9:6.2f} TB/s")
        rs.close()


if __name__ == "__main__":
    main()
