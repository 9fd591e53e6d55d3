"""Times the batched audio mixer's kernels (fmd_mixer_*) on 4096 stations x 4800 frames (48 kHz / 10, the reference's PortAudio block):
4096 one-station buses (the reference app's shape, k_mix_stream) and one bus of all 4096 stations (a monitoring mix, k_mix_staged), then
the bus-size sweep between them (4096 / K buses of K stations).  Run it under `rocprofv3 --kernel-trace --stats -- python tools/mix_probe.py`;
it also prints its own event times and the bytes each call moves (every source frame read once, every bus frame written once)."""
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
    ap.add_argument("--frames", type=int, default=4800)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sweep", type=int, nargs="*", default=[2, 8, 16, 32, 64, 256])
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    C, n = a.stations, a.frames
    x = 0.3 * torch.randn(C, n, 2, device="cuda")
    shapes = [("1-station buses", [[c] for c in range(C)]), ("one bus of all", [list(range(C))])]
    shapes += [(f"{k}-station buses", [list(range(b * k, (b + 1) * k)) for b in range(C // k)]) for k in a.sweep]
    for name, buses in shapes:
        m = pkg.AudioMixer(C, buses)
        out = torch.empty(len(buses), n, 2, device="cuda")
        for _ in range(5):
            m.process(x, out=out)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            m.process(x, out=out)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / a.iters
        nbytes = sum(len(b) for b in buses) * n * 8 + len(buses) * n * 8
        print(f"{name:18s} {len(buses):5d} buses x {n} frames: {ms * 1e3:8.1f} us  {nbytes / 1e6:7.1f} MB  {nbytes / ms / 1e9:6.2f} TB/s")
        m.close()


if __name__ == "__main__":
    main()
