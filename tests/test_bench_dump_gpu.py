"""bench.py --dump-outputs on the GPU: two runs with the same arguments time the requested number of steps and dump the same
outputs bit for bit (the inputs are seeded), in the tolerance and in the exact mode."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
FILES = ["audio.npy", "channels.npy", "rds_byte_counts.npy", "rds_bytes.npy", "rds_symbol_counts.npy", "rds_symbols.npy"]


def _run(out_dir, steps, extra=()):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--preroll", "8", "--channels", "64",
           "--no-cpu-baseline", "--no-other-mode", "--no-configs", "--no-kernel-times", "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [[], ["--exact"]], ids=["tolerance", "exact"])
def test_dumped_outputs_repeat_and_steps_are_the_timed_steps(tmp_path, mode):
    a = _run(tmp_path / "a", 3, mode)
    b = _run(tmp_path / "b", 3, mode)
    assert a["steps"] == b["steps"] == 3
    assert a["dumped_outputs"]["channels"] == 64 and sorted(a["dumped_outputs"]["files"]) == FILES
    for f in FILES:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and x.tobytes() == y.tobytes(), f
    audio = np.load(tmp_path / "a" / "audio.npy")
    assert audio.shape[0] == 64 and np.isfinite(audio).all() and np.abs(audio).max() > 0
    assert (np.load(tmp_path / "a" / "rds_symbol_counts.npy") > 0).all()
    # one more timed step is one more block demodulated: the last step's outputs are another block's
    c = _run(tmp_path / "c", 4, mode)
    assert c["steps"] == 4
    assert np.load(tmp_path / "c" / "audio.npy").tobytes() != audio.tobytes()
