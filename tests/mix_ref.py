"""The C restatement of the reference's audio mixer (tests/cpp/mix_ref.c), built with gcc and called through ctypes."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "mix_ref.c"


def build(tmp_dir: Path):
    """Returns mix(x, sources, active=None, gain=1.0, f64_log=False) -> [n, 2] float32 for x [C, n, 2] float32 (one bus), and the
    library (for mix_ref_scale)."""
    so = Path(tmp_dir) / "libmix_ref.so"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.mix_ref.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p]
    lib.mix_ref.restype = C.c_int
    lib.mix_ref_scale.argtypes = [C.c_float, C.c_int, C.c_int]
    lib.mix_ref_scale.restype = C.c_float

    def mix(x: np.ndarray, sources, active=None, gain: float = 1.0, f64_log: bool = False) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        src = np.ascontiguousarray(sources, np.int32)
        act = None if active is None else np.ascontiguousarray(active, np.uint8)
        n = x.shape[1]
        out = np.empty((n, 2), np.float32)
        lib.mix_ref(x.ctypes.data_as(C.c_void_p), n, n, src.ctypes.data_as(C.c_void_p), src.size,
                    None if act is None else act.ctypes.data_as(C.c_void_p), C.c_float(float(np.float32(gain))), int(f64_log),
                    out.ctypes.data_as(C.c_void_p))
        return out
    mix.lib = lib
    return mix


def fixture_case(g, key):
    """(x [nreg, n, 2], active [nreg] uint8, gain float32, expected [n, 2]) of one tests/golden/mix_ref.npz case; the sources are the
    rows 0 .. nreg - 1 in that order"""
    return g[key + "_in"], g[key + "_active"], np.float32(g[key + "_gain"]), g[key + "_out"]
