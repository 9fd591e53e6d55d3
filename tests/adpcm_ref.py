"""The C restatement of the ADPCM audio encoder's arithmetic contract (tests/cpp/adpcm_ref.c), built with gcc and called through ctypes;
Python's audioop as the independent IMA reference; and the signals shared by tests/test_adpcm_cpu.py and tests/test_gpu_adpcm.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "adpcm_ref.c"
SCALE = np.float32(32767.0) * np.float32(0.95)
DEFAULT_S = 1017
# include/fmdemod.h fmd_adpcm_status
STATUS_DTYPE = np.dtype([("frames", "<u8"), ("blocks", "<u8"), ("padded", "<u8"), ("clipped", "<u8", (2,)), ("nonfinite", "<u8"), ("fill", "<u4"),
                         ("pred", "<i2", (2,)), ("index", "u1", (2,)), ("reserved", "u1", (6,))])
assert STATUS_DTYPE.itemsize == 64 and STATUS_DTYPE.fields["clipped"][1] == 24 and STATUS_DTYPE.fields["nonfinite"][1] == 40
assert STATUS_DTYPE.fields["fill"][1] == 48 and STATUS_DTYPE.fields["pred"][1] == 52 and STATUS_DTYPE.fields["index"][1] == 56


class _Status(C.Structure):
    _fields_ = [("frames", C.c_ulonglong), ("blocks", C.c_ulonglong), ("padded", C.c_ulonglong), ("clipped", C.c_ulonglong * 2), ("nonfinite", C.c_ulonglong),
                ("fill", C.c_uint), ("pred", C.c_short * 2), ("index", C.c_ubyte * 2), ("reserved", C.c_ubyte * 6)]


class _Chan(C.Structure):
    _fields_ = [("st", _Status), ("S", C.c_int), ("align", C.c_int), ("last_q", C.c_int * 2), ("open", C.c_ubyte * 8192)]


assert C.sizeof(_Status) == 64


def block_align(S: int) -> int:
    return 8 * ((S - 1) // 8 + 1)


class Channel:
    """one station of the restatement: process(x [n, 2] float32) -> the completed blocks [nb, block_align] uint8; flush(); status()"""

    def __init__(self, lib, S: int = 0):
        self.lib = lib
        self.c = _Chan()
        if lib.adpcm_ref_create(C.byref(self.c), int(S)) != 0:
            raise ValueError(f"block_frames {S}")
        self.S, self.align = int(self.c.S), int(self.c.align)

    def process(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x)
        assert x.ndim == 2 and x.shape[1] == 2 and x.dtype == np.float32
        out = np.zeros(((self.S - 1 + x.shape[0]) // self.S + 1, self.align), np.uint8)
        want = (self.fill + x.shape[0]) // self.S
        nb = self.lib.adpcm_ref_process(C.byref(self.c), x.ctypes.data_as(C.c_void_p), x.shape[0], out.ctypes.data_as(C.c_void_p))
        assert nb == want
        return out[:nb].copy()

    def flush(self) -> np.ndarray:
        out = np.zeros((1, self.align), np.uint8)
        nb = self.lib.adpcm_ref_flush(C.byref(self.c), out.ctypes.data_as(C.c_void_p))
        return out[:nb].copy()

    def reset(self):
        self.lib.adpcm_ref_reset(C.byref(self.c))

    def status(self) -> np.ndarray:
        """a [1] STATUS_DTYPE record array (a copy)"""
        return np.frombuffer(bytes(self.c.st), STATUS_DTYPE).copy()

    def set_frames(self, frames: int):
        """the frame count alone, for a station that has been running for long"""
        self.c.st.frames = int(frames)

    @property
    def fill(self) -> int:
        return int(self.c.st.fill)


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def channel(self, S: int = 0) -> Channel:
        return Channel(self.lib, S)

    def sample(self, x) -> tuple:
        """(q int32 [...], flag [...]: 0 in range, 1 clamped, 2 not finite) of float32 samples"""
        x = np.ascontiguousarray(x, np.float32)
        q, fl = np.zeros(x.size, np.int32), np.zeros(x.size, np.int32)
        f = C.c_int()
        for i, v in enumerate(x.reshape(-1)):
            q[i] = self.lib.adpcm_ref_sample(C.c_float(float(v)), C.byref(f))
            fl[i] = f.value
        return q.reshape(x.shape), fl.reshape(x.shape)

    def step(self, q: int, pred: int, index: int) -> tuple:
        """(code, pred, index) after one step of the quantiser"""
        p, i = C.c_int(pred), C.c_int(index)
        code = self.lib.adpcm_ref_step(int(q), C.byref(p), C.byref(i))
        return code, p.value, i.value

    def decode(self, blocks: np.ndarray, S: int) -> np.ndarray:
        """blocks [nb, block_align] uint8 -> [nb * S, 2] int16"""
        blocks = np.ascontiguousarray(blocks, np.uint8)
        nb = blocks.size // block_align(S)
        pcm = np.zeros((nb * S, 2), np.int16)
        assert self.lib.adpcm_ref_decode(blocks.ctypes.data_as(C.c_void_p), int(S), nb, pcm.ctypes.data_as(C.c_void_p)) == 0
        return pcm


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "libadpcm_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.adpcm_ref_create.argtypes = [C.POINTER(_Chan), C.c_int]
    lib.adpcm_ref_reset.argtypes = [C.POINTER(_Chan)]
    lib.adpcm_ref_reset.restype = None
    lib.adpcm_ref_process.argtypes = [C.POINTER(_Chan), C.c_void_p, C.c_longlong, C.c_void_p]
    lib.adpcm_ref_process.restype = C.c_longlong
    lib.adpcm_ref_flush.argtypes = [C.POINTER(_Chan), C.c_void_p]
    lib.adpcm_ref_sample.argtypes = [C.c_float, C.POINTER(C.c_int)]
    lib.adpcm_ref_step.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.adpcm_ref_decode.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p]
    lib.adpcm_ref_max_blocks.argtypes = [C.c_int, C.c_longlong]
    lib.adpcm_ref_max_blocks.restype = C.c_longlong
    return Ref(lib)


def bits(a) -> np.ndarray:
    """an array's bytes"""
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


def parse_block(block: np.ndarray, S: int) -> dict:
    """one block -> per rail the header sample, the header index and the S - 1 codes in frame order"""
    block = np.asarray(block, np.uint8)
    out = {"sample": [], "index": [], "zero": [], "codes": []}
    body = block[8:].reshape(-1, 2, 4)                                       # [group][rail][byte]
    for rail in range(2):
        h = block[4 * rail:4 * rail + 4]
        out["sample"].append(int(np.frombuffer(h[:2].tobytes(), "<i2")[0]))
        out["index"].append(int(h[2]))
        out["zero"].append(int(h[3]))
        b = body[:, rail, :].reshape(-1)
        out["codes"].append(np.stack([b & 15, b >> 4], axis=1).reshape(-1)[:S - 1])
    return out


def audioop_block(q: np.ndarray, index_in) -> tuple:
    """one block by audioop: q [S, 2] integers in the 16-bit range, the two indices as they stand -> (codes [2][S - 1] in frame order,
    the indices and predictors afterwards).  audioop packs the earlier sample into the HIGH nibble: unpacked here, not compared as bytes."""
    import audioop
    codes, index_out, pred_out = [], [], []
    for rail in range(2):
        s = np.ascontiguousarray(q[1:, rail], "<i2")
        if s.size % 2:                                                       # (S - 1 is a multiple of 8)
            raise ValueError("S - 1 must be even")
        data, (pred, index) = audioop.lin2adpcm(s.tobytes(), 2, (int(q[0, rail]), int(index_in[rail])))
        b = np.frombuffer(data, np.uint8)
        codes.append(np.stack([b >> 4, b & 15], axis=1).reshape(-1))
        index_out.append(index)
        pred_out.append(pred)
    return codes, index_out, pred_out


def audioop_decode_block(parsed: dict, S: int) -> np.ndarray:
    """one parsed block through audioop.adpcm2lin -> [S, 2] int16"""
    import audioop
    pcm = np.zeros((S, 2), np.int16)
    for rail in range(2):
        c = parsed["codes"][rail].astype(np.uint8)
        data = ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes()
        lin, _ = audioop.adpcm2lin(data, 2, (parsed["sample"][rail], parsed["index"][rail]))
        pcm[0, rail] = parsed["sample"][rail]
        pcm[1:, rail] = np.frombuffer(lin, "<i2")
    return pcm


# ---- signals ------------------------------------------------------------------------------------------------------------------------

def noise(n: int, level: float, seed: int) -> np.ndarray:
    """[n, 2] float32: independent gaussian noise of RMS `level` a rail"""
    return (level * np.random.default_rng(seed).standard_normal((n, 2))).astype(np.float32)


def sine(n: int, fs: float = 32000.0, f: float = 1000.0, a: float = 0.25, start: int = 0) -> np.ndarray:
    """[n, 2] float32: a sine of amplitude a on L and its quadrature on R"""
    t = (np.arange(n, dtype=np.float64) + start) / fs
    return np.stack([a * np.sin(2.0 * np.pi * f * t), a * np.cos(2.0 * np.pi * f * t)], axis=1).astype(np.float32)


def square(n: int, period: int = 64, a: float = 1.2) -> np.ndarray:
    """[n, 2] float32: a square wave past full scale (1.2 x 31128.65 clamps); at period 2 every frame is a full-scale jump, which drives the
    index to 88 and the predictor into its clamp within a dozen frames"""
    s = np.where((np.arange(n) // (period // 2)) % 2 == 0, a, -a)
    return np.stack([s, -s], axis=1).astype(np.float32)


def silence(n: int) -> np.ndarray:
    return np.zeros((n, 2), np.float32)


def edge_ramp(n: int) -> np.ndarray:
    """[n, 2] float32: a ramp whose q runs through -32768 ... 32767 and a little past both ends, up on L and down on R"""
    v = np.linspace(-32775.0, 32775.0, n) / float(SCALE)
    return np.stack([v, -v], axis=1).astype(np.float32)


def snr_db(ref_pcm: np.ndarray, got_pcm: np.ndarray) -> float:
    r, g = np.asarray(ref_pcm, np.float64), np.asarray(got_pcm, np.float64)
    return float(10.0 * np.log10(np.sum(r * r) / np.sum((r - g) ** 2)))
