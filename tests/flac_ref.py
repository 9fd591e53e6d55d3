"""The C restatement of the FLAC audio encoder's contract (tests/cpp/flac_ref.c), built with gcc and called through ctypes; a FLAC
decoder written from RFC 9639 that shares nothing with the restatement's encoder and is strict about what the RFC reserves; and the
signals shared by tests/test_flac_cpu.py and tests/test_gpu_flac.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "flac_ref.c"
SCALE = np.float32(32767.0) * np.float32(0.95)
DEFAULT_S = 4096
MAXS = 4608
# include/fmdemod.h fmd_flac_status
STATUS_DTYPE = np.dtype([("frames", "<u8"), ("blocks", "<u8"), ("stream_samples", "<u8"), ("stream_bytes", "<u8"), ("clipped", "<u8", (2,)), ("nonfinite", "<u8"),
                         ("streams", "<u4"), ("frame_number", "<u4"), ("min_frame_bytes", "<u4"), ("max_frame_bytes", "<u4"), ("fill", "<u4"), ("wrapped", "<u4")])
assert STATUS_DTYPE.itemsize == 80 and STATUS_DTYPE.fields["clipped"][1] == 32 and STATUS_DTYPE.fields["streams"][1] == 56 and STATUS_DTYPE.fields["fill"][1] == 72


class _Status(C.Structure):
    _fields_ = [("frames", C.c_ulonglong), ("blocks", C.c_ulonglong), ("stream_samples", C.c_ulonglong), ("stream_bytes", C.c_ulonglong), ("clipped", C.c_ulonglong * 2),
                ("nonfinite", C.c_ulonglong), ("streams", C.c_uint), ("frame_number", C.c_uint), ("min_frame_bytes", C.c_uint), ("max_frame_bytes", C.c_uint),
                ("fill", C.c_uint), ("wrapped", C.c_uint)]


class _Chan(C.Structure):
    _fields_ = [("st", _Status), ("S", C.c_int), ("fs", C.c_int), ("open", C.c_int * (2 * MAXS))]


assert C.sizeof(_Status) == 80


def frame_bound(S: int) -> int:
    return 16 + 2 * (1 + 2 * S) + 2


def max_bytes(S: int, n: int) -> int:
    return ((S - 1 + n) // S * frame_bound(S) + 3) // 4 * 4


class Channel:
    """one station of the restatement: process(x [n, 2] float32) -> (the completed FLAC frames' bytes, their number); flush(); status()"""

    def __init__(self, lib, S: int = 0, fs: int = 32000):
        self.lib = lib
        self.c = _Chan()
        if lib.flac_ref_create(C.byref(self.c), int(S), int(fs)) != 0:
            raise ValueError(f"block_frames {S} or fs {fs}")
        self.S, self.fs = int(self.c.S), int(fs)

    def process(self, x) -> tuple:
        x = np.ascontiguousarray(x)
        assert x.ndim == 2 and x.shape[1] == 2 and x.dtype == np.float32
        out = np.zeros(max_bytes(self.S, x.shape[0]) + 4, np.uint8)
        want = (self.fill + x.shape[0]) // self.S
        nf = C.c_int()
        nbytes = self.lib.flac_ref_process(C.byref(self.c), x.ctypes.data_as(C.c_void_p), x.shape[0], out.ctypes.data_as(C.c_void_p), C.byref(nf))
        assert nf.value == want and nbytes <= want * frame_bound(self.S)
        return out[:nbytes].copy(), nf.value

    def flush(self) -> tuple:
        out = np.zeros(frame_bound(self.S), np.uint8)
        nf = C.c_int()
        nbytes = self.lib.flac_ref_flush(C.byref(self.c), out.ctypes.data_as(C.c_void_p), C.byref(nf))
        return out[:nbytes].copy(), nf.value

    def reset(self):
        self.lib.flac_ref_reset(C.byref(self.c))

    def status(self) -> np.ndarray:
        """a [1] STATUS_DTYPE record array (a copy)"""
        return np.frombuffer(bytes(self.c.st), STATUS_DTYPE).copy()

    def set_frame_number(self, v: int):
        self.lib.flac_ref_set_frame_number(C.byref(self.c), int(v))

    @property
    def fill(self) -> int:
        return int(self.c.st.fill)


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def channel(self, S: int = 0, fs: int = 32000) -> Channel:
        return Channel(self.lib, S, fs)

    def sample(self, x) -> tuple:
        """(q int32 [...], flag [...]: 0 in range, 1 clamped, 2 not finite) of float32 samples"""
        x = np.ascontiguousarray(x, np.float32)
        q, fl = np.zeros(x.size, np.int32), np.zeros(x.size, np.int32)
        f = C.c_int()
        for i, v in enumerate(x.reshape(-1)):
            q[i] = self.lib.flac_ref_sample(C.c_float(float(v)), C.byref(f))
            fl[i] = f.value
        return q.reshape(x.shape), fl.reshape(x.shape)

    def crc8(self, data: bytes) -> int:
        return int(self.lib.flac_ref_crc8(data, len(data)))

    def crc16(self, data: bytes) -> int:
        return int(self.lib.flac_ref_crc16(data, len(data)))

    def coded_number(self, v: int) -> bytes:
        out = (C.c_ubyte * 8)()
        return bytes(out[:self.lib.flac_ref_coded_number(int(v), out)])

    def encode_frame(self, q: np.ndarray, fs: int, number: int) -> np.ndarray:
        """one FLAC frame of q [n, 2] integers"""
        left, right = np.ascontiguousarray(q[:, 0], np.int32), np.ascontiguousarray(q[:, 1], np.int32)
        out = np.zeros(frame_bound(max(64, (q.shape[0] + 63) // 64 * 64)), np.uint8)
        n = self.lib.flac_ref_encode_frame(left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), q.shape[0], int(fs), int(number), out.ctypes.data_as(C.c_void_p))
        return out[:n].copy()


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "libflac_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.flac_ref_create.argtypes = [C.POINTER(_Chan), C.c_int, C.c_int]
    lib.flac_ref_reset.argtypes = [C.POINTER(_Chan)]
    lib.flac_ref_reset.restype = None
    lib.flac_ref_process.argtypes = [C.POINTER(_Chan), C.c_void_p, C.c_longlong, C.c_void_p, C.POINTER(C.c_int)]
    lib.flac_ref_process.restype = C.c_longlong
    lib.flac_ref_flush.argtypes = [C.POINTER(_Chan), C.c_void_p, C.POINTER(C.c_int)]
    lib.flac_ref_set_frame_number.argtypes = [C.POINTER(_Chan), C.c_uint]
    lib.flac_ref_set_frame_number.restype = None
    lib.flac_ref_sample.argtypes = [C.c_float, C.POINTER(C.c_int)]
    lib.flac_ref_crc8.argtypes = [C.c_char_p, C.c_longlong]
    lib.flac_ref_crc8.restype = C.c_uint
    lib.flac_ref_crc16.argtypes = [C.c_char_p, C.c_longlong]
    lib.flac_ref_crc16.restype = C.c_uint
    lib.flac_ref_coded_number.argtypes = [C.c_uint, C.c_void_p]
    lib.flac_ref_encode_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_void_p]
    lib.flac_ref_max_bytes.argtypes = [C.c_int, C.c_longlong]
    lib.flac_ref_max_bytes.restype = C.c_longlong
    return Ref(lib)


def bits(a) -> np.ndarray:
    """an array's bytes"""
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


# ---- a decoder from RFC 9639 -----------------------------------------------------------------------------------------------------------

class FlacError(ValueError):
    pass


def _crc(data: bytes, poly: int, width: int) -> int:
    top, mask, c = 1 << (width - 1), (1 << width) - 1, 0
    for byte in data:
        c ^= byte << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
    return c


_CRC16_TABLE = [_crc(bytes([i]), 0x8005, 16) for i in range(256)]


def crc8(data: bytes) -> int:
    """RFC 9639 section 9.1.8: polynomial x^8 + x^2 + x + 1, initialised with 0"""
    return _crc(data, 0x07, 8)


def crc16(data: bytes) -> int:
    """RFC 9639 section 9.3: polynomial x^16 + x^15 + x^2 + 1, initialised with 0"""
    c = 0
    for byte in data:
        c = ((c << 8) & 0xffff) ^ _CRC16_TABLE[(c >> 8) ^ byte]
    return c


_BLOCK_SIZES = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}


class _Bits:
    """a frame's bits as a string of '0' and '1', read from the left"""

    def __init__(self, data: bytes, pos: int = 0):
        self.s = bin(int.from_bytes(b"\x01" + data, "big"))[3:]
        self.pos = pos

    def u(self, n: int) -> int:
        if self.pos + n > len(self.s):
            raise FlacError("the frame ends inside a field")
        v = int(self.s[self.pos:self.pos + n], 2) if n else 0
        self.pos += n
        return v

    def s_(self, n: int) -> int:
        v = self.u(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self) -> int:
        at = self.s.find("1", self.pos)
        if at < 0:
            raise FlacError("the frame ends inside a unary number")
        q = at - self.pos
        self.pos = at + 1
        return q


def _subframe(b: _Bits, n: int, bps: int, info: dict) -> list:
    if b.u(1) != 0:
        raise FlacError("subframe padding bit set")
    kind = b.u(6)
    if b.u(1) != 0:
        raise FlacError("wasted bits flagged: not in this encoder's subset")
    if kind == 0:
        info["type"] = "CONSTANT"
        return [b.s_(bps)] * n
    if kind == 1:
        info["type"] = "VERBATIM"
        return [b.s_(bps) for _ in range(n)]
    if not 8 <= kind <= 12:
        raise FlacError(f"subframe type {kind:06b} is reserved or LPC")
    order = kind - 8
    info.update(type="FIXED", order=order)
    if order > n:
        raise FlacError("predictor order above the block size")
    x = [b.s_(bps) for _ in range(order)]
    method = b.u(2)
    if method != 0:
        raise FlacError(f"residual coding method {method}: not 00")
    p = b.u(4)
    info.update(porder=p, k=[])
    if n % (1 << p) or (n >> p) <= order and not (p == 0 and n > order):
        raise FlacError("partition order does not fit the block size and predictor order")
    coef = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}[order]
    for j in range(1 << p):
        k = b.u(4)
        if k == 15:
            raise FlacError("escaped partition: not in this encoder's subset")
        info["k"].append(k)
        for _ in range((n >> p) - (order if j == 0 else 0)):
            u = (b.unary() << k) | b.u(k)
            r = (u >> 1) if not u & 1 else -((u + 1) >> 1)
            if not -(1 << 31) < r < (1 << 31):
                raise FlacError("residual outside 32 bits")
            x.append(r + sum(c * x[-1 - i] for i, c in enumerate(coef)))
    return x


def decode_frame(data: bytes, at: int, fs: int, S: int, number: int) -> tuple:
    """the frame at data[at:] of a fixed-blocksize 16-bit stereo stream of rate fs and block size S whose number must be `number` ->
    (pcm [n, 2] int16, bytes consumed, info: code, n, and per subframe type / order / porder / k)"""
    d = data[at:]
    if len(d) < 6 or d[0] != 0xff or d[1] != 0xf8:
        raise FlacError("no sync code, a reserved bit set, or a variable-blocksize frame")
    bs_code, sr_code, ch_code, ss_code = d[2] >> 4, d[2] & 15, d[3] >> 4, (d[3] >> 1) & 7
    if d[3] & 1:
        raise FlacError("reserved bit set")
    if bs_code == 0 or sr_code in (0, 15) or ss_code != 4 or ch_code not in (1, 8, 9, 10):
        raise FlacError("reserved code, or not 16-bit stereo with its rate in the header")
    first = d[4]
    extra = 0 if first < 0x80 else 1 if first >> 5 == 6 else 2 if first >> 4 == 14 else 3 if first >> 3 == 30 else 4 if first >> 2 == 62 else 5 if first >> 1 == 126 else -1
    if extra < 0:
        raise FlacError("coded number's first byte")
    v = first if extra == 0 else first & (0x3f >> extra)
    for i in range(extra):
        if d[5 + i] >> 6 != 2:
            raise FlacError("coded number's continuation byte")
        v = (v << 6) | (d[5 + i] & 0x3f)
    if extra and v < (0x80, 0x800, 0x10000, 0x200000, 0x4000000)[extra - 1]:
        raise FlacError("coded number longer than it needs to be")
    if v != number:
        raise FlacError(f"frame number {v}, expected {number}")
    p = 5 + extra
    if bs_code == 6:
        n = d[p] + 1; p += 1
    elif bs_code == 7:
        n = (d[p] << 8 | d[p + 1]) + 1; p += 2
    else:
        n = _BLOCK_SIZES[bs_code]
    if bs_code in (6, 7) and (n in _BLOCK_SIZES.values() or (bs_code == 7 and n <= 256)):
        raise FlacError("block size not coded the shortest way")
    if sr_code == 12:
        rate = d[p] * 1000; p += 1
    elif sr_code == 13:
        rate = d[p] << 8 | d[p + 1]; p += 2
    elif sr_code == 14:
        rate = (d[p] << 8 | d[p + 1]) * 10; p += 2
    else:
        rate = _RATES[sr_code]
    if rate != fs or (sr_code > 11 and fs in _RATES.values()):
        raise FlacError("sample rate")
    if n > S:
        raise FlacError("frame longer than the stream's block size")
    if crc8(d[:p]) != d[p]:
        raise FlacError("CRC-8")
    p += 1
    b = _Bits(d[:p + 2 * (1 + (17 * n + 7) // 8) + 8], 8 * p)
    info = dict(code=ch_code, n=n, sub=[{}, {}])
    c0 = _subframe(b, n, 17 if ch_code == 9 else 16, info["sub"][0])
    c1 = _subframe(b, n, 17 if ch_code in (8, 10) else 16, info["sub"][1])
    if b.u((-b.pos) % 8) != 0:
        raise FlacError("padding bits set")
    end = b.pos // 8
    if end + 2 > len(d) or crc16(d[:end]) != (d[end] << 8 | d[end + 1]):
        raise FlacError("CRC-16")
    a0, a1 = np.array(c0, np.int64), np.array(c1, np.int64)
    if ch_code == 1:
        left, right = a0, a1
    elif ch_code == 8:
        left, right = a0, a0 - a1
    elif ch_code == 9:
        left, right = a0 + a1, a1
    else:
        mid = (a0 << 1) | (a1 & 1)
        left, right = (mid + a1) >> 1, (mid - a1) >> 1
    pcm = np.stack([left, right], axis=1)
    if pcm.min() < -32768 or pcm.max() > 32767:
        raise FlacError("decoded sample outside 16 bits")
    return pcm.astype(np.int16), end + 2, info


def decode_stream(data, fs: int, S: int) -> tuple:
    """frames back to back, numbered from 0; only the last may be shorter than S -> (pcm [total, 2] int16, [info per frame])"""
    data = bytes(np.asarray(data, np.uint8)) if not isinstance(data, (bytes, bytearray)) else bytes(data)
    at, number, pcm, infos = 0, 0, [], []
    while at < len(data):
        if infos and infos[-1]["n"] != S:
            raise FlacError("a short frame that is not the last")
        x, used, info = decode_frame(data, at, fs, S, number)
        info["bytes"] = used
        pcm.append(x); infos.append(info)
        at += used; number += 1
    return (np.concatenate(pcm) if pcm else np.zeros((0, 2), np.int16)), infos


def parse_stream_header(h: bytes) -> dict:
    """the 42 bytes `fLaC` + a last STREAMINFO block, field by field"""
    if len(h) != 42 or h[:4] != b"fLaC" or h[4] != 0x80 or int.from_bytes(h[5:8], "big") != 34:
        raise FlacError("stream marker or STREAMINFO block header")
    v = int.from_bytes(h[18:26], "big")
    return dict(min_block=int.from_bytes(h[8:10], "big"), max_block=int.from_bytes(h[10:12], "big"), min_frame=int.from_bytes(h[12:15], "big"),
                max_frame=int.from_bytes(h[15:18], "big"), fs=v >> 44, channels=((v >> 41) & 7) + 1, bps=((v >> 36) & 31) + 1, total=v & ((1 << 36) - 1),
                md5=h[26:42])


# ---- signals ------------------------------------------------------------------------------------------------------------------------

def noise(n: int, level: float, seed: int) -> np.ndarray:
    """[n, 2] float32: independent gaussian noise of RMS `level` a rail"""
    return (level * np.random.default_rng(seed).standard_normal((n, 2))).astype(np.float32)


def sine(n: int, fs: float = 32000.0, f: float = 1000.0, a: float = 0.25, start: int = 0) -> np.ndarray:
    """[n, 2] float32: a sine of amplitude a on L and its quadrature on R"""
    t = (np.arange(n, dtype=np.float64) + start) / fs
    return np.stack([a * np.sin(2.0 * np.pi * f * t), a * np.cos(2.0 * np.pi * f * t)], axis=1).astype(np.float32)


def full_scale_noise(n: int, seed: int) -> np.ndarray:
    """[n, 2] float32: uniform over the whole 16-bit range"""
    return (np.random.default_rng(seed).integers(-32768, 32768, (n, 2)) / float(SCALE) * (1.0 + 1e-7)).astype(np.float32)


def signals(n: int, S: int) -> dict:
    """the named test signals, each [n, 2] float32"""
    i = np.arange(n)
    nz = noise(n, 0.01, 7)
    sq = np.where((i // 32) % 2 == 0, 1.2, -1.2)
    edge = np.linspace(-32775.0, 32775.0, n) / float(SCALE)
    burst = noise(n, 0.4, 9)
    burst[:2 * S + S // 2] = 0.0
    dither = (np.random.default_rng(11).integers(0, 2, (n, 2)) / float(SCALE) * 1.0001).astype(np.float32)     # q in {0, 1}: Rice parameter 0
    tri = (np.abs((i % 200) - 100) / 400.0)                                  # piecewise linear: second-order prediction
    par = ((i % 512) / 512.0 - 0.5) ** 2                                     # piecewise quadratic: third order
    cub = ((i % 512) / 512.0 - 0.5) ** 3 * 4.0                               # piecewise cubic: fourth order
    return {
        "silence": np.zeros((n, 2), np.float32),
        "dc": np.full((n, 2), 0.1, np.float32) * np.array([1.0, -0.5], np.float32),
        "sine": sine(n),
        "noise_m40": nz,
        "noise_full": full_scale_noise(n, 8),
        "l_eq_r": np.repeat(sine(n)[:, :1] + nz[:, :1], 2, axis=1),
        "l_eq_minus_r": (sine(n, f=440.0)[:, :1] + nz[:, :1]) * np.array([1.0, -1.0], np.float32),
        "left_only": np.stack([sine(n)[:, 0] + nz[:, 0], np.zeros(n, np.float32)], axis=1),
        "square": np.stack([sq, -sq], axis=1).astype(np.float32),
        "edge_ramp": np.stack([edge, -edge], axis=1).astype(np.float32),
        "opposite_rails": np.stack([np.full(n, 1.5), np.where(i % 7 == 0, 0.0, -1.5)], axis=1).astype(np.float32),   # L = 32767 against R = -32768
        "burst": burst,
        "dither": dither,
        "triangle": np.stack([tri, 0.5 * tri], axis=1).astype(np.float32),
        "parabola": np.stack([par, par + 0.01], axis=1).astype(np.float32),
        "cubic": np.stack([cub, -0.5 * cub], axis=1).astype(np.float32),
    }
