"""The C restatement of the EAS SAME decoder's arithmetic contract (tests/cpp/same_ref.c), built with gcc and called through ctypes; a
float64 model of the same decoder as plain numpy sums; and the signals shared by tests/test_same_cpu.py and tests/test_gpu_same.py."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "same_ref.c"
MAXB, RING, HIST, PERIOD = 268, 8, 7, 12500
SYNCED, ALERT_OPEN = 1, 2
KIND_HEADER, KIND_EOM = 1, 2
TICKS_PER_SECOND = 12500.0 / 3.0
# include/fmdemod.h fmd_same_message and fmd_same_status
MESSAGE_DTYPE = np.dtype([("sync_tick", "<u8"), ("len", "<u2"), ("kind", "u1"), ("reserved", "u1"), ("bytes", "u1", (MAXB,))])
STATUS_DTYPE = np.dtype([("frames", "<u8"), ("ticks", "<u8"), ("bits", "<u8"), ("syncs", "<u8"), ("accepted", "<u8"), ("rejected", "<u8"),
                         ("sync_tick", "<u8"), ("last_accept_tick", "<u8"), ("open", "<f8", (4,)), ("hist", "<f8", (HIST, 4)), ("ph", "<u4"),
                         ("sh", "<u4"), ("nbit", "<u4"), ("msg_len", "<u4"), ("run", "<u4"), ("synced", "u1"), ("prev_s", "u1"), ("flags", "u1"),
                         ("ok", "u1"), ("msg", "u1", (MAXB,)), ("reserved", "u1", (4,)), ("ring", MESSAGE_DTYPE, (RING,))])
OFFSETS = {"frames": 0, "ticks": 8, "bits": 16, "syncs": 24, "accepted": 32, "rejected": 40, "sync_tick": 48, "last_accept_tick": 56, "open": 64,
           "hist": 96, "ph": 320, "sh": 324, "nbit": 328, "msg_len": 332, "run": 336, "synced": 340, "prev_s": 341, "flags": 342, "ok": 343, "msg": 344, "ring": 616}
assert MESSAGE_DTYPE.itemsize == 280 and STATUS_DTYPE.itemsize == 2856
assert all(STATUS_DTYPE.fields[k][1] == v for k, v in OFFSETS.items())

HEADER56 = b"ZCZC-WXR-TOR-039173-039051-039035+0030-1051700-KCLE/NWS-"
HEADER24 = b"ZCZC-EAS-RWT-012345+0015-"                    # a short one (no time, no call sign): about 5 000 frames a burst at 8 kHz
EOM = b"NNNN"
assert len(HEADER56) == 56 and len(HEADER24) == 25


class Params(C.Structure):
    _fields_ = [("pull", C.c_int), ("hold_ticks", C.c_uint), ("alarm_mask", C.c_uint), ("reserved", C.c_uint)]


class _Message(C.Structure):
    _fields_ = [("sync_tick", C.c_ulonglong), ("len", C.c_ushort), ("kind", C.c_ubyte), ("reserved", C.c_ubyte), ("bytes", C.c_ubyte * MAXB)]


class _Status(C.Structure):
    _fields_ = [("frames", C.c_ulonglong), ("ticks", C.c_ulonglong), ("bits", C.c_ulonglong), ("syncs", C.c_ulonglong), ("accepted", C.c_ulonglong),
                ("rejected", C.c_ulonglong), ("sync_tick", C.c_ulonglong), ("last_accept_tick", C.c_ulonglong), ("open", C.c_double * 4),
                ("hist", (C.c_double * 4) * HIST), ("ph", C.c_uint), ("sh", C.c_uint), ("nbit", C.c_uint), ("msg_len", C.c_uint), ("run", C.c_uint),
                ("synced", C.c_ubyte), ("prev_s", C.c_ubyte), ("flags", C.c_ubyte), ("ok", C.c_ubyte), ("msg", C.c_ubyte * MAXB), ("reserved", C.c_ubyte * 4), ("ring", _Message * RING)]


class _Chan(C.Structure):
    _fields_ = [("st", _Status), ("prm", Params), ("fs", C.c_int), ("P", C.c_int), ("mark_step", C.c_int), ("space_step", C.c_int), ("tab", C.c_void_p),
                ("out_flags", C.c_ubyte), ("out_ok", C.c_ubyte)]


class EncodeConfig(C.Structure):
    _fields_ = [("fs", C.c_int), ("repeats", C.c_int), ("gap_frames", C.c_longlong), ("clock_ratio", C.c_double), ("amplitude", C.c_double),
                ("mark_db", C.c_double)]


assert C.sizeof(_Status) == 2856 and C.sizeof(Params) == 16 and C.sizeof(_Message) == 280 and C.sizeof(EncodeConfig) == 40


def params_tuple(p) -> tuple:
    return (p.pull, p.hold_ticks, p.alarm_mask, p.reserved)


def ring_messages(record, since: int = 0) -> list:
    """the accepted messages number `since` ... of one STATUS_DTYPE record, oldest first, as (sync_tick, kind, bytes); those the ring has
    lost are left out"""
    acc = int(record["accepted"])
    out = []
    for k in range(max(since, acc - RING), acc):
        r = record["ring"][k % RING]
        out.append((int(r["sync_tick"]), int(r["kind"]), bytes(r["bytes"][:int(r["len"])])))
    return out


class Channel:
    """one station of the restatement: process(x [n, 2] float32) as often as wanted, then status(), flags, ok"""

    def __init__(self, ref, fs: int):
        self.lib, self.fs = ref.lib, int(fs)
        self.c = _Chan()
        self._tab = ref.table(fs) if 8000 <= fs <= 48000 and fs % 10 == 0 else np.zeros((1, 2))
        if self.lib.same_ref_create(C.byref(self.c), int(fs), self._tab.ctypes.data_as(C.c_void_p)) != 0:
            raise ValueError(f"fs {fs}")

    def process(self, x):
        x = np.ascontiguousarray(x)
        assert x.ndim == 2 and x.shape[1] == 2 and x.dtype == np.float32
        self.lib.same_ref_process(C.byref(self.c), x.ctypes.data_as(C.c_void_p), x.shape[0])
        return self

    def set_params(self, **fields) -> int:
        """0, or -1 where the restatement rejects the values (nothing changes then)"""
        p = Params.from_buffer_copy(bytes(self.c.prm))
        for k, v in fields.items():
            if k not in dict(Params._fields_):
                raise TypeError(k)
            setattr(p, k, v)
        return self.lib.same_ref_set_params(C.byref(self.c), C.byref(p))

    def reset(self):
        self.lib.same_ref_reset(C.byref(self.c))

    @property
    def flags(self) -> int:
        """the station's flags byte as of the last process call (0xAA before the first)"""
        return int(self.c.out_flags)

    @property
    def ok(self) -> int:
        return int(self.c.out_ok)

    def status(self) -> np.ndarray:
        """a [1] STATUS_DTYPE record array (a copy)"""
        return np.frombuffer(bytes(self.c.st), STATUS_DTYPE).copy()

    def messages(self, since: int = 0) -> list:
        return ring_messages(self.status()[0], since)


class Ref:
    def __init__(self, lib):
        self.lib = lib
        self._tables = {}

    def geometry(self, fs: int):
        """(P, mark step, space step), or None for a rate outside the contract"""
        v = [C.c_int(0) for _ in range(3)]
        return tuple(a.value for a in v) if self.lib.same_ref_geometry(int(fs), *(C.byref(a) for a in v)) == 0 else None

    def table(self, fs: int) -> np.ndarray:
        """[P, 2] float64: the restatement's cos and sin of 2 pi j / P (computed once per rate)"""
        if fs not in self._tables:
            P = self.geometry(fs)[0]
            t = np.zeros((P, 2), np.float64)
            self.lib.same_ref_table(P, t.ctypes.data_as(C.c_void_p))
            self._tables[fs] = t
        return self._tables[fs]

    def tick_starts(self, fs: int) -> np.ndarray:
        return np.array([self.lib.same_ref_tick_start(int(fs), r) for r in range(PERIOD + 1)], np.int64)

    def channel(self, fs: int, **params) -> Channel:
        ch = Channel(self, fs)
        if params:
            assert ch.set_params(**params) == 0
        return ch

    def run(self, fs: int, x, **params) -> Channel:
        return self.channel(fs, **params).process(x)

    def default_params(self) -> Params:
        p = Params()
        self.lib.same_ref_default_params(C.byref(p))
        return p

    def encode(self, text: bytes, fs: int, clock_ratio=1.0, amplitude=0.25, repeats=3, gap_frames=-1, mark_db=0.0):
        """[n, 2] float32, or None where the restatement rejects the values"""
        cfg = EncodeConfig(int(fs), int(repeats), int(gap_frames), float(clock_ratio), float(amplitude), float(mark_db))
        n = self.lib.same_ref_encode(C.byref(cfg), text, len(text), None)
        if n < 0:
            return None
        out = np.zeros((n, 2), np.float32)
        assert self.lib.same_ref_encode(C.byref(cfg), text, len(text), out.ctypes.data_as(C.c_void_p)) == n
        return out


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "libsame_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.same_ref_geometry.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.same_ref_table.argtypes = [C.c_int, C.c_void_p]
    lib.same_ref_table.restype = None
    lib.same_ref_tick_start.argtypes = [C.c_int, C.c_uint]
    lib.same_ref_tick_start.restype = C.c_uint
    lib.same_ref_default_params.argtypes = [C.POINTER(Params)]
    lib.same_ref_default_params.restype = None
    lib.same_ref_create.argtypes = [C.POINTER(_Chan), C.c_int, C.c_void_p]
    lib.same_ref_set_params.argtypes = [C.POINTER(_Chan), C.POINTER(Params)]
    lib.same_ref_reset.argtypes = [C.POINTER(_Chan)]
    lib.same_ref_reset.restype = None
    lib.same_ref_process.argtypes = [C.POINTER(_Chan), C.c_void_p, C.c_longlong]
    lib.same_ref_process.restype = None
    lib.same_ref_encode.argtypes = [C.POINTER(EncodeConfig), C.c_char_p, C.c_int, C.c_void_p]
    lib.same_ref_encode.restype = C.c_longlong
    return Ref(lib)


def bits(a) -> np.ndarray:
    """an array's bytes (status records and float arrays compare bit for bit, NaNs and signed zeros included)"""
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


# ---- the float64 model ----------------------------------------------------------------------------------------------------------

def model_decode(fs: int, x: np.ndarray, pull: int = 16) -> dict:
    """x [n, 2] float32 from a reset, as plain numpy sums: per whole tick the four sums by np.add.reduceat over numpy's own cos and sin of the
    exact phase 2 pi (4 or 3) i 3125 / (6 fs) (no table), the window sums as eight shifted arrays added up, then the contract's clock and
    framer.  Returns the decisions per tick and their |E1 - E0| / (E1 + E0), the clock's bits, those taken while synchronised as (tick, bit), every ended message as (sync_tick, accepted, bytes), and `margin`, the
    smallest |E1 - E0| / (E1 + E0) met at a tick where the clock took a bit while the framer was synchronised and a burst was on (E1 + E0 above
    a hundredth of its maximum)."""
    m = x[:, 0].astype(np.float64) + x[:, 1].astype(np.float64)
    n = m.shape[0]
    nt = 0
    while (3 * fs * (nt + 1) + 12499) // 12500 <= n:
        nt += 1
    B = np.array([(3 * fs * k + 12499) // 12500 for k in range(nt + 1)], np.int64)
    i = np.arange(B[-1], dtype=np.float64)
    sums = []
    for cyc in (4.0, 3.0):
        a = 2.0 * np.pi * np.mod(i * (cyc * 3125.0), 6.0 * fs) / (6.0 * fs)
        for t in (np.cos(a), np.sin(a)):
            s = np.add.reduceat(m[:B[-1]] * t, B[:-1]) if nt else np.zeros(0)
            sp = np.concatenate([np.zeros(7), s])
            sums.append(sum(sp[j:j + nt] for j in range(8)) if nt else s)   # ticks k - 7 ... k (nothing before the start)
    e1, e0 = sums[0] ** 2 + sums[1] ** 2, sums[2] ** 2 + sums[3] ** 2
    dec = (e1 > e0).astype(np.uint8)
    with np.errstate(all="ignore"):
        rel = np.abs(e1 - e0) / (e1 + e0)
    loud = (e1 + e0) > 0.01 * float(np.max(e1 + e0)) if nt else np.zeros(0, bool)   # a burst is on (its tail's noise bytes are not the point)
    ph = sh = nbit = prev = run = 0
    synced = False
    msg, out_bits, locked_bits, messages, margin, sync_tick = bytearray(), [], [], [], math.inf, 0
    for k in range(nt):
        s = int(dec[k])
        if s != prev:
            nb = (run + 4) >> 3
            if nb >= 1 and run <= 96:
                err = (ph - 16 * run - (0 if nb & 1 else 128)) & 255
                ph = (ph - min(pull, err)) & 255 if err < 128 else (ph + min(pull, 256 - err)) & 255
            run = 0
        run = min(run + 1, 255)
        prev = s
        ph += 32
        if ph >= 256:
            ph -= 256
            out_bits.append(s)
            sh = (sh >> 1) | (s << 15)
            if synced:
                locked_bits.append((k, s))
                if loud[k]:
                    margin = min(margin, float(rel[k]))
            if not synced:
                if sh == 0xABAB:
                    synced, nbit, msg, sync_tick = True, 0, bytearray(), k
            else:
                nbit += 1
                if nbit == 8:
                    nbit = 0
                    b = sh >> 8
                    if not (b == 0xAB and not msg):
                        valid = 0x20 <= b <= 0x7E or b in (0x0D, 0x0A)
                        if valid:
                            msg.append(b)
                        if not valid or len(msg) == MAXB:
                            messages.append((sync_tick, bytes(msg[:4]) in (b"ZCZC", b"NNNN"), bytes(msg)))
                            synced = False
    return {"decisions": dec, "rel": rel, "bits": out_bits, "locked_bits": locked_bits, "messages": messages, "margin": margin, "ticks": nt}


# ---- signals --------------------------------------------------------------------------------------------------------------------

def burst_power(amplitude: float) -> float:
    """the mean square of a burst's rail: a sine of that amplitude (mark and space alike at mark_db = 0)"""
    return 0.5 * amplitude * amplitude


def add_noise(x: np.ndarray, amplitude: float, db_below: float, seed: int) -> np.ndarray:
    """x [n, 2] float32 plus white Gaussian noise, the same in both rails as the burst is, `db_below` dB below the burst's power"""
    rng = np.random.default_rng(seed)
    sigma = math.sqrt(burst_power(amplitude) * 10.0 ** (-db_below / 10.0))
    w = (sigma * rng.standard_normal(x.shape[0])).astype(np.float32)
    return (x + w[:, None]).astype(np.float32)
