"""The C restatement of the audio tone detector's arithmetic contract (tests/cpp/tonedet_ref.c), built with gcc and called through
ctypes; a float64 model of the same sums as direct numpy sums; and the signals shared by tests/test_tonedet_cpu.py and
tests/test_gpu_tonedet.py."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "tonedet_ref.c"
NP, RING, NS = 64, 30, 8
NSUM = 1 + 2 * NS
DEFAULT_FREQ = (1000, 440, 400, 853, 960, 1050, 0, 0)
DEFAULT_SHARE = (3.0, 3.0, 3.0, 6.0, 6.0, 3.0, 3.0, 3.0)
# include/fmdemod.h fmd_tonedet_status
STATUS_DTYPE = np.dtype([("frames", "<u8"), ("intervals", "<u8"), ("intervals_flagged", "<u8", (NS,)), ("ring_mm", "<f8", (RING,)),
                         ("ring_pw", "<f8", (NS, RING)), ("run", "<u4", (NS,)), ("transitions", "<u4", (NS,)), ("nonfinite", "<u4"),
                         ("freq_hz", "<i4", (NS,)), ("flags", "u1"), ("ok", "u1"), ("reserved", "u1", (2,))])
assert STATUS_DTYPE.itemsize == 2344 and STATUS_DTYPE.fields["ring_mm"][1] == 80 and STATUS_DTYPE.fields["ring_pw"][1] == 320
assert STATUS_DTYPE.fields["run"][1] == 2240 and STATUS_DTYPE.fields["transitions"][1] == 2272 and STATUS_DTYPE.fields["nonfinite"][1] == 2304
assert STATUS_DTYPE.fields["freq_hz"][1] == 2308 and STATUS_DTYPE.fields["flags"][1] == 2340 and STATUS_DTYPE.fields["ok"][1] == 2341


class Params(C.Structure):
    _fields_ = [("freq_hz", C.c_int * NS), ("share_db", C.c_double * NS), ("floor_db", C.c_double), ("raise_intervals", C.c_int * NS),
                ("clear_intervals", C.c_int * NS), ("alarm_mask", C.c_uint)]


class _Status(C.Structure):
    _fields_ = [("frames", C.c_ulonglong), ("intervals", C.c_ulonglong), ("intervals_flagged", C.c_ulonglong * NS), ("ring_mm", C.c_double * RING),
                ("ring_pw", (C.c_double * RING) * NS), ("run", C.c_uint * NS), ("transitions", C.c_uint * NS), ("nonfinite", C.c_uint),
                ("freq_hz", C.c_int * NS), ("flags", C.c_ubyte), ("ok", C.c_ubyte), ("reserved", C.c_ubyte * 2)]


class _Chan(C.Structure):
    _fields_ = [("st", _Status), ("prm", Params), ("fs", C.c_int), ("M", C.c_int), ("tab", C.c_void_p), ("min_e", C.c_double), ("c", C.c_double * NS),
                ("p", (C.c_double * NP) * NSUM), ("out_flags", C.c_ubyte), ("out_ok", C.c_ubyte)]


assert C.sizeof(_Status) == 2344 and C.sizeof(Params) == 176

_ARRAYS = {"freq_hz": (C.c_int, int), "share_db": (C.c_double, float), "raise_intervals": (C.c_int, int), "clear_intervals": (C.c_int, int)}


def params_tuple(p) -> tuple:
    """every field of a Params-shaped structure (the 4 bytes of padding behind alarm_mask are not part of it)"""
    return (tuple(p.freq_hz), tuple(p.share_db), p.floor_db, tuple(p.raise_intervals), tuple(p.clear_intervals), p.alarm_mask)


def _apply(p, fields):
    for k, v in fields.items():
        if k in _ARRAYS:
            ct, py = _ARRAYS[k]
            v = (ct * NS)(*([py(v)] * NS if np.isscalar(v) else [py(a) for a in v]))
        elif k not in dict(Params._fields_):
            raise TypeError(k)
        setattr(p, k, v)


class Channel:
    """one station of the restatement: process(x [n, 2] float32) as often as wanted, then status(), flags, ok and the read-outs"""

    def __init__(self, ref, fs: int):
        self.lib, self.fs = ref.lib, int(fs)
        self.c = _Chan()
        self._tab = ref.table(fs) if 8000 <= fs <= 48000 and fs % 10 == 0 else np.zeros((1, 2))
        if self.lib.tonedet_ref_create(C.byref(self.c), int(fs), self._tab.ctypes.data_as(C.c_void_p)) != 0:
            raise ValueError(f"fs {fs}")

    def process(self, x):
        x = np.ascontiguousarray(x)
        assert x.ndim == 2 and x.shape[1] == 2 and x.dtype == np.float32
        self.lib.tonedet_ref_process(C.byref(self.c), x.ctypes.data_as(C.c_void_p), x.shape[0])
        return self

    def set_params(self, **fields) -> int:
        """0, or -1 where the restatement rejects the values (nothing changes then); the per-slot fields take eight values or one for all"""
        p = Params.from_buffer_copy(bytes(self.c.prm))
        _apply(p, fields)
        return self.lib.tonedet_ref_set_params(C.byref(self.c), C.byref(p))

    def reset(self):
        self.lib.tonedet_ref_reset(C.byref(self.c))

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

    def partials(self) -> np.ndarray:
        """the open interval's [17, 64] partials (a copy)"""
        return np.ctypeslib.as_array(self.c.p).copy()

    def thresholds(self) -> tuple:
        return (self.c.min_e,) + tuple(self.c.c)

    def _read(self, fn, slot, window):
        out = C.c_double(0.0)
        rc = getattr(self.lib, fn)(C.byref(self.c.st), self.fs, int(slot), int(window), C.byref(out))
        return out.value if rc == 0 else None

    def share_db(self, slot: int, window: int = 1):
        return self._read("tonedet_ref_share_db", slot, window)

    def level_db(self, slot: int, window: int = 1):
        return self._read("tonedet_ref_level_db", slot, window)


class Ref:
    def __init__(self, lib):
        self.lib = lib
        self._tables = {}

    def table(self, fs: int) -> np.ndarray:
        """[fs, 2] float64: the restatement's cos and sin of 2 pi j / fs (computed once per rate)"""
        if fs not in self._tables:
            t = np.zeros((fs, 2), np.float64)
            self.lib.tonedet_ref_table(int(fs), t.ctypes.data_as(C.c_void_p))
            self._tables[fs] = t
        return self._tables[fs]

    def channel(self, fs: int, **params) -> Channel:
        ch = Channel(self, fs)
        if params:
            assert ch.set_params(**params) == 0
        return ch

    def run(self, fs: int, x, **params) -> Channel:
        """a fresh station (with these parameters) fed x [n, 2] in one piece"""
        return self.channel(fs, **params).process(x)

    def default_params(self) -> Params:
        p = Params()
        self.lib.tonedet_ref_default_params(C.byref(p))
        return p

    def readout(self, fn: str, record, fs: int, slot: int, window: int):
        """(rc, value) of tonedet_ref_share_db / tonedet_ref_level_db over one record"""
        r = np.ascontiguousarray(record, STATUS_DTYPE).reshape(-1)
        out = C.c_double(0.0)
        rc = getattr(self.lib, fn)(r.ctypes.data_as(C.c_void_p), int(fs), int(slot), int(window), C.byref(out))
        return rc, out.value


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "libtonedet_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.tonedet_ref_create.argtypes = [C.POINTER(_Chan), C.c_int, C.c_void_p]
    lib.tonedet_ref_table.argtypes = [C.c_int, C.c_void_p]
    lib.tonedet_ref_table.restype = None
    lib.tonedet_ref_default_params.argtypes = [C.POINTER(Params)]
    lib.tonedet_ref_default_params.restype = None
    lib.tonedet_ref_set_params.argtypes = [C.POINTER(_Chan), C.POINTER(Params)]
    lib.tonedet_ref_reset.argtypes = [C.POINTER(_Chan)]
    lib.tonedet_ref_reset.restype = None
    lib.tonedet_ref_process.argtypes = [C.POINTER(_Chan), C.c_void_p, C.c_longlong]
    lib.tonedet_ref_process.restype = None
    for fn in ("tonedet_ref_share_db", "tonedet_ref_level_db"):
        getattr(lib, fn).argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    return Ref(lib)


def bits(a) -> np.ndarray:
    """an array's bytes (status records, float64 and float32 arrays compare bit for bit, NaNs and signed zeros included)"""
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


# ---- the float64 model ----------------------------------------------------------------------------------------------------------

def model_table(fs: int) -> np.ndarray:
    """[fs, 2]: numpy's cos and sin of 2 pi j / fs"""
    a = 2.0 * np.pi * np.arange(fs, dtype=np.float64) / float(fs)
    return np.stack([np.cos(a), np.sin(a)], axis=1)


def model_interval(fs: int, x: np.ndarray, freqs) -> dict:
    """an interval's first frames x [n <= M, 2] float32 as direct numpy sums: MM, RE [8], IM [8], PW [8], and abs_m = sum |m|, abs_mm = sum m^2, the sums
    of the terms' magnitudes that the error bound of a sum is made of"""
    M = fs // 10
    assert x.ndim == 2 and x.shape[0] <= M and x.shape[1] == 2
    m = x[:, 0].astype(np.float64) + x[:, 1].astype(np.float64)
    tab = model_table(fs)
    r = np.arange(x.shape[0], dtype=np.int64)
    RE, IM = np.zeros(NS), np.zeros(NS)
    for k, f in enumerate(freqs):
        if f:
            idx = (int(f) * r) % fs
            RE[k] = np.sum(m * tab[idx, 0])
            IM[k] = np.sum(m * tab[idx, 1])
    MM = float(np.sum(m * m))
    return {"MM": MM, "RE": RE, "IM": IM, "PW": RE * RE + IM * IM, "abs_m": float(np.sum(np.abs(m))), "abs_mm": MM}


def model_shares(fs: int, x: np.ndarray, freqs) -> list:
    """per whole interval of x [n, 2]: (level_db of the mid signal = 10 log10(MM / M), [share_db per slot]) in float64, -inf where a
    slot is unused or carries nothing"""
    M = fs // 10
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for g in range(x.shape[0] // M):
            iv = model_interval(fs, x[g * M:(g + 1) * M], freqs)
            share = [float(10.0 * np.log10(np.float64(2.0 * iv["PW"][k]) / np.float64(M * iv["MM"]))) if f and iv["MM"] > 0 else -math.inf
                     for k, f in enumerate(freqs)]
            out.append((float(10.0 * np.log10(np.float64(iv["MM"]) / M)), share))
    return out


# ---- signals --------------------------------------------------------------------------------------------------------------------

# the detector sequence with 3 intervals to raise and 2 to clear on the default slots: (condition, intervals).  t1000 x 2 is a run one
# interval short of raising; the EAS pair raises slots 3 and 4 together; a tone under the floor ("quiet") and zeros carry no tone and
# clear like noise; behind t400 x 3 the three intervals of t1000 clear slot 2 at the second and raise slot 0 at the third.
SEQ_PATTERN = (("noise", 2), ("t1000", 2), ("noise", 1), ("t1000", 3), ("noise", 2), ("eas", 3), ("quiet", 2), ("t440", 3), ("zeros", 2),
               ("t1050", 4), ("noise", 2), ("t400", 3), ("t1000", 3), ("noise", 2))
SEQ_PARAMS = dict(raise_intervals=3, clear_intervals=2)
SEQ_SEED = 20261020
SEQ_A = 0.25                                                      # -12 dBFS a rail
# the frequencies a condition is made of, and the slots (of the default set) it makes present
SEQ_TONES = {"noise": (), "zeros": (), "t1000": (1000,), "t440": (440,), "t400": (400,), "t1050": (1050,), "eas": (853, 960), "quiet": (1000,)}
SEQ_PRESENT = {"noise": (), "zeros": (), "quiet": (), "t1000": (0,), "t440": (1,), "t400": (2,), "eas": (3, 4), "t1050": (5,)}


def seq_conditions(lead: int = 0, total: int | None = None) -> list:
    """the pattern's condition per interval behind `lead` noise intervals, continued as noise up to `total` intervals"""
    cd = ["noise"] * lead + [c for c, k in SEQ_PATTERN for _ in range(k)]
    return cd + ["noise"] * (0 if total is None else total - len(cd))


def expected_flags(conditions, raise_intervals=3, clear_intervals=2) -> tuple:
    """the flags after every interval for intervals that read their nominal condition: (flags, transitions [8])"""
    flag, run, tr, out = [False] * NS, [0] * NS, [0] * NS, []
    for cd in conditions:
        for k in range(NS):
            b = k in SEQ_PRESENT[cd]
            if not flag[k]:
                run[k] = run[k] + 1 if b else 0
                if run[k] >= raise_intervals:
                    flag[k], run[k], tr[k] = True, 0, tr[k] + 1
            else:
                run[k] = 0 if b else run[k] + 1
                if run[k] >= clear_intervals:
                    flag[k], run[k], tr[k] = False, 0, tr[k] + 1
        out.append(sum(int(f) << k for k, f in enumerate(flag)))
    return out, tr


def condition_frames(cd: str, fs: int, m: int, rng, a: float = SEQ_A) -> np.ndarray:
    """[m, 2] float64 of one condition: its tones share the power of one sine of amplitude a, each from a phase of its own, on both
    rails alike, under independent noise 40 dB down a rail (noise: Gaussian at a / 2 a rail, half of it common to both rails)"""
    n1, n2 = rng.standard_normal(m), rng.standard_normal(m)
    ph = rng.uniform(0.0, 2.0 * np.pi, 2)
    if cd == "zeros":
        return np.zeros((m, 2))
    if cd == "noise":
        return np.stack([0.5 * a * n1, 0.5 * a * (0.6 * n1 + 0.8 * n2)], axis=1)
    tones = SEQ_TONES[cd]
    amp = (1e-4 if cd == "quiet" else a) / math.sqrt(len(tones))
    t = np.arange(m, dtype=np.float64) / float(fs)
    s = sum(amp * np.sin(2.0 * np.pi * f * t + ph[i]) for i, f in enumerate(tones))
    return np.stack([s + 0.01 * amp * n1, s + 0.01 * amp * n2], axis=1)


def seq_signal(fs: int, scale: float = 1.0, seed: int = SEQ_SEED, lead: int = 0, total: int | None = None, tail: int = 0) -> np.ndarray:
    """[n, 2] float64, n = intervals * M + tail: the condition of seq_conditions(lead, total) per whole interval, so that no interval
    mixes two conditions, and `tail` frames of an open 1000 Hz interval behind them, all times `scale`"""
    M = fs // 10
    rng = np.random.default_rng(seed)
    parts = [condition_frames(c, fs, M, rng) for c in seq_conditions(lead, total)]
    if tail:
        parts.append(condition_frames("t1000", fs, tail, rng))
    return scale * np.concatenate(parts)


def check_margins(fs: int, x: np.ndarray, conditions, freqs=DEFAULT_FREQ, share_db=DEFAULT_SHARE, floor_db=-50.0) -> dict:
    """asserts in float64 that every interval of x is far from every threshold: the mid signal's level 10 dB from the floor, a slot
    whose tone is on 2.5 dB above its share threshold (a sole sine reads 0 dB against the default -3, each of the EAS pair -3 against
    -6: there is no more room) and every other slot 10 dB below its own; returns the worst figures seen per kind"""
    fig = model_shares(fs, x, freqs)
    assert len(fig) >= len(conditions)
    worst = {}

    def note(key, v, pick):
        worst[key] = v if key not in worst else pick(worst[key], v)

    for g, cd in enumerate(conditions):
        level, share = fig[g]
        if cd in ("zeros", "quiet"):
            assert level < floor_db - 10.0, (g, cd, level)
            note("unusable level max", level, max)
            continue
        assert level > floor_db + 10.0, (g, cd, level)
        note("usable level min", level, min)
        for k, f in enumerate(freqs):
            if not f:
                continue
            if k in SEQ_PRESENT[cd]:
                assert share[k] > -share_db[k] + 2.5, (g, cd, k, share[k])
                note("present share min over threshold", share[k] + share_db[k], min)
            else:
                assert share[k] < -share_db[k] - 10.0, (g, cd, k, share[k])
                note("absent share max over threshold", share[k] + share_db[k], max)
    return worst
