"""The C restatement of the audio fault monitor's arithmetic contract (tests/cpp/audmon_ref.c), built with gcc and called through
ctypes; a float64 model of the same contract in plain Python loops (every fma evaluated exactly and rounded once); and the signals
shared by tests/test_audmon_cpu.py and tests/test_gpu_audmon.py."""
import ctypes as C
import math
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "cpp" / "audmon_ref.c"
NP, RING, ND = 64, 30, 5
SILENCE, LEFT_LOST, RIGHT_LOST, ANTIPHASE, MONO = 1, 2, 4, 8, 16
# include/fmdemod.h fmd_audmon_status
STATUS_DTYPE = np.dtype([("frames", "<u8"), ("intervals", "<u8"), ("intervals_flagged", "<u8", (ND,)), ("ring_ll", "<f8", (RING,)),
                         ("ring_rr", "<f8", (RING,)), ("ring_lr", "<f8", (RING,)), ("last_peak", "<f4", (2,)), ("hold_peak", "<f4", (2,)),
                         ("run", "<u4", (ND,)), ("transitions", "<u4", (ND,)), ("nonfinite", "<u4"), ("flags", "u1"), ("ok", "u1"),
                         ("reserved", "u1", (2,))])
assert STATUS_DTYPE.itemsize == 840 and STATUS_DTYPE.fields["ring_ll"][1] == 56 and STATUS_DTYPE.fields["ring_rr"][1] == 296
assert STATUS_DTYPE.fields["ring_lr"][1] == 536 and STATUS_DTYPE.fields["last_peak"][1] == 776 and STATUS_DTYPE.fields["run"][1] == 792
assert STATUS_DTYPE.fields["transitions"][1] == 812 and STATUS_DTYPE.fields["nonfinite"][1] == 832 and STATUS_DTYPE.fields["flags"][1] == 836


class Params(C.Structure):
    _fields_ = [("silence_db", C.c_double), ("loss_db", C.c_double), ("antiphase_corr", C.c_double), ("mono_db", C.c_double),
                ("raise_intervals", C.c_int * ND), ("clear_intervals", C.c_int * ND), ("alarm_mask", C.c_uint)]


class _Status(C.Structure):
    _fields_ = [("frames", C.c_ulonglong), ("intervals", C.c_ulonglong), ("intervals_flagged", C.c_ulonglong * ND), ("ring_ll", C.c_double * RING),
                ("ring_rr", C.c_double * RING), ("ring_lr", C.c_double * RING), ("last_peak", C.c_float * 2), ("hold_peak", C.c_float * 2),
                ("run", C.c_uint * ND), ("transitions", C.c_uint * ND), ("nonfinite", C.c_uint), ("flags", C.c_ubyte), ("ok", C.c_ubyte),
                ("reserved", C.c_ubyte * 2)]


class _Chan(C.Structure):
    _fields_ = [("st", _Status), ("prm", Params), ("M", C.c_int), ("min_e", C.c_double), ("c_loss", C.c_double), ("c_anti", C.c_double),
                ("c_mono", C.c_double), ("pk", C.c_float * 2), ("p", (C.c_double * NP) * 3), ("out_flags", C.c_ubyte), ("out_ok", C.c_ubyte)]


assert C.sizeof(_Status) == 840 and C.sizeof(Params) == 80


def params_tuple(p) -> tuple:
    """every field of a Params-shaped structure (the 4 bytes of padding behind alarm_mask are not part of it)"""
    return (p.silence_db, p.loss_db, p.antiphase_corr, p.mono_db, tuple(p.raise_intervals), tuple(p.clear_intervals), p.alarm_mask)


def _apply(p, fields):
    for k, v in fields.items():
        if k in ("raise_intervals", "clear_intervals"):
            v = (C.c_int * ND)(*([int(v)] * ND if np.isscalar(v) else [int(a) for a in v]))
        setattr(p, k, v)


class Channel:
    """one station of the restatement: process(x [n, 2] float32) as often as wanted, then status(), flags, ok and the read-outs"""

    def __init__(self, ref, fs: int):
        self.lib, self.fs = ref.lib, int(fs)
        self.c = _Chan()
        if self.lib.audmon_ref_create(C.byref(self.c), int(fs)) != 0:
            raise ValueError(f"fs {fs}")

    def process(self, x):
        x = np.ascontiguousarray(x)
        assert x.ndim == 2 and x.shape[1] == 2 and x.dtype == np.float32
        self.lib.audmon_ref_process(C.byref(self.c), x.ctypes.data_as(C.c_void_p), x.shape[0])
        return self

    def set_params(self, **fields) -> int:
        """0, or -1 where the restatement rejects the values (nothing changes then); raise_intervals and clear_intervals take five values
        or one for all five"""
        p = Params.from_buffer_copy(bytes(self.c.prm))
        _apply(p, fields)
        return self.lib.audmon_ref_set_params(C.byref(self.c), C.byref(p))

    def reset(self):
        self.lib.audmon_ref_reset(C.byref(self.c))

    def reset_peaks(self):
        self.lib.audmon_ref_reset_peaks(C.byref(self.c))

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

    def _read(self, fn, *args):
        out = C.c_double(0.0)
        rc = getattr(self.lib, fn)(C.byref(self.c.st), self.fs, *[C.c_int(a) for a in args], C.byref(out))
        return out.value if rc == 0 else None

    def level_db(self, rail: int = 2, window: int = 1):
        return self._read("audmon_ref_level_db", rail, window)

    def balance_db(self, window: int = 1):
        return self._read("audmon_ref_balance_db", window)

    def correlation(self, window: int = 1):
        return self._read("audmon_ref_correlation", window)

    def side_mid_db(self, window: int = 1):
        return self._read("audmon_ref_side_mid_db", window)


class Ref:
    def __init__(self, lib):
        self.lib = lib

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
        self.lib.audmon_ref_default_params(C.byref(p))
        return p

    def readout(self, fn: str, record, fs: int, *args):
        """(rc, value) of audmon_ref_level_db (rail, window) / _balance_db / _correlation / _side_mid_db (window) over one record"""
        r = np.ascontiguousarray(record, STATUS_DTYPE).reshape(-1)
        out = C.c_double(0.0)
        rc = getattr(self.lib, fn)(r.ctypes.data_as(C.c_void_p), int(fs), *[C.c_int(a) for a in args], C.byref(out))
        return rc, out.value


def build(tmp_dir: Path) -> Ref:
    so = Path(tmp_dir) / "libaudmon_ref.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.audmon_ref_create.argtypes = [C.POINTER(_Chan), C.c_int]
    lib.audmon_ref_default_params.argtypes = [C.POINTER(Params)]
    lib.audmon_ref_default_params.restype = None
    lib.audmon_ref_set_params.argtypes = [C.POINTER(_Chan), C.POINTER(Params)]
    for fn in ("audmon_ref_reset", "audmon_ref_reset_peaks"):
        getattr(lib, fn).argtypes = [C.POINTER(_Chan)]
        getattr(lib, fn).restype = None
    lib.audmon_ref_process.argtypes = [C.POINTER(_Chan), C.c_void_p, C.c_longlong]
    lib.audmon_ref_process.restype = None
    lib.audmon_ref_level_db.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    for fn in ("audmon_ref_balance_db", "audmon_ref_correlation", "audmon_ref_side_mid_db"):
        getattr(lib, fn).argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
    return Ref(lib)


def bits(a) -> np.ndarray:
    """an array's bytes (status records, float64 and float32 arrays compare bit for bit, NaNs and signed zeros included)"""
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


# ---- the float64 model ----------------------------------------------------------------------------------------------------------

def _fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (finite operands): exact in rationals, and float() of a Fraction rounds to nearest even"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def model_thresholds(M: int, silence_db=-60.0, loss_db=30.0, antiphase_corr=0.5, mono_db=40.0) -> tuple:
    """(min_e, c_loss, c_anti, c_mono)"""
    min_e = 0.0 if silence_db == -math.inf else math.pow(10.0, silence_db / 10.0) * (2.0 * float(M))
    return min_e, math.pow(10.0, -loss_db / 10.0), antiphase_corr * antiphase_corr, math.pow(10.0, -mono_db / 10.0)


def model_run(fs: int, x: np.ndarray, raise_intervals=3, clear_intervals=2, **thresholds) -> dict:
    """a fresh station fed x [n, 2] float32 (finite samples), frame after frame, every detector with the same two run lengths.
    {"intervals": [per completed interval a dict of LL, RR, LR, pk, bad, flags, run, transitions, flagged], "hold_peak", "pk" (the open
    interval's), "part": the open interval's [3][64] partials}"""
    M = fs // 10
    min_e, c_loss, c_anti, c_mono = model_thresholds(M, **thresholds)
    part = [[0.0] * NP for _ in range(3)]
    pk, hold = [0.0, 0.0], [0.0, 0.0]
    flag, run, trans, flagged = [False] * ND, [0] * ND, [0] * ND, [0] * ND
    out = {"intervals": []}
    for n in range(x.shape[0]):
        r = n % M
        j = (r >> 2) & 63
        L, R = float(x[n, 0]), float(x[n, 1])
        part[0][j] = _fma(L, L, part[0][j])
        part[1][j] = _fma(R, R, part[1][j])
        part[2][j] = _fma(L, R, part[2][j])
        pk = [max(pk[0], abs(L)), max(pk[1], abs(R))]
        hold = [max(hold[0], abs(L)), max(hold[1], abs(R))]
        if r + 1 == M:
            S = []
            for q in part:
                w = NP // 2
                while w >= 1:
                    for jj in range(w):
                        q[jj] += q[jj + w]
                    w //= 2
                S.append(q[0])
            LL, RR, LR = S
            E = LL + RR
            bad = [not (all(math.isfinite(v) for v in S) and E > min_e)] + [None] * 4
            if not bad[0]:
                Sd, Md = _fma(-2.0, LR, E), _fma(2.0, LR, E)
                bad[1:] = [LL < c_loss * RR, RR < c_loss * LL, LR < 0.0 and LR * LR > c_anti * (LL * RR), Sd < c_mono * Md]
            for k in range(ND):
                if bad[k] is None:
                    continue                                     # held
                if not flag[k]:
                    run[k] = run[k] + 1 if bad[k] else 0
                    if run[k] >= raise_intervals:
                        flag[k], run[k], trans[k] = True, 0, trans[k] + 1
                else:
                    run[k] = 0 if bad[k] else run[k] + 1
                    if run[k] >= clear_intervals:
                        flag[k], run[k], trans[k] = False, 0, trans[k] + 1
            for k in range(ND):
                flagged[k] += int(flag[k])
            out["intervals"].append({"LL": LL, "RR": RR, "LR": LR, "pk": list(pk), "bad": list(bad), "flags": sum(int(f) << k for k, f in enumerate(flag)),
                                     "run": list(run), "transitions": list(trans), "flagged": list(flagged)})
            part = [[0.0] * NP for _ in range(3)]
            pk = [0.0, 0.0]
    out.update(hold_peak=hold, pk=pk, part=part)
    return out


# ---- signals --------------------------------------------------------------------------------------------------------------------

# the detector sequence of tests/test_audmon_cpu.py and tests/test_gpu_audmon.py, with 3 intervals to raise and 2 to clear: (condition,
# intervals).  mono x 2 is a run one interval short of raising; the zeros inside the antiphase run hold it at 2, and the interval behind
# them raises ANTIPHASE; quiet and zeros raise SILENCE while ANTIPHASE and RIGHT_LOST stay as they were.
SEQ_PATTERN = (("stereo", 2), ("mono", 2), ("stereo", 1), ("mono", 3), ("stereo", 2), ("near_mono", 3), ("stereo", 2), ("antiphase", 2),
               ("zeros", 2), ("antiphase", 2), ("quiet", 3), ("stereo", 2), ("left_lost", 3), ("stereo", 2), ("right_lost", 3), ("zeros", 3),
               ("stereo", 2))
SEQ_PARAMS = dict(raise_intervals=3, clear_intervals=2)
SEQ_SEED = 20261019
SEQ_A = 0.1
# which detectors a condition makes bad (None: silent, detectors 1 ... 4 hold)
SEQ_BAD = {"stereo": (), "mono": (4,), "near_mono": (4,), "antiphase": (3,), "left_lost": (1,), "right_lost": (2,), "quiet": None, "zeros": None}
# the flags after each interval of the pattern
SEQ_FLAGS = [0, 0, 0, 0, 0, 0, 0, 16, 16, 0, 0, 0, 16, 16, 0, 0, 0, 0, 0, 8, 8, 8, 8, 9, 9, 0, 0, 0, 2, 2, 0, 0, 0, 4, 4, 4, 5, 5, 0]


def seq_conditions(lead: int = 0, total: int | None = None) -> list:
    """the pattern's condition per interval behind `lead` stereo intervals, continued as stereo up to `total` intervals"""
    cd = ["stereo"] * lead + [c for c, k in SEQ_PATTERN for _ in range(k)]
    return cd + ["stereo"] * (0 if total is None else total - len(cd))


def expected_flags(conditions, raise_intervals=3, clear_intervals=2) -> tuple:
    """the flags after every interval for intervals that read their nominal condition: (flags, transitions [5])"""
    flag, run, tr, out = [False] * ND, [0] * ND, [0] * ND, []
    for cd in conditions:
        bad = SEQ_BAD[cd]
        for k in range(ND):
            if bad is None and k > 0:
                continue
            b = (bad is None) if k == 0 else (k in bad)
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


def condition_frames(cd: str, n1: np.ndarray, n2: np.ndarray, a: float = SEQ_A) -> np.ndarray:
    """[n, 2] float64 of one condition from independent unit Gaussian n1, n2"""
    if cd == "stereo":
        L, R = a * n1, a * (0.6 * n1 + 0.8 * n2)
    elif cd == "mono":
        L = a * n1
        R = L
    elif cd == "near_mono":
        L, R = a * n1, a * (n1 + 0.003 * n2)
    elif cd == "antiphase":
        L, R = a * n1, a * (-0.8 * n1 + 0.6 * n2)
    elif cd == "left_lost":
        L, R = 1e-3 * a * n2, a * n1
    elif cd == "right_lost":
        L, R = a * n1, 1e-3 * a * n2
    elif cd == "quiet":
        L, R = 1e-4 * n1, 1e-4 * n2
    elif cd == "zeros":
        L, R = 0.0 * n1, 0.0 * n2
    else:
        raise ValueError(cd)
    return np.stack([L, R], axis=1)


def seq_signal(fs: int, scale: float = 1.0, seed: int = SEQ_SEED, lead: int = 0, total: int | None = None, tail: int = 0) -> np.ndarray:
    """[n, 2] float64, n = intervals * M + tail: the condition of seq_conditions(lead, total) per whole interval, so that no interval
    mixes two conditions, and `tail` frames of an open stereo interval behind them, all times `scale`"""
    M = fs // 10
    cd = seq_conditions(lead, total)
    rng = np.random.default_rng(seed)
    parts = []
    for c, m in [(c, M) for c in cd] + ([("stereo", tail)] if tail else []):
        parts.append(condition_frames(c, rng.standard_normal(m), rng.standard_normal(m)))
    return scale * np.concatenate(parts)


def interval_figures(x: np.ndarray, M: int) -> list:
    """the read-outs' definitions in vectorised float64 (plain sums, not the contract's order) per whole interval of x [n, 2]:
    dicts of level_db (both rails), balance_db, correlation, side_mid_db (NaN where 0 / 0)"""
    L, R = np.asarray(x[:, 0], np.float64), np.asarray(x[:, 1], np.float64)
    k = L.size // M
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for g in range(k):
            l, r = L[g * M:(g + 1) * M], R[g * M:(g + 1) * M]
            ll, rr, lr = float(l @ l), float(r @ r), float(l @ r)
            out.append({"level_db": float(10.0 * np.log10(np.float64(ll + rr) / (2.0 * M))), "balance_db": float(10.0 * np.log10(np.float64(ll) / np.float64(rr))),
                        "correlation": float(np.float64(lr) / np.sqrt(np.float64(ll * rr))),
                        "side_mid_db": float(10.0 * np.log10(np.float64(ll + rr - 2.0 * lr) / np.float64(ll + rr + 2.0 * lr)))})
    return out


def check_margins(x: np.ndarray, M: int, conditions, silence_db=-60.0, loss_db=30.0, antiphase_corr=0.5, mono_db=40.0) -> dict:
    """asserts in float64 that every interval of x stays at least 10 dB from every threshold it must not cross (0.2 in correlation for the
    antiphase threshold); returns the worst figures seen per kind"""
    fig = interval_figures(x, M)
    assert len(fig) >= len(conditions)
    worst = {}

    def note(key, v, pick):
        worst[key] = v if key not in worst else pick(worst[key], v)

    for g, cd in enumerate(conditions):
        f, bad = fig[g], SEQ_BAD[cd]
        if bad is None:                                           # silent: only the level speaks; the other detectors hold
            assert f["level_db"] < silence_db - 10.0, (g, cd, f)
            note("silent level max", f["level_db"], max)
            continue
        assert f["level_db"] > silence_db + 10.0, (g, cd, f)
        note("programme level min", f["level_db"], min)
        if 1 in bad:
            assert f["balance_db"] < -loss_db - 10.0, (g, cd, f)
            note("lost balance min |dB|", abs(f["balance_db"]), min)
        elif 2 in bad:
            assert f["balance_db"] > loss_db + 10.0, (g, cd, f)
            note("lost balance min |dB|", abs(f["balance_db"]), min)
        else:
            assert abs(f["balance_db"]) < loss_db - 10.0, (g, cd, f)
            note("present balance max |dB|", abs(f["balance_db"]), max)
        if 3 in bad:
            assert f["correlation"] < -antiphase_corr - 0.2, (g, cd, f)
            note("antiphase correlation max", f["correlation"], max)
        else:
            assert f["correlation"] > -antiphase_corr + 0.2, (g, cd, f)
            note("other correlation min", f["correlation"], min)
        if 4 in bad:
            assert f["side_mid_db"] < -mono_db - 10.0, (g, cd, f)
            note("mono side/mid max", f["side_mid_db"], max)
        else:
            assert f["side_mid_db"] > -mono_db + 10.0, (g, cd, f)
            note("stereo side/mid min", f["side_mid_db"], min)
    return worst
