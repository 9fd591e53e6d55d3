"""Carrier squelch on the GPU (fmd_squelch_*, Squelch): status records and masks against the C restatement of the arithmetic contract
(tests/cpp/squelch_ref.c, itself checked in test_squelch_cpu.py), bit for bit: the gate sequence in one call, split calls on alternating
streams, calls of M - 1, M and M + 1 samples and calls that end on or hold interval ends, n = 0, batch and row invariance, the `active`
mask, parameters, modes and resets, u8 against cf32 from odd strides, zero / denormal / inf / NaN samples, 256 and 250 kSa/s, the
device's records, argument errors, the C++ adaptor, and channeliser -> squelch -> demodulator -> mixer end to end."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import squelch_ref
import synth
from squelch_ref import bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FS = 192000
M = FS // 20
IV = 25                    # intervals of the shared signal
N1 = IV * M + squelch_ref.GATE_TAIL
AMPL = (100.0, 37.0, 250.0)
GP = squelch_ref.GATE_PARAMS


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return squelch_ref.build(tmp_path_factory.mktemp("squelch_ref_gpu"))


@pytest.fixture(scope="module")
def x1():
    """[3, N1, 2] float32: the gate sequence, station c with its own amplitude, its own noise and c intervals without a carrier in front"""
    return np.stack([squelch_ref.gate_signal(FS, AMPL[c], seed=squelch_ref.GATE_SEED + c, lead=c, total=IV) for c in range(3)]).astype(np.float32)


@pytest.fixture(scope="module")
def want1(ref, x1):
    """the restatement's three stations after x1 in one piece (computed once, not changed by any test)"""
    return [ref.run(FS, x1[c], **GP) for c in range(3)]


@pytest.fixture(scope="module")
def basic(pkg, x1):
    """(status [3], mask [3]) after x1 in one call"""
    q = pkg.Squelch(3, FS)
    q.set_params(**GP)
    mask = q.process(_cuda(x1))
    out = q.status(), mask.cpu().numpy()
    q.close()
    return out


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got_st, chans, what="", mask=None, nan_ok=False):
    """device records (and mask bytes) == the restatement's stations, bit for bit (nan_ok: a NaN's sign and payload are not part of the
    contract, so a field that is NaN in both compares equal)"""
    for c, ch in enumerate(chans):
        want = ch.status()[0]
        for f in squelch_ref.STATUS_DTYPE.names:
            g, w = np.atleast_1d(got_st[c][f]), np.atleast_1d(want[f])
            if nan_ok and g.dtype.kind == "f":
                nan = np.isnan(w)
                assert np.array_equal(np.isnan(g), nan), (what, c, f, g, w)
                g, w = g[~nan], w[~nan]
            assert np.array_equal(bits(g), bits(w)), (what, c, f, got_st[c][f], want[f])
        if mask is not None:
            assert int(mask[c]) == ch.mask, (what, c, int(mask[c]), ch.mask)


def test_gate_sequence_one_call(pkg, x1, want1, basic):
    st, mask = basic
    _same(st, want1, "one call", mask)
    assert [int(v) for v in st["samples"]] == [N1] * 3 and [int(v) for v in st["intervals"]] == [IV] * 3
    assert [int(v) for v in st["transitions"]] == [3] * 3 and mask.tolist() == [1, 1, 1] and not st["nonfinite"].any()
    for c in range(3):
        masks, tr = squelch_ref.expected_masks(squelch_ref.gate_levels(c, IV), **GP)
        assert tr == 3 and int(st[c]["intervals_open"]) == sum(masks) and int(st[c]["open"]) == masks[-1] == 1
        # the last twenty intervals: the read-outs are the restatement's, the newest interval is a 20 dB one, the level follows the amplitude
        assert pkg.squelch_cnr_db(st[c], FS, 1) == want1[c].cnr_db(1) and pkg.squelch_cnr_db(st[c], FS, 20) == want1[c].cnr_db(20)
        assert abs(pkg.squelch_cnr_db(st[c], FS, 1) - 20.0) < 0.5
        assert abs(pkg.squelch_level_db(st[c], FS) - 10.0 * math.log10(AMPL[c] ** 2 * 1.01)) < 0.1
        assert float(st[c]["hold_peak"]) >= float(st[c]["last_peak"]) > AMPL[c] * 0.9
    q = pkg.Squelch(3, FS)
    assert q.status_dev_ptr()


def test_gate_after_every_interval(pkg, ref, x1):
    """a call per interval: the mask after every interval is the pattern's"""
    xd = _cuda(x1)
    q = pkg.Squelch(3, FS, max_input_samples=M)
    q.set_params(**GP)
    chans = [ref.channel(FS) for _ in range(3)]
    want = [squelch_ref.expected_masks(squelch_ref.gate_levels(c, IV), **GP)[0] for c in range(3)]
    assert want[0][:23] == squelch_ref.GATE_MASK
    mask = None
    seen = []
    for g in range(IV):
        mask = q.process(xd[:, g * M:], n=M, mask=mask)
        seen.append(mask.cpu().numpy().tolist())
    for c in range(3):
        chans[c].set_params(**GP)
        for g in range(IV):
            chans[c].process(x1[c, g * M:(g + 1) * M])
            assert seen[g][c] == chans[c].mask == want[c][g], (c, g)
    _same(q.status(), chans, "a call per interval", mask.cpu().numpy())


def test_splits_on_alternating_streams(pkg, ref, x1, basic):
    """1 + 63 + 64 + 65 + 255 + 256 + 257 + (M - 1) + M + (M + 1) + rest, on two alternating streams: the one-call records, and the
    restatement's fed the same pieces"""
    import torch
    xd = _cuda(x1)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    q = pkg.Squelch(3, FS)
    q.set_params(**GP)
    chans = [ref.channel(FS) for _ in range(3)]
    for ch in chans:
        ch.set_params(**GP)
    a = 0
    mask = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    for k, step in enumerate((1, 63, 64, 65, 255, 256, 257, M - 1, M, M + 1, N1)):
        b = min(a + step, N1)
        q.process(xd[:, a:], n=b - a, mask=mask, stream=streams[k % 2])
        for c in range(3):
            chans[c].process(x1[c, a:b])
        a = b
    assert a == N1
    st = q.status()
    _same(st, chans, "splits", mask.cpu().numpy())
    assert np.array_equal(bits(st), bits(basic[0])) and np.array_equal(mask.cpu().numpy(), basic[1])


@pytest.mark.parametrize("step", [M - 1, M, M + 1, 2 * M + 5])
def test_call_lengths(pkg, x1, basic, step):
    """calls of one interval less, one interval (every call ends exactly on an interval's end), one more, and two interval ends a call"""
    xd = _cuda(x1)
    q = pkg.Squelch(3, FS, max_input_samples=step)
    q.set_params(**GP)
    mask = None
    for a in range(0, N1, step):
        mask = q.process(xd[:, a:], n=min(step, N1 - a), mask=mask)
    assert np.array_equal(bits(q.status()), bits(basic[0])) and np.array_equal(mask.cpu().numpy(), basic[1])


@pytest.mark.parametrize("first", [0, M - 2])
@pytest.mark.parametrize("fmt", ["cf32", "u8"])
def test_small_calls(pkg, ref, x1, fmt, first):
    """Calls of 1, 3, 4, 5, 255, 256 and 257 samples and one that runs to M + 2 behind their start, every station from sample 0 of a
    fresh squelch or behind a first call of M - 2 samples, so that the 1-, 3- and 4-sample calls straddle an interval's end inside one
    lane's four samples: a lone sample, a partial quad, a whole one, a quad plus one, a row less one, a whole row, a row plus one, and
    an interval's end inside a quad and inside a row.  Records and mask bytes are the restatement's after every call."""
    import torch
    x = x1[:, :2 * M] if fmt == "cf32" else squelch_ref.to_u8(x1[:, :2 * M] * (40.0 / np.float32(AMPL))[:, None, None])
    xd = _cuda(x)
    q = pkg.Squelch(3, FS)
    q.set_params(**GP)
    chans = [ref.channel(FS) for _ in range(3)]
    for ch in chans:
        assert ch.set_params(**GP) == 0
    mask = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    small = (1, 3, 4, 5, 255, 256, 257)
    a = 0
    for step in ((first,) if first else ()) + small + (M + 2 - sum(small),):      # the last call ends M + 2 samples behind the small calls' start
        q.process(xd[:, a:], n=step, mask=mask)
        for c in range(3):
            chans[c].process(x[c, a:a + step])
        a += step
        _same(q.status(), chans, f"{fmt}, first call {first}, {a} samples in", mask.cpu().numpy())
    assert a == first + M + 2 and [int(v) for v in q.status()["intervals"]] == [2 if first else 1] * 3


def test_n_zero_still_writes_the_mask(pkg, ref, x1):
    import torch
    xd = _cuda(x1)
    q = pkg.Squelch(3, FS)
    mask = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    q.process(xd, n=0, mask=mask)
    assert mask.cpu().numpy().tolist() == [0, 0, 0]
    _same(q.status(), [ref.channel(FS)] * 3, "n = 0 on a fresh squelch")
    q.set_params(**GP)
    n = 8 * M + 100                                               # station 0 is open behind interval 7, station 2 not before interval 9
    q.process(xd, n=n)
    before = q.status()
    mask.fill_(0xAA)
    assert q.process(xd[:, n:], n=0, mask=mask) is mask
    assert mask.cpu().numpy().tolist() == [1, 1, 0] and np.array_equal(bits(q.status()), bits(before))
    # and a NULL mask is allowed
    q._check(q.L.fmd_squelch_process_cf32_dev(q.q, xd.data_ptr(), N1, 0, None, None, None))
    q._check(q.L.fmd_squelch_process_cf32_dev(q.q, xd.data_ptr(), N1, 64, None, None, None))
    assert int(q.status()[0]["samples"]) == n + 64


def test_mask_allocated_by_the_call_on_a_side_stream(pkg, x1, want1):
    """mask = None on a stream that is not torch's current one: the tensor the call allocates is zeroed on that stream, so a skipped
    station's byte is 0 and the others are the gate's"""
    import torch
    xd = _cuda(x1)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    q = pkg.Squelch(3, FS)
    q.set_params(**GP)
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for stream in (s, s.cuda_stream):
        mask = q.process(xd, active=active, stream=stream)
        s.synchronize()
        assert mask.dtype == torch.uint8 and mask.cpu().numpy().tolist() == [1, 0, 1]
        q.reset()
    assert want1[0].mask == 1 and want1[2].mask == 1


def test_batch_and_row_invariance(pkg, ref, x1):
    """a station alone, and the same station at row 69 of a batch of 70 (every row checked), over the first ten intervals and a bit"""
    n = 10 * M + 777
    chans = [ref.run(FS, x1[c, :n], **GP) for c in range(3)]
    alone = pkg.Squelch(1, FS)
    alone.set_params(**GP)
    m1 = alone.process(_cuda(x1[:1, :n]))
    _same(alone.status(), chans[:1], "alone", m1.cpu().numpy())
    x = np.stack([x1[c % 3, :n] for c in range(70)])                         # row 69 carries station 0
    q = pkg.Squelch(70, FS)
    q.set_params(**GP)
    m70 = q.process(_cuda(x)).cpu().numpy()
    st = q.status()
    _same(st, [chans[c % 3] for c in range(70)], "C = 70", m70)
    assert np.array_equal(bits(st[69]), bits(alone.status()[0])) and m70[69] == m1.cpu().numpy()[0]


def test_active_mask(pkg, ref, x1):
    """a skipped station keeps its records and its mask byte: the mask buffer is pre-filled with 0xAA before every call"""
    import torch
    cuts = (0, 7 * M + 5, 9 * M + 100, 12 * M + 9)
    q = pkg.Squelch(3, FS)
    q.set_params(**GP)
    chans = [ref.channel(FS) for _ in range(3)]
    for ch in chans:
        ch.set_params(**GP)
    xd = _cuda(x1)
    for k in range(3):
        a, b = cuts[k], cuts[k + 1]
        active = torch.tensor([1, 0 if k == 1 else 1, 1], dtype=torch.uint8, device="cuda")
        mask = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
        q.process(xd[:, a:], n=b - a, active=active if k else None, mask=mask)
        for c in range(3):
            if not (k == 1 and c == 1):
                chans[c].process(x1[c, a:b])
        got = mask.cpu().numpy()
        _same(q.status(), chans, f"call {k}")
        assert [int(v) for v in got] == [chans[0].mask, 0xAA if k == 1 else chans[1].mask, chans[2].mask], (k, got)
    assert int(q.status()[1]["samples"]) == cuts[3] - (cuts[2] - cuts[1])
    before = q.status()
    mask = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    q.process(xd, active=torch.zeros(3, dtype=torch.bool, device="cuda"), mask=mask)
    assert np.array_equal(bits(q.status()), bits(before)) and mask.cpu().numpy().tolist() == [0xAA] * 3


def test_parameters_modes_and_resets(pkg, ref, x1):
    import torch
    xd = _cuda(x1)
    q = pkg.Squelch(3, FS)
    chans = [ref.channel(FS) for _ in range(3)]
    d = q.params(1)
    assert (d.open_db, d.close_db, d.min_level_db, d.open_intervals, d.close_intervals, d.mode) == (10.0, 7.0, -math.inf, 2, 10, 0)
    cuts = (0, 5 * M + 33, 11 * M + 1, 15 * M, 19 * M + 400)
    # between calls: station 1 gets the sequence's parameters first, then a level floor above its own level; station 2 is forced
    steps = [{1: GP}, {1: dict(min_level_db=40.0), 2: dict(mode=pkg.FMD_SQUELCH_FORCE_OPEN)}, {2: dict(mode=pkg.FMD_SQUELCH_FORCE_CLOSED)},
             {1: dict(min_level_db=-math.inf, close_intervals=1), 2: dict(mode=pkg.FMD_SQUELCH_AUTO, open_db=30.0, close_db=0.0)}]
    for k in range(4):
        for c, f in steps[k].items():
            q.set_params(c, **f)
            assert chans[c].set_params(**f) == 0
        mask = q.process(xd[:, cuts[k]:], n=cuts[k + 1] - cuts[k])
        for c in range(3):
            chans[c].process(x1[c, cuts[k]:cuts[k + 1]])
        _same(q.status(), chans, f"parameters, call {k}", mask.cpu().numpy())
        if k == 1:
            assert mask.cpu().numpy()[2] == 1 and int(q.status()[2]["mode"]) == 1
        if k == 2:
            assert mask.cpu().numpy()[2] == 0 and int(q.status()[2]["mode"]) == 2 and int(q.status()[2]["open"]) == 1   # the gate runs on
    p = q.params(1)
    assert (p.close_intervals, p.open_intervals, p.min_level_db) == (1, 2, -math.inf) and q.params(0).open_intervals == 2 and q.params(2).open_db == 30.0
    # the level floor kept station 1 (amplitude 37: 31.4 dB) shut while its carrier was there
    assert int(q.status()[1]["intervals_open"]) == 0 and int(q.status()[0]["intervals_open"]) > 0
    # refused parameters change nothing
    before = q.status()
    for f in (dict(open_db=61.0), dict(close_db=11.0), dict(close_db=-1.0), dict(open_intervals=0), dict(close_intervals=1001), dict(mode=3),
              dict(min_level_db=math.nan), dict(min_level_db=math.inf)):
        with pytest.raises(pkg.FmdError) as e:
            q.set_params(0, **f)
        assert e.value.status == -1, f
    p0 = q.params(0)
    assert (p0.open_db, p0.close_db, p0.min_level_db, p0.open_intervals, p0.close_intervals, p0.mode) == (10.0, 7.0, -math.inf, 2, 10, 0)
    assert np.array_equal(bits(q.status()), bits(before))
    # reset(1): station 1 as after create with its parameters kept, the others untouched; reset_peaks(0): the held peak alone
    q.reset(1)
    chans[1].reset()
    st = q.status()
    _same(st, chans, "after reset(1)")
    assert int(st[1]["samples"]) == 0 and st[1]["hold_peak"] == 0 and int(st[1]["open"]) == 0 and not st[1]["ring_s2"].any() and st[0]["ring_s2"].any()
    assert q.params(1).close_intervals == 1
    q.reset_peaks(0)
    chans[0].reset_peaks()
    _same(q.status(), chans, "after reset_peaks(0)")
    assert q.status()[0]["hold_peak"] == 0 and q.status()[2]["hold_peak"] > 0
    # the open interval survived reset_peaks and went with reset: the next call tells
    mask = q.process(xd[:, cuts[4]:], n=2 * M)
    for c in range(3):
        chans[c].process(x1[c, cuts[4]:cuts[4] + 2 * M])
    _same(q.status(), chans, "after the next call", mask.cpu().numpy())
    q.reset()
    for ch in chans:
        ch.reset()
    _same(q.status(), chans, "after reset()")
    assert not q.status()["samples"].any() and [int(v) for v in q.status()["mode"]] == [0, 0, 0]
    torch.cuda.synchronize()


def test_u8_odd_strides(pkg, ref, x1):
    """u8 against cf32 of the converted samples, both from rows with an odd in_stride > n (cf32 rows only 8-byte aligned, u8 rows only
    2-byte aligned) and in two calls"""
    import torch
    n = 8 * M + 333                                              # station 2 opens behind its ninth interval
    b8 = squelch_ref.to_u8(x1[:, :n] * (40.0 / np.float32(AMPL))[:, None, None])
    f32 = squelch_ref.from_u8(b8)
    assert 0 < b8.min() and b8.max() < 255
    chans = [ref.run(FS, b8[c], **GP) for c in range(3)]
    stride = n + 8
    assert stride % 2 == 1
    bp = torch.full((3, stride, 2), 7, dtype=torch.uint8, device="cuda")
    bp[:, :n] = _cuda(b8)
    fp = torch.full((3, stride, 2), float("nan"), device="cuda")
    fp[:, :n] = _cuda(f32)
    got = []
    for xp in (bp, fp):
        q = pkg.Squelch(3, FS)
        q.set_params(**GP)
        q.process(xp, n=1001)
        mask = q.process(xp[:, 1001:], n=n - 1001)
        got.append((q.status(), mask.cpu().numpy()))
        _same(got[-1][0], chans, str(xp.dtype), got[-1][1])
    assert np.array_equal(bits(got[0][0]), bits(got[1][0])) and np.array_equal(got[0][1], got[1][1])
    assert got[0][1].tolist() == [1, 1, 0]


def test_special_samples(pkg, ref, x1):
    """all-zero input: the gate stays closed (the comparisons are strict).  Denormals count (they are kept).  An inf or NaN sample makes
    its interval's sums non-finite: the interval counts in `nonfinite` and is not good, so a carrier that would open the gate does not
    while every second interval holds one; the peak drops a NaN."""
    n = 6 * M + 50
    clean = x1[0, 5 * M:5 * M + n]                                           # 20 dB throughout: opens behind its second interval
    x = np.stack([clean] * 6).copy()
    x[0] = 0.0                                                               # silence
    x[1] = np.float32(1e-42)                                                 # denormal I and Q throughout: p = 2e-84 is a normal double
    x[2, 0::2 * M, 0] = np.inf                                               # intervals 0, 2, 4
    x[2, M + 7::2 * M, 1] = -np.inf                                          # intervals 1, 3, 5
    x[3, 255::M] = np.nan                                                    # every interval, the last lane of a row
    x[4, M + 11, 1] = np.nan                                                 # interval 1 alone: the gate opens two intervals later
    q = pkg.Squelch(6, FS)
    q.set_params(open_intervals=2, close_intervals=1)
    mask = q.process(_cuda(x)).cpu().numpy()
    st = q.status()
    chans = [ref.run(FS, x[c], open_intervals=2, close_intervals=1) for c in range(6)]
    _same(st, chans, "special samples", mask, nan_ok=True)
    assert [int(v) for v in st["nonfinite"]] == [0, 0, 6, 6, 1, 0] and (st["intervals"] == 6).all()
    # (the denormal station is a carrier of constant envelope and nothing else: it opens)
    assert mask.tolist() == [0, 1, 0, 0, 1, 1] and [int(v) for v in st["transitions"]] == [0, 1, 0, 0, 1, 1]
    assert [int(v) for v in st["intervals_open"]] == [0, 5, 0, 0, 3, 5]
    assert st[0]["hold_peak"] == 0 and not st[0]["ring_s2"].any() and int(st[0]["run"]) == 0
    assert st[1]["ring_s2"][0] > 0 and st[1]["last_peak"] == np.float32(1e-42) and np.isinf(pkg.squelch_cnr_db(st[1], FS, 1))
    assert np.isinf(st[2]["hold_peak"]) and np.isnan(st[3]["ring_s2"][:6]).all()
    assert np.isfinite(st[3]["hold_peak"]) and st[3]["hold_peak"] <= st[5]["hold_peak"] and np.isfinite(st[3]["last_peak"])
    # clean again behind the NaN: intervals 2 ... 5 of station 4 are those of station 5
    for f in ("ring_s2", "ring_s4"):
        assert np.array_equal(bits(st[4][f][2:6]), bits(st[5][f][2:6])) and np.isnan(st[4][f][1])


@pytest.mark.parametrize("fs", [256000, 250000])
def test_other_rates(pkg, ref, fs):
    """at 250 kSa/s M = 12500 is no multiple of 256, so an interval's last row is partial and the next interval's rows start off the
    rows' grid in memory"""
    Mm = fs // 20
    n = 9 * Mm + 333
    x = np.stack([squelch_ref.gate_signal(fs, 80.0, seed=fs + c, lead=c)[:n] for c in range(2)]).astype(np.float32)
    q = pkg.Squelch(2, fs)
    q.set_params(**GP)
    mask = q.process(_cuda(x), n=4 * Mm + 1)
    mask = q.process(_cuda(x[:, 4 * Mm + 1:]), mask=mask)
    chans = [ref.run(fs, x[c], **GP) for c in range(2)]
    _same(q.status(), chans, f"{fs}", mask.cpu().numpy())
    assert (q.status()["intervals"] == 9).all() and mask.cpu().numpy().tolist() == [1, 1]


def test_device_records_and_argument_errors(pkg, x1, basic):
    import torch
    q = pkg.Squelch(3, FS, max_input_samples=N1)
    q.set_params(**GP)
    xd = _cuda(x1)
    q.process(xd)
    # the device's own records
    torch.cuda.synchronize()
    import ctypes as C
    ptr = q.status_dev_ptr()

    class _Arr:
        __cuda_array_interface__ = {"shape": (3 * 368,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    raw = torch.as_tensor(_Arr(), device="cuda").clone()
    assert np.array_equal(raw.cpu().numpy(), bits(basic[0]))
    bad = [lambda: q.process(xd, n=N1 + 1),                       # n > in_stride and > max_input_samples
           lambda: q.process(xd, n=-1),
           lambda: q.reset(3), lambda: q.reset(-2), lambda: q.reset_peaks(3), lambda: q.reset_peaks(-2), lambda: q.params(3), lambda: q.params(-1),
           lambda: q._check(q.L.fmd_squelch_set_params(q.q, 3, C.byref(pkg.squelch_default_params())))]
    for k, f in enumerate(bad):
        with pytest.raises(pkg.FmdError) as e:
            f()
        assert e.value.status == -1, k                            # FMD_ERR_ARG
    small = pkg.Squelch(3, FS, max_input_samples=4096)
    with pytest.raises(pkg.FmdError) as e:
        small.process(xd, n=4097)
    assert e.value.status == -1 and int(small.status()[0]["samples"]) == 0
    for f in (lambda: q.process(xd[:2]), lambda: q.process(xd, active=torch.ones(2, dtype=torch.uint8, device="cuda")),
              lambda: q.process(xd.double()), lambda: q.process(xd[:, :, :1]), lambda: q.process(xd, mask=torch.zeros(2, dtype=torch.uint8, device="cuda")),
              lambda: q.process(xd, mask=torch.zeros(3, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(TypeError):
        q.set_params(0, threshold=3.0)
    # pointers that are not aligned to a sample
    with pytest.raises(pkg.FmdError) as e:
        q._check(q.L.fmd_squelch_process_cf32_dev(q.q, xd.data_ptr() + 4, N1, 16, None, None, None))
    assert e.value.status == -1
    b = torch.zeros(3, 64, 2, dtype=torch.uint8, device="cuda")
    with pytest.raises(pkg.FmdError) as e:
        q._check(q.L.fmd_squelch_process_u8_dev(q.q, b.data_ptr() + 1, 64, 16, None, None, None))
    assert e.value.status == -1
    for cfg in ((0, FS, 64), (3, 1024000, 64), (3, 191000, 64), (3, FS, 0)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.Squelch(cfg[0], cfg[1], max_input_samples=cfg[2])
        assert e.value.status == -1
    assert np.array_equal(bits(q.status()), bits(basic[0]))


def test_cpp_adaptor(pkg, ref, x1, tmp_path):
    """tests/cpp/squelch_main.cpp takes a file of u8 baseband in calls of 10000 samples; what it prints is the restatement's, and it
    exits with 7 unless the records behind fmd_squelch_status_dev are those of fmd_squelch_get_status"""
    exe = tmp_path / "squelch_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'fm-radio_amd' / 'host'}", "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "squelch_main.cpp"),
                    f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)],
                   check=True)
    n = 22 * M + 123
    b8 = squelch_ref.to_u8(x1[:2, :n] * (40.0 / np.float32(AMPL[:2]))[:, None, None])
    b8.tofile(tmp_path / "cap.u8")
    out = subprocess.run([str(exe), str(tmp_path / "cap.u8"), "u8", "2", str(FS), "10000", "2", "3"], check=True, capture_output=True, text=True).stdout
    lines = out.strip().split("\n")
    assert len(lines) == 2
    for c, line in enumerate(lines):
        w = line.split()
        ch = ref.run(FS, b8[c], **GP)
        assert bytes.fromhex(w[0]) == ch.status()[0].tobytes(), c
        assert int(w[1]) == ch.mask
        assert [float(v) for v in w[2:5]] == [ch.level_db(), ch.cnr_db(1), ch.cnr_db(20)]


def test_band_end_to_end(pkg):
    """A 2.56 MSa/s capture of 0.6 s with oracle/synth.py's realistic stations at -900 kHz and +300 kHz, about 30 dB over the noise of
    their own 256 kHz channel, and nothing at -300 kHz and +900 kHz: Channelizer to 256 kSa/s -> Squelch -> BatchDemod (tolerance mode)
    -> AudioMixer with active = the squelch's mask.  The mask is [1, 0, 1, 0] from the first block that ends behind 150 ms on; the mixed
    bus is, bit for bit, the bus mixed with the same mask built on the host, and not the bus mixed with active = None."""
    import torch
    fs_in, fs, bs = 2_560_000, 256_000, 16384
    nb = 9                                                                   # 9 blocks of 64 ms = 0.576 s of the 0.6 s
    n_in = int(0.6 * fs_in)
    centers = np.array([-900e3, -300e3, 300e3, 900e3])
    t = np.arange(n_in) / fs_in
    wide = np.zeros(n_in, np.complex128)
    for k, f0 in ((0, centers[0]), (1, centers[2])):
        wide += synth.fm_capture_realistic(n_in, fs=float(fs_in), seed=90 + k, channel=k, cnr_db=200.0)["iq"] * np.exp(2j * np.pi * f0 * t)
    rng = np.random.default_rng(5)
    sigma = math.sqrt(0.5 * 10.0 ** (-30.0 / 10.0) * (fs_in / fs))           # 30 dB in 256 kHz
    wide += sigma * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))
    wt = torch.from_numpy(np.stack([wide.real, wide.imag], axis=1).astype(np.float32)).cuda()
    ch = pkg.Channelizer(float(fs_in), centers, fs_out=float(fs), max_input_samples=bs * 10)
    q = pkg.Squelch(4, fs, max_input_samples=bs)
    dm = pkg.BatchDemod(4, bs, fs, fast_math=True)
    mixers = [pkg.AudioMixer(4, [[0, 1, 2, 3]]) for _ in range(3)]
    host_mask = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device="cuda")
    masks, differs = [], False
    for b in range(nb):
        y = ch.process(wt[b * bs * 10:(b + 1) * bs * 10].contiguous()).contiguous()
        assert tuple(y.shape) == (4, bs, 2)
        mask = q.process(y)
        dm.process(y)
        dm.synchronize()
        a = dm.audio_tensor()
        bus = mixers[0].process(a, active=mask).clone()
        masks.append(mask.cpu().numpy().tolist())
        if (b + 1) * bs / fs >= 0.150:
            assert masks[-1] == [1, 0, 1, 0], (b, masks)
            assert torch.equal(bus.view(torch.int32), mixers[1].process(a, active=host_mask).view(torch.int32)), b
            differs = differs or not torch.equal(bus, mixers[2].process(a))
    st = q.status()
    print("masks per block", masks, "cnr_db", [pkg.squelch_cnr_db(st[c], fs, 1) for c in range(4)])
    assert differs and [int(v) for v in st["transitions"]] == [1, 0, 1, 0] and (st["intervals"] == nb * bs // (fs // 20)).all()
    assert min(pkg.squelch_cnr_db(st[0], fs, 5), pkg.squelch_cnr_db(st[2], fs, 5)) > 15.0 and max(pkg.squelch_cnr_db(st[1], fs, 5), pkg.squelch_cnr_db(st[3], fs, 5)) < 0.0
    ch.close(); dm.close(); q.close()
