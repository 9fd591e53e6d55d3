"""Audio fault monitor on the GPU (fmd_audmon_*, AudioMonitor): status records and the flags and ok bytes against the C restatement of
the arithmetic contract (tests/cpp/audmon_ref.c, itself checked in test_audmon_cpu.py), bit for bit: the detector sequence in one call,
a call per interval, split calls on alternating streams, calls of M - 1, M, M + 1 and 2 M + 5 frames, n = 0, batch and row invariance,
the `active` mask, NULL byte arrays, parameters, alarm masks and resets, odd strides and views, zero / denormal / inf / NaN samples, 32
and 48 kHz, the device's records, argument errors, the C++ adaptor, and demodulator -> monitor -> mixer end to end.

The main cases run at fs = 8000 (M = 800) with three stations.  Station c has its own amplitude, its own noise and c stereo intervals in
front of the pattern, and it has taken OFF[c] frames of its own before the calls under test, so that its intervals end at different
places of every call than its neighbours'."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import audmon_ref
import synth
from audmon_ref import bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FS = 8000
M = FS // 10
IV = 42                    # intervals of the shared signal: the ring of 30 wraps
TAIL = 100
N1 = IV * M + TAIL         # frames per station of the calls under test
SCALE = (1.0, 0.37, 2.5)
OFF = (0, 277, 531)        # frames each station has taken before (no multiples of 4)
SP = audmon_ref.SEQ_PARAMS


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return audmon_ref.build(tmp_path_factory.mktemp("audmon_ref_gpu"))


@pytest.fixture(scope="module")
def streams():
    """per station [OFF[c] + N1, 2] float32: the detector sequence on the station's own interval grid"""
    return [audmon_ref.seq_signal(FS, SCALE[c], seed=audmon_ref.SEQ_SEED + c, lead=c, total=IV, tail=TAIL + OFF[c]).astype(np.float32) for c in range(3)]


@pytest.fixture(scope="module")
def x1(streams):
    """[3, N1, 2] float32: what the calls under test take"""
    return np.stack([streams[c][OFF[c]:] for c in range(3)])


@pytest.fixture(scope="module")
def pre(streams):
    """[3, max(OFF), 2] float32: what each station took before, from row c's start"""
    p = np.zeros((3, max(OFF), 2), np.float32)
    for c in range(3):
        p[c, :OFF[c]] = streams[c][:OFF[c]]
    return p


@pytest.fixture(scope="module")
def want1(ref, streams):
    """the restatement's three stations after their whole streams (computed once, not changed by any test)"""
    return [ref.run(FS, streams[c], **SP) for c in range(3)]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _start(pkg, pre, **kw):
    """a monitor of three stations with the sequence's run lengths whose station c has taken its OFF[c] frames"""
    import torch
    m = pkg.AudioMonitor(3, FS, **kw)
    m.set_params(**SP)
    pd = _cuda(pre)
    for c in (1, 2):
        active = torch.zeros(3, dtype=torch.uint8, device="cuda")
        active[c] = 1
        m.process(pd, n=OFF[c], active=active, flags=False, ok=False)
    return m


def _ref_start(ref, pre):
    return [ref.channel(FS, **SP).process(pre[c, :OFF[c]]) for c in range(3)]


@pytest.fixture(scope="module")
def basic(pkg, x1, pre):
    """(status [3], flags [3], ok [3]) after x1 in one call"""
    m = _start(pkg, pre)
    flags, ok = m.process(_cuda(x1))
    out = m.status(), flags.cpu().numpy(), ok.cpu().numpy()
    m.close()
    return out


def _same(got_st, chans, what="", flags=None, ok=None, nan_ok=False):
    """device records (and the two bytes) == the restatement's stations, bit for bit (nan_ok: a NaN's sign and payload are not part of
    the contract, so a field that is NaN in both compares equal)"""
    for c, ch in enumerate(chans):
        want = ch.status()[0]
        for f in audmon_ref.STATUS_DTYPE.names:
            g, w = np.atleast_1d(got_st[c][f]), np.atleast_1d(want[f])
            if nan_ok and g.dtype.kind == "f":
                nan = np.isnan(w)
                assert np.array_equal(np.isnan(g), nan), (what, c, f, g, w)
                g, w = g[~nan], w[~nan]
            assert np.array_equal(bits(g), bits(w)), (what, c, f, got_st[c][f], want[f])
        if flags is not None:
            assert int(flags[c]) == ch.flags, (what, c, int(flags[c]), ch.flags)
        if ok is not None:
            assert int(ok[c]) == ch.ok, (what, c, int(ok[c]), ch.ok)


def test_sequence_one_call(pkg, want1, basic):
    st, flags, ok = basic
    _same(st, want1, "one call", flags, ok)
    assert [int(v) for v in st["frames"]] == [N1 + OFF[c] for c in range(3)] and [int(v) for v in st["intervals"]] == [IV] * 3
    assert flags.tolist() == [0, 0, 0] and ok.tolist() == [1, 1, 1] and not st["nonfinite"].any()
    for c in range(3):
        want, tr = audmon_ref.expected_flags(audmon_ref.seq_conditions(c, IV), **SP)
        assert tr == [4, 2, 2, 2, 4] == st[c]["transitions"].tolist()
        assert st[c]["intervals_flagged"].tolist() == [sum((f >> k) & 1 for f in want) for k in range(5)]
        # the newest intervals are stereo: the read-outs are the restatement's and follow the amplitude
        assert pkg.audmon_correlation(st[c], FS, 30) == want1[c].correlation(30) and pkg.audmon_side_mid_db(st[c], FS, 2) == want1[c].side_mid_db(2)
        assert abs(pkg.audmon_level_db(st[c], FS, 2, 1) - 20.0 * math.log10(0.1 * SCALE[c])) < 0.5 and abs(pkg.audmon_correlation(st[c], FS, 1) - 0.6) < 0.1
        assert (st[c]["hold_peak"] >= st[c]["last_peak"]).all() and (st[c]["last_peak"] > 0.2 * SCALE[c]).all()


def test_bytes_after_every_interval(pkg, ref, x1, pre):
    """a call per interval of M frames: the two bytes after every call are the restatement's, and the flags the pattern's"""
    xd = _cuda(x1)
    m = _start(pkg, pre, max_input_frames=M)
    chans = _ref_start(ref, pre)
    flags = ok = None
    seen = []
    for g in range(IV):
        flags, ok = m.process(xd[:, g * M:], n=M, flags=flags, ok=ok)
        seen.append((flags.cpu().numpy().tolist(), ok.cpu().numpy().tolist()))
    for c in range(3):
        want = audmon_ref.expected_flags(audmon_ref.seq_conditions(c, IV), **SP)[0]
        assert want[c:c + 39] == audmon_ref.SEQ_FLAGS
        for g in range(IV):
            chans[c].process(x1[c, g * M:(g + 1) * M])
            # station c's interval g ends OFF[c] frames before call g does
            assert seen[g][0][c] == chans[c].flags == want[g], (c, g)
            assert seen[g][1][c] == chans[c].ok == int((chans[c].flags & 15) == 0), (c, g)
    assert any(f[0] != f[1] for f, _ in seen)                     # the stations do differ within a call
    _same(m.status(), chans, "a call per interval", flags.cpu().numpy(), ok.cpu().numpy())


def test_splits_on_alternating_streams(pkg, ref, x1, pre, basic):
    """1 + 3 + 4 + 5 + 255 + 256 + 257 + (M - 1) + M + (M + 1) + rest, on two alternating streams: the restatement's records fed the same
    pieces, behind the ten short ones (whose four intervals the ring overwrites later) and at the end, where they are the one-call records"""
    import torch
    xd = _cuda(x1)
    m = _start(pkg, pre)
    chans = _ref_start(ref, pre)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    a = 0
    flags = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    ok = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k, step in enumerate((1, 3, 4, 5, 255, 256, 257, M - 1, M, M + 1, N1)):
        b = min(a + step, N1)
        m.process(xd[:, a:], n=b - a, flags=flags, ok=ok, stream=streams[k % 2])
        for c in range(3):
            chans[c].process(x1[c, a:b])
        a = b
        if k == 9:                                                # before the ring of 30 wraps over the intervals that were split
            _same(m.status(), chans, "the short pieces")
    assert a == N1
    st = m.status()
    _same(st, chans, "splits", flags.cpu().numpy(), ok.cpu().numpy())
    assert np.array_equal(bits(st), bits(basic[0])) and np.array_equal(flags.cpu().numpy(), basic[1]) and np.array_equal(ok.cpu().numpy(), basic[2])


@pytest.mark.parametrize("step", [M - 1, M, M + 1, 2 * M + 5])
def test_call_lengths(pkg, x1, pre, basic, step):
    """calls of one interval less, one interval (station 0's every call ends exactly on an interval's end), one more, and two interval
    ends a call"""
    xd = _cuda(x1)
    m = _start(pkg, pre, max_input_frames=step)
    flags = ok = None
    for a in range(0, N1, step):
        flags, ok = m.process(xd[:, a:], n=min(step, N1 - a), flags=flags, ok=ok)
    assert np.array_equal(bits(m.status()), bits(basic[0])) and np.array_equal(flags.cpu().numpy(), basic[1]) and np.array_equal(ok.cpu().numpy(), basic[2])


@pytest.mark.parametrize("first", [0, M - 2])
def test_small_calls(pkg, ref, x1, first):
    """Calls of 1, 3, 4, 5, 255, 256 and 257 frames and one that runs to M + 2 behind their start, every station from frame 0 of a fresh
    monitor or behind a first call of M - 2 frames, so that the 1-, 3- and 4-frame calls straddle an interval's end inside one lane's
    four frames: a lone frame, a partial quad, a whole one, a quad plus one, a row less one, a whole row, a row plus one, and an
    interval's end inside a quad and inside a row.  Records and bytes are the restatement's after every call."""
    import torch
    xd = _cuda(x1)
    m = pkg.AudioMonitor(3, FS)
    m.set_params(**SP)
    chans = [ref.channel(FS, **SP) for _ in range(3)]
    flags = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    ok = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    small = (1, 3, 4, 5, 255, 256, 257)
    a = 0
    for step in ((first,) if first else ()) + small + (M + 2 - sum(small),):      # the last call ends M + 2 frames behind the small calls' start
        m.process(xd[:, a:], n=step, flags=flags, ok=ok)
        for c in range(3):
            chans[c].process(x1[c, a:a + step])
        a += step
        _same(m.status(), chans, f"first call {first}, {a} frames in", flags.cpu().numpy(), ok.cpu().numpy())
    assert a == first + M + 2 and [int(v) for v in m.status()["intervals"]] == [2 if first else 1] * 3


def test_n_zero_still_writes_both_bytes(pkg, ref, x1, pre):
    import torch
    xd = _cuda(x1)
    m = pkg.AudioMonitor(3, FS)
    flags = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    ok = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    m.process(xd, n=0, flags=flags, ok=ok)
    assert flags.cpu().numpy().tolist() == [0, 0, 0] and ok.cpu().numpy().tolist() == [1, 1, 1]
    _same(m.status(), [ref.channel(FS)] * 3, "n = 0 on a fresh monitor")
    m = _start(pkg, pre)
    chans = _ref_start(ref, pre)
    n = 8 * M + 60                                                # MONO is up in station 0 (interval 7) and not yet in stations 1, 2
    m.process(xd, n=n)
    before = m.status()
    flags.fill_(0xAA)
    ok.fill_(0xAA)
    got = m.process(xd[:, n:], n=0, flags=flags, ok=ok)
    assert got[0] is flags and got[1] is ok
    for c in range(3):
        chans[c].process(x1[c, :n])
    assert flags.cpu().numpy().tolist() == [16, 0, 0] == [ch.flags for ch in chans] and ok.cpu().numpy().tolist() == [1, 1, 1]
    assert np.array_equal(bits(m.status()), bits(before))


def test_null_byte_arrays(pkg, ref, x1, pre):
    """d_flags or d_ok NULL: the other one is written, the records are the same; both NULL with n = 0 is allowed and does nothing"""
    xd = _cuda(x1)
    n = 20 * M + 60                                               # ANTIPHASE is up in station 0 and not yet in stations 1, 2: ok = [0, 1, 1]
    chans = _ref_start(ref, pre)
    for c in range(3):
        chans[c].process(x1[c, :n])
    assert [ch.flags for ch in chans] == [8, 0, 0]
    for kw in (dict(flags=False), dict(ok=False), dict(flags=False, ok=False)):
        m = _start(pkg, pre)
        flags, ok = m.process(xd, n=n, **kw)
        assert (flags is None) == ("flags" in kw) and (ok is None) == ("ok" in kw)
        _same(m.status(), chans, str(kw), None if flags is None else flags.cpu().numpy(), None if ok is None else ok.cpu().numpy())
        m._check(m.L.fmd_audmon_process_f32_dev(m.a, xd.data_ptr(), N1, 0, None, None, None, None))
        _same(m.status(), chans, str(kw) + ", then n = 0 with no bytes")


def test_batch_and_row_invariance(pkg, ref, x1):
    """a station alone, and the same station at row 69 of a batch of 70 (every row checked), over ten intervals and a bit"""
    n = 10 * M + 77
    chans = [ref.run(FS, x1[c, :n], **SP) for c in range(3)]
    alone = pkg.AudioMonitor(1, FS)
    alone.set_params(**SP)
    f1, o1 = alone.process(_cuda(x1[:1, :n]))
    _same(alone.status(), chans[:1], "alone", f1.cpu().numpy(), o1.cpu().numpy())
    x = np.stack([x1[c % 3, :n] for c in range(70)])                         # row 69 carries station 0
    m = pkg.AudioMonitor(70, FS)
    m.set_params(**SP)
    f70, o70 = m.process(_cuda(x))
    f70, o70 = f70.cpu().numpy(), o70.cpu().numpy()
    st = m.status()
    _same(st, [chans[c % 3] for c in range(70)], "C = 70", f70, o70)
    assert np.array_equal(bits(st[69]), bits(alone.status()[0])) and f70[69] == f1.cpu().numpy()[0] and o70[69] == o1.cpu().numpy()[0]


def test_active_mask(pkg, ref, x1, pre):
    """a skipped station keeps its records and its two bytes: both byte arrays are pre-filled with 0xAA before every call"""
    import torch
    cuts = (0, 7 * M + 5, 9 * M + 100, 12 * M + 9)
    m = _start(pkg, pre)
    chans = _ref_start(ref, pre)
    xd = _cuda(x1)
    for k in range(3):
        a, b = cuts[k], cuts[k + 1]
        active = torch.tensor([1, 0 if k == 1 else 1, 1], dtype=torch.uint8, device="cuda")
        flags = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
        ok = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
        m.process(xd[:, a:], n=b - a, active=active if k else None, flags=flags, ok=ok)
        for c in range(3):
            if not (k == 1 and c == 1):
                chans[c].process(x1[c, a:b])
        _same(m.status(), chans, f"call {k}")
        assert flags.cpu().numpy().tolist() == [chans[0].flags, 0xAA if k == 1 else chans[1].flags, chans[2].flags], k
        assert ok.cpu().numpy().tolist() == [chans[0].ok, 0xAA if k == 1 else chans[1].ok, chans[2].ok], k
    assert int(m.status()[1]["frames"]) == OFF[1] + cuts[3] - (cuts[2] - cuts[1])
    before = m.status()
    flags = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    ok = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    m.process(xd, active=torch.zeros(3, dtype=torch.bool, device="cuda"), flags=flags, ok=ok)
    assert np.array_equal(bits(m.status()), bits(before)) and flags.cpu().numpy().tolist() == [0xAA] * 3 == ok.cpu().numpy().tolist()


def test_parameters_alarm_masks_and_resets(pkg, ref, x1, pre):
    import torch
    xd = _cuda(x1)
    m = pkg.AudioMonitor(3, FS)
    chans = [ref.channel(FS) for _ in range(3)]
    assert audmon_ref.params_tuple(m.params(1)) == (-60.0, 30.0, 0.5, 40.0, (100, 100, 100, 50, 100), (10,) * 5, 15)
    cuts = (0, 7 * M + 33, 12 * M + 1, 20 * M, 26 * M + 400)
    # between calls: every station gets the sequence's run lengths first; then station 1 a silence threshold above its own level, MONO as
    # an alarm and its own run lengths per detector, station 2 a mono threshold that near-mono misses and no alarms at all
    steps = [{0: SP, 1: SP, 2: SP}, {1: dict(silence_db=-20.0, alarm_mask=31, raise_intervals=(1, 2, 3, 4, 5)), 2: dict(mono_db=70.0, alarm_mask=0)},
             {1: dict(silence_db=-math.inf, clear_intervals=(5, 4, 3, 2, 1)), 2: dict(antiphase_corr=0.9, loss_db=80.0)},
             {1: dict(alarm_mask=8), 2: dict(alarm_mask=31, antiphase_corr=0.5, mono_db=40.0, loss_db=30.0)}]
    for k in range(4):
        for c, f in steps[k].items():
            m.set_params(c, **f)
            assert chans[c].set_params(**f) == 0
        _same(m.status(), chans, f"parameters, before call {k}")             # (the record's ok follows the alarm mask at once)
        flags, ok = m.process(xd[:, cuts[k]:], n=cuts[k + 1] - cuts[k])
        for c in range(3):
            chans[c].process(x1[c, cuts[k]:cuts[k + 1]])
        _same(m.status(), chans, f"parameters, call {k}", flags.cpu().numpy(), ok.cpu().numpy())
    st = m.status()
    assert int(st[1]["intervals_flagged"][0]) > int(st[0]["intervals_flagged"][0]) > 0      # the -20 dB threshold silenced station 1 (-28.6 dB)
    p = m.params(1)
    assert tuple(p.raise_intervals) == (1, 2, 3, 4, 5) and tuple(p.clear_intervals) == (5, 4, 3, 2, 1) and p.alarm_mask == 8 and p.silence_db == -math.inf
    assert tuple(m.params(0).raise_intervals) == (3,) * 5 and m.params(2).mono_db == 40.0
    # refused parameters change nothing
    before = m.status()
    for f in (dict(silence_db=math.inf), dict(silence_db=math.nan), dict(loss_db=0.0), dict(loss_db=121.0), dict(antiphase_corr=0.0), dict(antiphase_corr=1.0),
              dict(mono_db=0.0), dict(mono_db=120.5), dict(raise_intervals=0), dict(raise_intervals=(3, 3, 3, 3, 36001)), dict(clear_intervals=0),
              dict(clear_intervals=(36001, 2, 2, 2, 2)), dict(alarm_mask=32)):
        with pytest.raises(pkg.FmdError) as e:
            m.set_params(0, **f)
        assert e.value.status == -1, f
    assert audmon_ref.params_tuple(m.params(0)) == (-60.0, 30.0, 0.5, 40.0, (3,) * 5, (2,) * 5, 15)
    assert np.array_equal(bits(m.status()), bits(before))
    # reset(1): station 1 as after create with its parameters kept, the others untouched; reset_peaks(0): the held peaks alone
    m.reset(1)
    chans[1].reset()
    st = m.status()
    _same(st, chans, "after reset(1)")
    assert int(st[1]["frames"]) == 0 and not st[1]["hold_peak"].any() and int(st[1]["flags"]) == 0 and int(st[1]["ok"]) == 1
    assert not st[1]["ring_ll"].any() and st[0]["ring_ll"].any() and m.params(1).alarm_mask == 8
    m.reset_peaks(0)
    chans[0].reset_peaks()
    _same(m.status(), chans, "after reset_peaks(0)")
    assert not m.status()[0]["hold_peak"].any() and m.status()[2]["hold_peak"].all()
    # the open interval survived reset_peaks and went with reset: the next call tells
    flags, ok = m.process(xd[:, cuts[4]:], n=2 * M)
    for c in range(3):
        chans[c].process(x1[c, cuts[4]:cuts[4] + 2 * M])
    _same(m.status(), chans, "after the next call", flags.cpu().numpy(), ok.cpu().numpy())
    m.reset()
    for ch in chans:
        ch.reset()
    _same(m.status(), chans, "after reset()")
    assert not m.status()["frames"].any() and m.status()["ok"].tolist() == [1, 1, 1]
    torch.cuda.synchronize()


def test_odd_stride_and_odd_view(pkg, ref, x1, pre):
    """rows with an odd in_stride > n, so that every other row starts 8 bytes off a 16-byte boundary, taken in two calls of which the
    second starts at an odd frame"""
    import torch
    n = 9 * M + 333
    stride = n + 8
    assert stride % 2 == 1
    xp = torch.full((3, stride, 2), float("nan"), device="cuda")
    xp[:, :n] = _cuda(x1[:, :n])
    assert xp[1].data_ptr() % 16 == 8
    chans = _ref_start(ref, pre)
    for c in range(3):
        chans[c].process(x1[c, :n])
    m = _start(pkg, pre)
    m.process(xp, n=1001)
    v = xp[:, 1001:]
    assert v.data_ptr() % 16 == 8
    flags, ok = m.process(v, n=n - 1001)
    _same(m.status(), chans, "odd stride", flags.cpu().numpy(), ok.cpu().numpy())
    assert flags.cpu().numpy().tolist() == [16, 16, 16] and [int(v) for v in m.status()["intervals"]] == [9, 9, 10]


def test_special_samples(pkg, ref, x1):
    """All-zero input is silent at silence_db = -inf (the comparison is strict) and the other detectors hold.  Denormals count (they are
    kept): a station of one denormal value on both rails is not silent there, and mono.  An inf or NaN sample makes its interval's sums
    non-finite: the interval counts in `nonfinite` and as silent; the peaks drop a NaN."""
    n = 6 * M + 50
    clean = x1[0, :n]                                                        # stereo x 2, mono x 2 (MONO), stereo (cleared), mono
    x = np.stack([clean] * 6).copy()
    x[0] = 0.0                                                               # silence
    x[1] = np.float32(1e-42)                                                 # denormal L and R throughout: l * l = 1e-84 is a normal double
    x[2, 0::2 * M, 0] = np.inf                                               # intervals 0, 2, 4
    x[2, M + 7::2 * M, 1] = -np.inf                                          # intervals 1, 3, 5
    x[3, 255::M] = np.nan                                                    # every interval, the last lane of a row
    x[4, M + 11, 1] = np.nan                                                 # interval 1 alone
    prm = dict(raise_intervals=2, clear_intervals=1, silence_db=-math.inf)
    m = pkg.AudioMonitor(6, FS)
    m.set_params(**prm)
    flags, ok = m.process(_cuda(x))
    flags, ok = flags.cpu().numpy(), ok.cpu().numpy()
    st = m.status()
    chans = [ref.run(FS, x[c], **prm) for c in range(6)]
    _same(st, chans, "special samples", flags, ok, nan_ok=True)
    assert [int(v) for v in st["nonfinite"]] == [0, 0, 6, 6, 1, 0] and (st["intervals"] == 6).all()
    assert flags.tolist() == [1, 16, 1, 1, 0, 0] and ok.tolist() == [0, 1, 0, 0, 1, 1]
    assert st[0]["run"].tolist() == [0] * 5 and not st[0]["hold_peak"].any() and not st[0]["ring_ll"].any()
    assert st[1]["ring_ll"][0] > 0 and (st[1]["last_peak"] == np.float32(1e-42)).all() and pkg.audmon_side_mid_db(st[1], FS, 1) == -math.inf
    assert np.isinf(st[2]["hold_peak"]).all() and np.isnan(st[3]["ring_ll"][:6]).all()
    assert np.isfinite(st[3]["hold_peak"]).all() and (st[3]["hold_peak"] <= st[5]["hold_peak"]).all() and np.isfinite(st[3]["last_peak"]).all()
    # clean again behind the NaN: intervals 2 ... 5 of station 4 are those of station 5, and its R alone was hit
    for f in ("ring_ll", "ring_rr", "ring_lr"):
        assert np.array_equal(bits(st[4][f][2:6]), bits(st[5][f][2:6]))
    assert np.isnan(st[4]["ring_rr"][1]) and np.isnan(st[4]["ring_lr"][1]) and np.isfinite(st[4]["ring_ll"][1])
    assert st[4]["transitions"].tolist() == st[5]["transitions"].tolist() == [0, 0, 0, 0, 2] and st[4]["run"].tolist() == [0, 0, 0, 0, 1]


@pytest.mark.parametrize("fs", [32000, 48000])
def test_other_rates(pkg, ref, fs):
    """M = 3200 and 4800: no multiples of 256, so an interval's last row is partial and the next interval's rows start off the rows' grid
    in memory"""
    Mm = fs // 10
    n = 9 * Mm + 333
    x = np.stack([audmon_ref.seq_signal(fs, 1.0 + c, seed=fs + c, lead=c)[:n] for c in range(2)]).astype(np.float32)
    m = pkg.AudioMonitor(2, fs)
    m.set_params(**SP)
    flags, ok = m.process(_cuda(x), n=4 * Mm + 1)
    flags, ok = m.process(_cuda(x[:, 4 * Mm + 1:]), flags=flags, ok=ok)
    chans = [ref.run(fs, x[c], **SP) for c in range(2)]
    _same(m.status(), chans, f"{fs}", flags.cpu().numpy(), ok.cpu().numpy())
    assert (m.status()["intervals"] == 9).all() and flags.cpu().numpy().tolist() == [16, 16]


def test_device_records_and_argument_errors(pkg, x1, pre, basic):
    import ctypes as C
    import torch
    m = _start(pkg, pre, max_input_frames=N1)
    xd = _cuda(x1)
    m.process(xd)
    # the device's own records
    torch.cuda.synchronize()
    ptr = m.status_dev_ptr()

    class _Arr:
        __cuda_array_interface__ = {"shape": (3 * 840,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    raw = torch.as_tensor(_Arr(), device="cuda").clone()
    assert np.array_equal(raw.cpu().numpy(), bits(basic[0])) and np.array_equal(bits(m.status()), bits(basic[0]))
    bad = [lambda: m.process(xd, n=N1 + 1),                       # n > in_stride and > max_input_frames
           lambda: m.process(xd, n=-1),
           lambda: m.reset(3), lambda: m.reset(-2), lambda: m.reset_peaks(3), lambda: m.reset_peaks(-2), lambda: m.params(3), lambda: m.params(-1),
           lambda: m._check(m.L.fmd_audmon_set_params(m.a, 3, C.byref(pkg.audmon_default_params())))]
    for k, f in enumerate(bad):
        with pytest.raises(pkg.FmdError) as e:
            f()
        assert e.value.status == -1, k                            # FMD_ERR_ARG
    small = pkg.AudioMonitor(3, FS, max_input_frames=4096)
    with pytest.raises(pkg.FmdError) as e:
        small.process(xd, n=4097)
    assert e.value.status == -1 and int(small.status()[0]["frames"]) == 0
    for f in (lambda: m.process(xd[:2]), lambda: m.process(xd, active=torch.ones(2, dtype=torch.uint8, device="cuda")),
              lambda: m.process(xd.double()), lambda: m.process(xd[:, :, :1]), lambda: m.process(xd, flags=torch.zeros(2, dtype=torch.uint8, device="cuda")),
              lambda: m.process(xd, ok=torch.zeros(3, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(TypeError):
        m.set_params(0, threshold=3.0)
    # a pointer that is not aligned to a frame
    with pytest.raises(pkg.FmdError) as e:
        m._check(m.L.fmd_audmon_process_f32_dev(m.a, xd.data_ptr() + 4, N1, 16, None, None, None, None))
    assert e.value.status == -1
    for cfg in ((0, FS, 64), (3, 7990, 64), (3, 192010, 64), (3, 8005, 64), (3, FS, 0), (3, FS, (1 << 30) + 1)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.AudioMonitor(cfg[0], cfg[1], max_input_frames=cfg[2])
        assert e.value.status == -1
    for fs in (8000, 192000):
        pkg.AudioMonitor(1, fs, max_input_frames=1 << 30).close()
    assert np.array_equal(bits(m.status()), bits(basic[0]))


def test_cpp_adaptor(pkg, ref, x1, tmp_path):
    """tests/cpp/audmon_main.cpp takes a file of audio in calls of 1000 frames; what it prints is the restatement's, and it exits with 7
    unless the records behind fmd_audmon_status_dev are those of fmd_audmon_get_status"""
    exe = tmp_path / "audmon_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'fm-radio_amd' / 'host'}", "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "audmon_main.cpp"),
                    f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)],
                   check=True)
    n = 37 * M + 123                                              # station 0 ends in its zeros: SILENCE and RIGHT_LOST
    a = np.ascontiguousarray(x1[:2, :n])
    a.tofile(tmp_path / "audio.f32")
    out = subprocess.run([str(exe), str(tmp_path / "audio.f32"), "2", str(FS), "1000", "3", "2"], check=True, capture_output=True, text=True).stdout
    lines = out.strip().split("\n")
    assert len(lines) == 2
    for c, line in enumerate(lines):
        w = line.split()
        ch = ref.run(FS, a[c], **SP)
        assert bytes.fromhex(w[0]) == ch.status()[0].tobytes(), c
        assert (int(w[1]), int(w[2])) == (ch.flags, ch.ok)
        got, want = [float(v) for v in w[3:7]], [ch.level_db(2, 1), ch.balance_db(2), ch.correlation(30), ch.side_mid_db(1)]
        assert all(g == v or (math.isnan(g) and math.isnan(v)) for g, v in zip(got, want)), (c, got, want)
    assert ref.run(FS, a[0], **SP).flags == 5


def test_demodulator_end_to_end(pkg, ref):
    """Three stations at 256 kSa/s through BatchDemod in the tolerance mode, ten blocks of 16384 samples (2048 frames of audio at 32 kHz
    each), the monitor with 3 intervals to raise and 2 to clear on audio_tensor() after each block.  Station 0 is oracle/synth.py's
    realistic stereo station with default controls, station 1 the same capture with audio_out = FMD_AUDIO_LPR (the demodulator then
    writes L == R bit for bit), station 2 all-zero IQ.  The CPU oracle's audio of the same three inputs reads [0, MONO, SILENCE] from the
    fifth block on (side / mid -2.7 ... -4.6 dB for station 0 and -inf for station 1, exact zeros for station 2).  Records and bytes equal
    the restatement run on the same audio copied to the host; the flags settle to [0, MONO, SILENCE]; a mixer bus mixed with active = ok
    is, bit for bit, the bus mixed with the same mask built on the host, and not the bus mixed with active = None."""
    import torch
    fs, bs, nb = 256_000, 16384, 10
    cap = synth.to_cf32(synth.fm_capture_realistic(bs * nb, fs=float(fs), seed=41)["iq"])
    x = torch.from_numpy(np.stack([cap, cap, np.zeros_like(cap)])).cuda()
    dm = pkg.BatchDemod(3, bs, fs, fast_math=True)
    ctl = pkg.default_controls()
    assert ctl.audio_out == pkg.FMD_AUDIO_STEREO
    ctl.audio_out = pkg.FMD_AUDIO_LPR
    dm.set_controls(ctl, 1)
    mon = pkg.AudioMonitor(3, 32000, max_input_frames=bs // 8)
    mon.set_params(**SP)
    chans = [ref.channel(32000, **SP) for _ in range(3)]
    mixers = [pkg.AudioMixer(3, [[0, 1, 2]]) for _ in range(3)]
    flags = ok = None
    seen, differs = [], False
    for b in range(nb):
        dm.process(x[:, b * bs:(b + 1) * bs].contiguous())
        dm.synchronize()
        a = dm.audio_tensor()
        assert tuple(a.shape) == (3, bs // 8, 2)
        flags, ok = mon.process(a, flags=flags, ok=ok)
        ah = a.cpu().numpy()
        for c in range(3):
            chans[c].process(ah[c])
        _same(mon.status(), chans, f"block {b}", flags.cpu().numpy(), ok.cpu().numpy())
        seen.append(flags.cpu().numpy().tolist())
        bus = mixers[0].process(a, active=ok).clone()
        host_mask = torch.tensor([ch.ok for ch in chans], dtype=torch.uint8, device="cuda")
        assert torch.equal(bus.view(torch.int32), mixers[1].process(a, active=host_mask).view(torch.int32)), b
        if seen[-1] == [0, 16, 1]:
            differs = differs or not torch.equal(bus, mixers[2].process(a))
        assert np.array_equal(ah[1, :, 0].view(np.uint32), ah[1, :, 1].view(np.uint32))    # FMD_AUDIO_LPR: L == R bit for bit
    st = mon.status()
    print("flags per block", seen, "level", [pkg.audmon_level_db(st[c], 32000, 2, 3) for c in range(3)],
          "side/mid", [pkg.audmon_side_mid_db(st[c], 32000, 3) for c in range(2)])
    assert seen[0] == [0, 0, 0] and all(s == [0, 16, 1] for s in seen[4:]) and ok.cpu().numpy().tolist() == [1, 1, 0]
    assert differs and (st["intervals"] == nb * (bs // 8) // 3200).all() and [t.tolist() for t in st["transitions"]] == [[0] * 5, [0, 0, 0, 0, 1], [1, 0, 0, 0, 0]]
    assert pkg.audmon_side_mid_db(st[1], 32000, 3) == -math.inf and pkg.audmon_level_db(st[2], 32000, 2, 3) < -70.0 < -30.0 < pkg.audmon_level_db(st[0], 32000, 2, 3)
    dm.close(); mon.close()
