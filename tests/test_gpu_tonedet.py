"""Audio tone detector on the GPU (fmd_tonedet_*, ToneDetector): status records and the flags and ok bytes against the C restatement of
the arithmetic contract (tests/cpp/tonedet_ref.c, itself checked in test_tonedet_cpu.py), bit for bit: the detector sequence in one call,
a call per interval, split calls on alternating streams, calls of M - 1, M, M + 1 and 2 M + 5 frames, n = 0, batch and row invariance,
the `active` mask, NULL byte arrays, per-station slot sets, parameter, alarm-mask and frequency changes and resets, odd strides and
views, zero / denormal / inf / NaN samples, 32 and 48 kHz, the device's records, argument errors, the C++ adaptor, and demodulator ->
detector -> mixer end to end.

The main cases run at fs = 8000 (M = 800) with three stations.  Station c has its own amplitude, its own noise and c noise intervals in
front of the pattern, and it has taken OFF[c] frames of its own before the calls under test, so that its intervals end at different
places of every call than its neighbours'."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import synth
import tonedet_ref
from tonedet_ref import bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FS = 8000
M = FS // 10
IV = 42                    # intervals of the shared signal: the ring of 30 wraps
TAIL = 100
N1 = IV * M + TAIL         # frames per station of the calls under test
SCALE = (1.0, 0.37, 2.5)
OFF = (0, 277, 531)        # frames each station has taken before (no multiples of 4)
SP = tonedet_ref.SEQ_PARAMS
ALL8 = (1000, 440, 400, 853, 960, 1050, 1, FS // 2 - 1)


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tonedet_ref.build(tmp_path_factory.mktemp("tonedet_ref_gpu"))


@pytest.fixture(scope="module")
def streams():
    """per station [OFF[c] + N1, 2] float32: the detector sequence on the station's own interval grid"""
    return [tonedet_ref.seq_signal(FS, SCALE[c], seed=tonedet_ref.SEQ_SEED + c, lead=c, total=IV, tail=TAIL + OFF[c]).astype(np.float32) for c in range(3)]


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
    """a detector of three stations with the sequence's run lengths whose station c has taken its OFF[c] frames"""
    import torch
    m = pkg.ToneDetector(3, FS, **kw)
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
        for f in tonedet_ref.STATUS_DTYPE.names:
            g, w = np.atleast_1d(got_st[c][f]).reshape(-1), np.atleast_1d(want[f]).reshape(-1)
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
        want, tr = tonedet_ref.expected_flags(tonedet_ref.seq_conditions(c, IV), **SP)
        assert tr == [4, 2, 2, 2, 2, 2, 0, 0] == st[c]["transitions"].tolist()
        assert st[c]["intervals_flagged"].tolist() == [sum((f >> k) & 1 for f in want) for k in range(8)]
        assert st[c]["freq_hz"].tolist() == list(tonedet_ref.DEFAULT_FREQ)
        # station c's last t1000 interval is number 31 + c: the read-outs are the restatement's and follow the amplitude
        w = IV - 31 - c
        assert pkg.tonedet_share_db(st[c], FS, 0, w) == want1[c].share_db(0, w) and pkg.tonedet_level_db(st[c], FS, 3, 30) == want1[c].level_db(3, 30)
        pw, mm = st[c]["ring_pw"][0][(31 + c) % 30], st[c]["ring_mm"][(31 + c) % 30]
        assert abs(10.0 * math.log10(2.0 * pw / (M * mm))) < 0.01 and abs(10.0 * math.log10(mm / M) - 10.0 * math.log10(2.0 * (0.25 * SCALE[c]) ** 2)) < 0.01


def test_bytes_after_every_interval(pkg, ref, x1, pre):
    """a call per interval of M frames: the two bytes after every call are the restatement's, and the flags the pattern's; slot 0 and
    the EAS pair are alarms"""
    xd = _cuda(x1)
    m = _start(pkg, pre, max_input_frames=M)
    m.set_params(alarm_mask=0x19)
    chans = _ref_start(ref, pre)
    flags = ok = None
    seen = []
    for g in range(IV):
        flags, ok = m.process(xd[:, g * M:], n=M, flags=flags, ok=ok)
        seen.append((flags.cpu().numpy().tolist(), ok.cpu().numpy().tolist()))
    for c in range(3):
        assert chans[c].set_params(alarm_mask=0x19) == 0
        want = tonedet_ref.expected_flags(tonedet_ref.seq_conditions(c, IV), **SP)[0]
        for g in range(IV):
            chans[c].process(x1[c, g * M:(g + 1) * M])
            # station c's interval g ends OFF[c] frames before call g does
            assert seen[g][0][c] == chans[c].flags == want[g], (c, g)
            assert seen[g][1][c] == chans[c].ok == int((chans[c].flags & 0x19) == 0), (c, g)
    assert any(f[0] != f[1] for f, _ in seen) and any(o != [1, 1, 1] for _, o in seen)   # the stations do differ within a call
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
    detector or behind a first call of M - 2 frames, so that the 1-, 3- and 4-frame calls straddle an interval's end inside one lane's
    four frames: a lone frame, a partial quad, a whole one, a quad plus one, a row less one, a whole row, a row plus one, and an
    interval's end inside a quad and inside a row.  Records and bytes are the restatement's after every call."""
    import torch
    xd = _cuda(x1)
    m = pkg.ToneDetector(3, FS)
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
    m = pkg.ToneDetector(3, FS)
    flags = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    ok = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    m.process(xd, n=0, flags=flags, ok=ok)
    assert flags.cpu().numpy().tolist() == [0, 0, 0] and ok.cpu().numpy().tolist() == [1, 1, 1]
    _same(m.status(), [ref.channel(FS)] * 3, "n = 0 on a fresh detector")
    m = _start(pkg, pre)
    m.set_params(alarm_mask=1)
    chans = _ref_start(ref, pre)
    n = 8 * M + 60                                                # slot 0 is up in station 0 (interval 7) and not yet in stations 1, 2
    m.process(xd, n=n)
    before = m.status()
    flags.fill_(0xAA)
    ok.fill_(0xAA)
    got = m.process(xd[:, n:], n=0, flags=flags, ok=ok)
    assert got[0] is flags and got[1] is ok
    for c in range(3):
        chans[c].set_params(alarm_mask=1)
        chans[c].process(x1[c, :n])
    assert flags.cpu().numpy().tolist() == [1, 0, 0] == [ch.flags for ch in chans] and ok.cpu().numpy().tolist() == [0, 1, 1]
    assert np.array_equal(bits(m.status()), bits(before))


def test_null_byte_arrays(pkg, ref, x1, pre):
    """d_flags or d_ok NULL: the other one is written, the records are the same; both NULL with n = 0 is allowed and does nothing"""
    xd = _cuda(x1)
    n = 13 * M + 60                                               # the EAS pair is up in station 0 and not yet in stations 1, 2
    chans = _ref_start(ref, pre)
    for c in range(3):
        chans[c].process(x1[c, :n])
    assert [ch.flags for ch in chans] == [24, 0, 0]
    for kw in (dict(flags=False), dict(ok=False), dict(flags=False, ok=False)):
        m = _start(pkg, pre)
        flags, ok = m.process(xd, n=n, **kw)
        assert (flags is None) == ("flags" in kw) and (ok is None) == ("ok" in kw)
        _same(m.status(), chans, str(kw), None if flags is None else flags.cpu().numpy(), None if ok is None else ok.cpu().numpy())
        m._check(m.L.fmd_tonedet_process_f32_dev(m.t, xd.data_ptr(), N1, 0, None, None, None, None))
        _same(m.status(), chans, str(kw) + ", then n = 0 with no bytes")


def test_batch_and_row_invariance(pkg, ref, x1):
    """a station alone, and the same station at row 69 of a batch of 70 (every row checked), over ten intervals and a bit"""
    n = 10 * M + 77
    chans = [ref.run(FS, x1[c, :n], **SP) for c in range(3)]
    alone = pkg.ToneDetector(1, FS)
    alone.set_params(**SP)
    f1, o1 = alone.process(_cuda(x1[:1, :n]))
    _same(alone.status(), chans[:1], "alone", f1.cpu().numpy(), o1.cpu().numpy())
    x = np.stack([x1[c % 3, :n] for c in range(70)])                         # row 69 carries station 0
    m = pkg.ToneDetector(70, FS)
    m.set_params(**SP)
    f70, o70 = m.process(_cuda(x))
    f70, o70 = f70.cpu().numpy(), o70.cpu().numpy()
    st = m.status()
    _same(st, [chans[c % 3] for c in range(70)], "C = 70", f70, o70)
    assert np.array_equal(bits(st[69]), bits(alone.status()[0])) and f70[69] == f1.cpu().numpy()[0] and o70[69] == o1.cpu().numpy()[0]
    assert int(st[69]["intervals"]) == 10 and int(st[69]["transitions"][0]) == 2


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


def test_slot_sets(pkg, ref, x1):
    """per-station slot sets on the same audio: f = 1 and f = fs / 2 - 1, unused slots between used ones, all eight used, none used and
    the defaults, in two calls of which the first ends inside an interval"""
    sets = ((1, FS // 2 - 1, 1000, 440, 0, 0, 0, 0), (1000, 0, 400, 0, 960, 0, 0, 1050), ALL8, (0,) * 8, tonedet_ref.DEFAULT_FREQ)
    n = 13 * M + 77
    x = np.stack([x1[0, :n]] * len(sets))
    m = pkg.ToneDetector(len(sets), FS)
    m.set_params(**SP)
    chans = []
    for c, f in enumerate(sets):
        m.set_params(c, freq_hz=f)
        chans.append(ref.channel(FS, freq_hz=f, **SP))
    xd = _cuda(x)
    flags, ok = m.process(xd, n=5 * M + 301)
    flags, ok = m.process(xd[:, 5 * M + 301:], flags=flags, ok=ok)
    for ch in chans:
        ch.process(x[0])
    st = m.status()
    _same(st, chans, "slot sets", flags.cpu().numpy(), ok.cpu().numpy())
    # t1000 raised at interval 7 and cleared at 9, the EAS pair raised at 12: each station sees what its slots cover
    assert flags.cpu().numpy().tolist() == [0, 16, 24, 0, 24] and [t.tolist()[:5] for t in st["transitions"]] == [
        [0, 0, 2, 0, 0], [2, 0, 0, 0, 1], [2, 0, 0, 1, 1], [0] * 5, [2, 0, 0, 1, 1]]
    assert not st[3]["ring_pw"].any() and st[3]["ring_mm"][:13].all() and not st[1]["ring_pw"][[1, 3, 5, 6]].any() and st[2]["ring_pw"][:, :13].all()
    # the mid signal's own sum does not depend on the slots, and a slot's sums not on its place or its neighbours
    for c in range(5):
        assert np.array_equal(bits(st[c]["ring_mm"]), bits(st[0]["ring_mm"]))
    assert np.array_equal(bits(st[0]["ring_pw"][2]), bits(st[2]["ring_pw"][0])) and np.array_equal(bits(st[0]["ring_pw"][1]), bits(st[2]["ring_pw"][7]))
    assert np.array_equal(bits(st[1]["ring_pw"][7]), bits(st[4]["ring_pw"][5]))


def test_parameters_frequencies_alarm_masks_and_resets(pkg, ref, x1, pre):
    import torch
    xd = _cuda(x1)
    m = pkg.ToneDetector(3, FS)
    chans = [ref.channel(FS) for _ in range(3)]
    assert tonedet_ref.params_tuple(m.params(1)) == (tonedet_ref.DEFAULT_FREQ, tonedet_ref.DEFAULT_SHARE, -50.0, (20,) * 8, (5,) * 8, 0)
    cuts = (0, 7 * M + 33, 12 * M, 20 * M + 1, 26 * M + 400)
    # between calls (the third set falls between two intervals, the others inside one): every station gets the sequence's
    # run lengths first; then station 1 a floor above its own level, its 1000 Hz slot moved to 1001 Hz and its own run lengths per slot,
    # station 2 share thresholds that the EAS pair misses, all slots alarms; then frequencies back, slots swapped and taken out of use
    steps = [{0: SP, 1: SP, 2: SP},
             {1: dict(floor_db=-15.0, alarm_mask=255, raise_intervals=(1, 2, 3, 4, 5, 6, 7, 8), freq_hz=(1001, 440, 400, 853, 960, 1050, 0, 0)),
              2: dict(share_db=2.0, alarm_mask=255)},
             {0: dict(freq_hz=(440, 1000, 0, 960, 853, 0, 1050, 400)), 1: dict(floor_db=-math.inf, clear_intervals=(8, 7, 6, 5, 4, 3, 2, 1), freq_hz=ALL8),
              2: dict(share_db=(3, 3, 3, 6, 6, 3, 3, 3), floor_db=0.0)},
             {0: dict(alarm_mask=2), 1: dict(alarm_mask=8, freq_hz=tonedet_ref.DEFAULT_FREQ), 2: dict(alarm_mask=0, floor_db=-50.0, freq_hz=0)}]
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
    # station 0 took its swap between two intervals, at once; station 1's open interval (20 M + 1 frames in) is still on all eight
    assert st[0]["freq_hz"].tolist() == [440, 1000, 0, 960, 853, 0, 1050, 400] and st[2]["freq_hz"].tolist() == [0] * 8
    m.set_params(1, freq_hz=(5, 6, 7, 8, 9, 10, 11, 12))
    chans[1].set_params(freq_hz=(5, 6, 7, 8, 9, 10, 11, 12))
    assert m.status()[1]["freq_hz"].tolist() == list(tonedet_ref.DEFAULT_FREQ) and tuple(m.params(1).freq_hz) == (5, 6, 7, 8, 9, 10, 11, 12)
    p = m.params(1)
    assert tuple(p.raise_intervals) == (1, 2, 3, 4, 5, 6, 7, 8) and tuple(p.clear_intervals) == (8, 7, 6, 5, 4, 3, 2, 1) and p.alarm_mask == 8 and p.floor_db == -math.inf
    assert tuple(m.params(0).raise_intervals) == (3,) * 8 and tuple(m.params(2).share_db) == tonedet_ref.DEFAULT_SHARE
    # refused parameters change nothing
    before = m.status()
    for f in (dict(floor_db=math.inf), dict(floor_db=math.nan), dict(share_db=-0.5), dict(share_db=60.5), dict(share_db=(3, 3, 3, 3, 3, 3, 3, math.nan)),
              dict(freq_hz=FS // 2), dict(freq_hz=-1), dict(freq_hz=(0, 0, 0, 0, 0, 0, 0, FS)), dict(raise_intervals=0),
              dict(raise_intervals=(3, 3, 3, 3, 3, 3, 3, 36001)), dict(clear_intervals=0), dict(clear_intervals=(36001, 2, 2, 2, 2, 2, 2, 2)), dict(alarm_mask=256)):
        with pytest.raises(pkg.FmdError) as e:
            m.set_params(0, **f)
        assert e.value.status == -1, f
    assert tonedet_ref.params_tuple(m.params(0)) == ((440, 1000, 0, 960, 853, 0, 1050, 400), tonedet_ref.DEFAULT_SHARE, -50.0, (3,) * 8, (2,) * 8, 2)
    assert np.array_equal(bits(m.status()), bits(before))
    # reset(1): station 1 as after create with its parameters kept and its pending frequencies in force, the others untouched
    m.reset(1)
    chans[1].reset()
    st = m.status()
    _same(st, chans, "after reset(1)")
    assert int(st[1]["frames"]) == 0 and int(st[1]["flags"]) == 0 and int(st[1]["ok"]) == 1 and st[1]["freq_hz"].tolist() == [5, 6, 7, 8, 9, 10, 11, 12]
    assert not st[1]["ring_mm"].any() and st[0]["ring_mm"].any() and m.params(1).alarm_mask == 8
    # the open interval went with the reset: the next call tells
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


def test_frequency_change_mid_interval(pkg, ref):
    """three intervals of a 700 Hz sine; slot 0 goes from 1000 to 700 Hz 300 frames into the second: the open interval finishes on
    1000 Hz, the third is measured on 700 Hz and raises the flag"""
    t = np.arange(3 * M, dtype=np.float64) / FS
    s = (0.25 * np.sin(2.0 * np.pi * 700.0 * t + 0.3)).astype(np.float32)
    x = np.stack([s, s], axis=1)[None]
    one = dict(raise_intervals=1, clear_intervals=1)
    f700 = (700,) + tonedet_ref.DEFAULT_FREQ[1:]
    m = pkg.ToneDetector(1, FS)
    m.set_params(**one)
    ch = ref.channel(FS, **one)
    xd = _cuda(x)
    m.process(xd, n=M + 300)
    ch.process(x[0, :M + 300])
    m.set_params(freq_hz=f700)
    assert ch.set_params(freq_hz=f700) == 0
    _same(m.status(), [ch], "pending")
    assert m.status()[0]["freq_hz"][0] == 1000
    flags, ok = m.process(xd[:, M + 300:], n=M - 300)
    ch.process(x[0, M + 300:2 * M])
    _same(m.status(), [ch], "the open interval finished", flags.cpu().numpy(), ok.cpu().numpy())
    assert m.status()[0]["freq_hz"][0] == 700 and int(flags[0]) == 0 and pkg.tonedet_share_db(m.status()[0], FS, 0, 1) < -60.0
    flags, ok = m.process(xd[:, 2 * M:], flags=flags, ok=ok)
    ch.process(x[0, 2 * M:])
    _same(m.status(), [ch], "the next interval", flags.cpu().numpy(), ok.cpu().numpy())
    assert int(flags[0]) == 1 and abs(pkg.tonedet_share_db(m.status()[0], FS, 0, 1)) < 1e-4


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
    assert flags.cpu().numpy().tolist() == [1, 1, 1] and [int(v) for v in m.status()["intervals"]] == [9, 9, 10]


def test_special_samples(pkg, ref, x1):
    """All-zero input carries no tone at floor_db = -inf (the comparison is strict).  Denormals count (they are kept): a station of a
    denormal 1000 Hz square wave is usable there.  An inf or NaN sample makes its interval's MM non-finite: the interval counts in
    `nonfinite` and carries no tone."""
    n = 6 * M + 50
    clean = x1[0, :n]                                                        # noise x 2, t1000 x 2, noise, t1000
    x = np.stack([clean] * 6).copy()
    x[0] = 0.0                                                               # silence
    sq = np.where((np.arange(n) % 8) < 4, np.float32(1e-42), np.float32(-1e-42)).astype(np.float32)   # 1000 Hz at fs = 8000, denormal
    x[1] = sq[:, None]
    x[2, 0::2 * M, 0] = np.inf                                               # intervals 0, 2, 4
    x[2, M + 7::2 * M, 1] = -np.inf                                          # intervals 1, 3, 5
    x[3, 255::M] = np.nan                                                    # every interval, the last lane of a row
    x[4, 2 * M + 11, 1] = np.nan                                             # interval 2 alone
    prm = dict(raise_intervals=2, clear_intervals=1, floor_db=-math.inf)
    m = pkg.ToneDetector(6, FS)
    m.set_params(**prm)
    flags, ok = m.process(_cuda(x))
    flags, ok = flags.cpu().numpy(), ok.cpu().numpy()
    st = m.status()
    chans = [ref.run(FS, x[c], **prm) for c in range(6)]
    _same(st, chans, "special samples", flags, ok, nan_ok=True)
    assert [int(v) for v in st["nonfinite"]] == [0, 0, 6, 6, 1, 0] and (st["intervals"] == 6).all()
    assert flags.tolist() == [0, 1, 0, 0, 0, 0] and st[5]["transitions"].tolist()[0] == 2 and st[4]["transitions"].tolist()[0] == 0
    assert not st[0]["ring_mm"].any() and not st[0]["ring_pw"].any() and st[0]["run"].tolist() == [0] * 8
    # the fundamental of a square wave of eight samples carries 1 / (8 sin^2(pi / 8)) = 0.854 of its power: -0.69 dB
    assert 0.0 < st[1]["ring_mm"][0] < 1e-80 and abs(pkg.tonedet_share_db(st[1], FS, 0, 6) - 10.0 * math.log10(0.125 / math.sin(math.pi / 8.0) ** 2)) < 0.01
    assert np.isnan(st[3]["ring_mm"][:6]).all() and np.isnan(st[4]["ring_mm"][2]) and np.isnan(st[4]["ring_pw"][:6, 2]).all()
    # clean again behind the NaN: intervals 3 ... 5 of station 4 are those of station 5
    assert np.array_equal(bits(st[4]["ring_mm"][3:6]), bits(st[5]["ring_mm"][3:6])) and np.array_equal(bits(st[4]["ring_pw"][:, 3:6]), bits(st[5]["ring_pw"][:, 3:6]))


@pytest.mark.parametrize("fs", [32000, 48000])
def test_other_rates(pkg, ref, fs):
    """M = 3200 and 4800: no multiples of 256, so an interval's last row is partial and the next interval's rows start off the rows' grid
    in memory; slots at both ends of the range"""
    Mm = fs // 10
    n = 9 * Mm + 333
    f = (1000, 440, 400, 853, 960, 1050, 1, fs // 2 - 1)
    x = np.stack([tonedet_ref.seq_signal(fs, 1.0 + c, seed=fs + c, lead=c)[:n] for c in range(2)]).astype(np.float32)
    m = pkg.ToneDetector(2, fs)
    m.set_params(freq_hz=f, **SP)
    flags, ok = m.process(_cuda(x), n=4 * Mm + 1)
    flags, ok = m.process(_cuda(x[:, 4 * Mm + 1:]), flags=flags, ok=ok)
    chans = [ref.run(fs, x[c], freq_hz=f, **SP) for c in range(2)]
    _same(m.status(), chans, f"{fs}", flags.cpu().numpy(), ok.cpu().numpy())
    assert (m.status()["intervals"] == 9).all() and flags.cpu().numpy().tolist() == [1, 1] and m.status()["ring_pw"][:, :, :9].all()


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
        __cuda_array_interface__ = {"shape": (3 * 2344,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    raw = torch.as_tensor(_Arr(), device="cuda").clone()
    assert np.array_equal(raw.cpu().numpy(), bits(basic[0])) and np.array_equal(bits(m.status()), bits(basic[0]))
    bad = [lambda: m.process(xd, n=N1 + 1),                       # n > in_stride and > max_input_frames
           lambda: m.process(xd, n=-1),
           lambda: m.reset(3), lambda: m.reset(-2), lambda: m.params(3), lambda: m.params(-1),
           lambda: m._check(m.L.fmd_tonedet_set_params(m.t, 3, C.byref(pkg.tonedet_default_params())))]
    for k, f in enumerate(bad):
        with pytest.raises(pkg.FmdError) as e:
            f()
        assert e.value.status == -1, k                            # FMD_ERR_ARG
    small = pkg.ToneDetector(3, FS, max_input_frames=4096)
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
        m._check(m.L.fmd_tonedet_process_f32_dev(m.t, xd.data_ptr() + 4, N1, 16, None, None, None, None))
    assert e.value.status == -1
    for cfg in ((0, FS, 64), (3, 7990, 64), (3, 48010, 64), (3, 96000, 64), (3, 8005, 64), (3, FS, 0), (3, FS, (1 << 30) + 1)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.ToneDetector(cfg[0], cfg[1], max_input_frames=cfg[2])
        assert e.value.status == -1
    for fs in (8000, 48000):
        pkg.ToneDetector(1, fs, max_input_frames=1 << 30).close()
    assert np.array_equal(bits(m.status()), bits(basic[0]))


def test_cpp_adaptor(pkg, ref, x1, tmp_path):
    """tests/cpp/tonedet_main.cpp takes a file of audio in calls of 1000 frames; what it prints is the restatement's, and it exits with 7
    unless the records behind fmd_tonedet_status_dev are those of fmd_tonedet_get_status"""
    exe = tmp_path / "tonedet_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'fm-radio_amd' / 'host'}", "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "tonedet_main.cpp"),
                    f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)],
                   check=True)
    n = 32 * M + 123                                              # station 0 ends behind its last t1000 interval: slot 0 is up, an alarm
    a = np.ascontiguousarray(x1[:2, :n])
    a.tofile(tmp_path / "audio.f32")
    out = subprocess.run([str(exe), str(tmp_path / "audio.f32"), "2", str(FS), "1000", "3", "2"], check=True, capture_output=True, text=True).stdout
    lines = out.strip().split("\n")
    assert len(lines) == 2
    for c, line in enumerate(lines):
        w = line.split()
        ch = ref.run(FS, a[c], alarm_mask=1, **SP)
        assert bytes.fromhex(w[0]) == ch.status()[0].tobytes(), c
        assert (int(w[1]), int(w[2])) == (ch.flags, ch.ok)
        got, want = [float(v) for v in w[3:7]], [ch.share_db(0, 1), ch.level_db(0, 2), ch.share_db(3, 30), ch.level_db(3, 1)]
        assert all(g == v or (math.isnan(g) and math.isnan(v)) for g, v in zip(got, want)), (c, got, want)
    assert (ref.run(FS, a[0], alarm_mask=1, **SP).flags, ref.run(FS, a[0], alarm_mask=1, **SP).ok) == (1, 0)


def test_demodulator_end_to_end(pkg, ref):
    """Three stations at 256 kSa/s through BatchDemod in the tolerance mode, ten blocks of 16384 samples (2048 frames of audio at 32 kHz
    each), the detector with 3 intervals to raise and 2 to clear on audio_tensor() after each block.  Station 0 is oracle/synth.py's
    fm_capture, whose programme is steady tones: by its own parameters 0.5 sin 1000 Hz + 0.3 sin 3300 Hz on the left and 0.5 sin 440 Hz +
    0.3 sin 5000 Hz on the right (channel 0: no jitter), so the slots are 1000, 440, 3300 and 5000 Hz, and 853 Hz as a slot that must stay
    clear.  In the mid signal the two 0.5 tones carry 0.25 each and the two 0.3 tones 0.09 each of 0.68: shares of -4.3 dB for 1000 and
    440 Hz (threshold 8 dB) and of -8.8 dB for 3300 and 5000 Hz (threshold 20 dB), which is what the CPU oracle's audio of the same capture
    reads (-4.35, -4.34, -8.79, -8.80 dB, and -36.6 dB at 853 Hz), with the flags at 15 from the fifth block on.  Station 1 is the realistic
    noise-like programme (the oracle's audio: no slot above -25 dB), station 2 all-zero IQ.  Records and bytes equal the restatement run on
    the same audio copied to the host; the flags settle to [15, 0, 0]: tone, no tone, no tone; with alarm_mask = 1 (the 1000 Hz slot) a
    mixer bus mixed with active = ok is, bit for bit, the bus mixed with the same mask built on the host, and not the bus mixed with
    active = None."""
    import torch
    fs, bs, nb = 256_000, 16384, 10
    tone = synth.to_cf32(synth.fm_capture(bs * nb, fs=float(fs), seed=43, channel=0)["iq"])
    prog = synth.to_cf32(synth.fm_capture_realistic(bs * nb, fs=float(fs), seed=41)["iq"])
    x = torch.from_numpy(np.stack([tone, prog, np.zeros_like(tone)])).cuda()
    dm = pkg.BatchDemod(3, bs, fs, fast_math=True)
    prm = dict(freq_hz=(1000, 440, 3300, 5000, 853, 0, 0, 0), share_db=(8, 8, 20, 20, 6, 3, 3, 3), alarm_mask=1, **SP)
    det = pkg.ToneDetector(3, 32000, max_input_frames=bs // 8)
    det.set_params(**prm)
    chans = [ref.channel(32000, **prm) for _ in range(3)]
    mixers = [pkg.AudioMixer(3, [[0, 1, 2]]) for _ in range(3)]
    flags = ok = None
    seen, differs = [], False
    for b in range(nb):
        dm.process(x[:, b * bs:(b + 1) * bs].contiguous())
        dm.synchronize()
        a = dm.audio_tensor()
        assert tuple(a.shape) == (3, bs // 8, 2)
        flags, ok = det.process(a, flags=flags, ok=ok)
        ah = a.cpu().numpy()
        for c in range(3):
            chans[c].process(ah[c])
        _same(det.status(), chans, f"block {b}", flags.cpu().numpy(), ok.cpu().numpy())
        seen.append(flags.cpu().numpy().tolist())
        bus = mixers[0].process(a, active=ok).clone()
        host_mask = torch.tensor([ch.ok for ch in chans], dtype=torch.uint8, device="cuda")
        assert torch.equal(bus.view(torch.int32), mixers[1].process(a, active=host_mask).view(torch.int32)), b
        if seen[-1] == [15, 0, 0]:
            differs = differs or not torch.equal(bus, mixers[2].process(a))
    st = det.status()
    print("flags per block", seen, "share of station 0", [pkg.tonedet_share_db(st[0], 32000, k, 3) for k in range(5)],
          "of station 1", [pkg.tonedet_share_db(st[1], 32000, k, 3) for k in range(5)])
    assert seen[0] == [0, 0, 0] and all(f == [15, 0, 0] for f in seen[4:]) and ok.cpu().numpy().tolist() == [0, 1, 1]
    assert differs and (st["intervals"] == nb * (bs // 8) // 3200).all() and [t.tolist() for t in st["transitions"]] == [[1, 1, 1, 1, 0, 0, 0, 0], [0] * 8, [0] * 8]
    assert abs(pkg.tonedet_share_db(st[0], 32000, 0, 3) + 4.35) < 0.5 and abs(pkg.tonedet_share_db(st[0], 32000, 1, 3) + 4.35) < 0.5
    assert abs(pkg.tonedet_share_db(st[0], 32000, 2, 3) + 8.8) < 0.5 and abs(pkg.tonedet_share_db(st[0], 32000, 3, 3) + 8.8) < 0.5
    assert pkg.tonedet_share_db(st[0], 32000, 4, 3) < -20.0 and max(pkg.tonedet_share_db(st[1], 32000, k, 3) for k in range(5)) < -20.0
    assert not st[2]["ring_pw"].any() or pkg.tonedet_level_db(st[2], 32000, 0, 3) < -100.0
    dm.close(); det.close()
