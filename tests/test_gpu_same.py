"""EAS SAME decoder on the GPU (fmd_same_*, SameDecoder): status records and the flags and ok bytes against the C restatement of the
arithmetic contract (tests/cpp/same_ref.c, itself checked in test_same_cpu.py), bit for bit: one call, a call per 100 frames on
alternating streams, calls of 1, 63, 64, 65 and 513 ticks' worth of frames +- 1, n = 0, batch and row invariance, the `active` mask, NULL
byte arrays, odd strides and views, parameter and mask changes and resets between bursts, the alert flag's three ways, a ring that wraps,
a 268-byte message, messages cut off by silence and by a reset, zero / denormal / inf / NaN frames, 32 and 48 kHz, argument errors, the
C++ adaptor, and demodulator -> decoder -> mixer end to end.

The main cases run at fs = 8000, where a tick is 1 or 2 frames, with three stations and a header of 25 characters (a burst of about 5 000
frames).  Station c has its own amplitude, clock ratio and noise, and has taken OFF[c] frames of its own before the calls under test, so
that its ticks, bits and bursts stand at different places of every call than its neighbours'."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import same_ref
import synth
from same_ref import EOM, HEADER24, bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FS = 8000
GAP = 700                  # frames of near-silence behind a burst: 45 bits
AMP = (0.25, 0.05, 1.5)
RATIO = (0.99, 1.0, 1.01)
OFF = (0, 277, 531)        # frames each station has taken before (no multiples of the tick, of 4 or of each other)
NOISE_DB = 30.0            # each station's noise floor below its burst's power


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return same_ref.build(tmp_path_factory.mktemp("same_ref_gpu"))


def _station(ref, c, fs=FS, gap=GAP):
    """station c's whole stream: three header bursts and three NNNN bursts under its own noise"""
    x = np.concatenate([np.zeros((OFF[c] + 150, 2), np.float32), ref.encode(HEADER24, fs, RATIO[c], AMP[c], 3, gap), ref.encode(EOM, fs, RATIO[c], AMP[c], 3, gap)])
    return same_ref.add_noise(x, AMP[c], NOISE_DB, 100 + c)


@pytest.fixture(scope="module")
def streams(ref):
    s = [_station(ref, c) for c in range(3)]
    n = min(a.shape[0] - OFF[c] for c, a in enumerate(s))
    return [a[:OFF[c] + n] for c, a in enumerate(s)]


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
    return [ref.run(FS, streams[c]) for c in range(3)]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _start(pkg, pre, **kw):
    """a decoder of three stations whose station c has taken its OFF[c] frames"""
    import torch
    m = pkg.SameDecoder(3, FS, **kw)
    pd = _cuda(pre)
    for c in (1, 2):
        active = torch.zeros(3, dtype=torch.uint8, device="cuda")
        active[c] = 1
        for a in range(0, OFF[c], kw.get("max_input_frames", 1 << 16)):
            m.process(pd[:, a:], n=min(OFF[c] - a, kw.get("max_input_frames", 1 << 16)), active=active, flags=False, ok=False)
    return m


def _ref_start(ref, pre, **params):
    return [ref.channel(FS, **params).process(pre[c, :OFF[c]]) for c in range(3)]


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
        for f in same_ref.STATUS_DTYPE.names:
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


def test_one_call(pkg, want1, basic, x1):
    st, flags, ok = basic
    _same(st, want1, "one call", flags, ok)
    for c in range(3):
        ms = same_ref.ring_messages(st[c])
        assert [m[1] for m in ms] == [1, 1, 1, 2, 2, 2] and all(m[2].startswith(HEADER24) for m in ms[:3]) and all(m[2].startswith(EOM) for m in ms[3:]), (c, ms)
        assert int(st[c]["frames"]) == x1.shape[1] + OFF[c] and int(st[c]["ticks"]) == (int(st[c]["frames"]) * 12500) // (3 * FS)
    assert flags.tolist() == [0, 0, 0] and ok.tolist() == [1, 1, 1] and (st["syncs"] >= 6).all()


def test_call_per_100_frames_on_alternating_streams(pkg, ref, x1, pre, basic):
    """with the restatement fed the same pieces: the records after the first 31 calls (inside the first burst: a message in progress) and at
    the end, where they are the one-call records"""
    import torch
    xd = _cuda(x1)
    m = _start(pkg, pre, max_input_frames=100)
    chans = _ref_start(ref, pre)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    flags = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    ok = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    N1 = x1.shape[1]
    for k, a in enumerate(range(0, N1, 100)):
        b = min(a + 100, N1)
        m.process(xd[:, a:], n=b - a, flags=flags, ok=ok, stream=streams[k % 2])
        if k <= 30:
            for c in range(3):
                chans[c].process(x1[c, a:b])
        if k == 30:
            st = m.status()
            _same(st, chans, "30 calls in", flags.cpu().numpy(), ok.cpu().numpy())
            assert (st["synced"] == 1).all() and (st["msg_len"] > 0).all() and flags.cpu().numpy().tolist() == [1, 1, 1]
    st = m.status()
    assert np.array_equal(bits(st), bits(basic[0])) and np.array_equal(flags.cpu().numpy(), basic[1]) and np.array_equal(ok.cpu().numpy(), basic[2])


@pytest.mark.parametrize("step", [1, 2, 3, 120, 121, 122, 123, 124, 125, 126, 984, 985, 986])
def test_call_lengths(pkg, ref, x1, pre, basic, step):
    """calls of 1, 63, 64, 65 and 513 ticks' worth of frames (1.92 frames a tick: 1.92, 120.96, 122.88, 124.8 and 984.96), each +- 1 frame:
    a row of 64 ticks that ends just before, at and just behind a call's end.  The shortest three run over the first 2 000 frames (into the
    first burst's message), the others over everything."""
    xd = _cuda(x1)
    N = 2000 if step <= 3 else x1.shape[1]
    m = _start(pkg, pre, max_input_frames=step)
    flags = ok = None
    for a in range(0, N, step):
        flags, ok = m.process(xd[:, a:], n=min(step, N - a), flags=flags, ok=ok)
    if step <= 3:
        chans = _ref_start(ref, pre)
        for c in range(3):
            chans[c].process(x1[c, :N])
        _same(m.status(), chans, f"step {step}", flags.cpu().numpy(), ok.cpu().numpy())
        assert (m.status()["synced"] == 1).all()
    else:
        assert np.array_equal(bits(m.status()), bits(basic[0])) and np.array_equal(flags.cpu().numpy(), basic[1]) and np.array_equal(ok.cpu().numpy(), basic[2])


def test_n_zero_and_null_byte_arrays(pkg, ref, x1, pre):
    import torch
    xd = _cuda(x1)
    m = pkg.SameDecoder(3, FS)
    flags = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    ok = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    m.process(xd, n=0, flags=flags, ok=ok)
    assert flags.cpu().numpy().tolist() == [0, 0, 0] and ok.cpu().numpy().tolist() == [1, 1, 1]
    _same(m.status(), [ref.channel(FS)] * 3, "n = 0 on a fresh decoder")
    n = 6000                                                      # behind the first burst: the alert is open, an alarm for station 0
    chans = _ref_start(ref, pre)
    chans[0].set_params(alarm_mask=2)
    for c in range(3):
        chans[c].process(x1[c, :n])
    assert [ch.flags & 2 for ch in chans] == [2, 2, 2] and [ch.ok for ch in chans] == [0, 1, 1]
    for kw in (dict(), dict(flags=False), dict(ok=False), dict(flags=False, ok=False)):
        m = _start(pkg, pre)
        m.set_params(0, alarm_mask=2)
        f, o = m.process(xd, n=n, **kw)
        assert (f is None) == ("flags" in kw) and (o is None) == ("ok" in kw)
        _same(m.status(), chans, str(kw), None if f is None else f.cpu().numpy(), None if o is None else o.cpu().numpy())
        before = m.status()
        flags.fill_(0xAA)
        ok.fill_(0xAA)
        m.process(xd[:, n:], n=0, flags=flags, ok=ok)
        assert flags.cpu().numpy().tolist() == [ch.flags for ch in chans] and ok.cpu().numpy().tolist() == [0, 1, 1]
        m._check(m.L.fmd_same_process_f32_dev(m.d, xd.data_ptr(), x1.shape[1], 0, None, None, None, None))
        assert np.array_equal(bits(m.status()), bits(before))


def test_batch_and_row_invariance(pkg, ref, x1):
    """a station alone, in a batch of 3, and the same stations in every row of a batch of 130, over the first burst and a half"""
    n = 8000
    chans = [ref.run(FS, x1[c, :n]) for c in range(3)]
    alone = pkg.SameDecoder(1, FS)
    f1, o1 = alone.process(_cuda(x1[:1, :n]))
    _same(alone.status(), chans[:1], "alone", f1.cpu().numpy(), o1.cpu().numpy())
    three = pkg.SameDecoder(3, FS)
    f3, o3 = three.process(_cuda(x1[:, :n]))
    _same(three.status(), chans, "C = 3", f3.cpu().numpy(), o3.cpu().numpy())
    x = np.stack([x1[(c + 1) % 3, :n] for c in range(130)])                  # row 129 carries station 1, row 2 station 0
    m = pkg.SameDecoder(130, FS)
    f, o = m.process(_cuda(x))
    st = m.status()
    _same(st, [chans[(c + 1) % 3] for c in range(130)], "C = 130", f.cpu().numpy(), o.cpu().numpy())
    assert np.array_equal(bits(st[2]), bits(alone.status()[0])) and np.array_equal(bits(st[129]), bits(three.status()[1]))
    assert (st["accepted"] == 1).all() and (st["synced"] == 1).all()


def test_active_mask(pkg, ref, x1, pre):
    """a skipped station keeps its records and its two bytes: both byte arrays are pre-filled with 0xAA before every call"""
    import torch
    cuts = (0, 3001, 5555, 9002)
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
    before = m.status()
    flags = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    m.process(xd, active=torch.zeros(3, dtype=torch.bool, device="cuda"), flags=flags, ok=False)
    assert np.array_equal(bits(m.status()), bits(before)) and flags.cpu().numpy().tolist() == [0xAA] * 3


def test_odd_stride_and_odd_view(pkg, ref, x1, pre):
    """rows with an odd in_stride > n, so that every other row starts 8 bytes off a 16-byte boundary, taken in two calls of which the second
    starts at an odd frame"""
    import torch
    n = 7333
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
    assert (m.status()["accepted"] == 1).all()


def test_parameters_masks_holds_and_resets(pkg, ref, x1, pre):
    """between bursts: station 0 gets pull = 0 (a free-running clock) and later 64, station 1 an alarm mask and a hold of 500 ticks, which
    closes its alert 960 frames behind every header burst, station 2 is reset inside the second burst, which cuts that message off.
    The alert opens with the first ZCZC and closes with the first NNNN."""
    xd = _cuda(x1)
    m = _start(pkg, pre)
    chans = _ref_start(ref, pre)
    assert same_ref.params_tuple(m.params(1)) == (16, 750000, 0, 0)
    N1 = x1.shape[1]
    cuts = (0, 5800, 8000, 11500, 17100, 19000, 21000, N1)
    steps = [{}, {0: dict(pull=0), 1: dict(alarm_mask=2, hold_ticks=500)}, {2: "reset"}, {0: dict(pull=64), 1: dict(alarm_mask=3)}, {}, {1: dict(alarm_mask=1)}, {0: dict(alarm_mask=3)}]
    seen = []
    for k in range(7):
        for c, f in steps[k].items():
            if f == "reset":
                m.reset(c)
                chans[c].reset()
            else:
                m.set_params(c, **f)
                assert chans[c].set_params(**f) == 0
        _same(m.status(), chans, f"before call {k}")             # (the record's ok follows the alarm mask at once)
        flags, ok = m.process(xd[:, cuts[k]:], n=cuts[k + 1] - cuts[k])
        for c in range(3):
            chans[c].process(x1[c, cuts[k]:cuts[k + 1]])
        _same(m.status(), chans, f"call {k}", flags.cpu().numpy(), ok.cpu().numpy())
        seen.append((flags.cpu().numpy().tolist(), ok.cpu().numpy().tolist()))
    st = m.status()
    assert [f[0] & 2 for f, _ in seen] == [2, 2, 2, 2, 2, 0, 0]                   # station 0: open from the first ZCZC to the first NNNN
    assert [f[1] & 2 for f, _ in seen] == [2, 0, 2, 2, 0, 0, 0] and seen[1][1][1] == 1 and seen[2][1][1] == 0   # station 1: closed by its hold, reopened by the next burst
    assert int(st[2]["accepted"]) == 4 and int(st[2]["frames"]) == N1 - cuts[2]    # station 2 lost the burst the reset cut, and the one before
    assert int(st[1]["accepted"]) == 6 and m.params(1).hold_ticks == 500 and m.params(0).pull == 64
    before = m.status()
    for f in (dict(pull=-1), dict(pull=129), dict(hold_ticks=0), dict(hold_ticks=1 << 31), dict(alarm_mask=4), dict(reserved=1)):
        with pytest.raises(pkg.FmdError) as e:
            m.set_params(0, **f)
        assert e.value.status == -1, f
    assert np.array_equal(bits(m.status()), bits(before)) and same_ref.params_tuple(m.params(0)) == (64, 750000, 3, 0)
    m.reset()
    for ch in chans:
        ch.reset()
    _same(m.status(), chans, "after reset()")
    assert not m.status()["frames"].any() and m.status()["ok"].tolist() == [1, 1, 1] and m.messages() == [[], [], []]


def test_ring_wrap_long_message_and_cut_off(pkg, ref):
    """station 0: eleven short messages (the ring keeps the newest eight; messages() hands out what is new); station 1: a 268-byte message,
    then one that starts with neither ZCZC nor NNNN; station 2: a message cut off by silence"""
    many = np.concatenate([ref.encode(b"ZCZC-MSG-%03d-" % i, FS, 1.0, 0.25, 1, 400) for i in range(11)])
    long = b"ZCZC-" + bytes(0x30 + i % 10 for i in range(263))
    two = np.concatenate([ref.encode(long, FS, 1.0, 0.25, 1, 800), ref.encode(b"HELLO-WORLD", FS, 1.0, 0.25, 1, 800)])
    cut = ref.encode(HEADER24, FS, 1.0, 0.25, 1, 0)
    cut = cut[:cut.shape[0] - 6 * 8 * 16]
    n = max(many.shape[0], two.shape[0])
    x = np.zeros((3, n, 2), np.float32)
    x[0, :many.shape[0]], x[1, :two.shape[0]], x[2, :cut.shape[0]] = many, two, cut
    chans = [ref.channel(FS) for _ in range(3)]
    m = pkg.SameDecoder(3, FS)
    xd = _cuda(x)
    half = many.shape[0] * 4 // 11 + 100                          # behind the fourth short message
    got = []
    for a, b in ((0, half), (half, n)):
        flags, ok = m.process(xd[:, a:], n=b - a)
        for c in range(3):
            chans[c].process(x[c, a:b])
        _same(m.status(), chans, f"to {b}", flags.cpu().numpy(), ok.cpu().numpy())
        got.append(m.messages())
    assert [t[2] for t in got[0][0]] == [b"ZCZC-MSG-%03d-" % i for i in range(4)] and [t[2] for t in got[1][0]] == [b"ZCZC-MSG-%03d-" % i for i in range(4, 11)]
    st = m.status()
    assert int(st[0]["accepted"]) == 11 and [t[2] for t in same_ref.ring_messages(st[0])] == [b"ZCZC-MSG-%03d-" % i for i in range(3, 11)]
    assert [t[2] for t in got[0][1] + got[1][1]] == [long] and (int(st[1]["accepted"]), int(st[1]["rejected"]), int(st[1]["syncs"])) == (1, 1, 2)
    text = (got[0][2] + got[1][2])[0][2]
    assert len(got[0][2] + got[1][2]) == 1 and text[:18] == HEADER24[:18] and len(text) < len(HEADER24)
    assert m.messages() == [[], [], []]


def test_special_samples(pkg, ref, x1):
    """all-zero frames decide 0 at every tick and take no message; a denormal burst decodes (denormals are kept); an inf or a NaN frame makes
    the eight windows it stands in undecided (s = 0) and the decoder goes on behind it"""
    n = 6000
    one = ref.encode(HEADER24, FS, 1.0, 0.25, 1, 962)[:n]
    x = np.zeros((5, n, 2), np.float32)
    x[1] = (one * np.float32(4e-42 / 0.25)).astype(np.float32)               # 2 900 denormal steps of amplitude
    x[2] = one
    x[2, 100, 0] = np.inf                                                    # in the preamble
    x[2, 5500, 1] = -np.inf                                                  # in the silence
    x[3] = one
    x[3, 150::1000] = np.nan
    x[4] = one
    x[4, 5999, 0] = np.nan                                                   # the last frame: the open tick carries a NaN
    assert np.abs(x[1]).max() < 1.2e-38 and np.count_nonzero(x[1]) > 4000
    m = pkg.SameDecoder(5, FS)
    flags, ok = m.process(_cuda(x), n=4000)
    flags, ok = m.process(_cuda(x[:, 4000:]), flags=flags, ok=ok)
    chans = [ref.run(FS, x[c]) for c in range(5)]
    st = m.status()
    _same(st, chans, "special samples", flags.cpu().numpy(), ok.cpu().numpy(), nan_ok=True)
    assert int(st[0]["bits"]) == int(st[0]["ticks"]) // 8 and int(st[0]["syncs"]) == 0 and not st[0]["hist"].any()
    assert [t[2] for t in same_ref.ring_messages(st[1])] == [HEADER24] == [t[2] for t in same_ref.ring_messages(st[2])]
    assert np.isnan(st[4]["open"]).any() or np.isnan(st[4]["hist"]).any()


@pytest.mark.parametrize("fs", [32000, 48000])
def test_other_rates(pkg, ref, fs):
    """7 or 8 and 11 or 12 frames a tick: rows of about 490 and 740 frames; two stations, two calls of which the first ends inside a tick"""
    x = [np.concatenate([np.zeros((OFF[c + 1], 2), np.float32), ref.encode(HEADER24, fs, RATIO[2 * c], AMP[c], 2, fs // 10), ref.encode(EOM, fs, RATIO[2 * c], AMP[c], 1, fs // 4)])
         for c in range(2)]
    n = min(a.shape[0] for a in x)
    x = np.stack([same_ref.add_noise(a[:n], AMP[c], NOISE_DB, fs + c) for c, a in enumerate(x)])
    m = pkg.SameDecoder(2, fs, max_input_frames=1 << 17)
    cut = 3 * fs // 10 + 1
    flags, ok = m.process(_cuda(x), n=cut)
    flags, ok = m.process(_cuda(x[:, cut:]), flags=flags, ok=ok)
    chans = [ref.run(fs, x[c]) for c in range(2)]
    st = m.status()
    _same(st, chans, f"{fs}", flags.cpu().numpy(), ok.cpu().numpy())
    assert [[t[1] for t in ms] for ms in m.messages()] == [[1, 1, 2], [1, 1, 2]] and flags.cpu().numpy().tolist() == [0, 0]


def test_device_records_and_argument_errors(pkg, x1, pre, basic):
    import ctypes as C
    import torch
    N1 = x1.shape[1]
    m = _start(pkg, pre, max_input_frames=N1)
    xd = _cuda(x1)
    m.process(xd)
    torch.cuda.synchronize()
    ptr = m.status_dev_ptr()

    class _Arr:
        __cuda_array_interface__ = {"shape": (3 * 2856,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    raw = torch.as_tensor(_Arr(), device="cuda").clone()
    assert np.array_equal(raw.cpu().numpy(), bits(basic[0])) and np.array_equal(bits(m.status()), bits(basic[0]))
    bad = [lambda: m.process(xd, n=N1 + 1), lambda: m.process(xd, n=-1), lambda: m.reset(3), lambda: m.reset(-2), lambda: m.params(3), lambda: m.params(-1),
           lambda: m._check(m.L.fmd_same_set_params(m.d, 3, C.byref(pkg.same_default_params())))]
    for k, f in enumerate(bad):
        with pytest.raises(pkg.FmdError) as e:
            f()
        assert e.value.status == -1, k                            # FMD_ERR_ARG
    small = pkg.SameDecoder(3, FS, max_input_frames=4096)
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
    with pytest.raises(AttributeError):
        m.reset_peaks()
    with pytest.raises(pkg.FmdError) as e:                        # a pointer that is not aligned to a frame
        m._check(m.L.fmd_same_process_f32_dev(m.d, xd.data_ptr() + 4, N1, 16, None, None, None, None))
    assert e.value.status == -1
    for cfg in ((0, FS, 64), (3, 7990, 64), (3, 48010, 64), (3, 96000, 64), (3, 8005, 64), (3, FS, 0), (3, FS, (1 << 30) + 1)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.SameDecoder(cfg[0], cfg[1], max_input_frames=cfg[2])
        assert e.value.status == -1
    for fs in (8000, 44100, 48000):
        pkg.SameDecoder(1, fs, max_input_frames=1 << 30).close()
    assert np.array_equal(bits(m.status()), bits(basic[0]))


def test_cpp_adaptor(pkg, ref, x1, tmp_path):
    """tests/cpp/same_main.cpp takes a file of audio in calls of 1000 frames; what it prints is the restatement's, and it exits with 7 unless
    the records behind fmd_same_status_dev are those of fmd_same_get_status"""
    exe = tmp_path / "same_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'fm-radio_amd' / 'host'}", "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "same_main.cpp"),
                    f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)],
                   check=True)
    n = 12000                                                     # two header bursts: the alert is open, an alarm
    a = np.ascontiguousarray(x1[:2, :n])
    a.tofile(tmp_path / "audio.f32")
    out = subprocess.run([str(exe), str(tmp_path / "audio.f32"), "2", str(FS), "1000", "500000", "2"], check=True, capture_output=True, text=True).stdout
    lines = out.strip().split("\n")
    assert len(lines) == 2
    for c, line in enumerate(lines):
        w = line.split(" ", 4)
        ch = ref.run(FS, a[c], hold_ticks=500000, alarm_mask=2)
        assert bytes.fromhex(w[0]) == ch.status()[0].tobytes(), c
        assert (int(w[1]), int(w[2]), int(w[3])) == (ch.flags, ch.ok, 1) and ch.ok == 0
        assert w[4] == " ".join(f"{t} {k} {b.decode()}|" for t, k, b in ch.messages()) and len(ch.messages()) == 2


def test_demodulator_end_to_end(pkg, ref):
    """fmd_same_encode's audio at 32 kHz, a header burst and later an NNNN burst, frequency-modulated the way oracle/synth.py builds its
    captures (mono MPX 0.40 (L + R) / 1.6 and a 0.10 pilot, 75 kHz deviation, 256 kSa/s, to_cf32) -> BatchDemod in the tolerance mode ->
    SameDecoder on audio_tensor() after each block of 2048 frames: station 0 gives the header's text back and opens and closes its alert;
    station 1 carries the realistic noise-like programme and station 2 nothing.  Records and bytes equal the restatement run on the same
    audio copied to the host; with alarm_mask = ALERT_OPEN a mixer bus mixed with active = ok is, bit for bit, the bus mixed with the same
    mask built on the host, and while the alert is open not the bus mixed with active = None."""
    import torch
    fs, bs, nb = 256_000, 16384, 20
    text = b"ZCZC-WXR-SVR-039173+0030-"
    audio = np.concatenate([np.zeros((1500, 2), np.float32), pkg.same_encode(text, 32000, 1.0, 0.4, 1, 3000), pkg.same_encode(EOM, 32000, 1.0, 0.4, 1, 3000)])
    assert audio.shape[0] <= nb * bs // 8
    mono = np.zeros(nb * bs // 8)
    mono[:audio.shape[0]] = audio[:, 0]
    t8 = np.arange(nb * bs, dtype=np.float64) / 8.0
    up = np.interp(t8, np.arange(mono.shape[0], dtype=np.float64), mono)     # to 256 kSa/s
    t = np.arange(nb * bs, dtype=np.float64) / fs
    mpx = 0.40 * (2.0 * up) / 1.6 + 0.10 * np.sin(2.0 * np.pi * 19000.0 * t)
    iq = np.exp(1j * 2.0 * np.pi * 75000.0 * np.cumsum(mpx) / fs)
    prog = synth.to_cf32(synth.fm_capture_realistic(bs * nb, fs=float(fs), seed=41)["iq"])
    tone = synth.to_cf32(iq)
    x = torch.from_numpy(np.stack([tone, prog, np.zeros_like(tone)])).cuda()
    dm = pkg.BatchDemod(3, bs, fs, fast_math=True)
    dec = pkg.SameDecoder(3, 32000, max_input_frames=bs // 8)
    dec.set_params(alarm_mask=same_ref.ALERT_OPEN)
    chans = [ref.channel(32000, alarm_mask=same_ref.ALERT_OPEN) for _ in range(3)]
    mixers = [pkg.AudioMixer(3, [[0, 1, 2]]) for _ in range(3)]
    flags = ok = None
    seen, differs, msgs = [], False, []
    for b in range(nb):
        dm.process(x[:, b * bs:(b + 1) * bs].contiguous())
        dm.synchronize()
        a = dm.audio_tensor()
        assert tuple(a.shape) == (3, bs // 8, 2)
        flags, ok = dec.process(a, flags=flags, ok=ok)
        ah = a.cpu().numpy()
        for c in range(3):
            chans[c].process(ah[c])
        _same(dec.status(), chans, f"block {b}", flags.cpu().numpy(), ok.cpu().numpy())
        seen.append(flags.cpu().numpy().tolist())
        msgs += dec.messages()[0]
        bus = mixers[0].process(a, active=ok).clone()
        host_mask = torch.tensor([ch.ok for ch in chans], dtype=torch.uint8, device="cuda")
        assert torch.equal(bus.view(torch.int32), mixers[1].process(a, active=host_mask).view(torch.int32)), b
        if seen[-1][0] & same_ref.ALERT_OPEN:
            differs = differs or not torch.equal(bus, mixers[2].process(a))
    st = dec.status()
    print("flags per block", seen, "messages", msgs)
    assert [(k, m[:len(text)] if k == 1 else m[:4]) for _, k, m in msgs] == [(1, text), (2, EOM)]
    assert pkg.same_parse(msgs[0][2])["event"] == "SVR" and pkg.same_parse(msgs[0][2])["locations"] == ["039173"]
    opened = [f[0] & same_ref.ALERT_OPEN for f in seen]
    assert opened[0] == 0 and 2 in opened and opened[-1] == 0 and differs and ok.cpu().numpy().tolist() == [1, 1, 1]
    assert int(st[1]["accepted"]) == 0 and int(st[2]["accepted"]) == 0 and int(st[2]["syncs"]) == 0
    dm.close(); dec.close()
