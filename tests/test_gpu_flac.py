"""FLAC audio encoder on the GPU (fmd_flac_*, FlacEncoder): the output bytes, both counts and the status records against the C
restatement of the contract (tests/cpp/flac_ref.c, whose streams test_flac_cpu.py decodes with a decoder written from RFC 9639), bit for
bit: one call, a call per block, ragged splits on alternating streams with the records checked behind every piece, n = 0, batch and row
invariance, the `active` mask over pre-filled outputs, the bytes behind the written frames, NULL count pointers, out_stride at its
minimum and below it, odd strides and views, resets and flushes mid-block and at fill 0, inf / NaN / denormal / overflowing samples,
the coded frame number's length boundaries and its wrap, the device's records, argument errors, the C++ recorder's files, and
demodulator -> encoder -> decoder against fmd_audio_pcm16_dev's PCM.

The main cases run three stations per block size S = 64, 576 and 4096.  Station c has its own amplitude, its own order of the CPU
tests' signals, and has taken OFF(S)[c] = 0, 5 or S - 1 frames of its own before the calls under test, so that its blocks end at
different places of every call than its neighbours'."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import flac_ref
import synth
from flac_ref import bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SIZES = (64, 576, 4096)
AMP = (0.05, 0.3, 0.9)
FS = 32000
FILL = 0xAA
FILL32 = -0x55555556


def _off(S):
    return (0, 5, S - 1)


def _n1(S):
    """frames per station of the calls under test: the ragged splits' 200 + 3 S frames and a rest that ends inside a block"""
    return 200 + 3 * S + 2 * S + 77


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return flac_ref.build(tmp_path_factory.mktemp("flac_ref_gpu"))


def _stream(S, c):
    """station c's whole stream [OFF[c] + N1, 2] float32: pieces of the CPU tests' signals, in the station's own order, at its amplitude
    (0.9: the square wave still clamps)"""
    n = _off(S)[c] + _n1(S)
    sig = flac_ref.signals(n, S)
    names = sorted(sig)
    piece = max(1, n // 11)
    x = np.zeros((n, 2), np.float32)
    for i, a in enumerate(range(0, n, piece)):
        x[a:a + piece] = sig[names[(5 * i + 3 * c) % len(names)]][a:a + piece]
    return (x * np.float32(AMP[c])).astype(np.float32)


_CACHE = {}


def _case(ref, S):
    """per S, computed once and not changed by any test: what the calls under test take (x1 [3, N1, 2]), what each station took before
    (pre [3, S - 1, 2]), and the restatement's bytes, frame counts and records after x1 in one piece"""
    if S not in _CACHE:
        off, n1 = _off(S), _n1(S)
        streams = [_stream(S, c) for c in range(3)]
        x1 = np.stack([streams[c][off[c]:] for c in range(3)])
        pre = np.zeros((3, S - 1, 2), np.float32)
        for c in range(3):
            pre[c, :off[c]] = streams[c][:off[c]]
        chans = _ref_start(ref, S, pre)
        want = [chans[c].process(x1[c]) for c in range(3)]
        _CACHE[S] = dict(x1=x1, pre=pre, want=want, status=[ch.status()[0] for ch in chans], n1=n1)
    return _CACHE[S]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _start(pkg, S, pre, **kw):
    """an encoder of three stations whose station c has taken its OFF[c] frames"""
    import torch
    e = pkg.FlacEncoder(3, S, FS, **kw)
    pd = _cuda(pre)
    for c in (1, 2):
        active = torch.zeros(3, dtype=torch.uint8, device="cuda")
        active[c] = 1
        out, nby, nfr = e.process(pd, n=_off(S)[c], active=active)
        assert nby.cpu().numpy().tolist() == [0, 0, 0] and nfr.cpu().numpy().tolist() == [0, 0, 0]
    return e


def _ref_start(ref, S, pre):
    chans = [ref.channel(S, FS) for _ in range(3)]
    for c in range(3):
        assert chans[c].process(pre[c, :_off(S)[c]])[1] == 0
    return chans


def _filled(shape, dtype):
    import torch
    return torch.full(shape, FILL if dtype == torch.uint8 else FILL32, dtype=dtype, device="cuda")


def _same_status(got, chans, what=""):
    for c, ch in enumerate(chans):
        want = ch.status()[0] if hasattr(ch, "status") else ch
        for f in flac_ref.STATUS_DTYPE.names:
            assert np.array_equal(np.atleast_1d(got[c][f]), np.atleast_1d(want[f])), (what, c, f, got[c][f], want[f])


def _same_call(out, nby, nfr, want, what=""):
    """a call's outputs == the restatement's (bytes, frames) of every station, and the bytes behind them as they were pre-filled"""
    out = out.cpu().numpy()
    nby = None if nby is None else nby.cpu().numpy()
    nfr = None if nfr is None else nfr.cpu().numpy()
    for c, (b, nf) in enumerate(want):
        if nby is not None:
            assert int(nby[c]) == b.size, (what, c, "bytes", int(nby[c]), b.size)
        if nfr is not None:
            assert int(nfr[c]) == nf, (what, c, "frames", int(nfr[c]), nf)
        k = b.size
        assert np.array_equal(out[c, :k], b), (what, c, "first difference at byte", int(np.argmax(out[c, :k] != b)), "of", k)
        assert (out[c, k:] == FILL).all(), (what, c, "bytes behind the frames")


def _process(pkg, e, xd, n, S, slack=8, **kw):
    """one call into pre-filled outputs of out_stride = the minimum + slack"""
    import torch
    out = _filled((e.n_channels, flac_ref.max_bytes(S, n) + slack), torch.uint8)
    kw.setdefault("nbytes", _filled((e.n_channels,), torch.int32))
    kw.setdefault("nframes", _filled((e.n_channels,), torch.int32))
    return e.process(xd, n=n, out=out, **kw)


@pytest.mark.parametrize("S", SIZES)
def test_one_call(pkg, ref, S):
    k = _case(ref, S)
    e = _start(pkg, S, k["pre"])
    out, nby, nfr = _process(pkg, e, _cuda(k["x1"]), k["n1"], S)
    _same_call(out, nby, nfr, k["want"], "one call")
    st = e.status()
    _same_status(st, k["status"], "one call")
    assert [int(v) for v in st["frames"]] == [k["n1"] + _off(S)[c] for c in range(3)] and [int(v) for v in nfr.cpu()] == [(_off(S)[c] + k["n1"]) // S for c in range(3)]
    assert int(st[2]["clipped"].sum()) > 0 and not st["nonfinite"].any() and not st["streams"].any() and not st["wrapped"].any()
    # the device's stream decodes, through the library and through the RFC's decoder, to exactly q: station 1's first frame starts 5
    # frames before the calls under test
    q, _ = ref.sample(np.concatenate([k["pre"][1, :5], k["x1"][1]]))
    data = out[1, :int(nby[1])].cpu().numpy()
    got = pkg.flac_decode(data, FS, S)
    assert got.shape[0] == int(nfr[1]) * S and np.array_equal(got, q[:got.shape[0]]) and np.array_equal(flac_ref.decode_stream(data, FS, S)[0], got)


@pytest.mark.parametrize("S", SIZES)
def test_a_call_per_block(pkg, ref, S):
    """calls of S frames: station 0 completes its block exactly at every call's end, station 2 one frame into it"""
    k = _case(ref, S)
    xd = _cuda(k["x1"])
    e = _start(pkg, S, k["pre"], max_input_frames=S)
    chans = _ref_start(ref, S, k["pre"])
    for a in range(0, k["n1"], S):
        n = min(S, k["n1"] - a)
        out, nby, nfr = _process(pkg, e, xd[:, a:], n, S)
        _same_call(out, nby, nfr, [chans[c].process(k["x1"][c, a:a + n]) for c in range(3)], f"call at {a}")
    _same_status(e.status(), k["status"], "a call per block")


@pytest.mark.parametrize("S", SIZES)
def test_ragged_splits_on_alternating_streams(pkg, ref, S):
    """1 + 7 + 63 + 64 + 65 + (S - 1) + S + (S + 1) + the rest on two alternating streams: every call's bytes and counts and the records
    behind every piece are the restatement's fed the same pieces, and at the end the one-call bytes and records"""
    import torch
    k = _case(ref, S)
    xd = _cuda(k["x1"])
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    a = 0
    got = [[] for _ in range(3)]
    for i, step in enumerate((1, 7, 63, 64, 65, S - 1, S, S + 1, k["n1"])):
        b = min(a + step, k["n1"])
        with torch.cuda.stream(streams[i % 2]):
            out, nby, nfr = _process(pkg, e, xd[:, a:], b - a, S, stream=streams[i % 2])
        want = [chans[c].process(k["x1"][c, a:b]) for c in range(3)]
        streams[i % 2].synchronize()
        _same_call(out, nby, nfr, want, f"piece {i}")
        _same_status(e.status(), chans, f"behind piece {i}")
        for c in range(3):
            got[c].append(want[c][0])
        a = b
    assert a == k["n1"]
    _same_status(e.status(), k["status"], "splits")
    for c in range(3):
        assert np.array_equal(np.concatenate(got[c]), k["want"][c][0])


def test_n_zero(pkg, ref):
    """n = 0: the counts are written as 0 and nothing else changes, on a fresh encoder and mid-block"""
    S = 64
    k = _case(ref, S)
    xd = _cuda(k["x1"])
    e = pkg.FlacEncoder(3, S, FS)
    out, nby, nfr = _process(pkg, e, xd, 0, S)
    assert nby.cpu().numpy().tolist() == [0, 0, 0] == nfr.cpu().numpy().tolist() and (out.cpu().numpy() == FILL).all() and not bits(e.status()).any()
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    _process(pkg, e, xd, 40, S)
    before = e.status()
    out, nby, nfr = _process(pkg, e, xd[:, 40:], 0, S)
    assert nby.cpu().numpy().tolist() == [0, 0, 0] == nfr.cpu().numpy().tolist() and (out.cpu().numpy() == FILL).all() and np.array_equal(bits(e.status()), bits(before))
    # the open blocks are untouched too: the next call tells
    for c in range(3):
        chans[c].process(k["x1"][c, :40])
    out, nby, nfr = _process(pkg, e, xd[:, 40:], 90, S)
    _same_call(out, nby, nfr, [chans[c].process(k["x1"][c, 40:130]) for c in range(3)], "after n = 0")


def test_batch_and_row_invariance(pkg, ref):
    """a station alone, and the same stations at rows 0 ... 69 of a batch of 70 (every row checked), row 69 carrying station 0"""
    S = 64
    k = _case(ref, S)
    n = 5 * S + 3
    want = [ref.channel(S, FS) for _ in range(3)]
    res = [want[c].process(k["x1"][c, :n]) for c in range(3)]
    alone = pkg.FlacEncoder(1, S, FS)
    out1, nby1, nfr1 = _process(pkg, alone, _cuda(k["x1"][:1, :n]), n, S)
    _same_call(out1, nby1, nfr1, res[:1], "alone")
    _same_status(alone.status(), want[:1], "alone")
    rows = [(69 - c) % 3 for c in range(70)]
    e = pkg.FlacEncoder(70, S, FS)
    out, nby, nfr = _process(pkg, e, _cuda(np.stack([k["x1"][r, :n] for r in rows])), n, S)
    _same_call(out, nby, nfr, [res[r] for r in rows], "C = 70")
    _same_status(e.status(), [want[r] for r in rows], "C = 70")
    assert rows[69] == 0 and np.array_equal(out[69].cpu().numpy(), out1[0].cpu().numpy()) and np.array_equal(bits(e.status()[69]), bits(alone.status()[0]))


def test_active_mask_and_null_counts(pkg, ref):
    """a skipped station keeps its record and its row of d_out, and its counts are 0: the outputs are pre-filled before every call;
    NULL count pointers write the same frames"""
    import torch
    S = 64
    k = _case(ref, S)
    assert k["n1"] >= 570
    cuts = (0, 70, 190, 300)
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    xd = _cuda(k["x1"])
    none = (np.zeros(0, np.uint8), 0)
    for i in range(3):
        a, b = cuts[i], cuts[i + 1]
        active = torch.tensor([1, 0 if i == 1 else 1, 1], dtype=torch.uint8, device="cuda")
        out, nby, nfr = _process(pkg, e, xd[:, a:], b - a, S, active=active if i else None)
        want = [chans[c].process(k["x1"][c, a:b]) if not (i == 1 and c == 1) else none for c in range(3)]
        _same_call(out, nby, nfr, want, f"call {i}")
        _same_status(e.status(), chans, f"call {i}")
    assert int(e.status()[1]["frames"]) == _off(S)[1] + 300 - 120
    before = e.status()
    out, nby, nfr = _process(pkg, e, xd, 100, S, active=torch.zeros(3, dtype=torch.bool, device="cuda"))
    assert np.array_equal(bits(e.status()), bits(before)) and (out.cpu().numpy() == FILL).all() and nby.cpu().numpy().tolist() == [0, 0, 0] == nfr.cpu().numpy().tolist()
    # no counts, then one of the two
    got = _process(pkg, e, xd[:, 300:], 90, S, nbytes=False, nframes=False)
    assert got[1] is None and got[2] is None
    _same_call(got[0], None, None, [chans[c].process(k["x1"][c, 300:390]) for c in range(3)], "no counts")
    _same_status(e.status(), chans, "no counts")
    got = _process(pkg, e, xd[:, 390:], 90, S, nbytes=False)
    assert got[1] is None
    _same_call(got[0], None, got[2], [chans[c].process(k["x1"][c, 390:480]) for c in range(3)], "frames only")
    got = _process(pkg, e, xd[:, 480:], 90, S, nframes=False)
    _same_call(got[0], got[1], None, [chans[c].process(k["x1"][c, 480:570]) for c in range(3)], "bytes only")
    e._check(e.L.fmd_flac_process_f32_dev(e.e, xd.data_ptr(), k["n1"], 0, None, got[0].data_ptr(), 0, None, None, None))      # n = 0 and no counts: nothing to do
    _same_status(e.status(), chans, "n = 0 and no counts")


def test_out_stride_at_and_below_the_minimum(pkg, ref):
    import torch
    S = 64
    k = _case(ref, S)
    xd = _cuda(k["x1"])
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    n = 3 * S + 2                                                            # station 2 (fill 63) completes 4 frames, the others 3
    need = pkg.flac_max_bytes(S, n)
    assert need == 4 * 276
    before = e.status()
    out = _filled((3, need), torch.uint8)
    nby, nfr = _filled((3,), torch.int32), _filled((3,), torch.int32)
    for stride in (need - 4, need + 2, need - 276):                          # 4 below the minimum; no multiple of 4; a frame short
        assert e.L.fmd_flac_process_f32_dev(e.e, xd.data_ptr(), k["n1"], n, None, out.data_ptr(), stride, nby.data_ptr(), nfr.data_ptr(), None) == -1, stride
    assert "out_stride" in e.L.fmd_flac_last_error(e.e).decode()
    assert (out.cpu().numpy() == FILL).all() and (nby.cpu().numpy() == FILL32).all() and (nfr.cpu().numpy() == FILL32).all() and np.array_equal(bits(e.status()), bits(before))
    with pytest.raises(ValueError):
        e.process(xd, n=n, out=_filled((3, need - 4), torch.uint8))          # the binding checks the rows it is given
    out, nby, nfr = _process(pkg, e, xd, n, S, slack=0)                      # exactly the minimum
    want = [chans[c].process(k["x1"][c, :n]) for c in range(3)]
    assert out.shape[1] == need and want[2][1] == 4
    _same_call(out, nby, nfr, want, "minimum out_stride")
    # the rows of one larger array: out_stride is the array's, not the row's
    big = _filled((3, 1500), torch.uint8)
    out, nby, nfr = e.process(xd[:, n:], n=n, out=big[:, 100:100 + need])
    assert out.stride(0) == 1500
    want = [chans[c].process(k["x1"][c, n:2 * n]) for c in range(3)]
    for c in range(3):
        assert int(nby[c]) == want[c][0].size and int(nfr[c]) == want[c][1] and np.array_equal(big[c, 100:100 + want[c][0].size].cpu().numpy(), want[c][0])
        assert (big[c, :100].cpu().numpy() == FILL).all() and (big[c, 100 + want[c][0].size:].cpu().numpy() == FILL).all()


def test_odd_stride_and_odd_view(pkg, ref):
    """rows with an odd in_stride > n, so that every other row starts 8 bytes off a 16-byte boundary, taken in two calls of which the
    second starts at an odd frame; the frames behind n are NaN and must not be seen"""
    import torch
    S = 64
    k = _case(ref, S)
    n = 317
    stride = n + 8
    assert stride % 2 == 1
    xp = torch.full((3, stride, 2), float("nan"), device="cuda")
    xp[:, :n] = _cuda(k["x1"][:, :n])
    assert xp[1].data_ptr() % 16 == 8
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    out, nby, nfr = _process(pkg, e, xp, 131, S)
    _same_call(out, nby, nfr, [chans[c].process(k["x1"][c, :131]) for c in range(3)], "odd stride")
    v = xp[:, 131:]
    assert v.data_ptr() % 16 == 8
    out, nby, nfr = _process(pkg, e, v, n - 131, S)
    _same_call(out, nby, nfr, [chans[c].process(k["x1"][c, 131:n]) for c in range(3)], "odd view")
    _same_status(e.status(), chans, "odd stride")
    assert not e.status()["nonfinite"].any()


def _flush(pkg, e, S, channel=-1, **kw):
    import torch
    out = _filled((e.n_channels, flac_ref.max_bytes(S, 1) + 4), torch.uint8)
    kw.setdefault("nbytes", _filled((e.n_channels,), torch.int32))
    kw.setdefault("nframes", _filled((e.n_channels,), torch.int32))
    return e.flush(channel, out=out, **kw)


@pytest.mark.parametrize("S", SIZES)
def test_resets_and_flushes(pkg, ref, S):
    """flush mid-block for one station and for all, flush at fill 0, reset mid-block for one station and for all: bytes, counts and
    records as the restatement's, and the call after each tells that the open blocks and the frame numbers went where they should"""
    k = _case(ref, S)
    xd = _cuda(k["x1"])
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    cuts = [0, S + 3, 2 * S + 10, 3 * S + 12, 4 * S + 20, 5 * S + 25]

    def call(i, what):
        a, b = cuts[i], cuts[i + 1]
        out, nby, nfr = _process(pkg, e, xd[:, a:], b - a, S)
        _same_call(out, nby, nfr, [chans[c].process(k["x1"][c, a:b]) for c in range(3)], what)
        _same_status(e.status(), chans, what)

    call(0, "before")
    # flush station 1 alone: the others' rows and counts are kept
    out, nby, nfr = _flush(pkg, e, S, 1)
    fill1 = chans[1].fill
    want = chans[1].flush()
    assert want[1] == 1 and fill1 > 0
    o = out.cpu().numpy()
    assert np.array_equal(o[1, :want[0].size], want[0]) and (o[1, want[0].size:] == FILL).all() and (o[[0, 2]] == FILL).all()
    assert nby.cpu().numpy().tolist() == [FILL32, want[0].size, FILL32] and nfr.cpu().numpy().tolist() == [FILL32, 1, FILL32]
    st = e.status()
    _same_status(st, chans, "flush(1)")
    assert (int(st[1]["streams"]), int(st[1]["frame_number"]), int(st[1]["fill"]), int(st[1]["stream_samples"])) == (1, 0, 0, 0)
    pcm, infos = flac_ref.decode_frame(bytes(want[0]), 0, FS, S, 1)[::2]     # (station 1 had written one frame: the short one is number 1)
    assert infos["n"] == fill1
    call(1, "after flush(1)")
    # flush all; then again at fill 0: only the streams' numbers move, counts 0, no byte written
    out, nby, nfr = _flush(pkg, e, S)
    _same_call(out, nby, nfr, [ch.flush() for ch in chans], "flush()")
    _same_status(e.status(), chans, "flush()")
    out, nby, nfr = _flush(pkg, e, S)
    assert (out.cpu().numpy() == FILL).all() and nby.cpu().numpy().tolist() == [0, 0, 0] == nfr.cpu().numpy().tolist()
    assert all(ch.flush() [1] == 0 for ch in chans)
    _same_status(e.status(), chans, "flush() at fill 0")
    call(2, "after flush()")
    # reset station 2 mid-block: its counters, stream and open block go, the others stay
    assert chans[2].fill > 0
    e.reset(2)
    chans[2].reset()
    st = e.status()
    _same_status(st, chans, "reset(2)")
    assert not bits(st[2]).any() and int(st[0]["frames"]) > 0
    call(3, "after reset(2)")
    e.reset()
    for ch in chans:
        ch.reset()
    assert not bits(e.status()).any()
    call(4, "after reset()")
    # flush without counts
    got = _flush(pkg, e, S, nbytes=False, nframes=False)
    assert got[1] is None and got[2] is None
    _same_call(got[0], None, None, [ch.flush() for ch in chans], "flush, no counts")
    _same_status(e.status(), chans, "flush, no counts")


def test_special_samples(pkg, ref):
    """full scale and past it on both sides, silence, denormals, inf and NaN, a finite sample whose scaled value overflows, and the
    clamps' edges: bytes, counts and records as the restatement's"""
    S = 64
    n = 5 * S + 40
    x = np.stack([flac_ref.noise(n, 0.1, 50 + c) for c in range(8)])
    x[0] = flac_ref.signals(n, S)["square"]
    x[1] = 0.0
    x[2] = np.where((np.arange(n) % 8) < 4, np.float32(1e-42), np.float32(-1e-42)).astype(np.float32)[:, None]   # denormals: q = 0
    x[3, 0::50, 0] = np.inf
    x[3, 7::50, 1] = -np.inf
    x[4, [0, 1, 63, 64, 65, n - 1], 0] = np.nan
    x[4, [2, 62, n - 2], 1] = np.nan
    x[5, 5, 0] = 3.0e38                                                      # finite, and infinite after the scale
    x[5, 6, 1] = -3.0e38
    x[5, 7, 0] = 1.0e30                                                      # finite after the scale: clamped
    x[6] = flac_ref.signals(n, S)["edge_ramp"]
    s = flac_ref.SCALE
    x[7, :4, 0] = [np.float32(32767.5) / s, np.float32(32768.5) / s, np.float32(-32768.5) / s, np.float32(-32769.5) / s]
    e = pkg.FlacEncoder(8, S, FS)
    out, nby, nfr = _process(pkg, e, _cuda(x), n, S)
    chans = [ref.channel(S, FS) for _ in range(8)]
    _same_call(out, nby, nfr, [chans[c].process(x[c]) for c in range(8)], "special samples")
    st = e.status()
    _same_status(st, chans, "special samples")
    with np.errstate(over="ignore", invalid="ignore"):
        nonfinite = [int((~np.isfinite(x[c] * s)).sum()) for c in range(8)]
    assert [int(v) for v in st["nonfinite"]] == nonfinite and nonfinite[3] > 0 and nonfinite[4:6] == [9, 2] and st[0]["clipped"].tolist() == [n, n] and st[5]["clipped"].tolist() == [1, 0]
    assert st[7]["clipped"].tolist() == [2, 0] and int(st[6]["clipped"].sum()) > 0
    assert int(nby[1]) == int(nby[2]) == 5 * 15                              # silence and denormals: CONSTANT subframes behind a 7-byte header
    _same_call(*_flush(pkg, e, S), [ch.flush() for ch in chans], "special samples, flushed")


def test_frame_number_boundaries(pkg, ref):
    """the coded frame number on both sides of 0x7F, 0x7FF, 0xFFFF, 0x1FFFFF, 0x3FFFFFF and at 0x7FFFFFFF with the wrap, through the
    debug setter: two frames from each start, bytes and records as the restatement's, and the RFC's decoder reads the numbers"""
    S = 64
    k = _case(ref, S)
    starts = (0x7F, 0x7FF, 0xFFFF, 0x1FFFFF, 0x3FFFFFF, 0x7FFFFFFE, 0x7FFFFFFF, 0)
    C = len(starts)
    x = np.stack([k["x1"][c % 3, :2 * S + 9] for c in range(C)])
    e = pkg.FlacEncoder(C, S, FS)
    chans = [ref.channel(S, FS) for _ in range(C)]
    for c, v in enumerate(starts):
        e.debug_set_frame_number(c, v)
        chans[c].set_frame_number(v)
    _same_status(e.status(), chans, "numbers set")
    out, nby, nfr = _process(pkg, e, _cuda(x), 2 * S + 9, S)
    want = [chans[c].process(x[c]) for c in range(C)]
    _same_call(out, nby, nfr, want, "frame numbers")
    st = e.status()
    _same_status(st, chans, "frame numbers")
    assert st["wrapped"].tolist() == [0, 0, 0, 0, 0, 1, 1, 0] and st["streams"].tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
    assert st["frame_number"].tolist() == [0x81, 0x801, 0x10001, 0x200001, 0x4000001, 0, 1, 2]
    o = out.cpu().numpy()
    for c, v in enumerate(starts):
        _, used, _ = flac_ref.decode_frame(bytes(o[c, :int(nby[c])]), 0, FS, S, v)
        flac_ref.decode_frame(bytes(o[c, :int(nby[c])]), used, FS, S, 0 if v == 0x7FFFFFFF else v + 1)
    # a flush whose short frame is number 2^31 - 1 starts one stream
    e.debug_set_frame_number(0, 0x7FFFFFFF)
    chans[0].set_frame_number(0x7FFFFFFF)
    _same_call(*_flush(pkg, e, S), [ch.flush() for ch in chans], "flush at the wrap")
    st = e.status()
    _same_status(st, chans, "flush at the wrap")
    assert (int(st[0]["streams"]), int(st[0]["wrapped"]), int(st[1]["streams"])) == (1, 1, 1)
    for bad in ((C, 0), (-1, 0), (0, 1 << 31)):
        with pytest.raises(pkg.FmdError) as err:
            e.debug_set_frame_number(*bad)
        assert err.value.status == -1


def _device_records(e, C):
    """a view of the device's own records as [C * 10] int64"""
    import torch
    ptr = e.status_dev_ptr()

    class _Arr:
        __cuda_array_interface__ = {"shape": (C * 10,), "typestr": "<i8", "data": (ptr, False), "version": 2}
    return torch.as_tensor(_Arr(), device="cuda")


def test_device_records_and_argument_errors(pkg, ref):
    import torch
    S = 64
    k = _case(ref, S)
    n1 = k["n1"]
    e = _start(pkg, S, k["pre"], max_input_frames=n1)
    xd = _cuda(k["x1"])
    _process(pkg, e, xd, n1, S)
    torch.cuda.synchronize()
    raw = _device_records(e, 3).clone().cpu().numpy()
    assert np.array_equal(bits(raw), bits(e.status())) and e.status().tobytes() == b"".join(r.tobytes() for r in k["status"])
    big = torch.zeros((3, 8192), dtype=torch.uint8, device="cuda")
    P = e.L.fmd_flac_process_f32_dev
    bad = [lambda: e.process(xd, n=n1 + 1, out=big),                         # n > in_stride and > max_input_frames
           lambda: e.process(xd, n=-1, out=big),
           lambda: e.reset(3), lambda: e.reset(-2), lambda: e.flush(3, out=big), lambda: e.flush(-2, out=big),
           lambda: e._check(e.L.fmd_flac_flush(e.e, -1, big.data_ptr(), 272, None, None, None)),      # below a frame's 276 bytes
           lambda: e._check(e.L.fmd_flac_flush(e.e, -1, big.data_ptr(), 278, None, None, None)),
           lambda: e._check(e.L.fmd_flac_flush(e.e, -1, big.data_ptr() + 2, 8192, None, None, None)),
           lambda: e._check(e.L.fmd_flac_flush(e.e, -1, None, 8192, None, None, None)),
           lambda: e._check(P(e.e, xd.data_ptr() + 4, n1, 16, None, big.data_ptr(), 8192, None, None, None)),      # not aligned to a frame
           lambda: e._check(P(e.e, xd.data_ptr(), n1, 16, None, big.data_ptr() + 2, 8188, None, None, None)),
           lambda: e._check(P(e.e, None, n1, 16, None, big.data_ptr(), 8192, None, None, None)),
           lambda: e._check(P(e.e, xd.data_ptr(), n1, 16, None, None, 8192, None, None, None))]
    for i, f in enumerate(bad):
        with pytest.raises(pkg.FmdError) as err:
            f()
        assert err.value.status == -1, i                                     # FMD_ERR_ARG
    # the other side of the same bounds
    e.process(xd[:, 1:], n=16, out=big)                                      # aligned to a frame, not to 16 bytes
    e._check(P(e.e, xd.data_ptr(), n1, 16, None, big.data_ptr() + 4, 8188, None, None, None))
    e.flush(out=big[:, :276])
    small = pkg.FlacEncoder(3, S, FS, max_input_frames=256)
    small.process(xd, n=256)
    with pytest.raises(pkg.FmdError) as err:
        small.process(xd, n=257)
    assert err.value.status == -1 and int(small.status()[0]["frames"]) == 256
    for f in (lambda: e.process(xd[:2], out=big), lambda: e.process(xd, active=torch.ones(2, dtype=torch.uint8, device="cuda"), out=big),
              lambda: e.process(xd.double(), out=big), lambda: e.process(xd[:, :, :1], out=big), lambda: e.process(xd, out=big[:2]), lambda: e.flush(out=big[:, :272]),
              lambda: e.process(xd, out=big.to(torch.int8)), lambda: e.process(xd, n=16, out=big, nbytes=torch.zeros(3, dtype=torch.int64, device="cuda")),
              lambda: e.process(xd, n=16, out=big, nframes=torch.zeros(2, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(AttributeError):
        e.reset_peaks()
    for cfg in ((0, S, FS, 64), (3, 65, FS, 64), (3, 32, FS, 64), (3, 4672, FS, 64), (3, S, 7999, 64), (3, S, 48001, 64), (3, S, FS, 0), (3, S, FS, (1 << 30) + 1)):
        with pytest.raises(pkg.FmdError) as err:
            pkg.FlacEncoder(cfg[0], cfg[1], cfg[2], max_input_frames=cfg[3])
        assert err.value.status == -1
    for Sv, fs in ((64, 8000), (4608, 48000), (0, 44100)):
        enc = pkg.FlacEncoder(1, Sv, fs, max_input_frames=1 << 30)
        assert enc.frame_bound == pkg.flac_frame_bound(Sv)
        enc.close()


def _read_flac(path, S):
    raw = Path(path).read_bytes()
    h = flac_ref.parse_stream_header(raw[:42])
    assert (h["min_block"], h["max_block"], h["channels"], h["bps"], h["md5"]) == (S, S, 2, 16, bytes(16))
    pcm, infos = flac_ref.decode_stream(raw[42:], h["fs"], S)
    return h, pcm, infos, raw[42:]


def test_cpp_recorder(pkg, ref, tmp_path):
    """tests/cpp/flac_main.cpp records a file of audio in calls of 100 frames through host/flac_recorder_gpu.hpp and ends station 0's
    stream once on the way: every file parses (stream header field by field, frames through the RFC's decoder), its bytes are the
    restatement's, its STREAMINFO states the stream's samples and frame sizes, and all files' samples together are the frames fed; a
    recorder left to its destructor leaves a complete file too"""
    exe = tmp_path / "flac_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'fm-radio_amd' / 'host'}", "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "flac_main.cpp"),
                    f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)],
                   check=True)
    S, n, cut = 64, 1000, 430
    k = _case(ref, 576)
    a = np.ascontiguousarray(k["x1"][:2, :n])
    a.tofile(tmp_path / "audio.f32")
    out = subprocess.run([str(exe), str(tmp_path / "audio.f32"), "2", str(FS), str(S), "100", str(cut), str(tmp_path)], check=True, capture_output=True, text=True).stdout
    lines = out.strip().split("\n")
    assert len(lines) == 2
    for c, line in enumerate(lines):
        w = line.split()
        ch = ref.channel(S, FS)
        q = ref.sample(a[c])[0]
        ends = [500, n] if c == 0 else [n]                                   # (the cut, rounded up to a call of 100)
        assert int(w[1]) == len(ends), c
        start = 0
        for s, end in enumerate(ends):
            body, _ = ch.process(a[c, start:end])
            last, _ = ch.flush()
            h, pcm, infos, raw = _read_flac(tmp_path / f"station_{c}_{s}.flac", S)
            sizes = [f["bytes"] for f in infos]
            assert raw == body.tobytes() + last.tobytes() and np.array_equal(pcm, q[start:end]), (c, s)
            assert (h["fs"], h["total"], h["min_frame"], h["max_frame"]) == (FS, end - start, min(sizes), max(sizes)), (c, s)
            assert np.array_equal(pkg.flac_decode(raw, FS, S), pcm)
            start = end
        assert bytes.fromhex(w[0]) == ch.status()[0].tobytes(), c
        assert not (tmp_path / f"station_{c}_{len(ends)}.flac").exists()
    h, pcm, infos, raw = _read_flac(tmp_path / "left_open_0.flac", S)
    assert h["total"] == 100 == pcm.shape[0] and np.array_equal(pcm, ref.sample(a[0, :100])[0]) and [f["n"] for f in infos] == [64, 36]


def test_demodulator_end_to_end(pkg, ref):
    """Three stations at 256 kSa/s through BatchDemod in the tolerance mode, ten blocks of 16384 samples (2048 frames of audio at 32 kHz
    each), the default encoder (S = 4096) on audio_tensor() after each block: every call's bytes, counts and records are the
    restatement's over the demodulator's own device audio copied to the host, and the stream, flushed, decodes to exactly
    fmd_audio_pcm16_dev's PCM of the same blocks."""
    import torch
    fs, bs, nb_ = 256_000, 16384, 10
    tone = synth.to_cf32(synth.fm_capture(bs * nb_, fs=float(fs), seed=43, channel=0)["iq"])
    prog = synth.to_cf32(synth.fm_capture_realistic(bs * nb_, fs=float(fs), seed=41)["iq"])
    x = torch.from_numpy(np.stack([tone, prog, np.zeros_like(tone)])).cuda()
    dm = pkg.BatchDemod(3, bs, fs, fast_math=True)
    enc = pkg.FlacEncoder(3, max_input_frames=bs // 8)
    S = enc.block_frames
    chans = [ref.channel() for _ in range(3)]
    pcm16 = torch.empty((3, bs // 8, 2), dtype=torch.int16, device="cuda")
    got, pcm = [[] for _ in range(3)], []
    for b in range(nb_):
        dm.process(x[:, b * bs:(b + 1) * bs].contiguous())
        dm.synchronize()
        a = dm.audio_tensor()
        assert tuple(a.shape) == (3, bs // 8, 2)
        out, nby, nfr = _process(pkg, enc, a, bs // 8, S)
        dm.audio_pcm16_into(pcm16)
        torch.cuda.synchronize()
        ah = a.cpu().numpy()
        _same_call(out, nby, nfr, [chans[c].process(ah[c]) for c in range(3)], f"block {b}")
        _same_status(enc.status(), chans, f"block {b}")
        pcm.append(pcm16.cpu().numpy().copy())
        for c in range(3):
            got[c].append(out[c, :int(nby[c])].cpu().numpy())
    out, nby, nfr = _flush(pkg, enc, S)
    _same_call(out, nby, nfr, [ch.flush() for ch in chans], "flush")
    assert nfr.cpu().numpy().tolist() == [0, 0, 0]                           # 10 x 2048 frames are five whole blocks
    pcm = np.concatenate(pcm, axis=1)
    st = enc.status()
    assert [int(v) for v in st["blocks"]] == [5] * 3 and not st["nonfinite"].any()
    for c in range(3):
        data = np.concatenate(got[c])
        dec = pkg.flac_decode(data, 32000)
        assert dec.shape == pcm[c].shape and np.array_equal(dec, pcm[c]), c
        assert np.array_equal(flac_ref.decode_stream(data, 32000, S)[0], pcm[c]), c
        print(f"station {c}: {data.size} bytes for {pcm[c].nbytes} of PCM16: {data.size / pcm[c].nbytes:.4f}")
    assert np.concatenate(got[2]).size == 5 * 14                             # the silent station: CONSTANT subframes
    dm.close(); enc.close()
