"""ADPCM audio encoder on the GPU (fmd_adpcm_*, AdpcmEncoder): the output bytes, the block counts and the status records against the C
restatement of the arithmetic contract (tests/cpp/adpcm_ref.c, itself checked against Python's audioop in test_adpcm_cpu.py), bit for
bit: one call, a call per block, ragged splits on alternating streams with the state checked behind the short pieces, n = 0, batch and
row invariance, the `active` mask over pre-filled outputs, the bytes behind the written blocks, d_nblocks NULL, out_stride at its
minimum and below it, odd strides and views, resets and flushes mid-block and at fill 0, full-scale / silent / denormal / inf / NaN
samples, a frame count above 2^32, the device's records, argument errors, the C++ recorder's files, and demodulator -> encoder end to
end.

The main cases run three stations per block size S = 9, 17 and 1017.  Station c has its own amplitude and has taken OFF(S)[c] = 0, 5 or
S - 1 frames of its own before the calls under test, so that its blocks end at different places of every call than its neighbours'."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import adpcm_ref
import synth
from adpcm_ref import bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SIZES = (9, 17, 1017)
TILE = 128                 # k_adpcm's tile (fm-radio_amd/csrc/fmd_adpcm.hip kTile): the splits below straddle it
AMP = (0.05, 0.3, 0.9)
FILL = 0xAA


def _off(S):
    return (0, 5, S - 1)


def _n1(S):
    """frames per station of the calls under test: the ragged splits' 25 + 3 S + 3 TILE frames and a rest that ends inside a block"""
    return 25 + 3 * S + 3 * TILE + 2 * S + 77


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return adpcm_ref.build(tmp_path_factory.mktemp("adpcm_ref_gpu"))


def _stream(S, c):
    """station c's whole stream [OFF[c] + N1, 2] float32: noise and a sine at the station's amplitude (0.9: past full scale at times)"""
    n = _off(S)[c] + _n1(S)
    return (adpcm_ref.noise(n, 0.5 * AMP[c], 100 * S + c) + adpcm_ref.sine(n, f=700.0 + 300.0 * c, a=AMP[c])).astype(np.float32)


_CACHE = {}


def _case(ref, S):
    """per S, computed once and not changed by any test: the streams, what the calls under test take (x1 [3, N1, 2]), what each station
    took before (pre [3, S - 1, 2]), and the restatement's blocks and records after x1 in one piece"""
    if S not in _CACHE:
        off, n1 = _off(S), _n1(S)
        streams = [_stream(S, c) for c in range(3)]
        x1 = np.stack([streams[c][off[c]:] for c in range(3)])
        pre = np.zeros((3, S - 1, 2), np.float32)
        for c in range(3):
            pre[c, :off[c]] = streams[c][:off[c]]
        chans = _ref_start(ref, S, pre)
        blocks = [chans[c].process(x1[c]) for c in range(3)]
        _CACHE[S] = dict(x1=x1, pre=pre, blocks=blocks, status=[ch.status()[0] for ch in chans], n1=n1)
    return _CACHE[S]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _start(pkg, S, pre, **kw):
    """an encoder of three stations whose station c has taken its OFF[c] frames"""
    import torch
    e = pkg.AdpcmEncoder(3, S, **kw)
    pd = _cuda(pre)
    for c in (1, 2):
        active = torch.zeros(3, dtype=torch.uint8, device="cuda")
        active[c] = 1
        out, nb = e.process(pd, n=_off(S)[c], active=active)
        assert nb.cpu().numpy().tolist() == [0, 0, 0]
    return e


def _ref_start(ref, S, pre):
    chans = [ref.channel(S) for _ in range(3)]
    for c in range(3):
        assert chans[c].process(pre[c, :_off(S)[c]]).shape[0] == 0
    return chans


def _filled(shape, dtype):
    import torch
    return torch.full(shape, FILL if dtype == torch.uint8 else -0x55555556, dtype=dtype, device="cuda")


def _same_status(got, chans, what=""):
    for c, ch in enumerate(chans):
        want = ch.status()[0] if hasattr(ch, "status") else ch
        for f in adpcm_ref.STATUS_DTYPE.names:
            assert np.array_equal(np.atleast_1d(got[c][f]), np.atleast_1d(want[f])), (what, c, f, got[c][f], want[f])


def _same_call(out, nb, blocks, what=""):
    """a call's outputs == the restatement's blocks of every station, and the bytes behind them as they were pre-filled"""
    out = out.cpu().numpy()
    nb = None if nb is None else nb.cpu().numpy()
    for c, b in enumerate(blocks):
        if nb is not None:
            assert int(nb[c]) == b.shape[0], (what, c, int(nb[c]), b.shape[0])
        k = b.size
        assert np.array_equal(out[c, :k], b.reshape(-1)), (what, c, "blocks", int(np.argmax(out[c, :k] != b.reshape(-1))))
        assert (out[c, k:] == FILL).all(), (what, c, "bytes behind the blocks")


def _process(pkg, e, xd, n, S, slack=8, **kw):
    """one call into pre-filled outputs of out_stride = the minimum + slack"""
    import torch
    align = adpcm_ref.block_align(S)
    out = _filled((e.n_channels, (S - 1 + n) // S * align + slack), torch.uint8)
    nb = _filled((e.n_channels,), torch.int32)
    return e.process(xd, n=n, out=out, nblocks=nb, **kw)


@pytest.mark.parametrize("S", SIZES)
def test_one_call(pkg, ref, S):
    k = _case(ref, S)
    e = _start(pkg, S, k["pre"])
    out, nb = _process(pkg, e, _cuda(k["x1"]), k["n1"], S)
    _same_call(out, nb, k["blocks"], "one call")
    st = e.status()
    _same_status(st, k["status"], "one call")
    assert [int(v) for v in st["frames"]] == [k["n1"] + _off(S)[c] for c in range(3)] and [int(v) for v in nb.cpu()] == [(_off(S)[c] + k["n1"]) // S for c in range(3)]
    assert int(st[2]["clipped"].sum()) > 0 and int(st[0]["clipped"].sum()) == 0 and not st["nonfinite"].any() and not st["padded"].any()
    # the library's decoder over the device's blocks follows the 16-bit samples they were made from: station 1's first block starts 5
    # frames before the calls under test (a sanity bar only: 4 bits a sample are worth more than 8 dB even on noise)
    q, _ = ref.sample(k["x1"][1])
    got = pkg.adpcm_decode(out[1, :int(nb[1]) * e.block_align].cpu().numpy(), S)
    assert adpcm_ref.snr_db(q[S - 5:got.shape[0] - 5], got[S:]) > 8.0


@pytest.mark.parametrize("S", SIZES)
def test_a_call_per_block(pkg, ref, S):
    """calls of S frames: station 0 completes its block exactly at every call's end, station 2 one frame into it"""
    k = _case(ref, S)
    xd = _cuda(k["x1"])
    e = _start(pkg, S, k["pre"], max_input_frames=S)
    chans = _ref_start(ref, S, k["pre"])
    for a in range(0, k["n1"], S):
        n = min(S, k["n1"] - a)
        out, nb = _process(pkg, e, xd[:, a:], n, S)
        _same_call(out, nb, [chans[c].process(k["x1"][c, a:a + n]) for c in range(3)], f"call at {a}")
    _same_status(e.status(), k["status"], "a call per block")


@pytest.mark.parametrize("S", SIZES)
def test_ragged_splits_on_alternating_streams(pkg, ref, S):
    """1 + 7 + 8 + 9 + (S - 1) + S + (S + 1) + (TILE - 1) + TILE + (TILE + 1) + the rest on two alternating streams: every call's blocks and
    the records behind every piece are the restatement's fed the same pieces, and at the end the one-call records"""
    import torch
    k = _case(ref, S)
    xd = _cuda(k["x1"])
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    a = 0
    got = [[] for _ in range(3)]
    for i, step in enumerate((1, 7, 8, 9, S - 1, S, S + 1, TILE - 1, TILE, TILE + 1, k["n1"])):
        b = min(a + step, k["n1"])
        with torch.cuda.stream(streams[i % 2]):
            out, nb = _process(pkg, e, xd[:, a:], b - a, S, stream=streams[i % 2])
        want = [chans[c].process(k["x1"][c, a:b]) for c in range(3)]
        streams[i % 2].synchronize()
        _same_call(out, nb, want, f"piece {i}")
        _same_status(e.status(), chans, f"behind piece {i}")
        for c in range(3):
            got[c].append(want[c])
        a = b
    assert a == k["n1"]
    _same_status(e.status(), k["status"], "splits")
    for c in range(3):
        assert np.array_equal(np.concatenate(got[c]), k["blocks"][c])


def test_n_zero(pkg, ref):
    """n = 0: the counts are written as 0 and nothing else changes, on a fresh encoder and mid-block"""
    S = 17
    k = _case(ref, S)
    xd = _cuda(k["x1"])
    e = pkg.AdpcmEncoder(3, S)
    out, nb = _process(pkg, e, xd, 0, S)
    assert nb.cpu().numpy().tolist() == [0, 0, 0] and (out.cpu().numpy() == FILL).all() and not bits(e.status()).any()
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    _process(pkg, e, xd, 40, S)
    before = e.status()
    out, nb = _process(pkg, e, xd[:, 40:], 0, S)
    assert nb.cpu().numpy().tolist() == [0, 0, 0] and (out.cpu().numpy() == FILL).all() and np.array_equal(bits(e.status()), bits(before))
    # the open blocks are untouched too: the next call tells
    for c in range(3):
        chans[c].process(k["x1"][c, :40])
    out, nb = _process(pkg, e, xd[:, 40:], 30, S)
    _same_call(out, nb, [chans[c].process(k["x1"][c, 40:70]) for c in range(3)], "after n = 0")


def test_batch_and_row_invariance(pkg, ref):
    """a station alone, and the same stations at rows 0 ... 69 of a batch of 70 (every row checked): two full groups of 32 stations
    and a group of six, row 69 carrying station 0"""
    S = 17
    k = _case(ref, S)
    n = 5 * S + 3 + TILE
    want = [ref.channel(S) for _ in range(3)]
    blocks = [want[c].process(k["x1"][c, :n]) for c in range(3)]
    alone = pkg.AdpcmEncoder(1, S)
    out1, nb1 = _process(pkg, alone, _cuda(k["x1"][:1, :n]), n, S)
    _same_call(out1, nb1, blocks[:1], "alone")
    _same_status(alone.status(), want[:1], "alone")
    rows = [(69 - c) % 3 for c in range(70)]
    e = pkg.AdpcmEncoder(70, S)
    out, nb = _process(pkg, e, _cuda(np.stack([k["x1"][r, :n] for r in rows])), n, S)
    _same_call(out, nb, [blocks[r] for r in rows], "C = 70")
    _same_status(e.status(), [want[r] for r in rows], "C = 70")
    assert rows[69] == 0 and np.array_equal(out[69].cpu().numpy(), out1[0].cpu().numpy()) and np.array_equal(bits(e.status()[69]), bits(alone.status()[0]))
    # a group with one member: C = 33
    e = pkg.AdpcmEncoder(33, S)
    out, nb = _process(pkg, e, _cuda(np.stack([k["x1"][c % 3, :n] for c in range(33)])), n, S)
    _same_call(out, nb, [blocks[c % 3] for c in range(33)], "C = 33")


def test_active_mask_and_null_counts(pkg, ref):
    """a skipped station keeps its record and its row of d_out, and its count is 0: both outputs are pre-filled before every call;
    d_nblocks NULL writes the same blocks"""
    import torch
    S = 17
    k = _case(ref, S)
    cuts = (0, 40, 90, 150)
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    xd = _cuda(k["x1"])
    for i in range(3):
        a, b = cuts[i], cuts[i + 1]
        active = torch.tensor([1, 0 if i == 1 else 1, 1], dtype=torch.uint8, device="cuda")
        out, nb = _process(pkg, e, xd[:, a:], b - a, S, active=active if i else None)
        want = [chans[c].process(k["x1"][c, a:b]) if not (i == 1 and c == 1) else np.zeros((0, 24), np.uint8) for c in range(3)]
        _same_call(out, nb, want, f"call {i}")
        _same_status(e.status(), chans, f"call {i}")
    assert int(e.status()[1]["frames"]) == _off(S)[1] + 150 - 50
    before = e.status()
    out, nb = _process(pkg, e, xd, 100, S, active=torch.zeros(3, dtype=torch.bool, device="cuda"))
    assert np.array_equal(bits(e.status()), bits(before)) and (out.cpu().numpy() == FILL).all() and nb.cpu().numpy().tolist() == [0, 0, 0]
    # no counts
    out = _filled((3, 7 * 24), torch.uint8)
    got = e.process(xd[:, 150:], n=100, out=out, nblocks=False)
    assert got[0] is out and got[1] is None
    _same_call(out, None, [chans[c].process(k["x1"][c, 150:250]) for c in range(3)], "no counts")
    _same_status(e.status(), chans, "no counts")
    e._check(e.L.fmd_adpcm_process_f32_dev(e.e, xd.data_ptr(), k["n1"], 0, None, out.data_ptr(), 0, None, None))      # n = 0 and no counts: nothing to do
    _same_status(e.status(), chans, "n = 0 and no counts")


def test_out_stride_at_and_below_the_minimum(pkg, ref):
    import torch
    S = 17
    k = _case(ref, S)
    xd = _cuda(k["x1"])
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    n = 3 * S + 2                                                            # station 2 (fill 16) completes 4 blocks = max_blocks, the others 3
    need = pkg.adpcm_max_blocks(S, n) * 24
    assert need == 96
    before = e.status()
    out = _filled((3, need), torch.uint8)
    nb = _filled((3,), torch.int32)
    for stride in (need - 4, need + 2, need - 24):                           # 4 below the minimum; no multiple of 4; a block short
        assert e.L.fmd_adpcm_process_f32_dev(e.e, xd.data_ptr(), k["n1"], n, None, out.data_ptr(), stride, nb.data_ptr(), None) == -1, stride
    assert "out_stride" in e.L.fmd_adpcm_last_error(e.e).decode()
    assert (out.cpu().numpy() == FILL).all() and (nb.cpu().numpy() == -0x55555556).all() and np.array_equal(bits(e.status()), bits(before))
    with pytest.raises(ValueError):
        e.process(xd, n=n, out=_filled((3, need - 4), torch.uint8))          # the binding checks the rows it is given
    out, nb = _process(pkg, e, xd, n, S, slack=0)                            # exactly the minimum: station 2's last block ends the row
    want = [chans[c].process(k["x1"][c, :n]) for c in range(3)]
    assert out.shape[1] == need and want[2].shape[0] == 4
    _same_call(out, nb, want, "minimum out_stride")
    # the rows of one larger array: out_stride is the array's, not the row's
    big = _filled((3, 200), torch.uint8)
    out, nb = e.process(xd[:, n:], n=n, out=big[:, 100:196], nblocks=None)
    assert out.stride(0) == 200
    want = [chans[c].process(k["x1"][c, n:2 * n]) for c in range(3)]
    for c in range(3):
        assert int(nb[c]) == want[c].shape[0] and np.array_equal(big[c, 100:100 + want[c].size].cpu().numpy(), want[c].reshape(-1))
        assert (big[c, :100].cpu().numpy() == FILL).all() and (big[c, 100 + want[c].size:].cpu().numpy() == FILL).all()


def test_odd_stride_and_odd_view(pkg, ref):
    """rows with an odd in_stride > n, so that every other row starts 8 bytes off a 16-byte boundary, taken in two calls of which the
    second starts at an odd frame; the frames behind n are NaN and must not be seen"""
    import torch
    S = 17
    k = _case(ref, S)
    n = 2 * TILE + 61
    stride = n + 8
    assert stride % 2 == 1
    xp = torch.full((3, stride, 2), float("nan"), device="cuda")
    xp[:, :n] = _cuda(k["x1"][:, :n])
    assert xp[1].data_ptr() % 16 == 8
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    out, nb = _process(pkg, e, xp, 131, S)
    _same_call(out, nb, [chans[c].process(k["x1"][c, :131]) for c in range(3)], "odd stride")
    v = xp[:, 131:]
    assert v.data_ptr() % 16 == 8
    out, nb = _process(pkg, e, v, n - 131, S)
    _same_call(out, nb, [chans[c].process(k["x1"][c, 131:n]) for c in range(3)], "odd view")
    _same_status(e.status(), chans, "odd stride")
    assert not e.status()["nonfinite"].any()


@pytest.mark.parametrize("S", SIZES)
def test_resets_and_flushes(pkg, ref, S):
    """flush mid-block for one station and for all, flush at fill 0, reset mid-block for one station and for all: bytes, counts and
    records as the restatement's, and the call after each tells that the open blocks went where they should"""
    import torch
    k = _case(ref, S)
    align = adpcm_ref.block_align(S)
    xd = _cuda(k["x1"])
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    cuts = [0, S + 3, 2 * S + 10, 3 * S + 12, 4 * S + 20, 5 * S + 25]

    def call(i, what):
        a, b = cuts[i], cuts[i + 1]
        out, nb = _process(pkg, e, xd[:, a:], b - a, S)
        _same_call(out, nb, [chans[c].process(k["x1"][c, a:b]) for c in range(3)], what)
        _same_status(e.status(), chans, what)

    call(0, "before")
    # flush station 1 alone: the others' rows and counts are kept
    out, nb = _filled((3, align + 4), torch.uint8), _filled((3,), torch.int32)
    e.flush(1, out=out, nblocks=nb)
    fill1 = chans[1].fill
    want = chans[1].flush()
    assert want.shape[0] == 1 and fill1 > 0
    o = out.cpu().numpy()
    assert np.array_equal(o[1, :align], want[0]) and (o[1, align:] == FILL).all() and (o[[0, 2]] == FILL).all() and nb.cpu().numpy().tolist() == [-0x55555556, 1, -0x55555556]
    st = e.status()
    _same_status(st, chans, "flush(1)")
    assert int(st[1]["padded"]) == S - fill1 and int(st[1]["fill"]) == 0
    call(1, "after flush(1)")
    # flush all; then again at fill 0: nothing changes, counts 0, no byte written
    out, nb = _filled((3, align), torch.uint8), _filled((3,), torch.int32)
    e.flush(out=out, nblocks=nb)
    want = [ch.flush() for ch in chans]
    _same_call(out, nb, want, "flush()")
    _same_status(e.status(), chans, "flush()")
    before = e.status()
    out, nb = _filled((3, align), torch.uint8), _filled((3,), torch.int32)
    e.flush(out=out, nblocks=nb)
    assert (out.cpu().numpy() == FILL).all() and nb.cpu().numpy().tolist() == [0, 0, 0] and np.array_equal(bits(e.status()), bits(before))
    assert all(ch.flush().shape[0] == 0 for ch in chans)
    call(2, "after flush()")
    # reset station 2 mid-block: its counters, predictor, index and open block go, the others stay
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
    out = _filled((3, align), torch.uint8)
    got = e.flush(out=out, nblocks=False)
    assert got[1] is None
    _same_call(out, None, [ch.flush() for ch in chans], "flush, no counts")


def test_special_samples(pkg, ref):
    """full scale and past it on both sides, silence, denormals, inf and NaN at the ends of a tile and of a lane's pair, and a finite
    sample whose scaled value overflows: bytes, counts and records as the restatement's"""
    S = 17
    n = 2 * TILE + 40
    x = np.stack([adpcm_ref.noise(n, 0.1, 50 + c) for c in range(8)])
    x[0] = adpcm_ref.square(n, 2)                                           # past full scale every frame: index 88, the predictor's clamps
    x[1] = 0.0                                                               # silence
    x[2] = np.where((np.arange(n) % 8) < 4, np.float32(1e-42), np.float32(-1e-42)).astype(np.float32)[:, None]   # denormals: q = 0
    x[3, 0::50, 0] = np.inf
    x[3, 7::50, 1] = -np.inf
    x[4, [0, 1, TILE - 1, TILE, TILE + 1, n - 1], 0] = np.nan
    x[4, [2, TILE - 2, n - 2], 1] = np.nan
    x[5, 5, 0] = 3.0e38                                                      # finite, and infinite after the scale
    x[5, 6, 1] = -3.0e38
    x[5, 7, 0] = 1.0e30                                                      # finite after the scale: clamped
    x[6] = adpcm_ref.edge_ramp(n)
    s = adpcm_ref.SCALE
    x[7, :4, 0] = [np.float32(32767.5) / s, np.float32(32768.5) / s, np.float32(-32768.5) / s, np.float32(-32769.5) / s]
    e = pkg.AdpcmEncoder(8, S)
    out, nb = _process(pkg, e, _cuda(x), n, S)
    chans = [ref.channel(S) for _ in range(8)]
    _same_call(out, nb, [chans[c].process(x[c]) for c in range(8)], "special samples")
    st = e.status()
    _same_status(st, chans, "special samples")
    assert [int(v) for v in st["nonfinite"]] == [0, 0, 0, 12, 9, 2, 0, 0] and st[0]["clipped"].tolist() == [n, n] and st[5]["clipped"].tolist() == [1, 0]
    assert st[7]["clipped"].tolist() == [2, 0] and int(st[6]["clipped"].sum()) > 0 and not st[1]["index"].any() and not st[2]["index"].any()
    assert not out[1, :int(nb[1]) * 24].cpu().numpy().any() and not out[2, :int(nb[2]) * 24].cpu().numpy().any()
    assert max(adpcm_ref.parse_block(b, S)["index"][0] for b in out[0, :int(nb[0]) * 24].cpu().numpy().reshape(-1, 24)) == 88


def _device_records(e, C):
    """a writable view of the device's own records as [C * 8] int64"""
    import torch
    ptr = e.status_dev_ptr()

    class _Arr:
        __cuda_array_interface__ = {"shape": (C * 8,), "typestr": "<i8", "data": (ptr, False), "version": 2}
    return torch.as_tensor(_Arr(), device="cuda")


def test_frame_count_above_2_32(pkg, ref):
    """a station that has been running for 37 hours: its frame count starts above 2^32 (set in the device's record) and goes on in 64 bits"""
    import torch
    S = 17
    k = _case(ref, S)
    e = _start(pkg, S, k["pre"])
    chans = _ref_start(ref, S, k["pre"])
    torch.cuda.synchronize()
    rec = _device_records(e, 3)
    start = (1 << 32) + (1 << 31) - 7
    rec[8 * 1] = start                                                       # station 1's frames
    torch.cuda.synchronize()
    chans[1].set_frames(start)
    out, nb = _process(pkg, e, _cuda(k["x1"]), 300, S)
    _same_call(out, nb, [chans[c].process(k["x1"][c, :300]) for c in range(3)], "past 2^32")
    st = e.status()
    _same_status(st, chans, "past 2^32")
    assert int(st[1]["frames"]) == start + 300 > 1 << 32 and int(st[0]["frames"]) == 300


def test_device_records_and_argument_errors(pkg, ref):
    import torch
    S = 17
    k = _case(ref, S)
    n1 = k["n1"]
    e = _start(pkg, S, k["pre"], max_input_frames=n1)
    xd = _cuda(k["x1"])
    _process(pkg, e, xd, n1, S)
    torch.cuda.synchronize()
    raw = _device_records(e, 3).clone().cpu().numpy()
    assert np.array_equal(bits(raw), bits(e.status())) and e.status().tobytes() == b"".join(r.tobytes() for r in k["status"])
    big = torch.zeros((3, 4096), dtype=torch.uint8, device="cuda")
    bad = [lambda: e.process(xd, n=n1 + 1, out=big),                         # n > in_stride and > max_input_frames
           lambda: e.process(xd, n=-1, out=big),
           lambda: e.reset(3), lambda: e.reset(-2), lambda: e.flush(3, out=big), lambda: e.flush(-2, out=big),
           lambda: e._check(e.L.fmd_adpcm_flush(e.e, -1, big.data_ptr(), 20, None, None)),      # below a block's 24 bytes
           lambda: e._check(e.L.fmd_adpcm_flush(e.e, -1, big.data_ptr(), 26, None, None)),
           lambda: e._check(e.L.fmd_adpcm_flush(e.e, -1, big.data_ptr() + 2, 4096, None, None)),
           lambda: e._check(e.L.fmd_adpcm_flush(e.e, -1, None, 4096, None, None)),
           lambda: e._check(e.L.fmd_adpcm_process_f32_dev(e.e, xd.data_ptr() + 4, n1, 16, None, big.data_ptr(), 4096, None, None)),      # not aligned to a frame
           lambda: e._check(e.L.fmd_adpcm_process_f32_dev(e.e, xd.data_ptr(), n1, 16, None, big.data_ptr() + 2, 4092, None, None)),
           lambda: e._check(e.L.fmd_adpcm_process_f32_dev(e.e, None, n1, 16, None, big.data_ptr(), 4096, None, None)),
           lambda: e._check(e.L.fmd_adpcm_process_f32_dev(e.e, xd.data_ptr(), n1, 16, None, None, 4096, None, None))]
    for i, f in enumerate(bad):
        with pytest.raises(pkg.FmdError) as err:
            f()
        assert err.value.status == -1, i                                     # FMD_ERR_ARG
    # the other side of the same bounds
    e.process(xd[:, 1:], n=16, out=big)                                      # aligned to a frame, not to 16 bytes
    e._check(e.L.fmd_adpcm_process_f32_dev(e.e, xd.data_ptr(), n1, 16, None, big.data_ptr() + 4, 4092, None, None))
    e.flush(out=big[:, :24])
    small = pkg.AdpcmEncoder(3, S, max_input_frames=256)
    small.process(xd, n=256)
    with pytest.raises(pkg.FmdError) as err:
        small.process(xd, n=257)
    assert err.value.status == -1 and int(small.status()[0]["frames"]) == 256
    for f in (lambda: e.process(xd[:2], out=big), lambda: e.process(xd, active=torch.ones(2, dtype=torch.uint8, device="cuda"), out=big),
              lambda: e.process(xd.double(), out=big), lambda: e.process(xd[:, :, :1], out=big), lambda: e.process(xd, out=big[:2]), lambda: e.flush(out=big[:, :20]),
              lambda: e.process(xd, out=big.to(torch.int8)), lambda: e.process(xd, out=big, nblocks=torch.zeros(3, dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(AttributeError):
        e.reset_peaks()
    for cfg in ((0, S, 64), (3, 10, 64), (3, 8193, 64), (3, S, 0), (3, S, (1 << 30) + 1)):
        with pytest.raises(pkg.FmdError) as err:
            pkg.AdpcmEncoder(cfg[0], cfg[1], max_input_frames=cfg[2])
        assert err.value.status == -1
    for Sv in (9, 8185, 0):
        enc = pkg.AdpcmEncoder(1, Sv, max_input_frames=1 << 30)
        assert enc.block_align == pkg.adpcm_block_align(Sv)
        enc.close()


def _parse_wav(path):
    raw = Path(path).read_bytes()
    riff, riff_size, wave = struct.unpack_from("<4sI4s", raw, 0)
    fmt, fmt_size, tag, channels, fs, avg, align, bps, cb, spb = struct.unpack_from("<4sIHHIIHHHH", raw, 12)
    fact, fact_size, frames = struct.unpack_from("<4sII", raw, 40)
    data, data_size = struct.unpack_from("<4sI", raw, 52)
    assert (riff, wave, fmt, fact, data) == (b"RIFF", b"WAVE", b"fmt ", b"fact", b"data") and (fmt_size, fact_size, tag, channels, bps, cb) == (20, 4, 0x0011, 2, 4, 2)
    assert riff_size == len(raw) - 8 and data_size == len(raw) - 60 and data_size % align == 0 and avg == fs * align // spb
    return dict(fs=fs, align=align, S=spb, frames=frames, blocks=np.frombuffer(raw[60:], np.uint8).reshape(-1, align))


def test_cpp_recorder(pkg, ref, tmp_path):
    """tests/cpp/adpcm_main.cpp records a file of audio in calls of 100 frames through host/adpcm_recorder_gpu.hpp: each station's WAV
    file parses, its `fact` chunk states the frames fed, its blocks are the restatement's (the flushed one included) and decode to the
    16-bit samples within ADPCM's error; a recorder left to its destructor leaves a complete file too"""
    exe = tmp_path / "adpcm_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'fm-radio_amd' / 'host'}", "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "adpcm_main.cpp"),
                    f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)],
                   check=True)
    S, n = 17, 1000
    k = _case(ref, 1017)
    a = np.ascontiguousarray(k["x1"][:2, :n])
    a.tofile(tmp_path / "audio.f32")
    out = subprocess.run([str(exe), str(tmp_path / "audio.f32"), "2", "32000", str(S), "100", str(tmp_path)], check=True, capture_output=True, text=True).stdout
    lines = out.strip().split("\n")
    assert len(lines) == 2
    for c, line in enumerate(lines):
        w = line.split()
        ch = ref.channel(S)
        blocks = np.concatenate([ch.process(a[c]), ch.flush()])
        assert blocks.shape[0] == 58 + 1 == int(w[1]) and bytes.fromhex(w[0]) == ch.status()[0].tobytes(), c
        f = _parse_wav(tmp_path / f"station_{c}.wav")
        assert (f["fs"], f["align"], f["S"], f["frames"]) == (32000, 24, S, n) and np.array_equal(f["blocks"], blocks), c
        pcm = pkg.adpcm_decode(f["blocks"], S)[:f["frames"]]
        q, _ = ref.sample(a[c])
        assert adpcm_ref.snr_db(q[S:], pcm[S:]) > 8.0, c
    f = _parse_wav(tmp_path / "left_open.wav")
    ch = ref.channel(S)
    blocks = np.concatenate([ch.process(a[0, :100]), ch.flush()])
    assert f["frames"] == 100 and np.array_equal(f["blocks"], blocks) and blocks.shape[0] == 6


def test_demodulator_end_to_end(pkg, ref):
    """Three stations at 256 kSa/s through BatchDemod in the tolerance mode, ten blocks of 16384 samples (2048 frames of audio at 32 kHz
    each), the default encoder (S = 1017) on audio_tensor() after each block: every call's blocks, counts and records are the
    restatement's over the demodulator's own device audio copied to the host.  The decoded PCM against fmd_audio_pcm16_dev's PCM of the
    same blocks has the restatement's SNR, because the bytes are equal; the figures are printed."""
    import torch
    fs, bs, nb_ = 256_000, 16384, 10
    tone = synth.to_cf32(synth.fm_capture(bs * nb_, fs=float(fs), seed=43, channel=0)["iq"])
    prog = synth.to_cf32(synth.fm_capture_realistic(bs * nb_, fs=float(fs), seed=41)["iq"])
    x = torch.from_numpy(np.stack([tone, prog, np.zeros_like(tone)])).cuda()
    dm = pkg.BatchDemod(3, bs, fs, fast_math=True)
    enc = pkg.AdpcmEncoder(3, max_input_frames=bs // 8)
    S = enc.block_frames
    chans = [ref.channel() for _ in range(3)]
    pcm16 = torch.empty((3, bs // 8, 2), dtype=torch.int16, device="cuda")
    got, want, pcm = [[] for _ in range(3)], [[] for _ in range(3)], []
    for b in range(nb_):
        dm.process(x[:, b * bs:(b + 1) * bs].contiguous())
        dm.synchronize()
        a = dm.audio_tensor()
        assert tuple(a.shape) == (3, bs // 8, 2)
        out, nb = _process(pkg, enc, a, bs // 8, S)
        dm.audio_pcm16_into(pcm16)
        torch.cuda.synchronize()
        ah = a.cpu().numpy()
        blocks = [chans[c].process(ah[c]) for c in range(3)]
        _same_call(out, nb, blocks, f"block {b}")
        _same_status(enc.status(), chans, f"block {b}")
        pcm.append(pcm16.cpu().numpy().copy())
        for c in range(3):
            want[c].append(blocks[c])
            got[c].append(out[c, :int(nb[c]) * 1024].cpu().numpy().reshape(-1, 1024))
    pcm = np.concatenate(pcm, axis=1)
    st = enc.status()
    assert [int(v) for v in st["blocks"]] == [nb_ * (bs // 8) // S] * 3 == [20] * 3 and not st["nonfinite"].any()
    for c in range(2):
        g, w = np.concatenate(got[c]), np.concatenate(want[c])
        dec_g, dec_w = pkg.adpcm_decode(g), ref.decode(w, S)
        snr_g, snr_w = adpcm_ref.snr_db(pcm[c, S:20 * S], dec_g[S:]), adpcm_ref.snr_db(pcm[c, S:20 * S], dec_w[S:])
        print(f"station {c}: decoded ADPCM against fmd_audio_pcm16_dev's PCM from the second block on: {snr_g:.2f} dB (the restatement's blocks: {snr_w:.2f} dB)")
        assert snr_g == snr_w and snr_g > 8.0
        # the headers' samples are fmd_audio_pcm16_dev's own
        assert np.array_equal(dec_g[::S], pcm[c, :20 * S:S])
    assert not np.concatenate(got[2]).any()
    dm.close(); enc.close()
