"""Look-ahead peak limiter on the GPU against the C restatement (tests/cpp/limiter_ref.c), bit for bit, on outputs, d_gr and status
records: three stations with gains 0.5, 1.7 and 4.0 that have taken 0, 5 and W - 1 frames of their own beforehand, at every (D, step) of
{0, 1, 47, 255} x {1, 6711, 2^30}, over streams of three kernel tiles and 2W + 77 frames of tests/limiter_ref.py's signal (that the
signal reaches every path of the limiter is tests/test_limiter_cpu.py's test_gpu_signals_reach_every_path)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import adpcm_ref
import limiter_ref as R
import synth
from limiter_ref import ONE, bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TILE = 1024                # k_limiter's tile (fm-radio_amd/csrc/fmd_limiter.hip kTile): the splits below straddle it
CONFIGS = [(D, step) for D in R.DS for step in R.STEPS]
FILL = 7.25


_off = R.offsets           # 0, 5 and W - 1 frames


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("limiter_ref_gpu"))


_CACHE = {}


def _case(ref, D, step):
    """per (D, step), computed once and not changed by any test: what the calls under test take (x1 [3, N1, 2]), what each station took
    before (pre [3, max(5, D), 2]), and the restatement's output, smallest gain and records after x1 in one piece"""
    if (D, step) not in _CACHE:
        off, n1 = _off(D), R.stream_length(D + 1, TILE)
        streams = R.gpu_streams(D, TILE)
        x1 = np.stack([streams[c][off[c]:] for c in range(3)])
        pre = np.zeros((3, max(5, D), 2), np.float32)
        for c in range(3):
            pre[c, :off[c]] = streams[c][:off[c]]
        chans = _ref_start(ref, D, step, pre)
        got = [chans[c].process(x1[c]) for c in range(3)]
        _CACHE[(D, step)] = dict(x1=x1, pre=pre, y=np.stack([g[0] for g in got]), gr=np.float32([g[1] for g in got]), status=[ch.status()[0] for ch in chans], n1=n1)
    return _CACHE[(D, step)]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _limiter(pkg, C, D, step, **kw):
    lim = pkg.Limiter(C, R.FS, R.LOOKAHEAD_MS[D], R.RELEASE_MS[step], R.CEILING_DB, **kw)
    assert lim.latency == D and lim.design.step == step
    return lim


def _start(pkg, D, step, pre, **kw):
    """a limiter of three stations at their gains whose station c has taken its OFF[c] frames"""
    import torch
    lim = _limiter(pkg, 3, D, step, **kw)
    for c in range(3):
        lim.set_gain(R.GAINS[c], c)
    pd = _cuda(pre)
    for c in (1, 2):
        if _off(D)[c]:
            active = torch.zeros(3, dtype=torch.uint8, device="cuda")
            active[c] = 1
            lim.process(pd, n=_off(D)[c], active=active)
    return lim


def _ref_start(ref, D, step, pre):
    chans = [ref.channel(D, step, R.ceiling(), R.GAINS[c]) for c in range(3)]
    for c in range(3):
        chans[c].process(pre[c, :_off(D)[c]])
    return chans


def _filled(shape, dtype=None):
    import torch
    dtype = dtype or torch.float32
    return torch.full(shape, FILL if dtype == torch.float32 else -0x55555556, dtype=dtype, device="cuda")


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError((what, "first difference at", bad[0].tolist(), "of", len(bad), got[tuple(bad[0])], want[tuple(bad[0])]))


def _same_status(got, chans, what=""):
    for c, ch in enumerate(chans):
        want = ch.status()[0] if hasattr(ch, "status") else ch
        for f in R.STATUS_DTYPE.names:
            assert np.array_equal(bits(np.atleast_1d(got[c][f])), bits(np.atleast_1d(want[f]))), (what, c, f, got[c][f], want[f])


def _run_splits(pkg, ref, D, step, pieces, streams=None, check_status_below=0):
    """x1 in calls of `pieces` frames (the last takes the rest) into one pre-filled output, on alternating streams where given; every
    call's d_gr, and the records behind the pieces shorter than check_status_below, against the restatement taking the same pieces"""
    import torch
    k = _case(ref, D, step)
    n1 = k["n1"]
    lim = _start(pkg, D, step, k["pre"])
    chans = _ref_start(ref, D, step, k["pre"])
    xd = _cuda(k["x1"])
    out = _filled((3, n1 + 3, 2))
    at = 0
    for i, piece in enumerate(list(pieces) + [n1]):
        take = min(piece, n1 - at)
        s = streams[i % len(streams)] if streams else None
        gr = _filled((3,))
        torch.cuda.synchronize()                                             # (the pre-filled tensors are there before another stream writes them)
        if take:
            lim.process(xd[:, at:at + take], out=out[:, at:at + take], gr=gr, stream=s)
        else:                                                                # (an empty view has no address)
            lim.process(xd, n=0, out=out, gr=gr, stream=s)
        want = np.float32([chans[c].process(k["x1"][c, at:at + take])[1] for c in range(3)])
        if s is not None:
            s.synchronize()
        _same(gr.cpu().numpy(), want, ("gr", i, at, take))
        if take < check_status_below:
            _same_status(lim.status(), chans, ("status", i, at, take))
        at += take
    assert at == n1
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    _same(o[:, :n1], k["y"], "output")
    assert (o[:, n1:] == FILL).all()
    _same_status(lim.status(), k["status"], "records")
    return lim, chans


@pytest.mark.parametrize("D,step", CONFIGS)
def test_one_call(pkg, ref, D, step):
    lim, _ = _run_splits(pkg, ref, D, step, [])
    st = lim.status()
    assert (st["limited"] > 0).all() and (st["nonfinite"] >= 4).all() and [float(g) for g in st["gain"]] == [float(np.float32(g)) for g in R.GAINS]


@pytest.mark.parametrize("D,step", CONFIGS)
def test_a_call_per_frame(pkg, ref, D, step):
    """a call per frame for the first 2W frames, the rest in one"""
    _run_splits(pkg, ref, D, step, [1] * (2 * (D + 1)))


@pytest.mark.parametrize("D,step", CONFIGS)
def test_ragged_splits_on_alternating_streams(pkg, ref, D, step):
    """pieces that straddle the tile's edges, calls alternating between two streams, the records read behind the short pieces"""
    import torch
    W = D + 1
    pieces = [3, TILE - 1, 2, TILE + W, 5, D, 1, TILE - 7 - W, 9, TILE + 1]
    _run_splits(pkg, ref, D, step, pieces, streams=[torch.cuda.Stream(), torch.cuda.Stream()], check_status_below=10)


@pytest.mark.parametrize("D", (1, 47, 255))
def test_call_lengths_around_the_look_ahead(pkg, ref, D):
    """n = 0, 1, D - 1, D, D + 1"""
    _run_splits(pkg, ref, D, 6711, [0, 1, D - 1, D, D + 1, 0, 2 * D + 3], check_status_below=3 * D + 5)


def test_n_zero(pkg, ref):
    """n = 0 writes 1.0f to d_gr and nothing else, with and without d_gr"""
    import torch
    D, step = 47, 6711
    k = _case(ref, D, step)
    lim = _start(pkg, D, step, k["pre"])
    xd = _cuda(k["x1"])
    lim.process(xd, n=300)
    before = lim.status()
    out, gr = _filled((3, 8, 2)), _filled((3,))
    lim.process(xd, n=0, out=out, gr=gr)
    lim.process(xd, n=0, out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all() and gr.cpu().numpy().tolist() == [1.0, 1.0, 1.0]
    assert lim.status().tobytes() == before.tobytes()
    y = lim.process(xd[:, 300:], n=k["n1"] - 300)
    _same(y.cpu().numpy(), k["y"][:, 300:], "behind n = 0")


def test_batch_and_row_invariance(pkg, ref):
    """station 1's stream alone, and as row 0 and row 2 of a batch of 70"""
    D, step = 47, 6711
    k = _case(ref, D, step)
    off, n1 = _off(D)[1], k["n1"]
    one = _limiter(pkg, 1, D, step)
    one.set_gain(R.GAINS[1])
    one.process(_cuda(k["pre"][1:2]), n=off)
    y, gr = one.process(_cuda(k["x1"][1:2]), gr=True)
    _same(y.cpu().numpy()[0], k["y"][1], "alone")
    _same(gr.cpu().numpy(), k["gr"][1:2], "alone, gr")
    _same_status(one.status(), [k["status"][1]], "alone")
    rng = np.random.default_rng(5)
    x = (0.6 * rng.standard_normal((70, n1, 2))).astype(np.float32)
    pre = (0.6 * rng.standard_normal((70, off, 2))).astype(np.float32)
    x[0] = x[2] = k["x1"][1]
    pre[0] = pre[2] = k["pre"][1, :off]
    many = _limiter(pkg, 70, D, step)
    many.set_gain(1.3)
    many.set_gain(R.GAINS[1], 0)
    many.set_gain(R.GAINS[1], 2)
    many.process(_cuda(pre))
    y, gr = many.process(_cuda(x), gr=True)
    y, st = y.cpu().numpy(), many.status()
    for row in (0, 2):
        _same(y[row], k["y"][1], f"row {row} of 70")
        _same_status([st[row]], [k["status"][1]], f"row {row} of 70")
    assert bits(gr.cpu().numpy()[[0, 2]]).tolist() == bits(k["gr"][[1, 1]]).tolist()
    ch = ref.channel(D, step, R.ceiling(), 1.3)
    ch.process(pre[69])
    _same(y[69], ch.process(x[69])[0], "row 69 of 70")


def test_active_masks_and_null_gr(pkg, ref):
    """a skipped station keeps its state, its row of the pre-filled output and its d_gr; the frames behind n are left as they were"""
    import torch
    D, step = 47, 6711
    k = _case(ref, D, step)
    lim = _start(pkg, D, step, k["pre"])
    chans = _ref_start(ref, D, step, k["pre"])
    xd = _cuda(k["x1"])
    at = [0, 0, 0]
    for i, (mask, n) in enumerate((([1, 0, 1], 700), ([0, 0, 0], 300), ([0, 1, 1], TILE + 9), ([1, 1, 0], 2))):
        active = torch.tensor(mask, dtype=torch.uint8, device="cuda")
        x = np.stack([k["x1"][c, at[c]:at[c] + n] for c in range(3)])
        out, gr = _filled((3, n + 5, 2)), _filled((3,))
        lim.process(_cuda(x), active=active.bool() if i % 2 else active, out=out, gr=gr)
        lim.process(xd, n=0, active=active)                                  # (and d_gr NULL)
        o, g = out.cpu().numpy(), gr.cpu().numpy()
        for c in range(3):
            if mask[c]:
                y, want = chans[c].process(x[c])
                _same(o[c, :n], y, (i, c))
                assert (o[c, n:] == FILL).all() and bits(g[c]).tolist() == bits(want).tolist()
                at[c] += n
            else:
                assert (o[c] == FILL).all() and g[c] == FILL, (i, c)
        _same_status(lim.status(), chans, i)


def test_odd_strides_and_views(pkg, ref):
    """rows aligned to a frame only (odd strides, views that start one frame in), input and output"""
    D, step = 47, 6711
    k = _case(ref, D, step)
    n1 = k["n1"]
    lim = _start(pkg, D, step, k["pre"])
    wide = _filled((3, n1 + 4, 2))
    wide[:, 1:n1 + 1] = _cuda(k["x1"])
    out = _filled((3, n1 + 2, 2))
    assert (wide.stride(0) // 2) % 2 == 1 and (out.stride(0) // 2) % 2 == 1 and wide[:, 1:].data_ptr() % 16 == 8
    lim.process(wide[:, 1:], n=n1, out=out[:, 1:])
    o = out.cpu().numpy()
    _same(o[:, 1:n1 + 1], k["y"], "odd strides")
    assert (o[:, 0] == FILL).all() and (o[:, n1 + 1:] == FILL).all()
    _same_status(lim.status(), k["status"])


def test_set_gain_between_calls(pkg, ref):
    D, step = 47, 6711
    k = _case(ref, D, step)
    lim = _start(pkg, D, step, k["pre"])
    chans = _ref_start(ref, D, step, k["pre"])
    xd = _cuda(k["x1"])
    at = 0
    for n, gains in ((500, None), (TILE, (2.0, 0.0, 0.25)), (700, (1.0, 9.5, 1.7))):
        if gains:
            for c in range(3):
                lim.set_gain(gains[c], c)
                chans[c].set_gain(gains[c])
                assert lim.get_gain(c) == float(np.float32(gains[c]))
        y = lim.process(xd[:, at:at + n]).cpu().numpy()
        for c in range(3):
            _same(y[c], chans[c].process(k["x1"][c, at:at + n])[0], (at, c))
        at += n
    _same_status(lim.status(), chans)
    lim.set_gain(0.75)
    assert [lim.get_gain(c) for c in range(3)] == [0.75] * 3 and [float(g) for g in lim.status()["gain"]] == [0.75] * 3


@pytest.mark.parametrize("D,step", [(0, 6711), (1, 1), (47, 6711), (255, ONE)])
def test_resets_and_flushes(pkg, ref, D, step):
    """reset and flush mid-stream, of one station and of all, flush right after reset, and flush twice"""
    import torch
    k = _case(ref, D, step)
    lim = _start(pkg, D, step, k["pre"])
    chans = _ref_start(ref, D, step, k["pre"])
    xd = _cuda(k["x1"])
    e0 = 5 * (D + 1) + 60                                                    # inside the bursts: the release is under way

    def flush(channel, what):
        out, nout = _filled((3, D + 2, 2)), _filled((3,), torch.int32)
        lim.flush(channel, out=out, nout=nout)
        o, nn = out.cpu().numpy(), nout.cpu().numpy()
        for c in range(3):
            if channel in (-1, c):
                _same(o[c, :D], chans[c].flush(), (what, c))
                assert (o[c, D:] == FILL).all() and int(nn[c]) == D
            else:
                assert (o[c] == FILL).all() and int(nn[c]) == -0x55555556
        _same_status(lim.status(), chans, what)

    def take(a, b, what):
        y = lim.process(xd[:, a:b]).cpu().numpy()
        for c in range(3):
            _same(y[c], chans[c].process(k["x1"][c, a:b])[0], (what, c))
        _same_status(lim.status(), chans, what)

    take(0, e0, "start")
    assert (lim.status()["eq"] < ONE).all() or step == ONE
    flush(1, "flush of one")
    take(e0, e0 + 300, "behind the flush of one")
    lim.reset(2)
    chans[2].reset()
    _same_status(lim.status(), chans, "reset of one")
    take(e0 + 300, e0 + 600, "behind the reset of one")
    flush(-1, "flush of all")
    flush(-1, "flush twice")
    take(0, e0, "behind the flushes")
    lim.reset()
    for ch in chans:
        ch.reset()
    flush(-1, "flush right after reset")
    st = lim.status()
    assert not st["frames"].any() and (st["eq"] == ONE).all() and (st["min_gain"] == 1.0).all() and [float(g) for g in st["gain"]] == [float(np.float32(g)) for g in R.GAINS]
    take(0, k["n1"], "behind the reset")
    lim.flush(out=None, nout=False)


def test_frame_count_above_2_32(pkg, ref):
    """a station that has been running for 37 hours: its frame count starts above 2^32 (the debug setter) and goes on in 64 bits"""
    D, step = 47, 6711
    k = _case(ref, D, step)
    lim = _start(pkg, D, step, k["pre"])
    chans = _ref_start(ref, D, step, k["pre"])
    start = (1 << 32) + (1 << 31) - 7
    lim.debug_set_frames(1, start)
    chans[1].set_frames(start)
    y = lim.process(_cuda(k["x1"]), n=TILE + 300).cpu().numpy()
    for c in range(3):
        _same(y[c], chans[c].process(k["x1"][c, :TILE + 300])[0], c)
    st = lim.status()
    _same_status(st, chans, "past 2^32")
    assert int(st[1]["frames"]) == start + TILE + 300 > 1 << 32 and int(st[0]["frames"]) == TILE + 300
    with pytest.raises(pkg.FmdError):
        lim.debug_set_frames(3, 0)


def test_device_records_and_argument_errors(pkg, ref):
    import torch
    D, step = 47, 6711
    k = _case(ref, D, step)
    n1 = k["n1"]
    lim = _start(pkg, D, step, k["pre"], max_input_frames=n1)
    xd = _cuda(k["x1"])
    big = _filled((3, n1 + 8, 2))
    lim.process(xd, out=big)
    torch.cuda.synchronize()
    ptr = lim.status_dev_ptr()

    class _Arr:
        __cuda_array_interface__ = {"shape": (3 * 8,), "typestr": "<i8", "data": (ptr, False), "version": 2}
    raw = torch.as_tensor(_Arr(), device="cuda").clone().cpu().numpy()
    assert np.array_equal(bits(raw), bits(lim.status())) and lim.status().tobytes() == b"".join(r.tobytes() for r in k["status"])
    before, kept = lim.status().tobytes(), big.clone()
    f = lim.L.fmd_limiter_process_f32_dev
    stride = n1 + 8
    both = torch.zeros((6 * n1, 2), device="cuda")                           # input rows at frames 0, n1, 2 n1; room for output rows behind them
    at = lambda frame: both.data_ptr() + 8 * frame
    bad = [lambda: lim.process(xd, n=n1 + 1, out=big),                       # n > in_stride and > max_input_frames
           lambda: lim.process(xd, n=-1, out=big),
           lambda: lim._check(f(lim.l, xd.data_ptr(), n1, 16, None, big.data_ptr(), 15, None, None)),                          # n > out_stride
           lambda: lim._check(f(lim.l, xd.data_ptr() + 4, n1, 16, None, big.data_ptr(), stride, None, None)),                  # not aligned to a frame
           lambda: lim._check(f(lim.l, xd.data_ptr(), n1, 16, None, big.data_ptr() + 4, stride, None, None)),
           lambda: lim._check(f(lim.l, None, n1, 16, None, big.data_ptr(), stride, None, None)),
           lambda: lim._check(f(lim.l, xd.data_ptr(), n1, 16, None, None, stride, None, None)),
           lambda: lim._check(f(lim.l, at(0), n1, 16, None, at(0), n1, None, None)),                                           # in place
           lambda: lim._check(f(lim.l, at(0), n1, 16, None, at(2 * n1 + 15), n1, None, None)),                                 # from the input's last frame on
           lambda: lim._check(f(lim.l, at(2 * n1 + 15), n1, 16, None, at(0), n1, None, None)),                                 # up to the input's first frame
           lambda: lim.reset(3), lambda: lim.reset(-2), lambda: lim.flush(3, out=big), lambda: lim.flush(-2, out=big),
           lambda: lim.set_gain(-0.5), lambda: lim.set_gain(float("inf")), lambda: lim.set_gain(float("nan")), lambda: lim.set_gain(1.0, 3),
           lambda: lim.get_gain(3), lambda: lim.get_gain(-1),
           lambda: lim._check(lim.L.fmd_limiter_flush(lim.l, -1, big.data_ptr(), D - 1, None, None)),
           lambda: lim._check(lim.L.fmd_limiter_flush(lim.l, -1, big.data_ptr() + 4, stride, None, None)),
           lambda: lim._check(lim.L.fmd_limiter_flush(lim.l, -1, None, stride, None, None))]
    for i, g in enumerate(bad):
        with pytest.raises(pkg.FmdError) as err:
            g()
        assert err.value.status == -1, i                                     # FMD_ERR_ARG
    torch.cuda.synchronize()
    assert lim.status().tobytes() == before and torch.equal(big, kept)       # and nothing changed
    # the other side of the same bounds
    lim._check(f(lim.l, at(0), n1, 16, None, at(2 * n1 + 16), n1, None, None))                             # the first frame behind the input's last
    lim._check(f(lim.l, at(2 * n1 + 16), n1, 16, None, at(0), n1, None, None))
    lim._check(f(lim.l, xd.data_ptr(), n1, 16, None, big.data_ptr(), 16, None, None))
    lim._check(lim.L.fmd_limiter_flush(lim.l, -1, big.data_ptr(), D, None, None))
    lim.set_gain(0.0)
    small = _limiter(pkg, 3, D, step, max_input_frames=256)
    small.process(xd, n=256)
    with pytest.raises(pkg.FmdError) as err:
        small.process(xd, n=257)
    assert err.value.status == -1 and int(small.status()[0]["frames"]) == 256
    for g in (lambda: lim.process(xd[:2], out=big), lambda: lim.process(xd, active=torch.ones(2, dtype=torch.uint8, device="cuda"), out=big),
              lambda: lim.process(xd.double(), out=big), lambda: lim.process(xd[:, :, :1], out=big), lambda: lim.process(xd, out=big[:2]),
              lambda: lim.process(xd, out=big[:, :100]), lambda: lim.process(xd, out=big.double()), lambda: lim.flush(out=big[:, :D - 1]),
              lambda: lim.process(xd, out=big, gr=torch.zeros(3, dtype=torch.float64, device="cuda")),
              lambda: lim.flush(out=big, nout=torch.zeros(3, dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            g()
    with pytest.raises(AttributeError):
        lim.reset_peaks()
    for kw in (dict(C=0), dict(lookahead_ms=8.0), dict(release_ms=-1.0), dict(ceiling_db=0.5), dict(ceiling_db=-41.0), dict(fs=7999), dict(fs=192001),
               dict(max_input_frames=0), dict(max_input_frames=(1 << 30) + 1)):
        args = dict(C=3, fs=32000, lookahead_ms=1.5, release_ms=500.0, ceiling_db=-1.0, max_input_frames=64)
        args.update(kw)
        with pytest.raises(pkg.FmdError) as err:
            pkg.Limiter(args.pop("C"), **args)
        assert err.value.status == -1, kw
    for fs in (8000, 192000):
        edge = pkg.Limiter(1, fs, lookahead_ms=1.0, max_input_frames=1 << 30)
        assert edge.latency == fs // 1000 and edge.get_gain(0) == 1.0
        edge.close()


def test_cpp_adaptor(pkg, ref, tmp_path):
    """tests/cpp/limiter_main.cpp runs a file of audio in calls of 100 frames through host/audio_limiter_gpu.hpp at the default time
    constants, station c at gain 0.5 + c, and flushes: outputs and records are the restatement's"""
    exe = tmp_path / "limiter_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'fm-radio_amd' / 'host'}", "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "limiter_main.cpp"),
                    f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)],
                   check=True)
    n = 1000
    a = np.ascontiguousarray(_case(ref, 47, 6711)["x1"][:2, :n])
    a.tofile(tmp_path / "audio.f32")
    out = subprocess.run([str(exe), str(tmp_path / "audio.f32"), "2", "32000", "1.5", "500", "100", str(tmp_path / "y.f32")], check=True, capture_output=True,
                         text=True).stdout
    lines = out.strip().split("\n")
    d = pkg.limiter_design(32000, 1.5, 500.0, -1.0)
    D = d.lookahead_frames
    y = np.fromfile(tmp_path / "y.f32", np.float32).reshape(2, n + D, 2)
    assert len(lines) == 2 and D == 48
    for c in range(2):
        ch = ref.channel(D, d.step, d.ceiling, 0.5 + c)
        want = np.concatenate([ch.process(a[c])[0], ch.flush()])
        _same(y[c], want, c)
        assert bytes.fromhex(lines[c]) == ch.status()[0].tobytes(), c


def test_demodulator_to_flac_end_to_end(pkg, ref, tmp_path_factory):
    """Three stations at 256 kSa/s through BatchDemod in the tolerance mode, four blocks of 16384 samples (2048 frames of audio at 32 kHz
    each), the default limiter at gain 8 on audio_tensor() after each block and the default FLAC encoder on the limiter's output: every
    call's output and records are the restatement's over the demodulator's own device audio copied to the host, and the FLAC stream,
    flushed, decodes on the host to the restatement's output as 16-bit PCM"""
    import torch
    fs, bs, nb_ = 256_000, 16384, 4
    tone = synth.to_cf32(synth.fm_capture(bs * nb_, fs=float(fs), seed=43, channel=0)["iq"])
    prog = synth.to_cf32(synth.fm_capture_realistic(bs * nb_, fs=float(fs), seed=41)["iq"])
    x = torch.from_numpy(np.stack([tone, prog, np.zeros_like(tone)])).cuda()
    dm = pkg.BatchDemod(3, bs, fs, fast_math=True)
    n = bs // 8
    lim = pkg.Limiter(3, 32000, max_input_frames=n)
    enc = pkg.FlacEncoder(3, max_input_frames=n)
    d = lim.design
    gain = 8.0
    lim.set_gain(gain)
    chans = [ref.channel(d.lookahead_frames, d.step, d.ceiling, gain) for _ in range(3)]
    got, want = [[] for _ in range(3)], [[] for _ in range(3)]

    def encode(y, frames):
        out, nby, _ = enc.process(y, n=frames)
        for c in range(3):
            got[c].append(out[c, :int(nby[c])].cpu().numpy())

    for b in range(nb_):
        dm.process(x[:, b * bs:(b + 1) * bs].contiguous())
        dm.synchronize()
        a = dm.audio_tensor()
        assert tuple(a.shape) == (3, n, 2)
        y = lim.process(a)
        encode(y, n)
        ah, yh = a.cpu().numpy(), y.cpu().numpy()
        for c in range(3):
            want[c].append(chans[c].process(ah[c])[0])
            _same(yh[c], want[c][-1], (b, c))
        _same_status(lim.status(), chans, f"block {b}")
    tail, nout = lim.flush()
    assert nout.cpu().numpy().tolist() == [lim.latency] * 3 == [48] * 3
    encode(tail, lim.latency)
    out, nby, _ = enc.flush()
    th = tail.cpu().numpy()
    for c in range(3):
        got[c].append(out[c, :int(nby[c])].cpu().numpy())
        want[c].append(chans[c].flush())
        _same(th[c, :lim.latency], want[c][-1], ("flush", c))
    st = lim.status()
    assert (st["frames"] == nb_ * n).all() and st["limited"][0] > 0 and st["limited"][2] == 0 and not st["nonfinite"].any()
    for c in range(3):
        w = np.concatenate(want[c])
        assert w.shape[0] == nb_ * n + lim.latency and float(np.abs(w).max()) <= float(d.ceiling)
        pcm = np.clip((w * adpcm_ref.SCALE).astype(np.float32).astype(np.int32), -32768, 32767).astype(np.int16)
        dec = pkg.flac_decode(np.concatenate(got[c]), 32000)
        assert dec.shape == pcm.shape and np.array_equal(dec, pcm), c
        print(f"station {c}: limited {int(st['limited'][c])} of {nb_ * n + lim.latency} output frames, smallest gain {float(st['min_gain'][c]):.4f}, clamped {st['clamped'][c].tolist()}")
    dm.close(); lim.close(); enc.close()


def test_mixer_bus_end_to_end(pkg, ref):
    """Eight stations at 256 kSa/s through BatchDemod and AudioMixer into four buses, the default limiter on the buses, three blocks on
    one stream: the limiter's output is the restatement's over the mixer's own device output read back.  The bus that sums every station
    five times stands in the mixer's clamp at +-1, 1 dB over the ceiling: the limiter is at work"""
    import torch
    C, bs, nb = 8, 16384, 3
    caps = np.stack([synth.to_cf32(synth.fm_capture(bs * nb, fs=256000.0, seed=60 + c, channel=c + 1)["iq"]) for c in range(C)])
    buses = [list(range(C)), [0], [2, 5, 2], list(range(C)) * 5]
    s = torch.cuda.Stream()
    dm = pkg.BatchDemod(C, bs, 256_000, fast_math=True)
    mx = pkg.AudioMixer(C, buses, gains=np.float32([1.0, 2.5, 0.8, 1.2]))
    lim = pkg.Limiter(len(buses), 32000, max_input_frames=bs // 8)
    d = lim.design
    chans = [ref.channel(d.lookahead_frames, d.step, d.ceiling) for _ in buses]
    d_in = [_cuda(caps[:, b * bs:(b + 1) * bs]) for b in range(nb)]
    mixed, limited = [], []
    torch.cuda.synchronize()
    for b in range(nb):
        dm.submit(d_in[b])
        dm.wait_outputs(s)
        with torch.cuda.stream(s):
            z = mx.process(dm.audio_tensor(), stream=s)
            y = lim.process(z, stream=s)
            mixed.append(z.clone())
            limited.append(y.clone())
        dm.release_outputs(s)
    torch.cuda.synchronize()
    dm.close()
    mixed, limited = torch.cat(mixed, 1).cpu().numpy(), torch.cat(limited, 1).cpu().numpy()
    for c in range(len(buses)):
        _same(limited[c], chans[c].process(mixed[c])[0], c)
    st = lim.status()
    _same_status(st, chans)
    assert float(np.abs(limited).max()) <= float(d.ceiling) and int(st["limited"][3]) > 0
