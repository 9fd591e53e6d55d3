"""Log-mel front end on the GPU (fmd_logmel_*, LogMel): rows, counts and status records against the C restatement of the arithmetic
contract (tests/cpp/logmel_ref.c, itself checked in test_logmel_cpu.py), bit for bit, compared as integer views of the floats: one call, a
call per hop, ragged calls on alternating streams, other hops, windows, scales and modes, the default geometry at 32 kHz, n = 0, batch and
row invariance, the `active` mask over pre-filled outputs, NULL counts, the smallest out_stride, odd strides and views, inf / NaN /
denormal / 1e30 samples, resets, the device's records, argument errors, the C++ adaptor, and demodulator -> LogMel end to end.

The main shape is fs = 8000, win = 64, hop = 16, 8 bands, K = 33 bins (no multiple of 16: the bin padding is live) with three stations.
Station c has its own amplitude and its own order of noise, tone, tone over faint noise and silence, and has taken OFF[c] frames of its own
before the calls under test; one call of 64 + 16 * 40 frames then completes 41 spectral frames or more, across the 16- and 32-row edges."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import logmel_ref
from logmel_ref import bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FS = 8000
MAIN = dict(fs=FS, win=64, hop=16, n_mels=8)
N1 = 64 + 16 * 40
SCALE = (1.0, 0.37, 2.5)
OFF = (0, 5, 37)             # frames each station has taken before (no multiples of hop or 4)
ORDER = (("noise", "tone", "tone_noise", "silence"), ("tone", "silence", "noise", "tone_noise"), ("silence", "tone_noise", "tone", "noise"))


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return logmel_ref.build(tmp_path_factory.mktemp("logmel_ref_gpu"))


@pytest.fixture(scope="module")
def streams():
    """per station [OFF[c] + N1, 2] float32"""
    return [logmel_ref.mixed_signal(FS, OFF[c] + N1, ORDER[c], 100 + 10 * c, SCALE[c]) for c in range(3)]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _split(streams, off=OFF):
    """(pre [3, max(off), 2], x1 [3, n, 2]): what each station took before, and what the calls under test take"""
    n = min(s.shape[0] - o for s, o in zip(streams, off))
    pre = np.zeros((len(streams), max(max(off), 1), 2), np.float32)
    for c, s in enumerate(streams):
        pre[c, :off[c]] = s[:off[c]]
    return pre, np.stack([s[o:o + n] for s, o in zip(streams, off)])


def _want(ref, g, streams, off=OFF):
    """the restatement's stations: (rows per station of the calls under test, records [C], the channels)"""
    cfg = logmel_ref.config(**g)
    chans, rows = [], []
    for s, o in zip(streams, off):
        ch = ref.channel(cfg)
        ch.process(s[:o])
        rows.append(ch.process(s[o:]))
        chans.append(ch)
    return rows, np.concatenate([ch.status() for ch in chans]), chans


def _start(pkg, g, pre, off=OFF, **kw):
    """a LogMel whose station c has taken its off[c] frames"""
    import torch
    f = {k: v for k, v in g.items() if k != "fs"}
    m = pkg.LogMel(len(off), g["fs"], **f, **kw)
    pd = _cuda(pre)
    for c, o in enumerate(off):
        if o:
            active = torch.zeros(len(off), dtype=torch.uint8, device="cuda")
            active[c] = 1
            m.process(pd, n=o, active=active, nframes=False)
    return m


def _take(m, xd, cuts):
    """feeds xd [C, n, 2] in the pieces that end at `cuts` and at n; per station the rows of all pieces"""
    C, n = xd.shape[0], xd.shape[1]
    got, at = [[] for _ in range(C)], 0
    for c in list(cuts) + [n]:
        out, cnt = m.process(xd[:, at:c])
        o, k = out.cpu().numpy(), cnt.cpu().numpy()
        for s in range(C):
            got[s].append(o[s, :k[s]])
        at = c
    return [np.concatenate(r) for r in got]


def _same(got_rows, got_st, want_rows, want_st, what=""):
    for c, (g, w) in enumerate(zip(got_rows, want_rows)):
        assert g.shape == w.shape, (what, c, g.shape, w.shape)
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, (what, c, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    assert got_st.tobytes() == want_st.tobytes(), (what, got_st, want_st)


@pytest.fixture(scope="module")
def want_main(ref, streams):
    return _want(ref, MAIN, streams)[:2]


def test_main_shape_one_call(pkg, streams, want_main):
    pre, x1 = _split(streams)
    m = _start(pkg, MAIN, pre)
    rows = _take(m, _cuda(x1), ())
    assert [r.shape[0] for r in rows] == [41, 41, 43]
    _same(rows, m.status(), *want_main)
    assert (m.status()["nonfinite"] == 0).all() and all(np.isfinite(r).all() for r in rows)
    m.close()


def test_call_per_hop_and_ragged_calls_on_alternating_streams(pkg, ref, streams, want_main):
    import torch
    pre, x1 = _split(streams)
    xd = _cuda(x1)
    m = _start(pkg, MAIN, pre)
    _same(_take(m, xd, range(16, N1, 16)), m.status(), *want_main, "a call per hop")
    m.close()
    # 1 + 7 + 15 + 16 + 17 + 63 + 64 + 65 + rest, the records behind every piece
    cuts = list(np.cumsum([1, 7, 15, 16, 17, 63, 64, 65]))
    m = _start(pkg, MAIN, pre)
    ss = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    cfg = logmel_ref.config(**MAIN)
    chans = [ref.channel(cfg) for _ in range(3)]
    for c in range(3):
        chans[c].process(streams[c][:OFF[c]])
    got, at = [[] for _ in range(3)], 0
    for i, c in enumerate(cuts + [N1]):
        out, cnt = m.process(xd[:, at:c], stream=ss[i % 2])
        st = m.status()
        o, k = out.cpu().numpy(), cnt.cpu().numpy()
        for s in range(3):
            w = chans[s].process(x1[s, at:c])
            assert k[s] == w.shape[0] and np.array_equal(bits(o[s, :k[s]]), bits(w)), (i, s)
            assert st[s:s + 1].tobytes() == chans[s].status().tobytes(), (i, s)
            got[s].append(o[s, :k[s]])
        at = c
    _same([np.concatenate(r) for r in got], m.status(), *want_main, "ragged")
    m.close()


@pytest.mark.parametrize("g", [dict(MAIN, hop=24), dict(MAIN, hop=64), dict(MAIN, win=80), dict(MAIN, hop=24, mel_scale=1, f_min_hz=100.0, f_max_hz=3000.0),
                               dict(MAIN, out_mode=0), dict(MAIN, out_mode=1, log_floor=1e-6)],
                         ids=["hop24", "hop64", "win80", "htk", "mode0", "mode1"])
def test_further_main_shape_cases(pkg, ref, streams, g):
    pre, x1 = _split(streams)
    want = _want(ref, g, streams)[:2]
    m = _start(pkg, g, pre)
    _same(_take(m, _cuda(x1), (100, 333)), m.status(), *want)
    m.close()


@pytest.fixture(scope="module")
def streams32():
    return [logmel_ref.mixed_signal(32000, 2048 + 800, ORDER[c], 200 + c, SCALE[c]) for c in range(2)]


def test_default_geometry_at_32k(pkg, ref, streams32):
    """800 / 320 / 80 bands, 201 bins: two stations x 2848 frames in one call, and as 2048 + 800"""
    g = logmel_ref.GEOMETRIES["32k"]
    off = (0, 0)
    pre, x = _split(streams32, off)
    want = _want(ref, g, streams32, off)[:2]
    assert want[0][0].shape == (7, 80)
    for cuts in ((), (2048,)):
        m = _start(pkg, g, pre, off)
        assert (m.win, m.hop, m.n_mels, m.n_bins) == (800, 320, 80, 201)
        _same(_take(m, _cuda(x), cuts), m.status(), *want, f"cuts {cuts}")
        m.close()


def test_n_zero_row_69_of_70_and_a_batch_of_one(pkg, ref, streams, want_main):
    import torch
    pre, x1 = _split(streams)
    # n = 0: counts 0, nothing else changes
    m = _start(pkg, MAIN, pre)
    before = m.status()
    out, cnt = m.process(_cuda(x1), n=0)
    assert cnt.cpu().numpy().tolist() == [0, 0, 0] and m.status().tobytes() == before.tobytes() and tuple(out.shape) == (3, 1, 8)
    _same(_take(m, _cuda(x1), ()), m.status(), *want_main, "behind n = 0")
    m.close()
    # row 69 of 70 and a batch of one are station 2's stream from the start
    s = streams[2]
    w = _want(ref, MAIN, [s], (0,))
    big = np.zeros((70, s.shape[0], 2), np.float32)
    big[69] = s
    big[:69] = streams[0][:1]
    m = pkg.LogMel(70, FS, **{k: v for k, v in MAIN.items() if k != "fs"})
    out, cnt = m.process(_cuda(big))
    k = int(cnt[69])
    assert np.array_equal(bits(out[69, :k].cpu().numpy()), bits(w[0][0])) and m.status()[69:70].tobytes() == w[1].tobytes()
    m.close()
    m = pkg.LogMel(1, FS, **{k: v for k, v in MAIN.items() if k != "fs"})
    pad = torch.zeros((1, s.shape[0] + 3, 2), device="cuda")
    pad[0, :s.shape[0]] = _cuda(s)
    out, cnt = m.process(pad, n=s.shape[0])
    assert np.array_equal(bits(out[0, :int(cnt[0])].cpu().numpy()), bits(w[0][0])) and m.status().tobytes() == w[1].tobytes()
    m.close()


def test_active_mask_null_counts_and_out_stride(pkg, ref, streams, want_main):
    import torch
    pre, x1 = _split(streams)
    xd = _cuda(x1)
    rows_max = pkg.logmel_max_frames(16, N1)
    assert rows_max == 44
    # station 1 inactive over outputs pre-filled with a NaN pattern, two rows more than the call may write
    pat = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]
    out = torch.full((3, rows_max + 2, 8), float("nan"), device="cuda")
    out.view(torch.int32).fill_(0x7FC0BEEF)
    cnt = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    m = _start(pkg, MAIN, pre)
    before = m.status()
    m.process(xd, active=torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda"), out=out, nframes=cnt)
    o, k, st = out.cpu().numpy(), cnt.cpu().numpy(), m.status()
    assert k.tolist() == [41, -7, 43] and st[1:2].tobytes() == before[1:2].tobytes()
    for c in (0, 2):
        assert np.array_equal(bits(o[c, :k[c]]), bits(want_main[0][c])) and st[c:c + 1].tobytes() == want_main[1][c:c + 1].tobytes()
        assert (bits(o[c, k[c]:]) == bits(pat)).all()                # the floats behind the rows are left alone
    assert (bits(o[1]) == bits(pat)).all()
    # the skipped station then takes the same frames: as if it had never been skipped
    m.process(xd, active=torch.tensor([0, 1, 0], dtype=torch.uint8, device="cuda"), out=out, nframes=cnt)
    assert np.array_equal(bits(out[1, :41].cpu().numpy()), bits(want_main[0][1])) and m.status().tobytes() == want_main[1].tobytes()
    m.close()
    # NULL d_nframes, and out_stride at its minimum; one row short is refused and changes nothing
    m = _start(pkg, MAIN, pre)
    out = torch.zeros((3, rows_max, 8), device="cuda")
    o2, none = m.process(xd, out=out, nframes=False)
    assert none is None and o2 is out
    o = out.cpu().numpy()
    for c in range(3):
        assert np.array_equal(bits(o[c, :want_main[0][c].shape[0]]), bits(want_main[0][c]))
    st = m.status()
    with pytest.raises(pkg.FmdError) as e:
        m._check(m.L.fmd_logmel_process_f32_dev(m.g, xd.data_ptr(), N1, N1, None, out.data_ptr(), rows_max * 8 - 8, None, None))
    assert e.value.status == -1 and m.status().tobytes() == st.tobytes()
    with pytest.raises(ValueError):
        m.process(xd, out=torch.zeros((3, rows_max - 1, 8), device="cuda"))
    m.close()


def test_odd_stride_and_odd_view(pkg, ref, streams, want_main):
    """an in_stride that is odd, a view that starts at an odd frame, and NaN behind n: not read"""
    import torch
    pre, x1 = _split(streams)
    buf = torch.full((3, N1 + 9, 2), float("nan"), device="cuda")
    buf[:, 3:3 + N1] = _cuda(x1)
    m = _start(pkg, MAIN, pre)
    out, cnt = m.process(buf[:, 3:], n=N1)
    k = cnt.cpu().numpy()
    _same([out[c, :k[c]].cpu().numpy() for c in range(3)], m.status(), *want_main, "odd view")
    m.close()


def test_special_samples(pkg, ref, streams):
    """+-inf, NaN, denormal and 1e30 samples: the frames that hold a non-finite sample (or overflow) are non-finite as the chains give them,
    a NaN is written as 0x7fc00000, and the counters agree; denormal input is kept, not flushed"""
    s = [a.copy() for a in streams]
    s[0][100, 0] = np.inf
    s[0][400, 1] = -np.inf
    s[1][200, 1] = np.nan
    s[1][500:520] = 1e30
    s[2][:] = 0.0
    s[2][37:300, 0] = np.float32(3e-39) * np.sign(streams[2][37:300, 0] + 1e-30)
    s[2][37:300, 1] = np.float32(1e-40)
    s[2][400:500] = streams[2][400:500] * 1e-18
    for mode in (0, 1):
        g = dict(MAIN, out_mode=mode, log_floor=float(np.float32(1.2e-38)))
        pre, x1 = _split(s)
        want = _want(ref, g, s)
        m = _start(pkg, g, pre)
        rows = _take(m, _cuda(x1), (300,))
        _same(rows, m.status(), want[0], want[1], f"mode {mode}")
        assert want[1]["nonfinite"][0] > 0 and want[1]["nonfinite"][1] > 0 and want[1]["nonfinite"][2] == 0
        m.close()


def test_reset_mid_window_records_and_argument_errors(pkg, ref, streams, want_main):
    import torch
    pre, x1 = _split(streams)
    xd = _cuda(x1)
    m = _start(pkg, MAIN, pre, max_input_frames=N1)
    m.process(xd, n=77)
    m.reset(1)                                                    # station 1 alone starts over, mid-window
    st = m.status()
    assert st[1].tobytes() == np.zeros(1, logmel_ref.STATUS_DTYPE).tobytes() and st[0]["frames"] == 77 and st[2]["fill"] == (37 + 77) - 4 * 16
    out, cnt = m.process(xd[:, 77:])
    cfg = logmel_ref.config(**MAIN)
    ch = ref.channel(cfg)
    w = ch.process(x1[1, 77:])
    assert np.array_equal(bits(out[1, :int(cnt[1])].cpu().numpy()), bits(w)) and m.status()[1:2].tobytes() == ch.status().tobytes()
    assert m.status()[[0, 2]].tobytes() == want_main[1][[0, 2]].tobytes()
    m.reset()
    assert m.status().tobytes() == np.zeros(3, logmel_ref.STATUS_DTYPE).tobytes()
    _same(_take(m, xd, ()), m.status(), *_want(ref, MAIN, list(x1), (0, 0, 0))[:2], "behind reset(-1)")
    # the device's own records
    torch.cuda.synchronize()
    ptr = m.status_dev_ptr()

    class _Arr:
        __cuda_array_interface__ = {"shape": (3 * 32,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    raw = torch.as_tensor(_Arr(), device="cuda").clone()
    assert raw.cpu().numpy().tobytes() == m.status().tobytes()
    st = m.status()
    out = torch.zeros((3, 44, 8), device="cuda")
    bad = [lambda: m.process(xd, n=N1 + 1), lambda: m.process(xd, n=-1), lambda: m.reset(3), lambda: m.reset(-2),
           lambda: m._check(m.L.fmd_logmel_process_f32_dev(m.g, xd.data_ptr() + 4, N1, 16, None, out.data_ptr(), 44 * 8, None, None)),
           lambda: m._check(m.L.fmd_logmel_process_f32_dev(m.g, xd.data_ptr(), N1, 16, None, out.data_ptr() + 2, 44 * 8, None, None)),
           lambda: m._check(m.L.fmd_logmel_process_f32_dev(m.g, None, N1, 16, None, out.data_ptr(), 44 * 8, None, None)),
           lambda: m._check(m.L.fmd_logmel_process_f32_dev(m.g, xd.data_ptr(), N1, 16, None, None, 44 * 8, None, None))]
    for k, f in enumerate(bad):
        with pytest.raises(pkg.FmdError) as e:
            f()
        assert e.value.status == -1, k
    small = pkg.LogMel(3, FS, win=64, hop=16, n_mels=8, max_input_frames=128)
    with pytest.raises(pkg.FmdError) as e:
        small.process(xd, n=129)
    assert e.value.status == -1 and int(small.status()[0]["frames"]) == 0
    small.close()
    for f in (lambda: m.process(xd[:2]), lambda: m.process(xd, active=torch.ones(2, dtype=torch.uint8, device="cuda")), lambda: m.process(xd.double()),
              lambda: m.process(xd, nframes=torch.zeros(3, dtype=torch.int64, device="cuda")), lambda: m.process(xd, out=torch.zeros((3, 44, 9), device="cuda"))):
        with pytest.raises(ValueError):
            f()
    for kw in (dict(win=48), dict(win=72), dict(hop=15), dict(hop=65), dict(n_mels=0), dict(n_mels=129), dict(f_max_hz=4001.0), dict(f_min_hz=-1.0), dict(mel_scale=2),
               dict(out_mode=2), dict(log_floor=0.0), dict(max_input_frames=0), dict(max_input_frames=(1 << 30) + 1)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.LogMel(3, FS, **{**dict(win=64, hop=16, n_mels=8), **kw})
        assert e.value.status == -1, kw
    with pytest.raises(pkg.FmdError):
        pkg.LogMel(0, FS)
    # a design with empty bands is accepted, and the largest window works
    e = pkg.LogMel(1, FS, win=64, hop=16, n_mels=40)
    out, cnt = e.process(xd[:1])
    assert int(cnt[0]) == 41 and np.array_equal(bits(out[0, :41].cpu().numpy()), bits(ref.run(logmel_ref.config(**dict(MAIN, n_mels=40)), x1[0])))
    e.close()
    big = pkg.LogMel(1, FS, win=2048, hop=2048, n_mels=128, mel_scale=1, max_input_frames=1 << 30)
    xb = logmel_ref.signal("noise", FS, 2 * 2048 + 5)
    out, cnt = big.process(_cuda(xb[None]))
    assert int(cnt[0]) == 2 and np.array_equal(bits(out[0, :2].cpu().numpy()),
                                                bits(ref.run(logmel_ref.config(fs=FS, win=2048, hop=2048, n_mels=128, mel_scale=1), xb)))
    big.close()
    assert m.status().tobytes() == st.tobytes()
    m.close()


def test_cpp_adaptor(pkg, ref, streams, tmp_path):
    """tests/cpp/logmel_main.cpp takes a file of audio in calls of 100 frames through LogMel_GPU; the rows its host views give and the
    records it prints are the restatement's, and it exits with 7 unless the device's views and records are the host's"""
    exe = tmp_path / "logmel_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}", f"-I{ROOT / 'fm-radio_amd' / 'host'}",
                    "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "logmel_main.cpp"), f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64",
                    f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    a = np.ascontiguousarray(np.stack([streams[0][:N1], streams[1][:N1]]))
    a.tofile(tmp_path / "audio.f32")
    r = subprocess.run([str(exe), str(tmp_path / "audio.f32"), "2", str(FS), "64", "16", "8", "100", str(tmp_path / "rows")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2
    cfg = logmel_ref.config(**MAIN)
    for c, line in enumerate(lines):
        ch = ref.channel(cfg)
        w = ch.process(a[c])
        assert bytes.fromhex(line.split()[0]) == ch.status().tobytes(), c
        got = np.fromfile(tmp_path / f"rows.{c}.f32", np.float32).reshape(-1, 8)
        assert np.array_equal(bits(got), bits(w)), c
    assert float(lines[0].split()[1]) == (40 * 16 + 32) / FS


def test_demodulator_end_to_end(pkg, ref):
    """Three stations at 256 kSa/s through BatchDemod in the tolerance mode, ten blocks of 16384 samples (2048 frames of audio at 32 kHz
    each), LogMel at the default geometry on audio_tensor() after each block: bit for bit the restatement on the same audio copied to the
    host.  Station 0 is a carrier frequency-modulated with a 1 kHz tone alone (37.5 kHz deviation, no pilot: mono): its strongest band,
    summed over the run, is the one whose triangle weighs the 1 kHz bin most."""
    import synth
    import torch
    fs, bs, nb = 256_000, 16384, 10
    t = np.arange(bs * nb, dtype=np.float64) / fs
    tone = synth.to_cf32(np.exp(1j * (37500.0 / 1000.0) * (1.0 - np.cos(2.0 * np.pi * 1000.0 * t))))
    prog = synth.to_cf32(synth.fm_capture_realistic(bs * nb, fs=float(fs), seed=41)["iq"])
    x = torch.from_numpy(np.stack([tone, prog, np.zeros_like(tone)])).cuda()
    dm = pkg.BatchDemod(3, bs, fs, fast_math=True)
    mel = pkg.LogMel(3, 32000, max_input_frames=bs // 8, out_mode=0)
    cfg = logmel_ref.config(**dict(logmel_ref.GEOMETRIES["32k"], out_mode=0))
    chans = [ref.channel(cfg) for _ in range(3)]
    total = np.zeros((3, 80))
    for b in range(nb):
        dm.process(x[:, b * bs:(b + 1) * bs].contiguous())
        dm.synchronize()
        a = dm.audio_tensor()
        assert tuple(a.shape) == (3, bs // 8, 2)
        out, cnt = mel.process(a)
        ah, o, k = a.cpu().numpy(), out.cpu().numpy(), cnt.cpu().numpy()
        for c in range(3):
            w = chans[c].process(ah[c])
            assert k[c] == w.shape[0] and np.array_equal(bits(o[c, :k[c]]), bits(w)), (b, c)
            total[c] += w.astype(np.float64).sum(axis=0)
        assert mel.status().tobytes() == np.concatenate([ch.status() for ch in chans]).tobytes(), b
    st = mel.status()
    assert (st["frames"] == nb * bs // 8).all() and (st["spectra"] == (nb * bs // 8 - 800) // 320 + 1).all() and (st["nonfinite"] == 0).all()
    fb = ref.design(cfg)[3]
    k1000 = 1000 * 800 // 32000                                   # bin 25 is exactly 1 kHz
    band = int(np.argmax(fb[:, k1000]))
    assert fb[band, k1000] > 0 and int(np.argmax(total[0])) == band, (band, int(np.argmax(total[0])))
    dm.close(); mel.close()
