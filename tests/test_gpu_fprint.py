"""Audio fingerprinter on the GPU (fmd_fprint_*, Fingerprinter): words, counts, energies and status records against the C restatement of
the arithmetic contract (tests/cpp/fprint_ref.c, itself checked in test_fprint_cpu.py), bit for bit, compared as integer views: one call,
a call per hop, ragged calls on alternating streams, R = 4, 8 and 32, the default geometry at 32 kHz, n = 0, batch and row invariance, the
row map of 1 to 2049 stations at different fills, the
`active` mask over pre-filled outputs, NULL counts and energies, the smallest out_stride, odd strides and views, inf / NaN / denormal
samples, resets, the device's records, argument errors, the C++ adaptor, and demodulator -> Fingerprinter end to end.

The main shape is fs = 8000, H = 16, R = 4, 9 bands from 250 to 3500 Hz: bin edges 2, 3, 4, 5, 6, 9, 12, 16, 21, 28, K = 28 bins (no
multiple of 16: the padding to 32 is live) with three stations.  Station c has its own amplitude and its own order of programme, tone,
noise and silence, and has taken OFF[c] frames of its own before the calls under test, so the stations' row maps differ; one call of
16 * 50 frames completes 50 sub-blocks or more, far more than R, and more than the 32 a piece holds, so the library cuts it in two."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fprint_ref
from fprint_ref import bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FS = 8000
MAIN = fprint_ref.SMALL
N1 = 16 * 50
SCALE = (1.0, 0.37, 2.5)
OFF = (0, 5, 37)             # frames each station has taken before (no multiples of hop or 4)
ORDER = (("programme", "tone", "noise", "silence"), ("tone", "silence", "programme", "noise"), ("silence", "noise", "tone", "programme"))
RAGGED = [1, 7, 15, 16, 17, 63, 64, 65]


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return fprint_ref.build(tmp_path_factory.mktemp("fprint_ref_gpu"))


@pytest.fixture(scope="module")
def streams():
    """per station [OFF[c] + N1, 2] float32"""
    return [fprint_ref.mixed_signal(FS, OFF[c] + N1, ORDER[c], 100 + 10 * c, SCALE[c]) for c in range(3)]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _split(streams, off=OFF):
    """(pre [C, max(off), 2], x1 [C, n, 2]): what each station took before, and what the calls under test take"""
    n = min(s.shape[0] - o for s, o in zip(streams, off))
    pre = np.zeros((len(streams), max(max(off), 1), 2), np.float32)
    for c, s in enumerate(streams):
        pre[c, :off[c]] = s[:off[c]]
    return pre, np.stack([s[o:o + n] for s, o in zip(streams, off)])


def _want(ref, g, streams, off=OFF):
    """the restatement's stations: (words per station of the calls under test, energies per station, records [C])"""
    cfg = fprint_ref.config(**g)
    ws, es, st = [], [], []
    for s, o in zip(streams, off):
        ch = ref.channel(cfg)
        ch.process(s[:o])
        w, e = ch.process(s[o:])
        ws.append(w); es.append(e); st.append(ch.status())
    return ws, es, np.concatenate(st)


def _start(pkg, g, pre, off=OFF, **kw):
    """a Fingerprinter whose station c has taken its off[c] frames"""
    import torch
    f = {k: v for k, v in g.items() if k != "fs"}
    m = pkg.Fingerprinter(len(off), g["fs"], **f, **kw)
    pd = _cuda(pre)
    for c, o in enumerate(off):
        if o:
            active = torch.zeros(len(off), dtype=torch.uint8, device="cuda")
            active[c] = 1
            m.process(pd, n=o, active=active, nprints=False)
    return m


def _take(m, xd, cuts):
    """feeds xd [C, n, 2] in the pieces that end at `cuts` and at n; per station the words and the energies of all pieces"""
    C, n = xd.shape[0], xd.shape[1]
    gw, ge, at = [[] for _ in range(C)], [[] for _ in range(C)], 0
    for c in list(cuts) + [n]:
        out, cnt, en = m.process(xd[:, at:c], energy=True)
        o, k, e = _u32(out), cnt.cpu().numpy(), en.cpu().numpy()
        assert (k <= m.L.fmd_fprint_max_prints(m.hop, c - at)).all()
        for s in range(C):
            gw[s].append(o[s, :k[s]]); ge[s].append(e[s, :k[s]])
        at = c
    return [np.concatenate(r) for r in gw], [np.concatenate(r) for r in ge]


def _same(got, got_st, want, what=""):
    (gw, ge), (ww, we, wst) = got, want
    for c in range(len(ww)):
        assert gw[c].shape == ww[c].shape and ge[c].shape == we[c].shape, (what, c, gw[c].shape, ww[c].shape)
        bad = np.argwhere(bits(ge[c]) != bits(we[c]))
        assert bad.size == 0, (what, c, len(bad), bad[:4].tolist(), ge[c][tuple(bad[0])], we[c][tuple(bad[0])])
        assert np.array_equal(gw[c], ww[c]), (what, c, np.flatnonzero(gw[c] != ww[c])[:4])
    assert got_st.tobytes() == wst.tobytes(), (what, got_st, wst)


@pytest.fixture(scope="module")
def want_main(ref, streams):
    return _want(ref, MAIN, streams)


def test_main_shape_one_call(pkg, streams, want_main):
    pre, x1 = _split(streams)
    m = _start(pkg, MAIN, pre)
    got = _take(m, _cuda(x1), ())
    assert [w.shape[0] for w in got[0]] == [46, 46, 48]
    _same(got, m.status(), want_main)
    assert (m.status()["nonfinite"] == 0).all() and all(np.isfinite(e).all() for e in got[1])
    assert all(len(set(w.tolist())) > 8 for w in got[0])              # the words are no constant
    m.close()


def test_call_per_hop_and_ragged_calls_on_alternating_streams(pkg, ref, streams, want_main):
    import torch
    pre, x1 = _split(streams)
    xd = _cuda(x1)
    m = _start(pkg, MAIN, pre)
    _same(_take(m, xd, range(16, N1, 16)), m.status(), want_main, "a call per hop")
    m.close()
    # 1 + 7 + 15 + 16 + 17 + 63 + 64 + 65 + rest, the records behind every piece
    cuts = list(np.cumsum(RAGGED))
    m = _start(pkg, MAIN, pre)
    ss = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    cfg = fprint_ref.config(**MAIN)
    chans = [ref.channel(cfg) for _ in range(3)]
    for c in range(3):
        chans[c].process(streams[c][:OFF[c]])
    gw, ge, at = [[] for _ in range(3)], [[] for _ in range(3)], 0
    for i, c in enumerate(cuts + [N1]):
        out, cnt, en = m.process(xd[:, at:c], energy=True, stream=ss[i % 2])
        st = m.status()
        o, k, e = _u32(out), cnt.cpu().numpy(), en.cpu().numpy()
        for s in range(3):
            w, we = chans[s].process(x1[s, at:c])
            assert k[s] == w.shape[0] and np.array_equal(o[s, :k[s]], w) and np.array_equal(bits(e[s, :k[s]]), bits(we)), (i, s)
            assert st[s:s + 1].tobytes() == chans[s].status().tobytes(), (i, s)
            gw[s].append(o[s, :k[s]]); ge[s].append(e[s, :k[s]])
        at = c
    _same(([np.concatenate(r) for r in gw], [np.concatenate(r) for r in ge]), m.status(), want_main, "ragged")
    m.close()


@pytest.mark.parametrize("g", [dict(MAIN, n_sub=8), dict(MAIN, n_sub=32), dict(MAIN, hop=32, n_bands=2), dict(MAIN, n_sub=32, n_bands=33)],
                         ids=["r8", "r32_h16", "h32_two_bands", "r32_33_bands"])
def test_further_geometries(pkg, ref, streams, g):
    """R = 8 and R = 32 at H = 16 (K = 54 and 210), a hop of 32 with one bit a word, and all 32 bits: one call, and ragged calls"""
    pre, x1 = _split(streams)
    want = _want(ref, g, streams)
    assert all(w.size >= 15 for w in want[0])
    for cuts in ((), list(np.cumsum(RAGGED)), (100, 333)):
        m = _start(pkg, g, pre)
        _same(_take(m, _cuda(x1), cuts), m.status(), want, f"cuts {cuts}")
        m.close()


@pytest.fixture(scope="module")
def streams32():
    return [fprint_ref.mixed_signal(32000, 48000, ORDER[c], 200 + c, SCALE[c]) for c in range(2)]


def test_default_geometry_at_32k(pkg, ref, streams32):
    """368 / 32 / 33 bands, 628 bins: two stations x 1.5 s in one call, and split in two"""
    g = fprint_ref.DEFAULT_32K
    off = (0, 0)
    pre, x = _split(streams32, off)
    want = _want(ref, g, streams32, off)
    assert want[0][0].shape == (48000 // 368 - 32,)
    for cuts in ((), (20011,)):
        m = _start(pkg, g, pre, off)
        assert (m.hop, m.n_sub, m.n_bands, m.n_bins) == (368, 32, 33, 628) and m.state_bytes > 2 * 158720
        _same(_take(m, _cuda(x), cuts), m.status(), want, f"cuts {cuts}")
        m.close()


def test_n_zero_row_69_of_70_and_a_batch_of_one(pkg, ref, streams, want_main):
    import torch
    pre, x1 = _split(streams)
    # n = 0: counts 0, nothing else changes
    m = _start(pkg, MAIN, pre)
    before = m.status()
    out, cnt = m.process(_cuda(x1), n=0)
    assert cnt.cpu().numpy().tolist() == [0, 0, 0] and m.status().tobytes() == before.tobytes() and tuple(out.shape) == (3, 1)
    _same(_take(m, _cuda(x1), ()), m.status(), want_main, "behind n = 0")
    m.close()
    # row 69 of 70 and a batch of one are station 2's stream from the start
    s = streams[2]
    w = _want(ref, MAIN, [s], (0,))
    big = np.zeros((70, s.shape[0], 2), np.float32)
    big[69] = s
    big[:69] = streams[0][:1]
    m = pkg.Fingerprinter(70, FS, **{k: v for k, v in MAIN.items() if k != "fs"})
    out, cnt, en = m.process(_cuda(big), energy=True)
    k = int(cnt[69])
    assert np.array_equal(_u32(out[69, :k]), w[0][0]) and np.array_equal(bits(en[69, :k].cpu().numpy()), bits(w[1][0])) and m.status()[69:70].tobytes() == w[2].tobytes()
    m.close()
    m = pkg.Fingerprinter(1, FS, **{k: v for k, v in MAIN.items() if k != "fs"})
    pad = torch.zeros((1, s.shape[0] + 3, 2), device="cuda")
    pad[0, :s.shape[0]] = _cuda(s)
    out, cnt = m.process(pad, n=s.shape[0])
    assert np.array_equal(_u32(out[0, :int(cnt[0])]), w[0][0]) and m.status().tobytes() == w[2].tobytes()
    m.close()


def test_active_mask_null_counts_and_out_stride(pkg, ref, streams, want_main):
    import torch
    pre, x1 = _split(streams)
    xd = _cuda(x1)
    rows_max = pkg.fprint_max_prints(16, N1)
    assert rows_max == 50
    # station 1 inactive over outputs pre-filled with a pattern, two rows more than the call may write
    PAT = 0x7FC0BEEF
    out = torch.full((3, rows_max + 2), PAT, dtype=torch.int32, device="cuda")
    en = torch.zeros((3, rows_max + 2, 9), device="cuda")
    en.view(torch.int32).fill_(PAT)
    cnt = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    m = _start(pkg, MAIN, pre)
    before = m.status()
    m.process(xd, active=torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda"), out=out, nprints=cnt, energy=en)
    o, k, e, st = _u32(out), cnt.cpu().numpy(), en.cpu().numpy(), m.status()
    assert k.tolist() == [46, -7, 48] and st[1:2].tobytes() == before[1:2].tobytes()
    for c in (0, 2):
        assert np.array_equal(o[c, :k[c]], want_main[0][c]) and np.array_equal(bits(e[c, :k[c]]), bits(want_main[1][c]))
        assert st[c:c + 1].tobytes() == want_main[2][c:c + 1].tobytes()
        assert (o[c, k[c]:] == PAT).all() and (bits(e[c, k[c]:]) == PAT).all()     # the slots behind the words are left alone
    assert (o[1] == PAT).all() and (bits(e[1]) == PAT).all()
    # the skipped station then takes the same frames: as if it had never been skipped
    m.process(xd, active=torch.tensor([0, 1, 0], dtype=torch.uint8, device="cuda"), out=out, nprints=cnt, energy=en)
    assert np.array_equal(_u32(out[1, :46]), want_main[0][1]) and m.status().tobytes() == want_main[2].tobytes()
    m.close()
    # NULL d_nprints and NULL d_energy, and out_stride at its minimum; one word short is refused and changes nothing
    m = _start(pkg, MAIN, pre)
    out = torch.zeros((3, rows_max), dtype=torch.int32, device="cuda")
    res = m.process(xd, out=out, nprints=False)
    assert len(res) == 2 and res[1] is None and res[0] is out
    o = _u32(out)
    for c in range(3):
        assert np.array_equal(o[c, :want_main[0][c].shape[0]], want_main[0][c])
    st = m.status()
    en = torch.zeros((3, rows_max, 9), device="cuda")
    for args in ((out.data_ptr(), rows_max - 1, None, None, 0), (out.data_ptr(), rows_max, None, en.data_ptr(), rows_max * 9 - 1)):
        with pytest.raises(pkg.FmdError) as e:
            m._check(m.L.fmd_fprint_process_f32_dev(m.g, xd.data_ptr(), N1, N1, None, *args, None))
        assert e.value.status == -1 and m.status().tobytes() == st.tobytes()
    with pytest.raises(ValueError):
        m.process(xd, out=torch.zeros((3, rows_max - 1), dtype=torch.int32, device="cuda"))
    m.close()


ROWMAP_CALLS = (7, 73)       # frames of the two calls under test, behind a first call of ROWMAP_PRE frames that every other station takes
ROWMAP_PRE = 91


@pytest.mark.parametrize("ends", [True, False], ids=["ends_taken", "ends_left_out"])
@pytest.mark.parametrize("C", [1, 1024, 1025, 2049])
def test_row_map_of_many_stations(pkg, ref, C, ends):
    """1, 1024, 1025 and 2049 stations (a thread of k_fprint_map takes 1, 1, 2 and 3 of them; the short and the empty shares fall on
    other threads) at the main shape.  A first call of 91 frames under a mask of its own (every other station) leaves the stations at
    fill 11 or 0; then two calls of 7 and 73 frames under a mask that leaves out a scattered third, stations 0 and C - 1 among them or,
    with `ends`, both taken.  A call has one n, so its stations' rows differ by one at most: the call of 7 frames completes 1 sub-block
    (fill 11) or none (fill 0), the call of 73 then 4 (fill 2) or 5 (fill 7), from the fills the call before wrote.  Every station's words,
    count and energies of both calls and its record behind each, bit for bit; an inactive station's are left as they were filled."""
    import torch
    rng = np.random.default_rng(5000 + 2 * C + int(ends))
    x = (rng.standard_normal((C, ROWMAP_PRE + sum(ROWMAP_CALLS), 2)) * rng.uniform(0.05, 2.0, (C, 1, 1))).astype(np.float32)
    c = np.arange(C)
    first = c % 2 == 0
    active = c % 3 != 1
    active[[0, C - 1]] = ends
    cfg = fprint_ref.config(**MAIN)
    chans = [ref.channel(cfg) for _ in range(C)]
    m = pkg.Fingerprinter(C, FS, **{k: v for k, v in MAIN.items() if k != "fs"})
    xd = _cuda(x)
    m.process(xd[:, :ROWMAP_PRE], active=_cuda(first.astype(np.uint8)), nprints=False)
    for s in np.flatnonzero(first):
        chans[s].process(x[s, :ROWMAP_PRE])
    assert m.status().tobytes() == np.concatenate([ch.status() for ch in chans]).tobytes()
    PAT, at, ad = 0x7FC0BEEF, ROWMAP_PRE, _cuda(active.astype(np.uint8))
    for n, subs in zip(ROWMAP_CALLS, ((1, 0), (4, 5))):
        fill = m.status()["fill"].astype(np.int64)
        assert C == 1 or set(((fill[active] + n) // 16).tolist()) == set(subs)
        rows = pkg.fprint_max_prints(16, n)
        out = torch.full((C, rows), PAT, dtype=torch.int32, device="cuda")
        en = torch.zeros((C, rows, 9), device="cuda")
        en.view(torch.int32).fill_(PAT)
        cnt = torch.full((C,), -7, dtype=torch.int32, device="cuda")
        m.process(xd[:, at:at + n], active=ad, out=out, nprints=cnt, energy=en)
        o, k, e = _u32(out), cnt.cpu().numpy(), bits(en.cpu().numpy())
        for s in range(C):
            if not active[s]:
                assert k[s] == -7 and (o[s] == PAT).all() and (e[s] == PAT).all(), (n, s)
                continue
            w, we = chans[s].process(x[s, at:at + n])
            assert k[s] == w.shape[0] and np.array_equal(o[s, :k[s]], w) and np.array_equal(e[s, :k[s]], bits(we)), (n, s)
            assert (o[s, k[s]:] == PAT).all() and (e[s, k[s]:] == PAT).all(), (n, s)
        assert m.status().tobytes() == np.concatenate([ch.status() for ch in chans]).tobytes(), n
        at += n
    st = m.status()
    assert C == 1 or (set(st["prints"][active & first].tolist()), set(st["prints"][active & ~first].tolist())) == ({6}, {1})
    m.close()


def test_odd_stride_and_odd_view(pkg, ref, streams, want_main):
    """an in_stride that is odd, a view that starts at an odd frame, and NaN behind n: not read"""
    import torch
    pre, x1 = _split(streams)
    buf = torch.full((3, N1 + 9, 2), float("nan"), device="cuda")
    buf[:, 3:3 + N1] = _cuda(x1)
    m = _start(pkg, MAIN, pre)
    out, cnt, en = m.process(buf[:, 3:], n=N1, energy=True)
    k = cnt.cpu().numpy()
    _same(([_u32(out[c, :k[c]]) for c in range(3)], [en[c, :k[c]].cpu().numpy() for c in range(3)]), m.status(), want_main, "odd view")
    m.close()


def test_special_samples(pkg, ref, streams):
    """+-inf, NaN and denormal samples: the frames that hold a non-finite sample are non-finite as the chains give them, a NaN energy is
    written as 0x7fc00000, and the counters agree; denormal input is kept, not flushed"""
    s = [a.copy() for a in streams]
    s[0][100, 0] = np.inf
    s[0][400, 1] = -np.inf
    s[1][200, 1] = np.nan
    s[2][:] = 0.0
    s[2][37:300, 0] = np.float32(3e-39) * np.sign(streams[2][37:300, 0] + 1e-30)
    s[2][37:300, 1] = np.float32(1e-40)
    s[2][400:500] = streams[2][400:500] * 1e-18
    pre, x1 = _split(s)
    want = _want(ref, MAIN, s)
    m = _start(pkg, MAIN, pre)
    got = _take(m, _cuda(x1), (300,))
    _same(got, m.status(), want, "special")
    assert want[2]["nonfinite"][0] > 0 and want[2]["nonfinite"][1] > 0 and want[2]["nonfinite"][2] == 0
    assert np.any(want[1][2] != 0.0)
    m.close()


def test_reset_mid_window_records_and_argument_errors(pkg, ref, streams, want_main):
    import torch
    pre, x1 = _split(streams)
    xd = _cuda(x1)
    m = _start(pkg, MAIN, pre, max_input_frames=N1)
    m.process(xd, n=77)
    m.reset(1)                                                    # station 1 alone starts over, mid-window
    st = m.status()
    assert st[1].tobytes() == np.zeros(1, fprint_ref.STATUS_DTYPE).tobytes() and st[0]["frames"] == 77 and st[2]["fill"] == (37 + 77) % 16
    out, cnt, en = m.process(xd[:, 77:], energy=True)
    cfg = fprint_ref.config(**MAIN)
    ch = ref.channel(cfg)
    w, we = ch.process(x1[1, 77:])
    k = int(cnt[1])
    assert np.array_equal(_u32(out[1, :k]), w) and np.array_equal(bits(en[1, :k].cpu().numpy()), bits(we)) and m.status()[1:2].tobytes() == ch.status().tobytes()
    assert m.status()[[0, 2]].tobytes() == want_main[2][[0, 2]].tobytes()
    m.reset()
    assert m.status().tobytes() == np.zeros(3, fprint_ref.STATUS_DTYPE).tobytes()
    _same(_take(m, xd, ()), m.status(), _want(ref, MAIN, list(x1), (0, 0, 0)), "behind reset(-1)")
    # the device's own records
    torch.cuda.synchronize()
    ptr = m.status_dev_ptr()

    class _Arr:
        __cuda_array_interface__ = {"shape": (3 * 32,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    raw = torch.as_tensor(_Arr(), device="cuda").clone()
    assert raw.cpu().numpy().tobytes() == m.status().tobytes()
    st = m.status()
    out = torch.zeros((3, 50), dtype=torch.int32, device="cuda")
    call = m.L.fmd_fprint_process_f32_dev
    bad = [lambda: m.process(xd, n=N1 + 1), lambda: m.process(xd, n=-1), lambda: m.reset(3), lambda: m.reset(-2),
           lambda: m._check(call(m.g, xd.data_ptr() + 4, N1, 16, None, out.data_ptr(), 50, None, None, 0, None)),
           lambda: m._check(call(m.g, xd.data_ptr(), N1, 16, None, out.data_ptr() + 2, 50, None, None, 0, None)),
           lambda: m._check(call(m.g, xd.data_ptr(), N1, 16, None, out.data_ptr(), 50, None, out.data_ptr() + 2, 450, None)),
           lambda: m._check(call(m.g, None, N1, 16, None, out.data_ptr(), 50, None, None, 0, None)),
           lambda: m._check(call(m.g, xd.data_ptr(), N1, 16, None, None, 50, None, None, 0, None))]
    for k, f in enumerate(bad):
        with pytest.raises(pkg.FmdError) as e:
            f()
        assert e.value.status == -1, k
    small = pkg.Fingerprinter(3, FS, **{**{k: v for k, v in MAIN.items() if k != "fs"}, "max_input_frames": 128})
    with pytest.raises(pkg.FmdError) as e:
        small.process(xd, n=129)
    assert e.value.status == -1 and int(small.status()[0]["frames"]) == 0
    small.close()
    for f in (lambda: m.process(xd[:2]), lambda: m.process(xd, active=torch.ones(2, dtype=torch.uint8, device="cuda")), lambda: m.process(xd.double()),
              lambda: m.process(xd, nprints=torch.zeros(3, dtype=torch.int64, device="cuda")), lambda: m.process(xd, out=torch.zeros((3, 50), device="cuda")),
              lambda: m.process(xd, energy=torch.zeros((3, 50, 8), device="cuda"))):
        with pytest.raises(ValueError):
            f()
    base = {k: v for k, v in MAIN.items() if k != "fs"}
    for kw in (dict(hop=24), dict(hop=0), dict(hop=1040), dict(n_sub=5), dict(n_sub=64), dict(n_bands=1), dict(n_bands=34), dict(f_min_hz=0.0), dict(f_max_hz=250.0),
               dict(f_max_hz=2000.0), dict(f_min_hz=60.0), dict(f_max_hz=4000.0), dict(max_input_frames=0), dict(max_input_frames=(1 << 30) + 1)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.Fingerprinter(3, FS, **{**base, **kw})
        assert e.value.status == -1 and str(e.value), kw
    with pytest.raises(pkg.FmdError):
        pkg.Fingerprinter(0, FS)
    assert m.status().tobytes() == st.tobytes()
    m.close()


def test_cpp_adaptor(pkg, ref, streams, tmp_path):
    """tests/cpp/fprint_main.cpp takes a file of audio in calls of 100 frames through AudioFingerprint_GPU; the words its host views give
    and the records it prints are the restatement's, and it exits with 7 unless the device's views and records are the host's"""
    exe = tmp_path / "fprint_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}", f"-I{ROOT / 'fm-radio_amd' / 'host'}",
                    "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "fprint_main.cpp"), f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64",
                    f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    a = np.ascontiguousarray(np.stack([streams[0][:N1], streams[1][:N1]]))
    a.tofile(tmp_path / "audio.f32")
    r = subprocess.run([str(exe), str(tmp_path / "audio.f32"), "2", str(FS), "16", "4", "9", "250", "3500", "100", str(tmp_path / "words")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2
    cfg = fprint_ref.config(**MAIN)
    for c, line in enumerate(lines):
        ch = ref.channel(cfg)
        w, _ = ch.process(a[c])
        assert bytes.fromhex(line.split()[0]) == ch.status().tobytes(), c
        assert np.array_equal(np.fromfile(tmp_path / f"words.{c}.u32", np.uint32), w), c
    assert float(lines[0].split()[1]) == 46 * 16 / FS


def _fm(audio32: np.ndarray, level: float) -> np.ndarray:
    """mono FM at 256 kSa/s of audio at 32 kHz (band-limited interpolation by 8, 75 kHz deviation at |m| = 0.5), [n, 2] float32"""
    n = audio32.size
    up = np.fft.irfft(np.fft.rfft(audio32), 8 * n) * 8.0
    ph = 2.0 * np.pi * 75000.0 * np.cumsum(np.clip(up / 0.5, -1.0, 1.0)) / 256000.0
    iq = level * 100.0 * np.exp(1j * ph)
    return np.stack([iq.real, iq.imag], axis=1).astype(np.float32)


def test_demodulator_end_to_end(pkg, ref):
    """Three stations at 256 kSa/s through BatchDemod in the tolerance mode, 24 blocks of 16384 samples (2048 frames of audio at 32 kHz
    each, 1.54 s), Fingerprinter at the default geometry on audio_tensor() after each block: bit for bit the restatement on the same
    audio copied to the host.  Stations 0 and 1 carry the same synthesised programme at carrier levels 1 and 0.3, station 2 another
    programme.  Conditions, far on the safe side of the paper's 0.35: BER(0, 1) < 0.15; BER(0, 2) and BER(1, 2) > 0.40; each against the
    float64 fingerprint of its source audio at the best alignment by fprint_match < 0.15.  Measured: DESIGN.md §6o."""
    import torch
    fs, bs, nb = 256_000, 16384, 24
    n32 = bs * nb // 8
    src = [fprint_ref.programme(32000, n32, 61)[:, 0].astype(np.float64), None, fprint_ref.programme(32000, n32, 62)[:, 0].astype(np.float64)]
    src[1] = src[0]
    x = torch.from_numpy(np.stack([_fm(src[0], 1.0), _fm(src[1], 0.3), _fm(src[2], 1.0)])).cuda()
    dm = pkg.BatchDemod(3, bs, fs, fast_math=True)
    fp = pkg.Fingerprinter(3, 32000, max_input_frames=bs // 8)
    cfg = fprint_ref.config(**fprint_ref.DEFAULT_32K)
    chans = [ref.channel(cfg) for _ in range(3)]
    words = [[] for _ in range(3)]
    for b in range(nb):
        dm.process(x[:, b * bs:(b + 1) * bs].contiguous())
        dm.synchronize()
        a = dm.audio_tensor()
        assert tuple(a.shape) == (3, bs // 8, 2)
        out, cnt, en = fp.process(a, energy=True)
        ah, o, k, e = a.cpu().numpy(), _u32(out), cnt.cpu().numpy(), en.cpu().numpy()
        for c in range(3):
            w, we = chans[c].process(ah[c])
            assert k[c] == w.shape[0] and np.array_equal(o[c, :k[c]], w) and np.array_equal(bits(e[c, :k[c]]), bits(we)), (b, c)
            words[c].append(w)
        assert fp.status().tobytes() == np.concatenate([ch.status() for ch in chans]).tobytes(), b
    st = fp.status()
    assert (st["frames"] == n32).all() and (st["prints"] == n32 // 368 - 32).all() and (st["nonfinite"] == 0).all()
    w = [np.concatenate(r) for r in words]
    assert w[0].size == 101
    b01, b02, b12 = pkg.fprint_ber(w[0], w[1]), pkg.fprint_ber(w[0], w[2]), pkg.fprint_ber(w[1], w[2])
    own = []
    for c in range(3):
        srcw = fprint_ref.model_words(cfg, np.stack([src[c], src[c]], axis=1).astype(np.float32))
        own.append(pkg.fprint_match(w[c][8:-8], srcw))
    print(f"BER(0, 1) = {b01:.4f}, BER(0, 2) = {b02:.4f}, BER(1, 2) = {b12:.4f}; against the source, (offset, BER): {own}")
    assert b01 < 0.15 and b02 > 0.40 and b12 > 0.40, (b01, b02, b12)
    assert all(r < 0.15 for _, r in own), own
    dm.close(); fp.close()
