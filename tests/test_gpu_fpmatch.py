"""Fingerprint matcher on the GPU (fmd_fpmatch_*, FingerprintMatcher): events, counts, bytes and status records against the numpy
restatement of the definition (tests/fpmatch_ref.py, itself checked in test_fpmatch_cpu.py), bit for bit: the whole stream in one call, a
call per word, ragged calls on alternating streams, n_bits 32 and 9, the default W = 256 / I = 64, a catalogue across several column tiles
with a duplicated track, more column tiles than column groups, n = 0, a batch of one, row 69 of 70, the row map of 1 to 2049 stations
with uneven counts, the `active` mask over pre-filled
outputs, d_nwords NULL and clamped, NULL counts and bytes, the smallest events_stride, load and reset in mid-stream, argument errors, the
C++ adaptor, and demodulator -> Fingerprinter -> FingerprintMatcher end to end.

The main shape is W = 16, I = 4, hold 2, three stations that have taken 0, 5 and 37 words before the calls under test (three query
phases), the catalogue's tracks 16, 17, 50 and 700 words long; the 140 words a station then takes fire 32, 33 and 35 queries, 13 query
blocks of the search."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fpmatch_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
RAGGED = [1, 3, 4, 5, 15, 16, 17]


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


def _cuda(words):
    """runs of uint32 (equally long) -> [C, n] int32 CUDA tensor, as Fingerprinter.process returns its words"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(w, np.uint32) for w in words])).view(np.int32)).cuda()


def _i32(v):
    import torch
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _pair(pkg, cfg, tracks):
    """(the object, the restatement) of cfg with `tracks` loaded"""
    lib_cfg = {k: v for k, v in cfg.items() if k != "n_channels"}
    m, ref = pkg.FingerprintMatcher(cfg["n_channels"], **lib_cfg), R.Matcher(**cfg)
    assert m.cfg.max_errs == ref.cfg["max_errs"]
    if tracks is not None:
        m.load(tracks)
        assert ref.load(tracks)
    return m, ref


def _same_call(pkg, got, want, what=""):
    """one call's outputs: the events' bytes, the counts and the two bytes of every station the restatement took"""
    (ev, cnt, fl, ok), (wev, wfl, wok) = got, want
    k = cnt.cpu().numpy()
    for c in range(len(wev)):
        if wev[c] is None:
            continue
        assert k[c] == wev[c].size, (what, c, k[c], wev[c].size)
        g = pkg.FingerprintMatcher.events_of(ev, k, c)
        assert g.tobytes() == wev[c].tobytes(), (what, c, g, wev[c])
        assert int(fl[c]) == wfl[c] and int(ok[c]) == wok[c], (what, c)


def _both(pkg, m, ref, words, cuts=(), each=False, alternate=False, **kw):
    """feeds `words` (runs of equal length) to both in the pieces that end at `cuts` and at the end, comparing every call's outputs (and
    with `each` the records); returns the restatement's events per station"""
    import torch
    n = len(words[0])
    xd = _cuda(words)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()] if alternate else [None]
    torch.cuda.synchronize()
    all_ev, at = [[] for _ in words], 0
    for i, c in enumerate(list(cuts) + [n]):
        s = streams[i % len(streams)]
        got = m.process(xd[:, at:c], stream=s, **kw) if c > at else m.process(xd[:, :1], n=0, stream=s, **kw)
        if s is not None:
            s.synchronize()
        want = ref.process([w[at:c] for w in words], n=c - at)
        _same_call(pkg, got, want, (at, c))
        if each:
            assert m.status().tobytes() == ref.status().tobytes(), (at, c)
        for r, e in zip(all_ev, want[0]):
            r.append(e)
        at = c
    assert m.status().tobytes() == ref.status().tobytes()
    return [np.concatenate(r) for r in all_ev]


def _main(pkg, n_bits=32, **over):
    """the main shape with every station's PRE words taken (one call with d_nwords = PRE): (object, restatement, the 140 words a station)"""
    tracks = R.main_catalogue(n_bits)
    streams = R.main_streams(tracks, n_bits)
    m, ref = _pair(pkg, dict(R.MAIN, n_bits=n_bits, **over), tracks)
    top = max(R.PRE)
    pre = [np.concatenate([s[:p], np.zeros(top - p, np.uint32)]) for s, p in zip(streams, R.PRE)]
    got = m.process(_cuda(pre), nwords=_i32(R.PRE))
    _same_call(pkg, got, ref.process(pre, nwords=list(R.PRE), n=top), "pre")
    assert m.status().tobytes() == ref.status().tobytes() and m.status()["words"].tolist() == list(R.PRE)
    return m, ref, [s[p:] for s, p in zip(streams, R.PRE)]


@pytest.mark.parametrize("n_bits", [32, 9])
def test_one_call(pkg, n_bits):
    """the whole stream in one call: 100 queries, more than one query block, hits, misses, a switch, a release and the splice"""
    m, ref, words = _main(pkg, n_bits)
    ev = _both(pkg, m, ref, words)
    d = m.design
    assert [e.size for e in ev] == [32, 33, 35] and 100 > 2 * d.query_block and all((e["flags"] == 1).any() and (e["flags"] == 0).any() for e in ev)
    assert all(k == 1 for _, _, k in ref.ties)                               # nothing here rests on the tie rule
    st = m.status()
    assert st["words"].tolist() == [140 + p for p in R.PRE] and (st["fill"] == 16).all() and (st["clamped"] == 0).all()
    m.close()


def test_a_call_per_word(pkg):
    m, ref, words = _main(pkg)
    one = _both(pkg, *_main(pkg)[:2], words)
    ev = _both(pkg, m, ref, words, cuts=range(1, 140))
    assert [e.tobytes() for e in ev] == [e.tobytes() for e in one]
    m.close()


@pytest.mark.parametrize("n_bits", [32, 9])
def test_ragged_calls_on_alternating_streams(pkg, n_bits):
    """1 + 3 + 4 + 5 + 15 + 16 + 17 + the rest, every other call on another stream, the records checked after every call"""
    m, ref, words = _main(pkg, n_bits)
    _both(pkg, m, ref, words, cuts=list(np.cumsum(RAGGED)), each=True, alternate=True)
    m.close()


def test_default_block_and_interval(pkg):
    """W = 256 / I = 64 (the default) on two stations: a programme at 5 % from its word 100, and unrelated words then another at 30 %"""
    tracks = [R.random_words(600, 301), R.random_words(300, 302)]
    cfg = dict(n_channels=2, max_words=400, max_tracks=2, max_catalogue_words=900)
    m, ref = _pair(pkg, cfg, tracks)
    assert (m.block, m.interval, m.max_errs, m.hold) == (256, 64, 2867, 3)
    words = [R.flip(tracks[0][100:500], 0.05, 303), np.concatenate([R.random_words(100, 304), R.flip(tracks[1], 0.30, 305)])]
    ev = _both(pkg, m, ref, words, cuts=[6, 11, 70, 200, 256, 257], each=True)
    assert ev[0]["offset"].tolist() == [100, 164, 228] and ev[0]["track"].tolist() == [0, 0, 0] and ev[1]["flags"].tolist() == [0, 0, 1]
    assert ev[1]["end"].tolist() == [256, 320, 384] and (ev[1]["track"][2], ev[1]["offset"][2]) == (1, 28)
    m.close()


def test_a_catalogue_across_column_tiles(pkg):
    """a catalogue longer than three of the search's column tiles (the tile's size from the design unit) with one track in two of them:
    station 0 plays that track, so the two tiles' partial minima tie and the lower position wins; station 1 plays across a tile's edge,
    station 2 the last track, exactly W words, whose one position is the catalogue's last"""
    cfg = dict(R.MAIN, max_catalogue_words=1 << 14)
    tile = pkg.fpmatch_design(pkg.fpmatch_default_config(**cfg)).tile
    tracks = R.tiled_catalogue(tile, 16)
    m, ref = _pair(pkg, cfg, tracks)
    assert m.design.groups >= 4
    starts = np.concatenate([[0], np.cumsum([t.size for t in tracks])])
    edge = 2 * tile - int(starts[2])                                         # track 2's word at the edge between tiles 1 and 2
    assert 40 < edge < tracks[2].size - 40
    words = [tracks[1][4:44], R.flip(tracks[2][edge - 20:edge + 20], 0.05, 710), np.concatenate([R.random_words(24, 711), tracks[4]])]
    ev = _both(pkg, m, ref, words, cuts=[13])
    ties = {c: [k for s, _, k in ref.ties if s == c] for c in range(3)}
    assert set(ties[0]) == {2} and set(ties[1]) == {1}
    assert (ev[0]["track"] == 1).all() and (ev[0]["errs"] == 0).all() and ev[0]["offset"].tolist() == list(range(4, 29, 4))
    assert ev[1]["track"].tolist() == [2] * 7 and (ev[1]["offset"] + 16 > edge - 20).all() and ev[1]["offset"][0] < edge - 16 < edge < ev[1]["offset"][-1] + 16
    assert (ev[2]["track"][-1], ev[2]["offset"][-1], ev[2]["errs"][-1]) == (4, 0, 0)
    m.close()


def test_more_column_tiles_than_groups(pkg):
    """a catalogue of more column tiles than the scratch has column groups, so that a workgroup of the search walks several tiles and
    carries its minimum from one to the next: one track twice, in two tiles of the same group"""
    cfg = dict(n_channels=1, block=16, interval=8, max_words=64, max_tracks=8)
    d = pkg.fpmatch_design(pkg.fpmatch_default_config(**cfg, max_catalogue_words=1 << 28))
    G, tile = d.groups, d.tile
    dup = R.random_words(40, 801)
    tracks = [R.random_words(tile + 100, 802), dup, R.random_words(G * tile - 40, 803), dup.copy(), R.random_words(tile, 804)]
    D = sum(t.size for t in tracks)
    m, ref = _pair(pkg, dict(cfg, max_catalogue_words=D), tracks)
    assert (D - 16 + 1 + tile - 1) // tile > m.design.groups == G
    starts = np.cumsum([0] + [t.size for t in tracks])
    assert (starts[3] // tile - starts[1] // tile) % G == 0                  # the same column group
    ev = _both(pkg, m, ref, [np.concatenate([dup[3:27], R.flip(tracks[4][500:524], 0.05, 805)])], cuts=[20])
    assert ev[0]["track"].tolist()[:3] == [1, 1, 1] and ev[0]["offset"].tolist()[:3] == [3, 11, 19][:3] and ev[0]["track"][-1] == 4 and ev[0]["offset"][-1] == 508
    assert [k for _, _, k in ref.ties][:2] == [2, 2]
    m.close()


def test_n_zero_and_a_batch_of_one(pkg):
    tracks = R.main_catalogue()
    streams = R.main_streams(tracks)
    m, ref = _pair(pkg, dict(R.MAIN, n_channels=1), tracks)
    w = [streams[0]]
    ev = _both(pkg, m, ref, w, cuts=[0, 30, 30, 77], each=True)              # n = 0 at the start and in mid-stream: the bytes are written
    m3, ref3, words = _main(pkg)
    one = _both(pkg, m3, ref3, words)
    assert ev[0].tobytes() == one[0].tobytes()
    m.close(); m3.close()


def test_row_69_of_70(pkg):
    """70 stations, station c with stream c mod 3 and its PRE words: every row gives what its stream gives in a batch of three"""
    import torch
    tracks = R.main_catalogue()
    streams = R.main_streams(tracks)
    m3, ref3, words = _main(pkg)
    want = _both(pkg, m3, ref3, words)
    m = pkg.FingerprintMatcher(70, **{k: v for k, v in R.MAIN.items() if k != "n_channels"})
    m.load(tracks)
    top = max(R.PRE)
    pre = [np.concatenate([streams[c % 3][:R.PRE[c % 3]], np.zeros(top - R.PRE[c % 3], np.uint32)]) for c in range(70)]
    m.process(_cuda(pre), nwords=_i32([R.PRE[c % 3] for c in range(70)]))
    ev, cnt, fl, ok = m.process(_cuda([words[c % 3] for c in range(70)]))
    k, st = cnt.cpu().numpy(), m.status()
    for c in range(70):
        assert pkg.FingerprintMatcher.events_of(ev, k, c).tobytes() == want[c % 3].tobytes(), c
        assert st[c].tobytes() == ref3.status()[c % 3].tobytes() and int(fl[c]) == int(st[c]["flags"]) and int(ok[c]) == int(st[c]["flags"]) & 1, c
    m.close(); m3.close()


def _rowmap(pkg, m, ref, C, ends, records):
    """R.rowmap_case through the object and the restatement: every station's events, count and bytes of both calls (an inactive station's
    are left as they were filled), and records(m, ref) behind each call"""
    import torch
    tracks, calls, active = R.rowmap_case(C, ends)
    m.load(tracks)
    assert ref.load(tracks)
    ad = torch.from_numpy(active.astype(np.uint8)).cuda()
    fired = []
    for i, (words, k) in enumerate(calls):
        n = words.shape[1]
        rows = pkg.fpmatch_max_events(m.interval, n)
        ev = torch.full((C, rows, 3), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        cnt = torch.full((C,), -7, dtype=torch.int32, device="cuda")
        fl, ok = torch.full((C,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((C,), 0xDD, dtype=torch.uint8, device="cuda")
        m.process(torch.from_numpy(words.view(np.int32)).cuda(), nwords=torch.from_numpy(k).cuda(), active=ad, events=ev, nevents=cnt, flags=fl, ok=ok)
        wev, wfl, wok = ref.process(words, nwords=k, n=n, active=active)
        raw = ev.cpu().numpy()
        got = raw.reshape(C, rows * 3).view(R.EVENT_DTYPE)
        cnt, fl, ok = cnt.cpu().numpy(), fl.cpu().numpy(), ok.cpu().numpy()
        for c in range(C):
            if not active[c]:
                assert wev[c] is None and (cnt[c], fl[c], ok[c]) == (-7, 0xEE, 0xDD) and (raw[c] == 0x5A5A5A5A5A5A5A5A).all(), (i, c)
                continue
            assert cnt[c] == wev[c].size and got[c, :cnt[c]].tobytes() == wev[c].tobytes() and (raw[c, cnt[c]:] == 0x5A5A5A5A5A5A5A5A).all(), (i, c, got[c], wev[c])
            assert (fl[c], ok[c]) == (wfl[c], wok[c]), (i, c)
        records(m, ref)
        fired.append(np.array([-1 if e is None else e.size for e in wev]))
    if C > 1:                                                                # in either call stations of no row and of several; hits, and tracks held
        assert all((f == 0).any() and (f >= 2).any() for f in fired) and ref.status()["hits"].sum() > C // 8 and (ref.status()["track"] >= 0).any()


def _same_status(m, ref):
    assert m.status().tobytes() == ref.status().tobytes()


@pytest.mark.parametrize("ends", [True, False], ids=["ends_taken", "ends_left_out"])
@pytest.mark.parametrize("C", R.ROWMAP_STATIONS)
def test_row_map_of_many_stations(pkg, C, ends):
    """1, 1024, 1025 and 2049 stations (a thread of k_fpmatch_map takes 1, 1, 2 and 3 of them; the short and the empty shares fall on
    other threads), a scattered third inactive, uneven d_nwords, two calls: every station's outputs and record, bit for bit"""
    m, ref = _pair(pkg, dict(R.MAIN, n_channels=C), None)
    _rowmap(pkg, m, ref, C, ends, _same_status)
    m.close()


def test_active_mask_over_prefilled_outputs(pkg):
    """a station whose byte is 0 keeps its ring, record, events, count and bytes; an active station's slots behind its events are left alone"""
    import torch
    m, ref, words = _main(pkg)
    xd = _cuda(words)
    rows = pkg.fpmatch_max_events(4, 41) + 2
    ev = torch.full((3, rows, 3), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    cnt = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    fl, ok = torch.full((3,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((3,), 0xDD, dtype=torch.uint8, device="cuda")
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    before = m.status()
    got = m.process(xd[:, :41], active=active, events=ev, nevents=cnt, flags=fl, ok=ok)
    want = ref.process([w[:41] for w in words], n=41, active=[1, 0, 1])
    _same_call(pkg, got, want)
    raw, k = ev.cpu().numpy(), cnt.cpu().numpy()
    assert k[1] == -7 and int(fl[1]) == 0xEE and int(ok[1]) == 0xDD and (raw[1] == 0x5A5A5A5A5A5A5A5A).all() and m.status()[1].tobytes() == before[1].tobytes()
    for c in (0, 2):
        assert 0 < k[c] < rows and (raw[c, k[c]:] == 0x5A5A5A5A5A5A5A5A).all()
    # the skipped station goes on as if the call had not been: its ring was kept
    got = m.process(xd[:, :41], active=active.logical_not())
    _same_call(pkg, got, ref.process([w[:41] for w in words], n=41, active=[0, 1, 0]))
    _both(pkg, m, ref, [w[41:] for w in words])
    m.close()


def test_nwords_null_and_clamped(pkg):
    """d_nwords NULL takes n of every station; counts of -3 and n + 5 are clamped into [0, n] and counted"""
    m, ref, words = _main(pkg)
    xd = _cuda(words)
    got = m.process(xd[:, :20], nwords=_i32([-3, 25, 7]))
    _same_call(pkg, got, ref.process([w[:20] for w in words], nwords=[-3, 25, 7], n=20))
    st = m.status()
    assert st.tobytes() == ref.status().tobytes() and st["clamped"].tolist() == [1, 1, 0] and st["words"].tolist() == [0, 25, 44]
    got = m.process(xd[:, 20:40])
    _same_call(pkg, got, ref.process([w[20:40] for w in words], n=20))
    assert m.status().tobytes() == ref.status().tobytes() and m.status()["clamped"].tolist() == [1, 1, 0]
    m.close()


def test_null_outputs_and_the_smallest_events_stride(pkg):
    import torch
    m, ref, words = _main(pkg)
    xd = _cuda(words)
    ev, cnt, fl, ok = m.process(xd[:, :50], nevents=False, flags=False, ok=False)
    want = ref.process([w[:50] for w in words], n=50)
    assert cnt is None and fl is None and ok is None
    for c in range(3):
        assert pkg.FingerprintMatcher.events_of(ev, None, c)[:want[0][c].size].tobytes() == want[0][c].tobytes()
    assert m.status().tobytes() == ref.status().tobytes()
    # 37 words: 10 events at most, and a station in the right phase writes all 10
    rows = pkg.fpmatch_max_events(4, 37)
    tight = torch.zeros((3, rows, 3), dtype=torch.int64, device="cuda")
    got = m.process(xd[:, 50:87], events=tight)
    _same_call(pkg, got, ref.process([w[50:87] for w in words], n=37))
    assert rows == 10 and int(got[1][1]) == 10
    before = m.status()
    with pytest.raises(pkg.FmdError) as e:
        m._check(m.L.fmd_fpmatch_process_dev(m.g, xd.data_ptr(), xd.stride(0), None, 37, None, tight.data_ptr(), rows - 1, None, None, None, None))
    assert e.value.status == -1 and "events_stride" in str(e.value) and m.status().tobytes() == before.tobytes()
    m.close()


def test_load_and_reset_in_mid_stream(pkg):
    """load to another catalogue (the same tracks in another order, one left out) and to an empty one, and the reset of one station, in
    mid-stream: the detector is cleared and the ring kept; the reset station starts over"""
    m, ref, words = _main(pkg)
    _both(pkg, m, ref, [w[:50] for w in words], each=True)
    other = [R.main_catalogue()[i] for i in (3, 0, 2)]
    m.load(other)
    assert ref.load(other) and m.status().tobytes() == ref.status().tobytes() and (m.status()["track"] == -1).all() and m.n_tracks == 3
    _both(pkg, m, ref, [w[50:62] for w in words], cuts=[2], each=True)       # the first query after the load looks back over the kept ring
    assert (m.status()["words"] == np.array(R.PRE) + 62).all()
    m.reset(1)
    ref.reset(1)
    assert m.status().tobytes() == ref.status().tobytes() and m.status()[1]["track"] == -1 and m.status()[1]["words"] == 0
    _both(pkg, m, ref, [w[62:100] for w in words], cuts=[7], each=True)
    m.load([])
    assert ref.load([]) and m.status().tobytes() == ref.status().tobytes() and m.catalogue_words == 0
    ev = _both(pkg, m, ref, [w[100:120] for w in words], each=True)
    assert all((e["track"] == -1).all() and (e["errs"] == 0xFFFFFFFF).all() and (e["offset"] == 0).all() and e.size == 5 for e in ev)
    with pytest.raises(pkg.FmdError) as e:
        m.load([R.random_words(15, 1)])                                      # refused: nothing changes
    assert e.value.status == -1 and m.status().tobytes() == ref.status().tobytes()
    m.load(R.main_catalogue())
    assert ref.load(R.main_catalogue())
    _both(pkg, m, ref, [w[120:] for w in words], each=True)
    m.reset()
    ref.reset()
    assert m.status().tobytes() == ref.status().tobytes()
    m.close()


def test_argument_errors(pkg):
    import torch
    m, ref, words = _main(pkg)
    xd = _cuda(words)
    ev = torch.zeros((3, 64, 3), dtype=torch.int64, device="cuda")
    st = m.status()
    call = m.L.fmd_fpmatch_process_dev
    bad = [lambda: m._check(call(m.g, None, 140, None, 16, None, ev.data_ptr(), 64, None, None, None, None)),
           lambda: m._check(call(m.g, xd.data_ptr() + 2, 140, None, 16, None, ev.data_ptr(), 64, None, None, None, None)),
           lambda: m._check(call(m.g, xd.data_ptr(), 140, None, 16, None, None, 64, None, None, None, None)),
           lambda: m._check(call(m.g, xd.data_ptr(), 140, None, 16, None, ev.data_ptr() + 4, 64, None, None, None, None)),
           lambda: m._check(call(m.g, xd.data_ptr(), 140, None, -1, None, ev.data_ptr(), 64, None, None, None, None)),
           lambda: m._check(call(m.g, xd.data_ptr(), 15, None, 16, None, ev.data_ptr(), 64, None, None, None, None)),
           lambda: m._check(call(m.g, xd.data_ptr(), 1024, None, 257, None, ev.data_ptr(), 65, None, None, None, None)),
           lambda: m._check(call(m.g, xd.data_ptr(), 140, None, 16, None, ev.data_ptr(), 3, None, None, None, None)),
           lambda: m.reset(3), lambda: m.reset(-2),
           lambda: m.load_raw(R.random_words(40, 1), [0, 20, 10], 2), lambda: m.load_raw(R.random_words(40, 1), [1, 40], 1),
           lambda: m.load([R.random_words(16, k) for k in range(17)]), lambda: m.load([R.random_words((1 << 16) + 1, 2)])]
    for k, f in enumerate(bad):
        with pytest.raises(pkg.FmdError) as e:
            f()
        assert e.value.status == -1 and str(e.value), k
    for f in (lambda: m.process(xd[:2]), lambda: m.process(xd, active=torch.ones(2, dtype=torch.uint8, device="cuda")), lambda: m.process(xd.long()),
              lambda: m.process(xd, nwords=torch.zeros(3, dtype=torch.int64, device="cuda")), lambda: m.process(xd, events=torch.zeros((3, 35, 2), dtype=torch.int64, device="cuda")),
              lambda: m.process(xd, events=torch.zeros((3, 34, 3), dtype=torch.int64, device="cuda")), lambda: m.process(xd, flags=torch.zeros(3, device="cuda"))):
        with pytest.raises(ValueError):
            f()
    base = {k: v for k, v in R.MAIN.items() if k != "n_channels"}
    for kw in (dict(n_bits=0), dict(n_bits=33), dict(block=24), dict(block=1040), dict(interval=0), dict(interval=1025), dict(max_errs=-1), dict(max_errs=513),
               dict(hold=0), dict(max_words=0), dict(max_words=65537), dict(max_tracks=0), dict(max_catalogue_words=15), dict(max_catalogue_words=(1 << 28) + 1)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.FingerprintMatcher(3, **{**base, **kw})
        assert e.value.status == -1 and str(e.value), kw
    with pytest.raises(pkg.FmdError):
        pkg.FingerprintMatcher(0)
    with pytest.raises(AttributeError):
        m.reset_peaks()
    assert m.status().tobytes() == st.tobytes()
    _both(pkg, m, ref, words)                                                # and nothing of the object changed
    m.close()


def test_cpp_adaptor(pkg, tmp_path):
    """tests/cpp/fpmatch_main.cpp takes a file of words in calls of 9 through FingerprintMatcher_GPU; the events its host views give and
    the records it prints are the restatement's, and it exits with 7 unless the device's views, bytes and records are the host's"""
    exe = tmp_path / "fpmatch_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}", f"-I{ROOT / 'fm-radio_amd' / 'host'}",
                    "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "fpmatch_main.cpp"), f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64",
                    f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    tracks = R.main_catalogue()
    words = [s[:140] for s in R.main_streams(tracks)[:2]]
    np.ascontiguousarray(np.stack(words)).tofile(tmp_path / "words.u32")
    np.concatenate(tracks).tofile(tmp_path / "cat.u32")
    starts = np.concatenate([[0], np.cumsum([t.size for t in tracks])])
    r = subprocess.run([str(exe), str(tmp_path / "words.u32"), "2", "32", "16", "4", "2", "9", str(tmp_path / "cat.u32"), str(tmp_path / "out")] + [str(s) for s in starts],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2
    ref = R.Matcher(**dict(R.MAIN, n_channels=2, max_words=9, max_tracks=4, max_catalogue_words=int(starts[-1])))
    assert ref.load(tracks)
    ev = [[], []]
    for a in range(0, 140, 9):
        for c, e in enumerate(ref.process([w[a:a + 9] for w in words], n=min(9, 140 - a))[0]):
            ev[c].append(e)
    for c, line in enumerate(lines):
        assert bytes.fromhex(line.split()[0]) == ref.status()[c].tobytes(), c
        assert int(line.split()[1]) == int(ref.status()[c]["flags"]) & 1
        assert (tmp_path / f"out.{c}.ev").read_bytes() == np.concatenate(ev[c]).tobytes(), c


def _fm(audio32: np.ndarray, level: float) -> np.ndarray:
    """mono FM at 256 kSa/s of audio at 32 kHz (band-limited interpolation by 8, 75 kHz deviation at |m| = 0.5), [n, 2] float32"""
    n = audio32.size
    up = np.fft.irfft(np.fft.rfft(audio32), 8 * n) * 8.0
    ph = 2.0 * np.pi * 75000.0 * np.cumsum(np.clip(up / 0.5, -1.0, 1.0)) / 256000.0
    iq = level * 100.0 * np.exp(1j * ph)
    return np.stack([iq.real, iq.imag], axis=1).astype(np.float32)


def test_demodulator_end_to_end(pkg):
    """Three stations at 256 kSa/s through BatchDemod in the tolerance mode, 24 blocks of 16384 samples, the Fingerprinter at the default
    geometry on audio_tensor() after each block, and its device outputs (words and counts) straight into the matcher at W = 64, I = 16.
    The catalogue is the float64 fingerprints of two source programmes; stations 0 and 1 carry programme 0 at carrier levels 1 and 0.3,
    station 2 a programme the catalogue does not hold.  Bit for bit the restatement on the same words; stations 0 and 1 end identified
    with track 0 at offsets that advance by I from query to query and errs / (W * 32) < 0.15; station 2 never hits and every errs /
    (W * 32) > 0.40.  The two bars carry the fingerprinter's own measured margins (BER 0.004 on the matching path, 0.496 on the other,
    against the threshold 0.35)."""
    import torch
    import fprint_ref
    fs, bs, nb = 256_000, 16384, 24
    n32 = bs * nb // 8
    src = [fprint_ref.programme(32000, n32, s)[:, 0].astype(np.float64) for s in (61, 63, 62)]
    fcfg = fprint_ref.config(**fprint_ref.DEFAULT_32K)
    tracks = [fprint_ref.model_words(fcfg, np.stack([s, s], axis=1).astype(np.float32)) for s in src[:2]]
    x = torch.from_numpy(np.stack([_fm(src[0], 1.0), _fm(src[0], 0.3), _fm(src[2], 1.0)])).cuda()
    dm = pkg.BatchDemod(3, bs, fs, fast_math=True)
    fp = pkg.Fingerprinter(3, 32000, max_input_frames=bs // 8)
    cfg = dict(n_channels=3, block=64, interval=16, max_words=pkg.fprint_max_prints(fp.hop, bs // 8), max_tracks=2, max_catalogue_words=sum(t.size for t in tracks))
    m, ref = _pair(pkg, cfg, tracks)
    assert m.max_errs == (35 * 64 * 32) // 100
    events = [[] for _ in range(3)]
    for b in range(nb):
        dm.process(x[:, b * bs:(b + 1) * bs].contiguous())
        dm.synchronize()
        out, cnt = fp.process(dm.audio_tensor())
        got = m.process(out, nwords=cnt)                                     # the fingerprinter's device outputs as they are
        k = cnt.cpu().numpy()
        want = ref.process(list(out.cpu().numpy().view(np.uint32)), nwords=list(k), n=out.shape[1])
        _same_call(pkg, got, want, b)
        for r, e in zip(events, want[0]):
            r.append(e)
    st = m.status()
    assert st.tobytes() == ref.status().tobytes() and (st["words"] == 101).all() and (st["queries"] == 3).all() and (st["clamped"] == 0).all()
    ev = [np.concatenate(r) for r in events]
    rate = [e["errs"] / (64.0 * 32.0) for e in ev]
    print("errs / (W * 32) per query:", [r.round(4).tolist() for r in rate], "offsets:", [e["offset"].tolist() for e in ev])
    for c in (0, 1):
        assert st[c]["track"] == 0 and st[c]["flags"] == 3 and (ev[c]["track"] == 0).all() and (ev[c]["flags"] == 1).all() and (rate[c] < 0.15).all(), (c, rate[c])
        assert np.diff(ev[c]["offset"]).tolist() == [16, 16] and st[c]["since"] == 64 and st[c]["hits"] == 3
    assert st[2]["track"] == -1 and st[2]["hits"] == 0 and (ev[2]["flags"] == 0).all() and (rate[2] > 0.40).all(), rate[2]
    dm.close(); fp.close(); m.close()
