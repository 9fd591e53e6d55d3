"""Indexed fingerprint matcher on the GPU (fmd_fpmatch_create_ex, FingerprintMatcher(index=...): k_fpmatch_probe and
k_fpmatch_finish_idx behind the brute-force object's map and gather): events, counts, bytes, status records and index status records
against the numpy restatement of the definition (tests/fpmatch_index_ref.py, itself checked in test_fpmatch_index_cpu.py), bit for bit.
The main shape is test_gpu_fpmatch.py's: W = 16, I = 4, hold 2, three stations that have taken 0, 5 and 37 words before the calls under
test, tracks of 16, 17, 50 and 700 words.  Every test needs fmd_fpmatch_create_ex."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fpmatch_index_ref as X
import fpmatch_ref as R
from test_gpu_fpmatch import RAGGED, _cuda, _fm, _i32, _rowmap, _same_call

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
COMBOS = [(n_bits, K, d) for n_bits in (32, 9) for K in (8, 2) for d in (0, 2)]


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


def _pair(pkg, cfg, idx, tracks):
    """(the indexed object, the restatement) of cfg and idx (None: the default index) with `tracks` loaded"""
    m = pkg.FingerprintMatcher(cfg["n_channels"], index=True if idx is None else idx, **{k: v for k, v in cfg.items() if k != "n_channels"})
    ref = X.IndexedMatcher(index=idx, **cfg)
    assert m.cfg.max_errs == ref.cfg["max_errs"] and (m.index.max_bucket, m.index.follow) == (ref.idx["max_bucket"], ref.idx["follow"])
    if tracks is not None:
        m.load(tracks)
        assert ref.load(tracks)
    return m, ref


def _same_records(m, ref, what=""):
    assert m.status().tobytes() == ref.status().tobytes(), what
    assert m.index_status().tobytes() == ref.index_status().tobytes(), (what, m.index_status(), ref.index_status())


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
            _same_records(m, ref, (at, c))
        for r, e in zip(all_ev, want[0]):
            r.append(e)
        at = c
    _same_records(m, ref)
    return [np.concatenate(r) for r in all_ev]


def _main(pkg, n_bits=32, K=8, d=2, **over):
    """the main shape with every station's PRE words taken (one call with d_nwords = PRE): (object, restatement, the 140 words a station)"""
    tracks = R.main_catalogue(n_bits)
    streams = R.main_streams(tracks, n_bits)
    m, ref = _pair(pkg, dict(R.MAIN, n_bits=n_bits, **over), dict(max_bucket=K, follow=d), tracks)
    top = max(R.PRE)
    pre = [np.concatenate([s[:p], np.zeros(top - p, np.uint32)]) for s, p in zip(streams, R.PRE)]
    got = m.process(_cuda(pre), nwords=_i32(R.PRE))
    _same_call(pkg, got, ref.process(pre, nwords=list(R.PRE), n=top), "pre")
    _same_records(m, ref, "pre")
    return m, ref, [s[p:] for s, p in zip(streams, R.PRE)]


def _case(pkg, case, cuts=(), **kw):
    cfg, idx, tracks, words = case
    m, ref = _pair(pkg, cfg, idx, tracks)
    ev = _both(pkg, m, ref, words, cuts=cuts, **kw)
    return m, ref, ev


@pytest.mark.parametrize("n_bits,K,d", COMBOS)
def test_one_call(pkg, n_bits, K, d):
    """the whole stream in one call: 100 queries, so the follow rule runs across the queries of one call; hits, misses, skipped words at
    9 bits and K = 2, empty candidate sets at 32 bits"""
    m, ref, words = _main(pkg, n_bits, K, d)
    ev = _both(pkg, m, ref, words)
    ix = m.index_status()
    assert [e.size for e in ev] == [32, 33, 35] and all((e["flags"] == 1).any() and (e["flags"] == 0).any() for e in ev)
    assert (ix["followed"].sum() > 0) == (d > 0) and (ix["skipped"].sum() > 0) == (n_bits == 9 and K == 2) and (ix["empty"].sum() > 0) == (n_bits == 32)
    m.close()


@pytest.mark.parametrize("n_bits,K,d", [(32, 8, 2), (32, 2, 0), (9, 8, 0), (9, 2, 2)])
def test_a_call_per_word(pkg, n_bits, K, d):
    m, ref, words = _main(pkg, n_bits, K, d)
    one = _both(pkg, *_main(pkg, n_bits, K, d)[:2], words)
    ev = _both(pkg, m, ref, words, cuts=range(1, 140))
    assert [e.tobytes() for e in ev] == [e.tobytes() for e in one]
    m.close()


@pytest.mark.parametrize("n_bits,K,d", COMBOS)
def test_ragged_calls_on_alternating_streams(pkg, n_bits, K, d):
    """1 + 3 + 4 + 5 + 15 + 16 + 17 + the rest, every other call on another stream, the records checked after every call"""
    m, ref, words = _main(pkg, n_bits, K, d)
    _both(pkg, m, ref, words, cuts=list(np.cumsum(RAGGED)), each=True, alternate=True)
    m.close()


@pytest.mark.parametrize("ends", [True, False], ids=["ends_taken", "ends_left_out"])
@pytest.mark.parametrize("C", R.ROWMAP_STATIONS)
def test_row_map_of_many_stations(pkg, C, ends):
    """test_gpu_fpmatch.py's row map shapes through the indexed object (the default index: K = 8, d = 2): every station's outputs, record
    and index record, bit for bit"""
    m, ref = _pair(pkg, dict(R.MAIN, n_channels=C), None, None)
    _rowmap(pkg, m, ref, C, ends, _same_records)
    assert C == 1 or ref.index_status()["followed"].sum() > 0
    m.close()


def test_skip_rule(pkg):
    m, ref, ev = _case(pkg, X.skip_case(), cuts=[9, 22], each=True)
    assert (ev[0]["errs"] == 0xFFFFFFFF).all() and m.index_status()[0].tolist() == (0, 7 * 16, 0, 7) and (ev[1]["flags"] == 1).all()
    m.close()


@pytest.mark.parametrize("d", [2, 0])
def test_follow_rule_dropped_word_and_the_tracks_ends(pkg, d):
    """held at 20 % with d = 2 and released with d = 0; a dropped word; p_exp +- d off the track's end, above D - W and across two tracks"""
    m, ref, ev = _case(pkg, X.follow_case(d), cuts=[31, 50, 51, 90], each=True)
    assert m.status()["track"].tolist() == ([1, 1, -1, -1] if d else [-1] * 4)
    if d:
        assert sorted(np.diff(ev[1]["offset"]).tolist()) == [4] * 25 + [5] and m.index_status()["followed"].tolist() == [26, 26, 8, 13]
    m.close()
    one = _case(pkg, X.follow_case(d))                                       # and the whole of it in one call
    assert [e.tobytes() for e in one[2]] == [e.tobytes() for e in ev]
    one[0].close()


def test_follow_rule_below_zero(pkg):
    m, ref, ev = _case(pkg, X.below_zero_case(), cuts=[17])
    assert (ev[0]["flags"] == 1).all() and m.index_status()[0]["followed"] == 20
    m.close()


def test_the_splice(pkg):
    """station 1's stream alone: the windows across the splice of track 1's tail to track 2's head have exact words whose proposals are
    positions no track holds (they straddle the two tracks)"""
    tracks = R.main_catalogue()
    m, ref = _pair(pkg, dict(R.MAIN, n_channels=1), dict(max_bucket=8, follow=0), tracks)
    w = R.main_streams(tracks)[1][:60]
    ev = _both(pkg, m, ref, [w], cuts=[21, 22])[0]
    starts = np.cumsum([0] + [t.size for t in tracks])
    across = [i for i, e in enumerate(ev["end"]) if 5 + 14 - 16 < e - 16 < 5 + 14 and e - 16 >= 5]   # the window starts inside the tail and is not all of it
    assert len(across) >= 2
    for i in across:
        p = int(starts[1]) + 3 + (int(ev["end"][i]) - 16 - 5)                # where the catalogue holds exactly these words
        assert np.array_equal(ref.cat[p:p + 16], w[ev["end"][i] - 16:ev["end"][i]]) and p not in ref.last[i][1] and ev["errs"][i] > 0
    m.close()


def test_default_block_and_interval(pkg):
    """W = 256 / I = 64 (the default) on two stations: a programme at 5 % from its word 100, and unrelated words then another at 30 %"""
    tracks = [R.random_words(600, 301), R.random_words(300, 302)]
    cfg = dict(n_channels=2, max_words=400, max_tracks=2, max_catalogue_words=900)
    m, ref = _pair(pkg, cfg, None, tracks)
    assert (m.block, m.interval, m.index.max_bucket, m.index.follow, m.index_design.chunk_words) == (256, 64, 8, 2, 256)
    words = [R.flip(tracks[0][100:500], 0.05, 303), np.concatenate([R.random_words(100, 304), R.flip(tracks[1], 0.30, 305)])]
    ev = _both(pkg, m, ref, words, cuts=[6, 11, 70, 200, 256, 257], each=True)
    assert ev[0]["offset"].tolist() == [100, 164, 228] and ev[0]["track"].tolist() == [0, 0, 0] and ev[1]["flags"].tolist() == [0, 0, 0]
    assert m.index_status()["empty"].tolist() == [0, 3]                     # at 30 % no word of 256 is exact: the prefilter misses what brute force finds
    m.close()


@pytest.mark.parametrize("copies", [64, 65])
def test_the_candidate_list_at_its_capacity(pkg, copies):
    """W = 1024 at K = 64 against 64 copies of one track: every window word's run is exactly K long, 16 chunks of 64 words fill the list
    to its 4096 entries with 65 536 proposals of 64 distinct positions, and the lowest copy wins; at 65 copies every word is skipped"""
    cfg, idx, tracks, words = X.capacity_case(copies)
    m, ref = _pair(pkg, cfg, idx, tracks)
    d = m.index_design
    assert d.chunk_words == 64 and d.chunk_words * 64 == d.chunk == 4096
    ev = _both(pkg, m, ref, words)[0]
    want = [(0, 0, 0, 1)] if copies == 64 else [(-1, 0, 0xFFFFFFFF, 0)]
    assert [(e["track"], e["offset"], e["errs"], e["flags"]) for e in ev] == want
    assert m.index_status()[0].tolist() == ((65536, 0, 0, 0) if copies == 64 else (0, 1024, 0, 1))
    m.close()


@pytest.mark.parametrize("kind", ["one", "ends"])
def test_directory_slices(pkg, kind):
    """a catalogue whose keys all lie in one directory slice (one binary search over the whole index) and one whose keys lie in the
    first and the last slice only"""
    cfg, idx, tracks, words = X.slice_case(kind)
    m, ref = _pair(pkg, cfg, idx, tracks)
    keys, pos, dirs = pkg.fpmatch_index_build(m.cfg, m.index, np.concatenate(tracks))
    filled = np.flatnonzero(np.diff(dirs))
    assert m.index_design.dir_bits == 8 and filled.tolist() == ([0x42] if kind == "one" else [0, 255])
    ev = _both(pkg, m, ref, words, cuts=[33])
    assert (ev[0]["flags"] == 1).all() and (ev[1]["flags"] == 1).all() and (ev[0]["track"] == 0).all() and (ev[1]["track"] == 2).all()
    m.close()


@pytest.mark.parametrize("extremes", [True, False])
def test_bucket_sizes_and_edge_keys(pkg, extremes):
    """keys 0 and 0xffffffff, a key in an empty slice, a key above every catalogue key, runs of exactly K and of K + 1"""
    m, ref, ev = _case(pkg, X.bucket_case(extremes), cuts=[30])
    ix = m.index_status()
    assert ix[1]["skipped"] > 0 and ix[1]["empty"] > 0 and ix[1]["candidates"] % 3 == 0 and (ix[2]["empty"] == 13) == (not extremes)
    m.close()


def test_a_duplicated_track(pkg):
    tracks = R.tiled_catalogue(1024, 16)
    m, ref = _pair(pkg, dict(R.MAIN, n_channels=1, max_catalogue_words=1 << 14), None, tracks)
    ev = _both(pkg, m, ref, [tracks[1][4:44]], cuts=[13])[0]
    assert (ev["track"] == 1).all() and (ev["errs"] == 0).all() and all(k == 2 for _, _, k in ref.ties)
    m.close()


def test_n_zero_and_a_batch_of_one(pkg):
    tracks = R.main_catalogue()
    streams = R.main_streams(tracks)
    m, ref = _pair(pkg, dict(R.MAIN, n_channels=1), None, tracks)
    ev = _both(pkg, m, ref, [streams[0]], cuts=[0, 30, 30, 77], each=True)  # n = 0 at the start and in mid-stream: the bytes are written
    m3, ref3, words = _main(pkg)
    one = _both(pkg, m3, ref3, words)
    assert ev[0].tobytes() == one[0].tobytes()
    m.close(); m3.close()


def test_row_69_of_70(pkg):
    """70 stations, station c with stream c mod 3 and its PRE words: every row gives what its stream gives in a batch of three"""
    tracks = R.main_catalogue()
    streams = R.main_streams(tracks)
    m3, ref3, words = _main(pkg)
    want = _both(pkg, m3, ref3, words)
    m = pkg.FingerprintMatcher(70, index=True, **{k: v for k, v in R.MAIN.items() if k != "n_channels"})
    m.load(tracks)
    top = max(R.PRE)
    pre = [np.concatenate([streams[c % 3][:R.PRE[c % 3]], np.zeros(top - R.PRE[c % 3], np.uint32)]) for c in range(70)]
    m.process(_cuda(pre), nwords=_i32([R.PRE[c % 3] for c in range(70)]))
    ev, cnt, fl, ok = m.process(_cuda([words[c % 3] for c in range(70)]))
    k, st, ix = cnt.cpu().numpy(), m.status(), m.index_status()
    for c in range(70):
        assert pkg.FingerprintMatcher.events_of(ev, k, c).tobytes() == want[c % 3].tobytes(), c
        assert st[c].tobytes() == ref3.status()[c % 3].tobytes() and ix[c].tobytes() == ref3.index_status()[c % 3].tobytes(), c
        assert int(fl[c]) == int(st[c]["flags"]) and int(ok[c]) == int(st[c]["flags"]) & 1, c
    m.close(); m3.close()


def test_active_mask_over_prefilled_outputs(pkg):
    """a station whose byte is 0 keeps its ring, records, events, count and bytes; an active station's slots behind its events are left alone"""
    import torch
    m, ref, words = _main(pkg)
    xd = _cuda(words)
    rows = pkg.fpmatch_max_events(4, 41) + 2
    ev = torch.full((3, rows, 3), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    cnt = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    fl, ok = torch.full((3,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((3,), 0xDD, dtype=torch.uint8, device="cuda")
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    before, ibefore = m.status(), m.index_status()
    got = m.process(xd[:, :41], active=active, events=ev, nevents=cnt, flags=fl, ok=ok)
    _same_call(pkg, got, ref.process([w[:41] for w in words], n=41, active=[1, 0, 1]))
    raw, k = ev.cpu().numpy(), cnt.cpu().numpy()
    assert k[1] == -7 and int(fl[1]) == 0xEE and int(ok[1]) == 0xDD and (raw[1] == 0x5A5A5A5A5A5A5A5A).all()
    assert m.status()[1].tobytes() == before[1].tobytes() and m.index_status()[1].tobytes() == ibefore[1].tobytes()
    for c in (0, 2):
        assert 0 < k[c] < rows and (raw[c, k[c]:] == 0x5A5A5A5A5A5A5A5A).all()
    got = m.process(xd[:, :41], active=active.logical_not())
    _same_call(pkg, got, ref.process([w[:41] for w in words], n=41, active=[0, 1, 0]))
    _both(pkg, m, ref, [w[41:] for w in words])
    m.close()


def test_nwords_null_and_clamped_and_null_outputs(pkg):
    """d_nwords NULL takes n of every station; counts of -3 and n + 5 are clamped into [0, n] and counted; NULL counts and bytes"""
    m, ref, words = _main(pkg)
    xd = _cuda(words)
    got = m.process(xd[:, :20], nwords=_i32([-3, 25, 7]))
    _same_call(pkg, got, ref.process([w[:20] for w in words], nwords=[-3, 25, 7], n=20))
    _same_records(m, ref)
    assert m.status()["clamped"].tolist() == [1, 1, 0]
    ev, cnt, fl, ok = m.process(xd[:, 20:70], nevents=False, flags=False, ok=False)
    want = ref.process([w[20:70] for w in words], n=50)
    assert cnt is None and fl is None and ok is None
    for c in range(3):
        assert pkg.FingerprintMatcher.events_of(ev, None, c)[:want[0][c].size].tobytes() == want[0][c].tobytes()
    _same_records(m, ref)
    m.close()


def test_load_and_reset_in_mid_stream(pkg):
    """load to another catalogue and to an empty one, a refused load, and the reset of one station, in mid-stream: the index is rebuilt,
    the index records are kept by a load and cleared by the reset"""
    m, ref, words = _main(pkg)
    _both(pkg, m, ref, [w[:50] for w in words], each=True)
    other = [R.main_catalogue()[i] for i in (3, 0, 2)]
    m.load(other)
    assert ref.load(other)
    _same_records(m, ref)
    _both(pkg, m, ref, [w[50:62] for w in words], cuts=[2], each=True)
    m.reset(1)
    ref.reset(1)
    _same_records(m, ref)
    assert m.index_status()[1].tolist() == (0, 0, 0, 0) and m.index_status()[0]["candidates"] > 0
    _both(pkg, m, ref, [w[62:100] for w in words], cuts=[7], each=True)
    with pytest.raises(pkg.FmdError) as e:
        m.load([R.random_words(15, 1)])                                      # refused: the old catalogue and its index stay
    assert e.value.status == -1
    _both(pkg, m, ref, [w[100:108] for w in words], each=True)
    m.load([])
    assert ref.load([])
    ev = _both(pkg, m, ref, [w[108:120] for w in words], each=True)
    assert all((e["track"] == -1).all() and (e["errs"] == 0xFFFFFFFF).all() and e.size == 3 for e in ev)
    m.load(R.main_catalogue())
    assert ref.load(R.main_catalogue())
    _both(pkg, m, ref, [w[120:] for w in words], each=True)
    m.reset()
    ref.reset()
    _same_records(m, ref)
    m.close()


def test_errors(pkg):
    """get_index_status on a brute-force object is FMD_ERR_STATE; refused index configurations; nothing of the object changes"""
    brute = pkg.FingerprintMatcher(3, **{k: v for k, v in R.MAIN.items() if k != "n_channels"})
    with pytest.raises(pkg.FmdError) as e:
        brute.index_status()
    assert e.value.status == -6 and "index" in str(e.value) and brute.index is None and brute.state_bytes == pkg.fpmatch_state_bytes(brute.cfg)
    brute.close()
    base = {k: v for k, v in R.MAIN.items() if k != "n_channels"}
    for idx in (dict(max_bucket=0), dict(max_bucket=65), dict(follow=-1), dict(follow=9)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.FingerprintMatcher(3, index=idx, **base)
        assert e.value.status == -1 and str(e.value), idx
    with pytest.raises(pkg.FmdError):
        pkg.FingerprintMatcher(3, index=True, **{**base, "block": 24})
    with pytest.raises(TypeError):
        pkg.FingerprintMatcher(3, index=dict(bucket=1), **base)
    m, ref, words = _main(pkg)
    assert m.state_bytes == pkg.fpmatch_index_state_bytes(m.cfg, m.index) == X.index_state_bytes(ref.cfg, ref.idx)
    assert m.L.fmd_fpmatch_get_index_status(m.g, None) == -1 and m.L.fmd_fpmatch_get_index_status(None, None) == -1
    with pytest.raises(pkg.FmdError):
        m.process(_cuda(words)[:, :4], n=257)
    with pytest.raises(pkg.FmdError):
        m.reset(3)
    _both(pkg, m, ref, words)
    m.close()


def test_cpp_adaptor(pkg, tmp_path):
    """tests/cpp/fpmatch_index_adaptor_main.cpp takes a file of words in calls of 9 through FingerprintMatcher_GPU(cfg, idx); the events
    its host views give and the two records it prints per station are the restatement's"""
    exe = tmp_path / "fpmatch_index_adaptor_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}", f"-I{ROOT / 'fm-radio_amd' / 'host'}",
                    "-I/opt/rocm/include", str(ROOT / "tests" / "cpp" / "fpmatch_index_adaptor_main.cpp"), f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64",
                    f"-Wl,-rpath,{csrc}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    tracks = R.main_catalogue()
    words = [s[:140] for s in R.main_streams(tracks)[:2]]
    np.ascontiguousarray(np.stack(words)).tofile(tmp_path / "words.u32")
    np.concatenate(tracks).tofile(tmp_path / "cat.u32")
    starts = np.concatenate([[0], np.cumsum([t.size for t in tracks])])
    r = subprocess.run([str(exe), str(tmp_path / "words.u32"), "2", "32", "16", "4", "2", "9", "8", "2", str(tmp_path / "cat.u32"), str(tmp_path / "out")] +
                       [str(s) for s in starts], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2
    ref = X.IndexedMatcher(**dict(R.MAIN, n_channels=2, max_words=9, max_tracks=4, max_catalogue_words=int(starts[-1])))
    assert ref.load(tracks)
    ev = [[], []]
    for a in range(0, 140, 9):
        for c, e in enumerate(ref.process([w[a:a + 9] for w in words], n=min(9, 140 - a))[0]):
            ev[c].append(e)
    for c, line in enumerate(lines):
        assert bytes.fromhex(line.split()[0]) == ref.status()[c].tobytes() and bytes.fromhex(line.split()[1]) == ref.index_status()[c].tobytes(), c
        assert (tmp_path / f"out.{c}.ev").read_bytes() == np.concatenate(ev[c]).tobytes(), c


@pytest.mark.parametrize("n_bits", [32, 9])
def test_beside_a_brute_force_object(pkg, n_bits):
    """the same streams through a brute-force object: at 32 bits every indexed hit's event is the brute-force object's; at both widths
    the indexed errs is never below it"""
    m, ref, words = _main(pkg, n_bits)
    tracks = R.main_catalogue(n_bits)
    b = pkg.FingerprintMatcher(3, **{k: v for k, v in dict(R.MAIN, n_bits=n_bits).items() if k != "n_channels"})
    b.load(tracks)
    streams = R.main_streams(tracks, n_bits)
    top = max(R.PRE)
    b.process(_cuda([np.concatenate([s[:p], np.zeros(top - p, np.uint32)]) for s, p in zip(streams, R.PRE)]), nwords=_i32(R.PRE))
    xd = _cuda(words)
    (ei, ci, _, _), (eb, cb, _, _) = m.process(xd), b.process(xd)
    hits = 0
    for c in range(3):
        gi, gb = pkg.FingerprintMatcher.events_of(ei, ci.cpu().numpy(), c), pkg.FingerprintMatcher.events_of(eb, cb.cpu().numpy(), c)
        assert gi.size == gb.size and (gi["errs"] >= gb["errs"]).all()
        for x, y in zip(gi, gb):
            if x["flags"] == 1:
                hits += 1
                assert n_bits != 32 or x.tobytes() == y.tobytes(), (c, x, y)
    assert hits > 30
    m.close(); b.close()


def test_demodulator_end_to_end(pkg):
    """test_gpu_fpmatch.py's end-to-end chain (three stations at 256 kSa/s through BatchDemod in the tolerance mode, the Fingerprinter,
    and its device outputs straight into the matcher at W = 64, I = 16) into an indexed and a brute-force matcher side by side.  Bit for
    bit the restatement; stations 0 and 1 end identified by both with the same track and offsets (their measured bit error rate of
    0.003 - 0.005 leaves about 85 % of the words exact); station 2 is never a hit in either."""
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
    m, ref = _pair(pkg, cfg, None, tracks)
    b = pkg.FingerprintMatcher(3, **{k: v for k, v in cfg.items() if k != "n_channels"})
    b.load(tracks)
    events, brute = [[] for _ in range(3)], [[] for _ in range(3)]
    for blk in range(nb):
        dm.process(x[:, blk * bs:(blk + 1) * bs].contiguous())
        dm.synchronize()
        out, cnt = fp.process(dm.audio_tensor())
        got = m.process(out, nwords=cnt)
        eb, cb, _, _ = b.process(out, nwords=cnt)
        k = cnt.cpu().numpy()
        want = ref.process(list(out.cpu().numpy().view(np.uint32)), nwords=list(k), n=out.shape[1])
        _same_call(pkg, got, want, blk)
        for c in range(3):
            events[c].append(want[0][c])
            brute[c].append(pkg.FingerprintMatcher.events_of(eb, cb.cpu().numpy(), c).copy())
    _same_records(m, ref)
    st, sb, ix = m.status(), b.status(), m.index_status()
    ev, bv = [np.concatenate(r) for r in events], [np.concatenate(r) for r in brute]
    print("index records:", ix.tolist(), "errs:", [e["errs"].tolist() for e in ev], "brute errs:", [e["errs"].tolist() for e in bv])
    for c in (0, 1):
        assert st[c]["track"] == 0 == sb[c]["track"] and st[c]["flags"] == 3 == sb[c]["flags"] and ev[c].tobytes() == bv[c].tobytes(), c
        assert (ev[c]["flags"] == 1).all() and np.diff(ev[c]["offset"]).tolist() == [16, 16] and st[c]["hits"] == 3 == sb[c]["hits"]
    assert st[2]["track"] == -1 == sb[2]["track"] and st[2]["hits"] == 0 == sb[2]["hits"] and (ev[2]["flags"] == 0).all() and (bv[2]["flags"] == 0).all()
    dm.close(); fp.close(); m.close(); b.close()
