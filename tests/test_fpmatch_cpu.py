"""Fingerprint matcher without a GPU (fmd_fpmatch_*, include/fmdemod.h "Fingerprint matcher"): the numpy restatement of the definition
(tests/fpmatch_ref.py) against the existing capi.fprint_match / fprint_ber, its split invariance, position validity, the tie rule, the
detector, `clamped`, the empty catalogue, the uniqueness of every minimum of the streams the GPU tests use, the library's host-only
functions against the restatement, dtype sizes, and the host-only unit as a stand-alone program under sanitizers.  Everything is an
integer: every comparison is equality."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fpmatch_ref as R

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["fmd_fpmatch_default_config", "fmd_fpmatch_max_events", "fmd_fpmatch_max_errs", "fmd_fpmatch_design", "fmd_fpmatch_check_catalogue", "fmd_fpmatch_state_bytes",
           "fmd_fpmatch_create", "fmd_fpmatch_destroy", "fmd_fpmatch_reset", "fmd_fpmatch_load", "fmd_fpmatch_process_dev", "fmd_fpmatch_get_status",
           "fmd_fpmatch_status_dev", "fmd_fpmatch_last_error"]
SMALL = dict(block=16, interval=4, hold=2, max_words=1024, max_tracks=16, max_catalogue_words=1 << 16)


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.build_library()
    return p


def _feed(m, streams, cuts, n_total):
    """feeds every station's stream in the pieces that end at `cuts` and at n_total; per station all events"""
    ev, at = [[] for _ in streams], 0
    for c in list(cuts) + [n_total]:
        e, _, _ = m.process([s[at:c] for s in streams], n=c - at)
        for i, r in enumerate(e):
            ev[i].append(r)
        at = c
    return [np.concatenate(r) for r in ev]


def test_symbols_are_declared_and_exported(pkg):
    declared = pkg.declared_symbols(debug=False)
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/fmdemod.h"
        assert hasattr(lib, s), f"{s} is not exported"
    assert lib.fmd_api_version() == 3
    for name in ("FingerprintMatcher", "FpmatchConfig", "FPMATCH_STATUS_DTYPE", "FPMATCH_EVENT_DTYPE", "fpmatch_default_config", "fpmatch_max_events",
                 "fpmatch_max_errs", "fpmatch_state_bytes", "fpmatch_design", "fpmatch_check_catalogue"):
        assert hasattr(pkg, name)
    assert pkg.FPMATCH_STATUS_DTYPE == R.STATUS_DTYPE and pkg.FPMATCH_STATUS_DTYPE.itemsize == 64
    assert pkg.FPMATCH_EVENT_DTYPE == R.EVENT_DTYPE and pkg.FPMATCH_EVENT_DTYPE.itemsize == 24
    assert C.sizeof(pkg.FpmatchConfig) == 48 and C.sizeof(pkg.FpmatchDesign) == 40
    assert tuple(n for n, _ in pkg.FpmatchConfig._fields_) == R.CONFIG_FIELDS


@pytest.mark.parametrize("n_bits", [32, 9, 1])
def test_restatement_against_fprint_match(pkg, n_bits):
    """a one-track catalogue and W = len(query): the restatement's offset and error count are fprint_match's, and fprint_ber's at that
    alignment, for a noisy excerpt and for unrelated words"""
    ref = R.random_words(300, 11)
    for q in (R.flip(ref[77:77 + 64], 0.1, 12), R.random_words(64, 13), ref[236:300]):
        m = R.Matcher(n_channels=1, n_bits=n_bits, block=64, interval=64, max_errs=0, max_words=64)
        assert m.load([ref])
        ev, _, _ = m.process([q])
        assert ev[0].size == 1 and ev[0]["end"][0] == 64 and ev[0]["track"][0] == 0
        at, rate = pkg.fprint_match(q, ref, n_bits=n_bits)
        assert ev[0]["offset"][0] == at
        assert ev[0]["errs"][0] == round(rate * 64 * n_bits) == round(pkg.fprint_ber(q, ref[at:at + 64], n_bits=n_bits) * 64 * n_bits)
        assert np.array_equal(m.errs(q), [round(pkg.fprint_ber(q, ref[p:p + 64], n_bits=n_bits) * 64 * n_bits) for p in range(300 - 63)])


@pytest.fixture(scope="module", params=[32, 9])
def main(request):
    tracks = R.main_catalogue(request.param)
    streams = R.main_streams(tracks, request.param)
    m = R.Matcher(**dict(R.MAIN, n_bits=request.param))
    assert m.load(tracks)
    n = streams[0].size - R.PRE[0]
    m.process([s[:max(R.PRE)] for s in streams], nwords=list(R.PRE), n=max(R.PRE))
    ev = _feed(m, [s[p:] for s, p in zip(streams, R.PRE)], [], n)
    return tracks, streams, n, ev, m.status(), m.ties


def test_the_shared_streams_are_what_the_gpu_tests_need(main):
    """every query's minimum is unique but for the intended duplicate (track 0 played twice gives no tie: it is one track), every station
    fires many queries in three phases, and the streams hit, miss, switch, release and run off a track's end"""
    tracks, streams, n, ev, st, ties = main
    assert all(k == 1 for _, _, k in ties), [t for t in ties if t[2] != 1]
    assert [int(e["end"][0]) % 4 for e in ev] == [0, 0, 0] and [int(e["end"][0]) for e in ev] == [16, 16, 40]
    assert all(e.size > 2 * 8 for e in ev) and n > 128
    hits0 = ev[0][ev[0]["flags"] == 1]
    assert set(hits0["track"]) == {3, 2} and (st["hits"] > 0).all() and (st["queries"] > st["hits"]).all()
    # station 0 plays track 2 to its end and on into unrelated words: the last hit lies at the track's last position, then it is released
    last = hits0[hits0["track"] == 2][-1]
    assert last["offset"] + 16 <= 50 and st["track"][0] == -1
    # station 1's splice: the windows across tracks 1 | 2 match no valid position exactly
    across = ev[1][(ev[1]["end"] > 5 + 16) & (ev[1]["end"] < 5 + 14 + 16)]
    assert across.size >= 2 and (across["errs"] > 0).any()
    assert 0 in set(ev[1][ev[1]["flags"] == 1]["track"]) and (ev[1]["errs"][ev[1]["track"] == 3] > 0).any()


@pytest.mark.parametrize("n_bits", [32, 9])
def test_restatement_split_invariance(n_bits):
    """one call, word by word, ragged calls: the same events and records"""
    tracks = R.main_catalogue(n_bits)
    streams = R.main_streams(tracks, n_bits)
    cfg = dict(R.MAIN, n_bits=n_bits)
    n = streams[0].size
    streams = [s[:n] for s in streams]
    want = None
    for cuts in ([], range(1, n), list(np.cumsum([1, 3, 4, 5, 15, 16, 17]))):
        m = R.Matcher(**cfg)
        assert m.load(tracks)
        ev = _feed(m, streams, cuts, n)
        got = ([e.tobytes() for e in ev], m.status().tobytes())
        want = want or got
        assert got == want
    assert m.status()["queries"].tolist() == [(n - 16) // 4 + 1] * 3


def test_positions_validity_and_ties():
    """a window straddling two adjacent tracks is never reported although its errs would be 0; a track of exactly W words has one
    position; a duplicated track ties to the lower position"""
    a, b = R.random_words(16, 1), R.random_words(20, 2)
    m = R.Matcher(n_channels=1, **SMALL)
    assert m.load([a, b, a])
    assert m.valid.tolist() == [True] + [False] * 15 + [True] * 5 + [False] * 15 + [True]
    q = np.concatenate([a[8:], b[:8]])                                       # position 8 holds exactly these words
    assert m.errs(q)[8] == 0
    t, off, errs, _ = m.search(q)
    assert errs > 0 and (t, off) != (0, 8)
    assert m.search(a) == (0, 0, 0, 2)                                       # tracks 0 and 2 tie: the lower position
    assert m.search(b[4:]) == (1, 4, 0, 1)
    m2 = R.Matcher(n_channels=1, **SMALL)
    assert m2.load([b, a]) and m2.search(a) == (1, 0, 0, 1) and np.count_nonzero(m2.valid[20:]) == 1


def test_detector():
    """identify, switch, release after exactly `hold` misses and not before, the end of a track, load clears the detector and keeps the ring"""
    tracks = [R.random_words(40, 21), R.random_words(40, 22)]
    m = R.Matcher(n_channels=1, **dict(SMALL, hold=3))
    assert m.load(tracks)
    junk = R.random_words(64, 23)
    step = lambda w: (m.process([w], n=len(w)), m.status()[0])[1]
    s = step(tracks[0][:16])
    assert (s["track"], s["since"], s["offset"], s["misses"], s["flags"], s["hits"], s["queries"]) == (0, 16, 0, 0, 3, 1, 1)
    s = step(tracks[0][16:24])
    assert (s["track"], s["since"], s["offset"], s["hits"]) == (0, 16, 8, 3)
    s = step(tracks[1][4:20])                                                # the switch: at e = 36 twelve of the window's words are track 1's (64 errs at most from the other four)
    assert (s["track"], s["since"], s["offset"]) == (1, 36, 4) and s["queries"] == 7
    s = step(tracks[1][20:40])                                               # to the track's end: the last valid position
    assert (s["track"], s["offset"], s["misses"]) == (1, 24, 0)
    s = step(junk[:8])                                                       # off the end: two misses hold
    assert (s["track"], s["misses"], s["flags"]) == (1, 2, 1)
    s = step(junk[8:12])                                                     # the third releases
    assert (s["track"], s["misses"], s["flags"], s["since"]) == (-1, 0, 0, 36)
    s = step(junk[12:16])
    assert (s["track"], s["misses"]) == (-1, 0)
    # load in mid-stream: the detector is cleared, the ring and the counters stay, and the next query finds the new catalogue at once
    s = step(tracks[0][:16])
    before = m.status()[0]
    assert before["track"] == 0
    assert m.load([tracks[1], tracks[0]])
    s = m.status()[0]
    assert (s["track"], s["misses"], s["flags"]) == (-1, 0, 2) and s["words"] == before["words"] and s["hits"] == before["hits"] and s["fill"] == 16
    s = step(tracks[0][16:20])
    assert (s["track"], s["offset"], s["since"]) == (1, 4, before["words"] + 4)
    # a refused catalogue changes nothing
    assert not m.load([tracks[0][:15]]) and not m.load_raw(tracks[0], [0, 20, 10], 2) and m.status()[0].tobytes() == s.tobytes() and m.cat.size == 80


def test_clamped_empty_catalogue_and_reset():
    m = R.Matcher(n_channels=3, **SMALL)
    w = [R.random_words(32, 31 + c) for c in range(3)]
    ev, flags, ok = m.process(w, nwords=[-3, 37, 20], n=32)
    st = m.status()
    assert st["words"].tolist() == [0, 32, 20] and st["clamped"].tolist() == [1, 1, 0] and st["fill"].tolist() == [0, 16, 16]
    # an empty catalogue: every query reports track -1, offset 0, errs 0xffffffff and is a miss
    assert [e.size for e in ev] == [0, 5, 2] and all((e["track"] == -1).all() and (e["offset"] == 0).all() and (e["errs"] == 0xFFFFFFFF).all() and (e["flags"] == 0).all() for e in ev)
    assert flags == [0, 0, 0] and ok == [0, 0, 0] and st["errs"].tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFF] and st["queries"].tolist() == [0, 5, 2]
    assert m.load([w[1]])
    ev, flags, ok = m.process(w, n=0)
    assert [e.size for e in ev] == [0, 0, 0] and flags == [0, 0, 0]
    ev, flags, ok = m.process([w[1][16:20]] * 3, n=4, active=[1, 0, 1])
    assert ev[1] is None and flags == [0, None, 3] and ok == [0, None, 1] and ev[2]["track"].tolist() == [0] and ev[2]["offset"].tolist() == [4] and ev[0].size == 0
    m.reset(2)
    st = m.status()
    assert st[2].tobytes() == np.array([(0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0)], R.STATUS_DTYPE).tobytes() and st["words"][1] == 32
    assert m.load([])
    assert m.process([w[0][:16]] * 3, n=16)[0][2]["errs"].tolist() == [0xFFFFFFFF]


def _lib_config(pkg, cfg):
    return pkg.FpmatchConfig(**cfg)


def test_library_host_functions_equal_the_restatement(pkg):
    """the default configuration, max_events and max_errs from both sides of every bound, every refused configuration and every refused
    catalogue: the library's answers are the restatement's"""
    L = pkg.load_library()
    d = pkg.fpmatch_default_config()
    assert {k: getattr(d, k) for k in R.CONFIG_FIELDS} == R.default_config()
    assert d.max_errs == int(0.35 * 256 * 32) == 2867
    assert pkg.fpmatch_default_config(block=64, n_bits=9).max_errs == R.max_errs(35, 64, 9) == 201
    for interval, n in ((1, 0), (1, 1), (64, 0), (64, 1), (64, 64), (64, 65), (1024, 65536), (4, 37), (1, 65536)):
        assert pkg.fpmatch_max_events(interval, n) == R.max_events(interval, n) == (n + interval - 1) // interval
    for interval, n in ((0, 1), (1025, 1), (4, -1), (4, 65537)):
        assert R.max_events(interval, n) == -1
        with pytest.raises(pkg.FmdError):
            pkg.fpmatch_max_events(interval, n)
    for p, w, b in ((35, 256, 32), (0, 16, 1), (100, 1024, 32), (35, 16, 9), (1, 16, 1), (99, 1008, 31)):
        assert pkg.fpmatch_max_errs(p, w, b) == R.max_errs(p, w, b) == (p * w * b) // 100
    for p, w, b in ((-1, 16, 1), (101, 16, 1), (35, 24, 1), (35, 0, 1), (35, 1040, 1), (35, 16, 0), (35, 16, 33)):
        assert R.max_errs(p, w, b) == -1
        with pytest.raises(pkg.FmdError):
            pkg.fpmatch_max_errs(p, w, b)
    base = R.default_config(n_channels=3, block=16, interval=4, max_errs=10, max_words=64, max_tracks=4, max_catalogue_words=100)
    edges = [("n_channels", 1, 0), ("n_bits", 1, 0), ("n_bits", 32, 33), ("block", 16, 0), ("block", 32, 24), ("block", 1024, 1040), ("interval", 1, 0), ("interval", 1024, 1025),
             ("max_errs", 0, -1), ("max_errs", 16 * 32, 16 * 32 + 1), ("hold", 1, 0), ("max_words", 1, 0), ("max_words", 65536, 65537), ("max_tracks", 1, 0),
             ("max_tracks", 1 << 20, (1 << 20) + 1), ("max_catalogue_words", 16, 15), ("max_catalogue_words", 1 << 28, (1 << 28) + 1)]
    for field, good, bad in edges:
        for v, ok in ((good, True), (bad, False)):
            cfg = {**base, field: v}
            if field == "block":
                cfg.update(max_catalogue_words=4096)
            assert R.check_config(cfg) == ok, (field, v)
            rc = L.fmd_fpmatch_state_bytes(C.byref(_lib_config(pkg, cfg)))
            assert (rc > 0) if ok else (rc == -1 and L.fmd_fpmatch_last_error(None)), (field, v)
    for ch, ok in ((256, True), (257, False)):                              # 2^24 queries a call at most
        cfg = {**base, "n_channels": ch, "interval": 1, "max_words": 65536}
        assert R.check_config(cfg) == ok and (L.fmd_fpmatch_design(C.byref(_lib_config(pkg, cfg)), None) == 0) == ok
    cfg = _lib_config(pkg, base)
    for starts, T in (([0, 25, 50, 75, 100], 4), ([0, 25, 50, 75, 100], 0), ([0, 16], 1), ([0, 15], 1), ([0, 25, 40, 75, 100], 4), ([0, 25, 20, 75, 100], 4),
                      ([1, 25, 50, 75, 100], 4), ([0, 26, 52, 78, 104], 4), ([0, 26, 52, 78, 104], 3), ([0, 20, 40, 60, 80, 100], 5), ([0, 100], 1), ([0, 101], 1),
                      ([], 0), ([0, 50, 50 + (1 << 62)], 2), ([0, -5], 1)):
        assert pkg.fpmatch_check_catalogue(cfg, starts, T) == R.check_catalogue(base, starts, T), (starts, T)
    assert [R.check_catalogue(base, s, len(s) - 1) for s in ([0, 25, 50, 75, 100], [0, 15], [0, 25, 20, 75, 100], [0, 101])] == [True, False, False, False]
    # the design: the mask, and the scratch's groups from the same tile the kernel uses
    for n_bits, mask in ((32, 0xFFFFFFFF), (9, 0xFF800000), (1, 0x80000000)):
        dd = pkg.fpmatch_design(pkg.fpmatch_default_config(n_bits=n_bits))
        assert dd.mask == mask == int(R.mask_of(n_bits))
    dd = pkg.fpmatch_design(pkg.fpmatch_default_config(n_channels=7, max_words=130, max_catalogue_words=3 * 1024 + 255))
    assert dd.tile == 1024 and dd.tile % 256 == 0 and dd.groups == 3 and dd.lds_bytes == 4 * (dd.tile + 255) and dd.max_events == 3 and dd.max_queries == 21
    assert pkg.fpmatch_design(pkg.fpmatch_default_config(max_catalogue_words=1 << 28)).groups == 256
    # the memory: the catalogue, the rings, the windows and the partial minima
    c = pkg.fpmatch_default_config(n_channels=4096, max_words=6, max_catalogue_words=1 << 18)
    assert pkg.fpmatch_state_bytes(c) == 4096 * (64 + 1024) + 4 * (1 << 18) + 4 * 4097 + 4 * 4097 + 4096 * 1024 + 4096 * 256 * 8


DESIGN_SETS = ((1, 32, 256, 64, 64, 4096, 1 << 22), (4096, 32, 256, 64, 6, 64, 1 << 18), (3, 9, 16, 4, 256, 16, 1 << 16), (2, 1, 1024, 1024, 65536, 1, 1024))


def test_host_unit_under_sanitizers(pkg, tmp_path):
    """fmd_fpmatch_design.cpp and tests/cpp/fpmatch_design_main.cpp, built with -fsanitize=address,undefined and run as a stand-alone
    program: clean, with exact-size arrays at the smallest and largest designs and at invalid ones, which write nothing; the figures it
    prints are the library's as built"""
    exe = tmp_path / "fpmatch_design_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}",
                    f"-I{csrc}", str(csrc / "fmd_fpmatch_design.cpp"), str(ROOT / "tests" / "cpp" / "fpmatch_design_main.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)] + [str(v) for s in DESIGN_SETS for v in s], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(DESIGN_SETS) + 2
    for line, (ch, bits, W, I, mw, mt, mc) in zip(lines, DESIGN_SETS):
        cfg = pkg.fpmatch_default_config(n_channels=ch, n_bits=bits, block=W, interval=I, max_words=mw, max_tracks=mt, max_catalogue_words=mc)
        d = pkg.fpmatch_design(cfg)
        assert [int(v) for v in line.split()] == [d.mask, d.tile, d.query_block, d.groups, d.lds_bytes, d.max_events, d.max_queries, pkg.fpmatch_state_bytes(cfg)]
        assert d.mask == int(R.mask_of(bits)) and d.max_events == R.max_events(I, mw) and d.max_queries == ch * d.max_events
    dflt = R.default_config()
    assert lines[-2].split() == ["default"] + [str(dflt[k]) for k in R.CONFIG_FIELDS[:-1]]
