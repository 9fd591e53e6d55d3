"""The fingerprint matcher's definition (include/fmdemod.h, "Fingerprint matcher") restated in plain numpy / Python: configuration and
catalogue checks, push, queries in ascending e, position validity, the arg-minimum with its tie rule, the detector, events, records and
bytes.  Everything is an integer, so whatever is compared with this file is compared for equality.  Also the streams and catalogues the
CPU and GPU tests share."""
import numpy as np

STATUS_DTYPE = np.dtype([("words", "<u8"), ("queries", "<u8"), ("hits", "<u8"), ("clamped", "<u8"), ("since", "<u8"), ("track", "<i4"), ("offset", "<i4"),
                         ("errs", "<u4"), ("misses", "<u4"), ("fill", "<u4"), ("flags", "<u4")])
EVENT_DTYPE = np.dtype([("end", "<u8"), ("track", "<i4"), ("offset", "<i4"), ("errs", "<u4"), ("flags", "<u4")])
assert STATUS_DTYPE.itemsize == 64 and EVENT_DTYPE.itemsize == 24
CONFIG_FIELDS = ("n_channels", "n_bits", "block", "interval", "max_errs", "hold", "max_words", "max_tracks", "max_catalogue_words", "device")
MAX_QUERIES = 1 << 24
_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.uint32)


def popcount(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.uint32)
    return _POP16[x & np.uint32(0xFFFF)] + _POP16[x >> np.uint32(16)]


def max_events(interval: int, n: int) -> int:
    if not (1 <= interval <= 1024 and 0 <= n <= 65536):
        return -1
    return (n + interval - 1) // interval


def max_errs(ber_percent: int, block: int, n_bits: int) -> int:
    if not (0 <= ber_percent <= 100 and 16 <= block <= 1024 and block % 16 == 0 and 1 <= n_bits <= 32):
        return -1
    return (ber_percent * block * n_bits) // 100


def default_config(**fields) -> dict:
    cfg = dict(n_channels=1, n_bits=32, block=256, interval=64, max_errs=(35 * 256 * 32) // 100, hold=3, max_words=64, max_tracks=4096,
               max_catalogue_words=1 << 22, device=-1)
    assert set(fields) <= set(cfg)
    cfg.update(fields)
    if "max_errs" not in fields:                                             # (as capi.fpmatch_default_config: the threshold follows block and n_bits)
        cfg["max_errs"] = (35 * cfg["block"] * cfg["n_bits"]) // 100
    return cfg


def check_config(cfg: dict) -> bool:
    c = cfg
    if c["n_channels"] <= 0 or not 1 <= c["n_bits"] <= 32:
        return False
    if not (16 <= c["block"] <= 1024 and c["block"] % 16 == 0) or not 1 <= c["interval"] <= 1024:
        return False
    if not 0 <= c["max_errs"] <= c["block"] * c["n_bits"] or c["hold"] < 1 or not 0 < c["max_words"] <= 65536:
        return False
    if not 1 <= c["max_tracks"] <= 1 << 20 or not c["block"] <= c["max_catalogue_words"] <= 1 << 28:
        return False
    return c["n_channels"] * max_events(c["interval"], c["max_words"]) <= MAX_QUERIES


def check_catalogue(cfg: dict, starts, n_tracks: int) -> bool:
    if not 0 <= n_tracks <= cfg["max_tracks"]:
        return False
    if n_tracks == 0:
        return starts is None or len(starts) == 0 or int(starts[0]) == 0
    if starts is None or int(starts[0]) != 0:
        return False
    for t in range(n_tracks):
        if int(starts[t + 1]) - int(starts[t]) < cfg["block"] or int(starts[t + 1]) > cfg["max_catalogue_words"]:
            return False
    return True


def mask_of(n_bits: int) -> np.uint32:
    return np.uint32((0xFFFFFFFF << (32 - n_bits)) & 0xFFFFFFFF)


class Matcher:
    """C stations; `cfg` as default_config gives it.  ties: per query (station, e, the number of valid positions at the minimum)."""

    def __init__(self, **fields):
        self.cfg = default_config(**fields)
        assert check_config(self.cfg)
        c = self.cfg
        self.C, self.W, self.I, self.mask = c["n_channels"], c["block"], c["interval"], mask_of(c["n_bits"])
        self.cat, self.starts, self.valid = np.zeros(0, np.uint32), np.zeros(1, np.int64), np.zeros(0, bool)
        self.hist = [np.zeros(0, np.uint32) for _ in range(self.C)]          # a station's newest W words (the ring)
        self.st = np.zeros(self.C, STATUS_DTYPE)
        self.st["track"] = -1
        self.ties = []

    def reset(self, channel: int = -1):
        for c in (range(self.C) if channel < 0 else (channel,)):
            self.hist[c] = np.zeros(0, np.uint32)
            self.st[c] = np.zeros(1, STATUS_DTYPE)[0]
            self.st[c]["track"] = -1

    def load(self, tracks) -> bool:
        tracks = [np.asarray(t, np.uint32).reshape(-1) for t in tracks]
        starts = np.concatenate([[0], np.cumsum([t.size for t in tracks])]).astype(np.int64)
        return self.load_raw(np.concatenate(tracks) if tracks else np.zeros(0, np.uint32), starts, len(tracks))

    def load_raw(self, words, starts, n_tracks: int) -> bool:
        """False, and nothing changed, for a catalogue the definition refuses"""
        if not check_catalogue(self.cfg, starts, n_tracks):
            return False
        D = int(starts[n_tracks]) if n_tracks else 0
        self.cat = np.array(words[:D], np.uint32) & self.mask
        self.starts = np.array(starts[:n_tracks + 1], np.int64) if n_tracks else np.zeros(1, np.int64)
        self.valid = np.zeros(max(D - self.W + 1, 0), bool)
        for t in range(n_tracks):
            self.valid[int(self.starts[t]):int(self.starts[t + 1]) - self.W + 1] = True
        self.st["track"] = -1
        self.st["misses"] = 0
        self.st["flags"] &= 2
        return True

    def errs(self, q: np.ndarray) -> np.ndarray:
        """errs(p) of every position p = 0 ... D - W, valid or not"""
        npos = self.cat.size - self.W + 1
        acc = np.zeros(max(npos, 0), np.uint32)
        for j in range(self.W if npos > 0 else 0):
            acc += popcount((q[j] & self.mask) ^ self.cat[j:j + npos])
        return acc

    def search(self, q: np.ndarray):
        """(track, offset, errs, positions at the minimum)"""
        if not self.valid.any():
            return -1, 0, 0xFFFFFFFF, 0
        e = self.errs(q).astype(np.int64)
        e[~self.valid] = 1 << 40
        p = int(np.argmin(e))                                                # the first of the smallest
        t = int(np.searchsorted(self.starts, p, side="right")) - 1
        return t, p - int(self.starts[t]), int(e[p]), int(np.count_nonzero(e == e[p]))

    def process(self, words, nwords=None, n=None, active=None):
        """words: per station a run of uint32 (a [C, >= n] array will do); returns (events per station or None where inactive, flags [C],
        ok [C]; the bytes of an inactive station are None in the lists)"""
        c_ = self.cfg
        n = int(n if n is not None else min(len(w) for w in words))
        assert 0 <= n <= c_["max_words"]
        events, flags, ok = [], [], []
        for c in range(self.C):
            if active is not None and not active[c]:
                events.append(None); flags.append(None); ok.append(None)
                continue
            s = self.st[c]
            k = n if nwords is None else int(nwords[c])
            if k < 0 or k > n:
                s["clamped"] += 1
                k = min(max(k, 0), n)
            before = int(s["words"])
            new = np.asarray(words[c], np.uint32)[:k]
            have = np.concatenate([self.hist[c], new])                       # words before - len(hist) ... before + k - 1
            first = before - self.hist[c].size
            ev = []
            for e in range((before // self.I + 1) * self.I, before + k + 1, self.I):
                if e < self.W:
                    continue
                q = have[e - self.W - first:e - first]
                assert q.size == self.W
                track, offset, errs, nmin = self.search(q)
                self.ties.append((c, e, nmin))
                hit = track >= 0 and errs <= c_["max_errs"]
                s["queries"] += 1
                s["errs"] = errs
                if hit:
                    s["hits"] += 1
                    if s["track"] != track:
                        s["track"], s["since"] = track, e
                    s["offset"], s["misses"] = offset, 0
                elif s["track"] >= 0:
                    s["misses"] += 1
                    if s["misses"] == c_["hold"]:
                        s["track"], s["misses"] = -1, 0
                s["flags"] = 2 if hit else 0
                ev.append((e, track, offset, errs, 1 if hit else 0))
            self.hist[c] = have[-self.W:] if have.size else have
            s["words"] = before + k
            s["fill"] = min(before + k, self.W)
            s["flags"] = (int(s["flags"]) & 2) | (1 if s["track"] >= 0 else 0)
            assert len(ev) <= max_events(self.I, n)
            events.append(np.array(ev, EVENT_DTYPE) if ev else np.zeros(0, EVENT_DTYPE))
            flags.append(int(s["flags"])); ok.append(int(s["flags"]) & 1)
        return events, flags, ok

    def status(self) -> np.ndarray:
        return self.st.copy()


# ---- the streams and catalogues the tests share

def flip(words: np.ndarray, share: float, seed: int, n_bits: int = 32) -> np.ndarray:
    """`words` with each of the top n_bits of every word flipped with probability `share`, by a seeded generator"""
    rng = np.random.default_rng(seed)
    w = np.array(words, np.uint32)
    bits = rng.random((w.size, 32)) < share
    x = (bits.astype(np.uint64) << np.arange(31, -1, -1, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return w ^ (x & mask_of(n_bits))


def random_words(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


MAIN = dict(n_channels=3, block=16, interval=4, hold=2, max_words=256, max_tracks=16, max_catalogue_words=1 << 16)
MAIN_TRACKS = (16, 17, 50, 700)
PRE = (0, 5, 37)             # words each station has taken before the calls under test: three query phases


def main_catalogue(n_bits: int = 32):
    return [random_words(n, CATALOGUE_SEED[n_bits] + i) for i, n in enumerate(MAIN_TRACKS)]


# per n_bits the seeds of the twelve generated pieces of main_streams, searched once so that every query's minimum is unique in this
# restatement (tests/test_fpmatch_cpu.py checks it; with 9 bits a random window ties at its minimum about every other time)
STREAM_SEEDS = {32: [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 2], 9: [0, 2, 1, 2, 3, 1, 0, 0, 0, 0, 0, 2]}
CATALOGUE_SEED = {32: 900, 9: 902}
# (piece, its first word, its end) per station, in the station's own word count
STREAM_PIECES = (((None, 0, 60), (1, 60, 80), (2, 80, 120), (3, 120, 140)),
                 ((4, 0, 5), (None, 5, 48), (5, 48, 108), (None, 108, 140), (6, 140, 145)),
                 ((7, 0, 37), (8, 37, 61), (9, 61, 111), (10, 111, 161), (11, 161, 177)))


def main_streams(tracks, n_bits: int = 32, seeds=None):
    """three stations' words (their PRE words in front), 140 behind them.  Station 0: track 3 from word 100 clean, unrelated words,
    track 2 from word 10 with 5 % of the bits flipped running off its end into unrelated words; station 1: the tail of track 1 spliced
    to the head of track 2 (the windows that straddle them have errs 0 against positions no track holds), track 3 at 30 %, track 0
    twice (a track of exactly W words: it is found only where a window is the whole track); station 2: has taken track 3 at 5 %, then unrelated words, track 3's start at 5 %, track 2 at 30 %, unrelated words."""
    seeds = STREAM_SEEDS[n_bits] if seeds is None else seeds
    r = lambda n, k: random_words(n, 1000 * seeds[k] + k)
    f = lambda w, share, k: flip(w, share, 1000 * seeds[k] + k, n_bits)
    s0 = np.concatenate([tracks[3][100:160], r(20, 1), f(tracks[2][10:], 0.05, 2), r(20, 3)])
    s1 = np.concatenate([r(PRE[1], 4), tracks[1][3:], tracks[2][:29], f(tracks[3][400:460], 0.30, 5), tracks[0], tracks[0], r(5, 6)])
    s2 = np.concatenate([f(tracks[3][300:300 + PRE[2]], 0.05, 7), r(24, 8), f(tracks[3][:50], 0.05, 9), f(tracks[2], 0.30, 10), r(16, 11)])
    assert [s.size - p for s, p in zip((s0, s1, s2), PRE)] == [140] * 3 and [s.size for s in (s0, s1, s2)] == [p[-1][2] for p in STREAM_PIECES]
    return [s0, s1, s2]


def tiled_catalogue(tile: int, block: int, seed: int = 700):
    """a catalogue that spans more than three column tiles of `tile` positions with one track twice, in different tiles: tracks 1 and 3
    are the same words, so a station playing them ties between two tiles and the lower position must win"""
    dup = random_words(3 * block, seed)
    tracks = [random_words(tile + 37, seed + 1), dup, random_words(2 * tile + 5, seed + 2), dup.copy(), random_words(block, seed + 3)]
    starts = np.concatenate([[0], np.cumsum([t.size for t in tracks])])
    assert starts[1] // tile != starts[3] // tile and starts[-1] - block + 1 > 3 * tile
    return tracks


ROWMAP_STATIONS = (1, 1024, 1025, 2049)      # shares of 1, 1, 2 and 3 stations a thread of the map's 1024; the short and empty shares move
ROWMAP_CALLS = (24, 16)                      # n of the two calls


def rowmap_case(C: int, ends: bool):
    """The row map's shapes on the main configuration with short tracks: (tracks, per call (words [C, n], nwords [C]), active [C]).  A
    scattered third of the stations is left out, stations 0 and C - 1 among them or, with `ends`, both taken.  Every station has its own
    run of 40 words and hands over an uneven number of them a call (0 ... n, both ends forced), so that in either call some active
    stations fire no query and others several, and the second call's map reads the counts the first one wrote.  A quarter of the stations
    play track 2 clean from their own offset and another quarter with 5 % of the bits flipped, so that there are hits to hold and lose."""
    rng = np.random.default_rng(4000 + 2 * C + int(ends))
    tracks = [random_words(n, 4100 + i) for i, n in enumerate((16, 23, 64))]
    c = np.arange(C)
    active = c % 3 != 1
    active[[0, C - 1]] = ends
    runs = rng.integers(0, 1 << 32, (C, sum(ROWMAP_CALLS)), dtype=np.uint64).astype(np.uint32)
    for s in range(0, C, 2):
        piece = tracks[2][s % 20:s % 20 + 40]
        runs[s] = piece if s % 4 == 0 else flip(piece, 0.05, 4200 + s)
    calls, at = [], np.zeros(C, np.int64)
    for n in ROWMAP_CALLS:
        k = rng.integers(0, n + 1, C)
        k[c % 7 == 2] = 0
        k[c % 7 == 4] = n
        calls.append((np.take_along_axis(runs, at[:, None] + np.arange(n)[None, :], axis=1), k.astype(np.int32)))
        at += k
    return tracks, calls, active
