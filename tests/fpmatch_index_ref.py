"""The indexed fingerprint matcher's definition (include/fmdemod.h, "Fingerprint matcher", "index") restated in plain numpy / Python on
top of tests/fpmatch_ref.py: the index configuration's checks, the index (a stable sort of the masked words), the candidate set S of a
query (look-ups with the skip rule, the follow rule, validity), the minimum over S with its tie rule, and the four statistics.
Everything else (push, the query schedule, the detector, events, records, bytes) is the base class's.  Everything is an integer, so
whatever is compared with this file is compared for equality."""
import numpy as np

import fpmatch_ref as R

INDEX_STATUS_DTYPE = np.dtype([("candidates", "<u8"), ("skipped", "<u8"), ("followed", "<u8"), ("empty", "<u8")])
assert INDEX_STATUS_DTYPE.itemsize == 32
INDEX_FIELDS = ("max_bucket", "follow")
CHUNK, TABLE, MAX_DIR_BITS = 4096, 8192, 24


def index_default_config(**fields) -> dict:
    idx = dict(max_bucket=8, follow=2)
    assert set(fields) <= set(idx)
    idx.update(fields)
    return idx


def check_index_config(idx: dict) -> bool:
    return 1 <= idx["max_bucket"] <= 64 and 0 <= idx["follow"] <= 8


def dir_bits(cfg: dict) -> int:
    """min(n_bits, ceil(log2(max_catalogue_words)) - 4 clamped into 1 ... 24)"""
    lg = (cfg["max_catalogue_words"] - 1).bit_length()
    return min(cfg["n_bits"], min(max(lg - 4, 1), MAX_DIR_BITS))


def index_design(cfg: dict, idx: dict) -> dict:
    b = dir_bits(cfg)
    return dict(dir_bits=b, chunk=CHUNK, chunk_words=min(256, CHUNK // idx["max_bucket"]), table=TABLE, dir_entries=(1 << b) + 1,
                index_bytes=8 * cfg["max_catalogue_words"] + 4 * ((1 << b) + 1))


def index_state_bytes(cfg: dict, idx: dict) -> int:
    C, W = cfg["n_channels"], cfg["block"]
    Q = C * R.max_events(cfg["interval"], cfg["max_words"])
    return (C * (64 + 4 * W) + 4 * cfg["max_catalogue_words"] + 4 * (cfg["max_tracks"] + 1) + 4 * (C + 1) + Q * W * 4 + Q * 8 + Q * 8 + C * 32 +
            index_design(cfg, idx)["index_bytes"])


def build_index(words, n_bits: int, bits: int):
    """(keys, pos, dir) of a catalogue: the masked words in ascending order, equal ones in ascending position"""
    k = np.asarray(words, np.uint32) & R.mask_of(n_bits)
    pos = np.argsort(k, kind="stable").astype(np.int32)
    keys = k[pos]
    d = np.searchsorted(keys >> np.uint32(32 - bits), np.arange((1 << bits) + 1), side="left").astype(np.int32)
    return keys, pos, d


class IndexedMatcher(R.Matcher):
    """R.Matcher whose search is over the candidate set S.  index: the fields of index_default_config.  last: per query (station, e, S
    as a sorted array), for the tests that compare with the brute-force search."""

    def __init__(self, index=None, **fields):
        super().__init__(**fields)
        self.idx = index_default_config(**(index or {}))
        assert check_index_config(self.idx)
        self.ist = np.zeros(self.C, INDEX_STATUS_DTYPE)
        self.keys, self.pos = np.zeros(0, np.uint32), np.zeros(0, np.int32)
        self.last = []
        self._station = 0

    def reset(self, channel: int = -1):
        super().reset(channel)
        for c in (range(self.C) if channel < 0 else (channel,)):
            self.ist[c] = np.zeros(1, INDEX_STATUS_DTYPE)[0]

    def load_raw(self, words, starts, n_tracks: int) -> bool:
        if not super().load_raw(words, starts, n_tracks):
            return False                                                     # the old index stays
        self.pos = np.argsort(self.cat, kind="stable").astype(np.int64)
        self.keys = self.cat[self.pos]
        return True

    def occ(self, k) -> np.ndarray:
        """the catalogue word positions whose masked word is k, ascending"""
        lo, hi = np.searchsorted(self.keys, k, side="left"), np.searchsorted(self.keys, k, side="right")
        return self.pos[lo:hi]

    def candidates(self, q: np.ndarray, c: int) -> np.ndarray:
        """S of a query of station c with window q, sorted; counts the statistics"""
        K, d, s, ix = self.idx["max_bucket"], self.idx["follow"], self.st[c], self.ist[c]
        proposed = [np.zeros(0, np.int64)]
        for j in range(self.W):
            o = self.occ(q[j] & self.mask)
            if o.size > K:
                ix["skipped"] += 1
                continue
            ix["candidates"] += o.size
            proposed.append(o - j)
        if d > 0 and s["track"] >= 0:
            ix["followed"] += 1
            p_exp = int(self.starts[int(s["track"])]) + int(s["offset"]) + self.I * (int(s["misses"]) + 1)
            proposed.append(np.arange(p_exp - d, p_exp + d + 1, dtype=np.int64))
        p = np.unique(np.concatenate(proposed))
        p = p[(p >= 0) & (p < self.valid.size)]
        return p[self.valid[p]]

    def search(self, q: np.ndarray):
        """(track, offset, errs, positions of S at the minimum) for the station process() is at"""
        S = self.candidates(q, self._station)
        self.last.append((self._station, S))
        if S.size == 0:
            self.ist[self._station]["empty"] += 1
            return -1, 0, 0xFFFFFFFF, 0
        qm = np.asarray(q, np.uint32) & self.mask
        e = np.array([int(R.popcount(qm ^ self.cat[p:p + self.W]).sum()) for p in S], np.int64)
        i = int(np.argmin(e))                                                # the first of the smallest: S ascends
        p = int(S[i])
        t = int(np.searchsorted(self.starts, p, side="right")) - 1
        return t, p - int(self.starts[t]), int(e[i]), int(np.count_nonzero(e == e[i]))

    def process(self, words, nwords=None, n=None, active=None):
        """the base class's, a station at a time, so that search() knows whose record the follow rule reads"""
        n = int(n if n is not None else min(len(w) for w in words))
        events, flags, ok = [], [], []
        for c in range(self.C):
            self._station = c
            only = [i == c and (active is None or bool(active[i])) for i in range(self.C)]
            e, f, o = super().process(words, nwords=nwords, n=n, active=only)
            events.append(e[c]); flags.append(f[c]); ok.append(o[c])
        return events, flags, ok

    def index_status(self) -> np.ndarray:
        return self.ist.copy()


# ---- the cases the CPU and GPU tests share: each (configuration, index configuration, tracks, per station its words)

SMALL = dict(block=16, interval=4, hold=2, max_words=256, max_tracks=16, max_catalogue_words=1 << 12)


def near(words: np.ndarray, keep=()) -> np.ndarray:
    """`words` with the lowest bit of every word flipped but those at `keep`: one error a word and no exact word (at 32 bits)"""
    w = np.array(words, np.uint32) ^ np.uint32(1)
    w[list(keep)] ^= np.uint32(1)
    return w


def skip_case():
    """a track of 50 zero words between two others at K = 8, and a station playing zeros: every word is skipped, S is empty and every
    query a miss, while the brute-force search hits with errs 0; station 1 plays track 0 and is found"""
    tracks = [R.random_words(40, 1201), np.zeros(50, np.uint32), R.random_words(30, 1202)]
    return dict(SMALL, n_channels=2), dict(max_bucket=8, follow=2), tracks, [np.zeros(40, np.uint32), tracks[0].copy()]


FOLLOW_SEED = 1303       # no word of the 20 % pieces is exact under this seed (the CPU test checks it, as it does for STREAM_SEEDS)


def follow_case(follow: int):
    """W = 16, max_errs at 35 %, hold 2.  Station 0: track 1 from its word 8 clean for 32 words, then on at 20 % flipped bits: with d = 2
    it stays identified, with d = 0 it is released after `hold` misses.  Station 1: the same with the track's word 60 dropped: the offset
    moves by 1 and is followed.  Station 2: track 2, the catalogue's last, clean up to its end and then unrelated words: the positions
    around p_exp fall off the track's end and above D - W.  Station 3: track 0's tail at 20 % running into track 1's head: around p_exp
    lie windows that straddle two tracks."""
    tracks = [R.random_words(64, 1311), R.random_words(200, 1312), R.random_words(48, 1313)]
    t1 = tracks[1]
    s0 = np.concatenate([t1[8:40], R.flip(t1[40:128], 0.20, FOLLOW_SEED)])
    dropped = np.concatenate([t1[8:60], t1[61:129]])
    s1 = np.concatenate([dropped[:32], R.flip(dropped[32:], 0.20, FOLLOW_SEED + 10)])
    s2 = np.concatenate([tracks[2][8:], R.random_words(80, 1314)])
    s3 = np.concatenate([tracks[0][4:36], R.flip(np.concatenate([tracks[0][36:], t1[:60]]), 0.20, FOLLOW_SEED + 20)])
    assert [s.size for s in (s0, s1, s2, s3)] == [120] * 4
    cfg = dict(SMALL, n_channels=4, max_errs=R.max_errs(35, 16, 32))
    return cfg, dict(max_bucket=8, follow=follow), tracks, [s0, s1, s2, s3]


def below_zero_case():
    """I = 1 and d = 2: a station identified at the catalogue's position 0 expects position 1 next, so position -1 is proposed and dropped"""
    tracks = [R.random_words(40, 1321)]
    return dict(SMALL, n_channels=1, interval=1), dict(max_bucket=8, follow=2), tracks, [np.concatenate([tracks[0][:18], near(tracks[0][18:36])])]


def bucket_case(extremes: bool):
    """K = 3, dir_bits 8.  The catalogue's ordinary words have a top byte in 0x10 ... 0x7f, so the directory slices above it are empty.
    Track 1 holds the word X three times (exactly K) and Y four times (K + 1: skipped); with `extremes` track 0 holds 0x00000000 and
    0xffffffff, the smallest and the largest key.  Station 0 plays track 0 exactly (its extreme words are looked up like any other);
    station 1 plays track 1 with every word one bit off but the X, Y (and nothing else): windows with an X have three proposals, windows
    with only Ys none; station 2 plays words in no slice the catalogue fills, above every key and below every key but 0."""
    rng = np.random.default_rng(1331)
    plain = lambda n: ((rng.integers(0x10, 0x80, n, dtype=np.uint64) << 24) | rng.integers(0, 1 << 24, n, dtype=np.uint64)).astype(np.uint32)
    t0, t1, t2 = plain(64), plain(80), plain(33)
    if extremes:
        t0[[7, 30]] = 0
        t0[[12, 44, 45]] = 0xFFFFFFFF
    X, Y = np.uint32(0x31415926), np.uint32(0x27182818)
    xs, ys = [5, 30, 55], [10, 20, 40, 60]
    t1[xs], t1[ys] = X, Y
    odd = np.array([0x90000000, 0xFFFFFFFE, 0x00000001, 0x0FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x00000000, 0xC0000000] * 8, np.uint32)
    words = [t0.copy(), np.concatenate([near(t1[:64], xs + ys)]), odd]
    cfg = dict(SMALL, n_channels=3, max_tracks=3)
    assert dir_bits(R.default_config(**cfg)) == 8
    return cfg, dict(max_bucket=3, follow=0), [t0, t1, t2], words


def slice_case(kind: str):
    """dir_bits 8.  "one": every catalogue word has the top byte 0x42, so one directory slice holds the whole index; "ends": top bytes
    0x00 and 0xff only, the first and the last slice.  Two stations play excerpts at 5 % flipped bits (of the low 24 bits), one unrelated words"""
    rng = np.random.default_rng(1341)
    low = lambda n: rng.integers(0, 1 << 24, n, dtype=np.uint64).astype(np.uint32)
    sizes = (300, 150, 90)
    if kind == "one":
        tracks = [low(n) | np.uint32(0x42000000) for n in sizes]
    else:
        tracks = [low(n) | (np.uint32(0xFF000000) * (rng.integers(0, 2, n).astype(np.uint32))) for n in sizes]
    noisy = lambda w, seed: w ^ (R.flip(np.zeros(w.size, np.uint32), 0.05, seed) & np.uint32(0x00FFFFFF))
    words = [noisy(tracks[0][100:180], 1342), noisy(tracks[2][5:85], 1343), low(80) | np.uint32(0x42000000 if kind == "one" else 0xFF000000)]
    return dict(SMALL, n_channels=3, max_tracks=3), dict(max_bucket=8, follow=2), tracks, words


def capacity_case(copies: int):
    """W = 1024, K = 64: a catalogue of `copies` copies of one 1024-word track and a station playing it.  At 64 copies every window word
    has a run of exactly K: 65 536 proposals, 64 distinct positions, and the lowest copy wins; at 65 every word is skipped"""
    track = R.random_words(1024, 1351)
    cfg = dict(n_channels=1, block=1024, interval=1024, hold=2, max_words=1024, max_tracks=copies, max_catalogue_words=copies * 1024)
    return cfg, dict(max_bucket=64, follow=2), [track.copy() for _ in range(copies)], [track.copy()]
