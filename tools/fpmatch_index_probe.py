"""Times the indexed fingerprint matcher's call (fmd_fpmatch_create_ex: k_fpmatch_map, k_fpmatch_gather, k_fpmatch_probe,
k_fpmatch_finish_idx) beside the brute-force object's in the same process, on tools/fpmatch_probe.py's protocol: 4096 stations at the
default configuration (W = 256, I = 64, 32 bits; index K = 8, d = 2), every 64 ms block hands a station alternately 5 and 6 words through
d_nwords, a round is 128 calls = 704 words = 11 searches a station; in the staggered run station c has taken c mod 64 words beforehand, in
the aligned run every station searches in the same call.  Five alternating rounds between device events after a warm-up round; median
and range.  Two catalogues: (a) 64 tracks x 2609 words (166 976 words), both methods; (b) `--big-words` words (default 2^26) in tracks
of 2609, the indexed method in full and the brute-force one for `--big-brute-calls` single staggered calls (its rings are filled against
an empty catalogue first, so that only the timed calls search).  Two station loads: every station plays unrelated words; or every other
station plays the catalogue from a track's start with 0.5 % of the bits flipped (the case that makes most of a window's look-ups propose
one position) and the others unrelated words.  Reports us per call, us per search, the index records per search and the load time.
Needs a GPU.  `--out FILE` also writes the report to a file (profiles/fpmatch/)."""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fmradio_loader  # noqa: E402

CALLS_ROUND, BLOCK_US, TRACK = 128, 64000.0, 2609


def station_words(cat: np.ndarray, C: int, length: int, playing: bool, seed: int) -> torch.Tensor:
    """[C, length] int32 on the device: unrelated words, and with `playing` every other station the catalogue from a track's start with
    0.5 % of the bits flipped"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randint(-(1 << 31), 1 << 31, (C, length), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    if playing:
        tracks = (cat.size - length) // TRACK
        rows = []
        for c in range(0, C, 2):
            at = ((c * 7919) % max(tracks, 1)) * TRACK
            rows.append(cat[at:at + length])
        clean = torch.from_numpy(np.stack(rows).view(np.int32)).cuda()
        weights = (1 << torch.arange(32, device="cuda", dtype=torch.int64))
        for r0 in range(0, clean.shape[0], 256):                             # (in slabs: 32 random numbers a word)
            part = clean[r0:r0 + 256]
            bits = (torch.rand((part.shape[0], length, 32), generator=g, device="cuda") < 0.005).to(torch.int64)
            flips = (bits * weights).sum(dim=2)
            w[2 * r0:2 * (r0 + part.shape[0]):2] = part ^ torch.where(flips >= (1 << 31), flips - (1 << 32), flips).to(torch.int32)
    return w.contiguous()


class Run:
    """one matcher with its stream: call(i) hands every station its next 5 or 6 words"""

    def __init__(self, pkg, C, T, D, tracks, words, staggered, index, counts):
        self.m = pkg.FingerprintMatcher(C, index=index, max_words=64, max_tracks=T, max_catalogue_words=D)
        t0 = time.perf_counter()
        if tracks is not None:
            self.m.load(tracks)
        self.load_s = time.perf_counter() - t0
        self.words, self.counts, self.at, self.i = words, counts, 64, 0
        if staggered:                                                        # station c has taken the c mod 64 words in front of column 64
            k = (torch.arange(C, device="cuda") % 64).to(torch.int32)
            cols = (64 - k.to(torch.int64)).unsqueeze(1) + torch.arange(64, device="cuda").unsqueeze(0)
            pre = torch.gather(words, 1, cols.clamp(max=words.shape[1] - 1)).contiguous()
            self.m.process(pre, nwords=k)
        rows = pkg.fpmatch_max_events(self.m.interval, 6)
        self.out = (torch.zeros((C, rows, 3), dtype=torch.int64, device="cuda"), torch.zeros(C, dtype=torch.int32, device="cuda"),
                    torch.zeros(C, dtype=torch.uint8, device="cuda"), torch.zeros(C, dtype=torch.uint8, device="cuda"))

    def call(self):
        ev, ne, fl, ok = self.out
        k = 5 + (self.i & 1)
        self.m.process(self.words[:, self.at:self.at + 6], nwords=self.counts[self.i & 1], events=ev, nevents=ne, flags=fl, ok=ok)
        self.at += k
        self.i += 1

    def round(self):
        for _ in range(CALLS_ROUND):
            self.call()


def timed(fn) -> float:
    """us of device time of fn()"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stations", type=int, default=4096)
    ap.add_argument("--big-words", type=int, default=1 << 26)
    ap.add_argument("--big-brute-calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    C = a.stations
    length = 64 + (a.rounds + 2) * 704 + 8
    counts = [torch.full((C,), k, dtype=torch.int32, device="cuda") for k in (5, 6)]
    searches_call = C * 11 / CALLS_ROUND
    lines = [f"{C} stations, W 256, I 64, 32 bits, index K 8, d 2; 5 / 6 words a call through d_nwords; {a.rounds} alternating rounds of {CALLS_ROUND} calls after a "
             f"warm-up round, device events (us per call, averaged over a round); {searches_call:.0f} searches a call on average"]
    rng = np.random.default_rng(1)
    for name, T in (("a", 64), ("b", (a.big_words + TRACK - 1) // TRACK)):
        D = T * TRACK
        cat = rng.integers(0, 1 << 32, D, dtype=np.uint64).astype(np.uint32)
        tracks = [cat[t * TRACK:(t + 1) * TRACK] for t in range(T)]
        runs = {}
        for load in ("unrelated", "playing"):
            words = station_words(cat, C, length, load == "playing", 7 if load == "unrelated" else 8)
            for method in ("indexed", "brute") if name == "a" else ("indexed",):
                for phase in ("staggered", "aligned"):
                    runs[(load, method, phase)] = Run(pkg, C, T, D, tracks, words, phase == "staggered", True if method == "indexed" else None, counts)
        some = runs[("unrelated", "indexed", "staggered")].m
        dsn = some.index_design
        lines.append(f"catalogue ({name}): {T} tracks x {TRACK} words = {D} words; indexed object {some.state_bytes / 1e6:.1f} MB (index {dsn.index_bytes / 1e6:.1f} MB at "
                     f"capacity, dir_bits {dsn.dir_bits}); load (host radix sort, copies, synchronised): "
                     f"{statistics.median(r.load_s for k, r in runs.items() if k[1] == 'indexed') * 1e3:.1f} ms indexed" +
                     (f", {statistics.median(r.load_s for k, r in runs.items() if k[1] == 'brute') * 1e3:.1f} ms brute force" if name == "a" else ""))
        print(f"catalogue ({name}) loaded into {len(runs)} objects", file=sys.stderr, flush=True)
        for r in runs.values():                                              # the warm-up round: every ring full, every station searching
            r.round()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, r in runs.items():
                times[k].append(timed(r.round) / CALLS_ROUND)
        for k, v in times.items():
            med = statistics.median(v)
            m = runs[k].m
            st = m.status()
            q = float(st["queries"].sum())
            line = (f"  ({name}) {k[0]:9s} {k[1]:7s} {k[2]:9s} median {med:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   {med / BLOCK_US * 100:6.3f} % of 64 ms  "
                    f"{med / searches_call:6.3f} us a search; hits {int(st['hits'].sum())} of {int(q)} searches")
            if k[1] == "indexed":
                ix = m.index_status()
                line += (f"; per search: candidates {ix['candidates'].sum() / q:.3f}, skipped {ix['skipped'].sum() / q:.3f}, followed {ix['followed'].sum() / q:.3f}, "
                         f"empty {ix['empty'].sum() / q:.3f}")
            if k[2] == "staggered":
                line += f"; under a tenth of the block's time: {'yes' if med < BLOCK_US / 10 else 'NO'}"
            lines.append(line)
        if name == "a":
            for load in ("unrelated", "playing"):
                for phase in ("staggered", "aligned"):
                    bi = statistics.median(times[(load, "brute", phase)]) / statistics.median(times[(load, "indexed", phase)])
                    lines.append(f"  (a) {load} {phase}: brute force / indexed = {bi:.2f}")
        elif a.big_brute_calls > 0:
            # brute force at (b): rings filled against an empty catalogue, then the catalogue, then single staggered calls
            words = station_words(cat, C, length, False, 7)
            b = Run(pkg, C, T, D, None, words, True, None, counts)
            b.round()
            t0 = time.perf_counter()
            b.m.load(tracks)
            load_s = time.perf_counter() - t0
            single = [timed(b.call) for _ in range(a.big_brute_calls)]
            q = [int(x) for x in b.out[1].cpu().numpy().sum(keepdims=True)]
            lines.append(f"  (b) unrelated brute   staggered single calls {', '.join(f'{s:.0f}' for s in single)} us (the last with {q[0]} searches; not a round: "
                         f"{a.big_brute_calls} calls only); load {load_s * 1e3:.1f} ms")
            b.m.close()
        for r in runs.values():
            r.m.close()
        del runs, tracks, cat
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
