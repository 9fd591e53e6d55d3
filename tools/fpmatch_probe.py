"""Times the fingerprint matcher's call (fmd_fpmatch_*: k_fpmatch_map, k_fpmatch_gather, k_fpmatch_search, k_fpmatch_finish) beside
fmd_fprint_process_f32_dev, the fingerprinter that feeds it, in the same process: 4096 stations at the default configuration (W = 256,
I = 64, 32 bits) against a catalogue of 64 tracks of 30 s (2609 words each at 11.5 ms a word, about 167 000 words).  The stations are fed
per 64 ms block, alternately 5 and 6 words (5.5 on average), through d_nwords.  In the staggered run station c has taken c mod 64 words
beforehand, so the searches spread over the blocks; in the aligned run every station searches in the same call.  A round is 128 calls =
704 words = 11 searches a station either way.  The calls are timed in alternating rounds with device events around a round's
back-to-back calls, after a warm-up round; the median, minimum and maximum over the rounds are printed with the share of the block's
real time, the device time a search and the XOR / population-count word pairs a second; one more round of the aligned run is timed
call by call for its slowest call.  `--tracks` changes the catalogue's size.  Needs a GPU.  `--out FILE` also writes the report to a
file (profiles/fpmatch/)."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fmradio_loader  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stations", type=int, default=4096)
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--track-words", type=int, default=2609)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    pkg = fmradio_loader.load()
    C, T, tw = a.stations, a.tracks, a.track_words
    calls_round, block_us = 128, 64000.0
    rng = np.random.default_rng(1)
    tracks = [rng.integers(0, 1 << 32, tw, dtype=np.uint64).astype(np.uint32) for _ in range(T)]
    D = T * tw
    words = torch.from_numpy(rng.integers(0, 1 << 32, (C, 6), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
    counts = [torch.full((C,), k, dtype=torch.int32, device="cuda") for k in (5, 6)]
    made = {}
    for name in ("staggered", "aligned"):
        m = pkg.FingerprintMatcher(C, max_words=64, max_tracks=T, max_catalogue_words=D)
        m.load(tracks)
        if name == "staggered":
            pre = torch.from_numpy(rng.integers(0, 1 << 32, (C, 64), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
            m.process(pre, nwords=(torch.arange(C, device="cuda") % 64).to(torch.int32))
        rows = pkg.fpmatch_max_events(m.interval, 6)
        made[name] = (m, torch.zeros((C, rows, 3), dtype=torch.int64, device="cuda"), torch.zeros(C, dtype=torch.int32, device="cuda"),
                      torch.zeros(C, dtype=torch.uint8, device="cuda"), torch.zeros(C, dtype=torch.uint8, device="cuda"))
    n_audio = 2048
    x = (0.1 * torch.randn(C, n_audio, 2, device="cuda")).contiguous()
    fp = pkg.Fingerprinter(C, 32000, max_input_frames=n_audio)
    out_w = torch.zeros((C, pkg.fprint_max_prints(fp.hop, n_audio)), dtype=torch.int32, device="cuda")
    cnt_w = torch.zeros(C, dtype=torch.int32, device="cuda")

    def matcher_call(name, i):
        m, ev, ne, fl, ok = made[name]
        m.process(words, nwords=counts[i & 1], events=ev, nevents=ne, flags=fl, ok=ok)

    calls = {"staggered": lambda i: matcher_call("staggered", i), "aligned": lambda i: matcher_call("aligned", i),
             "fprint": lambda i: fp.process(x, out=out_w, nprints=cnt_w)}
    for fn in calls.values():                                                # the warm-up round: every ring full, every station searching
        for i in range(calls_round):
            fn(i)
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(calls_round):
                fn(i)
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) / calls_round * 1e3)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(calls_round + 1)]
    evs[0].record()
    for i in range(calls_round):
        calls["aligned"](i)
        evs[i + 1].record()
    torch.cuda.synchronize()
    single = [evs[i].elapsed_time(evs[i + 1]) * 1e3 for i in range(calls_round)]
    rounds_made = a.rounds + 1
    searches_call = C * 11 / calls_round
    pairs_search = (D - T * (256 - 1)) * 256                                 # valid positions x W
    med = {k: statistics.median(v) for k, v in times.items()}
    m0 = made["staggered"][0]
    lines = [f"{C} stations, W {m0.block}, I {m0.interval}, {m0.n_bits} bits; catalogue {T} tracks x {tw} words = {D} words; 5 / 6 words a call through d_nwords; "
             f"tile {m0.design.tile}, query block {m0.design.query_block}, {m0.design.groups} column groups; state {m0.state_bytes / 1e6:.1f} MB; {a.rounds} alternating "
             f"rounds of {calls_round} calls after a warm-up round, device events (us per call, averaged over a round)"]
    for k, v in times.items():
        lines.append(f"{k:10s} median {med[k]:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   {med[k] / block_us * 100:6.3f} % of the 64 ms a block lasts")
    for k in ("staggered", "aligned"):
        per = med[k] / searches_call
        lines.append(f"{k}: {searches_call:.0f} searches a call on average, {per:.2f} us a search, {pairs_search * searches_call / med[k] / 1e6:.2f} T word pairs/s; "
                     f"{med[k] / med['fprint']:.2f} x the fingerprinter's call; under a tenth of the block's time: {'yes' if med[k] < block_us / 10 else 'NO'}")
    lines.append(f"aligned, call by call: slowest {max(single):.1f} us (every station searches: {C} searches, {pairs_search * C / max(single) / 1e6:.2f} T word pairs/s), "
                 f"median {statistics.median(single):.1f} us")
    st = [made[k][0].status() for k in ("staggered", "aligned")]
    want = 11 * rounds_made - 3                                              # (no search before a station has W = 4 I words)
    lines.append(f"check: searches a station since the start: staggered {int(st[0]['queries'].min())} ... {int(st[0]['queries'].max())} (expected {want}), aligned "
                 f"{int(st[1]['queries'].min())} ... {int(st[1]['queries'].max())} (expected {want + 11}: one more round, call by call); hits {int(st[0]['hits'].sum())}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
