"""A pool of distinct station inputs and its oracle runs, for checking EVERY station of a large batch (TEST INFRASTRUCTURE, CPU only).

Tiled batches (station c given capture c % 8) cannot see a kernel that reads or writes another station's row at an offset that is a
multiple of the tile count: the row it reads holds the same capture.  Here station c is given input idx[c] of a pool of P = 509 distinct
inputs (a prime: no power-of-two stride maps a station onto an input it shares), drawn at random so that duplicates fall at no fixed
stride.  Each input is a window at its own sample offset into one of 16 long base captures of oracle/synth.py (different seeds and PI
codes; plain, pilot-less, detuned or weak pilot, noisy, realistic programme with a carrier offset).

The oracle runs (oracle/fm_oracle.c through tests/oraclelib.py), one per pool input, go through a process pool with the spawn start method.
This module imports only numpy, synth and oraclelib, so its workers never import torch or open the GPU (the worker asserts it).

check_block() compares a batch's rows with the expected rows of the inputs the stations were given; describe() names the offset a wrong row
was taken from (the station whose input that row's output belongs to), which is what an indexing bug in a kernel looks like.
"""
from __future__ import annotations

import collections
import concurrent.futures as cf
import ctypes as C
import multiprocessing as mp
import os
import sys
import time

import numpy as np

import oraclelib as O
import synth

P = 509                 # pool inputs (prime)
N_BASES = 16
BLOCKS = 14             # blocks submitted per run: loops lock from about block 8
READ_AT = (4, 9, 13)    # blocks after which the host reads the outputs
WINDOW_STRIDE = 1009    # samples at 256 kSa/s between consecutive windows of one base (times the decimation at higher rates)
MAP_SEED = 20_261_015

# base captures: (generator, keyword arguments); channel k + 1 gives each its own PI code and tone jitter
BASES = (
    [("plain", dict(seed=61_000))] * 8
    + [("plain", dict(seed=62_000, pilot_level=0.0))] * 2                  # no pilot: the loop never locks
    + [("plain", dict(seed=63_000, pilot_hz=19_003.0))]                     # pilot 3 Hz off
    + [("plain", dict(seed=64_000, pilot_level=0.05, noise_sigma=0.05))]    # weak pilot, more noise
    + [("plain", dict(seed=65_000, noise_sigma=0.1))]                       # noisy
    + [("realistic", dict(seed=66_000, cnr_db=35.0, carrier_offset_hz=25_000.0)),
       ("realistic", dict(seed=67_000, cnr_db=35.0, carrier_offset_hz=-18_000.0)),
       ("realistic", dict(seed=68_000, cnr_db=40.0))]
)
assert len(BASES) == N_BASES
PILOTLESS_BASES = frozenset(k for k, (_, kw) in enumerate(BASES) if kw.get("pilot_level", 1.0) == 0.0)


# bases with a pilot 3 Hz off, a weak pilot or more noise: in a 14-block run the tolerance mode's RDS bits part from the oracle's on 3-14 % of
# their windows (measured on one MI355X; every input of the other bases keeps identical bits from lock on)
MARGINAL_BASES = frozenset({10, 11, 12})


def marginal(i: int) -> bool:
    """Pool input i is a window of a capture with a detuned, weak or noisy pilot."""
    return i % N_BASES in MARGINAL_BASES


def deemphasised(i: int, mixed: bool) -> bool:
    """Pool input i runs with de-emphasis on (applied to the whole MPX, as the reference does: the RDS subcarrier is 25-29 dB down)."""
    ctl = ctl_of(i, mixed)
    return ctl is not None and ctl[2] == 1


def pilotless(i: int) -> bool:
    """Pool input i is a window of a capture without a pilot (Pool.base_of[i] == i % N_BASES)."""
    return i % N_BASES in PILOTLESS_BASES


# Controls as tuples in fmd_controls / fmo_controls field order:
# (audio_out, audio_stereo_mix_factor, use_deemphasis, deemphasis_tus, lpr_cutoff_hz, lmr_cutoff_hz); None = the defaults
CONTROL_FIELDS = ("audio_out", "audio_stereo_mix_factor", "use_deemphasis", "deemphasis_tus", "lpr_cutoff_hz", "lmr_cutoff_hz")
DEFAULT_CONTROLS = (2, 1.0, 0, 1, 15000, 15000)
CONTROL_SET = (
    (2, 1.0, 1, 50, 15000, 15000),        # de-emphasis 50 us
    (2, 1.0, 1, 75, 15000, 15000),        # de-emphasis 75 us
    (0, 1.0, 0, 1, 15000, 15000),         # L+R only
    (1, 1.0, 0, 1, 15000, 15000),         # L-R only
    (2, 1.0, 0, 1, 12000, 15000),         # narrower L+R
    (2, 1.0, 0, 1, 15000, 9000),          # narrower L-R
    (2, 0.5, 1, 75, 13000, 11000),        # stereo mix factor, de-emphasis and both cut-offs
)


def block_size(fs: int) -> int:
    return fs * 64 // 1000


def n_rds(fs: int) -> int:
    """Width of a block's RDS symbol row (fmd_rates.n_rds: 16 kSa/s over the block)."""
    return 16000 * block_size(fs) // fs


def bytes_cap(fs: int) -> int:
    """Width of a block's Manchester byte row (capi.BatchDemod.bytes_cap)."""
    return 16 * (n_rds(fs) // 256 + 1)


def ctl_of(i: int, mixed: bool):
    """Controls of pool input i: the defaults, or (mixed, about half the inputs) one of CONTROL_SET — a function of the input index, so that
    each (input, controls) pair has one oracle run."""
    if not mixed:
        return None
    h = (i * 2_654_435_761) >> 7 & 0xFF         # a fixed scramble of the index
    return None if h < 128 else CONTROL_SET[h % len(CONTROL_SET)]


def oracle_controls(ctl) -> O.Controls:
    return O.Controls(*(ctl if ctl is not None else DEFAULT_CONTROLS))


def station_map(n_stations: int, n_inputs: int = P, seed: int = MAP_SEED) -> np.ndarray:
    """idx[c]: the pool input station c is given.  Every input is used once before any repeats (when n_stations >= n_inputs), in an
    order drawn at random, so equal inputs do not fall at a fixed stride."""
    rng = np.random.default_rng([seed, n_stations, n_inputs])
    reps = -(-n_stations // n_inputs)
    return np.concatenate([rng.permutation(n_inputs) for _ in range(reps)])[:n_stations].astype(np.int64)


class Pool:
    """The P inputs of one (rate, format): input i is the window of base_of[i] at offset[i], blocks * block_size samples long."""

    def __init__(self, fs: int, u8: bool, n_inputs: int = P, blocks: int = BLOCKS):
        self.fs, self.u8, self.n_inputs, self.blocks = fs, u8, n_inputs, blocks
        self.bs = block_size(fs)
        self.m = fs // 256_000
        self.base_of = np.arange(n_inputs) % N_BASES
        slot = np.arange(n_inputs) // N_BASES
        self.offset = slot * WINDOW_STRIDE * self.m + self.base_of * 37       # distinct offsets, also between bases
        self.base_len = blocks * self.bs + int(self.offset.max()) + 1

    def key(self):
        return (self.fs, self.u8, self.n_inputs, self.blocks)

    def window(self, bases, i: int) -> np.ndarray:
        o = int(self.offset[i])
        return bases[self.base_of[i]][o:o + self.blocks * self.bs]


def make_base(fs: int, u8: bool, k: int, n: int) -> np.ndarray:
    """Base capture k of a pool, n samples, [n, 2] u8 or float32 (deterministic)."""
    kind, kw = BASES[k]
    gen = synth.fm_capture if kind == "plain" else synth.fm_capture_realistic
    iq = gen(n, fs=float(fs), channel=k + 1, **kw)["iq"]
    return synth.to_u8(iq) if u8 else synth.to_cf32(iq)


_BASE_CACHE: dict = {}


def _base(fs, u8, k, n):
    key = (fs, u8, k, n)
    if key not in _BASE_CACHE:
        _BASE_CACHE.clear()                 # (a worker holds one base at a time: tasks are grouped by base)
        _BASE_CACHE[key] = make_base(fs, u8, k, n)
    return _BASE_CACHE[key]


def _run_one(x: np.ndarray, fs: int, u8: bool, blocks: int, read_at, full_streams, ctl, coeffs) -> dict:
    """One pool input through the oracle, block by block: the rows of the blocks in read_at (audio, pll_dt, RDS symbols, Manchester bytes),
    every block's Manchester bytes, and the whole-run arrays of full_streams."""
    bs = block_size(fs)
    d = O.Demod(bs, fs)
    if ctl is not None:
        d.set_controls(oracle_controls(ctl))
    if coeffs is not None:
        d.set_coeffs(O.Coeffs.from_buffer_copy(coeffs))
    rows, by_blocks, full = {}, [], {k: [] for k in full_streams}
    for b in range(blocks):
        blk = x[b * bs:(b + 1) * bs]
        assert (d.process_u8(blk) if u8 else d.process_cf32(blk)) == 0
        syms = d.get("rds_sym")
        assert syms.size == d.L.fmo_rds_symbol_count(d.h)
        by = np.frombuffer(d.manchester(syms), np.uint8)
        by_blocks.append(by)
        if b in read_at:
            rows[b] = dict(audio=d.get("audio"), pll=d.get("pll_dt"), syms=syms, by=by)
        for k in full_streams:
            full[k].append(d.get(k))
    return dict(rows=rows, bytes=by_blocks, full={k: np.concatenate(v) for k, v in full.items()})


def _oracle_task(task):
    """Worker: every listed input of one base.  Runs in a spawned process: numpy, synth and oraclelib only."""
    assert "torch" not in sys.modules, "a pool worker imported torch"
    (fs, u8, blocks, k, base_len, items, read_at, full_streams) = task
    base = _base(fs, u8, k, base_len)
    bs = block_size(fs)
    t0 = time.process_time()
    out = [(i, _run_one(base[off:off + blocks * bs], fs, u8, blocks, read_at, full_streams, ctl, coeffs)) for (i, off, ctl, coeffs) in items]
    return out, time.process_time() - t0, "torch" in sys.modules


def executor(max_workers: int | None = None) -> cf.ProcessPoolExecutor:
    n = max_workers or min(os.cpu_count() or 1, 16)
    return cf.ProcessPoolExecutor(max_workers=n, mp_context=mp.get_context("spawn"))


def run_oracle(pool: Pool, ex, mixed: bool = False, coeffs=None, read_at=READ_AT, full_streams=(), on_result=None):
    """Run every input of `pool` through the oracle on the executor `ex`, one task per base.  coeffs: {controls tuple or None: bytes of an
    fmd_coeffs} — the library's coefficients for those controls (None: the oracle designs its own).  on_result(i, result) sees each
    input's result as it arrives (and may drop its whole-run arrays); returns ({i: result}, CPU seconds of the workers)."""
    O.lib()                 # (builds oracle/liboracle.so here if it is missing or stale, not in several workers at once)
    tasks = []
    for k in range(N_BASES):
        items = []
        for i in np.flatnonzero(pool.base_of == k):
            ctl = ctl_of(int(i), mixed)
            items.append((int(i), int(pool.offset[i]), ctl, None if coeffs is None else coeffs[ctl]))
        tasks.append((pool.fs, pool.u8, pool.blocks, k, pool.base_len, items, tuple(read_at), tuple(full_streams)))
    res, cpu = {}, 0.0
    for fut in cf.as_completed([ex.submit(_oracle_task, t) for t in tasks]):
        out, t, torch_seen = fut.result()
        assert not torch_seen, "a pool worker imported torch"
        cpu += t
        for i, r in out:
            if on_result is not None:
                on_result(i, r)
            res[i] = r
    return res, cpu


class Expected:
    """Per read block, the rows every pool input must produce, as [P, ...] arrays (ragged rows zero-padded): audio, pll, cnt, syms, bc, by."""

    def __init__(self, fs: int, n_inputs: int, read_at):
        self.fs, self.n_inputs = fs, n_inputs
        self.rows = {}
        self.read_at = tuple(read_at)
        self.bytes = [[] for _ in range(n_inputs)]      # every block's Manchester bytes, per input

    def set_row(self, b, i, audio, pll, syms, by):
        if b not in self.rows:
            w, cap = n_rds(self.fs), bytes_cap(self.fs)
            self.rows[b] = dict(audio=np.zeros((self.n_inputs,) + np.shape(audio), np.float32), pll=np.zeros((self.n_inputs, np.size(pll)), np.float32),
                                cnt=np.zeros(self.n_inputs, np.int32), syms=np.zeros((self.n_inputs, w), np.float32),
                                bc=np.zeros(self.n_inputs, np.int32), by=np.zeros((self.n_inputs, cap), np.uint8))
        r = self.rows[b]
        r["audio"][i] = audio
        r["pll"][i] = np.reshape(pll, -1)
        r["cnt"][i] = len(syms)
        r["syms"][i, :len(syms)] = syms
        r["bc"][i] = len(by)
        r["by"][i, :len(by)] = by

    @classmethod
    def from_oracle(cls, fs: int, n_inputs: int, results: dict, read_at=READ_AT):
        e = cls(fs, n_inputs, read_at)
        for i, r in results.items():
            for b in read_at:
                row = r["rows"][b]
                e.set_row(b, i, row["audio"], row["pll"], row["syms"], row["by"])
            e.bytes[i] = list(r["bytes"])
        return e

    def gather(self, b, idx) -> dict:
        """The rows a batch with map idx must produce at block b (what a correct kernel's host read returns, padding aside)."""
        return {k: v[idx] for k, v in self.rows[b].items()}


STREAMS = ("audio", "pll", "cnt", "syms", "by")


def check_block(exp: Expected, b: int, got: dict, idx: np.ndarray, chunk: int = 2048) -> dict:
    """Compare every station's row of block b with the expected row of its input.  got: audio [C, ...], pll [C, w], cnt [C], syms [C, >= max cnt],
    bc [C], by [C, >= max bc].  Returns {stream: bool [C] — station differs}."""
    n = idx.size
    bad = {k: np.zeros(n, bool) for k in STREAMS}
    rows = exp.rows[b]
    for lo in range(0, n, chunk):
        s = slice(lo, min(n, lo + chunk))
        e = {k: v[idx[s]] for k, v in rows.items()}
        for k in ("audio", "pll"):
            g = np.ascontiguousarray(got[k][s]).reshape(e[k].shape[0], -1)
            bad[k][s] = (g.view(np.uint32) != e[k].reshape(g.shape[0], -1).view(np.uint32)).any(axis=1)
        bad["cnt"][s] = got["cnt"][s] != e["cnt"]
        bc_bad = got["bc"][s] != e["bc"]
        for k, ck, same_n in (("syms", "cnt", ~bad["cnt"][s]), ("by", "bc", ~bc_bad)):
            w = e[k].shape[1]
            g = np.ascontiguousarray(got[k][s][:, :w])
            mask = np.arange(w)[None, :] < e[ck][:, None]
            gv, ev = (g.view(np.uint32), e[k].view(np.uint32)) if k == "syms" else (g, e[k])
            bad[k][s] = ((gv != ev) & mask).any(axis=1) | ~same_n
    return bad


def describe(exp: Expected, b: int, got: dict, idx: np.ndarray, bad: dict, label: str = "", n_examples: int = 6) -> str:
    """Name what the wrong rows are: for each station that differs, the pool input whose expected output its row DOES equal (audio or pll
    row), and the nearest station given that input — the offset a kernel read or wrote the wrong station's data at."""
    flagged = np.zeros(idx.size, bool)
    for v in bad.values():
        flagged |= v
    stations = np.flatnonzero(flagged)
    if stations.size == 0:
        return f"{label}block {b}: every station equals its input's expected output"
    lines = [f"{label}block {b}: {stations.size} of {idx.size} stations differ from their own input's expected output "
             f"({', '.join(f'{k}: {int(v.sum())}' for k, v in bad.items())})"]
    lookup = {}
    for k in ("audio", "pll"):
        rows = exp.rows[b][k].reshape(exp.n_inputs, -1)
        lookup[k] = {rows[j].tobytes(): j for j in range(exp.n_inputs)}
    given = collections.defaultdict(list)
    for c, j in enumerate(idx):
        given[int(j)].append(c)
    offsets = collections.Counter()       # (station given the input a wrong row belongs to) - (station holding the row), every such pair
    unexplained = 0
    examples = []
    for c in stations:
        hit = None
        for k in ("audio", "pll"):
            row = np.ascontiguousarray(got[k][c]).reshape(-1)
            hit = lookup[k].get(row.tobytes())
            if hit is not None:
                break
        streams = [k for k, v in bad.items() if v[c]]
        owners = np.asarray(given.get(hit, []) if hit is not None else [], np.int64)
        if hit is None:
            unexplained += 1
        offsets.update((owners - c).tolist())
        if len(examples) < n_examples:
            examples.append(f"station {c} (input {idx[c]}): {streams} differ; " + (
                "its rows equal no pool input's output" if hit is None else
                f"its {k} row is input {hit}'s output, given to stations {owners[:8].tolist()}{'...' if owners.size > 8 else ''}"))
    if offsets:
        top, n_top = offsets.most_common(1)[0]
        lines.append(f"  {n_top} of the {stations.size} wrong rows are the output of the input given to the station {top:+d} away "
                     f"(next most common offsets: {', '.join(f'{d:+d} ({n})' for d, n in offsets.most_common(4)[1:])})")
        if top != 0 and n_top >= stations.size // 2:
            lines.append(f"  station c carries station c{top:+d}'s data: an indexing error at a stride of {abs(top)} stations")
        elif top == 0:
            lines.append("  most hold their own input's audio / pll row: the difference is in the RDS rows or counts")
    if unexplained:
        lines.append(f"  {unexplained} wrong rows equal no pool input's output")
    lines += ["  " + s for s in examples]
    return "\n".join(lines)
