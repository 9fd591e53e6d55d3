"""Control changes between blocks, per station (TEST INFRASTRUCTURE; importable without a GPU).

A SCHEDULE is a list of events `(block, station, {field: value})`.  An event takes effect on the block it names (include/fmdemod.h:
fmd_set_controls applies "at the next block boundary", so the call is made after block - 1 and before block).  The fields are those of
fmd_controls; a station's event changes the named fields and leaves its others as they are.  Station -1 is fmd_set_controls' channel
-1: EVERY station gets the same structure, the defaults with the named fields changed.  Events of one block apply in list order.

Two drivers with one signature step a schedule through block by block and return, per stream, per station, one array per block:

  run_oracle   one oraclelib demodulator per station; before block b the station's events through set_controls, then (unless
               coeffs is None) set_coeffs with the library's coefficients for the controls now in force — fmo_set_coeffs switches the
               oracle's own designers off, so the pair is set again after every event
  run_gpu      one BatchDemod; exact or tolerance mode, pipelined or not, through process (numpy), process (torch tensor) or submit

Also here: the schedules S1-S5 of tests/test_gpu_controls_midstream.py and tests/test_oracle_vs_ref.py, and their form as arguments
of oracle/ref_dump.cpp.
"""
from __future__ import annotations

import numpy as np

import oraclelib as O
from gpu_parity import STREAMS, lib_coeffs_to_oracle

FIELDS = ("audio_out", "audio_stereo_mix_factor", "use_deemphasis", "deemphasis_tus", "lpr_cutoff_hz", "lmr_cutoff_hz")
LPR, LMR, STEREO = 0, 1, 2
EXTRA = ["rds_sym", "rds_count", "rds_bytes"]


def defaults() -> dict:
    c = O.default_controls()
    return {k: getattr(c, k) for k in FIELDS}


def timeline(schedule, n_ch: int, n_blocks: int):
    """(calls, in_force): calls[b] = the set_controls calls in front of block b as (station, all six fields), in order;
    in_force[b][c] = station c's fields while block b runs."""
    cur = [defaults() for _ in range(n_ch)]
    calls, in_force = [], []
    for b in range(n_blocks):
        here = []
        for blk, st, fields in schedule:
            if blk != b:
                continue
            assert -1 <= st < n_ch and set(fields) <= set(FIELDS), (blk, st, fields)
            if st < 0:
                full = {**defaults(), **fields}
                cur = [dict(full) for _ in range(n_ch)]
            else:
                cur[st].update(fields)
                full = dict(cur[st])
            here.append((st, full))
        calls.append(here)
        in_force.append([dict(c) for c in cur])
    assert all(0 <= blk < n_blocks for blk, _, _ in schedule), "an event names a block the run does not have"
    return calls, in_force


def touched(schedule, n_ch: int) -> set:
    """The stations a schedule has an event for."""
    return set(range(n_ch)) if any(st < 0 for _, st, _ in schedule) else {st for _, st, _ in schedule}


def remapped(schedule, block_map: dict) -> list:
    """The same events on other blocks (block_map: old block -> new block, ascending)."""
    return [(block_map[b], st, f) for b, st, f in schedule]


def station_schedule(schedule, station: int) -> list:
    """One station's events as a one-station schedule (station 0); the schedule must hold no channel -1 event."""
    assert all(st >= 0 for _, st, _ in schedule)
    return [(b, 0, f) for b, st, f in schedule if st == station]


def _fill(ctl, fields: dict):
    for k, v in fields.items():
        setattr(ctl, k, v)
    return ctl


def run_oracle(caps: np.ndarray, block_size: int, fs: int, schedule, coeffs=None, streams=None) -> dict:
    """caps [C, n, 2] float32 or uint8.  coeffs: None (the oracle designs its own filters: its update_filters runs) or
    coeffs[b][c], the library's fmd_coeffs for station c in block b (run_gpu's "coeffs").
    -> {stream: [station][block] array}, stream over gpu_parity.STREAMS (or `streams`) + rds_sym, rds_count, rds_bytes."""
    n_ch, nb = caps.shape[0], caps.shape[1] // block_size
    u8 = caps.dtype == np.uint8
    calls, _ = timeline(schedule, n_ch, nb)
    names = list(streams) if streams is not None else list(STREAMS)
    out = {k: [[] for _ in range(n_ch)] for k in names + EXTRA}
    for c in range(n_ch):
        d = O.Demod(block_size, fs)
        for b in range(nb):
            changed = False
            for st, full in calls[b]:
                if st in (c, -1):
                    d.set_controls(_fill(O.Controls(), full))
                    changed = True
            if coeffs is not None and (changed or b == 0):
                d.set_coeffs(lib_coeffs_to_oracle(coeffs[b][c]))
            blk = caps[c, b * block_size:(b + 1) * block_size]
            assert (d.process_u8(blk) if u8 else d.process_cf32(blk)) == 0
            for k in names:
                out[k][c].append(d.get(k))
            sym = d.get("rds_sym")
            if "rds_sym" not in names:
                out["rds_sym"][c].append(sym)
            out["rds_count"][c].append(int(d.L.fmo_rds_symbol_count(d.h)))
            out["rds_bytes"][c].append(np.frombuffer(d.manchester(sym), dtype=np.uint8))
    return out


def run_gpu(pkg, caps: np.ndarray, block_size: int, fs: int, schedule, fast_math: bool = False, pipelined: bool = True,
            entry: str = "process", streams=None, pairing=None, reset_after=None) -> dict:
    """The same run on the library.  entry: "process" (numpy, host entry point), "torch" (process with a device tensor) or "submit".
    pairing: set_extract_pairing's mode.  reset_after: reset() behind that block (the controls stay; later events still apply).
    -> as run_oracle, plus "coeffs"[block][station] (get_coeffs behind that block's set_controls calls) and, in the tolerance mode, "pll_poly"."""
    from fm_radio_amd.capi import Controls
    n_ch, nb = caps.shape[0], caps.shape[1] // block_size
    calls, _ = timeline(schedule, n_ch, nb)
    dm = pkg.BatchDemod(n_ch, block_size, fs, keep_taps=True, fast_math=fast_math, pipelined=pipelined)
    if pairing is not None:
        dm.set_extract_pairing(pairing)
    names = list(streams) if streams is not None else list(STREAMS)
    out = {k: [[] for _ in range(n_ch)] for k in names + EXTRA}
    out["coeffs"] = []
    if entry != "process":
        import torch
    for b in range(nb):
        for st, full in calls[b]:
            dm.set_controls(_fill(Controls(), full), st)
        out["coeffs"].append([dm.get_coeffs(c) for c in range(n_ch)] if calls[b] or b == 0 else out["coeffs"][-1])
        blk = np.ascontiguousarray(caps[:, b * block_size:(b + 1) * block_size])
        if entry == "process":
            assert dm.process(blk) == 0
        else:
            t = torch.from_numpy(blk).cuda()
            assert (dm.submit(t) if entry == "submit" else dm.process(t)) == 0
            if entry == "submit":
                dm.synchronize()
        syms, counts = dm.rds_symbols()
        by, bc = dm.rds_bytes()
        got = {k: dm.audio().reshape(n_ch, -1) if k == "audio" else dm.stream(k) for k in names}
        for c in range(n_ch):
            for k in names:
                a = got[k][c]
                if k == "rds_raw_sym":              # only the first counts[c] symbols of a row are valid
                    a = a.reshape(-1, 2)[:counts[c]].reshape(-1)
                out[k][c].append(np.array(a, np.float32))
            out["rds_sym"][c].append(syms[c, :counts[c]].copy())
            out["rds_count"][c].append(int(counts[c]))
            out["rds_bytes"][c].append(by[c, :bc[c]].copy())
        if reset_after == b:
            dm.reset()
    dm.close()
    return out


def joined(res: dict, k: str, c: int) -> np.ndarray:
    """Station c's stream k, its blocks concatenated."""
    v = res[k][c]
    return np.asarray(v, np.int32) if k == "rds_count" else (np.concatenate(v) if len(v) else np.zeros(0, np.float32))


def differences(a: dict, b: dict, stations, keys=None, blocks=None) -> list:
    """Every (station, stream, block) at which two runs are not bit-identical, described (conftest.describe_diff)."""
    from conftest import bits_equal, describe_diff
    bad = []
    for k in (keys if keys is not None else [k for k in a if k != "coeffs" and k in b]):
        for c in stations:
            for blk in (blocks if blocks is not None else range(len(a[k][c]))):
                x, y = a[k][c][blk], b[k][c][blk]
                if k == "rds_count":
                    if x != y:
                        bad.append((c, k, blk, f"{x} vs {y}"))
                elif not bits_equal(np.asarray(x), np.asarray(y)):
                    bad.append((c, k, blk, describe_diff(np.asarray(x), np.asarray(y))))
    return bad


# ---- the schedules (six stations, twelve blocks) ---------------------------------------------------------------------------------
ON, OFF = dict(use_deemphasis=1), dict(use_deemphasis=0)

S1 = [  # cut-offs
    (3, 1, dict(lpr_cutoff_hz=9000)), (6, 1, dict(lpr_cutoff_hz=15000)),
    (3, 2, dict(lmr_cutoff_hz=5000)),
    (7, 4, dict(lpr_cutoff_hz=11000, lmr_cutoff_hz=7000)),
]
S2 = [  # mixing
    (2, 0, dict(audio_out=LPR)), (4, 0, dict(audio_out=LMR)), (6, 0, dict(audio_out=STEREO)),
    (5, 3, dict(audio_stereo_mix_factor=0.65)), (6, 3, dict(audio_stereo_mix_factor=0.2)),
]
S3 = [  # de-emphasis: the IIR state stays frozen while the filter is off and the filter resumes from it
    (2, 0, dict(use_deemphasis=1, deemphasis_tus=50)), (4, 0, OFF), (7, 0, ON),
    (0, 1, dict(use_deemphasis=1, deemphasis_tus=75)),
    (0, 2, dict(use_deemphasis=1, deemphasis_tus=50)), (5, 2, dict(deemphasis_tus=75)),
    (3, 3, dict(deemphasis_tus=50)), (8, 3, ON),
    (0, 4, dict(deemphasis_tus=50)), (6, 4, ON), (7, 4, OFF),
]
S4 = [  # the last one leaves: block 5 is the block the serial stage lingers for
    (0, 0, dict(use_deemphasis=1, deemphasis_tus=50)), (0, 1, dict(use_deemphasis=1, deemphasis_tus=75)),
    (3, 0, OFF), (5, 1, OFF),
    (6, 2, dict(lpr_cutoff_hz=10000)),
    (7, 0, ON),
]
S4B = [(5, st, f) if (blk, st) == (6, 2) else (blk, st, f) for blk, st, f in S4]       # ... with the cut-off change ON the linger block
S5 = [  # the call itself
    (2, 1, dict(lpr_cutoff_hz=7000)), (2, 1, dict(lpr_cutoff_hz=12000, audio_stereo_mix_factor=0.5)),      # twice before one block: the last call wins
    (3, 1, dict(lpr_cutoff_hz=12000)),                                                                         # the values already in force
    (3, 5, {}),                                                                                                # ... on an untouched station too
    (4, -1, dict(use_deemphasis=1, deemphasis_tus=50, lmr_cutoff_hz=12000)),                                   # every station
    (5, 2, dict(use_deemphasis=0, lmr_cutoff_hz=15000)),
]
SCHEDULES = {"S1": S1, "S2": S2, "S3": S3, "S4": S4, "S4b": S4B}
N_STATIONS, N_BLOCKS = 6, 12


def ref_args(schedule) -> list:
    """A one-station schedule as oracle/ref_dump.cpp's arguments (events of block 0 in front of the first at=)."""
    audio = {LPR: "lpr", LMR: "lmr", STEREO: "stereo"}
    fmt = {"audio_out": lambda v: f"audio={audio[v]}", "audio_stereo_mix_factor": lambda v: f"mix={v!r}",
           "use_deemphasis": lambda v: "deemph=on" if v else "deemph=off", "deemphasis_tus": lambda v: f"tus={v}",
           "lpr_cutoff_hz": lambda v: f"lpr={v}", "lmr_cutoff_hz": lambda v: f"lmr={v}"}
    args, at = [], 0
    for blk, st, fields in sorted(schedule, key=lambda e: e[0]):
        assert st == 0
        if blk != at:
            args.append(f"at={blk}")
            at = blk
        args += [fmt[k](v) for k, v in fields.items()]
    return args
