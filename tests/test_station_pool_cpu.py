"""CPU self-check of the every-station harness (tests/station_pool.py), no GPU.

A kernel that reads or writes station c + s's row instead of station c's is what the large-batch tests must catch.  Station rows shifted by
s are made from the oracle's expectations and handed to the checker: with the pool map (509 distinct inputs, drawn at random) it flags
every station but the few that share an input with their neighbour s away, at every stride; with the tiled map of the older large-batch
tests (station c given capture c % 8) it flags none at a stride that is a multiple of 8 — those tests could not see such a bug.
"""
import sys

import numpy as np
import pytest

import station_pool as SP

N_STATIONS = 4096
SHIFTS = (1, 2, 4, 8, 64, 256, 512, 2048)
FS = 256_000
READ = 5          # (6 blocks are enough here: the checker compares whatever rows it is given, Manchester bytes included)


@pytest.fixture(scope="module")
def expected():
    pool = SP.Pool(FS, u8=False, blocks=READ + 1)
    with SP.executor() as ex:
        res, cpu = SP.run_oracle(pool, ex, read_at=(READ,))
    print(f"oracle: {pool.n_inputs} inputs x {pool.blocks} blocks, {cpu:.1f} CPU-s in the workers")
    return SP.Expected.from_oracle(FS, pool.n_inputs, res, read_at=(READ,))


def _shifted(exp, idx, s):
    """What a batch returns when every station c carries station (c + s) mod C's outputs."""
    got = exp.gather(READ, np.roll(idx, -s))
    return got


def test_pool_inputs_are_distinct(expected):
    audio = expected.rows[READ]["audio"].reshape(SP.P, -1)
    assert len({r.tobytes() for r in audio}) == SP.P
    pll = expected.rows[READ]["pll"]
    assert len({r.tobytes() for r in pll}) == SP.P
    assert (expected.rows[READ]["cnt"] > 0).all() and (expected.rows[READ]["bc"] > 0).all()


def test_unshifted_rows_pass(expected):
    idx = SP.station_map(N_STATIONS)
    bad = SP.check_block(expected, READ, _shifted(expected, idx, 0), idx)
    assert not any(v.any() for v in bad.values())
    assert np.bincount(idx, minlength=SP.P).min() >= N_STATIONS // SP.P        # every input in use


@pytest.mark.parametrize("s", SHIFTS)
def test_pool_map_catches_every_shift(expected, s):
    idx = SP.station_map(N_STATIONS)
    got = _shifted(expected, idx, s)
    bad = SP.check_block(expected, READ, got, idx)
    flagged = np.zeros(N_STATIONS, bool)
    for v in bad.values():
        flagged |= v
    assert flagged.mean() >= 0.99, (s, flagged.mean())
    msg = SP.describe(expected, READ, got, idx, bad)
    assert f"station c{s:+d}'s data" in msg or f"stride of {s} stations" in msg, msg


@pytest.mark.parametrize("s", SHIFTS)
def test_tiled_map_is_blind_to_multiples_of_its_tile_count(expected, s):
    """The map of test_gpu_scale's _tiled_run: 8 captures over the batch."""
    idx = np.arange(N_STATIONS) % 8
    bad = SP.check_block(expected, READ, _shifted(expected, idx, s), idx)
    flagged = np.zeros(N_STATIONS, bool)
    for v in bad.values():
        flagged |= v
    if s % 8 == 0:
        assert not flagged.any(), s
    else:
        assert flagged.all(), s


def test_a_single_wrong_rds_symbol_is_caught(expected):
    idx = SP.station_map(N_STATIONS)
    got = _shifted(expected, idx, 0)
    c = 3001
    got["syms"][c, int(got["cnt"][c]) - 1] += np.float32(1e-6)
    got["by"][c + 1, 0] ^= 1
    got["cnt"][c + 2] -= 1
    bad = SP.check_block(expected, READ, got, idx)
    assert np.flatnonzero(bad["syms"]).tolist() == [c, c + 2]
    assert np.flatnonzero(bad["by"]).tolist() == [c + 1]
    assert np.flatnonzero(bad["cnt"]).tolist() == [c + 2]
    assert not bad["audio"].any() and not bad["pll"].any()


def test_pool_is_deterministic():
    a, b = SP.Pool(FS, u8=True), SP.Pool(FS, u8=True)
    assert np.array_equal(a.offset, b.offset) and np.array_equal(a.base_of, b.base_of)
    pairs = set(zip(a.base_of.tolist(), a.offset.tolist()))
    assert len(pairs) == SP.P                                                  # every input a window of its own
    assert np.array_equal(SP.station_map(4097), SP.station_map(4097))
    assert [SP.ctl_of(i, True) for i in range(SP.P)] == [SP.ctl_of(i, True) for i in range(SP.P)]
    mixed = sum(SP.ctl_of(i, True) is not None for i in range(SP.P))
    assert 0.35 * SP.P < mixed < 0.65 * SP.P
    assert {SP.ctl_of(i, True) for i in range(SP.P)} == set(SP.CONTROL_SET) | {None}
    k = 5
    x1 = SP.make_base(FS, True, k, 40_000)
    x2 = SP.make_base(FS, True, k, 40_000)
    assert np.array_equal(x1, x2)
    m = SP.station_map(4096)
    for s in (1, 8, 64, 256):           # duplicates fall at no fixed stride: a station shares its input with its neighbour s away rarely
        assert (m == np.roll(m, -s)).mean() < 0.01, s


def test_spawned_worker_does_not_import_torch():
    """The worker asserts it and reports it; the parent may well have torch loaded."""
    pool = SP.Pool(FS, u8=False, n_inputs=SP.N_BASES, blocks=1)
    with SP.executor(2) as ex:
        res, _ = SP.run_oracle(pool, ex, read_at=(0,))
        assert sorted(res) == list(range(SP.N_BASES))
        ok = ex.submit(_torch_in_worker).result()
    assert ok is False


def _torch_in_worker():
    return "torch" in sys.modules
