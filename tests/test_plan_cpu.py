"""CPU-only: which kernels a configuration gets (fm-radio_amd/csrc/fmd_plan.h through fmd_debug_plan, no GPU) against the rules restated in
tests/plan_model.py, and the batch sizes of tests/test_gpu_every_station.py against the switches they are there for: a threshold that moves
fails here until the case moves with it."""
import ctypes as C
import itertools

import pytest

import fmradio_loader
import plan_model as M

K256, K1024, K2048 = 256_000, 1_024_000, 2_048_000
SELECTORS = (0, M.PLL_TIME_PARALLEL, M.PLL_LOW_WORK, M.PLL_K8, M.PLL_TIME_PARALLEL | M.PLL_K8, M.PLL_STREAM_ORDER)


@pytest.fixture(scope="module")
def pkg():
    p = fmradio_loader.load()
    p.build_library()
    p.load_library()
    return p


def _got(pkg, n, bs, fs, flags, thresholds=None, unlocked=False) -> tuple:
    info = pkg.plan(pkg.Config(n, bs, fs, -1, flags), thresholds, unlocked)
    return tuple((C.c_int * len(M.FIELDS)).from_buffer(info))


def _want(n, bs, fs, flags, thresholds=None, unlocked=False) -> tuple:
    return M.plan(n, *M.lengths(fs, bs), flags, thresholds, unlocked)


def test_the_binding_names_the_fields_in_the_model_s_order(pkg):
    assert tuple(n for n, _ in pkg.PlanInfo._fields_) == M.FIELDS
    assert pkg.PLL_KERNELS == ("low-work", 16, 8) and (M.LOW_WORK, M.TIME_PARALLEL_16, M.TIME_PARALLEL_8) == (0, 1, 2)


def test_every_station_count_against_the_model(pkg):
    """Every station count 1 .. 17000 at the three rates, both modes, loops in and out of lock (64 ms blocks, default flags)."""
    for fs, fast, unlocked in itertools.product((K256, K1024, K2048), (0, M.FAST_MATH), (False, True)):
        bs = 16384 * (fs // K256)
        lens = M.lengths(fs, bs)
        for n in range(1, 17001):
            got = _got(pkg, n, bs, fs, fast, None, unlocked)
            assert got == M.plan(n, *lens, fast, None, unlocked), (n, fs, fast, unlocked, dict(zip(M.FIELDS, got)))


def test_every_flag_and_block_length_near_the_switches_against_the_model(pkg):
    """The whole product — rate x mode x FMD_FLAG_KEEP_TAPS x pipelined x FMD_FLAG_PLL_* selector x in / out of lock x block length — at the station counts
    within 3 of every switch (as a station count and as an effective batch) and every 97th in between.  Block lengths: 16384 and 10240 samples at
    256 kSa/s (a block is a multiple of 1024 m samples, so m times as many at the higher rates), and 65536, whose L-R phase estimates no longer fit
    k_extract's inline form."""
    counts = M.stations_to_try(step=97)
    assert {2816, 2817, 3328, 3329, 3584, 3585, 4096, 4097, 6144, 6145, 7168, 7169, 16384, 16385, 1023, 1024, 1792, 1793, 3070, 3071, 1877, 1878, 2731, 2732} <= set(counts)
    checked = 0
    for fs, fast, keep, nopipe, sel, unlocked, bs256 in itertools.product((K256, K1024, K2048), (0, M.FAST_MATH), (0, M.KEEP_TAPS), (0, M.NO_PIPELINE), SELECTORS,
                                                                          (False, True), (16384, 10240, 65536)):
        flags, bs = fast | keep | nopipe | sel, bs256 * (fs // K256)
        lens = M.lengths(fs, bs)
        for n in counts:
            got = _got(pkg, n, bs, fs, flags, None, unlocked)
            assert got == M.plan(n, *lens, flags, None, unlocked), (n, bs, fs, flags, unlocked, dict(zip(M.FIELDS, got)))
        checked += len(counts)
    assert checked > 250_000


@pytest.mark.parametrize("thresholds", [(4, 7168), (4, 4), (2, 7168), (2, 2)])
def test_moved_thresholds_against_the_model(pkg, thresholds):
    """What fmd_debug_pll_adaptive leaves behind, at the batches tests/test_gpu_parity.py moves the thresholds for: adaptive whenever a threshold lies
    below the batch, never the per-wavefront hand-over, the hand-over array as allocated."""
    for n, keep, nopipe, sel, unlocked in itertools.product((5, 12), (0, M.KEEP_TAPS), (0, M.NO_PIPELINE), SELECTORS, (False, True)):
        flags = keep | nopipe | sel
        got = dict(zip(M.FIELDS, _got(pkg, n, 16384, K256, flags, thresholds, unlocked)))
        assert tuple(got.values()) == _want(n, 16384, K256, flags, thresholds, unlocked), (n, flags, unlocked, got)
        assert got["pll_k_adaptive"] == 1 and got["pll_chained"] == 0
        assert got["pll_waves"] == _want(n, 16384, K256, flags)[M.FIELDS.index("pll_waves")]
    k = M.FIELDS.index("pll_kernel")
    calm = {(4, 7168): 8, (4, 4): "low-work", (2, 7168): 8, (2, 2): "low-work"}[thresholds]
    assert pkg.PLL_KERNELS[_got(pkg, 12, 16384, K256, 0, thresholds, False)[k]] == calm
    assert pkg.PLL_KERNELS[_got(pkg, 12, 16384, K256, 0, thresholds, True)[k]] == 16


def test_what_the_hook_refuses(pkg):
    """One threshold without the other, the tolerance mode or more than 4096 effective stations with moved thresholds (fmd_debug_pll_adaptive refuses
    them), and configurations fmd_create refuses."""
    ok = pkg.Config(12, 16384, K256, -1, 0)
    pkg.plan(ok, (4, 4))
    for cfg, th in ((ok, (4, -1)), (ok, (-1, 4)), (pkg.Config(12, 16384, K256, -1, M.FAST_MATH), (4, 4)), (pkg.Config(4097, 16384, K256, -1, 0), (4, 4)),
                    (pkg.Config(2732, 65536, K1024, -1, 0), (4, 4)), (pkg.Config(0, 16384, K256, -1, 0), None), (pkg.Config(12, 10240, K1024, -1, 0), None),
                    (pkg.Config(12, 16384, 48_000, -1, 0), None), (pkg.Config(12, 16384, K256, -1, 1 << 20), None)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.plan(cfg, th)
        assert e.value.status == -1, (cfg.n_channels, th)
    pkg.plan(pkg.Config(2731, 65536, K1024, -1, 0), (4, 4))            # 4096 effective stations: still the hook's range
    assert pkg.load_library().fmd_debug_plan(C.byref(ok), -1, -1, 0, None) == -1


# The cases of tests/test_gpu_every_station.py whose "why" names a switch: (mode, stations, rate) -> (the plan fields that change there, the largest
# station count on the other side).  "pll_kernel" is the kernel while every loop holds lock, "pll_kernel/unlocked" the one while some do not.  A case
# sits on the first count past its switch, with two exceptions that sit on the second: 1025 (1024 is the first on the put-off schedule and with
# the pad, but fills its last wavefront: the case is the first ragged one) and 2733 at 1.024 MSa/s (2731 + 1365 = 4096, 2732 + 1366 = 4098).
AIMED = {
    ("exact", 2817, K256): (("pilot_power_rows",), 2816),
    ("exact", 3329, K256): (("pll_chained",), 3328),
    ("exact", 3585, K256): (("pll_k_adaptive", "pll_kernel"), 3584),
    ("exact", 4097, K256): (("pll_k_adaptive", "pll_kernel/unlocked"), 4096),
    ("exact", 7169, K256): (("pll_k_adaptive", "pll_kernel"), 7168),
    ("exact", 16385, K256): (("pll_k_adaptive",), 16384),
    ("tolerance", 1025, K256): (("lazy_capable", "front_lds_pad"), 1023),
    ("tolerance", 3071, K256): (("extract_auto_pair",), 3070),
    ("tolerance", 6145, K256): (("lmr_inline",), 6144),
    ("exact", 1878, K1024): (("pilot_power_rows",), 1877),
    ("exact", 2733, K1024): (("pll_k_adaptive", "pll_kernel/unlocked"), 2731),
    ("tolerance", 4097, K1024): (("lmr_inline",), 4096),
}
# ... and those that sit inside a range on purpose (the timed configuration, the top of the range)
INSIDE = {("tolerance", 4096, K256), ("tolerance", 16384, K256), ("exact", 4096, K256)}


def _fields(pkg, mode, n, fs) -> dict:
    import station_pool as SP
    flags = M.FAST_MATH if mode == "tolerance" else 0       # (BatchDemod's default flags, as the cases run)
    out = dict(zip(M.FIELDS, _got(pkg, n, SP.block_size(fs), fs, flags)))
    out["pll_kernel/unlocked"] = _got(pkg, n, SP.block_size(fs), fs, flags, None, True)[M.FIELDS.index("pll_kernel")]
    return out


def test_every_station_cases_sit_on_the_switches_they_name(pkg):
    import test_gpu_every_station as E
    keys = {(c[0], c[1], c[2]) for c in E.CASES}
    assert keys == set(AIMED) | INSIDE, keys ^ (set(AIMED) | INSIDE)            # a new case says here what it is aimed at
    assert {k[1] for k in AIMED} >= {2817, 3329, 3585, 4097, 6145, 7169, 16385, 1025, 1878, 2733}
    for (mode, n, fs), (names, below) in AIMED.items():
        assert n - 2 <= below < n
        at, under, other = _fields(pkg, mode, n, fs), _fields(pkg, mode, n - 1, fs), _fields(pkg, mode, below, fs)
        for name in names:
            assert at[name] != other[name], f"{mode} {n} stations at {fs}: {name} is {at[name]} at {below} stations too: the switch has moved"
            assert under[name] == (other if below == n - 1 else at)[name], (mode, n, fs, name)


def test_every_station_cases_get_the_kernels_their_comments_name(pkg):
    """The kernel each exact-mode case's "why" names while every loop holds lock and, where the choice follows what is out of lock, while some do not
    (every batch has pilot-less stations, so both run)."""
    want = {2817: (16, 16), 3329: (16, 16), 3585: (8, 16), 4096: (8, 16), 4097: (8, 8), 7169: ("low-work", 8), 16385: ("low-work", "low-work")}
    for n, (calm, busy) in want.items():
        f = _fields(pkg, "exact", n, K256)
        assert pkg.PLL_KERNELS[f["pll_kernel"]] == calm and f["pll_k_adaptive"] == (calm != busy), n
        if f["pll_k_adaptive"]:
            assert pkg.PLL_KERNELS[f["pll_kernel/unlocked"]] == busy, n
