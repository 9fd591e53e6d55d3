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


# ---- the block plan: each stage's kernel form and launch geometry (fmd_debug_block_plan) ------------------------------------------------------------

BLOCK_KS = tuple(range(1, 71)) + (128, 1024)          # block = 1024 m k samples: every tile count up to 70 front tiles, and two long ones (n_est > 512)
BLOCK_STATIONS = (1, 2, 3) + tuple(t + d for t in (384, 768, 1024, 1536, 1792, 3071, 3072, 6144, 12288) for d in (-2, -1, 0, 1, 2))
DEEMPH = ((0, 0), (0, 1), (1, 0))                     # (any_deemph, deemph_in_tile): no de-emphasis, inside the front tile, as a stage


def test_the_binding_names_the_block_plan_fields_in_the_model_s_order(pkg):
    assert tuple(n for n, _ in pkg.BlockPlanInfo._fields_) == M.BLOCK_FIELDS
    assert tuple(n for n, _ in pkg.PlanFacts._fields_) == ("any_deemph", "deemph_in_tile", "split_front", "uniform_cutoffs", "extract_pairing")


def test_block_plan_against_the_model_and_its_invariants(pkg):
    """fmd_debug_block_plan against tests/plan_model.py over the whole product — rate x cf32 / u8 x mode x FMD_FLAG_KEEP_TAPS x block length x de-emphasis (none, in
    the tile, as a stage) x fmd_debug_split_front x equal cut-offs x pairing mode x station count — and, on the library's answer alone, what any plan must
    satisfy: tiles divide the stream they tile and cover it exactly once, nt fits its 15 bits, paired and unpaired grids are what k_extract_bp indexes by,
    the first decimator is a stage exactly when the front end does not take the capture, and the interleaved streams are left out only where nothing reads
    them."""
    lib, F = pkg.load_library(), M.BLOCK_FIELDS
    out, facts = pkg.BlockPlanInfo(), pkg.PlanFacts()
    view = (C.c_int * len(F)).from_buffer(out)
    i_ = {n: k for k, n in enumerate(F)}
    (I_IQ, I_FK, I_FT, I_FW, I_PK, I_PT, I_PW, I_ET, I_BP, I_NT, I_PAIR, I_GRID) = (i_[n] for n in (
        "iq_streams", "front_kernel", "front_tile", "front_workgroups", "predecim_kernel", "predecim_tile", "predecim_workgroups", "extract_tile", "extract_bp", "extract_nt",
        "extract_pair", "extract_grid_x"))
    checked = 0
    for fs, u8, fast, keep, k in itertools.product((K256, K1024, K2048), (False, True), (0, M.FAST_MATH), (0, M.KEEP_TAPS), BLOCK_KS):
        m, flags = fs // K256, fast | keep
        bs = 1024 * m * k
        n_in, n_fo, n_au = bs // m, bs // m // 2, bs // m // 8
        for n in BLOCK_STATIONS:
            cfg = pkg.Config(n, bs, fs, -1, flags)
            for (any_de, in_tile), split, uniform, pairing in itertools.product(DEEMPH, (0, 1), (0, 1), (0, 1, 2)):
                facts.any_deemph, facts.deemph_in_tile, facts.split_front, facts.uniform_cutoffs, facts.extract_pairing = any_de, in_tile, split, uniform, pairing
                assert lib.fmd_debug_block_plan(C.byref(cfg), C.byref(facts), u8, C.byref(out)) == 0
                g = tuple(view)
                want = M.block_plan(n, fs, bs, flags, u8, bool(any_de), bool(in_tile), bool(split), bool(uniform), pairing)
                assert g == want, (n, bs, fs, flags, u8, any_de, in_tile, split, uniform, pairing, dict(zip(F, g)), dict(zip(F, want)))
                # invariants, from the answer alone
                assert n_fo % g[I_FT] == 0 and g[I_FW] * g[I_FT] == n_fo * n
                assert n_au % g[I_ET] == 0
                takes_capture = m == 1 or g[I_FK] == M.K_FRONT_PRE_MFMA
                assert (g[I_PK] == M.NO_PREDECIM) == takes_capture
                if not takes_capture:
                    assert n_in % g[I_PT] == 0 and g[I_PW] * g[I_PT] == n_in * n
                if g[I_BP]:
                    tiles = n_au // g[I_ET]
                    assert 1 <= g[I_NT] <= 0x7fff
                    if g[I_PAIR]:
                        assert g[I_GRID] == (n + 1) // 2 and 4 * g[I_NT] >= 2 * tiles
                    else:
                        assert g[I_GRID] == -(-tiles // (4 * g[I_NT])) * n and (g[I_GRID] >= 1536 or g[I_NT] == 1)
                else:
                    assert not g[I_PAIR] and g[I_GRID] * g[I_ET] == n_au * n
                assert g[I_IQ] == int(not (fast and not keep and n_fo % 1024 == 0))
                checked += 1
    assert checked == 3 * 2 * 2 * 2 * len(BLOCK_KS) * len(BLOCK_STATIONS) * 36


def test_what_the_block_plan_hook_refuses(pkg):
    lib = pkg.load_library()
    ok, facts, out = pkg.Config(12, 16384, K256, -1, 0), pkg.PlanFacts(), pkg.BlockPlanInfo()
    assert lib.fmd_debug_block_plan(C.byref(ok), C.byref(facts), 0, C.byref(out)) == 0
    assert lib.fmd_debug_block_plan(C.byref(ok), None, 0, C.byref(out)) == -1 and lib.fmd_debug_block_plan(C.byref(ok), C.byref(facts), 0, None) == -1
    assert lib.fmd_debug_block_plan(C.byref(pkg.Config(12, 10240, K1024, -1, 0)), C.byref(facts), 0, C.byref(out)) == -1      # no multiple of 1024 m
    facts.extract_pairing = 3
    assert lib.fmd_debug_block_plan(C.byref(ok), C.byref(facts), 0, C.byref(out)) == -1


def test_seam_geometry_agrees_with_the_block_plan(pkg):
    """tests/seam_stats.geometry keeps its own arithmetic (it is the independent side of tests/test_gpu_fast_seams.py); for every configuration that test runs,
    its front tile, extract tile and first-decimator period are the plan's."""
    import seam_stats as S
    import test_gpu_fast_seams as T
    for name, f in T.FORMS.items():
        u8, deemph, split = f.get("u8", False), f.get("deemph", False), f.get("split_front", False)
        geo = S.geometry(f["fs"], f["bs"], u8, deemph, split, n_ch=f["n_ch"])
        facts = pkg.PlanFacts(0, int(deemph), int(split), 1, 0)         # (50 us on every station: inside the front tile)
        got = pkg.block_plan(pkg.Config(f["n_ch"], f["bs"], f["fs"], -1, M.FAST_MATH), facts, u8)
        assert (geo["front_tile"], geo["extract_tile"]) == (got.front_tile, got.extract_tile), name
        assert geo["fm_out_iq"]["periods"].get("predecim", 0) == got.predecim_tile // 2, name
    # cf32 captures get 2048-output tiles from 12288 such workgroups on, at any batch size
    for n_ch, want in ((3071, 1024), (3072, 2048)):
        assert S.geometry(K256, 16384, n_ch=n_ch)["front_tile"] == want == pkg.block_plan(pkg.Config(n_ch, 16384, K256, -1, M.FAST_MATH)).front_tile


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
