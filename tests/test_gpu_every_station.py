"""GPU tests (pytest -m gpu): EVERY station of a large batch against its own expected output, at the batch sizes where the library's
kernel selection changes (k_pilot_power's two forms, the pilot-PLL hand-over chain, the time-parallel PLL's 16 / adaptive 8-16 / 8 lanes, the
8-lane adaptive and low-work PLL kernels, the put-off extract stage, the front end's LDS pad, k_extract_bp with two stations per workgroup,
the L-R phase in and out of the extract stage), with a ragged last wavefront, workgroup or station pair.

The large-batch tests of test_gpu_scale.py / test_gpu_parity.py / test_gpu_fast.py tile a few captures over the batch, so a kernel that
reads or writes another station's row at an offset that is a multiple of the tile count passes them.  Here station c is given input idx[c]
of a pool of 509 distinct inputs (tests/station_pool.py; tests/test_station_pool_cpu.py shows the difference), built block by block on the
device, and each case opens one BatchDemod with the default flags (as bench.py does), submits 14 blocks back to back and reads after
blocks 4, 9 and 13 (loops in lock from about block 8).  At each read every station's audio, PLL result (pll_dt; tolerance mode: pll_poly),
RDS symbol count, every symbol value and the Manchester bytes are compared:
  exact mode:     bit-identical to the CPU oracle's run of the station's input (the library's coefficients, the station's controls);
  tolerance mode: bit-identical to the station's input in one small run of the 509 pool inputs (deterministic, independent of the batch),
                  and that small run within the north-star tolerance of the oracle for every input (test_gpu_fast.py's helpers).
Two cases also decode RDS on the GPU (FMD_FLAG_RDS_DECODE): every station's database equals tests/rds_oracle.RdsChain fed that station's bytes.
"""
import time

import numpy as np
import pytest

import station_pool as SP

pytestmark = pytest.mark.gpu

K256, K1024 = 256_000, 1_024_000
# (mode, stations, rate, u8, mixed per-station controls, rds_decode, why), grouped by pool: one pool's inputs are on the device at a time
CASES = [
    ("exact", 2817, K256, True, False, False, "k_pilot_power<false>, one-lane last wavefront"),
    ("exact", 4097, K256, True, False, True, "8-lane time-parallel PLL past 4096, RDS decoder"),
    ("exact", 3329, K256, False, False, False, "no PLL hand-over chain, 16-lane time-parallel PLL"),
    ("exact", 3585, K256, False, False, False, "adaptive 8/16 lanes, pilot-less stations out of lock"),
    ("exact", 7169, K256, False, False, False, "8-lane adaptive PLL past the time-parallel range"),
    ("exact", 16385, K256, False, False, False, "low-work PLL past the 8-lane range"),
    ("tolerance", 1025, K256, False, False, False, "put-off extract stage, LDS pad, ragged"),
    ("tolerance", 3071, K256, False, False, True, "k_extract_bp<2>, half-empty last pair, RDS decoder"),
    ("tolerance", 4096, K256, False, False, False, "configs[2], the timed path"),
    ("tolerance", 6145, K256, False, False, False, "L-R phase out of line (k_lmr_phase)"),
    ("tolerance", 16384, K256, False, False, False, "top of the range"),
    ("exact", 4096, K256, False, True, False, "configs[2], per-station controls"),
    ("tolerance", 3071, K256, False, True, False, "station pairing off (per-station cut-offs)"),
    ("exact", 1878, K1024, False, False, False, "effective 2817 behind k_predecim"),
    ("exact", 2733, K1024, True, False, False, "effective 4099.5 behind k_predecim"),
    ("tolerance", 4097, K1024, True, False, False, "L-R phase out of line at 1.024 MSa/s u8"),
]
MODES_OF = {}
for _m, _n, _fs, _u8, _mx, _r, _w in CASES:
    MODES_OF.setdefault((_fs, _u8, _mx), set()).add(_m)
TOL_STREAMS = ("fm_out_iq", "lpr", "lmr", "audio", "lmr_phase")


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    import torch
    assert torch.cuda.is_available()
    return p


@pytest.fixture(scope="module")
def ex():
    with SP.executor() as e:
        yield e


def _controls(pkg, ctl):
    c = pkg.default_controls()
    for f, v in zip(SP.CONTROL_FIELDS, ctl if ctl is not None else SP.DEFAULT_CONTROLS):
        setattr(c, f, v)
    return c


def _lib_coeffs(pkg, fs, fast, mixed) -> dict:
    """{controls: bytes of the library's fmd_coeffs} for every controls value the pool uses."""
    ctls = [None] + (list(SP.CONTROL_SET) if mixed else [])
    dm = pkg.BatchDemod(len(ctls), SP.block_size(fs), fs, fast_math=fast)
    for ch, ctl in enumerate(ctls):
        dm.set_controls(_controls(pkg, ctl), ch)
    out = {ctl: bytes(dm.get_coeffs(ch)) for ch, ctl in enumerate(ctls)}
    dm.close()
    return out


_INPUTS, _STATE = {}, {}


def _device_inputs(ex, pool):
    """[P, blocks * block_size, 2] on the device: every pool input's window, cut from its base capture there (built on the CPU workers)."""
    import torch
    if pool.key() not in _INPUTS:
        _INPUTS.clear()                         # (one pool's inputs on the device at a time: 0.9 GB, 3.7 GB at 1.024 MSa/s cf32)
        dt = torch.uint8 if pool.u8 else torch.float32
        n = pool.blocks * pool.bs
        w = torch.empty((pool.n_inputs, n, 2), dtype=dt, device="cuda")
        ks = list(range(SP.N_BASES))
        for k, base in zip(ks, ex.map(SP.make_base, [pool.fs] * len(ks), [pool.u8] * len(ks), ks, [pool.base_len] * len(ks))):
            db = torch.from_numpy(base).cuda()
            for i in np.flatnonzero(pool.base_of == k):
                o = int(pool.offset[i])
                w[i] = db[o:o + n]
        torch.cuda.synchronize()
        _INPUTS[pool.key()] = w
    return _INPUTS[pool.key()]


def _run(pkg, w, pool, idx, fast, mixed, read_at, keep_taps=False, full=False, rds_decode=False, on_read=None):
    """Station c given pool input idx[c]: each block gathered on the device from w, submitted back to back (fmd_submit_*_dev, as bench.py);
    the host reads after the blocks in read_at.  on_read(b, got, dm) sees each read.  full: every block is read, with TOL_STREAMS."""
    import torch
    n = idx.size
    dm = pkg.BatchDemod(n, pool.bs, pool.fs, fast_math=fast, keep_taps=keep_taps, rds_decode=rds_decode)
    assert dm.rates.n_rds == SP.n_rds(pool.fs) and dm.bytes_cap == SP.bytes_cap(pool.fs)
    if mixed:
        objs = {}
        for c in range(n):
            ctl = SP.ctl_of(int(idx[c]), True)
            if ctl is not None:
                dm.set_controls(objs.setdefault(ctl, _controls(pkg, ctl)), c)
    idx_t = torch.from_numpy(idx).cuda()
    # the blocks are gathered on a stream of their own: fmd_submit_* reads a block behind what is queued on the stream it is handed, and a
    # null handle (torch's default stream) means "the data is in place now"
    gs = torch.cuda.Stream()
    gs.wait_stream(torch.cuda.current_stream())
    rec = {k: [] for k in TOL_STREAMS + ("bytes",)} if full else None
    for b in range(pool.blocks):
        with torch.cuda.stream(gs):
            blk = w[:, b * pool.bs:(b + 1) * pool.bs][idx_t].contiguous()
            assert dm.submit(blk, ready_stream=gs) == 0
            dm.wait_input(gs)                   # (the buffer's memory is reused only behind the library's read of it)
            del blk
        if b in read_at or full:
            syms, cnt = dm.rds_symbols()
            by, bc = dm.rds_bytes()
            got = dict(audio=dm.audio(), pll=dm.stream("pll_poly" if fast else "pll_dt"), cnt=cnt, syms=syms, bc=bc, by=by)
            if full:
                for k in TOL_STREAMS:
                    rec[k].append(got["audio"].reshape(n, -1) if k == "audio" else dm.stream(k))
                rec["bytes"].append([by[c, :bc[c]].copy() for c in range(n)])
            if on_read is not None and b in read_at:
                on_read(b, got, dm)
    dm.close()
    if full:
        return {k: (np.concatenate(v, axis=1) if k != "bytes" else v) for k, v in rec.items()}
    return None


def lmr_audio_ratio(g, o, nb):
    """Worst per-block RMS error of L-R (audio: twice the bar) over its allowance: TOL_RMS, or what a difference between the two runs' L-R phase
    offsets explains, 0.7 x |offset difference| (tests/test_gpu_fast.py lmr_audio_excess).  The offset difference a block's L-R is rotated by
    is taken as the largest of that block's and the two before it: a block is mixed with offsets that move, estimate by estimate, from the
    previous block's to its own (block 0: both runs start at 0, yet its L-R differs by up to 2.4e-4 where its own offsets differ by 7.7e-4
    turns, measured), and after a flipped estimate the tracker pulls the two offsets together over more than one block."""
    import test_gpu_fast as F
    doff = np.abs(np.asarray(g["lmr_phase"][0], np.float64).reshape(-1)[:nb] - o["lmr_phase"].reshape(-1)[:nb].astype(np.float64))
    p = np.concatenate([[0.0, 0.0], doff])
    win = np.maximum(np.maximum(p[:-2], p[1:-1]), p[2:])
    worst = 0.0
    for k, scale in (("lmr", 1.0), ("audio", 2.0)):
        d = np.asarray(g[k][0], np.float64).reshape(nb, -1) - o[k].reshape(nb, -1)
        worst = max(worst, float(np.max(np.sqrt((d ** 2).mean(axis=1)) / np.maximum(F.TOL_RMS, scale * 0.7 * win))))
    return worst


def _tolerance_bar(i, mixed, g, o, nb):
    """The north-star tolerance of one pool input's small GPU run against the oracle (tests/test_gpu_fast.py's helpers and bar), asserted for
    every input.  Named classes of inputs, by what they carry (measured on one MI355X over the three pools):
      pilot-less: L+R only — their L-R is demodulated noise and they carry no RDS the loops could lock to;
      detuned, weak or noisy pilot (station_pool.marginal) and de-emphasis on (the reference de-emphasises the whole MPX, the 57 kHz RDS
      subcarrier 25-29 dB down): the RDS bits are not identical from lock on for 3-14 % of them (decisions of the synchroniser on symbols near
      its margins); >= 80 % of their bits must agree chunk by chunk (tests/test_gpu_realistic.py bit_agreement; measured >= 83 %).
    Every other input's RDS bits are identical to the oracle's from lock on.  Returns a list of failures."""
    import test_gpu_fast as F
    from test_gpu_realistic import bit_agreement
    bad = []
    for k in ("fm_out_iq", "lpr"):
        e = F.rms(np.asarray(g[k][0], np.float64).reshape(-1) - o["full"][k].reshape(-1))
        if not e <= F.TOL_RMS:
            bad.append(f"input {i}: {k} rms error {e:.2e}")
    if SP.pilotless(i):
        return bad
    oo = {k: o["full"][k] for k in ("lmr", "audio", "lmr_phase")}
    r = lmr_audio_ratio(g, oo, nb)
    if not r <= 1.0:
        bad.append(f"input {i}: L-R / audio {r:.2f} x the allowance")
    gb = np.concatenate(g["bytes"][0])
    ob = np.concatenate(o["bytes"])
    if SP.marginal(i) or SP.deemphasised(i, mixed):
        ag = bit_agreement(gb, ob, skip_bits=5 * 76)
        if not ag >= 0.8:
            bad.append(f"input {i}: {ag:.3f} of the RDS bits agree")
    elif not F.same_bits_once_in_lock(gb, ob, skip_bits=5 * 76):
        bad.append(f"input {i}: RDS bits differ from lock on ({gb.size} / {ob.size} bytes)")
    return bad


def _pool_state(pkg, ex, fs, u8, mixed):
    """Everything the cases of one (rate, format, controls) pool compare against, computed once: the exact mode's expected rows (oracle),
    the tolerance mode's expected rows (small GPU run of the pool inputs) after checking that run against the oracle.  One oracle run serves
    both modes where the library designs the same coefficients for both."""
    key = (fs, u8, mixed)
    if key not in _STATE:
        try:
            _STATE[key] = _make_pool_state(pkg, ex, fs, u8, mixed)
        except AssertionError as e:       # (computed once: the cases of the same pool fail with the same message)
            _STATE[key] = {"error": str(e)}
    if "error" in _STATE[key]:
        pytest.fail(_STATE[key]["error"])
    return _STATE[key]


def _make_pool_state(pkg, ex, fs, u8, mixed):
    key = (fs, u8, mixed)
    modes = MODES_OF[key]
    pool = SP.Pool(fs, u8)
    t0 = time.time()
    w = _device_inputs(ex, pool)
    st = {"pool": pool, "inputs_s": time.time() - t0, "oracle_s": 0.0, "oracle_cpu_s": 0.0, "gpu_small_s": 0.0}
    coeffs = {m: _lib_coeffs(pkg, fs, m == "tolerance", mixed) for m in modes}
    nb = pool.blocks
    small = None
    if "tolerance" in modes:
        # the small run checked against the oracle (FMD_FLAG_KEEP_TAPS: fm_out_iq, L+R and L-R materialised); its rows at the read blocks are
        # what every station of a large batch must reproduce bit for bit (the PLL result: pll_poly)
        tol = SP.Expected(fs, pool.n_inputs, SP.READ_AT)

        def keep(b, got, dm):
            for i in range(pool.n_inputs):
                tol.set_row(b, i, got["audio"][i], got["pll"][i], got["syms"][i, :got["cnt"][i]], got["by"][i, :got["bc"][i]])
        t0 = time.time()
        small = _run(pkg, w, pool, np.arange(pool.n_inputs), True, mixed, read_at=SP.READ_AT, keep_taps=True, full=True, on_read=keep)
        st["gpu_small_s"] = time.time() - t0
        tol.bytes = [[small["bytes"][b][i] for b in range(nb)] for i in range(pool.n_inputs)]
        st["tolerance"] = tol
        st["tolerance_coeffs"] = coeffs["tolerance"]
    failures = []

    def verify(i, r):
        g = {k: [small[k][i]] for k in TOL_STREAMS}
        g["bytes"] = [[small["bytes"][b][i] for b in range(nb)]]
        failures.extend(_tolerance_bar(i, mixed, g, r, nb))
        r["full"] = None

    shared = small is not None and "exact" in modes and coeffs["exact"] == coeffs["tolerance"]
    st["shared_oracle_run"] = shared
    runs = []
    if "exact" in modes:
        runs.append(("exact", coeffs["exact"], TOL_STREAMS if shared else (), verify if shared else None, SP.READ_AT))
    if small is not None and not shared:
        runs.append(("tolerance", coeffs["tolerance"], TOL_STREAMS, verify, ()))
    for mode, cf_, full_streams, cb, read_at in runs:
        t0 = time.time()
        res, cpu = SP.run_oracle(pool, ex, mixed=mixed, coeffs=cf_, read_at=read_at, full_streams=full_streams, on_result=cb)
        st["oracle_s"] += time.time() - t0
        st["oracle_cpu_s"] += cpu
        if mode == "exact":
            st["exact"] = SP.Expected.from_oracle(fs, pool.n_inputs, res)
            st["exact_coeffs"] = coeffs["exact"]
    if small is not None:
        assert not failures, f"the tolerance mode's small run of the pool ({len(failures)} problems):\n" + "\n".join(failures[:40])
        # the same pool inputs with the default flags, as the large batches run: every stream at the read blocks equals the checked run's
        # (FMD_FLAG_KEEP_TAPS changes which streams are materialised, so it may change kernel selection)
        problems = []

        def same(b, got, dm):
            idx = np.arange(pool.n_inputs)
            bad = SP.check_block(tol, b, got, idx)
            if any(v.any() for v in bad.values()):
                problems.append(SP.describe(tol, b, got, idx, bad, label="default flags vs FMD_FLAG_KEEP_TAPS, "))
        _run(pkg, w, pool, np.arange(pool.n_inputs), True, mixed, read_at=SP.READ_AT, on_read=same)
        assert not problems, "\n".join(problems)
        small = None
    print(f"pool fs={fs} {'u8' if u8 else 'cf32'} {'mixed' if mixed else 'uniform'} controls: inputs {st['inputs_s']:.1f} s, "
          f"oracle {st['oracle_s']:.1f} s wall / {st['oracle_cpu_s']:.1f} CPU-s ({'one run for both modes' if shared else 'per mode'}), "
          f"small GPU run {st['gpu_small_s']:.1f} s")
    return st


def _rds_dbs(exp, read_at):
    """{block: uint8 [P, 120]}: the oracle chain's database of each pool input after the bytes up to that block."""
    import rds_oracle as R
    out = {b: np.zeros((exp.n_inputs, 120), np.uint8) for b in read_at}
    for i in range(exp.n_inputs):
        ch = R.RdsChain()
        for b in range(max(read_at) + 1):
            ch.process(exp.bytes[i][b])
            if b in read_at:
                out[b][i] = np.frombuffer(ch.db(), np.uint8)
    return out


@pytest.mark.parametrize("mode,n_st,fs,u8,mixed,rds_decode,why", CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[2] // 1000}k-{'u8' if c[3] else 'cf32'}{'-controls' if c[4] else ''}{'-rds' if c[5] else ''}" for c in CASES])
def test_every_station_equals_its_own_input(pkg, ex, mode, n_st, fs, u8, mixed, rds_decode, why):
    st = _pool_state(pkg, ex, fs, u8, mixed)
    pool = st["pool"]
    exp = st[mode]
    idx = SP.station_map(n_st)
    assert np.bincount(idx, minlength=pool.n_inputs).min() >= 1      # every pool input in the batch
    assert sum(SP.pilotless(int(i)) for i in idx) > 0                # stations whose pilot loop never locks are in every batch
    dbs = _rds_dbs(exp, SP.READ_AT) if rds_decode else None
    w = _device_inputs(ex, pool)
    problems, compared = [], {}

    def check(b, got, dm):
        bad = SP.check_block(exp, b, got, idx)
        assert all(v.size == n_st for v in bad.values())
        compared[b] = n_st
        if any(v.any() for v in bad.values()):
            problems.append(SP.describe(exp, b, got, idx, bad, label=f"{mode} {n_st} stations ({why}), "))
        if rds_decode:
            db = dm.rds_db().view(np.uint8).reshape(n_st, 120)
            wrong = np.flatnonzero((db != dbs[b][idx]).any(axis=1))
            compared[("db", b)] = n_st
            if wrong.size:
                problems.append(f"block {b}: the RDS database of {wrong.size} stations differs from the oracle chain fed their bytes: {wrong[:10].tolist()}")

    t0 = time.time()
    _run(pkg, w, pool, idx, mode == "tolerance", mixed, SP.READ_AT, rds_decode=rds_decode, on_read=check)
    gpu_s = time.time() - t0
    if mixed:       # the coefficients the stations run with are those the pool was run with
        dm = pkg.BatchDemod(n_st, pool.bs, fs, fast_math=mode == "tolerance")
        want = st[f"{mode}_coeffs"]
        for ctl in [None] + list(SP.CONTROL_SET):
            c = int(np.flatnonzero([SP.ctl_of(int(i), True) == ctl for i in idx])[0])
            dm.set_controls(_controls(pkg, ctl), c)
            assert bytes(dm.get_coeffs(c)) == want[ctl], ctl
        dm.close()
    print(f"{mode} {n_st} stations @ {fs} {'u8' if u8 else 'cf32'}: GPU run {gpu_s:.1f} s (pool: oracle {st['oracle_s']:.1f} s wall, "
          f"{st['oracle_cpu_s']:.1f} CPU-s; small GPU run {st['gpu_small_s']:.1f} s)")
    assert not problems, "\n".join(problems)
    assert sorted(b for b in compared if isinstance(b, int)) == list(SP.READ_AT)
    assert all(v == n_st for v in compared.values())                   # every station compared at every read, not a sample
