"""CPU sanitizer run (SURVEY §4 "sanitizers on the CPU build"; never on the GPU box's device code): the oracle (oracle/fm_oracle.c),
the library's host-side filter designer (fm-radio_amd/csrc/fmd_design.cpp), the designers of the tolerance mode's tables
(fmd_tables.cpp), the kernel-selection plan (fmd_plan.cpp), the block schedule (fmd_schedule.cpp) and the host-side drivers (group synchroniser, scraper writers) built with
-fsanitize=address,undefined (`make -C oracle asan`) as stand-alone programs and fed the golden fixtures.  Any out-of-bounds access, use after
free, leak, signed overflow or misaligned access aborts the run (-fno-sanitize-recover); the outputs must still be the fixtures'.

The reference's own trouble spots on this path: a static lambda capture in its designer (src/dsp/filter_designer.cpp:235,288,345) and
the re-blocking buffer's span arithmetic (src/utility/reconstruction_buffer.h:16-26) — the driver re-blocks ragged pieces the same way."""
import ctypes as C
import hashlib
import json
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oraclelib as O

ROOT = Path(__file__).resolve().parent.parent
ASAN = ROOT / "oracle" / "_asan"
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def asan_build():
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "oracle"), "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return ASAN


def _run(cmd):
    r = subprocess.run([str(c) for c in cmd], env=ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r


@pytest.mark.parametrize("fixture,u8,bs,fs", [("chain_b16384", True, 16384, 1_024_000), ("chain_cf32_b8192", False, 8192, 1_024_000)])
def test_oracle_under_sanitizers_reproduces_the_golden_chain(asan_build, tmp_path, fixture, u8, bs, fs):
    g = np.load(ROOT / "tests" / "golden" / f"{fixture}.npz")
    cap = tmp_path / "cap.bin"
    np.ascontiguousarray(g["capture"]).tofile(cap)
    _run([asan_build / "sanitizer_main", "chain", cap, "u8" if u8 else "cf32", bs, fs, tmp_path / "out"])
    audio = np.fromfile(str(tmp_path / "out") + ".audio.f32", np.float32)
    counts = np.fromfile(str(tmp_path / "out") + ".rds_count.i32", np.int32)
    phase = np.fromfile(str(tmp_path / "out") + ".lmr_phase.f32", np.float32)
    # the fixtures were dumped from the compiled reference (tests/golden/make_golden.py); its pilot gain goes through rsqrtss, which
    # differs between CPUs: the north-star tolerance here, bit-identity is tests/test_oracle_vs_ref.py's business
    nb = g["capture"].shape[0] // bs
    assert audio.size == g["audio"].size
    assert np.sqrt(np.mean((audio.astype(np.float64) - g["audio"]) ** 2)) <= 1e-4
    assert counts.size == nb and np.array_equal(counts, g["rds_count"])
    assert np.allclose(phase[-g["lmr_phase"].size:], g["lmr_phase"], atol=1e-4)


def test_designer_under_sanitizers_equals_the_oracle_design(asan_build, tmp_path):
    for fs in (256_000, 1_024_000, 2_048_000):
        out = tmp_path / f"coeffs_{fs}.bin"
        _run([asan_build / "sanitizer_main", "design", fs, out])
        k = O.Coeffs.from_buffer_copy(out.read_bytes())
        want = O.design(fs, rsqrt_mode=0)
        for name in ("b_fm_in", "b_fm_out", "b_hilbert", "pll_lpf_b", "pll_lpf_a", "b_lpr", "b_lmr", "b_rds", "ted_lpf_b", "bpsk_lpf_b"):
            a, b = k.arr(name), want.arr(name)
            assert np.array_equal(a, b), (fs, name, np.abs(a - b).max())
        assert np.allclose(k.arr("pilot_b"), want.arr("pilot_b"), rtol=3e-7) and np.array_equal(k.arr("pilot_a"), want.arr("pilot_a"))
        k2 = O.Coeffs.from_buffer_copy(Path(str(out) + ".ctl").read_bytes())
        ctl = O.default_controls(); ctl.use_deemphasis, ctl.deemphasis_tus, ctl.lpr_cutoff_hz = 1, 50, 12000
        want2 = O.design(fs, controls=ctl, rsqrt_mode=0)
        for name in ("deemph_b", "deemph_a", "b_lpr", "b_lmr"):
            assert np.array_equal(k2.arr(name), want2.arr(name)), (fs, name)


def test_host_drivers_under_sanitizers(asan_build, tmp_path):
    g = np.load(ROOT / "tests" / "golden" / "long_b65536.npz")
    # the RDS group synchroniser on the golden byte stream: the groups the reference's decoder logged (tests/golden/make_golden.py)
    (tmp_path / "rds.bin").write_bytes(g["rds_bytes"].tobytes())
    out = _run([asan_build / "group_sync_main", tmp_path / "rds.bin"]).stdout.splitlines()
    groups = [l for l in out if l.startswith("[group]")]
    want = ["[group] [" + " ".join(f"{int(v):04X}" for v in row) + "]" for row in g["groups"]]
    assert len(groups) >= 15 and all(x in want for x in groups if "----" not in x)
    # the scraper-compatible writers on golden audio blocks
    audio = g["audio"].astype(np.float32)                                    # [3][4096] = 3 blocks of 2048 frames
    audio.tofile(tmp_path / "audio.f32")
    _run([asan_build / "scraper_writer_main", tmp_path / "audio.f32", tmp_path / "rds.bin", 2048, tmp_path / "o.wav", tmp_path / "o.bin"])
    wav = (tmp_path / "o.wav").read_bytes()
    assert wav[:4] == b"RIFF" and wav[8:12] == b"WAVE" and len(wav) == 44 + audio.size * 2
    pcm = np.frombuffer(wav[44:], np.int16)
    assert np.array_equal(pcm, (audio.reshape(-1) * (np.float32(32767.0) * np.float32(0.95))).astype(np.int32).astype(np.int16))
    assert (tmp_path / "o.bin").read_bytes() == g["rds_bytes"].tobytes()[:len(g["rds_bytes"]) // 16 * 16]


def test_kernel_selection_plan_under_sanitizers_equals_the_model(asan_build, tmp_path):
    """fm-radio_amd/csrc/fmd_plan.cpp built with plain g++ (no HIP, no library) under the sanitizers: the corners of tests/test_plan_cpu.py's sweep — the
    station counts within 3 of every switch at each rate and block length, every FMD_FLAG_PLL_* selector, both modes, in and out of lock, and the
    moved thresholds of the parity tests — give tests/plan_model.py's answers."""
    import plan_model as M
    cases = []
    for fs in (256_000, 1_024_000, 2_048_000):
        for bs in (16384, 10240, 65536):
            m, n_fm_out, n_est = M.lengths(fs, bs * (fs // 256_000))
            for flags in (0, M.FAST_MATH, M.KEEP_TAPS, M.NO_PIPELINE, M.PLL_TIME_PARALLEL, M.PLL_LOW_WORK, M.PLL_K8, M.PLL_TIME_PARALLEL | M.PLL_K8,
                          M.PLL_STREAM_ORDER, M.FAST_MATH | M.NO_PIPELINE):
                cases += [(c, m, n_fm_out, n_est, flags, None, u) for c in M.stations_to_try() for u in (0, 1)]
    cases += [(c, 1, 8192, 205, 0, th, u) for c in (5, 12) for th in ((4, 7168), (4, 4), (2, 7168), (2, 2)) for u in (0, 1)]
    (tmp_path / "cases.txt").write_text("".join(f"{c} {m} {nf} {ne} {fl} {th[0] if th else -1} {th[1] if th else -1} {u}\n" for c, m, nf, ne, fl, th, u in cases))
    # ... and the block plan (make_block_plan) over a handful of tests/test_plan_cpu.py's product: the three rates, both modes and input types, every
    # fact, at block lengths with 1, 3, 6, 9, 16, 64 and 1024 half-tiles and station counts on the tile, pad and pairing switches
    import itertools
    blocks = []
    for fs, k, c, fl, u8 in itertools.product((256_000, 1_024_000, 2_048_000), (1, 3, 6, 9, 16, 64, 1024), (1, 3, 1024, 1793, 3071, 3072, 12290), (0, M.FAST_MATH, M.FAST_MATH | M.KEEP_TAPS),
                                               (0, 1)):
        blocks += [(c, fs, 1024 * (fs // 256_000) * k, fl, u8) + facts
                   for facts in ((0, 0, 0, 0, 0), (0, 1, 0, 1, 0), (1, 0, 0, 1, 1), (0, 0, 1, 1, 0), (0, 0, 0, 1, 1), (0, 0, 1, 1, 2), (1, 0, 1, 0, 1))]
    (tmp_path / "blocks.txt").write_text("".join(f"{c} {M.lengths(fs, bs)[0]} {M.lengths(fs, bs)[1]} {M.lengths(fs, bs)[2]} {fl} {u8} {a} {t} {s} {u} {p}\n"
                                                 for c, fs, bs, fl, u8, a, t, s, u, p in blocks))
    out = _run([asan_build / "plan_main", tmp_path / "cases.txt", tmp_path / "blocks.txt"]).stdout.split("\n")[:-1]
    assert len(out) == len(cases) + 1 + len(blocks) and len(cases) > 20_000 and out[len(cases)] == "--" and len(blocks) > 5000
    for line, (c, m, nf, ne, fl, th, u) in zip(out, cases):
        assert tuple(map(int, line.split())) == M.plan(c, m, nf, ne, fl, th, bool(u)), (c, m, nf, ne, fl, th, u)
    for line, (c, fs, bs, fl, u8, a, t, s, u, p) in zip(out[len(cases) + 1:], blocks):
        want = M.block_plan(c, fs, bs, fl, bool(u8), bool(a), bool(t), bool(s), bool(u), p)
        names = (("k_front", "k_front_mfma", "k_front_pre_mfma")[want[M.BLOCK_FIELDS.index("front_kernel")]], "k_extract_bp" if fl & M.FAST_MATH else "k_extract")
        assert tuple(line.split()) == tuple(map(str, want)) + names, (c, fs, bs, fl, u8, a, t, s, u, p)


def test_table_designers_under_sanitizers_reproduce_the_pinned_tables(asan_build, tmp_path):
    """fm-radio_amd/csrc/fmd_tables.cpp with fmd_design.cpp, plain g++ (no HIP, no library), under the sanitizers: every table the tolerance mode
    uploads — PilotFastTab, PllSpanTab, PllSparseTab with its wrap ties, the Toeplitz operand images, the 12 + 6 band-pass tap tables and the
    block-edge matrix — at the three rates, with both audio cut-offs at 15, 12 and 9 kHz, byte for byte what the designers gave while they were
    part of fmd_api.cpp (tests/golden/design_tables.json: SHA-256 per table, made from that code before it moved)."""
    want = json.loads((ROOT / "tests" / "golden" / "design_tables.json").read_text())
    out = tmp_path / "tables.bin"
    records = [l.split() for l in _run([asan_build / "tables_main", out]).stdout.splitlines()]
    blob = out.read_bytes()
    got = [{"fs": int(fs), "table": name, "bytes": int(n), "sha256": hashlib.sha256(blob[int(off):int(off) + int(n)]).hexdigest()} for fs, name, off, n in records]
    assert len(want["tables"]) == 21 and [(t["fs"], t["table"], t["bytes"]) for t in got] == [(t["fs"], t["table"], t["bytes"]) for t in want["tables"]]
    differing = [(g["fs"], g["table"]) for g, w in zip(got, want["tables"]) if g["sha256"] != w["sha256"]]
    assert not differing, f"first differing table: {differing[0]}; all: {differing}"
    assert len(blob) == want["bytes"] == sum(t["bytes"] for t in got) and hashlib.sha256(blob).hexdigest() == want["sha256"]


def test_block_schedule_under_sanitizers_gives_the_recorded_graphs(asan_build, tmp_path):
    """fm-radio_amd/csrc/fmd_schedule.cpp with fmd_plan.cpp, plain g++ (no HIP, no library), under the sanitizers: tests/cpp/schedule_main.cpp on every scenario of
    tests/golden/schedule_traces.json gives the dependency graphs recorded from the code the unit replaced (tests/test_schedule_cpu.py states the comparison)."""
    import schedule_graph as G
    golden = json.loads((ROOT / "tests" / "golden" / "schedule_traces.json").read_text())
    (tmp_path / "scenarios.txt").write_text(G.scenario_text(golden["scenarios"]))
    got = G.split_log(_run([asan_build / "schedule_main", tmp_path / "scenarios.txt"]).stdout)
    assert sorted(got) == sorted(golden["traces"]) and len(got) >= 25
    for name, want in golden["traces"].items():
        assert G.normalise(got[name]).queues == G.normalise(want).queues, name
