"""GPU tests (pytest -m gpu): the RDS decoding chain on the GPU (k_rds_decode, fm-radio_amd/csrc/fmd_kernels_rds.inc) against the
oracle's chain (oracle/rds_chain.c fmo_rds_chain_*, itself bit-identical to the reference's RDS_Decoding_Chain: tests/test_rds_chain_cpu.py).

  * the standalone decoder (fmd_rdsdec_*): 4096 channels, each its own stream, the groups and the database after every call bit-identical
    to the oracle's; the same result whether a stream comes in 16-byte chunks, odd chunks or one piece; the named streams of
    tests/rds_streams.py (every group type, A/B flips, bit errors, MJD edges, 1 MiB of random bytes) and the two rds_group_sync captures;
  * the demodulator with FMD_FLAG_RDS_DECODE, both arithmetic modes, 256 kSa/s cf32 and 1.024 MSa/s u8, through fmd_process_* (pipelined),
    fmd_submit_* with fmd_set_output_lag, the put-off extract stage (1024 stations, device views one block behind) and FMD_FLAG_NO_PIPELINE:
    every block's groups and database == the oracle chain on that handle's own RDS bytes, and at the end every station's PI / PS / RT /
    PTY / date and time == what the synthesiser encoded;
  * the exact mode on the recorded captures: the final database == the reference chain's on the reference's bytes;
  * state blobs, fmd_reset, fmd_reset_rds_db; without the flag the getters refuse and the blob does not grow."""
import hashlib

import numpy as np
import pytest

import oraclelib
import rds_oracle as O
import rds_streams as R
import rds_synth as RS
import synth

pytestmark = pytest.mark.gpu
FMD_ERR_ARG = -1


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.load_library()
    import torch
    assert torch.cuda.is_available()
    return p


def _oracle_per_call(stream: np.ndarray, chunks, reset_db_after=()):
    """[(groups uint8 [n, 16], db bytes)] after every chunk."""
    ch = O.RdsChain()
    out, pos = [], 0
    for k, n in enumerate(chunks):
        g = ch.process(stream[pos:pos + n])
        pos += n
        out.append((g, ch.db()))
        if k in reset_db_after:
            ch.reset_db()
    return out


def _run_standalone(pkg, streams, chunk_lists, reset_db_after=()):
    """Feed channel c its stream in the chunks chunk_lists[c] (padded with empty chunks), one process() call per chunk index; returns
    per call (raw groups [C, cap, 16], counts [C], db uint8 [C, 120])."""
    n_ch = len(streams)
    n_calls = max(len(c) for c in chunk_lists)
    dec = pkg.RDSDecoder(n_ch)
    pos = [0] * n_ch
    out = []
    for k in range(n_calls):
        sizes = [cl[k] if k < len(cl) else 0 for cl in chunk_lists]
        cap = max(max(sizes), 1)
        data = np.zeros((n_ch, cap), np.uint8)
        for c in range(n_ch):
            data[c, :sizes[c]] = streams[c][pos[c]:pos[c] + sizes[c]]
            pos[c] += sizes[c]
        dec.process(data, np.array(sizes, np.int32))
        raw, counts = dec.groups_raw()
        out.append((raw, counts, dec.db().view(np.uint8).reshape(n_ch, 120).copy()))
        if k in reset_db_after:
            dec.reset_db(-1)
    dec.close()
    return out


def _compare(gpu, streams, chunk_lists, reset_db_after=()):
    n_calls = len(gpu)
    for c in range(len(streams)):
        cl = list(chunk_lists[c]) + [0] * (n_calls - len(chunk_lists[c]))
        ref = _oracle_per_call(streams[c], cl, reset_db_after)
        for k in range(n_calls):
            raw, counts, db = gpu[k]
            g_ref, db_ref = ref[k]
            assert counts[c] == g_ref.shape[0], (c, k, counts[c], g_ref.shape[0])
            assert np.array_equal(raw[c, :counts[c]], g_ref), (c, k)
            assert db[c].tobytes() == db_ref, (c, k, np.flatnonzero(db[c] != np.frombuffer(db_ref, np.uint8)))


def test_standalone_4096_streams_match_oracle_and_chunking_does_not_matter(pkg):
    named = [v for k, v in R.synthetic_streams().items() if k != "random_1MiB"]
    streams = named + [R.mixed(c) for c in range(4096 - len(named))]
    kinds = []
    for c, s in enumerate(streams):
        cl = R.chunk_lists(s.size, seed=c)
        kinds.append(cl["chunk16"] if c % 3 == 0 else cl["odd"] if c % 3 == 1 else [97] * (s.size // 97) + [s.size % 97])
    gpu = _run_standalone(pkg, streams, kinds)
    _compare(gpu, streams, kinds)
    # the same streams in one piece: the same final databases and the same groups in the same order
    whole = _run_standalone(pkg, streams, [[s.size] for s in streams])
    assert np.array_equal(whole[-1][2], gpu[-1][2])
    for c in range(0, len(streams), 7):
        cat = np.concatenate([g[0][c, :g[1][c]] for g in gpu])
        assert np.array_equal(whole[0][0][c, :whole[0][1][c]], cat), c
    total_groups = sum(int(g[1].sum()) for g in gpu)
    locks = gpu[-1][2][:, 116:120].copy().view(np.uint32).ravel()
    assert total_groups > 4096 * 20 and (locks >= 2).mean() > 0.5, (total_groups, np.bincount(np.minimum(locks, 9)))


def test_standalone_named_streams_and_captures(pkg):
    rec = oraclelib.ref_records()
    caps = [np.frombuffer(bytes.fromhex(rec[f"rds_group_sync/noise={n}/seed={s}"]["rds_bytes_hex"]), np.uint8) for n, s in ((0.02, 21), (0.45, 22))]
    named = R.synthetic_streams()
    streams = caps + list(named.values())
    chunk_lists = []
    for c, s in enumerate(streams):
        cl = R.chunk_lists(s.size, seed=c)
        chunk_lists.append([4096] * (s.size // 4096) if s.size >= 1 << 20 else cl["odd"] if c % 2 else cl["chunk16"])
    resets = (5,)
    gpu = _run_standalone(pkg, streams, chunk_lists, reset_db_after=resets)
    _compare(gpu, streams, chunk_lists, reset_db_after=resets)


def test_standalone_reset_and_reset_db_keep_what_the_reference_keeps(pkg):
    """fmd_rdsdec_reset_db mid-stream (in lock, mid-group, radiotext with A/B = 1 under way) == the oracle with RDS_Database::Reset() at
    the same point (the synchroniser and the handler's A/B memories carry on); fmd_rdsdec_reset returns to the freshly constructed chain."""
    g = [RS.g2a(0xBEEF, s, b"ab%02d" % s, ab=1) for s in range(16)]
    g += [RS.g0a(0xBEEF, s, b"RESETDB!"[2 * s:2 * s + 2]) for s in range(4)]
    s = RS.pack_bits(RS.encode_groups(g))
    chunks = [16] * (s.size // 16) + ([s.size % 16] if s.size % 16 else [])
    resets = (len(chunks) // 2,)
    gpu = _run_standalone(pkg, [s, s[:200]], [chunks, [200]], reset_db_after=resets)
    _compare(gpu, [s, s[:200]], [chunks, [200]], reset_db_after=resets)
    dec = pkg.RDSDecoder(2)
    data = np.zeros((2, s.size), np.uint8)
    data[0] = s
    dec.process(data, np.array([s.size, 0], np.int32))
    before = dec.db()
    assert before["groups"][0] == len(g) and before["in_sync"][0] == 1 and before["PI_code"][0] == 0xBEEF
    dec.reset()
    assert dec.db()["groups"][0] == len(g)          # (the snapshot is the last call's until the next call)
    dec.process(data, np.array([s.size, 0], np.int32))
    assert dec.db().tobytes() == before.tobytes()
    dec.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# Integrated: FMD_FLAG_RDS_DECODE behind the demodulator's RDS stage

N_ST = 32
SECONDS = 5.0


def _station_texts(c):
    return 0x1234 + c, f"FM{c:03d}STN", (f"Station {c:02d} on the GPU, radiotext segment by segment" + " " * 64)[:64]


def _sent_rt(rt: str) -> bytes:
    """The radiotext the synthesiser's group mix carries: its 4A group takes the slot of every 2A group with segment 7 or 15
    (oracle/synth.py rds_bitstream_mixed), so those two segments stay empty in any decoder."""
    b = bytearray(rt.encode())
    b[28:32] = bytes(4)
    b[60:64] = bytes(4)
    return bytes(b)


_CAPS = {}


def _synth_station(args):
    """(worker process) one station's capture"""
    fs, n, c = args
    pi, ps, rt = _station_texts(c)
    cap = RS.capture_realistic(n, ps, rt, fs=float(fs), seed=4242, channel=c, cnr_db=35.0)
    assert cap["pi"] == pi
    return cap["iq"]


def _captures(fs):
    if fs not in _CAPS:
        from concurrent.futures import ProcessPoolExecutor
        import os
        bs = 16384 * fs // 256000
        n = int(SECONDS * fs) // bs * bs
        with ProcessPoolExecutor(max_workers=min(N_ST, os.cpu_count() or 1)) as ex:
            _CAPS[fs] = np.stack(list(ex.map(_synth_station, [(fs, n, c) for c in range(N_ST)])))
    return _CAPS[fs]


def _blocks(fs, u8):
    caps = _captures(fs)
    bs = 16384 * fs // 256000
    nb = caps.shape[1] // bs
    data = np.stack([synth.to_u8(x) if u8 else synth.to_cf32(x) for x in caps])
    return [np.ascontiguousarray(data[:, b * bs:(b + 1) * bs]) for b in range(nb)], bs


def _check_block(chains, by, bc, raw, counts, db):
    for c in range(len(chains)):
        g = chains[c].process(by[c, :bc[c]])
        assert counts[c] == g.shape[0] and np.array_equal(raw[c, :counts[c]], g), c
        assert db[c].tobytes() == chains[c].db(), (c, np.flatnonzero(db[c] != np.frombuffer(chains[c].db(), np.uint8)))


def _known_answer(db, n_st):
    """What the synthesiser encoded (oracle/synth.py rds_bitstream_mixed: 0A / 2A with the station's PS / RT, 4A at MJD 60586, 12:mm UTC)."""
    for c in range(n_st):
        pi, ps, rt = _station_texts(c)
        d = db[c]
        assert (d["PI_code"], d["service_name"], bytes(db[c:c + 1].view(np.uint8)[16:80])) == (pi, ps.encode(), _sent_rt(rt)), (c, d)
        assert d["programme_type"] == 0 and d["in_sync"] == 1 and d["sync_acquisitions"] >= 1, (c, d)
        assert (d["year"], d["month"], d["day"], d["hour"], d["local_time_offset"]) == (2024, 10, 3, 12, 0), (c, d)


@pytest.mark.parametrize("fs,u8", [(256_000, False), (1_024_000, True)])
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("path", ["process", "submit_lag", "no_pipeline"])
def test_integrated_matches_oracle_and_the_encoded_answer(pkg, fs, u8, fast, path):
    import torch
    if fs == 1_024_000 and path == "submit_lag" and not fast:
        pytest.skip("the exact mode queues every stage at submission: the same schedule as 'process' at this size")
    blocks, bs = _blocks(fs, u8)
    dm = pkg.BatchDemod(N_ST, bs, fs, fast_math=fast, pipelined=path != "no_pipeline", rds_decode=True)
    if path == "submit_lag":
        dm.set_output_lag(True)
    chains = [O.RdsChain() for _ in range(N_ST)]
    for b, blk in enumerate(blocks):
        t = torch.from_numpy(blk).cuda()
        assert (dm.submit(t) if path == "submit_lag" else dm.process(t)) == 0
        dm.synchronize()
        by, bc = dm.rds_bytes()
        raw, counts = dm.rds_groups_raw()
        _check_block(chains, by, bc, raw, counts, dm.rds_db().view(np.uint8).reshape(N_ST, 120))
    db = dm.rds_db()
    dm.close()
    _known_answer(db, N_ST)


def test_integrated_put_off_extract_stage_device_views(pkg):
    """Tolerance mode, 1024 stations at 256 kSa/s through fmd_submit_* with output lag: a block's extract + RDS + decode stages are queued
    when the next block is submitted; the device views (fmd_rds_bytes_dev, fmd_rds_db_dev, fmd_rds_groups_dev) of block k - 1, read
    behind submit(k), equal the oracle chain on those bytes."""
    import torch
    blocks, bs = _blocks(256_000, False)
    n = 1024
    dm = pkg.BatchDemod(n, bs, 256_000, fast_math=True, rds_decode=True)
    dm.set_output_lag(True)
    chains = [O.RdsChain() for _ in range(n)]
    seen, inputs = [], []      # (the input tensors stay alive: the library reads them on its own streams)
    for b, blk in enumerate(blocks[:40]):
        inputs.append(torch.from_numpy(np.ascontiguousarray(blk[np.arange(n) % N_ST])).cuda())
        assert dm.submit(inputs[-1]) == 0
        k = dm.outputs_block()
        if k < 0 or (seen and seen[-1] == k):
            continue
        seen.append(k)
        dm.wait_outputs()
        by, bc = (x.cpu().numpy() for x in dm.rds_bytes_tensors())
        raw, counts = (x.cpu().numpy() for x in dm.rds_groups_tensors())
        _check_block(chains, by, bc, raw, counts, dm.rds_db_tensor().cpu().numpy())
    dm.close()
    assert seen == list(range(len(seen))) and len(seen) >= 38 and seen[-1] < 39, seen   # one block behind: the put-off schedule ran


def test_exact_mode_final_database_equals_the_reference_chain(pkg):
    """The two recorded rds_group_sync captures (1.024 MSa/s u8): the exact mode's own bytes decode, block by block, to exactly what the
    reference's chain makes of the reference's bytes (recorded digest of fm_rds_db_dump's records, tests/golden/rds_chain_records.json)."""
    import test_rds_chain_cpu as RC
    import test_rds_group_sync as G
    rec = oraclelib.ref_records()
    caps = np.stack([G.capture(n, s) for n, s in G.CASES])
    dm = pkg.BatchDemod(2, 65536, 1_024_000, rds_decode=True)
    for b in range(caps.shape[1] // 65536):
        dm.process(np.ascontiguousarray(caps[:, b * 65536:(b + 1) * 65536]))
    db = dm.rds_db().view(np.uint8).reshape(2, 120)
    dm.close()
    for i, (n, s) in enumerate(G.CASES):
        ref_bytes = np.frombuffer(bytes.fromhex(rec[G.record_key(n, s)]["rds_bytes_hex"]), np.uint8)
        name = f"capture_noise={n}_seed={s}"
        whole = RC.mask_in_sync(O.rds_chain_records(ref_bytes, [ref_bytes.size]))
        assert hashlib.sha256(whole).hexdigest() == O.records()[RC.record_key(name, "whole")]["sha256"]   # oracle == reference on these bytes
        ch = O.RdsChain()
        ch.process(ref_bytes)
        assert db[i].tobytes() == ch.db(), i


def test_state_blob_resets_and_flag_off(pkg):
    import torch
    blocks, bs = _blocks(256_000, False)
    for fast in (False, True):
        a = pkg.BatchDemod(4, bs, 256_000, fast_math=fast, rds_decode=True)
        off = pkg.BatchDemod(4, bs, 256_000, fast_math=fast)
        assert a.L.fmd_state_size(a.h) == a.L.fmd_state_size(off.h) + 8 * 4 + 16 + 120
        import ctypes as C
        buf = np.zeros(4096, np.uint8)
        assert a.L.fmd_get_rds_db(off.h, buf.ctypes.data_as(C.c_void_p)) == FMD_ERR_ARG
        assert a.L.fmd_reset_rds_db(off.h, -1) == FMD_ERR_ARG
        assert a.L.fmd_get_rds_groups(off.h, buf.ctypes.data_as(C.c_void_p), 1, buf.ctypes.data_as(C.c_void_p)) == FMD_ERR_ARG
        off.close()
        sub = [np.ascontiguousarray(blk[:4]) for blk in blocks]
        for b in range(30):
            a.process(torch.from_numpy(sub[b]).cuda())
        blob = a.get_state(2)
        bb = pkg.BatchDemod(3, bs, 256_000, fast_math=fast, rds_decode=True)
        for b in range(3):      # other history, other block parity
            bb.process(torch.from_numpy(np.ascontiguousarray(sub[b][1:4])).cuda())
        bb.set_state(0, blob)
        for b in range(30, 50):
            a.process(torch.from_numpy(sub[b]).cuda())
            x = np.ascontiguousarray(np.stack([sub[b][2], sub[b][0], sub[b][1]]))
            bb.process(torch.from_numpy(x).cuda())
            ra, ca = a.rds_groups_raw()
            rb, cb = bb.rds_groups_raw()
            assert ca[2] == cb[0] and np.array_equal(ra[2, :ca[2]], rb[0, :cb[0]]), b
            assert a.rds_db()[2].tobytes() == bb.rds_db()[0].tobytes(), b
        bb.close()
        # fmd_reset_rds_db: the database cleared, the synchroniser and A/B memories kept — the oracle chain with RDS_Database::Reset() there
        chain = O.RdsChain()
        a.reset()
        for b in range(40):
            a.process(torch.from_numpy(sub[b]).cuda())
            by, bc = a.rds_bytes()
            chain.process(by[1, :bc[1]])
            if b == 20:
                a.reset_rds_db(1)
                chain.reset_db()
                assert a.rds_db()[1].tobytes() != chain.db()    # (the snapshot of block 20 is taken before the reset)
            assert a.rds_db()[1].tobytes() == chain.db() or b == 20, b
        # fmd_reset: back to a fresh decoder — the same databases as a new handle on the same blocks
        a.reset()
        c2 = pkg.BatchDemod(4, bs, 256_000, fast_math=fast, rds_decode=True)
        for b in range(12):
            a.process(torch.from_numpy(sub[b]).cuda())
            c2.process(torch.from_numpy(sub[b]).cuda())
            assert a.rds_db().tobytes() == c2.rds_db().tobytes(), b
        a.close()
        c2.close()


def test_cpp_app_gpu_rds_database(pkg, tmp_path):
    """tests/cpp/rds_app_main.cpp: App_GPU fed a realistic u8 capture in odd pieces; GetRDSDatabase() holds the encoded station, Reset()
    clears it (and the decoder's database: the next block shows only what that block decoded), GetRDSRawSymbols() has the block's symbols."""
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "rds_app_main"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{root / 'include'}", f"-I{root / 'fm-radio_amd' / 'host'}", str(root / "tests" / "cpp" / "rds_app_main.cpp"),
                    f"-L{root / 'fm-radio_amd' / 'csrc'}", "-lfmdemod", f"-Wl,-rpath,{root / 'fm-radio_amd' / 'csrc'}", "-o", str(exe)], check=True)
    bs = 65536
    cap = RS.capture_realistic(bs * 60, "APPGPUDB", "R" * 64, fs=1_024_000.0, seed=77, cnr_db=35.0)     # PI 0x1234
    synth.to_u8(cap["iq"]).tofile(tmp_path / "cap.u8")
    out = subprocess.run([str(exe), str(tmp_path / "cap.u8"), str(bs)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0].startswith("PI=1234 PTY=0 PS='APPGPUDB' RT='" + ("R" * 28 + "....") * 2 + "' date=03/10/2024 time=12:"), out[0]   # (see _sent_rt)
    n_raw, n_pred = (int(x.split("=")[1]) for x in out[1].split()[:2])
    assert n_raw == n_pred > 0, out[1]
    assert out[2].startswith("PI=0000 PTY=0 PS='........' RT='" + "." * 64 + "' date=00/00/0000 time=00:00"), out[2]
    assert out[3].startswith("PI=1234"), out[3]
