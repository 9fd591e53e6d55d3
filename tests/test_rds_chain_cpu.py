"""The oracle's RDS decoding chain (oracle/rds_chain.c fmo_rds_chain_*) against the reference's own RDS_Decoding_Chain
(oracle/_ref/fm_rds_db_dump), bit for bit: the groups delivered and the database record after every chunk, on the RDS bytes of the
two rds_group_sync captures and on the synthesised streams of tests/rds_streams.py, cut three ways.  Where oracle/_ref is absent the
reference's records come as digests from tests/golden/rds_chain_records.json (tests/golden/make_rds_chain_records.py).
Also: the new public header compiles as C with the layouts it promises."""
import hashlib
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rds_oracle as O
import rds_streams as R
import test_rds_group_sync as G

ROOT = Path(__file__).resolve().parent.parent
CAPTURES = {f"capture_noise={n}_seed={s}": (n, s) for n, s in G.CASES}
STREAMS = list(CAPTURES) + list(R.synthetic_streams())
CHUNKINGS = ["chunk16", "odd", "whole"]


def record_key(stream: str, chunking: str) -> str:
    return f"rds_chain/{stream}/{chunking}"


def stream_bytes(name: str, tmp: Path) -> np.ndarray:
    if name in CAPTURES:
        return G._reference(*CAPTURES[name], tmp)[2]   # the reference's own RDS bytes of the capture (live or recorded)
    return R.synthetic_streams()[name]


def case(name: str, chunking: str, tmp: Path):
    x = stream_bytes(name, tmp)
    chunks = R.chunk_lists(x.size)[chunking]
    resets = (len(chunks) // 2,)
    return x, chunks, resets


def mask_in_sync(records: bytes) -> bytes:
    """The records with every database's in_sync zeroed (the reference harness cannot see the synchroniser's state)."""
    out = bytearray(records)
    pos = 0
    while pos < len(out):
        n = int(np.frombuffer(bytes(out[pos:pos + 4]), np.int32)[0])
        pos += 4 + 16 * n
        out[pos + 108:pos + 112] = b"\0\0\0\0"
        pos += 120
    return bytes(out)


def parse(records: bytes):
    """[(groups uint8 [n, 16], db bytes)] per chunk."""
    out, pos = [], 0
    while pos < len(records):
        n = int(np.frombuffer(records[pos:pos + 4], np.int32)[0])
        pos += 4
        g = np.frombuffer(records[pos:pos + 16 * n], np.uint8).reshape(n, 16)
        pos += 16 * n
        out.append((g, records[pos:pos + 120]))
        pos += 120
    return out


@pytest.mark.parametrize("chunking", CHUNKINGS)
@pytest.mark.parametrize("name", STREAMS)
def test_oracle_chain_matches_reference(tmp_path, name, chunking):
    x, chunks, resets = case(name, chunking, tmp_path)
    mine = mask_in_sync(O.rds_chain_records(x, chunks, reset_db_after=resets))
    if O.have_ref_chain():
        ref = O.run_ref_rds_chain(x, chunks, tmp_path / "ref", reset_db_after=resets)
        if ref != mine:
            a, b = parse(mine), parse(ref)
            first = next(k for k in range(min(len(a), len(b))) if not (np.array_equal(a[k][0], b[k][0]) and a[k][1] == b[k][1]))
            pytest.fail(f"chunk {first} of {len(chunks)} differs: oracle {a[first][0].shape[0]} groups, reference {b[first][0].shape[0]}")
    else:
        rec = O.records()[record_key(name, chunking)]
        assert rec["bytes"] == len(mine)
        assert rec["sha256"] == hashlib.sha256(mine).hexdigest()


def test_streams_cover_what_they_claim(tmp_path):
    """The synthesised streams reach the paths they are named after (a stream that never left the hunting state would pass the
    comparison above without testing anything)."""
    def final(name):
        x = R.synthetic_streams()[name]
        ch = O.RdsChain()
        g = ch.process(x)
        return g, np.frombuffer(ch.db(), np.uint8)

    g, db = final("all_types")
    assert db[:8].tobytes() == b"ALLTYPES" and db[8:16].tobytes() == b"PTYNAME!"
    assert db[16:80].tobytes() == b"Every group type the reference decodes, B versions and the rest."
    types = {(int(b) >> 12, (int(b) >> 11) & 1) for b in g.view("<u2")[:, 2]}
    assert {(c, 0) for c in (0, 1, 2, 3, 4, 10, 11, 14)} <= types and {(c, 1) for c in range(16)} <= types
    assert (g[:, 10] == 3).any(), "version B groups carry block 3 under C'"

    g, db = final("errors")
    valid = g[:, 3::4]
    assert (valid == 0).any() and (valid == 1).sum() > 0.8 * valid.size
    assert int(np.frombuffer(db[116:120].tobytes(), np.uint32)[0]) >= 2, "three errored groups in a row must force a re-lock"

    g, db = final("ab_flips")
    # the last 2A / 10A groups flip A/B back (text cleared) and arrive under C': only block 4's two characters land
    assert db[16:80].tobytes() == bytes(22) + b"RM" + bytes(40) and db[8:16].tobytes() == b"\0\0TC\0\0\0\0"
    assert db[4:6].tobytes() == b"O\0", "'\\r' is stored as 0"

    g, db = final("dates")
    day, month, year = np.frombuffer(db[88:100].tobytes(), np.int32)
    assert (year, month, day) == (2020, 5, 31) and np.int8(db[104]) == -3   # MJD 59000 (its block 4 errored), the C' group's offset

    g, db = final("random_1MiB")
    assert int(np.frombuffer(db[116:120].tobytes(), np.uint32)[0]) > 100, "random bytes must produce false locks"


def test_header_layouts_in_c(tmp_path):
    """include/fmdemod.h compiles as C11 and its RDS records have the fixed layout the GPU, the oracle and the harness share."""
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stddef.h>\n#include "fmdemod.h"\n'
        "_Static_assert(sizeof(fmd_rds_db) == 120, \"db\");\n"
        "_Static_assert(sizeof(fmd_rds_group) == 16 && sizeof(fmd_rds_block) == 4, \"group\");\n"
        "_Static_assert(offsetof(fmd_rds_db, PI_code) == 80 && offsetof(fmd_rds_db, datetime) == 88, \"db fields\");\n"
        "_Static_assert(offsetof(fmd_rds_db, local_time_offset) == 104 && offsetof(fmd_rds_db, in_sync) == 108, \"db fields\");\n"
        "_Static_assert(offsetof(fmd_rds_db, sync_acquisitions) == 116 && FMD_FLAG_RDS_DECODE == 128u, \"db fields\");\n"
        "int main(void) { return FMD_RDS_TA_NOW_EON_ANNOUNCE == 3 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "layout")], check=True)
    subprocess.run([str(tmp_path / "layout")], check=True)


def test_cpp_adaptor_rds_surface_compiles(tmp_path):
    """App_GPU::GetRDSDatabase() (the reference's App::GetRDSDatabase, src/app.h:42: same field names, Reset()) and
    Broadcast_FM_Demod_GPU::GetRDSRawSymbols() (broadcast_fm_demod.h:254) compile in a program written against them."""
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", f"-I{ROOT / 'fm-radio_amd' / 'host'}",
                    str(ROOT / "tests" / "cpp" / "rds_app_main.cpp"), "-o", str(tmp_path / "rds_app_main.o")], check=True)
