"""ctypes binding of oracle/liboracle_rds.so (TEST INFRASTRUCTURE: oracle/rds_chain.c, the reference's RDS decoding chain restated in C)
and the runner of the reference's own chain (oracle/_ref/fm_rds_db_dump, built by oracle/rds_chain.mk from the reference's sources).
Records where oracle/_ref is absent: tests/golden/rds_chain_records.json (tests/golden/make_rds_chain_records.py)."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
ORACLE_DIR = ROOT / "oracle"
LIB_PATH = ORACLE_DIR / "liboracle_rds.so"
REF_RDS_DB_DUMP = ORACLE_DIR / "_ref" / "fm_rds_db_dump"
RECORDS = ROOT / "tests" / "golden" / "rds_chain_records.json"


def build() -> None:
    subprocess.run(["make", "-s", "-C", str(ORACLE_DIR), "-f", "rds_chain.mk", "oracle"], check=True)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if (not LIB_PATH.exists()) or any((ORACLE_DIR / f).stat().st_mtime > LIB_PATH.stat().st_mtime for f in ("rds_chain.c", "rds_chain.h")):
        build()
    L = C.CDLL(str(LIB_PATH))
    L.fmo_rds_chain_size.restype = C.c_size_t
    L.fmo_rds_chain_init.argtypes = [C.c_void_p]
    L.fmo_rds_chain_get_db.argtypes = [C.c_void_p, C.c_void_p]
    L.fmo_rds_chain_reset_db.argtypes = [C.c_void_p]
    L.fmo_rds_chain_process.restype = C.c_long
    L.fmo_rds_chain_process.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    _lib = L
    return L


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def have_ref_chain() -> bool:
    return REF_RDS_DB_DUMP.exists()


def records() -> dict:
    return json.loads(RECORDS.read_text())


class RdsChain:
    """The oracle's RDS decoding chain (rds_chain.c fmo_rds_chain_*: the reference's RDS_Decoding_Chain).  Records as raw bytes in
    include/fmdemod.h's layouts: a group is 16 bytes (4 x data u16, block type u8, valid u8), the database 120."""

    GROUP_BYTES, DB_BYTES = 16, 120

    def __init__(self):
        self._buf = (C.c_uint8 * lib().fmo_rds_chain_size())()
        lib().fmo_rds_chain_init(self._buf)

    def process(self, x: np.ndarray) -> np.ndarray:
        """Feed bytes; returns the groups delivered as uint8 [n, 16]."""
        x = np.ascontiguousarray(x, dtype=np.uint8)
        cap = x.size * 8 // 79 + 2
        out = np.zeros((cap, self.GROUP_BYTES), dtype=np.uint8)
        n = lib().fmo_rds_chain_process(self._buf, _ptr(x), x.size, _ptr(out), cap)
        assert n <= cap
        return out[:n]

    def db(self) -> bytes:
        out = np.zeros(self.DB_BYTES, dtype=np.uint8)
        lib().fmo_rds_chain_get_db(self._buf, _ptr(out))
        return out.tobytes()

    def reset_db(self) -> None:
        lib().fmo_rds_chain_reset_db(self._buf)


def rds_chain_records(stream: np.ndarray, chunks, reset_db_after=()) -> bytes:
    """What oracle/_ref/fm_rds_db_dump writes for (stream, chunks, resets): per chunk int32 n_groups, the groups, the database record."""
    ch = RdsChain()
    out = bytearray()
    pos = 0
    for k, n in enumerate(chunks):
        g = ch.process(stream[pos:pos + n])
        pos += n
        out += np.int32(len(g)).tobytes() + g.tobytes() + ch.db()
        if k in reset_db_after:
            ch.reset_db()
    return bytes(out)


def run_ref_rds_chain(stream: np.ndarray, chunks, tmp: Path, reset_db_after=()) -> bytes:
    """The reference chain's records through oracle/_ref/fm_rds_db_dump (in_sync written as 0: not observable there)."""
    tmp.mkdir(parents=True, exist_ok=True)
    np.ascontiguousarray(stream, dtype=np.uint8).tofile(tmp / "rds.bin")
    (tmp / "chunks.txt").write_text(" ".join(str(int(n)) for n in chunks))
    subprocess.run([str(REF_RDS_DB_DUMP), str(tmp / "rds.bin"), str(tmp / "chunks.txt"), str(tmp / "out.bin")] + [str(k) for k in reset_db_after],
                   check=True, capture_output=True)
    return (tmp / "out.bin").read_bytes()

