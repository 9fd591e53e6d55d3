#!/usr/bin/env python3
"""Record the reference's RDS decoding chain (oracle/_ref/fm_rds_db_dump, `make -C oracle -f rds_chain.mk ref`) on the streams of
tests/test_rds_chain_cpu.py, into rds_chain_records.json: per (stream, chunking) the size and sha256 of the harness's records (the groups
and the database after every chunk).  What that test compares against where oracle/_ref is absent.  Data only.

    python tests/golden/make_rds_chain_records.py
"""
from __future__ import annotations

import hashlib
import json
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "oracle")]

import rds_oracle as O  # noqa: E402
import test_rds_chain_cpu as RC  # noqa: E402


def main() -> None:
    assert O.have_ref_chain(), "build oracle/_ref/fm_rds_db_dump first: make -C oracle -f rds_chain.mk ref"
    rec = {}
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        for name in RC.STREAMS:
            for chunking in RC.CHUNKINGS:
                x, chunks, resets = RC.case(name, chunking, td)
                out = O.run_ref_rds_chain(x, chunks, td / "rds_chain", reset_db_after=resets)
                rec[RC.record_key(name, chunking)] = {"bytes": len(out), "sha256": hashlib.sha256(out).hexdigest()}
    O.RECORDS.write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print(O.RECORDS, O.RECORDS.stat().st_size, "bytes,", len(rec), "cases")


if __name__ == "__main__":
    main()
