#!/usr/bin/env python3
"""Record the compiled reference's outputs on the inputs of the tests that compare against it, into ref_records.json.

Run where the reference can be built (`make -C oracle ref` must have produced oracle/_ref/):

    python tests/golden/make_ref_records.py

Data only, keyed by case:
  oracle_vs_ref/...       sha256 of the capture + a digest (dtype, size, sha256) of every stream fm_ref_dump writes
                          (tests/test_oracle_vs_ref.py)
  rds_group_sync/...      the RDS bytes, group log lines and lock lines of fm_ref_dump (tests/test_rds_group_sync.py)
  scraper_outputs/...     sha256 of the capture + size and sha256 of fm_demod_scraper's WAV and RDS files (tests/test_scraper_outputs.py)
"""
from __future__ import annotations

import json
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "oracle")]

import oraclelib as O  # noqa: E402
import test_oracle_vs_ref as V  # noqa: E402
import test_rds_group_sync as G  # noqa: E402
import test_scraper_outputs as S  # noqa: E402


def main() -> None:
    assert O.have_ref() and S.REF_SCRAPER.exists(), "build oracle/_ref first: make -C oracle ref"
    rec = {}
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)

        def chain(key, cap, **kw):
            rec[key] = {"capture_sha256": V.capture_sha256(cap), "streams": V.digests(O.run_ref_chain(cap, td / "chain", **kw))}

        cap = V.chain_capture()
        for bs, nb in V.CHAIN_CASES:
            chain(V.chain_key(bs, nb), cap[: bs * nb], block_size=bs)
        for args, _ in V.CONTROL_CASES:
            chain(V.controls_key(args), cap[: 65536 * 6], block_size=65536, extra_args=args)
        chain("oracle_vs_ref/cf32", V.cf32_capture(), block_size=65536, u8=False)
        chain("oracle_vs_ref/noise", V.noise_capture(), block_size=65536)
        import control_schedules as CS  # noqa: E402
        for name, sched, cf32 in V.schedule_cases():
            chain(V.schedule_key(name), V.schedule_capture(cf32), block_size=16384, u8=not cf32, extra_args=CS.ref_args(sched))

        for noise, seed in G.CASES:
            d = td / f"gs_{seed}"
            d.mkdir()
            groups, locks, rds = G._ref_log(G.capture(noise, seed), d)
            rec[G.record_key(noise, seed)] = {"groups": groups, "locks": locks, "rds_bytes_hex": rds.tobytes().hex()}

        cap = S.capture()
        d = td / "scraper"
        d.mkdir()
        wav, rds = S.reference_files(cap, d)
        rec[S.RECORD_KEY] = {"capture_sha256": V.capture_sha256(cap), "wav": S.file_record(wav), "rds": S.file_record(rds)}
    O.REF_RECORDS.write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print(O.REF_RECORDS, O.REF_RECORDS.stat().st_size, "bytes,", len(rec), "cases")


if __name__ == "__main__":
    main()
