"""Scraper-compatible outputs: the host-side WAV / RDS-bytes writers against the files the reference's own
`fm_demod_scraper` produces (oracle/_ref/fm_demod_scraper, built from /root/reference).  CPU only: the writers are fed the
oracle's audio, which is bit-identical to the reference's.  Where oracle/_ref is absent, the reference scraper's two files for the
same capture are known by their sizes and sha256 from tests/golden/ref_records.json (tests/golden/make_ref_records.py)."""
import hashlib
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oraclelib as O
import synth

ROOT = Path(__file__).resolve().parent.parent
REF_SCRAPER = ROOT / "oracle" / "_ref" / "fm_demod_scraper"
RECORD_KEY = "scraper_outputs/seed=808"
BS, NB = 65536, 30


def capture() -> np.ndarray:
    return synth.to_u8(synth.fm_capture(BS * NB, seed=808)["iq"])


def file_record(data: bytes) -> dict:
    return {"size": len(data), "sha256": hashlib.sha256(data).hexdigest()}


def reference_files(cap, tmp_path) -> tuple[bytes, bytes]:
    """The reference scraper's (WAV, RDS bytes) files for the capture."""
    cap.tofile(tmp_path / "cap.u8")
    ref_dir = tmp_path / "ref"
    subprocess.run([str(REF_SCRAPER), "-i", str(tmp_path / "cap.u8"), "-o", str(ref_dir), "-b", str(BS)], check=True, stderr=subprocess.DEVNULL)
    return next(ref_dir.glob("*_audio.wav")).read_bytes(), next(ref_dir.glob("*_rds.bin")).read_bytes()


def test_wav_and_rds_files_match_reference_scraper(tmp_path):
    bs, nb = BS, NB
    cap = capture()
    if REF_SCRAPER.exists():
        ref_wav, ref_rds = reference_files(cap, tmp_path)
        ref_wav_rec, ref_rds_rec = file_record(ref_wav), file_record(ref_rds)
    else:
        rec = O.ref_records()[RECORD_KEY]
        if hashlib.sha256(cap.tobytes()).hexdigest() != rec["capture_sha256"]:
            pytest.skip("synthetic capture not bit-reproducible with this numpy build")
        ref_wav_rec, ref_rds_rec = rec["wav"], rec["rds"]

    o = O.run_chain(cap, bs, 1_024_000, u8=True, streams=["audio", "rds_sym"])
    o["audio"].tofile(tmp_path / "audio.f32")
    o["rds_bytes"].tofile(tmp_path / "rds_bytes.u8")
    exe = tmp_path / "scraper_writer_main"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'fm-radio_amd' / 'host'}", str(ROOT / "tests" / "cpp" / "scraper_writer_main.cpp"), "-o", str(exe)], check=True)
    subprocess.run([str(exe), str(tmp_path / "audio.f32"), str(tmp_path / "rds_bytes.u8"), str(bs // 32), str(tmp_path / "out.wav"), str(tmp_path / "out_rds.bin")], check=True)
    assert file_record((tmp_path / "out.wav").read_bytes()) == ref_wav_rec
    assert file_record((tmp_path / "out_rds.bin").read_bytes()) == ref_rds_rec
    assert ref_rds_rec["size"] > 0 and ref_wav_rec["size"] == 44 + nb * (bs // 32) * 4
