"""TEST INFRASTRUCTURE: RDS group synthesis for the decoding chain's tests (tests/rds_streams.py, tests/test_gpu_rds_decode.py).

A generic "these groups -> bit stream" encoder with any offset word per block (C' included), group builders for the types the reference's
decoder handles (reference src/rds_decoder/rds_decoder.cpp:82-540: 0A, 1A, 2A, 3A, 4A, 10A, 11A, 14A) and for version B groups, and
synth.fm_capture_realistic with a programme service name and radiotext of the station's own.  Coding constants as synth.py's
(reference rds_constants.h:15-28); synth.py itself is left as it is.
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np

import synth

OFFSETS = {**synth.RDS_OFFSET, "C'": 0x350}   # C' (C1): rds_constants.h:22


def block_bits(data16: int, offset: str) -> list[int]:
    word = ((data16 & 0xFFFF) << 10) | (synth.rds_crc10(data16 & 0xFFFF) ^ OFFSETS[offset])
    return [(word >> (25 - i)) & 1 for i in range(26)]


def encode_groups(groups, offsets=("A", "B", "C", "D")) -> np.ndarray:
    """Bits (uint8 0/1) of `groups`: each an (A, B, C, D) word tuple, or (words, offsets) to choose e.g. C' for block 3."""
    bits: list[int] = []
    for g in groups:
        words, offs = (g[0], g[1]) if isinstance(g[0], (tuple, list)) else (g, offsets)
        for w, o in zip(words, offs):
            bits += block_bits(int(w), o)
    return np.array(bits, dtype=np.uint8)


def pack_bits(bits: np.ndarray) -> np.ndarray:
    """0/1 bits, MSB first, to the bytes a Manchester decoder emits (a short last byte padded with zeros)."""
    return np.packbits(np.asarray(bits, dtype=np.uint8))


def group_words(pi: int, code: int, version_b: bool, low5: int, c: int, d: int, tp: int = 0, pty: int = 0) -> tuple[int, int, int, int]:
    """(A, B, C, D) of a group: block B = group code, version, TP, PTY and the type-specific 5 low bits; version B repeats PI in C'."""
    b = ((code & 15) << 12) | (int(version_b) << 11) | ((tp & 1) << 10) | ((pty & 31) << 5) | (low5 & 31)
    return (pi & 0xFFFF, b, (pi if version_b else c) & 0xFFFF, d & 0xFFFF)


def g0a(pi, seg, chars2: bytes, tp=0, ta=0, ms=1, di=0, pty=0, af=0xE0CD):
    return group_words(pi, 0, False, (ta << 4) | (ms << 3) | (di << 2) | (seg & 3), af, (chars2[0] << 8) | chars2[1], tp, pty)


def g1a(pi, variant=0, data12=0x0E1, day=15, hour=12, minute=30, paging=3, pty=0):
    return group_words(pi, 1, False, paging, ((variant & 7) << 12) | (data12 & 0xFFF), ((day & 31) << 11) | ((hour & 31) << 6) | (minute & 63), 0, pty)


def g2a(pi, seg, chars4: bytes, ab=0, pty=0):
    return group_words(pi, 2, False, (ab << 4) | (seg & 15), (chars4[0] << 8) | chars4[1], (chars4[2] << 8) | chars4[3], 0, pty)


def g3a(pi, app_code=0b01100, message=0x1234, aid=0xCD46, pty=0):
    return group_words(pi, 3, False, app_code, message, aid, 0, pty)


def g4a(pi, mjd, hour, minute, lto=0, pty=0):
    """Clock time and date; lto in half hours, signed."""
    sign, val = (1, -lto) if lto < 0 else (0, lto)
    c = ((mjd & 0x7FFF) << 1) | ((hour >> 4) & 1)
    d = ((hour & 15) << 12) | ((minute & 63) << 6) | (sign << 5) | (val & 31)
    return group_words(pi, 4, False, (mjd >> 15) & 3, c, d, 0, pty)


def g10a(pi, seg, chars4: bytes, ab=0, pty=0):
    return group_words(pi, 10, False, (ab << 4) | (seg & 1), (chars4[0] << 8) | chars4[1], (chars4[2] << 8) | chars4[3], 0, pty)


def g11a(pi, low5=0b00101, c=0xBEEF, d=0x5A5A, pty=0):
    return group_words(pi, 11, False, low5, c, d, 0, pty)


def g14a(pi, variant=0, data=0x4142, pi_on=0xC0DE, tp_on=1, pty=0):
    return group_words(pi, 14, False, (tp_on << 4) | (variant & 15), data, pi_on, 0, pty)


def version_b(pi, code, low5=0, d=0x2020, pty=0):
    """A version-B group of any type (block 3 carries PI under offset C'); the reference decodes none of them."""
    return (group_words(pi, code, True, low5, 0, d, 0, pty), ("A", "B", "C'", "D"))


def mixed_bits(n_bits: int, pi: int, ps: str, rt: str) -> np.ndarray:
    """synth.rds_bitstream_mixed (0A / 2A alternating, a 4A every 16 groups) with the station's own PS (8) and RT (64 characters)."""
    with station_texts(ps, rt):
        return synth.rds_bitstream_mixed(n_bits, pi)[0]


@contextlib.contextmanager
def station_texts(ps: str, rt: str):
    """Inside: synth's 0A / 2A builders carry this PS / RT (synth.rds_bitstream_mixed and fm_capture_realistic look them up at call time)."""
    assert len(ps) == 8 and len(rt) == 64
    saved = synth.rds_group_0a, synth.rds_group_2a
    synth.rds_group_0a = functools.partial(saved[0], ps_name=ps)
    synth.rds_group_2a = functools.partial(saved[1], text=rt)
    try:
        yield
    finally:
        synth.rds_group_0a, synth.rds_group_2a = saved


def capture_realistic(n_samples: int, ps: str, rt: str, **kw) -> dict:
    """synth.fm_capture_realistic (PI 0x1234 + channel) whose 0A / 2A groups carry `ps` / `rt`."""
    with station_texts(ps, rt):
        return synth.fm_capture_realistic(n_samples, **kw)
