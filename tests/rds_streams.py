"""Byte streams and chunk lists the RDS decoding chain's tests feed to the reference chain (oracle/_ref/fm_rds_db_dump), the oracle
(rds_oracle.RdsChain) and the GPU kernel (fmd_rdsdec_*, FMD_FLAG_RDS_DECODE).  Deterministic: every stream is a function of its name."""
from __future__ import annotations

import numpy as np

import rds_synth as RS

PI = 0xC201


def _bytes(bits: np.ndarray) -> np.ndarray:
    return RS.pack_bits(bits)


def _flip(bits: np.ndarray, positions) -> np.ndarray:
    b = bits.copy()
    for p in positions:
        b[p] ^= 1
    return b


def all_types() -> np.ndarray:
    """Every group type the reference decodes, version B groups and unsupported codes, behind 300 random bits (hunting)."""
    rng = np.random.default_rng(101)
    ps, rt, ptyn = b"ALLTYPES", b"Every group type the reference decodes, B versions and the rest.", b"PTYNAME!"
    g = []
    for k in range(8):
        g.append(RS.g0a(PI, k & 3, ps[2 * (k & 3): 2 * (k & 3) + 2], tp=k & 1, ta=(k >> 1) & 1, ms=(k >> 2) & 1, di=(k * 5 >> 1) & 1, pty=k + 3))
    g += [RS.g1a(PI, variant=v, day=v + 3, hour=v, minute=7 * v) for v in range(8)]
    g += [RS.g2a(PI, s, rt[4 * s: 4 * s + 4], pty=9) for s in range(16)]
    g += [RS.g3a(PI), RS.g4a(PI, 60586, 13, 45, lto=2), RS.g10a(PI, 0, ptyn[:4]), RS.g10a(PI, 1, ptyn[4:])]
    g += [RS.g11a(PI), RS.g14a(PI, variant=0), RS.g14a(PI, variant=4, data=0x0A0B), RS.g14a(PI, variant=12)]
    g += [RS.version_b(PI, code, low5=code, d=0x4142 + code) for code in range(16)]
    g += [RS.group_words(PI, code, False, 0x15, 0x1111 * (code & 3), 0x2222, 1, 17) for code in (5, 6, 7, 8, 9, 12, 13, 15)]
    bits = np.concatenate([rng.integers(0, 2, 300).astype(np.uint8), RS.encode_groups(g)])
    return _bytes(bits)


def ab_flips() -> np.ndarray:
    """RadioText / PTYN A/B flips, '\\r' characters, 2A / 10A groups whose block 3 arrives under C' (not C)."""
    g = []
    for ab in (0, 1, 1, 0, 0, 1):
        g += [RS.g2a(PI, s, (b"AB%d-" % ab) if s != 2 else b"x\rZ\r", ab=ab) for s in range(4)]
        g += [RS.g10a(PI, s, b"P%d\rq" % ab, ab=ab) for s in range(2)]
    g += [(RS.g2a(PI, 5, b"CPRM", ab=0), ("A", "B", "C'", "D")), (RS.g10a(PI, 0, b"NOTC", ab=0), ("A", "B", "C'", "D"))]
    g += [(RS.g0a(PI, 1, b"\r\r"), ("A", "B", "C'", "D")), RS.g0a(PI, 2, b"O\r")]
    return _bytes(RS.encode_groups(g))


def errors() -> np.ndarray:
    """Single-bit errors in data and checksum positions of every block, double-bit errors, three errored groups in a row (re-sync)."""
    base = [RS.g0a(PI, k & 3, b"ERRORSxx"[2 * (k & 3): 2 * (k & 3) + 2]) for k in range(64)]
    bits = RS.encode_groups(base)
    flips = []
    for k in range(4, 30):              # group k, block k % 4, bit position k - 4 of the 26: data bits 0..15, checksum bits 16..25
        flips.append(104 * k + 26 * (k % 4) + (k - 4))
    flips += [104 * 32 + 3, 104 * 32 + 9]                     # two errors in block A: uncorrectable
    flips += [104 * 33 + 26 + 20, 104 * 33 + 26 + 21]         # two errors in block B's checksum
    for k in (40, 41, 42):                                     # three errored groups in a row: back to FINDING_SYNC
        flips += [104 * k + 52 + 1, 104 * k + 52 + 12]
    flips += [104 * 50 + 78 + 5, 104 * 50 + 78 + 6, 104 * 51 + 40]
    return _bytes(_flip(bits, flips))


def dates() -> np.ndarray:
    """4A groups at MJD edges (0, the 17-bit maximum, leap days, century years) with negative and positive local time offsets,
    and 4A groups with block 3 under C' (no date) or an errored block 4 (date only)."""
    g = []
    for mjd, h, m, lto in [(0, 0, 0, 0), (0x1FFFF, 23, 59, -31), (51543, 23, 59, -1), (51544, 0, 0, 1), (51603, 12, 0, -24),
                           (15078, 1, 2, 24), (15079, 31, 63, -12), (60586, 13, 45, 2), (88069, 7, 30, -6), (65535, 22, 1, 31)]:
        g.append(RS.g4a(PI, mjd, h, m, lto))
    g.append((RS.g4a(PI, 60000, 5, 5, -3), ("A", "B", "C'", "D")))
    bits = RS.encode_groups(g + [RS.g4a(PI, 59000, 6, 6, 4)])
    bits = _flip(bits, [104 * len(g) + 78 + 2, 104 * len(g) + 78 + 3])   # the last group's block 4 uncorrectable
    return _bytes(bits)


def random_bytes(n: int = 1 << 20, seed: int = 7) -> np.ndarray:
    """Random bytes: false locks, hunting, errored groups."""
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def mixed(seed: int) -> np.ndarray:
    """A station-like stream with a seed of its own: random runs (hunting), the synthesiser's 0A / 2A / 4A mix with a PI / PS / RT
    of its own, and bit errors at a seed-dependent rate."""
    rng = np.random.default_rng(1000 + seed)
    pi = int(rng.integers(1, 0xFFFF))
    ps = "".join(chr(c) for c in rng.integers(0x20, 0x7F, 8))
    rt = "".join(chr(c) for c in rng.integers(0x20, 0x7F, 64))
    parts = []
    for _ in range(3):
        parts.append(rng.integers(0, 2, int(rng.integers(0, 400))).astype(np.uint8))
        b = RS.mixed_bits(int(rng.integers(104, 104 * 24)), pi, ps, rt)
        p_err = [0.0, 1e-3, 1e-2, 4e-2][seed % 4]
        parts.append(b ^ (rng.random(b.size) < p_err).astype(np.uint8))
    return _bytes(np.concatenate(parts))


def synthetic_streams() -> dict[str, np.ndarray]:
    return {"all_types": all_types(), "ab_flips": ab_flips(), "errors": errors(), "dates": dates(), "random_1MiB": random_bytes()}


def chunk_lists(n: int, seed: int = 3) -> dict[str, list[int]]:
    """Ways to cut a stream of n bytes: 16-byte chunks (the Manchester decoder's), odd sizes 0..37, one piece."""
    rng = np.random.default_rng(seed)
    odd, left = [], n
    while left > 0:
        k = min(left, int(rng.integers(0, 38)))
        odd.append(k)
        left -= k
    return {"chunk16": [16] * (n // 16) + ([n % 16] if n % 16 else []), "odd": odd, "whole": [n]}
