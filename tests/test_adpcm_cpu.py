"""ADPCM audio encoder, the parts that need no GPU: the C restatement (tests/cpp/adpcm_ref.c) against Python's audioop bit for bit, the
library's host-only functions against the restatement, the host-only unit as a stand-alone program under sanitizers (from source and
linked with the library as built), the conversion's known answers, the restatement's split invariance, flush, and every argument bound
from both sides.

audioop is part of the standard library up to Python 3.12: where it exists these tests run, none is skipped."""
import ctypes as C
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import adpcm_ref
from adpcm_ref import bits

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["fmd_adpcm_block_align", "fmd_adpcm_max_blocks", "fmd_adpcm_decode_blocks", "fmd_adpcm_wav_header", "fmd_adpcm_create", "fmd_adpcm_destroy",
           "fmd_adpcm_reset", "fmd_adpcm_process_f32_dev", "fmd_adpcm_flush", "fmd_adpcm_get_status", "fmd_adpcm_status_dev", "fmd_adpcm_last_error"]
SIZES = (9, 17, 1017)


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.build_library()
    return p


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return adpcm_ref.build(tmp_path_factory.mktemp("adpcm_ref"))


def _signals(S: int) -> dict:
    """the signals of the issue, each 6 blocks and a bit of S frames"""
    n = 6 * S + 5
    return {"noise -40 dB": adpcm_ref.noise(n, 0.01, 1), "noise -20 dB": adpcm_ref.noise(n, 0.1, 2), "noise -6 dB": adpcm_ref.noise(n, 0.5, 3),
            "sine 1 kHz": adpcm_ref.sine(n), "square, full scale": np.concatenate([adpcm_ref.square(n // 2, 2), adpcm_ref.square(n - n // 2, 64)]), "silence": adpcm_ref.silence(n), "edge ramp": adpcm_ref.edge_ramp(n)}


def test_symbols_are_declared_and_exported(pkg):
    declared = pkg.declared_symbols(debug=False)
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/fmdemod.h"
        assert hasattr(lib, s), f"{s} is not exported"
    assert lib.fmd_api_version() == 3
    for name in ("AdpcmEncoder", "AdpcmConfig", "ADPCM_STATUS_DTYPE", "adpcm_decode", "adpcm_block_align", "adpcm_wav_header", "adpcm_max_blocks"):
        assert hasattr(pkg, name)
    assert pkg.ADPCM_STATUS_DTYPE == adpcm_ref.STATUS_DTYPE and pkg.ADPCM_STATUS_DTYPE.itemsize == 64
    assert pkg.ADPCM_DEFAULT_BLOCK_FRAMES == adpcm_ref.DEFAULT_S and pkg.ADPCM_WAV_HEADER_BYTES == 60


@pytest.mark.parametrize("S", SIZES)
def test_restatement_equals_audioop(ref, S):
    """Every block of every signal: the header is the first frame's q and the index carried in; the codes, repacked (audioop puts the
    earlier sample into the high nibble), are audioop.lin2adpcm's from (header sample, that index); the index audioop leaves is the next
    block's header index; and the restatement's decoder gives audioop.adpcm2lin's samples."""
    import audioop  # noqa: F401  (present: the test runs)
    for name, x in _signals(S).items():
        ch = ref.channel(S)
        blocks = ch.process(x)
        assert blocks.shape == (6, adpcm_ref.block_align(S)), name
        q, _ = ref.sample(x)
        index = [0, 0]
        pcm = ref.decode(blocks, S)
        for b in range(6):
            p = adpcm_ref.parse_block(blocks[b], S)
            qb = q[b * S:(b + 1) * S]
            assert p["sample"] == [int(qb[0, 0]), int(qb[0, 1])] and p["index"] == index and p["zero"] == [0, 0], (name, b)
            codes, index, pred = adpcm_ref.audioop_block(qb, index)
            for rail in range(2):
                assert np.array_equal(p["codes"][rail], codes[rail]), (name, b, rail)
            assert np.array_equal(pcm[b * S:(b + 1) * S], adpcm_ref.audioop_decode_block(p, S)), (name, b)
            assert pcm[(b + 1) * S - 1].tolist() == pred, (name, b)                # the decoder tracks the encoder's predictor
        # the open seventh block: its header frame and four codes, carried in the record
        _, index, pred = adpcm_ref.audioop_block(q[6 * S:], index)
        st = ch.status()[0]
        assert st["index"].tolist() == index and st["pred"].tolist() == pred, name
        assert int(st["fill"]) == 5 and int(st["blocks"]) == 6 and int(st["frames"]) == 6 * S + 5 and int(st["padded"]) == 0, name
        if name == "square, full scale":
            # the index reaches 88 and the predictor both clamps; every sample is past full scale and counted
            index_path, i = [], 0
            for b in range(6):
                for code in adpcm_ref.parse_block(blocks[b], S)["codes"][0]:
                    i = max(0, min(88, i + (-1, -1, -1, -1, 2, 4, 6, 8)[code & 7]))
                    index_path.append(i)
            assert max(index_path) == 88, (S, max(index_path))
            assert pcm.max() == 32767 and pcm.min() == -32768, (S, pcm.max(), pcm.min())
            assert int(st["clipped"][0]) == 6 * S + 5 == int(st["clipped"][1])
        if name == "silence":
            assert not blocks.any() and st["index"].tolist() == [0, 0]


def test_steps_against_audioop_from_every_index(ref):
    """single steps from every index, at differences around the three thresholds and at the predictor's clamps"""
    import audioop
    rng = np.random.default_rng(7)
    for index in range(89):
        for pred in (-32768, -30000, -1, 0, 12345, 32767):
            for q in list(rng.integers(-32768, 32768, 6)) + [pred, -32768, 32767]:
                code, p2, i2 = ref.step(int(q), pred, index)
                # audioop packs two codes a byte: the step under test first, a second sample behind it
                data, _ = audioop.lin2adpcm(struct.pack("<hh", int(q), int(q)), 2, (pred, index))
                assert data[0] >> 4 == code, (index, pred, q)
                one, (p1, i1) = audioop.adpcm2lin(bytes([code << 4]), 2, (pred, index))
                # (adpcm2lin decodes both nibbles of the byte: the state after the first is read from its first sample)
                assert struct.unpack("<hh", one)[0] == p2, (index, pred, q)
                assert i2 == max(0, min(88, index + (-1, -1, -1, -1, 2, 4, 6, 8)[code & 7]))


def test_library_host_functions_equal_the_restatement(pkg, ref):
    lib = ref.lib
    for S in (0, 9, 17, 1017, 1025, 8185):
        Sv = S or 1017
        assert pkg.adpcm_block_align(S) == lib.adpcm_ref_block_align(Sv) == 8 * ((Sv - 1) // 8 + 1)
        for n in (0, 1, Sv - 1, Sv, Sv + 1, 2048, 1 << 30):
            assert pkg.adpcm_max_blocks(S, n) == lib.adpcm_ref_max_blocks(Sv, n) == (Sv - 1 + n) // Sv
    assert pkg.adpcm_block_align(0) == 1024 and pkg.adpcm_max_blocks(0, 2048) == 3
    for S in (1, 8, 10, 1016, 8193, -9):
        with pytest.raises(pkg.FmdError) as e:
            pkg.adpcm_block_align(S)
        assert e.value.status == -1
        with pytest.raises(pkg.FmdError):
            pkg.adpcm_max_blocks(S, 5)
    with pytest.raises(pkg.FmdError):
        pkg.adpcm_max_blocks(9, -1)
    # the decoder over the restatement's blocks of every signal
    for S in SIZES:
        for name, x in _signals(S).items():
            blocks = ref.channel(S).process(x)
            assert np.array_equal(pkg.adpcm_decode(blocks, S), ref.decode(blocks, S)), (S, name)
    assert pkg.adpcm_decode(b"", 9).shape == (0, 2)
    bad = np.zeros(16, np.uint8)
    bad[6] = 89
    with pytest.raises(pkg.FmdError) as e:
        pkg.adpcm_decode(bad, 9)
    assert e.value.status == -1
    with pytest.raises(ValueError):
        pkg.adpcm_decode(np.zeros(15, np.uint8), 9)


def _parse_wav_header(h: bytes) -> dict:
    """every field of the 60 bytes, by struct"""
    riff, riff_size, wave = struct.unpack_from("<4sI4s", h, 0)
    fmt, fmt_size, tag, channels, fs, avg, align, bps, cb, spb = struct.unpack_from("<4sIHHIIHHHH", h, 12)
    fact, fact_size, frames = struct.unpack_from("<4sII", h, 40)
    data, data_size = struct.unpack_from("<4sI", h, 52)
    return dict(riff=riff, riff_size=riff_size, wave=wave, fmt=fmt, fmt_size=fmt_size, tag=tag, channels=channels, fs=fs, avg=avg, align=align, bps=bps, cb=cb, spb=spb,
                fact=fact, fact_size=fact_size, frames=frames, data=data, data_size=data_size)


def _want_wav_header(fs, S, nb, frames) -> dict:
    align = 8 * ((S - 1) // 8 + 1)
    return dict(riff=b"RIFF", riff_size=52 + nb * align, wave=b"WAVE", fmt=b"fmt ", fmt_size=20, tag=0x0011, channels=2, fs=fs, avg=fs * align // S, align=align, bps=4,
                cb=2, spb=S, fact=b"fact", fact_size=4, frames=frames, data=b"data", data_size=nb * align)


def test_wav_header_field_by_field(pkg):
    for fs, S, nb, frames in ((32000, 1017, 3, 3000), (48000, 9, 0, 0), (44100, 8185, 11, 11 * 8185), (8000, 17, 1, 1), (32000, 0, 100, 100 * 1017 - 1016)):
        h = pkg.adpcm_wav_header(fs, S, nb, frames)
        assert len(h) == 60 == pkg.ADPCM_WAV_HEADER_BYTES
        assert _parse_wav_header(h) == _want_wav_header(fs, S or 1017, nb, frames), (fs, S, nb, frames)
    assert _parse_wav_header(pkg.adpcm_wav_header(32000, 1017, 1, 1017))["avg"] == 32220     # 32000 * 1024 / 1017 in integers
    for args, status in (((0, 9, 1, 1), -1), ((1000001, 9, 1, 1), -1), ((32000, 9, -1, 0), -1), ((32000, 9, 1, 10), -1), ((32000, 9, 1, -1), -1), ((32000, 10, 1, 1), -1),
                         ((32000, 1017, (0xffffffff - 52) // 1024 + 1, 0), -2)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.adpcm_wav_header(*args)
        assert e.value.status == status, args
    pkg.adpcm_wav_header(32000, 1017, (0xffffffff - 52) // 1024, 0)
    pkg.adpcm_wav_header(1, 9, 1, 9)
    pkg.adpcm_wav_header(1000000, 9, 1, 0)


_CHECKS = "0 -1 -1 0 0 -1 -1 0 0 -1 0 -1 0 -1 -1 -1"       # adpcm_design_main.cpp's sixteen process calls, in its order
_WAV_CODES = "-1 0 0 -1 -1 0 -1 -1 0 -2 -1"


def _run_design_main(exe, tmp_path, ref, sanitized):
    sizes = (0, 9, 17, 1017, 8185)
    r = subprocess.run([str(exe), str(tmp_path)] + [str(s) for s in sizes], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    if sanitized:
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == 2 * len(sizes) + 4
    for S, line in zip(sizes, lines):
        Sv = S or 1017
        align = 8 * ((Sv - 1) // 8 + 1)
        assert [int(v) for v in line.split()] == [S, align, 0, 1, 1 + (Sv - 1) // Sv, (Sv - 1 + 2048) // Sv], S
        blocks = np.fromfile(tmp_path / f"blocks_{Sv}.u8", np.uint8)
        pcm = np.fromfile(tmp_path / f"pcm_{Sv}.i16", np.int16).reshape(-1, 2)
        assert blocks.size == 5 * align and np.array_equal(pcm, ref.decode(blocks, Sv)), S
        assert pcm[0].tolist() == [32767, -32768]
    bad = lines[len(sizes)].split()
    want = []
    for S in (1, 8, 10, 16, 1016, 1018, 1025, 8177, 8186, 8193, -7):
        ok = 9 <= S <= 8185 and S % 8 == 1
        want += [str(8 * ((S - 1) // 8 + 1)), str((S + 4) // S), str(S)] if ok else ["-1", "-1", "0"]
    assert bad == want + ["-1", str((8 + (1 << 62)) // 9)]
    for k, S in enumerate(sizes):
        Sv = S or 1017
        assert _parse_wav_header(bytes.fromhex(lines[len(sizes) + 1 + k])) == _want_wav_header(32000 + 2 + k, Sv, 7, 7 * Sv - 3), S
    assert lines[-3] == _WAV_CODES and lines[-2] == _CHECKS


def test_host_unit_under_sanitizers(ref, tmp_path):
    """fmd_adpcm_design.cpp and tests/cpp/adpcm_design_main.cpp, built with -fsanitize=address,undefined and run as a stand-alone program:
    clean; the decoder writes exactly its buffer and gives the restatement's samples; the headers parse field by field; the process
    call's checks hold each bound from both sides"""
    exe = tmp_path / "adpcm_design_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{csrc}", str(csrc / "fmd_adpcm_design.cpp"),
                    str(ROOT / "tests" / "cpp" / "adpcm_design_main.cpp"), "-o", str(exe)], check=True)
    _run_design_main(exe, tmp_path, ref, True)


def test_library_host_unit_as_built(pkg, ref, tmp_path):
    """the same program, itself under the sanitizers, linked with libfmdemod.so as it is built (its compiler and flags)"""
    exe = tmp_path / "adpcm_design_lib"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{csrc}",
                    str(ROOT / "tests" / "cpp" / "adpcm_design_main.cpp"), f"-L{csrc}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    _run_design_main(exe, tmp_path, ref, True)


def test_conversion_known_answers(ref):
    s = float(adpcm_ref.SCALE)                                               # 31128.65 in fp32
    x = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 1e-42, -1e-42, 0.9999, 3.2e-5, -3.3e-5, 1.05, -1.05], np.float32)
    q, fl = ref.sample(x)
    want = (x * adpcm_ref.SCALE).astype(np.int32)                            # (int16)(int)(x * scale): one fp32 multiply, truncated toward zero
    assert np.array_equal(q, want) and not fl.any() and q.tolist()[:6] == [0, 0, 15564, -15564, 31128, -31128] and q.tolist()[-2:] == [32685, -32685]
    assert np.array_equal(q.astype(np.int16), want.astype(np.int16))
    # NaN and both infinities give 0 and are counted; so does a finite sample whose product overflows
    q, fl = ref.sample(np.array([np.nan, np.inf, -np.inf, 3.0e38, -3.0e38], np.float32))
    assert q.tolist() == [0] * 5 and fl.tolist() == [2] * 5
    # the clamp from both sides: the last sample that converts to 32767 and the first that is clamped, and the same at -32768
    def last_below(limit, toward):
        """the float32 x nearest `toward`'s far side whose product with the scale has not reached `limit`"""
        x = np.float32(limit) / adpcm_ref.SCALE
        reached = (lambda v: np.float32(v * adpcm_ref.SCALE) >= np.float32(limit)) if limit > 0 else (lambda v: np.float32(v * adpcm_ref.SCALE) <= np.float32(limit))
        while not reached(x):
            x = np.nextafter(x, np.float32(toward))
        while reached(x):
            x = np.nextafter(x, np.float32(0.0))
        return x
    up, lo = last_below(32768.0, 2.0), last_below(-32769.0, -2.0)
    q, fl = ref.sample(np.array([up, np.nextafter(up, np.float32(2.0)), lo, np.nextafter(lo, np.float32(-2.0)), 1e9, -1e9, 1e30, -1e30], np.float32))
    assert q.tolist() == [32767, 32767, -32768, -32768, 32767, -32768, 32767, -32768] and fl.tolist() == [0, 1, 0, 1, 1, 1, 1, 1], (q, fl, s)
    # through a station: the counts per rail
    ch = ref.channel(9)
    x = np.zeros((20, 2), np.float32)
    x[3, 0] = 2.0; x[4, 0] = -2.0; x[5, 1] = 1.5; x[7, 0] = np.nan; x[8, 1] = np.inf; x[9, 1] = -np.inf
    ch.process(x)
    st = ch.status()[0]
    assert st["clipped"].tolist() == [2, 1] and int(st["nonfinite"]) == 3 and int(st["frames"]) == 20 and int(st["blocks"]) == 2 and int(st["fill"]) == 2


@pytest.mark.parametrize("S", SIZES)
def test_restatement_split_invariance(ref, S):
    """one call, a call per frame, and ragged calls: the same blocks and the same record"""
    x = np.concatenate([adpcm_ref.noise(2 * S + 3, 0.2, 5), adpcm_ref.square(S), adpcm_ref.sine(S + 11, a=0.9)])
    n = x.shape[0]
    whole = ref.channel(S)
    want = whole.process(x)
    per_frame = ref.channel(S)
    got = [per_frame.process(x[i:i + 1]) for i in range(n)]
    assert np.array_equal(np.concatenate(got), want) and np.array_equal(bits(per_frame.status()), bits(whole.status()))
    assert bytes(per_frame.c.open[:per_frame.align]) == bytes(whole.c.open[:whole.align])
    ragged = ref.channel(S)
    got, a = [], 0
    for step in (1, 7, 8, 9, S - 1, S, S + 1, 0, 127, 128, 129, n):
        b = min(a + step, n)
        got.append(ragged.process(x[a:b]))
        a = b
    assert a == n and np.array_equal(np.concatenate(got), want) and np.array_equal(bits(ragged.status()), bits(whole.status()))


@pytest.mark.parametrize("S", SIZES)
def test_flush(ref, S):
    """padded = S - fill; nothing happens at fill 0; the flushed block decodes to the real frames and then settles on the last frame
    without a jump at the padding's start; the index is carried on into the next block's header"""
    fill = 5 if S > 9 else 4
    x = adpcm_ref.sine(S + fill, a=0.5)
    ch = ref.channel(S)
    first = ch.process(x)
    assert first.shape[0] == 1 and ch.fill == fill
    before = ch.status()[0].copy()
    blk = ch.flush()
    st = ch.status()[0]
    assert blk.shape[0] == 1 and int(st["padded"]) == S - fill and int(st["fill"]) == 0 and int(st["blocks"]) == 2 and int(st["frames"]) == S + fill
    assert st["clipped"].tolist() == before["clipped"].tolist() and int(st["nonfinite"]) == 0
    # the same block as encoding the repeats as real frames
    twin = ref.channel(S)
    got = twin.process(np.concatenate([x, np.repeat(x[-1:], S - fill, axis=0)]))
    assert np.array_equal(got[1:], blk) and twin.status()[0]["index"].tolist() == st["index"].tolist() and twin.status()[0]["pred"].tolist() == st["pred"].tolist()
    pcm = ref.decode(blk, S).astype(np.int32)
    q, _ = ref.sample(x)
    last = q[-1].astype(np.int32)
    # the real frames, then the padding: the decoder moves on from where it stood, by no more than it moved between real frames (a new
    # header there would jump to the exact sample), and with ~1000 repeats it settles on the last frame within the smallest steps
    real = np.concatenate([ref.decode(first, S).astype(np.int32), pcm[:fill]])
    assert np.abs(pcm[fill] - pcm[fill - 1]).max() <= np.abs(np.diff(real, axis=0)).max()
    if S == 1017:
        assert np.abs(pcm[-100:] - last).max() <= 16
    # flush at fill 0: nothing
    before = bits(ch.status()).copy()
    assert ch.flush().shape[0] == 0 and np.array_equal(bits(ch.status()), before)
    # the next block's header carries the index
    nxt = ch.process(adpcm_ref.sine(S, a=0.5, start=S + fill))
    assert adpcm_ref.parse_block(nxt[0], S)["index"] == st["index"].tolist()
    fresh = ref.channel(S)
    assert fresh.flush().shape[0] == 0 and not bits(fresh.status()).any()


def test_argument_bounds_of_the_restatement_and_the_library(pkg, ref):
    """block_frames from both sides of every bound (the process call's bounds: adpcm_design_main.cpp's sixteen calls above)"""
    for S, ok in ((9, True), (8, False), (1, False), (17, True), (16, False), (18, False), (8185, True), (8177, True), (8193, False), (8186, False), (0, True), (-1, False)):
        assert (ref.lib.adpcm_ref_block_frames(S) != 0) == ok, S
        if ok:
            assert ref.channel(S).S == (S or 1017)
        else:
            with pytest.raises(ValueError):
                ref.channel(S)
    # create's checks come before the device is looked for
    for args, text in (((0, 9), "n_channels 0 is not positive or max_input_frames 65536 outside (0, 2^30]"), ((2, 9, 0), None), ((2, 9, (1 << 30) + 1), None),
                       ((2, 10), "block_frames 10 is neither 0 nor 1 (mod 8) in 9 ... 8185"), ((2, 8193), None), ((2, 1), None)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.AdpcmEncoder(*args)
        assert e.value.status == -1, args
        if text:
            assert str(e.value) == f"fmdemod status -1: {text}"
    lib = pkg.load_library()
    assert lib.fmd_adpcm_destroy(None) == -1 and lib.fmd_adpcm_reset(None, 0) == -1 and lib.fmd_adpcm_flush(None, 0, None, 0, None, None) == -1
    assert lib.fmd_adpcm_process_f32_dev(None, None, 0, 0, None, None, 0, None, None) == -1 and lib.fmd_adpcm_get_status(None, None) == -1
    assert C.sizeof(pkg.AdpcmConfig) == 24


def test_quality_figures_through_the_library(pkg, ref):
    """For the record: a -12 dBFS 1 kHz sine at 32 kHz, S = 1017, decoded by the library's decoder against the 16-bit
    samples it was made from.  No bar beyond sanity: ADPCM at 4 bits is worth more than 20 dB on a sine, and the first block, which starts
    at index 0, is the worst."""
    S = 1017
    x = adpcm_ref.sine(8 * S, a=0.25)
    x[:, 1] = x[:, 0]
    blocks = ref.channel(S).process(x)
    pcm = pkg.adpcm_decode(blocks, S)
    q, _ = ref.sample(x)
    first, rest = adpcm_ref.snr_db(q[:S], pcm[:S]), adpcm_ref.snr_db(q[S:], pcm[S:])
    print(f"SNR of a -12 dBFS 1 kHz sine, S = 1017: first block {first:.1f} dB, from the second block on {rest:.1f} dB")
    assert first > 20.0 and rest > 30.0 and rest > first
