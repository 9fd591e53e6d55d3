"""Batched audio resampler on the GPU (fmd_resampler_*, AudioResampler): the reference method bit for bit against the restatement of the
reference's Resample (tests/cpp/resample_ref.c, itself checked against the reference's outputs in test_resample_cpu.py), the polyphase
method against a float64 restatement of its definition, its streaming and batch invariances, what the two do to a tone, and the chain
from the demodulator's device views through the resampler."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import resample_ref
import station_pool as SP
import synth
from conftest import GOLDEN, bits_equal, describe_diff

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FS_IN = 32000
SCALE = np.float32(32767.0) * np.float32(0.95)


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return resample_ref.build(tmp_path_factory.mktemp("resample_ref_gpu"))


def pcm16(y: np.ndarray) -> np.ndarray:
    return (y * SCALE).astype(np.int32).astype(np.int16)


@pytest.fixture(scope="module")
def pool_audio(pkg):
    """Real demodulator audio of the 509 pool stations: 3 consecutive 64 ms blocks at 256 kSa/s, [3][509][2048][2] float32."""
    import torch
    pool = SP.Pool(256_000, True, blocks=3)
    bases = [SP.make_base(256_000, True, k, pool.base_len) for k in range(SP.N_BASES)]
    x = np.stack([pool.window(bases, i) for i in range(SP.P)])
    dm = pkg.BatchDemod(SP.P, pool.bs, 256_000, fast_math=True)
    blocks = []
    for b in range(3):
        dm.process(torch.from_numpy(np.ascontiguousarray(x[:, b * pool.bs:(b + 1) * pool.bs])).cuda())
        dm.synchronize()
        blocks.append(dm.audio_tensor().cpu().numpy().copy())
    dm.close()
    return np.stack(blocks)


@pytest.mark.parametrize("fs_out", [48000, 44100, 16000])
def test_reference_method_every_station_bit_identical(pkg, ref, pool_audio, fs_out):
    import torch
    rs = pkg.AudioResampler(SP.P, fs_out, method="reference", max_input_frames=2048)
    for b in range(3):
        x = torch.from_numpy(pool_audio[b]).cuda()
        y = rs.process(x).cpu().numpy()
        p = rs.process_pcm16(x).cpu().numpy()
        for c in range(SP.P):
            e = ref(pool_audio[b, c], fs_out)
            assert bits_equal(y[c], e), (b, c, describe_diff(y[c], e))
        assert np.array_equal(p, pcm16(y))


def test_reference_method_on_the_fixture(pkg):
    import torch
    g = np.load(GOLDEN / "resample_ref.npz")
    for key in (str(k) for k in g["cases"]):
        if key in {str(k) for k in g["rejected"]}:
            continue
        N, fs = (int(v[1:] if v[0] == "n" else v[2:]) for v in key.split("_"))
        rs = pkg.AudioResampler(1, fs, method="reference", max_input_frames=N)
        y = rs.process(torch.from_numpy(g[key + "_in"][None]).cuda()).cpu().numpy()[0]
        assert bits_equal(y, g[key + "_out"]), (key, describe_diff(y, g[key + "_out"]))
        p = rs.process_pcm16(torch.from_numpy(g[key + "_in"][None]).cuda()).cpu().numpy()[0]
        assert np.array_equal(p, pcm16(g[key + "_out"]))


def test_equal_rates_copy_and_drifting_call_is_rejected(pkg):
    import torch
    x = torch.randn(7, 1000, 2, device="cuda")
    for method in ("reference", "polyphase"):
        rs = pkg.AudioResampler(7, FS_IN, method=method, max_input_frames=4096)
        assert torch.equal(rs.process(x).view(torch.int32), x.view(torch.int32))
    rs = pkg.AudioResampler(3, 48000, method="reference", max_input_frames=16384)
    x = torch.randn(3, 16384, 2, device="cuda")
    out = torch.full((3, 24576, 2), 7.0, device="cuda")
    with pytest.raises(pkg.FmdError) as e:
        rs.process(x, out=out)
    assert e.value.status == -1                                             # FMD_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def _poly_expected(pkg, x, fs_out):
    taps, L, M = pkg.resampler_design(FS_IN, fs_out)
    n1 = -(-x.shape[1] * L // M)
    return np.stack([resample_ref.polyphase_f64(x[c], taps, L, M, 0, n1) for c in range(x.shape[0])])


@pytest.mark.parametrize("fs_out", [48000, 44100, 16000])
def test_polyphase_against_float64_restatement(pkg, pool_audio, fs_out):
    import torch
    x = np.concatenate([pool_audio[b, :64] for b in range(3)], axis=1)      # 64 stations x 3 blocks, one stream
    rs = pkg.AudioResampler(64, fs_out, method="polyphase", max_input_frames=2048)
    got = np.concatenate([rs.process(torch.from_numpy(np.ascontiguousarray(x[:, b * 2048:(b + 1) * 2048])).cuda()).cpu().numpy() for b in range(3)], axis=1)
    e = _poly_expected(pkg, x, fs_out)
    assert got.shape == e.shape
    err = np.max(np.abs(got - e))
    print(f"polyphase {fs_out}: max |err| vs float64 {err:.3e}")
    assert err < 7e-7   # measured 2.4e-7 (48 and 44.1 kHz), 3.4e-7 (16 kHz): DESIGN.md §6b


@pytest.mark.parametrize("fs_out", [48000, 44100])
def test_polyphase_streaming_is_split_invariant(pkg, fs_out):
    import torch
    rng = np.random.default_rng(5)
    n = 8192
    x = torch.from_numpy((0.3 * rng.standard_normal((5, n, 2))).astype(np.float32)).cuda()
    one = pkg.AudioResampler(5, fs_out, max_input_frames=n)
    whole = one.process(x).cpu().numpy()
    _, L, M = pkg.resampler_design(FS_IN, fs_out)
    assert whole.shape[1] == -(-n * L // M)
    for splits in ([2048] * 4, [1, 777, 2048, 3000, 8192 - 1 - 777 - 2048 - 3000]):
        rs = pkg.AudioResampler(5, fs_out, max_input_frames=n)
        parts, pos, counts = [], 0, []
        for k in splits:
            assert rs.output_frames(k) == -(-(pos + k) * L // M) - -(-pos * L // M)
            y = rs.process(x[:, pos:pos + k].contiguous())
            counts.append(y.shape[1])
            parts.append(y.cpu().numpy())
            pos += k
        assert bits_equal(np.concatenate(parts, axis=1), whole), splits
        if fs_out == 44100 and splits[0] == 2048:
            assert counts == [2823, 2822, 2823, 2822]


def test_polyphase_station_independent_of_batch_and_reset_is_per_channel(pkg, pool_audio):
    import torch
    x = pool_audio[0]                                                       # [509][2048][2]
    big = np.concatenate([x] * 8 + [x[: 4096 - 8 * SP.P]])                  # 4096 stations
    outs = {}
    for C, xs in ((1, x[200:201]), (SP.P, x), (4096, big)):
        rs = pkg.AudioResampler(C, 48000, max_input_frames=2048)
        outs[C] = rs.process(torch.from_numpy(np.ascontiguousarray(xs)).cuda()).cpu().numpy()
    assert bits_equal(outs[SP.P][200], outs[1][0]) and bits_equal(outs[4096][200], outs[1][0]) and bits_equal(outs[4096][SP.P + 200], outs[1][0])
    # reset(c): only channel c's history is cleared
    rs_a = pkg.AudioResampler(8, 48000, max_input_frames=2048)
    rs_b = pkg.AudioResampler(8, 48000, max_input_frames=2048)
    b0, b1 = (torch.from_numpy(np.ascontiguousarray(pool_audio[k, :8])).cuda() for k in (0, 1))
    rs_a.process(b0); rs_b.process(b0)
    rs_b.reset(3)
    ya, yb = rs_a.process(b1).cpu().numpy(), rs_b.process(b1).cpu().numpy()
    for c in range(8):
        assert bits_equal(ya[c], yb[c]) == (c != 3), c


def _tone_db(y: np.ndarray, fs: float, f: float) -> float:
    w = np.hanning(y.size)
    S = np.abs(np.fft.rfft(y * w)) / (w.sum() / 2)
    k = int(round(f * y.size / fs))
    return 20 * np.log10(S[max(k - 3, 0):k + 4].max() + 1e-30)


def _blocks(pkg, rs, x, bs=2048):
    """x [1][n][2] fed as the demodulator delivers it, one 64 ms block per call; channel 0 of the concatenated output"""
    import torch
    return np.concatenate([rs.process(torch.from_numpy(np.ascontiguousarray(x[:, i:i + bs])).cuda()).cpu().numpy()[0, :, 0]
                           for i in range(0, x.shape[1], bs)])


def test_tones(pkg):
    n = 2048 * 16
    t = np.arange(n) / FS_IN
    for method in ("polyphase", "reference"):
        # 1 kHz at 32 kHz comes out at 48 kHz as 1 kHz
        x = np.stack([np.sin(2 * np.pi * 1000 * t)] * 2, -1).astype(np.float32)[None]
        rs = pkg.AudioResampler(1, 48000, method=method, max_input_frames=2048)
        y = _blocks(pkg, rs, x)
        y = y[len(y) // 4:]
        assert _tone_db(y, 48000, 1000) > -1.0, method
        S = np.abs(np.fft.rfft(y * np.hanning(y.size)))
        assert abs(np.argmax(S) * 48000 / y.size - 1000) < 5, method
        # 12 kHz down to 16 kHz: the alias falls at 4 kHz
        x = np.stack([np.sin(2 * np.pi * 12000 * t)] * 2, -1).astype(np.float32)[None]
        rs = pkg.AudioResampler(1, 16000, method=method, max_input_frames=2048)
        y = _blocks(pkg, rs, x)
        y = y[len(y) // 4:]
        alias = _tone_db(y, 16000, 4000)
        print(method, "alias at 4 kHz", alias, "dB")
        if method == "polyphase":
            assert alias < -60.0
        else:
            assert alias > -20.0        # the reference's interpolator does not filter: why the polyphase method exists


def test_end_to_end_device_chain_with_output_lag(pkg, tmp_path):
    import torch
    C, bs, nb = 8, 16384, 8
    caps = np.stack([synth.to_cf32(synth.fm_capture(bs * nb, fs=256000.0, seed=40 + c, channel=c + 1)["iq"]) for c in range(C)])
    s = torch.cuda.Stream()
    # device-side: wait_outputs -> resample the audio view on the same stream -> release_outputs
    dm = pkg.BatchDemod(C, bs, 256_000, fast_math=True)
    dm.set_output_lag(True)
    rs = pkg.AudioResampler(C, 48000, max_input_frames=2048)
    got, order = [], []
    d_in = [torch.from_numpy(np.ascontiguousarray(caps[:, b * bs:(b + 1) * bs])).cuda() for b in range(nb)]   # alive until the end
    torch.cuda.synchronize()
    for b in range(nb):
        dm.submit(d_in[b])
        if dm.outputs_block() < 0:
            continue
        order.append(dm.outputs_block())
        dm.wait_outputs(s)
        with torch.cuda.stream(s):
            y = rs.process(dm.audio_tensor(), stream=s).clone()
        dm.release_outputs(s)
        got.append(y)
    torch.cuda.synchronize()
    got = torch.cat(got, 1).cpu().numpy()
    dm.close()
    # host-side: the same blocks through the host getter, resampled block by block
    dm = pkg.BatchDemod(C, bs, 256_000, fast_math=True)
    rs2 = pkg.AudioResampler(C, 48000, max_input_frames=2048)
    want = []
    for b in range(nb):
        dm.process(np.ascontiguousarray(caps[:, b * bs:(b + 1) * bs]))
        a = dm.audio()
        if b in order:
            want.append(rs2.process(torch.from_numpy(a).cuda()).cpu().numpy())
    dm.close()
    assert order == sorted(order) and len(order) >= nb - 1
    assert bits_equal(got, np.concatenate(want, 1))
    # the player adaptor: channel 0 at 48 kHz into a WAV file, against the pcm16 form of the same chain (exact mode, host process)
    exe = tmp_path / "resample_player_main"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'include'}", f"-I{ROOT / 'fm-radio_amd' / 'host'}", str(ROOT / "tests" / "cpp" / "resample_player_main.cpp"),
                    f"-L{ROOT / 'fm-radio_amd' / 'csrc'}", "-lfmdemod", f"-Wl,-rpath,{ROOT / 'fm-radio_amd' / 'csrc'}", "-o", str(exe)], check=True)
    C2, nb2 = 2, 3
    np.ascontiguousarray(caps[:C2, : bs * nb2]).tofile(tmp_path / "cap.cf32")
    subprocess.run([str(exe), str(tmp_path / "cap.cf32"), str(C2), str(bs), "256000", "48000", str(tmp_path / "o.wav")], check=True)
    dm = pkg.BatchDemod(C2, bs, 256_000)
    rs3 = pkg.AudioResampler(C2, 48000, max_input_frames=2048)
    pcm = []
    for b in range(nb2):
        dm.process(np.ascontiguousarray(caps[:C2, b * bs:(b + 1) * bs]))
        dm.synchronize()
        pcm.append(rs3.process_pcm16(dm.audio_tensor()).cpu().numpy()[0])
    dm.close()
    pcm = np.concatenate(pcm)
    wav = (tmp_path / "o.wav").read_bytes()
    assert wav[:4] == b"RIFF" and wav[8:12] == b"WAVE"
    assert int.from_bytes(wav[24:28], "little") == 48000 and int.from_bytes(wav[22:24], "little") == 2
    assert np.array_equal(np.frombuffer(wav[44:], np.int16).reshape(-1, 2), pcm)
