"""Batched audio mixer on the GPU (fmd_mixer_*, AudioMixer): the reference's own UpdateMixer outputs (tests/golden/mix_ref.npz) through the
library, and everything else bit for bit against the C restatement of the reference's rule (tests/cpp/mix_ref.c, itself checked against
the fixture in test_mix_cpu.py): the reference app's shape (4096 one-station buses), mixed membership with a device `active` mask, stride,
split and control invariances, argument errors, and the chain from the demodulator through the resampler and the mixer to a WAV file."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mix_ref
import station_pool as SP
import synth
from conftest import GOLDEN, bits_equal, describe_diff

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SCALE = np.float32(32767.0) * np.float32(0.95)


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    import torch
    assert torch.cuda.is_available()
    return fmradio_loader.load()


@pytest.fixture(scope="module")
def mix(tmp_path_factory):
    return mix_ref.build(tmp_path_factory.mktemp("mix_ref_gpu"))


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _expected(mix, x, buses, gains, active=None, n=None):
    n = x.shape[1] if n is None else n
    xs = np.ascontiguousarray(x[:, :n])
    return np.stack([mix(xs, b, active, g) if len(b) else np.zeros((n, 2), np.float32) for b, g in zip(buses, gains)])


def test_fixture_cases_bit_identical(pkg):
    """Every recorded case, once as its own bus (every case's bus is below 256 sources: the streaming kernel) and once padded with 256
    silent rows after its sources, which changes nothing in the reference's rule and moves every bus onto the staged kernel."""
    import torch
    g = np.load(GOLDEN / "mix_ref.npz")
    for key in (str(c) for c in g["cases"]):
        x, act, gain, want = mix_ref.fixture_case(g, key)
        nreg = x.shape[0]
        m = pkg.AudioMixer(nreg, [list(range(nreg))], gains=[gain])
        got = m.process(_cuda(x), active=_cuda(act)).cpu().numpy()[0]
        assert bits_equal(got, want), (key, describe_diff(got, want))
        xp = np.concatenate([x, np.full((256,) + x.shape[1:], 0.5, np.float32)])
        ap = np.concatenate([act, np.zeros(256, np.uint8)])
        m = pkg.AudioMixer(nreg + 256, [list(range(nreg + 256))], gains=[gain])
        got = m.process(_cuda(xp), active=_cuda(ap)).cpu().numpy()[0]
        assert bits_equal(got, want), ("padded " + key, describe_diff(got, want))
        if act.all():
            m = pkg.AudioMixer(nreg, [list(range(nreg))], gains=[gain])
            assert bits_equal(m.process(_cuda(x)).cpu().numpy()[0], want), key
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def pool48(pkg):
    """Real demodulator audio of the 509 pool stations (64 ms at 256 kSa/s), through the resampler's reference method to 48 kHz, tiled to
    4096 rows: [4096][3072][2] float32 on the host."""
    import torch
    pool = SP.Pool(256_000, True, blocks=1)
    bases = [SP.make_base(256_000, True, k, pool.base_len) for k in range(SP.N_BASES)]
    x = np.stack([pool.window(bases, i) for i in range(SP.P)])
    dm = pkg.BatchDemod(SP.P, pool.bs, 256_000, fast_math=True)
    dm.process(torch.from_numpy(np.ascontiguousarray(x[:, :pool.bs])).cuda())
    dm.synchronize()
    a = dm.audio_tensor().clone()
    dm.close()
    rs = pkg.AudioResampler(SP.P, 48000, method="reference", max_input_frames=a.shape[1])
    y = rs.process(a).cpu().numpy()
    return np.concatenate([y] * 8 + [y[: 4096 - 8 * SP.P]])


def test_one_station_buses_every_station(pkg, mix, pool48):
    """The reference app's own shape: 4096 buses of one station each, random gains (a third of them clip)."""
    rng = np.random.default_rng(7)
    C = pool48.shape[0]
    gains = rng.uniform(0.3, 6.0, C).astype(np.float32)
    m = pkg.AudioMixer(C, [[c] for c in range(C)], gains=gains)
    got = m.process(_cuda(pool48)).cpu().numpy()
    for c in range(C):
        e = mix(pool48[c:c + 1], [0], None, gains[c])
        assert bits_equal(got[c], e), (c, describe_diff(got[c], e))
    assert (np.abs(got) == 1.0).any()


def _membership(C, rng):
    buses = [[], [5], [7, 7], list(rng.integers(0, C, 23)), list(rng.integers(0, 64, 25)), list(range(64)), list(range(C)),
             list(rng.permutation(C)[:300]) + [3, 3, 3], list(range(C)) + list(range(0, C, 2))]
    gains = np.float32([1.0, 1.5, 0.7, 1.0, 2.0, 3.0, 1.0, 0.9, 0.25])
    return buses, gains


def test_mixed_membership_with_a_device_active_mask(pkg, mix):
    import torch
    rng = np.random.default_rng(11)
    C, n = 4096, 1000
    x = (0.4 * rng.standard_normal((C, n, 2))).astype(np.float32)
    buses, gains = _membership(C, rng)
    m = pkg.AudioMixer(C, buses, gains=gains)
    for p_on in (1.0, 0.6, 0.02):
        active = (rng.random(C) < p_on).astype(np.uint8)
        got = m.process(_cuda(x), active=_cuda(active) if p_on < 1.0 else None).cpu().numpy()
        want = _expected(mix, x, buses, gains, active if p_on < 1.0 else None)
        for b in range(len(buses)):
            assert bits_equal(got[b], want[b]), (p_on, b, len(buses[b]), describe_diff(got[b], want[b]))
    # a bool mask and a mask with nothing delivering
    got = m.process(_cuda(x), active=torch.zeros(C, dtype=torch.bool, device="cuda")).cpu().numpy()
    assert not got.any() and not np.signbit(got).any()


def test_strides_splits_and_controls(pkg, mix):
    import torch
    rng = np.random.default_rng(12)
    C, n = 4096, 777
    x = (0.5 * rng.standard_normal((C, n, 2))).astype(np.float32)
    buses, gains = _membership(C, rng)
    m = pkg.AudioMixer(C, buses, gains=gains)
    whole = m.process(_cuda(x)).cpu().numpy()                                          # odd stride: one frame per lane
    assert bits_equal(whole, _expected(mix, x, buses, gains))
    # padded strides (even: two frames per lane) on both sides
    xp = torch.zeros(C, n + 9, 2, device="cuda")
    xp[:, :n] = _cuda(x)
    xp2 = torch.zeros(C, n + 11, 2, device="cuda")[:, 1:]                           # rows 8-byte aligned only
    xp2[:, :n] = _cuda(x)
    for xin in (xp, xp2):
        out = torch.full((len(buses), n + 5, 2), 9.0, device="cuda")
        got = m.process(xin, n=n, out=out)
        assert bits_equal(got.cpu().numpy(), whole)
        assert bool((out[:, n:] == 9.0).all())
    # n split across calls
    parts = [m.process(_cuda(x[:, a:b])).cpu().numpy() for a, b in ((0, 1), (1, 300), (300, 301), (301, n))]
    assert bits_equal(np.concatenate(parts, 1), whole)
    # set_gain / set_sources apply at the next call and touch nothing else
    m.set_gain(3, 4.0)
    assert m.gain(3) == np.float32(4.0) and m.gain(2) == np.float32(0.7)
    new = [9, 1, 9, 4095]
    m.set_sources(6, new)
    got = m.process(_cuda(x)).cpu().numpy()
    for b in range(len(buses)):
        if b == 3:
            assert bits_equal(got[b], mix(x, buses[3], None, 4.0))
        elif b == 6:
            assert bits_equal(got[b], mix(x, new, None, 1.0))                          # (4096 sources -> 4: staged -> streaming kernel)
        else:
            assert bits_equal(got[b], whole[b]), b
    m.set_gain(-1, 0.5)
    assert all(m.gain(b) == 0.5 for b in range(len(buses)))
    m.set_sources(1, list(range(C)))                                                   # (1 source -> 4096: streaming -> staged)
    got = m.process(_cuda(x)).cpu().numpy()
    assert bits_equal(got[1], mix(x, list(range(C)), None, 0.5))


def test_argument_errors_write_nothing(pkg):
    import torch
    C, n = 6, 64
    x = torch.randn(C, n, 2, device="cuda")
    with pytest.raises(pkg.FmdError):
        pkg.AudioMixer(C, [[0, C]])
    with pytest.raises(pkg.FmdError):
        pkg.AudioMixer(C, [[-1]])
    m = pkg.AudioMixer(C, [[0, 1], [2], []])
    out = torch.full((3, n, 2), 7.0, device="cuda")
    for kw in ({"n": n + 1}, {"n": -1}):
        with pytest.raises(pkg.FmdError) as e:
            m.process(x, out=out, **kw)
        assert e.value.status == -1                                                    # FMD_ERR_ARG
    with pytest.raises(pkg.FmdError):
        m.process(x, out=torch.full((3, n - 1, 2), 7.0, device="cuda"))                # out_stride < n
    for bad in (lambda: m.set_sources(0, [C]), lambda: m.set_sources(3, [0]), lambda: m.set_gain(3, 1.0), lambda: m.gain(-1)):
        with pytest.raises(pkg.FmdError):
            bad()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the failed calls changed nothing: n == 0 writes nothing either, and a valid call works
    m.process(x, n=0, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    y = m.process(x, out=out)
    assert not bool((y[2] != 0).any()) and bool((y[:2] != 7.0).all())


def test_end_to_end_chain_and_cpp_adaptor(pkg, mix, tmp_path):
    """A synthesized capture through BatchDemod, AudioResampler and AudioMixer on one stream equals the restatement applied to the
    resampler's output read back; the C++ adaptor's host UpdateMixer writes the same frames to a WAV file."""
    import torch
    C, bs, nb = 8, 16384, 3
    caps = np.stack([synth.to_cf32(synth.fm_capture(bs * nb, fs=256000.0, seed=60 + c, channel=c + 1)["iq"]) for c in range(C)])
    buses = [list(range(C)), [0], [2, 5, 2], list(range(C)) * 5]
    gains = np.float32([1.0, 2.5, 0.8, 1.2])
    s = torch.cuda.Stream()
    dm = pkg.BatchDemod(C, bs, 256_000, fast_math=True)
    rs = pkg.AudioResampler(C, 48000, max_input_frames=2048)
    mx = pkg.AudioMixer(C, buses, gains=gains)
    active = torch.ones(C, dtype=torch.uint8, device="cuda")
    active[3] = 0
    r48, mixed = [], []
    d_in = [_cuda(caps[:, b * bs:(b + 1) * bs]) for b in range(nb)]                      # alive until the end
    torch.cuda.synchronize()
    for b in range(nb):
        dm.submit(d_in[b])
        assert dm.outputs_block() == b
        dm.wait_outputs(s)
        with torch.cuda.stream(s):
            y = rs.process(dm.audio_tensor(), stream=s)
            z = mx.process(y, active=active, stream=s)
            r48.append(y.clone())
            mixed.append(z.clone())
        dm.release_outputs(s)
    torch.cuda.synchronize()
    dm.close()
    r48 = torch.cat(r48, 1).cpu().numpy()
    mixed = torch.cat(mixed, 1).cpu().numpy()
    want = _expected(mix, r48, buses, gains, active.cpu().numpy())
    assert bits_equal(mixed, want), describe_diff(mixed, want)
    # the C++ adaptor: bus 0 (every station) at 32 kHz into a WAV file, block by block
    exe = tmp_path / "mixer_main"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'include'}", f"-I{ROOT / 'fm-radio_amd' / 'host'}", str(ROOT / "tests" / "cpp" / "mixer_main.cpp"),
                    f"-L{ROOT / 'fm-radio_amd' / 'csrc'}", "-lfmdemod", f"-Wl,-rpath,{ROOT / 'fm-radio_amd' / 'csrc'}", "-o", str(exe)], check=True)
    C2 = 3
    np.ascontiguousarray(caps[:C2]).tofile(tmp_path / "cap.cf32")
    subprocess.run([str(exe), str(tmp_path / "cap.cf32"), str(C2), str(bs), "256000", str(tmp_path / "o.wav")], check=True)
    dm = pkg.BatchDemod(C2, bs, 256_000)
    mx2 = pkg.AudioMixer(C2, [list(range(C2)), [0]], gains=[1.0, 2.5])
    frames = []
    for b in range(nb):
        dm.process(np.ascontiguousarray(caps[:C2, b * bs:(b + 1) * bs]))
        dm.synchronize()
        a = dm.audio_tensor()
        z = mx2.process(a).cpu().numpy()
        assert bits_equal(z[0], mix(a.cpu().numpy(), list(range(C2)), None, 1.0))
        frames.append(z[0])
    dm.close()
    pcm = (np.concatenate(frames) * SCALE).astype(np.int32).astype(np.int16)
    wav = (tmp_path / "o.wav").read_bytes()
    assert wav[:4] == b"RIFF" and wav[8:12] == b"WAVE"
    assert int.from_bytes(wav[24:28], "little") == 32000 and int.from_bytes(wav[22:24], "little") == 2
    assert np.array_equal(np.frombuffer(wav[44:], np.int16).reshape(-1, 2), pcm)
