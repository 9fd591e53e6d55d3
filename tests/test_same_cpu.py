"""EAS SAME decoder, the parts that need no GPU: the ABI is declared and exported and the record's layout agrees everywhere; the library's
host unit against the C restatement (tests/cpp/same_ref.c) bit for bit; known answers through the restatement; the restatement against a
float64 numpy model; its split invariance and a frame count past 2^32; the parser and the vote; parameter validation; and the host unit
with the restatement under sanitizers, as a stand-alone program."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import same_ref
from same_ref import EOM, HEADER24, HEADER56, bits

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "fm-radio_amd" / "csrc"
SYMBOLS = ["fmd_same_default_params", "fmd_same_encode", "fmd_same_parse", "fmd_same_vote", "fmd_same_create", "fmd_same_destroy", "fmd_same_reset",
           "fmd_same_set_params", "fmd_same_get_params", "fmd_same_process_f32_dev", "fmd_same_get_status", "fmd_same_status_dev", "fmd_same_last_error"]
RATES = (8000, 32000, 44100, 48000)
MAIN_TEXT = b"ZCZC-CIV-EVI-006037-006059+0100-2931415-KABC/FM -"


@pytest.fixture(scope="module")
def pkg():
    import fmradio_loader
    p = fmradio_loader.load()
    p.build_library()
    return p


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return same_ref.build(tmp_path_factory.mktemp("same_ref"))


def _texts(ch):
    return [m[2] for m in ch.messages()]


def test_symbols_are_declared_and_exported(pkg):
    declared = pkg.declared_symbols(debug=False)
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/fmdemod.h"
        assert hasattr(lib, s), f"{s} is not exported"
    assert lib.fmd_api_version() == 3
    for name in ("SameDecoder", "SAME_STATUS_DTYPE", "same_encode", "same_parse", "same_vote", "same_default_params", "SameParams"):
        assert hasattr(pkg, name)
    assert pkg.SAME_STATUS_DTYPE == same_ref.STATUS_DTYPE and pkg.SAME_STATUS_DTYPE.itemsize == 2856
    assert pkg.SAME_MESSAGE_DTYPE == same_ref.MESSAGE_DTYPE and pkg.SAME_MESSAGE_DTYPE.itemsize == 280
    assert C.sizeof(pkg.SameParams) == C.sizeof(same_ref.Params) == 16 and C.sizeof(pkg.SameEncodeConfig) == C.sizeof(same_ref.EncodeConfig) == 40
    # the header's own words on the layout
    text = (ROOT / "include" / "fmdemod.h").read_text()
    line = text[text.index("one per station, 2856 bytes"):text.index("typedef struct {\n    unsigned long long frames;            /* frames seen since reset */")]
    for name, at in same_ref.OFFSETS.items():
        assert (f"{name} at byte {at}" if name == "frames" else f"{name} {at}") in line, name


def test_library_host_unit_equals_the_restatement(pkg, ref, tmp_path):
    """tests/cpp/same_design_main.cpp linked against libfmdemod.so itself, so that the table, the tick starts and the encoder's audio are those
    of the library as it is built (its compiler and flags): bit for bit the restatement's at 8, 32, 44.1 and 48 kHz"""
    exe = tmp_path / "same_design_lib"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "same_design_main.cpp"),
                    f"-L{CSRC}", "-lfmdemod", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(tmp_path)] + [str(f) for f in RATES], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok"
    for fs, line in zip(RATES, lines):
        geo = ref.geometry(fs)
        assert tuple(int(v) for v in line.split()) == (fs,) + geo
        g = np.gcd(3125, 6 * fs)
        assert geo == (6 * fs // g, (4 * 3125 // g) % (6 * fs // g), (3 * 3125 // g) % (6 * fs // g)) and geo[0] <= 57600
        # the two steps are the two tones: step / P of fs
        assert abs(geo[1] / geo[0] * fs - 6250.0 / 3.0) < 1e-9 and abs(geo[2] / geo[0] * fs - 1562.5) < 1e-9
        tab = np.fromfile(tmp_path / f"same_table_{fs}.f64", np.float64).reshape(-1, 2)
        assert tab.shape == (geo[0], 2) and np.array_equal(bits(tab), bits(ref.table(fs))), fs
        a = 2.0 * np.pi * np.arange(geo[0]) / geo[0]
        assert np.abs(tab - np.stack([np.cos(a), np.sin(a)], axis=1)).max() <= 2.0 ** -52
        ticks = np.fromfile(tmp_path / f"same_ticks_{fs}.u32", np.uint32).astype(np.int64)
        assert np.array_equal(ticks, ref.tick_starts(fs)) and ticks[0] == 0 and ticks[-1] == 3 * fs
        assert np.array_equal(ticks, -((-3 * fs * np.arange(12501, dtype=np.int64)) // 12500))     # ceil(k 3 fs / 12500)
        d = np.diff(ticks)
        assert d.min() == (3 * fs) // 12500 and d.max() == -((-3 * fs) // 12500)                   # 1 or 2 at 8 kHz, 7 or 8 at 32 kHz
        audio = np.fromfile(tmp_path / f"same_audio_{fs}.f32", np.float32).reshape(-1, 2)
        want = ref.encode(MAIN_TEXT, fs, 1.01, 0.3, 2, fs // 8, -3.0)
        assert audio.shape == want.shape and np.array_equal(bits(audio), bits(want)), fs
        assert np.array_equal(bits(pkg.same_encode(MAIN_TEXT, fs, 1.01, 0.3, 2, fs // 8, -3.0)), bits(want))
    d = pkg.same_default_params()
    assert same_ref.params_tuple(d) == same_ref.params_tuple(ref.default_params()) == (16, 750000, 0, 0)
    assert bytes.fromhex(lines[len(RATES)]) == bytes(d) and 750000 == 180 * 12500 // 3
    # the encoder's argument checks are the restatement's
    for kw in (dict(fs=7990), dict(clock_ratio=0.89), dict(clock_ratio=1.11), dict(amplitude=-1.0), dict(amplitude=float("inf")), dict(mark_db=41.0),
               dict(repeats=0), dict(repeats=17), dict(text=b""), dict(text=b"Z" * 269)):
        a = dict(text=HEADER24, fs=8000, clock_ratio=1.0, amplitude=0.25, repeats=1, gap_frames=0, mark_db=0.0)
        a.update(kw)
        assert ref.encode(**a) is None, kw
        with pytest.raises(pkg.FmdError) as e:
            pkg.same_encode(**a)
        assert e.value.status == -1, kw
    assert pkg.same_encode(b"Z" * 268, 8000, repeats=1, gap_frames=0).shape == ref.encode(b"Z" * 268, 8000, repeats=1, gap_frames=0).shape


@pytest.mark.parametrize("fs", [8000, 32000, 48000])
def test_known_answers(ref, fs):
    """a 56-character header and NNNN, three bursts each, decode to the exact bytes at clock ratios 0.98, 1 and 1.02 and with the mark tone
    6 dB below and above the space tone (each at every ratio), and at amplitudes from 1e-4 to 4; the alert opens and closes"""
    for ratio in (0.98, 1.0, 1.02):
        for mark_db, amp in ((0.0, 0.25), (-6.0, 0.25), (6.0, 0.25), (0.0, 1e-4), (0.0, 4.0)):
            head = ref.encode(HEADER56, fs, ratio, amp, 3, fs // 2, mark_db)
            ch = ref.run(fs, head)
            assert _texts(ch) == [HEADER56] * 3 and ch.flags == same_ref.ALERT_OPEN, (ratio, mark_db, amp, _texts(ch))
            ch.process(ref.encode(EOM, fs, ratio, amp, 3, fs // 2, mark_db))
            st = ch.status()[0]
            assert _texts(ch) == [HEADER56] * 3 + [EOM] * 3 and ch.flags == 0 and ch.ok == 1, (ratio, mark_db, amp, _texts(ch))
            assert [m[1] for m in ch.messages()] == [1, 1, 1, 2, 2, 2] and int(st["syncs"]) == 6 and int(st["rejected"]) == 0
            ticks = [m[0] for m in ch.messages()]
            assert ticks == sorted(ticks) and int(st["last_accept_tick"]) > ticks[-1]


def test_noise_and_tones(pkg, ref):
    """a header under white noise 10 dB below the burst's power decodes once the vote is taken (32 kHz, fixed seeds, also with the sender's
    clock 2 % off); 60 s of noise and 60 s of a steady 2083.3 Hz tone and of 1000 + 1700 Hz accept nothing"""
    fs = 32000
    repaired = 0
    for seed, ratio in ((1, 1.0), (2, 0.98), (3, 1.02), (4, 1.0)):
        x = same_ref.add_noise(ref.encode(HEADER56, fs, ratio, 0.25, 3, fs // 2), 0.25, 10.0, seed)
        ms = ref.run(fs, x).messages()
        assert len(ms) == 3, (seed, ms)
        voted, fixed, unresolved = pkg.same_vote(ms)
        # (the noise behind a burst may append a byte or two before one ends the message: what stands behind the last '-' is no part of it)
        assert voted[2][:56] == HEADER56 and pkg.same_parse(voted[2])["valid"] == 63, (seed, ms)
        repaired += fixed + unresolved + sum(m[2] != HEADER56 for m in ms)
    print("bytes outvoted or appended over the four noisy transmissions:", repaired)
    fs = 8000
    rng = np.random.default_rng(20261020)
    w = (0.1 * rng.standard_normal(60 * fs)).astype(np.float32)
    t = np.arange(60 * fs, dtype=np.float64) / fs
    counts = {}
    for name, s in (("noise", w), ("2083.3 Hz", (0.25 * np.sin(2 * np.pi * 6250.0 / 3.0 * t)).astype(np.float32)),
                    ("1000 + 1700 Hz", (0.2 * np.sin(2 * np.pi * 1000.0 * t) + 0.2 * np.sin(2 * np.pi * 1700.0 * t)).astype(np.float32))):
        st = ref.run(fs, np.stack([s, s], axis=1)).status()[0]
        counts[name] = (int(st["syncs"]), int(st["rejected"]), int(st["accepted"]))
        assert int(st["accepted"]) == 0 and int(st["flags"]) & same_ref.ALERT_OPEN == 0, name
    print("(syncs, rejected, accepted) over 60 s each:", counts)


def test_restatement_against_the_float64_model(ref):
    """The model correlates against numpy's own cos and sin of the exact phase, sums each tick with np.add.reduceat (no fma) and adds the
    window's eight ticks as whole arrays: other roundings throughout.  On clean bursts -- at the nominal clock and
    2 % off, mark level with space and 6 dB off -- it takes the same bits and ends the same messages at the same ticks; the smallest
    |E1 - E0| / (E1 + E0) at a bit instant while synchronised says how far from marginal they were (a rounding moves it by about 1e-15).  Off the bit instants the smallest figure at any tick is checked to be above 1e-9."""
    worst = {}
    for fs, ratio, mark_db, text in ((8000, 1.0, 0.0, HEADER24), (8000, 1.02, 6.0, HEADER24), (32000, 0.98, -6.0, HEADER24), (48000, 1.0, 0.0, EOM)):
        x = ref.encode(text, fs, ratio, 0.25, 3, fs // 2, mark_db)
        x = x[:x.shape[0] - fs // 4]                             # (not a whole number of ticks)
        # a noise floor 60 dB down: in exact silence every decision is 0 > 0, and a burst's first frame alone in the window has E1 = E0
        # exactly (cos^2 + sin^2 on both sides) -- marginal decisions by construction, after which two roundings may part for a byte
        x = same_ref.add_noise(x, 0.25, 60.0, fs)
        md = same_ref.model_decode(fs, x)
        ch = ref.run(fs, x)
        st = ch.status()[0]
        assert md["ticks"] == int(st["ticks"])
        assert [(t, b) for t, ok, b in md["messages"] if ok] == [(m[0], m[2]) for m in ch.messages()]
        assert all(m[2].startswith(text) for m in ch.messages())    # (the floor behind a burst may add a byte before one ends the message)
        assert len(md["messages"]) == int(st["accepted"]) + int(st["rejected"]) and int(st["accepted"]) == 3
        # the restatement fed tick by tick decides as the model does at every tick, takes the same bits, and those from synchronisation on at
        # the same ticks
        ch2 = ref.channel(fs)
        got, nbits, marginal = [], 0, 0
        for k in range(md["ticks"]):
            a, b = (3 * fs * k + 12499) // 12500, (3 * fs * (k + 1) + 12499) // 12500
            was_synced = int(ch2.c.st.synced)
            ch2.process(x[a:b])
            if ch2.c.st.bits != nbits:
                nbits = ch2.c.st.bits
                if was_synced:
                    got.append((k, int(ch2.c.st.prev_s)))
            if md["rel"][k] > 1e-9:
                assert int(ch2.c.st.prev_s) == int(md["decisions"][k]), k
            else:
                marginal += 1
        assert got == md["locked_bits"] and len(got) >= 3 * 8 * len(text) and len(md["bits"]) == int(st["bits"]) and marginal == 0
        ch2.process(x[(3 * fs * md["ticks"] + 12499) // 12500:])    # the open tick's frames
        assert np.array_equal(bits(ch2.status()), bits(ch.status()))
        worst[(fs, ratio, mark_db)] = md["margin"]
        assert md["margin"] > 1e-6
    print("smallest |E1 - E0| / (E1 + E0) at a bit instant while synchronised:", worst)


def test_restatement_split_invariance_and_counts_past_2_32(ref):
    """pieces of 1, 7 and 8 frames, a tick, a tick +- 1 and a bit at 32 kHz, and pieces of 1 and 2 frames at 8 kHz: the record's every byte;
    then a station whose counters start past 2^32 (at a multiple of the tick grid's period: 12500 ticks are 3 fs frames)"""
    for fs, steps in ((32000, (1, 7, 8, 9, 61, 62, 0, 1000)), (8000, (1, 2, 3, 15, 16, 0, 500))):
        x = np.concatenate([ref.encode(HEADER24, fs, 1.01, 0.3, 2, 777), ref.encode(EOM, fs, 0.99, 0.2, 1, fs // 16)])
        whole = ref.run(fs, x)
        assert _texts(whole) == [HEADER24, HEADER24, EOM]
        ch = ref.channel(fs)
        a, k = 0, 0
        while a < x.shape[0]:
            b = min(a + steps[k % len(steps)], x.shape[0])
            ch.process(x[a:b])
            a, k = b, k + 1
        assert np.array_equal(bits(ch.status()), bits(whole.status())), fs
        Q = (1 << 33) // (3 * fs) + 5
        far = ref.channel(fs)
        far.c.st.frames, far.c.st.ticks = Q * 3 * fs, Q * 12500
        far.process(x[:4321]).process(x[4321:])
        fst, wst = far.status()[0], whole.status()[0]
        assert int(fst["frames"]) == Q * 3 * fs + x.shape[0] > 1 << 32 and int(fst["ticks"]) == Q * 12500 + int(wst["ticks"])
        for f in same_ref.STATUS_DTYPE.names:
            if f not in ("frames", "ticks", "sync_tick", "last_accept_tick", "ring"):
                assert np.array_equal(bits(fst[f]), bits(wst[f])), f
        assert [(t - Q * 12500, k, b) for t, k, b in far.messages()] == whole.messages()
        assert int(fst["last_accept_tick"]) - Q * 12500 == int(wst["last_accept_tick"])


def test_framer_edges(ref):
    """a 268-byte message is accepted whole and the 269th byte starts nothing; a message cut off by silence is accepted with what it has; one
    that starts with neither ZCZC nor NNNN is rejected; the ring keeps the newest eight; a short hold closes the alert"""
    fs = 8000
    long = b"ZCZC-" + bytes(0x30 + i % 10 for i in range(263))
    ch = ref.run(fs, ref.encode(long, fs, 1.0, 0.25, 1, 2000))
    assert len(long) == 268 and _texts(ch) == [long] and int(ch.status()[0]["rejected"]) == 0
    x = ref.encode(HEADER24, fs, 1.0, 0.25, 1, 0)
    cut = x[:x.shape[0] - 6 * 8 * 16]                            # six bytes short (a byte is 8 bits of 15.36 frames)
    ch = ref.run(fs, np.concatenate([cut, np.zeros((2000, 2), np.float32)]))
    assert len(_texts(ch)) == 1 and HEADER24[:18] == _texts(ch)[0][:18] and len(_texts(ch)[0]) < len(HEADER24)
    ch = ref.run(fs, ref.encode(b"HELLO-WORLD", fs, 1.0, 0.25, 2, 1000))
    st = ch.status()[0]
    assert (int(st["accepted"]), int(st["rejected"]), int(st["syncs"])) == (0, 2, 2) and ch.flags == 0
    many = np.concatenate([ref.encode(b"ZCZC-MSG-%03d-" % i, fs, 1.0, 0.25, 1, 500) for i in range(11)])
    ch = ref.run(fs, many)
    assert int(ch.status()[0]["accepted"]) == 11 and _texts(ch) == [b"ZCZC-MSG-%03d-" % i for i in range(3, 11)]
    assert ch.messages(9) == ch.messages()[-2:]
    hold = ref.channel(fs, hold_ticks=3000, alarm_mask=2)
    hold.process(ref.encode(HEADER24, fs, 1.0, 0.25, 1, 600))
    assert hold.flags == 2 and hold.ok == 0
    hold.process(np.zeros((fs, 2), np.float32))                  # 4167 ticks of silence
    assert hold.flags == 0 and hold.ok == 1 and int(hold.status()[0]["accepted"]) == 1


def test_parser_and_vote(pkg):
    p = pkg.same_parse(HEADER56)
    assert p == {"kind": 1, "valid": 63, "org": "WXR", "event": "TOR", "locations": ["039173", "039051", "039035"], "duration_min": 30, "day": 105,
                 "hour": 17, "minute": 0, "callsign": "KCLE/NWS"}
    assert pkg.same_parse(EOM) == {"kind": 2, "valid": 0, "org": "", "event": "", "locations": [], "duration_min": 0, "day": 0, "hour": 0, "minute": 0,
                                   "callsign": ""}
    assert pkg.same_parse(HEADER56 + b"\x22garbage-+-")== p     # what stands behind the last '-' is ignored
    locs = ["%06d" % (1000 + i) for i in range(31)]
    big = ("ZCZC-EAS-RMT-" + "-".join(locs) + "+0145-3662359-WXYZ-FM-").encode()
    q = pkg.same_parse(big)
    assert q["valid"] == 63 and q["callsign"] == "WXYZ" and q["locations"] == locs and q["duration_min"] == 105 and (q["day"], q["hour"], q["minute"]) == (366, 23, 59)
    assert pkg.same_parse(("ZCZC-EAS-RMT-" + "-".join(locs) + "+0145-3662359-WXYZ/FM-").encode())["valid"] == 63
    one = pkg.same_parse(b"ZCZC-PEP-EAN-000000+0015-0010000-WHITEHSE-")
    assert one["valid"] == 63 and one["locations"] == ["000000"] and one["callsign"] == "WHITEHSE"
    V = {"org": 1, "event": 2, "locations": 4, "duration": 8, "time": 16, "callsign": 32}
    for text, lost in ((b"ZCZC-wXR-TOR-039173+0030-1051700-KCLE/NWS-", "org"), (b"ZCZC-WXRR-TOR-039173+0030-1051700-KCLE/NWS-", "org"),
                       (b"ZCZC-WXR-T0R-039173+0030-1051700-KCLE/NWS-", "event"), (b"ZCZC-WXR-TOR-03917+0030-1051700-KCLE/NWS-", "locations"),
                       (b"ZCZC-WXR-TOR-039173-03905X+0030-1051700-KCLE/NWS-", "locations"),
                       (("ZCZC-WXR-TOR-" + "-".join(locs + ["000001"]) + "+0030-1051700-KCLE/NWS-").encode(), "locations"),
                       (b"ZCZC-WXR-TOR-039173+0075-1051700-KCLE/NWS-", "duration"), (b"ZCZC-WXR-TOR-039173+030-1051700-KCLE/NWS-", "duration"),
                       (b"ZCZC-WXR-TOR-039173+0030-0001700-KCLE/NWS-", "time"), (b"ZCZC-WXR-TOR-039173+0030-3671700-KCLE/NWS-", "time"),
                       (b"ZCZC-WXR-TOR-039173+0030-1052400-KCLE/NWS-", "time"), (b"ZCZC-WXR-TOR-039173+0030-1051760-KCLE/NWS-", "time"),
                       (b"ZCZC-WXR-TOR-039173+0030-105170-KCLE/NWS-", "time"), (b"ZCZC-WXR-TOR-039173+0030-1051700-KCLE/NWSX-", "callsign"),
                       (b"ZCZC-WXR-TOR-039173+0030-1051700--", "callsign"), (b"ZCZC-WXR-TOR-039173+0030-1051700-KCLE/NWS", "callsign")):
        got = pkg.same_parse(text)
        assert got["valid"] == 63 - V[lost], (text, got)
        assert {"org": got["org"] == "", "event": got["event"] == "", "locations": got["locations"] == [], "duration": got["duration_min"] == 0,
                "time": got["day"] == 0, "callsign": got["callsign"] == ""}[lost], (text, got)
    assert pkg.same_parse(b"ZCZC-WXR-TOR-039173")["valid"] == 3 and pkg.same_parse(b"ZCZC")["valid"] == 0
    for bad in (b"ZCZ", b"HELLO", b"", b"Z" * 269):
        with pytest.raises(pkg.FmdError) as e:
            pkg.same_parse(bad)
        assert e.value.status == -1
    # the vote
    gap = 9000                                                   # 2.16 s of ticks: a 56-character burst and its second of silence
    good = [(100 + i * gap, 1, HEADER56) for i in range(3)]
    assert pkg.same_vote(good) == ((100, 1, HEADER56), 0, 0) and pkg.same_vote(good[:1]) == ((100, 1, HEADER56), 0, 0)
    hit = bytearray(HEADER56)
    hit[7], hit[30] = ord("X"), ord("?")
    for k in range(3):
        ms = [(t, kind, bytes(hit) if i == k else b) for i, (t, kind, b) in enumerate(good)]
        assert pkg.same_vote(ms) == ((100, 1, HEADER56), 2, 0), k
    ms = [good[0], (good[1][0], 1, HEADER56[:-3]), (good[2][0], 1, HEADER56 + b"!")]
    assert pkg.same_vote(ms)[0][2] == HEADER56
    # three different copies at one byte: no majority, the first copy's stands and is counted
    a, b = bytearray(HEADER56), bytearray(HEADER56)
    a[12], b[12] = ord("1"), ord("2")
    assert pkg.same_vote([good[0], (good[1][0], 1, bytes(a)), (good[2][0], 1, bytes(b))]) == ((100, 1, HEADER56), 0, 1)
    assert pkg.same_vote([good[0], (good[1][0], 1, bytes(a))]) == ((100, 1, HEADER56), 0, 1)
    for ms, status in (([good[0], (good[0][0] + 10417 + 64 * 56, 1, HEADER56)], -6), ([good[1], good[0]], -1), ([good[0], (good[1][0], 2, EOM)], -1),
                       ([], -1), (good + good[:1], -1)):
        with pytest.raises(pkg.FmdError) as e:
            pkg.same_vote(ms)
        assert e.value.status == status, ms
    assert pkg.same_vote([good[0], (good[0][0] + 10416 + 64 * 56, 1, HEADER56)])[1:] == (0, 0)


def test_parameter_validation(ref):
    """the restatement's checks, which the library's fmd_same_set_params shares (tests/test_gpu_same.py and the sanitizer program run the
    library's): each bound on both sides, and a rejected set changes nothing"""
    ch = ref.channel(8000)
    before = bytes(ch.c.prm)
    for bad in (dict(pull=-1), dict(pull=129), dict(hold_ticks=0), dict(hold_ticks=1 << 31), dict(alarm_mask=4), dict(alarm_mask=0x80000000), dict(reserved=1)):
        assert ch.set_params(**bad) == -1, bad
        assert bytes(ch.c.prm) == before
    for ok in (dict(pull=0), dict(pull=128), dict(hold_ticks=1), dict(hold_ticks=(1 << 31) - 1), dict(alarm_mask=3), dict(alarm_mask=0)):
        assert ch.set_params(**ok) == 0, ok
    for fs in (7990, 48010, 8005, 44101, 0, -8000, 96000):
        with pytest.raises(ValueError):
            ref.channel(fs)
        assert ref.geometry(fs) is None
    with pytest.raises(TypeError):
        ch.set_params(threshold=1)


def test_host_unit_and_restatement_under_sanitizers(ref, tmp_path):
    """fmd_same_design.cpp, tests/cpp/same_ref.c and tests/cpp/same_design_main.cpp as one stand-alone program built with
    -fsanitize=address,undefined and run directly: clean; the restatement inside it decodes the library unit's audio in pieces of 1 ... 97
    frames; what the parser and the vote print is what they must"""
    exe = tmp_path / "same_design_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DSAME_WITH_REF", f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-I{ROOT / 'tests' / 'cpp'}",
                    str(CSRC / "fmd_same_design.cpp"), str(ROOT / "tests" / "cpp" / "same_design_main.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(tmp_path), "8000", "44100"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok"
    text = MAIN_TEXT.decode()
    assert lines[1] == lines[3] == f"decoded 2 0 {text}| {text}|"
    for fs in (8000, 44100):
        audio = np.fromfile(tmp_path / f"same_audio_{fs}.f32", np.float32).reshape(-1, 2)
        assert np.array_equal(bits(audio), bits(ref.encode(MAIN_TEXT, fs, 1.01, 0.3, 2, fs // 8, -3.0)))
    parsed = [ln for ln in lines if ln.startswith("parse ")]
    assert parsed[0].rstrip() == "parse 0 1 63 CIV EVI 2 006037 006059 60 293 14 15 KABC/FM"        # (the call sign ends in a blank)
    assert parsed[1] == "parse 0 2 0 - - 0 0 0 0 0 -"
    assert parsed[2] == "parse 0 1 63 WXR TOR 1 039173 30 105 17 0 KCLE/NWS" and parsed[3] == "parse 0 1 31 WXR TOR 1 039173 30 105 17 0 -"
    assert parsed[4] == "parse 0 1 59 WXR TOR 0 30 105 17 0 KCLE/NWS" and parsed[5] == "parse 0 1 4 - - 1 039173 0 0 0 0 -"
    assert parsed[6] == "parse 0 1 3 WXR TOR 0 0 0 0 0 -" and parsed[7] == parsed[8] == parsed[9] == "parse 0 1 0 - - 0 0 0 0 0 -"
    assert parsed[10] == "parse 0 1 59 EAS RMT 0 15 1 0 0 WXYZ" and parsed[11].startswith("parse 0 1 0 - - 0")
    votes = [ln for ln in lines if ln.startswith("vote ")]
    assert votes[0] == f"vote 0 3 0 {text}" and votes[1] == f"vote 0 2 1 {text[:9]}Y{text[10:]}" and votes[2].startswith("vote 0 0 1 ")
    assert votes[3] == "vote -6" and votes[4] == "vote -1"
