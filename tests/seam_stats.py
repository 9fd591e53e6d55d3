"""Peak and by-position statistics of the tolerance mode's error against the oracle (pure numpy; no GPU, no library).

An RMS over a block cannot see a defect that sits at ONE position of a tile, a span or a block: one wrong sample per 256-sample tile may
be sqrt(256) times the RMS bar.  The tolerance-mode kernels are tiled, and their special code is at tile, span and block edges, so the
statistics here fold the squared error by position inside those periods.

The error of a stream is kept per station and block, e[S, nb, n] in the stream's own samples (float64):
  fm_out_iq  complex samples                 e2 = |e|^2
  pll_dt     the difference modulo one turn  e2 = e^2
  lpr, lmr   the samples as they are         e2 = e^2
  audio      stereo frames, e[S, nb, n, 2]   e2 = e_L^2 + e_R^2
Statistics (all on e2[S, nb, n], with `keep[S, nb]` selecting the (station, block) pairs that count):
  peak                  sqrt(max e2)
  fold profile          E2[p] = mean of e2 over the samples whose index in the block is p modulo T (phase origin: the block start)
  worst-position ratio  max_p E2[p] / median_p E2[p], only where every position pools at least MIN_POOL samples
  zone ratio            mean_{p in Z} E2[p] / median_p E2[p] for at least MIN_ZONE adjacent positions Z
  detrended ratio       (pll_dt) the worst-position ratio of the error with each period's own mean taken off
  edge zones            (lmr, audio) the block's first 31 outputs over the kept block edges both of whose mixed offsets agree with the oracle's, and
                        over those of them that mix two offsets more than 0.01 apart ("moving"), each over the median position of the block
                        fold; the folds at shorter periods leave those 31 outputs out (geometry)
  clean peak            (lmr, audio) the peak over the pairs with no offset difference in the block or the two in front (kept_pairs)
and an injector that puts a defect into an error array on the host, to prove what the statistics catch.
"""
from __future__ import annotations

import numpy as np

MIN_POOL = 200      # samples every position of a fold must pool before single positions are compared
MIN_ZONE = 16       # adjacent positions a zone must have

STREAMS = ("fm_out_iq", "pll_dt", "lpr", "lmr", "audio")
# today's RMS bars (tests/test_gpu_fast.py): the largest once-per-period defect they pass is A = B sqrt(T)
DETUNED_HZ = 19003.7       # the pilot of the runs that decide the ratios (at 19 000 Hz it makes exactly 19 cycles a span: test_gpu_fast_seams.py)
RMS_BAR = {"audio": 1e-4, "lmr": 1e-4, "lpr": 2e-6, "fm_out_iq": 2e-6, "pll_dt": 5e-5}


def stream_error(stream: str, got, want, n_blocks: int) -> np.ndarray:
    """got, want: [S, ...] whole runs of one stream (blocks concatenated).  Returns e[S, nb, n] (audio: [S, nb, n, 2]; fm_out_iq: complex)."""
    g = np.asarray(got, np.float64)
    w = np.asarray(want, np.float64)
    n_st = g.shape[0]
    g = g.reshape(n_st, -1)
    w = w.reshape(n_st, -1)
    assert g.shape == w.shape, (stream, g.shape, w.shape)
    e = g - w
    if stream == "pll_dt":
        e -= np.round(e)
        return e.reshape(n_st, n_blocks, -1)
    if stream == "fm_out_iq":
        e = e.reshape(n_st, n_blocks, -1, 2)
        return e[..., 0] + 1j * e[..., 1]
    if stream == "audio":
        return e.reshape(n_st, n_blocks, -1, 2)
    return e.reshape(n_st, n_blocks, -1)


def squared(e: np.ndarray) -> np.ndarray:
    """e2[S, nb, n] of an error array of any of the streams."""
    if np.iscomplexobj(e):
        return e.real ** 2 + e.imag ** 2
    if e.ndim == 4:
        return (e ** 2).sum(axis=3)
    return e ** 2


def peak(e2: np.ndarray, keep=None) -> float:
    if keep is not None:
        e2 = e2[keep]
    return float(np.sqrt(e2.max())) if e2.size else 0.0


def fold_profile(e2: np.ndarray, period: int, keep=None, skip_first: int = 0):
    """E2[p], count[p] for p in 0 .. period-1: mean of e2 over the kept samples with (index in the block) % period == p.
    skip_first: the block's first samples that are left out of the fold (a zone that is barred on its own)."""
    n = e2.shape[2]
    assert 1 <= period <= n, (period, n)
    rows = e2[keep] if keep is not None else e2.reshape(-1, n)          # [pairs, n]
    w = np.ones(n)
    w[:skip_first] = 0.0
    col = rows.sum(axis=0) * w
    ccol = rows.shape[0] * w
    full = n // period
    tot = col[:full * period].reshape(full, period).sum(axis=0)
    cnt = ccol[:full * period].reshape(full, period).sum(axis=0)
    rest = n - full * period
    if rest:
        tot[:rest] += col[full * period:]
        cnt[:rest] += ccol[full * period:]
    return tot / np.maximum(cnt, 1), cnt.astype(np.int64)


def detrended(e: np.ndarray, period: int) -> np.ndarray:
    """e with the mean of each period taken off (real streams whose block is a whole number of periods).  The pilot loop's error is a slow drift,
    nearly the same at every position of a span: folded as it is, a defect of its own size at one position can even CANCEL against it; with each
    period's mean removed the drift is gone and a once-per-period defect of amplitude a stays as a (1 - 1 / T)."""
    n = e.shape[2]
    assert e.ndim == 3 and not np.iscomplexobj(e) and n % period == 0, (e.shape, period)
    x = e.reshape(e.shape[0], e.shape[1], n // period, period)
    return (x - x.mean(axis=3, keepdims=True)).reshape(e.shape)


def worst_position_ratio(prof: np.ndarray, cnt: np.ndarray):
    """max_p E2[p] / median_p E2[p] and the position, or (None, None) where a position pools fewer than MIN_POOL samples."""
    if cnt.min() < MIN_POOL:
        return None, None
    med = float(np.median(prof))
    p = int(np.argmax(prof))
    return float(prof[p] / med), p


def zone_ratio(prof: np.ndarray, lo: int, hi: int) -> float:
    """mean of E2 over the positions lo .. hi-1 over the median of all positions."""
    assert hi - lo >= MIN_ZONE and 0 <= lo and hi <= prof.size, (lo, hi, prof.size)
    return float(prof[lo:hi].mean() / np.median(prof))


def inject(e: np.ndarray, period: int, amplitude: float, lo: int, hi: int | None = None) -> np.ndarray:
    """A copy of the error array e with `amplitude` added at the positions lo .. hi-1 (one position when hi is None) of every period,
    the phase origin at the block start: onto the real part of complex samples, onto the left channel of stereo frames."""
    hi = lo + 1 if hi is None else hi
    out = e.copy()
    n = e.shape[2]
    idx = np.arange(n)
    sel = idx[(idx % period >= lo) & (idx % period < hi)]
    if out.ndim == 4:
        out[:, :, sel, 0] += amplitude
    else:
        out[:, :, sel] += amplitude
    return out


# ---- the geometry of one configuration: which periods and zones each stream has ---------------------------------------------------------

def geometry(fs: int, block_size: int, u8: bool = False, deemph: bool = False, split_front: bool = False, n_ch: int = 8) -> dict:
    """Periods and zones per stream of the tolerance mode, from the kernels' geometry constants (fm-radio_amd/csrc) and the tiles the block plan picks
    (fmd_plan.h BlockPlan; restated here on purpose: tests/test_plan_cpu.py holds the two together for the configurations the seam test runs):
      n_fm_out = block / (fs / 256 k) / 2, n_audio = n_fm_out / 4                                            (fmd_kernels.h Dims)
      front tile (BlockPlan::Input::front_tile): 1024 fm_out samples when n_fm_out % 1024 == 0, else 512; captures at 256 kSa/s without de-emphasis:
        2048 when n_fm_out % 2048 == 0, u8 always, cf32 in batches of at least 12288 such tiles (n_ch stations); k_front_pre_mfma: 1024.  63-sample
        halo (FrontGeomM::NW), de-emphasis (deemph: inside the tile) from a zero state kDeemphWarmup = 128 samples early, MFMA outputs in 16-column accumulators
      first decimator on its own (predecim_tile): (8192 u8 | 2048 cf32) / M input samples per tile, else 256 outputs -> in fm_out samples / 2
      pilot loop: kSpan = 128, kSparseDec = 16 (fmd_tables.h)
      extract (extract_tile): 256 audio samples per tile when n_audio % 256 == 0, else 128; four tiles a round; kFoPad = 192 fm_out
        samples = 47 audio samples of reach into the tile in front; the block's first 31 outputs through S_old (kBpEdgeRows = 31 * 8)
    Each entry: periods {kind: T}, zones [(name, kind of the period it is folded at, lo, hi)]."""
    m = fs // 256_000
    n_fo = block_size // m // 2
    n_au = n_fo // 4
    if m > 1 and not deemph and not split_front and n_fo % 1024 == 0:
        ft = 1024                                                   # k_front_pre_mfma (fmd_plan.h front_takes_capture)
    elif m == 1 and not deemph and n_fo % 2048 == 0 and (u8 or n_ch * (n_fo // 2048) >= 12288):
        ft = 2048
    else:
        ft = 1024 if n_fo % 1024 == 0 else 512
    et = 256 if n_au % 256 == 0 else 128
    geo = {"n_fm_out": n_fo, "n_audio": n_au, "front_tile": ft, "extract_tile": et}
    fo_p = {"16": 16, "tile": ft, "block": n_fo}
    if ft > 1024:
        fo_p["1024"] = 1024
    if m > 1 and (split_front or deemph or n_fo % 1024):
        n_in = block_size // m
        tpm = (8192 if u8 else 2048) // m
        fo_p["predecim"] = (tpm if n_in % tpm == 0 else 256) // 2
    fo_z = [("tile_first64", "tile", 0, 64), ("tile_last64", "tile", ft - 64, ft), ("block_first192", "block", 0, 192), ("block_last64", "block", n_fo - 64, n_fo)]
    if deemph:
        fo_z.append(("tile_first128", "tile", 0, 128))
    geo["fm_out_iq"] = {"periods": fo_p, "zones": fo_z}
    geo["pll_dt"] = {"periods": {"16": 16, "span": 128, "block": n_fo}, "detrend": True,
                     "zones": [("span_first16", "span", 0, 16), ("span_last16", "span", 112, 128), ("block_first_span", "block", 0, 128)]}
    au_p = {"16": 16, "tile": et, "block": n_au}
    if 4 * et <= n_au:
        au_p["4tiles"] = 4 * et
    au_z = [("block_first31", "block", 0, 31), ("tile_first47", "tile", 0, 47), ("block_last_tile", "block", n_au - et, n_au)]
    # the block's first 31 outputs take a path of their own (S_old) and have zones and bars of their own: the folds at the periods shorter than
    # the block leave them out, so that the other positions keep a tight ratio; on L-R and audio the zone is also taken over the block edges
    # that really mix two different offsets ("moving": kept_pairs)
    for k in ("lpr", "lmr", "audio"):
        geo[k] = {"periods": dict(au_p), "zones": list(au_z), "skip_first": 31}
    # (L-R, audio: those 31 outputs mix the offsets the TWO blocks in front left, so their zone is taken over the kept pairs whose older
    #  offset agrees with the oracle's as well — kept_pairs' `edge` — once over all of them and once over the moving ones)
    for k in ("lmr", "audio"):
        geo[k]["zones"] = [z for z in au_z if z[0] != "block_first31"]
        geo[k]["edge_zones"] = [("block_first31", 0, 31, False), ("block_first31_moving", 0, 31, True)]
    return geo


def figures(e: np.ndarray, spec: dict, keep=None, kinds=None, moving=None, clean=None, edge=None) -> dict:
    """Every statistic of one stream: {"rms", "peak", "ratio": {kind: value or None}, "ratio_at": {kind: p}, "zone": {name: ratio}, "zone_ms": {name: mean square}}.
    kinds: only these periods (and their zones).  edge[S, nb], moving[S, nb]: the (station, block) pairs of spec["edge_zones"] (kept_pairs);
    clean[S, nb]: the pairs "peak_clean" is taken over."""
    e2 = squared(e)
    rows = e2[keep] if keep is not None else e2
    out = {"rms": float(np.sqrt(rows.mean())), "peak": peak(e2, keep), "ratio": {}, "ratio_at": {}, "zone": {}, "zone_ms": {}}
    if clean is not None:
        out["peak_clean"] = peak(e2, clean)
        out["clean_pairs"] = int(clean.sum())
    profs = {}
    for kind, t in spec["periods"].items():
        if kinds is not None and kind not in kinds:
            continue
        skip = spec.get("skip_first", 0) if t < e2.shape[2] else 0
        prof, cnt = fold_profile(e2, t, keep, skip)
        profs[kind] = prof
        if t < e2.shape[2]:
            out["ratio"][kind], out["ratio_at"][kind] = worst_position_ratio(prof, cnt)
            if spec.get("detrend"):
                d2 = squared(detrended(e, t))
                out["ratio"][kind + "_detrended"], out["ratio_at"][kind + "_detrended"] = worst_position_ratio(*fold_profile(d2, t, keep))
    for name, kind, lo, hi in spec["zones"]:
        if kind in profs:
            out["zone"][name] = zone_ratio(profs[kind], lo, hi)
            out["zone_ms"][name] = float(profs[kind][lo:hi].mean())
    if "block" in profs and spec.get("edge_zones"):
        ek = np.ones(e2.shape[:2], bool) if edge is None else edge
        mv = ek if moving is None else ek & moving
        out["edge_pairs"], out["moving_edge_pairs"] = int(ek.sum()), int(mv.sum())
        for name, lo, hi, only_moving in spec["edge_zones"]:
            sel = mv if only_moving else ek
            ms = float(e2[sel][:, lo:hi].mean()) if sel.any() else float("inf")
            out["zone"][name] = ms / float(np.median(profs["block"]))
            out["zone_ms"][name] = ms
    return out


def violations(stream: str, fig: dict, bars: dict) -> list:
    """What of one stream's figures exceeds its bars {"peak": x, "peak_clean": x, "ratio": {kind: x}, "zone": {name: x}, "zone_ms": {name: x}};
    a figure without a bar is a violation too.  A zone named in "zone_ms" is held to that absolute mean square INSTEAD of its ratio (structure
    that is intended, above a floor that differs between configurations)."""
    bad = []
    for pk in ("peak", "peak_clean"):
        if pk in fig and not fig[pk] <= bars.get(pk, 0.0):
            bad.append((stream, pk, fig[pk], bars.get(pk)))
    for kind, v in fig["ratio"].items():
        if v is not None and not v <= bars["ratio"].get(kind, 0.0):
            bad.append((stream, "ratio:" + kind, v, bars["ratio"].get(kind)))
    absolute = bars.get("zone_ms", {})
    for name, v in fig["zone"].items():
        if name in absolute:
            if not fig["zone_ms"][name] <= absolute[name]:
                bad.append((stream, "zone_ms:" + name, fig["zone_ms"][name], absolute[name]))
        elif not v <= bars["zone"].get(name, 0.0):
            bad.append((stream, "zone:" + name, v, bars["zone"].get(name)))
    return bad


def sensitivity(errs: dict, geo: dict, keep, bars: dict, moving=None, edge=None):
    """The defects today's RMS bars pass, injected on the host into an error (the GPU's own, or a surrogate): which of them the bars catch.
    A / 4 ... A / 64 (A = B sqrt(T)) at position 0, T / 2 and T - 1 of every period T shorter than the block whose positions pool MIN_POOL samples;
    B sqrt(block / |Z|) / 4 over the block's first 31 outputs (lpr, lmr, audio) and first span (pll_dt).
    Returns (misses at the required amplitude, {stream: {kind: smallest caught multiple of A}}, {stream: {zone: caught}})."""
    misses, smallest, zones = [], {}, {}
    for k in STREAMS:
        e, spec = errs[k], geo[k]
        kp = keep if k in ("lmr", "audio") else None
        mv = moving if k in ("lmr", "audio") else None
        ed = edge if k in ("lmr", "audio") else None
        n = squared(e[:1, :1]).shape[2]
        smallest[k] = {}
        for kind, t in spec["periods"].items():
            if t >= n:
                continue
            if figures(e, spec, kp, kinds=[kind])["ratio"][kind] is None:        # fewer than MIN_POOL samples a position: zones only
                continue
            a_full = RMS_BAR[k] * np.sqrt(t)
            caught_down_to = None
            for mult in (1 / 4, 1 / 8, 1 / 16, 1 / 32, 1 / 64):
                ok = all(violations(k, figures(inject(e, t, a_full * mult, pos), spec, kp, kinds=[kind]), bars[k]) for pos in (0, t // 2, t - 1))
                if not ok:
                    break
                caught_down_to = mult
            smallest[k][kind] = caught_down_to
            if caught_down_to is None:
                misses.append((k, kind, t, "A/4 = %.3g" % (a_full / 4)))
        zone = {"pll_dt": ("block_first_span", 0, 128)}.get(k, ("block_first31", 0, 31)) if k != "fm_out_iq" else None
        if zone is not None:
            name, lo, hi = zone
            a = RMS_BAR[k] * np.sqrt(n / (hi - lo)) / 4
            hit = bool(violations(k, figures(inject(e, n, a, lo, hi), spec, kp, kinds=["block"], moving=mv, edge=ed), bars[k]))
            zones[k] = {name: hit}
            if not hit:
                misses.append((k, "zone:" + name, n, "%.3g" % a))
    return misses, smallest, zones


def kept_pairs(off_gpu: np.ndarray, off_oracle: np.ndarray, limit: float = 1e-4 / 0.7):
    """keep[S, nb] for L-R and audio: a (station, block) pair is dropped only where the PREVIOUS block's L-R offset (the one this block is mixed
    with) differs from the oracle's by more than `limit` (the one documented discontinuity, test_gpu_fast.lmr_audio_excess);
    and moving[S, nb]: the oracle's own offset changed by more than 0.01 between the two blocks in front — the old and the new offset the
    block-edge path (S_old) mixes; and clean[S, nb]: neither the block's own offset nor those of the two blocks in front differ by more than
    `limit` (a flipped estimate shows in the block itself and in the two behind it); and edge[S, nb]: kept, and the offset
    of the block before the previous one agrees as well — both offsets the block's first 31 outputs mix are the oracle's."""
    d = np.abs(np.asarray(off_gpu, np.float64) - np.asarray(off_oracle, np.float64))
    prev = np.concatenate([np.zeros((d.shape[0], 1)), d[:, :-1]], axis=1)
    o = np.concatenate([np.zeros((d.shape[0], 2)), np.asarray(off_oracle, np.float64)], axis=1)      # o[:, b + 1]: the offset block b is mixed with
    moving = np.abs(o[:, 1:-1] - o[:, :-2]) > 0.01
    prev2 = np.concatenate([np.zeros((d.shape[0], 2)), d[:, :-2]], axis=1)
    return prev <= limit, moving, (prev <= limit) & (prev2 <= limit) & (d <= limit), (prev <= limit) & (prev2 <= limit)
