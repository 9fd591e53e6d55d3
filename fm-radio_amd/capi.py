"""ctypes binding of libfmdemod.so (include/fmdemod.h) + a small batched-demodulator wrapper.

`BatchDemod` mirrors the reference's `Broadcast_FM_Demod` usage (construct with a block size, call
`process`, read audio / RDS symbols; reference src/fm_demod/broadcast_fm_demod.h:229-298) for C
channels at once.  It only moves pointers: inputs may be torch CUDA tensors (zero-copy, device entry
points) or numpy arrays (host entry points).
"""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path
from typing import NamedTuple

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
ROOT = PKG_DIR.parent
CSRC = PKG_DIR / "csrc"
HEADER = ROOT / "include" / "fmdemod.h"
DEBUG_HEADER = ROOT / "include" / "fmdemod_debug.h"   # self-test / profiling hooks: not part of the drop-in boundary

FMD_AUDIO_LPR, FMD_AUDIO_LMR, FMD_AUDIO_STEREO = 0, 1, 2
FMD_FLAG_KEEP_TAPS = 1
FMD_FLAG_NO_PIPELINE = 2
FMD_FLAG_PLL_TIME_PARALLEL = 4
FMD_FLAG_PLL_LOW_WORK = 8
FMD_FLAG_PLL_K8 = 16
FMD_FLAG_PLL_STREAM_ORDER = 32
FMD_FLAG_FAST_MATH = 64
FMD_FLAG_RDS_DECODE = 128

# include/fmdemod.h fmd_rds_db (the reference's RDS_Database + sync status, 120 bytes) and fmd_rds_group (4 x fmd_rds_block, 16 bytes)
RDS_DB_DTYPE = np.dtype({
    "names": ["service_name", "programme_type_name", "radio_text", "PI_code", "programme_type", "is_stereo", "is_music",
              "is_artificial_head", "is_compressed", "is_dynamic_program_type", "day", "month", "year", "hour", "minute",
              "local_time_offset", "traffic_announcement", "in_sync", "groups", "sync_acquisitions"],
    "formats": ["S8", "S8", "S64", "<u2", "u1", "u1", "u1", "u1", "u1", "u1", "<i4", "<i4", "<i4", "u1", "u1", "i1", "u1", "<i4", "<u4", "<u4"],
    "offsets": [0, 8, 16, 80, 82, 83, 84, 85, 86, 87, 88, 92, 96, 100, 101, 104, 105, 108, 112, 116],
    "itemsize": 120})
RDS_GROUP_DTYPE = np.dtype([("data", "<u2", (4,)), ("block_type", "u1", (4,)), ("is_valid", "u1", (4,))])   # a view, see _groups_view
FMD_OK, FMD_ERR_ARG, FMD_ERR_SIZE, FMD_ERR_DEVICE, FMD_ERR_NO_DEVICE, FMD_ERR_NAME, FMD_ERR_STATE = 0, -1, -2, -3, -4, -5, -6
FMD_OUTPUT_LIFETIME_BLOCKS = 5   # include/fmdemod.h; checked against the loaded library in load_library()


class FmdError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"fmdemod status {status}: {msg}")
        self.status = status


class Config(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("block_size", C.c_int), ("fs_baseband", C.c_int), ("device", C.c_int), ("flags", C.c_uint)]


class Controls(C.Structure):
    _fields_ = [("audio_out", C.c_int), ("audio_stereo_mix_factor", C.c_float), ("use_deemphasis", C.c_int),
                ("deemphasis_tus", C.c_int), ("lpr_cutoff_hz", C.c_int), ("lmr_cutoff_hz", C.c_int)]


class Rates(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("fs_baseband", "fs_fm_in", "fs_fm_out", "fs_rds", "fs_audio",
                                       "n_baseband", "n_fm_in", "n_fm_out", "n_rds", "n_audio")]


class Coeffs(C.Structure):
    _fields_ = [("fs_baseband", C.c_int), ("m_fm_in", C.c_int), ("b_fm_in", C.c_float * 64), ("b_fm_out", C.c_float * 64),
                ("b_hilbert", C.c_float * 65), ("pilot_b", C.c_float * 3), ("pilot_a", C.c_float * 3),
                ("pll_lpf_b", C.c_float * 2), ("pll_lpf_a", C.c_float * 2), ("deemph_b", C.c_float * 2), ("deemph_a", C.c_float * 2),
                ("b_lpr", C.c_float * 128), ("b_lmr", C.c_float * 128), ("b_rds", C.c_float * 128),
                ("ted_lpf_b", C.c_float * 2), ("ted_lpf_a", C.c_float * 2), ("bpsk_lpf_b", C.c_float * 2), ("bpsk_lpf_a", C.c_float * 2),
                ("fm_gain", C.c_float)]


class ChanConfig(C.Structure):
    _fields_ = [("fs_in", C.c_double), ("fs_out", C.c_double), ("n_stations", C.c_int), ("center_hz", C.POINTER(C.c_double)),
                ("taps_per_phase", C.c_int), ("max_input_samples", C.c_longlong), ("device", C.c_int)]


class ScanConfig(C.Structure):
    _fields_ = [("fs_in", C.c_double), ("nfft", C.c_int), ("max_input_samples", C.c_longlong), ("device", C.c_int)]


class ScanParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("raster_hz", "raster_origin_hz", "channel_bw_hz", "min_snr_db", "usable_fraction", "noise_quantile",
                                          "min_spacing_hz")]


# include/fmdemod.h fmd_scan_station
SCAN_STATION_DTYPE = np.dtype([("offset_hz", "<f8"), ("power_db", "<f8"), ("snr_db", "<f8")])


class ResamplerConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("fs_in", C.c_int), ("fs_out", C.c_int), ("method", C.c_int), ("taps_per_phase", C.c_int),
                ("max_input_frames", C.c_longlong), ("device", C.c_int)]


FMD_RESAMPLE_REFERENCE, FMD_RESAMPLE_POLYPHASE = 0, 1


class IqcorrConfig(C.Structure):
    _fields_ = [("max_input_samples", C.c_longlong), ("device", C.c_int)]


class _IqMomentsC(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("n", "sum_i", "sum_q", "sum_ii", "sum_qq", "sum_iq")]


class _IqCorrectionC(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("dc_i", "dc_q", "w_re", "w_im")]


class IqMoments(NamedTuple):
    """include/fmdemod.h fmd_iq_moments: the count and the five fp64 sums over the raw converted samples"""
    n: float
    sum_i: float
    sum_q: float
    sum_ii: float
    sum_qq: float
    sum_iq: float


class IqCorrection(NamedTuple):
    """include/fmdemod.h fmd_iq_correction (fp32 values): y = z + (w_re + j w_im) conj(z), z = x - (dc_i + j dc_q)"""
    dc_i: float = 0.0
    dc_q: float = 0.0
    w_re: float = 0.0
    w_im: float = 0.0


class MixerConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("n_buses", C.c_int), ("bus_offsets", C.c_void_p), ("bus_sources", C.c_void_p),
                ("gains", C.c_void_p), ("device", C.c_int)]


class MeterConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("fs", C.c_int), ("max_input_frames", C.c_longlong), ("device", C.c_int)]


class MeterDesign(C.Structure):
    """include/fmdemod.h fmd_meter_design_t"""
    _fields_ = [("pre_b", C.c_double * 3), ("pre_a", C.c_double * 3), ("rlb_b", C.c_double * 3), ("rlb_a", C.c_double * 3),
                ("frames_per_subblock", C.c_int), ("edge", C.c_double * 1001), ("centre", C.c_double * 1000)]


# include/fmdemod.h fmd_meter_status (280 bytes)
METER_STATUS_DTYPE = np.dtype([("frames", "<u8"), ("subblocks", "<u8"), ("energy_ring", "<f8", (30,)), ("peak_call", "<f4", (2,)),
                               ("peak_hold", "<f4", (2,)), ("below_gate", "<u4"), ("nonfinite", "<u4")])
METER_BINS = 1000
# fmd_meter_create_ex's feature bits
METER_TRUE_PEAK = 1
METER_RANGE = 2
# include/fmdemod.h fmd_meter_r128_status (24 bytes)
METER_R128_DTYPE = np.dtype([("tp_call", "<f4", (2,)), ("tp_hold", "<f4", (2,)), ("st_below", "<u4"), ("st_nonfinite", "<u4")])


class MeterTpDesign(C.Structure):
    """include/fmdemod.h fmd_meter_tp_design_t"""
    _fields_ = [("L", C.c_int), ("taps_per_phase", C.c_int), ("taps", (C.c_float * 12) * 3)]


class ModmonConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("fs", C.c_int), ("max_input_samples", C.c_longlong), ("device", C.c_int)]


class ModmonDesign(C.Structure):
    """include/fmdemod.h fmd_modmon_design_t"""
    _fields_ = [("fs", C.c_int), ("M", C.c_int), ("P", C.c_int), ("reserved", C.c_int), ("hz_per_rad", C.c_double), ("pilot_gain", C.c_double),
                ("h", C.c_float * 33), ("reserved_f", C.c_float), ("pilot_cos", C.c_double * 384), ("pilot_sin", C.c_double * 384),
                ("edge", C.c_double * 301)]


# include/fmdemod.h fmd_modmon_status (1792 bytes)
MODMON_STATUS_DTYPE = np.dtype([("samples", "<u8"), ("intervals", "<u8"), ("seconds", "<u8"), ("last_hi", "<f4"), ("last_lo", "<f4"),
                                ("hold_hi", "<f4"), ("hold_lo", "<f4"), ("last_s1", "<f8"), ("last_s2", "<f8"), ("last_sc", "<f8"),
                                ("last_ss", "<f8"), ("sec_e", "<f8", (60,)), ("sec_f", "<f8", (60,)), ("sec_q", "<f8", (60,)),
                                ("sec_n", "<u4", (60,)), ("open_e", "<f8"), ("open_f", "<f8"), ("open_q", "<f8"), ("open_n", "<u4"),
                                ("over", "<u4"), ("nonfinite", "<u4"), ("reserved", "<u4")])
MODMON_BINS = 300


class SquelchConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("fs", C.c_int), ("max_input_samples", C.c_longlong), ("device", C.c_int)]


class SquelchParams(C.Structure):
    """include/fmdemod.h fmd_squelch_params"""
    _fields_ = [("open_db", C.c_double), ("close_db", C.c_double), ("min_level_db", C.c_double), ("open_intervals", C.c_int),
                ("close_intervals", C.c_int), ("mode", C.c_int)]


# include/fmdemod.h fmd_squelch_status (368 bytes)
SQUELCH_STATUS_DTYPE = np.dtype([("samples", "<u8"), ("intervals", "<u8"), ("intervals_open", "<u8"), ("ring_s2", "<f8", (20,)),
                                 ("ring_s4", "<f8", (20,)), ("last_peak", "<f4"), ("hold_peak", "<f4"), ("run", "<u4"), ("transitions", "<u4"),
                                 ("nonfinite", "<u4"), ("open", "u1"), ("mode", "u1"), ("reserved", "u1", (2,))])
FMD_SQUELCH_AUTO, FMD_SQUELCH_FORCE_OPEN, FMD_SQUELCH_FORCE_CLOSED = 0, 1, 2


class AudmonConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("fs", C.c_int), ("max_input_frames", C.c_longlong), ("device", C.c_int)]


class AudmonParams(C.Structure):
    """include/fmdemod.h fmd_audmon_params"""
    _fields_ = [("silence_db", C.c_double), ("loss_db", C.c_double), ("antiphase_corr", C.c_double), ("mono_db", C.c_double),
                ("raise_intervals", C.c_int * 5), ("clear_intervals", C.c_int * 5), ("alarm_mask", C.c_uint)]


# include/fmdemod.h fmd_audmon_status (840 bytes)
AUDMON_STATUS_DTYPE = np.dtype([("frames", "<u8"), ("intervals", "<u8"), ("intervals_flagged", "<u8", (5,)), ("ring_ll", "<f8", (30,)),
                                ("ring_rr", "<f8", (30,)), ("ring_lr", "<f8", (30,)), ("last_peak", "<f4", (2,)), ("hold_peak", "<f4", (2,)),
                                ("run", "<u4", (5,)), ("transitions", "<u4", (5,)), ("nonfinite", "<u4"), ("flags", "u1"), ("ok", "u1"),
                                ("reserved", "u1", (2,))])
AUDMON_SILENCE, AUDMON_LEFT_LOST, AUDMON_RIGHT_LOST, AUDMON_ANTIPHASE, AUDMON_MONO = 1, 2, 4, 8, 16


class TonedetConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("fs", C.c_int), ("max_input_frames", C.c_longlong), ("device", C.c_int)]


class TonedetParams(C.Structure):
    """include/fmdemod.h fmd_tonedet_params"""
    _fields_ = [("freq_hz", C.c_int * 8), ("share_db", C.c_double * 8), ("floor_db", C.c_double), ("raise_intervals", C.c_int * 8),
                ("clear_intervals", C.c_int * 8), ("alarm_mask", C.c_uint)]


# include/fmdemod.h fmd_tonedet_status (2344 bytes)
TONEDET_STATUS_DTYPE = np.dtype([("frames", "<u8"), ("intervals", "<u8"), ("intervals_flagged", "<u8", (8,)), ("ring_mm", "<f8", (30,)),
                                 ("ring_pw", "<f8", (8, 30)), ("run", "<u4", (8,)), ("transitions", "<u4", (8,)), ("nonfinite", "<u4"),
                                 ("freq_hz", "<i4", (8,)), ("flags", "u1"), ("ok", "u1"), ("reserved", "u1", (2,))])
TONEDET_SLOTS = 8


class AdpcmConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("block_frames", C.c_int), ("max_input_frames", C.c_longlong), ("device", C.c_int)]


# include/fmdemod.h fmd_adpcm_status (64 bytes)
ADPCM_STATUS_DTYPE = np.dtype([("frames", "<u8"), ("blocks", "<u8"), ("padded", "<u8"), ("clipped", "<u8", (2,)), ("nonfinite", "<u8"), ("fill", "<u4"),
                               ("pred", "<i2", (2,)), ("index", "u1", (2,)), ("reserved", "u1", (6,))])
ADPCM_DEFAULT_BLOCK_FRAMES = 1017
ADPCM_WAV_HEADER_BYTES = 60


class LimiterConfig(C.Structure):
    """include/fmdemod.h fmd_limiter_config"""
    _fields_ = [("n_channels", C.c_int), ("fs", C.c_int), ("lookahead_ms", C.c_double), ("release_ms", C.c_double), ("ceiling_db", C.c_double),
                ("max_input_frames", C.c_longlong), ("device", C.c_int)]


class LimiterDesign(C.Structure):
    """include/fmdemod.h fmd_limiter_design_t"""
    _fields_ = [("lookahead_frames", C.c_int), ("step", C.c_uint), ("ceiling", C.c_float), ("latency_frames", C.c_int)]


# include/fmdemod.h fmd_limiter_status (64 bytes)
LIMITER_STATUS_DTYPE = np.dtype([("frames", "<u8"), ("limited", "<u8"), ("clamped", "<u8", (2,)), ("nonfinite", "<u8"), ("min_gain", "<f4"), ("gain", "<f4"),
                                 ("eq", "<u4"), ("reserved", "u1", (12,))])
assert LIMITER_STATUS_DTYPE.itemsize == 64


class FlacConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("block_frames", C.c_int), ("sample_rate", C.c_int), ("max_input_frames", C.c_longlong), ("device", C.c_int)]


# include/fmdemod.h fmd_flac_status (80 bytes)
FLAC_STATUS_DTYPE = np.dtype([("frames", "<u8"), ("blocks", "<u8"), ("stream_samples", "<u8"), ("stream_bytes", "<u8"), ("clipped", "<u8", (2,)), ("nonfinite", "<u8"),
                              ("streams", "<u4"), ("frame_number", "<u4"), ("min_frame_bytes", "<u4"), ("max_frame_bytes", "<u4"), ("fill", "<u4"), ("wrapped", "<u4")])
assert FLAC_STATUS_DTYPE.itemsize == 80
FLAC_DEFAULT_BLOCK_FRAMES = 4096
FLAC_STREAM_HEADER_BYTES = 42


class LogmelConfig(C.Structure):
    """include/fmdemod.h fmd_logmel_config"""
    _fields_ = [("n_channels", C.c_int), ("fs", C.c_int), ("win", C.c_int), ("hop", C.c_int), ("n_mels", C.c_int), ("f_min_hz", C.c_double),
                ("f_max_hz", C.c_double), ("mel_scale", C.c_int), ("out_mode", C.c_int), ("log_floor", C.c_float), ("max_input_frames", C.c_longlong),
                ("device", C.c_int)]


class LogmelDesign(C.Structure):
    _fields_ = [("n_bins", C.c_int), ("empty_bands", C.c_int)]


# include/fmdemod.h fmd_logmel_status (32 bytes)
LOGMEL_STATUS_DTYPE = np.dtype([("frames", "<u8"), ("spectra", "<u8"), ("nonfinite", "<u8"), ("fill", "<u4"), ("reserved", "<u4")])
assert LOGMEL_STATUS_DTYPE.itemsize == 32
LOGMEL_SLANEY, LOGMEL_HTK = 0, 1
LOGMEL_POWER, LOGMEL_LOG10 = 0, 1


class FprintConfig(C.Structure):
    """include/fmdemod.h fmd_fprint_config"""
    _fields_ = [("n_channels", C.c_int), ("fs", C.c_int), ("hop", C.c_int), ("n_sub", C.c_int), ("n_bands", C.c_int), ("f_min_hz", C.c_double),
                ("f_max_hz", C.c_double), ("max_input_frames", C.c_longlong), ("device", C.c_int)]


class FprintDesign(C.Structure):
    _fields_ = [("n_bins", C.c_int), ("first_bin", C.c_int)]


# include/fmdemod.h fmd_fprint_status (32 bytes)
FPRINT_STATUS_DTYPE = np.dtype([("frames", "<u8"), ("prints", "<u8"), ("nonfinite", "<u8"), ("fill", "<u4"), ("reserved", "<u4")])
assert FPRINT_STATUS_DTYPE.itemsize == 32


class FpmatchConfig(C.Structure):
    """include/fmdemod.h fmd_fpmatch_config"""
    _fields_ = [("n_channels", C.c_int), ("n_bits", C.c_int), ("block", C.c_int), ("interval", C.c_int), ("max_errs", C.c_int), ("hold", C.c_int),
                ("max_words", C.c_int), ("max_tracks", C.c_int), ("max_catalogue_words", C.c_longlong), ("device", C.c_int)]


class FpmatchDesign(C.Structure):
    """include/fmdemod.h fmd_fpmatch_design_t"""
    _fields_ = [("mask", C.c_uint), ("tile", C.c_int), ("query_block", C.c_int), ("groups", C.c_int), ("lds_bytes", C.c_int), ("max_events", C.c_longlong),
                ("max_queries", C.c_longlong)]


# include/fmdemod.h fmd_fpmatch_status (64 bytes) and fmd_fpmatch_event (24 bytes)
FPMATCH_STATUS_DTYPE = np.dtype([("words", "<u8"), ("queries", "<u8"), ("hits", "<u8"), ("clamped", "<u8"), ("since", "<u8"), ("track", "<i4"), ("offset", "<i4"),
                                 ("errs", "<u4"), ("misses", "<u4"), ("fill", "<u4"), ("flags", "<u4")])
FPMATCH_EVENT_DTYPE = np.dtype([("end", "<u8"), ("track", "<i4"), ("offset", "<i4"), ("errs", "<u4"), ("flags", "<u4")])
assert FPMATCH_STATUS_DTYPE.itemsize == 64 and FPMATCH_EVENT_DTYPE.itemsize == 24


class FpmatchIndexConfig(C.Structure):
    """include/fmdemod.h fmd_fpmatch_index_config"""
    _fields_ = [("max_bucket", C.c_int), ("follow", C.c_int)]


class FpmatchIndexDesign(C.Structure):
    """include/fmdemod.h fmd_fpmatch_index_design_t"""
    _fields_ = [("dir_bits", C.c_int), ("chunk", C.c_int), ("chunk_words", C.c_int), ("table", C.c_int), ("dir_entries", C.c_longlong), ("index_bytes", C.c_longlong)]


# include/fmdemod.h fmd_fpmatch_index_status (32 bytes)
FPMATCH_INDEX_STATUS_DTYPE = np.dtype([("candidates", "<u8"), ("skipped", "<u8"), ("followed", "<u8"), ("empty", "<u8")])
assert FPMATCH_INDEX_STATUS_DTYPE.itemsize == 32


class SameConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("fs", C.c_int), ("max_input_frames", C.c_longlong), ("device", C.c_int)]


class SameParams(C.Structure):
    """include/fmdemod.h fmd_same_params"""
    _fields_ = [("pull", C.c_int), ("hold_ticks", C.c_uint), ("alarm_mask", C.c_uint), ("reserved", C.c_uint)]


class SameEncodeConfig(C.Structure):
    """include/fmdemod.h fmd_same_encode_config"""
    _fields_ = [("fs", C.c_int), ("repeats", C.c_int), ("gap_frames", C.c_longlong), ("clock_ratio", C.c_double), ("amplitude", C.c_double),
                ("mark_db", C.c_double)]


class SameHeader(C.Structure):
    """include/fmdemod.h fmd_same_header"""
    _fields_ = [("kind", C.c_int), ("valid", C.c_uint), ("org", C.c_char * 4), ("event", C.c_char * 4), ("n_locations", C.c_int),
                ("locations", (C.c_char * 8) * 31), ("duration_min", C.c_int), ("day", C.c_int), ("hour", C.c_int), ("minute", C.c_int),
                ("callsign", C.c_char * 12)]


# include/fmdemod.h fmd_same_message (280 bytes) and fmd_same_status (2856 bytes)
SAME_MESSAGE_DTYPE = np.dtype([("sync_tick", "<u8"), ("len", "<u2"), ("kind", "u1"), ("reserved", "u1"), ("bytes", "u1", (268,))])
SAME_STATUS_DTYPE = np.dtype([("frames", "<u8"), ("ticks", "<u8"), ("bits", "<u8"), ("syncs", "<u8"), ("accepted", "<u8"), ("rejected", "<u8"),
                              ("sync_tick", "<u8"), ("last_accept_tick", "<u8"), ("open", "<f8", (4,)), ("hist", "<f8", (7, 4)), ("ph", "<u4"),
                              ("sh", "<u4"), ("nbit", "<u4"), ("msg_len", "<u4"), ("run", "<u4"), ("synced", "u1"), ("prev_s", "u1"), ("flags", "u1"),
                              ("ok", "u1"), ("msg", "u1", (268,)), ("reserved", "u1", (4,)), ("ring", SAME_MESSAGE_DTYPE, (8,))])
SAME_SYNCED, SAME_ALERT_OPEN = 1, 2
SAME_KIND_HEADER, SAME_KIND_EOM = 1, 2
SAME_VALID_ORG, SAME_VALID_EVENT, SAME_VALID_LOCATIONS, SAME_VALID_DURATION, SAME_VALID_TIME, SAME_VALID_CALLSIGN = 1, 2, 4, 8, 16, 32
SAME_RING = 8


class PlanInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("effective_channels", "pilot_power_rows", "pll_k_adaptive", "pll_chained", "pll_waves", "lmr_inline", "lazy_capable",
                                       "front_lds_pad", "front_big_tile", "extract_auto_pair", "pll_kernel")]


class PlanFacts(C.Structure):
    """fmd_plan_facts: what the controls and the debug hooks leave behind."""
    _fields_ = [(n, C.c_int) for n in ("any_deemph", "deemph_in_tile", "split_front", "uniform_cutoffs", "extract_pairing")]


class BlockPlanInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("iq_streams", "front_kernel", "front_input", "front_tile", "front_warmup", "front_workgroups", "front_lds_pad", "predecim_kernel",
                                       "predecim_tile", "predecim_workgroups", "deemph_pilot_sums", "deemph_workgroups", "pilot_power_rows", "lmr_phase", "extract_tile",
                                       "extract_bp", "extract_nt", "extract_pair", "extract_grid_x", "rds_kernel", "rds_partials")]


PLL_KERNELS = ("low-work", 16, 8)      # fmd_plan_info.pll_kernel (FMD_PLL_KERNEL_*): the low-work kernel, the time-parallel one's lanes a station


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("total_ms", C.c_double), ("launches", C.c_int)]


def lib_path() -> Path:
    return CSRC / "libfmdemod.so"


def build_library(force: bool = False) -> Path:
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-s", "-C", str(CSRC), "clean"], check=True)
    subprocess.run(["make", "-s", "-C", str(CSRC)], check=True)
    return lib_path()


def declared_symbols(debug: bool = True) -> list[str]:
    """Every function include/fmdemod.h declares (+ include/fmdemod_debug.h's hooks)."""
    names = set()
    for hdr in (HEADER, DEBUG_HEADER) if debug else (HEADER,):
        text = re.sub(r"/\*.*?\*/", "", hdr.read_text(), flags=re.S)
        names |= set(re.findall(r"\b(fmd_[a-z0-9_]+)\s*\(", text))
    return sorted(names)


_lib = None


def load_library():
    """Load libfmdemod.so; raises if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not p.exists():
        raise FileNotFoundError(f"{p} missing: run __graft_entry__.build() / make -C {CSRC}")
    try:
        # torch bundles its own HIP runtime; load it FIRST so this process ends up with a single libamdhip64
        # (two runtimes in one process do not see each other's devices, streams or allocations)
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(str(p))
    H = C.c_void_p
    L.fmd_api_version.restype = C.c_int
    L.fmd_status_string.restype = C.c_char_p
    L.fmd_status_string.argtypes = [C.c_int]
    L.fmd_device_count.restype = C.c_int
    L.fmd_default_controls.argtypes = [C.POINTER(Controls)]
    L.fmd_default_config.argtypes = [C.POINTER(Config), C.c_int, C.c_int]
    L.fmd_create.argtypes = [C.POINTER(Config), C.POINTER(H)]
    L.fmd_destroy.argtypes = [H]
    L.fmd_reset.argtypes = [H]
    L.fmd_set_controls.argtypes = [H, C.c_int, C.POINTER(Controls)]
    L.fmd_get_controls.argtypes = [H, C.c_int, C.POINTER(Controls)]
    L.fmd_get_rates.argtypes = [H, C.POINTER(Rates)]
    L.fmd_get_coeffs.argtypes = [H, C.c_int, C.POINTER(Coeffs)]
    for name in ("fmd_process_cf32_dev", "fmd_process_u8_dev", "fmd_submit_cf32_dev", "fmd_submit_u8_dev"):
        getattr(L, name).argtypes = [H, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    for name in ("fmd_process_cf32_host", "fmd_process_u8_host"):
        getattr(L, name).argtypes = [H, C.c_void_p, C.c_int, C.c_int]
    L.fmd_synchronize.argtypes = [H]
    L.fmd_wait_outputs.argtypes = [H, C.c_void_p]
    L.fmd_set_output_lag.argtypes = [H, C.c_int]
    L.fmd_outputs_block.argtypes = [H, C.POINTER(C.c_long)]
    L.fmd_wait_input.argtypes = [H, C.c_void_p]
    L.fmd_release_outputs.argtypes = [H, C.c_void_p]
    L.fmd_output_lifetime_blocks.restype = C.c_int
    L.fmd_state_size.restype = C.c_size_t
    L.fmd_state_size.argtypes = [H]
    L.fmd_get_state.argtypes = [H, C.c_int, C.c_void_p, C.c_size_t]
    L.fmd_set_state.argtypes = [H, C.c_int, C.c_void_p, C.c_size_t]
    L.fmd_audio_dev.argtypes = [H, C.POINTER(C.c_void_p)]
    L.fmd_audio_pcm16_dev.argtypes = [H, C.c_void_p, C.c_void_p]
    L.fmd_rds_dev.argtypes = [H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.fmd_get_audio.argtypes = [H, C.c_void_p]
    L.fmd_get_rds_symbols.argtypes = [H, C.c_void_p, C.c_void_p]
    L.fmd_get_rds_bytes.argtypes = [H, C.c_void_p, C.c_int, C.c_void_p]
    L.fmd_rds_bytes_dev.argtypes = [H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.fmd_get_stream.argtypes = [H, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.fmd_selftest_atan2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.fmd_selftest_atan2_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.fmd_selftest_atan2_table_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.fmd_selftest_atan2_small.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.fmd_selftest_fast_math.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.fmd_get_spec_stats.argtypes = [H, C.c_void_p, C.c_int]
    L.fmd_design_pll_span.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fmd_profile_enable.argtypes = [H, C.c_int]
    L.fmd_debug_split_front.argtypes = [H, C.c_int]
    L.fmd_debug_pll_adaptive.argtypes = [H, C.c_int, C.c_int]
    L.fmd_debug_extract_pairing.argtypes = [H, C.c_int]
    L.fmd_debug_plan.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int, C.POINTER(PlanInfo)]
    L.fmd_debug_block_plan.argtypes = [C.POINTER(Config), C.POINTER(PlanFacts), C.c_int, C.POINTER(BlockPlanInfo)]
    L.fmd_profile_read.argtypes = [H, C.POINTER(KernelTime), C.c_int, C.POINTER(C.c_int)]
    L.fmd_chan_design.argtypes = [C.c_double, C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.fmd_chan_default_taps_per_phase.restype = C.c_int
    L.fmd_chan_default_taps_per_phase.argtypes = [C.c_double, C.c_double]
    L.fmd_chan_create.argtypes = [C.POINTER(ChanConfig), C.POINTER(C.c_void_p)]
    L.fmd_chan_reset.argtypes = [C.c_void_p]
    L.fmd_chan_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
    L.fmd_chan_get_taps.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.fmd_chan_kernel_form.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    for fmt in ("cf32", "u8", "s8", "s16"):
        getattr(L, f"fmd_chan_process_{fmt}_dev").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.fmd_scan_default_nfft.restype = C.c_int
    L.fmd_scan_default_nfft.argtypes = [C.c_double]
    L.fmd_scan_default_params.restype = None
    L.fmd_scan_default_params.argtypes = [C.POINTER(ScanParams)]
    L.fmd_scan_detect.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(ScanParams), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.fmd_scan_create.argtypes = [C.POINTER(ScanConfig), C.POINTER(C.c_void_p)]
    L.fmd_scan_reset.argtypes = [C.c_void_p]
    for fmt in ("cf32", "u8", "s8", "s16"):
        getattr(L, f"fmd_scan_process_{fmt}_dev").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.fmd_scan_get_psd.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
    L.fmd_scan_stations.argtypes = [C.c_void_p, C.POINTER(ScanParams), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.fmd_iqcorr_create.argtypes = [C.POINTER(IqcorrConfig), C.POINTER(C.c_void_p)]
    for name in ("fmd_iqcorr_reset", "fmd_iqcorr_reset_moments"):
        getattr(L, name).argtypes = [C.c_void_p]
    for fmt in ("cf32", "u8", "s8", "s16"):
        getattr(L, f"fmd_iqcorr_process_{fmt}_dev").argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    L.fmd_iqcorr_get_moments.argtypes = [C.c_void_p, C.POINTER(_IqMomentsC)]
    L.fmd_iqcorr_solve.argtypes = [C.POINTER(_IqMomentsC), C.POINTER(_IqCorrectionC)]
    L.fmd_iqcorr_set_correction.argtypes = [C.c_void_p, C.POINTER(_IqCorrectionC)]
    L.fmd_iqcorr_get_correction.argtypes = [C.c_void_p, C.POINTER(_IqCorrectionC)]
    L.fmd_iqcorr_calibrate.argtypes = [C.c_void_p, C.POINTER(_IqCorrectionC)]
    L.fmd_resampler_design.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.fmd_resampler_create.argtypes = [C.POINTER(ResamplerConfig), C.POINTER(C.c_void_p)]
    L.fmd_resampler_reset.argtypes = [C.c_void_p, C.c_int]
    L.fmd_resampler_set_input_rate.argtypes = [C.c_void_p, C.c_int]
    L.fmd_resampler_output_frames.argtypes = [C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong)]
    for name in ("fmd_resampler_process_f32_dev", "fmd_resampler_process_pcm16_dev", "fmd_resampler_process_f32_host"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong), C.c_void_p]
    L.fmd_mixer_create.argtypes = [C.POINTER(MixerConfig), C.POINTER(C.c_void_p)]
    L.fmd_mixer_set_sources.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.fmd_mixer_set_gain.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.fmd_mixer_get_gain.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    for name in ("fmd_mixer_process_f32_dev", "fmd_mixer_process_f32_host"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    L.fmd_meter_design.argtypes = [C.c_int, C.POINTER(MeterDesign)]
    L.fmd_meter_lufs.restype = C.c_double
    L.fmd_meter_lufs.argtypes = [C.c_double]
    L.fmd_meter_integrated.argtypes = [C.c_void_p, C.POINTER(MeterDesign), C.POINTER(C.c_double)]
    L.fmd_meter_momentary.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.fmd_meter_short_term.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.fmd_meter_create.argtypes = [C.POINTER(MeterConfig), C.POINTER(C.c_void_p)]
    L.fmd_meter_process_f32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p]
    L.fmd_meter_get_histogram.argtypes = [C.c_void_p, C.c_void_p]
    L.fmd_meter_create_ex.argtypes = [C.POINTER(MeterConfig), C.c_uint, C.POINTER(C.c_void_p)]
    L.fmd_meter_features.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    L.fmd_meter_tp_design.argtypes = [C.c_int, C.POINTER(MeterTpDesign)]
    L.fmd_meter_dbtp.restype = C.c_double
    L.fmd_meter_dbtp.argtypes = [C.c_float]
    L.fmd_meter_get_r128_status.argtypes = [C.c_void_p, C.c_void_p]
    L.fmd_meter_r128_status_dev.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.fmd_meter_get_range_histogram.argtypes = [C.c_void_p, C.c_void_p]
    L.fmd_meter_range.argtypes = [C.c_void_p, C.POINTER(MeterDesign), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.fmd_modmon_design.argtypes = [C.c_int, C.POINTER(ModmonDesign)]
    for fn in ("fmd_modmon_deviation_hz", "fmd_modmon_offset_hz", "fmd_modmon_pilot_hz"):
        getattr(L, fn).argtypes = [C.c_void_p, C.POINTER(ModmonDesign), C.POINTER(C.c_double)]
    L.fmd_modmon_mpx_power_dbr.argtypes = [C.c_void_p, C.POINTER(ModmonDesign), C.c_int, C.POINTER(C.c_double)]
    L.fmd_modmon_exceedance.argtypes = [C.c_void_p, C.c_uint, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)]
    L.fmd_modmon_percentile.argtypes = [C.c_void_p, C.c_uint, C.c_double, C.POINTER(C.c_double)]
    L.fmd_modmon_create.argtypes = [C.POINTER(ModmonConfig), C.POINTER(C.c_void_p)]
    L.fmd_modmon_process_cf32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p]
    L.fmd_modmon_process_u8_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p]
    L.fmd_modmon_get_histogram.argtypes = [C.c_void_p, C.c_void_p]
    L.fmd_squelch_default_params.argtypes = [C.POINTER(SquelchParams)]
    L.fmd_squelch_default_params.restype = None
    L.fmd_squelch_threshold.argtypes = [C.c_double]
    L.fmd_squelch_threshold.restype = C.c_double
    L.fmd_squelch_level_db.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    L.fmd_squelch_cnr_db.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.fmd_squelch_powers.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.fmd_squelch_create.argtypes = [C.POINTER(SquelchConfig), C.POINTER(C.c_void_p)]
    L.fmd_squelch_set_params.argtypes = [C.c_void_p, C.c_int, C.POINTER(SquelchParams)]
    L.fmd_squelch_get_params.argtypes = [C.c_void_p, C.c_int, C.POINTER(SquelchParams)]
    L.fmd_squelch_process_cf32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fmd_squelch_process_u8_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fmd_audmon_default_params.argtypes = [C.POINTER(AudmonParams)]
    L.fmd_audmon_default_params.restype = None
    L.fmd_audmon_level_db.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.fmd_audmon_balance_db.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.fmd_audmon_correlation.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.fmd_audmon_side_mid_db.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.fmd_audmon_create.argtypes = [C.POINTER(AudmonConfig), C.POINTER(C.c_void_p)]
    L.fmd_audmon_set_params.argtypes = [C.c_void_p, C.c_int, C.POINTER(AudmonParams)]
    L.fmd_audmon_get_params.argtypes = [C.c_void_p, C.c_int, C.POINTER(AudmonParams)]
    L.fmd_audmon_process_f32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fmd_tonedet_default_params.argtypes = [C.POINTER(TonedetParams)]
    L.fmd_tonedet_default_params.restype = None
    L.fmd_tonedet_share_db.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.fmd_tonedet_level_db.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.fmd_tonedet_create.argtypes = [C.POINTER(TonedetConfig), C.POINTER(C.c_void_p)]
    L.fmd_tonedet_set_params.argtypes = [C.c_void_p, C.c_int, C.POINTER(TonedetParams)]
    L.fmd_tonedet_get_params.argtypes = [C.c_void_p, C.c_int, C.POINTER(TonedetParams)]
    L.fmd_tonedet_process_f32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fmd_adpcm_block_align.argtypes = [C.c_int]
    L.fmd_adpcm_max_blocks.argtypes = [C.c_int, C.c_longlong]
    L.fmd_adpcm_max_blocks.restype = C.c_longlong
    L.fmd_adpcm_decode_blocks.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p]
    L.fmd_adpcm_wav_header.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p, C.POINTER(C.c_int)]
    L.fmd_adpcm_create.argtypes = [C.POINTER(AdpcmConfig), C.POINTER(C.c_void_p)]
    L.fmd_adpcm_process_f32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    L.fmd_adpcm_flush.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    L.fmd_limiter_design.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(LimiterDesign)]
    L.fmd_limiter_default_config.argtypes = [C.c_int, C.POINTER(LimiterConfig)]
    L.fmd_limiter_gain_for_loudness.argtypes = [C.c_double, C.c_double]
    L.fmd_limiter_gain_for_loudness.restype = C.c_float
    L.fmd_limiter_create.argtypes = [C.POINTER(LimiterConfig), C.POINTER(C.c_void_p)]
    L.fmd_limiter_set_gain.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.fmd_limiter_get_gain.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    L.fmd_limiter_process_f32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    L.fmd_limiter_flush.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    L.fmd_limiter_debug_set_frames.argtypes = [C.c_void_p, C.c_int, C.c_ulonglong]
    L.fmd_flac_frame_bound.argtypes = [C.c_int]
    L.fmd_flac_max_bytes.argtypes = [C.c_int, C.c_longlong]
    L.fmd_flac_max_bytes.restype = C.c_longlong
    L.fmd_flac_stream_header.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    L.fmd_flac_decode.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong)]
    L.fmd_flac_create.argtypes = [C.POINTER(FlacConfig), C.POINTER(C.c_void_p)]
    L.fmd_flac_process_f32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fmd_flac_flush.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fmd_debug_flac_set_frame_number.argtypes = [C.c_void_p, C.c_int, C.c_uint]
    L.fmd_logmel_default_config.argtypes = [C.c_int, C.POINTER(LogmelConfig)]
    L.fmd_logmel_design.argtypes = [C.POINTER(LogmelConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LogmelDesign)]
    L.fmd_logmel_bins.argtypes = [C.POINTER(LogmelConfig)]
    L.fmd_logmel_max_frames.argtypes = [C.c_int, C.c_longlong]
    L.fmd_logmel_max_frames.restype = C.c_longlong
    L.fmd_logmel_flog10.argtypes = [C.c_float]
    L.fmd_logmel_flog10.restype = C.c_float
    L.fmd_logmel_create.argtypes = [C.POINTER(LogmelConfig), C.POINTER(C.c_void_p)]
    L.fmd_logmel_process_f32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    L.fmd_fprint_default_config.argtypes = [C.c_int, C.POINTER(FprintConfig)]
    L.fmd_fprint_design.argtypes = [C.POINTER(FprintConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FprintDesign)]
    L.fmd_fprint_bins.argtypes = [C.POINTER(FprintConfig)]
    L.fmd_fprint_max_prints.argtypes = [C.c_int, C.c_longlong]
    L.fmd_fprint_max_prints.restype = C.c_longlong
    L.fmd_fprint_state_bytes.argtypes = [C.POINTER(FprintConfig), C.c_int]
    L.fmd_fprint_state_bytes.restype = C.c_longlong
    L.fmd_fprint_create.argtypes = [C.POINTER(FprintConfig), C.POINTER(C.c_void_p)]
    L.fmd_fprint_process_f32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                             C.c_longlong, C.c_void_p]
    L.fmd_fpmatch_default_config.argtypes = [C.POINTER(FpmatchConfig)]
    L.fmd_fpmatch_max_events.argtypes = [C.c_int, C.c_longlong]
    L.fmd_fpmatch_max_events.restype = C.c_longlong
    L.fmd_fpmatch_max_errs.argtypes = [C.c_int, C.c_int, C.c_int]
    L.fmd_fpmatch_max_errs.restype = C.c_longlong
    L.fmd_fpmatch_design.argtypes = [C.POINTER(FpmatchConfig), C.POINTER(FpmatchDesign)]
    L.fmd_fpmatch_check_catalogue.argtypes = [C.POINTER(FpmatchConfig), C.c_void_p, C.c_int]
    L.fmd_fpmatch_state_bytes.argtypes = [C.POINTER(FpmatchConfig)]
    L.fmd_fpmatch_state_bytes.restype = C.c_longlong
    L.fmd_fpmatch_create.argtypes = [C.POINTER(FpmatchConfig), C.POINTER(C.c_void_p)]
    L.fmd_fpmatch_load.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.fmd_fpmatch_index_default_config.argtypes = [C.POINTER(FpmatchIndexConfig)]
    L.fmd_fpmatch_index_design.argtypes = [C.POINTER(FpmatchConfig), C.POINTER(FpmatchIndexConfig), C.POINTER(FpmatchIndexDesign)]
    L.fmd_fpmatch_index_state_bytes.argtypes = [C.POINTER(FpmatchConfig), C.POINTER(FpmatchIndexConfig)]
    L.fmd_fpmatch_index_state_bytes.restype = C.c_longlong
    L.fmd_fpmatch_index_build.argtypes = [C.POINTER(FpmatchConfig), C.POINTER(FpmatchIndexConfig), C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fmd_fpmatch_create_ex.argtypes = [C.POINTER(FpmatchConfig), C.POINTER(FpmatchIndexConfig), C.POINTER(C.c_void_p)]
    L.fmd_fpmatch_get_index_status.argtypes = [C.c_void_p, C.c_void_p]
    L.fmd_fpmatch_process_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
    L.fmd_same_default_params.argtypes = [C.POINTER(SameParams)]
    L.fmd_same_default_params.restype = None
    L.fmd_same_encode.argtypes = [C.POINTER(SameEncodeConfig), C.c_char_p, C.c_int, C.c_void_p, C.c_longlong]
    L.fmd_same_encode.restype = C.c_longlong
    L.fmd_same_parse.argtypes = [C.c_char_p, C.c_int, C.POINTER(SameHeader)]
    L.fmd_same_vote.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.fmd_same_create.argtypes = [C.POINTER(SameConfig), C.POINTER(C.c_void_p)]
    L.fmd_same_set_params.argtypes = [C.c_void_p, C.c_int, C.POINTER(SameParams)]
    L.fmd_same_get_params.argtypes = [C.c_void_p, C.c_int, C.POINTER(SameParams)]
    L.fmd_same_process_f32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # what every side object declares alike
    for pre in ("chan", "scan", "iqcorr", "resampler", "mixer", "meter", "modmon", "squelch", "audmon", "tonedet", "adpcm", "same", "flac", "logmel", "fprint", "fpmatch", "limiter", "rdsdec"):
        getattr(L, f"fmd_{pre}_destroy").argtypes = [C.c_void_p]
        getattr(L, f"fmd_{pre}_last_error").restype = C.c_char_p
        getattr(L, f"fmd_{pre}_last_error").argtypes = [C.c_void_p]
    for pre in ("meter", "modmon", "squelch", "audmon", "tonedet", "adpcm", "same", "flac", "logmel", "fprint", "fpmatch", "limiter"):
        getattr(L, f"fmd_{pre}_reset").argtypes = [C.c_void_p, C.c_int]
        if pre not in ("tonedet", "adpcm", "same", "flac", "logmel", "fprint", "fpmatch", "limiter"):   # (the tone detector, the encoders, the SAME decoder, the log-mel front end, the fingerprinter, the matcher and the limiter hold no peaks)
            getattr(L, f"fmd_{pre}_reset_peaks").argtypes = [C.c_void_p, C.c_int]
        getattr(L, f"fmd_{pre}_get_status").argtypes = [C.c_void_p, C.c_void_p]
        getattr(L, f"fmd_{pre}_status_dev").argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.fmd_last_error.restype = C.c_char_p
    L.fmd_last_error.argtypes = [H]
    if L.fmd_output_lifetime_blocks() != FMD_OUTPUT_LIFETIME_BLOCKS:
        raise RuntimeError("libfmdemod.so and capi.py disagree on FMD_OUTPUT_LIFETIME_BLOCKS")
    _lib = L
    return L


def selftest_atan2(y: np.ndarray, x: np.ndarray, table_form: bool = False) -> np.ndarray:
    """The kernels' atan2f evaluated on the device (fmd_selftest_atan2; table_form: the discriminator's variant)."""
    y = np.ascontiguousarray(y, np.float32); x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(y)
    L = load_library()
    fn = L.fmd_selftest_atan2_table_u8 if table_form == "u8" else (L.fmd_selftest_atan2_table if table_form else L.fmd_selftest_atan2)
    rc = fn(y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), y.size)
    if rc != FMD_OK:
        raise FmdError(rc, load_library().fmd_last_error(None).decode())
    return out


def selftest_fast_math(kind: str, a: np.ndarray, b: np.ndarray | None = None) -> np.ndarray:
    """The tolerance mode's primitives on the device: kind in {"atan2", "sin_turns", "cos_turns", "atan2_turns"}."""
    a = np.ascontiguousarray(a, np.float32)
    b = a if b is None else np.ascontiguousarray(b, np.float32)
    out = np.empty_like(a)
    rc = load_library().fmd_selftest_fast_math({"atan2": 0, "sin_turns": 1, "cos_turns": 2, "atan2_turns": 3}[kind], a.ctypes.data_as(C.c_void_p),
                                               b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), a.size)
    if rc != FMD_OK:
        raise FmdError(rc, load_library().fmd_last_error(None).decode())
    return out


def selftest_atan2_small(y: np.ndarray, x: np.ndarray):
    """The locked-loop short form of atan2f on the device: (values, ok) — values are exact wherever ok is True."""
    y = np.ascontiguousarray(y, np.float32); x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(y); ok = np.empty(y.size, np.uint8)
    rc = load_library().fmd_selftest_atan2_small(y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                                 ok.ctypes.data_as(C.c_void_p), y.size)
    if rc != FMD_OK:
        raise FmdError(rc, load_library().fmd_last_error(None).decode())
    return out, ok.astype(bool).reshape(y.shape)


def default_controls() -> Controls:
    c = Controls()
    load_library().fmd_default_controls(C.byref(c))
    return c


def default_config(n_channels: int, fs_baseband: int = 1_024_000) -> "Config":
    """fmd_default_config: 64 ms blocks, the tolerance mode (what a many-station deployment wants; flags = 0 is the bit-exact mode)."""
    cfg = Config()
    rc = load_library().fmd_default_config(C.byref(cfg), n_channels, fs_baseband)
    if rc != FMD_OK:
        raise FmdError(rc, "unsupported configuration")
    return cfg


def plan(cfg: "Config", pll_thresholds=None, unlocked_now: bool = False) -> PlanInfo:
    """fmd_debug_plan (host only, no GPU): which kernels the library picks for cfg; pll_thresholds = (k16_max, time_parallel_max) as after
    BatchDemod.pll_adaptive, None = the defaults.  PLL_KERNELS[info.pll_kernel] is what tests read off spec_stats."""
    out = PlanInfo()
    k16, tp = (-1, -1) if pll_thresholds is None else pll_thresholds
    rc = load_library().fmd_debug_plan(C.byref(cfg), int(k16), int(tp), 1 if unlocked_now else 0, C.byref(out))
    if rc != FMD_OK:
        raise FmdError(rc, "unsupported configuration")
    return out


def block_plan(cfg: "Config", facts: "PlanFacts" = None, u8: bool = False) -> BlockPlanInfo:
    """fmd_debug_block_plan (host only, no GPU): each stage's kernel form and launch geometry for cfg, for u8 or cf32 captures, given the run-time facts
    (None: a fresh handle's, no fact set)."""
    out = BlockPlanInfo()
    rc = load_library().fmd_debug_block_plan(C.byref(cfg), C.byref(facts if facts is not None else PlanFacts()), 1 if u8 else 0, C.byref(out))
    if rc != FMD_OK:
        raise FmdError(rc, "unsupported configuration")
    return out


def _groups_view(raw: np.ndarray) -> np.ndarray:
    """uint8 [..., 16] group records -> RDS_GROUP_DTYPE [...] (the C layout interleaves data / type / valid per block)."""
    blocks = raw.reshape(raw.shape[:-1] + (4, 4))
    out = np.empty(raw.shape[:-1], RDS_GROUP_DTYPE)
    out["data"] = blocks[..., 0].astype(np.uint16) | (blocks[..., 1].astype(np.uint16) << 8)
    out["block_type"] = blocks[..., 2]
    out["is_valid"] = blocks[..., 3]
    return out


def _groups_lists(raw: np.ndarray, counts: np.ndarray) -> list:
    return [_groups_view(raw[c, : int(counts[c])]) for c in range(raw.shape[0])]


def _stream_ptr(stream, device=None):
    """a call's stream as a raw stream pointer: None is torch's current stream on `device`; a torch stream (anything with .cuda_stream) or
    an int is taken as given"""
    if stream is None:
        import torch
        return torch.cuda.current_stream(device).cuda_stream
    return getattr(stream, "cuda_stream", stream)


def _batch_input(x, n_channels: int, n, dtypes: tuple, noun: str):
    """the per-station input of a side object, x: [C, >= n, 2] of one of `dtypes` (torch dtype names) on the device with contiguous `noun`
    (frames or samples) -> (pointer, in_stride, n), n defaulting to all of x"""
    import torch
    if not (x.is_cuda and x.dtype in [getattr(torch, d) for d in dtypes] and x.dim() == 3 and x.shape[0] == n_channels and x.shape[2] == 2
            and x.stride(2) == 1 and x.stride(1) == 2):
        raise ValueError(f"x must be a CUDA {' or '.join(dtypes)} tensor [C, n, 2] with contiguous {noun}")
    in_stride = x.stride(0) // 2 if x.shape[0] > 1 else x.shape[1]     # (a batch of one may carry any stride on its first axis)
    return C.c_void_p(x.data_ptr()), in_stride, int(x.shape[1]) if n is None else int(n)


def _active_ptr(active, n_channels: int):
    """the `active` argument of a process call, None or a [C] uint8 / bool CUDA tensor -> the pointer the library takes (None: every station)"""
    if active is None:
        return None
    import torch
    if active.dtype == torch.bool:
        active = active.view(torch.uint8)
    if not (active.is_cuda and active.dtype == torch.uint8 and active.shape == (n_channels,) and active.is_contiguous()):
        raise ValueError("active must be a contiguous [C] uint8 or bool CUDA tensor")
    return C.c_void_p(active.data_ptr())


def _byte_out(t, name: str, n_channels: int, device, stream):
    """a [C] uint8 output of a process call -> (tensor, pointer): the caller's tensor, None = a new one, False = not written (None, None)"""
    import torch
    if t is False:
        return None, None
    if t is None:
        # zeroed on the stream the call then writes it on (0 is the default stream, on which torch works unless told otherwise)
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device) if stream else torch.cuda.default_stream(device)):
            t = torch.zeros(n_channels, dtype=torch.uint8, device=device)
    elif not (t.is_cuda and t.dtype == torch.uint8 and t.shape == (n_channels,) and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous [C] uint8 CUDA tensor")
    return t, C.c_void_p(t.data_ptr())


def _global_error(L, prefix: str, rc: int) -> FmdError:
    """the FmdError of a call without a handle (a create, a host-only function): the object's global message, else the status string"""
    return FmdError(rc, getattr(L, f"{prefix}_last_error")(None).decode() or L.fmd_status_string(rc).decode())


def _record_read(prefix: str, fn: str, record, dtype, *args, outs: int = 1):
    """prefix_fn(record, *args, &out ...) of one status record of `dtype` (host only): the double read out, or a tuple of `outs` of them"""
    L = load_library()
    r = np.ascontiguousarray(record, dtype).reshape(-1)
    if r.size != 1:
        raise ValueError("one status record at a time")
    out = [C.c_double(0.0) for _ in range(outs)]
    rc = getattr(L, f"{prefix}_{fn}")(r.ctypes.data_as(C.c_void_p), *args, *(C.byref(o) for o in out))
    if rc != FMD_OK:
        raise _global_error(L, prefix, rc)
    return out[0].value if outs == 1 else tuple(o.value for o in out)


class _Handle:
    """What the side classes and RDSDecoder share: the library in self.L and one opaque handle of the C object `_prefix`, kept in the
    attribute named `_attr` (None after a failed create and after close())."""
    _prefix = ""
    _attr = "h"

    @property
    def _h(self):
        return getattr(self, self._attr, None)

    def _fn(self, name: str):
        """the library's function prefix_name"""
        return getattr(self.L, f"{self._prefix}_{name}")

    def _create(self, fn: str, *args):
        """self.L and the handle from prefix_fn(*args, &handle); raises FmdError with create's own message (else the status string)"""
        self.L = load_library()
        h = C.c_void_p()
        rc = self._fn(fn)(*args, C.byref(h))
        setattr(self, self._attr, h if rc == FMD_OK else None)
        if rc != FMD_OK:
            raise _global_error(self.L, self._prefix, rc)

    def close(self):
        """destroys the C object (waiting for its work); safe to repeat, and after a failed create"""
        if self._h:
            self._fn("destroy")(self._h)
            setattr(self, self._attr, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        """a C call's status: raises FmdError for an error, with the handle's message (else the status string); returns rc otherwise"""
        if rc < 0:
            raise FmdError(rc, (self._fn("last_error")(self._h) or b"").decode() or self.L.fmd_status_string(rc).decode())
        return rc


class _Monitor(_Handle):
    """The five per-station monitors (meter, modmon, squelch, audmon, tonedet), the ADPCM encoder and the SAME decoder: [C] status records of `_status_dtype` that reset
    the same way."""
    _status_dtype = None

    def reset(self, channel: int = -1):
        """station `channel` (-1 = every station) as after create; waits for the object's work"""
        self._check(self._fn("reset")(self._h, int(channel)))

    def reset_peaks(self, channel: int = -1):
        """the held peaks alone of station `channel` (-1 = every station)"""
        self._check(self._fn("reset_peaks")(self._h, int(channel)))

    def status(self) -> np.ndarray:
        """[C] records of the class's status dtype; waits for the object's work"""
        out = np.zeros(self.n_channels, self._status_dtype)
        self._check(self._fn("get_status")(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def status_dev_ptr(self) -> int:
        """prefix_status_dev: the address of the device's own [C] records, valid until the next process call"""
        p = C.c_void_p()
        self._check(self._fn("status_dev")(self._h, C.byref(p)))
        return p.value


class _Gated(_Monitor):
    """The objects with per-station parameters (squelch, audmon, tonedet, same): a ctypes structure `_params_type` read and set by field name."""
    _params_type = None

    def _field(self, name: str, value):
        """a field's value as the structure takes it"""
        return value

    def set_params(self, channel: int = -1, **fields):
        """prefix_set_params: the named fields of the parameters for station `channel` (-1 = every station, each keeping its other
        fields); ordered behind the object's earlier work, they apply from the next interval that ends"""
        for c in (range(self.n_channels) if channel < 0 else (int(channel),)):
            p = self.params(c)
            for k, v in fields.items():
                if k not in dict(self._params_type._fields_):
                    raise TypeError(f"{self._params_type.__name__} has no field {k}")
                setattr(p, k, self._field(k, v))
            self._check(self._fn("set_params")(self._h, c, C.byref(p)))

    def params(self, channel: int):
        """prefix_get_params: station `channel`'s parameters, as set"""
        p = self._params_type()
        self._check(self._fn("get_params")(self._h, int(channel), C.byref(p)))
        return p


class RDSDecoder(_Handle):
    """Standalone batched RDS decoding chain on the GPU (fmd_rdsdec_*): the reference's RDS_Decoding_Chain for C byte streams from
    any source (a demodulator's RDS bytes, the scraper's _rds.bin files).  State carries over between process() calls."""
    _prefix, _attr = "fmd_rdsdec", "d"

    def __init__(self, n_channels: int, device: int = -1):
        self._create("create", n_channels, device)
        self.n_channels = n_channels
        self._gcap = 0

    def reset(self):
        self._check(self.L.fmd_rdsdec_reset(self.d))

    def reset_db(self, channel: int = -1):
        self._check(self.L.fmd_rdsdec_reset_db(self.d, channel))

    def process(self, data: np.ndarray, counts) -> None:
        """data: uint8 [C, cap] host array, counts[c] bytes of row c (any number 0..cap).  Synchronous."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        assert data.ndim == 2 and data.shape[0] == self.n_channels and counts.shape == (self.n_channels,)
        self._check(self.L.fmd_rdsdec_process_host(self.d, data.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), data.shape[1]))
        self._gcap = self.L.fmd_rdsdec_groups_cap(data.shape[1])

    def process_tensor(self, data, counts, stream=None) -> None:
        """data: torch uint8 [C, cap] and counts int32 [C] on the device; asynchronous on `stream` (default: torch's current stream)."""
        import torch
        s = _stream_ptr(stream)
        assert data.is_contiguous() and counts.is_contiguous() and data.dtype == torch.uint8 and counts.dtype == torch.int32
        self._check(self.L.fmd_rdsdec_process_dev(self.d, C.c_void_p(data.data_ptr()), C.c_void_p(counts.data_ptr()), data.shape[1], C.c_void_p(s)))
        self._gcap = self.L.fmd_rdsdec_groups_cap(data.shape[1])

    def db(self) -> np.ndarray:
        """RDS_DB_DTYPE [C]: every channel's database after the last call."""
        out = np.zeros(self.n_channels, RDS_DB_DTYPE)
        self._check(self.L.fmd_rdsdec_get_db(self.d, out.ctypes.data_as(C.c_void_p)))
        return out

    def groups_raw(self) -> tuple[np.ndarray, np.ndarray]:
        """(uint8 [C, cap, 16] group records in the C layout, counts [C]) of the last call."""
        cap = max(self._gcap, 1)
        raw = np.zeros((self.n_channels, cap, 16), np.uint8)
        counts = np.zeros(self.n_channels, np.int32)
        self._check(self.L.fmd_rdsdec_get_groups(self.d, raw.ctypes.data_as(C.c_void_p), cap, counts.ctypes.data_as(C.c_void_p)))
        return raw, counts

    def groups(self) -> list:
        """Per channel the groups the last call delivered, RDS_GROUP_DTYPE [n]."""
        return _groups_lists(*self.groups_raw())


class BatchDemod:
    """C broadcast-FM demodulators advanced in lock-step on one MI355X."""

    def __init__(self, n_channels: int, block_size: int = 65536, fs_baseband: int = 1_024_000, device: int = -1, keep_taps: bool = False,
                 pipelined: bool = True, pll_kernel: str = "auto", pll_stream_order: bool = False, fast_math: bool = False,
                 rds_decode: bool = False):
        self.L = load_library()
        self.h = C.c_void_p()
        flags = (FMD_FLAG_KEEP_TAPS if keep_taps else 0) | (0 if pipelined else FMD_FLAG_NO_PIPELINE)
        flags |= {"auto": 0, "time_parallel": FMD_FLAG_PLL_TIME_PARALLEL, "time_parallel8": FMD_FLAG_PLL_TIME_PARALLEL | FMD_FLAG_PLL_K8,
                  "low_work": FMD_FLAG_PLL_LOW_WORK}[pll_kernel]
        flags |= FMD_FLAG_PLL_STREAM_ORDER if pll_stream_order else 0
        flags |= FMD_FLAG_FAST_MATH if fast_math else 0
        flags |= FMD_FLAG_RDS_DECODE if rds_decode else 0
        cfg = Config(n_channels, block_size, fs_baseband, device, flags)
        rc = self.L.fmd_create(C.byref(cfg), C.byref(self.h))
        if rc != FMD_OK:
            msg = self.L.fmd_last_error(None).decode()
            self.h = None
            raise FmdError(rc, msg or self.L.fmd_status_string(rc).decode())
        self.n_channels, self.block_size, self.fs_baseband = n_channels, block_size, fs_baseband
        r = Rates()
        self._check(self.L.fmd_get_rates(self.h, C.byref(r)))
        self.rates = r
        self.bytes_cap = 16 * (r.n_rds // 256 + 1)
        self.groups_cap = self.bytes_cap * 8 // 79 + 2     # fmd_rds_groups_dev's cap (k_rds_decode: one group per >= 79 new bits)
        self.rds_decode = rds_decode

    def close(self):
        if getattr(self, "h", None):
            self.L.fmd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != FMD_OK:
            raise FmdError(rc, self.L.fmd_last_error(self.h).decode() or self.L.fmd_status_string(rc).decode())

    # -- controls (reference GetControls(), broadcast_fm_demod.h:294) --
    def set_controls(self, controls: Controls, channel: int = -1):
        self._check(self.L.fmd_set_controls(self.h, channel, C.byref(controls)))

    def get_coeffs(self, channel: int = 0) -> Coeffs:
        k = Coeffs()
        self._check(self.L.fmd_get_coeffs(self.h, channel, C.byref(k)))
        return k

    def reset(self):
        self._check(self.L.fmd_reset(self.h))

    # -- Process (reference broadcast_fm_demod.cpp:309-328) --
    def process(self, iq, stream=None) -> int:
        """iq: [C, N, 2] float32 or uint8; torch CUDA tensor (device entry point) or numpy array (host entry point).
        Returns the status code (FMD_ERR_SIZE for a dropped block) without raising for size mismatches."""
        is_torch = hasattr(iq, "data_ptr")
        shape = tuple(iq.shape)
        if len(shape) != 3 or shape[2] != 2:
            raise ValueError("iq must be [C, N, 2]")
        if is_torch:
            import torch
            if not iq.is_cuda or not iq.is_contiguous():
                raise ValueError("torch input must be a contiguous CUDA tensor")
            if stream is None:
                stream = torch.cuda.current_stream(iq.device).cuda_stream
            fn = {torch.float32: self.L.fmd_process_cf32_dev, torch.uint8: self.L.fmd_process_u8_dev}[iq.dtype]
            rc = fn(self.h, iq.data_ptr(), shape[0], shape[1], C.c_void_p(stream))
        else:
            a = np.ascontiguousarray(iq)
            fn = {np.dtype(np.float32): self.L.fmd_process_cf32_host, np.dtype(np.uint8): self.L.fmd_process_u8_host}[a.dtype]
            rc = fn(self.h, a.ctypes.data_as(C.c_void_p), shape[0], shape[1])
        if rc not in (FMD_OK, FMD_ERR_SIZE):
            self._check(rc)
        return rc

    def submit(self, iq, ready_stream=None) -> int:
        """fmd_submit_*_dev: like process() for a torch CUDA tensor, but nothing is queued on the caller's streams.  The block is
        read after everything already queued on `ready_stream` (None: the data is in place now); wait_input() tells when the
        buffer may be rewritten.  For hosts that rotate input buffers (bench.py's resident blocks, station_ring.hpp)."""
        import torch
        shape = tuple(iq.shape)
        if len(shape) != 3 or shape[2] != 2 or not iq.is_cuda or not iq.is_contiguous():
            raise ValueError("iq must be a contiguous CUDA tensor [C, N, 2]")
        if hasattr(ready_stream, "cuda_stream"):
            ready_stream = ready_stream.cuda_stream
        fn = {torch.float32: self.L.fmd_submit_cf32_dev, torch.uint8: self.L.fmd_submit_u8_dev}[iq.dtype]
        rc = fn(self.h, iq.data_ptr(), shape[0], shape[1], C.c_void_p(ready_stream) if ready_stream else None)
        if rc not in (FMD_OK, FMD_ERR_SIZE):
            self._check(rc)
        return rc

    def wait_input(self, stream=None):
        """Make `stream` wait (on the device) until the newest submitted block's input buffer has been read."""
        stream = _stream_ptr(stream)
        self._check(self.L.fmd_wait_input(self.h, C.c_void_p(stream)))

    def synchronize(self):
        self._check(self.L.fmd_synchronize(self.h))

    def pll_adaptive(self, k16_max_channels: int, time_parallel_max_channels: int = 7168) -> None:
        """fmd_debug_pll_adaptive: exact mode — the batch sizes from which the pilot-PLL kernel (its lane count; low-work or time-parallel) is picked
        by what is out of lock (small values let a small batch exercise the switches)."""
        self._check(self.L.fmd_debug_pll_adaptive(self.h, int(k16_max_channels), int(time_parallel_max_channels)))

    def set_extract_pairing(self, mode: int) -> None:
        """fmd_debug_extract_pairing: 0 auto, 1 wherever possible, 2 never (k_extract_bp with two stations per workgroup)."""
        self._check(self.L.fmd_debug_extract_pairing(self.h, int(mode)))

    def set_output_lag(self, on: bool) -> None:
        """fmd_set_output_lag: with on=True the device-side output calls (wait_outputs, release_outputs, audio_tensor, audio_pcm16_into,
        ...) refer to the newest block whose output stages are QUEUED — behind submit() of block k that is block k - 1 in the
        tolerance mode — and never force a put-off stage."""
        self._check(self.L.fmd_set_output_lag(self.h, 1 if on else 0))

    def outputs_block(self) -> int:
        """fmd_outputs_block: index (0 = first since create / reset) of the block the device-side output calls refer to, -1 = none yet."""
        b = C.c_long(-1)
        self._check(self.L.fmd_outputs_block(self.h, C.byref(b)))
        return int(b.value)

    def wait_outputs(self, stream=None):
        """Make `stream` (torch stream or raw handle; default: torch current stream) wait for the newest block's outputs."""
        stream = _stream_ptr(stream)
        self._check(self.L.fmd_wait_outputs(self.h, C.c_void_p(stream)))

    def release_outputs(self, stream=None):
        """Tell the library that everything queued on `stream` so far reads the newest block's output views: their buffers are
        not reused before that work has finished (fmd_release_outputs; device-side ordering, the host never blocks)."""
        stream = _stream_ptr(stream)
        self._check(self.L.fmd_release_outputs(self.h, C.c_void_p(stream)))

    # -- per-channel state snapshot / restore --
    def get_state(self, channel: int) -> bytes:
        n = self.L.fmd_state_size(self.h)
        buf = C.create_string_buffer(n)
        self._check(self.L.fmd_get_state(self.h, channel, buf, n))
        return buf.raw

    def set_state(self, channel: int, blob: bytes):
        self._check(self.L.fmd_set_state(self.h, channel, blob, len(blob)))

    # -- outputs --
    def audio(self) -> np.ndarray:
        out = np.empty((self.n_channels, self.rates.n_audio, 2), np.float32)
        self._check(self.L.fmd_get_audio(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def rds_symbols(self) -> tuple[np.ndarray, np.ndarray]:
        syms = np.empty((self.n_channels, self.rates.n_rds), np.float32)
        counts = np.empty(self.n_channels, np.int32)
        self._check(self.L.fmd_get_rds_symbols(self.h, syms.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)))
        return syms, counts

    def rds_bytes(self) -> tuple[np.ndarray, np.ndarray]:
        b = np.zeros((self.n_channels, self.bytes_cap), np.uint8)
        counts = np.empty(self.n_channels, np.int32)
        self._check(self.L.fmd_get_rds_bytes(self.h, b.ctypes.data_as(C.c_void_p), self.bytes_cap, counts.ctypes.data_as(C.c_void_p)))
        return b, counts

    def rds_db(self) -> np.ndarray:
        """App::GetRDSDatabase() per channel after the newest block (FMD_FLAG_RDS_DECODE): RDS_DB_DTYPE [C]."""
        out = np.zeros(self.n_channels, RDS_DB_DTYPE)
        self._check(self.L.fmd_get_rds_db(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def rds_groups_raw(self) -> tuple[np.ndarray, np.ndarray]:
        """(uint8 [C, groups_cap, 16] group records in the C layout, counts [C]) delivered in the newest block."""
        raw = np.zeros((self.n_channels, self.groups_cap, 16), np.uint8)
        counts = np.zeros(self.n_channels, np.int32)
        self._check(self.L.fmd_get_rds_groups(self.h, raw.ctypes.data_as(C.c_void_p), self.groups_cap, counts.ctypes.data_as(C.c_void_p)))
        return raw, counts

    def rds_groups(self) -> list:
        """Per channel the groups delivered in the newest block, RDS_GROUP_DTYPE [n]."""
        return _groups_lists(*self.rds_groups_raw())

    def reset_rds_db(self, channel: int = -1):
        """RDS_Database::Reset() (the database only; sync state and A/B memories stay)."""
        self._check(self.L.fmd_reset_rds_db(self.h, channel))

    def stream(self, name: str) -> np.ndarray:
        n = C.c_size_t(0)
        probe = np.empty(1, np.float32)
        self.L.fmd_get_stream(self.h, name.encode(), probe.ctypes.data_as(C.c_void_p), 0, C.byref(n))
        if n.value == 0:
            self._check(self.L.fmd_get_stream(self.h, name.encode(), probe.ctypes.data_as(C.c_void_p), 0, C.byref(n)))
        out = np.empty(n.value, np.float32)
        self._check(self.L.fmd_get_stream(self.h, name.encode(), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)))
        return out.reshape(self.n_channels, -1)

    def profile(self, on):
        """False/0: off; True/1: bracket every kernel of every block; 2: the dominant kernel every block, the rest every 4th;
        3: every kernel of every 4th block, plus the dominant kernel of the block behind it."""
        self._check(self.L.fmd_profile_enable(self.h, int(on)))

    def spec_stats(self, reset: bool = False) -> dict:
        """Speculation counters of the pilot PLL kernel (fmd_get_spec_stats) since creation / the last reset."""
        a = np.zeros(8, np.uint64)
        self._check(self.L.fmd_get_spec_stats(self.h, a.ctypes.data_as(C.c_void_p), 1 if reset else 0))
        out = {"pll": {"chunks": int(a[0]), "serial_chunks": int(a[1]), "exact_spans": int(a[2]), "spans": int(a[3]), "samples": int(a[4]),
                       "samples_per_span": float(a[4]) / float(a[3]) if a[3] else 0.0, "sequence_spans": int(a[5])}}
        if a[7]:
            out["pll_clock_mhz"] = float(a[6]) / float(a[7]) * 100.0
        return out

    def profile_read(self) -> dict:
        """{kernel name: (total ms, launches)} since the last read (HIP events on the processing stream)."""
        arr = (KernelTime * 16)()
        n = C.c_int(0)
        self._check(self.L.fmd_profile_read(self.h, arr, 16, C.byref(n)))
        return {arr[i].name.decode(): (arr[i].total_ms, arr[i].launches) for i in range(n.value)}

    def audio_pcm16_into(self, out, stream=None):
        """Convert the newest block's audio to the reference scraper's 16-bit PCM frames into `out` (torch int16 CUDA tensor
        [C, n_audio, 2]) on `stream` (default: torch current stream), ordered behind the block's outputs."""
        import torch
        stream = _stream_ptr(stream)
        assert out.dtype == torch.int16 and out.is_contiguous() and out.numel() == self.n_channels * self.rates.n_audio * 2
        self._check(self.L.fmd_audio_pcm16_dev(self.h, C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def audio_tensor(self):
        """Zero-copy torch view of the newest block's device audio buffer [C, n_audio, 2] (the library alternates
        between its pipeline slots: call again after each process(); contents are complete after wait_outputs/synchronize and stay
        valid while at most FMD_OUTPUT_LIFETIME_BLOCKS = 5 further blocks have been submitted — or longer for a consumer that
        calls release_outputs())."""
        import torch
        p = C.c_void_p()
        self._check(self.L.fmd_audio_dev(self.h, C.byref(p)))
        n = self.n_channels * self.rates.n_audio * 2

        class _Arr:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (p.value, False), "version": 2}
        return torch.as_tensor(_Arr(), device="cuda").view(self.n_channels, self.rates.n_audio, 2)

    def rds_db_tensor(self):
        """Zero-copy torch view of the newest block's databases: uint8 [C, 120] (fmd_rds_db_dev; RDS_DB_DTYPE after .cpu().numpy().view())."""
        import torch
        p = C.c_void_p()
        self._check(self.L.fmd_rds_db_dev(self.h, C.byref(p)))
        nC = self.n_channels

        class _D:
            __cuda_array_interface__ = {"shape": (nC * 120,), "typestr": "|u1", "data": (p.value, False), "version": 2}
        return torch.as_tensor(_D(), device="cuda").view(nC, 120)

    def rds_groups_tensors(self):
        """Zero-copy torch views of the newest block's groups: (records [C, cap, 16] uint8, counts [C] int32) — fmd_rds_groups_dev."""
        import torch
        pg, pc, cap = C.c_void_p(), C.c_void_p(), C.c_int(0)
        self._check(self.L.fmd_rds_groups_dev(self.h, C.byref(pg), C.byref(pc), C.byref(cap)))
        nC = self.n_channels

        class _G:
            __cuda_array_interface__ = {"shape": (nC * cap.value * 16,), "typestr": "|u1", "data": (pg.value, False), "version": 2}

        class _C:
            __cuda_array_interface__ = {"shape": (nC,), "typestr": "<i4", "data": (pc.value, False), "version": 2}
        return torch.as_tensor(_G(), device="cuda").view(nC, cap.value, 16), torch.as_tensor(_C(), device="cuda")

    def rds_bytes_tensors(self):
        """Zero-copy torch views of the newest block's RDS byte buffers: (bytes [C, cap] uint8, counts [C] int32) — fmd_rds_bytes_dev; same
        lifetime rule as audio_tensor()."""
        import torch
        pb, pc, cap = C.c_void_p(), C.c_void_p(), C.c_int(0)
        self._check(self.L.fmd_rds_bytes_dev(self.h, C.byref(pb), C.byref(pc), C.byref(cap)))
        nC = self.n_channels

        class _B:
            __cuda_array_interface__ = {"shape": (nC * cap.value,), "typestr": "|u1", "data": (pb.value, False), "version": 2}

        class _C:
            __cuda_array_interface__ = {"shape": (nC,), "typestr": "<i4", "data": (pc.value, False), "version": 2}
        return torch.as_tensor(_B(), device="cuda").view(nC, cap.value), torch.as_tensor(_C(), device="cuda")


def chan_design(fs_in: float, fs_out: float, taps_per_phase: int = 640):
    """Host-only prototype design of the wideband channeliser: (taps [T, L] float32, L, M).  Needs no GPU."""
    lib = load_library()
    L, M = C.c_int(0), C.c_int(0)
    rc = lib.fmd_chan_design(fs_in, fs_out, taps_per_phase, None, C.byref(L), C.byref(M))
    if rc != FMD_OK:
        raise FmdError(rc, "unsupported channeliser rates")
    taps = np.empty((taps_per_phase, L.value), np.float32)
    lib.fmd_chan_design(fs_in, fs_out, taps_per_phase, taps.ctypes.data_as(C.c_void_p), None, None)
    return taps, L.value, M.value


def chan_default_taps(fs_in: float, fs_out: float = 256_000.0) -> int:
    """The taps per phase Channelizer(..., taps_per_phase=0) uses for a rate pair (fmd_chan_default_taps_per_phase).  Needs no GPU."""
    t = load_library().fmd_chan_default_taps_per_phase(float(fs_in), float(fs_out))
    if t <= 0:
        raise FmdError(t, f"unsupported channeliser rates {fs_in} -> {fs_out}")
    return t


CHAN_FORMS = ("k_channelize", "k_channelize16", "k_channelize16_mfma", "k_channelize_band_mfma")     # by FMD_CHAN_FORM_*


class Channelizer(_Handle):
    """Wideband capture (cf32, u8, s8 or s16) -> [C][n_out] cf32 stations at fs_out on the GPU (fmd_chan_*); feeds BatchDemod.process directly.

    Accepts every pair of integer rates with fs_out / fs_in = L / M, L <= 64 and M / L <= 128 (fs_in up to 32.768 MSa/s at 256 kSa/s:
    the whole FM band in one capture), with 4 to 4096 taps per phase; taps_per_phase=0 takes chan_default_taps(fs_in, fs_out).  Kernels:
    10 MSa/s -> 256 kSa/s with 640 taps per phase on the matrix cores (k_channelize16_mfma); the whole-band pairs with L dividing 16
    (16, 20, 20.48, 24, 30.72, 32, 32.768 MSa/s) on the matrix cores too (k_channelize_band_mfma); every other pair on the vector ALUs.
    A station's output does not depend on its row or on the number of stations.  `form` names the kernel that serves the handle (one of
    CHAN_FORMS) and `tile_outputs` the outputs a workgroup of it takes per tile (fmd_chan_kernel_form)."""
    _prefix = "fmd_chan"

    def __init__(self, fs_in: float, center_hz, fs_out: float = 256_000.0, max_input_samples: int = 640_000, taps_per_phase: int = 0, device: int = -1):
        self.centers = np.ascontiguousarray(center_hz, np.float64)
        cfg = ChanConfig(fs_in, fs_out, int(self.centers.size), self.centers.ctypes.data_as(C.POINTER(C.c_double)), taps_per_phase, max_input_samples, device)
        self._create("create", C.byref(cfg))
        l, m, t, c = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self.L.fmd_chan_info(self.h, C.byref(l), C.byref(m), C.byref(t), C.byref(c))
        self.interp, self.decim, self.taps_per_phase, self.n_stations = l.value, m.value, t.value, c.value
        f, to = C.c_int(), C.c_int()
        self._check(self.L.fmd_chan_kernel_form(self.h, C.byref(f), C.byref(to)))
        # which kernel serves process() (CHAN_FORMS: fixed at create) and the consecutive outputs one of its workgroups takes per tile
        self.form, self.tile_outputs = CHAN_FORMS[f.value], to.value

    def taps(self) -> np.ndarray:
        a = np.empty((self.taps_per_phase, self.interp), np.float32)
        rc = self.L.fmd_chan_get_taps(self.h, a.ctypes.data_as(C.c_void_p), a.size)
        if rc != FMD_OK:
            raise FmdError(rc, "fmd_chan_get_taps")
        return a

    def process(self, wide, out=None, stream=None):
        """wide: contiguous CUDA tensor [n_in, 2] of interleaved I, Q: float32, or a receiver's uint8 (RTL-SDR: v - 127), int8 (HackRF) or
        int16 (Airspy, SDRplay, USRP sc16), read as is (no conversion pass); returns a CUDA float32 tensor [C, n_out, 2] (asynchronous on
        the stream).  An integer capture gives the bits the float32 call gives on its conversion; formats may change from call to call."""
        import torch
        fns = {torch.float32: self.L.fmd_chan_process_cf32_dev, torch.uint8: self.L.fmd_chan_process_u8_dev,
               torch.int8: self.L.fmd_chan_process_s8_dev, torch.int16: self.L.fmd_chan_process_s16_dev}
        if not (wide.is_cuda and wide.is_contiguous() and wide.dtype in fns and wide.dim() == 2 and wide.shape[1] == 2):
            raise ValueError("wide must be a contiguous CUDA tensor [n_in, 2] of float32, uint8, int8 or int16")
        n_in = int(wide.shape[0])
        n_out = n_in * self.interp // self.decim
        if out is None:
            out = torch.empty((self.n_stations, n_out, 2), dtype=torch.float32, device=wide.device)
        got = C.c_size_t(0)
        self._check(fns[wide.dtype](self.h, wide.data_ptr(), n_in, out.data_ptr(), int(out.shape[1]), C.byref(got),
                                    C.c_void_p(_stream_ptr(stream, wide.device))))
        return out[:, :got.value]

    def reset(self):
        self._check(self.L.fmd_chan_reset(self.h))


def scan_default_nfft(fs_in: float) -> int:
    """The FFT size BandScanner(fs_in, nfft=0) uses (fmd_scan_default_nfft): the smallest power of two with fs_in / N <= 5 kHz, clamped
    to 256 ... 16384.  Needs no GPU."""
    n = load_library().fmd_scan_default_nfft(float(fs_in))
    if n <= 0:
        raise FmdError(n, f"fs_in {fs_in} must be > 0")
    return n


def scan_default_params() -> dict:
    """The detection parameters fmd_scan_default_params gives, as a dict (the keyword arguments of scan_detect / BandScanner.stations)."""
    p = ScanParams()
    load_library().fmd_scan_default_params(C.byref(p))
    return {name: getattr(p, name) for name, _ in ScanParams._fields_}


def _scan_params(params: dict) -> ScanParams:
    p = ScanParams()
    load_library().fmd_scan_default_params(C.byref(p))
    for k, v in params.items():
        if k not in scan_default_params():
            raise TypeError(f"unknown detection parameter {k!r}")
        setattr(p, k, float(v))
    return p


def _stations(call, msg) -> np.ndarray:
    """run a detection call (out, cap, n_found) -> rc twice if needed: the count first, then every station"""
    n = C.c_int(0)
    out = np.zeros(64, SCAN_STATION_DTYPE)
    rc = call(out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
    if rc == FMD_OK and n.value > out.size:
        out = np.zeros(n.value, SCAN_STATION_DTYPE)
        rc = call(out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
    if rc != FMD_OK:
        raise FmdError(rc, msg())
    return out[:n.value].copy()


def scan_detect(psd, fs_in: float, **params) -> np.ndarray:
    """Host-only detection (fmd_scan_detect) on an fft-shifted PSD [nfft] (BandScanner.psd()'s layout): a structured array of stations
    (offset_hz, power_db, snr_db) ascending by offset.  params override fmd_scan_default_params (scan_default_params()).  Needs no GPU."""
    lib = load_library()
    a = np.ascontiguousarray(psd, np.float64)
    if a.ndim != 1:
        raise ValueError("psd must be one-dimensional")
    p = _scan_params(params)
    return _stations(lambda out, cap, n: lib.fmd_scan_detect(a.ctypes.data_as(C.c_void_p), int(a.size), float(fs_in), C.byref(p), out, cap, n),
                     lambda: lib.fmd_scan_last_error(None).decode())


class BandScanner(_Handle):
    """Finds the stations of a wideband capture (fmd_scan_*): an averaged periodogram on the GPU (Hann window, N = nfft, hop N / 2, fp64
    sums in frame order: bit-identical however the capture is split into calls), then detection on an FM raster on the host.
    stations()["offset_hz"] goes straight to Channelizer(fs_in, ...)."""
    _prefix = "fmd_scan"

    def __init__(self, fs_in: float, nfft: int = 0, max_input_samples: int = 2_097_152, device: int = -1):
        self.fs_in = float(fs_in)
        cfg = ScanConfig(self.fs_in, int(nfft), int(max_input_samples), int(device))
        self._create("create", C.byref(cfg))
        self.nfft = int(nfft) if nfft else scan_default_nfft(fs_in)

    def process(self, wide, stream=None) -> None:
        """wide: contiguous CUDA tensor [n_in, 2] of interleaved I, Q: float32, or a receiver's uint8 (v - 127), int8 or int16, read in place
        and asynchronously on the stream (the tensor belongs to the call until its work there has completed)."""
        import torch
        fns = {torch.float32: self.L.fmd_scan_process_cf32_dev, torch.uint8: self.L.fmd_scan_process_u8_dev,
               torch.int8: self.L.fmd_scan_process_s8_dev, torch.int16: self.L.fmd_scan_process_s16_dev}
        if not (wide.is_cuda and wide.is_contiguous() and wide.dtype in fns and wide.dim() == 2 and wide.shape[1] == 2):
            raise ValueError("wide must be a contiguous CUDA tensor [n_in, 2] of float32, uint8, int8 or int16")
        self._check(fns[wide.dtype](self.h, wide.data_ptr(), int(wide.shape[0]), C.c_void_p(_stream_ptr(stream, wide.device))))

    def psd(self) -> tuple[np.ndarray, np.ndarray]:
        """(freqs_hz, psd) float64 [nfft], low to high frequency: bin i at (i - nfft / 2) fs_in / nfft.  Synchronises with the scanner."""
        a = np.empty(self.nfft, np.float64)
        self._check(self.L.fmd_scan_get_psd(self.h, a.ctypes.data_as(C.c_void_p), a.size, None))
        return (np.arange(self.nfft, dtype=np.float64) - self.nfft // 2) * (self.fs_in / self.nfft), a

    @property
    def n_frames(self) -> int:
        a = np.empty(self.nfft, np.float64)
        n = C.c_longlong(0)
        self._check(self.L.fmd_scan_get_psd(self.h, a.ctypes.data_as(C.c_void_p), a.size, C.byref(n)))
        return n.value

    def stations(self, **params) -> np.ndarray:
        """Detection on the PSD so far: structured array (offset_hz, power_db, snr_db) ascending by offset; params as scan_detect."""
        p = _scan_params(params)
        return _stations(lambda out, cap, n: self.L.fmd_scan_stations(self.h, C.byref(p), out, cap, n),
                         lambda: self.L.fmd_scan_last_error(self.h).decode())

    def reset(self):
        self._check(self.L.fmd_scan_reset(self.h))


def iqcorr_solve(moments) -> IqCorrection:
    """Host-only solve step (fmd_iqcorr_solve): the six moments (IqMoments, or n, sum i, sum q, sum i^2, sum q^2, sum i q in that order)
    -> the correction that removes the DC term and the image, exactly the root of E[(z + w conj(z))^2] = 0.  Needs no GPU."""
    lib = load_library()
    m = _IqMomentsC(*(float(v) for v in moments))
    c = _IqCorrectionC()
    rc = lib.fmd_iqcorr_solve(C.byref(m), C.byref(c))
    if rc != FMD_OK:
        raise _global_error(lib, "fmd_iqcorr", rc)
    return IqCorrection(c.dc_i, c.dc_q, c.w_re, c.w_im)


class IqCorrector(_Handle):
    """Removes a receiver's DC offset and IQ imbalance from a wideband capture on the GPU (fmd_iqcorr_*), ahead of BandScanner and
    Channelizer.  process() adds every raw sample to fp64 moments (a fixed summation order: bit-identical however the capture is split into
    calls) and returns the samples as float32, corrected with the correction in force: identity until calibrate() or `correction` sets one."""

    _prefix = "fmd_iqcorr"
    solve = staticmethod(iqcorr_solve)

    def __init__(self, max_input_samples: int = 2_097_152, device: int = -1):
        cfg = IqcorrConfig(int(max_input_samples), int(device))
        self._create("create", C.byref(cfg))
        self.max_input_samples = int(max_input_samples)

    def process(self, wide, out=None, stream=None):
        """wide: contiguous CUDA tensor [n_in, 2] of interleaved I, Q: float32, or a receiver's uint8 (v - 127), int8 or int16.  Returns the
        corrected samples, a CUDA float32 tensor [n_in, 2] (asynchronous on the stream).  out: the tensor to write (`wide` itself is allowed
        for float32), or False to measure only (returns None)."""
        import torch
        fns = {torch.float32: self.L.fmd_iqcorr_process_cf32_dev, torch.uint8: self.L.fmd_iqcorr_process_u8_dev,
               torch.int8: self.L.fmd_iqcorr_process_s8_dev, torch.int16: self.L.fmd_iqcorr_process_s16_dev}
        if not (wide.is_cuda and wide.is_contiguous() and wide.dtype in fns and wide.dim() == 2 and wide.shape[1] == 2):
            raise ValueError("wide must be a contiguous CUDA tensor [n_in, 2] of float32, uint8, int8 or int16")
        n_in = int(wide.shape[0])
        if out is None:
            out = torch.empty((n_in, 2), dtype=torch.float32, device=wide.device)
        if out is not False and not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (n_in, 2)):
            raise ValueError("out must be a contiguous CUDA float32 tensor [n_in, 2]")
        self._check(fns[wide.dtype](self.h, C.c_void_p(wide.data_ptr()), n_in, None if out is False else C.c_void_p(out.data_ptr()),
                                    C.c_void_p(_stream_ptr(stream, wide.device))))
        return None if out is False else out

    def measure(self, wide, stream=None) -> None:
        """process(wide, out=False): adds the samples to the moments and writes nothing"""
        self.process(wide, out=False, stream=stream)

    def moments(self) -> IqMoments:
        """the moments of every sample since create / reset; synchronises with the corrector's work"""
        m = _IqMomentsC()
        self._check(self.L.fmd_iqcorr_get_moments(self.h, C.byref(m)))
        return IqMoments(m.n, m.sum_i, m.sum_q, m.sum_ii, m.sum_qq, m.sum_iq)

    def calibrate(self) -> IqCorrection:
        """moments() -> solve() -> correction: applies from the next process call; the moments are kept"""
        c = _IqCorrectionC()
        self._check(self.L.fmd_iqcorr_calibrate(self.h, C.byref(c)))
        return IqCorrection(c.dc_i, c.dc_q, c.w_re, c.w_im)

    @property
    def correction(self) -> IqCorrection:
        c = _IqCorrectionC()
        self._check(self.L.fmd_iqcorr_get_correction(self.h, C.byref(c)))
        return IqCorrection(c.dc_i, c.dc_q, c.w_re, c.w_im)

    @correction.setter
    def correction(self, value):
        c = _IqCorrectionC(*(float(v) for v in value))
        self._check(self.L.fmd_iqcorr_set_correction(self.h, C.byref(c)))

    def reset(self):
        """moments to zero and the correction to identity"""
        self._check(self.L.fmd_iqcorr_reset(self.h))

    def reset_moments(self):
        self._check(self.L.fmd_iqcorr_reset_moments(self.h))


def resampler_design(fs_in: int, fs_out: int, taps_per_phase: int = 0):
    """Host-only polyphase design of the audio resampler: (taps [T, L] float32 with taps[t, p] = h[p + t L], L, M).  Needs no GPU."""
    lib = load_library()
    L, M = C.c_int(0), C.c_int(0)
    rc = lib.fmd_resampler_design(int(fs_in), int(fs_out), int(taps_per_phase), None, C.byref(L), C.byref(M))
    if rc != FMD_OK:
        raise FmdError(rc, f"unsupported resampler rates {fs_in} -> {fs_out} ({taps_per_phase} taps per phase)")
    T = taps_per_phase if taps_per_phase > 0 else 32 * -(-M.value // L.value)    # include/fmdemod.h: the default grows with M / L
    taps = np.empty((T, L.value), np.float32)
    lib.fmd_resampler_design(int(fs_in), int(fs_out), int(taps_per_phase), taps.ctypes.data_as(C.c_void_p), None, None)
    return taps, L.value, M.value


class AudioResampler(_Handle):
    """C stations' stereo audio from fs_in to fs_out on the GPU (fmd_resampler_*): the reference's Resampled_PCM_Player for a batch.
    method "reference" is its block-local linear interpolation, bit-identical; "polyphase" streams through an anti-aliasing filter.
    Feed it BatchDemod.audio_tensor() (or any [C, n, 2] float32 CUDA tensor whose frames are contiguous)."""

    _prefix, _attr = "fmd_resampler", "r"
    design = staticmethod(resampler_design)

    def __init__(self, n_channels: int, fs_out: int, fs_in: int = 32000, method: str = "polyphase", taps_per_phase: int = 0,
                 max_input_frames: int = 1 << 16, device: int = -1):
        m = {"reference": FMD_RESAMPLE_REFERENCE, "polyphase": FMD_RESAMPLE_POLYPHASE}[method]
        cfg = ResamplerConfig(n_channels, int(fs_in), int(fs_out), m, int(taps_per_phase), int(max_input_frames), device)
        self._create("create", C.byref(cfg))
        self.n_channels, self.fs_in, self.fs_out, self.method = n_channels, int(fs_in), int(fs_out), method

    def output_frames(self, n_in: int) -> int:
        """frames per channel the next call with n_in input frames emits"""
        n = C.c_longlong(0)
        self._check(self.L.fmd_resampler_output_frames(self.r, int(n_in), C.byref(n)))
        return n.value

    def reset(self, channel: int = -1):
        self._check(self.L.fmd_resampler_reset(self.r, int(channel)))

    def set_input_rate(self, fs_in: int) -> bool:
        """SetInputSampleRate: True if the rate changed"""
        changed = self._check(self.L.fmd_resampler_set_input_rate(self.r, int(fs_in))) == 1
        self.fs_in = int(fs_in)
        return changed

    def _run(self, fn, x, n_in, dtype, out, stream):
        import torch
        px, in_stride, n_in = _batch_input(x, self.n_channels, n_in, ("float32",), "frames")
        want = self.output_frames(n_in)
        if out is None:
            out = torch.empty((self.n_channels, max(want, 1), 2), dtype=dtype, device=x.device)
        assert out.dtype == dtype and out.dim() == 3 and out.stride(2) == 1 and out.stride(1) == 2 and out.shape[1] >= want
        got = C.c_longlong(0)
        out_stride = out.stride(0) // 2 if out.shape[0] > 1 else out.shape[1]
        self._check(fn(self.r, px, in_stride, n_in, C.c_void_p(out.data_ptr()), out_stride, C.byref(got), C.c_void_p(_stream_ptr(stream, x.device))))
        return out[:, :got.value]

    def process(self, x, n_in: int | None = None, out=None, stream=None):
        """x: [C, n, 2] float32 on the device (the first n_in frames are read, default all).  Returns [C, n_out, 2] float32, asynchronous on
        `stream` (default: torch's current stream)."""
        import torch
        return self._run(self.L.fmd_resampler_process_f32_dev, x, n_in, torch.float32, out, stream)

    def process_pcm16(self, x, n_in: int | None = None, out=None, stream=None):
        """The same as the scraper's 16-bit PCM frames: [C, n_out, 2] int16."""
        import torch
        return self._run(self.L.fmd_resampler_process_pcm16_dev, x, n_in, torch.int16, out, stream)

    def process_host(self, x, out: np.ndarray, n_in: int | None = None, stream=None) -> int:
        """process() into a host array (fmd_resampler_process_f32_host): out [C, out_stride, 2] float32, C-contiguous; the first n_out frames
        of every row are written, nothing behind them.  Synchronises `stream`; returns n_out."""
        px, in_stride, n_in = _batch_input(x, self.n_channels, n_in, ("float32",), "frames")
        if not (out.dtype == np.float32 and out.ndim == 3 and out.shape[0] == self.n_channels and out.shape[2] == 2 and out.flags.c_contiguous):
            raise ValueError("out must be a C-contiguous float32 array [C, out_stride, 2]")
        got = C.c_longlong(0)
        self._check(self.L.fmd_resampler_process_f32_host(self.r, px, in_stride, n_in, out.ctypes.data_as(C.c_void_p), int(out.shape[1]), C.byref(got),
                                                          C.c_void_p(_stream_ptr(stream, x.device))))
        return got.value


class AudioMixer(_Handle):
    """B output buses on the GPU (fmd_mixer_*), each one reference AudioMixer: bus b plays
    clamp(sum over its delivering sources, in order, of fmaf(x, gain_b / log10f(10 k), acc)), bit-identical to the reference's build.
    buses: a list of B lists of station rows in registration (CreateManagedBuffer) order; a row may appear in many buses.
    Feed it the same [C, n, 2] float32 CUDA tensors as AudioResampler (BatchDemod.audio_tensor() or a resampler's output)."""
    _prefix, _attr = "fmd_mixer", "m"

    def __init__(self, n_channels: int, buses, gains=None, device: int = -1):
        buses = [list(map(int, b)) for b in buses]
        offs = np.zeros(len(buses) + 1, np.int32)
        offs[1:] = np.cumsum([len(b) for b in buses])
        src = np.array([r for b in buses for r in b] or [0], np.int32)
        g = None if gains is None else np.ascontiguousarray(gains, np.float32)
        if g is not None and g.shape != (len(buses),):
            raise ValueError("gains must hold one value per bus")
        cfg = MixerConfig(int(n_channels), len(buses), offs.ctypes.data, src.ctypes.data, None if g is None else g.ctypes.data, device)
        self._create("create", C.byref(cfg))
        self.n_channels, self.n_buses = int(n_channels), len(buses)

    def set_sources(self, bus: int, sources):
        """replace a bus's sources (registration order); applies from the next process call"""
        rows = [int(r) for r in sources]
        src = np.array(rows or [0], np.int32)
        self._check(self.L.fmd_mixer_set_sources(self.m, int(bus), src.ctypes.data_as(C.c_void_p), len(rows)))

    def set_gain(self, bus: int, g: float):
        """AudioMixer::GetOutputGain() = g for one bus (-1: every bus); applies from the next process call"""
        self._check(self.L.fmd_mixer_set_gain(self.m, int(bus), C.c_float(g)))

    def gain(self, bus: int) -> float:
        g = C.c_float(0.0)
        self._check(self.L.fmd_mixer_get_gain(self.m, int(bus), C.byref(g)))
        return g.value

    def process(self, x, n: int | None = None, active=None, out=None, stream=None):
        """AudioMixer::UpdateMixer for every bus.  x: [C, >= n, 2] float32 on the device, contiguous frames (the first n frames are
        read, default all); active: None (every station delivered) or a [C] uint8 / bool CUDA tensor; out: [B, >= n, 2] float32.
        Returns [B, n, 2] float32, asynchronous on `stream` (default: torch's current stream)."""
        import torch
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32",), "frames")
        if out is None:
            out = torch.empty((self.n_buses, max(n, 1), 2), dtype=torch.float32, device=x.device)
        if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 3 and out.shape[0] == self.n_buses and out.stride(2) == 1
                and out.stride(1) == 2):
            raise ValueError("out must be a CUDA float32 tensor [B, n, 2] with contiguous frames")
        out_stride = out.stride(0) // 2 if out.shape[0] > 1 else out.shape[1]
        self._check(self.L.fmd_mixer_process_f32_dev(self.m, px, in_stride, n, _active_ptr(active, self.n_channels), C.c_void_p(out.data_ptr()),
                                                     out_stride, C.c_void_p(_stream_ptr(stream, x.device))))
        return out[:, :n]


def meter_design(fs: int) -> MeterDesign:
    """fmd_meter_design (host only, no GPU needed): the K-weighting biquads, the sub-block length and the histogram's edges and centres"""
    L = load_library()
    d = MeterDesign()
    rc = L.fmd_meter_design(int(fs), C.byref(d))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_meter", rc)
    return d


def meter_lufs(energy: float) -> float:
    """fmd_meter_lufs: -0.691 + 10 log10(energy); -inf for 0"""
    return load_library().fmd_meter_lufs(float(energy))


def meter_integrated(hist, design: MeterDesign) -> float:
    """fmd_meter_integrated (host only): the gated programme loudness, in LUFS, of one station's [1000] histogram; -inf when it is empty"""
    L = load_library()
    h = np.ascontiguousarray(hist, np.uint32)
    if h.shape != (METER_BINS,):
        raise ValueError("hist must hold 1000 bins")
    out = C.c_double(0.0)
    rc = L.fmd_meter_integrated(h.ctypes.data_as(C.c_void_p), C.byref(design), C.byref(out))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_meter", rc)
    return out.value


def meter_momentary(record) -> float:
    """fmd_meter_momentary of one METER_STATUS_DTYPE record: the last 400 ms, in LUFS (FMD_ERR_STATE before 4 sub-blocks)"""
    return _record_read("fmd_meter", "momentary", record, METER_STATUS_DTYPE)


def meter_short_term(record) -> float:
    """fmd_meter_short_term of one METER_STATUS_DTYPE record: the last 3 s, in LUFS (FMD_ERR_STATE before 30 sub-blocks)"""
    return _record_read("fmd_meter", "short_term", record, METER_STATUS_DTYPE)


def meter_tp_design(fs: int) -> MeterTpDesign:
    """fmd_meter_tp_design (host only): the true-peak interpolator's oversampling factor L and its (L - 1) x 12 float taps"""
    L = load_library()
    d = MeterTpDesign()
    rc = L.fmd_meter_tp_design(int(fs), C.byref(d))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_meter", rc)
    return d


def meter_dbtp(x):
    """fmd_meter_dbtp: 20 log10 of a float32 peak, in dBTP (dBFS for a sample peak); -inf for 0.  Scalars or arrays"""
    L = load_library()
    a = np.asarray(x, np.float32)
    out = np.array([L.fmd_meter_dbtp(C.c_float(float(v))) for v in a.reshape(-1)], np.float64).reshape(a.shape)
    return float(out) if out.ndim == 0 else out


def meter_range(hist, design: MeterDesign):
    """fmd_meter_range (host only): (lra in LU, low, high in LUFS) of one station's [1000] range histogram.  FmdError with status
    FMD_ERR_STATE when no bin survives the gates"""
    L = load_library()
    h = np.ascontiguousarray(hist, np.uint32)
    if h.shape != (METER_BINS,):
        raise ValueError("hist must hold 1000 bins")
    lra, low, high = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    rc = L.fmd_meter_range(h.ctypes.data_as(C.c_void_p), C.byref(design), C.byref(lra), C.byref(low), C.byref(high))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_meter", rc)
    return lra.value, low.value, high.value


class LoudnessMeter(_Monitor):
    """ITU-R BS.1770 loudness and sample peak of C stations' audio on the GPU (fmd_meter_*).  Feed it the same [C, n, 2] float32 CUDA
    tensors as AudioResampler and AudioMixer (BatchDemod.audio_tensor() at 32 kHz, or a resampler's output at fs); it changes nothing in
    them.  status() returns METER_STATUS_DTYPE records, histogram() the gating blocks' [C, 1000] counts; momentary / short_term /
    integrated turn them into LUFS on the host.  features = METER_TRUE_PEAK | METER_RANGE adds the maximum true-peak level
    (r128_status(), true_peak_dbtp()) and the loudness range (range_histogram(), loudness_range())."""
    _prefix, _attr, _status_dtype = "fmd_meter", "m", METER_STATUS_DTYPE

    def __init__(self, n_channels: int, fs: int, max_input_frames: int = 1 << 16, device: int = -1, features: int = 0):
        cfg = MeterConfig(int(n_channels), int(fs), int(max_input_frames), device)
        self._create("create_ex", C.byref(cfg), int(features))
        self.n_channels, self.fs, self.features = int(n_channels), int(fs), int(features)
        self.design = meter_design(fs)

    def process(self, x, n: int | None = None, active=None, stream=None):
        """meters the first n frames (default all) of x: [C, >= n, 2] float32 on the device, contiguous frames; active: None or a [C]
        uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole).  Asynchronous on `stream` (default: torch's current)."""
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32",), "frames")
        self._check(self.L.fmd_meter_process_f32_dev(self.m, px, in_stride, n, _active_ptr(active, self.n_channels),
                                                     C.c_void_p(_stream_ptr(stream, x.device))))

    def histogram(self) -> np.ndarray:
        """[C, 1000] uint32 counts of gating blocks per 0.1 LU bin from -70 LUFS; waits for the meter's work"""
        out = np.zeros((self.n_channels, METER_BINS), np.uint32)
        self._check(self.L.fmd_meter_get_histogram(self.m, out.ctypes.data_as(C.c_void_p)))
        return out

    def integrated(self, hist=None) -> np.ndarray:
        """[C] float64 LUFS: the gated programme loudness since reset (-inf where no gating block passed -70 LUFS)"""
        hist = self.histogram() if hist is None else hist
        return np.array([meter_integrated(h, self.design) for h in hist], np.float64)

    def r128_status(self) -> np.ndarray:
        """[C] METER_R128_DTYPE records (true peaks, the short-term values' counters); waits for the meter's work.  FMD_ERR_STATE on a
        meter without features"""
        out = np.zeros(self.n_channels, METER_R128_DTYPE)
        self._check(self.L.fmd_meter_get_r128_status(self.m, out.ctypes.data_as(C.c_void_p)))
        return out

    def r128_status_dev_ptr(self) -> int:
        """fmd_meter_r128_status_dev: the address of the device's own [C] records, valid until the next process call"""
        p = C.c_void_p()
        self._check(self.L.fmd_meter_r128_status_dev(self.m, C.byref(p)))
        return p.value

    def range_histogram(self) -> np.ndarray:
        """[C, 1000] uint32 counts of short-term values (one per 100 ms) per 0.1 LU bin from -70 LUFS; needs METER_RANGE"""
        out = np.zeros((self.n_channels, METER_BINS), np.uint32)
        self._check(self.L.fmd_meter_get_range_histogram(self.m, out.ctypes.data_as(C.c_void_p)))
        return out

    def loudness_range(self, hist=None):
        """(lra, low, high): three [C] float64 arrays, the loudness range in LU and its 10th / 95th percentiles in LUFS; NaN where no
        short-term value survives the gates yet"""
        hist = self.range_histogram() if hist is None else hist
        out = np.full((3, len(hist)), np.nan, np.float64)
        for c, h in enumerate(hist):
            try:
                out[:, c] = meter_range(h, self.design)
            except FmdError as e:
                if e.status != FMD_ERR_STATE:
                    raise
        return out[0], out[1], out[2]

    def true_peak_dbtp(self) -> np.ndarray:
        """[C, 2] float64: the held maximum true-peak level of L and R in dBTP (-inf for silence); needs METER_TRUE_PEAK"""
        if not self.features & METER_TRUE_PEAK:
            raise FmdError(FMD_ERR_STATE, "the meter was created without METER_TRUE_PEAK")
        return meter_dbtp(self.r128_status()["tp_hold"])


def modmon_design(fs: int) -> ModmonDesign:
    """fmd_modmon_design (host only, no GPU needed): the interval length M, the MPX low-pass's 33 taps, the pilot table and its gain,
    and the histogram's edges"""
    L = load_library()
    d = ModmonDesign()
    rc = L.fmd_modmon_design(int(fs), C.byref(d))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_modmon", rc)
    return d


def modmon_deviation_hz(record, design: ModmonDesign) -> float:
    """fmd_modmon_deviation_hz of one MODMON_STATUS_DTYPE record: half the peak-to-peak swing of the newest 50 ms interval, in Hz
    (FMD_ERR_STATE before the first interval)"""
    return _record_read("fmd_modmon", "deviation_hz", record, MODMON_STATUS_DTYPE, C.byref(design))


def modmon_offset_hz(record, design: ModmonDesign) -> float:
    """fmd_modmon_offset_hz: the carrier's frequency offset over the newest interval, in Hz"""
    return _record_read("fmd_modmon", "offset_hz", record, MODMON_STATUS_DTYPE, C.byref(design))


def modmon_pilot_hz(record, design: ModmonDesign) -> float:
    """fmd_modmon_pilot_hz: the 19 kHz pilot's deviation over the newest interval, in Hz"""
    return _record_read("fmd_modmon", "pilot_hz", record, MODMON_STATUS_DTYPE, C.byref(design))


def modmon_mpx_power_dbr(record, design: ModmonDesign, window_s: int = 60) -> float:
    """fmd_modmon_mpx_power_dbr: ITU-R BS.412 multiplex power over the newest window_s completed seconds, in dBr (FMD_ERR_STATE while
    fewer are complete)"""
    return _record_read("fmd_modmon", "mpx_power_dbr", record, MODMON_STATUS_DTYPE, C.byref(design), int(window_s))


def _modmon_hist(hist):
    h = np.ascontiguousarray(hist, np.uint32)
    if h.shape != (MODMON_BINS,):
        raise ValueError("hist must hold 300 bins")
    return h


def modmon_exceedance(hist, over: int, limit_hz: int = 75000):
    """fmd_modmon_exceedance (host only): (fraction, count) of one station's 50 ms intervals whose peak deviation is at least limit_hz
    (a multiple of 500 up to 150000)"""
    L = load_library()
    h = _modmon_hist(hist)
    frac, cnt = C.c_double(0.0), C.c_ulonglong(0)
    rc = L.fmd_modmon_exceedance(h.ctypes.data_as(C.c_void_p), int(over), int(limit_hz), C.byref(frac), C.byref(cnt))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_modmon", rc)
    return frac.value, cnt.value


def modmon_percentile(hist, over: int, q: float) -> float:
    """fmd_modmon_percentile (host only): the q-quantile (0 ... 1) of one station's interval peaks, as its 500 Hz bin's centre in Hz"""
    L = load_library()
    h = _modmon_hist(hist)
    out = C.c_double(0.0)
    rc = L.fmd_modmon_percentile(h.ctypes.data_as(C.c_void_p), int(over), float(q), C.byref(out))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_modmon", rc)
    return out.value


class ModulationMonitor(_Monitor):
    """Peak deviation (ITU-R SM.1268), multiplex power (ITU-R BS.412), carrier offset and pilot deviation of C stations' baseband on the
    GPU (fmd_modmon_*).  Feed it the [C, n, 2] float32 or uint8 CUDA tensors the demodulator takes (a channeliser's output); it changes
    nothing in them.  status() returns MODMON_STATUS_DTYPE records, histogram() the interval peaks' [C, 300] counts; the modmon_*
    functions turn them into Hz and dBr on the host."""
    _prefix, _attr, _status_dtype = "fmd_modmon", "m", MODMON_STATUS_DTYPE

    def __init__(self, n_channels: int, fs: int, max_input_samples: int = 1 << 20, device: int = -1):
        cfg = ModmonConfig(int(n_channels), int(fs), int(max_input_samples), device)
        self._create("create", C.byref(cfg))
        self.n_channels, self.fs = int(n_channels), int(fs)
        self.design = modmon_design(fs)

    def process(self, x, n: int | None = None, active=None, stream=None):
        """monitors the first n samples (default all) of x: [C, >= n, 2] float32 or uint8 on the device, contiguous samples; active: None
        or a [C] uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole).  Asynchronous on `stream` (default: torch's
        current)."""
        import torch
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32", "uint8"), "samples")
        fn = self.L.fmd_modmon_process_cf32_dev if x.dtype == torch.float32 else self.L.fmd_modmon_process_u8_dev
        self._check(fn(self.m, px, in_stride, n, _active_ptr(active, self.n_channels), C.c_void_p(_stream_ptr(stream, x.device))))

    def histogram(self) -> np.ndarray:
        """[C, 300] uint32 counts of 50 ms intervals per 500 Hz bin of peak deviation; waits for the monitor's work"""
        out = np.zeros((self.n_channels, MODMON_BINS), np.uint32)
        self._check(self.L.fmd_modmon_get_histogram(self.m, out.ctypes.data_as(C.c_void_p)))
        return out


def squelch_default_params() -> SquelchParams:
    """fmd_squelch_default_params: 10 dB to open, 7 dB to stay open, no level floor, 2 intervals to open, 10 to close, FMD_SQUELCH_AUTO"""
    p = SquelchParams()
    load_library().fmd_squelch_default_params(C.byref(p))
    return p


def squelch_threshold(db: float) -> float:
    """fmd_squelch_threshold (host only): (k k) / ((1 + k) (1 + k)), k = 10^(db / 10) -- what the gate compares (2 S2^2 - M S4) / S2^2 with"""
    return load_library().fmd_squelch_threshold(float(db))


def squelch_level_db(record, fs: int) -> float:
    """fmd_squelch_level_db of one SQUELCH_STATUS_DTYPE record: the newest interval's mean power in dB of the input's own units
    (FMD_ERR_STATE before the first interval)"""
    return _record_read("fmd_squelch", "level_db", record, SQUELCH_STATUS_DTYPE, int(fs))


def squelch_cnr_db(record, fs: int, window: int = 1) -> float:
    """fmd_squelch_cnr_db: the envelope-constancy carrier-to-noise ratio over the newest `window` (1 ... 20) intervals in dB, -inf where no
    carrier shows and +inf where no noise does (FMD_ERR_STATE while fewer intervals are complete)"""
    return _record_read("fmd_squelch", "cnr_db", record, SQUELCH_STATUS_DTYPE, int(fs), int(window))


def squelch_powers(record, fs: int, window: int = 1):
    """fmd_squelch_powers: (carrier, noise) power per sample over the newest `window` intervals, in the input's own units squared"""
    return _record_read("fmd_squelch", "powers", record, SQUELCH_STATUS_DTYPE, int(fs), int(window), outs=2)


class Squelch(_Gated):
    """Carrier squelch of C stations' baseband on the GPU (fmd_squelch_*): per station and 50 ms interval the power moments behind an
    envelope-constancy CNR, a hysteresis gate, and the [C] uint8 mask that AudioMixer.process(active=...), LoudnessMeter.process and
    ModulationMonitor.process take as it is.  Feed it the [C, n, 2] float32 or uint8 CUDA tensors the demodulator takes (a channeliser's
    output); it changes nothing in them.  status() returns SQUELCH_STATUS_DTYPE records; the squelch_* functions turn them into dB."""
    _prefix, _attr, _status_dtype, _params_type = "fmd_squelch", "q", SQUELCH_STATUS_DTYPE, SquelchParams

    def __init__(self, n_channels: int, fs: int, max_input_samples: int = 1 << 20, device: int = -1):
        cfg = SquelchConfig(int(n_channels), int(fs), int(max_input_samples), device)
        self._create("create", C.byref(cfg))
        self.n_channels, self.fs = int(n_channels), int(fs)

    def process(self, x, n: int | None = None, active=None, mask=None, stream=None):
        """takes the first n samples (default all) of x: [C, >= n, 2] float32 or uint8 on the device, contiguous samples; active: None or a
        [C] uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole and keeps its mask byte); mask: the [C] uint8 CUDA tensor
        to write, None = a new one.  Returns the mask tensor.  Asynchronous on `stream` (default: torch's current)."""
        import torch
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32", "uint8"), "samples")
        pa, stream = _active_ptr(active, self.n_channels), _stream_ptr(stream, x.device)
        mask, pm = _byte_out(mask, "mask", self.n_channels, x.device, stream)
        fn = self.L.fmd_squelch_process_cf32_dev if x.dtype == torch.float32 else self.L.fmd_squelch_process_u8_dev
        self._check(fn(self.q, px, in_stride, n, pa, pm, C.c_void_p(stream)))
        return mask


def audmon_default_params() -> AudmonParams:
    """fmd_audmon_default_params: silence at -60 dB, a rail lost 30 dB down, antiphase below a correlation of -0.5, mono with side 40 dB
    under mid; 100, 100, 100, 50, 100 intervals to raise and 10 to clear; alarm_mask 15 (MONO is an indication, not an alarm)"""
    p = AudmonParams()
    load_library().fmd_audmon_default_params(C.byref(p))
    return p


def audmon_level_db(record, fs: int, rail: int = 2, window: int = 1) -> float:
    """fmd_audmon_level_db of one AUDMON_STATUS_DTYPE record: the mean power of rail 0 (L), 1 (R) or 2 (both) over the newest `window`
    (1 ... 30) intervals in dB of full scale 1.0, -inf for silence (FMD_ERR_STATE while fewer intervals are complete)"""
    return _record_read("fmd_audmon", "level_db", record, AUDMON_STATUS_DTYPE, int(fs), int(rail), int(window))


def audmon_balance_db(record, fs: int, window: int = 1) -> float:
    """fmd_audmon_balance_db: L over R in dB (NaN for 0 / 0)"""
    return _record_read("fmd_audmon", "balance_db", record, AUDMON_STATUS_DTYPE, int(fs), int(window))


def audmon_correlation(record, fs: int, window: int = 1) -> float:
    """fmd_audmon_correlation: sum L R / sqrt(sum L^2 sum R^2), -1 ... 1 (NaN for 0 / 0)"""
    return _record_read("fmd_audmon", "correlation", record, AUDMON_STATUS_DTYPE, int(fs), int(window))


def audmon_side_mid_db(record, fs: int, window: int = 1) -> float:
    """fmd_audmon_side_mid_db: sum (L - R)^2 over sum (L + R)^2 in dB, -inf for R == L (NaN for 0 / 0)"""
    return _record_read("fmd_audmon", "side_mid_db", record, AUDMON_STATUS_DTYPE, int(fs), int(window))


class AudioMonitor(_Gated):
    """Audio fault monitor of C stations' audio on the GPU (fmd_audmon_*): per station and 100 ms interval the sums of L^2, R^2 and L R
    and the rail peaks, five hysteresis detectors (AUDMON_SILENCE, _LEFT_LOST, _RIGHT_LOST, _ANTIPHASE, _MONO), and two [C] uint8 tensors:
    the flags and the ok bytes, which AudioMixer.process(active=...) and LoudnessMeter.process take as they are.  Feed it the same
    [C, n, 2] float32 CUDA tensors as AudioResampler, AudioMixer and LoudnessMeter (BatchDemod.audio_tensor() at 32 kHz, or a resampler's
    output at fs); it changes nothing in them.  status() returns AUDMON_STATUS_DTYPE records; the audmon_* functions turn them into dB."""
    _prefix, _attr, _status_dtype, _params_type = "fmd_audmon", "a", AUDMON_STATUS_DTYPE, AudmonParams

    def __init__(self, n_channels: int, fs: int, max_input_frames: int = 1 << 16, device: int = -1):
        cfg = AudmonConfig(int(n_channels), int(fs), int(max_input_frames), device)
        self._create("create", C.byref(cfg))
        self.n_channels, self.fs = int(n_channels), int(fs)

    def process(self, x, n: int | None = None, active=None, flags=None, ok=None, stream=None):
        """takes the first n frames (default all) of x: [C, >= n, 2] float32 on the device, contiguous frames; active: None or a [C]
        uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole and keeps its two bytes); flags, ok: the [C] uint8 CUDA
        tensors to write, None = a new one, False = not written.  Returns (flags, ok), None for one not written.  Asynchronous on
        `stream` (default: torch's current)."""
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32",), "frames")
        pa, stream = _active_ptr(active, self.n_channels), _stream_ptr(stream, x.device)
        flags, pf = _byte_out(flags, "flags", self.n_channels, x.device, stream)
        ok, po = _byte_out(ok, "ok", self.n_channels, x.device, stream)
        self._check(self.L.fmd_audmon_process_f32_dev(self.a, px, in_stride, n, pa, pf, po, C.c_void_p(stream)))
        return flags, ok

    def _field(self, name: str, value):
        """raise_intervals and clear_intervals take five values or one for all five"""
        if name in ("raise_intervals", "clear_intervals"):
            return (C.c_int * 5)(*([int(value)] * 5 if np.isscalar(value) else [int(a) for a in value]))
        return value


def tonedet_default_params() -> TonedetParams:
    """fmd_tonedet_default_params: slots at 1000, 440, 400, 853, 960 and 1050 Hz and two unused; a tone present within 3 dB of the mid
    signal's power (6 dB for the EAS pair, which shares it); a floor of -50 dB; 20 intervals to raise and 5 to clear; alarm_mask 0 (a tone
    is an indication until the user makes it an alarm)"""
    p = TonedetParams()
    load_library().fmd_tonedet_default_params(C.byref(p))
    return p


def tonedet_share_db(record, fs: int, slot: int, window: int = 1) -> float:
    """fmd_tonedet_share_db of one TONEDET_STATUS_DTYPE record: the power of slot `slot`'s tone over the mid signal's power over the newest
    `window` (1 ... 30) intervals in dB, 0 for a pure sine at the slot's frequency (FMD_ERR_STATE while fewer intervals are complete)"""
    return _record_read("fmd_tonedet", "share_db", record, TONEDET_STATUS_DTYPE, int(fs), int(slot), int(window))


def tonedet_level_db(record, fs: int, slot: int, window: int = 1) -> float:
    """fmd_tonedet_level_db: the mean square of the slot's tone in the mid signal L + R, in dB of full scale 1.0"""
    return _record_read("fmd_tonedet", "level_db", record, TONEDET_STATUS_DTYPE, int(fs), int(slot), int(window))


class ToneDetector(_Gated):
    """Tone detector of C stations' audio on the GPU (fmd_tonedet_*): per station and 100 ms interval the power of the mid signal L + R at
    up to eight integer frequencies (a Goertzel bank) against its total power, one hysteresis detector per slot, and two [C] uint8
    tensors: the flags (bit k: slot k's tone is present) and the ok bytes, which AudioMixer.process(active=...) takes as they are.  Feed
    it the same [C, n, 2] float32 CUDA tensors as AudioMixer, LoudnessMeter and AudioMonitor; it changes nothing in them.  status()
    returns TONEDET_STATUS_DTYPE records; tonedet_share_db and tonedet_level_db turn them into dB."""
    _prefix, _attr, _status_dtype, _params_type = "fmd_tonedet", "t", TONEDET_STATUS_DTYPE, TonedetParams

    def __init__(self, n_channels: int, fs: int, max_input_frames: int = 1 << 16, device: int = -1):
        cfg = TonedetConfig(int(n_channels), int(fs), int(max_input_frames), device)
        self._create("create", C.byref(cfg))
        self.n_channels, self.fs = int(n_channels), int(fs)

    def reset_peaks(self, channel: int = -1):
        raise AttributeError("the tone detector holds no peaks")

    def process(self, x, n: int | None = None, active=None, flags=None, ok=None, stream=None):
        """takes the first n frames (default all) of x: [C, >= n, 2] float32 on the device, contiguous frames; active: None or a [C]
        uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole and keeps its two bytes); flags, ok: the [C] uint8 CUDA
        tensors to write, None = a new one, False = not written.  Returns (flags, ok), None for one not written.  Asynchronous on
        `stream` (default: torch's current)."""
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32",), "frames")
        pa, stream = _active_ptr(active, self.n_channels), _stream_ptr(stream, x.device)
        flags, pf = _byte_out(flags, "flags", self.n_channels, x.device, stream)
        ok, po = _byte_out(ok, "ok", self.n_channels, x.device, stream)
        self._check(self.L.fmd_tonedet_process_f32_dev(self.t, px, in_stride, n, pa, pf, po, C.c_void_p(stream)))
        return flags, ok

    def _field(self, name: str, value):
        """freq_hz, share_db, raise_intervals and clear_intervals take eight values or one for all eight"""
        kinds = {"freq_hz": (C.c_int, int), "raise_intervals": (C.c_int, int), "clear_intervals": (C.c_int, int), "share_db": (C.c_double, float)}
        if name in kinds:
            ct, py = kinds[name]
            return (ct * 8)(*([py(value)] * 8 if np.isscalar(value) else [py(a) for a in value]))
        return value


def same_default_params() -> SameParams:
    """fmd_same_default_params: pull 16, hold_ticks 750000 (180 s), alarm_mask 0"""
    p = SameParams()
    load_library().fmd_same_default_params(C.byref(p))
    return p


def same_encode(text, fs: int, clock_ratio: float = 1.0, amplitude: float = 0.25, repeats: int = 3, gap_frames: int = -1, mark_db: float = 0.0) -> np.ndarray:
    """fmd_same_encode (host only): `text` (bytes or str, 1 ... 268 bytes) as [n, 2] float32 audio at fs: `repeats` bursts of 16 bytes 0xAB
    and the text at 520.83 bit/s times clock_ratio, each followed by gap_frames of silence (negative: one second)"""
    L = load_library()
    text = text.encode("ascii") if isinstance(text, str) else bytes(text)
    cfg = SameEncodeConfig(int(fs), int(repeats), int(gap_frames), float(clock_ratio), float(amplitude), float(mark_db))
    n = L.fmd_same_encode(C.byref(cfg), text, len(text), None, 0)
    if n < 0:
        raise _global_error(L, "fmd_same", int(n))
    out = np.zeros((n, 2), np.float32)
    rc = L.fmd_same_encode(C.byref(cfg), text, len(text), out.ctypes.data_as(C.c_void_p), n)
    if rc != n:
        raise _global_error(L, "fmd_same", int(rc))
    return out


def same_parse(message) -> dict:
    """fmd_same_parse (host only): one message's bytes -> {"kind", "valid", "org", "event", "locations", "duration_min", "day", "hour",
    "minute", "callsign"}; a field whose SAME_VALID_* bit is clear is empty or 0"""
    L = load_library()
    b = bytes(message)
    h = SameHeader()
    rc = L.fmd_same_parse(b, len(b), C.byref(h))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_same", rc)
    return {"kind": h.kind, "valid": h.valid, "org": h.org.decode(), "event": h.event.decode(),
            "locations": [h.locations[i].value.decode() for i in range(h.n_locations)], "duration_min": h.duration_min, "day": h.day, "hour": h.hour,
            "minute": h.minute, "callsign": h.callsign.decode()}


def same_vote(messages) -> tuple:
    """fmd_same_vote (host only): one to three (sync_tick, kind, bytes) messages of one transmission -> ((sync_tick, kind, bytes) voted byte
    by byte two out of three, corrected, unresolved)"""
    L = load_library()
    m = np.zeros(len(messages), SAME_MESSAGE_DTYPE)
    for i, (tick, kind, b) in enumerate(messages):
        if len(b) > 268:
            raise ValueError("a message has more than 268 bytes")
        m[i]["sync_tick"], m[i]["len"], m[i]["kind"] = tick, len(b), kind
        m[i]["bytes"][:len(b)] = np.frombuffer(bytes(b), np.uint8)
    out = np.zeros(1, SAME_MESSAGE_DTYPE)
    fixed, unresolved = C.c_int(0), C.c_int(0)
    rc = L.fmd_same_vote(m.ctypes.data_as(C.c_void_p), len(messages), out.ctypes.data_as(C.c_void_p), C.byref(fixed), C.byref(unresolved))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_same", rc)
    r = out[0]
    return (int(r["sync_tick"]), int(r["kind"]), bytes(r["bytes"][:int(r["len"])])), fixed.value, unresolved.value


class SameDecoder(_Gated):
    """EAS SAME decoder of C stations' audio on the GPU (fmd_same_*): per station the 520.83 bit/s AFSK bursts in front of and behind an
    alert, decoded to `ZCZC-...` headers and `NNNN` end-of-message marks, and two [C] uint8 tensors: the flags (SAME_SYNCED,
    SAME_ALERT_OPEN) and the ok bytes, which AudioMixer.process(active=...) takes as they are.  Feed it the same [C, n, 2] float32 CUDA
    tensors as AudioMixer and the monitors; it changes nothing in them.  status() returns SAME_STATUS_DTYPE records; messages() the
    messages accepted since it was last asked; same_parse and same_vote are the host's side."""
    _prefix, _attr, _status_dtype, _params_type = "fmd_same", "d", SAME_STATUS_DTYPE, SameParams

    def __init__(self, n_channels: int, fs: int, max_input_frames: int = 1 << 16, device: int = -1):
        cfg = SameConfig(int(n_channels), int(fs), int(max_input_frames), device)
        self._create("create", C.byref(cfg))
        self.n_channels, self.fs = int(n_channels), int(fs)
        self._seen = [0] * self.n_channels

    def reset_peaks(self, channel: int = -1):
        raise AttributeError("the SAME decoder holds no peaks")

    def reset(self, channel: int = -1):
        super().reset(channel)
        for c in (range(self.n_channels) if channel < 0 else (int(channel),)):
            self._seen[c] = 0

    def process(self, x, n: int | None = None, active=None, flags=None, ok=None, stream=None):
        """takes the first n frames (default all) of x: [C, >= n, 2] float32 on the device, contiguous frames; active: None or a [C]
        uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole and keeps its two bytes); flags, ok: the [C] uint8 CUDA
        tensors to write, None = a new one, False = not written.  Returns (flags, ok), None for one not written.  Asynchronous on
        `stream` (default: torch's current)."""
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32",), "frames")
        pa, stream = _active_ptr(active, self.n_channels), _stream_ptr(stream, x.device)
        flags, pf = _byte_out(flags, "flags", self.n_channels, x.device, stream)
        ok, po = _byte_out(ok, "ok", self.n_channels, x.device, stream)
        self._check(self.L.fmd_same_process_f32_dev(self.d, px, in_stride, n, pa, pf, po, C.c_void_p(stream)))
        return flags, ok

    def messages(self, status=None) -> list:
        """per station the messages accepted since the last messages() (or the reset), oldest first, as (sync_tick, kind, bytes); of more
        than eight new ones the ring holds the newest eight.  Waits for the decoder's work unless `status` (its status() records) is given."""
        st = self.status() if status is None else status
        out = []
        for c in range(self.n_channels):
            acc = int(st[c]["accepted"])
            new = []
            for k in range(max(self._seen[c], acc - SAME_RING), acc):
                r = st[c]["ring"][k % SAME_RING]
                new.append((int(r["sync_tick"]), int(r["kind"]), bytes(r["bytes"][:int(r["len"])])))
            self._seen[c] = acc
            out.append(new)
        return out


def adpcm_block_align(block_frames: int = 0) -> int:
    """fmd_adpcm_block_align (host only): bytes of a block of `block_frames` frames (0 = the default 1017: 1024 bytes)"""
    L = load_library()
    rc = L.fmd_adpcm_block_align(int(block_frames))
    if rc < 0:
        raise _global_error(L, "fmd_adpcm", rc)
    return rc


def adpcm_max_blocks(block_frames: int, n: int) -> int:
    """fmd_adpcm_max_blocks (host only): the most blocks a call of n frames completes for a station, (S - 1 + n) / S"""
    L = load_library()
    rc = L.fmd_adpcm_max_blocks(int(block_frames), int(n))
    if rc < 0:
        raise _global_error(L, "fmd_adpcm", int(rc))
    return int(rc)


def adpcm_decode(blocks, block_frames: int = 0) -> np.ndarray:
    """fmd_adpcm_decode_blocks (host only): whole blocks (any uint8 array or bytes of n_blocks * block_align bytes) -> [n_blocks * S, 2] int16"""
    L = load_library()
    align = adpcm_block_align(block_frames)
    b = np.ascontiguousarray(np.frombuffer(blocks, np.uint8) if isinstance(blocks, (bytes, bytearray)) else blocks, np.uint8).reshape(-1)
    if b.size % align:
        raise ValueError(f"{b.size} bytes are no whole number of blocks of {align} bytes")
    nb = b.size // align
    S = (align // 8 - 1) * 8 + 1
    pcm = np.zeros((nb * S, 2), np.int16)
    rc = L.fmd_adpcm_decode_blocks(b.ctypes.data_as(C.c_void_p), int(block_frames), nb, pcm.ctypes.data_as(C.c_void_p))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_adpcm", rc)
    return pcm


def adpcm_wav_header(fs: int, block_frames: int, n_blocks: int, n_frames: int) -> bytes:
    """fmd_adpcm_wav_header (host only): the 60 bytes in front of n_blocks blocks in a WAV file of format 0x0011 whose `fact` chunk states
    n_frames, the true length"""
    L = load_library()
    out = (C.c_ubyte * ADPCM_WAV_HEADER_BYTES)()
    n = C.c_int(0)
    rc = L.fmd_adpcm_wav_header(int(fs), int(block_frames), int(n_blocks), int(n_frames), out, C.byref(n))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_adpcm", rc)
    return bytes(out)[:n.value]


class AdpcmEncoder(_Monitor):
    """Block IMA / DVI ADPCM encoder of C stations' stereo audio on the GPU (fmd_adpcm_*): a quarter of the 16-bit PCM bytes, in blocks that
    a WAV file of format 0x0011 holds as they are.  Feed it the same [C, n, 2] float32 CUDA tensors as AudioMixer and the monitors; it
    changes nothing in them.  process() returns the [C, out_stride] uint8 rows with each station's completed blocks back to back and
    the [C] int32 block counts; flush() closes the open blocks.  status() returns ADPCM_STATUS_DTYPE records; adpcm_decode and
    adpcm_wav_header are the host's side."""
    _prefix, _attr, _status_dtype = "fmd_adpcm", "e", ADPCM_STATUS_DTYPE

    def __init__(self, n_channels: int, block_frames: int = 0, max_input_frames: int = 1 << 16, device: int = -1):
        cfg = AdpcmConfig(int(n_channels), int(block_frames), int(max_input_frames), device)
        self._create("create", C.byref(cfg))
        self.n_channels = int(n_channels)
        self.block_frames = int(block_frames) or ADPCM_DEFAULT_BLOCK_FRAMES
        self.block_align = adpcm_block_align(self.block_frames)

    def reset_peaks(self, channel: int = -1):
        raise AttributeError("the encoder holds no peaks")

    def _outputs(self, out, nblocks, need: int, device, stream):
        """(out, its pointer, out_stride, nblocks, its pointer): out None = a new zeroed [C, need] tensor; nblocks None = new, False = not written"""
        import torch
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device) if stream else torch.cuda.default_stream(device)):
            if out is None:
                out = torch.zeros((self.n_channels, max(need, 4)), dtype=torch.uint8, device=device)
            if nblocks is None:
                nblocks = torch.zeros(self.n_channels, dtype=torch.int32, device=device)
        if not (out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == self.n_channels and out.stride(1) == 1):
            raise ValueError("out must be a [C, out_stride] uint8 CUDA tensor with contiguous rows")
        if out.shape[1] < need:
            raise ValueError(f"out's rows hold {out.shape[1]} bytes; the call may write {need}")
        if nblocks is False:
            nblocks = None
        elif not (nblocks.is_cuda and nblocks.dtype == torch.int32 and nblocks.shape == (self.n_channels,) and nblocks.is_contiguous()):
            raise ValueError("nblocks must be a contiguous [C] int32 CUDA tensor")
        stride = out.stride(0) if self.n_channels > 1 else out.shape[1]
        return out, C.c_void_p(out.data_ptr()), stride, nblocks, None if nblocks is None else C.c_void_p(nblocks.data_ptr())

    def process(self, x, n: int | None = None, active=None, out=None, nblocks=None, stream=None):
        """takes the first n frames (default all) of x: [C, >= n, 2] float32 on the device, contiguous frames; active: None or a [C]
        uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole: its row of out is kept, its count is 0); out: the
        [C, out_stride] uint8 CUDA tensor to write, out_stride a multiple of 4 and at least adpcm_max_blocks(S, n) * block_align, None =
        a new zeroed one of exactly that; nblocks: the [C] int32 CUDA tensor to write, None = a new one, False = not written.  Returns
        (out, nblocks).  Asynchronous on `stream` (default: torch's current)."""
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32",), "frames")
        pa, stream = _active_ptr(active, self.n_channels), _stream_ptr(stream, x.device)
        need = (self.block_frames - 1 + max(n, 0)) // self.block_frames * self.block_align
        out, po, stride, nblocks, pn = self._outputs(out, nblocks, need, x.device, stream)
        self._check(self.L.fmd_adpcm_process_f32_dev(self.e, px, in_stride, n, pa, po, stride, pn, C.c_void_p(stream)))
        return out, nblocks

    def flush(self, channel: int = -1, out=None, nblocks=None, stream=None, device=None):
        """fmd_adpcm_flush: closes the open block of station `channel` (-1 = of every station) with repeats of its last frame: 0 or 1
        block at out[c] and its number in nblocks[c]; the other stations' rows and counts are kept.  out, nblocks as in process (None =
        new, zeroed).  Returns (out, nblocks)."""
        import torch
        device = device if device is not None else (out.device if out is not None and out is not False else torch.device("cuda", torch.cuda.current_device()))
        stream = _stream_ptr(stream, device)
        out, po, stride, nblocks, pn = self._outputs(out, nblocks, self.block_align, device, stream)
        self._check(self.L.fmd_adpcm_flush(self.e, int(channel), po, stride, pn, C.c_void_p(stream)))
        return out, nblocks


def flac_frame_bound(block_frames: int = 0) -> int:
    """fmd_flac_frame_bound (host only): the most bytes of a FLAC frame of `block_frames` frames (0 = the default 4096)"""
    L = load_library()
    rc = L.fmd_flac_frame_bound(int(block_frames))
    if rc < 0:
        raise _global_error(L, "fmd_flac", rc)
    return rc


def flac_max_bytes(block_frames: int, n: int) -> int:
    """fmd_flac_max_bytes (host only): the most bytes a call of n frames writes for a station, rounded up to 4"""
    L = load_library()
    rc = L.fmd_flac_max_bytes(int(block_frames), int(n))
    if rc < 0:
        raise _global_error(L, "fmd_flac", int(rc))
    return int(rc)


def flac_stream_header(fs: int, block_frames: int = 0, total_samples: int = 0, min_frame_bytes: int = 0, max_frame_bytes: int = 0) -> bytes:
    """fmd_flac_stream_header (host only): the 42 bytes `fLaC` + STREAMINFO in front of a stream's frames in a .flac file; zeros where
    unknown; the MD5 signature is all zero, which the format reads as not computed"""
    L = load_library()
    out = (C.c_ubyte * FLAC_STREAM_HEADER_BYTES)()
    n = C.c_int()
    rc = L.fmd_flac_stream_header(int(fs), int(block_frames), int(total_samples), int(min_frame_bytes), int(max_frame_bytes), out, C.byref(n))
    if rc != 0:
        raise _global_error(L, "fmd_flac", rc)
    return bytes(out[:n.value])


def flac_decode(data, fs: int, block_frames: int = 0) -> np.ndarray:
    """fmd_flac_decode (host only): one stream's FLAC frames (any uint8 array or bytes, no stream header) -> [frames, 2] int16; raises
    FmdError(FMD_ERR_ARG) for anything but a whole, intact stream of this encoder's subset"""
    L = load_library()
    b = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8).reshape(-1)
    n = C.c_longlong()
    rc = L.fmd_flac_decode(b.ctypes.data_as(C.c_void_p), b.size, int(fs), int(block_frames), None, 0, C.byref(n))
    if rc != 0:
        raise _global_error(L, "fmd_flac", rc)
    pcm = np.zeros((n.value, 2), np.int16)
    rc = L.fmd_flac_decode(b.ctypes.data_as(C.c_void_p), b.size, int(fs), int(block_frames), pcm.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
    if rc != 0:
        raise _global_error(L, "fmd_flac", rc)
    return pcm


class FlacEncoder(_Monitor):
    """FLAC encoder of C stations' stereo audio on the GPU (fmd_flac_*): per station a lossless stream that decodes to exactly the 16-bit
    PCM fmd_audio_pcm16_dev writes.  Feed it the same [C, n, 2] float32 CUDA tensors as AudioMixer and the monitors; it changes nothing in
    them.  process() returns the [C, out_stride] uint8 rows with each station's completed FLAC frames back to back, the [C] int32 byte
    counts and the [C] int32 frame counts; flush() ends the streams behind a short last frame.  status() returns FLAC_STATUS_DTYPE
    records; flac_decode and flac_stream_header are the host's side."""
    _prefix, _attr, _status_dtype = "fmd_flac", "e", FLAC_STATUS_DTYPE

    def __init__(self, n_channels: int, block_frames: int = 0, sample_rate: int = 32000, max_input_frames: int = 1 << 16, device: int = -1):
        cfg = FlacConfig(int(n_channels), int(block_frames), int(sample_rate), int(max_input_frames), device)
        self._create("create", C.byref(cfg))
        self.n_channels = int(n_channels)
        self.block_frames = int(block_frames) or FLAC_DEFAULT_BLOCK_FRAMES
        self.sample_rate = int(sample_rate)
        self.frame_bound = flac_frame_bound(self.block_frames)

    def reset_peaks(self, channel: int = -1):
        raise AttributeError("the encoder holds no peaks")

    def _outputs(self, out, nbytes, nframes, need: int, device, stream):
        """(out, its pointer, out_stride, nbytes, its pointer, nframes, its pointer): out None = a new zeroed [C, need] tensor; a count
        None = new, False = not written"""
        import torch
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device) if stream else torch.cuda.default_stream(device)):
            if out is None:
                out = torch.zeros((self.n_channels, max(need, 4)), dtype=torch.uint8, device=device)
            if nbytes is None:
                nbytes = torch.zeros(self.n_channels, dtype=torch.int32, device=device)
            if nframes is None:
                nframes = torch.zeros(self.n_channels, dtype=torch.int32, device=device)
        if not (out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == self.n_channels and out.stride(1) == 1):
            raise ValueError("out must be a [C, out_stride] uint8 CUDA tensor with contiguous rows")
        if out.shape[1] < need:
            raise ValueError(f"out's rows hold {out.shape[1]} bytes; the call may write {need}")
        ptrs = []
        for name, t in (("nbytes", nbytes), ("nframes", nframes)):
            if t is False:
                ptrs.append((None, None))
            elif not (t.is_cuda and t.dtype == torch.int32 and t.shape == (self.n_channels,) and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous [C] int32 CUDA tensor")
            else:
                ptrs.append((t, C.c_void_p(t.data_ptr())))
        stride = out.stride(0) if self.n_channels > 1 else out.shape[1]
        return out, C.c_void_p(out.data_ptr()), stride, ptrs[0][0], ptrs[0][1], ptrs[1][0], ptrs[1][1]

    def process(self, x, n: int | None = None, active=None, out=None, nbytes=None, nframes=None, stream=None):
        """takes the first n frames (default all) of x: [C, >= n, 2] float32 on the device, contiguous frames; active: None or a [C]
        uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole: its row of out is kept, its counts are 0); out: the
        [C, out_stride] uint8 CUDA tensor to write, out_stride a multiple of 4 and at least flac_max_bytes(S, n), None = a new zeroed
        one of exactly that; nbytes, nframes: the [C] int32 CUDA tensors to write, None = new ones, False = not written.  Returns
        (out, nbytes, nframes).  Asynchronous on `stream` (default: torch's current)."""
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32",), "frames")
        pa, stream = _active_ptr(active, self.n_channels), _stream_ptr(stream, x.device)
        need = ((self.block_frames - 1 + max(n, 0)) // self.block_frames * self.frame_bound + 3) // 4 * 4
        out, po, stride, nbytes, pb, nframes, pf = self._outputs(out, nbytes, nframes, need, x.device, stream)
        self._check(self.L.fmd_flac_process_f32_dev(self.e, px, in_stride, n, pa, po, stride, pb, pf, C.c_void_p(stream)))
        return out, nbytes, nframes

    def flush(self, channel: int = -1, out=None, nbytes=None, nframes=None, stream=None, device=None):
        """fmd_flac_flush: ends the stream of station `channel` (-1 = of every station): a short last frame of the open block's frames
        at out[c] where there are any, its bytes in nbytes[c] and 0 or 1 in nframes[c]; the other stations' rows and counts are kept.
        out, nbytes, nframes as in process (None = new, zeroed).  Returns (out, nbytes, nframes)."""
        import torch
        device = device if device is not None else (out.device if out is not None and out is not False else torch.device("cuda", torch.cuda.current_device()))
        stream = _stream_ptr(stream, device)
        out, po, stride, nbytes, pb, nframes, pf = self._outputs(out, nbytes, nframes, (self.frame_bound + 3) // 4 * 4, device, stream)
        self._check(self.L.fmd_flac_flush(self.e, int(channel), po, stride, pb, pf, C.c_void_p(stream)))
        return out, nbytes, nframes

    def debug_set_frame_number(self, channel: int, value: int):
        """fmd_debug_flac_set_frame_number (include/fmdemod_flac_debug.h): a test hook"""
        self._check(self.L.fmd_debug_flac_set_frame_number(self.e, int(channel), int(value)))


def logmel_default_config(fs: int, **fields) -> LogmelConfig:
    """fmd_logmel_default_config (host only): win = fs / 40 rounded up to a multiple of 16, hop = fs / 100, 80 Slaney bands from 0 Hz to
    min(8000, fs / 2), log10 with floor 1e-10; `fields` then replace the named fields"""
    L = load_library()
    cfg = LogmelConfig()
    rc = L.fmd_logmel_default_config(int(fs), C.byref(cfg))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_logmel", rc)
    for k, v in fields.items():
        if k not in dict(LogmelConfig._fields_):
            raise TypeError(f"LogmelConfig has no field {k}")
        setattr(cfg, k, v)
    return cfg


def logmel_max_frames(hop: int, n: int) -> int:
    """fmd_logmel_max_frames (host only): (n + hop - 1) / hop, the most spectral frames a call of n frames completes for a station"""
    L = load_library()
    rc = L.fmd_logmel_max_frames(int(hop), int(n))
    if rc < 0:
        raise _global_error(L, "fmd_logmel", int(rc))
    return int(rc)


def logmel_design(cfg: LogmelConfig | None = None, fs: int = 32000, **fields):
    """fmd_logmel_design (host only) of `cfg` (default: logmel_default_config(fs, **fields)): (w [win] float32, fb [n_mels, K] float32, K,
    empty_bands); logmel_tables gives the cos / sin table too"""
    w, tc, ts, fb, K, empty = logmel_tables(cfg, fs, **fields)
    return w, fb, K, empty


def logmel_tables(cfg: LogmelConfig | None = None, fs: int = 32000, **fields):
    """as logmel_design, with the DFT's table: (w, tc [win], ts [win], fb, K, empty_bands)"""
    L = load_library()
    cfg = cfg if cfg is not None else logmel_default_config(fs, **fields)
    K = L.fmd_logmel_bins(C.byref(cfg))
    if K < 0:
        raise _global_error(L, "fmd_logmel", K)
    w, tc, ts = (np.zeros(cfg.win, np.float32) for _ in range(3))
    fb = np.zeros((cfg.n_mels, K), np.float32)
    d = LogmelDesign()
    rc = L.fmd_logmel_design(C.byref(cfg), *(a.ctypes.data_as(C.c_void_p) for a in (w, tc, ts, fb)), C.byref(d))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_logmel", rc)
    return w, tc, ts, fb, d.n_bins, d.empty_bands


def logmel_flog10(x) -> np.ndarray:
    """fmd_logmel_flog10 (host only) of every element of x: the fixed base-10 logarithm the kernel applies"""
    L = load_library()
    a = np.ascontiguousarray(x, np.float32)
    return np.array([L.fmd_logmel_flog10(float(v)) for v in a.reshape(-1)], np.float32).reshape(a.shape)


class LogMel(_Monitor):
    """Log-mel front end of C stations' audio on the GPU (fmd_logmel_*): per station the log-mel spectrogram a model takes, kept
    continuous across calls.  Feed it the same [C, n, 2] float32 CUDA tensors as AudioMixer and the monitors; it changes nothing in
    them.  process() returns the [C, max_frames, n_mels] float32 rows (the completed spectral frames first, oldest first) and the [C]
    int32 counts.  status() returns LOGMEL_STATUS_DTYPE records.  **config: the fields of LogmelConfig over logmel_default_config(fs)."""
    _prefix, _attr, _status_dtype = "fmd_logmel", "g", LOGMEL_STATUS_DTYPE

    def __init__(self, n_channels: int, fs: int = 32000, **config):
        self.L = load_library()
        self.g = None
        self.cfg = logmel_default_config(fs, n_channels=int(n_channels), **config)
        self._create("create", C.byref(self.cfg))
        self.n_channels, self.fs = int(n_channels), int(fs)
        self.win, self.hop, self.n_mels = self.cfg.win, self.cfg.hop, self.cfg.n_mels
        self.n_bins = self.L.fmd_logmel_bins(C.byref(self.cfg))

    def reset_peaks(self, channel: int = -1):
        raise AttributeError("the front end holds no peaks")

    def frame_time(self, t):
        """the centre of spectral frame t (counted from the station's reset) in seconds"""
        return (np.asarray(t, np.float64) * self.hop + self.win / 2) / self.fs

    def process(self, x, n: int | None = None, active=None, out=None, nframes=None, stream=None):
        """takes the first n frames (default all) of x: [C, >= n, 2] float32 on the device, contiguous frames; active: None or a [C]
        uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole: its rows and its count are kept); out: the
        [C, >= logmel_max_frames(hop, n), n_mels] float32 CUDA tensor to write, None = a new zeroed one of exactly that; nframes: the
        [C] int32 CUDA tensor to write, None = a new one, False = not written.  Returns (out, nframes).  Asynchronous on `stream`
        (default: torch's current)."""
        import torch
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32",), "frames")
        pa, stream = _active_ptr(active, self.n_channels), _stream_ptr(stream, x.device)
        rows = (max(n, 0) + self.hop - 1) // self.hop
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=x.device) if stream else torch.cuda.default_stream(x.device)):
            if out is None:
                out = torch.zeros((self.n_channels, max(rows, 1), self.n_mels), dtype=torch.float32, device=x.device)
            if nframes is None:
                nframes = torch.zeros(self.n_channels, dtype=torch.int32, device=x.device)
        if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 3 and out.shape[0] == self.n_channels and out.shape[2] == self.n_mels
                and out.stride(2) == 1 and out.stride(1) == self.n_mels):
            raise ValueError("out must be a [C, max_frames, n_mels] float32 CUDA tensor with contiguous rows")
        if out.shape[1] < rows:
            raise ValueError(f"out holds {out.shape[1]} rows a station; the call may write {rows}")
        if nframes is not False and not (nframes.is_cuda and nframes.dtype == torch.int32 and nframes.shape == (self.n_channels,) and nframes.is_contiguous()):
            raise ValueError("nframes must be a contiguous [C] int32 CUDA tensor")
        stride = out.stride(0) if self.n_channels > 1 else out.shape[1] * self.n_mels
        pn = None if nframes is False else C.c_void_p(nframes.data_ptr())
        self._check(self.L.fmd_logmel_process_f32_dev(self.g, px, in_stride, n, pa, C.c_void_p(out.data_ptr()), stride, pn, C.c_void_p(stream)))
        return out, (None if nframes is False else nframes)


def fprint_default_config(fs: int, **fields) -> FprintConfig:
    """fmd_fprint_default_config (host only): hop = fs * 0.0115 rounded to a multiple of 16, 32 sub-blocks a window, 33 bands from 300 to
    2000 Hz; `fields` then replace the named fields"""
    L = load_library()
    cfg = FprintConfig()
    rc = L.fmd_fprint_default_config(int(fs), C.byref(cfg))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_fprint", rc)
    for k, v in fields.items():
        if k not in dict(FprintConfig._fields_):
            raise TypeError(f"FprintConfig has no field {k}")
        setattr(cfg, k, v)
    return cfg


def fprint_max_prints(hop: int, n: int) -> int:
    """fmd_fprint_max_prints (host only): (n + hop - 1) / hop, the most words a call of n frames completes for a station"""
    L = load_library()
    rc = L.fmd_fprint_max_prints(int(hop), int(n))
    if rc < 0:
        raise _global_error(L, "fmd_fprint", int(rc))
    return int(rc)


def fprint_state_bytes(cfg: FprintConfig, channels: int) -> int:
    """fmd_fprint_state_bytes (host only): the device memory an object of `channels` stations holds"""
    L = load_library()
    rc = L.fmd_fprint_state_bytes(C.byref(cfg), int(channels))
    if rc < 0:
        raise _global_error(L, "fmd_fprint", int(rc))
    return int(rc)


def fprint_design(cfg: FprintConfig | None = None, fs: int = 32000, **fields):
    """fmd_fprint_design (host only) of `cfg` (default: fprint_default_config(fs, **fields)): (bc [hop, K] float32, bs [hop, K] float32,
    wc [n_sub], ws [n_sub], edges [n_bands + 1] int32, K, first_bin)"""
    L = load_library()
    cfg = cfg if cfg is not None else fprint_default_config(fs, **fields)
    K = L.fmd_fprint_bins(C.byref(cfg))
    if K < 0:
        raise _global_error(L, "fmd_fprint", K)
    bc, bs = (np.zeros((cfg.hop, K), np.float32) for _ in range(2))
    wc, ws = (np.zeros(cfg.n_sub, np.float32) for _ in range(2))
    edges = np.zeros(cfg.n_bands + 1, np.int32)
    d = FprintDesign()
    rc = L.fmd_fprint_design(C.byref(cfg), *(a.ctypes.data_as(C.c_void_p) for a in (bc, bs, wc, ws, edges)), C.byref(d))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_fprint", rc)
    return bc, bs, wc, ws, edges, d.n_bins, d.first_bin


def _fprint_words(a, n_bits: int) -> np.ndarray:
    a = np.ascontiguousarray(a, np.uint32).reshape(-1)
    if not 1 <= n_bits <= 32:
        raise ValueError("n_bits outside 1 ... 32")
    return a


def fprint_ber(a, b, n_bits: int = 32) -> float:
    """the bit error rate between two equally long runs of words (host, numpy): differing bits among the top n_bits of each word, over
    their number.  Identical programmes give a few per cent, unrelated ones about 0.5; the paper's threshold is 0.35"""
    a, b = _fprint_words(a, n_bits), _fprint_words(b, n_bits)
    if a.size != b.size or a.size == 0:
        raise ValueError("two runs of the same, non-zero length")
    x = (a ^ b) >> np.uint32(32 - n_bits)
    return float(np.unpackbits(x.view(np.uint8)).sum()) / (a.size * n_bits)


def fprint_match(query, reference, n_bits: int = 32):
    """where `query` lies in `reference` (host, numpy): (offset, ber), the offset in words 0 ... len(reference) - len(query) with the
    smallest bit error rate over the query's whole length, the first such, and that rate.  That rate is what a caller compares with the
    paper's 0.35"""
    q, r = _fprint_words(query, n_bits), _fprint_words(reference, n_bits)
    if q.size == 0 or r.size < q.size:
        raise ValueError("the reference must be at least as long as the non-empty query")
    win = np.lib.stride_tricks.sliding_window_view(r, q.size)
    x = (win ^ q[None, :]) >> np.uint32(32 - n_bits)
    errs = np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=1).sum(axis=1)
    at = int(np.argmin(errs))
    return at, float(errs[at]) / (q.size * n_bits)


class Fingerprinter(_Monitor):
    """Audio fingerprinter of C stations' audio on the GPU (fmd_fprint_*): per station the Haitsma-Kalker robust hash, one uint32 word a
    hop, kept continuous across calls.  Feed it the same [C, n, 2] float32 CUDA tensors as AudioMixer and the monitors; it changes nothing
    in them.  process() returns the [C, max_prints] words (int32 tensors holding the uint32 bit patterns; the completed words first,
    oldest first) and the [C] int32 counts.  status() returns FPRINT_STATUS_DTYPE records.  **config: the fields of FprintConfig over
    fprint_default_config(fs)."""
    _prefix, _attr, _status_dtype = "fmd_fprint", "g", FPRINT_STATUS_DTYPE

    def __init__(self, n_channels: int, fs: int = 32000, **config):
        self.L = load_library()
        self.g = None
        self.cfg = fprint_default_config(fs, n_channels=int(n_channels), **config)
        self._create("create", C.byref(self.cfg))
        self.n_channels, self.fs = int(n_channels), int(fs)
        self.hop, self.n_sub, self.n_bands, self.n_bits = self.cfg.hop, self.cfg.n_sub, self.cfg.n_bands, self.cfg.n_bands - 1
        self.n_bins = self.L.fmd_fprint_bins(C.byref(self.cfg))
        self.state_bytes = fprint_state_bytes(self.cfg, self.n_channels)

    def reset_peaks(self, channel: int = -1):
        raise AttributeError("the fingerprinter holds no peaks")

    def word_time(self, i):
        """the start of word i (counted from the station's reset) in seconds: sample (i + 1) hop"""
        return (np.asarray(i, np.float64) + 1.0) * self.hop / self.fs

    def process(self, x, n: int | None = None, active=None, out=None, nprints=None, energy=None, stream=None):
        """takes the first n frames (default all) of x: [C, >= n, 2] float32 on the device, contiguous frames; active: None or a [C]
        uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole: its state, words and count are kept); out: the
        [C, >= fprint_max_prints(hop, n)] int32 CUDA tensor to write, None = a new zeroed one of exactly that; nprints: the [C] int32
        CUDA tensor to write, None = a new one, False = not written; energy: None = not written, True = a new zeroed
        [C, max_prints, n_bands] float32 tensor, or such a tensor.  Returns (out, nprints), or (out, nprints, energy) where energy
        was asked for.  Asynchronous on `stream` (default: torch's current)."""
        import torch
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32",), "frames")
        pa, stream = _active_ptr(active, self.n_channels), _stream_ptr(stream, x.device)
        rows = (max(n, 0) + self.hop - 1) // self.hop
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=x.device) if stream else torch.cuda.default_stream(x.device)):
            if out is None:
                out = torch.zeros((self.n_channels, max(rows, 1)), dtype=torch.int32, device=x.device)
            if nprints is None:
                nprints = torch.zeros(self.n_channels, dtype=torch.int32, device=x.device)
            if energy is True:
                energy = torch.zeros((self.n_channels, max(rows, 1), self.n_bands), dtype=torch.float32, device=x.device)
        if not (out.is_cuda and out.dtype == torch.int32 and out.dim() == 2 and out.shape[0] == self.n_channels and out.stride(1) == 1):
            raise ValueError("out must be a [C, max_prints] int32 CUDA tensor with contiguous rows")
        if out.shape[1] < rows:
            raise ValueError(f"out holds {out.shape[1]} words a station; the call may write {rows}")
        if nprints is not False and not (nprints.is_cuda and nprints.dtype == torch.int32 and nprints.shape == (self.n_channels,) and nprints.is_contiguous()):
            raise ValueError("nprints must be a contiguous [C] int32 CUDA tensor")
        pe, estride = None, 0
        if energy is not None:
            if not (energy.is_cuda and energy.dtype == torch.float32 and energy.dim() == 3 and energy.shape[0] == self.n_channels and energy.shape[2] == self.n_bands
                    and energy.stride(2) == 1 and energy.stride(1) == self.n_bands):
                raise ValueError("energy must be a [C, max_prints, n_bands] float32 CUDA tensor with contiguous rows")
            if energy.shape[1] < rows:
                raise ValueError(f"energy holds {energy.shape[1]} rows a station; the call may write {rows}")
            pe, estride = C.c_void_p(energy.data_ptr()), (energy.stride(0) if self.n_channels > 1 else energy.shape[1] * self.n_bands)
        stride = out.stride(0) if self.n_channels > 1 else out.shape[1]
        pn = None if nprints is False else C.c_void_p(nprints.data_ptr())
        self._check(self.L.fmd_fprint_process_f32_dev(self.g, px, in_stride, n, pa, C.c_void_p(out.data_ptr()), stride, pn, pe, estride, C.c_void_p(stream)))
        res = (out, None if nprints is False else nprints)
        return res if energy is None else res + (energy,)


def fpmatch_default_config(**fields) -> FpmatchConfig:
    """fmd_fpmatch_default_config (host only): 32 bits, blocks of 256 words searched every 64, the threshold at a bit error rate of
    0.35, hold 3; `fields` then replace the named fields.  Where block or n_bits is given and max_errs is not, max_errs follows them at
    0.35"""
    L = load_library()
    cfg = FpmatchConfig()
    rc = L.fmd_fpmatch_default_config(C.byref(cfg))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_fpmatch", rc)
    for k, v in fields.items():
        if k not in dict(FpmatchConfig._fields_):
            raise TypeError(f"FpmatchConfig has no field {k}")
        setattr(cfg, k, v)
    if "max_errs" not in fields and ("block" in fields or "n_bits" in fields):
        cfg.max_errs = (35 * cfg.block * cfg.n_bits) // 100
    return cfg


def fpmatch_max_events(interval: int, n: int) -> int:
    """fmd_fpmatch_max_events (host only): (n + interval - 1) / interval, the most events a call of n words writes for a station"""
    L = load_library()
    rc = L.fmd_fpmatch_max_events(int(interval), int(n))
    if rc < 0:
        raise _global_error(L, "fmd_fpmatch", int(rc))
    return int(rc)


def fpmatch_max_errs(ber_percent: int, block: int = 256, n_bits: int = 32) -> int:
    """fmd_fpmatch_max_errs (host only): (ber_percent * block * n_bits) / 100 in integers"""
    L = load_library()
    rc = L.fmd_fpmatch_max_errs(int(ber_percent), int(block), int(n_bits))
    if rc < 0:
        raise _global_error(L, "fmd_fpmatch", int(rc))
    return int(rc)


def fpmatch_state_bytes(cfg: FpmatchConfig) -> int:
    """fmd_fpmatch_state_bytes (host only): the device memory an object of cfg holds"""
    L = load_library()
    rc = L.fmd_fpmatch_state_bytes(C.byref(cfg))
    if rc < 0:
        raise _global_error(L, "fmd_fpmatch", int(rc))
    return int(rc)


def fpmatch_design(cfg: FpmatchConfig) -> FpmatchDesign:
    """fmd_fpmatch_design (host only): the mask and what the search kernel is built on (tile, query_block, groups, lds_bytes)"""
    L = load_library()
    d = FpmatchDesign()
    rc = L.fmd_fpmatch_design(C.byref(cfg), C.byref(d))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_fpmatch", rc)
    return d


def fpmatch_check_catalogue(cfg: FpmatchConfig, starts, n_tracks: int | None = None) -> bool:
    """fmd_fpmatch_check_catalogue (host only): whether load() would take a catalogue whose tracks start at `starts` [T + 1]"""
    L = load_library()
    st = np.ascontiguousarray(starts if starts is not None else [], np.int64).reshape(-1)
    T = int(n_tracks) if n_tracks is not None else max(st.size - 1, 0)
    if T + 1 > st.size and T > 0:
        raise ValueError("starts holds n_tracks + 1 entries")
    return L.fmd_fpmatch_check_catalogue(C.byref(cfg), st.ctypes.data_as(C.c_void_p) if st.size else None, T) == FMD_OK


def fpmatch_index_default_config(**fields) -> FpmatchIndexConfig:
    """fmd_fpmatch_index_default_config (host only): max_bucket 8, follow 2; `fields` then replace the named fields"""
    L = load_library()
    idx = FpmatchIndexConfig()
    rc = L.fmd_fpmatch_index_default_config(C.byref(idx))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_fpmatch", rc)
    for k, v in fields.items():
        if k not in dict(FpmatchIndexConfig._fields_):
            raise TypeError(f"FpmatchIndexConfig has no field {k}")
        setattr(idx, k, v)
    return idx


def fpmatch_index_design(cfg: FpmatchConfig, idx: FpmatchIndexConfig) -> FpmatchIndexDesign:
    """fmd_fpmatch_index_design (host only): the directory's bits and entries, the index bytes and the probe kernel's chunk and set"""
    L = load_library()
    d = FpmatchIndexDesign()
    rc = L.fmd_fpmatch_index_design(C.byref(cfg), C.byref(idx), C.byref(d))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_fpmatch", rc)
    return d


def fpmatch_index_state_bytes(cfg: FpmatchConfig, idx: FpmatchIndexConfig) -> int:
    """fmd_fpmatch_index_state_bytes (host only): the device memory an indexed object of cfg and idx holds"""
    L = load_library()
    rc = L.fmd_fpmatch_index_state_bytes(C.byref(cfg), C.byref(idx))
    if rc < 0:
        raise _global_error(L, "fmd_fpmatch", int(rc))
    return int(rc)


def fpmatch_index_build(cfg: FpmatchConfig, idx: FpmatchIndexConfig, words):
    """fmd_fpmatch_index_build (host only): the index load() builds for a catalogue of `words`, as (keys uint32 [D], pos int32 [D], dir
    int32 [dir_entries])"""
    L = load_library()
    words = _fpmatch_words(words)
    d = fpmatch_index_design(cfg, idx)
    keys, pos, dirs = np.zeros(words.size, np.uint32), np.zeros(words.size, np.int32), np.zeros(d.dir_entries, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = L.fmd_fpmatch_index_build(C.byref(cfg), C.byref(idx), ptr(words), words.size, ptr(keys), ptr(pos), ptr(dirs))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_fpmatch", rc)
    return keys, pos, dirs


def _fpmatch_words(t) -> np.ndarray:
    """a run of fingerprint words as uint32: int32 arrays (what Fingerprinter's tensors give on the host) keep their bit patterns"""
    t = np.ascontiguousarray(t).reshape(-1)
    return t.view(np.uint32) if t.dtype == np.int32 else t.astype(np.uint32)


class FingerprintMatcher(_Monitor):
    """Catalogue search for C stations' fingerprints on the GPU (fmd_fpmatch_*): holds a catalogue of reference fingerprints and per
    station its newest `block` words, takes what Fingerprinter.process returns (the [C, max_prints] int32 words and the [C] int32 counts)
    and, whenever a station's word count crosses a multiple of `interval`, searches the whole catalogue for the station's newest words.
    process() returns the events ([C, max_events, 3] int64 tensor: view a station's row with events_of()), their [C] int32 counts and the
    [C] uint8 flags and ok bytes, all on the device.  status() returns FPMATCH_STATUS_DTYPE records.  **config: the fields of FpmatchConfig
    over fpmatch_default_config().  index: None searches by brute force; True or a dict of FpmatchIndexConfig's fields (max_bucket,
    follow) over fpmatch_index_default_config() makes an indexed object (fmd_fpmatch_create_ex), which looks the query's words up in a
    sorted index of the catalogue and counts errors only at the positions they propose; index_status() then returns its
    FPMATCH_INDEX_STATUS_DTYPE records."""
    _prefix, _attr, _status_dtype = "fmd_fpmatch", "g", FPMATCH_STATUS_DTYPE

    def __init__(self, n_channels: int, index=None, **config):
        self.L = load_library()
        self.g = None
        self.cfg = fpmatch_default_config(n_channels=int(n_channels), **config)
        self.index = None if index is None or index is False else fpmatch_index_default_config(**({} if index is True else dict(index)))
        if self.index is None:
            self._create("create", C.byref(self.cfg))
        else:
            self._create("create_ex", C.byref(self.cfg), C.byref(self.index))
            self.index_design = fpmatch_index_design(self.cfg, self.index)
        self.n_channels = int(n_channels)
        self.block, self.interval, self.n_bits, self.max_errs, self.hold = self.cfg.block, self.cfg.interval, self.cfg.n_bits, self.cfg.max_errs, self.cfg.hold
        self.design = fpmatch_design(self.cfg)
        self.state_bytes = fpmatch_state_bytes(self.cfg) if self.index is None else fpmatch_index_state_bytes(self.cfg, self.index)
        self.n_tracks, self.catalogue_words = 0, 0

    def index_status(self) -> np.ndarray:
        """fmd_fpmatch_get_index_status: [C] FPMATCH_INDEX_STATUS_DTYPE records; waits for the object's work.  FMD_ERR_STATE on an object
        without an index"""
        out = np.zeros(self.n_channels, FPMATCH_INDEX_STATUS_DTYPE)
        self._check(self.L.fmd_fpmatch_get_index_status(self.g, out.ctypes.data_as(C.c_void_p)))
        return out

    def reset_peaks(self, channel: int = -1):
        raise AttributeError("the matcher holds no peaks")

    def load(self, tracks):
        """replaces the catalogue by `tracks`, a sequence of runs of uint32 words (an empty one empties it); waits for the object's work"""
        tracks = [_fpmatch_words(t) for t in tracks]
        starts = np.concatenate([[0], np.cumsum([t.size for t in tracks])]).astype(np.int64)
        self.load_raw(np.concatenate(tracks) if tracks else np.zeros(0, np.uint32), starts, len(tracks))

    def load_raw(self, words, starts, n_tracks: int):
        """fmd_fpmatch_load: words [starts[n_tracks]] uint32 and starts [n_tracks + 1] in host memory"""
        words = np.ascontiguousarray(words, np.uint32).reshape(-1)
        starts = np.ascontiguousarray(starts, np.int64).reshape(-1)
        if starts.size < int(n_tracks) + 1 or (int(n_tracks) > 0 and 0 <= int(starts[int(n_tracks)]) and words.size < int(starts[int(n_tracks)])):
            raise ValueError("starts holds n_tracks + 1 entries and words starts[n_tracks] words")
        self._check(self.L.fmd_fpmatch_load(self.g, words.ctypes.data_as(C.c_void_p) if words.size else None, starts.ctypes.data_as(C.c_void_p), int(n_tracks)))
        self.n_tracks, self.catalogue_words = int(n_tracks), int(starts[int(n_tracks)]) if n_tracks else 0

    @staticmethod
    def events_of(events, nevents=None, channel: int = 0) -> np.ndarray:
        """station `channel`'s row of process()'s events as FPMATCH_EVENT_DTYPE records on the host, the first nevents[channel] where the
        counts are given"""
        row = events[channel].cpu().numpy().reshape(-1).view(FPMATCH_EVENT_DTYPE)
        return row if nevents is None else row[:int(nevents[channel])]

    def process(self, words, nwords=None, n: int | None = None, active=None, events=None, nevents=None, flags=None, ok=None, stream=None):
        """takes up to n words (default: all columns) of every station.  words: [C, >= n] int32 CUDA tensor with contiguous rows, as
        Fingerprinter.process returns it; nwords: the [C] int32 counts on the device, None = n for every station; active: None or a [C]
        uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole); events: the [C, >= fpmatch_max_events(interval, n), 3]
        int64 CUDA tensor to write, None = a new zeroed one of exactly that; nevents: [C] int32, flags, ok: [C] uint8 CUDA tensors to
        write, None = new ones, False = not written.  Returns (events, nevents, flags, ok).  Asynchronous on `stream` (default:
        torch's current)."""
        import torch
        Cn = self.n_channels
        if not (words.is_cuda and words.dtype == torch.int32 and words.dim() == 2 and words.shape[0] == Cn and (words.stride(1) == 1 or words.shape[1] <= 1)):
            raise ValueError("words must be a [C, n] int32 CUDA tensor with contiguous rows")
        n = int(words.shape[1]) if n is None else int(n)
        wstride = words.stride(0) if Cn > 1 else words.shape[1]
        if nwords is not None and not (nwords.is_cuda and nwords.dtype == torch.int32 and nwords.shape == (Cn,) and nwords.is_contiguous()):
            raise ValueError("nwords must be a contiguous [C] int32 CUDA tensor")
        pa, stream = _active_ptr(active, Cn), _stream_ptr(stream, words.device)
        rows = (max(n, 0) + self.interval - 1) // self.interval
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=words.device) if stream else torch.cuda.default_stream(words.device)):
            if events is None:
                events = torch.zeros((Cn, max(rows, 1), 3), dtype=torch.int64, device=words.device)
            if nevents is None:
                nevents = torch.zeros(Cn, dtype=torch.int32, device=words.device)
        if not (events.is_cuda and events.dtype == torch.int64 and events.dim() == 3 and events.shape[0] == Cn and events.shape[2] == 3 and events.stride(2) == 1
                and events.stride(1) == 3):
            raise ValueError("events must be a [C, max_events, 3] int64 CUDA tensor with contiguous rows")
        if events.shape[1] < rows:
            raise ValueError(f"events holds {events.shape[1]} events a station; the call may write {rows}")
        if nevents is not False and not (nevents.is_cuda and nevents.dtype == torch.int32 and nevents.shape == (Cn,) and nevents.is_contiguous()):
            raise ValueError("nevents must be a contiguous [C] int32 CUDA tensor")
        flags, pf = _byte_out(flags, "flags", Cn, words.device, stream)
        ok, po = _byte_out(ok, "ok", Cn, words.device, stream)
        estride = events.stride(0) // 3 if Cn > 1 else events.shape[1]
        pn = None if nevents is False else C.c_void_p(nevents.data_ptr())
        pw = None if nwords is None else C.c_void_p(nwords.data_ptr())
        self._check(self.L.fmd_fpmatch_process_dev(self.g, C.c_void_p(words.data_ptr()), wstride, pw, n, pa, C.c_void_p(events.data_ptr()), estride, pn, pf, po,
                                                   C.c_void_p(stream)))
        return events, (None if nevents is False else nevents), flags, ok


def limiter_design(fs: int, lookahead_ms: float, release_ms: float, ceiling_db: float) -> LimiterDesign:
    """fmd_limiter_design (host only): D = llround(lookahead_ms * fs / 1000) in [0, 255], step = clamp(llround(2^30 / (release_ms * fs / 1000)), 1, 2^30)
    (release_ms = 0: 2^30), T = (float)10^(ceiling_db / 20) with ceiling_db in [-40, 0], and the latency, D frames"""
    L = load_library()
    out = LimiterDesign()
    rc = L.fmd_limiter_design(int(fs), float(lookahead_ms), float(release_ms), float(ceiling_db), C.byref(out))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_limiter", rc)
    return out


def limiter_default_config(fs: int, **fields) -> LimiterConfig:
    """fmd_limiter_default_config (host only): one station, 1.5 ms look-ahead, 500 ms release, -1 dBFS ceiling (conventional values, not
    tuned by listening); `fields` then replace the named fields"""
    L = load_library()
    cfg = LimiterConfig()
    rc = L.fmd_limiter_default_config(int(fs), C.byref(cfg))
    if rc != FMD_OK:
        raise _global_error(L, "fmd_limiter", rc)
    for k, v in fields.items():
        if k not in dict(LimiterConfig._fields_):
            raise TypeError(f"LimiterConfig has no field {k}")
        setattr(cfg, k, v)
    return cfg


def limiter_gain_for_loudness(lufs: float, target_lufs: float = -23.0) -> float:
    """fmd_limiter_gain_for_loudness (host only): 10^((target_lufs - lufs) / 20) as a float: what takes meter_integrated's result to
    Limiter.set_gain"""
    return float(load_library().fmd_limiter_gain_for_loudness(float(lufs), float(target_lufs)))


class Limiter(_Monitor):
    """Look-ahead peak limiter of C stations' (or buses') stereo audio on the GPU (fmd_limiter_*): a gain per station and a brick-wall
    ceiling.  Feed it the same [C, n, 2] float32 CUDA tensors as AudioMixer, the monitors and the encoders; it changes nothing in them.
    process() returns the [C, n, 2] float32 output, the input delayed by `latency` frames; flush() pushes the last `latency` frames out.
    status() returns LIMITER_STATUS_DTYPE records."""
    _prefix, _attr, _status_dtype = "fmd_limiter", "l", LIMITER_STATUS_DTYPE

    def __init__(self, n_channels: int, fs: int = 32000, lookahead_ms: float = 1.5, release_ms: float = 500.0, ceiling_db: float = -1.0,
                 max_input_frames: int = 1 << 16, device: int = -1):
        cfg = LimiterConfig(int(n_channels), int(fs), float(lookahead_ms), float(release_ms), float(ceiling_db), int(max_input_frames), device)
        self._create("create", C.byref(cfg))
        self.n_channels = int(n_channels)
        self.design = limiter_design(fs, lookahead_ms, release_ms, ceiling_db)

    @property
    def latency(self) -> int:
        """frames by which the output trails the input: D"""
        return int(self.design.latency_frames)

    def reset_peaks(self, channel: int = -1):
        raise AttributeError("the limiter holds no peaks")

    def set_gain(self, gain: float, channel: int = -1):
        """fmd_limiter_set_gain: the gain of station `channel` (-1 = of every station), finite and >= 0, for the frames later calls take"""
        self._check(self.L.fmd_limiter_set_gain(self.l, int(channel), float(gain)))

    def get_gain(self, channel: int) -> float:
        g = C.c_float(0.0)
        self._check(self.L.fmd_limiter_get_gain(self.l, int(channel), C.byref(g)))
        return float(g.value)

    def _out(self, out, rows: int, device, stream):
        """(out, its pointer, out_stride): out None = a new zeroed [C, rows, 2] tensor"""
        import torch
        if out is None:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device) if stream else torch.cuda.default_stream(device)):
                out = torch.zeros((self.n_channels, max(rows, 1), 2), dtype=torch.float32, device=device)
        if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 3 and out.shape[0] == self.n_channels and out.shape[2] == 2 and out.stride(2) == 1
                and out.stride(1) == 2):
            raise ValueError("out must be a [C, >= n, 2] float32 CUDA tensor with contiguous frames")
        if out.shape[1] < rows:
            raise ValueError(f"out's rows hold {out.shape[1]} frames; the call writes {rows}")
        return out, C.c_void_p(out.data_ptr()), out.stride(0) // 2 if self.n_channels > 1 else out.shape[1]

    def process(self, x, n: int | None = None, active=None, out=None, gr=False, stream=None):
        """takes the first n frames (default all) of x: [C, >= n, 2] float32 on the device, contiguous frames; active: None or a [C]
        uint8 / bool CUDA tensor (a station whose byte is 0 is skipped whole: its state, its row of out and its gr are kept); out: the
        [C, >= n, 2] float32 CUDA tensor to write (frames behind n are kept), None = a new zeroed one of n frames; gr: False = not
        written, True = a new [C] float32 tensor, or the tensor to write: the smallest gain among the call's output frames.  Returns
        out, or (out, gr) where gr was asked for.  Asynchronous on `stream` (default: torch's current)."""
        import torch
        px, in_stride, n = _batch_input(x, self.n_channels, n, ("float32",), "frames")
        pa, stream = _active_ptr(active, self.n_channels), _stream_ptr(stream, x.device)
        out, po, stride = self._out(out, max(n, 0), x.device, stream)
        pg = None
        if gr is True:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=x.device) if stream else torch.cuda.default_stream(x.device)):
                gr = torch.ones(self.n_channels, dtype=torch.float32, device=x.device)
        if gr is not False and gr is not None:
            if not (gr.is_cuda and gr.dtype == torch.float32 and gr.shape == (self.n_channels,) and gr.is_contiguous()):
                raise ValueError("gr must be a contiguous [C] float32 CUDA tensor")
            pg = C.c_void_p(gr.data_ptr())
        self._check(self.L.fmd_limiter_process_f32_dev(self.l, px, in_stride, n, pa, po, stride, pg, C.c_void_p(stream)))
        return out if pg is None else (out, gr)

    def flush(self, channel: int = -1, out=None, nout=None, stream=None, device=None):
        """fmd_limiter_flush: the `latency` frames that as many frames of silence push out of station `channel` (-1 = of every station), at
        out[c], and their number in nout[c] (None = a new [C] int32 tensor, False = not written); then the station's signal state is as
        after a reset, counters and gain kept.  Returns (out, nout)."""
        import torch
        device = device if device is not None else (out.device if out is not None else torch.device("cuda", torch.cuda.current_device()))
        stream = _stream_ptr(stream, device)
        out, po, stride = self._out(out, self.latency, device, stream)
        pn = None
        if nout is None:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device) if stream else torch.cuda.default_stream(device)):
                nout = torch.zeros(self.n_channels, dtype=torch.int32, device=device)
        if nout is False:
            nout = None
        else:
            if not (nout.is_cuda and nout.dtype == torch.int32 and nout.shape == (self.n_channels,) and nout.is_contiguous()):
                raise ValueError("nout must be a contiguous [C] int32 CUDA tensor")
            pn = C.c_void_p(nout.data_ptr())
        self._check(self.L.fmd_limiter_flush(self.l, int(channel), po, stride, pn, C.c_void_p(stream)))
        return out, nout

    def debug_set_frames(self, channel: int, frames: int):
        """fmd_limiter_debug_set_frames (include/fmdemod_limiter_debug.h): a test's way to a frame count past 2^32"""
        self._check(self.L.fmd_limiter_debug_set_frames(self.l, int(channel), int(frames)))
