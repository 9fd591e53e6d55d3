"""fm-radio_amd — MI355X-native batched broadcast-FM demodulator.

The product is `csrc/libfmdemod.so` (hand-written HIP kernels behind the C ABI in include/fmdemod.h).
This package is the thin Python plumbing around it: building the library, a ctypes binding, and
helpers that hand torch device tensors (device memory, streams, torch.distributed) to the C ABI.
Nothing here computes anything on the CPU: if the library or a gfx950 device is missing, calls raise.

The directory name contains a hyphen, so import it through `fmradio_loader.load()` (repo root) or
`importlib` with the module name `fm_radio_amd`.
"""
from .capi import (  # noqa: F401
    FMD_FLAG_FAST_MATH, FMD_FLAG_RDS_DECODE, RDS_DB_DTYPE, RDS_GROUP_DTYPE, RDSDecoder,
    FMD_AUDIO_LMR, FMD_AUDIO_LPR, FMD_AUDIO_STEREO, FMD_FLAG_KEEP_TAPS, FMD_FLAG_NO_PIPELINE, BatchDemod, Coeffs, Config, Controls, FmdError,
    AudioResampler, FMD_RESAMPLE_POLYPHASE, FMD_RESAMPLE_REFERENCE, resampler_design, AudioMixer,
    BandScanner, SCAN_STATION_DTYPE, scan_default_nfft, scan_default_params, scan_detect,
    IqCorrector, IqCorrection, IqMoments, IqcorrConfig, iqcorr_solve,
    LoudnessMeter, METER_BINS, METER_STATUS_DTYPE, MeterConfig, MeterDesign, meter_design, meter_integrated, meter_lufs, meter_momentary, meter_short_term,
    METER_R128_DTYPE, METER_RANGE, METER_TRUE_PEAK, MeterTpDesign, meter_dbtp, meter_range, meter_tp_design,
    ModulationMonitor, MODMON_BINS, MODMON_STATUS_DTYPE, ModmonConfig, ModmonDesign, modmon_design, modmon_deviation_hz, modmon_exceedance, modmon_mpx_power_dbr, modmon_offset_hz, modmon_percentile, modmon_pilot_hz,
    Squelch, SQUELCH_STATUS_DTYPE, SquelchConfig, SquelchParams, FMD_SQUELCH_AUTO, FMD_SQUELCH_FORCE_CLOSED, FMD_SQUELCH_FORCE_OPEN, squelch_cnr_db, squelch_default_params, squelch_level_db, squelch_powers, squelch_threshold,
    ToneDetector, TONEDET_STATUS_DTYPE, TONEDET_SLOTS, TonedetConfig, TonedetParams, tonedet_default_params, tonedet_level_db, tonedet_share_db,
    AdpcmEncoder, ADPCM_STATUS_DTYPE, ADPCM_DEFAULT_BLOCK_FRAMES, ADPCM_WAV_HEADER_BYTES, AdpcmConfig, adpcm_block_align, adpcm_decode, adpcm_max_blocks, adpcm_wav_header,
    FlacEncoder, FLAC_STATUS_DTYPE, FLAC_DEFAULT_BLOCK_FRAMES, FLAC_STREAM_HEADER_BYTES, FlacConfig, flac_decode, flac_frame_bound, flac_max_bytes, flac_stream_header,
    LogMel, LOGMEL_STATUS_DTYPE, LOGMEL_SLANEY, LOGMEL_HTK, LOGMEL_POWER, LOGMEL_LOG10, LogmelConfig, LogmelDesign, logmel_default_config, logmel_design, logmel_flog10, logmel_max_frames, logmel_tables,
    Fingerprinter, FPRINT_STATUS_DTYPE, FprintConfig, FprintDesign, fprint_ber, fprint_default_config, fprint_design, fprint_match, fprint_max_prints, fprint_state_bytes,
    FingerprintMatcher, FPMATCH_STATUS_DTYPE, FPMATCH_EVENT_DTYPE, FpmatchConfig, FpmatchDesign, fpmatch_check_catalogue, fpmatch_default_config, fpmatch_design, fpmatch_max_errs, fpmatch_max_events, fpmatch_state_bytes,
    FPMATCH_INDEX_STATUS_DTYPE, FpmatchIndexConfig, FpmatchIndexDesign, fpmatch_index_build, fpmatch_index_default_config, fpmatch_index_design, fpmatch_index_state_bytes,
    Limiter, LIMITER_STATUS_DTYPE, LimiterConfig, LimiterDesign, limiter_default_config, limiter_design, limiter_gain_for_loudness,
    SameDecoder, SAME_STATUS_DTYPE, SAME_MESSAGE_DTYPE, SAME_SYNCED, SAME_ALERT_OPEN, SAME_KIND_HEADER, SAME_KIND_EOM, SAME_RING, SameConfig, SameParams, SameHeader, SameEncodeConfig,
    SAME_VALID_ORG, SAME_VALID_EVENT, SAME_VALID_LOCATIONS, SAME_VALID_DURATION, SAME_VALID_TIME, SAME_VALID_CALLSIGN, same_default_params, same_encode, same_parse, same_vote,
    AudioMonitor, AUDMON_STATUS_DTYPE, AudmonConfig, AudmonParams, AUDMON_SILENCE, AUDMON_LEFT_LOST, AUDMON_RIGHT_LOST, AUDMON_ANTIPHASE, AUDMON_MONO, audmon_balance_db, audmon_correlation, audmon_default_params, audmon_level_db, audmon_side_mid_db,
    Channelizer, Rates, build_library, chan_default_taps, chan_design, declared_symbols, default_config, default_controls, plan, PlanInfo, PLL_KERNELS, block_plan, BlockPlanInfo, PlanFacts, lib_path, load_library, selftest_atan2, selftest_atan2_small, selftest_fast_math,
)
from .sharding import AudioGather, channel_range, padded_shard  # noqa: F401,E402
