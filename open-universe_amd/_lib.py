"""
ctypes binding of libouniverse.so (the C ABI declared in include/ouniverse.h).

This is the only bridge between the Python host side and the HIP kernels.  There is no fallback: if the
shared library is missing (not built) every entry point raises, loudly.
"""
import ctypes
import os
from ctypes import (POINTER, Structure, byref, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint32, c_uint64,
                    c_void_p)

OU_MAX_RATES = 8
OU_ABI_VERSION = 7
OU_OK, OU_EINVAL, OU_ENOTIMPL, OU_EMISSING, OU_ESHAPE, OU_EHIP, OU_ENOMEM, OU_ESYNC = 0, -1, -2, -3, -4, -5, -6, -7
OU_KIND_UNIVERSE, OU_KIND_UNIVERSE_GAN = 0, 1
OU_ACT_NONE, OU_ACT_PRELU, OU_ACT_SNAKE, OU_ACT_SNAKEBETA = 0, 1, 2, 3
OU_ACT_IDENTITY = -1  # act_type "none" in the four *_act fields of ou_config, where 0 means "not set" = PReLU
# encoder_act_type / decoder_act_type -> ou_config.*_act ("prelu" stays 0: the config of a PReLU model is what it always was)
# normalization_norm -> the mode of ou_set_normalization
OU_NORM_2, OU_NORM_MAX, OU_NORM_2MAX = 0, 1, 2
NORM_MODES = {"2": OU_NORM_2, "max": OU_NORM_MAX, "2-max": OU_NORM_2MAX}
OU_SEQ_GRU, OU_SEQ_NONE, OU_SEQ_GRU_SANDWICH = 0, 2, 3  # ou_config.score.seq_bottleneck (1: a legacy spelling of the plain GRU)
BODY_ACTS = {"prelu": 0, "snake": OU_ACT_SNAKE, "snakebeta": OU_ACT_SNAKEBETA, "none": OU_ACT_IDENTITY}
OU_ENH_KEEP_RMS, OU_ENH_USE_AUX_SIGNAL, OU_ENH_NO_PEAK_GUARD, OU_ENH_SERIAL = 1, 2, 4, 8
OU_MAX_ENSEMBLE = 32
OU_ENS_MEAN, OU_ENS_MEDIAN, OU_ENS_SIGNAL_MEDIAN = 0, 1, 2
ENSEMBLE_STATS = {"mean": OU_ENS_MEAN, "median": OU_ENS_MEDIAN, "signal_median": OU_ENS_SIGNAL_MEDIAN}


class _NetConfigLast(ctypes.Union):
    """The last slot of ou_net_config: encoder_gru_residual in ou_config.cond, seq_bottleneck (OU_SEQ_*) in ou_config.score."""
    _fields_ = [("encoder_gru_residual", c_int32), ("seq_bottleneck", c_int32)]


class NetConfig(Structure):
    _anonymous_ = ("_last",)
    _fields_ = [
        ("n_rates", c_int32),
        ("rate_factors", c_int32 * OU_MAX_RATES),
        ("n_channels", c_int32),
        ("fb_kernel_size", c_int32),
        ("n_rff", c_int32),
        ("noise_cond_dim", c_int32),
        ("extra_conv_block", c_int32),
        ("use_weight_norm", c_int32),
        ("use_antialiasing", c_int32),
        ("time_embedding_simple", c_int32),
        ("n_mels", c_int32),
        ("n_mel_oversample", c_int32),
        ("_last", _NetConfigLast),
    ]


class Config(Structure):
    _fields_ = [
        ("abi_version", c_int32),
        ("kind", c_int32),
        ("fs", c_int32),
        ("level_db", c_float),
        ("has_edm", c_int32),
        ("edm_noise", c_float),
        ("sigma_min", c_double),
        ("sigma_max", c_double),
        ("use_signal_decoupling", c_int32),
        ("signal_decoupling_act", c_int32),
        ("score", NetConfig),
        ("cond", NetConfig),
        ("has_edm_data_level", c_int32),
        ("edm_data_level_db", c_float),
        ("fir_fold", c_int32),
        ("no_split_copy", c_int32),
        ("score_enc_act", c_int32),
        ("score_dec_act", c_int32),
        ("cond_enc_act", c_int32),
        ("cond_dec_act", c_int32),
    ]


class NoiseSpec(Structure):
    """ou_noise_spec: counter-based noise source of a handle (include/ouniverse.h)."""
    _fields_ = [
        ("seed", c_uint64),
        ("streams", POINTER(c_uint64)),
        ("n_streams", c_int32),
        ("scratch", c_void_p),
        ("scratch_bytes", c_size_t),
    ]


class StreamSpec(Structure):
    """ou_stream_spec: what a streaming enhance session is created with (include/ouniverse.h, "streaming enhance")."""
    _fields_ = [
        ("C", c_int32),
        ("segment", c_int32),
        ("overlap", c_int32),
        ("n_steps", c_int32),
        ("epsilon", c_double),
        ("sigma_host", POINTER(c_float)),
        ("warm_start", c_int32),
        ("enh_flags", c_uint32),
        ("stream_flags", c_uint32),
        ("seed", c_uint64),
        ("ids", POINTER(c_uint64)),
    ]


OU_STREAM_CLIP = 1


class MetricsSpec(Structure):
    """ou_metrics_spec: one STFT resolution of the scores (include/ouniverse.h, "scoring")."""
    _fields_ = [("n_fft", c_int32), ("hop", c_int32), ("eps", c_float), ("flags", c_int32)]


OU_METRICS_MAX_NFFT, OU_METRICS_MAX_SPECS = 1024, 8
OU_MET_SCALE_INVARIANT, OU_MET_NATURAL_LOG = 1, 2


class LibraryNotBuilt(RuntimeError):
    pass


_LIB = None


def lib_path():
    return os.environ.get("OU_LIBRARY", os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libouniverse.so"))


def load():
    """Load libouniverse.so.  Raises LibraryNotBuilt (never falls back) when it is absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise LibraryNotBuilt(
            f"{path} not found: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C open-universe_amd/csrc`).  open_universe_amd has no CPU / eager fallback."
        )
    L = ctypes.CDLL(path)
    vp, sz, i32 = c_void_p, c_size_t, c_int32
    sig = {
        "ou_version": (c_char_p, []),
        "ou_last_error": (c_char_p, [vp]),
        "ou_packer_last_error": (c_char_p, [vp]),
        "ou_packer_create": (i32, [POINTER(Config), POINTER(vp)]),
        "ou_packer_set": (i32, [vp, c_char_p, vp, POINTER(c_int64), i32]),
        "ou_packer_finish": (i32, [vp, POINTER(vp), POINTER(sz)]),
        "ou_packer_destroy": (None, [vp]),
        "ou_packed_bytes": (i32, [POINTER(Config), POINTER(sz)]),
        "ou_create": (i32, [POINTER(Config), vp, sz, i32, POINTER(vp)]),
        "ou_destroy": (None, [vp]),
        "ou_workspace_bytes": (i32, [vp, i32, i32, POINTER(sz)]),
        "ou_schedule": (i32, [POINTER(Config), i32, c_double, POINTER(c_float), POINTER(c_double), POINTER(c_double)]),
        "ou_condition": (i32, [vp, vp, i32, i32, vp, sz, vp]),
        "ou_score": (i32, [vp, vp, POINTER(c_float), vp, i32, i32, vp, sz, vp]),
        "ou_aux_to_wav": (i32, [vp, vp, i32, i32, vp, sz, vp]),
        "ou_enhance": (i32, [vp, vp, vp, vp, i32, i32, i32, c_double, POINTER(c_float), i32, c_uint32, vp, sz, vp]),
        "ou_enhance_var": (i32, [vp, vp, vp, vp, i32, i32, POINTER(i32), i32, c_double, POINTER(c_float), i32, c_uint32, vp, sz, vp]),
        "ou_ensemble_workspace_bytes": (i32, [vp, i32, i32, i32, POINTER(sz)]),
        "ou_enhance_ensemble": (i32, [vp, vp, vp, vp, vp, i32, i32, POINTER(i32), i32, i32, i32, c_double, POINTER(c_float), i32,
                                      c_uint32, vp, sz, vp]),
        "ou_ensemble_reduce_scratch_bytes": (sz, [i32, i32]),
        "ou_ensemble_reduce": (i32, [vp, vp, i32, i32, c_int64, c_int64, POINTER(c_int64), i32, vp, sz, vp]),
        "ou_segment_plan": (i32, [i32, c_int64, i32, i32, i32, POINTER(c_int64), POINTER(i32), POINTER(c_int64),
                                  POINTER(c_int64), POINTER(i32), POINTER(i32), POINTER(c_int64)]),
        "ou_segments_workspace_bytes": (i32, [vp, i32, c_int64, i32, i32, i32, POINTER(sz), POINTER(i32), POINTER(i32)]),
        "ou_enhance_segments": (i32, [vp, vp, vp, vp, i32, c_int64, i32, i32, i32, i32, c_double, POINTER(c_float), i32,
                                      c_uint32, vp, sz, vp]),
        "ou_segment_groups": (i32, [i32, i32, POINTER(c_int64), i32, i32, i32, i32, POINTER(i32), POINTER(i32), POINTER(i32),
                                    POINTER(i32), POINTER(i32), POINTER(i32), POINTER(i32), POINTER(i32), POINTER(i32)]),
        "ou_segments_var_workspace_bytes": (i32, [vp, i32, POINTER(c_int64), i32, i32, i32, POINTER(sz), POINTER(i32),
                                                  POINTER(i32)]),
        "ou_enhance_segments_var": (i32, [vp, vp, vp, vp, i32, c_int64, POINTER(c_int64), i32, i32, i32, i32, c_double,
                                          POINTER(c_float), i32, c_uint32, vp, sz, vp]),
        "ou_segments_ensemble_workspace_bytes": (i32, [vp, i32, c_int64, i32, i32, i32, i32, POINTER(sz), POINTER(i32),
                                                       POINTER(i32)]),
        "ou_enhance_segments_ensemble": (i32, [vp, vp, vp, vp, vp, i32, c_int64, i32, i32, i32, i32, i32, i32, c_double,
                                               POINTER(c_float), i32, c_uint32, vp, sz, vp]),
        "ou_segments_var_ensemble_workspace_bytes": (i32, [vp, i32, POINTER(c_int64), i32, i32, i32, i32, POINTER(sz),
                                                           POINTER(i32), POINTER(i32)]),
        "ou_enhance_segments_var_ensemble": (i32, [vp, vp, vp, vp, vp, i32, c_int64, POINTER(c_int64), i32, i32, i32, i32, i32,
                                                   i32, c_double, POINTER(c_float), i32, c_uint32, vp, sz, vp]),
        "ou_stream_plan": (i32, [i32, c_int64, i32, i32, i32, POINTER(c_int64), POINTER(i32), POINTER(c_int64),
                                 POINTER(c_int64), POINTER(i32), POINTER(i32), POINTER(c_int64)]),
        "ou_stream_emitted": (c_int64, [i32, c_int64, i32, i32]),
        "ou_stream_workspace_bytes": (i32, [vp, i32, i32, i32, POINTER(sz)]),
        "ou_stream_create": (i32, [vp, POINTER(StreamSpec), vp, sz, POINTER(vp)]),
        "ou_stream_destroy": (None, [vp]),
        "ou_stream_push": (i32, [vp, vp, c_int64, c_int64, vp, c_int64, c_int64, POINTER(c_int64), vp]),
        "ou_stream_flush": (i32, [vp, vp, c_int64, c_int64, POINTER(c_int64), vp]),
        "ou_set_noise_source": (i32, [vp, POINTER(NoiseSpec)]),
        "ou_noise_scratch_bytes": (i32, [vp, i32, i32, POINTER(sz)]),
        "ou_noise_fill": (i32, [vp, c_int64, c_int64, i32, POINTER(c_uint64), POINTER(c_int64), POINTER(c_int64), c_uint64,
                                i32, vp]),
        "ou_resample_plan": (i32, [i32, i32, POINTER(i32), POINTER(i32), POINTER(i32), POINTER(i32), POINTER(sz)]),
        "ou_resample_table": (i32, [i32, i32, vp, sz]),
        "ou_resample_length": (c_int64, [i32, i32, c_int64]),
        "ou_resample_tile": (i32, [i32, i32]),
        "ou_resample": (i32, [vp, c_int64, POINTER(c_int64), vp, c_int64, c_int64, i32, i32, i32, vp, sz, vp]),
        "ou_check_device_status": (i32, [vp, vp]),
        "ou_set_option": (i32, [vp, c_char_p, c_double]),
        "ou_get_option": (i32, [vp, c_char_p, POINTER(c_double)]),
        "ou_reset_options": (i32, [vp]),
        "ou_option_count": (i32, []),
        "ou_option_name": (c_char_p, [i32]),
        "ou_option_doc": (c_char_p, [i32]),
        "ou_option_default": (c_double, [i32]),
        "ou_set_stamp_layer": (i32, [vp, c_char_p]),
        "ou_plan_json": (c_char_p, [vp]),
        "ou_packer_plan_json": (c_char_p, [vp]),
        "ou_tensor": (i32, [vp, c_char_p, POINTER(sz), POINTER(i32), POINTER(i32)]),
        "ou_launch_stats": (i32, [vp, POINTER(i32), POINTER(i32)]),
        "ou_workspace_init": (i32, [vp, i32, i32, vp, sz, vp]),
        "ou_sampler_step": (i32, [vp, vp, vp, vp, c_float, c_float, sz, vp]),
        "ou_snake_act": (i32, [vp, vp, i32, i32, i32, c_int64, POINTER(i32), vp, vp, vp, vp, vp]),
        "ou_snake_tile": (i32, []),
        "ou_set_normalization": (i32, [vp, i32, i32, c_float]),
        "ou_set_gru_publish_mode": (i32, [vp, i32]),
        "ou_get_gru_publish_mode": (i32, [vp]),
        "ou_set_lanes": (i32, [vp, i32, i32]),
        "ou_set_lane_batch": (i32, [vp, i32]),
        "ou_lane_capacity": (i32, [vp, i32]),
        "ou_metrics_frames": (c_int64, [c_int64, i32]),
        "ou_metrics_scratch_bytes": (i32, [i32, c_int64, POINTER(MetricsSpec), i32, POINTER(sz)]),
        "ou_lsd": (i32, [vp, vp, c_int64, POINTER(c_int64), i32, POINTER(MetricsSpec), vp, vp, sz, vp]),
        "ou_spectral_mae": (i32, [vp, vp, c_int64, POINTER(c_int64), i32, POINTER(MetricsSpec), i32, c_float, c_float, i32, vp,
                                 vp, sz, vp]),
        "ou_si_sdr": (i32, [vp, vp, c_int64, POINTER(c_int64), i32, c_float, vp, vp, vp, sz, vp]),
        "ou_sdr_scratch_bytes": (i32, [i32, c_int64, i32, POINTER(sz)]),
        "ou_sdr": (i32, [vp, vp, c_int64, POINTER(c_int64), i32, i32, c_float, vp, vp, sz, vp]),
        "ou_stoi_scratch_bytes": (i32, [i32, c_int64, i32, POINTER(sz)]),
        "ou_stoi": (i32, [vp, vp, c_int64, POINTER(c_int64), i32, i32, i32, vp, vp, sz, vp]),
        "ou_stoi_frame_tile": (i32, []),
        "ou_transform_frames": (i32, [i32, i32, i32]),
        "ou_transform_forward": (i32, [vp, i32, i32, vp, i32, i32, i32, c_float, c_float, vp, vp]),
        "ou_transform_inverse": (i32, [vp, i32, i32, vp, i32, i32, i32, c_float, c_float, i32, vp, vp, vp]),
        "ou_flac_last_error": (c_char_p, []),
        "ou_flac_info": (i32, [vp, sz, POINTER(i32), POINTER(i32), POINTER(i32), POINTER(ctypes.c_int64), vp]),
        "ou_flac_decode": (i32, [vp, sz, vp, ctypes.c_int64, POINTER(ctypes.c_int64)]),
        "ou_flac_encode_sizes": (i32, [i32, POINTER(i32), POINTER(c_int64), i32, POINTER(sz), POINTER(c_int64), POINTER(sz),
                                       POINTER(c_int64)]),
        "ou_flac_encode_frames": (i32, [vp, c_int64, i32, POINTER(i32), POINTER(c_int64), i32, vp, sz, vp, vp, sz, vp]),
        "ou_flac_assemble": (i32, [vp, vp, vp, i32, POINTER(i32), POINTER(c_int64), i32, i32, vp, sz, POINTER(c_int64)]),
        "ou_flac_encode_choices_bytes": (i32, [i32, POINTER(i32), POINTER(c_int64), POINTER(sz)]),
        "ou_flac_encode_frames_level": (i32, [vp, c_int64, i32, POINTER(i32), POINTER(c_int64), i32, i32, vp, sz, vp, vp, sz, vp, sz,
                                              vp]),
        "ou_profile_enable": (i32, [vp, i32]),
        "ou_variant_family": (c_char_p, [i32]),
        "ou_bench_conv": (i32, [vp, c_char_p, i32, i32, i32, i32, i32, i32, vp, sz, vp, POINTER(c_float), POINTER(i32)]),
        "ou_profile_read": (i32, [vp, i32, POINTER(c_float), POINTER(c_double), POINTER(c_double), POINTER(i32), POINTER(i32)]),
        "ou_profile_read_ticks": (i32, [vp, i32, POINTER(ctypes.c_uint64), POINTER(ctypes.c_uint64), POINTER(i32), POINTER(i32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


EXPORTED_SYMBOLS = [
    "ou_version", "ou_last_error", "ou_packer_last_error", "ou_packer_create", "ou_packer_set", "ou_packer_finish",
    "ou_packer_destroy", "ou_packed_bytes", "ou_create", "ou_destroy", "ou_workspace_bytes", "ou_schedule",
    "ou_condition", "ou_score", "ou_aux_to_wav", "ou_enhance", "ou_enhance_var", "ou_check_device_status",
    "ou_segment_plan", "ou_segments_workspace_bytes", "ou_enhance_segments",
    "ou_segment_groups", "ou_segments_var_workspace_bytes", "ou_enhance_segments_var",
    "ou_ensemble_workspace_bytes", "ou_enhance_ensemble", "ou_ensemble_reduce_scratch_bytes", "ou_ensemble_reduce",
    "ou_segments_ensemble_workspace_bytes", "ou_enhance_segments_ensemble",
    "ou_segments_var_ensemble_workspace_bytes", "ou_enhance_segments_var_ensemble",
    "ou_set_noise_source", "ou_noise_scratch_bytes", "ou_noise_fill",
    "ou_stream_plan", "ou_stream_emitted", "ou_stream_workspace_bytes", "ou_stream_create", "ou_stream_destroy",
    "ou_stream_push", "ou_stream_flush",
    "ou_resample_plan", "ou_resample_table", "ou_resample_length", "ou_resample_tile", "ou_resample",
    "ou_snake_act", "ou_snake_tile", "ou_set_normalization",
    "ou_metrics_frames", "ou_metrics_scratch_bytes", "ou_lsd", "ou_spectral_mae", "ou_si_sdr",
    "ou_sdr_scratch_bytes", "ou_sdr", "ou_stoi_scratch_bytes", "ou_stoi", "ou_stoi_frame_tile",
    "ou_set_option", "ou_get_option", "ou_reset_options", "ou_option_count", "ou_option_name", "ou_option_doc", "ou_option_default", "ou_plan_json",
    "ou_packer_plan_json", "ou_tensor", "ou_launch_stats", "ou_workspace_init", "ou_sampler_step",
    "ou_set_gru_publish_mode", "ou_get_gru_publish_mode", "ou_set_lanes", "ou_set_lane_batch", "ou_lane_capacity",
    "ou_transform_frames", "ou_transform_forward", "ou_transform_inverse",
    "ou_flac_last_error", "ou_flac_info", "ou_flac_decode",
    "ou_flac_encode_sizes", "ou_flac_encode_frames", "ou_flac_assemble",
    "ou_flac_encode_choices_bytes", "ou_flac_encode_frames_level",
]
TUNING_SYMBOLS = ["ou_profile_enable", "ou_profile_read", "ou_profile_read_ticks", "ou_bench_conv", "ou_set_stamp_layer",
                  "ou_variant_family",
]

_EXC = {OU_EINVAL: ValueError, OU_ENOTIMPL: NotImplementedError, OU_EMISSING: KeyError, OU_ESHAPE: ValueError,
        OU_EHIP: RuntimeError, OU_ENOMEM: MemoryError, OU_ESYNC: RuntimeError}


def check(code, handle=None, packer=None):
    """Map a C status code to the exception type the reference raises for the same condition."""
    if code == OU_OK:
        return
    L = load()
    if packer is not None:
        msg = L.ou_packer_last_error(packer)
    else:
        msg = L.ou_last_error(handle)
    msg = msg.decode() if msg else f"libouniverse error {code}"
    raise _EXC.get(code, RuntimeError)(msg)


def option_names():
    """Keys of ou_set_option, with their one-line descriptions."""
    L = load()
    return {L.ou_option_name(i).decode(): L.ou_option_doc(i).decode() for i in range(L.ou_option_count())}


def option_defaults():
    L = load()
    return {L.ou_option_name(i).decode(): L.ou_option_default(i) for i in range(L.ou_option_count())}


def segment_plan(tot_ds, T_raw, segment, overlap):
    """The library's window plan of a segmented enhance (ou_segment_plan): dict of numpy arrays `starts`, `lengths`,
    `core_begin`, `core_end` (one entry per window) and the ints `overlap` (as used) and `T_pad`.  Pure host code."""
    import numpy as np

    L = load()
    n, ov, tp = c_int32(), c_int32(), c_int64()
    check(L.ou_segment_plan(int(tot_ds), int(T_raw), int(segment), int(overlap), 0, None, None, None, None, byref(n),
                            byref(ov), byref(tp)))
    k = n.value
    starts, ce0, ce1 = (c_int64 * k)(), (c_int64 * k)(), (c_int64 * k)()
    lens = (c_int32 * k)()
    check(L.ou_segment_plan(int(tot_ds), int(T_raw), int(segment), int(overlap), k, starts, lens, ce0, ce1, byref(n),
                            byref(ov), byref(tp)))
    return {"starts": np.ctypeslib.as_array(starts).copy(), "lengths": np.ctypeslib.as_array(lens).copy(),
            "core_begin": np.ctypeslib.as_array(ce0).copy(), "core_end": np.ctypeslib.as_array(ce1).copy(),
            "overlap": ov.value, "T_pad": tp.value}


def stream_plan(tot_ds, T, segment, overlap):
    """The library's window plan of a stream flushed after T samples (ou_stream_plan): the dict of `segment_plan`.  Pure host
    code."""
    import numpy as np

    L = load()
    n, ov, tp = c_int32(), c_int32(), c_int64()
    check(L.ou_stream_plan(int(tot_ds), int(T), int(segment), int(overlap), 0, None, None, None, None, byref(n), byref(ov),
                           byref(tp)))
    k = n.value
    starts, ce0, ce1 = (c_int64 * max(k, 1))(), (c_int64 * max(k, 1))(), (c_int64 * max(k, 1))()
    lens = (c_int32 * max(k, 1))()
    if k:
        check(L.ou_stream_plan(int(tot_ds), int(T), int(segment), int(overlap), k, starts, lens, ce0, ce1, byref(n), byref(ov),
                               byref(tp)))
    return {"starts": np.ctypeslib.as_array(starts)[:k].copy(), "lengths": np.ctypeslib.as_array(lens)[:k].copy(),
            "core_begin": np.ctypeslib.as_array(ce0)[:k].copy(), "core_end": np.ctypeslib.as_array(ce1)[:k].copy(),
            "overlap": ov.value, "T_pad": tp.value}


def stream_emitted(tot_ds, P, segment, overlap):
    """Samples per row a stream has emitted once P are pushed, before a flush (ou_stream_emitted).  Pure host code."""
    n = load().ou_stream_emitted(int(tot_ds), int(P), int(segment), int(overlap))
    if n < 0:
        check(OU_EINVAL)
    return n


def segment_groups(tot_ds, t_raw, segment, overlap, max_batch):
    """The library's window groups for rows of lengths `t_raw` (ou_segment_groups): dict of numpy arrays `row`, `window`,
    `length` (one entry per window: class FULL row-major, then class SHORT), `group_first`, `group_ragged` (one per group) and the
    ints `batch` and `length_max`.  Pure host code."""
    import numpy as np

    L = load()
    C = len(t_raw)
    tr = (c_int64 * max(C, 1))(*[int(v) for v in t_raw])
    ne, ng, b, ln = c_int32(), c_int32(), c_int32(), c_int32()
    args = (int(tot_ds), C, tr, int(segment), int(overlap), int(max_batch))
    check(L.ou_segment_groups(*args, 0, None, None, None, None, None, byref(ne), byref(ng), byref(b), byref(ln)))
    n = ne.value
    row, win, length, first, ragged = ((c_int32 * n)() for _ in range(5))
    check(L.ou_segment_groups(*args, n, row, win, length, first, ragged, byref(ne), byref(ng), byref(b), byref(ln)))
    as_np = lambda a, k: np.ctypeslib.as_array(a)[:k].copy()  # noqa: E731
    return {"row": as_np(row, n), "window": as_np(win, n), "length": as_np(length, n),
            "group_first": as_np(first, ng.value), "group_ragged": as_np(ragged, ng.value),
            "batch": b.value, "length_max": ln.value}


def segment_weights(plan, k):
    """Crossfade weight of window k over its own samples (float32), as the stitch applies it: a(i) = 0.5 - 0.5 cos(pi (i + 0.5)
    / O) over the crossfade [e_{k-1} - O, e_{k-1}) with the window in front (which gets 1 - a(i)), 1 on the rest of what the
    window writes, 0 on samples that a shifted last window covers but does not write."""
    import numpy as np

    s, n, O = plan["starts"], len(plan["starts"]), plan["overlap"]
    L = int(plan["lengths"][k])
    u = np.arange(s[k], s[k] + L, dtype=np.int64)
    w = np.zeros(L, dtype=np.float32)
    ramp = lambda i: (np.float32(0.5) - np.float32(0.5) * np.cos(
        np.float32(np.pi) * ((i.astype(np.float32) + np.float32(0.5)) / np.float32(O)))).astype(np.float32)
    w0 = 0 if k == 0 else s[k - 1] + L - O
    w1 = plan["T_pad"] if k == n - 1 else s[k] + L - O
    own = (u >= w0) & (u < w1)
    w[own] = 1.0
    if k > 0 and O > 0:
        m = own & (u < s[k - 1] + L)
        w[m] = ramp(u[m] - w0)
    if k < n - 1 and O > 0:
        m = u >= w1
        w[m] = np.float32(1.0) - ramp(u[m] - w1)
    return w


def resample_plan(fs_in, fs_out):
    """ou_resample_plan: dict of the ints `orig`, `new`, `width`, `taps`, `table_bytes` of a rate pair.  Pure host code."""
    L = load()
    o, n, w, t, nb = c_int32(), c_int32(), c_int32(), c_int32(), c_size_t()
    check(L.ou_resample_plan(int(fs_in), int(fs_out), byref(o), byref(n), byref(w), byref(t), byref(nb)))
    return {"orig": o.value, "new": n.value, "width": w.value, "taps": t.value, "table_bytes": nb.value}


def resample_table(fs_in, fs_out):
    """ou_resample_table as numpy arrays: (first (new,) int32, coef (taps, new) float32, the raw table as uint8).  Pure host code."""
    import numpy as np

    L = load()
    plan = resample_plan(fs_in, fs_out)
    raw = np.zeros(plan["table_bytes"], dtype=np.uint8)
    check(L.ou_resample_table(int(fs_in), int(fs_out), raw.ctypes.data_as(c_void_p), c_size_t(raw.nbytes)))
    n = plan["new"]
    return raw[:4 * n].view(np.int32), raw[4 * n:].view(np.float32).reshape(plan["taps"], n), raw


def norm_args(spec):
    """ModelSpec.norm / zero_mean / norm_eps -> the arguments of ou_set_normalization (mode, zero_mean, eps).  (0, 1, 0.0) is
    the handle's state after ou_create -- normalization_norm 2 with zero_mean, every shipped config -- and is never sent."""
    norm = str(spec.norm)
    if norm not in NORM_MODES:
        raise NotImplementedError(f"Norm {norm} is not implemented for batch normalization")  # utils/norm.py:41-43
    eps = float(spec.norm_eps)
    if not eps > 0.0:
        raise ValueError(f"normalization_kwargs.eps={eps!r} must be positive")
    # utils/norm.py:31-39 hands eps to the 2-max branch alone: the other two are sent 0 (= their 1e-5) whatever the key says
    return NORM_MODES[norm], 1 if spec.zero_mean else 0, eps if norm == "2-max" and eps != 1e-5 else 0.0


def make_config(spec, fir_fold=0, split_copy=True):
    """ModelSpec -> ou_config.  `fir_fold`, `split_copy`: packing choices (ou_config.fir_fold / .no_split_copy), the same for the
    packer and ou_create."""
    def net(n):
        c = NetConfig()
        c.n_rates = len(n.rate_factors)
        for i, r in enumerate(n.rate_factors):
            c.rate_factors[i] = int(r)
        c.n_channels = n.n_channels
        c.fb_kernel_size = n.fb_kernel_size
        c.n_rff = n.n_rff
        c.noise_cond_dim = n.noise_cond_dim
        c.extra_conv_block = int(n.extra_conv_block)
        c.use_weight_norm = int(n.use_weight_norm)
        c.use_antialiasing = int(n.use_antialiasing)
        c.time_embedding_simple = int(n.time_embedding == "simple")
        c.n_mels = n.n_mels
        c.n_mel_oversample = n.n_mel_oversample
        c.encoder_gru_residual = int(n.encoder_gru_residual)
        return c

    cfg = Config()
    cfg.abi_version = OU_ABI_VERSION
    cfg.kind = OU_KIND_UNIVERSE_GAN if spec.kind == "universe_gan" else OU_KIND_UNIVERSE
    cfg.fs = spec.fs
    cfg.level_db = spec.level_db
    cfg.has_edm = int(spec.edm_noise is not None)
    cfg.edm_noise = spec.edm_noise if spec.edm_noise is not None else 0.0
    cfg.sigma_min = spec.sigma_min
    cfg.sigma_max = spec.sigma_max
    cfg.use_signal_decoupling = int(spec.use_signal_decoupling)
    cfg.signal_decoupling_act = {"snake": OU_ACT_SNAKE, "prelu": OU_ACT_PRELU}.get(spec.signal_decoupling_act, OU_ACT_NONE)
    cfg.score = net(spec.score)
    cfg.cond = net(spec.cond)
    data_level = getattr(spec, "edm_data_level_db", None)
    cfg.has_edm_data_level = int(data_level is not None)
    cfg.edm_data_level_db = float(data_level) if data_level is not None else 0.0
    cfg.fir_fold = int(fir_fold)
    cfg.no_split_copy = 0 if split_copy else 1

    def body_act(n, key):
        v = getattr(n, key, "prelu")
        if v not in BODY_ACTS:
            raise ValueError(f"{key}={v!r}: 'act_type' should be one of [{' | '.join(BODY_ACTS)}]")
        return BODY_ACTS[v]

    cfg.score_enc_act = body_act(spec.score, "encoder_act_type")
    cfg.score_dec_act = body_act(spec.score, "decoder_act_type")
    cfg.cond_enc_act = body_act(spec.cond, "encoder_act_type")
    cfg.cond_dec_act = body_act(spec.cond, "decoder_act_type")
    # (ScoreNetwork has no encoder_gru_residual: in ou_config.score that slot says what sits in the encoder's bottleneck)
    seq = getattr(spec.score, "seq_model", "gru")
    if seq not in ("gru", "none"):
        raise NotImplementedError(f"score_model.seq_model={seq!r}: gru | none")
    sandwich = bool(getattr(spec.score, "encoder_gru_conv_sandwich", False))
    cfg.score.seq_bottleneck = OU_SEQ_NONE if seq == "none" else OU_SEQ_GRU_SANDWICH if sandwich else OU_SEQ_GRU
    norm_args(spec)  # (an unknown norm is refused here, where every other key is; the values travel by ou_set_normalization)
    return cfg


def pack_weights(spec, state_dict, fir_fold=0, split_copy=True):
    """Fold + lay out a reference-keyed state dict into the device blob (host side, no GPU needed).
    Returns (torch.FloatTensor blob [CPU], plan_json str)."""
    import numpy as np
    import torch

    L = load()
    cfg = make_config(spec, fir_fold, split_copy)
    packer = c_void_p()
    check(L.ou_packer_create(byref(cfg), byref(packer)))
    try:
        for key, t in state_dict.items():
            t = t.detach().to(torch.float32).cpu().contiguous()
            shape = (c_int64 * max(1, t.ndim))(*t.shape)
            check(L.ou_packer_set(packer, key.encode(), c_void_p(t.data_ptr()), shape, t.ndim), packer=packer)
        blob_p, nbytes = c_void_p(), c_size_t()
        check(L.ou_packer_finish(packer, byref(blob_p), byref(nbytes)), packer=packer)
        arr = np.ctypeslib.as_array(ctypes.cast(blob_p, POINTER(c_float)), shape=(nbytes.value // 4,))
        blob = torch.from_numpy(arr.copy())
        plan = L.ou_packer_plan_json(packer).decode()
    finally:
        L.ou_packer_destroy(packer)
    return blob, plan


def packed_bytes(spec, fir_fold=0, split_copy=True):
    L = load()
    cfg = make_config(spec, fir_fold, split_copy)
    n = c_size_t()
    check(L.ou_packed_bytes(byref(cfg), byref(n)))
    return n.value
