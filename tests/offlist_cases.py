"""Topologies the library accepts (build_model, ou_model.cpp) that no shipped configuration has: overrides of
config.builtin_config, as narrow as the packer allows (the GRU's hidden size OC / 2 = n_channels 2^n / 2 has to be a multiple of
64, so OC = 128: n_channels 64 / 32 / 16 / 8 over 1 / 2 / 3 / 4 levels).  tests/test_offlist_cpu.py packs every case and holds the
coverage of BRANCHES; tests/test_gpu_offlist.py runs them on the GPU against the float64 references.

Every case names the branches it is there for; `branches_of(spec, base)` evaluates the same names from the spec alone, and the CPU
test asserts that every claim follows from the spec and that the union of the claims is BRANCHES.  Weights:
state_dict.synthetic_state_dict(spec, SEED)."""
from open_universe_amd import config as C
from open_universe_amd import state_dict as S

SEED = 11
FIR4_TAPS = (5, 7, 9, 11, 17)          # fir4_kernel<NT> instantiations of launch_fir (ou_small.hip)
LISTED_RATES = (2, 3, 4, 5, 8)         # up / stride with a fused up-FIR form, a conv_direct3s store form (the shipped factors)
SHIPPED_MEL = ((80, 4), (128, 4))      # (n_mels, n_mel_oversample)

# branch -> what it brings up (the issue's list)
BRANCHES = {
    "fir_scalar_13": "fir_kernel (scalar form) with 13 taps: rate factor 6, anti-aliased, both paths",
    "fir_scalar_15": "fir_kernel (scalar form) with 15 taps: rate factor 7, anti-aliased, both paths",
    "rate_6": "up / stride 6 in every conv family's plan function",
    "rate_7": "up / stride 7 in every conv family's plan function",
    "rate_67_tot_ds_4": "a 6 and a 7 in a model whose tot_ds is a multiple of 4: the only new thing is the rate",
    "tot_ds_odd": "tot_ds % 4 != 0: whole rows of odd length, row starts off 16 bytes, out_conv's scalar path",
    "tot_ds_odd_pp_aa": "tot_ds % 4 != 0 on UNIVERSE++ weights with anti-aliasing",
    "tot_ds_odd_or": "tot_ds % 4 != 0 on the original UNIVERSE",
    "tot_ds_2_mod_4_rate_small": "tot_ds % 4 == 2 with a first factor 2 at 32 / 48 channels: rate_up_kernel's scalar store loop and "
                                 "rate_down_kernel's loads on rows that start 8 bytes off a 16-byte boundary, with and without FIR",
    "kw_1": "in_conv / out_conv with fb_kernel_size 1",
    "kw_5": "in_conv / out_conv with fb_kernel_size 5",
    "kw_7": "in_conv / out_conv with fb_kernel_size 7",
    "kw_wide_tot_ds_odd": "fb_kernel_size 5 or 7 with tot_ds % 4 != 0: out_conv's scalar path with a wide kernel",
    "film_d_64": "film_kernel / sigma_embed_kernel (simple) with noise_cond_dim 64: D / 64 = 1",
    "film_d_1024": "film_kernel / sigma_embed_kernel (simple) with noise_cond_dim 1024: D / 64 = 16",
    "rff_other": "sigma_embed_kernel's random-Fourier-feature MLP with n_rff != 32",
    "aa_off_pp": "use_antialiasing false on a UNIVERSE++ model: fir_mode 0 on every level",
    "rates_1": "one rate factor: no st conv, sum_kernel with 2 operands",
    "rates_2": "two rate factors: one st conv, sum_kernel with 3 operands",
    "rates_3": "three rate factors: sum_kernel with 4 operands, widths 16 -> 128",
    "extra_conv_block_flipped": "extra_conv_block against the base configuration's value",
    "mel_other": "n_mels / n_mel_oversample other than the shipped pairs",
}

# name -> (base configuration, overrides, claimed branches)
CASES = {
    "r67": ("PP16", {"score_model.rate_factors": [2, 6, 7], "score_model.n_channels": 16},
            ("fir_scalar_13", "fir_scalar_15", "rate_6", "rate_7", "rate_67_tot_ds_4", "rates_3")),
    "odd_pp": ("PP16", {"score_model.rate_factors": [7, 3], "score_model.n_channels": 32, "score_model.fb_kernel_size": 5},
               ("tot_ds_odd", "tot_ds_odd_pp_aa", "kw_5", "kw_wide_tot_ds_odd", "fir_scalar_15", "rate_7", "rates_2")),
    # (rate_down_kernel / rate_up_kernel are built for R = 2 at 32 -> 64 and 48 -> 96 channels only: the outermost level of this
    # model, anti-aliased in the score network and plain in the conditioner; T = 14, 42, 182: all 2 modulo 4)
    "r27": ("PP16", {"score_model.rate_factors": [2, 7], "score_model.n_channels": 32},
            ("tot_ds_odd", "tot_ds_odd_pp_aa", "tot_ds_2_mod_4_rate_small", "fir_scalar_15", "rate_7", "rates_2")),
    "odd_or": ("OR16", {"score_model.rate_factors": [3, 7, 3], "score_model.n_channels": 16, "score_model.n_rff": 16,
                        "score_model.extra_conv_block": False},
               ("tot_ds_odd", "tot_ds_odd_or", "rff_other", "rate_7", "rates_3", "extra_conv_block_flipped")),
    "one": ("PP16", {"score_model.rate_factors": [4], "score_model.n_channels": 64, "score_model.fb_kernel_size": 1,
                     "condition_model.n_mels": 16, "condition_model.n_mel_oversample": 8},
            ("rates_1", "kw_1", "mel_other")),
    "kw7": ("PP16", {"score_model.n_channels": 8, "score_model.fb_kernel_size": 7, "score_model.noise_cond_dim": 64,
                     "score_model.use_antialiasing": False},
            ("kw_7", "film_d_64", "aa_off_pp")),
    "d1024": ("PP24", {"score_model.n_channels": 8, "score_model.noise_cond_dim": 1024, "score_model.extra_conv_block": False,
                       "condition_model.n_mels": 64, "condition_model.n_mel_oversample": 2},
              ("film_d_1024", "extra_conv_block_flipped", "mel_other")),
}
ODD = ("odd_pp", "odd_or", "r27")             # tot_ds % 4 != 0 (21, 63: odd; 14: 2 modulo 4)
RAGGED = ("odd_pp", "odd_or", "r27", "r67")   # ragged batches
OPTION_CASES = ("r67", "odd_pp", "r27")       # repeated under the option sets that pick another rate-change family
RATE_SMALL = ("r27",)                         # cases whose outermost level rate_down_kernel / rate_up_kernel take by default
RATE_SMALL_SHAPES = ((2, 32), (2, 48))        # (first rate factor, n_channels) those kernels are built for (ou_conv_chain.hip)
# (frames, batch): T = frames * tot_ds -- a sub-tile row, an odd row, more than one tile
SHAPES = ((1, 1), (3, 3), (13, 1), (13, 3))
RAGGED_ROWS = (13, 4, 1)               # frames per row; samples: frames * tot_ds - 3


def config_of(case):
    base, over, _ = CASES[case]
    return C.builtin_config(base, **over)


def spec_of(case):
    return C.spec_from_config(config_of(case))


def base_spec_of(case):
    return C.spec_from_config(C.builtin_config(CASES[case][0]))


def state_dict_of(case):
    return S.synthetic_state_dict(spec_of(case), seed=SEED)


def branches_of(spec, base):
    """The branches of BRANCHES a model of `spec` reaches, from the spec alone (`base`: the spec of the base configuration)."""
    s, c = spec.score, spec.cond
    out = set()
    rates = list(s.rate_factors)
    odd = spec.tot_ds % 4 != 0
    for r in rates:
        if r not in LISTED_RATES:
            out.add(f"rate_{r}")
            if s.use_antialiasing and 2 * r + 1 not in FIR4_TAPS:
                out.add(f"fir_scalar_{2 * r + 1}")
    if 6 in rates and 7 in rates and not odd and s.use_antialiasing:
        out.add("rate_67_tot_ds_4")
    if odd:
        out.add("tot_ds_odd")
        if spec.kind == "universe_gan" and s.use_antialiasing:
            out.add("tot_ds_odd_pp_aa")
        if spec.kind == "universe":
            out.add("tot_ds_odd_or")
        if s.fb_kernel_size >= 5:
            out.add("kw_wide_tot_ds_odd")
        if spec.tot_ds % 4 == 2 and (rates[0], s.n_channels) in RATE_SMALL_SHAPES:
            out.add("tot_ds_2_mod_4_rate_small")
    if s.fb_kernel_size != 3:
        out.add(f"kw_{s.fb_kernel_size}")
    if s.time_embedding == "simple" and s.noise_cond_dim // 64 != 8:
        out.add(f"film_d_{s.noise_cond_dim}")
    if s.time_embedding != "simple" and s.n_rff != 32:
        out.add("rff_other")
    if spec.kind == "universe_gan" and not s.use_antialiasing:
        out.add("aa_off_pp")
    if len(rates) + 1 != 5:  # (sum_kernel's operands: the mel block, n - 1 st convs, the encoder's output)
        out.add(f"rates_{len(rates)}")
    if bool(s.extra_conv_block) != bool(base.score.extra_conv_block):
        out.add("extra_conv_block_flipped")
    if (c.n_mels, c.n_mel_oversample) not in SHIPPED_MEL:
        out.add("mel_other")
    return out
