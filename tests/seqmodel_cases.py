"""Score networks with another bottleneck than the plain GRU (ScoreEncoder, score.py:81-123): `encoder_gru_conv_sandwich` (a ConvBlock
in front of the GRU and one behind it) and `seq_model: none` (no GRU).  Overrides of config.builtin_config, as narrow as the packer
allows: n_channels 8 over four levels gives OC = 128, hidden size 64.  tests/golden/make_golden_seqmodel.py records the real
reference on them, tests/test_seqmodel_cpu.py packs them, tests/test_gpu_seqmodel.py runs them.

Weights: state_dict.synthetic_state_dict(spec, SEED[case], GAIN[case])."""
import os

import numpy as np
import torch

from open_universe_amd import config as C
from open_universe_amd import state_dict as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES_JSON = os.path.join(GOLDEN, "seqmodel_names.json")
SANDWICH = {"score_model.encoder_gru_conv_sandwich": True}
NONE = {"score_model.seq_model": "none"}
NARROW = {"score_model.n_channels": 8}
# name -> (base configuration, overrides, what it is for)
CASES = {
    "sand_pp": ("PP16", dict(NARROW, **SANDWICH),
                "extra_conv_block true: the un-fused residual in front of decoder block 0"),
    "sand_or": ("OR16", dict(NARROW, **SANDWICH, **{"score_model.extra_conv_block": False}),
                "decoder block 0 with a rate change; RFF embedding"),
    "none_pp": ("PP16", dict(NARROW, **NONE), "residual with no GRU to carry it"),
    "none_or": ("OR16", dict(NARROW, **NONE, **{"score_model.extra_conv_block": False}), "the shortest walk"),
    "sand_snake": ("PP16", dict(NARROW, **SANDWICH, **{"score_model.encoder_act_type": "snake"}),
                   "a Snake launch in front of the convs of cb1 / cb2"),
}
SAND = tuple(c for c in CASES if c.startswith("sand"))
NONES = tuple(c for c in CASES if c.startswith("none"))
# keys builtin_config mirrors into the conditioner (the reference's yaml has to be told the same)
MIRRORED = ("rate_factors", "n_channels", "extra_conv_block", "use_weight_norm", "fb_kernel_size")
REFERENCE_YAML = {"PP16": "default", "OR16": "universe_original"}
SEED = {c: 17 for c in CASES}
# (see tests/snake_cases.py: the recipe's gain 1.0 is tuned for PReLU; Snake layers need 0.6 for the reference to agree with itself)
GAIN = {c: (0.6 if c == "sand_snake" else 1.0) for c in CASES}
N_STEPS = 3
B = 2
FILE_LENGTHS = (2731, 1600, 977)  # a ragged length, a multiple of tot_ds, a short one
NOISE_SEED = 41
# (frames, batch): T = frames * tot_ds -- a sub-tile row, an odd row, more than one tile
SHAPES = ((1, 1), (3, 3), (13, 3))
RAGGED_ROWS = (13, 4, 1)  # frames per row; samples: frames * tot_ds - 3


def config_of(case):
    base, over, _ = CASES[case]
    return C.builtin_config(base, **over)


def spec_of(case):
    return C.spec_from_config(config_of(case))


def state_dict_of(case):
    return S.synthetic_state_dict(spec_of(case), seed=SEED[case], gain=GAIN[case])


def reference_overrides(case):
    """The overrides of a case for the reference's own yaml (oracle/ref_import.build_reference_model)."""
    out = {}
    for k, v in CASES[case][1].items():
        out[k] = v
        if k.startswith("score_model.") and k.split(".", 1)[1] in MIRRORED:
            out[k.replace("score_model", "condition_model")] = v
    return out


def batch_length(spec):
    return spec.tot_ds * 16 + 37


def golden_path(case):
    return os.path.join(GOLDEN, f"seqmodel_{case}.npz")


def load_golden(case):
    return np.load(golden_path(case))


def noise_planes(seed, n, rows, T):
    """n planes (rows, 1, T) of N(0, 1), drawn plane by plane from one CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(rows, 1, T, generator=g) for _ in range(n)]
