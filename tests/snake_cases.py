"""The narrow models with non-PReLU ConvBlock activations that tests/golden/make_golden_snake.py records the real reference on
and tests/test_gpu_snake_parity.py runs: PP16s (UNIVERSE++ 16 kHz at n_channels = 8, the model of the small goldens) with
encoder_act_type / decoder_act_type turned."""
import os

import numpy as np
import torch

from open_universe_amd import config as C
from open_universe_amd import state_dict as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BASE = {"score_model.n_channels": 8}
CASES = {
    # score encoder + decoder snake
    "snake": {"score_model.encoder_act_type": "snake", "score_model.decoder_act_type": "snake"},
    # score snakebeta with conditioner snake
    "snakebeta": {"score_model.encoder_act_type": "snakebeta", "score_model.decoder_act_type": "snakebeta",
                  "condition_model.encoder_act_type": "snake", "condition_model.decoder_act_type": "snake"},
    # mixed: encoder none, decoder prelu
    "mixed": {"score_model.encoder_act_type": "none", "score_model.decoder_act_type": "prelu"},
}
SEED = 3          # of the synthetic weights
# Gain of the synthetic weight-norm gains (state_dict.synthetic_state_dict).  The recipe's 1.0 is tuned for PReLU, which shrinks
# what it passes; Snake adds a non-negative sin^2 / beta to it, and at gain 1.0 the activations of these models grow to 1e3 ..
# 1e5 -- sines of such arguments are ill-conditioned, and the REFERENCE run in fp32 then agrees with the reference run in float64
# to 21 dB only (snakebeta; 42 dB at gain 0.8).  At 0.6 the activations reach 3 .. 5 (sine arguments up to ~25 rad: well inside
# the non-linear regime) and the reference agrees with itself to 92 .. 104 dB; every fixture records that figure (`self_db`).
GAIN = {"snake": 0.6, "snakebeta": 0.6, "mixed": 1.0}
N_STEPS = 3
B = 2
FILE_LENGTHS = (2731, 1600, 977)  # the three files of the ragged call: a ragged length, a multiple of tot_ds, a short one
NOISE_SEED = 29


def overrides(case):
    return dict(BASE, **CASES[case])


def spec_of(case):
    return C.spec_from_config(C.builtin_config("PP16", **overrides(case)))


def state_dict_of(case):
    """The seeded synthetic weights of a case (a recipe: state_dict.synthetic_state_dict draws the Snake parameters from a
    spread of log-scale values)."""
    return S.synthetic_state_dict(spec_of(case), seed=SEED, gain=GAIN[case])


def batch_length(spec):
    return spec.tot_ds * 16 + 37


def golden_path(case):
    return os.path.join(GOLDEN, f"snake_{case}.npz")


def load_golden(case):
    return np.load(golden_path(case))


def noise_planes(seed, n, rows, T):
    """n planes (rows, 1, T) of N(0, 1), drawn plane by plane from one CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(rows, 1, T, generator=g) for _ in range(n)]
