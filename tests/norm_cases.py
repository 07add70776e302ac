"""The level-normalisation cases (normalization_norm max | 2-max, zero_mean false) that tests/golden/make_golden_norm.py records
the real reference on and tests/test_norm_cpu.py / tests/test_gpu_norm.py run, their inputs, and the float64 restatement of
utils/norm.py the statistics are held against."""
import math
import os

import numpy as np
import torch

from helpers import SMALL, synth_mix
from open_universe_amd import config as C
from open_universe_amd import state_dict as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = ("PP16s", "OR16s")
# mode -> overrides of the model yaml
MODES = {
    "max": {"normalization_norm": "max"},
    "2max": {"normalization_norm": "2-max"},
    "keepmean": {"normalization_norm": 2, "normalization_kwargs.zero_mean": False},
    "max_keepmean": {"normalization_norm": "max", "normalization_kwargs.zero_mean": False},
    "2max_keepmean": {"normalization_norm": "2-max", "normalization_kwargs.zero_mean": False},
    "2max_eps": {"normalization_norm": "2-max", "normalization_kwargs.eps": 1e-3},
}
# mode -> (norm, zero_mean, eps) as ModelSpec holds them
MODE_ARGS = {"max": ("max", True, 1e-5), "2max": ("2-max", True, 1e-5), "keepmean": ("2", False, 1e-5),
             "max_keepmean": ("max", False, 1e-5), "2max_keepmean": ("2-max", False, 1e-5), "2max_eps": ("2-max", True, 1e-3)}
CASES = [(m, mode) for m in MODELS for mode in MODES]
SEED = 0          # of the synthetic weights
N_STEPS = 3
B = 2             # rows of the batch; 2max_eps has a third, the quiet row (batch_rows)
FILE_LENGTHS = (2731, 1600, 977)  # a ragged length, a multiple of tot_ds, a short one; file 1 carries the spike
NOISE_SEED = 41
DC = 0.02         # offset of every input: what zero_mean false leaves in the row
SPIKE = 60.0      # the spike, in standard deviations of the smooth signal: crest factor 60 / sqrt(1 + 3600 / T) > 1 / level = 20


def overrides(model, mode):
    return dict(SMALL[model][1], **MODES[mode])


def config_of(model, mode):
    return C.builtin_config(SMALL[model][0], **overrides(model, mode))


def spec_of(model, mode):
    return C.spec_from_config(config_of(model, mode))


def state_dict_of(model, mode):
    return S.synthetic_state_dict(spec_of(model, mode), seed=SEED)


def batch_length(spec):
    return spec.tot_ds * 16 + 37


def golden_path(model, mode):
    return os.path.join(GOLDEN, f"norm_{model}_{mode}.npz")


def load_golden(model, mode):
    return np.load(golden_path(model, mode))


def noise_planes(seed, n, rows, T):
    """n planes (rows, 1, T) of N(0, 1), drawn plane by plane from one CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(rows, 1, T, generator=g) for _ in range(n)]


def with_spike(x, at):
    """Row x (T,) with ONE sample at `at` raised to SPIKE standard deviations of the row."""
    x = x.clone()
    x[at] = SPIKE * float(x.double().std())
    return x


def batch_rows(mode):
    return B + 1 if mode == "2max_eps" else B


def batch_mix(spec, mode=None):
    """(B, T): row 0 smooth (2-max takes its std branch), row 1 with one spike (2-max takes its max branch), both on a DC offset.
    Mode 2max_eps: a third row, the quiet one (quiet_row: sd above 1e-5, mx below the mode's eps 1e-3 -- the row on which
    normalization_kwargs.eps decides the gain)."""
    T = batch_length(spec)
    mix = synth_mix(spec, B, T) + DC
    mix[1] = with_spike(mix[1], T // 3)
    if mode == "2max_eps":
        mix = torch.cat([mix, quiet_row(spec, T)[None, :]])
    return mix


QUIET = 2e-3      # scale of the quiet row: synth_mix has sd 0.05 and peak 0.2 -> sd about 1e-4, mx about 4e-4


def quiet_row(spec, T, seed=77):
    """A smooth row without offset whose sd lies above the 1e-5 clamp and whose maximum below an eps of 1e-3."""
    return synth_mix(spec, 1, T, seed=seed)[0] * QUIET


def file_mix(spec, i):
    x = synth_mix(spec, 1, FILE_LENGTHS[i], seed=2000 + i) + DC
    if i == 1:
        x[0] = with_spike(x[0], FILE_LENGTHS[i] - 7)
    return x


# ---- utils/norm.py in float64 ---------------------------------------------------------------------------------------------
def padded(x, tot_ds):
    """universe.py:219-223: the row (T,) between pad // 2 zeros in front and the rest behind, pad = tot_ds - T % tot_ds."""
    T = x.shape[-1]
    pad = tot_ds - T % tot_ds
    return torch.nn.functional.pad(x, (pad // 2, pad - pad // 2))


def norm_stats(xp, norm, level_db, zero_mean=True, eps=1e-5):
    """normalize_batch (utils/norm.py:47-87) of ONE padded row `xp` (T_pad,), every operation in float64: -> dict of
    mean (what is removed: 0 with zero_mean false), sd (unbiased, around the row's own mean, unclamped), mx (max |x - mean|,
    unclamped), gain, branch ("std" | "max": which norm set the gain).  eps reaches the 2-max branch alone, as in the reference."""
    x = xp.double()
    level = 10.0 ** (level_db / 20.0)
    mean = float(x.mean()) if zero_mean else 0.0
    d = x - mean
    sd = float(d.std()) if d.numel() > 1 else float("nan")
    mx = float(d.abs().max())
    if norm == "2":
        gain, branch = level / max(sd, 1e-5), "std"
    elif norm == "max":
        gain, branch = level / max(mx, 1e-5), "max"
    elif norm == "2-max":
        g2, gm = level / max(sd, eps), 1.0 / max(mx, eps)
        gain, branch = (g2, "std") if g2 <= gm else (gm, "max")
    else:
        raise NotImplementedError(f"Norm {norm} is not implemented for batch normalization")
    return {"mean": mean, "sd": sd, "mx": mx, "gain": gain, "branch": branch, "level": level}


U = 2.0 ** -24  # unit roundoff of fp32


def stats_bounds(xp, st, norm, zero_mean):
    """What the device's fp32 (mean, gain) may differ from `st` = norm_stats(xp, ..) by.  The sums run in double on the device
    (n 2^-53: nothing against u), so what is left is the rounding of a few fp32 scalars, as tests/small_fp64.py derives it for
    pad_normalize_kernel:
      mean   one rounding of the double mean: u |mean|  (+ 1/2 ulp of the result is that same rounding: 2 u |mean| in all)
      sd     d = fl(x - mean_f) carries u |d| + u |mean|; in l2 the relative error of sd is at most u + 1.01 u |mean| / sd;
             (float) sd: u; the division level / sd: u               -> rho_sd  = 3 u + 1.01 u |mean| / sd  (relative, of the gain)
      mx     the fp32 maximum of fl(x - mean_f): one rounding u mx and the mean's u |mean|; the division: u
                                                                      -> rho_max = 2 u + 1.01 u |mean| / mx
    fl(level) itself is one more u in both.  A clamped norm (all-zero row) has the gain exactly fl(level) / fl(eps): u from the
    division, u from each constant.  -> (bound on |mean|, relative bound on the gain)"""
    am = abs(float(xp.double().mean()))  # (with zero_mean false the device still forms the mean: sd is taken around it)
    b_mean = 2 * U * abs(st["mean"]) if zero_mean else 0.0
    rho_sd = 4 * U + 1.01 * U * am / max(st["sd"], 1e-30) if st["sd"] == st["sd"] else 4 * U
    rho_mx = 3 * U + 1.01 * U * (am if zero_mean else 0.0) / max(st["mx"], 1e-30)
    if norm == "2":
        rho = rho_sd if st["sd"] > 1e-5 else 3 * U
    elif norm == "max":
        rho = rho_mx if st["mx"] > 1e-5 else 3 * U
    else:
        rho = max(rho_sd, rho_mx)  # (whichever branch the device took within rounding of a tie, it is within the larger)
        if st["sd"] <= 1e-5 or st["mx"] <= 1e-5:
            rho = max(rho, 3 * U)
    return b_mean, rho


def exact_max(x_raw, T_pad, mean_f):
    """The maximum the device must hold bit for bit: max |fl32(x - mean_f)| over the raw samples and, where the row is padded,
    |fl32(0 - mean_f)| (numpy float32 arithmetic; `mean_f` = the fp32 value the device removed)."""
    m = np.float32(mean_f)
    v = np.abs(x_raw.numpy().astype(np.float32) - m).max() if x_raw.numel() else np.float32(0)
    if T_pad > x_raw.numel():
        v = max(v, np.abs(np.float32(0) - m))
    return np.float32(v)


def gain32(norm, level_db, sd32, mx32, eps=1e-5):
    """NormMode::gain in numpy float32: every operation rounded once, as on the device."""
    f = np.float32
    level = f(10.0 ** (level_db / 20.0))
    if norm == "max":
        return level / max(f(mx32), f(1e-5))
    if norm == "2-max":
        return min(level / max(f(sd32), f(eps)), f(1) / max(f(mx32), f(eps)))
    return level / max(f(sd32), f(1e-5))


def undetermined(st, norm, rho, eps=1e-5):
    """Why rounding, not the input, would decide the gain of the row with the float64 statistics `st` (norm_stats) on a device
    that forms them within the relative `rho` of stats_bounds -- or None.  A norm within rho of its clamp (1e-5; eps under
    2-max) may or may not be clamped; under 2-max two candidate gains within rho of each other leave the branch open."""
    c = eps if norm == "2-max" else 1e-5
    if norm in ("2", "2-max") and abs(st["sd"] - c) <= rho * c:
        return f"sd {st['sd']!r} within {rho:.2e} of its clamp {c!r}"
    if norm in ("max", "2-max") and abs(st["mx"] - c) <= rho * c:
        return f"mx {st['mx']!r} within {rho:.2e} of its clamp {c!r}"
    if norm == "2-max":
        g2, gm = st["level"] / max(st["sd"], eps), 1.0 / max(st["mx"], eps)
        if abs(g2 - gm) <= rho * max(g2, gm):
            return f"level / sd = {g2!r} and 1 / mx = {gm!r} within {rho:.2e} of each other"
    return None


# ---- the rows the element tests hold (tests/test_norm_cpu.py, tests/test_gpu_norm_fp64.py) ---------------------------------------
ALL_MODES = [(n, z) for n in ("2", "max", "2-max") for z in (True, False)]   # every (norm, zero_mean) of ou_set_normalization
ROW_KINDS = ("smooth", "spike0", "spike_last", "spike_1029", "zero", "const", "quiet")
EDGE = 1024 + 5   # the third spike: past the first 1024 samples, thread 5's second sample


def mode_overrides(model, norm, zero_mean, eps=None):
    ov = dict(SMALL[model][1], **{"normalization_norm": int(norm) if norm == "2" else norm,
                                   "normalization_kwargs.zero_mean": bool(zero_mean)})
    if eps is not None:
        ov["normalization_kwargs.eps"] = eps
    return ov


def mode_spec(model, norm, zero_mean, eps=None):
    return C.spec_from_config(C.builtin_config(SMALL[model][0], **mode_overrides(model, norm, zero_mean, eps)))


def lengths(td):
    """pad_normalize_kernel's register window from one sample to its end (65 536), the first length of its loops, and both
    sides of a multiple of tot_ds."""
    return {"1": 1, "td-1": td - 1, "td": td, "td+1": td + 1, "65536": 65536, "65537": 65537}


def element_rows(spec, T):
    """{kind: row (T,)} of the kinds that exist at T samples: a smooth row on the DC offset; that row with the spike at the
    first sample, the last, and past the 1024th (needs T > 1029; a spike needs a standard deviation to be measured in: T > 3);
    all zero; the constant DC alone; the quiet row."""
    base = synth_mix(spec, 1, T, seed=77)[0] + DC
    rows = {"smooth": base}
    if T > 3:
        rows["spike0"] = with_spike(base, 0)
        rows["spike_last"] = with_spike(base, T - 1)
    if T > EDGE:
        rows["spike_1029"] = with_spike(base, EDGE)
    rows["zero"] = torch.zeros(T)
    rows["const"] = torch.full((T,), DC)
    rows["quiet"] = quiet_row(spec, T)
    return rows


def crest_needed(level_db):
    return 1.0 / 10.0 ** (level_db / 20.0)


assert SPIKE / math.sqrt(1 + SPIKE ** 2 / min(FILE_LENGTHS)) > crest_needed(-26.0)
