"""The measuring stick of the resampler tests: a float64 evaluation of the definition in include/ouniverse.h ("resampling"),
written in numpy over the DENSE kernel.  It shares no code with audio.py or the library.

    g = gcd(fs_in, fs_out), orig = fs_in / g, new = fs_out / g, base = min(orig, new) * 0.99, width = ceil(6 * orig / base)
    y[j] = sum_i k[p][i] * x[f * orig - width + i],  i in [0, 2 * width + orig),  f = j // new, p = j % new, j < ceil(new n / orig)
    k[p][i]: float64, rounded once to fp32
"""
import math

import numpy as np

PAIRS = [(44100, 16000), (16000, 44100), (48000, 16000), (16000, 48000), (22050, 24000), (8000, 16000), (96000, 16000),
         (16000, 16001)]


def geometry(fs_in, fs_out):
    g = math.gcd(fs_in, fs_out)
    orig, new = fs_in // g, fs_out // g
    base = min(orig, new) * 0.99
    return orig, new, base, int(math.ceil(6 * orig / base))


def argument(fs_in, fs_out, phases):
    """The unclamped window argument (-p / new + (i - width) / orig) * base of the rows `phases` of the dense kernel."""
    orig, new, base, width = geometry(fs_in, fs_out)
    i = np.arange(2 * width + orig, dtype=np.float64)
    p = np.asarray(phases, dtype=np.float64)[:, None]
    return (-p / new + (i[None, :] - width) / orig) * base


def dense_rows(fs_in, fs_out, phases):
    """Rows `phases` of the dense kernel: float64, rounded once to fp32 (returned as float64 again)."""
    orig, new, base, width = geometry(fs_in, fs_out)
    t = np.clip(argument(fs_in, fs_out, phases), -6.0, 6.0)
    window = np.cos(t * math.pi / 6 / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(t == 0, 1.0, np.sin(t) / t) * window * (base / orig)
    return k.astype(np.float32).astype(np.float64)


def out_length(fs_in, fs_out, n):
    orig, new, _, _ = geometry(fs_in, fs_out)
    return -((-new * n) // orig)


def resample64(x, fs_in, fs_out):
    """x: (n,) -> (ceil(new n / orig),) float64"""
    x = np.asarray(x, dtype=np.float64)
    orig, new, base, width = geometry(fs_in, fs_out)
    n = x.shape[0]
    J = out_length(fs_in, fs_out, n)
    L = 2 * width + orig
    j = np.arange(J)
    f, p = j // new, j % new
    phases = np.unique(p)
    k = dense_rows(fs_in, fs_out, phases)                      # (phases, L)
    row = np.searchsorted(phases, p)
    xp = np.zeros(width + (int(f.max()) + 1 if J else 0) * orig + L + n, dtype=np.float64)
    xp[width:width + n] = x
    y = np.empty(J, dtype=np.float64)
    step = max(1, (1 << 22) // L)
    for a in range(0, J, step):                                 # windows of the padded row, a slab at a time
        b = min(J, a + step)
        idx = (f[a:b] * orig)[:, None] + np.arange(L)[None, :]
        y[a:b] = np.einsum("jl,jl->j", k[row[a:b]], xp[idx])
    return y


def snr_db(ref, est):
    ref = np.asarray(ref, dtype=np.float64)
    err = ref - np.asarray(est, dtype=np.float64)
    den = float((err ** 2).sum())
    return float("inf") if den == 0.0 else 10.0 * math.log10(float((ref ** 2).sum()) / den)


def noise_rows(rows, n, seed):
    """`rows` rows of Gaussian noise at 0.1 RMS, float32"""
    return (0.1 * np.random.default_rng(seed).standard_normal((rows, n))).astype(np.float32)
