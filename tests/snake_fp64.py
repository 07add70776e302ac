"""float64 restatement of ou_snake_act (include/ouniverse.h, "alias-free Snake activation") and the cases its GPU test runs.

The restatement is numpy, written from the definition in the header -- two dense FIRs around the Snake non-linearity -- and
shares no code with the kernel.  tests/test_snake_cpu.py holds it against the reference's own Activation1d(Snake / SnakeBeta)
(through oracle/ref_import.py) on exactly these inputs, and tests/golden/make_golden_snake.py records how far the reference's
fp32 evaluation is from it: tests/golden/snake_fp64_ref_error.json.  The kernel's allowance (test_gpu_snake_fp64.py) is 4 x
that figure, per tensor, relative to the largest output magnitude of the tensor.
"""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ERROR_JSON = os.path.join(HERE, "golden", "snake_fp64_ref_error.json")
KERNEL_FACTOR = 4.0  # the kernel may be this many times further from float64 than the reference's own fp32 evaluation


def sinc_kernel(orig, new):
    """torchaudio's sinc_interp_hann kernel (lowpass_filter_width 6, rolloff 0.99) for orig -> new, float64 rounded once to
    float32 as the reference's buffer is: (new, 2 width + orig) and width."""
    base = min(orig, new) * 0.99
    width = math.ceil(6 * orig / base)
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = (np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx) * base
    t = np.clip(t, -6.0, 6.0)
    window = np.cos(t * math.pi / 6 / 2) ** 2
    t = t * math.pi
    k = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t))
    return (k * (window * (base / orig))).astype(np.float32), width


UP_K, UP_W = sinc_kernel(1, 2)      # (2, 15), 7
DOWN_K, DOWN_W = sinc_kernel(2, 1)  # (1, 28), 13


def snake_act(x, ea, eb=None, lens=None, up=UP_K, down=DOWN_K):
    """y[b, c, t] of ou_snake_act in float64.  x: (B, C, T); ea, eb: (C,) = exp(alpha), exp(beta) (eb None: eb = ea);
    lens: None or B lengths -- row b is the call on x[b, :, :lens[b]] alone, zero behind."""
    x = np.asarray(x, dtype=np.float64)
    B, C, T = x.shape
    up = np.asarray(up, dtype=np.float64).reshape(2, 15)
    down = np.asarray(down, dtype=np.float64).reshape(28)
    a = np.asarray(ea, dtype=np.float64)[:, None]
    bsum = np.asarray(ea if eb is None else eb, dtype=np.float64)[:, None] + 1e-9
    y = np.zeros((B, C, T), dtype=np.float64)
    for b in range(B):
        n = T if lens is None else int(lens[b])
        if n == 0:
            continue
        xp = np.zeros((C, n + 14), dtype=np.float64)
        xp[:, 7:7 + n] = x[b, :, :n]
        u = np.zeros((C, 2 * n), dtype=np.float64)
        for k in range(15):  # u[2 q + p] = sum_k up[p][k] x[q + k - 7]
            u[:, 0::2] += up[0, k] * xp[:, k:k + n]
            u[:, 1::2] += up[1, k] * xp[:, k:k + n]
        s = u + (1.0 / bsum) * np.sin(u * a) ** 2
        sp = np.zeros((C, 2 * n + 28), dtype=np.float64)
        sp[:, 13:13 + 2 * n] = s
        acc = np.zeros((C, n), dtype=np.float64)
        for k in range(28):  # y[t] = sum_k down[k] s[2 t + k - 13]
            acc += down[k] * sp[:, k:k + 2 * n:2]
        y[b, :, :n] = acc
    return y


def log_params(C, flip=False):
    """The log-scale parameter (alpha; flip: beta) of C channels as the reference holds it, fp32: exp of it is log-spaced over
    [1e-3, 1e2]; one channel: one end of the range."""
    v = np.linspace(-3.0, 2.0, C) if C > 1 else np.array([-3.0])
    if flip:
        v = np.linspace(2.0, -3.0, C) if C > 1 else np.array([2.0])
    return (v * math.log(10.0)).astype(np.float32)


def exp32(log_param):
    """exp of an fp32 log-scale parameter in fp32, as the reference's forward computes it (torch.exp): what the kernel is given."""
    import torch

    return None if log_param is None else torch.exp(torch.from_numpy(np.asarray(log_param, dtype=np.float32))).numpy()


def lengths(tile):
    return [1, 2, 11, 12, 13, tile - 1, tile, tile + 1, 2 * tile + 5]


CHANNELS = (1, 3, 64)
BATCHES = (1, 3)


def case_input(T, C, B, beta):
    """The seeded input of a case: x (B, C, T) float32 and the fp32 log-scale parameters alpha, beta (None without beta)."""
    rng = np.random.default_rng(1000003 * T + 1009 * C + 17 * B + int(beta))
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    return x, log_params(C), (log_params(C, flip=True) if beta else None)


def cases(tile):
    """(tag, T, C, B, beta, lens): the full product the test asks for, then the ragged batches -- rows of 1, tile - 1, tile and
    tile + 1 samples in ONE batch of T = tile + 1 (and of 2 tile + 5, where the rows end inside other workgroups' tiles)."""
    out = []
    for beta in (False, True):
        for C in CHANNELS:
            for B in BATCHES:
                for T in lengths(tile):
                    out.append((f"T{T}.C{C}.B{B}.{'beta' if beta else 'alpha'}", T, C, B, beta, None))
        for C in (3, 64):
            for T in (tile + 1, 2 * tile + 5):
                out.append((f"ragged.T{T}.C{C}.{'beta' if beta else 'alpha'}", T, C, 4, beta, [1, tile - 1, tile, tile + 1]))
    return out


def ref_error():
    """What make_golden_snake.py recorded: {"tile": .., "max_rel": the largest max|ref32 - f64| / max|f64| over the cases, ...}."""
    with open(REF_ERROR_JSON) as f:
        return json.load(f)


def rel_error(y, ref):
    """max |y - ref| / max |ref| of one tensor (every element takes part)."""
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    return float(np.abs(np.asarray(y, dtype=np.float64) - ref).max()) / (scale if scale > 0 else 1.0)


def reference_activation(C, log_a, log_b):
    """The reference's Activation1d around Snake / SnakeBeta with log-scale parameters (bigvgan.AliasFreeSnake, as PReLU_Conv
    builds it, blocks.py:176-181), through oracle/ref_import.py.  Needs the reference checkout."""
    import importlib

    import torch

    import ref_import as R

    R.install_stubs()
    snake = importlib.import_module("open_universe.networks.bigvgan.snake")
    m = snake.AliasFreeSnake(C, alpha_logscale=True, beta=log_b is not None)
    with torch.no_grad():
        m.act.act.alpha.copy_(torch.from_numpy(log_a))
        if log_b is not None:
            m.act.act.beta.copy_(torch.from_numpy(log_b))
    return m.eval()


def reference_output(x, log_a, log_b, lens, dtype):
    """The reference on every row alone (its own length), evaluated in `dtype`."""
    import torch

    B, C, T = x.shape
    m = reference_activation(C, log_a, log_b).to(dtype)
    y = np.zeros((B, C, T), dtype=np.float64)
    with torch.no_grad():
        for b in range(B):
            n = T if lens is None else int(lens[b])
            if n:
                y[b, :, :n] = m(torch.from_numpy(x[b:b + 1, :, :n]).to(dtype)).double().numpy()[0]
    return y


def f64_of_logs(log_param):
    """exp of the fp32 log-scale parameter in float64: what the reference evaluated in float64 works with."""
    return None if log_param is None else np.exp(np.asarray(log_param, dtype=np.float64))
