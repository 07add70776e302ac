"""Restatement of the streaming enhance (include/ouniverse.h, "streaming enhance"): the window plan and the emitted
count in plain Python, and the stitch in float64 from window results it is handed.  Nothing here calls the library."""
import math

import numpy as np


def geometry(tot, segment, overlap):
    S, V = segment - segment % tot, overlap - overlap % tot
    if S < 2 * tot:
        raise ValueError("segment must be at least two total down-sampling factors")
    if overlap < 0 or 2 * V > S:
        raise ValueError("overlap must lie in [0, segment / 2]")
    return S, V


def plan(tot, T, segment, overlap):
    """Windows of a stream flushed after T samples: dict of lists `starts`, `lengths`, `core_begin`, `core_end`, ints `overlap`
    (as used) and `T_pad`."""
    S, V = geometry(tot, segment, overlap)
    T_pad = -(-T // tot) * tot
    if T_pad == 0:
        return {"starts": [], "lengths": [], "core_begin": [], "core_end": [], "overlap": 0, "T_pad": 0}
    if T_pad <= S:
        return {"starts": [0], "lengths": [T_pad], "core_begin": [0], "core_end": [T_pad], "overlap": 0, "T_pad": T_pad}
    starts = list(range(0, T_pad - S + 1, S - V))
    if starts[-1] + S < T_pad:
        starts.append(T_pad - S)
    n = len(starts)
    mid = [starts[k] + S - V + V // 2 for k in range(n - 1)]  # the middle of the crossfade behind window k
    return {"starts": starts, "lengths": [S] * n, "core_begin": [0] + mid, "core_end": mid + [T_pad], "overlap": V, "T_pad": T_pad}


def emitted(tot, P, segment, overlap):
    """Samples emitted once P are pushed, before a flush: everything below s_k + S - V of the newest complete window k."""
    S, V = geometry(tot, segment, overlap)
    if P < S:
        return 0
    return (P - S) // (S - V) * (S - V) + S - V


def weight(i, V, exact=False):
    """a(i), the later window's share at offset i of a crossfade of V samples.  The definition names the weight of ou_segment.hip,
    an fp32-valued function: 0.5 - 0.5 cos(pi_f32 (i + 0.5) / V) with every operation rounded to fp32 -- restated here in numpy's fp32,
    in the kernel's order of operations -- and returned as float64.  `exact`: the real-valued raised cosine."""
    if exact:
        return 0.5 - 0.5 * np.cos(math.pi * (np.asarray(i, dtype=np.float64) + 0.5) / V)
    i = np.asarray(i)
    a = np.float32(0.5) - np.float32(0.5) * np.cos((np.float32(np.pi) * (i.astype(np.float32) + np.float32(0.5))) / np.float32(V))
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def stitch(p, T, results, exact=False):
    """The stream's first T samples from the plan `p` and its windows' results (list of (C, L_k) arrays, None where a window is not
    needed), sample by sample from the definition.  -> (out float64 (C, T), fade bool (T,), scale float64 (C, T)): `fade` marks
    the crossfaded samples, `scale` = |y_k| + |y_{k+1}| there (the operands' magnitude), |sample| elsewhere.  `exact`: with the
    real-valued weight instead of the fp32-valued one of the definition."""
    starts, lens, V = p["starts"], p["lengths"], p["overlap"]
    C = next(r for r in results if r is not None).shape[0]
    out = np.full((C, T), np.nan)
    fade = np.zeros(T, dtype=bool)
    scale = np.zeros((C, T))
    for u in range(T):
        k = next((k for k in range(len(starts) - 1) if starts[k] + lens[k] - V <= u < starts[k] + lens[k]), None)
        if k is not None:
            a = weight(u - (starts[k] + lens[k] - V), V, exact)
            ya, yb = results[k][:, u - starts[k]].astype(np.float64), results[k + 1][:, u - starts[k + 1]].astype(np.float64)
            out[:, u] = (1.0 - a) * ya + a * yb
            fade[u] = True
            scale[:, u] = np.abs(ya) + np.abs(yb)
        else:
            k = next(k for k in range(len(starts)) if starts[k] <= u < starts[k] + lens[k])  # the earliest window that covers u
            out[:, u] = results[k][:, u - starts[k]]
            scale[:, u] = np.abs(out[:, u])
    return out, fade, scale


def needed(p, T):
    """The windows of the plan that reach the first T samples."""
    starts, lens, V = p["starts"], p["lengths"], p["overlap"]
    need = set()
    for u in range(T):
        k = next((k for k in range(len(starts) - 1) if starts[k] + lens[k] - V <= u < starts[k] + lens[k]), None)
        if k is not None:
            need.update((k, k + 1))
        else:
            need.add(next(k for k in range(len(starts)) if starts[k] <= u < starts[k] + lens[k]))
    return sorted(need)
