"""Shared by test_flac_level_cpu.py and test_gpu_flac_level.py: the signals of the compression-level tests (built once per
process, never modified), an independent restatement of the pricing rules of DESIGN.md 4.24 (what each candidate and each
partition order costs, written from the contract, not from audio._subframe_level), and the translation of a choice record into
a subframe spec of the bit-level test encoder (flac_ref_encoder.py)."""
import functools

import numpy as np

import flac_encode_cases as C
import flac_ref_encoder as R
from open_universe_amd import audio as A

BLOCK = 4096
FS = 16000
LENGTHS = [1, 2, 5, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8192 + 48]
KINDS = {A.FLAC_CONSTANT: "constant", A.FLAC_VERBATIM: "verbatim", A.FLAC_FIXED: "fixed", A.FLAC_LPC: "lpc"}


def from_ints(q, bps):
    """integers within bps bits -> the float32 samples that quantise to them"""
    x = (np.asarray(q, np.float64) / float(1 << (bps - 1))).astype(np.float32)
    x = x if x.ndim == 2 else x[None]
    assert np.array_equal(C.quantise(x, bps), np.asarray(q, np.int64).reshape(x.shape))
    return x


def ar8(n, seed, scale):
    """order-8 autoregressive process driven by white noise: four resonances (formant-like, radii falling with frequency: a
    spectral tilt of speech), unit-variance input, output scaled to `scale` steps"""
    g = np.random.default_rng(seed)
    poles = [0.97 * np.exp(1j * 0.12), 0.95 * np.exp(1j * 0.45), 0.90 * np.exp(1j * 1.0), 0.80 * np.exp(1j * 1.9)]
    a = np.real(np.poly(poles + [p.conjugate() for p in poles]))  # 1, a1 .. a8
    e = g.standard_normal(n + 512)
    y = np.zeros(n + 512)
    for t in range(n + 512):
        acc = e[t]
        for j in range(1, 9):
            if t - j >= 0:
                acc -= a[j] * y[t - j]
        y[t] = acc
    y = y[512:]
    return np.rint(y / np.abs(y).max() * scale).astype(np.int64)


# one sample at the head of a block of silence: every fixed order has ONE residual, +-SPIKE, and k = 11 from the block's mean
# leaves it a quotient of 8182: all five candidates leave by the quotient exit (2 SPIKE < (2^12 - 1) 4092)
SPIKE = 8378369


@functools.lru_cache(maxsize=None)
def content_cases(bps):
    """name -> float32 (1, T), T = 2 blocks and a last block of 48 samples (partition orders 0 and 1 only)"""
    full = 1 << (bps - 1)
    n = 2 * BLOCK + 48
    t = np.arange(n, dtype=np.float64)
    g = np.random.default_rng(2024)
    amp = full // 4
    small = lambda s: g.integers(-s, s + 1, n)  # noqa: E731
    out = {
        "zeros": np.zeros(n, np.int64),
        "constant": np.full(n, full - 5, np.int64),
        "ramp": (3 * (t - n // 2)).astype(np.int64),
        "quadratic": np.rint(1e-3 * (t - 4000.0) ** 2).astype(np.int64) % (full // 2) + small(2),
        "cubic": np.rint(2e-7 * (t - 4000.0) ** 3).astype(np.int64) + small(1),
        "sine_slow": np.rint(amp * np.sin(0.005 * t)).astype(np.int64),
        "sine": np.rint(amp * np.sin(0.031 * t)).astype(np.int64),
        "walk": np.clip(np.cumsum(g.integers(-40, 41, n)), -full + 1, full - 1),
        "ar8": ar8(n, 7, full // 3),
        "ar8_quiet": ar8(n, 8, 900),
        "kink": C.quantise(C.content_cases(bps)["kink"][:, :n], bps)[0],
        "spike": np.zeros(n, np.int64),
        "burst": small(3),
        "steps": np.repeat(g.integers(-full // 2, full // 2, n // 64 + 1), 64)[:n] + small(1),
    }
    out["tail"] = small(2)
    out["tail"][2 * BLOCK + 24:] = g.integers(-2000, 2001, 24)  # the last block: 24 quiet samples, 24 loud ones
    out["spike"][0] = SPIKE if bps == 24 else 0
    out["spike"][BLOCK] = -(full - 1)
    out["burst"][BLOCK + 640:BLOCK + 704] = g.integers(-full // 2, full // 2, 64)  # one loud 64-sample stretch: partitions pay
    # white noise from one step to full scale; the levels change inside a block, at partition boundaries of every order
    for i, a in enumerate([1, 6, 40, 300, 5000, full // 16, full - 1]):
        out[f"noise{i}"] = g.integers(-a, a + 1, n)
    gains = np.repeat([1, 30, 2, 900, 5, 70, 1, 8000 if bps == 24 else 300], BLOCK // 8)
    out["levels"] = (g.integers(-3, 4, n) * np.resize(gains, n)).astype(np.int64)
    res = {}
    for k, v in out.items():
        x = from_ints(np.clip(v, -full, full - 1), bps)
        x.setflags(write=False)
        res[k] = x
    return res


def multichannel(ch, n, bps, seed):
    """channels of different kinds (every subframe form mixes inside a frame, subframes end off byte boundaries)"""
    cases = content_cases(bps)
    names = ["ar8", "zeros", "noise2", "sine", "levels", "constant", "noise6", "walk"]
    x = np.stack([np.roll(cases[names[(c + seed) % len(names)]][0], 17 * c)[:n] for c in range(ch)])
    return np.ascontiguousarray(x.astype(np.float32))


def oracle(x, bps, level, override=None):
    """-> (stream, choice records, quantised samples)"""
    q = C.quantise(x, bps)
    s, rec = A.flac_encode(q, FS, bps, level=level, lpc_override=override, return_choices=True)
    return s, rec, q


def override_from(records, ch):
    """choice records of one file -> the lpc_override that hands their coefficients back"""
    out = {}
    for i, r in enumerate(records):
        if r[0] == A.FLAC_LPC:
            out[(i // ch, i % ch)] = ([int(v) for v in r[6:6 + r[1]]], int(r[4]))
    return out


# ---- the contract, restated --------------------------------------------------------------------------------------------------

def rice_k(total, cnt):
    k = 0
    while k < 14 and ((1 << (k + 1)) - 1) * cnt <= total:
        k += 1
    return k


def residuals(x, coefs, shift):
    p = len(coefs)
    return [int(x[i]) - (sum(coefs[j] * int(x[i - 1 - j]) for j in range(p)) >> shift) for i in range(p, len(x))]


def price(x, bps, coefs, shift, lpc, po=0):
    """exact bits of a predictor subframe with partition order po, or None when a quotient exceeds 4096"""
    n, p = len(x), len(coefs)
    u = [2 * r if r >= 0 else -2 * r - 1 for r in residuals(x, coefs, shift)]
    bits = 8 + p * bps + ((4 + 5 + p * 14) if lpc else 0) + 2 + 4
    size = n >> po
    for j in range(1 << po):
        seg = u[max(j * size - p, 0):(j + 1) * size - p]
        k = rice_k(sum(seg), len(seg))
        if max(seg, default=0) >> k > 4096:
            return None
        bits += 4 + len(seg) * (k + 1) + sum(v >> k for v in seg)
    return bits


def allowed_orders(n):
    return [po for po in range(7) if n % (1 << po) == 0 and (n >> po) >= 16]


def fixed_prices(x, bps):
    """candidate name -> stage-1 bits (None: dropped), in tie-break order, for level 1"""
    out = {}
    if len(set(int(v) for v in x)) == 1:
        out["constant"] = 8 + bps
    for p in range(5):
        if len(x) > p:
            out[f"fixed{p}"] = price(x, bps, R.FIXED[p], 0, False)
    return out


def spec_of(rec):
    """choice record -> subframe spec of flac_ref_encoder.subframe (the Rice parameters follow from its own mean rule, which is
    the integer rule; see test_flac_encode_cpu.py)"""
    kind, order, po, prec, shift = (int(v) for v in rec[:5])
    if kind == A.FLAC_CONSTANT:
        return ("constant",)
    if kind == A.FLAC_VERBATIM:
        return ("verbatim",)
    if kind == A.FLAC_FIXED:
        return ("fixed", order, po, 0)
    return ("lpc", [int(v) for v in rec[6:6 + order]], prec, shift, po, 0)


def rebuild(q, bps, records):
    """the stream of these choices from the bit-level test encoder"""
    ch, n = q.shape
    frames = []
    for fno, s0 in enumerate(range(0, n, BLOCK)):
        chans = [[int(v) for v in q[c, s0:s0 + BLOCK]] for c in range(ch)]
        frames.append(R.frame(chans, bps, FS, fno, [spec_of(records[fno * ch + c]) for c in range(ch)], force_explicit_block=True))
    return frames


# ---- ties: found by a search over seeds with the restated prices above; the seeds are committed, the samples are not -----------
TIE_BPS = 16
TIE_SEEDS = {"candidate": (16, 16), "partition": (28, 32)}  # which tie -> (seed, samples of the block)


def tie_signal(which):
    """"candidate": fixed 0 and fixed 1 cost the same and the least (fixed 0 wins); "partition": the winner costs the same with
    partition orders 0 and 1 (0 wins)"""
    seed, n = TIE_SEEDS[which]
    return from_ints(np.cumsum(np.random.default_rng(seed).integers(-6, 7, n)).astype(np.int64), TIE_BPS)
