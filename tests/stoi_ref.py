"""Two float64 restatements of the score of ou_stoi / metrics.stoi (include/ouniverse.h): STOI (Taal et al. 2011) and
extended STOI (Jensen & Taal 2016) with the constants and conventions of the authors' MATLAB code.

The package the reference asks for these numbers (pystoi, metrics/wrapper.py:116-128) is not a dependency of this project and no
recording of it exists here: the definition is the contract, and the two routes below pin it.

  stoi_vec     vectorised: scipy.signal.resample_poly, numpy.kaiser / sinc, numpy.fft.rfft, a band matrix, sliding windows.
  stoi_direct  from the sums: the Kaiser window by the power series of I0, the polyphase sum output by output, the DFT as a
               product with an explicit cos / sin matrix, loops over kept frames, bands, segments and frames.

They share the constants below and ONE rule: `frame_starts` -- which frames a signal of n samples has.  It is the MATLAB rule
(`range(0, n - 256, 128)`, end exclusive: a frame that would start exactly at n - 256 is not counted); whether the package counts
that frame is the one point of the definition nobody here could check, and this function is the one place to flip it.

Arguments are (est, ref, fs) as in metrics.stoi: `ref` is the clean signal.  Both routes return Result(score, margin, frames):
margin is the smallest distance of any frame energy to the silent-frame threshold in dB (inf without frames), frames the number
of STFT frames after the silent frames are gone (the score is 1e-5 below 30)."""
import math
from typing import NamedTuple

import numpy as np
import scipy.signal

FS = 10000
N_FRAME, HOP, NFFT = 256, 128, 512
N_BANDS, MIN_FREQ = 15, 150.0
SEGMENT = 30
BETA_DB = -15.0
DYN_RANGE = 40.0
EPS = float(np.finfo(np.float64).eps)  # 2^-52
SHORT = 1e-5
#: [lo, hi) of the fifteen one-third-octave bands on the grid 10000 i / 512 (test_stoi_cpu.py recomputes them)
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219))


class Result(NamedTuple):
    score: float
    margin: float
    frames: int


def frame_starts(n):
    """THE frame rule: the starts of the frames of 256 at hop 128 of a signal of n samples."""
    return range(0, n - N_FRAME, HOP)


def ratio(fs):
    g = math.gcd(FS, int(fs))
    return FS // g, int(fs) // g


def filter_half_length(p, q):
    fc = 1.0 / (2.0 * max(p, q))
    return int(np.ceil(52.0 / (28.714 * fc / 10.0)))


def band_edges():
    """The bands from their definition: centre 150 * 2^(k/3) Hz, edges the bins nearest to 150 * 2^((2k -+ 1)/6) Hz."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(N_BANDS, dtype=np.float64)
    lo = MIN_FREQ * 2.0 ** ((2 * k - 1) / 6)
    hi = MIN_FREQ * 2.0 ** ((2 * k + 1) / 6)
    return tuple((int(np.argmin((f - a) ** 2)), int(np.argmin((f - b) ** 2))) for a, b in zip(lo, hi))


def window():
    return np.hanning(N_FRAME + 2)[1:-1]


def ulp32(v):
    """One fp32 ulp at v."""
    return float(np.spacing(np.float32(abs(v))))


# ---- the vectorised route ------------------------------------------------------------------------------------------------
def kaiser_filter_vec(p, q):
    L = filter_half_length(p, q)
    fc = 1.0 / (2.0 * max(p, q))
    t = np.arange(-L, L + 1)
    return 2 * p * fc * np.sinc(2 * fc * t) * np.kaiser(2 * L + 1, 0.1102 * (60.0 - 8.7))


def resample_vec(x, fs):
    if fs == FS:
        return np.asarray(x, np.float64)
    p, q = ratio(fs)
    h = kaiser_filter_vec(p, q)
    return scipy.signal.resample_poly(np.asarray(x, np.float64), p, q, window=h / np.sum(h))


def _frames_vec(x):
    starts = np.asarray(frame_starts(len(x)), dtype=np.int64)
    if starts.size == 0:
        return np.zeros((0, N_FRAME))
    return x[starts[:, None] + np.arange(N_FRAME)[None, :]] * window()[None, :]


def remove_silent_vec(x, y):
    """x: clean.  -> (x', y', margin)."""
    fx, fy = _frames_vec(x), _frames_vec(y)
    if fx.shape[0] == 0:
        return np.zeros(0), np.zeros(0), float("inf")
    e = 20.0 * np.log10(np.linalg.norm(fx, axis=1) + EPS)
    thr = np.max(e) - DYN_RANGE
    keep = e > thr
    out = []
    for f in (fx[keep], fy[keep]):
        z = np.zeros((f.shape[0] + 1, HOP))
        z[:-1] += f[:, :HOP]
        z[1:] += f[:, HOP:]
        out.append(z.reshape(-1))
    return out[0], out[1], float(np.min(np.abs(e - thr)))


def bands_of_vec(z):
    """(15, frames) band values of a compacted signal."""
    spec = np.fft.rfft(_frames_vec(z), n=NFFT, axis=1)  # (frames, 257)
    obm = np.zeros((N_BANDS, NFFT // 2 + 1))
    for k, (lo, hi) in enumerate(BANDS):
        obm[k, lo:hi] = 1.0
    return np.sqrt(obm @ (np.abs(spec) ** 2).T)


def score_vec(X, Y, extended):
    """X: clean, Y: estimate, (15, frames)."""
    J = X.shape[1]
    if J < SEGMENT:
        return SHORT
    xs = np.lib.stride_tricks.sliding_window_view(X, SEGMENT, axis=1).transpose(1, 0, 2)  # (M, 15, 30): m = 30 .. J
    ys = np.lib.stride_tricks.sliding_window_view(Y, SEGMENT, axis=1).transpose(1, 0, 2)
    M = xs.shape[0]

    def rows(a):
        a = a - np.mean(a, axis=2, keepdims=True)
        return a / (np.linalg.norm(a, axis=2, keepdims=True) + EPS)

    def cols(a):
        a = a - np.mean(a, axis=1, keepdims=True)
        return a / (np.linalg.norm(a, axis=1, keepdims=True) + EPS)

    if extended:
        return float(np.sum(cols(rows(xs)) * cols(rows(ys))) / (SEGMENT * M))
    c = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    yp = np.minimum(ys * c, xs * (1 + 10 ** (-BETA_DB / 20)))
    return float(np.sum(rows(xs) * rows(yp)) / (N_BANDS * M))


def bands_vec(est, ref, fs):
    """-> (X clean, Y estimate, margin)."""
    x, y = resample_vec(ref, fs), resample_vec(est, fs)
    x, y, margin = remove_silent_vec(x, y)
    return bands_of_vec(x), bands_of_vec(y), margin


def stoi_vec(est, ref, fs, extended=False):
    X, Y, margin = bands_vec(est, ref, fs)
    return Result(score_vec(X, Y, extended), margin, X.shape[1])


# ---- the route from the sums ---------------------------------------------------------------------------------------------
def i0_series(x):
    """I0(x) = sum_k ((x / 2)^k / k!)^2."""
    term, total, k = 1.0, 1.0, 0
    while term > 1e-20 * total:
        k += 1
        term *= (x / 2.0 / k) ** 2
        total += term
    return total


def kaiser_filter_direct(p, q):
    L = filter_half_length(p, q)
    fc = 1.0 / (2.0 * max(p, q))
    beta = 0.1102 * (60.0 - 8.7)
    h = np.zeros(2 * L + 1)
    for t in range(-L, L + 1):
        a = math.pi * 2.0 * fc * t
        sinc = 1.0 if t == 0 else math.sin(a) / a
        kaiser = i0_series(beta * math.sqrt(1.0 - (t / L) ** 2)) / i0_series(beta)
        h[t + L] = 2 * p * fc * sinc * kaiser
    return h


def resample_direct(x, fs):
    """Output j = sum_k h[k] xup[j q + L - k], xup[i p] = x[i]: only k = (j q + L) mod p, + p, + 2 p .. meet a sample."""
    x = np.asarray(x, np.float64)
    if fs == FS:
        return x
    p, q = ratio(fs)
    h = kaiser_filter_direct(p, q)
    h = h / math.fsum(h) * p
    L, T = (len(h) - 1) // 2, len(x)
    out = np.zeros(-(-T * p // q))
    for j in range(len(out)):
        n = j * q + L
        k = np.arange(n % p, 2 * L + 1, p)
        i = (n - k) // p
        ok = (i >= 0) & (i < T)
        out[j] = np.dot(h[k[ok]], x[i[ok]])
    return out


def remove_silent_direct(x, y):
    w = window()
    starts = list(frame_starts(len(x)))
    if not starts:
        return np.zeros(0), np.zeros(0), float("inf")
    e = [20.0 * math.log10(math.sqrt(math.fsum((w * x[s:s + N_FRAME]) ** 2)) + EPS) for s in starts]
    thr = max(e) - DYN_RANGE
    kept = [s for s, v in zip(starts, e) if v > thr]
    zx, zy = np.zeros(HOP * (len(kept) - 1) + N_FRAME), np.zeros(HOP * (len(kept) - 1) + N_FRAME)
    for k, s in enumerate(kept):  # ascending: every output sample is the sum of at most two windowed frames
        zx[HOP * k:HOP * k + N_FRAME] += w * x[s:s + N_FRAME]
        zy[HOP * k:HOP * k + N_FRAME] += w * y[s:s + N_FRAME]
    return zx, zy, min(abs(v - thr) for v in e)


_DFT = None


def dft_matrices():
    """cos and -sin of 2 pi k bin / 512 for k < 256 (the upper half of the zero-padded frame is zero), bins 0 .. 256."""
    global _DFT
    if _DFT is None:
        m = (np.arange(NFFT // 2 + 1)[:, None] * np.arange(N_FRAME)[None, :]) % NFFT
        ang = 2.0 * np.pi * m / NFFT
        _DFT = np.cos(ang), -np.sin(ang)
    return _DFT


def bands_of_direct(z):
    w = window()
    c, s = dft_matrices()
    starts = list(frame_starts(len(z)))
    out = np.zeros((N_BANDS, len(starts)))
    for m, s0 in enumerate(starts):
        f = w * z[s0:s0 + N_FRAME]
        re, im = c @ f, s @ f
        pw = re * re + im * im
        for k, (lo, hi) in enumerate(BANDS):
            out[k, m] = math.sqrt(math.fsum(pw[lo:hi]))
    return out


def _unit(v):
    v = v - math.fsum(v) / len(v)
    return v / (math.sqrt(math.fsum(v * v)) + EPS)


def score_direct(X, Y, extended):
    J = X.shape[1]
    if J < SEGMENT:
        return SHORT
    clip = 1.0 + 10.0 ** (15.0 / 20.0)
    terms, M = [], 0
    for m in range(SEGMENT, J + 1):
        xs, ys = X[:, m - SEGMENT:m], Y[:, m - SEGMENT:m]
        M += 1
        if extended:
            xn = np.stack([_unit(xs[k]) for k in range(N_BANDS)])
            yn = np.stack([_unit(ys[k]) for k in range(N_BANDS)])
            for j in range(SEGMENT):
                terms.append(float(np.dot(_unit(xn[:, j]), _unit(yn[:, j]))))
        else:
            for k in range(N_BANDS):
                c = math.sqrt(math.fsum(xs[k] ** 2)) / (math.sqrt(math.fsum(ys[k] ** 2)) + EPS)
                yp = np.minimum(c * ys[k], xs[k] * clip)
                terms.append(float(np.dot(_unit(xs[k]), _unit(yp))))
    return math.fsum(terms) / ((SEGMENT if extended else N_BANDS) * M)


def bands_direct(est, ref, fs):
    x, y = resample_direct(ref, fs), resample_direct(est, fs)
    x, y, margin = remove_silent_direct(x, y)
    return bands_of_direct(x), bands_of_direct(y), margin


def stoi_direct(est, ref, fs, extended=False):
    X, Y, margin = bands_direct(est, ref, fs)
    return Result(score_direct(X, Y, extended), margin, X.shape[1])
