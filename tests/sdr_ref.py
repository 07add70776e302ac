"""Two float64 restatements of the score of ou_sdr / metrics.sdr (include/ouniverse.h): the BSS-eval SDR with a distortion filter
of L taps, zero_mean=False.  With s_l = ref delayed by l samples (l < L), everything zero-extended to T + L - 1, and P the
orthogonal projection onto span{s_l}:   c = ||P est||^2 / ||est||^2,   SDR = 10 log10(c / (1 - c)).

The package the reference asks for this number (fast_bss_eval, metrics/wrapper.py:179-195) is not a dependency of this project
and no recording of it exists here: the definition is the contract, and the two routes below -- which share nothing but the
definition -- pin it.  Neither clamps: the cases of tests/sdr_cases.py that are gated lie far inside +-clamp_db."""
import numpy as np


def shift_matrix(ref, L):
    """(T + L - 1, L): column l is ref delayed by l samples."""
    ref = np.asarray(ref, np.float64)
    T = ref.shape[0]
    A = np.zeros((T + L - 1, L))
    for l in range(L):
        A[l:l + T, l] = ref
    return A


def sdr_lstsq(est, ref, L=512):
    """The projection itself: least squares on the explicit shift matrix; the ratio is ||P est||^2 / ||est - P est||^2."""
    est, ref = np.asarray(est, np.float64), np.asarray(ref, np.float64)
    A = shift_matrix(ref, L)
    e = np.zeros(A.shape[0])
    e[:est.shape[0]] = est
    h = np.linalg.lstsq(A, e, rcond=None)[0]
    proj = A @ h
    res = e - proj
    return 10.0 * np.log10(np.dot(proj, proj) / np.dot(res, res))


def correlations(est, ref, L):
    """r[l] = sum_t ref[t] ref[t + l], x[l] = sum_t ref[t] est[t + l], l < L (zero behind the signals)."""
    est, ref = np.asarray(est, np.float64), np.asarray(ref, np.float64)
    T = ref.shape[0]
    r, x = np.zeros(L), np.zeros(L)
    for l in range(min(L, T)):
        r[l] = np.dot(ref[:T - l], ref[l:])
        x[l] = np.dot(ref[:T - l], est[l:])
    return r, x


def toeplitz(r):
    i = np.arange(r.shape[0])
    return r[np.abs(i[:, None] - i[None, :])]


def sdr_normal(est, ref, L=512):
    """The normal equations: R = toeplitz(r), R h = x by a dense solve, c = x.h / sum est^2."""
    est = np.asarray(est, np.float64)
    r, x = correlations(est, ref, L)
    h = np.linalg.solve(toeplitz(r), x)
    c = np.dot(x, h) / np.dot(est, est)
    return 10.0 * np.log10(c / (1.0 - c))


def cond_R(ref, L):
    """2-norm condition number of toeplitz(r)."""
    r, _ = correlations(ref, ref, L)
    w = np.linalg.eigvalsh(toeplitz(r))
    return float(w[-1] / w[0])


def si_sdr(est, ref):
    """metrics/wrapper.py:197-213 without the clamp: what the SDR is at L = 1."""
    est, ref = np.asarray(est, np.float64), np.asarray(ref, np.float64)
    c = np.dot(est, ref) ** 2 / (np.dot(est, est) * np.dot(ref, ref))
    return 10.0 * np.log10(c / (1.0 - c))


def ulp32(v):
    """One fp32 ulp at v."""
    return float(np.spacing(np.float32(abs(v))))
