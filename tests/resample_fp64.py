"""float64 reference and per-sample bounds of the library's resampler (csrc/ou_resample.hip) for the tests, in the style of
small_fp64.py (its `Report`, `ulp32` and `U`).  Two kinds of bound, none tuned, no sample excluded:

* chain   noise rows.  The kernels accumulate taps ascending, one fp32 FMA each, so a sample is a sum of `taps` products in
          fp32: |gpu - f64| <= (taps + 2) u A + 1/2 ulp(|gpu|), f64 = resample_reference.resample64 (the dense kernel, no code
          shared with the library), A = the float64 sum of |k[p][i] x[.]| over the same dense row, taps = the library's own count
          for the pair (_lib.resample_table).  The two spare u also cover a table entry one fp32 ulp (<= 2 u relative) from the
          dense kernel's, which test_resample_cpu.py allows (libm against numpy in the last float64 bit before the rounding).
* exact   impulse rows.  An input that is 0 but for isolated samples of amplitude 1, -2 or 0.5 has at most one nonzero input
          under any output's taps, so the sample is amplitude x one fp32 coefficient (a power of two: no rounding) and zeros
          added to it: it has to equal that product bit for bit (compared with ==, so -0.0 equals 0.0), and be 0 elsewhere.

Behind a row's own output length every sample is exactly 0.

Impulse rows of a pair (one ragged call): a comb with D samples between its impulses, D the smallest integer above the dense
filter span 2 width + orig that is coprime to orig, so that over D frames every phase meets every tap; its first impulse is
input sample 0 and its last one sample len - 1.  Four more rows carry ONE impulse each: the input under the first and under the
last live tap of the last output of tile 0 and of the first output of tile 1 (ou_resample_tile).  Where orig x span exceeds
COMB_SAMPLES (16 000 -> 16 001: 256 M samples) the comb's D is taken from the table's `taps` instead -- the kernels read no
other input, so the windows still hold one impulse at most, which `impulse_case` asserts for every window of every row."""
import functools
import math

import numpy as np
import torch

import resample_reference as R
from open_universe_amd import _lib
from small_fp64 import U, Report

AMPLITUDES = (1.0, -2.0, 0.5)
COMB_SAMPLES = 1 << 20
# the kernel a pair takes (ou_resample.hip, geometry()), with the tile the launcher reports for it
PATHS = {(192000, 8000): ("lds_table_128_threads", 512), (16000, 16001): ("global_table_256_threads", 1024),
         (1000000, 16000): ("direct", 256)}
DEFAULT_PATH = ("lds_table_256_threads", 1024)


class Pair:
    """Geometry, table and tile of a rate pair, as the library states them (pure host code)."""

    def __init__(self, fs_in, fs_out):
        self.fs_in, self.fs_out = fs_in, fs_out
        self.orig, self.new, _, self.width = R.geometry(fs_in, fs_out)
        self.first, self.coef, _ = _lib.resample_table(fs_in, fs_out)
        self.taps = self.coef.shape[0]
        self.span = 2 * self.width + self.orig
        self.tile = int(_lib.load().ou_resample_tile(fs_in, fs_out))
        self.path = PATHS.get((fs_in, fs_out), DEFAULT_PATH)[0]
        # the last nonzero tap of every phase (a phase's support may be shorter than `taps`: zeros behind it)
        self.last_live = self.taps - 1 - (self.coef[::-1] != 0).argmax(axis=0)

    def out_len(self, n):
        return R.out_length(self.fs_in, self.fs_out, n)

    def start(self, j):
        """The first input under the taps of output j."""
        j = np.asarray(j, dtype=np.int64)
        return (j // self.new) * self.orig + self.first[j % self.new].astype(np.int64)

    def windows(self, x):
        """(J, taps): the inputs under the taps of every output of the row x, 0 outside the row -- what the kernels read."""
        x = np.asarray(x)
        n = x.shape[0]
        pos = self.start(np.arange(self.out_len(n)))[:, None] + np.arange(self.taps)[None, :]
        return np.where((pos >= 0) & (pos < n), x[np.clip(pos, 0, n - 1)], 0).astype(x.dtype)


@functools.lru_cache(maxsize=None)
def pair(fs_in, fs_out):
    return Pair(fs_in, fs_out)


def lengths(P):
    """Row lengths of the noise case: 1, width - 1, orig -+ 1, the three lengths around the launcher's tile (a row whose last
    output is the last of tile 0, or as close as the ratio allows, and the rows that just cross into tile 1) and one row of just
    over two tiles (tile 1 is then neither first nor last: a non-zero first frame).  16 000 -> 16 001: 300 only (16 014 dense
    coefficients per output)."""
    if (P.fs_in, P.fs_out) == (16000, 16001):
        return [300]
    t, o, n = P.tile, P.orig, P.new
    at_tile = [t * o // n, -(-t * o // n), -(-(t + 1) * o // n)]
    return sorted({m for m in [1, P.width - 1, o - 1, o + 1] + at_tile + [-(-(2 * t + 1) * o // n)] if m >= 1})


def abs_sum(P, x):
    """A of the chain bound: sum_i |k[p][i] x[f orig - width + i]| over the dense row of every output, float64."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    n, J, L = x.shape[0], P.out_len(x.shape[0]), P.span
    j = np.arange(J)
    f, p = j // P.new, j % P.new
    phases = np.unique(p)
    k = np.abs(R.dense_rows(P.fs_in, P.fs_out, phases))
    xp = np.zeros(P.width + (int(f.max()) + 1) * P.orig + L + n)
    xp[P.width:P.width + n] = x
    return np.einsum("jl,jl->j", k[np.searchsorted(phases, p)], xp[(f * P.orig)[:, None] + np.arange(L)[None, :]])


def _padded(rows, cols):
    out = torch.zeros(len(rows), cols, dtype=torch.float64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = torch.from_numpy(np.asarray(r, dtype=np.float64))
    return out


@functools.lru_cache(maxsize=None)
def noise_case(fs_in, fs_out):
    """The noise rows of a pair (two per length, resample_reference.noise_rows) with their float64 reference and chain bound,
    computed once: dict of rows (list of fp32 arrays), lens, out_lens, cols, ref and bound ((rows, cols) float64 tensors)."""
    P = pair(fs_in, fs_out)
    lens, rows = [], []
    for i, n in enumerate(lengths(P)):
        rows += list(R.noise_rows(2, n, 100 + i))
        lens += [n, n]
    out_lens = [P.out_len(n) for n in lens]
    cols = max(out_lens)
    ref = _padded([R.resample64(r, fs_in, fs_out) for r in rows], cols)
    bound = (P.taps + 2) * U * _padded([abs_sum(P, r) for r in rows], cols)
    return {"rows": rows, "lens": lens, "out_lens": out_lens, "cols": cols, "ref": ref, "bound": bound}


def _coprime_from(d, orig):
    while math.gcd(d, orig) != 1:
        d += 1
    return d


def comb_spacing(P):
    span = P.span if P.orig * (P.span + 1) <= COMB_SAMPLES else P.taps - 1
    return _coprime_from(span + 1, P.orig)


@functools.lru_cache(maxsize=None)
def impulse_case(fs_in, fs_out):
    """The impulse rows of a pair with what they have to give, from the library's table: dict of rows, lens, out_lens, cols,
    want ((rows, cols) float64 tensor, every entry an fp32 number), hits ((new, taps) bool: phase p met tap t in some row),
    seams (the (output, tap, input) of the four one-impulse rows)."""
    P = pair(fs_in, fs_out)
    D = comb_spacing(P)
    K = -(-(D + 2) * P.orig // D) + -(-P.span // D) + 1  # D + 2 frames and a filter span: every residue of every phase
    comb = np.zeros(K * D + 1, dtype=np.float32)
    comb[::D] = np.resize(np.asarray(AMPLITUDES, dtype=np.float32), K + 1)
    rows, seams = [comb], []
    n_seam = -(-(P.tile + P.new + 1) * P.orig // P.new) + P.span
    for i, (j, last) in enumerate(((P.tile - 1, False), (P.tile - 1, True), (P.tile, False), (P.tile, True))):
        t = int(P.last_live[j % P.new]) if last else 0
        s = int(P.start(j)) + t
        assert 0 <= s < n_seam, (j, t, s)
        row = np.zeros(n_seam, dtype=np.float32)
        row[s] = AMPLITUDES[i % 3]
        rows.append(row)
        seams.append((j, t, s))
    hits = np.zeros((P.new, P.taps), dtype=bool)
    want = []
    for r in rows:
        xv = P.windows(r)
        assert ((xv != 0).sum(axis=1) <= 1).all()  # one impulse at most under any output's taps
        p = np.arange(xv.shape[0]) % P.new
        jj, tt = np.nonzero(xv)
        hits[p[jj], tt] = True
        y = (P.coef[:, p].T.astype(np.float64) * xv.astype(np.float64)).sum(axis=1)
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y)  # one product with a power of two: an fp32 number
        want.append(y)
    lens = [len(r) for r in rows]
    out_lens = [P.out_len(n) for n in lens]
    cols = max(out_lens)
    return {"rows": rows, "lens": lens, "out_lens": out_lens, "cols": cols, "want": _padded(want, cols), "hits": hits,
            "seams": seams, "spacing": D}


def check_noise(name, case, y):
    """y: (rows, cols) of the library (or of a restatement) for noise_case -> Report at the chain bound."""
    return Report(name, torch.as_tensor(y)[:, :case["cols"]], case["ref"], case["bound"], case["out_lens"])


def check_impulses(name, case, y):
    """y: (rows, cols) for impulse_case -> Report of the `exact` kind (bound 0)."""
    return Report(name, torch.as_tensor(y)[:, :case["cols"]], case["want"], 0.0, case["out_lens"])


def figures(rep, seconds=None):
    """What a case logs: the worst err / bound with its row and sample, and the counts."""
    w = rep.worst
    out = {"ratio": round(rep.ratio, 4), "err": rep.err, "row": w["index"][0], "sample": w["index"][-1], "worst": w, "flagged": rep.n_bad,
           "tail_bad": rep.tail_bad, "checked": rep.checked, "excluded": rep.excluded}
    if seconds is not None:
        out["seconds"] = round(seconds, 2)
    return out
