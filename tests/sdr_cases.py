"""The cases of the SDR tests (tests/test_sdr_cpu.py, tests/test_gpu_sdr.py) and their float64 references (tests/sdr_ref.py),
computed once per process and shared.

Every filter length L in FILTER_LENGTHS meets every length T in {1, 5, L - 1, L, L + 1, 700, 4097, 8192} (T >= 1, duplicates
once): 37 pairs.  L = 512 stays at T <= 8192, where the explicit shift matrix of `sdr_lstsq` is 8703 x 512 doubles (35 MB).
Signals: the reference is seeded white noise; the estimate is the reference through a 3-tap FIR (so L = 1 and 2 leave part of
it outside the span) plus white noise, at target ratios cycling through -20, -5, 10, 20 and 35 dB; fp32 values, as the library
reads them.  COLOURED is the same at L = 64, T = 4097 with a one-pole low-passed reference (pole 0.9: cond(R) about 320).

A case is `gated` when the accuracy gate of test_gpu_sdr.py applies to it: cond(R) <= 1e8 and the restatement inside [-40, 60]
dB, so that neither the clamp nor hopeless conditioning is what the gate measures -- both are asserted by test_sdr_cpu.py.
The cases with T = 1 cannot be: one sample of the estimate is always a multiple of one sample of the reference, the
projection is the estimate itself and the SDR is infinite.  They stay in the table and must score +clamp_db.

`edge` holds what that table stops short of: filter lengths either side of the switch between one and two accumulator tiles
of the correlation kernel (255, 256, 257) and 511, a coloured reference at 257 taps, a row of 32 correlation tiles.  MANY are
ragged calls of 130 rows -- three launch groups -- with the one longest row last or first."""
import functools

import numpy as np

import sdr_ref as R

FILTER_LENGTHS = (1, 2, 17, 64, 512)
TARGET_DB = (-20.0, -5.0, 10.0, 20.0, 35.0)
FIR = (1.0, -0.5, 0.25)
COND_MAX, DB_MIN, DB_MAX = 1e8, -40.0, 60.0


def lengths(L):
    return sorted({T for T in (1, 5, L - 1, L, L + 1, 700, 4097, 8192) if T >= 1})


def make_pair(T, target_db, seed, pole=0.0):
    """-> (est, ref) float32 of T samples."""
    g = np.random.default_rng(seed)
    ref = g.standard_normal(T)
    if pole:
        for t in range(1, T):
            ref[t] += pole * ref[t - 1]
    clean = np.convolve(ref, FIR)[:T]
    noise = g.standard_normal(T)
    gain = np.sqrt(np.dot(clean, clean) / np.dot(noise, noise)) * 10.0 ** (-target_db / 20.0)
    return (clean + gain * noise).astype(np.float32), ref.astype(np.float32)


class Case:
    def __init__(self, name, L, T, target_db, seed, pole=0.0):
        self.name, self.L, self.T, self.target_db, self.seed, self.pole = name, L, T, target_db, seed, pole
        self.gated = T > 1

    def __repr__(self):
        return self.name

    @functools.cached_property
    def pair(self):
        return make_pair(self.T, self.target_db, self.seed, self.pole)

    @functools.cached_property
    def lstsq(self):
        return float(R.sdr_lstsq(*self.pair, self.L))

    @functools.cached_property
    def normal(self):
        return float(R.sdr_normal(*self.pair, self.L))

    @property
    def d_ref(self):
        """How far apart the two float64 routes are, in dB."""
        return abs(self.lstsq - self.normal)

    @functools.cached_property
    def cond(self):
        return R.cond_R(self.pair[1], self.L)

    def bound(self):
        """The accuracy gate: 4 d_ref + one fp32 ulp of the score."""
        return 4.0 * self.d_ref + R.ulp32(self.lstsq)


def _table():
    out, i = [], 0
    for L in FILTER_LENGTHS:
        for T in lengths(L):
            out.append(Case(f"L{L}-T{T}", L, T, TARGET_DB[i % len(TARGET_DB)], 1000 + i))
            i += 1
    return out


CASES = _table()
COLOURED = Case("coloured-L64-T4097", 64, 4097, 20.0, 77, pole=0.9)
GATED = [c for c in CASES if c.gated] + [COLOURED]
UNGATED = [c for c in CASES if not c.gated]
#: the ragged batch: five rows mixing the lengths above, one filter length
RAGGED_L = 64
RAGGED = [c for c in CASES if c.L == RAGGED_L and c.T in (5, 63, 65, 700, 4097)]
assert len(RAGGED) == 5


def by_name(name):
    return next(c for c in CASES + [COLOURED] if c.name == name)


# ---- the edges the table above stops short of ----
#: filter lengths either side of the switch between one accumulator tile of 256 lags and two, and one below the cap
EDGE_FILTER_LENGTHS = (255, 256, 257, 511)
#: every edge case by name; "T+" stands for the first length with a second correlation tile, which the caller finds from the
#: scratch sizer (the `_tile()` of test_gpu_sdr.py) and hands to `edge`
EDGE_NAMES = tuple(f"edge-L{L}-T{T}" for L in EDGE_FILTER_LENGTHS for T in ("L+1", "tile+1")) + (
    "edge-coloured-L257-T4097", "edge-L64-T65537")


def tile_from(scratch_bytes):
    """Samples per correlation tile, from the scratch sizer (pure host code): the last T that costs what T = 1 costs."""
    lo, hi, base = 1, 1 << 20, scratch_bytes(1, 1, 512)
    assert scratch_bytes(1, hi, 512) > base
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if scratch_bytes(1, mid, 512) == base else (lo, mid - 1)
    return lo


@functools.lru_cache(maxsize=None)
def edge(tile):
    """{name: Case} of EDGE_NAMES for a correlation tile of `tile` samples: L in EDGE_FILTER_LENGTHS at T = L + 1 (one tile,
    barely more samples than lags) and T = tile + 1 (one sample in a second tile); a coloured reference (pole 0.9) on the
    two-accumulator-tile path; and a row of 32 correlation tiles at L = 64 (the shift matrix of `sdr_lstsq` is 34 MB)."""
    out, i = {}, 0
    for L in EDGE_FILTER_LENGTHS:
        for label, T in (("L+1", L + 1), ("tile+1", tile + 1)):
            out[f"edge-L{L}-T{label}"] = Case(f"edge-L{L}-T{T}", L, T, TARGET_DB[i % len(TARGET_DB)], 2000 + i)
            i += 1
    out["edge-coloured-L257-T4097"] = Case("edge-coloured-L257-T4097", 257, 4097, 20.0, 78, pole=0.9)
    out["edge-L64-T65537"] = Case("edge-L64-T65537", 64, 65537, 10.0, 2010)
    assert tuple(out) == EDGE_NAMES
    return out


class Many:
    """A ragged call of 130 rows -- launch groups of 64, 64 and 2 -- at one filter length.  The lengths cycle over a short list,
    so the rows reuse a few pairs and every distinct pair has its references computed once; rows 63, 64, 127 and 128 -- the
    last and first rows of the groups -- hold one sample; `longest_at` (0 or 129) holds the one row of `longest` samples, so
    either the first group or the last is the one whose grid is as large as the call's strides."""
    ROWS, DEGENERATE = 130, (63, 64, 127, 128)

    def __init__(self, L, cycle, longest, longest_at, seed):
        assert longest > max(cycle) and longest_at in (0, self.ROWS - 1)
        self.L, self.longest_at = L, longest_at
        pool = {T: Case(f"many-L{L}-T{T}", L, T, TARGET_DB[k % len(TARGET_DB)], seed + k)
                for k, T in enumerate(list(cycle) + [1, longest])}
        self.cases = [pool[1] if b in self.DEGENERATE else pool[longest] if b == longest_at else pool[cycle[b % len(cycle)]]
                      for b in range(self.ROWS)]

    def __repr__(self):
        return f"many-L{self.L}-longest-at-{self.longest_at}"


#: the 130-row calls: L = 64 and L = 257 (one and two accumulator tiles), the longest row last and first
MANY = [Many(L, (5, L - 1, L + 1, 700), 4097, at, 3000 + 100 * k + 10 * j)
        for k, L in enumerate((64, 257)) for j, at in enumerate((129, 0))]
