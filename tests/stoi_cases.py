"""The cases of the STOI tests (tests/test_stoi_cpu.py, tests/test_gpu_stoi.py) and their float64 references (tests/stoi_ref.py),
computed once per process and shared.

Signals: the clean one is seeded white noise under a slow amplitude modulation, the estimate is the clean one plus white noise
at ratios cycling over -5, 0, 5, 15, 30 dB; fp32 values, as the library reads them.  A silent stretch is the clean signal scaled
by 1e-4 (-80 dB) over whole hops of 128 samples at 10 kHz: a frame that lies wholly inside one is 80 dB down and removed, a
frame that straddles its edge keeps half its energy (-3 dB), so every silent-frame decision is decibels from its threshold.

With no silent frame a signal of n samples at 10 kHz has K = ceil((n - 256) / 128) frames and K - 1 STFT frames after the
overlap-add, so n = 256 + 128 (J + 1) has exactly J STFT frames and one sample more has J + 1 (`frame_starts` of stoi_ref.py).

`frames` below always means STFT frames after the silent frames are gone: the number the cut of 30 applies to.  With frames
overlapping by half, "every other frame silent" cannot be made from samples (a kept frame between two removed ones would share
a hop with each): the `alternate` case removes every third frame, the densest pattern there is.

A case is `gated` when the restatements' threshold margin is at least 1e-6 dB and it has at least 30 frames: a condition on the
inputs, not a measurement.  The cases built to have fewer than 30 frames carry `short`: they must score float32(1e-5).

EDGE holds what those tables stop short of: rows of more than 1024 energy frames (the chunk of the kernel's kept-frame scan),
45 and 46 frames (its segment tile), 48, 22.05, 6 and 12 kHz, and 14 s at 48 kHz.  MANY are ragged calls of 130 rows -- three
launch groups -- with the one longest row last or first, at 10 and at 16 kHz."""
import functools

import numpy as np

import stoi_ref as R

TARGET_DB = (-5.0, 0.0, 5.0, 15.0, 30.0)
MARGIN_MIN_DB = 1e-6


def length_for(frames):
    """Samples at 10 kHz that give exactly `frames` STFT frames with no silent frame (one more sample gives one more)."""
    return R.N_FRAME + R.HOP * (frames + 1)


def make_pair(T, fs, target_db, seed, silent_hops=(), zero_clean=False):
    """-> (est, ref) float32 of T samples at fs; silent_hops: hops of 128 samples at 10 kHz over which the clean signal is -80 dB."""
    g = np.random.default_rng(seed)
    t = np.arange(T) / fs
    clean = g.standard_normal(T) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t + 0.3)) * 0.1
    for h in silent_hops:
        a, b = (int(round(R.HOP * h * fs / R.FS)), int(round(R.HOP * (h + 1) * fs / R.FS)))
        clean[a:b] *= 1e-4
    noise = g.standard_normal(T)
    power = np.dot(clean, clean) if T > 1 else 1.0
    gain = np.sqrt(power / np.dot(noise, noise)) * 10.0 ** (-target_db / 20.0)
    if zero_clean:
        clean = np.zeros(T)
    return (clean + gain * noise).astype(np.float32), clean.astype(np.float32)


class Case:
    def __init__(self, name, T, seed, fs=R.FS, silent_hops=(), short=False, zero_clean=False):
        self.name, self.T, self.fs, self.seed, self.short = name, T, fs, seed, short
        self.silent_hops, self.zero_clean = tuple(silent_hops), zero_clean
        self.target_db = TARGET_DB[seed % len(TARGET_DB)]

    def __repr__(self):
        return self.name

    @functools.cached_property
    def pair(self):
        return make_pair(self.T, self.fs, self.target_db, self.seed, self.silent_hops, self.zero_clean)

    @functools.cached_property
    def _vec(self):
        return R.bands_vec(*self.pair, self.fs)

    @functools.cached_property
    def _direct(self):
        return R.bands_direct(*self.pair, self.fs)

    @functools.lru_cache(maxsize=None)
    def vec(self, extended=False):
        X, Y, margin = self._vec
        return R.Result(R.score_vec(X, Y, extended), margin, X.shape[1])

    @functools.lru_cache(maxsize=None)
    def direct(self, extended=False):
        X, Y, margin = self._direct
        return R.Result(R.score_direct(X, Y, extended), margin, X.shape[1])

    @property
    def frames(self):
        return self.vec().frames

    @property
    def margin(self):
        return min(self.vec().margin, self.direct().margin)

    @property
    def gated(self):
        return self.margin >= MARGIN_MIN_DB and self.frames >= R.SEGMENT and self.direct().frames == self.frames

    def d_ref(self, extended=False):
        """How far apart the two float64 routes are."""
        return abs(self.vec(extended).score - self.direct(extended).score)

    def bound(self, extended=False):
        """The accuracy gate: 4 d_ref + one fp32 ulp of the score."""
        return 4.0 * self.d_ref(extended) + R.ulp32(self.vec(extended).score)


def _static():
    n = length_for
    out = [
        # the frame count around the cut, no silent frame
        Case("frames-28", n(28), 100, short=True), Case("frames-29", n(29), 101, short=True),
        Case("frames-30", n(30), 102), Case("frames-31", n(31), 103),
        # one sample either side of a frame start: 256 + 128 k has k - 1 frames, one sample more has k
        Case("start-k31", 256 + 128 * 31, 104), Case("start-k31+1", 256 + 128 * 31 + 1, 105),
        Case("start-k30", 256 + 128 * 30, 106, short=True), Case("start-k30+1", 256 + 128 * 30 + 1, 107),
        # silent stretches: 45 frames before removal (46 energy frames, hops 0 .. 46)
        Case("silent-leading", n(45), 110, silent_hops=range(0, 7)),       # frames 0 .. 5 removed
        Case("silent-trailing", n(45), 111, silent_hops=range(41, 47)),    # frames 41 .. 45 removed
        Case("silent-interior", n(45), 112, silent_hops=range(18, 25)),    # frames 18 .. 23 removed
        Case("silent-alternate", n(60), 113, silent_hops=[h for h in range(62) if h % 3 != 2]),  # every third frame removed
        Case("silent-leaves-30", n(40), 114, silent_hops=range(0, 11)),    # frames 0 .. 9 of 41 removed: 31 kept, 30 frames
        Case("silent-leaves-29", n(40), 115, silent_hops=range(0, 12), short=True),
        # other rates, 41 frames before removal, an interior stretch of five hops (four frames) removed
        Case("fs-8000", 4480, 120, fs=8000, silent_hops=range(20, 25)), Case("fs-16000", 8960, 121, fs=16000, silent_hops=range(9, 14)),
        Case("fs-24000", 13440, 122, fs=24000, silent_hops=range(30, 35)), Case("fs-44100", 24696, 123, fs=44100, silent_hops=range(3, 8)),
        # degenerate and long rows
        Case("one-sample", 1, 130, short=True), Case("T-255", 255, 131, short=True),
        Case("zero-clean", 6000, 132, zero_clean=True),
        Case("long-16000", 48000, 133, fs=16000, silent_hops=range(100, 140)),
    ]
    return out


STATIC = _static()


@functools.lru_cache(maxsize=None)
def tile_cases(tile):
    """Frame counts round the STFT frame tile of the kernel (ou_stoi_frame_tile): tile - 1, tile, tile + 1, two tiles + 1 as the
    issue asks -- below the cut of 30 where the tile is 16 --, and the same round two and three tiles, which score."""
    counts = sorted({tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 3 * tile - 1, 3 * tile, 3 * tile + 1})
    return tuple(Case(f"tile-{j}", length_for(j), 200 + j, short=j < R.SEGMENT) for j in counts)


def table(tile):
    return STATIC + list(tile_cases(tile))


def by_name(name, tile=16):
    return next(c for c in table(tile) if c.name == name)


#: the ragged batch: six rows at 10 kHz mixing the above
RAGGED = [by_name(n) for n in ("frames-29", "start-k30+1", "silent-leading", "T-255", "silent-alternate", "frames-31")]


# ---- the edges the tables above stop short of ----
MASK_CHUNK = 1024  # frames per pass of the kept-frame scan (stoi_mask_kernel)
SEG_TILE_FRAMES = 45  # 16 segments of 30 frames: one segment tile (stoi_seg_kernel); 46 frames start a second


def _edge():
    n = length_for
    out = [
        # energy frames round one and two chunks of the kept-frame scan, no silent frame: length_for(J) has J + 1 of them
        *(Case(f"mask-{e}", n(e - 1), 300 + i) for i, e in enumerate((1023, 1024, 1025, 2048, 2049))),
        # 2101 energy frames, a silent stretch across frame 1024 and one across frame 2048: the running base of chunks 2 and 3
        # is not the chunk's first frame, and kept frames are missing on both sides of each border
        Case("mask-silent-2100", n(2100), 310, silent_hops=list(range(1000, 1040)) + list(range(2040, 2060))),
        # exactly one segment tile, and the first segment of a second
        Case("segtile-45", n(SEG_TILE_FRAMES), 320), Case("segtile-46", n(SEG_TILE_FRAMES + 1), 321),
        # rates: one second each, an interior stretch of five hops removed; 6 kHz up-samples by 5 / 3
        Case("fs-48000", 48000, 330, fs=48000, silent_hops=range(30, 35)), Case("fs-22050", 22050, 331, fs=22050, silent_hops=range(40, 45)),
        Case("fs-6000", 6000, 332, fs=6000, silent_hops=range(20, 25)), Case("fs-12000", 12000, 333, fs=12000, silent_hops=range(50, 55)),
        # 14 s at 48 kHz: the resampler feeds a second chunk of the scan, a silent stretch across energy frame 1024
        Case("long-48000", 14 * 48000, 334, fs=48000, silent_hops=range(1010, 1040)),
    ]
    return out


EDGE = _edge()


def edge_by_name(name):
    return next(c for c in EDGE if c.name == name)


class Many:
    """A ragged call of 130 rows -- launch groups of 64, 64 and 2 -- at one rate.  The rows cycle over a short list of cases, so
    every distinct pair has its references computed once; rows 63, 64, 127 and 128 -- the last and first rows of the groups --
    hold one sample and a row of fewer than 30 frames; `longest_at` (0 or 129) holds the one longest row, so either the first
    group or the last is the one whose grid is as large as the call's strides."""
    ROWS, DEGENERATE = 130, (63, 64, 127, 128)

    def __init__(self, fs, cycle, degenerate, longest, longest_at):
        assert longest.T > max(c.T for c in cycle) and longest_at in (0, self.ROWS - 1) and {c.fs for c in cycle + [longest]} == {fs}
        self.fs, self.longest_at = fs, longest_at
        self.cases = [degenerate[self.DEGENERATE.index(b) % len(degenerate)] if b in self.DEGENERATE else
                      longest if b == longest_at else cycle[b % len(cycle)] for b in range(self.ROWS)]

    def __repr__(self):
        return f"many-fs{self.fs}-longest-at-{self.longest_at}"


def _many():
    n = by_name
    cycle = [n("frames-29"), n("frames-30"), n("start-k31+1"), n("silent-leading"), n("silent-leaves-30"), n("tile-33"),
             edge_by_name("segtile-46")]
    short = [n("one-sample"), n("T-255"), n("frames-28"), n("one-sample")]
    out = [Many(R.FS, cycle, short, n("silent-alternate"), at) for at in (129, 0)]  # the longest row: length_for(60)
    # 16 kHz: rows of 41 and 43 frames before removal and one below the cut, one sample at the group borders, 1.2 s the longest
    cycle16 = [n("fs-16000"), Case("fs-16000-b", 9300, 340, fs=16000, silent_hops=range(20, 24)),
               Case("fs-16000-short", 6000, 341, fs=16000, short=True)]
    short16 = [Case("fs-16000-one-sample", 1, 342, fs=16000, short=True), Case("fs-16000-T-300", 300, 343, fs=16000, short=True)]
    longest16 = Case("fs-16000-long", 19200, 344, fs=16000, silent_hops=range(60, 66))
    return out + [Many(16000, cycle16, short16, longest16, at) for at in (129, 0)]


MANY = _many()
