"""Case lists of tests/test_gpu_table_blocks.py: every by-value row table of the library driven past its first block.

The library hands per-row values to its kernels as kernel arguments, a fixed block at a time, and a host loop issues one launch
per block with an offset.  A case of this module makes that loop take at least two turns (BLOCK[table] rows per launch; counts of
block + 1 and 2 block + 1), and gives the rows either side of the first block's edge -- indices block - 1, block, block + 1 --
values that no other row of the call has, so that a repeated, swapped or dropped row cannot compare equal.  Cases whose count IS
the block (`BOUNDARY`: count == block, one full launch, no short one behind it) are listed beside them: N = 64, B = 16, 64 entries.
tests/test_table_blocks_cpu.py holds all of this against the lists, without a GPU; `blocked_table` there restates the host loops."""
import math

import torch

# rows per launch of every table (ou_kernels.h: CoefBlock, RowBlock, kSegRowsPerLaunch, kSegEntriesPerLaunch, kEnsRowsPerLaunch,
# kSnakeRowsPerLaunch)
BLOCK = {"coef": 64, "rows": 64, "seg_rows": 64, "seg_entries": 64, "ens": 16, "snake": 64}
# the largest count any older test of the suite reaches, per table (what `blocked_table`'s mutants must leave unchanged)
OLD_MAX = {"coef": 64, "rows": 12, "seg_rows": 6, "seg_entries": 32, "ens": 3, "snake": 3}


def launches(count, block):
    return -(-count // block)


def edge_rows(count, block):
    """The rows either side of the first block's edge that the call has."""
    return [i for i in (block - 1, block, block + 1) if i < count]


def blocked_table(values, block, filler, mut=False):
    """The host loop of every table, restated: `block` values per launch, `filler` behind the n real ones, launch `off` writes
    dst[off + i] = blk[i] for i < n.  mut: the kernel drops the offset (dst[i]) -- the class of error the cases exist for.
    -> the table as the device holds it (None: never written)."""
    dst = [None] * len(values)
    for off in range(0, len(values), block):
        n = min(block, len(values) - off)
        blk = [values[off + i] if i < n else filler for i in range(block)]
        for i in range(n):
            dst[(0 if mut else off) + i] = blk[i]
    return dst


# ---- 1. coefficient, embedding and FiLM rows ---------------------------------------------------------------------------------
# (a) ou_score: (model, B) at one frame.  OR16s: the random-Fourier-feature embedding (and the plain, non-EDM score).
SCORE_CASES = [("PP16s", 65), ("PP16s", 129), ("OR16s", 65)]
# (b) the sampler's step table: enhance(n_steps = N, warm_start = N - 1) is one step at table row N - 1.  N = 64 is the BOUNDARY
# case (one full launch); 256 = kMaxSteps.
STEP_MODEL, STEP_B, STEP_FRAMES = "PP16s", 3, 3
STEP_N = (64, 65, 66, 129, 256)


def score_sigmas(spec, B, seed=11):
    """B per-row sigmas, log-spaced over [sigma_min, sigma_max] (fp32), shuffled with a fixed seed: every row its own."""
    s = torch.logspace(math.log10(spec.sigma_min), math.log10(spec.sigma_max), B, dtype=torch.float64).float()
    return s[torch.randperm(B, generator=torch.Generator().manual_seed(seed))].contiguous()


def sigma_table(spec, N):
    """The host's schedule (Universe._sigma_table) from the spec alone."""
    time = torch.linspace(0, 1, N).to(torch.float32).flip(dims=[0])
    return (spec.sigma_min * (spec.sigma_max / spec.sigma_min) ** time).to(torch.float32)


# ---- 2. ragged batch (ou_enhance_var) ------------------------------------------------------------------------------------------
RAGGED_CASES = [("PP16s", 65), ("PP16s", 129), ("PP24s", 65)]
ALONE_ROWS = lambda B: sorted({0, 63, 64, B - 1})  # noqa: E731


def ragged_rows(B, td):
    """-> (frames, t_raw) per row.  Frames cycle through 1 .. 5, so every level's length differs between neighbouring rows; the
    raw lengths are frames * td - (3 + row % 7).  Rows 63, 64, 65 hold the call's shortest row (1 sample), its longest
    (5 td - 1) and a length of their own (3 td - 11)."""
    frames = [1 + i % 5 for i in range(B)]
    t_raw = [f * td - 3 - i % 7 for i, f in enumerate(frames)]
    for i, (f, n) in {63: (1, 1), 64: (5, 5 * td - 1), 65: (3, 3 * td - 11)}.items():
        if i < B:
            frames[i], t_raw[i] = f, n
    return frames, t_raw


# ---- 3. segmented ragged call ----------------------------------------------------------------------------------------------------
SEG_MODEL = "PP16s"
SEG_C = 70


def seg_many_rows(td):
    """3 (a) / (b): C = 70 rows, S = 16 td, O = 2 td.  Rows 0 and 64 have several windows (row 0: S raw samples, which pad to
    S + td -- two windows, the second one shifted; row 64: 70 td + 3, five windows, the call's longest); the other 68 have one
    window and lengths of their own <= S - 1, among them 1, 57 and S - 1 (a row of S raw samples cannot be one of them: it pads
    past S).  Single-window row i has frames 1 + 5 i mod 16 (neighbours 5 frames apart) and t_raw = frames * td - (1 + i).
    In input order the rows 63, 64, 65 hold 7 td - 63, the longest row and the shortest (1); the last group's entries 63, 64, 65 are the
    rows 65, 66, 67: 1 sample (length td), S - 1 (length S) and 9 td - 5."""
    S = 16 * td
    single = [(1 + (5 * i) % 16) * td - (1 + i) for i in range(68)]
    single[2], single[63], single[64], single[65] = 57, 1, S - 1, 9 * td - 5
    lens = [S] + single[:63] + [70 * td + 3] + single[63:]
    assert len(lens) == SEG_C
    return lens


# max_batch of 3 (a) and of 3 (b) with E = 2 members (a group holds max_batch / E entries: the same groups as (a))
SEG_MANY = {1: 96, 2: 192}


def seg_exact_rows(td, n_real):
    """3 (c): rows of several windows only (no SHORT group: the last group is FULL), 2 n_real entries in two groups of n_real at
    max_batch = n_real.  One row of 3 windows, then rows of 2, then one of 3: the entries 3 + 2 i are second windows, so the last
    group's first entry (entry n_real of the call) is a second window with seg.carry in front of it, and so is the first entry of
    every 64-entry launch block inside the group (its window in front is the walk row of the block before)."""
    assert n_real % 64 == 0
    two = (2 * n_real - 6) // 2
    return [41 * td + 7] + [(17 + i % 13) * td + 1 + i % 7 for i in range(two)] + [41 * td + 7]


SEG_EXACT = (64, 128)  # real entries of the last group = max_batch = Bw

# ---- 4. ensemble reduce ----------------------------------------------------------------------------------------------------------
ENS_B = (16, 17, 33)  # 16: the BOUNDARY case
ENS_E = (2, 3, 8, 32)
ENS_COLS = (3, 4097)


def ens_strides(cols):
    """Row strides of the members and of the output: one off 16-byte boundaries (rs % 4 != 0: the kernels go word by word), one
    on them (rs % 4 == 0: 16-byte loads and stores wherever a whole quad is valid).  3 -> 7, 8; 4097 -> 4101, 4104."""
    return ((cols + 3) | 1, (cols + 8) // 4 * 4)


def ens_lens(B, cols):
    """Valid samples per input.  cols 4097: all different, input 15 has 1 and input 16 all of them.  cols 3 has three lengths
    only: they cycle, neighbours differ, and the inputs 15, 16, 17 hold 1, 3, 2."""
    if cols < B:
        lens = [1 + (2 * i) % cols for i in range(B)]
        for i, v in {15: 1, 16: cols, 17: 2}.items():
            if i < B:
                lens[i] = v
        return lens
    lens = [cols - 97 * i for i in range(B)]
    lens[15] = 1
    if B > 16:
        lens[0], lens[16] = lens[16], lens[0]
    assert len(set(lens)) == B and min(lens) == 1 and all(1 <= v <= cols for v in lens)
    return lens


def ens_members(E, B, cols, ties=False):
    """Seeded members (ensemble_ref.draw_members).  With a second launch (B > 16) the candidate members of the signal median are
    moved 4 down for input 0 and 4 up for input 16: input 0 then picks rank position 0 and input 16 the last position its
    candidates can take -- another member, whatever E (with E = 3 and random members alone both would pick position 0)."""
    import ensemble_ref as R

    lens = ens_lens(B, cols)
    x = R.draw_members(E, B, cols, seed=50000 + 1000 * E + 10 * B + cols % 7, ties=ties)
    if B > 16:
        c = R.candidates(E)
        x[c, 0] -= 4.0
        x[c, 16] += 4.0
    return x, lens


# ---- 5. stateless Snake -----------------------------------------------------------------------------------------------------------
SNAKE_B = (65, 130)
SNAKE_C = 2


def snake_T(tile):
    return 2 * tile + 5


def snake_lens(B, tile):
    """Row lengths either side of the tile edges, cycling; rows 63, 64, 65: 1 (the shortest), T (the longest), 2 tile + 3."""
    T = snake_T(tile)
    cyc = (tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1)
    lens = [cyc[i % len(cyc)] for i in range(B)]
    for i, v in {63: 1, 64: T, 65: 2 * tile + 3}.items():
        if i < B:
            lens[i] = v
    return lens
