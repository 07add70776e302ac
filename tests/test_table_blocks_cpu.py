"""CPU: the case lists of tests/table_blocks_cases.py against what tests/test_gpu_table_blocks.py needs of them -- so that a case
which no longer crosses a block fails here instead of passing quietly on the GPU.  For every case: the table launches it implies
are at least 2 (ceil(count / block); a BOUNDARY case has count == block exactly), the rows either side of the first block's edge
hold values no other row has, and the group shapes of the segmented cases are as stated (ou_segment_groups, seg_fp64.last_group).
The host loops are restated (`blocked_table`): a kernel that drops its block offset changes the table of every case and of no
older test of the suite."""
import pytest
import torch

import ensemble_ref as R
import seg_fp64 as G
import snake_fp64 as SN
import table_blocks_cases as K
from helpers import get_spec
from open_universe_amd import _lib


def _unique_at_edges(values, block, what):
    for i in K.edge_rows(len(values), block):
        assert list(values).count(values[i]) == 1, (what, i, values[i])


def _crosses(count, table, boundary=False):
    n = K.launches(count, K.BLOCK[table])
    if boundary:
        assert count == K.BLOCK[table] and n == 1, (table, count)
    else:
        assert n >= 2, (table, count)
    # the restated loop: the true table is the values; a dropped offset shows at this count and at no count the suite had before
    vals = list(range(100, 100 + count))
    assert K.blocked_table(vals, K.BLOCK[table], -1) == vals
    if not boundary:
        assert K.blocked_table(vals, K.BLOCK[table], -1, mut=True) != vals
    old = list(range(K.OLD_MAX[table]))
    assert K.blocked_table(old, K.BLOCK[table], -1, mut=True) == old, (table, "an older test already crossed this block")


def test_block_sizes_are_the_library_s():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "open-universe_amd", "csrc", "ou_kernels.h")) as f:
        src = f.read()

    def found(pattern, what):
        m = re.search(pattern, src)
        assert m is not None, f"ou_kernels.h: {what} not found as `{pattern}` (the header was reworded: adapt this test)"
        return int(m.group(1))

    const = lambda n: found(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % n, n)  # noqa: E731
    assert const("kSegRowsPerLaunch") == K.BLOCK["seg_rows"] and const("kSegEntriesPerLaunch") == K.BLOCK["seg_entries"]
    assert const("kEnsRowsPerLaunch") == K.BLOCK["ens"] and const("kSnakeRowsPerLaunch") == K.BLOCK["snake"]
    assert found(r"struct\s+CoefBlock\s*\{\s*StepCoef\s+c\[(\d+)\]", "struct CoefBlock") == K.BLOCK["coef"]
    assert found(r"struct\s+RowBlock\s*\{\s*int\s+t_raw\[(\d+)\]", "struct RowBlock") == K.BLOCK["rows"]


@pytest.mark.parametrize("name,B", K.SCORE_CASES)
def test_score_cases(name, B):
    spec = get_spec(name)
    _crosses(B, "coef")
    sig = K.score_sigmas(spec, B)
    assert sig.dtype == torch.float32 and len(set(sig.tolist())) == B  # every row its own: the edge rows among them
    _unique_at_edges(sig.tolist(), 64, "sigma")
    assert abs(float(sig.min()) / spec.sigma_min - 1) < 1e-6 and abs(float(sig.max()) / spec.sigma_max - 1) < 1e-6
    assert not torch.equal(sig, sig.sort().values)  # shuffled
    if name.startswith("OR16"):
        assert spec.score.time_embedding != "simple" and spec.edm_noise is None  # the random-Fourier-feature MLP
    else:
        assert spec.score.time_embedding == "simple"


@pytest.mark.parametrize("N", K.STEP_N)
def test_step_table_cases(N):
    spec = get_spec(K.STEP_MODEL)
    _crosses(N, "coef", boundary=N == 64)
    sig = K.sigma_table(spec, N)
    assert len(set(sig.tolist())) == N and bool((sig[1:] < sig[:-1]).all())
    _unique_at_edges(sig.tolist(), 64, "step sigma")
    assert 2 <= N <= 256
    assert {64, 65, 66, 129, 256} == set(K.STEP_N)


@pytest.mark.parametrize("name,B", K.RAGGED_CASES)
def test_ragged_cases(name, B):
    td = get_spec(name).tot_ds
    _crosses(B, "rows")
    assert B % 64 != 0  # the table is [level][B]
    frames, t_raw = K.ragged_rows(B, td)
    assert all(1 <= f <= 5 for f in frames) and set(frames) == {1, 2, 3, 4, 5}
    assert all(n + (td - n % td) == f * td for f, n in zip(frames, t_raw))
    assert all(a != b for a, b in zip(frames, frames[1:]))  # every level's length differs between neighbours
    _unique_at_edges(t_raw, 64, "t_raw")
    assert t_raw[63] == min(t_raw) and t_raw[64] == max(t_raw)
    assert K.ALONE_ROWS(B) == sorted({0, 63, 64, B - 1})
    # a dropped offset in the lens index alone: row 0 would get the frames of row 64, which differ
    lens = K.blocked_table(frames, 64, 1, mut=True)
    assert lens[0] != frames[0] and lens[64] is None


def _groups(lens, td, max_batch, E):
    Sg, Ov = G.seg_so(td)
    geos = [G.Row(n, td, Sg, Ov) for n in lens]
    return geos, G.last_group(geos, max_batch, True, E)


@pytest.mark.parametrize("E", sorted(K.SEG_MANY))
def test_segmented_many_rows(E):
    td = get_spec(K.SEG_MODEL).tot_ds
    S = 16 * td
    lens = K.seg_many_rows(td)
    C = len(lens)
    assert C == 70 and C > 64
    _crosses(C, "seg_rows")
    geos, (Bw, real, slots, n_groups, T) = _groups(lens, td, K.SEG_MANY[E], E)
    single = [n for n, g in zip(lens, geos) if g.n_win == 1]
    multi = [c for c, g in enumerate(geos) if g.n_win > 1]
    assert len(single) == 68 and multi == [0, 64]
    assert len(set(single)) == 68 and max(single) == S - 1 and {1, 57, S - 1} <= set(single)
    assert geos[0].t_raw == S and geos[0].n_win == 2  # (S raw samples pad past S)
    _unique_at_edges(lens, 64, "segment rows")
    assert lens[65] == min(lens) and lens[64] == max(lens)
    # the last group: the 68 single-window rows, one ragged walk of Bw = 68 rows
    assert K.SEG_MANY[E] // E == 96
    assert Bw >= 65 and len(real) >= 65 and Bw == 68 and len(real) == 68 and n_groups == 2
    _crosses(len(real), "seg_entries")
    assert all(k == 0 for _, k in real) and [c for c, _ in real] == [c for c in range(C) if c not in multi]
    assert E * Bw >= (130 if E == 2 else 65)
    ent_len = [geos[c].L for c, _ in slots]
    assert ent_len[63] == td and ent_len[64] == S and ent_len[65] == 9 * td and T == S
    assert ent_len[62] != ent_len[63] and ent_len[65] != ent_len[66]
    assert [geos[c].t_raw for c, _ in slots[63:66]] == [1, S - 1, 9 * td - 5]
    # a dropped j0 in slot(): the second block's entries would land on the walk rows 0 .. 3
    rows = [c for c, _ in slots]
    assert K.blocked_table(rows, 64, rows[-1], mut=True)[:4] == rows[64:68] != rows[:4]


@pytest.mark.parametrize("n_real", K.SEG_EXACT)
def test_segmented_exact_blocks(n_real):
    td = get_spec(K.SEG_MODEL).tot_ds
    lens = K.seg_exact_rows(td, n_real)
    geos, (Bw, real, slots, n_groups, T) = _groups(lens, td, n_real, 1)
    assert all(g.n_win > 1 for g in geos) and sum(g.n_win for g in geos) == 2 * n_real
    assert Bw == n_real and len(real) == n_real and slots == real and n_groups == 2  # no filler, no short block
    _crosses(n_real, "seg_entries", boundary=n_real == 64)
    assert n_real % K.BLOCK["seg_entries"] == 0
    assert real[0][1] > 0  # the group's first entry has seg.carry in front of it
    for j in range(0, n_real, 64):  # ... and every launch block starts on a window with a window in front
        assert real[j][1] > 0 and (j == 0 or real[j - 1] == (real[j][0], real[j][1] - 1))
    # ou_segment_groups itself
    Gr = _lib.segment_groups(td, lens, 16 * td, 2 * td, n_real)
    assert int(Gr["batch"]) == n_real and [int(v) for v in Gr["group_first"]] == [0, n_real]


@pytest.mark.parametrize("B", K.ENS_B)
@pytest.mark.parametrize("cols", K.ENS_COLS)
def test_ensemble_cases(B, cols):
    _crosses(B, "ens", boundary=B == 16)
    lens = K.ens_lens(B, cols)
    assert len(lens) == B and all(1 <= v <= cols for v in lens) and 1 in lens and cols in lens
    if cols >= B:
        assert len(set(lens)) == B
        _unique_at_edges(lens, 16, "len")
        assert lens[15] == 1 and (B == 16 or lens[16] == cols)
    else:  # three lengths for more than three inputs: the neighbours differ and the edge inputs hold all three
        assert all(a != b for a, b in zip(lens[14:], lens[15:]))
        assert B == 16 or {lens[15], lens[16]} == {1, cols}
    assert set(K.ENS_E) == {2, 3, 8, 32} and set(K.ENS_COLS) == {3, 4097}
    off, on = K.ens_strides(cols)
    assert off >= cols and on >= cols and off % 4 != 0 and on % 4 == 0  # vec_ok of ou_ensemble.hip: row_stride % 4 == 0
    assert -(-max(K.ENS_COLS) // 1024) > 1  # more than one column block per input (1024 columns per block)


@pytest.mark.parametrize("E", K.ENS_E)
def test_input_16_picks_another_member_than_input_0(E):
    """... in every case with a second launch, by the restatement alone; a pick kernel that drops b0 would give input 16 the
    pick (and the length) of input 0."""
    for B in K.ENS_B:
        if B <= 16:
            continue
        for cols in K.ENS_COLS:
            x, lens = K.ens_members(E, B, cols)
            pick = R.reduce_ref(x[:, [0, 16]], "signal_median", [lens[0], lens[16]])[1]
            assert int(pick[0]) != int(pick[1]), (E, B, cols)
            assert lens[0] != lens[16]


@pytest.mark.parametrize("B", K.SNAKE_B)
def test_snake_cases(B):
    tile = SN.ref_error()["tile"]
    assert tile == _lib.load().ou_snake_tile()
    _crosses(B, "snake")
    T = K.snake_T(tile)
    lens = K.snake_lens(B, tile)
    assert len(lens) == B and all(1 <= v <= T for v in lens)
    _unique_at_edges(lens, 64, "snake len")
    assert lens[63] == 1 == min(lens) and lens[64] == T == max(lens)
    for e in (tile, 2 * tile):  # either side of every tile edge
        assert {e - 1, e, e + 1} <= set(lens)
    assert all(a != b for a, b in zip(lens, lens[1:]))
    assert K.SNAKE_C == 2 and set(K.SNAKE_B) == {65, 130}
