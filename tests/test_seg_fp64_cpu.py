"""CPU: the checks of tests/seg_fp64.py bite.  A plain fp32 restatement of every segmented-enhance operation in the kernel's order
of operations passes its check at the shapes of tests/test_gpu_seg_fp64.py; every mutation of it fails.  Also: the module's
float64 crossfade weights against _lib.segment_weights, and the alignment / residue coverage of the GPU cases from the lengths
alone.  The walk's output is stood in for by random windows (no network runs here)."""
import pytest
import torch

import seg_fp64 as G
import small_fp64 as F
from helpers import get_spec
from open_universe_amd import _lib
from open_universe_amd import state_dict as S

TD = {m: get_spec(m).tot_ds for m in G.MODELS}
_td = sorted(set(TD.values()))


def _windows(n, T, seed):
    return 0.05 * torch.randn(n, 1, T, generator=torch.Generator().manual_seed(seed))


def _scene(td, kind):
    """(geos, max_batch, ragged, E) of a GPU case."""
    Sg, Ov = G.seg_so(td)
    if kind.startswith("len"):
        return [G.Row(G.lengths(td)[int(kind[3:])], td, Sg, Ov)] * 2, 32, False, 1
    if kind == "O0":
        return [G.Row(58 * td + 3, td, Sg, 0)] * 2, 32, False, 1
    if kind == "Ohalf":
        return [G.Row(58 * td + 3, td, Sg, Sg // 2)] * 2, 32, False, 1
    if kind == "carry":
        return [G.Row(G.CARRY_LENGTH(td), td, Sg, Ov)] * 2, 4, False, 1
    if kind == "ragged":
        return [G.Row(n, td, Sg, Ov) for n in G.ragged_lengths(td)], 32, True, 1
    if kind == "ragged_multi":
        return [G.Row(n, td, Sg, Ov) for n in G.ragged_multi(td)], 4, True, 1
    if kind == "ens":
        return [G.Row(41 * td + 7, td, Sg, Ov)] * 2, 32, False, 2
    if kind == "ens_ragged":
        return [G.Row(n, td, Sg, Ov) for n in (41 * td + 7, 57, 16 * td)], 32, True, 2
    raise KeyError(kind)


KINDS = [f"len{i}" for i in range(10)] + ["O0", "Ohalf", "carry", "ragged", "ragged_multi", "ens", "ens_ragged"]


def _stitch_case(td, kind, mut=(), seed=3):
    geos, mb, ragged, E = _scene(td, kind)
    C = len(geos)
    Bw, real, slots, n_groups, T = G.last_group(geos, mb, ragged, E)
    y = _windows(E * Bw, T, seed)
    for m in range(E):  # (the walk's rows are 0 behind an entry's length)
        for j, (c, _) in enumerate(slots):
            y[m * Bw + j, 0, geos[c].L:] = 0
    carry = _windows(E, T, seed + 1) if real[0][1] > 0 else None
    stride = max(g.t_raw for g in geos)
    out = G.stitch(geos, real, y, carry, Bw, E, C, stride, dtype=torch.float32, mut=mut)
    if ragged:
        for q in range(E * C):
            out[q, geos[q % C].t_raw:] = 0
    # what no entry of the last group writes stays with the earlier groups: the check does not look at it
    rep = G.check_stitch(out, geos, real, y, carry, Bw, E, C, whole=n_groups == 1, tails=ragged)
    return rep, geos, real


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("td", _td)
def test_stitch_restatement_passes_and_mutants_fail(td, kind):
    rep, geos, real = _stitch_case(td, kind)
    assert rep.ok() and rep.excluded == 0, str(rep)
    # (the restatement's weights ARE the fp32 torch evaluation: what is left over e32 is the three roundings the figure carries)
    assert rep.e32 == 0 or rep.lib_ratio <= 1.0 + 3 * F.U / rep.e32, (rep.lib_ratio, rep.e32)
    faded = any(k > 0 and geos[c].O > 0 for c, k in real)
    cut = any(k > 0 for c, k in real)
    shifted = any(k == geos[c].n_win - 1 and k > 0 and geos[c].starts[k] != k * geos[c].hop for c, k in real)
    for mut, applies in (("no_half", faded), ("swap", faded), ("fade_plus1", faded), ("w0_off", cut), ("no_shift", shifted)):
        if applies:
            bad, _, _ = _stitch_case(td, kind, (mut,))
            assert not bad.ok(), (kind, mut, str(bad))
    # the 16-byte mover's single words: the mutants show wherever a span has any
    singles = False
    C = len(geos)
    stride = max(g.t_raw for g in geos)
    for c, k in real:
        g = geos[c]
        s, _, w0, w1, _ = g.window(k)
        u0, u1 = max(w0, g.pad_left, s), min(w1, g.pad_left + g.t_raw, s + g.L)
        if u1 > u0:
            n, head = u1 - u0, min(G.dest_head(c * stride + u0 - g.pad_left), u1 - u0)
            singles = singles or head > 0 or (n - head) % 4 > 0
    if singles:
        for mut in ("drop_first", "drop_last"):
            bad, _, _ = _stitch_case(td, kind, (mut,))
            assert not bad.ok(), (kind, mut, str(bad))
    if kind.startswith("len") and int(kind[3:]) >= 5:
        assert singles, kind  # (odd row stride: row 1 starts off a 16-byte boundary)


@pytest.mark.parametrize("td", _td)
def test_the_edge_cases_hold_a_shifted_last_window(td):
    Sg, Ov = G.seg_so(td)
    for O in (0, Sg // 2):
        g = G.Row(58 * td + 3, td, Sg, O)
        assert g.n_win >= 4 and g.O == O
        assert g.starts[-1] != (g.n_win - 1) * g.hop, "the last window of the overlap edge case is not shifted"
    g = G.Row(16 * td, td, Sg, Ov)
    assert g.n_win == 2 and g.starts[1] == td


@pytest.mark.parametrize("td", _td)
def test_coverage_of_the_one_group_lengths(td):
    t4, p4, heads, wins = G.coverage(td)
    assert t4 == {0, 1, 2, 3} and p4 == {0, 1, 2, 3} and heads == {0, 1, 2, 3}, (t4, p4, heads)
    Sg, Ov = G.seg_so(td)
    assert all(3 <= G.Row(n, td, Sg, Ov).n_win <= 5 and n % 2 == 1 or n == 30 * td + 2 for n in G.lengths(td)[5:])
    assert G.Row(16 * td - 1, td, Sg, Ov).T_pad == Sg and G.Row(16 * td, td, Sg, Ov).n_win == 2
    # the carry case: the last group is not the first and starts inside a row
    geos = [G.Row(G.CARRY_LENGTH(td), td, Sg, Ov)] * 2
    Bw, real, _, n_groups, _ = G.last_group(geos, 4, False)
    assert n_groups > 1 and real[0][1] > 0
    # the ragged call: one FULL and one SHORT group, the SHORT one last; only multi-window rows: the last group FULL with a carry
    rows = [G.Row(n, td, Sg, Ov) for n in G.ragged_lengths(td)]
    Bw, groups, full = G.groups_ragged(rows, td, Sg, Ov, 32)
    assert full == [True, False] and len({rows[c].L for c, _ in groups[1]}) > 1
    rows = [G.Row(n, td, Sg, Ov) for n in G.ragged_multi(td)]
    Bw, groups, full = G.groups_ragged(rows, td, Sg, Ov, 4)
    assert len(groups) > 1 and all(full) and groups[-1][0][1] > 0
    # multi-block: 2 blocks alike; 2 / 1 / 3 blocks of a stride of 3 ragged
    nb = lambda n: max(1, -(-n // 2 ** 18))  # noqa: E731
    assert nb(G.MULTI_BLOCK_ALIKE) == 2 and [nb(n) for n in G.MULTI_BLOCK_RAGGED] == [2, 1, 3]


def test_float64_weights_against_the_library_helper():
    """The plans of tests/test_segments_cpu.py: the module's a(i) in float64 against _lib.segment_weights (fp32), rising and
    falling side, within the fp32 evaluation's own error; 1 and 0 elsewhere exactly."""
    TOT, SEG, OV = 256, 8 * 16000, 16000
    for T_raw in (1, TOT, 5 * TOT, SEG - TOT, SEG + 1, 3 * SEG + 77, 10 * SEG):
        for ov in (0, TOT, OV, SEG // 2):
            p = _lib.segment_plan(TOT, T_raw, SEG, ov)
            g = G.Row(T_raw, TOT, SEG, ov)
            for k in range(g.n_win):
                w = torch.from_numpy(_lib.segment_weights(p, k)).double()
                s, sp, w0, w1, e_prev = g.window(k)
                u = torch.arange(s, s + g.L)
                want = ((u >= w0) & (u < w1)).double()
                if k > 0 and g.O > 0:
                    m = (u >= w0) & (u < e_prev)
                    want[m] = G.weight(u[m] - w0, g.O)
                if k < g.n_win - 1 and g.O > 0:
                    m = u >= w1
                    want[m] = 1.0 - G.weight(u[m] - w1, g.O)
                tol = 4 * G.weight_e32(g.O) + 2 * F.U if g.O else 0.0
                assert float((w - want).abs().max()) <= tol, (T_raw, ov, k)


# ---- statistics ----------------------------------------------------------------------------------------------------------------
def _rows(spec, lens, seed=0):
    return G.case_mix(spec, lens, seed)


@pytest.mark.parametrize("model", G.MODELS)
def test_statistics_restatement_and_mutants(model):
    spec = get_spec(model)
    td = spec.tot_ds
    lens_small = [n for n in G.lengths(td)] + G.ragged_lengths(td)
    for norm, zm in G.NORM_MODES:
        for n in (1, 16 * td - 1):
            rows = _rows(spec, [n, n])
            st = torch.stack([G.stats_fp32(x, td, spec.level_db, norm, zm) for x in rows])
            rep = G.check_stats(st, rows, td, spec.level_db, norm, zm)
            assert rep.ok() and rep.excluded == 0, (norm, zm, n, str(rep))
    for lens in ([n, n] for n in lens_small + [G.MULTI_BLOCK_ALIKE]):
        rows = _rows(spec, lens)
        st = torch.stack([G.stats_fp32(x, td, spec.level_db) for x in rows])
        rep = G.check_stats(st, rows, td, spec.level_db)
        assert rep.ok() and rep.excluded == 0, (lens, str(rep))
        for mut in ("mean_traw", "biased", "no_pad_term"):
            bad = G.check_stats(torch.stack([G.stats_fp32(x, td, spec.level_db, mut=(mut,)) for x in rows]), rows, td, spec.level_db)
            assert not bad.ok(), (lens, mut, str(bad))
    # rows exchanged: the 1e-3 between the rows shows
    rows = _rows(spec, [41 * td + 7] * 2)
    st = torch.stack([G.stats_fp32(x, td, spec.level_db) for x in rows])
    assert not G.check_stats(st.flip(0), rows, td, spec.level_db).ok()


@pytest.mark.parametrize("model", G.MODELS)
def test_gather_restatement_and_mutants(model):
    spec = get_spec(model)
    td = spec.tot_ds
    for kind in KINDS:
        geos, mb, ragged, E = _scene(td, kind)
        Bw, real, slots, _, T = G.last_group(geos, mb, ragged, E)
        rows = _rows(spec, [g.t_raw for g in geos])
        st = torch.stack([G.stats_fp32(x, td, spec.level_db) for x in rows])
        mixn = G.gather_input(rows, geos, st, slots, T, torch.float32)[0]
        rep = G.check_gather(mixn, rows, geos, st, slots)
        assert rep.ok() and rep.excluded == 0, (kind, str(rep))
        muts = ["pad_plus", "pad_minus"]
        if any(c == 1 for c, _ in slots):
            muts.append("row0_stats")
        if any(geos[c].L < T for c, _ in slots):
            muts.append("no_tail_zero")
        for mut in muts:
            bad = G.check_gather(G.gather_input(rows, geos, st, slots, T, torch.float32, (mut,))[0], rows, geos, st, slots)
            assert not bad.ok(), (kind, mut, str(bad))
        # the noise gather: exact, and a copy from one sample off is not
        nz = torch.randn(E * len(geos), max(g.T_pad for g in geos), generator=torch.Generator().manual_seed(5))
        z, _ = G.gather_noise(nz, geos, slots, Bw, E, len(geos), T)
        assert G.check_noise(z, nz, geos, slots, Bw, E, len(geos)).ok()
        assert not G.check_noise(z.roll(1, -1), nz, geos, slots, Bw, E, len(geos)).ok()


@pytest.mark.parametrize("model", G.MODELS)
def test_post_restatement_and_mutants(model):
    """The stitched rows are stood in for by the restatement's stitch of random windows at the walk's level; the loud row makes
    the guard divide, and the reference's max|x| g stays clear of 1 by more than the bound, so the branch is never ambiguous."""
    spec = get_spec(model)
    td = spec.tot_ds
    for kind in ("len0", "len1", "len2", "len5", "len8", "ragged", "ens"):
        geos, mb, ragged, E = _scene(td, kind)
        C = len(geos)
        stride = max(g.t_raw for g in geos)
        x = 0.05 * torch.randn(E * C, stride, generator=torch.Generator().manual_seed(11))
        for q in range(E * C):
            x[q, geos[q % C].t_raw:] = 0
        rows = _rows(spec, [g.t_raw for g in geos])
        out = G.post_fp32(x, rows, geos, E)
        rep, divided, margin = G.check_post(out, x, rows, geos, E)
        assert rep.ok() and rep.excluded == 0, (kind, str(rep))
        assert divided[0] and not divided[1], (kind, divided)
        assert margin > 1.0, (kind, margin)
        for mut in ("rms_tpad", "guard_nogain"):
            bad, _, _ = G.check_post(G.post_fp32(x, rows, geos, E, (mut,)), x, rows, geos, E)
            assert not bad.ok(), (kind, mut, str(bad))


def test_row_scale_restatement_passes():
    """The whole-row mel scale in fp32 (small_fp64.mel's fp32 evaluation on the row normalised in fp32) is inside the bound, and a
    scale taken over one frame more is not."""
    spec = get_spec("PP16s")
    td = spec.tot_ds
    P = F.Params(spec, S.synthetic_state_dict(spec, seed=0))
    Sg, Ov = G.seg_so(td)
    lens = [41 * td + 7, 16 * td - 1]
    geos = [G.Row(n, td, Sg, Ov) for n in lens]
    rows = _rows(spec, lens)
    st = torch.stack([G.stats_fp32(x, td, spec.level_db) for x in rows])
    sc = torch.tensor([G.row_scale(rows[c], geos[c], st[c, 0], st[c, 1], P, torch.float32)[0] for c in range(2)])
    rep = G.check_row_scale(sc, rows, geos, st, P)
    assert rep.ok() and rep.excluded == 0, str(rep)
    frames = torch.tensor([g.T_pad // td for g in geos], dtype=torch.float32)
    assert not G.check_row_scale(sc * torch.sqrt((frames + 1) / frames), rows, geos, st, P).ok()
    assert not G.check_row_scale(sc.flip(0), rows, geos, st, P).ok()
