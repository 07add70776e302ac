"""CPU tests of the checks of tests/rate_fp64.py themselves (no GPU): an fp32 torch emulation of every form at reduced width stays
within its bound (ratios printed), every defect a rate-change / 1x1 kernel could have is flagged at the element where it was made,
and the pairing of profile records with the walk survives colliding FLOPs."""
import types

import pytest
import torch

import rate_fp64 as R
from small_fp64 import Report

F32 = torch.float32


def _layer(up, Cin=16, Cout=32, r=4, aa=True, seed=0):
    """A RateL at reduced width with an ASYMMETRIC filter (the shipped binomial one is symmetric: a reversed filter would not show)."""
    g = torch.Generator().manual_seed(seed)
    rl = R.RateL.__new__(R.RateL)
    rl.name, rl.tap, rl.up, rl.r, rl.Cin, rl.Cout, rl.aa = "t", "t", up, r, Cin, Cout, aa
    shape = (Cin, Cout, r) if up else (Cout, Cin, r)
    rl.w64 = (torch.randn(shape, generator=g) / (Cin * r) ** 0.5).float().double()
    rl.w = rl.w64.float()
    rl.f = (torch.rand(2 * r + 1, generator=g) + 0.1).float() if aa else None
    rl.b = torch.randn(Cout, generator=g).float()
    rl.alpha = torch.tensor(0.2)
    return rl


def _x(B, Cc, T, seed=1):
    return torch.randn(B, Cc, T, generator=torch.Generator().manual_seed(seed)).float()


def _flagged(rep, b, t, name):
    """The report fails, and it does at (row b, frame t) -- on some channel."""
    assert not rep.ok(), name
    assert bool(rep.bad[b, :, t].any()), (name, "not flagged where it was made", rep.worst)


# ---- the fp32 emulations stay within their bounds ----------------------------------------------------------------------------
@pytest.mark.parametrize("form,aa", [("conv", False), ("fused", True), ("folded", True), ("after_fir", True)])
def test_down_forms_within_bound(form, aa):
    rl = _layer(False, aa=aa)
    x = _x(2, rl.Cin, 4 * 65)
    src = R._fir(R.prelu(x, rl.alpha), rl.f, F32) if form == "after_fir" else x
    ref, bound = R.down(src, rl, form)
    y, _ = R.down(src, rl, form, dtype=F32)
    rep = Report(form, y, ref, bound)
    print(f"down {form}: err / bound {rep.ratio:.3f}")
    assert rep.ok() and rep.excluded == 0 and 0 < rep.ratio < 1


@pytest.mark.parametrize("form,aa", [("conv", False), ("upc", True), ("fused", True), ("folded", True)])
def test_up_forms_within_bound(form, aa):
    rl = _layer(True, Cin=32, Cout=16, aa=aa)
    x = _x(2, rl.Cin, 65)
    res = None if form in ("conv", "upc") else _x(2, rl.Cout, 65 * rl.r, seed=2)
    ref, bound = R.up(x, rl, form, res)
    y, _ = R.up(x, rl, form, res, dtype=F32)
    rep = Report(form, y, ref, bound)
    print(f"up {form}: err / bound {rep.ratio:.3f}")
    assert rep.ok() and rep.excluded == 0 and 0 < rep.ratio < 1


def test_1x1_forms_within_bound():
    g = torch.Generator().manual_seed(3)
    for Cin, KW, scaled in ((640, 1, False), (32, 1, False), (80, 3, True)):
        ol = types.SimpleNamespace(w=(torch.randn(24, Cin, KW, generator=g) / Cin ** 0.5).float(), b=torch.randn(24, generator=g).float())
        x = _x(3, Cin, 13)
        sc = torch.tensor([0.5, 3.0, 11.0]) if scaled else None
        ref, bound = R.conv_1x1(x, ol, sc)
        y, _ = R.conv_1x1(x, ol, sc, dtype=F32)
        rep = Report("1x1", y, ref, bound)
        print(f"1x1 K = {Cin * KW}: err / bound {rep.ratio:.3f}")
        assert rep.ok() and rep.excluded == 0 and 0 < rep.ratio < 1


# ---- injected defects ---------------------------------------------------------------------------------------------------------
def test_halo_frame_of_the_up_fir_read_as_zero_at_a_tile_seam():
    """rate_up_kernel finishes 62 frames per block: frame 62 is the halo of the first block, frame 61 of the second."""
    rl = _layer(True, Cin=32, Cout=16)
    x, res = _x(1, rl.Cin, 130), _x(1, rl.Cout, 130 * rl.r, seed=2)
    ref, bound = R.up(x, rl, "fused", res)
    # the block that finishes frames 0 .. 61 sees frame 62 as zero: its own outputs of frame 61 are wrong
    uu = R._phases(R._gemm(R.prelu(x, rl.alpha), rl.rows(), dtype=F32), rl.r)
    halo_zero = uu.clone()
    halo_zero[..., 62 * rl.r: 63 * rl.r] = 0
    good = R._fir(uu, rl.f, F32)
    bad = good.clone()
    bad[..., 61 * rl.r: 62 * rl.r] = R._fir(halo_zero, rl.f, F32)[..., 61 * rl.r: 62 * rl.r]
    s2 = torch.tensor(R.F.INV_SQRT2)
    y = ((bad + rl.b[None, :, None]) + res) * s2
    rep = Report("halo", y, ref, bound)
    _flagged(rep, 0, 62 * rl.r - 1, "halo frame read as zero")
    assert not bool(rep.bad[..., : 61 * rl.r].any()) and not bool(rep.bad[..., 62 * rl.r:].any())


def test_edge_replication_instead_of_zero_padding_at_a_rows_end():
    rl = _layer(True, Cin=32, Cout=16)
    x = _x(1, rl.Cin, 20)
    ref, bound = R.up(x, rl, "fused")
    uu = R._phases(R._gemm(R.prelu(x, rl.alpha), rl.rows(), dtype=F32), rl.r)
    rpl = torch.nn.functional.pad(uu, (rl.r, rl.r), mode="replicate")
    y = torch.nn.functional.conv1d(rpl.reshape(-1, 1, rpl.shape[-1]), rl.f.reshape(1, 1, -1)).reshape(uu.shape) + rl.b[None, :, None]
    rep = Report("replicate", y, ref, bound)
    _flagged(rep, 0, uu.shape[-1] - 1, "edge replication")
    assert not bool(rep.bad[..., rl.r: -rl.r].any())


def test_bias_added_before_the_filter():
    rl = _layer(True, Cin=32, Cout=16)
    x = _x(1, rl.Cin, 20)
    ref, bound = R.up(x, rl, "fused")
    y, _ = R.up(x, rl, "fused", dtype=F32, bias_first=True)
    rep = Report("bias first", y, ref, bound)
    _flagged(rep, 0, 40, "bias before the filter")


def test_phase_rows_permuted():
    """co r + ph taken as ph Cout + co."""
    rl = _layer(True, Cin=32, Cout=16, aa=False)
    x = _x(1, rl.Cin, 9)
    ref, bound = R.up(x, rl, "conv")

    def hook(stage, t):
        if stage != "gemm":
            return t
        B, M, Q = t.shape
        return t.reshape(B, M // rl.r, rl.r, Q).permute(0, 2, 1, 3).reshape(B, M, Q)
    y, _ = R.up(x, rl, "conv", dtype=F32, hook=hook)
    rep = Report("phases", y, ref, bound)
    _flagged(rep, 0, 1, "phase rows permuted")


def test_last_output_frame_of_a_strided_conv_dropped():
    rl = _layer(False, aa=False)
    x = _x(2, rl.Cin, 4 * 33)
    ref, bound = R.down(x, rl, "conv")
    y, _ = R.down(x, rl, "conv", dtype=F32)
    y[..., -1] = 0
    _flagged(Report("last frame", y, ref, bound), 1, 32, "last frame dropped")


@pytest.mark.parametrize("up", [False, True])
def test_folded_weight_built_with_the_fir_reversed(up):
    rl = _layer(up, Cin=32 if up else 16, Cout=16 if up else 32)
    x = _x(1, rl.Cin, 12 if up else 48)
    fn = R.up if up else R.down
    ref, bound = fn(x, rl, "folded")
    good, _ = fn(x, rl, "folded", dtype=F32)
    assert Report("folded", good, ref, bound).ok()
    y, _ = fn(x, rl, "folded", dtype=F32, W=rl.folded64(reverse_fir=True).float())
    _flagged(Report("reversed", y, ref, bound), 0, 5, "folded with the FIR reversed")
    # ... and the blob identity sees it at the first weight
    assert R.first_wrong(rl.folded64(reverse_fir=True).float(), rl.folded64().float()) is not None


def test_one_nonzero_sample_behind_a_ragged_rows_end():
    rl = _layer(False, aa=False)
    lens_in, lens = [4 * 13, 4 * 4], [13, 4]
    x = _x(2, rl.Cin, 4 * 13) * R.valid_mask(lens_in, 2, 4 * 13)
    ref, bound = R.down(x, rl, "conv", lens)
    y, _ = R.down(x, rl, "conv", dtype=F32)
    y = y * R.valid_mask(lens, 2, 13)
    assert Report("ragged", y, ref, bound, lens).ok()
    y[1, 7, 4] = 1e-30
    rep = Report("ragged", y, ref, bound, lens)
    assert not rep.ok() and rep.tail_bad == 1 and bool(rep.bad[1, 7, 4])


def test_mel_conv_on_a_minimal_filtering_family_within_bound():
    import conv_fp64 as C

    g = torch.Generator().manual_seed(6)
    w64 = (torch.randn(24, 80, 3, generator=g) / 15).float().double()
    u = sum(C.G[3][:, k] * w64[..., k:k + 1] for k in range(3))
    ol = types.SimpleNamespace(w=w64.float(), b=torch.randn(24, generator=g).float(), KW=3, U=u.float())
    x, sc = _x(2, 80, 13), torch.tensor([0.5, 3.0])
    ref, bound = R.conv_1x1(x, ol, sc, wino=True)
    y = C.wino_fp32(x * sc.reshape(-1, 1, 1), ol) + ol.b[None, :, None]
    rep = Report("mel wino", y, ref, bound)
    print(f"mel conv, minimal filtering: err / bound {rep.ratio:.3f}")
    assert rep.ok() and 0 < rep.ratio < 1
    bad = C.wino_fp32(x * sc[[0, 0]].reshape(-1, 1, 1), ol) + ol.b[None, :, None]
    assert not Report("mel wino", bad, ref, bound).ok()


def test_in_scale_of_row_0_applied_to_row_1():
    g = torch.Generator().manual_seed(5)
    ol = types.SimpleNamespace(w=(torch.randn(24, 80, 3, generator=g) / 15).float(), b=torch.randn(24, generator=g).float())
    x = _x(2, 80, 9)
    sc = torch.tensor([0.5, 3.0])
    ref, bound = R.conv_1x1(x, ol, sc)
    y, _ = R.conv_1x1(x, ol, sc[[0, 0]], dtype=F32)
    rep = Report("in_scale", y, ref, bound)
    assert not rep.ok() and not bool(rep.bad[0].any()) and bool(rep.bad[1].all(0).any())


# ---- the pairing ----------------------------------------------------------------------------------------------------------
def test_pairing_with_colliding_flops():
    """A walk of two body blocks around a down conv, a recurrence and an up conv whose FLOPs collide (64 both)."""
    slots = [("score", "body", "e0"), ("score", "rate", "e0"), ("score", "gruproj", "g"), ("score", "rec", "g"),
             ("score", "rate", "d1"), ("score", "body", "d1")]
    body = [100.0, 60.0, 60.0]
    fo = {("body", "e0"): body, ("body", "d1"): body, ("rate", "e0"): 64.0, ("rate", "d1"): 64.0}
    recs = [(0, 100.0, 0, 485), (0, 120.0, 0, 192), (0, 64.0, 0, 42), (0, 7.0, 0, 322), (0, 9.0, 0, 1003), (0, 64.0, 0, 47),
            (0, 220.0, 0, 193)]
    assert R.pair_walk(slots, recs, fo) == {(0, "e0"): 42, (0, "d1"): 47}
    two = R.pair_walk(slots, recs + recs, fo, score_passes=2)
    assert two[(1, "d1")] == 47 and len(two) == 4
    # a record too many, one too few, a recurrence out of place, wrong FLOPs, a code of no family: all fail
    for broken in (recs + [(0, 64.0, 0, 42)], recs[:-1], recs[:3] + [recs[4], recs[3]] + recs[5:],
                   recs[:2] + [(0, 65.0, 0, 42)] + recs[3:], recs[:2] + [(0, 64.0, 0, 850)] + recs[3:]):
        with pytest.raises(AssertionError):
            R.pair_walk(slots, broken, fo)


def test_variant_codes_do_not_collide():
    assert R.family_of(42) == "rate_down" and R.family_of(47) == "rate_up" and all(R.family_of(i) == "lds" for i in range(8))
    assert R.kind_of(42, 1, False) == "down_fir" and R.kind_of(42, 0, False) == "chain"
    assert R.kind_of(47, 2, True) == "up_fir" and R.kind_of(47, 0, False) == "chain"
    assert R.kind_of(72, 2, True) == "up_fir" and R.kind_of(322, 2, False) == "chain" and R.kind_of(5, 3, False) == "folded"
    with pytest.raises(AssertionError):
        R.family_of(850)
