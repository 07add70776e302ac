"""CPU: the checks of tests/conv_fp64.py check.  fp32 emulations of each arithmetic pass their bound (worst err / bound printed);
every planted defect -- one at a time -- is flagged at the element where it was planted, while the coarse check the suite had
(>= 100 dB SNR over the tensor) stays blind wherever it is; and the case list of tests/test_gpu_conv_fp64.py meets every edge
class its shapes can reach."""
import json

import pytest
import torch

import conv_fp64 as C
import small_fp64 as F
from helpers import get_spec
from open_universe_amd import _lib, state_dict as S

_cache = {}


def _model(name):
    if name not in _cache:
        spec = get_spec(name)
        sd = S.synthetic_state_dict(spec, seed=0)
        _cache[name] = (spec, sd, C.ConvParams(spec, sd))
    return _cache[name]


def _randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("name", C.MODELS)
def test_rebuilt_conv_parameters_are_the_blob(name, built_lib):
    spec, sd, P = _model(name)
    blob, plan = _lib.pack_weights(spec, sd)
    P.check_against_blob(blob, json.loads(plan))


def test_one_transformed_weight_off_by_an_ulp_is_flagged_at_its_blob_offset(built_lib):
    """F(2, 5): one U value moved by one ulp of the UNTRANSFORMED weight's scale.  The element-wise bound cannot see it (module
    docstring): the blob identity names the offset."""
    spec, sd, P = _model("PP16")
    blob, plan = _lib.pack_weights(spec, sd)
    convs = {c["name"]: c for c in json.loads(plan)["convs"]}
    cv = P.blocks["score.enc1"].c[0]
    L = convs[cv.name]
    assert cv.KW == 5 and C.first_wrong_u(blob, L, cv) is None
    ci, m, x = 7, 33, 3
    off = L["wu_off"] + (ci * L["Mp"] + m) * L["KWP"] + x
    bad = blob.clone()
    bad[off] += float(F.ulp32(cv.w[m, ci].abs().max().double().reshape(1))[0])
    assert bad[off] != blob[off] and C.first_wrong_u(bad, L, cv) == off
    # ... and the coarse check is blind to it
    a = _randn(1, 64, 130, seed=3)
    U2 = cv.U.clone()
    U2[m, ci, x] = bad[off]
    assert C.snr_db(C.wino_fp32(a, cv), C.wino_fp32(a, cv, U2)) >= 100


# ---- fp32 emulations pass ------------------------------------------------------------------------------------------------------
def _layer(block="score.enc1", i=0):
    spec, sd, P = _model("PP16")
    return P.blocks[block].c[i]


def _fma_conv32(a, cv, slices=1, hook=None):
    """fp32 conv summed in `slices` K slices (channel groups), each by torch's fp32 conv, the partial sums added in fp32."""
    t = F._taps(a.float(), cv.KW)                       # (B, Cin, T, KW)
    if hook is not None:
        t = hook(t)
    Cin = a.shape[1]
    acc = None
    for s in range(slices):
        sl = slice(s * Cin // slices, (s + 1) * Cin // slices)
        part = torch.einsum("bctk,ock->bot", t[:, sl], cv.w[:, sl])
        acc = part if acc is None else acc + part
    return acc


def _epi32(v, cv, ep):
    return C._epilogue(v + cv.b[None, :, None], None, ep, torch.float32)[0]


SHAPES = [(1, 1), (2, 5), (3, 65), (2, 131)]


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("i", [0, 1])
def test_fp32_emulations_pass(B, T, i):
    cv = _layer(i=i)
    Cc = cv.w.shape[0]
    x = _randn(B, Cc, T, seed=T)
    ep = C.Epi(add=_randn(B, Cc, T, seed=1), film=(_randn(B, Cc, 1, seed=2) + 1, _randn(B, Cc, 1, seed=3)), res=_randn(B, Cc, T, seed=4),
               out_alpha=torch.tensor(0.2))
    a32 = C.prelu(x, cv.alpha)
    for slices in (1, 4, 8):
        ref, bound, _ = C.body_conv(x, cv, ep, "chain")
        rep = C.Report(f"chain/{slices}", _epi32(_fma_conv32(a32, cv, slices), cv, ep), ref, bound)
        print(rep)
        assert rep.ok() and rep.excluded == 0 and rep.checked == ref.numel(), rep
    ref, bound, _ = C.body_conv(x, cv, ep, "wino")
    rep = C.Report("wino", _epi32(C.wino_fp32(a32, cv), cv, ep), ref, bound)
    print(rep)
    assert rep.ok() and rep.excluded == 0, rep
    # bf16 split: the bound's own yardstick is split_fp32, so what is shown to pass is something else -- the same six piece
    # products summed by torch's blocked fp32 conv, and the kernel's order with the six products of a (chunk, tap) met first
    ref, bound, ex = C.body_conv(x, cv, ep, "split")
    ap, wp = C.bf16_pieces(a32), C.bf16_pieces(cv.w)
    blocked = sum(C._conv(ap[i_], wp[j_], torch.float32) for i_, j_ in C.SPLIT_KEPT)
    for nm, v in (("blocked", blocked), ("reversed products", C.split_fp32(a32, cv, kept=C.SPLIT_KEPT[::-1]))):
        rep = C.split_report(f"split/{nm}", _epi32(v, cv, ep), ref, bound, ex)
        print(rep, rep.lib_ratio)
        assert rep.ok() and rep.excluded == 0 and rep.lib_ratio <= C.M_SPLIT, rep


def test_fused_body_emulation_passes():
    spec, sd, P = _model("PP16")
    bp = P.blocks["score.enc0"]
    x = _randn(2, bp.C, 260, seed=9)
    ep1 = C.Epi(film=(_randn(2, bp.C, 1, seed=2) + 1, _randn(2, bp.C, 1, seed=3)))
    ref, bound, c1r, c1b = C.fused_body(x, bp, 3, ep1, x)
    h = _epi32(C.wino_fp32(C.prelu(x, bp.c[0].alpha), bp.c[0]), bp.c[0], ep1)
    assert C.Report("c1", h, c1r, c1b).ok()
    h = _epi32(C.wino_fp32(C.prelu(h, bp.c[1].alpha), bp.c[1]), bp.c[1], C.Epi())
    h = _epi32(C.wino_fp32(C.prelu(h, bp.c[2].alpha), bp.c[2]), bp.c[2], C.Epi(res=x))
    rep = C.Report("fused3", h, ref, bound)
    print(rep)
    assert rep.ok() and rep.excluded == 0, rep
    # a stage's halo column not recomputed (taken as 0) at a tile seam of the fused kernel: flagged there
    h1 = _epi32(C.wino_fp32(C.prelu(x, bp.c[0].alpha), bp.c[0]), bp.c[0], ep1)
    h1[:, :, 252] = 0
    h2 = _epi32(C.wino_fp32(C.prelu(h1, bp.c[1].alpha), bp.c[1]), bp.c[1], C.Epi())
    h3 = _epi32(C.wino_fp32(C.prelu(h2, bp.c[2].alpha), bp.c[2]), bp.c[2], C.Epi(res=x))
    rep = C.Report("fused3", h3, ref, bound)
    assert not rep.ok() and 250 <= rep.worst["index"][2] <= 254, rep


# ---- planted defects fail, the coarse check is blind ---------------------------------------------------------------------------
def _case():
    """conv3 of a 64-channel block on rows of odd length 131: partial row tile is modelled by the rows >= 48 (PP24's 48 channels
    of a 64-row tile), the residual of the size of the network's (hu ~ 1, conv products small against it)."""
    cv = _layer(i=2)
    Cc = cv.w.shape[0]
    x = _randn(3, Cc, 131, seed=11, scale=0.3)
    hu = _randn(3, Cc, 131, seed=12)
    return cv, x, hu


def _flagged(name, got, ref, bound, where=None, lens=None, blind=True):
    rep = C.Report(name, got, ref, bound, lens)
    assert not rep.ok() and rep.excluded == 0, rep
    if where is not None:
        assert where(rep.worst["index"]), rep
    if blind is not None:
        db = C.snr_db(ref, got)
        print(f"{name}: flagged {rep.n_bad}, worst {rep.worst['index']}, coarse check {db:.1f} dB")
        assert (db >= 100) == blind, (name, db)
    return rep


def _emul(kind, a, cv, hook=None):
    """fp32 emulation of the conv proper for a bound kind; `hook` = (damage of the (B, Cin, T, KW) tap windows, damage of the
    (B, Cin, P, KW + 1) pair windows) -- the same defect in the two layouts."""
    if kind == "chain":
        return _fma_conv32(a, cv, hook=hook and hook[0])
    return C.wino_fp32(a, cv, hook=hook and hook[1])


@pytest.mark.parametrize("kind", ["chain", "wino"])
def test_planted_defects_in_the_window_are_flagged_where_they_were_planted(kind):
    """k3, pad 1: tap window t holds a[t - 1 .. t + 1], pair window p holds a[2 p - 1 .. 2 p + 2]."""
    cv, x, hu = _case()
    ep = C.Epi(res=hu)
    ref, bound, _ = C.body_conv(x, cv, ep, kind)
    a = C.prelu(x, cv.alpha)
    assert C.Report("good", _epi32(_emul(kind, a, cv), cv, ep), ref, bound).ok()
    prev = a[0, 5, -1]

    def halo_t(t):    # the sample in front of row 1 taken from the end of row 0 instead of 0 (one channel)
        t = t.clone()
        t[1, 5, 0, 0] = prev
        return t

    def halo_p(d):
        d[1, 5, 0, 0] = prev
        return d

    def last_t(t):    # the last tap of column 129 dropped, one channel: the last whole column pair of the odd-length row
        t = t.clone()
        t[:, 9, 129, 2] = 0
        return t

    def last_p(d):
        d[:, 9, 64, 3] = 0
        return d
    # coarse check on these 25 152 elements: printed, not asserted (the same few wrong elements among the 10^7 of a workload-sized
    # tensor stand 26 dB higher)
    _flagged("halo", _epi32(_emul(kind, a, cv, (halo_t, halo_p)), cv, ep), ref, bound, lambda i: i[0] == 1 and i[2] == 0, blind=None)
    _flagged("last tap", _epi32(_emul(kind, a, cv, (last_t, last_p)), cv, ep), ref, bound, lambda i: i[2] == 129, blind=None)
    # taps in reversed order: y_rev = flip(conv(flip(a)))
    _flagged("reversed taps", _epi32(_emul(kind, a.flip(-1), cv).flip(-1), cv, ep), ref, bound, blind=False)
    # bias omitted on the rows of a partial row tile (rows 48 .. 63 of a 64-row tile)
    v = _emul(kind, a, cv)
    b2 = cv.b.clone()
    b2[48:] = 0
    got = C._epilogue(v + b2[None, :, None], None, ep, torch.float32)[0]
    _flagged("bias", got, ref, bound, lambda i: i[1] >= 48, blind=None)
    # one non-zero element behind a row's end
    lens = [131, 70, 3]
    m = C.valid_mask(lens, 3, 131)
    refm, boundm, _ = C.body_conv(x * m, cv, C.Epi(res=hu * m), kind, lens)
    goodm = _epi32(_emul(kind, C.prelu(x * m, cv.alpha), cv), cv, C.Epi(res=hu * m)) * m
    assert C.Report("ragged", goodm, refm, boundm, lens).ok()
    bad = goodm.clone()
    bad[1, 3, 70] = 1e-6
    rep = _flagged("tail", bad, refm, boundm, lambda i: i == [1, 3, 70], lens)
    assert rep.tail_bad == 1


@pytest.mark.parametrize("kind", ["chain", "wino"])
def test_planted_defects_in_the_prologue_and_epilogue_are_flagged(kind):
    cv, x, hu = _case()
    Cc = cv.w.shape[0]
    c1 = _randn(3, Cc, 131, seed=13)
    ep = C.Epi(res=hu)
    ref, bound, _ = C.body_conv(x, cv, ep, kind)
    a = C.prelu(x, cv.alpha)
    v = _emul(kind, a, cv) + cv.b[None, :, None]
    # PReLU slope applied to positive values
    _flagged("slope", _epi32(_emul(kind, x * cv.alpha, cv), cv, ep), ref, bound, blind=False)
    # activation applied twice
    _flagged("twice", _epi32(_emul(kind, C.prelu(a, cv.alpha), cv), cv, ep), ref, bound, blind=False)
    # residual scale 0.7071 instead of the fp32 1 / sqrt2
    rep = _flagged("0.7071", (v + hu) * torch.tensor(0.7071), ref, bound, blind=True)
    print(kind, "0.7071: flagged", rep.n_bad, "of", rep.checked, "worst ratio", rep.ratio)
    # residual taken from c1 instead of hu
    _flagged("res from c1", (v + c1) * torch.tensor(C.INV_SQRT2), ref, bound, blind=False)
    # conv1: FiLM shift and scale swapped; condition add without its 1 / sqrt2
    cv1 = _layer(i=0)
    add, ga, be = _randn(3, Cc, 131, seed=14), _randn(3, Cc, 1, seed=15) + 1, _randn(3, Cc, 1, seed=16)
    ep1 = C.Epi(add=add, film=(ga, be))
    ref1, bound1, _ = C.body_conv(x, cv1, ep1, kind)
    v1 = _emul(kind, C.prelu(x, cv1.alpha), cv1) + cv1.b[None, :, None]
    s2 = torch.tensor(C.INV_SQRT2)
    assert C.Report("good", ga * ((v1 + add) * s2) + be, ref1, bound1).ok()
    _flagged("film swapped", be * ((v1 + add) * s2) + ga, ref1, bound1, blind=False)
    _flagged("add unscaled", ga * (v1 + add) + be, ref1, bound1, blind=False)


def test_the_residual_scale_defect_passes_the_coarse_check_at_its_tolerance():
    """0.7071 for 1 / sqrt2 is a relative 9.6e-6: 100.4 dB on the residual alone -- the >= 100 dB checks of the parity tests pass it
    wherever the conv's own part is not larger than the residual; the element-wise bound does not."""
    cv, x, hu = _case()
    good = hu * torch.tensor(C.INV_SQRT2)
    assert C.snr_db(good, hu * torch.tensor(0.7071)) >= 100


def test_the_smallest_bf16_piece_dropped_is_flagged_and_the_coarse_check_is_blind():
    """On a 32-channel k3 conv (n = 96): the defect stands 64 / sqrt(6 n / 16) ~ 10 times above e32, M_SPLIT = 7 flags it.  This
    shows the check working, NOT the kernel held: conv_split_kernel takes layers of 64 rows and more (n >= 192), where the
    defect stands at or below M e32 -- on the layers the kernel runs, a dropped smallest piece is not caught by this bound."""
    spec, sd, P = _model("PP16")
    cv = P.blocks["score.enc0"].c[2]
    x = _randn(2, cv.w.shape[0], 131, seed=21)
    ep = C.Epi()
    ref, bound, ex = C.body_conv(x, cv, ep, "split")
    a = C.prelu(x, cv.alpha)
    good = _epi32(C.split_fp32(a, cv), cv, ep)
    assert C.split_report("split", good, ref, bound, ex).ok()
    bad = _epi32(C.split_fp32(a, cv, x_pieces=2), cv, ep)
    rep = C.split_report("split", bad, ref, bound, ex)
    db = C.snr_db(ref, bad)
    print(rep, rep.lib_ratio, db)
    assert not rep.ok() and rep.lib_ratio > C.M_SPLIT and db >= 100


# ---- coverage --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.MODELS)
def test_the_gpu_cases_meet_every_reachable_edge_class(name, built_lib):
    spec, sd, P = _model(name)
    plan = json.loads(_lib.pack_weights(spec, sd)[1])
    ms = sorted({m for m, _ in F.levels(plan, "condition_model")} | {m for m, _ in F.levels(plan, spec.score_prefix)} | {1})
    assert ms == ([1, 5, 20, 80, 160] if name == "PP16" else [1, 8, 40, 120, 240])
    # per family: the tiles of ITS launcher over the shapes ITS cases run, against what whole batches of the batch sizes it
    # works at reach within MAX_FRAMES frames (from the fewest frames at which it takes a layer)
    for tag, (opts, fams, batches, fmin) in C.FAMILIES.items():
        shapes = {(f, B) for t_, mm, B, f in C.CASES if mm == name and t_ == tag}
        if "preact" in opts or not shapes:
            continue  # (the preact = 0 variants repeat one shape of their family)
        for fam in fams:
            for tile in C.FAMILY_TILES[fam]:
                for m in ms:
                    if fam == "fused" and m != {126: 80, 252: 160}[tile]:
                        continue  # (conv_chainw_kernel: 64 channels / 126 columns, 32 channels / 252 columns)
                    hit = set()
                    for f, B in shapes:
                        hit |= C.edge_classes(f * m, tile, 2, B)
                    missing = C.reachable_within(m, tile, 2, range(fmin, C.MAX_FRAMES + 1), batches) - hit
                    assert not missing, (name, tag, fam, m, tile, sorted(missing))
    # ragged rows: an end inside a tile, on a tile edge and on a pair edge / inside a pair, on some level
    ends = [(f * m, tile) for f in C.RAGGED_ROWS[1:] for m in ms for tile in (64, 128)]
    assert any(n % tile and n > tile for n, tile in ends) and any(n % tile == 0 for n, tile in ends)
    assert any(n % 2 for n, _ in ends) and any(n % 2 == 0 for n, _ in ends)
    # a partial row tile (M no multiple of 64): PP24's 48 / 96 channels
    if name == "PP24":
        assert {48, 96} <= {bp.C for bp in P.blocks.values()}


def test_the_recorded_widths_name_every_family_under_test():
    """tests/golden/conv_fp64_widths.json (what each family took per case on an MI355X; the GPU cases assert it): every case has
    its record, and every family under test took layers of both kernel sizes in at least one case of every model it exists in --
    a family that the case list never brings up cannot hide behind an empty record."""
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_fp64_widths.json")) as f:
        rec = json.load(f)
    for tag, name, B, frames in C.CASES:
        assert C.case_id(tag, name, B, frames) in rec
    for tag, (opts, fams, batches, fmin) in C.FAMILIES.items():
        for name in C.MODELS:
            cases = [C.case_id(t, m, B, f) for t, m, B, f in C.CASES if t == tag and m == name]
            for fam in fams if cases else ():
                took = {tuple(v) for c in cases for v in rec[c].get(fam, [])}
                assert {kw for _, kw in took} == ({0} if fam == "fused" else {3, 5}), (tag, name, fam, sorted(took))
    for name, mf in C.RAGGED:
        assert rec[f"ragged.mask_fused{mf}.{name}"]
    # the fused body exists for 32 / 64 channels: mask_fused = 0 forbids it (Runner::plan_chain), so the two ragged PP16 cases differ
    assert "fused" in rec["ragged.mask_fused1.PP16"] and "fused" not in rec["ragged.mask_fused0.PP16"]
