"""CPU: the off-list topologies of tests/offlist_cases.py.

* the packer accepts every case and the rebuilt parameters of small_fp64 / conv_fp64 / rate_fp64 (and gru_fp64's layers) are the
  packed blob's -- the rebuilders are generic over the spec, nothing is special-cased here;
* coverage: every case's claimed branches follow from its spec, and the union of the claims is offlist_cases.BRANCHES;
* the boundary of the accepted space: ou_packed_bytes refuses each configuration just outside with OU_ENOTIMPL and a message that
  names the field, and accepts the neighbour just inside;
* the checks bite: an fp32 torch restatement of each newly reached stage passes its bound, a handful of mutants each fail."""
import copy
import json
import math

import pytest
import torch

import conv_fp64 as CF
import gru_fp64 as G
import offlist_cases as K
import rate_fp64 as R
import small_fp64 as F
from open_universe_amd import _lib

_cache = {}


def _case(case):
    if case not in _cache:
        spec = K.spec_of(case)
        _cache[case] = (spec, K.state_dict_of(case))
    return _cache[case]


def _randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- the packer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(K.CASES))
def test_packer_accepts_the_case_and_the_rebuilt_parameters_are_the_blob(case, built_lib):
    spec, sd = _case(case)
    assert _lib.packed_bytes(spec) > 0
    blob, plan = _lib.pack_weights(spec, sd)
    assert blob.numel() * 4 == _lib.packed_bytes(spec)
    plan = json.loads(plan)
    assert plan["tot_ds"] == spec.tot_ds
    F.Params(spec, sd).check_against_blob(blob, plan)
    CF.ConvParams(spec, sd).check_against_blob(blob, plan)
    P = R.RateParams(spec, sd)
    P.check_against_blob(blob, plan)
    OC = spec.score.n_channels << len(spec.score.rate_factors)
    for prefix, layer in (("condition_model.encoder.gru", 0), ("condition_model.encoder.gru", 1), (spec.score_prefix + ".encoder.gru", 0)):
        L = G.Layer(sd, prefix, layer)
        assert L.H == OC // 2 and L.H % 64 == 0, (prefix, layer, L.H)
    # what the plan says of the branches the case is there for
    convs = {c["name"]: c for c in plan["convs"]}
    want = set(K.CASES[case][2])
    fir_lens = {c["fir_len"] for c in convs.values() if c["fir_mode"] in (1, 2)}
    for b in want:
        if b.startswith("fir_scalar_"):
            assert int(b[len("fir_scalar_"):]) in fir_lens and int(b[len("fir_scalar_"):]) not in K.FIR4_TAPS
        if b.startswith("rate_") and b[5:].isdigit():
            r = int(b[5:])
            assert any(c["stride"] == r for c in convs.values()) and any(c["up"] == r for c in convs.values())
        if b == "aa_off_pp":
            assert not fir_lens and all(c["fir_mode"] == 0 for c in convs.values())
    if "tot_ds_odd" in want:
        assert plan["tot_ds"] % 4 != 0
    n_st = sum(1 for n in convs if ".st_convs." in n)
    assert n_st == len(spec.cond.rate_factors) - 1 and len(P.slots) > 0


def test_every_branch_has_a_case_and_every_claim_follows_from_the_spec():
    union = set()
    for case, (base, over, claimed) in K.CASES.items():
        spec = K.spec_of(case)
        derived = K.branches_of(spec, K.base_spec_of(case))
        assert set(claimed) == derived, (case, "claimed", sorted(claimed), "the spec gives", sorted(derived))
        assert derived <= set(K.BRANCHES), (case, sorted(derived - set(K.BRANCHES)))
        union |= derived
    assert union == set(K.BRANCHES), ("branches without a case", sorted(set(K.BRANCHES) - union))
    assert 6 <= len(K.CASES) <= 8
    # the case lists of the GPU file name cases of the table
    assert set(K.ODD) | set(K.RAGGED) | set(K.OPTION_CASES) <= set(K.CASES)
    assert all(K.spec_of(c).tot_ds % 4 for c in K.ODD) and all(K.spec_of(c).tot_ds % 4 == 0 for c in set(K.CASES) - set(K.ODD))


def test_the_shipped_topologies_reach_none_of_the_branches():
    from open_universe_amd import config as C

    for name in ("PP16", "PP24", "OR16"):
        spec = C.spec_from_config(C.builtin_config(name))
        assert K.branches_of(spec, spec) == set(), name


# ---- the boundary of the accepted space --------------------------------------------------------------------------------------------
def _with(case, **kw):
    """The spec of `case` with fields replaced: rates=, cond_<field>= (conditioner only), <field>= (both networks)."""
    spec = copy.deepcopy(K.spec_of(case))
    for k, v in kw.items():
        if k == "rates":
            spec.score.rate_factors, spec.cond.rate_factors = list(v), list(v)
        elif k.startswith("cond_"):
            setattr(spec.cond, k[len("cond_"):], v)
        else:
            setattr(spec.score, k, v)
            setattr(spec.cond, k, v)
    return spec


# (case, what is refused, the word the message has to hold, the neighbours just inside)
BOUNDARY = [
    ("r67", dict(rates=[2, 6, 1]), "rate factors", [dict(rates=[2, 6, 2])]),
    ("r67", dict(rates=[2, 6, 9]), "rate factors", [dict(rates=[2, 6, 8])]),
    ("r67", dict(fb_kernel_size=9), "fb_kernel_size", [dict(fb_kernel_size=7)]),
    ("r67", dict(fb_kernel_size=4), "fb_kernel_size", [dict(fb_kernel_size=3), dict(fb_kernel_size=5)]),
    ("one", dict(n_channels=63), "n_channels", [dict(n_channels=64)]),
    ("one", dict(n_channels=66), "n_channels", [dict(n_channels=64)]),
    ("kw7", dict(noise_cond_dim=96), "noise_cond_dim", [dict(noise_cond_dim=64), dict(noise_cond_dim=128)]),
    ("kw7", dict(noise_cond_dim=1088), "noise_cond_dim", [dict(noise_cond_dim=1024)]),
    ("kw7", dict(noise_cond_dim=0), "noise_cond_dim", [dict(noise_cond_dim=64)]),
    ("odd_or", dict(n_rff=0), "n_rff", [dict(n_rff=1)]),
    ("odd_or", dict(n_rff=65), "n_rff", [dict(n_rff=64)]),
    # n_fft = n_mel_oversample * prod(rate_factors): 6 * 343 = 2058 is the first product of admissible factors above 2048
    ("r67", dict(rates=[7, 7, 7], cond_n_mel_oversample=6), "n_fft", [dict(rates=[7, 7, 7], cond_n_mel_oversample=5),
                                                                       dict(rates=[4, 8, 8], cond_n_mel_oversample=8)]),
    ("r67", dict(cond_n_mels=81), "n_mels", [dict(cond_n_mels=80), dict(cond_n_mels=82)]),
    ("r67", dict(cond_n_mels=258), "n_mels", [dict(cond_n_mels=256)]),
    # the GRU's hidden size OC / 2 = 8 * 8 / 2 = 32
    ("r67", dict(n_channels=8), "GRU hidden size", [dict(n_channels=16)]),
    ("r67", dict(cond_n_channels=32), "score/cond", []),
    ("r67", dict(cond_rate_factors=[2, 6]), "score/cond", []),
    ("r67", dict(cond_rate_factors=[2, 7, 6]), "rate factors", []),
    ("r67", dict(cond_fb_kernel_size=5), "fb_kernel_size", []),
    ("r67", dict(cond_extra_conv_block=False), "extra_conv_block", []),
    # found by reading the walk for this table: sum_kernel has five operands (four rate factors), s2d_kernel's tile is 33 R + 1
    # floats of LDS -- both used to pass the packer and fail in the first call
    ("r67", dict(rates=[2, 2, 2, 2, 2], n_channels=4), "n_rates", [dict(rates=[2, 2, 2, 2], n_channels=8)]),
    ("r67", dict(rates=[8, 8, 8]), "prod(rate_factors)", [dict(rates=[8, 8, 7])]),
]


@pytest.mark.parametrize("case,refused,word,inside", BOUNDARY, ids=[f"{c}.{'.'.join(f'{k}={v}' for k, v in r.items())}" for c, r, w, i in BOUNDARY])
def test_boundary_of_the_accepted_space(case, refused, word, inside, built_lib):
    with pytest.raises(NotImplementedError) as e:  # OU_ENOTIMPL
        _lib.packed_bytes(_with(case, **refused))
    assert word in str(e.value), (refused, str(e.value))
    for kw in inside:
        assert _lib.packed_bytes(_with(case, **kw)) > 0, kw


# ---- the checks bite -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [13, 15])
def test_scalar_fir_restatement_passes_and_a_dropped_last_tap_fails(nt):
    """fir_kernel at the tap counts of rate factors 6 and 7, both forms, on rows of odd length."""
    B, C, T = 2, 3, 1029
    x, res = _randn(B, C, T, seed=30), _randn(B, C, T, seed=31)
    taps = torch.tensor([math.comb(nt - 1, k) for k in range(nt)], dtype=torch.float64).div(2.0 ** (nt - 1)).float()
    bias = _randn(C, seed=32)
    for kw in (dict(alpha=0.2), dict(bias=bias, res=res, res_scale=F.INV_SQRT2)):
        ref, bound = F.fir(x, taps, **kw)
        good, _ = F.fir(x, taps, dtype=torch.float32, **kw)
        rep = F.Report("fir", good, ref, bound)
        assert rep.ok() and rep.excluded == 0 and rep.checked == ref.numel(), rep

        def drop_last(w):  # a loop over ntaps - 1 taps (the binomial end tap is 2^-(nt - 1): the smallest defect a tap can be)
            w = w.clone()
            w[..., nt - 1] = 0
            return w
        bad, _ = F.fir(x, taps, dtype=torch.float32, hook=drop_last, **kw)
        assert not F.Report("fir", bad, ref, bound).ok(), (nt, sorted(kw))


@pytest.mark.parametrize("case", ["odd_pp", "kw7"])
def test_wide_in_conv_restatement_passes_and_a_shifted_window_fails(case):
    spec, sd = _case(case)
    P = F.Params(spec, sd)
    KW = P.s_in_w.shape[1]
    assert KW == spec.score.fb_kernel_size and KW in (5, 7)
    x = _randn(3, 1, 13 * 21, seed=33)
    w_in = torch.tensor([0.7, 1.3, 0.05])
    ref, bound = F.in_conv(x, P.s_in_w, P.s_in_b, w_in)
    rep = F.Report("in_conv", F.in_conv_fp32(x, P.s_in_w, P.s_in_b, w_in), ref, bound)
    assert rep.ok() and rep.excluded == 0, rep
    # pad computed for KW = 3: the window one sample late ... and two late
    for shift in (1, 2):
        hook = lambda t: torch.roll(t, -shift, dims=2)
        assert not F.Report("in_conv", F.in_conv_fp32(x, P.s_in_w, P.s_in_b, w_in, hook=hook), ref, bound).ok(), shift


@pytest.mark.parametrize("case", ["odd_pp", "odd_or", "one", "kw7"])
def test_out_conv_restatement_passes_and_an_unwritten_last_quad_fails(case):
    """KW 1 / 3 / 5 / 7, the EDM form and the plain one; T % 4 != 0 for the two odd cases (the kernel's scalar path)."""
    spec, sd = _case(case)
    P = F.Params(spec, sd)
    B, T = 2, 13 * spec.tot_ds if spec.tot_ds % 4 else 13 * spec.tot_ds + 3
    assert T % 4 != 0
    s, x = _randn(B, P.out_w.shape[0], T, seed=34), _randn(B, 1, T, seed=35, scale=0.5)
    coef = F.edm_coef(spec, [0.3, 1.7])
    ref, bound = F.out_conv_score(s, x, P, coef)
    good = F.out_conv_fp32(s, x, P, coef)
    rep = F.Report("out_conv", good, ref, bound)
    assert rep.ok() and rep.excluded == 0, rep
    bad = good.clone()
    bad[..., T - T % 4:] = 0.0  # the last T % 4 samples left as the buffer was
    rep = F.Report("out_conv", bad, ref, bound)
    assert not rep.ok() and rep.worst["index"][2] >= T - T % 4, rep


@pytest.mark.parametrize("case", ["kw7", "d1024"])
def test_film_restatement_passes_and_a_row_offset_with_d_512_fails(case):
    spec, sd = _case(case)
    P = F.Params(spec, sd)
    D = spec.score.noise_cond_dim
    assert D // 64 != 8 and P.film_w.shape[1] == D
    g = F.sigma_embed(torch.tensor([0.3, 1.7, 0.05]), P, torch.float32)
    assert g.shape == (3, D)
    ref, bound = F.film(g, P.film_w, P.film_b)
    rep = F.Report("film", F.film_fp32(g, P.film_w, P.film_b), ref, bound)
    assert rep.ok() and rep.excluded == 0, rep
    rows = P.film_w.shape[0]
    flat = torch.cat([P.film_w.reshape(-1), torch.zeros(rows * 512 + D)])
    W512 = torch.stack([flat[r * 512: r * 512 + D] for r in range(rows)])   # row r read at r * 512
    rep = F.Report("film", F.film_fp32(g, W512, P.film_b), ref, bound)
    assert not rep.ok() and rep.worst["index"][-1] >= 1, rep  # (row 0 starts at 0 either way)
    # and the embedding at this D: halves exchanged fails the `library` check
    sig = torch.tensor([0.3, 1.7, 0.05])
    assert F.check_sigma_embed(F.sigma_embed(sig, P, torch.float32), sig, P).ok()
    assert not F.check_sigma_embed(F.sigma_embed(sig, P, torch.float32, swap_halves=True), sig, P).ok()


def test_rff_embedding_at_another_n_rff_passes_and_swapped_halves_fail():
    spec, sd = _case("odd_or")
    P = F.Params(spec, sd)
    assert not P.simple and P.n_rff == 16 and P.mlp[0][1].shape == (64, 32)
    sig = torch.tensor([0.3, 1.7, 0.05])
    assert F.check_sigma_embed(F.sigma_embed(sig, P, torch.float32), sig, P).ok()
    assert not F.check_sigma_embed(F.sigma_embed(sig, P, torch.float32, swap_halves=True), sig, P).ok()


def test_fused_up_fir_restatement_passes_and_the_arithmetic_of_up_8_on_up_6_fails():
    """rate_fp64's up_fir bound on the rate-6 up conv of case r67: the fp32 restatement passes; fir_up<8>'s index arithmetic
    (sample t of a channel = phase row t % 8 of frame t / 8, channel rows 8 apart) applied to up = 6 fails."""
    spec, sd = _case("r67")
    P = R.RateParams(spec, sd)
    key = next(k for k, rl in P.rate.items() if rl.up and rl.r == 6 and k.startswith("score."))
    rl = P.rate[key]
    B, Q = 2, 14
    x, res = _randn(B, rl.Cin, Q, seed=36), _randn(B, rl.Cout, Q * 6, seed=37)
    ref, bound = R.up(x, rl, "fused", res)
    good, _ = R.up(x, rl, "fused", res, dtype=torch.float32)
    rep = R.Report(key, good, ref, bound)
    assert rep.ok() and rep.excluded == 0, rep
    seen = {}

    def as_up8(stage, t):
        if stage == "gemm":
            seen["rows"] = t
            return t
        rows, M = seen["rows"], seen["rows"].shape[1]
        tt = torch.arange(t.shape[-1])
        co = torch.arange(t.shape[1])
        m = (co[:, None] * 8 + (tt % 8)[None, :]) % M                  # (Cout, T): the row fir_up<8> would read
        q = (tt // 8)[None, :].expand_as(m)
        return rows[:, m, q]
    bad, _ = R.up(x, rl, "fused", res, dtype=torch.float32, hook=as_up8)
    assert not R.Report(key, bad, ref, bound).ok()
    # the unfused pair the library runs instead: phase GEMMs alone, then the scalar FIR pass
    ref, bound = R.up(x, rl, "upc")
    good, _ = R.up(x, rl, "upc", dtype=torch.float32)
    assert R.Report(key + ".upc", good, ref, bound).ok()


@pytest.mark.parametrize("n", [2, 3, 4])
def test_sum_with_fewer_operands_holds_a_one_ulp_defect(n):
    parts = [_randn(2, 8, 13, seed=40 + i) for i in range(n)]
    scale = F.sum_scale_of(n)
    ref, bound = F.sum_scaled(parts, scale)
    assert F.Report("sum", ref.clone(), ref, bound).ok()
    bad = ref.clone()
    bad[1, 3, 5] = torch.nextafter(bad[1, 3, 5], torch.tensor(float("inf")))
    assert not F.Report("sum", bad, ref, bound).ok()
    wrong, _ = F.sum_scaled(parts, F.sum_scale_of(5))  # the shipped topologies' 1 / sqrt(5)
    assert not F.Report("sum", wrong, ref, bound).ok()
