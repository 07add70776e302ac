"""Level normalisation modes (normalization_norm max | 2-max, normalization_kwargs.zero_mean / eps) on the CPU: the config reader,
the loader's arguments of ou_set_normalization, the unchanged ou_config, and the float64 restatement of utils/norm.py that the
GPU tests hold the kernels against (tests/norm_cases.py) against what the REAL reference recorded in the goldens."""
import ctypes
import math

import pytest
import torch
import yaml

import norm_cases as K
from helpers import get_spec
from open_universe_amd import _lib
from open_universe_amd import config as C


# ---- config ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given,want", [(2, "2"), ("2", "2"), (2.0, "2"), ("max", "max"), ("2-max", "2-max")])
def test_normalization_norm_is_read(given, want):
    spec = C.spec_from_config(C.builtin_config("PP16", normalization_norm=given))
    assert spec.norm == want and spec.zero_mean is True and spec.norm_eps == 1e-5


def test_default_spec_is_norm_2_zero_mean():
    cfg = C.builtin_config("OR16")
    del cfg["model"]["normalization_norm"]  # the reference's constructor argument has no default, its yaml files all say 2
    spec = C.spec_from_config(cfg)
    assert (spec.norm, spec.zero_mean, spec.norm_eps) == ("2", True, 1e-5)
    assert _lib.norm_args(spec) == (0, 1, 0.0)


def test_zero_mean_and_eps_are_read_through_yaml(tmp_path):
    cfg = C.builtin_config("PP16", **{"normalization_norm": "2-max", "normalization_kwargs.zero_mean": False,
                                      "normalization_kwargs.eps": 1e-3})
    p = tmp_path / "config.yaml"
    p.write_text(yaml.safe_dump(cfg).replace("eps: 0.001", "eps: 1e-3"))  # (PyYAML reads 1e-3 as a string: coerced)
    spec = C.spec_from_config(C.load_config(p))
    assert (spec.norm, spec.zero_mean, spec.norm_eps) == ("2-max", False, 1e-3)
    assert _lib.norm_args(spec) == (_lib.OU_NORM_2MAX, 0, 1e-3)
    assert spec.to_dict()["norm"] == "2-max"
    # builtin_config's overrides reach both keys and leave the other models' dicts alone
    assert C.spec_from_config(C.builtin_config("PP16")).zero_mean is True


@pytest.mark.parametrize("bad", ["1", 1, "inf", "max-2", 3.0, True])
def test_unknown_norm_is_refused_with_the_references_message(bad):
    with pytest.raises(NotImplementedError, match=r"Norm .* is not implemented for batch normalization"):
        C.spec_from_config(C.builtin_config("PP16", normalization_norm=bad))


def test_unknown_norm_in_a_hand_made_spec_is_refused_by_the_loader():
    spec = get_spec("PP16s")
    spec.norm = "1"
    with pytest.raises(NotImplementedError, match="Norm 1 is not implemented"):
        _lib.make_config(spec)
    spec.norm, spec.norm_eps = "max", 0.0
    with pytest.raises(ValueError, match="eps"):
        _lib.norm_args(spec)
    with pytest.raises(ValueError, match="eps"):
        C.spec_from_config(C.builtin_config("PP16", **{"normalization_kwargs.eps": -1.0}))


@pytest.mark.parametrize("mode", list(K.MODES))
def test_cases_parse_to_the_mode_they_name(mode):
    spec = K.spec_of("PP16s", mode)
    want = {"max": (_lib.OU_NORM_MAX, 1, 0.0), "2max": (_lib.OU_NORM_2MAX, 1, 0.0), "keepmean": (_lib.OU_NORM_2, 0, 0.0),
            "max_keepmean": (_lib.OU_NORM_MAX, 0, 0.0), "2max_keepmean": (_lib.OU_NORM_2MAX, 0, 0.0),
            "2max_eps": (_lib.OU_NORM_2MAX, 1, 1e-3)}[mode]
    assert _lib.norm_args(spec) == want


# ---- the C boundary ------------------------------------------------------------------------------------------------------------
def test_ou_config_is_what_it_was_and_the_setter_is_exported(built_lib):
    """The mode travels by ou_set_normalization, not in ou_config: the struct keeps the size version 7 callers compiled against
    (it ends with the four *_act fields), the ABI number stays 7, and a spec with another mode gives the same bytes."""
    assert _lib.OU_ABI_VERSION == 7 and _lib.make_config(get_spec("PP16s")).abi_version == 7
    assert ctypes.sizeof(_lib.Config) == _lib.Config.cond_dec_act.offset + 4 == 240
    assert (_lib.OU_NORM_2, _lib.OU_NORM_MAX, _lib.OU_NORM_2MAX) == (0, 1, 2)
    plain = bytes(_lib.make_config(get_spec("PP16s")))
    for mode in K.MODES:
        assert bytes(_lib.make_config(K.spec_of("PP16s", mode))) == plain
    assert "ou_set_normalization" in _lib.EXPORTED_SYMBOLS and hasattr(built_lib, "ou_set_normalization")
    assert built_lib.ou_set_normalization(None, 0, 1, 0.0) == _lib.OU_EINVAL  # no handle: refused before anything is touched


def test_packed_blob_does_not_depend_on_the_mode(built_lib):
    from open_universe_amd import state_dict as S

    spec = get_spec("PP16s")
    sd = S.synthetic_state_dict(spec, seed=0)
    blob0, plan0 = _lib.pack_weights(spec, sd)
    for mode in ("max", "keepmean"):
        blob, plan = _lib.pack_weights(K.spec_of("PP16s", mode), sd)
        assert torch.equal(blob, blob0) and plan == plan0


# ---- the restatement against the reference's recorded statistics -----------------------------------------------------------------
def _norm_of(mode):
    return K.MODE_ARGS[mode][:2]


@pytest.mark.parametrize("model,mode", K.CASES)
def test_restatement_equals_the_references_recorded_mean_and_std(model, mode):
    """norm_stats (float64) against (mean, std = 1 / gain) of the reference's normalize_batch, which works in fp32 with torch's
    reductions over the n = T_pad samples of a row: a pairwise / vectorised sum of n terms is within (log2 n + 8) u relative of
    the sum of the absolute values [Higham (4.6) with blocks of 8 lanes]; the std takes the square root of a sum of positive
    terms (half that), and its inputs x - mean carry the mean's error u' = (log2 n + 8) u mean|x| each: relative to the norm at
    most u' / sd (resp. / mx); the final level / norm and 1 / gain round twice more."""
    gold = K.load_golden(model, mode)
    spec = K.spec_of(model, mode)
    norm, zero_mean = _norm_of(mode)
    assert (spec.norm, spec.zero_mean) == (norm, zero_mean)
    eps = K.MODE_ARGS[mode][2]
    assert spec.norm_eps == eps and gold["mix"].shape[0] == K.batch_rows(mode)
    rows = [(torch.from_numpy(gold["mix"])[b], gold["norm_mean"][b], gold["norm_std"][b]) for b in range(K.batch_rows(mode))]
    rows += [(torch.from_numpy(gold[f"mix_f{i}"])[0], gold[f"norm_mean_f{i}"][0], gold[f"norm_std_f{i}"][0])
             for i in range(len(K.FILE_LENGTHS))]
    branches = []
    for x, ref_mean, ref_std in rows:
        xp = K.padded(x, spec.tot_ds)
        st = K.norm_stats(xp, norm, spec.level_db, zero_mean, eps)
        n = xp.numel()
        c = (math.log2(n) + 8) * K.U
        du = c * float(xp.double().abs().mean())
        assert abs(float(ref_mean) - st["mean"]) <= (du if zero_mean else 0.0)
        rel = c + du / min(st["sd"], st["mx"]) + 3 * K.U
        assert abs(float(ref_std) * st["gain"] - 1.0) <= rel, (model, mode, float(ref_std), 1.0 / st["gain"], rel)
        branches.append(st["branch"])
    if mode in ("2max", "2max_keepmean"):  # the fixtures reach both branches: the smooth rows the std, the spiked ones the max
        assert branches == ["std", "max", "std", "max", "std"]
    if mode == "2max_eps":  # the quiet row: both norms under eps, where 2-max's gain is level / eps
        assert branches == ["std", "max", "std", "std", "max", "std"]
        st = K.norm_stats(K.padded(rows[2][0], spec.tot_ds), norm, spec.level_db, zero_mean, eps)
        assert 1e-5 < st["sd"] < st["mx"] < eps and st["gain"] == st["level"] / eps


def test_restatement_takes_the_norms_as_the_reference_does():
    """Hand-made rows: the std is taken around the row's own mean whatever zero_mean says (torch's std), the maximum around
    what is removed; eps reaches 2-max alone."""
    x = torch.tensor([1.0, 3.0, 1.0, 3.0])
    st = K.norm_stats(x, "max", 0.0, zero_mean=False)
    assert st["mean"] == 0.0 and st["mx"] == 3.0 and abs(st["sd"] - math.sqrt(4.0 / 3.0)) < 1e-15
    assert K.norm_stats(x, "max", 0.0)["mx"] == 1.0
    z = torch.zeros(8)
    for norm, want in (("2", 1e5), ("max", 1e5), ("2-max", 1e3)):
        assert K.norm_stats(z, norm, 0.0, eps=1e-3)["gain"] == pytest.approx(want, rel=1e-12)
    assert float(K.gain32("2-max", 0.0, 0.0, 0.0, 1e-3)) == pytest.approx(1e3, rel=1e-6)
    assert K.exact_max(torch.tensor([0.5, -2.0]), 4, 0.25) == 2.25 and K.exact_max(torch.tensor([0.1]), 2, 0.5) == 0.5


# ---- the element reference of the GPU tests (tests/small_fp64.pad_normalize in every mode) ------------------------------------------
def _element_cases():
    """(length tag, T, kind, row) of every row tests/test_gpu_norm_fp64.py holds."""
    spec = get_spec("PP16s")
    for tag, T in K.lengths(spec.tot_ds).items():
        for kind, x in K.element_rows(spec, T).items():
            yield tag, T, kind, x


def _live_normalize_batch():
    """utils/norm.py of the reference checkout, loaded from its file (it imports torch alone)."""
    import importlib.util
    import os

    import ref_import as R

    if not R.reference_available():
        pytest.skip("reference checkout not present")
    s = importlib.util.spec_from_file_location("_ref_norm", os.path.join(R.REFERENCE_ROOT, "open_universe", "utils", "norm.py"))
    m = importlib.util.module_from_spec(s)
    s.loader.exec_module(m)
    return m.normalize_batch


def test_element_rows_exist_at_every_length_and_are_what_they_are_named():
    spec = get_spec("PP16s")
    td = spec.tot_ds
    assert K.element_rows(spec, 65537).keys() == set(K.ROW_KINDS) and list(K.lengths(td).values()) == [1, td - 1, td, td + 1, 65536, 65537]
    assert set(K.element_rows(spec, 1)) == {"smooth", "zero", "const", "quiet"} and "spike_1029" not in K.element_rows(spec, td + 1)
    for T in (td + 1, 65537):
        rows = K.element_rows(spec, T)
        q = K.norm_stats(K.padded(rows["quiet"], td), "2-max", spec.level_db, True, 1e-3)
        assert 1e-5 < q["sd"] < q["mx"] < 1e-3, q  # what separates the eps routing: under eps 1e-3 both clamp, under 1e-5 neither
        # (a spike of 60 sd has the crest factor 1 / level = 20 needs only in a row of more than 450 samples)
        assert K.norm_stats(K.padded(rows["spike0"], td), "2-max", spec.level_db)["branch"] == ("max" if T > 450 else "std")
        assert K.norm_stats(K.padded(rows["smooth"], td), "2-max", spec.level_db)["branch"] == "std"
        z = K.norm_stats(K.padded(rows["zero"], td), "2", spec.level_db)
        assert z["sd"] == 0.0 and z["gain"] == z["level"] / 1e-5


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("norm,zero_mean", K.ALL_MODES)
def test_every_element_row_is_determined(norm, zero_mean, eps):
    """No row of the element tests leaves a clamp or the 2-max branch to rounding: none is left out."""
    spec = get_spec("PP16s")
    n = 0
    for tag, T, kind, x in _element_cases():
        xp = K.padded(x, spec.tot_ds)
        st = K.norm_stats(xp, norm, spec.level_db, zero_mean, eps)
        rho = K.stats_bounds(xp, st, norm, zero_mean)[1]
        assert K.undetermined(st, norm, rho, eps) is None, (tag, kind, K.undetermined(st, norm, rho, eps))
        n += 1
    assert n == 4 + 3 * 6 + 2 * 7
    # and the condition does refuse: a norm one part in 10^8 from its clamp, two gains that close to each other
    st = {"sd": 1e-5 * (1 + 1e-8), "mx": 1.0, "level": 0.05}
    assert K.undetermined(st, "2", 4 * K.U) and K.undetermined(st, "max", 4 * K.U) is None
    assert K.undetermined(dict(st, sd=0.5, mx=1e-3 * (1 - 1e-8)), "2-max", 4 * K.U, 1e-3)
    assert K.undetermined(dict(st, sd=0.05, mx=1 + 1e-8), "2-max", 4 * K.U) and not K.undetermined(dict(st, sd=0.05, mx=1.1), "2-max", 4 * K.U)


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("norm,zero_mean", K.ALL_MODES)
def test_element_reference_is_the_live_normalize_batch_in_float64(norm, zero_mean, eps):
    """small_fp64.pad_normalize against normalize_batch of the reference checkout on the padded row, both in float64.  They
    differ in how they sum.  With e = 2^-53, n = T_pad, c = log2 n + 8 (a blocked pairwise sum, as above) and
    kappa = mean |x| / max |x - mu| of the row: each side's mean is within c e mean |x| of the true one, i.e. c kappa e of the
    largest |x - mu|, which goes into every y and into the maximum (2 sides x 2: 4 c kappa); torch.std is an updating (Welford)
    pass, whose sum of squares is within n k e relative, k = sqrt(1 + mean^2 / var) of what it is handed -- x - mean with
    zero_mean (k = 1), x itself without [Chan, Golub, LeVeque 1983, (5.1)] -- and the root halves it (n k / 2 each side; the
    mean's own error enters the std in second order); the subtraction, the division and the product round once on each side
    (6, + 2 spare):   |y - y_ref| <= (4 c kappa + n k + 8) 2^-53 max |y|,   kappa = 0 with zero_mean false."""
    import small_fp64 as F

    normalize_batch = _live_normalize_batch()
    spec = get_spec("PP16s")
    td = spec.tot_ds
    level = torch.tensor(10.0 ** (spec.level_db / 20.0), dtype=torch.float64)
    worst = 0.0
    for tag, T, kind, x in _element_cases():
        Tp = T + (td - T % td)
        mine, _, lens = F.pad_normalize(x[None, :], [T], Tp, level, td, norm=norm, zero_mean=zero_mean, eps=eps)
        xp = K.padded(x, td).double()
        (theirs, _), _, _ = normalize_batch((xp[None, None, :], None), norm=2 if norm == "2" else norm, level_db=spec.level_db, eps=eps,
                                            zero_mean=zero_mean)
        assert lens == [Tp] and theirs.dtype == torch.float64 and theirs.shape == mine.shape
        mu = float(xp.mean()) if zero_mean else 0.0
        kappa = float(xp.abs().mean()) / max(float((xp - mu).abs().max()), 1e-300) if zero_mean else 0.0
        c = math.log2(Tp) + 8
        k = 1.0 if zero_mean else math.sqrt(1.0 + float(xp.mean()) ** 2 / max(float(xp.var(unbiased=False)), 1e-300))
        room = (4 * c * kappa + Tp * k + 8) * 2.0 ** -53 * float(theirs.abs().max())
        err = float((mine - theirs).abs().max())
        worst = max(worst, err / room if room else float(err != 0))
        assert err <= room, (tag, kind, err, room)
    print(f"pad_normalize vs normalize_batch, float64, {norm} zero_mean {zero_mean} eps {eps}: worst err / room {worst:.3f}")


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("norm,zero_mean", K.ALL_MODES)
def test_fp32_evaluation_of_the_element_reference_stays_inside_its_bound(norm, zero_mean, eps):
    """The derived per-element bound is not one only the kernel can meet: the same reference evaluated in fp32 (sums in double,
    every scalar and every element rounded once) stays inside it on every row, none excluded -- and a padding value that is not
    the row's, or a gain clamped at another constant, does not."""
    import small_fp64 as F

    spec = get_spec("PP16s")
    td = spec.tot_ds
    level = torch.tensor(10.0 ** (spec.level_db / 20.0), dtype=torch.float64).float()
    worst = 0.0
    for tag, T, kind, x in _element_cases():
        Tp = T + (td - T % td)
        kw = dict(norm=norm, zero_mean=zero_mean, eps=eps)
        ref, bound, lens = F.pad_normalize(x[None, :], [T], Tp, level, td, **kw)
        got, _, _ = F.pad_normalize(x[None, :], [T], Tp, level, td, torch.float32, **kw)
        rep = F.Report(f"{tag}.{kind}", got, ref, bound, lens)
        worst = max(worst, rep.ratio)
        assert rep.ok() and rep.excluded == 0, str(rep)
        if not zero_mean:
            assert not got[0, 0, : (Tp - T) // 2].any() and not got[0, 0, (Tp - T) // 2 + T:].any() and float(bound[0, 0, -1]) == 0.0
            bad = got.clone()
            bad[0, 0, -1] = 1e-30  # any padding value but 0
            assert not F.Report("pad", bad, ref, bound, lens).ok()
    print(f"fp32 evaluation, {norm} zero_mean {zero_mean} eps {eps}: worst err / bound {worst:.3f}")
    # the clamp constant: the all-zero row's gain does not reach a sample (0 * gain), the quiet row's does under 2-max with eps 1e-3
    if norm == "2-max" and eps == 1e-3:
        x = K.element_rows(spec, td + 1)["quiet"]
        Tp = 2 * td
        ref, bound, lens = F.pad_normalize(x[None, :], [td + 1], Tp, level, td, norm=norm, zero_mean=zero_mean, eps=eps)
        other, _, _ = F.pad_normalize(x[None, :], [td + 1], Tp, level, td, torch.float32, norm=norm, zero_mean=zero_mean, eps=1e-5)
        assert not F.Report("eps", other, ref, bound, lens).ok()


def test_eps_is_sent_to_the_2max_branch_alone():
    """normalization_kwargs.eps reaches ou_set_normalization under 2-max; max and 2 are handed 0, under which the library keeps
    their clamp at 1e-5 (utils/norm.py:31-39 passes eps to the 2-max branch alone)."""
    for zero_mean in (True, False):
        for norm, mode in (("2", _lib.OU_NORM_2), ("max", _lib.OU_NORM_MAX), ("2-max", _lib.OU_NORM_2MAX)):
            spec = K.mode_spec("PP16s", norm, zero_mean, 1e-3)
            assert (spec.norm, spec.zero_mean, spec.norm_eps) == (norm, zero_mean, 1e-3)
            assert _lib.norm_args(spec) == (mode, int(zero_mean), 1e-3 if norm == "2-max" else 0.0)
            assert _lib.norm_args(K.mode_spec("PP16s", norm, zero_mean)) == (mode, int(zero_mean), 0.0)
