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
    want = {"max": (_lib.OU_NORM_MAX, 1, 0.0), "2max": (_lib.OU_NORM_2MAX, 1, 0.0), "keepmean": (_lib.OU_NORM_2, 0, 0.0)}[mode]
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
    return {"max": ("max", True), "2max": ("2-max", True), "keepmean": ("2", False)}[mode]


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
    rows = [(torch.from_numpy(gold["mix"])[b], gold["norm_mean"][b], gold["norm_std"][b]) for b in range(K.B)]
    rows += [(torch.from_numpy(gold[f"mix_f{i}"])[0], gold[f"norm_mean_f{i}"][0], gold[f"norm_std_f{i}"][0])
             for i in range(len(K.FILE_LENGTHS))]
    branches = []
    for x, ref_mean, ref_std in rows:
        xp = K.padded(x, spec.tot_ds)
        st = K.norm_stats(xp, norm, spec.level_db, zero_mean)
        n = xp.numel()
        c = (math.log2(n) + 8) * K.U
        du = c * float(xp.double().abs().mean())
        assert abs(float(ref_mean) - st["mean"]) <= (du if zero_mean else 0.0)
        rel = c + du / min(st["sd"], st["mx"]) + 3 * K.U
        assert abs(float(ref_std) * st["gain"] - 1.0) <= rel, (model, mode, float(ref_std), 1.0 / st["gain"], rel)
        branches.append(st["branch"])
    if mode == "2max":  # the fixtures reach both branches: the smooth rows the std, the spiked ones the max
        assert branches == ["std", "max", "std", "max", "std"]


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
