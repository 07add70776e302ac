"""CPU: the bottleneck of the score encoder (seq_model gru | none, encoder_gru_conv_sandwich) through config, state-dict schema,
ABI struct and packer.  The cases are tests/seqmodel_cases.py; tests/golden/seqmodel_names.json holds the real reference's own
state_dict() and model_parameters() orders for them (tests/golden/make_golden_seqmodel.py)."""
import ctypes
import json

import pytest
import torch

import seqmodel_cases as K
from helpers import get_spec, lora_style_state_dict
from open_universe_amd import _lib
from open_universe_amd import config as C
from open_universe_amd import state_dict as S


def _names():
    with open(K.NAMES_JSON) as f:
        return json.load(f)


def _plan(case):
    blob, plan = _lib.pack_weights(K.spec_of(case), K.state_dict_of(case))
    return blob, json.loads(plan)


# ---- config ------------------------------------------------------------------------------------------------------------------
def test_cases_parse_to_what_they_name():
    for case in K.CASES:
        s = K.spec_of(case).score
        assert s.seq_model == ("none" if case in K.NONES else "gru")
        assert s.encoder_gru_conv_sandwich == (case in K.SAND)
        c = _lib.make_config(K.spec_of(case))
        assert c.score.seq_bottleneck == (_lib.OU_SEQ_NONE if case in K.NONES else _lib.OU_SEQ_GRU_SANDWICH)
        assert c.cond.seq_bottleneck == c.cond.encoder_gru_residual == int(K.spec_of(case).cond.encoder_gru_residual)
        assert K.spec_of(case).cond.seq_model == "gru"
    for name in ("PP16", "OR16", "PP24"):
        c = _lib.make_config(get_spec(name))
        assert c.score.seq_bottleneck == _lib.OU_SEQ_GRU == 0
        assert get_spec(name).score.seq_model == "gru" and not get_spec(name).score.encoder_gru_conv_sandwich


def test_the_sandwich_is_ignored_without_a_gru():
    """score.py:81-98: gru_conv_sandwich is set in the gru branch only."""
    spec = C.spec_from_config(C.builtin_config("PP16", **dict(K.NONE, **K.SANDWICH, **K.NARROW)))
    assert spec.score.seq_model == "none" and spec.score.encoder_gru_conv_sandwich is False
    plain = K.spec_of("none_pp")
    assert [k for k, _, _ in S.model_schema(spec)] == [k for k, _, _ in S.model_schema(plain)]
    assert bytes(_lib.make_config(spec)) == bytes(_lib.make_config(plain))


def test_refusals_name_the_field():
    with pytest.raises(NotImplementedError, match=r"seq_model.*no such module"):
        C.spec_from_config(C.builtin_config("PP16", **{"score_model.seq_model": "attention"}))
    for junk in ("lstm", "GRU", 3):
        with pytest.raises(ValueError, match=r"seq_model.*gru\|attention\|none"):
            C.spec_from_config(C.builtin_config("PP16", **{"score_model.seq_model": junk}))
    for v in ("none", "attention", "lstm"):
        with pytest.raises(NotImplementedError, match=r"condition_model\.seq_model") as e:
            C.spec_from_config(C.builtin_config("PP16", **{"condition_model.seq_model": v}))
        assert "condition_model.seq_model: gru" in str(e.value)
    # universe_original.yaml hands the score network's value on: ${model.score_model.seq_model}
    cfg = C.builtin_config("OR16", **{"score_model.seq_model": "none", "condition_model.seq_model": "${model.score_model.seq_model}"})
    with pytest.raises(NotImplementedError, match=r"condition_model\.seq_model"):
        C.spec_from_config(cfg)
    cfg["model"]["condition_model"]["seq_model"] = "gru"
    assert C.spec_from_config(cfg).score.seq_model == "none"


@pytest.mark.parametrize("value", [4, -1, 1 << 16])
def test_abi_refuses_other_values_and_names_the_field(built_lib, value):
    field = "seq_bottleneck"
    cfg = _lib.make_config(get_spec("PP16s"))
    cfg.score.seq_bottleneck = value
    n, packer = ctypes.c_size_t(), ctypes.c_void_p()
    assert built_lib.ou_packed_bytes(ctypes.byref(cfg), ctypes.byref(n)) == _lib.OU_ENOTIMPL
    assert field in built_lib.ou_last_error(None).decode()
    assert built_lib.ou_packer_create(ctypes.byref(cfg), ctypes.byref(packer)) == _lib.OU_ENOTIMPL
    assert field in built_lib.ou_last_error(None).decode()
    h = ctypes.c_void_p()
    dummy = (ctypes.c_float * 4)()  # (never read: the configuration is refused before the blob is looked at)
    assert built_lib.ou_create(ctypes.byref(cfg), dummy, 16, 0, ctypes.byref(h)) == _lib.OU_ENOTIMPL
    assert field in built_lib.ou_last_error(None).decode()


def test_the_struct_keeps_its_size_and_the_slot_is_the_one_the_score_network_never_used():
    """ou_config is what version 7 callers compiled against: it still ends with cond_dec_act, and the bottleneck travels in the
    slot that is encoder_gru_residual for the conditioner -- ScoreNetwork has no such argument, every caller left 0 there."""
    assert ctypes.sizeof(_lib.Config) == _lib.Config.cond_dec_act.offset + 4 == 240
    assert _lib.NetConfig.seq_bottleneck.offset == _lib.NetConfig.encoder_gru_residual.offset == ctypes.sizeof(_lib.NetConfig) - 4
    assert _lib.OU_ABI_VERSION == 7 and (_lib.OU_SEQ_GRU, _lib.OU_SEQ_NONE, _lib.OU_SEQ_GRU_SANDWICH) == (0, 2, 3)
    # the conditioner's reading of the slot is untouched by the score network's
    c = _lib.make_config(K.spec_of("sand_pp"))
    assert (c.score.seq_bottleneck, c.cond.encoder_gru_residual) == (_lib.OU_SEQ_GRU_SANDWICH, 1)


# ---- schema ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(K.CASES))
def test_schema_and_parameter_order_are_the_reference_s(case):
    spec = K.spec_of(case)
    p = spec.score_prefix
    want = _names()[case]
    keys = [k for k, _, _ in S.score_schema(p, spec.score)]
    assert keys == want["state_dict"]
    assert [n for n in S.parameter_names(spec) if n.startswith(p + ".")] == want["parameters"]
    assert list(K.state_dict_of(case)) == [k for k, _, _ in S.model_schema(spec)]
    has = lambda frag: any(frag in k for k in keys)
    assert has(".encoder.gru.") == (case not in K.NONES)
    assert has(".encoder.conv_block1.") == has(".encoder.conv_block2.") == (case in K.SAND)
    if case in K.SAND:
        # registration order of ScoreEncoder.__init__: ds_modules, cond_proj, gru, conv_block1, conv_block2
        first = lambda frag: next(i for i, k in enumerate(keys) if frag in k)
        order = [first(f) for f in (".encoder.ds_modules.", ".encoder.cond_proj.", ".encoder.gru.", ".encoder.conv_block1.",
                                    ".encoder.conv_block2.", ".decoder.")]
        assert order == sorted(order)
        assert not has("conv_block1.rate_change_conv") and not has("conv_block1.conv1.low_pass_filter")
    if case == "sand_snake":
        assert p + ".encoder.conv_block2.conv3.prelu.act.act.alpha" in keys and p + ".encoder.conv_block2.conv3.prelu.weight" not in keys


# ---- packer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(K.CASES))
def test_every_case_packs_and_the_plan_names_the_bottleneck(built_lib, case):
    spec = K.spec_of(case)
    blob, plan = _plan(case)
    names = [c["name"] for c in plan["convs"]]
    p = spec.score_prefix
    assert _lib.packed_bytes(spec) == blob.numel() * 4 == plan["total_floats"] * 4
    sand = [f"{p}.encoder.conv_block{b}.conv{i}" for b in (1, 2) for i in (1, 2, 3)]  # the walk's score.cb1 / score.cb2
    if case in K.SAND:
        assert all(n in names for n in sand)
        assert (plan["score_seq_model"], plan["score_gru_sandwich"]) == ("gru", 1)
        convs = {c["name"]: c for c in plan["convs"]}
        for n in sand:
            L = convs[n]
            assert (L["Cin"], L["Cout"], L["stride"], L["up"], L["fir_mode"]) == (128, 128, 1, 1, 0)
            # every copy the level's kernels read: taps-innermost, Winograd, bf16-split
            assert L["KWP"] in (4, 8) and L["wd_off"] and L["wu_off"] and L["ws_on"] == 1 and L["ws_off"]
            assert L["activation"] == ("snake" if case == "sand_snake" else "prelu")
        # in walk order behind the GRU's projection
        assert names.index(f"{p}.encoder.gru#l0") < names.index(sand[0]) < names.index(sand[3]) < names.index(f"{p}.decoder.up_modules.0.conv1")
    else:
        assert not any(n in names for n in sand)
        assert not any(n.startswith(f"{p}.encoder.gru") for n in names)
        assert (plan["score_seq_model"], plan["score_gru_sandwich"]) == ("none", 0)
        # no GRU tensor of the score network is asked for: a checkpoint without them packs to the same blob
        sd = K.state_dict_of(case)
        assert not any(".encoder.gru." in k and k.startswith(p) for k in sd)
        assert sum(1 for n in names if n.startswith("condition_model.encoder.gru")) == 2


def _pack_raw(L, cfg, sd):
    packer = ctypes.c_void_p()
    _lib.check(L.ou_packer_create(ctypes.byref(cfg), ctypes.byref(packer)))
    try:
        for key, t in sd.items():
            shape = (ctypes.c_int64 * max(1, t.ndim))(*t.shape)
            _lib.check(L.ou_packer_set(packer, key.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.ndim), packer=packer)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _lib.check(L.ou_packer_finish(packer, ctypes.byref(p), ctypes.byref(n)), packer=packer)
        return bytes(ctypes.string_at(p, n.value)), L.ou_packer_plan_json(packer).decode()
    finally:
        L.ou_packer_destroy(packer)


@pytest.mark.parametrize("name", ["PP16", "OR16", "PP24"])
def test_shipped_config_blob_and_plan_are_the_parent_commit_s(built_lib, name):
    """ou_config as make_config fills it, the blob bytes and the plan text of the shipped topologies are what the commit before this
    feature produced: tests/golden/seqmodel_parent_pack.json holds that commit's ou_config bytes and the SHA-256 of its blob and
    plan.  (n_channels 8: the shipped topologies at the width the CPU suite packs in seconds; the layout code has no branch on
    the width.)  A caller that spells the slot out as OU_SEQ_GRU gets the same."""
    import hashlib
    import os

    with open(os.path.join(K.GOLDEN, "seqmodel_parent_pack.json")) as f:
        want = json.load(f)[name]
    spec = C.spec_from_config(C.builtin_config(name, **K.NARROW))
    sd = S.synthetic_state_dict(spec, seed=0)
    cfg = _lib.make_config(spec)
    assert cfg.score.seq_bottleneck == 0 and bytes(cfg).hex() == want["config_hex"]
    blob, plan = _pack_raw(built_lib, cfg, sd)
    assert hashlib.sha256(blob).hexdigest() == want["blob_sha256"]
    assert hashlib.sha256(plan.encode()).hexdigest() == want["plan_sha256"]
    assert "score_seq_model" not in plan and "conv_block1" not in plan.split("condition_model")[0]
    blob2, plan2 = _lib.pack_weights(spec, sd)
    assert blob2.numpy().tobytes() == blob and plan2 == plan
    # a caller that filled `score` from its conditioner block: encoder_gru_residual = 1 there was always ignored, and still is
    cfg.score.encoder_gru_residual = 1
    assert _pack_raw(built_lib, cfg, sd) == (blob, plan)


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------
def test_ema_lora_and_weight_norm_removed_checkpoints_of_a_sandwich_model(built_lib):
    spec = K.spec_of("sand_pp")
    sd = K.state_dict_of("sand_pp")
    blob, _ = _lib.pack_weights(spec, S.inference_state_dict(spec, {"state_dict": sd}))
    # EMA: the shadow weights win, the two blocks included
    ck = S.checkpoint_from_state_dict(spec, sd, with_ema=True, ema_jitter=0.01)
    assert len(ck["ema"]["shadow_params"]) == len(S.parameter_names(spec))
    got = S.inference_state_dict(spec, ck)
    names = S.parameter_names(spec)
    key = spec.score_prefix + ".encoder.conv_block2.conv3.conv.weight_v"
    assert torch.equal(got[key], ck["ema"]["shadow_params"][names.index(key)]) and not torch.equal(got[key], sd[key])
    # the LoRA-style form (keys under `model.`, weight-norm removed, adapters on the transposed convs) and the weight-norm-removed
    # merged form resolve to the same blob, bit for bit; the weight-normed original to the same weights up to the fold's rounding
    lora, merged = lora_style_state_dict(sd)
    cb = spec.score_prefix + ".encoder.conv_block1.conv1.conv"
    assert "model." + cb + ".weight" in lora and cb + ".weight" in merged and cb + ".weight_v" not in merged
    assert any(".lora_weight_a" in k for k in lora)
    blob_l, _ = _lib.pack_weights(spec, S.inference_state_dict(spec, {"state_dict": lora}))
    blob_m, _ = _lib.pack_weights(spec, S.inference_state_dict(spec, {"state_dict": merged}))
    assert torch.equal(blob_l.view(torch.int32), blob_m.view(torch.int32))
    unnormed = {k: v for k, v in merged.items()}
    for k in list(unnormed):  # the merged form without the adapters' contribution: the original model with weight-norm removed
        if k.endswith("rate_change_conv.conv.weight") and ".decoder.up_modules." in k:
            unnormed[k] = torch._weight_norm(sd[k + "_v"], sd[k + "_g"], 0)
    blob_u, plan_u = _lib.pack_weights(spec, S.inference_state_dict(spec, {"state_dict": unnormed}))
    convs = {c["name"]: c for c in json.loads(plan_u)["convs"]}
    for b_ in (1, 2):
        L = convs[f"{spec.score_prefix}.encoder.conv_block{b_}.conv2"]
        n = L["Cin"] * L["KW"] * L["Mp"]
        assert torch.allclose(blob_u[L["w_off"]: L["w_off"] + n], blob[L["w_off"]: L["w_off"] + n], rtol=1e-5, atol=1e-8)
        assert blob[L["w_off"]: L["w_off"] + n].abs().max() > 0


def test_a_sandwich_checkpoint_and_a_plain_config_and_the_other_way_round(built_lib):
    sand, plain = K.spec_of("sand_pp"), C.spec_from_config(C.builtin_config("PP16", **K.NARROW))
    sd = K.state_dict_of("sand_pp")
    # unchanged behaviour: the plain configuration walks its own schema and never looks at keys it does not know
    got = S.inference_state_dict(plain, {"state_dict": sd})
    assert not any("conv_block1" in k and k.startswith(plain.score_prefix) for k in got)
    _lib.pack_weights(plain, got)
    # the sandwich configuration on a checkpoint without the blocks names what is missing
    bare = {k: v for k, v in sd.items() if ".encoder.conv_block" not in k or k.startswith("condition_model")}
    with pytest.raises(KeyError, match="conv_block1"):
        S.inference_state_dict(sand, {"state_dict": bare})
    with pytest.raises(KeyError, match="conv_block1"):
        _lib.pack_weights(sand, bare)
    # ... and an EMA checkpoint of the sandwich model no longer fails on a parameter count
    ck = S.checkpoint_from_state_dict(sand, sd, with_ema=True)
    S.inference_state_dict(sand, ck)
