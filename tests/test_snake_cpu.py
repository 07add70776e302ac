"""CPU: Snake activations of the ConvBlock body convs (encoder_act_type / decoder_act_type) through config, ABI struct, state-dict
schema and packer; the host-side refusals of ou_snake_act; and the float64 restatement of tests/snake_fp64.py against the
reference's own Activation1d where the reference checkout is present."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import yaml

import ref_import as R
import snake_cases as K
import snake_fp64 as F
from helpers import get_spec
from open_universe_amd import _lib
from open_universe_amd import config as C
from open_universe_amd import state_dict as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- config ------------------------------------------------------------------------------------------------------------------
def test_yaml_act_types_reach_the_spec(tmp_path):
    cfg = C.builtin_config("PP16", **{"score_model.encoder_act_type": "snake", "condition_model.decoder_act_type": "snakebeta"})
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(cfg))
    spec = C.spec_from_config(C.load_config(path))
    assert spec.score.encoder_act_type == "snake" and spec.score.decoder_act_type == "prelu"
    assert spec.cond.encoder_act_type == "prelu" and spec.cond.decoder_act_type == "snakebeta"
    c = _lib.make_config(spec)
    assert (c.score_enc_act, c.score_dec_act, c.cond_enc_act, c.cond_dec_act) == (_lib.OU_ACT_SNAKE, 0, 0, _lib.OU_ACT_SNAKEBETA)
    # the shipped configurations spell `prelu` out or leave it out: both are the zeroed tail
    for name in ("PP16", "OR16", "PP24"):
        c = _lib.make_config(get_spec(name))
        assert (c.score_enc_act, c.score_dec_act, c.cond_enc_act, c.cond_dec_act) == (0, 0, 0, 0)
    none = C.spec_from_config(C.builtin_config("OR16", **{"score_model.decoder_act_type": "none"}))
    assert _lib.make_config(none).score_dec_act == _lib.OU_ACT_IDENTITY


@pytest.mark.parametrize("key", ["score_model.encoder_act_type", "condition_model.decoder_act_type"])
def test_unknown_act_type_is_refused(key):
    with pytest.raises(ValueError, match="act_type"):
        C.spec_from_config(C.builtin_config("PP16", **{key: "gelu"}))


def test_abi_refuses_an_unknown_activation_code(built_lib):
    cfg = _lib.make_config(get_spec("PP16s"))
    cfg.cond_enc_act = 7
    n = ctypes.c_size_t()
    assert built_lib.ou_packed_bytes(ctypes.byref(cfg), ctypes.byref(n)) == _lib.OU_ENOTIMPL


# ---- schema and packer ---------------------------------------------------------------------------------------------------------
def test_schema_carries_the_reference_keys():
    spec = K.spec_of("snakebeta")
    keys = {k: (shape, is_p) for k, shape, is_p in S.model_schema(spec)}
    p = "_edm_model.encoder.ds_modules.1.conv2"
    assert keys[p + ".prelu.act.act.alpha"] == ((16,), True) and keys[p + ".prelu.act.act.beta"] == ((16,), True)
    assert keys[p + ".prelu.act.upsample.kernel"] == ((2, 1, 15), False)
    assert keys[p + ".prelu.act.downsample.kernel"] == ((1, 1, 28), False)
    assert p + ".prelu.weight" not in keys
    # act_type reaches conv1 .. conv3 only: rate-change convs, st convs and the mel ConvBlock keep their PReLU
    for q in ("_edm_model.encoder.ds_modules.1.rate_change_conv", "condition_model.encoder.st_convs.0",
              "condition_model.input_mel.conv_block.conv1"):
        assert q + ".prelu.weight" in keys
    c = "condition_model.decoder.up_modules.2.conv1"
    assert c + ".prelu.act.act.alpha" in keys and c + ".prelu.act.act.beta" not in keys
    mixed = {k for k, _, _ in S.model_schema(K.spec_of("mixed"))}
    e = "_edm_model.encoder.ds_modules.0.conv1"
    assert not any(k.startswith(e + ".prelu") for k in mixed) and e + ".conv.weight_v" in mixed
    # the recorded fixtures hold exactly the Snake parameters of the recipe
    gold = K.load_golden("snakebeta")
    sd = K.state_dict_of("snakebeta")
    for k in gold.files:
        if k.startswith("sd:"):
            assert np.array_equal(gold[k], sd[k[3:]].numpy()), k
    spread = np.concatenate([gold[k] for k in gold.files if k.startswith("sd:")])
    assert spread.std() > 0.5  # not the zero init


def test_packer_takes_snake_layers_and_names_a_missing_alpha(built_lib):
    spec = K.spec_of("snakebeta")
    sd = K.state_dict_of("snakebeta")
    blob, plan = _lib.pack_weights(spec, sd)
    plan = json.loads(plan)
    convs = {c["name"]: c for c in plan["convs"]}
    L = convs["_edm_model.decoder.up_modules.1.conv3"]
    assert L["activation"] == "snakebeta" and L["act"] == 0
    assert convs["condition_model.encoder.conv_block1.conv1"]["activation"] == "snake"
    assert convs["condition_model.input_mel.conv_block.conv1"]["activation"] == "prelu"
    assert convs["_edm_model.decoder.up_modules.1.rate_change_conv"]["activation"] == "prelu"
    assert convs["_edm_model.decoder.signal_cond_proj.0"]["activation"] == "none"
    p = L["name"] + ".prelu.act.act."
    assert torch.equal(blob[L["sa_off"]: L["sa_off"] + L["Cin"]], torch.exp(sd[p + "alpha"]))
    assert torch.equal(blob[L["sb_off"]: L["sb_off"] + L["Cin"]], torch.exp(sd[p + "beta"]))
    assert plan["n_snake"] > 0
    up = blob[plan["snake_up_off"]: plan["snake_up_off"] + 30]
    down = blob[plan["snake_down_off"]: plan["snake_down_off"] + 28]
    assert torch.equal(up, S.sinc_resample_kernel(1, 2).reshape(-1)) and torch.equal(down, S.sinc_resample_kernel(2, 1).reshape(-1))
    assert _lib.packed_bytes(spec) == blob.numel() * 4 == plan["total_floats"] * 4
    # a checkpoint without the Resample buffers: the packer computes the same two kernels
    bare = {k: v for k, v in sd.items() if not k.endswith("sample.kernel") or k.startswith("signal_decoupling_layer")}
    assert len(bare) < len(sd)
    blob2, _ = _lib.pack_weights(spec, bare)
    assert torch.equal(blob2.view(torch.int32), blob.view(torch.int32))
    # a missing parameter is named
    for leaf in ("alpha", "beta"):
        key = "_edm_model.encoder.ds_modules.2.conv1.prelu.act.act." + leaf
        with pytest.raises(KeyError, match=re.escape(key)):
            _lib.pack_weights(spec, {k: v for k, v in sd.items() if k != key})
    # ... and so is a layer whose tensors are those of another act_type: a PReLU checkpoint under a Snake config and back
    prelu_spec = get_spec("PP16s")
    prelu_sd = S.synthetic_state_dict(prelu_spec, seed=K.SEED)
    with pytest.raises(KeyError, match="prelu"):
        _lib.pack_weights(spec, prelu_sd)
    with pytest.raises(KeyError, match="prelu"):
        _lib.pack_weights(prelu_spec, sd)
    with pytest.raises(KeyError, match=r"conv1\.prelu\.weight"):
        _lib.pack_weights(K.spec_of("mixed"), prelu_sd)  # act_type none carries no activation tensor


def test_all_prelu_blob_does_not_depend_on_how_the_tail_is_spelled(built_lib):
    spec = get_spec("PP16s")
    sd = S.synthetic_state_dict(spec, seed=0)
    blob0, plan0 = _lib.pack_weights(spec, sd)
    assert json.loads(plan0)["n_snake"] == 0 and all(c["sa_off"] == 0 for c in json.loads(plan0)["convs"])

    def packed(cfg):
        packer = ctypes.c_void_p()
        _lib.check(built_lib.ou_packer_create(ctypes.byref(cfg), ctypes.byref(packer)))
        try:
            for key, t in sd.items():
                shape = (ctypes.c_int64 * max(1, t.ndim))(*t.shape)
                _lib.check(built_lib.ou_packer_set(packer, key.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.ndim), packer=packer)
            p, n = ctypes.c_void_p(), ctypes.c_size_t()
            _lib.check(built_lib.ou_packer_finish(packer, ctypes.byref(p), ctypes.byref(n)), packer=packer)
            return bytes(ctypes.string_at(p, n.value))
        finally:
            built_lib.ou_packer_destroy(packer)

    zero_tail = _lib.make_config(spec)
    assert (zero_tail.score_enc_act, zero_tail.cond_dec_act) == (0, 0)
    spelled = _lib.make_config(spec)
    spelled.score_enc_act = spelled.score_dec_act = spelled.cond_enc_act = spelled.cond_dec_act = _lib.OU_ACT_PRELU
    # a caller compiled before the fields existed: its struct ends at no_split_copy, and what follows in its buffer is zero
    old_size = _lib.Config.no_split_copy.offset + 4
    assert ctypes.sizeof(_lib.Config) == old_size + 16
    raw = (ctypes.c_char * ctypes.sizeof(_lib.Config))()
    ctypes.memmove(raw, ctypes.byref(zero_tail), old_size)
    old_caller = _lib.Config.from_buffer(raw)
    want = blob0.numpy().tobytes()
    for cfg in (zero_tail, spelled, old_caller):
        n = ctypes.c_size_t()
        _lib.check(built_lib.ou_packed_bytes(ctypes.byref(cfg), ctypes.byref(n)))
        assert n.value == len(want)
        assert packed(cfg) == want


# ---- the stateless entry point ---------------------------------------------------------------------------------------------------
def test_snake_act_refusals_are_decided_on_the_host(built_lib):
    L = built_lib
    assert L.ou_snake_tile() >= 64 and L.ou_snake_tile() % 4 == 0
    p = ctypes.c_void_p(4096)  # never dereferenced: every refusal below comes before the first HIP call (there is no device here)

    def call(B=1, C=1, T=8, stride=None, lens=None, x=p, y=p, ea=p, up=p, down=p):
        ln = None if lens is None else (ctypes.c_int32 * len(lens))(*lens)
        return L.ou_snake_act(x, y, B, C, T, T if stride is None else stride, ln, ea, None, up, down, None)

    for kw in (dict(B=0), dict(C=0), dict(T=0), dict(B=-1), dict(C=65536), dict(T=2**31 - 1), dict(stride=7),
               dict(B=2, lens=[3, 9]), dict(B=2, lens=[-1, 8]), dict(x=None), dict(y=None), dict(ea=None), dict(up=None),
               dict(down=None), dict(B=2**20, C=2**15, T=8, stride=2**40)):
        assert call(**kw) == _lib.OU_EINVAL, kw
        assert b"ou_snake_act" in L.ou_last_error(None)


def test_library_exports_every_declared_symbol(built_lib):
    for name in _lib.EXPORTED_SYMBOLS + _lib.TUNING_SYMBOLS:
        assert hasattr(built_lib, name), name
    assert {"ou_snake_act", "ou_snake_tile"} <= set(_lib.EXPORTED_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "ouniverse.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ou_[a-z0-9_]+)\s*\(", header))
    assert declared - set(_lib.EXPORTED_SYMBOLS) == set(), declared - set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(built_lib, name), name


# ---- the float64 restatement -----------------------------------------------------------------------------------------------------
def test_restatement_kernels_are_the_checkpoint_buffers():
    assert np.array_equal(F.UP_K, S.sinc_resample_kernel(1, 2).numpy().reshape(2, 15)) and F.UP_W == 7
    assert np.array_equal(F.DOWN_K, S.sinc_resample_kernel(2, 1).numpy().reshape(1, 28)) and F.DOWN_W == 13


def test_recorded_reference_error_covers_the_cases(built_lib):
    rec = F.ref_error()
    assert rec["tile"] == built_lib.ou_snake_tile()
    tags = [c[0] for c in F.cases(rec["tile"])]
    assert sorted(tags) == sorted(rec["cases"]) and len(set(tags)) == len(tags)
    assert rec["max_rel"] == max(v["ref_fp32"] for v in rec["cases"].values())
    # fp32 round-off of sums of 15 + 28 products and a sine whose argument reaches a few hundred: 1e-7 .. 1e-4
    assert 1e-7 < rec["max_rel"] < 1e-4 and rec["max_rel_fp64"] < 1e-12
    Ts = {c[1] for c in F.cases(rec["tile"])}
    t = rec["tile"]
    assert {1, 2, 11, 12, 13, t - 1, t, t + 1, 2 * t + 5} <= Ts


@pytest.mark.skipif(not R.reference_available(), reason="reference checkout not present")
def test_restatement_matches_the_reference_activation1d():
    rec = F.ref_error()
    worst64 = worst32 = 0.0
    for tag, T, C, B, beta, lens in F.cases(rec["tile"]):
        x, la, lb = F.case_input(T, C, B, beta)
        ref64 = F.reference_output(x, la, lb, lens, torch.float64)
        mine = F.snake_act(x, F.f64_of_logs(la), F.f64_of_logs(lb), lens)
        assert mine.shape == ref64.shape
        worst64 = max(worst64, F.rel_error(ref64, mine))
        if lens is not None:  # zero behind every row's own end
            for b, n in enumerate(lens):
                assert not mine[b, :, n:].any()
        r32 = F.rel_error(F.reference_output(x, la, lb, lens, torch.float32), F.snake_act(x, F.exp32(la), F.exp32(lb), lens))
        worst32 = max(worst32, r32)
    print(f"reference float64 vs restatement: {worst64:.3e}; reference fp32 vs restatement: {worst32:.3e} (recorded {rec['max_rel']:.3e})")
    assert worst64 < 1e-12
    # the recorded figure is this machine-dependent number (thread count, conv algorithm) up to a small factor
    assert rec["max_rel"] / 2 < worst32 < rec["max_rel"] * 2
