"""CPU: the oracle and the key schema against what the reference itself produced for these exact cases: its resolved model
configs, state-dict key shapes, enhance outputs, buffers and transform windows, recorded from the reference's own classes by
`tests/golden/make_golden.py live` (tests/golden/live_ref.npz / live_ref.json)."""
import json
import os

import numpy as np
import pytest
import torch

import restatement as O
from helpers import get_spec, synth_mix
from open_universe_amd import config as C
from open_universe_amd import state_dict as S

G = os.path.join(os.path.dirname(__file__), "golden")
GOLD = np.load(os.path.join(G, "live_ref.npz"))
with open(os.path.join(G, "live_ref.json")) as _f:
    META = json.load(_f)


def _loads_into_reference(sd, ref_shapes):
    """What the reference's `load_state_dict(sd, strict=False)` checks: no key it does not have, every key it has that `sd`
    lacks is a training loss module's, and every shared key has the reference's shape."""
    unexpected = set(sd) - set(ref_shapes)
    missing = set(ref_shapes) - set(sd)
    assert not unexpected and all(k.startswith("loss_") for k in missing)
    for k, v in sd.items():
        assert list(v.shape) == ref_shapes[k], k


def _ref(name, ref_cfg, width):
    case = META["cases"][name]
    assert case["ref_cfg"] == ref_cfg
    spec = C.spec_from_config(C.builtin_config(name, **{"score_model.n_channels": width}))
    assert spec.to_dict() == C.spec_from_config({"model": case["model_cfg"]}).to_dict()
    sd = S.synthetic_state_dict(spec, seed=5)
    _loads_into_reference(sd, case["state_dict_shapes"])
    return spec, sd


@pytest.mark.parametrize("name,ref_cfg", [("PP16", "default"), ("OR16", "universe_original"), ("PP24", "universepp_24k")])
def test_oracle_enhance_matches_live_reference(name, ref_cfg):
    spec, sd = _ref(name, ref_cfg, 8)
    mix = synth_mix(spec, 2, spec.tot_ds * 10 + 13)
    ref = torch.from_numpy(GOLD[name + "_enh"])
    out = O.enhance(sd, spec.to_dict(), mix, n_steps=3, rng=torch.Generator().manual_seed(3))
    assert O.si_sdr(ref, out) > 100
    # oracle-score diagnostic mode bypasses the network: bit-exact
    tgt = 0.5 * mix[:, None, :]
    ref = torch.from_numpy(GOLD[name + "_fake"])
    out = O.enhance(sd, spec.to_dict(), mix[:, None, :], n_steps=3, target=tgt, fake_score_snr=10.0,
                    rng=torch.Generator().manual_seed(3))
    assert torch.equal(ref, out)


def test_buffers_bit_exact_vs_reference():
    spec = get_spec("PP16")
    bufs = {k[len("buf:"):] for k in GOLD.files if k.startswith("buf:")}
    mine = set()
    for k, shape, is_p in S.model_schema(spec):
        if not is_p:
            mine.add(k)
            assert torch.equal(torch.from_numpy(GOLD["buf:" + k]), S.buffer_value(k, shape)), k
    assert mine == bufs


def test_edm_data_level_and_noisy_ref_match_live_reference():
    """Config options no shipped yaml sets: `edm.data_level_db` (universe.py:176-178) and
    `normalization_kwargs.ref = noisy` (utils/norm.py:83-84, only visible with `target`)."""
    spec = C.spec_from_config({"model": META["edm"]["model_cfg"]})
    assert spec.edm_data_level_db == -20.0 and spec.norm_ref == "noisy"
    sd = S.synthetic_state_dict(spec, seed=5)
    _loads_into_reference(sd, META["edm"]["state_dict_shapes"])
    mix = synth_mix(spec, 2, spec.tot_ds * 6 + 5)
    ref = torch.from_numpy(GOLD["edm_enh"])
    out = O.enhance(sd, spec.to_dict(), mix, n_steps=3, rng=torch.Generator().manual_seed(3))
    assert O.si_sdr(ref, out) > 100
    tgt = 0.5 * mix[:, None, :] + 0.01
    ref = torch.from_numpy(GOLD["edm_fake"])
    out = O.enhance(sd, spec.to_dict(), mix[:, None, :], n_steps=3, target=tgt, fake_score_snr=10.0,
                    rng=torch.Generator().manual_seed(3))
    assert torch.equal(ref, out)


from helpers import TRANSFORM_CASES  # noqa: E402


def test_transform_restatement_matches_live_reference():
    """CompressedMagSTFT(Padded) of the oracle against the reference's classes
    (layers/dyn_range_comp.py), forward and inverse, incl. the Padded variant's double `_pad` -- with the window the
    reference's class builds (live_ref.npz) and its outputs (transform.npz)."""
    fwd_inv = np.load(os.path.join(G, "transform.npz"))
    x = synth_mix(get_spec("PP16"), 2, 4000)[:, None, :] * 5.0
    for tag, stft_kw, spec_kw, pad_block in TRANSFORM_CASES:
        kw = dict(n_fft=stft_kw["n_fft"], hop_length=stft_kw["hop_length"], window=torch.from_numpy(GOLD["window:" + tag]),
                  pad_block=pad_block, **spec_kw)
        y_ref = torch.from_numpy(fwd_inv[tag + "_fwd"])
        y = O.compressed_mag_stft(x, **kw)
        assert y.shape == y_ref.shape and torch.equal(y, y_ref), tag
        length = None if pad_block else 4000
        assert torch.equal(O.compressed_mag_stft(y, inv=True, length=length, **kw), torch.from_numpy(fwd_inv[tag + "_inv"])), tag
