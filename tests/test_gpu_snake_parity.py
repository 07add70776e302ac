"""GPU (-m gpu): networks whose ConvBlocks use Snake activations (encoder_act_type / decoder_act_type), loaded through
`load_model` from a config.yaml + checkpoint, against recordings of the REAL reference (tests/golden/snake_<case>.npz, written by
tests/golden/make_golden_snake.py).

Floor: what the small-model golden tests of test_gpu_parity.py apply -- helpers.record(), SI-SDR and plain SNR >= 60 dB
(BASELINE.json's tolerance; no gate of tests/parity_gates.json names these figures).  The observed dB also go to
build/observed/snake_fp64_observed.json (untracked; section "parity_db"; profiles/snake_fp64_observed.json is a committed copy)."""
import numpy as np
import pytest
import torch
import yaml

import restatement as O
import snake_cases as K
from helpers import get_spec, record, synth_mix
from open_universe_amd import config as C
from open_universe_amd import inference_utils
from open_universe_amd import state_dict as S
from open_universe_amd import universe as U
from test_gpu_snake_fp64 import observe

pytestmark = pytest.mark.gpu

_models = {}


def get_model(case, tmp_path_factory):
    if case not in _models:
        d = tmp_path_factory.mktemp("snake_" + case)
        with open(d / "config.yaml", "w") as f:
            yaml.safe_dump(C.builtin_config("PP16", **K.overrides(case)), f)
        torch.save({"state_dict": K.state_dict_of(case)}, d / "weights.ckpt")
        _models[case] = inference_utils.load_model(d / "weights.ckpt", device="cuda:0")
    return _models[case]


def parity(name, ref, out):
    v = O.si_sdr(ref, out)
    observe("parity_db", name, {"si_sdr": round(float(v), 2), "snr": round(float(getattr(v, "snr", float("nan"))), 2)})
    return record(name, v)


def enhance(model, mix, noise, **kw):
    """model._enhance on a given noise tensor (n, B, 1, T_pad) -- the arguments of `enhance` plus the noise."""
    a = dict(n_steps=K.N_STEPS, warm_start=None, keep_rms=False)
    a.update(kw)
    return model._enhance(mix.cuda(), a["n_steps"], None, None, None, None, False, a["keep_rms"], None, "median", a["warm_start"],
                          noise.cuda()).cpu()


@pytest.mark.parametrize("case", list(K.CASES))
def test_enhance_vs_reference_golden(case, tmp_path_factory):
    gold = K.load_golden(case)
    model = get_model(case, tmp_path_factory)
    assert model.spec.score.encoder_act_type == K.CASES[case]["score_model.encoder_act_type"]
    mix = torch.from_numpy(gold["mix"])
    out = enhance(model, mix, torch.from_numpy(gold["noise"]))
    ref = torch.from_numpy(gold["enh"])
    assert out.shape == ref.shape and torch.isfinite(out).all()
    parity(f"snake.{case}.plain", ref, out)
    out = enhance(model, mix, torch.from_numpy(gold["noise_warm"]), warm_start=1)
    parity(f"snake.{case}.warm", torch.from_numpy(gold["enh_warm"]), out)


@pytest.mark.parametrize("case", list(K.CASES))
def test_ragged_enhance_many_vs_per_file_goldens(case, tmp_path_factory, monkeypatch):
    """ONE enhance_many call over three files of different lengths (ou_enhance_var) against the reference run on every file alone.
    The noise of the call is the recorded noise of the three files, handed over where enhance_many draws its own."""
    gold = K.load_golden(case)
    model = get_model(case, tmp_path_factory)
    files = [torch.from_numpy(gold[f"mix_f{i}"])[0].cuda() for i in range(len(K.FILE_LENGTHS))]
    Tmax = max(gold[f"noise_f{i}"].shape[-1] for i in range(len(files)))
    planes = torch.zeros(K.N_STEPS, len(files), 1, Tmax)
    for i in range(len(files)):
        nz = torch.from_numpy(gold[f"noise_f{i}"])
        planes[:, i:i + 1, :, :nz.shape[-1]] = nz
    drawn = []

    def recorded_noise(tot_ds, entries, n, **kw):
        drawn.append(([int(e[1]) for e in entries], n))
        return planes.cuda()

    monkeypatch.setattr(U, "draw_noise", recorded_noise)
    outs = model.enhance_many(files, n_steps=K.N_STEPS)
    assert drawn == [(list(K.FILE_LENGTHS), K.N_STEPS)]
    for i, o in enumerate(outs):
        ref = torch.from_numpy(gold[f"enh_f{i}"])[0]
        assert o.shape == ref.shape
        parity(f"snake.{case}.many.file{i}", ref, o.cpu())


@pytest.mark.parametrize("case", ["snakebeta"])
def test_enhance_long_of_one_window_is_enhance(case, tmp_path_factory):
    model = get_model(case, tmp_path_factory)
    gold = K.load_golden(case)
    x = torch.from_numpy(gold["mix_f0"])[0].cuda()
    a = model.enhance(x, n_steps=K.N_STEPS, rng=torch.Generator(device="cuda").manual_seed(5))
    b = model.enhance_long(x, n_steps=K.N_STEPS, rng=torch.Generator(device="cuda").manual_seed(5))
    assert torch.equal(a, b)


def test_no_fused_convblock_body_for_a_snake_model(tmp_path_factory):
    """ou_launch_stats: with every ConvBlock of both networks on a non-PReLU activation no fused body may run -- the counts of a call
    are those of the same call with the fused bodies switched off (option fuse = 0); the PReLU model of the same width does fuse."""
    gold = K.load_golden("snakebeta")
    mix, nz = torch.from_numpy(gold["mix"]), torch.from_numpy(gold["noise"])
    counts = {}
    for name, model in (("snakebeta", get_model("snakebeta", tmp_path_factory)),
                        ("prelu", U.UniverseGAN(get_spec("PP16s"), state_dict=S.synthetic_state_dict(get_spec("PP16s"), K.SEED),
                                                device="cuda:0"))):
        out = enhance(model, mix, nz)
        default = model.launch_stats()
        model.set_option("fuse", 0)
        out0 = enhance(model, mix, nz)
        counts[name] = (default, model.launch_stats())
        model.reset_options()
        if name == "snakebeta":
            assert torch.equal(out, out0)
    (d, u), (pd, pu) = counts["snakebeta"], counts["prelu"]
    assert d == u, f"a fused body ran for the Snake model: {d} launches against {u} unfused"
    assert pd[1] < pu[1], "the PReLU model of the same shape takes fused bodies (else this test shows nothing)"
    # the Snake launches are counted: 3 per ConvBlock on top of the unfused PReLU walk, none of them a conv launch
    assert u[1] == pu[1] and u[0] > pu[0]
    plan = __import__("json").loads(get_model("snakebeta", tmp_path_factory)._L.ou_plan_json(
        get_model("snakebeta", tmp_path_factory)._handle).decode())
    n_snake = plan["n_snake"]
    blocks = 2 * (len(get_spec("PP16s").score.rate_factors) + 1)
    # conditioner once (3 blocks more than its encoder / decoder ladders: conv_block1, conv_block2, input_conv_block; the mel
    # ConvBlock keeps PReLU), score network once per step
    assert n_snake == 3 * (2 * blocks + 3)
    assert u[0] - pu[0] == 3 * (blocks + 3) + K.N_STEPS * 3 * blocks


def test_prelu_model_is_untouched_by_a_snake_model_in_the_process(tmp_path_factory):
    spec = get_spec("PP16s")
    prelu = U.UniverseGAN(spec, state_dict=S.synthetic_state_dict(spec, seed=0), device="cuda:0")
    B, T = 2, spec.tot_ds * 9 + 11
    mix = synth_mix(spec, B, T)
    nz = torch.stack(K.noise_planes(3, 4, B, T + (spec.tot_ds - T % spec.tot_ds)))
    before = enhance(prelu, mix, nz, n_steps=4)
    stats = prelu.launch_stats()
    gold = K.load_golden("snake")
    enhance(get_model("snake", tmp_path_factory), torch.from_numpy(gold["mix"]), torch.from_numpy(gold["noise"]))
    after = enhance(prelu, mix, nz, n_steps=4)
    assert torch.equal(before, after) and prelu.launch_stats() == stats
    assert np.isfinite(before.numpy()).all()
