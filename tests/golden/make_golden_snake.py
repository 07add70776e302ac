"""
Golden vectors of the REAL reference for models whose ConvBlocks use Snake activations (encoder_act_type / decoder_act_type:
score.py:223-224, condition.py:283-284, blocks.py:176-187), and the reference's own fp32 error on the inputs of the
snake_act_kernel test.  Needs the reference checkout (oracle/ref_import.py); run on a CPU:

    python tests/golden/make_golden_snake.py

Writes
    snake_<case>.npz   per case of tests/snake_cases.py (PP16s with the activations turned; seeded synthetic weights whose Snake
                       parameters are spread over log-scale values, not the reference's zero init), 3 steps, fixed seeds:
                         mix, noise, enh              a batch of two rows of a ragged length (T % tot_ds != 0)
                         noise_warm, enh_warm         the same batch with warm_start = 1 (aux_to_wav + noise, universe.py:328-331)
                         mix_f<i>, noise_f<i>, enh_f<i>   three files of different lengths, each enhanced ALONE
                         sd:<key>                     the Snake parameters of the state dict (alpha, beta)
                         self_db                      SI-SDR of the reference in fp32 against the reference in float64 on the batch
    snake_fp64_ref_error.json   max |Activation1d in fp32 - float64 restatement| / max |restatement| over the cases of
                       tests/snake_fp64.py, per case and overall, and max |Activation1d in float64 - restatement| likewise
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ref_import as R  # noqa: E402
import snake_cases as K  # noqa: E402
import snake_fp64 as F  # noqa: E402
from helpers import synth_mix  # noqa: E402
from make_golden import enhance_with_noise  # noqa: E402
from restatement import si_sdr  # noqa: E402

TILE = 512  # ou_snake_tile() of the library the figures were recorded for (the test checks that it still is)


def reference_model(case):
    ov = {}
    for k, v in K.overrides(case).items():
        ov[k] = v
        if k in K.BASE:
            ov[k.replace("score_model", "condition_model")] = v
    m, _ = R.build_reference_model("default", ov)
    sd = K.state_dict_of(case)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("loss_") for k in missing), (missing, unexpected)
    if m.ema is not None:
        m.ema.shadow_params = [p.clone().detach() for p in m.model_parameters()]
    return m.eval(), sd


def make_models():
    for case in K.CASES:
        m, sd = reference_model(case)
        spec = K.spec_of(case)
        out = {}
        T = K.batch_length(spec)
        Tp = T + (spec.tot_ds - T % spec.tot_ds)
        mix = synth_mix(spec, K.B, T)
        nz = K.noise_planes(K.NOISE_SEED, K.N_STEPS, K.B, Tp)
        out["mix"], out["noise"] = mix.numpy(), torch.stack(nz).numpy()
        out["enh"] = enhance_with_noise(m, mix, nz, n_steps=K.N_STEPS).numpy()
        nzw = K.noise_planes(K.NOISE_SEED + 100, K.N_STEPS - 1, K.B, Tp)
        out["noise_warm"] = torch.stack(nzw).numpy()
        out["enh_warm"] = enhance_with_noise(m, mix, nzw, n_steps=K.N_STEPS, warm_start=1).numpy()
        for i, L in enumerate(K.FILE_LENGTHS):
            Lp = L + (spec.tot_ds - L % spec.tot_ds)
            mf = synth_mix(spec, 1, L, seed=2000 + i)
            nf = K.noise_planes(K.NOISE_SEED + 1 + i, K.N_STEPS, 1, Lp)
            out[f"mix_f{i}"], out[f"noise_f{i}"] = mf.numpy(), torch.stack(nf).numpy()
            out[f"enh_f{i}"] = enhance_with_noise(m, mf, nf, n_steps=K.N_STEPS).numpy()
        for k, v in sd.items():
            if k.endswith(".prelu.act.act.alpha") or k.endswith(".prelu.act.act.beta"):
                out["sd:" + k] = v.numpy()
        # the reference's own agreement on these weights, fp32 against float64: what the 60 dB floor of the tests has to clear
        e64 = enhance_with_noise(m.double(), mix.double(), [z.double() for z in nz], n_steps=K.N_STEPS)
        out["self_db"] = float(si_sdr(e64.float(), torch.from_numpy(out["enh"])))
        assert out["self_db"] > 80.0, (case, out["self_db"])
        np.savez_compressed(K.golden_path(case), **out)
        print(case, "self_db %.1f" % out["self_db"], {k: getattr(v, "shape", v) for k, v in out.items() if not k.startswith("sd:")},
              sum(1 for k in out if k.startswith("sd:")), "snake tensors", os.path.getsize(K.golden_path(case)), "bytes")


def make_ref_error():
    per_case, worst32, worst64 = {}, 0.0, 0.0
    for tag, T, C, B, beta, lens in F.cases(TILE):
        x, la, lb = F.case_input(T, C, B, beta)
        # the reference in float64 against the restatement on the parameters float64 sees ...
        r64 = F.rel_error(F.reference_output(x, la, lb, lens, torch.float64), F.snake_act(x, F.f64_of_logs(la), F.f64_of_logs(lb), lens))
        # ... and in fp32 against the restatement of the function the fp32 parameters define (what the kernel is held to)
        ref = F.snake_act(x, F.exp32(la), F.exp32(lb), lens)
        r32 = F.rel_error(F.reference_output(x, la, lb, lens, torch.float32), ref)
        per_case[tag] = {"ref_fp32": r32, "ref_fp64": r64}
        worst32, worst64 = max(worst32, r32), max(worst64, r64)
    with open(F.REF_ERROR_JSON, "w") as f:
        json.dump({"tile": TILE, "max_rel": worst32, "max_rel_fp64": worst64, "cases": per_case}, f, indent=1, sort_keys=True)
    print("reference fp32 vs float64 restatement: max rel", worst32, "; reference float64 vs restatement:", worst64)


if __name__ == "__main__":
    torch.set_num_threads(8)
    what = set(sys.argv[1:]) or {"models", "ref_error"}
    if "ref_error" in what:
        make_ref_error()
    if "models" in what:
        make_models()
