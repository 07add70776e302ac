"""
Golden vectors of the REAL reference for score networks with a conv sandwich round the GRU (encoder_gru_conv_sandwich) or with no
GRU (seq_model: none) -- score.py:32-36, 81-102, 113-123.  Needs the reference checkout (oracle/ref_import.py); run on a CPU:

    python tests/golden/make_golden_seqmodel.py

Writes
    seqmodel_<case>.npz   per case of tests/seqmodel_cases.py (seeded synthetic weights, loaded with strict=False; the weights
                          themselves are not stored), 3 steps, fixed seeds:
                            mix, noise, enh              a batch of two rows of a ragged length (T % tot_ds != 0)
                            noise_warm, enh_warm         the same batch with warm_start = 1 (UNIVERSE++ cases: the original UNIVERSE
                                                         has no aux signal to start from)
                            mix_f<i>, noise_f<i>, enh_f<i>   three files of different lengths, each enhanced ALONE
                            self_db                      SI-SDR of the reference in fp32 against the reference in float64 on the batch
    seqmodel_names.json   per case: the reference's state_dict() key order and model_parameters() name order of the score network

    python tests/golden/make_golden_seqmodel.py parent_pack      (in a checkout of the commit BEFORE this feature, library built)

writes seqmodel_parent_pack.json: for PP16 / OR16 / PP24 at n_channels 8, seeded weights 0, that commit's ou_config bytes and the
SHA-256 of its packed blob and of its plan text -- what "the shipped models keep blob and plan bit for bit" is held against.  It
needs neither the reference nor tests/seqmodel_cases.py.
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

if "parent_pack" not in sys.argv[1:]:
    import ref_import as R  # noqa: E402
    import seqmodel_cases as K  # noqa: E402
    from helpers import synth_mix  # noqa: E402
    from make_golden import enhance_with_noise  # noqa: E402
    from restatement import si_sdr  # noqa: E402

FLOOR = 60.0  # the project's end-to-end floor (helpers.record): every case's self_db has to clear it


def reference_model(case):
    m, _ = R.build_reference_model(K.REFERENCE_YAML[K.CASES[case][0]], K.reference_overrides(case))
    sd = K.state_dict_of(case)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("loss_") for k in missing), (missing, unexpected)
    if m.ema is not None:
        m.ema.shadow_params = [p.clone().detach() for p in m.model_parameters()]
    return m.eval(), sd


def names_of(m, prefix):
    """state_dict() keys and model_parameters() names of the score network, in the reference's own order."""
    keys = [k for k in m.state_dict() if k.startswith(prefix + ".")]
    by_id = {id(p): n for n, p in m.named_parameters()}
    params = [by_id[id(p)] for p in m.model_parameters()]
    return keys, [n for n in params if n.startswith(prefix + ".")]


def parent_pack():
    import hashlib

    from open_universe_amd import _lib
    from open_universe_amd import config as C
    from open_universe_amd import state_dict as S

    out = {}
    for name in ("PP16", "OR16", "PP24"):
        spec = C.spec_from_config(C.builtin_config(name, **{"score_model.n_channels": 8}))
        blob, plan = _lib.pack_weights(spec, S.synthetic_state_dict(spec, seed=0))
        out[name] = {"blob_sha256": hashlib.sha256(blob.numpy().tobytes()).hexdigest(),
                     "plan_sha256": hashlib.sha256(plan.encode()).hexdigest(), "config_hex": bytes(_lib.make_config(spec)).hex()}
    with open(os.path.join(HERE, "seqmodel_parent_pack.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


def main():
    names = {}
    for case in K.CASES:
        m, sd = reference_model(case)
        spec = K.spec_of(case)
        keys, params = names_of(m, spec.score_prefix)
        names[case] = {"state_dict": keys, "parameters": params}
        out = {}
        T = K.batch_length(spec)
        Tp = T + (spec.tot_ds - T % spec.tot_ds)
        mix = synth_mix(spec, K.B, T)
        nz = K.noise_planes(K.NOISE_SEED, K.N_STEPS, K.B, Tp)
        out["mix"], out["noise"] = mix.numpy(), torch.stack(nz).numpy()
        out["enh"] = enhance_with_noise(m, mix, nz, n_steps=K.N_STEPS).numpy()
        if spec.use_signal_decoupling:
            nzw = K.noise_planes(K.NOISE_SEED + 100, K.N_STEPS - 1, K.B, Tp)
            out["noise_warm"] = torch.stack(nzw).numpy()
            out["enh_warm"] = enhance_with_noise(m, mix, nzw, n_steps=K.N_STEPS, warm_start=1).numpy()
        for i, L in enumerate(K.FILE_LENGTHS):
            Lp = L + (spec.tot_ds - L % spec.tot_ds)
            mf = synth_mix(spec, 1, L, seed=2000 + i)
            nf = K.noise_planes(K.NOISE_SEED + 1 + i, K.N_STEPS, 1, Lp)
            out[f"mix_f{i}"], out[f"noise_f{i}"] = mf.numpy(), torch.stack(nf).numpy()
            out[f"enh_f{i}"] = enhance_with_noise(m, mf, nf, n_steps=K.N_STEPS).numpy()
        # the reference's own agreement on these weights, fp32 against float64: what the 60 dB floor of the tests has to clear
        e64 = enhance_with_noise(m.double(), mix.double(), [z.double() for z in nz], n_steps=K.N_STEPS)
        out["self_db"] = float(si_sdr(e64.float(), torch.from_numpy(out["enh"])))
        assert out["self_db"] > FLOOR, (case, out["self_db"], "change the case's seed or step count, not the floor")
        np.savez_compressed(K.golden_path(case), **out)
        print(case, "self_db %.1f" % out["self_db"], {k: getattr(v, "shape", v) for k, v in out.items()},
              os.path.getsize(K.golden_path(case)), "bytes")
    with open(K.NAMES_JSON, "w") as f:
        json.dump(names, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    torch.set_num_threads(8)
    if "parent_pack" in sys.argv[1:]:
        parent_pack()
    else:
        main()
