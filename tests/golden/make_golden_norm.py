"""
Golden vectors of the REAL reference for models with another level normalisation than every shipped config's
(normalization_norm max | 2-max, normalization_kwargs.zero_mean false, normalization_kwargs.eps: utils/norm.py:22-87).  Needs
the reference checkout (oracle/ref_import.py); run on a CPU, no GPU test uses this script:

    python tests/golden/make_golden_norm.py [mode ...]      (no mode: every mode of tests/norm_cases.py)

Writes norm_<model>_<mode>.npz per case of tests/norm_cases.py (PP16s and OR16s x max | 2max | keepmean | max_keepmean |
2max_keepmean | 2max_eps; seeded synthetic weights), 3 steps, fixed noise planes:
    mix, noise, enh                  a batch of two rows of a ragged length (T % tot_ds != 0) on a DC offset: row 0 smooth (2-max
                                     takes its std branch), row 1 with one spike of crest factor > 1 / level (its max branch);
                                     2max_eps (eps = 1e-3): a third, quiet row (sd about 1e-4, maximum about 4e-4) whose gain
                                     the key decides -- level / eps where eps = 1e-5 would give 1 / mx
    norm_mean, norm_std              what the reference's normalize_batch returns for the padded batch (mean, 1 / gain)
    noise_warm, enh_warm             PP16s: the same batch with warm_start = 1
    mix_f<i>, noise_f<i>, enh_f<i>, norm_mean_f<i>, norm_std_f<i>    three files of different lengths, each enhanced ALONE
    self_db                          SI-SDR of the reference in fp32 against the reference in float64 on the batch
The quiet row stays in the 2max_eps batch: on it too the reference agrees with its own float64 evaluation well above the 60 dB
floor of the tests (asserted row by row below; printed).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import norm_cases as K  # noqa: E402
import ref_import as R  # noqa: E402
from helpers import SMALL  # noqa: E402
from make_golden import REF_CFG, enhance_with_noise  # noqa: E402
from restatement import si_sdr  # noqa: E402


def reference_model(model, mode):
    ov = {}
    for k, v in K.overrides(model, mode).items():
        ov[k] = v
        if k.startswith("score_model."):
            ov[k.replace("score_model", "condition_model")] = v
    m, _ = R.build_reference_model(REF_CFG[SMALL[model][0]], ov)
    sd = K.state_dict_of(model, mode)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("loss_") for k in missing), (missing, unexpected)
    if m.ema is not None:
        m.ema.shadow_params = [p.clone().detach() for p in m.model_parameters()]
    return m.eval()


def reference_stats(m, mix):
    """The reference's own (mean, std = 1 / gain) of the padded batch (universe.py:268-272)."""
    with torch.no_grad():
        mp, _ = m.pad(mix[:, None, :])
        _, mean, std = m.normalize_batch((mp, None))
    mean = mean if torch.is_tensor(mean) else torch.full((mix.shape[0], 1, 1), float(mean))
    return mean.reshape(-1).numpy().astype(np.float32), std.reshape(-1).numpy().astype(np.float32)


def main(modes=()):
    for model, mode in K.CASES:
        if modes and mode not in modes:
            continue
        m = reference_model(model, mode)
        spec = K.spec_of(model, mode)
        td = spec.tot_ds
        out = {}
        mix = K.batch_mix(spec, mode)
        rows = K.batch_rows(mode)
        assert mix.shape[0] == rows and (spec.norm, spec.zero_mean, spec.norm_eps) == K.MODE_ARGS[mode]
        T = mix.shape[-1]
        Tp = T + (td - T % td)
        # which branch of 2-max each row takes (float64): the smooth row its std, the spiked row its max
        for b, want in enumerate(("std", "max")):
            st = K.norm_stats(K.padded(mix[b], td), "2-max", spec.level_db)
            assert st["branch"] == want, (b, st)
            assert (st["mx"] / st["sd"] > K.crest_needed(spec.level_db)) == (want == "max")
        if mode == "2max_eps":  # the quiet row: both norms between 1e-5 and eps
            st = K.norm_stats(K.padded(mix[2], td), "2-max", spec.level_db, True, spec.norm_eps)
            assert 1e-5 < st["sd"] < st["mx"] < spec.norm_eps and st["gain"] == st["level"] / spec.norm_eps, st
        nz = K.noise_planes(K.NOISE_SEED, K.N_STEPS, rows, Tp)
        out["mix"], out["noise"] = mix.numpy(), torch.stack(nz).numpy()
        out["enh"] = enhance_with_noise(m, mix, nz, n_steps=K.N_STEPS).numpy()
        out["norm_mean"], out["norm_std"] = reference_stats(m, mix)
        if model == "PP16s":
            nzw = K.noise_planes(K.NOISE_SEED + 100, K.N_STEPS - 1, rows, Tp)
            out["noise_warm"] = torch.stack(nzw).numpy()
            out["enh_warm"] = enhance_with_noise(m, mix, nzw, n_steps=K.N_STEPS, warm_start=1).numpy()
        for i, L in enumerate(K.FILE_LENGTHS):
            Lp = L + (td - L % td)
            mf = K.file_mix(spec, i)
            nf = K.noise_planes(K.NOISE_SEED + 1 + i, K.N_STEPS, 1, Lp)
            out[f"mix_f{i}"], out[f"noise_f{i}"] = mf.numpy(), torch.stack(nf).numpy()
            out[f"enh_f{i}"] = enhance_with_noise(m, mf, nf, n_steps=K.N_STEPS).numpy()
            out[f"norm_mean_f{i}"], out[f"norm_std_f{i}"] = reference_stats(m, mf)
        # the reference's own agreement, fp32 against float64: what the 60 dB floor of the tests has to clear
        e64 = enhance_with_noise(m.double(), mix.double(), [z.double() for z in nz], n_steps=K.N_STEPS)
        out["self_db"] = float(si_sdr(e64.float(), torch.from_numpy(out["enh"])))
        assert out["self_db"] > 80.0, (model, mode, out["self_db"])
        per_row = [float(si_sdr(e64[b].float(), torch.from_numpy(out["enh"])[b])) for b in range(rows)]
        assert min(per_row) > 80.0, (model, mode, per_row)
        np.savez_compressed(K.golden_path(model, mode), **out)
        size = os.path.getsize(K.golden_path(model, mode))
        assert size < 1 << 20, size
        print(model, mode, "self_db %.1f" % out["self_db"], "per row", ["%.1f" % v for v in per_row], "std", out["norm_std"], "mean",
              out["norm_mean"], size, "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main(tuple(sys.argv[1:]))
