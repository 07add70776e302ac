"""GPU (-m gpu): the level normalisation modes (normalization_norm max | 2-max, zero_mean false) on the small models.

1. the statistics (mean removed, gain) of pad_normalize_kernel, pad_normalize_var_kernel and the segmented statistics, row by row
   against the float64 restatement of utils/norm.py (tests/norm_cases.py) within the bound derived there, the maximum itself
   bit for bit -- in one reduce block and in several;
2. enhance, enhance_many and warm_start = 1 against recordings of the REAL reference (tests/golden/norm_*.npz) at the project's
   60 dB, printed beside the reference's own fp32-vs-float64 figure;
3. enhance_long of a file that fits one window is enhance, bit for bit;
4. enhance_long over several windows against the whole-file call; per-window statistics fail the same gate;
5. the ensemble entry points equal their member-by-member computation;
6. a norm 2 model is what it was: output, launches and blob of a model whose spec never mentions the new fields."""
import ctypes
import dataclasses
import json
import math

import numpy as np
import pytest
import torch
import yaml

import norm_cases as K
import restatement as O
from helpers import get_spec, record, synth_mix
from open_universe_amd import _lib
from open_universe_amd import inference_utils
from open_universe_amd import state_dict as S
from open_universe_amd import universe as U
from test_gpu_ensemble import _members_by_enhance, _share

pytestmark = pytest.mark.gpu

_models = {}
NORM_OF = {mode: K.MODE_ARGS[mode][:2] for mode in K.MODES}


def get_model(model, mode, tmp_path_factory):
    """Through load_model, from a config.yaml + checkpoint, as a user's model comes in."""
    if (model, mode) not in _models:
        d = tmp_path_factory.mktemp(f"norm_{model}_{mode}")
        with open(d / "config.yaml", "w") as f:
            yaml.safe_dump(K.config_of(model, mode), f)
        torch.save({"state_dict": K.state_dict_of(model, mode)}, d / "weights.ckpt")
        _models[(model, mode)] = inference_utils.load_model(d / "weights.ckpt", device="cuda:0")
    return _models[(model, mode)]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _enhance(model, mix, noise, **kw):
    a = dict(n_steps=K.N_STEPS, warm_start=None, keep_rms=False, t_raw=None)
    a.update(kw)
    extra = {} if a["t_raw"] is None else {"t_raw": a["t_raw"]}
    return model._enhance(mix.cuda(), a["n_steps"], None, None, None, None, False, a["keep_rms"], None, "median", a["warm_start"],
                          noise.cuda(), **extra).cpu()


# ---- 1. statistics -----------------------------------------------------------------------------------------------------------
def _variants(spec, T, edge):
    """Rows of T samples: the spike at the first sample, at the last, past `edge` (a block edge of the reduction); an all-zero
    row (both norms clamped); a smooth row on a large DC offset (what zero_mean false leaves in)."""
    base = synth_mix(spec, 1, T, seed=77)[0] + K.DC
    amp = K.SPIKE * float(base.double().std()) if T > 3 else 1.0
    rows = []
    for at in (0, T - 1, min(T - 1, edge)):
        r = base.clone()
        r[at] = amp
        rows.append(r)
    rows.append(torch.zeros(T))
    rows.append(base + 0.3)
    return rows


def _hold_stats(tag, stats, rows, t_pad, spec, mode):
    """stats: (n, 4) of the device; rows: the raw rows; t_pad: each row's padded length; mode: a key of norm_cases.MODES or
    (norm, zero_mean).  The clamp of the 2-max branch is the spec's normalization_kwargs.eps."""
    norm, zero_mean = NORM_OF.get(mode, mode)
    eps = float(spec.norm_eps)
    td = spec.tot_ds
    for i, (x, Tp) in enumerate(zip(rows, t_pad)):
        xp = K.padded(x, td)
        assert xp.numel() == Tp
        st = K.norm_stats(xp, norm, spec.level_db, zero_mean, eps)
        b_mean, rho = K.stats_bounds(xp, st, norm, zero_mean)
        mean_g, gain_g = float(stats[i, 0]), float(stats[i, 1])
        err_m, err_g = abs(mean_g - st["mean"]), abs(gain_g / st["gain"] - 1.0)
        print(f"{tag} row {i}: mean {mean_g:.9g} (f64 {st['mean']:.9g}, err {err_m:.2e} of {b_mean:.2e}); 1/gain {1 / gain_g:.9g} "
              f"(f64 {1 / st['gain']:.9g}, rel {err_g:.2e} of {rho + K.U:.2e}); branch {st['branch']}")
        assert err_m <= b_mean, (tag, i, "mean")
        assert err_g <= rho + K.U, (tag, i, "gain")  # (+ u: the final rounding of the stored gain)
        assert float(stats[i, 2]) == pytest.approx(math.sqrt(float(x.double().square().mean())), rel=4 * K.U, abs=0.0) or not x.any()
        assert float(stats[i, 3]) == 0.0
        if norm != "2":
            # the maximum, bit for bit: where it sets the gain, the gain is fl(level / mx) (resp. fl(1 / mx)) of exactly that fp32
            mx = K.exact_max(x, Tp, np.float32(mean_g) if zero_mean else np.float32(0))
            if norm == "max":
                assert np.float32(gain_g) == K.gain32("max", spec.level_db, 0.0, mx), (tag, i, "max is not exact")
            elif st["branch"] == "max" and st["mx"] > eps:
                assert np.float32(gain_g) == np.float32(1) / mx, (tag, i, "max is not exact")


@pytest.mark.parametrize("mode", list(K.MODES))
@pytest.mark.parametrize("length", ["1", "td-1", "td", "td+1", "2^18-3"])
def test_statistics_pad_normalize(mode, length, tmp_path_factory):
    """pad_normalize_kernel: its register path (up to 65 536 samples) and its loops (2^18 - 3)."""
    model = get_model("PP16s", mode, tmp_path_factory)
    spec = model.spec
    td = spec.tot_ds
    T = {"1": 1, "td-1": td - 1, "td": td, "td+1": td + 1, "2^18-3": 2 ** 18 - 3}[length]
    rows = _variants(spec, T, 1024 + 5)
    Tp = T + (td - T % td)
    mix = torch.stack(rows)
    _enhance(model, mix, torch.stack(K.noise_planes(3, 2, len(rows), Tp)), n_steps=2)
    stats = model.tensor("stats").cpu().clone()[:, :, 0]
    _hold_stats(f"pad_normalize.{mode}.T{T}", stats, rows, [Tp] * len(rows), spec, mode)
    if T > 60000:
        model.reset_workspace()


@pytest.mark.parametrize("mode", list(K.MODES))
def test_statistics_pad_normalize_var(mode, tmp_path_factory):
    """pad_normalize_var_kernel: one ragged call whose rows have the five lengths, every variant of each length in turn."""
    model = get_model("PP16s", mode, tmp_path_factory)
    spec = model.spec
    td = spec.tot_ds
    lengths = [2 ** 18 - 3, td + 1, td, td - 1, 1]
    per_len = [_variants(spec, T, 1024 + 5) for T in lengths]
    lm = max(lengths)
    Tm = lm + (td - lm % td)
    for v in range(5):
        rows = [per_len[j][(v + j) % 5] for j in range(len(lengths))]
        mix = torch.stack([torch.nn.functional.pad(r, (0, lm - r.numel())) for r in rows])
        nz = torch.zeros(2, len(rows), 1, Tm)
        for b, n in enumerate(lengths):
            nz[:, b, 0, :n + (td - n % td)] = 1.0
        nz *= torch.stack(K.noise_planes(5 + v, 2, len(rows), Tm))
        _enhance(model, mix, nz, n_steps=2, t_raw=list(lengths))
        stats = model.tensor("stats").cpu().clone()[:, :, 0]
        _hold_stats(f"pad_normalize_var.{mode}.v{v}", stats, rows, [n + (td - n % td) for n in lengths], spec, mode)
    model.reset_workspace()


@pytest.mark.parametrize("mode", list(K.MODES))
@pytest.mark.parametrize("T", [2 ** 18 + 5, 2 ** 18 * 3 + 1])
def test_statistics_segmented(mode, T, tmp_path_factory):
    """seg_stats1 / seg_stats2 / seg_stats_finish over 2 and 4 reduce blocks (one block holds up to 2^18 samples): the maximum of the
    block maxima is the exact maximum whatever the number of blocks."""
    model = get_model("PP16s", mode, tmp_path_factory)
    spec = model.spec
    td = spec.tot_ds
    rows = _variants(spec, T, 2 ** 18 + 2)  # (the third spike: in the second reduce block's share)
    x = torch.stack(rows).cuda()
    model.enhance_long(x, segment_s=200 * td / spec.fs * 8, overlap_s=16 * td / spec.fs, max_batch=8, n_steps=2, rng=_gen(2))
    stats = model.tensor("seg.stats").cpu().clone()[:len(rows), :, 0]
    Tp = T + (td - T % td)
    _hold_stats(f"segmented.{mode}.T{T}", stats, rows, [Tp] * len(rows), spec, mode)
    model._seg_ws = None


def test_segment_workspace_holds_the_block_maxima_for_every_mode(tmp_path_factory):
    """seg_stats2_kernel stores one maximum per reduce block behind the [C][nb][3] sums for every mode but (norm 2, zero_mean) --
    zero_mean false under norm 2 included, which never reads it -- and nb reaches 1024 for rows of 768 * 2^18 samples and more,
    too long to run here.  So the sizer is held instead: its answer is the same for every mode (nothing depends on when
    ou_set_normalization is called) and leaves room, behind the walk, for the stats, the row scales, the four partials of 1024
    blocks and the two window planes -- at the row length where all 1024 blocks are in use."""
    C, S, Ov, mb = 3, 4096, 512, 4
    T = 2 ** 28 + 7  # seg_nb = 1024
    need = {}
    for mode in (None,) + tuple(K.MODES):
        if mode is None:
            from test_gpu_parity import get_model as plain_model
            model = plain_model("PP16s")[0]
        else:
            model = get_model("PP16s", mode, tmp_path_factory)
        L = model._L
        n, B, Ln, walk = ctypes.c_size_t(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_size_t()
        _lib.check(L.ou_segments_workspace_bytes(model._handle, C, T, S, Ov, mb, ctypes.byref(n), ctypes.byref(B), ctypes.byref(Ln)),
                   model._handle)
        _lib.check(L.ou_workspace_bytes(model._handle, B.value, Ln.value, ctypes.byref(walk)), model._handle)
        need[mode] = (n.value, walk.value, B.value, Ln.value)
    assert len(set(need.values())) == 1, need
    n, walk, B, Ln = need[None]
    assert n >= walk + C * 16 + C * 4 + C * 4 * 1024 * 8 + B * Ln * 4 + Ln * 4


# ---- 2. parity with the reference ---------------------------------------------------------------------------------------------
def _parity(name, ref, out, self_db):
    v = O.si_sdr(ref, out)
    print(f"{name}: SI-SDR {float(v):.2f} dB, SNR {float(getattr(v, 'snr', float('nan'))):.2f} dB; the reference fp32 vs float64: "
          f"{self_db:.1f} dB")
    return record(name, v)


@pytest.mark.parametrize("model_name,mode", K.CASES)
def test_enhance_vs_reference_golden(model_name, mode, tmp_path_factory):
    gold = K.load_golden(model_name, mode)
    model = get_model(model_name, mode, tmp_path_factory)
    assert (model.spec.norm, model.spec.zero_mean) == NORM_OF[mode]
    plan = json.loads(model._L.ou_plan_json(model._handle).decode())
    assert (plan["norm"], plan["zero_mean"]) == (NORM_OF[mode][0], int(NORM_OF[mode][1]))
    assert np.float32(plan["norm_eps"]) == np.float32(K.MODE_ARGS[mode][2]) and model.spec.norm_eps == K.MODE_ARGS[mode][2]
    self_db = float(gold["self_db"])
    mix = torch.from_numpy(gold["mix"])
    out = _enhance(model, mix, torch.from_numpy(gold["noise"]))
    ref = torch.from_numpy(gold["enh"])
    assert out.shape == ref.shape and torch.isfinite(out).all()
    _parity(f"norm.{model_name}.{mode}.plain", ref, out, self_db)
    # the statistics the reference recorded: (mean, std = 1 / gain)
    stats = model.tensor("stats").cpu()[:, :, 0]
    assert torch.allclose(stats[:, 0], torch.from_numpy(gold["norm_mean"]), rtol=1e-5, atol=1e-8)
    assert torch.allclose(1.0 / stats[:, 1], torch.from_numpy(gold["norm_std"]), rtol=1e-5, atol=0.0)
    if model_name == "PP16s":
        out = _enhance(model, mix, torch.from_numpy(gold["noise_warm"]), warm_start=1)
        _parity(f"norm.{model_name}.{mode}.warm", torch.from_numpy(gold["enh_warm"]), out, self_db)


@pytest.mark.parametrize("model_name,mode", K.CASES)
def test_ragged_enhance_many_vs_per_file_goldens(model_name, mode, tmp_path_factory, monkeypatch):
    """ONE enhance_many call over three files of different lengths (ou_enhance_var) against the reference run on every file alone."""
    gold = K.load_golden(model_name, mode)
    model = get_model(model_name, mode, tmp_path_factory)
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
        _parity(f"norm.{model_name}.{mode}.many.file{i}", ref, o.cpu(), float(gold["self_db"]))


# ---- 3. one window covering the file -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["max", "2max"])
def test_enhance_long_of_one_window_is_enhance(mode, tmp_path_factory):
    model = get_model("PP16s", mode, tmp_path_factory)
    x = K.batch_mix(model.spec).cuda()
    a = model.enhance(x, n_steps=K.N_STEPS, rng=_gen(5), keep_rms=True)
    b = model.enhance_long(x, n_steps=K.N_STEPS, rng=_gen(5), keep_rms=True)
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- 4. several windows ---------------------------------------------------------------------------------------------------------
# SI-SDR in dB of enhance_long (4 windows of 2 s over 7 s, 2 rows, max_batch 3) against the whole-file call on the same noise,
# measured on an MI355X: the spiked input under max / 2-max, and the norm 2 model on the same input beside them.
# The gate is the measured figure less 6 dB, the margin DESIGN 4.9 gives its own gates for the spread from box to box.
MEASURED_GAP_DB = {"max": 67.26, "2max": 67.26, "2": 67.26}
SEG = dict(segment_s=2.0, overlap_s=0.32, max_batch=3)


def _long_input(spec):
    T = 7 * spec.fs
    x = synth_mix(spec, 2, T, seed=31) + K.DC
    for r in range(2):
        x[r, 1000 + 17 * r] = K.SPIKE * float(x[r].double().std())  # window 0 only
    return x.cuda()


def _gap(model, x, keep_rms=False):
    spec = model.spec
    starts = _lib.segment_plan(spec.tot_ds, x.shape[-1], int(SEG["segment_s"] * spec.fs), int(SEG["overlap_s"] * spec.fs))["starts"]
    assert len(starts) == 4
    whole = model.enhance(x, n_steps=K.N_STEPS, rng=_gen(9), keep_rms=keep_rms)
    y = model.enhance_long(x, n_steps=K.N_STEPS, rng=_gen(9), keep_rms=keep_rms, **SEG)
    return whole, y, min(float(O.si_sdr(whole[r].cpu(), y[r].cpu())) for r in range(x.shape[0]))


def test_segmented_gap_of_the_norm_2_model_at_the_same_shape():
    from test_gpu_parity import get_model as plain_model

    model, spec, _ = plain_model("PP16s")
    _, _, fig = _gap(model, _long_input(spec))
    print(f"segmented vs whole, norm 2: {fig:.2f} dB (recorded {MEASURED_GAP_DB['2']})")
    assert fig >= MEASURED_GAP_DB["2"] - 6.0


@pytest.mark.parametrize("mode", ["max", "2max"])
def test_segmented_with_whole_file_statistics(mode, tmp_path_factory):
    model = get_model("PP16s", mode, tmp_path_factory)
    spec = model.spec
    x = _long_input(spec)
    whole, y, fig = _gap(model, x)
    print(f"segmented vs whole, {mode}: {fig:.2f} dB (recorded {MEASURED_GAP_DB[mode]})")
    # test-only computation with PER-WINDOW statistics: every 2 s piece enhanced as a file of its own on its slice of the same
    # noise, concatenated -- only the first piece holds the spike, so the others come out at another level
    T = x.shape[-1]
    n = 2 * spec.fs
    noise = model.draw_noise_like_enhance(_gen(9), 2, T, K.N_STEPS)
    pad_left = (spec.tot_ds - T % spec.tot_ds) // 2
    parts = []
    for s in range(0, T, n):
        xs = x[:, s:s + n]
        Tp = xs.shape[-1] + (spec.tot_ds - xs.shape[-1] % spec.tot_ds)
        nz = noise[:, :, pad_left + s: pad_left + s + Tp]
        nz = torch.nn.functional.pad(nz, (0, Tp - nz.shape[-1]))
        parts.append(model._enhance(xs[:, None, :].contiguous(), K.N_STEPS, None, None, None, None, False, False, None, "median", None,
                                    nz[:, :, None, :].contiguous())[:, 0])
    pw = torch.cat(parts, dim=-1)
    fig_pw = min(float(O.si_sdr(whole[r].cpu(), pw[r].cpu())) for r in range(2))
    print(f"per-window statistics vs whole, {mode}: {fig_pw:.2f} dB")
    gate = MEASURED_GAP_DB[mode] - 6.0
    assert fig >= gate
    assert fig_pw < gate


# ---- 5. ensembles ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["max", "2max"])
def test_ensemble_is_its_members(mode, tmp_path_factory):
    """enhance_ensemble(E = 3, median) with the conditioner unshared is enhance on the replicated batch bit for bit, and the result
    is enhance(ensemble = 3); with the shared conditioner (the default) the members stay within fp32 round-off of those."""
    model = get_model("PP16s", mode, tmp_path_factory)
    mix = K.batch_mix(model.spec).cuda()
    want = _members_by_enhance(model, mix, 3, _gen(21), n_steps=K.N_STEPS)
    with _share(model, 0):
        out, mem = model.enhance_ensemble(mix, 3, "median", n_steps=K.N_STEPS, rng=_gen(21), return_members=True)
    assert torch.equal(mem, want)
    assert torch.equal(out, model.enhance(mix, n_steps=K.N_STEPS, rng=_gen(21), ensemble=3, ensemble_stat="median"))
    out_s, mem_s = model.enhance_ensemble(mix, 3, "median", n_steps=K.N_STEPS, rng=_gen(21), return_members=True)
    fig = min(float(O.si_sdr(want[e, b].cpu(), mem_s[e, b].cpu())) for e in range(3) for b in range(2))
    print(f"ensemble.{mode}: shared-conditioner members vs enhance on the replicated batch {fig:.1f} dB")
    assert fig >= 100.0  # the gate of tests/test_gpu_ensemble.py's shared path: fp32 round-off between kernel selections


@pytest.mark.parametrize("mode", ["max", "2max"])
def test_long_ensemble_members_are_their_rows_alone(mode, tmp_path_factory):
    """enhance_long_ensemble: member e of row c is enhance_long of row c alone on that member's noise (gate: the 100 dB of
    tests/test_gpu_segments_ensemble.py), and the result is the median of the members bit for bit."""
    model = get_model("PP16s", mode, tmp_path_factory)
    spec = model.spec
    td = spec.tot_ds
    Sg, Ov, T, E, C = 16 * td, 2 * td, 40 * td + 3, 3, 2
    x = synth_mix(spec, C, T, seed=2400) + K.DC
    x[1, 5] = K.SPIKE * float(x[1].double().std())
    x = x.cuda()
    kw = dict(segment_s=Sg / spec.fs, overlap_s=Ov / spec.fs, n_steps=K.N_STEPS)
    out, mem = model.enhance_long_ensemble(x, E, "median", rng=_gen(300), return_members=True, max_batch=6, **kw)
    noise = model.draw_noise_like_enhance(_gen(300), E * C, T, K.N_STEPS)
    rows = mem.reshape(E * C, -1)
    figs = []
    for r in range(E * C):
        alone = model._segments_call(x[r % C][None, :].contiguous(), Sg, Ov, 4, K.N_STEPS, model.diff_kwargs.epsilon, False,
                                     noise[:, r:r + 1].contiguous(), None)[0]
        figs.append(float(O.si_sdr(alone.cpu(), rows[r].cpu())))
    print(f"long ensemble.{mode}: worst member vs its row alone {min(figs):.1f} dB")
    assert min(figs) >= 100.0
    assert torch.equal(out, U.ensemble_reduce(mem.contiguous(), "median"))


# ---- 6. the default is untouched -------------------------------------------------------------------------------------------------
def test_norm_2_model_is_what_it_was():
    spec = get_spec("PP16s")
    assert (spec.norm, spec.zero_mean, spec.norm_eps) == ("2", True, 1e-5)
    new = ("norm", "zero_mean", "norm_eps")
    # a spec as code from before the fields existed builds it: the constructor call names none of them
    old = type(spec)(**{f.name: getattr(spec, f.name) for f in dataclasses.fields(spec) if f.init and f.name not in new})
    sd = S.synthetic_state_dict(spec, seed=0)
    a = U.UniverseGAN(spec, state_dict=sd, device="cuda:0")
    b = U.UniverseGAN(old, state_dict=sd, device="cuda:0")
    assert torch.equal(a._weights, b._weights) and bytes(a._cfg) == bytes(b._cfg)
    B, T = 2, spec.tot_ds * 9 + 11
    mix = synth_mix(spec, B, T) + K.DC
    nz = torch.stack(K.noise_planes(3, K.N_STEPS, B, T + (spec.tot_ds - T % spec.tot_ds)))
    ya = _enhance(a, mix, nz, keep_rms=True)
    na = a.launch_stats()
    yb = _enhance(b, mix, nz, keep_rms=True)
    assert torch.equal(ya, yb) and a.launch_stats() == na == b.launch_stats()
    assert json.loads(a._L.ou_plan_json(a._handle).decode())["norm"] == "2"
    # and a model of another mode in the process does not reach it
    ym = _enhance(U.UniverseGAN(K.spec_of("PP16s", "max"), state_dict=sd, device="cuda:0"), mix, nz, keep_rms=True)
    assert not torch.equal(ym, ya)
    assert torch.equal(_enhance(a, mix, nz, keep_rms=True), ya)
