"""GPU (-m gpu): every launch shape of the GRU recurrence (gru_ring_kernel: four hidden sizes, both gather layouts, 8 / 16
units per workgroup, sub-launches of a batch that does not fit, the residual epilogue, per-row lengths held by
gru_tail_fill_kernel) and its input projection against the float64 reference of tests/gru_fp64.py, element by element:
every (row, direction, frame, unit) of a tap is held against float64, none is left out.

The layers are driven through the public seams (condition_model / score_model, a whole _enhance for the overlapped
schedule and for ragged batches) and isolated by reading the GPU's own intermediates: the reference gets the very gx plane
the kernel read and -- teacher-forced -- the kernel's own previous state.  Tolerances: gru_fp64's docstring (M x the fp32
torch evaluation's own error + 1/2 ulp).  Every case logs its err / e32 ratios to build/observed/gru_fp64_observed.json (untracked) before
it asserts; profiles/gru_fp64_observed.json is the committed copy the M values were taken from."""
import json
import os
import time

import pytest
import torch

import gru_fp64 as G
import restatement as O
from helpers import get_spec, synth_mix, varlen_lengths
from open_universe_amd import state_dict as S
from test_gpu_parity import get_model, noise_list, run_enhance

pytestmark = pytest.mark.gpu

_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed")
_layers = {}


def _log(case, reps, seconds):
    try:
        os.makedirs(_OUT, exist_ok=True)
        path = os.path.join(_OUT, "gru_fp64_observed.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[case] = {"seconds": round(seconds, 2), **{k: r.summary() for k, r in reps.items()}}
        for k, r in reps.items():
            if hasattr(r, "e32_explicit"):
                old[case][k].update(e32_explicit=r.e32_explicit, e32_aten=r.e32_aten)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _gru_layers(key, spec, sd):
    if key not in _layers:
        _layers[key] = (G.Layer(sd, "condition_model.encoder.gru", 0), G.Layer(sd, "condition_model.encoder.gru", 1),
                        G.Layer(sd, spec.score_prefix + ".encoder.gru", 0))
    return _layers[key]


def _tap(model, name):
    return model.tensor(name).cpu().clone()  # copied out before the next call re-uses the workspace


def _check_layer(reps, tag, L, x, gx, out, res, lens, ragged, free):
    reps[tag + ".proj"] = G.check_projection(L, x, gx, lens, ragged)
    reps[tag + ".step"] = G.check_step(L, gx, out, lens, res)
    if free:
        reps[tag + ".free"] = G.check_free(L, gx, out, lens, res)


def _check_taps(case, model, spec, layers, t0, lens=None, ragged=False, free=False, cond=True, score=True):
    """Read the GRU taps of the last call(s), check all of them, log, then assert."""
    reps = {}
    if cond:
        cb1, gx0, g0 = _tap(model, "cond.cb1.v"), _tap(model, "cond.gru0.gx"), _tap(model, "cond.gru0")
        gx1, g1 = _tap(model, "cond.gru.gx"), _tap(model, "cond.gru")
        _check_layer(reps, "cond.gru0", layers[0], cb1, gx0, g0, None, lens, ragged, free)
        _check_layer(reps, "cond.gru", layers[1], g0, gx1, g1, cb1 if spec.cond.encoder_gru_residual else None, lens, ragged, free)
    if score:
        last = len(spec.score.rate_factors) + int(spec.score.extra_conv_block) - 1
        # (with the extra conv block neither the last encoder block nor decoder block 0 changes the rate: the GRU reads the
        # block's output `.v` and the decoder's residual add is fused into the recurrence's epilogue)
        x = _tap(model, f"score.enc{last}.v" if spec.score.extra_conv_block else f"score.enc{last}.h")
        gx, out = _tap(model, "score.gru.gx"), _tap(model, "score.gru")
        _check_layer(reps, "score.gru", layers[2], x, gx, out, x if spec.score.extra_conv_block else None, lens, ragged, free)
    _log(case, reps, time.time() - t0)
    for k, r in reps.items():
        print(f"{case} {k} {r}")
    for k, r in reps.items():
        assert r.excluded == 0 and r.ok(), f"{case} {k} {r}"
        assert r.ratio <= G.M_CAP, f"{case} {k}: err / e32 = {r.ratio:.2f} is a finding, not a tolerance -- {r}"
    return reps


def _seams(case, name, B, frames, free=False, model_spec_sd=None, key=None, seed=0):
    """condition_model -> score_model on (B, frames) and the check of all three GRU layers."""
    t0 = time.time()
    model, spec, sd = model_spec_sd or get_model(name)
    T = spec.tot_ds * frames
    xin = O.normalize(synth_mix(spec, B, T, seed=1000 + seed)[:, None, :], spec.level_db)
    model.condition_model(xin.cuda(), train=True)
    sig = torch.tensor([0.3, 1.7, 0.05, 4.0] * ((B + 3) // 4))[:B]
    xs = torch.randn(xin.shape, generator=torch.Generator().manual_seed(5 + seed)) * sig[:, None, None]
    model.score_model(xs.cuda(), sig)
    return _check_taps(case, model, spec, _gru_layers(key or name, spec, sd), t0, free=free)


def _own_model(name, scale):
    """A model of the test's own whose GRU weights (weight_ih, weight_hh of every layer) are scaled."""
    from open_universe_amd import Universe, UniverseGAN

    spec = get_spec(name)
    sd = dict(S.synthetic_state_dict(spec, seed=0))
    for k in list(sd):
        if ".gru.weight_ih" in k or ".gru.weight_hh" in k:
            sd[k] = sd[k] * float(scale)
    cls = UniverseGAN if spec.kind == "universe_gan" else Universe
    return cls(spec, state_dict=sd, device="cuda:0", split_copy=False), spec, sd


@pytest.mark.parametrize("frames", [1, 2, 3, 37, 401])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", ["PP16s", "PP16m", "PP16", "OR16", "PP24"])
def test_every_hidden_size_default_dispatch(name, B, frames):
    """H = 64 / 128 / 256 / 384 as the launcher dispatches them; 1-3 frames: first / last frame of both directions."""
    _seams(f"sizes.{name}.b{B}.f{frames}", name, B, frames)


@pytest.mark.parametrize("frames", [3000, 12000])
@pytest.mark.parametrize("name", ["PP16", "PP24"])
def test_real_lengths(name, frames):
    """30 s and 120 s in one call: teacher-forced at both, free-running (accumulated drift) at 3 000 frames."""
    _seams(f"long.{name}.f{frames}", name, 1, frames, free=frames == 3000)
    get_model(name)[0].reset_workspace()  # (gigabytes at these lengths)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,upw", [(n, u) for n in ("PP16", "PP16m") for u in (0, 8, 16, 17)] + [("PP24", u) for u in (0, 16, 17)])
def test_gather_layouts_and_cluster_splits(name, upw, B, steer):
    """option gru_upw: wide layout with 16 / 8 units per workgroup, the round-2 layout (17), the launcher's choice (0) -- each
    against float64, not against each other."""
    steer.set(gru_upw=upw)
    model = get_model(name)[0]
    model.reset_workspace()
    try:
        _seams(f"layout.{name}.upw{upw}.b{B}", name, B, 401, seed=1)
    finally:
        model.reset_workspace()


@pytest.mark.parametrize("B", [5, 9])
def test_batches_off_the_xcd_grid(B):
    """2 B clusters that are not a multiple of the 8 XCDs."""
    _seams(f"offgrid.PP16.b{B}", "PP16", B, 100, seed=2)


@pytest.mark.parametrize("bmax", [1, 2, 3])
@pytest.mark.parametrize("name", ["PP16", "PP16m"])
def test_forced_sub_launches(name, bmax, steer):
    """option gru_bmax: the batch runs as sub-launches that share one exchange area (launch_gru, b0 += bmax); the first frame
    of every sub-launch is where a stale tag would show."""
    steer.set(gru_bmax=bmax)
    _seams(f"chunked.{name}.bmax{bmax}.b5", name, 5, 100, seed=3)


def test_natural_sub_launches():
    """What bench.py runs at B = 32: a batch beyond what one launch may carry.  At H = 256 with 16 units per workgroup on the
    256 CUs of an MI355X the launcher's cap (gru_ring_batch_cap) is 8 or 16 utterances -- one or two resident workgroups per
    CU, from the occupancy query; the library does not export it.  B = 33 is one more than twice the larger cap and one more
    than four times the smaller: at least three sub-launches, the last of a single utterance, either way."""
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256
    _seams("chunked.PP16.natural.b33", "PP16", 33, 100, seed=4)
    get_model("PP16")[0].reset_workspace()


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("name", ["PP16", "PP24"])
def test_overlapped_schedule(name, B):
    """A whole enhance: the conditioner's two GRU layers run beside the first score pass' (share = 2: other units per
    workgroup, half the batch cap).  Taps after the call: cond.* from that overlapped pass, score.gru from the last step."""
    t0 = time.time()
    model, spec, sd = get_model(name)
    model.reset_workspace()
    T = spec.tot_ds * 401 - 5
    mix = synth_mix(spec, B, T)
    run_enhance(model, mix, noise_list(71, 2, B, T + 5), n_steps=2)
    _check_taps(f"overlap.{name}.b{B}", model, spec, _gru_layers(name, spec, sd), t0)
    model.reset_workspace()


def _ragged(case, name, lens_samples):
    t0 = time.time()
    model, spec, sd = get_model(name)
    td = spec.tot_ds
    B, lm = len(lens_samples), max(lens_samples)
    T = lm + (td - lm % td)
    sigs = [synth_mix(spec, 1, n, seed=300 + i)[0] for i, n in enumerate(lens_samples)]
    mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs])[:, None, :]
    nz = torch.zeros(2, B, 1, T)
    for b, n in enumerate(lens_samples):
        tb = n + (td - n % td)
        nz[:, b, 0, :tb] = torch.randn(2, tb, generator=torch.Generator().manual_seed(900 + b))
    model._enhance(mix.cuda(), 2, None, None, None, None, False, False, None, "median", None, nz.cuda(), t_raw=list(lens_samples))
    frames = [(n + (td - n % td)) // td for n in lens_samples]
    _check_taps(case, model, spec, _gru_layers(name, spec, sd), t0, lens=frames, ragged=True)
    model.reset_workspace()
    return frames


@pytest.mark.parametrize("name", ["PP16", "PP24s"])
def test_ragged_rows(name):
    """Per-row lengths (ou_enhance_var): gx tail fill exact, outputs exactly zero behind a row's end, backward pass from the row's
    own last frame.  Rows of 1, 2, 250 and 401 frames; and the eight lengths of the variable-length benchmark batch."""
    td = get_spec(name).tot_ds
    assert _ragged(f"ragged.{name}.four", name, [td - 3, 2 * td - 3, 250 * td - 3, 401 * td - 3]) == [1, 2, 250, 401]
    _ragged(f"ragged.{name}.varlen8", name, varlen_lengths(get_spec(name).fs))


@pytest.mark.parametrize("scale", [2, 4, 8])
@pytest.mark.parametrize("name", ["PP16", "PP24"])
def test_full_range_and_saturated_gates(name, scale):
    """The stock synthetic weights never leave the linear part of the gates (|h| <= 0.32).  GRU weights x 2: |h| up to 0.9, still
    admissible free-running; x 4 and x 8: saturated gates -- large arguments of the kernel's exp2-prescaled sigmoid / tanh --,
    where fp32 and float64 trajectories diverge, so teacher-forced only."""
    own = _own_model(name, scale)
    try:
        _seams(f"range.{name}.x{scale}", name, 2, 3000, free=scale == 2, model_spec_sd=own, key=(name, scale), seed=6)
    finally:
        own[0].reset_workspace()
        _layers.pop((name, scale), None)


def test_agent_scope_publish_form():
    """ou_set_gru_publish_mode(h, 1): every publish an agent-scope store."""
    model = get_model("PP16")[0]
    model.reset_workspace()
    assert model._L.ou_set_gru_publish_mode(model._handle, 1) == 0
    try:
        _seams("publish1.PP16.b1", "PP16", 1, 401, seed=7)
    finally:
        model._L.ou_set_gru_publish_mode(model._handle, 0)
        model.reset_workspace()
