"""GPU (-m gpu): the small kernels of ou_small.hip against the float64 references of tests/small_fp64.py, element by element:
every element of a tap is held against its derived bound (or, behind a row's end, against exactly 0), none is left out.

The kernels are driven through the public seams (condition_model(train=True), score_model, a whole _enhance, also with
t_raw= for ragged batches) and isolated by reading the library's own intermediates with model.tensor(name): the reference
gets the very input the kernel read.  Tap pairs:

    mel_kernel, mel_scale_kernel   normalised input -> cond.mel, mel_scale (ragged: the row's own frames)
    in_conv_kernel                 input -> cond.in;  x, w_in -> score.in (per-row sigma)
    s2d_kernel                     cond.enc{i}.v -> cond.s2d{i}
    sum_kernel                     cond.melblock.v, cond.st{i}, last encoder output -> cond.enc_sum
    sigma_embed_kernel             per-row sigma -> sigma.g      (simple: PP*; random Fourier features: OR16s)
    film_kernel                    sigma.g -> sigma.film
    out_conv_kernel (OUT_SCORE)    score.dec{last}.v, x -> returned score (EDM: PP*; plain model: OR16s)
    out_conv_kernel (OUT_UPDATE), in_conv_kernel with ONE shared sigma, init_x_kernel with a base:
                                   a warm-started enhance of one step: wav, noise -> x0 (exact) -> score.in;
                                   score.dec{last}.v, x0 -> tap x (the update without the noise term)
    sampler_step_kernel            ou_sampler_step, with and without the noise term
    fir4_kernel<5 / 7 / 9 / 11 / 17>   options fuse_upfir = 0, rate_small = 0: score.enc{i}.v -> score.enc{i}.fir (PReLU, no bias),
                                   score.dec{j}.upc, residual -> score.dec{j}.up (bias, residual); ragged with mask_fused = 0,
                                   where mask_tail_kernel runs behind every producer
    pad_normalize_kernel (both paths), pad_normalize_var_kernel     mix -> mixn
    post_reg_kernel, post_kernel, post_var_kernel                   tap x -> returned output

Cases and edge classes: small_fp64.CASES / RAGGED (tests/test_small_fp64_cpu.py asserts their coverage).  What is not covered
yet and the branches no seam reaches: the docstring of tests/small_fp64.py.  Every case logs its figures to
build/observed/small_fp64_observed.json (untracked) before it asserts; profiles/small_fp64_observed.json is the committed
copy."""
import json
import os
import time

import pytest
import torch

import restatement as O
import small_fp64 as F
from helpers import synth_mix
from open_universe_amd import _lib
from test_gpu_parity import get_model, noise_list, run_enhance

pytestmark = pytest.mark.gpu

_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed")
_params = {}


def _P(name, spec, sd):
    if name not in _params:
        _params[name] = F.Params(spec, sd)
    return _params[name]


def _tap(model, name):
    return model.tensor(name).cpu().clone()  # copied out before the next call re-uses the workspace


def _finish(case, reps, t0, group=None):
    """Log, print, then assert; `group`: the case list of small_fp64.REPORTED whose kernels this case has to have held."""
    log_error = None
    try:
        os.makedirs(_OUT, exist_ok=True)
        path = os.path.join(_OUT, "small_fp64_observed.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[case] = {"seconds": round(time.time() - t0, 2)}
        for k, r in reps.items():
            old[case][k] = r.summary()
            if hasattr(r, "lib_ratio"):
                old[case][k].update(e32=r.e32, lib_ratio=round(r.lib_ratio, 3))
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError as e:  # (the figures follow on stdout; the test fails for it behind its own assertions)
        log_error = e
    for k, r in reps.items():
        print(f"{case} {r}" + (f" err / e32 = {r.lib_ratio:.2f}" if hasattr(r, "lib_ratio") else ""))
    for k, r in reps.items():
        assert r.excluded == 0 and r.ok(), f"{case} {r}"
        if hasattr(r, "lib_ratio"):
            assert r.lib_ratio <= F.M_CAP, f"{case} {k}: err / e32 = {r.lib_ratio:.2f} is a finding, not a tolerance"
    if group is not None:
        held = {F.family(k) for k in reps}
        assert set(F.REPORTED[group]) <= held, (case, group, sorted(held))
    assert log_error is None, f"{case}: could not write the observed figures: {log_error}"


def _condition_reports(reps, model, spec, P, xin, lens_T=None, frames=None):
    """The conditioner's small kernels from the taps of the last conditioner pass.  `xin`: the normalised input it read (CPU)."""
    td = spec.tot_ds
    B, _, T = xin.shape
    n = len(spec.cond.rate_factors)
    last = n + int(spec.cond.extra_conv_block) - 1
    ref, bound = F.mel(xin, P)
    reps["mel"] = F.Report("mel", _tap(model, "cond.mel"), ref, bound, frames)
    mel_tap = _tap(model, "cond.mel")
    ref, bound = F.mel_scale(mel_tap, frames)
    reps["mel_scale"] = F.Report("mel_scale", _tap(model, "mel_scale"), ref, bound)
    ref, bound = F.in_conv(xin, P.c_in_w, P.c_in_b)
    reps["cond.in"] = F.Report("cond.in", _tap(model, "cond.in"), ref, bound, lens_T)
    parts = [_tap(model, "cond.melblock.v")]
    for i in range(n - 1):
        ref, bound = F.s2d(_tap(model, f"cond.enc{i}.v"), P.st_alpha[i], P.st_rate[i])
        reps[f"s2d{i}"] = F.Report(f"s2d{i}", _tap(model, f"cond.s2d{i}"), ref, bound, frames)
        parts.append(_tap(model, f"cond.st{i}"))
    parts.append(_tap(model, f"cond.enc{last}.v" if spec.cond.extra_conv_block else f"cond.enc{last}.h"))
    ref, bound = F.sum_scaled(parts, F.sum_scale_of(len(parts)))
    reps["enc_sum"] = F.Report("enc_sum", _tap(model, "cond.enc_sum"), ref, bound, frames)


def _score_reports(reps, model, spec, P, shape, sig, seed):
    """ou_score on x = sig[b] * N(0, 1) of `shape` with the per-row sigmas `sig` (any number of rows), behind a conditioner pass
    of the same shape: score.in, sigma.g, sigma.film and the returned score, every row."""
    B = shape[0]
    assert sig.numel() == B
    xs = (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * sig[:, None, None]).float().contiguous()
    score = model.score_model(xs.cuda(), sig).cpu()
    coef = F.edm_coef(spec, sig)
    ref, bound = F.in_conv(xs, P.s_in_w, P.s_in_b, coef["w_in"] if P.edm else None)
    reps["score.in"] = F.Report("score.in", _tap(model, "score.in"), ref, bound)
    g = _tap(model, "sigma.g")
    reps["sigma_embed"] = F.check_sigma_embed(g, coef["sigma_net"], P)
    ref, bound = F.film(g, P.film_w, P.film_b)
    reps["film"] = F.Report("film", _tap(model, "sigma.film"), ref.reshape(B, -1, 1), bound)
    last = len(spec.score.rate_factors) + int(spec.score.extra_conv_block) - 1
    ref, bound = F.out_conv_score(_tap(model, f"score.dec{last}.v"), xs, P, coef)
    reps["out_conv"] = F.Report("out_conv", score, ref, bound)


@pytest.mark.parametrize("name,B,frames", F.CASES)
def test_conditioner_and_score_seams(name, B, frames):
    t0 = time.time()
    model, spec, sd = get_model(name)
    P = _P(name, spec, sd)
    T = spec.tot_ds * frames
    xin = O.normalize(synth_mix(spec, B, T, seed=1000 + frames)[:, None, :], spec.level_db).float().contiguous()
    model.condition_model(xin.cuda(), train=True)
    reps = {}
    _condition_reports(reps, model, spec, P, xin)

    _score_reports(reps, model, spec, P, xin.shape, torch.tensor([0.3, 1.7, 0.05, 4.0])[:B], 5 + frames)
    _finish(f"seams.{name}.b{B}.f{frames}", reps, t0, "CASES")


@pytest.mark.parametrize("name,rows", F.RAGGED)
def test_ragged_batch(name, rows):
    """ou_enhance_var: pad_normalize_var / post_var with every row's own geometry, the row's own frames in mel_scale, exactly 0
    behind every row's end on every tap.  (upload_rows_kernel's table is not readable through a tensor name: a wrong per-level
    length shows here as a tail that is not zero or a row cut short, not as a number compared.)"""
    t0 = time.time()
    model, spec, sd = get_model(name)
    P = _P(name, spec, sd)
    td = spec.tot_ds
    t_raw = [f * td - 3 for f in rows]
    B, lm = len(t_raw), max(t_raw)
    T = lm + (td - lm % td)
    sigs = [synth_mix(spec, 1, n, seed=300 + i)[0] for i, n in enumerate(t_raw)]
    mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs])[:, None, :]
    nz = torch.zeros(2, B, 1, T)
    for b, n in enumerate(t_raw):
        tb = n + (td - n % td)
        nz[:, b, 0, :tb] = torch.randn(2, tb, generator=torch.Generator().manual_seed(900 + b))
    out = model._enhance(mix.cuda(), 2, None, None, None, None, False, True, None, "median", None, nz.cuda(), t_raw=list(t_raw)).cpu()
    reps = {}
    ref, bound, lens_T = F.pad_normalize(mix, t_raw, T, P.level, td)
    assert lens_T == [f * td for f in rows]
    mixn = _tap(model, "mixn")
    reps["pad_normalize_var"] = F.Report("pad_normalize_var", mixn, ref, bound, lens_T)
    _condition_reports(reps, model, spec, P, mixn, lens_T, list(rows))
    pl = [(td - n % td) // 2 for n in t_raw]
    ref, bound, _ = F.post(_tap(model, "x"), mix, t_raw, pl, True)
    reps["post_var"] = F.Report("post_var", out, ref, bound, t_raw)
    _finish(f"ragged.{name}", reps, t0, "RAGGED")
    model.reset_workspace()


@pytest.mark.parametrize("keep,loud", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("T_raw", [1, 1023, 1025, 65536, 65537])
def test_pad_normalize_and_post(T_raw, keep, loud):
    """A whole enhance at the lengths where the register-window kernels end (65 536) and their buffer accesses run past the
    row: keep_rms off / on, the peak guard idle and dividing (one row 60 times louder)."""
    t0 = time.time()
    model, spec, sd = get_model("PP16s")
    P = _P("PP16s", spec, sd)
    td = spec.tot_ds
    B = 2
    mix = synth_mix(spec, B, T_raw, seed=40) + 0.01
    if loud:
        mix[1] *= 60.0
    T = T_raw + (td - T_raw % td)
    out = run_enhance(model, mix, noise_list(17, 2, B, T), n_steps=2, keep_rms=keep)
    reps = {}
    ref, bound, lens = F.pad_normalize(mix, [T_raw] * B, T, P.level, td)
    mixn = _tap(model, "mixn")
    reps["pad_normalize"] = F.Report("pad_normalize", mixn, ref, bound)
    pl = (T - T_raw) // 2
    for b in range(B):  # the padding value: one fp32 number per row, exactly
        padv = torch.cat([mixn[b, 0, :pl], mixn[b, 0, pl + T_raw:]])
        assert bool((padv == padv[0]).all()), (b, "padding values differ")
    ref, bound, divided = F.post(_tap(model, "x"), mix[:, None, :], [T_raw] * B, [pl] * B, keep)
    if loud and keep and T_raw > 1:  # (without keep_rms the output stays at the normalised level whatever the mix's)
        assert divided[1], "the loud row was meant to make the peak guard divide"
    reps["post"] = F.Report("post", out.reshape(B, 1, -1), ref, bound)
    _finish(f"prepost.T{T_raw}.keep{int(keep)}.loud{int(loud)}", reps, t0)
    if T_raw > 60000:
        model.reset_workspace()


_blobs = {}


def _blob(name, spec, sd):
    if name not in _blobs:
        blob, plan = _lib.pack_weights(spec, sd)
        _blobs[name] = (blob, {c["name"]: c for c in json.loads(plan)["convs"]}, json.loads(plan))
    return _blobs[name]


def _fir_reports(reps, model, name, spec, sd, frames=None):
    """Both stand-alone FIR passes of the score network from the taps of its last pass.  `frames`: per-row frames (ragged)."""
    blob, convs, plan = _blob(name, spec, sd)
    sp = spec.score_prefix
    nb = len(spec.score.rate_factors) + int(spec.score.extra_conv_block)
    seen = set()
    for i in range(len(spec.score.rate_factors)):
        c = convs[f"{sp}.encoder.ds_modules.{i}.rate_change_conv"]
        assert c["fir_mode"] == 1
        taps = blob[c["fir_off"]: c["fir_off"] + c["fir_len"]]
        x = _tap(model, f"score.enc{i}.v")
        ref, bound = F.fir(x, taps, alpha=blob[c["a_off"]])
        # (ragged: the library leaves this pass unmasked -- the k = s = r conv that reads it has no halo --, so the NT / 2 samples
        # behind a row's end hold the filter's run-out of the row, not 0: the whole buffer is held against the reference of the
        # whole buffer, whose input is 0 behind the row)
        reps[f"fir.down{i}.nt{c['fir_len']}"] = F.Report(f"fir.down{i}", _tap(model, f"score.enc{i}.fir"), ref, bound)
        seen.add(c["fir_len"])
    for j in range(nb):
        c = convs.get(f"{sp}.decoder.up_modules.{j}.rate_change_conv")
        if c is None or c["fir_mode"] != 2:
            continue
        taps = blob[c["fir_off"]: c["fir_off"] + c["fir_len"]]
        bias = blob[c["fbias_off"]: c["fbias_off"] + c["Cout"]]
        upc, res = _tap(model, f"score.dec{j}.upc"), _tap(model, f"score.enc{nb - 1 - j}.v")
        ref, bound = F.fir(upc, taps, bias=bias, res=res, res_scale=F.INV_SQRT2)
        lens = None if frames is None else [f * (upc.shape[-1] // max(frames)) for f in frames]
        reps[f"fir.up{j}.nt{c['fir_len']}"] = F.Report(f"fir.up{j}", _tap(model, f"score.dec{j}.up"), ref, bound, lens)
    return seen


@pytest.mark.parametrize("name,B,frames", F.FIR_CASES)
def test_stand_alone_fir_passes(name, B, frames, steer):
    """fuse_upfir = 0 and rate_small = 0 bring up launch_fir on both paths.  Tap counts 5, 9, 11 (PP16) and 5, 7, 11, 17 (PP24):
    every fir4_kernel instantiation; the scalar fir_kernel takes only tap counts no shipped topology has (unreached)."""
    t0 = time.time()
    steer.set(fuse_upfir=0, rate_small=0)
    model, spec, sd = get_model(name)
    model.reset_workspace()
    try:
        T = spec.tot_ds * frames
        xin = O.normalize(synth_mix(spec, B, T, seed=2000 + frames)[:, None, :], spec.level_db).float().contiguous()
        model.condition_model(xin.cuda(), train=True)
        sig = torch.tensor([0.3, 1.7, 0.05])[:B]
        xs = (torch.randn(xin.shape, generator=torch.Generator().manual_seed(frames)) * sig[:, None, None]).float().contiguous()
        model.score_model(xs.cuda(), sig)
        reps = {}
        seen = _fir_reports(reps, model, name, spec, sd)
        assert seen == ({5, 9, 11} if name.startswith("PP16") else {5, 7, 11, 17})
        _finish(f"fir.{name}.b{B}.f{frames}", reps, t0, "FIR_CASES")
    finally:
        model.reset_workspace()


@pytest.mark.parametrize("mask_fused", [0, 1])
@pytest.mark.parametrize("name,rows", F.FIR_RAGGED)
def test_ragged_batch_with_stand_alone_fir(name, rows, mask_fused, steer):
    """mask_fused = 0: every producer is followed by mask_tail_kernel and the FIR pass runs WITHOUT the rows' lengths (the mask
    launch zeroes behind it).  mask_fused = 1: the up-path FIR pass gets the lengths and masks in its own epilogue
    (fir4_kernel's ragged_mask4: bias + residual would stand behind the row's end otherwise).  Both: the conditioner's taps and
    both FIR passes, tails exactly 0."""
    t0 = time.time()
    steer.set(fuse_upfir=0, rate_small=0, mask_fused=mask_fused)
    model, spec, sd = get_model(name)
    model.reset_workspace()
    try:
        P = _P(name, spec, sd)
        td = spec.tot_ds
        t_raw = [f * td - 3 for f in rows]
        B, lm = len(t_raw), max(t_raw)
        T = lm + (td - lm % td)
        sigs = [synth_mix(spec, 1, n, seed=400 + i)[0] for i, n in enumerate(t_raw)]
        mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs])[:, None, :]
        nz = torch.zeros(2, B, 1, T)
        for b, n in enumerate(t_raw):
            nz[:, b, 0, :rows[b] * td] = torch.randn(2, rows[b] * td, generator=torch.Generator().manual_seed(950 + b))
        model._enhance(mix.cuda(), 2, None, None, None, None, False, False, None, "median", None, nz.cuda(), t_raw=list(t_raw))
        reps = {}
        _condition_reports(reps, model, spec, P, _tap(model, "mixn"), [f * td for f in rows], list(rows))
        _fir_reports(reps, model, name, spec, sd, list(rows))
        _finish(f"fir_ragged.mask_fused{mask_fused}.{name}", reps, t0, "FIR_RAGGED_FUSED" if mask_fused else "FIR_RAGGED_MASKS")
    finally:
        model.reset_workspace()


@pytest.mark.parametrize("name,B,frames", F.SHARED)
def test_shared_sigma_and_fused_update(name, B, frames):
    """enhance(n_steps=2, warm_start=1) is ONE sampler step at sigma_min, shared by the rows (coefficient stride 0), from
    x0 = wav + sigma * noise -- known exactly from the wav tap.  score.in against x0 and the shared w_in; the tap x holds the
    fused update x0 + c1 score (the last step: no noise term) from score.dec{last}.v.  (The update WITH its noise term is never
    the last step, and the steps before the last leave no taps: it is held through sampler_step_kernel below, same arithmetic.)"""
    t0 = time.time()
    model, spec, sd = get_model(name)
    P = _P(name, spec, sd)
    td = spec.tot_ds
    T = td * frames
    mix = synth_mix(spec, B, T - 5, seed=70)
    noise = noise_list(23, 1, B, T)
    run_enhance(model, mix, noise, n_steps=2, warm_start=1)
    sigma = float(model._sigma_table(2)[1])
    coef = F.edm_coef(spec, [sigma] * B)
    x0 = F.init_x(noise[0], sigma, _tap(model, "wav"))
    reps = {}
    ref, bound = F.in_conv(x0, P.s_in_w, P.s_in_b, coef["w_in"] if P.edm else None)
    reps["score.in"] = F.Report("score.in(shared)", _tap(model, "score.in"), ref, bound)
    last = len(spec.score.rate_factors) + int(spec.score.extra_conv_block) - 1
    score, sb = F.out_conv_score(_tap(model, f"score.dec{last}.v"), x0, P, coef)
    ref, bound = F.sampler_update(x0, score, float(coef["sig2"][0]), score_bound=sb)
    reps["out_conv.update"] = F.Report("out_conv.update", _tap(model, "x"), ref, bound)
    _finish(f"shared.{name}.b{B}.f{frames}", reps, t0)


@pytest.mark.parametrize("with_noise", [False, True])
def test_sampler_step(with_noise):
    import ctypes

    t0 = time.time()
    model = get_model("PP16s")[0]
    n = 3 * 1025 + 1
    g = torch.Generator().manual_seed(3)
    x, sc, z = (torch.randn(1, 1, n, generator=g) for _ in range(3))
    c1, c2 = torch.tensor(0.37).item(), torch.tensor(0.11).item()
    xd, sd_, zd = x.cuda(), sc.cuda(), z.cuda()
    _lib.check(model._L.ou_sampler_step(model._handle, ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(sd_.data_ptr()),
                                        ctypes.c_void_p(zd.data_ptr()) if with_noise else None, c1, c2, n,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), model._handle)
    torch.cuda.synchronize()
    ref, bound = F.sampler_update(x, sc, c1, z if with_noise else None, c2)
    _finish(f"sampler_step.noise{int(with_noise)}", {"sampler_step": F.Report("sampler_step", xd.cpu(), ref, bound)}, t0)


@pytest.mark.parametrize("name,rows", F.RAGGED_STEP)
def test_ragged_warm_started_step(name, rows):
    """ou_enhance_var, n_steps=2, warm_start=1: one step from x0 = (wav + sigma noise) masked to the rows.  in_conv_kernel and
    out_conv_kernel of the score network with per-row lengths: score.in and the update in tap x, exactly 0 behind every row."""
    t0 = time.time()
    model, spec, sd = get_model(name)
    P = _P(name, spec, sd)
    td = spec.tot_ds
    t_raw = [f * td - 3 for f in rows]
    B, lm = len(t_raw), max(t_raw)
    T = max(rows) * td
    lens = [f * td for f in rows]
    sigs = [synth_mix(spec, 1, n, seed=500 + i)[0] for i, n in enumerate(t_raw)]
    mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs])[:, None, :]
    nz = torch.zeros(1, B, 1, T)
    for b in range(B):
        nz[0, b, 0, :lens[b]] = torch.randn(lens[b], generator=torch.Generator().manual_seed(960 + b))
    model._enhance(mix.cuda(), 2, None, None, None, None, False, False, None, "median", 1, nz.cuda(), t_raw=list(t_raw))
    sigma = float(model._sigma_table(2)[1])
    coef = F.edm_coef(spec, [sigma] * B)
    valid = F.valid_mask(lens, B, T)
    wav = _tap(model, "wav")
    assert bool((wav[~valid] == 0).all()), "wav is not zero behind a row's end"
    x0 = F.init_x(nz[0], sigma, wav) * valid
    reps = {}
    ref, bound = F.in_conv(x0, P.s_in_w, P.s_in_b, coef["w_in"] if P.edm else None)
    reps["score.in"] = F.Report("score.in(ragged)", _tap(model, "score.in"), ref, bound, lens)
    last = len(spec.score.rate_factors) + int(spec.score.extra_conv_block) - 1
    score, sb = F.out_conv_score(_tap(model, f"score.dec{last}.v"), x0, P, coef)
    ref, bound = F.sampler_update(x0, score, float(coef["sig2"][0]), score_bound=sb)
    reps["out_conv.update"] = F.Report("out_conv.update(ragged)", _tap(model, "x"), ref, bound, lens)
    _finish(f"ragged_step.{name}", reps, t0, "RAGGED_STEP")
    model.reset_workspace()


_snake = {}


@pytest.mark.parametrize("name,B,frames", F.SNAKE_CASES)
def test_snake_decoupling(name, B, frames):
    """cond.aux -> aux_to_wav(): snake_up_kernel + snake_down_conv_kernel as one stage (the up-sampled signal has no name)."""
    t0 = time.time()
    model, spec, sd = get_model(name)
    if name not in _snake:
        _snake[name] = F.SnakeParams(sd)
    T = spec.tot_ds * frames
    xin = O.normalize(synth_mix(spec, B, T, seed=3000 + frames)[:, None, :], spec.level_db).float().contiguous()
    model.condition_model(xin.cuda(), train=True)
    aux = _tap(model, "cond.aux")
    wav = model.aux_to_wav().cpu()
    ref = F.snake(aux, _snake[name])
    rep = F.lib_report("snake", wav, ref, F.snake(aux, _snake[name], torch.float32), F.M_SNAKE)
    _finish(f"snake.{name}.b{B}.f{frames}", {"snake": rep}, t0)


@pytest.mark.parametrize("case", F.STFT_CASES, ids=[c[0] for c in F.STFT_CASES])
def test_stft_pair(case):
    """ou_transform_forward / ou_transform_inverse (what the CompressedMagSTFT* layers call) with the inverse's frame scratch
    read back: forward and inverse frames at the `library` bound, overlap-add at its chain bound from the GPU's own frames --
    once at the default length and once at a length whose last samples lie behind every frame (envelope 0: exactly 0)."""
    import ctypes
    from ctypes import c_void_p

    from open_universe_amd.layers.dyn_range_comp import _TYPES, get_window

    t0 = time.time()
    tag, N, hop, wn, kind, e, fac, T, B = case
    e, fac = torch.tensor(e).item(), torch.tensor(fac).item()  # the fp32 values the C ABI's float arguments carry
    L = _lib.load()
    win = get_window(wn, N)
    x = (synth_mix(get_model("PP16s")[1], B, T, seed=80) * 5.0).float().contiguous()
    F_, nf = N // 2 + 1, F.stft_frames_count(T, N, hop)
    assert nf == L.ou_transform_frames(T, N, hop)
    xd, wd = x.cuda(), win.cuda()
    out = torch.empty(B, 2 * F_, nf, dtype=torch.float32, device="cuda")
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.ou_transform_forward(c_void_p(xd.data_ptr()), B, T, c_void_p(wd.data_ptr()), N, hop, _TYPES[kind], e, fac,
                                      c_void_p(out.data_ptr()), st))
    reps = {}
    spec_gpu = out.cpu()
    reps["stft.forward"] = F.lib_report("stft.forward", spec_gpu, F.stft_forward(x, win, N, hop, kind, e, fac),
                                        F.stft_forward(x, win, N, hop, kind, e, fac, torch.float32), F.M_STFT_FWD)
    fr_ref = F.stft_inverse_frames(spec_gpu, win, N, kind, e, fac)
    fr_32 = F.stft_inverse_frames(spec_gpu, win, N, kind, e, fac, torch.float32)
    for which, length in (("default", max(1, hop * (nf - 1))), ("zero_env", (nf - 1) * hop + N - N // 2 + 3)):
        y = torch.empty(B, length, dtype=torch.float32, device="cuda")
        scratch = torch.zeros(B * nf * N, dtype=torch.float32, device="cuda")
        _lib.check(L.ou_transform_inverse(c_void_p(out.data_ptr()), B, nf, c_void_p(wd.data_ptr()), N, hop, _TYPES[kind], e, fac,
                                          int(length), c_void_p(y.data_ptr()), c_void_p(scratch.data_ptr()), st))
        frames = scratch.cpu().view(B, nf, N)
        reps[f"stft.inverse_frames.{which}"] = F.lib_report("stft.inverse_frames", frames, fr_ref, fr_32, F.M_STFT_INV)
        ref, bound = F.stft_overlap_add(frames, win, N, hop, length)
        reps[f"stft.overlap_add.{which}"] = F.Report("stft.overlap_add", y.cpu(), ref, bound)
    _finish(f"stft.{tag}", reps, t0)
