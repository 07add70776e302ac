"""GPU (-m gpu): level normalisation held sample by sample in every mode and at every clamp.

pad_normalize_kernel (register window and loops), pad_normalize_var_kernel and the post kernels behind them, in all six
(normalization_norm, zero_mean) modes of ou_set_normalization, against the float64 reference of tests/small_fp64.py
(pad_normalize with norm / zero_mean / eps; post) on the rows of tests/norm_cases.py (element_rows: smooth on a DC offset,
the spike at three places, all zero, constant, quiet) at the lengths of norm_cases.lengths.  Models are built from a spec;
every call is PP16s, two steps; taps mixn, stats, x and the returned output.

    test_pad_normalize_every_mode            mixn element by element, the padding value, stats
    test_eps_reaches_the_2max_branch_alone   normalization_kwargs.eps under 2 / max / 2-max, through the spec and through the C setter
    test_pad_normalize_var_every_mode        one ragged call of the six lengths: mixn per row, zero tails, each row bit for bit the
                                             row of the whole-call kernel
    test_post_after_every_mode               post_reg / post / post_var of rows that kept their DC offset, the silent row under keep_rms

Figures: build/observed/norm_fp64_observed.json (untracked) before anything is asserted; profiles/norm_fp64_observed.json is the
committed copy.  The bounds are derived in tests/small_fp64.py and tests/norm_cases.py; the figures record what room they leave."""
import json
import os
import time

import numpy as np
import pytest
import torch

import norm_cases as K
import small_fp64 as F
from open_universe_amd import Universe, UniverseGAN, _lib
from open_universe_amd import state_dict as S
from test_gpu_norm import _enhance, _hold_stats

pytestmark = pytest.mark.gpu

_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed")
_models = {}
_uniform = {}
LOUD = "spike0_x60"  # test_post_after_every_mode


def get_model(norm, zero_mean, eps=None):
    key = (norm, zero_mean, eps)
    if key not in _models:
        spec = K.mode_spec("PP16s", norm, zero_mean, eps)
        sd = S.synthetic_state_dict(spec, seed=K.SEED)
        cls = UniverseGAN if spec.kind == "universe_gan" else Universe
        _models[key] = (cls(spec, state_dict=sd, device="cuda:0"), spec)
    model, spec = _models[key]
    assert (str(spec.norm), bool(spec.zero_mean), spec.norm_eps) == (norm, zero_mean, 1e-5 if eps is None else eps)
    return model, spec


def _level(spec):
    """The fp32 level the library is handed."""
    return torch.tensor(10.0 ** (spec.level_db / 20.0), dtype=torch.float64).float()


def _tap(model, name):
    return model.tensor(name).cpu().clone()


def _plan(model):
    return json.loads(model._L.ou_plan_json(model._handle).decode())


def _finish(case, reps, t0, **extra):
    """Log, print, then assert."""
    log_error = None
    try:
        os.makedirs(_OUT, exist_ok=True)
        path = os.path.join(_OUT, "norm_fp64_observed.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[case] = dict({"seconds": round(time.time() - t0, 2)}, **extra)
        for k, r in reps.items():
            old[case][k] = r.summary()
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError as e:
        log_error = e
    for k, r in reps.items():
        print(f"{case} {r}")
    for k, r in reps.items():
        assert r.excluded == 0 and r.ok(), f"{case} {r}"
    assert log_error is None, f"{case}: could not write the observed figures: {log_error}"


def _padded_len(T, td):
    return T + (td - T % td)


def _whole_call(model, spec, T, keep_rms=False, seed=3, more=None):
    """One enhance of every row kind that exists at T samples (and the rows `more` makes of them) -> (kinds, mix, mixn, stats, x, out)."""
    rows = K.element_rows(spec, T)
    if more is not None:
        rows.update(more(rows))
    mix = torch.stack(list(rows.values()))
    Tp = _padded_len(T, spec.tot_ds)
    out = _enhance(model, mix, torch.stack(K.noise_planes(seed, 2, len(rows), Tp)), n_steps=2, keep_rms=keep_rms)
    return list(rows), mix, _tap(model, "mixn"), _tap(model, "stats")[:, :, 0], _tap(model, "x"), out


def _check_padding(tag, mixn, stats, T, Tp, lens_pad, zero_mean):
    """The padding of row b: ONE fp32 value, fl((0 - mu) * gain) of the row's stored statistics -- exactly 0 with zero_mean false."""
    for b in range(mixn.shape[0]):
        pl = (lens_pad[b] - T[b]) // 2
        padv = torch.cat([mixn[b, 0, :pl], mixn[b, 0, pl + T[b]: lens_pad[b]]])
        assert padv.numel() == lens_pad[b] - T[b] > 0
        want = (np.float32(0) - np.float32(stats[b, 0])) * np.float32(stats[b, 1])
        assert bool((padv == padv[0]).all()) and np.float32(padv[0]) == want, (tag, b, "padding value", float(padv[0]), float(want))
        if not zero_mean:
            assert not padv.any() and float(stats[b, 0]) == 0.0, (tag, b, "the padding of a row that keeps its mean is not 0")


# ---- 1. pad_normalize_kernel<true> (and <false> in the plain mode), sample by sample ---------------------------------------------
@pytest.mark.parametrize("length", list(K.lengths(160)))
@pytest.mark.parametrize("norm,zero_mean", K.ALL_MODES)
def test_pad_normalize_every_mode(norm, zero_mean, length):
    t0 = time.time()
    model, spec = get_model(norm, zero_mean)
    td = spec.tot_ds
    T = K.lengths(td)[length]
    Tp = _padded_len(T, td)
    kinds, mix, mixn, stats, _, _ = _whole_call(model, spec, T)
    B = len(kinds)
    assert mixn.shape == (B, 1, Tp)
    ref, bound, lens = F.pad_normalize(mix, [T] * B, Tp, _level(spec), td, norm=norm, zero_mean=zero_mean)
    rep = F.Report("pad_normalize", mixn, ref, bound)
    case = f"pad_normalize.{norm}.zm{int(zero_mean)}.T{T}"
    _finish(case, {"pad_normalize": rep}, t0, kinds=kinds)
    _check_padding(case, mixn, stats, [T] * B, Tp, lens, zero_mean)
    _hold_stats(case, stats, list(mix), [Tp] * B, spec, (norm, zero_mean))
    _uniform[(norm, zero_mean, T)] = (kinds, mixn, stats)
    if T > 60000:
        model.reset_workspace()


# ---- 2. normalization_kwargs.eps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["2", "max", "2-max"])
def test_eps_reaches_the_2max_branch_alone(norm):
    """eps = 1e-3 on the quiet row (1e-5 < sd < mx < 1e-3): under 2-max both norms clamp at eps and the gain is
    fl(min(level / 1e-3, 1 / 1e-3)); under 2 and max the key changes nothing -- whether it comes in through the spec or straight
    through ou_set_normalization (the host rule of ou_api.cpp; NormMode::gain itself applies whatever eps it is handed)."""
    with_eps, spec = get_model(norm, True, 1e-3)
    without, _ = get_model(norm, True)
    td = spec.tot_ds
    T = td + 1
    Tp = _padded_len(T, td)
    f = np.float32
    kinds, mix, mixn_e, stats_e, _, _ = _whole_call(with_eps, spec, T)
    _, _, mixn_d, stats_d, _, _ = _whole_call(without, spec, T)
    q = kinds.index("quiet")
    st = K.norm_stats(K.padded(mix[q], td), norm, spec.level_db, True, 1e-3)
    assert 1e-5 < st["sd"] < st["mx"] < 1e-3
    if norm == "2-max":
        assert f(_plan(with_eps)["norm_eps"]) == f(1e-3) and f(_plan(without)["norm_eps"]) == f(1e-5)
        want = K.gain32("2-max", spec.level_db, f(st["sd"]), f(st["mx"]), 1e-3)
        assert want == f(10.0 ** (spec.level_db / 20.0)) / f(1e-3)
        assert f(stats_e[q, 1]) == want, (float(stats_e[q, 1]), float(want))
        assert f(stats_d[q, 1]) != want  # (eps at 1e-5 clamps neither norm: level / sd of the row)
        _hold_stats("eps.2-max.unset", stats_d, list(mix), [Tp] * len(kinds), without.spec, (norm, True))
        ref, bound, _ = F.pad_normalize(mix, [T] * len(kinds), Tp, _level(spec), td, norm=norm, zero_mean=True, eps=1e-3)
        rep = F.Report("pad_normalize", mixn_e, ref, bound)
        print(f"eps.2-max {rep}")
        assert rep.ok() and rep.excluded == 0, str(rep)
        _hold_stats("eps.2-max", stats_e, list(mix), [Tp] * len(kinds), spec, (norm, True))
        return
    assert f(_plan(with_eps)["norm_eps"]) == f(1e-5) == f(_plan(without)["norm_eps"])
    assert torch.equal(stats_e, stats_d) and torch.equal(mixn_e, mixn_d)
    # the same key straight through the C setter: the library keeps the clamp of 2 and max at 1e-5
    mode = {"2": _lib.OU_NORM_2, "max": _lib.OU_NORM_MAX}[norm]
    try:
        _lib.check(without._L.ou_set_normalization(without._handle, mode, 1, 1e-3), without._handle)
        assert f(_plan(without)["norm_eps"]) == f(1e-5)
        _, _, mixn_c, stats_c, _, _ = _whole_call(without, spec, T)
    finally:
        _lib.check(without._L.ou_set_normalization(without._handle, mode, 1, 0.0), without._handle)
    assert torch.equal(stats_c, stats_d) and torch.equal(mixn_c, mixn_d)
    _hold_stats(f"eps.{norm}", stats_e, list(mix), [Tp] * len(kinds), without.spec, (norm, True))  # (the clamp in force: 1e-5)


# ---- 3. pad_normalize_var_kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm,zero_mean", K.ALL_MODES)
def test_pad_normalize_var_every_mode(norm, zero_mean):
    """One ragged call whose rows have the six lengths, the row kinds rotated through them.  Each row: mixn against float64,
    exactly 0 from its own T_pad on, and -- stats and mixn[:T_pad] -- bit for bit what pad_normalize_kernel makes of that row
    (its header comment promises the maximum; the sums run over the same elements per thread in the same order).  The
    whole-call kernel runs one block per row and knows nothing of the batch: the row is taken from the call on all kinds of its
    length, and for the first rotation also from a call on that row alone."""
    t0 = time.time()
    model, spec = get_model(norm, zero_mean)
    td = spec.tot_ds
    lengths = sorted(K.lengths(td).values(), reverse=True)
    per_len = [K.element_rows(spec, T) for T in lengths]
    lm = lengths[0]
    Tm = _padded_len(lm, td)
    t_pad = [_padded_len(n, td) for n in lengths]
    for T in lengths:
        if (norm, zero_mean, T) not in _uniform:
            kinds, _, mixn, stats, _, _ = _whole_call(model, spec, T)
            _uniform[(norm, zero_mean, T)] = (kinds, mixn, stats)
    reps, picked = {}, set()
    for v in range(len(K.ROW_KINDS)):
        kinds = [list(per_len[j])[(v + j) % len(per_len[j])] for j in range(len(lengths))]
        picked |= set(zip(lengths, kinds))
        rows = [per_len[j][k] for j, k in enumerate(kinds)]
        mix = torch.stack([torch.nn.functional.pad(r, (0, lm - r.numel())) for r in rows])
        nz = torch.zeros(2, len(rows), 1, Tm)
        for b, tp in enumerate(t_pad):
            nz[:, b, 0, :tp] = 1.0
        nz *= torch.stack(K.noise_planes(5 + v, 2, len(rows), Tm))
        _enhance(model, mix, nz, n_steps=2, t_raw=list(lengths))
        mixn, stats = _tap(model, "mixn"), _tap(model, "stats")[:, :, 0]
        assert mixn.shape == (len(rows), 1, Tm)
        ref, bound, lens = F.pad_normalize(mix, lengths, Tm, _level(spec), td, norm=norm, zero_mean=zero_mean)
        assert lens == t_pad
        reps[f"v{v}"] = F.Report(f"pad_normalize_var.v{v}", mixn, ref, bound, lens)
        case = f"pad_normalize_var.{norm}.zm{int(zero_mean)}.v{v}"
        for b, (T, kind) in enumerate(zip(lengths, kinds)):
            assert not mixn[b, 0, t_pad[b]:].any(), (case, b, "not zero behind the row's own T_pad")
            ukinds, umixn, ustats = _uniform[(norm, zero_mean, T)]
            u = ukinds.index(kind)
            assert torch.equal(stats[b], ustats[u]), (case, b, kind, "stats differ from the whole-call kernel's", stats[b], ustats[u])
            assert torch.equal(mixn[b, 0, :t_pad[b]], umixn[u, 0]), (case, b, kind, "mixn differs from the whole-call kernel's")
            if v == 0:
                _enhance(model, rows[b][None, :], torch.stack(K.noise_planes(9, 2, 1, t_pad[b])), n_steps=2)
                assert torch.equal(_tap(model, "stats")[0, :, 0], stats[b]) and torch.equal(_tap(model, "mixn")[0, 0], umixn[u, 0]), (case, b)
        _check_padding(case, mixn, stats, lengths, Tm, t_pad, zero_mean)
        _hold_stats(case, stats, rows, t_pad, spec, (norm, zero_mean))
    assert picked == {(T, k) for j, T in enumerate(lengths) for k in per_len[j]}  # every kind at every length it exists at
    _finish(f"pad_normalize_var.{norm}.zm{int(zero_mean)}", reps, t0)
    model.reset_workspace()


# ---- 4. the post kernels behind every mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", ["td+1", "65537"])
@pytest.mark.parametrize("norm,zero_mean", K.ALL_MODES)
@pytest.mark.parametrize("keep", [False, True])
def test_post_after_every_mode(keep, norm, zero_mean, length):
    """post_reg_kernel (td + 1) / post_kernel (65 537) after a whole call and post_var_kernel after a ragged one (the same rows
    and one short row), from the tap x.  Under keep_rms the silent row comes out exactly 0 (mix_rms = 0: g = 0 / max(x_rms, 1e-5)).
    The peak guard: keep_rms gives the output the mix's rms, which for the spike rows is 0.26 (td + 1 samples) and 0.058 (65 537)
    -- the output would need a crest factor of 4 resp. 17 to pass 1, and the two-step output of the seeded network has 2.7 resp. 5
    (peaks 0.70 and 0.30): measured on an MI355X, no row of norm_cases.element_rows makes the guard divide in any mode, max
    included.  So that the
    guard's division behind keep_rms is held in every mode all the same, the batch gets one more row, the spike row 60 times
    louder (mix_rms 15 resp. 3.5: x g has that rms, so its peak is above 1 whatever its shape), and the reference must say that it
    divides."""
    t0 = time.time()
    model, spec = get_model(norm, zero_mean)
    td = spec.tot_ds
    T = K.lengths(td)[length]
    Tp = _padded_len(T, td)
    pl = (Tp - T) // 2
    kinds, mix, _, _, x, out = _whole_call(model, spec, T, keep_rms=keep, seed=13, more=lambda r: {LOUD: r["spike0"] * 60.0})
    B = len(kinds)
    reps = {}
    ref, bound, divided = F.post(x, mix[:, None, :], [T] * B, [pl] * B, keep)
    reps["post"] = F.Report("post", out.reshape(B, 1, -1), ref, bound)
    # ragged: the same rows and one of td - 1 samples
    short = K.element_rows(spec, td - 1)["smooth"]
    t_raw = [T] * B + [td - 1]
    mixr = torch.cat([mix, torch.nn.functional.pad(short, (0, T - short.numel()))[None, :]])
    nz = torch.stack(K.noise_planes(13, 2, B + 1, Tp))
    nz[:, B, 0, td:] = 0.0
    outr = _enhance(model, mixr, nz, n_steps=2, keep_rms=keep, t_raw=list(t_raw))
    plr = [(_padded_len(n, td) - n) // 2 for n in t_raw]
    refr, boundr, dividedr = F.post(_tap(model, "x"), mixr[:, None, :], t_raw, plr, keep)
    reps["post_var"] = F.Report("post_var", outr.reshape(B + 1, 1, -1), refr, boundr, t_raw)
    peaks = {k: round(float(ref[b].abs().max()), 4) for b, k in enumerate(kinds)}
    print(f"post.{norm}.zm{int(zero_mean)}.keep{int(keep)}.T{T}: divided {dict(zip(kinds, divided))}; ragged {dividedr}; peaks {peaks}")
    _finish(f"post.{norm}.zm{int(zero_mean)}.keep{int(keep)}.T{T}", reps, t0, divided=[bool(d) for d in divided], peaks=peaks)
    assert torch.isfinite(out).all() and torch.isfinite(outr).all()
    if keep:
        z = kinds.index("zero")
        assert not out[z].any() and not outr[z].any(), "the silent row under keep_rms is not exactly 0"
        b = kinds.index(LOUD)
        assert divided[b] and dividedr[b], "the loud spike row was meant to make the peak guard divide"
        assert float(ref[b].abs().max()) == 1.0 and float(refr[b].abs().max()) == 1.0
    if T > 60000:
        model.reset_workspace()
