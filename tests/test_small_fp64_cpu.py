"""CPU: the checks of tests/small_fp64.py check.  For every reference a torch emulation of the kernel's arithmetic (fp32, the
kernel's summation order) passes the very check function the GPU test uses with nothing excluded, and every planted defect --
one at a time -- fails it.  And the case list of tests/test_gpu_small_fp64.py meets every edge class a call through the seams
can meet."""
import json
import math

import pytest
import torch

import small_fp64 as F
from helpers import get_spec, synth_mix
from open_universe_amd import _lib, state_dict as S

_cache = {}


def _params(name):
    if name not in _cache:
        spec = get_spec(name)
        sd = S.synthetic_state_dict(spec, seed=0)
        _cache[name] = (spec, sd, F.Params(spec, sd))
    return _cache[name]


def _randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("name", F.MODELS)
def test_rebuilt_parameters_are_the_blob(name, built_lib):
    spec, sd, P = _params(name)
    blob, plan = _lib.pack_weights(spec, sd)
    P.check_against_blob(blob, json.loads(plan))


# ---- in_conv -----------------------------------------------------------------------------------------------------------------
def _in_conv_case(scaled):
    spec, sd, P = _params("PP16s")
    x = _randn(3, 1, 257, seed=1)
    w_in = torch.tensor([0.7, 1.3, 0.05]) if scaled else None
    return P, x, w_in


@pytest.mark.parametrize("scaled", [False, True])
def test_in_conv_emulation_passes(scaled):
    P, x, w_in = _in_conv_case(scaled)
    ref, bound = F.in_conv(x, P.s_in_w, P.s_in_b, w_in)
    rep = F.Report("in_conv", F.in_conv_fp32(x, P.s_in_w, P.s_in_b, w_in), ref, bound)
    assert rep.ok() and rep.excluded == 0 and rep.checked == ref.numel(), rep


def test_in_conv_halo_from_the_neighbouring_row_fails():
    P, x, w_in = _in_conv_case(False)
    ref, bound = F.in_conv(x, P.s_in_w, P.s_in_b)

    def hook(t):  # the sample in front of row 1 read from the end of row 0 instead of 0
        t = t.clone()
        t[1, 0, 0, 0] = x[0, 0, -1]
        return t
    rep = F.Report("in_conv", F.in_conv_fp32(x, P.s_in_w, P.s_in_b, hook=hook), ref, bound)
    assert not rep.ok() and rep.worst["index"][0] == 1 and rep.worst["index"][2] == 0, rep


def test_in_conv_last_tap_dropped_at_the_end_fails():
    P, x, w_in = _in_conv_case(False)
    ref, bound = F.in_conv(x, P.s_in_w, P.s_in_b)

    def hook(t):  # the element behind a tile seam (t = 256 of 257) loses its first tap
        t = t.clone()
        t[:, :, 256, 0] = 0
        return t
    rep = F.Report("in_conv", F.in_conv_fp32(x, P.s_in_w, P.s_in_b, hook=hook), ref, bound)
    assert not rep.ok() and rep.n_bad <= 3 * P.s_in_w.shape[0], rep


def test_tail_holding_the_bias_fails():
    P, x, w_in = _in_conv_case(False)
    lens = [257, 100, 1]
    ref, bound = F.in_conv(x, P.s_in_w, P.s_in_b)
    good = F.in_conv_fp32(x, P.s_in_w, P.s_in_b) * F.valid_mask(lens, 3, 257)
    assert F.Report("in_conv", good, ref, bound, lens).ok()
    bad = good.clone()
    bad[1, :, 100:] = P.s_in_b[:, None]
    rep = F.Report("in_conv", bad, ref, bound, lens)
    assert not rep.ok() and rep.tail_bad == P.s_in_w.shape[0] * 157 and rep.excluded == 0, rep


# ---- out_conv ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["PP16s", "OR16s"])
def test_out_conv_emulation_passes_and_damages_fail(name):
    """EDM form (PP16s) and plain model (OR16s).  Damages: one tap dropped at the last partial quad; the window reading across
    a row end."""
    spec, sd, P = _params(name)
    B, T = 2, 1030
    s, x = _randn(B, P.out_w.shape[0], T, seed=2), _randn(B, 1, T, seed=3, scale=0.5)
    coef = F.edm_coef(spec, [0.3, 1.7])
    ref, bound = F.out_conv_score(s, x, P, coef)
    rep = F.Report("out_conv", F.out_conv_fp32(s, x, P, coef), ref, bound)
    assert rep.ok() and rep.excluded == 0, rep

    def drop(t):
        t = t.clone()
        t[:, 3, T - 2, 2] = 0
        return t

    def across(t):  # the sample behind the end of row 0 taken from the start of row 1
        t = t.clone()
        t[0, :, T - 1, 2] = t[1, :, 0, 1]
        return t
    for hook, where in ((drop, T - 2), (across, T - 1)):
        rep = F.Report("out_conv", F.out_conv_fp32(s, x, P, coef, hook), ref, bound)
        assert not rep.ok() and rep.worst["index"][2] == where, rep


# ---- FiLM, embedding ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["PP16s", "OR16s"])
def test_film_emulation_passes_and_damages_fail(name):
    spec, sd, P = _params(name)
    g = F.sigma_embed(torch.tensor([0.3, 1.7, 0.05]), P, torch.float32)
    ref, bound = F.film(g, P.film_w, P.film_b)
    rep = F.Report("film", F.film_fp32(g, P.film_w, P.film_b), ref, bound)
    assert rep.ok() and rep.excluded == 0, rep
    for stage in (32, 16, 8, 4, 2, 1):
        assert not F.Report("film", F.film_fp32(g, P.film_w, P.film_b, skip_stage=stage), ref, bound).ok(), stage
    assert not F.Report("film", F.film_fp32(g, P.film_w, P.film_b, swap_rows=spec.score.n_channels), ref, bound).ok()


@pytest.mark.parametrize("name", ["PP16s", "OR16s"])
def test_embedding_halves_swapped_fails(name):
    spec, sd, P = _params(name)
    sn = torch.tensor([0.3, 1.7, 0.05, 4.0])
    good = F.sigma_embed(sn, P, torch.float32)
    rep = F.check_sigma_embed(good[:, :, None], sn, P)
    assert rep.ok() and rep.excluded == 0, rep
    bad = F.sigma_embed(sn, P, torch.float32, swap_halves=True)
    assert not F.check_sigma_embed(bad[:, :, None], sn, P).ok()


# ---- mel ---------------------------------------------------------------------------------------------------------------------
def test_mel_emulation_passes_and_shifted_frame_fails():
    spec, sd, P = _params("PP16s")
    x = synth_mix(spec, 2, 3 * spec.tot_ds)[:, None, :] * 3
    ref, bound = F.mel(x, P)
    good, _ = F.mel(x, P, torch.float32)
    rep = F.Report("mel", good, ref, bound)
    assert rep.ok() and rep.excluded == 0, rep
    bad, _ = F.mel(x, P, torch.float32, shift=1)
    assert not F.Report("mel", bad, ref, bound).ok()
    sc, sb = F.mel_scale(good)
    assert F.Report("mel_scale", sc.float(), sc, sb).ok()
    sc_all, _ = F.mel_scale(good, None)
    sc_own, _ = F.mel_scale(good, [3, 2])   # a ragged row's scale over ALL frames instead of its own
    assert not F.Report("mel_scale", sc_all.float(), sc_own, sb).ok()


# ---- pad + normalise, post -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_raw", [1, 1023, 1025])
def test_pad_normalize_emulation_passes_and_biased_std_fails(T_raw):
    spec, sd, P = _params("PP16s")
    mix = synth_mix(spec, 2, T_raw) + 0.01
    t_raw = [T_raw, T_raw]
    Tp = T_raw + (spec.tot_ds - T_raw % spec.tot_ds)
    ref, bound, lens = F.pad_normalize(mix, t_raw, Tp, P.level, spec.tot_ds)
    good, _, _ = F.pad_normalize(mix, t_raw, Tp, P.level, spec.tot_ds, torch.float32)
    rep = F.Report("pad_normalize", good, ref, bound, lens)
    assert rep.ok() and rep.excluded == 0, rep
    bad, _, _ = F.pad_normalize(mix, t_raw, Tp, P.level, spec.tot_ds, torch.float32, std_den_off=0)
    assert not F.Report("pad_normalize", bad, ref, bound, lens).ok()
    shifted = torch.roll(good, 1, -1)  # placement one sample off
    assert not F.Report("pad_normalize", shifted, ref, bound, lens).ok()


def _post_fp32(x, mix, t_raw, pl, keep, always=False):
    """post_kernel's arithmetic: rms in double rounded to fp32, the rest in fp32."""
    out = torch.zeros(x.shape[0], 1, mix.shape[-1])
    for b in range(x.shape[0]):
        n = t_raw[b]
        v = x[b, 0, pl[b]: pl[b] + n].float()
        if keep:
            mr = mix[b].reshape(-1)[:n].double().pow(2).mean().sqrt().float()
            xr = v.double().pow(2).mean().sqrt().float().clamp(min=1e-5)
            v = v * (mr / xr)
        mx = v.abs().max()
        if mx > 1.0 or always:
            v = v / mx
        out[b, 0, :n] = v
    return out


@pytest.mark.parametrize("keep", [False, True])
def test_post_emulation_passes_and_unconditional_division_fails(keep):
    spec, sd, P = _params("PP16s")
    n, pl = 1025, 47
    x = _randn(2, 1, n + 2 * pl, seed=5, scale=0.05)
    mix = synth_mix(spec, 2, n)
    mix[1] *= 60.0     # with keep_rms the second row's peak is above 1: the guard divides there and only there
    if not keep:
        x[1] *= 40.0
    ref, bound, divided = F.post(x, mix, [n, n], [pl, pl], keep)
    assert divided == [False, True]
    rep = F.Report("post", _post_fp32(x, mix, [n, n], [pl, pl], keep), ref, bound)
    assert rep.ok() and rep.excluded == 0, rep
    rep = F.Report("post", _post_fp32(x, mix, [n, n], [pl, pl], keep, always=True), ref, bound)
    assert not rep.ok() and rep.worst["index"][0] == 0, rep


# ---- exact operations ----------------------------------------------------------------------------------------------------------
def test_exact_operations_hold_a_one_ulp_defect():
    x = _randn(2, 4, 66 * 5, seed=7)
    ref, bound = F.s2d(x, torch.tensor(0.25), 5)
    assert F.Report("s2d", ref.clone(), ref, bound).ok()
    bad = ref.clone()
    bad[1, 7, 65] = torch.nextafter(bad[1, 7, 65], torch.tensor(float("inf")))
    rep = F.Report("s2d", bad, ref, bound)
    assert not rep.ok() and rep.n_bad == 1 and rep.worst["index"] == [1, 7, 65], rep
    parts = [_randn(2, 8, 33, seed=10 + i) for i in range(5)]
    ref, bound = F.sum_scaled(parts, F.sum_scale_of(5))
    other = ((parts[4] + parts[3]) + (parts[2] + parts[1]) + parts[0]) * torch.tensor(F.sum_scale_of(5))  # another order
    assert F.Report("sum", ref.clone(), ref, bound).ok() and not F.Report("sum", other, ref, bound).ok()


# ---- FIR, sampler update -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [5, 7, 9, 11, 17])
def test_fir_emulation_passes_and_damages_fail(nt):
    """Both forms: pre (PReLU, no bias) and post (bias, residual).  Damages: one tap dropped at the last partial quad; the halo
    behind a row's end read from the neighbouring row instead of zero."""
    B, C, T = 2, 3, 1027
    x, res = _randn(B, C, T, seed=20), _randn(B, C, T, seed=21)
    taps = torch.tensor([math.comb(nt - 1, k) for k in range(nt)], dtype=torch.float64).div(2.0 ** (nt - 1)).float()
    bias = _randn(C, seed=22)
    for kw in (dict(alpha=0.2), dict(bias=bias, res=res, res_scale=F.INV_SQRT2)):
        ref, bound = F.fir(x, taps, **kw)
        good, _ = F.fir(x, taps, dtype=torch.float32, **kw)
        rep = F.Report("fir", good, ref, bound)
        assert rep.ok() and rep.excluded == 0, rep

        def drop(w):
            w = w.clone()
            w[:, :, T - 2, nt // 2 + 1] = 0   # sample T - 1 missing from the window of output T - 2 (quad 1024 .. 1026)
            return w

        def neighbour(w):
            w = w.clone()
            w[0, :, T - 1, nt // 2 + 1] = x[1, :, 0] if "alpha" not in kw else F.prelu(x[1, :, 0], torch.tensor(0.2))
            return w
        for hook, where in ((drop, T - 2), (neighbour, T - 1)):
            bad, _ = F.fir(x, taps, dtype=torch.float32, hook=hook, **kw)
            rep = F.Report("fir", bad, ref, bound)
            assert not rep.ok() and rep.worst["index"][2] == where, rep


def test_sampler_update_holds_a_wrong_coefficient_row():
    x, sc, z = _randn(3, 1, 64, seed=30), _randn(3, 1, 64, seed=31), _randn(3, 1, 64, seed=32)
    ref, bound = F.sampler_update(x, sc, 0.37, z, 0.11)
    good = (x + torch.tensor(0.37) * sc) + torch.tensor(0.11) * z
    assert F.Report("update", good, ref, bound).ok()
    bad = (x + torch.tensor(0.37) * sc) + torch.tensor(0.11).mul(1 + 2.0 ** -20) * z
    assert not F.Report("update", bad, ref, bound).ok()
    assert torch.equal(F.init_x(z, 0.5, x), x + z * 0.5)


def test_a_nan_bound_shows_as_excluded():
    ref = torch.ones(1, 1, 4, dtype=torch.float64)
    bound = torch.full((1, 1, 4), 1e-6, dtype=torch.float64)
    bound[0, 0, 2] = float("nan")
    rep = F.Report("nan", ref.float(), ref, bound)
    assert rep.excluded == 1 and not rep.ok()


# ---- coverage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.MODELS)
def test_cases_meet_every_reachable_edge_class(name, built_lib):
    """Per tap, on the tap's own time axis (samples per frame of its level from plan_json): what the case lists of the GPU file
    hit against what number theory says a call of up to MAX_FRAMES frames can reach."""
    spec, sd, P = _params(name)
    plan = json.loads(_lib.pack_weights(spec, sd)[1])
    for tap, (m, tile, halo, takes_lens) in F.kernel_axes(plan, spec).items():
        fam = F.family(tap)
        if fam == "fir" and name not in {mm for mm, _, _ in F.FIR_CASES}:
            # (PP16m is PP16s' topology at twice the width: same levels, same tap counts, same fir4_kernel launches per row;
            # OR16s has no anti-alias FIR)
            assert name in ("PP16m", "OR16s")
            continue
        hit = set()
        for group, cases in F.GROUPS.items():
            if fam in F.REPORTED[group]:
                for mm, B, frames in cases:
                    if mm == name:
                        hit |= F.classes_of(frames * m, tile, halo, B)
        for group, (cases, with_lens) in F.RAGGED_GROUPS.items():
            if fam in F.REPORTED[group]:
                for mm, rows in cases:
                    if mm == name:
                        hit |= F.classes_of(max(rows) * m, tile, halo, len(rows), ragged=with_lens and takes_lens)
                        # (f): a short row has to end inside a tile
                        assert tile == 1 or any((r * m) % tile for r in rows[1:]), (tap, "no short row ends inside a tile")
        reach = F.reachable_classes(m, tile, halo, takes_lens)
        if fam == "out_conv" and name not in {mm for mm, _ in F.RAGGED_STEP}:
            reach.discard("f")  # (the ragged step is warm-started from the Snake layer's wav: PP16s and PP24s have it)
        missing = reach - hit
        assert not missing, (name, tap, sorted(missing))


# ---- Snake, STFT ------------------------------------------------------------------------------------------------------------------
def test_snake_fp32_passes_and_a_lost_halo_sample_fails():
    spec = get_spec("PP16s")
    S_ = F.SnakeParams(S.synthetic_state_dict(spec, seed=0))
    aux = _randn(2, spec.score.n_channels, 257, seed=40, scale=0.3)
    ref = F.snake(aux, S_)
    r32 = F.snake(aux, S_, torch.float32)
    assert F.lib_report("snake", r32, ref, r32, 1).ok()

    def lost(u):  # the last up-sampled sample, which only the down filter's halo of the last output reads
        u = u.clone()
        u[:, :, -1] = 0
        return u
    rep = F.lib_report("snake", F.snake(aux, S_, torch.float32, hook=lost), ref, r32, F.M_CAP)
    assert not rep.ok() and rep.worst["index"][2] >= 250, rep


@pytest.mark.parametrize("case", F.STFT_CASES, ids=[c[0] for c in F.STFT_CASES])
def test_stft_fp32_passes_and_damages_fail(case):
    from open_universe_amd.layers.dyn_range_comp import get_window

    tag, N, hop, wn, kind, e, fac, T, B = case
    win = get_window(wn, N)
    x = _randn(B, T, seed=50)
    ref = F.stft_forward(x, win, N, hop, kind, e, fac)
    r32 = F.stft_forward(x, win, N, hop, kind, e, fac, torch.float32)
    assert F.lib_report("fwd", r32, ref, r32, 1).ok()
    assert not F.lib_report("fwd", F.stft_forward(x, win, N, hop, kind, e, fac, torch.float32, shift=1), ref, r32, F.M_CAP).ok()
    fr = F.stft_inverse_frames(r32, win, N, kind, e, fac)
    f32 = F.stft_inverse_frames(r32, win, N, kind, e, fac, torch.float32)
    assert F.lib_report("inv", f32, fr, f32, 1).ok()
    swapped = torch.cat([r32[:, N // 2 + 1:], r32[:, :N // 2 + 1]], 1)  # real / imaginary halves exchanged
    assert not F.lib_report("inv", F.stft_inverse_frames(swapped, win, N, kind, e, fac, torch.float32), fr, f32, F.M_CAP).ok()
    nf = fr.shape[1]
    length = (nf - 1) * hop + N - N // 2 + 3   # the last 3 samples lie behind every frame: envelope 0, exactly 0 expected
    y, bound = F.stft_overlap_add(f32, win, N, hop, length)
    assert bool((bound[:, -3:] == 0).all()) and bool((y[:, -3:] == 0).all())
    good = y.float()
    assert F.Report("ola", good, y, bound).ok()
    bad = good.clone()
    bad[:, -1] = 1e-9  # a division by a zero envelope let through
    assert not F.Report("ola", bad, y, bound).ok()
    one_off = torch.roll(good, 1, -1)
    assert not F.Report("ola", one_off, y, bound).ok()


def test_pad_and_post_lengths_meet_the_register_window_and_tile_edges():
    """pad_normalize / post: 1 024 threads, 64-sample register windows up to 65 536 samples, loops above."""
    hit = set()
    for n in F.PREPOST_T:
        hit |= F.classes_of(n, 1024, 1, 2)
    assert {"a", "b", "c", "d"} <= hit and 64 * 1024 in F.PREPOST_T and 64 * 1024 + 1 in F.PREPOST_T
