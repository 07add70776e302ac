"""GPU (-m gpu): the topologies of tests/offlist_cases.py -- configurations build_model accepts and no shipped model has -- loaded
through `load_model` from a config.yaml + checkpoint and held with the tools of the shipped topologies' harnesses, nothing new:

    element by element   one conditioner pass + one score pass under model.profile, option no_overlap = 1: the small kernels
                         (small_fp64: mel, mel_scale, both in-convs, s2d, sum, sigma_embed, film, out_conv OUT_SCORE), every body
                         conv (conv_fp64), every rate-change / 1x1 / mel conv (rate_fp64, paired with the variant code the launcher
                         chose) and the GRU (gru_fp64); the same under the option sets that give rate-change layers to another
                         family, where fuse_upfir = 0 with rate_small = 0 sends 13 / 15 taps through the scalar fir_kernel;
    a whole enhance      pad_normalize, post, and -- warm-started, UNIVERSE++ -- init_x and out_conv OUT_UPDATE;
    ragged               _enhance(t_raw=...), two steps, mask_fused 0 / 1: every tap inside the rows, exactly 0 behind them;
    end to end           enhance against oracle.restatement.enhance in float64 (helpers.record, 60 dB), a row alone against the
                         row in a batch, enhance_long of one window against enhance.

Bound kinds and constants are those of small_fp64 / conv_fp64 / rate_fp64 / gru_fp64; `excluded == 0` everywhere.  Which family took
which rate-change / 1x1 layer is recorded per case in tests/golden/offlist_variants.json (from an MI355X) and asserted.  Every case
logs its figures to build/observed/offlist_observed.json (untracked) before it asserts; profiles/offlist_observed.json is the
committed copy.

Measured on an MI355X (worst err / bound): small kernels chain 0.53, statistic 0.68, exact 0, embedding err / e32 1.00 (simple, D 64
and 1024) and 2.18 (random Fourier features, n_rff 16: under M_EMBED_RFF = 5, which stays); body convs chain 0.36, minimal filtering
0.06; rate-change / 1x1 convs chain 0.29, down_fir 0.05 and up_fir 0.03 (rate_down_kernel / rate_up_kernel at T % 4 == 2, case r27:
the only off-list model they are built for); GRU err / e32 5.0; ragged tails all exactly 0; end to end 106 .. 121 dB; at
most 1.2 s per case."""
import json
import os
import time

import pytest
import torch
import yaml

import conv_fp64 as CF
import gru_fp64 as G
import offlist_cases as K
import rate_fp64 as R
import restatement as O
import small_fp64 as F
from helpers import record, synth_mix
from open_universe_amd import _lib, inference_utils
from open_universe_amd import variants as V
from test_gpu_conv_fp64 import _check_blocks, _last_pass, _pair_with_profile
from test_gpu_parity import noise_list, run_enhance
from test_gpu_rate_fp64 import _check as _check_rate
from test_gpu_rate_fp64 import _flops_of, _poison
from test_gpu_small_fp64 import _condition_reports

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_OUT = os.path.join(os.path.dirname(_HERE), "build", "observed")
_GOLDEN = os.path.join(_HERE, "golden", "offlist_variants.json")
_models, _params = {}, {}
# option sets that pick another family for rate-change layers (rate_fp64.FAMILIES)
OPTION_SETS = {"lds": dict(conv_direct=0), "gen1": dict(conv_direct=3), "rate_small0": dict(rate_small=0), "d4_fir0": dict(d4_fir=0),
               "fuse_upfir0": dict(fuse_upfir=0), "fir_passes": dict(fuse_upfir=0, rate_small=0)}


def get_model(case, tmp_path_factory):
    """(model, spec, sd): built once per case, the way a user's checkpoint arrives."""
    if case not in _models:
        d = tmp_path_factory.mktemp("offlist_" + case)
        with open(d / "config.yaml", "w") as f:
            yaml.safe_dump(K.config_of(case), f)
        sd = K.state_dict_of(case)
        torch.save({"state_dict": sd}, d / "weights.ckpt")
        model = inference_utils.load_model(d / "weights.ckpt", device="cuda:0")
        assert model.spec.to_dict() == K.spec_of(case).to_dict()
        _models[case] = (model, model.spec, sd)
    return _models[case]


def _P(case, spec, sd):
    """The rebuilt parameters of all four harnesses, held once per case against the blob the library packs for it."""
    if case not in _params:
        blob, plan = _lib.pack_weights(spec, sd)
        plan = json.loads(plan)
        Ps, Pc, Pr = F.Params(spec, sd), CF.ConvParams(spec, sd), R.RateParams(spec, sd)
        for P in (Ps, Pc, Pr):
            P.check_against_blob(blob, plan)
        gru = (G.Layer(sd, "condition_model.encoder.gru", 0), G.Layer(sd, "condition_model.encoder.gru", 1),
               G.Layer(sd, spec.score_prefix + ".encoder.gru", 0))
        _params[case] = (Ps, Pc, Pr, gru, {c["name"]: c for c in plan["convs"]}, blob)
    return _params[case]


def _tap(model, name):
    return model.tensor(name).cpu().clone()


def _has(model, name):
    try:
        model.tensor(name)
        return True
    except KeyError:
        return False


def _kind_of_small(key):
    if key in ("sigma_embed",):
        return "library"
    if key.startswith(("s2d", "enc_sum", "init_x")):
        return "exact"
    if key.startswith(("pad_normalize", "post", "mel_scale")):
        return "statistic"
    return "chain"


def _log(case, rec):
    os.makedirs(_OUT, exist_ok=True)
    path = os.path.join(_OUT, "offlist_observed.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[case] = rec
    with open(path, "w") as f:  # one line per case
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(old.items())) + "\n}\n")


def _finish(case, t0, small=None, conv=None, rate=None, gru=None, ran_rate=None, ran_conv=None, extra=None):
    """Log, print, then assert.  small: {key: small_fp64.Report}; conv / rate: {'tap|kind|variant': Report}; gru: {key: gru_fp64.Report}."""
    small, conv, rate, gru = small or {}, conv or {}, rate or {}, gru or {}
    worst, counts = {}, {"taps": 0, "checked": 0, "excluded": 0, "bad": 0, "tail_bad": 0}
    every = [(_kind_of_small(k), k, r) for k, r in small.items()]
    every += [("conv." + k.split("|")[1], k, r) for k, r in conv.items()] + [("rate." + k.split("|")[1], k, r) for k, r in rate.items()]
    for kind, k, r in every:
        if r.ratio >= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (round(r.ratio, 4), k)
        counts["taps"] += 1
        counts["checked"] += r.checked
        counts["excluded"] += r.excluded
        counts["bad"] += r.n_bad
        counts["tail_bad"] += r.tail_bad
    fams = {}
    for fam, *layer in ran_rate or []:
        fams.setdefault(fam, set()).add(tuple(layer))
    fams = {f: [list(v) for v in sorted(s)] for f, s in fams.items()}
    body = {}
    for p, cv, cfg, Cc, KW in ran_conv or []:
        body.setdefault(CF.family_of(cfg), set()).add((Cc, KW))
    rec = {"seconds": round(time.time() - t0, 2), "worst": {k: list(v) for k, v in worst.items()}, "counts": counts,
           "families": fams, "body_families": {f: sorted(v) for f, v in body.items()}}
    if "sigma_embed" in small:
        rec["sigma_embed"] = {"e32": small["sigma_embed"].e32, "lib_ratio": round(small["sigma_embed"].lib_ratio, 3)}
    if gru:
        rec["gru"] = {k: round(r.ratio, 3) for k, r in gru.items()}
    rec.update(extra or {})
    log_error = None
    try:
        _log(case, rec)
    except OSError as e:
        log_error = e
    print(f"{case}: {rec}")
    for kind, k, r in every:
        if not r.ok():
            print(f"{case} {k} {r}")
    for kind, k, r in every:
        assert r.excluded == 0 and r.ok(), f"{case} {k} {r}"
        if hasattr(r, "lib_ratio"):
            assert r.lib_ratio <= F.M_CAP, f"{case} {k}: err / e32 = {r.lib_ratio:.2f} is a finding, not a tolerance"
    for k, r in gru.items():
        assert r.excluded == 0 and r.ok(), f"{case} {k} {r}"
        assert r.ratio <= G.M_CAP, f"{case} {k}: err / e32 = {r.ratio:.2f} is a finding, not a tolerance -- {r}"
    if ran_rate is not None:
        # which family took which layer: as recorded on an MI355X, every family, every layer
        with open(_GOLDEN) as f:
            expected = json.load(f).get(case)
        assert expected is not None, (case, "no recorded layers for this case")
        for fam in sorted(set(fams) | set(expected)):
            assert fams.get(fam, []) == expected.get(fam, []), (case, fam, "took", fams.get(fam, []), "recorded", expected.get(fam, []))
    assert log_error is None, f"{case}: could not write the observed figures: {log_error}"
    return rec


def _gru_reports(model, spec, gru, lens=None, ragged=False):
    reps = {}

    def layer(tag, L, x, gx, out, res):
        reps[tag + ".proj"] = G.check_projection(L, x, gx, lens, ragged)
        reps[tag + ".step"] = G.check_step(L, gx, out, lens, res)
    cb1, g0 = _tap(model, "cond.cb1.v"), _tap(model, "cond.gru0")
    layer("cond.gru0", gru[0], cb1, _tap(model, "cond.gru0.gx"), g0, None)
    layer("cond.gru", gru[1], g0, _tap(model, "cond.gru.gx"), _tap(model, "cond.gru"), cb1 if spec.cond.encoder_gru_residual else None)
    last = len(spec.score.rate_factors) + int(spec.score.extra_conv_block) - 1
    x = _tap(model, f"score.enc{last}.v" if spec.score.extra_conv_block else f"score.enc{last}.h")
    layer("score.gru", gru[2], x, _tap(model, "score.gru.gx"), _tap(model, "score.gru"), x if spec.score.extra_conv_block else None)
    return reps


def _score_reports(small, model, spec, Ps, xs, sig, score):
    B = xs.shape[0]
    coef = F.edm_coef(spec, sig)
    ref, bound = F.in_conv(xs, Ps.s_in_w, Ps.s_in_b, coef["w_in"] if Ps.edm else None)
    small["score.in"] = F.Report("score.in", _tap(model, "score.in"), ref, bound)
    g = _tap(model, "sigma.g")
    small["sigma_embed"] = F.check_sigma_embed(g, coef["sigma_net"], Ps)
    ref, bound = F.film(g, Ps.film_w, Ps.film_b)
    small["film"] = F.Report("film", _tap(model, "sigma.film"), ref.reshape(B, -1, 1), bound)
    last = len(spec.score.rate_factors) + int(spec.score.extra_conv_block) - 1
    ref, bound = F.out_conv_score(_tap(model, f"score.dec{last}.v"), xs, Ps, coef)
    small["out_conv"] = F.Report("out_conv", score, ref, bound)


def _fir_reports(small, model, spec, Pr, convs, blob, lens_of=None):
    """Both stand-alone FIR passes of the score network ({blk}.v -> {blk}.fir; {blk}.upc, residual -> {blk}.up) where they ran."""
    seen = set()
    for key, rl in Pr.rate.items():
        if not key.startswith("score.") or not rl.aa:
            continue
        c = convs[rl.name]
        taps = blob[c["fir_off"]: c["fir_off"] + c["fir_len"]]
        if not rl.up and _has(model, key + ".fir"):
            ref, bound = F.fir(_tap(model, Pr.src[key]), taps, alpha=blob[c["a_off"]])
            # ({blk}.fir is not masked behind the rows: the whole buffer against the reference of the whole buffer)
            small[f"fir.down.{key}.nt{c['fir_len']}"] = F.Report(key + ".fir", _tap(model, key + ".fir"), ref, bound)
            seen.add(("down", c["fir_len"]))
        if rl.up and _has(model, key + ".upc"):
            upc = _tap(model, key + ".upc")
            if bool((upc == 12345.0).all()):
                continue  # (the sentinel of test_gpu_rate_fp64._poison: not written, the fused form ran)
            bias = blob[c["fbias_off"]: c["fbias_off"] + c["Cout"]]
            ref, bound = F.fir(upc, taps, bias=bias, res=_tap(model, Pr.res[key]), res_scale=F.INV_SQRT2)
            lens = None if lens_of is None else lens_of(upc.shape[-1])
            small[f"fir.up.{key}.nt{c['fir_len']}"] = F.Report(key + ".up", _tap(model, key + ".up"), ref, bound, lens)
            seen.add(("up", c["fir_len"]))
    return seen


def _passes(case, B, frames, steer, opts, tmp_path_factory, tag):
    t0 = time.time()
    steer.set(no_overlap=1, **opts)
    model, spec, sd = get_model(case, tmp_path_factory)
    model.reset_workspace()
    try:
        Ps, Pc, Pr, gru, convs, blob = _P(case, spec, sd)
        T = spec.tot_ds * frames
        xin = O.normalize(synth_mix(spec, B, T, seed=5100 + frames)[:, None, :], spec.level_db).float().contiguous()
        sig = torch.tensor([0.3, 1.7, 0.05])[:B]
        xs = (torch.randn(xin.shape, generator=torch.Generator().manual_seed(11 + frames)) * sig[:, None, None]).float().contiguous()
        for profiled in (False, True):  # two identical passes, the sentinel in every {blk}.upc between them
            model.profile(profiled)
            model.condition_model(xin.cuda(), train=True)
            score = model.score_model(xs.cuda(), sig).cpu()
            if not profiled:
                _poison(model, Pr)
        records = model.profile_read(32768)
        model.profile(False)
        small, conv, rate = {}, {}, {}
        _condition_reports(small, model, spec, Ps, xin)
        _score_reports(small, model, spec, Ps, xs, sig, score)
        seen = _fir_reports(small, model, spec, Pr, convs, blob)
        T_of = {p: model.tensor(vn).shape[-1] for p, q, i, f, a, c1n, vn, ex in Pc.walk}
        ran_conv = _check_blocks(conv, Pc, model, _pair_with_profile(Pc, records, B, T_of), True, _tap(model, "sigma.film"))
        paired = R.pair_walk(Pr.slots, records, _flops_of(Pr, convs, model, B))
        ran_rate = []
        _check_rate(rate, ran_rate, Pr, convs, model, paired, 0)
        g = _gru_reports(model, spec, gru)
        name = f"{tag}.{case}.b{B}.f{frames}"
        _finish(name, t0, small, conv, rate, g, ran_rate, ran_conv, extra={"fir_passes": sorted(f"{d}{n}" for d, n in seen)})
        return seen, ran_rate, small
    finally:
        model.profile(False)
        model.reset_workspace()


@pytest.mark.parametrize("frames,B", K.SHAPES)
@pytest.mark.parametrize("case", list(K.CASES))
def test_element_by_element(case, frames, B, steer, tmp_path_factory):
    seen, ran, small = _passes(case, B, frames, steer, {}, tmp_path_factory, "seams")
    spec = K.spec_of(case)
    n = len(spec.score.rate_factors)
    assert sum(1 for k in small if k.startswith("s2d")) == n - 1  # (sum_kernel: the mel block, n - 1 st convs, the encoder's output)
    # every rate-change layer of both networks and every st / sc / mel conv is in the record
    assert len(ran) == 4 * n + (n - 1) + (n + int(spec.score.extra_conv_block)) + 1, ran
    if case in K.RATE_SMALL:
        # both networks' outermost level, with the FIR (score) and without (conditioner), on rows of 2 modulo 4 samples
        took = {(fam, cls) for fam, cls, *_ in ran if fam in ("rate_down", "rate_up")}
        assert took == {("rate_down", "down"), ("rate_up", "up")} and (frames * spec.tot_ds) % 4 == 2, took
        assert sum(1 for fam, *_ in ran if fam in ("rate_down", "rate_up")) == 4, ran
    if spec.tot_ds % 4:
        assert small["out_conv"].checked == B * frames * spec.tot_ds and (frames * spec.tot_ds) % 4 != 0


@pytest.mark.parametrize("tag", list(OPTION_SETS))
@pytest.mark.parametrize("case", K.OPTION_CASES)
def test_element_by_element_under_other_families(case, tag, steer, tmp_path_factory):
    seen, ran, small = _passes(case, 3, 13, steer, OPTION_SETS[tag], tmp_path_factory, tag)
    spec = K.spec_of(case)
    fams = {fam for fam, *_ in ran}
    if tag == "fir_passes":
        # Every anti-aliased layer of the score network ran as a conv WITHOUT its filter -- from the profile: the variant code
        # paired with the layer names no fused family (_check_rate's classes `down.after_fir` / `up.unfused`) -- and the
        # stand-alone pass beside it wrote its tap.  The profile carries no record of the FIR launches themselves (prof_open
        # brackets convs and recurrences only), so WHICH of launch_fir's kernels ran follows from the tap count: 13 and 15 have
        # no fir4_kernel instantiation (offlist_cases.FIR4_TAPS restates launch_fir's switch).
        want = {(d, 2 * r + 1) for r in spec.score.rate_factors for d in ("down", "up")}
        assert seen == want, (seen, want)
        scalar = {nt for d, nt in seen if nt not in K.FIR4_TAPS}
        assert scalar == {2 * r + 1 for r in spec.score.rate_factors if r in (6, 7)} and scalar and scalar <= {13, 15}, scalar
        n = len(spec.score.rate_factors)
        classes = sorted((cls, r) for fam, cls, ci, co, r in ran if cls in ("down.after_fir", "up.unfused"))
        assert classes == sorted([("down.after_fir", r) for r in spec.score.rate_factors] + [("up.unfused", r) for r in spec.score.rate_factors]), classes
        assert not fams & {"rate_down", "rate_up"}, fams
    if case in K.RATE_SMALL:
        # rate_down_kernel / rate_up_kernel take the outermost level by default (T % 4 == 2: rate_up_kernel's scalar store loop,
        # rate_down_kernel's rows 8 bytes off a 16-byte boundary) and decline under rate_small = 0
        small = "rate_small" in OPTION_SETS[tag] and OPTION_SETS[tag]["rate_small"] == 0
        assert ({"rate_down", "rate_up"} <= fams) == (not small) and bool({"rate_down", "rate_up"} & fams) == (not small), (tag, fams)
        assert (13 * spec.tot_ds) % 4 == 2


@pytest.mark.parametrize("case", list(K.CASES))
def test_whole_enhance_taps(case, tmp_path_factory):
    """T_raw = 13 frames - 3, batch 3, keep_rms: pad_normalize and post; UNIVERSE++ warm-started (one step from x0 = wav + sigma
    noise): init_x through score.in, out_conv OUT_UPDATE in tap x."""
    t0 = time.time()
    model, spec, sd = get_model(case, tmp_path_factory)
    Ps = _P(case, spec, sd)[0]
    td, B = spec.tot_ds, 3
    T_raw, T = 13 * td - 3, 13 * td
    mix = synth_mix(spec, B, T_raw, seed=71) + 0.01
    warm = spec.use_signal_decoupling
    noise = noise_list(29, 1 if warm else 2, B, T)
    out = run_enhance(model, mix, noise, n_steps=2, keep_rms=True, warm_start=1 if warm else None)
    small = {}
    ref, bound, lens = F.pad_normalize(mix, [T_raw] * B, T, Ps.level, td)
    small["pad_normalize"] = F.Report("pad_normalize", _tap(model, "mixn"), ref, bound)
    pl = (T - T_raw) // 2
    ref, bound, _ = F.post(_tap(model, "x"), mix[:, None, :], [T_raw] * B, [pl] * B, True)
    small["post"] = F.Report("post", out.reshape(B, 1, -1), ref, bound)
    if warm:
        sigma = float(model._sigma_table(2)[1])
        coef = F.edm_coef(spec, [sigma] * B)
        x0 = F.init_x(noise[0], sigma, _tap(model, "wav"))
        ref, bound = F.in_conv(x0, Ps.s_in_w, Ps.s_in_b, coef["w_in"] if Ps.edm else None)
        small["score.in"] = F.Report("score.in(init_x)", _tap(model, "score.in"), ref, bound)
        last = len(spec.score.rate_factors) + int(spec.score.extra_conv_block) - 1
        score, sb = F.out_conv_score(_tap(model, f"score.dec{last}.v"), x0, Ps, coef)
        ref, bound = F.sampler_update(x0, score, float(coef["sig2"][0]), score_bound=sb)
        small["out_conv.update"] = F.Report("out_conv.update", _tap(model, "x"), ref, bound)
    _finish(f"enhance.{case}", t0, small)
    model.reset_workspace()


@pytest.mark.parametrize("mask_fused", [0, 1])
@pytest.mark.parametrize("case", K.RAGGED)
def test_ragged(case, mask_fused, steer, tmp_path_factory):
    t0 = time.time()
    steer.set(mask_fused=mask_fused, no_overlap=1)
    model, spec, sd = get_model(case, tmp_path_factory)
    model.reset_workspace()
    try:
        Ps, Pc, Pr, gru, convs, blob = _P(case, spec, sd)
        td, rows = spec.tot_ds, K.RAGGED_ROWS
        t_raw = [f * td - 3 for f in rows]
        B, lm, T = len(rows), max(t_raw), max(rows) * td
        sigs = [synth_mix(spec, 1, n, seed=800 + i)[0] for i, n in enumerate(t_raw)]
        mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs])[:, None, :]
        nz = torch.zeros(2, B, 1, T)
        for b in range(B):
            nz[:, b, 0, :rows[b] * td] = torch.randn(2, rows[b] * td, generator=torch.Generator().manual_seed(880 + b))
        for profiled in (False, True):
            model.profile(profiled)
            out = model._enhance(mix.cuda(), 2, None, None, None, None, False, True, None, "median", None, nz.cuda(), t_raw=list(t_raw)).cpu()
            if not profiled:
                _poison(model, Pr)
        records = model.profile_read(32768)
        model.profile(False)
        small, conv, rate = {}, {}, {}
        ref, bound, lens_T = F.pad_normalize(mix, t_raw, T, Ps.level, td)
        assert lens_T == [f * td for f in rows]
        mixn = _tap(model, "mixn")
        small["pad_normalize_var"] = F.Report("pad_normalize_var", mixn, ref, bound, lens_T)
        _condition_reports(small, model, spec, Ps, mixn, lens_T, list(rows))
        pl = [(td - n % td) // 2 for n in t_raw]
        ref, bound, _ = F.post(_tap(model, "x"), mix, t_raw, pl, True)
        small["post_var"] = F.Report("post_var", out, ref, bound, t_raw)
        lens_of = lambda Tl: [f * (Tl // max(rows)) for f in rows]
        _fir_reports(small, model, spec, Pr, convs, blob, lens_of)
        T_of = {p: model.tensor(vn).shape[-1] for p, q, i, f, a, c1n, vn, ex in Pc.walk}
        n_cond = sum(1 for p, *_ in Pc.walk if p.startswith("cond."))
        full = Pc.walk
        try:  # the conditioner ran once, the score network twice: its blocks are paired from the records of the last pass
            Pc.walk = full[:n_cond]
            paired = _pair_with_profile(Pc, records, B, T_of)
            Pc.walk = full[n_cond:]
            paired.update(_pair_with_profile(Pc, _last_pass(records), B, T_of))
        finally:
            Pc.walk = full
        film = _tap(model, "sigma.film")[1:2].expand(B, -1, -1)
        ran_conv = _check_blocks(conv, Pc, model, paired, True, film, lens_of)
        ran_rate = []
        _check_rate(rate, ran_rate, Pr, convs, model, R.pair_walk(Pr.slots, records, _flops_of(Pr, convs, model, B), score_passes=2), 1, lens_of)
        for k, r in list(small.items()) + list(conv.items()) + list(rate.items()):
            assert r.tail_bad == 0, f"{k}: {r.tail_bad} nonzero elements behind a row's end"
        g = _gru_reports(model, spec, gru, lens=list(rows), ragged=True)
        _finish(f"ragged.mask_fused{mask_fused}.{case}", t0, small, conv, rate, g, ran_rate, ran_conv)
    finally:
        model.profile(False)
        model.reset_workspace()


@pytest.mark.parametrize("case", list(K.CASES))
def test_enhance_against_the_float64_restatement(case, tmp_path_factory):
    """4 steps, B = 2, 13 frames (T_raw = 13 tot_ds - 3) against oracle.restatement.enhance in float64 from the same (spec, sd,
    noise) at the project's 60 dB floor; enhance_long of one window is enhance, bit for bit.  A row enhanced alone against the same
    row in the batch: at 100 dB through helpers.record, not at equality -- the launcher picks its families by batch size (batch 1:
    conv_direct4_kernel, batch 2: conv_mfma_kernel for most layers of these models), so the two runs sum in different orders;
    100 dB is the floor test_gpu_parity.test_batch_independence_and_rank_conventions holds the shipped models to (observed here:
    127 .. 138 dB)."""
    t0 = time.time()
    model, spec, sd = get_model(case, tmp_path_factory)
    td, B, N = spec.tot_ds, 2, 4
    T_raw, T = 13 * td - 3, 13 * td
    mix = synth_mix(spec, B, T_raw, seed=91)
    nz = noise_list(31, N, B, T)
    out = run_enhance(model, mix, nz, n_steps=N)
    assert out.shape == mix.shape and bool(torch.isfinite(out).all())
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    ref = O.enhance(sd64, spec.to_dict(), mix.double(), n_steps=N, noise=[z.double() for z in nz])
    assert ref.dtype == torch.float64
    v = O.si_sdr(ref, out)
    alone = [O.si_sdr(out[b], run_enhance(model, mix[b], [z[b:b + 1] for z in nz], n_steps=N)) for b in range(B)]
    log_error = None
    try:
        _log(f"end_to_end.{case}", {"seconds": round(time.time() - t0, 2), "si_sdr": round(float(v), 2), "snr": round(float(v.snr), 2),
                                     "row_alone_db": [round(float(a), 2) for a in alone]})
    except OSError as e:  # (the test fails for it behind its own assertions)
        log_error = e
    print(f"end_to_end.{case}: SI-SDR {float(v):.2f} dB, SNR {float(v.snr):.2f} dB, rows alone {[round(float(a), 2) for a in alone]}")
    record(f"offlist.{case}.restatement", v)
    for b, a in enumerate(alone):
        record(f"offlist.{case}.row_alone.{b}", a, 100)
    x = mix[0].cuda()
    a = model.enhance(x, n_steps=N, rng=torch.Generator(device="cuda").manual_seed(5))
    b = model.enhance_long(x, n_steps=N, rng=torch.Generator(device="cuda").manual_seed(5))
    assert torch.equal(a, b)
    model.reset_workspace()
    assert log_error is None, f"end_to_end.{case}: could not write the observed figures: {log_error}"
