"""GPU (-m gpu): score networks with a conv sandwich round the GRU (encoder_gru_conv_sandwich) or with no GRU (seq_model: none) --
the cases of tests/seqmodel_cases.py, loaded through `load_model` from a config.yaml + checkpoint.

    against the reference   enhance (plain, warm-started where the model has an aux signal), three files alone and together through
                            enhance_many, against recordings of the REAL reference (tests/golden/seqmodel_<case>.npz) at the
                            project's end-to-end floor, 60 dB through helpers.record; the stored self_db of the case (the reference in
                            fp32 against itself in float64) has to clear that floor first;
    element by element      one conditioner pass + one score pass under model.profile, no_overlap = 1: every body conv of both
                            networks with conv_fp64 -- the walk of conv_fp64.blocks_of with score.cb1 / score.cb2 put where
                            run_score_enc runs them, paired with the variant the launcher chose --, score.gru with gru_fp64 fed the
                            library's own score.cb1 output, and the input of decoder block 0: with extra_conv_block the tap
                            score.dec0.in = (score.cb2 or the encoder's output + residual) / sqrt(2) as small_fp64.sum_scaled
                            defines it (kind `exact`), computed from score.cb2 and never from score.gru; without, decoder block 0
                            is an up block that reads score.cb2.v / the encoder's output in place (no tap of its own: asserted
                            absent; its up conv is held end to end by the goldens only);
                            sand_snake: conv_fp64 has no Snake form, so of its bottleneck blocks conv3 is held, reading the
                            block's activated plane, and that plane against snake_fp64.snake_act;
    ragged                  _enhance(t_raw=...), rows of 13, 4 and 1 frames - 3 samples, two steps, mask_fused 0 / 1: the bottleneck's
                            taps inside the rows, exactly 0 behind them (the input of conv_block2 in particular), the bottleneck
                            convs with their per-row bounds, a row alone against the row in the batch at 100 dB;
    entry points (sand_pp)  one small call each against what the existing test of that entry point holds it to.

`excluded == 0` everywhere.  Every case logs its figures to build/observed/seqmodel_observed.json (untracked) before it asserts;
profiles/seqmodel_observed.json is the committed copy from an MI355X.

Measured on an MI355X (profiles/seqmodel_observed.json): against the reference 108.2 .. 129.1 dB (the reference against itself in
float64: 98.7 .. 121.6 dB); worst err / bound of the body convs chain 0.42, minimal filtering 0.11, fused 0.008; score.dec0.in exact
(0); Snake plane 2.8e-7 of the allowed 1.0e-4; GRU err / e32 4.1 (step), 0.71 (projection); ragged tails all exactly 0, a row alone
108.8 .. 159.5 dB; enhance_long_many 120.4 dB, shared against unshared ensemble members 119.8 dB; 31 cases in 7 s."""
import json
import os
import time

import pytest
import torch
import yaml

import conv_fp64 as CF
import gru_fp64 as G
import restatement as O
import seqmodel_cases as K
import small_fp64 as F
import snake_fp64 as SF
from helpers import record, synth_mix
from open_universe_amd import _lib, inference_utils
from open_universe_amd import universe as U
from open_universe_amd.noise import CounterNoise
from test_gpu_conv_fp64 import _check_blocks, _last_pass, _pair_with_profile

pytestmark = pytest.mark.gpu

FLOOR = 60.0
_HERE = os.path.dirname(os.path.abspath(__file__))
_OUT = os.path.join(os.path.dirname(_HERE), "build", "observed")
_models, _params = {}, {}


def get_model(case, tmp_path_factory):
    """(model, spec, sd): built once per case, the way a user's checkpoint arrives."""
    if case not in _models:
        d = tmp_path_factory.mktemp("seqmodel_" + case)
        with open(d / "config.yaml", "w") as f:
            yaml.safe_dump(K.config_of(case), f)
        sd = K.state_dict_of(case)
        torch.save({"state_dict": sd}, d / "weights.ckpt")
        model = inference_utils.load_model(d / "weights.ckpt", device="cuda:0")
        assert model.spec.to_dict() == K.spec_of(case).to_dict()
        _models[case] = (model, model.spec, sd)
    return _models[case]


def _log(case, rec):
    os.makedirs(_OUT, exist_ok=True)
    path = os.path.join(_OUT, "seqmodel_observed.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[case] = rec
    with open(path, "w") as f:  # one line per case
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(old.items())) + "\n}\n")


def _tap(model, name):
    return model.tensor(name).cpu().clone()


def _has(model, name):
    try:
        model.tensor(name)
        return True
    except KeyError:
        return False


def _enhance(model, mix, noise, n_steps=K.N_STEPS, warm_start=None, keep_rms=False, t_raw=None):
    """model._enhance on a given noise tensor (n, B, 1, T_pad) -- the arguments of `enhance` plus the noise."""
    return model._enhance(mix.cuda(), n_steps, None, None, None, None, False, keep_rms, None, "median", warm_start, noise.cuda(),
                          t_raw=t_raw).cpu()


def _n_blocks(spec):
    return len(spec.score.rate_factors) + int(spec.score.extra_conv_block)


def _enc_out(spec):
    """Tap of the score encoder's output (what the bottleneck reads)."""
    last = _n_blocks(spec) - 1
    return f"score.enc{last}.v" if spec.score.extra_conv_block else f"score.enc{last}.h"


def _conv_params(case, spec, sd):
    """conv_fp64.ConvParams with the walk this model runs: score.cb1 / score.cb2 behind the score encoder, decoder block 0 reading
    what run_score_dec hands it.  sand_snake: conv_fp64 knows PReLU layers only; its Snake layers get a slope that is never
    applied (they are paired by their FLOPs, and only conv3 of the bottleneck blocks is held, with its activation off)."""
    if case in _params:
        return _params[case]
    s, sp = spec.score, spec.score_prefix
    sd_c = dict(sd)
    snake = [k[: -len(".prelu.act.act.alpha")] for k in sd if k.endswith(".prelu.act.act.alpha") and not k.startswith("signal_")]
    for p in snake:
        sd_c[p + ".prelu.weight"] = torch.ones(1)
    Pc = CF.ConvParams(spec, sd_c)
    sand = s.seq_model == "gru" and s.encoder_gru_conv_sandwich
    walk = []
    for e in Pc.walk:
        p, q, inp, fidx, add, c1n, vn, ex = e
        if p == "score.dec0":
            if sand:
                for b, src in ((1, _enc_out(spec)), (2, "score.gru")):
                    walk.append((f"score.cb{b}", f"{sp}.encoder.conv_block{b}", src, None, None, f"score.cb{b}.c1", f"score.cb{b}.v", False))
                    Pc.blocks[f"score.cb{b}"] = CF.BlockP(sd_c, f"{sp}.encoder.conv_block{b}")
            if inp is not None:  # (extra_conv_block: a block without a rate change, reading the un-fused residual sum)
                inp = "score.dec0.in"
            e = (p, q, inp, fidx, add, c1n, vn, ex)
        walk.append(e)
    Pc.walk = walk
    if not snake:
        blob, plan = _lib.pack_weights(spec, sd)
        plan = json.loads(plan)
        Pc.check_against_blob(blob, plan)  # (walks Pc.blocks: the two new blocks included)
        if sand:
            assert all(f"{sp}.encoder.conv_block{b}.conv{i}" in {c["name"] for c in plan["convs"]} for b in (1, 2) for i in (1, 2, 3))
    _params[case] = (Pc, set(snake))
    return _params[case]


def _summary(reps):
    worst = {}
    for k, r in reps.items():
        kind = k.split("|")[1] if "|" in k else "other"
        if r.ratio >= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (round(float(r.ratio), 4), k)
    return {k: list(v) for k, v in worst.items()}


def _assert_reports(case, reps):
    for k, r in reps.items():
        if not r.ok():
            print(f"{case} {k} {r}")
    for k, r in reps.items():
        assert r.excluded == 0 and r.ok(), f"{case} {k} {r}"
        if hasattr(r, "lib_ratio"):
            assert r.lib_ratio <= F.M_CAP, f"{case} {k}: err / e32 = {r.lib_ratio:.2f} is a finding, not a tolerance"


def _bottleneck_reports(case, model, spec, sd, records, B, lens_of=None, lens_frames=None, ragged=False):
    """-> (conv reports, gru reports, exact reports) of the bottleneck and of every other body conv conv_fp64 can hold."""
    Pc, snake = _conv_params(case, spec, sd)
    s, sp = spec.score, spec.score_prefix
    sand = s.seq_model == "gru" and s.encoder_gru_conv_sandwich
    T_of = {p: model.tensor(vn).shape[-1] for p, q, i, f, a, c1n, vn, ex in Pc.walk}
    full = Pc.walk
    if not ragged:
        paired = _pair_with_profile(Pc, records, B, T_of)
    else:  # the conditioner ran once, the score network once per step: its blocks are paired from the records of the last pass
        n_cond = sum(1 for p, *_ in full if p.startswith("cond."))
        try:
            Pc.walk = full[:n_cond]
            paired = _pair_with_profile(Pc, records, B, T_of)
            Pc.walk = full[n_cond:]
            paired.update(_pair_with_profile(Pc, _last_score_pass(records, s.seq_model == "gru"), B, T_of))
        finally:
            Pc.walk = full
    conv, gru, exact = {}, {}, {}
    film = _tap(model, "sigma.film")
    if ragged:
        film = film[1:2].expand(B, -1, -1)
    try:
        # Snake blocks: held below by hand; everything else through the shared checker
        Pc.walk = [e for e in full if not any(q.startswith(e[1] + ".") for q in snake)]
        _check_blocks(conv, Pc, model, paired, True, film, lens_of)
    finally:
        Pc.walk = full
    for b in (1, 2):
        p = f"score.cb{b}"
        if not sand or not any(q.startswith(f"{sp}.encoder.conv_block{b}.") for q in snake):
            continue
        depth, cfgs = paired[p]
        assert depth == 0 and len(cfgs) == 3, (p, "a Snake block takes no fused body", depth)
        hu, c2, act, v = _tap(model, _enc_out(spec) if b == 1 else "score.gru"), _tap(model, p + ".c2"), _tap(model, p + ".act"), _tap(model, p + ".v")
        lens = None if lens_of is None else lens_of(hu.shape[-1])
        # the plane holds what the block's last Snake launch wrote: the activated input of conv3
        al = torch.exp(sd[f"{sp}.encoder.conv_block{b}.conv3.prelu.act.act.alpha"]).numpy()
        want = torch.from_numpy(SF.snake_act(c2.numpy(), al, None, lens))
        rel = SF.rel_error(act.numpy(), want.numpy())
        lim = SF.KERNEL_FACTOR * SF.ref_error()["max_rel"]
        exact[f"{p}.act|snake_rel"] = (rel, lim)
        kind = CF.kind_of(cfgs[2])
        ref, bound, ex = CF.body_conv(act, Pc.blocks[p].c[2], CF.Epi(act=False, res=hu), kind, lens)
        key = f"{p}.v|{kind}|{cfgs[2]}"
        conv[key] = CF.split_report(key, v, ref, bound, ex, lens) if kind == "split" else CF.Report(key, v, ref, bound, lens)
    if sand:
        for b in (1, 2):
            assert any(k.startswith(f"score.cb{b}.") for k in conv), (case, f"score.cb{b} was not held")
    # the GRU, fed the library's own score.cb1 output (plain model: the encoder's output, with the fused residual)
    if s.seq_model == "gru":
        L = G.Layer(sd, sp + ".encoder.gru", 0)
        x = _tap(model, "score.cb1.v" if sand else _enc_out(spec))
        gx, out = _tap(model, "score.gru.gx"), _tap(model, "score.gru")
        gru["score.gru.proj"] = G.check_projection(L, x, gx, lens_frames, ragged)
        gru["score.gru.step"] = G.check_step(L, gx, out, lens_frames, None if sand else (x if s.extra_conv_block else None))
    else:
        assert not _has(model, "score.gru") and not _has(model, "score.gru.gx") and not _has(model, "score.cb1.v")
    # the input of decoder block 0
    if s.extra_conv_block:
        src = _tap(model, "score.cb2.v" if sand else _enc_out(spec))
        res = _tap(model, _enc_out(spec))
        ref, bound = F.sum_scaled([src, res], F.INV_SQRT2)
        lens = None if lens_of is None else lens_of(src.shape[-1])
        exact["score.dec0.in|exact"] = F.Report("score.dec0.in", _tap(model, "score.dec0.in"), ref, bound, lens)
        if sand:  # (the residual in front of conv_block2 instead of behind it would be this:)
            wrong, _ = F.sum_scaled([_tap(model, "score.gru"), res], F.INV_SQRT2)
            assert not torch.equal(_tap(model, "score.dec0.in"), wrong)
    else:
        assert not _has(model, "score.dec0.in")  # an up block: reads score.cb2.v / the encoder's output in place
    return conv, gru, exact


def _last_score_pass(records, has_gru):
    """The records of the last of two score passes.  Both passes enqueue the same launches, so the record list ends with the same
    sequence of (algorithmic FLOPs, variant) twice: the longest such ending.  With a score GRU that is what
    test_gpu_conv_fp64._last_pass finds from the recurrence records (a model without one has only the conditioner's two)."""
    key = [(r[1], r[3]) for r in records]
    n = len(key)
    P = max(p for p in range(1, n // 2 + 1) if key[n - p:] == key[n - 2 * p: n - p])
    if has_gru:
        assert records[n - P:] == _last_pass(records)
    else:
        assert sum(1 for r in records if r[3] >= 1000) == 2
    return records[n - P:]


def _finish(name, t0, conv, gru, exact, extra=None):
    reports = {k: r for k, r in exact.items() if not isinstance(r, tuple)}
    rels = {k: r for k, r in exact.items() if isinstance(r, tuple)}
    counts = {"taps": len(conv) + len(reports), "checked": sum(r.checked for r in list(conv.values()) + list(reports.values())),
              "excluded": sum(r.excluded for r in list(conv.values()) + list(reports.values())),
              "tail_bad": sum(r.tail_bad for r in list(conv.values()) + list(reports.values()))}
    rec = {"seconds": round(time.time() - t0, 2), "worst": _summary(dict(conv, **reports)), "counts": counts,
           "gru": {k: round(float(r.ratio), 3) for k, r in gru.items()}, "snake_rel": {k: [float(a), float(b)] for k, (a, b) in rels.items()}}
    rec.update(extra or {})
    log_error = None
    try:
        _log(name, rec)
    except OSError as e:
        log_error = e
    print(f"{name}: {rec}")
    _assert_reports(name, dict(conv, **reports))
    for k, r in gru.items():
        assert r.excluded == 0 and r.ok(), f"{name} {k} {r}"
        assert r.ratio <= G.M_CAP, f"{name} {k}: err / e32 = {r.ratio:.2f} is a finding, not a tolerance -- {r}"
    for k, (rel, lim) in rels.items():
        assert rel <= lim, (name, k, rel, lim)
    assert counts["excluded"] == 0
    assert log_error is None, f"{name}: could not write the observed figures: {log_error}"
    return rec


# ---- 1. against the reference ------------------------------------------------------------------------------------------------
def _parity(log, name, ref, out):
    v = O.si_sdr(ref, out)
    log[name] = {"si_sdr": round(float(v), 2), "snr": round(float(getattr(v, "snr", float("nan"))), 2)}
    return v


@pytest.mark.parametrize("case", list(K.CASES))
def test_enhance_against_the_reference_goldens(case, tmp_path_factory, monkeypatch):
    t0 = time.time()
    gold = K.load_golden(case)
    assert float(gold["self_db"]) >= FLOOR, (case, float(gold["self_db"]), "the floor is a condition of the fixture")
    model, spec, sd = get_model(case, tmp_path_factory)
    figs, log = [], {"self_db": round(float(gold["self_db"]), 2)}
    mix = torch.from_numpy(gold["mix"])
    out = _enhance(model, mix, torch.from_numpy(gold["noise"]))
    ref = torch.from_numpy(gold["enh"])
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    figs.append((f"seqmodel.{case}.plain", _parity(log, "plain", ref, out)))
    assert ("enh_warm" in gold.files) == bool(spec.use_signal_decoupling)
    if "enh_warm" in gold.files:
        out = _enhance(model, mix, torch.from_numpy(gold["noise_warm"]), warm_start=1)
        figs.append((f"seqmodel.{case}.warm", _parity(log, "warm", torch.from_numpy(gold["enh_warm"]), out)))
    n = len(K.FILE_LENGTHS)
    for i in range(n):
        out = _enhance(model, torch.from_numpy(gold[f"mix_f{i}"]), torch.from_numpy(gold[f"noise_f{i}"]))
        figs.append((f"seqmodel.{case}.alone.file{i}", _parity(log, f"alone.file{i}", torch.from_numpy(gold[f"enh_f{i}"]), out)))
    # ONE enhance_many call over the three files, handed their recorded noise where it draws its own
    files = [torch.from_numpy(gold[f"mix_f{i}"])[0].cuda() for i in range(n)]
    Tmax = max(gold[f"noise_f{i}"].shape[-1] for i in range(n))
    planes = torch.zeros(K.N_STEPS, n, 1, Tmax)
    for i in range(n):
        nz = torch.from_numpy(gold[f"noise_f{i}"])
        planes[:, i:i + 1, :, :nz.shape[-1]] = nz
    drawn = []

    def recorded_noise(tot_ds, entries, n_planes, **kw):
        drawn.append(([int(e[1]) for e in entries], n_planes))
        return planes.cuda()

    monkeypatch.setattr(U, "draw_noise", recorded_noise)
    outs = model.enhance_many(files, n_steps=K.N_STEPS)
    assert drawn == [(list(K.FILE_LENGTHS), K.N_STEPS)]
    for i, o in enumerate(outs):
        ref = torch.from_numpy(gold[f"enh_f{i}"])[0]
        assert o.shape == ref.shape
        figs.append((f"seqmodel.{case}.many.file{i}", _parity(log, f"many.file{i}", ref, o.cpu())))
    log["seconds"] = round(time.time() - t0, 2)
    log_error = None
    try:
        _log(f"reference.{case}", log)
    except OSError as e:
        log_error = e
    print(f"reference.{case}: {log}")
    for name, v in figs:
        record(name, v)
    model.reset_workspace()
    assert log_error is None, log_error


# ---- 2. element by element ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,B", K.SHAPES)
@pytest.mark.parametrize("case", list(K.CASES))
def test_element_by_element(case, frames, B, steer, tmp_path_factory):
    t0 = time.time()
    steer.set(no_overlap=1)
    model, spec, sd = get_model(case, tmp_path_factory)
    model.reset_workspace()
    try:
        T = spec.tot_ds * frames
        xin = O.normalize(synth_mix(spec, B, T, seed=6100 + frames)[:, None, :], spec.level_db).float().contiguous()
        sig = torch.tensor([0.3, 1.7, 0.05])[:B]
        xs = (torch.randn(xin.shape, generator=torch.Generator().manual_seed(13 + frames)) * sig[:, None, None]).float().contiguous()
        model.profile(True)
        model.condition_model(xin.cuda(), train=True)
        model.score_model(xs.cuda(), sig)
        records = model.profile_read(32768)
        model.profile(False)
        conv, gru, exact = _bottleneck_reports(case, model, spec, sd, records, B)
        _finish(f"seams.{case}.b{B}.f{frames}", t0, conv, gru, exact)
    finally:
        model.profile(False)
        model.reset_workspace()


# ---- 3. ragged ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_fused", [0, 1])
@pytest.mark.parametrize("case", list(K.CASES))
def test_ragged(case, mask_fused, steer, tmp_path_factory):
    t0 = time.time()
    steer.set(mask_fused=mask_fused, no_overlap=1)
    model, spec, sd = get_model(case, tmp_path_factory)
    model.reset_workspace()
    try:
        td, rows = spec.tot_ds, K.RAGGED_ROWS
        t_raw = [f * td - 3 for f in rows]
        B, lm, T = len(rows), max(t_raw), max(rows) * td
        sigs = [synth_mix(spec, 1, n, seed=900 + i)[0] for i, n in enumerate(t_raw)]
        mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs])[:, None, :]
        nz = torch.zeros(2, B, 1, T)
        for b in range(B):
            nz[:, b, 0, :rows[b] * td] = torch.randn(2, rows[b] * td, generator=torch.Generator().manual_seed(980 + b))
        model.profile(True)
        out = _enhance(model, mix, nz, n_steps=2, keep_rms=True, t_raw=list(t_raw))
        records = model.profile_read(32768)
        model.profile(False)
        lens_of = lambda Tl: [f * (Tl // max(rows)) for f in rows]  # noqa: E731
        conv, gru, exact = _bottleneck_reports(case, model, spec, sd, records, B, lens_of, list(rows), ragged=True)
        # every tap of the bottleneck: something inside the rows, exactly 0 behind them
        s = spec.score
        sand = s.seq_model == "gru" and s.encoder_gru_conv_sandwich
        names = [_enc_out(spec)] + (["score.gru"] if s.seq_model == "gru" else []) + (["score.dec0.in"] if s.extra_conv_block else [])
        if sand:
            names += [f"score.cb{b}.{t}" for b in (1, 2) for t in ("c1", "c2", "v")]
        tails = {}
        for nme in names:
            t = _tap(model, nme)
            assert t.shape[-1] == max(rows), nme
            for b, f in enumerate(rows):
                assert bool(torch.isfinite(t[b]).all()) and float(t[b, :, :f].abs().max()) > 0, (nme, b)
                tails[nme] = tails.get(nme, 0) + int((t[b, :, f:] != 0).sum())
        for k, r in list(conv.items()) + [(k, r) for k, r in exact.items() if not isinstance(r, tuple)]:
            assert r.tail_bad == 0, f"{k}: {r.tail_bad} nonzero elements behind a row's end"
        # a row alone against the row in the batch
        alone = []
        for b in range(B):
            one = _enhance(model, sigs[b][None], nz[:, b:b + 1, :, :rows[b] * td], n_steps=2, keep_rms=True)
            alone.append(O.si_sdr(one[0], out[b, 0, :t_raw[b]]))
        _finish(f"ragged.mask_fused{mask_fused}.{case}", t0, conv, gru, exact,
                extra={"tails": tails, "row_alone_db": [round(float(a), 2) for a in alone]})
        assert all(v == 0 for v in tails.values()), tails
        for b, a in enumerate(alone):
            record(f"seqmodel.{case}.mask_fused{mask_fused}.row_alone.{b}", a, 100)
    finally:
        model.profile(False)
        model.reset_workspace()


# ---- 4. the entry points on sand_pp ------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def test_entry_points_on_the_sandwich_model(tmp_path_factory, tmp_path):
    """One small call of each family, each against the plain `enhance` of the same rows at the gate of that entry point's own test:
    bit identity wherever the same kernels run on the same rows (enhance_long of one window, E = 1, the unshared ensemble's members,
    graphed_enhance, lanes, the CLI), the ensemble tests' gates for the shared conditioner, 100 dB for rows batched differently."""
    from open_universe_amd import audio as A
    from open_universe_amd import distributed as D
    from open_universe_amd.bin import enhance as cli
    import ensemble_ref as R
    from test_gpu_ensemble import GATE_DB, _check_reduced, _members_by_enhance, _share

    t0 = time.time()
    model, spec, sd = get_model("sand_pp", tmp_path_factory)
    td, N = spec.tot_ds, 3
    mix = synth_mix(spec, 2, td * 10 + 77, seed=61).cuda()
    x = mix[0]
    log = {}
    plain = model.enhance(x, n_steps=N, rng=_gen(5))
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0
    # enhance_long of one window is enhance; enhance_long_many of the rows is enhance_long of each
    assert torch.equal(plain, model.enhance_long(x, n_steps=N, rng=_gen(5)))
    many = model.enhance_long_many([mix[0], mix[1][: td * 6 + 5]], [CounterNoise(3, 0), CounterNoise(3, 1)], n_steps=N)
    for i, (sgl, src) in enumerate(((mix[0], CounterNoise(3, 0)), (mix[1][: td * 6 + 5], CounterNoise(3, 1)))):
        one = model.enhance_long(sgl, n_steps=N, rng=src)
        v = O.si_sdr(one.cpu(), many[i].cpu())
        log[f"long_many.row{i}"] = round(float(v), 2)
        record(f"seqmodel.sand_pp.long_many.row{i}", v, 80)  # (test_gpu_segments_var.FLOOR_DB)
    # counter noise: repeatable, and the one-member ensemble is the plain call bit for bit
    a = model.enhance(mix, n_steps=N, rng=CounterNoise(5, 2))
    assert torch.equal(a, model.enhance(mix, n_steps=N, rng=CounterNoise(5, 2)))
    b, mem = model.enhance_ensemble(mix, 1, "median", n_steps=N, rng=CounterNoise(5, 2), return_members=True)
    assert torch.equal(a, b) and torch.equal(mem[0], b)
    # E = 2: unshared members are enhance on the replicated batch; the shared conditioner at the ensemble tests' gates
    E = 2
    want = _members_by_enhance(model, mix, E, CounterNoise(33, 7), n_steps=N)
    with _share(model, 0):
        out_u, mem_u = model.enhance_ensemble(mix, E, "mean", n_steps=N, rng=CounterNoise(33, 7), return_members=True)
        assert torch.equal(mem_u, want)
        ref = model.enhance(mix, n_steps=N, rng=CounterNoise(33, 7), ensemble=E, ensemble_stat="mean")
        _check_reduced(out_u.cpu(), ref.cpu(), mem_u.cpu(), "mean")
    out_s, mem_s = model.enhance_ensemble(mix, E, "mean", n_steps=N, rng=CounterNoise(33, 7), return_members=True)
    # (test_gpu_ensemble._check_shared_against_unshared: members >= 100 dB, the mean 1-Lipschitz in the members)
    ms, mu = mem_s.cpu().reshape(E, -1, mem_s.shape[-1]), mem_u.cpu().reshape(E, -1, mem_u.shape[-1])
    worst = min(float(O.si_sdr(mu[e, b], ms[e, b])) for e in range(E) for b in range(ms.shape[1]))
    log["ensemble.shared_vs_unshared"] = round(worst, 2)
    dev = (ms.double() - mu.double()).abs().max(dim=0).values
    slack = R.mean_bound(ms, ms.double().mean(dim=0)) + R.mean_bound(mu, mu.double().mean(dim=0))
    shared_ok = bool(((out_s.cpu().double() - out_u.cpu().double()).abs().reshape(dev.shape) <= dev + slack).all())
    # warm start and the aux exit: the aux exit runs no score pass and is what warm start begins from
    aux = model.enhance(x, n_steps=N, use_aux_signal=True)
    assert torch.equal(aux, model.enhance_long(x, n_steps=N, use_aux_signal=True)) and bool(torch.isfinite(aux).all())
    warm = model.enhance(x, n_steps=N, warm_start=1, rng=_gen(8))
    assert torch.equal(warm, model.enhance_long(x, n_steps=N, warm_start=1, rng=_gen(8)))
    assert not torch.equal(warm, aux) and not torch.equal(warm, plain)
    # graphed_enhance replays the same launches
    run = model.graphed_enhance(1, x.shape[-1], n_steps=N)
    assert torch.equal(run(x, rng=_gen(5)), plain)
    assert torch.equal(run(x, rng=_gen(5)), plain)
    # lanes through distributed.enhance_sharded: bit-identical to the serial loop
    sigs = [synth_mix(spec, 1, n, seed=700 + i)[0] for i, n in enumerate((1500, 2100, 900, 1500))]
    serial = D.enhance_sharded(model, sigs, seed=2, n_steps=N)
    flying = D.enhance_sharded(model, sigs, seed=2, n_steps=N, in_flight=3)
    assert all(torch.equal(u, v) for u, v in zip(serial, flying))
    # the CLI
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    A.save(src / "a.wav", (synth_mix(spec, 1, 3000, seed=70) * 0.5).clamp(-1, 1), spec.fs)
    done = cli.main([str(src), str(dst), "--seed", "99", "--n_steps", str(N)], model=model)
    assert [p.relative_to(dst).as_posix() for p in done] == ["a.wav"]
    y_in, _ = A.load(src / "a.wav")
    y, fs = A.load(dst / "a.wav")
    direct = model.enhance(y_in.cuda(), n_steps=N, rng=torch.Generator(device="cuda:0").manual_seed(99))
    assert fs == spec.fs and torch.equal(y, direct.cpu())
    log["seconds"] = round(time.time() - t0, 2)
    _log("entry_points.sand_pp", log)
    print(f"entry_points.sand_pp: {log}")
    model.reset_workspace()
    assert worst >= GATE_DB and shared_ok, (worst, shared_ok)
