"""GPU (-m gpu): the rate-change convs of every block of both networks, the st / sc convs and the mel conv against the float64
references of tests/rate_fp64.py, element by element, through the taps one conditioner pass and one score pass leave behind.
Every checked launch is paired with the variant code the launcher chose (model.profile, walk order under option no_overlap = 1:
rate_fp64.pair_walk), which picks the bound kind.  One parametrised test over rate_fp64.CASES (an option set per kernel family) and
one over ragged batches (mask_fused 0 / 1, default dispatch and rate_small = 0).  Before it asserts each case logs, per (bound
kind, variant code), the worst tap with its element, the counts and the seconds to build/observed/rate_fp64_observed.json
(untracked); profiles/rate_fp64_observed.json is a committed copy.  Every case asserts that the families it is about took exactly
the layers recorded for it on an MI355X (tests/golden/rate_fp64_variants.json).

Measured on an MI355X (worst err / bound): chain 0.14, down_fir 0.07, up_fir 0.05, folded 0.02, minimal filtering (the mel conv on
conv_direct4w) 0.02; ragged tails all exactly 0; at most 3.1 s per case."""
import json
import os
import time

import pytest
import torch

import rate_fp64 as R
import restatement as O
from helpers import get_spec, synth_mix
from open_universe_amd import _lib
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_OUT = os.path.join(os.path.dirname(_HERE), "build", "observed")
_GOLDEN = os.path.join(_HERE, "golden", "rate_fp64_variants.json")
_SENTINEL = 12345.0
_params, _folded = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_folded_models():
    """The second model objects (a packed blob each) live for this module only."""
    yield
    _folded.clear()


def _model(name, fold):
    """(model, spec, sd): the shared model object, or -- fir_fold -- a second one built on the folded blob."""
    model, spec, sd = get_model(name)
    if fold:
        if name not in _folded:
            _folded[name] = type(model)(spec, state_dict=sd, device="cuda:0", fir_fold=fold)
        model = _folded[name]
    return model, spec, sd


def _P(name, spec, sd, fold):
    """The rebuilt parameters and the plan, held once per (model, fir_fold) against the blob the library packs for it."""
    if (name, fold) not in _params:
        P = R.RateParams(spec, sd)
        blob, plan = _lib.pack_weights(spec, sd, fir_fold=fold)
        plan = json.loads(plan)
        P.check_against_blob(blob, plan)
        _params[(name, fold)] = (P, {c["name"]: c for c in plan["convs"]})
    return _params[(name, fold)]


def _tap(model, name):
    return model.tensor(name).cpu().clone()


def _has(model, name):
    try:
        model.tensor(name)
        return True
    except KeyError:
        return False


def _flops_of(P, convs, model, B):
    """Algorithmic FLOPs of every slot of the walk as Runner::conv / Runner::body count them (the packed layer's own KW)."""
    out = {}
    for net, kind, key in P.slots:
        if kind == "body":
            Cc, T = P.body_C[key], model.tensor(P.v_tap[key]).shape[-1]
            out[(kind, key)] = [2.0 * Cc * float(T) * Cc * KW * B for KW in (5, 3, 3)]
        elif kind in ("rate", "conv"):
            L = convs[P.plan_name(key)]
            tap = (key + (".up" if P.rate[key].up else ".h")) if kind == "rate" else key
            Nq = model.tensor(tap).shape[-1] // L["up"]
            out[(kind, key)] = 2.0 * L["M"] * float(Nq) * L["Cin"] * L["KW"] * B
    return out


def _poison(model, P):
    """The sentinel into every {blk}.upc of the last pass's layout (module docstring of rate_fp64: who wrote the tap?)."""
    for key, rl in P.rate.items():
        if rl.up and _has(model, key + ".upc"):
            model.tensor(key + ".upc").fill_(_SENTINEL)


def _check(reps, ran, P, convs, model, paired, pas, lens_of=None):
    """Every layer of the table from the taps of the last passes."""
    def lens(T):
        return None if lens_of is None else lens_of(T)

    def put(tap, kind, cfg, gpu, ref, bound, T):
        reps[f"{tap}|{kind}|{cfg}"] = R.Report(tap, gpu, ref, bound, lens(T))
    for key, rl in P.rate.items():
        cfg = paired[(pas if key.startswith("score.") else 0, key)]
        L = convs[rl.name]
        mode = L["fir_mode"]
        cls = "up" if rl.up else "down"
        if not rl.up:
            h = _tap(model, key + ".h")
            x = _tap(model, P.src[key])
            kind = R.kind_of(cfg, mode, False)
            if kind == "folded":
                form, src = "folded", x
            elif kind == "down_fir":
                form, src = "fused", x
            elif mode == 1:
                # FIR pass + conv: {blk}.fir is not masked behind the rows (down_path) and nothing is asserted of it here
                form, src = "after_fir", _tap(model, key + ".fir")
                cls = "down.after_fir"
            else:
                form, src = "conv", x
            ref, bound = R.down(src, rl, form, lens(h.shape[-1]))
            put(key + ".h", kind, cfg, h, ref, bound, h.shape[-1])
        else:
            x = _tap(model, P.src[key])
            res = _tap(model, P.res[key]) if key in P.res else None
            hu = _tap(model, key + ".up")
            T = hu.shape[-1]
            upc = _tap(model, key + ".upc") if _has(model, key + ".upc") else None
            unfused = upc is not None and not bool((upc == _SENTINEL).all()) and R.family_of(cfg) != "rate_up"
            if unfused:
                # conv + FIR pass: the conv's own output (no bias, no residual); the FIR pass behind it is held by
                # tests/test_gpu_small_fp64.py
                assert mode == 2, (key, mode)
                ref, bound = R.up(x, rl, "upc", None, lens(T))
                put(key + ".upc", "chain", cfg, upc, ref, bound, T)
                cls = "up.unfused"
            else:
                kind = R.kind_of(cfg, mode, mode == 2)
                form = {"folded": "folded", "up_fir": "fused", "chain": "conv"}[kind]
                ref, bound = R.up(x, rl, form, res, lens(T))
                put(key + ".up", kind, cfg, hu, ref, bound, T)
        ran.append((R.family_of(cfg), cls, rl.Cin, rl.Cout, rl.r))
    scale = _tap(model, "mel_scale")
    for key, ol in P.one.items():
        cfg = paired[(0, key)]
        y = _tap(model, key)
        wino = 400 <= cfg < 800
        ref, bound = R.conv_1x1(_tap(model, ol.src), ol, scale if key == "cond.melconv" else None, lens(y.shape[-1]), wino=wino)
        put(key, "wino" if wino else "chain", cfg, y, ref, bound, y.shape[-1])
        ran.append((R.family_of(cfg), key.rstrip("0123456789").split(".")[1], ol.w.shape[1], ol.w.shape[0], 1))


def _merge(case, rec):
    path = os.path.join(_OUT, "rate_fp64_observed.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[case] = rec
    with open(path, "w") as f:  # one line per case
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(old.items())) + "\n}\n")


def _finish(case, reps, ran, want, t0):
    """Log, print, then assert."""
    fams = {}
    for fam, *layer in ran:
        fams.setdefault(fam, set()).add(tuple(layer))
    fams = {f: [list(v) for v in sorted(s)] for f, s in fams.items()}
    worst, groups = {}, {}
    for k, r in reps.items():
        tap, kind, cfg = k.split("|")
        worst[kind] = max(worst.get(kind, 0.0), r.ratio)
        g = groups.setdefault(f"{kind}|{cfg}", {"taps": 0, "checked": 0, "excluded": 0, "bad": 0, "tail_bad": 0, "ratio": -1.0})
        g["taps"] += 1
        g["checked"] += r.checked
        g["excluded"] += r.excluded
        g["bad"] += r.n_bad
        g["tail_bad"] += r.tail_bad
        if r.ratio > g["ratio"]:
            g.update(ratio=round(r.ratio, 4), worst_tap=tap, err=float(f"{r.err:.3e}"), index=r.worst["index"])
    log_error = None
    try:
        os.makedirs(_OUT, exist_ok=True)
        _merge(case, {"seconds": round(time.time() - t0, 2), "families": fams, "by_kind_and_variant": groups})
    except OSError as e:
        log_error = e
    print(f"{case}: {time.time() - t0:.1f} s, worst err / bound per kind {worst}, families {fams}")
    for k, r in reps.items():
        if not r.ok():
            print(f"{case} {r}")
    for k, r in reps.items():
        assert r.excluded == 0 and r.ok(), f"{case} {r}"
    # a case that silently fell back to another kernel fails: every family the case is about has to have taken exactly the
    # layers recorded for it on an MI355X
    with open(_GOLDEN) as f:
        expected = json.load(f).get(case)
    assert expected is not None, (case, "no recorded layers for this case")
    for fam in sorted(set(want) | set(fams) | set(expected)):
        assert fams.get(fam, []) == expected.get(fam, []), (case, fam, "took", fams.get(fam, []), "recorded", expected.get(fam, []))
    assert log_error is None, f"{case}: could not write the observed figures: {log_error}"


@pytest.mark.parametrize("tag,name,B,frames", R.CASES)
def test_rate_change_and_1x1_convs(tag, name, B, frames, steer):
    t0 = time.time()
    opts, fold, want = R.FAMILIES[tag]
    steer.set(no_overlap=1, **opts)
    model, spec, sd = _model(name, fold)
    model.reset_workspace()
    try:
        P, convs = _P(name, spec, sd, fold)
        T = spec.tot_ds * frames
        xin = O.normalize(synth_mix(spec, B, T, seed=4100 + frames)[:, None, :], spec.level_db).float().contiguous()
        sig = torch.tensor([0.3, 1.7, 0.05, 4.0])[:B]
        xs = (torch.randn(xin.shape, generator=torch.Generator().manual_seed(9 + frames)) * sig[:, None, None]).float().contiguous()
        for profiled in (False, True):  # two identical passes, the sentinel between them
            model.profile(profiled)
            model.condition_model(xin.cuda(), train=True)
            model.score_model(xs.cuda(), sig)
            if not profiled:
                _poison(model, P)
        records = model.profile_read(32768)
        model.profile(False)
        paired = R.pair_walk(P.slots, records, _flops_of(P, convs, model, B))
        reps, ran = {}, []
        _check(reps, ran, P, convs, model, paired, 0)
        _finish(R.case_id(tag, name, B, frames), reps, ran, want, t0)
    finally:
        model.profile(False)
        model.reset_workspace()


@pytest.mark.parametrize("name,mask_fused,rate_small", R.RAGGED)
def test_rate_change_and_1x1_convs_of_a_ragged_batch(name, mask_fused, rate_small, steer):
    """ou_enhance_var, two steps: the conditioner's taps and those of the LAST score pass -- every layer of the table inside the
    rows, exactly 0 behind every row's end on every tap of the table ({blk}.fir excepted: nothing is asserted of it)."""
    t0 = time.time()
    steer.set(mask_fused=mask_fused, no_overlap=1, rate_small=rate_small)
    model, spec, sd = get_model(name)
    model.reset_workspace()
    try:
        P, convs = _P(name, spec, sd, 0)
        td = spec.tot_ds
        rows = R.RAGGED_ROWS
        t_raw = [f * td - 3 for f in rows]
        B, lm = len(t_raw), max(t_raw)
        T = max(rows) * td
        sigs = [synth_mix(spec, 1, n, seed=700 + i)[0] for i, n in enumerate(t_raw)]
        mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs])[:, None, :]
        nz = torch.zeros(2, B, 1, T)
        for b in range(B):
            nz[:, b, 0, :rows[b] * td] = torch.randn(2, rows[b] * td, generator=torch.Generator().manual_seed(870 + b))
        for profiled in (False, True):
            model.profile(profiled)
            model._enhance(mix.cuda(), 2, None, None, None, None, False, False, None, "median", None, nz.cuda(), t_raw=list(t_raw))
            if not profiled:
                _poison(model, P)
        records = model.profile_read(32768)
        model.profile(False)
        paired = R.pair_walk(P.slots, records, _flops_of(P, convs, model, B), score_passes=2)
        lens_of = lambda Tl: [f * (Tl // max(rows)) for f in rows]
        reps, ran = {}, []
        _check(reps, ran, P, convs, model, paired, 1, lens_of)
        for k, r in reps.items():
            assert r.tail_bad == 0, f"{k}: {r.tail_bad} nonzero elements behind a row's end"
        _finish(f"ragged.mask_fused{mask_fused}.rate_small{rate_small}.{name}", reps, ran, ("rate_down", "rate_up", "direct4", "direct", "strided"), t0)
    finally:
        model.profile(False)
        model.reset_workspace()
