"""GPU (-m gpu): the ConvBlock body convs (conv1, conv2, conv3 of every block of both networks) against the float64 references
of tests/conv_fp64.py, element by element, through the taps one conditioner pass and one score pass leave behind
({block}.up / .c1 / .c2 / .v, model.tensor(name)); every checked layer is paired with the variant code the launcher chose
(model.profile), which picks the bound kind and decides whether the tap holds the activated value.  One parametrised test over
conv_fp64.CASES (an option set per kernel family) and one over ragged batches (mask_fused 0 / 1).  Before it asserts each case logs
every tap's figures to build/observed/conv_fp64_taps.json and, per (bound kind, variant code), the worst tap with its element and
the counts to build/observed/conv_fp64_observed.json (both untracked); profiles/conv_fp64_observed.json is a committed copy of
the latter.

Measured on an MI355X (worst err / bound): chain 0.37, minimal filtering 0.33, fused depth 2 / 3 0.002 / 0.009, ragged tails all
exactly 0; bf16 split: err / e32 at most 3.21, median 1.36 (M_SPLIT = 7, tests/conv_fp64.py)."""
import json
import os
import time

import pytest
import torch

import conv_fp64 as C
import restatement as O
import small_fp64 as F
from helpers import synth_mix
from open_universe_amd import _lib, variants as V
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed")
_params = {}


def _P(name, spec, sd):
    """The rebuilt parameters, held once per model against the blob the library packs for it (weights, bias, slopes, U)."""
    if name not in _params:
        P = C.ConvParams(spec, sd)
        blob, plan = _lib.pack_weights(spec, sd)
        P.check_against_blob(blob, json.loads(plan))
        _params[name] = P
    return _params[name]


def _widths():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_fp64_widths.json")) as f:
        return json.load(f)


def _tap(model, name):
    return model.tensor(name).cpu().clone()


def _pair_with_profile(P, records, B, T_of):
    """Walk order -> {block: (depth, [variant code per launch])}: the body convs of a block are consecutive records whose
    algorithmic FLOPs are those of (c1, c2, c3), (c1, c2 + c3) or (c1 + c2 + c3); everything else (rate-change, 1x1, GRU) is
    passed over.  A block that is not found fails the test."""
    out, i = {}, 0
    body = lambda cfg: not V.is_recurrence_record(cfg) and V.family_of(cfg) not in ("direct4", "direct3s")
    for p, *_ in P.walk:
        bp = P.blocks[p]
        fl = [2.0 * bp.C * float(T_of[p]) * bp.C * cv.KW * B for cv in bp.c]
        pats = ((3, [sum(fl)]), (2, [fl[0], fl[1] + fl[2]]), (0, fl))
        found = None
        while i < len(records) and found is None:
            for depth, pat in pats:
                got = records[i: i + len(pat)]
                if len(got) == len(pat) and all(body(r[3]) and r[1] == f for r, f in zip(got, pat)) and \
                        all((V.family_of(r[3]) == "fused") == (depth > 0 and k == len(pat) - 1) for k, r in enumerate(got)):
                    found = (depth, [r[3] for r in got])
                    i += len(pat)
                    break
            else:
                i += 1
        assert found is not None, (p, "no profile records match this block's body convs")
        out[p] = found
    return out


def _check_blocks(reps, P, model, paired, preact, film_tap, lens_of=None):
    """Every body conv of every block from the taps of the last passes.  -> [(block, conv, variant, C, KW)]."""
    ran = []
    for p, q, inp, fidx, add, c1n, vn, exported in P.walk:
        bp = P.blocks[p]
        depth, cfgs = paired[p]
        hu = _tap(model, inp if inp is not None else p + ".up")
        lens = None if lens_of is None else lens_of(hu.shape[-1])
        ep1 = C.Epi()
        if add is not None:
            ep1.add = _tap(model, add)
        if fidx is not None:
            o = P.film_off[p]
            ep1.film = (film_tap[:, o: o + bp.C], film_tap[:, o + bp.C: o + 2 * bp.C])
        v_gpu = _tap(model, vn)
        if depth == 3:
            ref, bound, c1r, c1b = C.fused_body(hu, bp, 3, ep1, hu, lens)
            reps[f"{p}.v|fused3|{cfgs[0]}"] = C.Report(p + ".v", v_gpu, ref, bound, lens)
            if exported:
                reps[f"{p}.c1|fused3|{cfgs[0]}"] = C.Report(p + ".c1", _tap(model, c1n), c1r, c1b, lens)
            ran.append((p, "body", cfgs[0], bp.C, 0))
            continue
        # conv1
        a1 = preact and not exported
        if depth == 0 and C.stores_activated(cfgs[0], a1):
            ep1.out_alpha = bp.c[1].alpha
        kind = C.kind_of(cfgs[0])
        c1 = _tap(model, c1n)
        ref, bound, ex = C.body_conv(hu, bp.c[0], ep1, kind, lens)
        key = f"{p}.c1|{kind}|{cfgs[0]}"
        reps[key] = C.split_report(key, c1, ref, bound, ex, lens) if kind == "split" else C.Report(key, c1, ref, bound, lens)
        ran.append((p, "conv1", cfgs[0], bp.C, 5))
        if depth == 2:
            ref, bound, _, _ = C.fused_body(c1, bp, 2, None, hu, lens)
            reps[f"{p}.v|fused2|{cfgs[1]}"] = C.Report(p + ".v", v_gpu, ref, bound, lens)
            ran.append((p, "body", cfgs[1], bp.C, 0))
            continue
        # conv2: reads c1 (activated by its producer or by itself), may store activated for conv3
        ep2 = C.Epi(act=ep1.out_alpha is None)
        if C.stores_activated(cfgs[1], preact):
            ep2.out_alpha = bp.c[2].alpha
        kind = C.kind_of(cfgs[1])
        c2 = _tap(model, p + ".c2")
        ref, bound, ex = C.body_conv(c1, bp.c[1], ep2, kind, lens)
        key = f"{p}.c2|{kind}|{cfgs[1]}"
        reps[key] = C.split_report(key, c2, ref, bound, ex, lens) if kind == "split" else C.Report(key, c2, ref, bound, lens)
        ran.append((p, "conv2", cfgs[1], bp.C, 3))
        # conv3: + the block's residual
        ep3 = C.Epi(act=ep2.out_alpha is None, res=hu)
        kind = C.kind_of(cfgs[2])
        ref, bound, ex = C.body_conv(c2, bp.c[2], ep3, kind, lens)
        key = f"{p}.v|{kind}|{cfgs[2]}"
        reps[key] = C.split_report(key, v_gpu, ref, bound, ex, lens) if kind == "split" else C.Report(key, v_gpu, ref, bound, lens)
        ran.append((p, "conv3", cfgs[2], bp.C, 3))
    return ran


def _merge(fname, case, rec, indent):
    path = os.path.join(_OUT, fname)
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[case] = rec
    with open(path, "w") as f:
        if indent is None:  # one line per case
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(old.items())) + "\n}\n")
        else:
            json.dump(old, f, indent=indent, sort_keys=True)


def _finish(case, reps, ran, want, t0):
    """Log, print, then assert."""
    fams = {}
    for p, conv, cfg, Cc, KW in ran:
        fams.setdefault(C.family_of(cfg), set()).add((Cc, KW))
    worst = {}
    for k, r in reps.items():
        kind = k.split("|")[1]
        worst[kind] = max(worst.get(kind, 0.0), r.ratio)
    log_error = None
    try:
        os.makedirs(_OUT, exist_ok=True)
        # every tap's figures: conv_fp64_taps.json (5 000 records over the cases: untracked only)
        taps = {}
        for k, r in reps.items():
            taps[k] = r.summary()
            if hasattr(r, "lib_ratio"):
                taps[k].update(e32=r.e32, lib_ratio=round(r.lib_ratio, 3))
        _merge("conv_fp64_taps.json", case, taps, indent=1)
        # per case and (kind, variant code): the worst tap with its element, the counts over the taps, the split kernel's ratios
        groups = {}
        for k, r in reps.items():
            tap, kind, cfg = k.split("|")
            g = groups.setdefault(f"{kind}|{cfg}", {"taps": 0, "checked": 0, "excluded": 0, "bad": 0, "tail_bad": 0, "ratio": -1.0})
            g["taps"] += 1
            for f in ("checked", "excluded"):
                g[f] += getattr(r, f)
            g["bad"] += r.n_bad
            g["tail_bad"] += r.tail_bad
            if r.ratio > g["ratio"]:
                g.update(ratio=round(r.ratio, 4), worst_tap=tap, err=float(f"{r.err:.3e}"), index=r.worst["index"])
            if hasattr(r, "lib_ratio"):
                g["lib_ratio"] = max(g.get("lib_ratio", 0.0), round(r.lib_ratio, 3))
        _merge("conv_fp64_observed.json", case, {"seconds": round(time.time() - t0, 2), "families": {f: sorted(v) for f, v in fams.items()},
                                                 "by_kind_and_variant": groups}, indent=None)
    except OSError as e:
        log_error = e
    print(f"{case}: {time.time() - t0:.1f} s, worst err / bound per kind {worst}, families {fams}")
    for k, r in reps.items():
        if not r.ok() or hasattr(r, "lib_ratio"):
            print(f"{case} {r}" + (f" err / e32 = {r.lib_ratio:.2f}" if hasattr(r, "lib_ratio") else ""))
    for k, r in reps.items():
        assert r.excluded == 0 and r.ok(), f"{case} {r}"
        if hasattr(r, "lib_ratio"):
            assert r.lib_ratio <= F.M_CAP, f"{case} {k}: err / e32 = {r.lib_ratio:.2f} is a finding, not a tolerance"
    # a case that silently fell back to another family, on all layers or on one channel width, fails: every family under test
    # has to have taken exactly the (channels, kernel size) recorded for this case on an MI355X
    expected = _widths().get(case)
    assert expected is not None, (case, "no recorded widths for this case")
    for fam in want:
        got = [list(v) for v in sorted(fams.get(fam, ()))]
        assert got == expected.get(fam, []), (case, fam, "took", got, "recorded", expected.get(fam, []))
    assert log_error is None, f"{case}: could not write the observed figures: {log_error}"


@pytest.mark.parametrize("tag,name,B,frames", C.CASES)
def test_body_convs(tag, name, B, frames, steer):
    t0 = time.time()
    opts, want = C.FAMILIES[tag][:2]
    steer.set(**opts)
    model, spec, sd = get_model(name)
    model.reset_workspace()
    try:
        P = _P(name, spec, sd)
        T = spec.tot_ds * frames
        xin = O.normalize(synth_mix(spec, B, T, seed=4000 + frames)[:, None, :], spec.level_db).float().contiguous()
        model.profile(True)
        model.condition_model(xin.cuda(), train=True)
        sig = torch.tensor([0.3, 1.7, 0.05, 4.0])[:B]
        xs = (torch.randn(xin.shape, generator=torch.Generator().manual_seed(7 + frames)) * sig[:, None, None]).float().contiguous()
        model.score_model(xs.cuda(), sig)
        records = model.profile_read(32768)
        model.profile(False)
        T_of = {p: (model.tensor(vn).shape[-1]) for p, q, i, f, a, c1n, vn, ex in P.walk}
        paired = _pair_with_profile(P, records, B, T_of)
        reps = {}
        ran = _check_blocks(reps, P, model, paired, opts.get("preact", 1) != 0, _tap(model, "sigma.film"))
        _finish(C.case_id(tag, name, B, frames), reps, ran, want, t0)
    finally:
        model.profile(False)
        model.reset_workspace()


@pytest.mark.parametrize("name,mask_fused", C.RAGGED)
def test_body_convs_of_a_ragged_batch(name, mask_fused, steer):
    """ou_enhance_var, two steps: the conditioner's taps and those of the LAST score pass (step 1: FiLM row 1 of the table, shared
    by the rows) -- every body conv inside the rows, exactly 0 behind every row's end on every tap."""
    t0 = time.time()
    steer.set(mask_fused=mask_fused, no_overlap=1)
    model, spec, sd = get_model(name)
    model.reset_workspace()
    try:
        P = _P(name, spec, sd)
        td = spec.tot_ds
        rows = C.RAGGED_ROWS
        t_raw = [f * td - 3 for f in rows]
        B, lm = len(t_raw), max(t_raw)
        T = max(rows) * td
        sigs = [synth_mix(spec, 1, n, seed=600 + i)[0] for i, n in enumerate(t_raw)]
        mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs])[:, None, :]
        nz = torch.zeros(2, B, 1, T)
        for b in range(B):
            nz[:, b, 0, :rows[b] * td] = torch.randn(2, rows[b] * td, generator=torch.Generator().manual_seed(970 + b))
        # who places the zeros: with mask_fused = 0 a mask_tail launch follows every producer, with 1 the producers mask in
        # their own epilogues -- the same call under the other setting enqueues more / fewer launches
        steer.set(mask_fused=1 - mask_fused, no_overlap=1)
        model._enhance(mix.cuda(), 2, None, None, None, None, False, False, None, "median", None, nz.cuda(), t_raw=list(t_raw))
        other = model.launch_stats()[0]
        steer.set(mask_fused=mask_fused, no_overlap=1)
        model.reset_workspace()
        model.profile(True)
        model._enhance(mix.cuda(), 2, None, None, None, None, False, False, None, "median", None, nz.cuda(), t_raw=list(t_raw))
        mine = model.launch_stats()[0]
        print(f"ragged {name} mask_fused {mask_fused}: {mine} launches, {other} under the other setting")
        assert (mine > other) == (mask_fused == 0) and mine != other, (mask_fused, mine, other)
        records = model.profile_read(32768)
        model.profile(False)
        T_of = {p: (model.tensor(vn).shape[-1]) for p, q, i, f, a, c1n, vn, ex in P.walk}
        # the conditioner ran once, the score network twice: the conditioner's blocks are paired from the front, the score
        # network's from the records of the last pass (option no_overlap: the calls enqueue in walk order)
        n_cond = sum(1 for p, *_ in P.walk if p.startswith("cond."))
        full = P.walk
        try:
            P.walk = full[:n_cond]
            paired = _pair_with_profile(P, records, B, T_of)
            P.walk = full[n_cond:]
            paired.update(_pair_with_profile(P, _last_pass(records), B, T_of))
        finally:
            P.walk = full
        film = _tap(model, "sigma.film")[1:2].expand(B, -1, -1)
        lens_of = lambda Tl: [f * (Tl // max(rows)) for f in rows]
        reps = {}
        ran = _check_blocks(reps, P, model, paired, True, film, lens_of)
        case = f"ragged.mask_fused{mask_fused}.{name}"
        _finish(case, reps, ran, tuple(_widths().get(case, {})), t0)
    finally:
        model.profile(False)
        model.reset_workspace()


def _last_pass(records):
    """The records of the last score pass.  Recurrences (variant >= 1000): two of the conditioner, one per score pass; both
    passes enqueue the same launches, so a pass is as long as the distance between their recurrences."""
    gru = [i for i, r in enumerate(records) if r[3] >= 1000]
    assert len(gru) == 4, len(gru)
    return records[len(records) - (gru[3] - gru[2]):]
