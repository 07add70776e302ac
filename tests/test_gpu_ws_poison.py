"""GPU (-m gpu): every enhance call independent of what its workspace held before (tests/ws_poison.py has the helper, the calls
and the case table).  A case runs its call once, then again after each fill of the workspace's body (zero, NaN, seeded finite
values in +-2^10).  `out`, `members_out` and every named tap the call writes have to come back torch.equal after every fill, in
every case, plain ones included; where the taps hold a ragged walk -- ou_enhance_var, ou_enhance_ensemble with t_raw, and the
last group of ou_enhance_segments_var / _var_ensemble -- every tap is also exactly 0 behind its rows' ends.  No tolerance anywhere.

    test_positive_control      condition_model, poison, score_model: the poison reaches what the kernels consume
    test_case                  a. the seven entry points, b. every kernel family at full width, c. the other model kinds,
                               d. (inside the ragged cases) every tap exactly 0 behind its rows' ends under poison
    test_outside_the_rows      e. NaN in mix / noise behind the rows changes no bit; out / members_out 0 from the rows' ends on
    test_call_order            f. the second of two calls on a shared workspace equals that call alone on a fresh one

A tap the call does not write (an interior .c1 / .c2 of a fused body, `wav` without a warm start, `x` of the aux exit) still
holds the fill word for word after the call: that is how it is told from a written one, and it is logged as `unwritten`.

Figures: build/observed/ws_poison_observed.json (untracked, started afresh by the module's first test) before anything is
asserted; profiles/ws_poison_observed.json is the committed copy of the MI355X run.

Measured on an MI355X: 280 cases -- the control, 243 of test_case, 6 of (e), 30 of (f) -- in 15.9 s run alone (11.1 s inside the
whole suite, whose earlier modules have built the models); outputs and taps equal under every fill in every case, no exemption
(ws_poison.NAN_EXEMPT is empty), every tail 0; no library change was needed.  The
chunked GRU path is asserted by its option alone: the launch count and the profile have one entry per recurrence, however many
sub-launches launch_gru split it into (gru_bmax below the batch size caps every sub-launch, ou_gru.hip)."""
import ctypes
import json
import os
import time

import pytest
import torch

import conv_fp64 as CF
import ws_poison as W
from open_universe_amd import _lib, variants as V
from open_universe_amd.universe import padded

pytestmark = pytest.mark.gpu

_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed")
_T0 = []  # when the module's first test began


def _begin():
    """A test of this module begins; the first one starts the figures afresh (no entry of an earlier run or table survives)."""
    if not _T0:
        try:
            os.remove(os.path.join(_OUT, "ws_poison_observed.json"))
        except OSError:
            pass
    _T0.append(time.time())
    return _T0[-1]


def _log(case, rec):
    """-> None or the error that kept the figures from being written (asserted last)."""
    try:
        os.makedirs(_OUT, exist_ok=True)
        path = os.path.join(_OUT, "ws_poison_observed.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[case] = rec
        cases = [k for k in old if not k.startswith("_")]
        old["_total"] = {"cases": len(cases), "case_seconds": round(sum(old[k].get("seconds", 0.0) for k in cases), 2),
                         "module_seconds": round(time.time() - _T0[0], 2)}
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(old.items())) + "\n}\n")
    except OSError as e:
        return e
    return None


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))


def _fresh(model):
    model.reset_workspace()
    model._seg_ws = None


# ---- 2. the positive control (first in the module) ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["PP16s"])
def test_positive_control(name):
    """Between condition_model and score_model the body legitimately carries the conditioner's results: poisoned there, the
    score has to show it -- NaN under `nan`, other bits under `finite`.  (The helper reaches memory the kernels consume.)"""
    t0 = _begin()
    model, spec = W.get(("zoo", name))
    _fresh(model)
    B, T = 2, W.FRAMES * spec.tot_ds
    x = W.mix_of(spec, [T] * B, seed=610).cuda() * 10.0
    sig = torch.tensor([0.3, 1.7])
    xs = (torch.randn(B, 1, T, generator=torch.Generator().manual_seed(7)) * sig[:, None, None]).cuda()
    model.condition_model(x)
    clean = model.score_model(xs, sig).clone()
    assert bool(torch.isfinite(clean).all())
    hdr = W.header_bytes(model)
    seen = {}
    for fill in ("nan", "finite"):
        model.condition_model(x)
        W.poison(model, fill)
        seen[fill] = model.score_model(xs, sig).clone()
    # unpoisoned, the pair repeats bit for bit (what makes a difference under `finite` mean something)
    model.condition_model(x)
    again = model.score_model(xs, sig)
    rec = {"header_bytes": hdr, "nan_elements": int(torch.isnan(seen["nan"]).sum()), "finite_differs": not torch.equal(seen["finite"], clean),
           "repeats": bool(torch.equal(again, clean)), "seconds": round(time.time() - t0, 2)}
    err = _log(f"control.{name}", rec)
    print(rec)
    _fresh(model)
    assert rec["repeats"]
    assert rec["nan_elements"] > 0, "NaN in the conditioner's results did not reach the score"
    assert rec["finite_differs"], "finite poison in the conditioner's results did not change the score"
    assert err is None, err


# ---- 3a - d. the cases --------------------------------------------------------------------------------------------------------
def _widths():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_fp64_widths.json")) as f:
        return json.load(f)


def _families_taken(model, spec, case, state):
    """An unpoisoned, profiled pass of the case's call: the families of its conv launches, and its launch count."""
    model.profile(True)
    try:
        W.RUNNERS[case.call](model, spec, state, **case.kw)
        records = model.profile_read(32768)
    finally:
        model.profile(False)
    return {V.family_of(r[3]) for r in records if not V.is_recurrence_record(r[3])}, model.launch_stats()[0]


@pytest.mark.parametrize("cid", [c.id for c in W.CASES])
def test_case(cid, steer):
    t0 = _begin()
    case = W.BY_ID[cid]
    fills = W.NAN_EXEMPT[cid][0] if cid in W.NAN_EXEMPT else W.FILLS
    assert "finite" in fills and "zero" in fills
    model, spec = W.get(case.model)
    run = W.RUNNERS[case.call]
    state = {}
    took = None
    try:
        if case.opts:
            steer.set(**case.opts)
        _fresh(model)
        if case.family in CF.FAMILIES:
            fams, _ = _families_taken(model, spec, case, state)
            want = CF.FAMILIES[case.family][1]
            took = sorted(fams)
            if want == ("fused",) and case.call == "var" and case.opts["mask_fused"] == 0:
                # Runner::plan_chain: with separate mask launches a ragged batch takes no fused body (it has no place to mask
                # inside): the option set runs, the three generic launches take the layers
                assert "fused" not in fams, (cid, "took", took)
            else:
                # every family under test that took layers in the same case of test_gpu_conv_fp64.py (same options, batch and
                # frames: tests/golden/conv_fp64_widths.json) has to have taken some here; a ragged call under a family's options
                # and the batch-4 one-frame cases have no record there: one of the wanted families
                rec = _widths().get(CF.case_id(case.family, case.model[1], case.kw["B"], case.kw["frames"])) if case.call == "plain" else None
                need = [f for f in want if rec.get(f)] if rec else []
                assert all(f in fams for f in need) and any(f in fams for f in want), (cid, "took", took, "wanted", need or want)
            _fresh(model)
        elif case.family == "fir_alone":
            n_with = _families_taken(model, spec, case, state)[1]
            steer.unset("fuse_upfir", "rate_small")
            n_default = _families_taken(model, spec, case, state)[1]
            steer.set(**case.opts)
            took = [n_with, n_default]
            assert n_with > n_default, (cid, "the stand-alone FIR passes add launches", n_with, n_default)
            _fresh(model)
        elif case.family == "gru_chunked":
            assert int(model.get_option("gru_bmax")) == 1
        base = run(model, spec, state, **case.kw)
        frames, cond_rows, aux = base.get("frames"), base.get("cond_rows"), base.get("aux", False)
        taps = W.read_taps(model, spec, cond_rows)
        base_taps = (taps, W.copy_taps(model, taps))
        equal, taps_equal, tails, differ, n_tail, n_cmp, unwritten, written = {}, {}, {}, {}, 0, 0, [], set()
        for fill in [f for f in fills if f != "zero"] + ["zero"]:  # (`zero` last: which taps the call writes is known by then)
            snap = W.poison(model, fill)
            got = run(model, spec, state, **case.kw)
            equal[fill] = _same(base, got)
            rep = W.check_taps(model, spec, snap, base_taps, fill, written, frames, cond_rows, aux)
            taps_equal[fill] = not rep["differ"]
            n_cmp += rep["compared"]
            n_tail += rep["tail_elements"]
            unwritten = sorted(set(unwritten) | set(rep["unwritten"]))
            if rep["differ"]:
                differ[fill] = rep["differ"]
            if rep["tail_bad"]:
                tails[fill] = rep["tail_bad"]
        finite_out = all(bool(torch.isfinite(v).all()) for v in base.values() if torch.is_tensor(v))
        rec = {"equal": equal, "taps_equal": taps_equal, "taps_compared": n_cmp, "taps_differ": differ, "unwritten": unwritten,
               "seconds": round(time.time() - t0, 2), "fns": list(case.fns)}
        if frames is not None:
            rec.update(tail_elements=n_tail, tail_bad=tails)
        if took is not None:
            rec["took"] = took
        err = _log(cid, rec)
        print(cid, rec)
        assert finite_out, (cid, "the unpoisoned call's output is not finite")
        assert all(equal.values()), (cid, "the call's result depends on what its workspace held before", equal)
        assert n_cmp > 0 and not differ, (cid, "taps depend on what the workspace held before", differ)
        if case.call == "var" or case.kw.get("rows") or case.kw.get("which") in ("var", "var_ens"):
            assert frames is not None, (cid, "a ragged call whose taps hold no ragged walk")
        if frames is not None:
            assert n_tail > 0 and not tails, (cid, "non-zero elements behind a row's end", tails)
        assert err is None, err
    finally:
        state.clear()
        _fresh(model)


# ---- 3e. inputs and outputs outside the rows ----------------------------------------------------------------------------------
SENTINEL = 7.0


def _forward(model, fn, bufs, dims, n_steps, eps, ws, scratch):
    """Universe._forward by keyword.  (e) calls it directly because the front end's methods allocate `out` / `members_out`
    themselves, and these tests have to hand in buffers prefilled with a sentinel."""
    model._forward(fn, bufs, dims, n_steps, eps, warm_start=None, flags=0, ws=ws, counter=None, scratch=scratch, cond_key=None)


def _call_var(model, mix, nz, lens, out):
    n_steps, eps = model._begin(W.N_STEPS, None)
    B, _, L = mix.shape
    T = padded(L, model.tot_ds)
    ws = model._workspace(B, T)
    _forward(model, model._L.ou_enhance_var, (mix, out, nz), (B, L, (ctypes.c_int32 * B)(*lens)), n_steps, eps, ws, (B, T))


def _call_ens(model, mix, nz, lens, out, members):
    n_steps, eps = model._begin(W.N_STEPS, None)
    B, _, L = mix.shape
    T = padded(L, model.tot_ds)
    need = ctypes.c_size_t()
    _lib.check(model._L.ou_ensemble_workspace_bytes(model._handle, B, T, W.ENS, ctypes.byref(need)), model._handle)
    ws = model._workspace(W.ENS * B, T, need=need.value)
    _forward(model, model._L.ou_enhance_ensemble, (mix, out, members, nz),
             (B, L, (ctypes.c_int32 * B)(*lens), W.ENS, _lib.ENSEMBLE_STATS["median"]), n_steps, eps, ws, (W.ENS * B, T))


@pytest.mark.parametrize("name,call", W.OUTSIDE)
def test_outside_the_rows(name, call):
    """ou_enhance_var / ou_enhance_ensemble with t_raw: NaN in `mix` behind every row's own samples and in `noise` behind its
    own padded columns changes no bit; `out` and `members_out`, prefilled with a sentinel, are exactly 0 from every row's
    length to the stride."""
    t0 = _begin()
    model, spec = W.get(("zoo", name))
    td = spec.tot_ds
    lens = W.row_sets(td)["mult"]
    B, L = len(lens), max(lens)
    E = W.ENS if call == "ens_var" else 1
    mix = W.mix_of(spec, lens)
    nz = W.noise_of(W.N_STEPS, lens, td, E)
    mix_n, nz_n = mix.clone(), nz.clone()
    for b, n in enumerate(lens):
        mix_n[b, 0, n:] = float("nan")
    for q in range(E * B):
        nz_n[:, q, 0, padded(lens[q % B], td):] = float("nan")
    assert bool(torch.isnan(mix_n).any()) and bool(torch.isnan(nz_n).any())
    _fresh(model)
    res = []
    try:
        for m, z in ((mix, nz), (mix_n, nz_n)):
            out = torch.full((B, 1, L), SENTINEL, device="cuda")
            members = torch.full((E, B, 1, L), SENTINEL, device="cuda") if E > 1 else None
            if E > 1:
                _call_ens(model, m.cuda(), z.cuda(), lens, out, members)
            else:
                _call_var(model, m.cuda(), z.cuda(), lens, out)
            res.append((out, members))
        tail_bad, n_tail = 0, 0
        for out, members in res:
            for b, n in enumerate(lens):
                for t in [out[b, 0, n:]] + ([members[:, b, 0, n:]] if members is not None else []):
                    n_tail += t.numel()
                    tail_bad += int((t != 0).sum())
        same = torch.equal(res[0][0], res[1][0]) and (E == 1 or torch.equal(res[0][1], res[1][1]))
        finite = bool(torch.isfinite(res[0][0]).all())
        rec = {"equal": {"nan_outside": same}, "tail_elements": n_tail, "tail_bad": tail_bad, "seconds": round(time.time() - t0, 2)}
        err = _log(f"e.{call}.{name}", rec)
        print(rec)
        assert finite and same, "NaN behind the rows of mix / noise changed the result"
        assert n_tail > 0 and tail_bad == 0, "out / members_out are not 0 behind the rows"
        assert err is None, err
    finally:
        _fresh(model)


# ---- 3f. call order through the header ----------------------------------------------------------------------------------------
_alone = {}


def _order_call(model, spec, key):
    call, kw = W.ORDER_CALLS[key]
    return W.RUNNERS[call](model, spec, {}, **kw)["out"].clone()


@pytest.mark.parametrize("first,second", W.ORDER_PAIRS)
def test_call_order(first, second):
    """The header carries rows, lens, the coefficient rows, stats and the GRU tags from call to call: the second call's output on
    the shared workspace equals the same call alone on a freshly initialised one."""
    t0 = _begin()
    model, spec = W.get(("zoo", "PP16s"))
    try:
        if second not in _alone:
            _fresh(model)
            _alone[second] = _order_call(model, spec, second)
        _fresh(model)
        _order_call(model, spec, first)
        ws = model._ws
        got = _order_call(model, spec, second)
        shared = model._ws is ws
        same = torch.equal(got, _alone[second])
        err = _log(f"f.{first}.then.{second}", {"equal": {"order": same}, "seconds": round(time.time() - t0, 2)})
        assert shared, "the two calls did not share a workspace"
        assert same, (first, second, "the second call's output depends on the call before it")
        assert err is None, err
    finally:
        _fresh(model)
