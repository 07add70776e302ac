"""GPU (-m gpu): the segmented-enhance kernels of ou_segment.hip against the float64 definitions of tests/seg_fp64.py, sample by
sample.  Every check takes the kernel's inputs from the library's own taps of the same call (`seg.stats`, `seg.row_scale`,
`seg.carry`, `seg.z`, and the walk's `mixn`, `mel_scale`, `x`, which hold the LAST group's rows), evaluates in float64 and holds
every element; none is excluded.

    seg_stats1 / 2 / finish (plain and GEN)   mix rows -> seg.stats
    seg_mel_energy, mel scale (both forms)    mix, seg.stats -> seg.row_scale; mel_scale tap == the row's scale, exactly
    seg_gather_input                          mix, seg.stats -> mixn
    seg_gather_noise                          the call's noise, last draw -> seg.z (exact)
    seg_stitch                                x (and seg.carry) -> returned rows of the call with keep_rms off, guard idle
    seg_post_reduce / seg_post_scale          those rows -> the rows of the same call with keep_rms on (two runs are bit-identical)
    seg_upload_rows / seg_upload_lens         through the rows and zero tails they place

What only earlier groups wrote cannot be seen element by element (their walk rows are overwritten): with several groups the
stitch is held from the last group's first w0 to the rows' ends.  Figures: build/observed/seg_fp64_observed.json (untracked)
before anything is asserted; profiles/seg_fp64_observed.json is the committed copy."""
import json
import os
import time
from ctypes import byref, c_int32, c_size_t

import pytest
import torch

import seg_fp64 as G
import small_fp64 as F
from helpers import SMALL
from open_universe_amd import Universe, UniverseGAN
from open_universe_amd import config as Cfg
from open_universe_amd import state_dict as S
from open_universe_amd import universe as Umod
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed")
_params = {}
N_STEPS = 2


def _P(name, spec, sd):
    if name not in _params:
        _params[name] = F.Params(spec, sd)
    return _params[name]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _seg_tap(model, name, rows):
    """A tap of the segmented call's own area: `rows` rows of the registered (C, T) at ou_tensor's byte offset (Universe.tensor
    sizes its view by the walk's batch, which these areas do not have)."""
    off, C, T = c_size_t(), c_int32(), c_int32()
    if model._L.ou_tensor(model._handle, name.encode(), byref(off), byref(C), byref(T)) != 0:
        raise KeyError(name)
    n = rows * C.value * T.value
    return model._ws[off.value: off.value + 4 * n].view(torch.float32).view(rows, C.value, T.value).cpu().clone()


def _tap(model, name):
    return model.tensor(name).cpu().clone()


def _finish(case, reps, t0):
    log_error = None
    try:
        os.makedirs(_OUT, exist_ok=True)
        path = os.path.join(_OUT, "seg_fp64_observed.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[case] = {"seconds": round(time.time() - t0, 2)}
        for k, r in reps.items():
            old[case][k] = r.summary()
            if hasattr(r, "lib_ratio"):
                old[case][k].update(e32=r.e32, lib_ratio=round(r.lib_ratio, 3))
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError as e:
        log_error = e
    for k, r in reps.items():
        print(f"{case} {r}" + (f" err / e32 = {r.lib_ratio:.2f}" if hasattr(r, "lib_ratio") else ""))
    for k, r in reps.items():
        assert r.excluded == 0 and r.ok(), f"{case} {r}"
        if hasattr(r, "lib_ratio"):
            assert r.lib_ratio <= F.M_CAP, f"{case} {k}: err / e32 = {r.lib_ratio:.2f} is a finding, not a tolerance"
    assert log_error is None, f"{case}: could not write the observed figures: {log_error}"


class _Spy:
    """Keeps what Universe._segments_run got and returned: the full (C, stride) output with its tails, the members."""

    def __init__(self, model):
        self.model, self.out, self.members = model, None, None
        self.orig = model._segments_run

    def __enter__(self):
        def run(plan, x, n_steps, epsilon, keep_rms, noise, counter, members=None):
            self.out = self.orig(plan, x, n_steps, epsilon, keep_rms, noise, counter, members)
            self.members = members
            return self.out
        self.model._segments_run = run
        return self

    def __exit__(self, *a):
        del self.model._segments_run


def _call(model, rows, Sg, Ov, max_batch, ragged, E, keep_rms, seed):
    """The public call of the case on a generator; -> the (E C, stride) rows before the reduce (E = 1: the result)."""
    fs = model.fs
    kw = dict(segment_s=Sg / fs, overlap_s=Ov / fs, max_batch=max_batch, n_steps=N_STEPS, keep_rms=keep_rms)
    with _Spy(model) as spy:
        if ragged and E > 1:
            model.enhance_long_many_ensemble([r.cuda() for r in rows], E, "median", rngs=_gen(seed), return_members=True, **kw)
        elif ragged:
            model.enhance_long_many([r.cuda() for r in rows], rngs=_gen(seed), **kw)
        elif E > 1:
            model.enhance_long_ensemble(torch.stack(rows).cuda(), E, "median", rng=_gen(seed), return_members=True, **kw)
        else:
            model.enhance_long(torch.stack(rows).cuda(), rng=_gen(seed), **kw)
    torch.cuda.synchronize()
    res = spy.out if E == 1 else spy.members
    return res.reshape(E * len(rows), -1).cpu().clone()


def _noise(model, rows, ragged, E, seed):
    """The noise the call draws from that generator: (n_steps, E C, T_pad max), by the front end's own draw function."""
    if ragged:
        nz = Umod.draw_noise(model.tot_ds, [(1, int(r.numel()), g) for r, g in zip(rows, [_gen(seed)] * len(rows))], N_STEPS, E,
                             device=model.device)
        return nz[:, :, 0].cpu()
    return model.draw_noise_like_enhance(_gen(seed), E * len(rows), rows[0].numel(), N_STEPS).cpu()


def _run_case(case, name, lens, Sg, Ov, max_batch=32, ragged=False, E=1, stitch=True, post=True, model_spec=None, seed=50):
    """One segmented call (twice: keep_rms off, then on) and every check its taps allow."""
    t0 = time.time()
    if model_spec is None:
        model, spec, sd = get_model(name)
    else:
        model, spec, sd = model_spec
    P = _P(name, spec, sd)
    td = spec.tot_ds
    geos = [G.Row(n, td, Sg, Ov) for n in lens]
    C = len(geos)
    rows = G.case_mix(spec, lens)
    Bw, real, slots, n_groups, T = G.last_group(geos, max_batch, ragged, E)
    reps = {}

    out = _call(model, rows, Sg, Ov, max_batch, ragged, E, False, seed)
    stats = _seg_tap(model, "seg.stats", C)[:, :, 0]
    reps["stats"] = G.check_stats(stats, rows, td, spec.level_db, str(spec.norm), bool(spec.zero_mean), float(spec.norm_eps))
    scale = _seg_tap(model, "seg.row_scale", C)[:, 0, 0]
    reps["row_scale"] = G.check_row_scale(scale, rows, geos, stats, P)
    x = _tap(model, "x")
    assert x.shape == (E * Bw, 1, T), (x.shape, E, Bw, T)
    share = E > 1 and int(model.get_option("ens_share")) != 0
    mixn = _tap(model, "mixn")[: (Bw if share or E == 1 else E * Bw)]
    ms = _tap(model, "mel_scale")[: mixn.shape[0], 0, 0]
    want = torch.stack([scale[c] for c, _ in slots] * (mixn.shape[0] // Bw))
    assert torch.equal(ms, want), (case, "mel_scale tap is not the row's scale", ms, want)
    reps["gather"] = G.check_gather(mixn, rows, geos, stats, slots * (mixn.shape[0] // Bw))
    nz = _noise(model, rows, ragged, E, seed)
    reps["noise"] = G.check_noise(_seg_tap(model, "seg.z", E * Bw), nz[N_STEPS - 1], geos, slots, Bw, E, C)
    if stitch:
        carry = None
        if real[0][1] > 0:
            assert n_groups > 1
            carry = _seg_tap(model, "seg.carry", E)
        reps["stitch"] = G.check_stitch(out, geos, real, x, carry, Bw, E, C, whole=n_groups == 1, tails=ragged)
        # the premise of reading the stitch's bits in the output: the post step returned early (keep_rms off, guard idle)
        assert reps["stitch"].ref_peak < 1.0 - 1e-3, (case, "the peak guard was not idle", reps["stitch"].ref_peak)
    if post:
        kept = _call(model, rows, Sg, Ov, max_batch, ragged, E, True, seed)
        assert torch.equal(_seg_tap(model, "seg.stats", C)[:, :, 0], stats), "two runs differ"
        reps["post"], divided, margin = G.check_post(kept, out, rows, geos, E)
        print(f"{case} post: divided {divided}, |peak - 1| over the bound's 8 u: {margin:.3g}")
        assert margin > 1.0, (case, "the reference's peak is within the post bound of 1: the branch is ambiguous")
        if lens[0] >= 16:  # (keep_rms restores the mix's rms: the loud row's peak is the mix's own, 6; a row of 1 or 3 samples has none)
            assert divided[0] and not divided[1], (case, "the loud row was meant to make the peak guard divide, the quiet one not")
    _finish(case, reps, t0)
    return reps, model


@pytest.mark.parametrize("idx", range(10))
@pytest.mark.parametrize("name", G.MODELS)
def test_one_group_sees_every_window(name, idx):
    """enhance_long on 2 rows of one length, max_batch >= entries: every window of the call is in the taps."""
    td = get_model(name)[1].tot_ds
    Sg, Ov = G.seg_so(td)
    n = G.lengths(td)[idx]
    t4, p4, heads, _ = G.coverage(td)
    assert t4 == p4 == heads == {0, 1, 2, 3}
    reps, _ = _run_case(f"one_group.{name}.T{n}", name, [n, n], Sg, Ov)
    assert reps["stitch"].held == 2 * n


@pytest.mark.parametrize("edge", G.OVERLAP_EDGES)
@pytest.mark.parametrize("name", G.MODELS)
def test_overlap_edges(name, edge):
    """O = 0: no crossfade, the shifted last window still cut at w0; O = S / 2: the largest overlap the plan takes."""
    td = get_model(name)[1].tot_ds
    Sg, _ = G.seg_so(td)
    Ov = 0 if edge == "0" else Sg // 2
    n = 58 * td + 3
    g = G.Row(n, td, Sg, Ov)
    assert g.n_win >= 4 and g.starts[-1] != (g.n_win - 1) * g.hop
    _run_case(f"overlap_edge.{name}.O{Ov}", name, [n, n], Sg, Ov, post=False)


@pytest.mark.parametrize("name", G.MODELS)
def test_several_groups_with_a_carry(name):
    """max_batch 4: the taps hold the last group, whose first entry crossfades with seg.carry.  The regions of the earlier groups
    cannot be seen element by element (their walk rows are gone): the stitch is held from the last group's first w0 on."""
    td = get_model(name)[1].tot_ds
    Sg, Ov = G.seg_so(td)
    n = G.CARRY_LENGTH(td)
    geos = [G.Row(n, td, Sg, Ov)] * 2
    _, real, _, n_groups, _ = G.last_group(geos, 4, False)
    assert n_groups > 1 and real[0][1] > 0
    reps, _ = _run_case(f"carry.{name}", name, [n, n], Sg, Ov, max_batch=4)
    c, k = real[0]
    assert reps["stitch"].held == n - (geos[0].window(k)[2] - geos[0].pad_left)


@pytest.mark.parametrize("which", ["full_and_short", "full_with_carry"])
@pytest.mark.parametrize("name", G.MODELS)
def test_ragged_call(name, which):
    """enhance_long_many: once with one FULL and one SHORT group (the SHORT one is the last: its rows and every row's zero tail),
    once with the multi-window rows alone in groups of 4 (the last group FULL, in front of it a carry)."""
    td = get_model(name)[1].tot_ds
    Sg, Ov = G.seg_so(td)
    lens, mb = (G.ragged_lengths(td), 32) if which == "full_and_short" else (G.ragged_multi(td), 4)
    _, model = _run_case(f"ragged.{which}.{name}", name, lens, Sg, Ov, max_batch=mb, ragged=True)
    model._seg_ws = None


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", G.MODELS)
def test_ensemble_members(name, ragged):
    """E = 2, return_members: the member rows (member-major walk rows, noise rows m C + c).  The reduce is test_gpu_ensemble.py's."""
    td = get_model(name)[1].tot_ds
    Sg, Ov = G.seg_so(td)
    lens = [41 * td + 7, 57, 16 * td] if ragged else [41 * td + 7] * 2
    _, model = _run_case(f"ensemble.{'ragged' if ragged else 'alike'}.{name}", name, lens, Sg, Ov, ragged=ragged, E=2)
    model._seg_ws = None


@pytest.mark.parametrize("ragged", [False, True])
def test_multi_block_reductions(ragged):
    """Rows longer than 2^18 samples: 2 reduce blocks per row alike; 2 / 1 / 3 blocks of a partial stride of 3 in the ragged call,
    where blocks past a row's own share return early.  Statistics, row scale and the post step with keep_rms."""
    name = "PP16s"
    model, spec, _ = get_model(name)
    Sg, Ov = 8 * spec.fs, spec.fs
    lens = G.MULTI_BLOCK_RAGGED if ragged else [G.MULTI_BLOCK_ALIKE] * 2
    _run_case(f"multi_block.{'ragged' if ragged else 'alike'}.{name}", name, lens, Sg, Ov, ragged=ragged, stitch=False)
    model._seg_ws = None
    model.reset_workspace()


_norm_models = {}


@pytest.mark.parametrize("norm,zero_mean,eps", [pytest.param(n, z, None, id=f"{n}-{z}") for n, z in G.NORM_MODES]
                         + [pytest.param("2-max", True, 1e-3, id="2-max-True-eps0.001")])
def test_statistics_in_every_norm_mode(norm, zero_mean, eps):
    """Every NormMode of ou_set_normalization, zero_mean on and off, at the smallest cases (1 sample; one window): the plain and
    the GEN statistics kernels -- and 2-max with normalization_kwargs.eps = 1e-3, which seg_stats_finish_kernel and
    seg_gather_input_kernel then see routed (the one-sample rows have both norms under it)."""
    key = (norm, zero_mean, eps)
    if key not in _norm_models:
        base, over = SMALL["PP16s"]
        over = dict(over, **{"normalization_norm": int(norm) if norm == "2" else norm, "normalization_kwargs.zero_mean": zero_mean})
        if eps is not None:
            over["normalization_kwargs.eps"] = eps
        spec = Cfg.spec_from_config(Cfg.builtin_config(base, **over))
        sd = S.synthetic_state_dict(spec, seed=0)
        cls = UniverseGAN if spec.kind == "universe_gan" else Universe
        _norm_models[key] = (cls(spec, state_dict=sd, device="cuda:0"), spec, sd)
    ms = _norm_models[key]
    assert (str(ms[1].norm), bool(ms[1].zero_mean), float(ms[1].norm_eps)) == (norm, zero_mean, 1e-5 if eps is None else eps)
    td = ms[1].tot_ds
    Sg, Ov = G.seg_so(td)
    for n in (1, 16 * td - 1):
        _run_case(f"norm.{norm}.zm{int(zero_mean)}{'' if eps is None else '.eps%g' % eps}.T{n}", "PP16s", [n, n], Sg, Ov, stitch=False,
                  post=False, model_spec=ms)
