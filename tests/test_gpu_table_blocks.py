"""GPU (-m gpu): every by-value row table of the library past its first block.

The library passes per-row values to kernels by value, as kernel arguments, a fixed block at a time; a host loop issues one
launch per block with an offset (`off`, `b0`, `j0`, `dst + i`).  The cases of tests/table_blocks_cases.py make every such loop
take a second (and a third) turn, with values at the rows 63, 64, 65 (15, 16, 17 for the reduce) that no other row has; the
checks are those of the float64 modules the suite already trusts (small_fp64, seg_fp64, ensemble_ref, snake_fp64) at their own
a-priori bounds, which are per element and know nothing of the batch size, or bit identity.  Every element is held
(`excluded == 0`), behind a row's end against exactly 0.  tests/test_table_blocks_cpu.py holds the case lists.

| Table (block size) | Host loop | Largest count a test reaches |
|---|---|---|
| `CoefBlock` (64 rows): `upload_coefs` -> `upload_coef_kernel`; the sampler's step table (`n_steps` rows, up to `kMaxSteps` = 256) and `ou_score`'s per-row sigmas (B rows); then `launch_sigma_embed` / `launch_film` over the same S rows | `ou_walk.cpp` `upload_coefs` | `n_steps` 256 (all rows of sigma.g / sigma.film read by offset), B 129 (`test_score_rows`, `test_step_table`) |
| `RowBlock` (64): `upload_row_lengths` -> `upload_rows_kernel`, `rows[off + i]` and `lens[l * B + off + i]` | `ou_sampler.cpp` | ragged batches of 129 rows (`test_ragged_batch`) |
| `SegRowBlock` (64): `launch_seg_upload_rows(geom, blk, n, off, ...)` | `ou_segments.cpp` ragged driver | C = 127 (`test_segmented_exact_blocks`; 70 with single-window rows, `test_segmented_many_rows`) |
| `SegEntriesList` (64 entries, `j0`): `for_blocks` feeds `seg_upload_lens`, `seg_gather_input`, `seg_gather_noise`, `seg_stitch`; walk rows `E * Bw` | `ou_segments.cpp` | Bw 128 with 128 real entries; Bw 68 x E 2 = 136 walk rows |
| `EnsLens` (16 inputs, `b0`): `ensemble_reduce_kernel`, `ensemble_pick_kernel` (`hist + b * E`, `pick[b]`) | `ou_ensemble.hip` | B = 33 (`test_ensemble_reduce`) |
| `SnakeRows` (64): `ou_snake_act` stateless loop | `ou_stateless.cpp` | B = 130 (`test_stateless_snake`) |
| `NoiseRows`, `ResampleRows`, `MetRows` (64) | -- | 70, 65 and 130 rows (tests/test_gpu_noise.py, test_gpu_resample_fp64.py, test_gpu_metrics.py) |

`Replicator` (16 tensors per launch) cannot reach a second launch at any accepted topology: with at most 4 rate levels it adds
at most 14 entries (two per conditioner decoder block, aux, latent, mixn, stats, mel_scale, wav).  No case is built for it.
The next by-value table added to the library gets a row above and a case list in tests/table_blocks_cases.py.

The sampler uploads ALL n_steps rows of its table (coefficients, embeddings and FiLM rows) whatever warm_start says, so
`test_step_table` holds all of them.  Figures: build/observed/table_blocks_observed.json (untracked) before anything is asserted --
the worst err / bound per check and the seconds of every test --; profiles/table_blocks_observed.json is the committed copy.
The segmented cases run through test_gpu_seg_fp64._run_case, which logs them a second time, as `table_blocks.*` entries of the
untracked build/observed/seg_fp64_observed.json: profiles/seg_fp64_observed.json, the committed copy of that file's own cases,
does not hold them."""
import json
import os
import time

import numpy as np
import pytest
import torch

import ensemble_ref as R
import restatement as O
import seg_fp64 as G
import small_fp64 as F
import snake_fp64 as SN
import table_blocks_cases as K
from helpers import record, synth_mix, worst
from open_universe_amd.universe import ensemble_reduce
from test_gpu_parity import get_model, noise_list, run_enhance
from test_gpu_ragged import _run_alone
from test_gpu_seg_fp64 import _run_case, _seg_tap
from test_gpu_small_fp64 import _condition_reports, _P, _score_reports, _tap
from test_gpu_snake_fp64 import _tile, snake_act

pytestmark = pytest.mark.gpu

_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed")


def _finish(case, reps, t0, extra=None):
    """Log (the way the fp64 modules do), print, then assert.  `reps`: {check: small_fp64.Report}; `extra`: plain figures."""
    log_error = None
    try:
        os.makedirs(_OUT, exist_ok=True)
        path = os.path.join(_OUT, "table_blocks_observed.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[case] = {"seconds": round(time.time() - t0, 2)}
        old[case].update(extra or {})
        for k, r in reps.items():
            old[case][k] = {"err": r.err, "ratio": round(r.ratio, 4), "bad": r.n_bad, "tail_bad": r.tail_bad, "checked": r.checked,
                            "excluded": r.excluded}
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


# ---- 1. coefficient, embedding and FiLM rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", K.SCORE_CASES)
def test_score_rows(name, B):
    """ou_score with one sigma per row, B = 65 and 129 at one frame: upload_coefs in 2 and 3 launches, sigma_embed_kernel and
    film_kernel over all B rows, in_conv_kernel and out_conv_kernel with row b's own coefficients."""
    t0 = time.time()
    model, spec, sd = get_model(name)
    P = _P(name, spec, sd)
    xin = O.normalize(synth_mix(spec, B, spec.tot_ds, seed=1100)[:, None, :], spec.level_db).float().contiguous()
    model.condition_model(xin.cuda(), train=True)
    reps = {}
    _score_reports(reps, model, spec, P, xin.shape, K.score_sigmas(spec, B), 41)
    assert all(r.checked and r.checked % B == 0 for r in reps.values())  # every row of every tap
    _finish(f"score_rows.{name}.b{B}", reps, t0)
    model.reset_workspace()


@pytest.mark.parametrize("N", K.STEP_N)
def test_step_table(N):
    """enhance(n_steps = N, warm_start = N - 1): one step at table row N - 1 -- score.in and the fused update against that row's
    sigma --, and ALL N rows of sigma.g and sigma.film (read by their workspace offset: the named taps are sized by B) against the
    host's sigma table.  The driver uploads every row of the table, not only those from warm_start on.  Of the rows other than
    N - 1 this holds the field sigma_net alone (what the embedding reads): their other StepCoef fields (c1, the noise
    coefficients) are read by no launch of a one-step call and leave no tap."""
    t0 = time.time()
    name, B, frames = K.STEP_MODEL, K.STEP_B, K.STEP_FRAMES
    model, spec, sd = get_model(name)
    P = _P(name, spec, sd)
    T = spec.tot_ds * frames
    mix = synth_mix(spec, B, T - 5, seed=70)
    noise = noise_list(23, 1, B, T)
    run_enhance(model, mix, noise, n_steps=N, warm_start=N - 1)
    table = model._sigma_table(N).cpu()
    assert torch.equal(table, K.sigma_table(spec, N)), "the case list's schedule is not the host's"
    sigma = float(table[N - 1])
    coef = F.edm_coef(spec, [sigma] * B)
    x0 = F.init_x(noise[0], sigma, _tap(model, "wav"))
    reps = {}
    ref, bound = F.in_conv(x0, P.s_in_w, P.s_in_b, coef["w_in"] if P.edm else None)
    reps["score.in"] = F.Report("score.in(shared)", _tap(model, "score.in"), ref, bound)
    last = len(spec.score.rate_factors) + int(spec.score.extra_conv_block) - 1
    score, sb = F.out_conv_score(_tap(model, f"score.dec{last}.v"), x0, P, coef)
    ref, bound = F.sampler_update(x0, score, float(coef["sig2"][0]), score_bound=sb)
    reps["out_conv.update"] = F.Report("out_conv.update", _tap(model, "x"), ref, bound)
    g = _seg_tap(model, "sigma.g", N)
    assert g.shape == (N, P.D, 1)
    reps["sigma_embed"] = F.check_sigma_embed(g, F.edm_coef(spec, table)["sigma_net"], P)
    ref, bound = F.film(g, P.film_w, P.film_b)
    reps["film"] = F.Report("film", _seg_tap(model, "sigma.film", N), ref.reshape(N, -1, 1), bound)
    assert reps["sigma_embed"].checked == N * P.D and reps["film"].checked == N * P.film_w.shape[0]
    _finish(f"step_table.{name}.N{N}", reps, t0)


# ---- 2. ragged batch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_fused", [0, 1])
@pytest.mark.parametrize("name,B", K.RAGGED_CASES)
def test_ragged_batch(name, B, mask_fused, steer):
    """ou_enhance_var on 65 and 129 rows of 1 .. 5 frames (the body of test_gpu_small_fp64.test_ragged_batch): upload_rows_kernel
    in 2 and 3 launches into a [level][B] table with B no multiple of 64.  pad_normalize_var / post_var (keep_rms) with every
    row's own geometry, the conditioner's seams with the row's own frames, exactly 0 behind every row's end; the rows 0, 63, 64
    and B - 1 against the same row alone at the gate tests/test_gpu_ragged.py applies to its small models (80 dB, SI-SDR and
    plain SNR)."""
    t0 = time.time()
    steer.set(mask_fused=mask_fused)
    model, spec, sd = get_model(name)
    model.reset_workspace()
    try:
        P = _P(name, spec, sd)
        td = spec.tot_ds
        rows, t_raw = K.ragged_rows(B, td)
        lm = max(t_raw)
        T = lm + (td - lm % td)
        sigs = [synth_mix(spec, 1, n, seed=300 + i)[0] for i, n in enumerate(t_raw)]
        mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs])[:, None, :]
        nz = torch.zeros(2, B, 1, T)
        for b, f in enumerate(rows):
            nz[:, b, 0, :f * td] = torch.randn(2, f * td, generator=torch.Generator().manual_seed(900 + b))
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
        alone = []
        for b in K.ALONE_ROWS(B):
            one = _run_alone(model, sigs[b], [nz[k, b:b + 1, :, :rows[b] * td] for k in range(2)], 2, keep_rms=True)
            alone.append(O.si_sdr(one, out[b, 0, :t_raw[b]]))
        w = worst(alone)
        case = f"ragged.{name}.b{B}.mask_fused{mask_fused}"
        _finish(case, reps, t0, {"worst_row_vs_alone_db": min(float(w), 999.0)})
        record(f"table_blocks.{case}.worst_row_vs_alone", w, 80)
    finally:
        model.reset_workspace()


# ---- 3. segmented ragged call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,share", [(1, 1), (2, 1), (2, 0)])
def test_segmented_many_rows(E, share):
    """enhance_long_many (E = 2: enhance_long_many_ensemble, ens_share at its default and at 0) on 70 rows: the SegRow table in two
    launches, and a last group of 68 single-window entries of lengths of their own -- seg_upload_lens, seg_gather_input,
    seg_gather_noise and seg_stitch in two launches each, E x 68 walk rows (member rows m Bw + slot, noise rows m C + c).  Every
    check of test_gpu_seg_fp64._run_case: stats, row_scale, gather, noise, stitch with the tails, post for every row."""
    t0 = time.time()
    name = K.SEG_MODEL
    model, spec, sd = get_model(name)
    td = spec.tot_ds
    Sg, Ov = G.seg_so(td)
    lens = K.seg_many_rows(td)
    C, mb = len(lens), K.SEG_MANY[E]
    assert C > 64
    geos = [G.Row(n, td, Sg, Ov) for n in lens]
    Bw, real, slots, n_groups, T = G.last_group(geos, mb, True, E)
    assert Bw >= 65 and len(real) >= 65 and E * Bw >= 65 * E
    model.set_option("ens_share", share)
    try:
        case = f"seg_many.{name}.E{E}.share{share}"
        reps, _ = _run_case("table_blocks." + case, name, lens, Sg, Ov, max_batch=mb, ragged=True, E=E)
        assert {"stats", "row_scale", "gather", "noise", "stitch", "post"} <= set(reps)
        assert reps["noise"].checked == E * Bw * T and reps["gather"].checked >= Bw * T
        _finish(case, reps, t0)
    finally:
        model.set_option("ens_share", 1)
        model._seg_ws = None
        model.reset_workspace()


@pytest.mark.parametrize("n_real", K.SEG_EXACT)
def test_segmented_exact_blocks(n_real):
    """A FULL last group of exactly 64 and exactly 128 real entries (n == kSegEntriesPerLaunch: no short block, no filler), whose
    first entry -- and the first entry of every launch block in it -- is a second window: the group's first crossfades with
    seg.carry, a block's first with the walk row in front of it, which the launch before handled."""
    t0 = time.time()
    name = K.SEG_MODEL
    model, spec, sd = get_model(name)
    td = spec.tot_ds
    Sg, Ov = G.seg_so(td)
    lens = K.seg_exact_rows(td, n_real)
    geos = [G.Row(n, td, Sg, Ov) for n in lens]
    Bw, real, slots, n_groups, T = G.last_group(geos, n_real, True, 1)
    assert Bw == len(real) == n_real and n_groups == 2 and real[0][1] > 0
    try:
        case = f"seg_exact.{name}.n{n_real}"
        reps, _ = _run_case("table_blocks." + case, name, lens, Sg, Ov, max_batch=n_real, ragged=True)
        assert {"stats", "row_scale", "gather", "noise", "stitch", "post"} <= set(reps)
        _finish(case, reps, t0)
    finally:
        model._seg_ws = None
        model.reset_workspace()


# ---- 4. ensemble reduce -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", K.ENS_E)
def test_ensemble_reduce(E):
    """ou_ensemble_reduce on 16 (one full launch), 17 and 33 inputs with a length of its own each: median and signal median bit
    for bit against ensemble_ref.reduce_ref (the picks too: input 16 picks another member than input 0), the mean within
    mean_bound, 0 from len[b] on, nothing behind `cols` touched, two runs identical.  Row strides off (rs % 4 != 0: every access
    word by word) and on 16-byte boundaries (the 16-byte loads and stores, which 3 columns are too few for: there both strides
    run word by word); 4097 columns are five column blocks per input."""
    t0 = time.time()
    worst_mean, n = 0.0, 0
    for B in K.ENS_B:
        for cols in K.ENS_COLS:
            x, lens = K.ens_members(E, B, cols, ties=(B + cols) % 2 == 0)
            refs = {stat: R.reduce_ref(x, stat, lens) for stat in R.STATS if stat != "mean"}
            if B > 16:
                assert int(refs["signal_median"][1][0]) != int(refs["signal_median"][1][16])
            xv = x.clone()
            for b in range(B):
                xv[:, b, lens[b]:] = 0
            m64 = xv.double().mean(dim=0)
            bound = R.mean_bound(xv, m64)
            for rs in K.ens_strides(cols):  # rows off, then on 16-byte boundaries: the scalar and -- cols 4097 -- the 16-byte path
                buf = torch.full((E * B, rs), 9.0)
                buf[:, :cols] = x.reshape(E * B, cols)
                buf = buf.cuda()
                mem = buf.view(E, B, rs)[:, :, :cols]
                for stat in R.STATS:
                    outs, picks = [], []
                    for rep in range(2):
                        full = torch.full((B, rs), 7.0, device="cuda:0")
                        out, pick = ensemble_reduce(mem, stat, lens, return_pick=True, out=full[:, :cols])
                        outs.append(out.cpu())
                        picks.append(None if pick is None else pick.cpu())
                        assert (full[:, cols:] == 7.0).all()  # nothing behind `cols` is touched
                    what = (E, B, cols, rs, stat)
                    assert torch.equal(outs[0], outs[1]), what  # two runs: identical bits
                    got = outs[0]
                    for b in range(B):
                        assert not got[b, lens[b]:].any(), what + (b,)  # zero from len[b] on
                    if stat == "mean":
                        err = (got.double() - m64).abs()
                        worst_mean = max(worst_mean, float((err / bound.clamp(min=1e-300))[err > 0].max()) if bool((err > 0).any()) else 0.0)
                        assert (err <= bound).all(), what
                    else:
                        assert torch.equal(got, refs[stat][0]), what  # bit-exact
                    if stat == "signal_median":
                        assert torch.equal(picks[0], refs[stat][1]) and torch.equal(picks[1], refs[stat][1]), what
                    n += 1
    _finish(f"ensemble_reduce.E{E}", {}, t0, {"mean_worst_err_over_bound": round(worst_mean, 4), "reduces_held": n})


# ---- 5. stateless Snake ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [False, True])
@pytest.mark.parametrize("B", K.SNAKE_B)
def test_stateless_snake(B, beta):
    """ou_snake_act on 65 and 130 rows of 2 channels with lengths of their own either side of the tile edges (and 1, and T):
    SnakeRows in 2 and 3 launches.  Against snake_fp64.snake_act at the allowance of test_gpu_snake_fp64.py; exactly 0 behind
    every row; the rows at the block edges equal the same row run alone, bit for bit."""
    t0 = time.time()
    rec = SN.ref_error()
    tile = _tile()
    assert rec["tile"] == tile
    allowed = SN.KERNEL_FACTOR * rec["max_rel"]
    C, T = K.SNAKE_C, K.snake_T(tile)
    lens = K.snake_lens(B, tile)
    x, la, lb = SN.case_input(T, C, B, beta)
    ea, eb = SN.exp32(la), SN.exp32(lb)
    ref = SN.snake_act(x, ea, eb, lens)
    figures = {}
    for stride in (None, (T + 3) // 4 * 4 + 4):
        y = snake_act(x, ea, eb, lens, stride)
        assert np.isfinite(y).all()
        err = SN.rel_error(y, ref)
        figures["rel_err" + ("" if stride is None else ".padded")] = err
        print(f"snake.b{B}.beta{int(beta)} stride {stride}: kernel {err:.3e} allowed {allowed:.3e}")
        for b, n in enumerate(lens):
            assert not y[b, :, n:].any(), f"row {b} is not zero behind its end"
        for b in sorted(set(K.edge_rows(B, 64)) | {0, B - 1}):
            alone = snake_act(np.ascontiguousarray(x[b:b + 1, :, :lens[b]]), ea, eb)
            assert np.array_equal(alone.view(np.int32), y[b:b + 1, :, :lens[b]].view(np.int32)), (b, stride)
    figures["allowed"] = allowed
    figures["ratio"] = round(max(v for k, v in figures.items() if k.startswith("rel_err")) / allowed, 4)
    _finish(f"snake.b{B}.{'beta' if beta else 'alpha'}", {}, t0, figures)
    assert figures["ratio"] <= 1.0, figures
