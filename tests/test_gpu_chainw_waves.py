"""GPU (-m gpu): the two forms of conv_chainw_kernel (eight waves, two per SIMD, 16x16x4 MFMAs: a wave owns 32 rows x 16 tile
positions) at the shapes where the division of a tile over eight waves can go wrong, through `Universe` and the taps, with the
helpers of tests/test_gpu_conv_fp64.py and tests/conv_fp64.py (imported, not copied).

What the library can be asked for: the 32-channel level runs at T = tot_ds x frames = 160 f columns and the 64-channel level at
80 f, and chainw_kind() takes a body only for T % 4 == 0 and T >= 252 (C = 32) / 126 (C = 64).  T = 250, 254 or 506 can therefore
not reach the kernel; the frame counts below are the smallest that put the same seams under it:

    f =  2   T = 320 / 160      two tiles, the second partial (68 / 34 live columns), rows shorter than two tiles
    f = 52   T = 8320 / 4160    33 whole tiles and a last tile 4 / 2 columns wide: the last wave-owned pair on the seam's halo
    f = 63   T = 10080 / 5040   exactly 40 tiles: the last tile whole, nothing behind it

Every wave's first and last column lies on another wave's window in every tile (a wave owns 32 columns; windows reach 2 + 1 + 1
columns over), so any wrong wave / lane -> column mapping shows at every shape.  Per form and shape: every fused tap element-wise
against float64 within the fused-body bound of conv_fp64.fused_body (v, and the raw conv1 result c1 of the depth-3 form where it
is exported), and against the unfused walk (option fuse = 0) at >= 100 dB per tap.  Ragged: B = 2 through ou_enhance_var (so
ChainArgs::lens is set), rows of 63 and 52 frames: row 0 ends exactly on a seam, row 1 ends 4 / 2 columns behind one with six
whole tiles behind its end -- float64 bound inside the rows, exactly 0 behind them."""
import pytest
import torch

import conv_fp64 as C
import restatement as O
import test_gpu_conv_fp64 as G
from helpers import synth_mix
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

FRAMES = (2, 52, 63)
RAGGED_ROWS = (63, 52)


def _passes(model, spec, frames):
    T = spec.tot_ds * frames
    xin = O.normalize(synth_mix(spec, 1, T, seed=4100 + frames)[:, None, :], spec.level_db).float().contiguous()
    sig = torch.tensor([0.3])
    xs = (torch.randn(xin.shape, generator=torch.Generator().manual_seed(17 + frames)) * sig[:, None, None]).float().contiguous()
    model.condition_model(xin.cuda(), train=True)
    model.score_model(xs.cuda(), sig)


def _fused_reports(reps, form):
    """The reports of the taps the fused kernel wrote, by output kind."""
    v = {k: r for k, r in reps.items() if k.endswith(f".v|fused{form}|19{form}")}
    c1 = {k: r for k, r in reps.items() if k.endswith(f".c1|fused{form}|19{form}")}
    return v, c1


@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("form", [3, 2])
def test_fused_bodies_on_eight_waves(form, frames, steer):
    """form 3: C = 32, depth 3 (cond add + FiLM + c1_out); form 2: C = 64, depth 2."""
    steer.set(fuse=form)
    model, spec, sd = get_model("PP16")
    model.reset_workspace()
    try:
        P = G._P("PP16", spec, sd)
        model.profile(True)
        _passes(model, spec, frames)
        records = model.profile_read(32768)
        model.profile(False)
        T_of = {p: (model.tensor(vn).shape[-1]) for p, q, i, f, a, c1n, vn, ex in P.walk}
        paired = G._pair_with_profile(P, records, 1, T_of)
        reps = {}
        G._check_blocks(reps, P, model, paired, True, G._tap(model, "sigma.film"))
        v, c1 = _fused_reports(reps, form)
        width = 32 if form == 3 else 64
        fused_blocks = [p for p, (d, cfgs) in paired.items() if d == form]
        assert fused_blocks and all(P.blocks[p].C == width for p in fused_blocks), (form, fused_blocks)
        assert len(v) == len(fused_blocks), "every fused body's v is checked"
        if form == 3:
            # conv1's three epilogue operands are under test: a block with the cond add, one with FiLM, an exported c1
            assert c1, "no exported c1 among the depth-3 bodies"
            assert any(a is not None for p, q, i, f, a, *_ in P.walk if p in fused_blocks), "no cond add"
            assert any(f is not None for p, q, i, f, *_ in P.walk if p in fused_blocks), "no FiLM"
        for k, r in list(v.items()) + list(c1.items()):
            print(f"form {form} f{frames} {r}")
        for k, r in list(v.items()) + list(c1.items()):
            assert r.excluded == 0 and r.ok(), f"form {form} f{frames} {r}"
        # the same passes unfused: >= 100 dB per tap
        names = [(p, c1n if ex else None, vn) for p, q, i, f, a, c1n, vn, ex in P.walk if p in fused_blocks]
        got = {n: G._tap(model, n) for p, c1n, vn in names for n in (c1n, vn) if n}
        steer.set(fuse=0)
        model.reset_workspace()
        _passes(model, spec, frames)
        for n, t in got.items():
            snr = O.si_sdr(G._tap(model, n).flatten()[None], t.flatten()[None])
            print(f"form {form} f{frames} {n}: {snr:.1f} dB against the unfused walk")
            assert snr >= 100.0, (n, snr)
    finally:
        model.profile(False)
        model.reset_workspace()


def test_fused_bodies_of_a_ragged_batch_on_eight_waves(steer):
    steer.set(mask_fused=1, no_overlap=1)  # (fuse: the cost model -- small ragged batches keep both fused forms)
    model, spec, sd = get_model("PP16")
    model.reset_workspace()
    try:
        P = G._P("PP16", spec, sd)
        td, rows = spec.tot_ds, RAGGED_ROWS
        t_raw = [f * td - 3 for f in rows]
        B, lm, T = len(t_raw), max(t_raw), max(rows) * td
        sigs = [synth_mix(spec, 1, n, seed=700 + i)[0] for i, n in enumerate(t_raw)]
        mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs])[:, None, :]
        nz = torch.zeros(2, B, 1, T)
        for b in range(B):
            nz[:, b, 0, :rows[b] * td] = torch.randn(2, rows[b] * td, generator=torch.Generator().manual_seed(980 + b))
        model.profile(True)
        model._enhance(mix.cuda(), 2, None, None, None, None, False, False, None, "median", None, nz.cuda(), t_raw=list(t_raw))
        records = model.profile_read(32768)
        model.profile(False)
        T_of = {p: (model.tensor(vn).shape[-1]) for p, q, i, f, a, c1n, vn, ex in P.walk}
        n_cond = sum(1 for p, *_ in P.walk if p.startswith("cond."))
        full = P.walk
        try:
            P.walk = full[:n_cond]
            paired = G._pair_with_profile(P, records, B, T_of)
            P.walk = full[n_cond:]
            paired.update(G._pair_with_profile(P, G._last_pass(records), B, T_of))
        finally:
            P.walk = full
        film = G._tap(model, "sigma.film")[1:2].expand(B, -1, -1)
        lens_of = lambda Tl: [f * (Tl // max(rows)) for f in rows]  # noqa: E731
        reps = {}
        G._check_blocks(reps, P, model, paired, True, film, lens_of)
        for form in (3, 2):
            v, c1 = _fused_reports(reps, form)
            assert v, f"no depth-{form} body ran fused on this ragged batch"
            assert form == 2 or c1, "no exported c1 among the depth-3 bodies"
            for k, r in list(v.items()) + list(c1.items()):
                print(f"ragged {r}")
                assert r.excluded == 0 and r.ok(), f"ragged {r}"
                assert r.tail_bad == 0, f"ragged {k}: {r.tail_bad} elements behind a row's end are not exactly 0"
    finally:
        model.profile(False)
        model.reset_workspace()
