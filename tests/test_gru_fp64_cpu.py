"""CPU: the float64 GRU reference of tests/gru_fp64.py against torch.nn.GRU, and the sensitivity of its element-by-element
checks -- one defect at a time is planted into an fp32 CPU evaluation of a UNIVERSE++-sized layer (H = 256, 401 frames) and
the teacher-forced check has to flag it where it is, under the tolerance the GPU tests use (tests/test_gpu_gru_fp64.py).
The defects live in CPU tensors only."""
import math

import pytest
import torch

import gru_fp64 as G
import restatement as O

H, I, T, B = 256, 512, 401, 2
P = "g"


def _state_dict(H, I, layers, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for layer in range(layers):
        i = I if layer == 0 else 2 * H
        for sfx in ("", "_reverse"):
            k = f"_l{layer}{sfx}"
            for nm, shape in (("weight_ih", (3 * H, i)), ("weight_hh", (3 * H, H)), ("bias_ih", (3 * H,)), ("bias_hh", (3 * H,))):
                sd[f"{P}.{nm}{k}"] = (torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(H)
    return sd


@pytest.mark.parametrize("H,I", [(64, 128), (384, 768)])
def test_reference_agrees_with_nn_gru_in_float64(H, I):
    """Two layers, bidirectional, against torch.nn.GRU in float64 (<= 1e-12): projection + free-running recurrence, and
    the teacher-forced step fed the module's own states."""
    sd = _state_dict(H, I, 2, seed=H)
    m = torch.nn.GRU(I, H, num_layers=2, batch_first=True, bidirectional=True).double()
    m.load_state_dict({k[len(P) + 1:]: v.double() for k, v in sd.items()})
    x = torch.randn(3, I, 29, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    with torch.no_grad():
        want = m(x.transpose(1, 2))[0].transpose(1, 2)
    L0, L1 = G.Layer(sd, P, 0), G.Layer(sd, P, 1)
    # (the folded bias is rounded to fp32 once, as the packer does: 1/2 ulp of a bias below 2 / sqrt(H) is < 1e-8 -- so the
    # 1e-12 comparison runs on the unrounded fold)
    for L, lay in ((L0, 0), (L1, 1)):
        for d, sfx in enumerate(("", "_reverse")):
            k = f"_l{lay}{sfx}"
            fold = sd[f"{P}.bias_ih{k}"].double().clone()
            fold[: 2 * H] += sd[f"{P}.bias_hh{k}"].double()[: 2 * H]
            L.bias = L.bias.double()
            L.bias[d * 3 * H:(d + 1) * 3 * H] = fold
    h0 = G.free_run(L0, G.project(L0, x))
    gx1 = G.project(L1, h0)
    h1 = G.free_run(L1, gx1)
    assert float((h1 - want).abs().max()) <= 1e-12
    assert float((G.step(L1, gx1, G.shift_prev(want)) - want).abs().max()) <= 1e-12
    # the ATen route through an identity input weight is the same recurrence (fp32)
    assert float((G.free_run_aten_fp32(L1, gx1).double() - want).abs().max()) < 1e-5


def test_ragged_rows_of_the_reference_equal_the_rows_alone():
    sd = _state_dict(64, 128, 1, seed=3)
    L = G.Layer(sd, P, 0)
    gx = G.project(L, torch.randn(3, 128, 20, generator=torch.Generator().manual_seed(2)))
    lens = [20, 1, 7]
    out = G.free_run(L, gx, lens)
    for b, n in enumerate(lens):
        # (not bit for bit: the library's matmul sums a batch of three in another order than a batch of one)
        assert float((out[b:b + 1, :, :n] - G.free_run(L, gx[b:b + 1, :, :n])).abs().max()) <= 1e-13
        assert not out[b, :, n:].any()
    assert float((G.step(L, gx, G.shift_prev(out, lens))[0] - out[0]).abs().max()) <= 1e-13
    assert float((G.free_run_aten_fp32(L, gx, lens).double() - out).abs().max()) < 1e-5


@pytest.fixture(scope="module")
def case():
    sd = _state_dict(H, I, 1, seed=11)
    L = G.Layer(sd, P, 0)
    g = torch.Generator().manual_seed(5)
    x = 0.5 * torch.randn(B, I, T, generator=g)
    res = 0.5 * torch.randn(B, 2 * H, T, generator=g)
    gx = G.project(L, x, torch.float32)
    clean = G.free_run(L, gx, dtype=torch.float32)
    return L, gx, clean, res


def _sdr(name, clean, planted):
    print(f"planted defect {name}: SI-SDR against the clean tensor {float(O.si_sdr(clean, planted)):.1f} dB")


def test_clean_fp32_evaluation_passes_every_check(case):
    L, gx, clean, res = case
    for rep in (G.check_step(L, gx, clean), G.check_free(L, gx, clean),
                G.check_step(L, gx, G.residual(clean, res, torch.float32), res=res)):
        print(rep)
        assert rep.ok() and rep.ratio <= 1.0 + 1e-9, str(rep)
    lens = [T, 250]
    gxr = gx.clone()
    gxr[1, :, 250:] = 0
    gxr[1, H:2 * H, 250:] = G.TAIL_Z
    gxr[1, 4 * H:5 * H, 250:] = G.TAIL_Z
    rag = G.free_run(L, gxr, lens, dtype=torch.float32)
    # (the kernel's way: z = 1 behind the row's end holds the zero state -- the same values as starting at len - 1)
    held = G.free_run(L, gxr, dtype=torch.float32)
    held[1, :, 250:] = 0
    assert torch.equal(rag[1, H:, :250], held[1, H:, :250])
    assert G.check_step(L, gxr, rag, lens).ok()


def test_defect_i_sixteen_units_of_one_frame_from_a_stale_state(case):
    L, gx, clean, _ = case
    d0, t0, u0 = 0, 200, 96

    def hook(d, t, hn, out):
        if d == d0 and t == t0:
            stale = G.cell(L.whh[d], L.bhn[d], gx[:, d * 3 * H:(d + 1) * 3 * H, t], out[:, d * H:(d + 1) * H, t - 2])
            hn = hn.clone()
            hn[:, u0:u0 + 16] = stale[:, u0:u0 + 16]
        return hn

    bad = G.free_run(L, gx, dtype=torch.float32, hook=hook)
    _sdr("i", clean, bad)
    rep = G.check_step(L, gx, bad)
    rows, dirs, frames, units = rep.where()
    assert dirs == [d0] and frames == [t0] and units and set(units) <= set(range(u0, u0 + 16)), str(rep)
    assert rep.worst["dir"] == d0 and rep.worst["frame"] == t0 and rep.worst["unit"] // 16 == u0 // 16


def test_defect_ii_b_hn_of_the_backward_direction_dropped(case):
    L, gx, clean, _ = case
    L2 = G.Layer.__new__(G.Layer)
    L2.__dict__.update(L.__dict__)
    L2.bhn = L.bhn.clone()
    L2.bhn[1] = 0
    bad = G.free_run(L2, gx, dtype=torch.float32)
    _sdr("ii", clean, bad)
    rep = G.check_step(L, gx, bad)
    rows, dirs, frames, units = rep.where()
    assert dirs == [1] and len(frames) == T and len(units) > H // 2, str(rep)


def test_defect_iii_backward_pass_started_one_frame_late(case):
    L, gx, clean, _ = case
    bad = G.free_run(L, gx, dtype=torch.float32, bwd_start=[T - 2] * B)
    _sdr("iii", clean, bad)
    rep = G.check_step(L, gx, bad)
    rows, dirs, frames, units = rep.where()
    assert dirs == [1] and frames == [T - 1] and rows == list(range(B)), str(rep)


def test_defect_iv_r_and_z_slices_of_one_unit_group_swapped(case):
    L, gx, clean, _ = case
    d0, u0 = 1, 40
    L2 = G.Layer.__new__(G.Layer)
    L2.__dict__.update(L.__dict__)
    L2.whh = L.whh.clone()
    gx2 = gx.clone()
    r, z = slice(u0, u0 + 8), slice(H + u0, H + u0 + 8)
    L2.whh[d0, r], L2.whh[d0, z] = L.whh[d0, z], L.whh[d0, r]
    base = d0 * 3 * H
    gx2[:, base + u0: base + u0 + 8], gx2[:, base + H + u0: base + H + u0 + 8] = \
        gx[:, base + H + u0: base + H + u0 + 8], gx[:, base + u0: base + u0 + 8]
    bad = G.free_run(L2, gx2, dtype=torch.float32)
    _sdr("iv", clean, bad)
    rep = G.check_step(L, gx, bad)
    rows, dirs, frames, units = rep.where()
    assert dirs == [d0] and set(units) <= set(range(u0, u0 + 8)) and len(units) >= 4 and len(frames) > T // 2, str(rep)


def test_defect_v_ragged_row_whose_backward_pass_started_at_the_batch_end(case):
    L, gx, clean, _ = case
    lens = [T, 250]
    ok = G.free_run(L, gx, lens, dtype=torch.float32)
    bad = G.free_run(L, gx, lens, dtype=torch.float32, bwd_start=[T - 1, T - 1])
    _sdr("v", ok, bad)
    assert G.check_step(L, gx, ok, lens).ok()
    rep = G.check_step(L, gx, bad, lens)
    rows, dirs, frames, units = rep.where()
    assert rows == [1] and dirs == [1] and frames == [249], str(rep)


def test_defect_vi_residual_not_scaled_on_one_frame(case):
    L, gx, clean, res = case
    t0 = 123
    ok = G.residual(clean, res, torch.float32)
    bad = ok.clone()
    bad[:, :, t0] = clean[:, :, t0] + res[:, :, t0]
    _sdr("vi", ok, bad)
    assert G.check_step(L, gx, ok, res=res).ok()
    rep = G.check_step(L, gx, bad, res=res)
    rows, dirs, frames, units = rep.where()
    # (the neighbours' previous state is recovered from the faulty frame: the forward pass one frame on and the backward
    # pass one frame back see it too)
    assert t0 in frames and set(frames) <= {t0 - 1, t0, t0 + 1} and rep.worst["frame"] == t0, str(rep)
    assert int(rep.bad[:, :, t0].sum()) > 0.9 * B * 2 * H
    assert not rep.bad[:, :H, t0 - 1].any() and not rep.bad[:, H:, t0 + 1].any()


def test_defect_vii_gate_function_of_reduced_accuracy(case):
    """tanh with an absolute error of 4 x the step bound everywhere: no element is far off."""
    L, gx, clean, _ = case
    base = G.check_step(L, gx, clean)
    bound = G.M_STEP * base.e32 + 0.5 * 2.0 ** -24

    def poor_tanh(v):
        sign = 1.0 - 2.0 * ((torch.arange(v.shape[-1]) + v.shape[0]) % 2).to(v.dtype)
        return torch.tanh(v) + 4.0 * bound * sign

    bad = G.free_run(L, gx, dtype=torch.float32, tanh=poor_tanh)
    noise = G.free_run(L, gx).float()  # the clean tensor's own rounding noise: fp32 against float64
    print(f"planted defect vii: max |planted - clean| = {float((bad - clean).abs().max()):.3e}; clean fp32 vs float64 "
          f"{float(O.si_sdr(noise, clean)):.1f} dB, planted vs float64 {float(O.si_sdr(noise, bad)):.1f} dB")
    _sdr("vii", clean, bad)
    rep = G.check_step(L, gx, bad)
    assert rep.n_bad > 0, str(rep)
    assert rep.n_bad > 0.25 * rep.checked, str(rep)  # (1 - z) * 4 bounds > 1 bound wherever z < 3/4
