"""GPU (-m gpu): segmented enhance (Universe.enhance_long, ou_enhance_segments) against the whole-file `enhance`.

  1. one window covers the file: the `enhance` result, the same normalised input and mel scale in the workspace;
  2. several windows: SI-SDR against the whole-file call on the same noise, gated at the measured figure minus a margin
     (DESIGN 4.9), and more overlap never costs more than noise;
  3. whole-file statistics: a loud first half and a near-silent second half -- per-window statistics fail the same gate;
  4. past the length guard of `ou_enhance`: refused up front there; bounded memory, finite and repeatable here;
  5. the CLI with --segment-seconds on a .flac file."""
import ctypes
import math
import time

import pytest
import torch

from open_universe_amd import _lib
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

N_STEPS = 4
# segmented vs whole-file SI-SDR, default segment (8 s) and overlap (1 s): measured figure minus a margin
GAP_GATE_DB = {"PP16": 50.0, "PP24": 53.0}  # measured: PP16 60.2 / 56.6 dB, PP24 63.6 / 62.2 dB (60 / 180 s)
NOISE_DB = 0.5  # "more overlap never lowers the figure by more than noise"


def _signal(fs, T, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(T, device="cuda", dtype=torch.float64) / fs
    x = 0.1 * torch.sin(2 * math.pi * 220.0 * t) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3 * t))
    return x.float() + 0.03 * torch.randn(T, device="cuda", generator=g)


def _rng(seed=5):
    return torch.Generator(device="cuda").manual_seed(seed)


def _si_sdr(ref, est):
    ref, est = ref.double().flatten(), est.double().flatten()
    a = (ref @ est) / (ref @ ref)
    e = a * ref - est
    return float(10 * torch.log10((a * ref).square().sum() / e.square().sum()))


@pytest.mark.parametrize("name", ["PP16", "PP24"])
@pytest.mark.parametrize("secs", [4.0, 8.0])
def test_one_window_is_the_whole_file_call(name, secs):
    model, spec, _ = get_model(name)
    T = int(round(secs * spec.fs))
    x = torch.stack([_signal(spec.fs, T, 1), _signal(spec.fs, T, 2)])
    ref = model.enhance(x, n_steps=N_STEPS, rng=_rng(), keep_rms=True)
    mixn_ref = model.tensor("mixn").clone()
    mel_ref = model.tensor("mel_scale").clone()
    g = _rng()
    y = model.enhance_long(x, segment_s=10.0, n_steps=N_STEPS, rng=g, keep_rms=True)
    g_ref = _rng()
    model.advance_generator_like_enhance(g_ref, 2, T, n_steps=N_STEPS)
    assert torch.equal(g.get_state(), g_ref.get_state())
    assert y.shape == x.shape
    assert torch.equal(model.tensor("mixn"), mixn_ref)
    assert torch.equal(model.tensor("mel_scale"), mel_ref)
    if not torch.equal(y, ref):
        worst = min(_si_sdr(ref[b], y[b]) for b in range(2))
        print(f"{name} {secs} s one window: not bit-identical, {worst:.1f} dB")
        assert worst >= 100.0


def _gap(model, x, overlap_s, whole):
    y = model.enhance_long(x, segment_s=8.0, overlap_s=overlap_s, n_steps=N_STEPS, rng=_rng())
    assert y.shape == x.shape and torch.isfinite(y).all()
    return _si_sdr(whole, y)


@pytest.mark.parametrize("name", ["PP16", "PP24"])
@pytest.mark.parametrize("secs", [60.0, 180.0])
def test_several_windows_against_the_whole_file(name, secs):
    model, spec, _ = get_model(name)
    x = _signal(spec.fs, int(round(secs * spec.fs)), 3)
    whole = model.enhance(x, n_steps=N_STEPS, rng=_rng())
    figs = {ov: _gap(model, x, ov, whole) for ov in (0.25, 1.0, 2.0)}
    print(f"{name} {secs} s: segmented vs whole SI-SDR per overlap {figs}")
    assert figs[1.0] >= GAP_GATE_DB[name]
    assert figs[2.0] >= figs[1.0] - NOISE_DB and figs[1.0] >= figs[0.25] - NOISE_DB


def test_global_statistics_loud_then_quiet():
    model, spec, _ = get_model("PP16")
    T = 60 * spec.fs
    x = _signal(spec.fs, T, 4)
    x[T // 2:] *= 1e-3
    whole = model.enhance(x, n_steps=N_STEPS, rng=_rng())
    y = model.enhance_long(x, n_steps=N_STEPS, rng=_rng())
    fig = _si_sdr(whole, y)
    print(f"loud / quiet: segmented vs whole {fig:.2f} dB")
    assert fig >= GAP_GATE_DB["PP16"]
    # the quiet half keeps the whole file's level: no jump towards the loud half's level
    lvl = lambda z: float(z.double().square().mean().sqrt())  # noqa: E731
    q = slice(T // 2 + spec.fs, T)
    assert abs(20 * math.log10(lvl(y[q]) / lvl(whole[q]))) < 1.0
    # test-only reference computation with PER-WINDOW statistics: every 8 s piece enhanced as a file of its own on its slice
    # of the same noise, concatenated -- fails the same gate
    n = 8 * spec.fs
    noise = model.draw_noise_like_enhance(_rng(), 1, T, N_STEPS)
    pad_left = (spec.tot_ds - T % spec.tot_ds) // 2
    parts = []
    for s in range(0, T, n):
        xs = x[s:s + n]
        Tp = xs.shape[-1] + (spec.tot_ds - xs.shape[-1] % spec.tot_ds)
        nz = noise[:, :, pad_left + s: pad_left + s + Tp]
        nz = torch.nn.functional.pad(nz, (0, Tp - nz.shape[-1]))
        parts.append(model._enhance(xs[None, None], N_STEPS, None, None, None, None, False, False, None, "median", None,
                                    nz[:, :, None, :].contiguous())[0, 0])
    fig_pw = _si_sdr(whole, torch.cat(parts))
    print(f"loud / quiet: per-window statistics vs whole {fig_pw:.2f} dB")
    assert fig_pw < GAP_GATE_DB["PP16"]


def test_past_the_plane_limit_of_one_pass():
    model, spec, _ = get_model("PP24")
    T = int(24.5 * 60 * spec.fs)  # PP24: level 0 (32 channels) reaches 2^32 bytes at about 23 min
    x = _signal(spec.fs, T, 6)
    L = model._L
    # ou_enhance refuses before any launch (status word untouched) ...
    ws = model._workspace(1, 8 * spec.tot_ds)
    torch.cuda.synchronize()
    status0 = ws[:256].clone()
    out = torch.empty(1, T, device="cuda")
    rc = L.ou_enhance(model._handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                      ctypes.c_void_p(x.data_ptr()), 1, T, N_STEPS, 1.0, None, -1, 0, ctypes.c_void_p(ws.data_ptr()),
                      ctypes.c_size_t(ws.numel()), model._stream())
    assert rc == _lib.OU_EINVAL and b"ou_enhance_segments" in L.ou_last_error(model._handle)
    torch.cuda.synchronize()
    assert torch.equal(ws[:256], status0)
    # ... and so does enhance, before it sizes a workspace
    with pytest.raises(ValueError, match="ou_enhance_segments"):
        model.enhance(x, n_steps=N_STEPS, rng=_rng())
    t0 = time.perf_counter()
    y = model.enhance_long(x, n_steps=N_STEPS, max_batch=32, rng=_rng())
    torch.cuda.synchronize()
    print(f"PP24 {T / spec.fs / 60:.1f} min: enhance_long {time.perf_counter() - t0:.1f} s")
    assert y.shape == x.shape and torch.isfinite(y).all() and float(y.abs().max()) <= 1.0
    y2 = model.enhance_long(x, n_steps=N_STEPS, max_batch=32, rng=_rng())
    assert torch.equal(y, y2)
    need, Bs, Ls = ctypes.c_size_t(), ctypes.c_int32(), ctypes.c_int32()
    _lib.check(L.ou_segments_workspace_bytes(model._handle, 1, T, 8 * spec.fs, spec.fs, 32, ctypes.byref(need),
                                             ctypes.byref(Bs), ctypes.byref(Ls)), model._handle)
    assert Bs.value <= 32 and Ls.value == 8 * spec.fs - (8 * spec.fs) % spec.tot_ds
    assert model._seg_ws[1].numel() == need.value
    walk = ctypes.c_size_t()
    _lib.check(L.ou_workspace_bytes(model._handle, 32, Ls.value, ctypes.byref(walk)), model._handle)
    assert need.value <= walk.value + (64 << 20)  # bounded by (32, L), not by the length of the row


def test_cli_segment_seconds_end_to_end(tmp_path):
    from open_universe_amd import audio as A
    from open_universe_amd.bin import enhance as cli

    model, spec, _ = get_model("PP16")
    x = (_signal(spec.fs, 90 * spec.fs, 7) * 0.5).clamp(-1, 1).cpu()
    src = tmp_path / "long.flac"
    A.save(src, x[None], spec.fs)
    y_file, _ = A.load(src)
    dst = tmp_path / "out.wav"
    cli.main([str(src), str(dst), "--segment-seconds", "8", "--seed", "9", "--n_steps", str(N_STEPS)], model=model)
    y, fs = A.load(dst)
    direct = model.enhance_long(y_file.cuda(), segment_s=8.0, n_steps=N_STEPS, rng=torch.Generator(device="cuda").manual_seed(9))
    assert fs == spec.fs and tuple(y.shape) == tuple(direct.shape)
    assert torch.equal(y, direct.cpu())
