"""GPU (-m gpu): segmented enhance of rows with lengths of their own (Universe.enhance_long_many, ou_enhance_segments_var).

Row c of the call is, by definition, `enhance_long` of that row alone on its own noise.  Reduced-width models, 3 steps, windows
of 16 tot_ds samples overlapping by 2 tot_ds, at most 4 windows per group; the six lengths cover a row of several windows, one
of exactly one full window (T_pad = S), one of two windows with the second shifted (T_pad = S + tot_ds), short rows down to 57
samples -- so the call has full FULL groups, a partly filled last FULL group and a ragged SHORT group.

  1. every row against itself alone (noise tensor and CounterNoise): >= 80 dB SI-SDR and plain SNR, the floor of "ragged row vs
     the utterance alone" on these models (test_gpu_ragged.py); one-window rows also against plain `enhance`;
  2. equal lengths: bit-identical to `enhance_long` on the (C, T) tensor, same (batch, length) as ou_segments_workspace_bytes;
  3. C = 1: bit-identical to ou_enhance_segments;
  4. two runs are bit-identical; keep_rms restores every row's own RMS; peaks <= 1;
  5. a shared generator ends where the loop of advance_generator_like_enhance over the files leaves it;
  6. fewer launches than the six single-row calls together (ou_launch_stats);
  7. the CLI's --segment-files 3 against --segment-files 1 with --noise counter."""
import ctypes

import pytest
import torch

import restatement as O
from helpers import synth_mix, worst
from open_universe_amd import _lib
from open_universe_amd.noise import CounterNoise
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

N = 3
MAX_BATCH = 4
FLOOR_DB = 80.0
MODELS = ["PP16s", "PP16m", "PP24s"]


def _geom(spec):
    td = spec.tot_ds
    return 16 * td, 2 * td, [41 * td + 7, 9 * td, 57, 16 * td - 1, 16 * td, 70 * td + 3]


def _kw(spec):
    S, Ov, _ = _geom(spec)
    return dict(segment_s=S / spec.fs, overlap_s=Ov / spec.fs, max_batch=MAX_BATCH, n_steps=N)


def _signals(spec, lens, seed=2000):
    return [synth_mix(spec, 1, L, seed=seed + i)[0].cuda() for i, L in enumerate(lens)]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _check_rows(tag, refs, outs):
    figs = [O.si_sdr(r.cpu(), y.cpu()) for r, y in zip(refs, outs)]
    w = worst(figs)
    print(f"{tag}: worst row vs alone SI-SDR {float(w):.1f} dB, SNR {w.snr:.1f} dB; per row "
          + ", ".join(f"{float(f):.1f}/{f.snr:.1f}" for f in figs))
    assert float(w) >= FLOOR_DB and w.snr >= FLOOR_DB


_CACHE = {}


def _six_rows(name, mode):
    """The ragged call on the six lengths and each row alone, computed once per (model, noise mode)."""
    key = (name, mode)
    if key not in _CACHE:
        model, spec, _ = get_model(name)
        _, _, lens = _geom(spec)
        sigs = _signals(spec, lens)
        if mode == "tensor":
            src = lambda i: _gen(300 + i)  # noqa: E731
        else:
            src = lambda i: CounterNoise(77, 5 + i)  # noqa: E731
        alone = [model.enhance_long(s, rng=src(i), **_kw(spec)) for i, s in enumerate(sigs)]
        outs = model.enhance_long_many(sigs, [src(i) for i in range(len(sigs))], **_kw(spec))
        _CACHE[key] = (sigs, alone, outs)
    return _CACHE[key]


@pytest.mark.parametrize("mode", ["tensor", "counter"])
@pytest.mark.parametrize("name", MODELS)
def test_every_row_is_the_row_alone(name, mode):
    model, spec, _ = get_model(name)
    S, _, lens = _geom(spec)
    sigs, alone, outs = _six_rows(name, mode)
    assert len(outs) == len(sigs)
    for s, y in zip(sigs, outs):
        assert y.shape == s.shape and torch.isfinite(y).all()
    _check_rows(f"segments_var.{name}.{mode}", alone, outs)
    # rows of one window: also the plain `enhance` result on the same noise
    one = [i for i, L in enumerate(lens) if L + (spec.tot_ds - L % spec.tot_ds) <= S]
    assert one == [1, 2, 3]
    src = (lambda i: _gen(300 + i)) if mode == "tensor" else (lambda i: CounterNoise(77, 5 + i))
    plain = [model.enhance(sigs[i], n_steps=N, rng=src(i)) for i in one]
    _check_rows(f"segments_var.{name}.{mode}.one_window_vs_enhance", plain, [outs[i] for i in one])


def _call_var(model, spec, sigs, noise, keep_rms=False):
    """ou_enhance_segments_var through ctypes on explicit noise (n_steps, C, T_pad_max) -> the whole (C, T_raw_max) output."""
    S, Ov, _ = _geom(spec)
    lens = [int(s.shape[-1]) for s in sigs]
    C, lm = len(sigs), max(lens)
    tr = (ctypes.c_int64 * C)(*lens)
    need, B, L = ctypes.c_size_t(), ctypes.c_int32(), ctypes.c_int32()
    _lib.check(model._L.ou_segments_var_workspace_bytes(model._handle, C, tr, S, Ov, MAX_BATCH, ctypes.byref(need),
                                                        ctypes.byref(B), ctypes.byref(L)), model._handle)
    ws = model._segments_workspace(B.value, L.value, need.value)
    mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs]).contiguous()
    for c, n in enumerate(lens):
        mix[c, n:] = 123.0  # the rest of a mix row is ignored
    out = torch.full((C, lm), 7.0, device="cuda")
    _lib.check(model._L.ou_enhance_segments_var(
        model._handle, ctypes.c_void_p(mix.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(noise.data_ptr()), C, lm,
        tr, S, Ov, MAX_BATCH, N, float(model.diff_kwargs.epsilon), None, -1, _lib.OU_ENH_KEEP_RMS if keep_rms else 0,
        ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(ws.numel()), model._stream()), model._handle)
    model._status()
    torch.cuda.synchronize()
    return out, (B.value, L.value)


def _noise_rows(model, spec, lens, seed):
    td = spec.tot_ds
    tp = [n + (td - n % td) for n in lens]
    noise = torch.zeros(N, len(lens), max(tp), device="cuda")
    for c, (n, t) in enumerate(zip(lens, tp)):
        noise[:, c, :t] = model.draw_noise_like_enhance(_gen(seed + c), 1, n, N)[:, 0]
    return noise


@pytest.mark.parametrize("name", MODELS)
def test_out_rows_are_zero_behind_their_end_and_mix_tails_are_ignored(name):
    model, spec, _ = get_model(name)
    _, _, lens = _geom(spec)
    sigs = _signals(spec, lens)
    out, _ = _call_var(model, spec, sigs, _noise_rows(model, spec, lens, 300))
    assert torch.isfinite(out).all()
    for c, n in enumerate(lens):
        assert not out[c, n:].any()
    # same per-row draws as the "tensor" case above: the same rows, bit for bit, garbage behind the mix rows or not
    _, _, outs = _six_rows(name, "tensor")
    for c, n in enumerate(lens):
        assert torch.equal(out[c, :n], outs[c])


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("windows", ["several", "one"])
def test_equal_lengths_are_bit_identical_to_enhance_long(name, windows):
    model, spec, _ = get_model(name)
    S, Ov, _ = _geom(spec)
    td = spec.tot_ds
    T = 70 * td + 3 if windows == "several" else 9 * td + 5
    C = 3
    x = torch.stack(_signals(spec, [T] * C, seed=2100))
    ref = model.enhance_long(x, rng=_gen(9), **_kw(spec))
    # enhance_long draws (C, 1, T_pad) per step from ONE generator: the same values through the noise tensor of the var call
    noise = model.draw_noise_like_enhance(_gen(9), C, T, N)
    out, (B, L) = _call_var(model, spec, list(x), noise)
    assert torch.equal(out, ref)
    need, Bs, Ls = ctypes.c_size_t(), ctypes.c_int32(), ctypes.c_int32()
    _lib.check(model._L.ou_segments_workspace_bytes(model._handle, C, T, S, Ov, MAX_BATCH, ctypes.byref(need), ctypes.byref(Bs),
                                                    ctypes.byref(Ls)), model._handle)
    assert (B, L) == (Bs.value, Ls.value)
    if windows == "several":
        n_win = len(_lib.segment_plan(td, T, S, Ov)["starts"])
        assert n_win == 5 and B == 4 and (C * n_win) % B != 0  # 15 entries in groups of 4: a partly filled last group


@pytest.mark.parametrize("name", MODELS)
def test_one_row_is_bit_identical_to_ou_enhance_segments(name):
    model, spec, _ = get_model(name)
    td = spec.tot_ds
    for T in (70 * td + 3, 16 * td, 57):
        x = _signals(spec, [T], seed=2200)[0]
        ref = model.enhance_long(x, rng=_gen(11), **_kw(spec))
        out, _ = _call_var(model, spec, [x], model.draw_noise_like_enhance(_gen(11), 1, T, N))
        assert torch.equal(out[0], ref), T


@pytest.mark.parametrize("name", MODELS)
def test_repeatable_keep_rms_and_peak(name):
    model, spec, _ = get_model(name)
    _, _, lens = _geom(spec)
    sigs = _signals(spec, lens)
    run = lambda: model.enhance_long_many(sigs, [_gen(300 + i) for i in range(len(sigs))], keep_rms=True, **_kw(spec))  # noqa: E731
    a, b = run(), run()
    for s, y, z in zip(sigs, a, b):
        assert torch.equal(y, z)
        peak = float(y.abs().max())
        assert peak <= 1.0
        # keep_rms: out = x * (mix_rms / x_rms), all fp32: the gain carries a few roundings of 2^-24 relative, every product one
        # more, and the RMS over >= 57 samples averages the latter -- 1e-5 relative is about 100 ulp, far above that and far
        # below any wrong-row or wrong-length RMS.  (Holds where the peak guard did not divide: peak < 1.)
        assert peak < 1.0
        rms = lambda v: float(v.double().square().mean().sqrt())  # noqa: E731
        assert rms(y) == pytest.approx(rms(s), rel=1e-5)


def test_shared_generator_advances_like_the_loop_over_the_files():
    model, spec, _ = get_model("PP16s")
    _, _, lens = _geom(spec)
    sigs = _signals(spec, lens[:4])
    ent = [torch.stack([sigs[0], sigs[0].flip(0)]), sigs[1], sigs[2], sigs[3]]  # a two-channel file and three mono ones
    g = _gen(21)
    outs = model.enhance_long_many(ent, g, **_kw(spec))
    g_ref = _gen(21)
    for e in ent:
        model.advance_generator_like_enhance(g_ref, e.shape[0] if e.ndim == 2 else 1, e.shape[-1], n_steps=N)
    assert torch.equal(g.get_state(), g_ref.get_state())
    # ... and every file got the draws of the serial loop: enhance_long file by file from one generator
    g2 = _gen(21)
    serial = [model.enhance_long(e, rng=g2, **_kw(spec)) for e in ent]
    assert [tuple(o.shape) for o in outs] == [tuple(e.shape) for e in ent]
    _check_rows("segments_var.PP16s.shared_generator", [s.flatten() for s in serial], [o.flatten() for o in outs])


@pytest.mark.parametrize("name", MODELS)
def test_fewer_launches_than_the_single_row_calls(name):
    model, spec, _ = get_model(name)
    _, _, lens = _geom(spec)
    sigs = _signals(spec, lens)
    alone = 0
    for i, s in enumerate(sigs):
        model.enhance_long(s, rng=CounterNoise(77, 5 + i), **_kw(spec))
        alone += model.launch_stats()[0]
    model.enhance_long_many(sigs, [CounterNoise(77, 5 + i) for i in range(len(sigs))], **_kw(spec))
    together = model.launch_stats()[0]
    print(f"{name}: launches of the six single-row calls {alone}, of the one call {together}")
    assert 0 < together < alone


def test_cli_segment_files_end_to_end(tmp_path):
    from open_universe_amd import audio as A
    from open_universe_amd.bin import enhance as cli

    model, spec, _ = get_model("PP16s")
    td = spec.tot_ds
    S, Ov, _ = _geom(spec)
    src = tmp_path / "in"
    src.mkdir()
    for i, T in enumerate((41 * td + 7, 9 * td, 20 * td + 100)):
        x = (synth_mix(spec, 1, T, seed=2300 + i) * 0.5).clamp(-1, 1)
        A.save(src / f"f{i}.wav", x, spec.fs)
    common = ["--segment-seconds", repr(S / spec.fs), "--segment-overlap", repr(Ov / spec.fs), "--noise", "counter", "--seed", "9",
              "--n_steps", str(N)]
    cli.main([str(src), str(tmp_path / "o1"), "--segment-files", "1"] + common, model=model)
    cli.main([str(src), str(tmp_path / "o3"), "--segment-files", "3"] + common, model=model)
    refs, outs = [], []
    for i in range(3):
        r, _ = A.load(tmp_path / "o1" / f"f{i}.wav")
        y, fs = A.load(tmp_path / "o3" / f"f{i}.wav")
        assert fs == spec.fs and y.shape == r.shape
        refs.append(r.flatten())
        outs.append(y.flatten())
    _check_rows("segments_var.cli", refs, outs)
