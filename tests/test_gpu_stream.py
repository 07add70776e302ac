"""GPU (-m gpu): streaming enhance (ou_stream_*, Universe.stream) against its definition.

  1. Definition.  At C = 1, outside the crossfades the stream's output is bit-identical to ou_enhance of the window alone (counter
     noise of stream id + k, no peak guard); inside them it lies within one fp32 ulp of the float64 stitch (tests/stream_ref.py) of
     those same fp32 window results.  Two readings were fixed before any figure was seen to pass.  The weight a(i) of the float64
     stitch is the one the definition names, the fp32-valued function of ou_segment.hip, evaluated on the host in fp32
     (stream_ref.weight).  The ulp is taken at |y_k| + |y_{k+1}|, the magnitude of the operands: the two products may cancel, so
     the spacing of the result is no yardstick (it is 0 where the windows cancel).  What the bound has to cover: the kernel's own
     evaluation -- stream_emit_kernel recovers the rounding errors of 1 - a, the products and the sum and rounds once, at most
     half an ulp of the result -- and the distance between the device's weight and the host's (device cosf against numpy's, a
     last place of the cosine: up to ~3e-8 (|y_k| + |y_{k+1}|), half an ulp of the operands).  Against the REAL-valued raised
     cosine the fp32 weight's own error (up to ~1.3e-7, tests/seg_fp64.py) counts too; that figure is printed per case, not gated.
     MEASURED (PP16s, tot_ds = 160, S = 4 tot_ds), max error in ulps of the operands, fp32-valued weight / real-valued weight:
       two_windows 0.461 / 1.042     two_plus_one 0.639 / 1.209     half_overlap 0.967 / 2.144
       warm_start 0.550 / 0.744     use_aux_signal 0.498 / 0.656     keep_rms 0.494 / 1.269
     A first version evaluated the blend as ou_segment.hip does, four roundings: 1.128 (two_windows) and 1.467 (half_overlap)
     ulp, over the bound; the bound stayed and the kernel's arithmetic was made exact.  Outside the crossfades every case is
     bit-identical.
  2. Chunking.  One push, pushes of 1 sample, of stride +- 1, one push across three windows, empty pushes in between: identical
     bytes, and the plan's n_out after every call.
  3. A flush resets the stream; every call leaves the handle's noise source as it found it.
  4. State isolation: a workspace full of NaN before create, a sentinel behind n_out.
  5. Rows: C = 3 against every row streamed alone, >= 100 dB (the batch-versus-alone gate of test_gpu_segments.py).  The measured
     minimum goes to build/observed/stream_observed.json (untracked; profiles/stream_observed.json is a committed copy).
  6. warm_start, use_aux_signal, keep_rms, clip.
  7. Refusals that need a handle; the workspace size; the Python object and the CLI."""
import ctypes
import json
import os
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

import stream_ref as R
from helpers import synth_mix
from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

NAME = "PP16s"  # the smallest model of helpers.py; UNIVERSE++: it has the snake decoupling layer the cheap modes need
N_STEPS = 2
SEED = 77
SENTINEL = 7.5
OBSERVED = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed", "stream_observed.json")
NO_GUARD_SERIAL = _lib.OU_ENH_NO_PEAK_GUARD | _lib.OU_ENH_SERIAL


def _ptr(t):
    return c_void_p(t.data_ptr())


def _ids(C):
    return [c << 32 for c in range(C)]


def _signal(spec, C, T, seed=1000, gain=1.0):
    return (gain * synth_mix(spec, C, T, seed=seed)).cuda().contiguous()


class RawStream:
    """ou_stream_* through ctypes, on a workspace of its own; every output buffer is wider than asked for and holds a sentinel."""

    def __init__(self, model, C, segment, overlap, ids=None, seed=SEED, n_steps=N_STEPS, warm_start=None, enh_flags=0,
                 stream_flags=0, poison=False):
        self.m, self.C, self.seg, self.ov = model, C, segment, overlap
        L = self.L = model._L
        need = ctypes.c_size_t()
        _lib.check(L.ou_stream_workspace_bytes(model._handle, C, segment, overlap, byref(need)), model._handle)
        self.need = need.value
        self.ws = torch.zeros(self.need, dtype=torch.uint8, device="cuda")
        if poison:
            self.ws.view(torch.float32).fill_(float("nan"))
        sigma = model._sigma_table(n_steps)
        spec = _lib.StreamSpec()
        spec.C, spec.segment, spec.overlap, spec.n_steps = C, segment, overlap, n_steps
        spec.epsilon = float(model.diff_kwargs.epsilon)
        spec.sigma_host = ctypes.cast(sigma.data_ptr(), ctypes.POINTER(ctypes.c_float))
        spec.warm_start = -1 if warm_start is None else warm_start
        spec.enh_flags, spec.stream_flags, spec.seed = enh_flags, stream_flags, seed
        ids = _ids(C) if ids is None else ids
        spec.ids = (ctypes.c_uint64 * C)(*ids)
        self.s = c_void_p()
        _lib.check(L.ou_stream_create(model._handle, byref(spec), _ptr(self.ws), self.need, byref(self.s)), model._handle)
        self.pushed = 0
        self.tot = model.tot_ds

    def _call(self, fn, head, cap):
        out = torch.full((self.C, cap + 8), SENTINEL, device="cuda")
        n_out = ctypes.c_int64(-1)
        with torch.cuda.device(self.m.device):
            _lib.check(fn(self.s, *head, _ptr(out), out.stride(0), cap, byref(n_out), self.m._stream()), self.m._handle)
        assert n_out.value == cap, (n_out.value, cap)  # the plan's count
        assert bool((out[:, cap:] == SENTINEL).all()), "written behind n_out"
        return out[:, :cap].clone()

    def push(self, x):
        n = x.shape[1]
        cap = R.emitted(self.tot, self.pushed + n, self.seg, self.ov) - R.emitted(self.tot, self.pushed, self.seg, self.ov)
        y = self._call(self.L.ou_stream_push, (_ptr(x) if n else None, x.stride(0), n), cap)
        self.pushed += n
        return y

    def flush(self):
        y = self._call(self.L.ou_stream_flush, (), self.pushed - R.emitted(self.tot, self.pushed, self.seg, self.ov))
        self.pushed = 0
        return y

    def run(self, x, sizes=None):
        """x (C, T) in pushes of `sizes` (default: one push), then the flush -> (C, T)"""
        parts, at = [], 0
        for n in ([x.shape[1]] if sizes is None else sizes):
            parts.append(self.push(x[:, at:at + n]))
            at += n
        assert at == x.shape[1]
        parts.append(self.flush())
        y = torch.cat(parts, dim=1)
        assert y.shape == x.shape
        return y

    def close(self):
        if self.s.value:
            self.L.ou_stream_destroy(self.s)
            self.s = c_void_p()


def window_alone(model, w, ids, n_steps=N_STEPS, warm_start=None, enh_flags=0, seed=SEED):
    """ou_enhance(B = C, T_raw = L) of the window w (C, L) alone: counter noise of the given stream ids, no peak guard."""
    C, Lw = w.shape
    T = Lw + (model.tot_ds - Lw % model.tot_ds)
    ws = model._workspace(C, T)
    out = torch.empty(C, Lw, device="cuda")
    sigma = model._sigma_table(n_steps)
    with torch.cuda.device(model.device), model._counter_source(seed, ids, C, T):
        _lib.check(model._L.ou_enhance(model._handle, _ptr(w), _ptr(out), None, C, Lw, n_steps, float(model.diff_kwargs.epsilon),
                                       ctypes.cast(sigma.data_ptr(), ctypes.POINTER(ctypes.c_float)),
                                       -1 if warm_start is None else warm_start, enh_flags | NO_GUARD_SERIAL, _ptr(ws),
                                       ctypes.c_size_t(ws.numel()), model._stream()), model._handle)
    torch.cuda.synchronize()
    return out


def hold_definition(model, x, y, segment, overlap, name, ids=None, clip=False, **modes):
    """y (C, T), the stream's output for x, against the definition; -> the largest crossfade error in operand ulps."""
    C, T = x.shape
    tot = model.tot_ds
    p = R.plan(tot, T, segment, overlap)
    xp = torch.nn.functional.pad(x, (0, p["T_pad"] - T)).contiguous()
    ids = _ids(C) if ids is None else ids
    results = [None] * len(p["starts"])
    for k in R.needed(p, T):
        w = xp[:, p["starts"][k]:p["starts"][k] + p["lengths"][k]].contiguous()
        results[k] = window_alone(model, w, [i + k for i in ids], **modes).cpu().numpy()
    ref, fade, scale = R.stitch(p, T, results)
    if clip:
        ref = np.clip(ref, -1.0, 1.0)
    got = y.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got[:, ~fade], ref[:, ~fade].astype(np.float32)), (name, "outside the crossfades: not the window's bits")
    ratio = 0.0
    if fade.any():
        ulp = np.spacing(scale[:, fade].astype(np.float32)).astype(np.float64)
        err = np.abs(got[:, fade].astype(np.float64) - ref[:, fade])
        ratio = float((err / ulp).max())
        # (for the record: against the real-valued raised cosine, i.e. with the fp32 weight's own error of up to ~1.3e-7 counted in)
        real = R.stitch(p, T, results, exact=True)[0]
        if clip:
            real = np.clip(real, -1.0, 1.0)
        ratio_real = float((np.abs(got[:, fade].astype(np.float64) - real[:, fade]) / ulp).max())
        print(f"{name}: {int(fade.sum())} crossfaded samples, max |gpu - f64| = {ratio:.3f} ulp of the operands "
              f"({ratio_real:.3f} against the real-valued weight)")
        assert ratio <= 1.0, (name, ratio)
    return ratio


def _cases(tot):
    S = 4 * tot
    return {
        "short_odd": (S, tot, 3 * tot - 5),          # T < S, T % tot_ds != 0: one short window with zeros behind T
        "one_window": (S, tot, S),                   # exactly one window; its tail comes out of the carry at the flush
        "two_windows": (S, tot, 2 * S - tot),        # exactly two
        "two_plus_one": (S, tot, 2 * S - tot + 1),   # one sample more: the shifted last window overlaps beyond its crossfade
        "no_overlap": (S, 0, 2 * S + 5),             # V = 0
        "half_overlap": (S, 2 * tot, 2 * S + 7),     # V = S / 2
    }


@pytest.mark.parametrize("case", ["short_odd", "one_window", "two_windows", "two_plus_one", "no_overlap", "half_overlap"])
def test_definition(case):
    model, spec, _ = get_model(NAME)
    S, V, T = _cases(spec.tot_ds)[case]
    x = _signal(spec, 1, T)
    st = RawStream(model, 1, S, V)
    y = st.run(x)
    st.close()
    hold_definition(model, x, y, S, V, case)


def test_chunking_gives_identical_bytes():
    model, spec, _ = get_model(NAME)
    tot = spec.tot_ds
    S, V = 4 * tot, tot
    hop = S - V
    T = S + 3 * hop + 37
    x = _signal(spec, 2, T, seed=1010)

    def fill(sizes):
        rest = T - sum(sizes)
        assert rest >= 0
        return sizes + ([rest] if rest else [])

    ways = {
        "one push": [T],
        "stride + 1": fill([hop + 1] * (T // (hop + 1))),
        "stride - 1": fill([hop - 1] * (T // (hop - 1))),
        "three windows in one push": fill([7, S + 2 * hop]),
        "empty pushes": fill([0, 100, 0, 0, S, 0, hop + 3, 0]) + [0],
        "single samples": [1] * T,
    }
    st = RawStream(model, 2, S, V)
    ref = None
    for name, sizes in ways.items():
        y = st.run(x, sizes)  # (n_out of every call is held against the plan inside)
        if ref is None:
            ref = y
            assert torch.isfinite(ref).all()
        assert torch.equal(y, ref), name
    st.close()


def test_flush_resets_and_the_noise_source_is_restored():
    model, spec, _ = get_model(NAME)
    tot = spec.tot_ds
    S, V = 4 * tot, tot
    T = 2 * S + 11
    x = _signal(spec, 1, T, seed=1020)
    L, h = model._L, model._handle
    source = lambda: json.loads(L.ou_plan_json(h).decode())["noise_source"]  # noqa: E731
    st = RawStream(model, 1, S, V)
    assert source() == "tensor"
    y1 = st.run(x, [S + 5, T - S - 5])
    assert source() == "tensor"
    y2 = st.run(x, [S + 5, T - S - 5])
    assert torch.equal(y1, y2)
    # with a source of the caller's set: still that one after every stream call, key and ids included
    w = x[:, :S].contiguous()
    Tw = S + tot
    ws = model._workspace(1, Tw)
    sigma = model._sigma_table(N_STEPS)

    def enhance_on_current_source():
        out = torch.empty(1, S, device="cuda")
        _lib.check(L.ou_enhance(h, _ptr(w), _ptr(out), None, 1, S, N_STEPS, float(model.diff_kwargs.epsilon),
                                ctypes.cast(sigma.data_ptr(), ctypes.POINTER(ctypes.c_float)), -1, NO_GUARD_SERIAL, _ptr(ws),
                                ctypes.c_size_t(ws.numel()), model._stream()), h)
        torch.cuda.synchronize()
        return out

    with torch.cuda.device(model.device), model._counter_source(4242, [99], 1, Tw):
        before = enhance_on_current_source()
        for part in (st.push(x[:, :S + 5]), st.push(x[:, S + 5:]), st.flush()):
            assert source() == "counter"
        assert torch.equal(enhance_on_current_source(), before)
    assert source() == "tensor"
    st.close()


def test_state_isolation_nan_workspace_and_sentinel():
    model, spec, _ = get_model(NAME)
    tot = spec.tot_ds
    S, V = 4 * tot, tot
    T = 2 * S + 3
    x = _signal(spec, 2, T, seed=1030)
    clean = RawStream(model, 2, S, V)
    ref = clean.run(x, [S - 1, 2, T - S - 1])
    clean.close()
    del clean  # (its buffer goes back to the allocator: the poisoned one below may stand at the address the handle remembers as
    #            prepared -- the session must clear the header itself)
    st = RawStream(model, 2, S, V, poison=True)
    y = st.run(x, [S - 1, 2, T - S - 1])  # (the sentinel behind n_out is held inside)
    st.close()
    assert not torch.isnan(y).any() and torch.equal(y, ref)


def _si_sdr(ref, est):
    ref, est = ref.double().flatten(), est.double().flatten()
    a = (ref @ est) / (ref @ ref)
    e = a * ref - est
    return float(10 * torch.log10((a * ref).square().sum() / e.square().sum().clamp(min=1e-300)))


def test_rows_against_every_row_alone():
    model, spec, _ = get_model(NAME)
    tot = spec.tot_ds
    S, V = 4 * tot, tot
    T = 2 * S + 9
    x = _signal(spec, 3, T, seed=1040)
    st = RawStream(model, 3, S, V)
    y = st.run(x, [S + 1, T - S - 1])
    st.close()
    figs = []
    for c in range(3):
        alone = RawStream(model, 1, S, V, ids=[c << 32])
        yc = alone.run(x[c:c + 1].contiguous(), [S + 1, T - S - 1])
        alone.close()
        figs.append(200.0 if torch.equal(yc[0], y[c]) else _si_sdr(yc[0], y[c]))
    print(f"rows of a C = 3 stream against the rows alone: {figs} dB (200 = identical)")
    os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
    with open(OBSERVED, "w") as f:
        json.dump({"model": NAME, "C": 3, "segment": S, "overlap": V, "T": T, "n_steps": N_STEPS,
                   "row_vs_alone_si_sdr_db": figs, "min_db": min(figs), "note": "200 = bit-identical"}, f, indent=1)
    assert min(figs) >= 100.0, figs


@pytest.mark.parametrize("mode", ["warm_start", "use_aux_signal", "keep_rms"])
def test_modes_hold_the_definition(mode):
    model, spec, _ = get_model(NAME)
    tot = spec.tot_ds
    S, V = 4 * tot, tot
    T = 2 * S - tot + 1
    x = _signal(spec, 1, T, seed=1050)
    kw = {"warm_start": dict(n_steps=3, warm_start=1), "use_aux_signal": dict(enh_flags=_lib.OU_ENH_USE_AUX_SIGNAL),
          "keep_rms": dict(enh_flags=_lib.OU_ENH_KEEP_RMS)}[mode]
    st = RawStream(model, 1, S, V, **kw)
    y = st.run(x)
    st.close()
    hold_definition(model, x, y, S, V, mode, **kw)
    if mode == "keep_rms":  # (the flag reaches the windows: the plain stream gives something else)
        plain = RawStream(model, 1, S, V)
        assert not torch.equal(plain.run(x), y)
        plain.close()


def test_clip_clamps_what_is_emitted():
    model, spec, _ = get_model(NAME)
    tot = spec.tot_ds
    S, V = 4 * tot, tot
    T = 2 * S - tot + 1
    x = _signal(spec, 1, T, seed=1060, gain=20.0)  # with keep_rms the windows come back at this level: far above 1
    loud = RawStream(model, 1, S, V, enh_flags=_lib.OU_ENH_KEEP_RMS)
    y0 = loud.run(x)
    loud.close()
    assert float(y0.abs().max()) > 1.0, "the case does not reach the clamp"
    st = RawStream(model, 1, S, V, enh_flags=_lib.OU_ENH_KEEP_RMS, stream_flags=_lib.OU_STREAM_CLIP)
    y = st.run(x)
    st.close()
    assert torch.equal(y, y0.clamp(-1.0, 1.0)) and float(y.abs().max()) == 1.0


def _create_rc(model, **over):
    L = model._L
    tot = model.tot_ds
    a = dict(C=1, segment=4 * tot, overlap=tot, n_steps=N_STEPS, warm_start=-1, enh_flags=0, stream_flags=0, ws_bytes=None)
    a.update(over)
    spec = _lib.StreamSpec()
    spec.C, spec.segment, spec.overlap, spec.n_steps = a["C"], a["segment"], a["overlap"], a["n_steps"]
    spec.epsilon, spec.warm_start, spec.enh_flags, spec.stream_flags = 1.0, a["warm_start"], a["enh_flags"], a["stream_flags"]
    spec.ids = (ctypes.c_uint64 * max(a["C"], 1))()
    ws = torch.empty(1 << 20 if a["ws_bytes"] is None else max(a["ws_bytes"], 256), dtype=torch.uint8, device="cuda")
    s = c_void_p()
    n0 = model.launch_stats()
    rc = L.ou_stream_create(model._handle, byref(spec), _ptr(ws), ws.numel() if a["ws_bytes"] is None else a["ws_bytes"], byref(s))
    msg = L.ou_last_error(model._handle).decode()
    assert rc != 0 and not s.value and model.launch_stats() == n0
    return rc, msg


def test_refusals_that_need_a_handle():
    model, spec, _ = get_model(NAME)
    tot = spec.tot_ds
    assert _create_rc(model, C=0) == (_lib.OU_EINVAL, "stream: C must be at least 1")
    rc, msg = _create_rc(model, segment=2 * tot - 1)
    assert rc == _lib.OU_EINVAL and f"segment must be at least two total down-sampling factors ({2 * tot} samples)" in msg
    rc, msg = _create_rc(model, overlap=3 * tot)
    assert rc == _lib.OU_EINVAL and "overlap must lie in [0, segment / 2]" in msg
    rc, msg = _create_rc(model, n_steps=1)
    assert rc == _lib.OU_EINVAL and "n_steps must be in [2, 256]" in msg
    rc, msg = _create_rc(model, warm_start=N_STEPS)
    assert rc == _lib.OU_EINVAL and "warm_start must be < n_steps" in msg
    rc, msg = _create_rc(model, enh_flags=_lib.OU_ENH_NO_PEAK_GUARD << 4)
    assert rc == _lib.OU_EINVAL and "enh_flags" in msg
    rc, msg = _create_rc(model, segment=(1 << 31) - 1 - tot, overlap=0)
    assert rc == _lib.OU_EINVAL and "segment too long for one pass of ou_enhance" in msg
    rc, msg = _create_rc(model, ws_bytes=4096)
    assert rc == _lib.OU_ENOMEM and "ou_stream_workspace_bytes" in msg
    # the cheap modes on a model without the decoupling layer: the message of ou_enhance
    plain, _, _ = get_model("OR16s")
    for over in (dict(warm_start=0), dict(enh_flags=_lib.OU_ENH_USE_AUX_SIGNAL)):
        rc, msg = _create_rc(plain, **over)
        assert rc == _lib.OU_ENOTIMPL and msg == "aux_to_wav needs the snake signal-decoupling layer (UNIVERSE++)"


def test_capacity_is_checked_before_anything_is_launched_and_destroyed_streams_are_refused():
    model, spec, _ = get_model(NAME)
    tot = spec.tot_ds
    S, V = 4 * tot, tot
    x = _signal(spec, 1, S + 3, seed=1070)
    st = RawStream(model, 1, S, V)
    L = model._L
    out = torch.full((1, S), SENTINEL, device="cuda")
    n_out = ctypes.c_int64(-1)
    n0 = model.launch_stats()
    rc = L.ou_stream_push(st.s, _ptr(x), x.stride(0), S + 3, _ptr(out), out.stride(0), S - V - 1, byref(n_out), model._stream())
    assert rc == _lib.OU_EINVAL and f"is below the {S - V} samples this call emits" in L.ou_last_error(model._handle).decode()
    torch.cuda.synchronize()
    assert model.launch_stats() == n0 and bool((out == SENTINEL).all()) and n_out.value == -1
    y = st.run(x)  # the refused push left the stream where it was
    ref = RawStream(model, 1, S, V)
    assert torch.equal(y, ref.run(x))
    ref.close()
    dead = c_void_p(st.s.value)
    st.close()
    rc = L.ou_stream_push(dead, _ptr(x), x.stride(0), 1, _ptr(out), out.stride(0), S, byref(n_out), model._stream())
    assert rc == _lib.OU_EINVAL and "not a live stream" in L.ou_last_error(None).decode()


def test_workspace_is_the_walk_plus_the_stream_areas():
    model, spec, _ = get_model(NAME)
    tot = spec.tot_ds
    L = model._L
    al = lambda n: (n + 255) & ~255  # noqa: E731
    for C, S, V in ((1, 4 * tot, tot), (3, 6 * tot, 0), (2, 4 * tot, 2 * tot)):
        need, walk = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(L.ou_stream_workspace_bytes(model._handle, C, S + 3, V + 1, byref(need)), model._handle)
        _lib.check(L.ou_workspace_bytes(model._handle, C, S + tot, byref(walk)), model._handle)
        assert need.value == al(walk.value) + 3 * al(C * S * 4) + al(C * V * 4) + al(2 * C * (S + tot) * 4)


def test_python_object_and_cli(tmp_path, monkeypatch):
    monkeypatch.setattr(A, "_torchaudio", lambda: None)  # the built-in WAV codec, whatever else this process has imported
    model, spec, _ = get_model(NAME)
    tot = spec.tot_ds
    S, V = 4 * tot, tot
    T = 2 * S - tot
    src = tmp_path / "in.wav"
    A.save(src, synth_mix(spec, 2, T, seed=1080), spec.fs)
    x = A.load(src)[0].cuda().contiguous()
    raw = RawStream(model, 2, S, V, seed=5)
    ref = raw.run(x)
    raw.close()
    with model.stream(channels=2, segment_s=S / spec.fs, overlap_s=V / spec.fs, seed=5, n_steps=N_STEPS) as st:
        assert st.latency_samples == S
        parts = [st.push(x[:, :100]), st.push(x[:, 100:100]), st.push(x[:, 100:])]
        assert [p.shape[1] for p in parts] == [0, 0, 2 * (S - V)]  # the third push completes both windows
        parts.append(st.flush())
        assert torch.equal(torch.cat(parts, dim=1), ref)
        one = st.push(x[:, :S])  # the stream starts over after a flush
        assert torch.equal(one, ref[:, :S - V])
        st.flush()
    with pytest.raises(ValueError):
        st.push(x)
    with model.stream(segment_s=S / spec.fs, overlap_s=V / spec.fs, seed=5, n_steps=N_STEPS) as st1:  # one channel: 1-D in and out
        y = torch.cat([st1.push(x[0]), st1.flush()])
    raw1 = RawStream(model, 1, S, V, seed=5)  # (row 0 alone: a C = 2 stream gives its rows to round-off, not bit for bit)
    assert y.shape == (T,) and torch.equal(y, raw1.run(x[:1].contiguous())[0])
    raw1.close()
    out = tmp_path / "out.wav"
    cli.main([str(src), str(out), "--segment-seconds", repr(S / spec.fs), "--segment-overlap", repr(V / spec.fs), "--stream",
              repr(0.37 * S / spec.fs), "--seed", "5", "--n_steps", str(N_STEPS)], model=model)
    want = tmp_path / "want.wav"
    A.save(want, ref.cpu(), spec.fs)
    assert torch.equal(A.load(out)[0], A.load(want)[0])
