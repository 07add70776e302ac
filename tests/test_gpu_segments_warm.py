"""GPU (-m gpu): the two cheap modes of `enhance` in the segmented calls ou_enhance_segments / ou_enhance_segments_var
(Universe.enhance_long / enhance_long_many): `use_aux_signal` -- a window's result is its own conditioner estimate
through the decoupling layer -- and `warm_start=k` -- the sampler starts at step k from that estimate plus noise.

  1. one window is `enhance` with the same arguments, bit for bit, and the generator ends where `enhance` leaves it;
  2. the noise planes are those of ou_enhance's convention (plane d - k = draw d of the absolute step d - 1);
  3. the aux exit stitches the windows' `wav`: the last group's taps through the float64 stitch of tests/seg_fp64.py;
  4. rows of lengths of their own (a ragged group and a FULL row): every row is the call on that row alone, zero behind its end;
  5. what is decided on the host: no decoupling layer, warm_start = n_steps, a cold-sized workspace runs both modes;
  6. against the whole-file call on the same noise: measured once, gated 6 dB below.

The ensemble forms (ou_enhance_segments_ensemble, _var_ensemble) keep refusing both modes: tests/test_gpu_segments_ensemble.py and
tests/test_gpu_segments_var_ensemble.py hold that."""
import json
import os
from ctypes import byref, c_int32, c_int64, c_size_t, c_void_p

import pytest
import torch

import seg_fp64 as G
from open_universe_amd import _lib
from open_universe_amd.noise import CounterNoise
from test_gpu_parity import get_model
from test_gpu_segments import _si_sdr, _signal

pytestmark = pytest.mark.gpu

NAME = "PP16s"
N = 4
SEED = 0x5EED0123456789AB
SECS, SEG_S, OV_S, MAX_BATCH = 7.0, 2.0, 0.5, 3  # 5 windows per row; two rows: 10 entries in groups of 3, 3, 3, 1 (+ 2 fillers)
# segmented vs whole-file `enhance` with the same mode on the same noise, one 7 s row in 2 s windows with 0.5 s overlap: the figure
# measured on an MI355X minus 6 dB, the box-to-box margin of DESIGN 4.9 / 4.17 (profiles/segments_warm_observed.json)
GAP_MEASURED_DB = {"use_aux_signal": 75.86, "warm_start_2": 75.41}  # (the cold start on the same input: 76.48 dB)
GAP_MARGIN_DB = 6.0
_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed")


def _rng(seed=5):
    return torch.Generator(device="cuda").manual_seed(seed)


def _rows(spec, n_rows=2, secs=SECS, amp=1.0):
    T = int(round(secs * spec.fs))
    return torch.stack([amp * _signal(spec.fs, T, 10 + c) for c in range(n_rows)])  # (|x| <= 0.13 + noise: the peak guard stays idle)


def _kw(**kw):
    return dict(segment_s=SEG_S, overlap_s=OV_S, max_batch=MAX_BATCH, n_steps=N, **kw)


def _worst(a, b):
    return min(_si_sdr(a[r], b[r]) for r in range(a.shape[0]))


class _Spy:
    """Keeps what Universe._segments_run returned: the full (C, stride) rows with their tails."""

    def __init__(self, model):
        self.model, self.out, self.orig = model, None, model._segments_run

    def __enter__(self):
        def run(*a, **k):
            self.out = self.orig(*a, **k)
            return self.out
        self.model._segments_run = run
        return self

    def __exit__(self, *a):
        del self.model._segments_run


# ---- 1. one window ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_rms", [False, True])
@pytest.mark.parametrize("mode", [{"warm_start": 1}, {"warm_start": 3}, {"use_aux_signal": True}])
def test_one_window_is_the_whole_file_call(mode, keep_rms):
    model, spec, _ = get_model(NAME)
    x = _rows(spec, secs=1.5)
    T = x.shape[-1]
    ref = model.enhance(x, n_steps=N, rng=_rng(), keep_rms=keep_rms, **mode)
    g = _rng()
    y = model.enhance_long(x, segment_s=10.0, n_steps=N, rng=g, keep_rms=keep_rms, **mode)
    g_ref = _rng()
    model.advance_generator_like_enhance(g_ref, 2, T, n_steps=N, **mode)
    assert torch.equal(g.get_state(), g_ref.get_state())
    if mode.get("use_aux_signal"):
        assert torch.equal(g.get_state(), _rng().get_state())  # no draw at all
    assert y.shape == x.shape
    if not torch.equal(y, ref):
        worst = _worst(ref, y)
        print(f"{mode} keep_rms={keep_rms} one window: not bit-identical, {worst:.1f} dB")
        assert worst >= 100.0


# ---- 2. the noise planes ---------------------------------------------------------------------------------------------------------
def test_noise_planes_follow_the_absolute_step():
    model, spec, _ = get_model(NAME)
    x = _rows(spec)
    C, T = x.shape
    Tp = T + (spec.tot_ds - T % spec.tot_ds)
    k = 2
    src = CounterNoise(SEED, 3)
    ids = src.stream_ids(C)
    got = model.enhance_long(x, rng=src, warm_start=k, **_kw())

    def planes(draws):
        return torch.stack([model.noise_fill(ids, [0] * C, [Tp] * C, SEED, d, Tp) for d in draws]).contiguous()

    S, Ov = int(SEG_S * spec.fs), int(OV_S * spec.fs)

    def on_tensor(noise):
        return model._segments_call(x, S, Ov, MAX_BATCH, N, model.diff_kwargs.epsilon, False, noise, None, k)

    warm = planes([0] + [n + 1 for n in range(k, N - 1)])  # draw 0, then draw n + 1 of the absolute steps n = k .. N - 2: draws 0, 3
    assert warm.shape == (N - k, C, Tp)
    assert torch.equal(on_tensor(warm), got)
    cold = planes([0, 1, 2, 3])[: N - k]  # the first planes of a cold start's tensor (draws 0, 1) are a different call
    assert not torch.equal(on_tensor(cold), got)


# ---- 3. the aux exit ---------------------------------------------------------------------------------------------------------------
def test_aux_exit_stitches_wav():
    model, spec, _ = get_model(NAME)
    x = _rows(spec)
    C, T = x.shape
    S, Ov = int(SEG_S * spec.fs), int(OV_S * spec.fs)
    model.enhance_long(x, rng=_rng(), **_kw())
    cold_stats = model.launch_stats()
    g = _rng()
    out = model.enhance_long(x, rng=g, use_aux_signal=True, **_kw())
    torch.cuda.synchronize()
    aux_stats = model.launch_stats()
    assert torch.equal(g.get_state(), _rng().get_state())
    print(f"launches (all, conv): cold {cold_stats}, aux exit {aux_stats}")
    assert aux_stats[1] < cold_stats[1] and aux_stats[0] < cold_stats[0]
    geos = [G.Row(T, spec.tot_ds, S, Ov) for _ in range(C)]
    Bw, real, slots, n_groups, Tw = G.last_group(geos, MAX_BATCH, False)
    assert (Bw, n_groups, len(real)) == (3, 4, 1) and real[0][1] > 0  # the last group: one real entry behind a carry, two fillers
    wav = model.tensor("wav").cpu().clone()
    assert wav.shape == (Bw, 1, Tw)
    off, c_, t_ = c_size_t(), c_int32(), c_int32()
    assert model._L.ou_tensor(model._handle, b"seg.carry", byref(off), byref(c_), byref(t_)) == 0
    carry = model._ws[off.value: off.value + 4 * t_.value].view(torch.float32).view(1, 1, t_.value).cpu().clone()
    with pytest.raises(KeyError):
        model.tensor("seg.z")  # no noise was read
    rep = G.check_stitch(out.cpu(), geos, real, wav, carry, Bw, 1, C, whole=False)
    print(f"aux exit {rep} err / e32 = {rep.lib_ratio:.2f}")
    assert rep.ref_peak < 1.0 - 1e-3, "the peak guard was not idle"
    assert rep.held > 0 and rep.excluded == 0 and rep.ok(), str(rep)
    again = model.enhance_long(x, rng=_rng(), use_aux_signal=True, **_kw())
    assert torch.equal(out, again)


# ---- 4. rows of lengths of their own -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [{"warm_start": 2}, {"use_aux_signal": True}])
def test_rows_of_their_own_lengths(mode):
    model, spec, _ = get_model(NAME)
    fs = spec.fs
    lens = [spec.tot_ds - 1, int(1.0 * fs), int(1.3 * fs), int(SECS * fs)]  # three SHORT entries (one ragged group), one FULL row
    groups = _lib.segment_groups(spec.tot_ds, lens, int(SEG_S * fs), int(OV_S * fs), MAX_BATCH)
    assert list(groups["group_ragged"]) == [0, 0, 1]
    sigs = [_signal(fs, n, 20 + i) for i, n in enumerate(lens)]
    srcs = [CounterNoise(SEED, 50 + i) for i in range(len(lens))]
    with _Spy(model) as spy:
        outs = model.enhance_long_many(sigs, srcs, **_kw(**mode))
    full = spy.out
    assert full.shape == (len(lens), max(lens))
    for i, n in enumerate(lens):
        assert torch.isfinite(outs[i]).all() and float(outs[i].abs().max()) > 0
        assert not bool(full[i, n:].any()), f"row {i} is not zero behind its end"
        alone = model.enhance_long(sigs[i], rng=srcs[i], **_kw(**mode))
        fig = _si_sdr(alone, outs[i])
        print(f"{mode} row {i} ({n} samples): {fig:.1f} dB from the call on the row alone")
        assert fig >= 100.0


@pytest.mark.parametrize("mode", [{"warm_start": 2}, {"use_aux_signal": True}])
def test_rows_of_one_length_are_the_plain_call(mode):
    model, spec, _ = get_model(NAME)
    x = _rows(spec)
    C, T = x.shape
    S, Ov = int(SEG_S * spec.fs), int(OV_S * spec.fs)
    eps = model.diff_kwargs.epsilon
    counter = (SEED, CounterNoise(SEED, 7).stream_ids(C))
    warm, aux = mode.get("warm_start"), bool(mode.get("use_aux_signal"))
    plan = model._segments_plan(C, T, S, Ov, MAX_BATCH, t_raw=(c_int64 * C)(*([T] * C)), warm_start=warm, use_aux_signal=aux)
    var = model._segments_run(plan, x, N, eps, False, None, counter)
    plain = model._segments_call(x, S, Ov, MAX_BATCH, N, eps, False, None, counter, warm, aux)
    assert torch.equal(var, plain)


# ---- 5. decided on the host --------------------------------------------------------------------------------------------------------
def test_refusals_decided_on_the_host():
    model, spec, _ = get_model("OR16s")  # no signal decoupling layer
    x = _rows(spec, n_rows=1, secs=3.0)
    many = [x[0], x[0, :5000]]
    # (a good call of the same shape first: it leaves the prepared workspace and its own launch records, which a refusal keeps)
    for good, bad in ((lambda **kw: model.enhance_long(x, rng=_rng(), **kw), "enhance_long"),
                      (lambda **kw: model.enhance_long_many(many, _rng(), **kw), "enhance_long_many")):
        good(**_kw())
        torch.cuda.synchronize()
        stats0 = model.launch_stats()
        for mode in ({"warm_start": 1}, {"use_aux_signal": True}):
            with pytest.raises(NotImplementedError, match="decoupling"):
                good(**_kw(**mode))
            assert model.launch_stats() == stats0, (bad, mode)  # nothing was enqueued
    model, spec, _ = get_model(NAME)
    x = _rows(spec, n_rows=1, secs=3.0)
    for bad in (N, N + 1, -1):
        with pytest.raises(ValueError, match="warm_start"):
            model.enhance_long(x, rng=_rng(), **_kw(warm_start=bad))
    assert torch.isfinite(model.enhance_long(x, rng=_rng(), **_kw(warm_start=N - 1))).all()  # and the model takes a warm start


@pytest.mark.parametrize("warm,flags", [(1, 0), (-1, _lib.OU_ENH_USE_AUX_SIGNAL)])
def test_a_cold_sized_workspace_runs_both_modes(warm, flags):
    model, spec, _ = get_model(NAME)
    L, h = model._L, model._handle
    x = _rows(spec).contiguous()
    C, T = x.shape
    Tp = T + (spec.tot_ds - T % spec.tot_ds)
    S, Ov = int(SEG_S * spec.fs), int(OV_S * spec.fs)
    need, B, Lw = c_size_t(), c_int32(), c_int32()
    assert L.ou_segments_workspace_bytes(h, C, T, S, Ov, MAX_BATCH, byref(need), byref(B), byref(Lw)) == _lib.OU_OK
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")  # exactly what the sizer asks for
    st = model._stream()
    with torch.cuda.device(model.device):
        assert L.ou_workspace_init(h, B.value, Lw.value, c_void_p(ws.data_ptr()), c_size_t(need.value), st) == _lib.OU_OK
        n_planes = N - warm if warm >= 0 else 0
        noise = torch.randn(max(n_planes, 1), C, Tp, device="cuda", generator=_rng(9))
        out = torch.empty(C, T, device="cuda")
        rc = L.ou_enhance_segments(h, c_void_p(x.data_ptr()), c_void_p(out.data_ptr()), c_void_p(noise.data_ptr()) if n_planes else None,
                                   C, T, S, Ov, MAX_BATCH, N, float(model.diff_kwargs.epsilon), None, warm, flags,
                                   c_void_p(ws.data_ptr()), c_size_t(need.value), st)
    assert rc == _lib.OU_OK, L.ou_last_error(h)
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0  # the status word of the walk
    assert torch.isfinite(out).all() and float(out.abs().max()) > 0
    # ... and it is the call of the front end on the same noise
    want = model._segments_call(x, S, Ov, MAX_BATCH, N, model.diff_kwargs.epsilon, False, noise if n_planes else None, None,
                                warm if warm >= 0 else None, bool(flags))
    assert torch.equal(out, want)


# ---- 6. against the whole-file call ------------------------------------------------------------------------------------------------
def test_against_the_whole_file_call():
    model, spec, _ = get_model(NAME)
    x = _rows(spec, n_rows=1)[0]
    kw = dict(segment_s=SEG_S, overlap_s=OV_S, n_steps=N)
    figs = {}
    for key, mode in (("use_aux_signal", {"use_aux_signal": True}), ("warm_start_2", {"warm_start": 2}), ("cold", {})):
        whole = model.enhance(x, n_steps=N, rng=_rng(), **mode)
        y = model.enhance_long(x, rng=_rng(), **kw, **mode)
        assert y.shape == x.shape and torch.isfinite(y).all()
        figs[key] = _si_sdr(whole, y)
    print("segmented vs whole-file SI-SDR, 7 s in 2 s windows, 0.5 s overlap: " + ", ".join(f"{k} {v:.2f} dB" for k, v in figs.items()))
    os.makedirs(_OUT, exist_ok=True)
    with open(os.path.join(_OUT, "segments_warm_observed.json"), "w") as f:
        json.dump({k: round(v, 2) for k, v in figs.items()}, f, indent=1, sort_keys=True)
    for key, measured in GAP_MEASURED_DB.items():
        assert figs[key] >= measured - GAP_MARGIN_DB, (key, figs[key], measured)
