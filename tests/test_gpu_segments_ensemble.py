"""GPU (-m gpu): ensembles of segmented rows (Universe.enhance_long_ensemble, ou_enhance_segments_ensemble).

Member e of row c is, by definition, `enhance_long` of row c alone on that member's noise, and out[c] is `ensemble_reduce` over
the post-processed members of row c.  Reduced-width models, 3 steps, the geometry of test_gpu_segments_var.py: windows of 16
tot_ds samples overlapping by 2 tot_ds.  Base case: C = 2 rows of 70 tot_ds + 3 samples (5 windows each, the last one shifted),
E = 3, max_batch = 12 -- so Bw = 4 entries per group and three groups: a full one, one that crosses from row 0 to row 1 (a
carry, and no crossfade across the rows) and a last one with two filler entries per member.

The gate of test 1.  A member and the single-row call differ only in which kernels a group batch selects; the project's gate
for that is 100 dB (test_gpu_ensemble.py).  The same-shaped difference WITHOUT this feature -- `enhance_long` of the (2, T)
tensor at max_batch = 12 against each row alone at max_batch = 4, same models, geometry and noise, through the entry point this
feature leaves untouched -- was measured first (PARENT_MIN_DB below, profiles/segments_ensemble_observed.json), and the gate is
min(100 dB, that minimum - 3 dB), the 3 dB for draw-to-draw spread.

  1. every member against its row alone (noise tensor and CounterNoise), SI-SDR and plain SNR;
  2. E = 1 is `enhance_long` bit for bit, for all three statistics;
  3. ens_share = 0 is `enhance_long` of the replicated batch bit for bit (same (batch, length)); the default stays within the gate;
  4. `out` is the stateless `ensemble_reduce` of the members bit for bit; keep_rms restores every member to its input row's RMS;
     a loud input leaves every member's peak <= 1;
  5. two runs are bit-identical; `enhance_long` and `enhance_ensemble` around the new call are bit-identical to themselves;
  6. a shared generator ends where advance_generator_like_enhance(g, E * C, T) leaves it;
  7. every refusal returns its code and enqueues nothing;
  8. the shared conditioner enqueues fewer launches than ens_share = 0."""
import ctypes
import json
import os
from ctypes import c_int32, c_size_t, c_void_p

import pytest
import torch

import restatement as O
from helpers import synth_mix
from open_universe_amd import _lib
from open_universe_amd.noise import CounterNoise
from open_universe_amd.universe import ensemble_reduce
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

N = 3
E, C, MAX_BATCH, ALONE_BATCH = 3, 2, 12, 4
MODELS = ["PP16s", "PP16m", "PP24s"]
STATS = ["mean", "median", "signal_median"]
# `enhance_long` of the (2, T) tensor at max_batch = 12 against each row alone at max_batch = 4 (gpu: MI355X), the worst row of
# {noise tensor, CounterNoise} x three draws each: (SI-SDR, SNR) in dB per model -- measured before the gate was fixed.  The
# smallest, 119.82 dB, less 3 dB is above the project's 100 dB: the gate is 100 dB.
PARENT_MIN_DB = {"PP16s": (120.07, 120.07), "PP16m": (119.82, 119.82), "PP24s": (125.87, 125.87)}
GATE_DB = min(100.0, min(min(v) for v in PARENT_MIN_DB.values()) - 3.0)
_OBSERVED = {}


def _observe(case, si, snr):
    _OBSERVED[case] = {"si_sdr_db": round(float(si), 2), "snr_db": round(float(snr), 2)}
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "segments_ensemble_observed.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(_OBSERVED)
        old["parent_min_db"] = {k: {"si_sdr_db": v[0], "snr_db": v[1]} for k, v in PARENT_MIN_DB.items()}
        old["gate_db"] = GATE_DB
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def _geom(spec):
    td = spec.tot_ds
    return 16 * td, 2 * td, 70 * td + 3


def _kw(spec, max_batch=MAX_BATCH):
    S, Ov, _ = _geom(spec)
    return dict(segment_s=S / spec.fs, overlap_s=Ov / spec.fs, max_batch=max_batch, n_steps=N)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _rows(spec, C_=C, T=None, seed=2400):
    return synth_mix(spec, C_, _geom(spec)[2] if T is None else T, seed=seed).cuda()


def _alone(model, spec, row, noise=None, counter=None, keep_rms=False):
    """`enhance_long` of ONE row on an explicit (n_steps, 1, T_pad) noise tensor, or on one explicit stream id."""
    S, Ov, _ = _geom(spec)
    return model._segments_call(row[None, :].contiguous(), S, Ov, ALONE_BATCH, N, model.diff_kwargs.epsilon, keep_rms,
                                None if noise is None else noise.contiguous(), counter)[0]


def _batch_length(model, spec, C_, T, max_batch, E_=None):
    S, Ov, _ = _geom(spec)
    need, B, L = c_size_t(), c_int32(), c_int32()
    if E_ is None:
        _lib.check(model._L.ou_segments_workspace_bytes(model._handle, C_, T, S, Ov, max_batch, ctypes.byref(need),
                                                        ctypes.byref(B), ctypes.byref(L)), model._handle)
    else:
        _lib.check(model._L.ou_segments_ensemble_workspace_bytes(model._handle, C_, T, S, Ov, max_batch, E_, ctypes.byref(need),
                                                                 ctypes.byref(B), ctypes.byref(L)), model._handle)
    return B.value, L.value


def _worst(refs, gots):
    figs = [O.si_sdr(r.cpu(), y.cpu()) for r, y in zip(refs, gots)]
    return min(float(f) for f in figs), min(f.snr for f in figs)


class _share:
    """`with _share(model, 0):` -- ens_share for the calls inside, back to the default behind them."""

    def __init__(self, model, v):
        self.model, self.v = model, v

    def __enter__(self):
        self.model.set_option("ens_share", self.v)

    def __exit__(self, *a):
        self.model.set_option("ens_share", 1)


_CACHE = {}


def _base(name, mode):
    """The base case and every member's row alone, computed once per (model, noise mode)."""
    key = (name, mode)
    if key not in _CACHE:
        model, spec, _ = get_model(name)
        T = _geom(spec)[2]
        x = _rows(spec)
        if mode == "tensor":
            out, mem = model.enhance_long_ensemble(x, E, "median", rng=_gen(300), return_members=True, **_kw(spec))
            noise = model.draw_noise_like_enhance(_gen(300), E * C, T, N)  # what the call drew: (n_steps, E * C, T_pad)
            alone = [_alone(model, spec, x[r % C], noise=noise[:, r:r + 1]) for r in range(E * C)]
        else:
            src = CounterNoise(77, 5)
            out, mem = model.enhance_long_ensemble(x, E, "median", rng=src, return_members=True, **_kw(spec))
            ids = src.stream_ids(C, E)
            alone = [_alone(model, spec, x[r % C], counter=(src.seed, [ids[r]])) for r in range(E * C)]
        _CACHE[key] = (x, out, mem, alone)
    return _CACHE[key]


# ---- 1. every member is its row alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["tensor", "counter"])
@pytest.mark.parametrize("name", MODELS)
def test_every_member_is_the_row_alone(name, mode):
    model, spec, _ = get_model(name)
    td = spec.tot_ds
    S, Ov, T = _geom(spec)
    n_win = len(_lib.segment_plan(td, T, S, Ov)["starts"])
    assert n_win == 5 and _batch_length(model, spec, C, T, MAX_BATCH, E) == (12, S)  # Bw = 4: groups of 4, 4 and 2 entries
    x, out, mem, alone = _base(name, mode)
    assert out.shape == x.shape and mem.shape == (E,) + tuple(x.shape)
    assert torch.isfinite(mem).all() and torch.isfinite(out).all()
    si, snr = _worst(alone, list(mem.reshape(E * C, -1)))
    print(f"segments_ensemble.{name}.{mode}: worst member vs its row alone SI-SDR {si:.1f} dB, SNR {snr:.1f} dB; gate {GATE_DB:.1f}")
    _observe(f"member_vs_alone.{name}.{mode}", si, snr)
    assert si >= GATE_DB and snr >= GATE_DB


# ---- 2. E = 1 is enhance_long ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_one_member_is_enhance_long_bit_for_bit(name):
    model, spec, _ = get_model(name)
    x = _rows(spec)
    kw = _kw(spec, max_batch=ALONE_BATCH)
    ref = model.enhance_long(x, rng=_gen(5), **kw)
    ref_c = model.enhance_long(x, rng=CounterNoise(5, 2), keep_rms=True, **kw)
    assert _batch_length(model, spec, C, x.shape[-1], ALONE_BATCH, 1) == _batch_length(model, spec, C, x.shape[-1], ALONE_BATCH)
    for stat in STATS:
        out, mem = model.enhance_long_ensemble(x, 1, stat, rng=_gen(5), return_members=True, **kw)
        assert torch.equal(out, ref) and torch.equal(mem[0], ref), stat
        out = model.enhance_long_ensemble(x, 1, stat, rng=CounterNoise(5, 2), keep_rms=True, **kw)
        assert torch.equal(out, ref_c), stat
    # a single (T,) signal keeps its shape
    out, mem = model.enhance_long_ensemble(x[0], 1, rng=_gen(6), return_members=True, **kw)
    assert out.shape == x[0].shape and mem.shape == (1,) + tuple(x[0].shape)
    assert torch.equal(out, model.enhance_long(x[0], rng=_gen(6), **kw))


# ---- 3. ens_share = 0 is the replicated batch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_unshared_path_is_enhance_long_on_the_replicated_batch(name):
    model, spec, _ = get_model(name)
    td = spec.tot_ds
    S, Ov, _ = _geom(spec)
    T = 55 * td + 9  # T_pad = 56 tot_ds: 4 windows, the last one shifted
    assert len(_lib.segment_plan(td, T, S, Ov)["starts"]) == 4
    x = _rows(spec, 1, T, seed=2500)[0]
    assert _batch_length(model, spec, 1, T, 4, 2) == _batch_length(model, spec, 2, T, 4) == (4, S)
    want = model.enhance_long(torch.stack([x, x]), rng=_gen(9), **_kw(spec, 4))  # draws (2, 1, T_pad) per step, as E * C = 2 does
    with _share(model, 0):
        _, mem = model.enhance_long_ensemble(x, 2, "median", rng=_gen(9), return_members=True, **_kw(spec, 4))
    assert torch.equal(mem, want)
    _, mem_s = model.enhance_long_ensemble(x, 2, "median", rng=_gen(9), return_members=True, **_kw(spec, 4))
    si, snr = _worst(list(want), list(mem_s))
    print(f"segments_ensemble.{name}.shared_vs_unshared: SI-SDR {si:.1f} dB, SNR {snr:.1f} dB")
    _observe(f"shared_vs_unshared.{name}", si, snr)
    assert si >= GATE_DB and snr >= GATE_DB


# ---- 4. reduce and post ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat", STATS)
def test_out_is_the_reduce_of_the_members(stat):
    model, spec, _ = get_model("PP16m")
    x = _rows(spec)
    out, mem = model.enhance_long_ensemble(x, E, stat, rng=CounterNoise(77, 5), return_members=True, **_kw(spec))
    assert torch.equal(out, ensemble_reduce(mem, stat))
    if stat == "median":  # (the members do not depend on the statistic: those of the base case)
        assert torch.equal(mem, _base("PP16m", "counter")[2])


@pytest.mark.parametrize("name", MODELS)
def test_keep_rms_and_peak_guard_per_member(name):
    model, spec, _ = get_model(name)
    x = _rows(spec)
    rms = lambda v: float(v.double().square().mean().sqrt())  # noqa: E731
    quiet = x * torch.tensor([[0.02], [0.3]], device=x.device)  # two rows of different levels: row r % C decides
    _, mem = model.enhance_long_ensemble(quiet, E, rng=CounterNoise(3, 1), keep_rms=True, return_members=True, **_kw(spec))
    for e in range(E):
        for c in range(C):
            assert float(mem[e, c].abs().max()) < 1.0  # (the peak guard did not divide)
            assert rms(mem[e, c]) == pytest.approx(rms(quiet[c]), rel=1e-4), (e, c)
    # loud (as tests/golden/make_golden.py::make_loud): the RMS restore puts every member far above full scale, so the guard
    # divides the member row by its own peak -- x / max|x| is 1 to an ulp at the peak, never above
    loud = x * 40.0
    assert rms(loud[0]) > 2.0 and rms(loud[1]) > 2.0
    _, mem = model.enhance_long_ensemble(loud, E, rng=CounterNoise(3, 1), keep_rms=True, return_members=True, **_kw(spec))
    peaks = [float(mem[e, c].abs().max()) for e in range(E) for c in range(C)]
    print(f"{name}: member peaks of the loud input " + ", ".join(f"{p:.7f}" for p in peaks))
    for p in peaks:
        assert 1.0 - 1e-6 <= p <= 1.0
    # without keep_rms the guard sees the member's own level
    _, mem = model.enhance_long_ensemble(loud, E, rng=CounterNoise(3, 1), return_members=True, **_kw(spec))
    assert float(mem.abs().max()) <= 1.0


# ---- 5. repeatability and isolation -----------------------------------------------------------------------------------------------
def test_repeatable_and_leaves_the_other_entry_points_alone():
    model, spec, _ = get_model("PP16m")
    x = _rows(spec)
    short = synth_mix(spec, 2, spec.tot_ds * 11 + 5).cuda()
    long_before = model.enhance_long(x, rng=_gen(4), **_kw(spec, ALONE_BATCH))
    long_stats = model.launch_stats()
    ens_before = model.enhance_ensemble(short, 3, "median", n_steps=N, rng=_gen(4))
    ens_stats = model.launch_stats()
    a = model.enhance_long_ensemble(x, E, "signal_median", rng=_gen(8), return_members=True, **_kw(spec))
    b = model.enhance_long_ensemble(x, E, "signal_median", rng=_gen(8), return_members=True, **_kw(spec))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(model.enhance_long(x, rng=_gen(4), **_kw(spec, ALONE_BATCH)), long_before)
    assert model.launch_stats() == long_stats
    assert torch.equal(model.enhance_ensemble(short, 3, "median", n_steps=N, rng=_gen(4)), ens_before)
    assert model.launch_stats() == ens_stats
    assert model.options() == _lib.option_defaults()


# ---- 6. generator -------------------------------------------------------------------------------------------------------------------
def test_shared_generator_advances_like_enhance_of_the_member_rows():
    model, spec, _ = get_model("PP16s")
    x = _rows(spec)
    g, g_ref = _gen(21), _gen(21)
    model.enhance_long_ensemble(x, E, rng=g, **_kw(spec))
    model.advance_generator_like_enhance(g_ref, E * C, x.shape[-1], n_steps=N)
    assert torch.equal(g.get_state(), g_ref.get_state())


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    model, spec, _ = get_model("PP16m")
    L, h = model._L, model._handle
    S, Ov, T = _geom(spec)
    Tp = T + (spec.tot_ds - T % spec.tot_ds)
    x = _rows(spec)
    model.enhance_long_ensemble(x, E, rng=_gen(1), **_kw(spec))  # a good call first: leaves the prepared workspace
    ws = model._ws
    small = model._private_workspace(4, S)  # prepared for another batch size
    torch.cuda.synchronize()
    stats0, word0 = model.launch_stats(), int(ws[:4].view(torch.int32).item())
    out = torch.empty(C, T, device="cuda")
    mem = torch.empty(E * C, T, device="cuda")
    noise = torch.zeros(N, E * C, Tp, device="cuda")
    sig = (ctypes.c_float * 3)(1.0, 0.5, 0.1)

    def call(E_=E, stat=1, flags=0, noise_p=noise, mem_p=mem, warm=-1, max_batch=MAX_BATCH, ws_t=ws, ws_n=None):
        return L.ou_enhance_segments_ensemble(
            h, c_void_p(x.data_ptr()), c_void_p(out.data_ptr()), c_void_p(mem_p.data_ptr()) if mem_p is not None else None,
            c_void_p(noise_p.data_ptr()) if noise_p is not None else None, C, T, E_, stat, S, Ov, max_batch, N, 1.3, sig, warm,
            flags, c_void_p(ws_t.data_ptr()), c_size_t(ws_t.numel() if ws_n is None else ws_n), model._stream())

    assert call(E_=0) == _lib.OU_EINVAL and call(E_=33, max_batch=64) == _lib.OU_EINVAL
    assert call(E_=3, max_batch=2) == _lib.OU_EINVAL  # E > max_batch
    assert call(stat=3) == _lib.OU_EINVAL and call(stat=-1) == _lib.OU_EINVAL
    assert call(mem_p=None) == _lib.OU_EINVAL
    assert call(warm=0) == _lib.OU_EINVAL and call(warm=1) == _lib.OU_EINVAL
    assert call(flags=_lib.OU_ENH_USE_AUX_SIGNAL) == _lib.OU_EINVAL
    assert call(noise_p=None) == _lib.OU_EINVAL  # tensor mode without a tensor
    assert call(ws_t=small) == _lib.OU_ENOMEM  # the walk's workspace of another batch size: too small
    # large enough, never prepared by ou_workspace_init (a view 256 bytes into a fresh block: the caching allocator may hand
    # torch.empty_like(ws) the address of a freed workspace this handle once prepared, and the library knows workspaces by address)
    never = torch.empty(ws.numel() + 256, dtype=ws.dtype, device=ws.device)[256:]
    assert call(ws_t=never) == _lib.OU_EINVAL
    assert call(ws_n=1 << 20) == _lib.OU_ENOMEM
    with model._counter_source(3, CounterNoise(3, 0).stream_ids(C)):  # n_streams = C != E * C
        assert call(noise_p=None) == _lib.OU_EINVAL
    with model._counter_source(3, CounterNoise(3, 0).stream_ids(C, E)):
        assert call() == _lib.OU_EINVAL  # a noise pointer while a source is set
    n, b, ln = c_size_t(), c_int32(), c_int32()
    for bad_e, mb in ((0, 12), (33, 64), (3, 2)):
        assert L.ou_segments_ensemble_workspace_bytes(h, C, T, S, Ov, mb, bad_e, ctypes.byref(n), ctypes.byref(b),
                                                      ctypes.byref(ln)) == _lib.OU_EINVAL
    torch.cuda.synchronize()
    assert model.launch_stats() == stats0 and int(ws[:4].view(torch.int32).item()) == word0
    assert call() == _lib.OU_OK  # and the same arguments without a fault are taken
    model._status(force=True)
    assert model.launch_stats()[0] > 0


# ---- 8. the shared conditioner ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_shared_conditioner_enqueues_fewer_launches(name):
    model, spec, _ = get_model(name)
    x = _rows(spec)
    model.enhance_long_ensemble(x, E, rng=CounterNoise(77, 5), **_kw(spec))
    shared = model.launch_stats()[0]
    with _share(model, 0):
        model.enhance_long_ensemble(x, E, rng=CounterNoise(77, 5), **_kw(spec))
        unshared = model.launch_stats()[0]
    print(f"{name}: launches with the shared conditioner {shared}, with ens_share = 0 {unshared}")
    assert 0 < shared < unshared
