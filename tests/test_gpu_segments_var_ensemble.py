"""GPU (-m gpu): ensembles of segmented rows with lengths of their own (Universe.enhance_long_many_ensemble,
ou_enhance_segments_var_ensemble).

Member e of row c is, by definition, `enhance_long` of row c alone on that member's noise, and out[c] is `ensemble_reduce` over
the post-processed members of row c at the row's own length.  The geometry of test_gpu_segments_var.py: reduced-width models, 3
steps, windows of 16 tot_ds samples overlapping by 2 tot_ds, the six lengths [41 td + 7, 9 td, 57, 16 td - 1, 16 td, 70 td + 3];
E = 3 at max_batch = 12, so Bw = 4: 10 FULL entries in groups of 4, 4 and 2 (a partly filled last group with fillers; the carry
crosses a group boundary and a row boundary) and one ragged SHORT group of 3 entries plus a filler.  No row stride is a multiple
of 4 samples (T_raw_max = 70 td + 3).

  1. every member of every row against that row alone (noise tensor and CounterNoise): >= 80 dB SI-SDR and plain SNR, the floor
     of "ragged row vs the row alone" on these models (FLOOR_DB of test_gpu_segments_var.py); the observed minima are printed;
  2. E = 1 is ou_enhance_segments_var bit for bit for all three stats, same (batch, length);
  3. equal lengths (2 rows of 41 td + 7) are ou_enhance_segments_ensemble bit for bit in out and members, same (batch, length);
  4. C = 1 is ou_enhance_segments_ensemble of that row bit for bit;
  5. ens_share = 0 is ou_enhance_segments_var on the E-times replicated list of rows with the same noise, bit for bit -- on rows
     whose two plans put the same window into the same walk row of walks of one size (the library promises equal bits only
     between walks of one batch size: another size may select other kernels): the rows [41 td + 7, 9 td, 57, 16 td - 1] at E = 2
     and max_batch = 6 have 3 FULL and 3 SHORT entries, Bw = 3, so the call runs [3 entries x 2 members] where the var call on
     the 8 rows runs [3 entries of copy 0, 3 of copy 1], FULL and SHORT alike; the default stays within the floor of 1;
  6. out is the stateless ensemble_reduce(members, lengths) bit for bit for the three stats; out and every member row are zero
     behind t_raw[c]; large values in the mix tails change nothing; keep_rms restores every member to its own row's RMS; peaks <= 1;
  7. two runs are bit-identical; enhance_long_many and enhance_long_ensemble before and after are bit-identical to themselves;
  8. a shared generator ends where the loop of advance_generator_like_enhance(g, E * C_i, T_i) leaves it; per-input generators
     give, per input, the result of enhance_long_ensemble(signal_i, rng=gen_i) within the floor of 1;
  9. every refusal returns its code and enqueues nothing;
 10. fewer launches than the six enhance_long_ensemble calls together;
 11. the CLI's --segment-ensemble-files 3 against --segment-ensemble-files 1 with --noise counter."""
import ctypes
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
E, MAX_BATCH, ALONE_BATCH = 3, 12, 4
FLOOR_DB = 80.0
MODELS = ["PP16s", "PP16m", "PP24s"]
STATS = ["mean", "median", "signal_median"]


def _geom(spec):
    td = spec.tot_ds
    return 16 * td, 2 * td, [41 * td + 7, 9 * td, 57, 16 * td - 1, 16 * td, 70 * td + 3]


def _kw(spec, max_batch=MAX_BATCH):
    S, Ov, _ = _geom(spec)
    return dict(segment_s=S / spec.fs, overlap_s=Ov / spec.fs, max_batch=max_batch, n_steps=N)


def _signals(spec, lens, seed=2600):
    return [synth_mix(spec, 1, L, seed=seed + i)[0].cuda() for i, L in enumerate(lens)]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _padded(spec, n):
    return n + (spec.tot_ds - n % spec.tot_ds)


def _alone(model, spec, row, noise=None, counter=None, keep_rms=False):
    """`enhance_long` of ONE row on an explicit (n_steps, 1, T_pad) noise tensor, or on one explicit stream id."""
    S, Ov, _ = _geom(spec)
    return model._segments_call(row[None, :].contiguous(), S, Ov, ALONE_BATCH, N, model.diff_kwargs.epsilon, keep_rms,
                                None if noise is None else noise.contiguous(), counter)[0]


def _check(tag, refs, gots):
    figs = [O.si_sdr(r.cpu(), y.cpu()) for r, y in zip(refs, gots)]
    si, snr = min(float(f) for f in figs), min(f.snr for f in figs)
    print(f"{tag}: worst SI-SDR {si:.1f} dB, SNR {snr:.1f} dB over {len(figs)} rows (floor {FLOOR_DB:.0f})")
    assert si >= FLOOR_DB and snr >= FLOOR_DB


def _sizer(model, spec, lens, max_batch, E_):
    S, Ov, _ = _geom(spec)
    C = len(lens)
    tr = (ctypes.c_int64 * C)(*lens)
    need, B, L = c_size_t(), c_int32(), c_int32()
    if E_ is None:
        rc = model._L.ou_segments_var_workspace_bytes(model._handle, C, tr, S, Ov, max_batch, ctypes.byref(need), ctypes.byref(B),
                                                      ctypes.byref(L))
    else:
        rc = model._L.ou_segments_var_ensemble_workspace_bytes(model._handle, C, tr, S, Ov, max_batch, E_, ctypes.byref(need),
                                                               ctypes.byref(B), ctypes.byref(L))
    _lib.check(rc, model._handle)
    return need.value, B.value, L.value


def _call(model, spec, sigs, E_, stat, noise, max_batch=MAX_BATCH, keep_rms=False, tail=123.0):
    """ou_enhance_segments_var_ensemble through ctypes on explicit noise (n_steps, E * C, T_pad_max) -> out (C, T_raw_max), members
    (E * C, T_raw_max), (batch, length).  The mix tails hold `tail`, out and members start full of 7."""
    S, Ov, _ = _geom(spec)
    lens = [int(s.shape[-1]) for s in sigs]
    C, lm = len(sigs), max(lens)
    tr = (ctypes.c_int64 * C)(*lens)
    need, B, L = _sizer(model, spec, lens, max_batch, E_)
    ws = model._segments_workspace(B, L, need)
    mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs]).contiguous()
    for c, n in enumerate(lens):
        mix[c, n:] = tail
    out = torch.full((C, lm), 7.0, device="cuda")
    mem = torch.full((E_ * C, lm), 7.0, device="cuda")
    _lib.check(model._L.ou_enhance_segments_var_ensemble(
        model._handle, c_void_p(mix.data_ptr()), c_void_p(out.data_ptr()), c_void_p(mem.data_ptr()), c_void_p(noise.data_ptr()), C, lm,
        tr, E_, _lib.ENSEMBLE_STATS[stat], S, Ov, max_batch, N, float(model.diff_kwargs.epsilon), None, -1,
        _lib.OU_ENH_KEEP_RMS if keep_rms else 0, c_void_p(ws.data_ptr()), c_size_t(ws.numel()), model._stream()), model._handle)
    model._status()
    torch.cuda.synchronize()
    return out, mem, (B, L)


def _member_noise(model, spec, lens, E_, seed):
    """(n_steps, E * C, T_pad_max), member-major: input c draws (E, T_pad_c) per step from its own generator seed + c -- what
    enhance_long_ensemble(signal_c, E, rng=that generator) draws."""
    C, tp = len(lens), [_padded(spec, n) for n in lens]
    noise = torch.zeros(N, E_, C, max(tp), device="cuda")
    for c, (n, t) in enumerate(zip(lens, tp)):
        noise[:, :, c, :t] = model.draw_noise_like_enhance(_gen(seed + c), E_, n, N)
    return noise.reshape(N, E_ * C, max(tp))


_CACHE = {}


def _base(name, mode):
    """The call on the six lengths (median, with members) and every member's row alone, once per (model, noise mode)."""
    key = (name, mode)
    if key not in _CACHE:
        model, spec, _ = get_model(name)
        _, _, lens = _geom(spec)
        sigs = _signals(spec, lens)
        C = len(sigs)
        if mode == "tensor":
            outs, mems = model.enhance_long_many_ensemble(sigs, E, "median", rngs=[_gen(300 + i) for i in range(C)],
                                                          return_members=True, **_kw(spec))
            alone = []
            for i, s in enumerate(sigs):
                noise = model.draw_noise_like_enhance(_gen(300 + i), E, lens[i], N)  # (n_steps, E, T_pad_i): what input i drew
                alone.append([_alone(model, spec, s, noise=noise[:, e:e + 1]) for e in range(E)])
        else:
            srcs = [CounterNoise(77, 5 + i) for i in range(C)]
            outs, mems = model.enhance_long_many_ensemble(sigs, E, "median", rngs=srcs, return_members=True, **_kw(spec))
            alone = [[_alone(model, spec, s, counter=(77, [srcs[i].stream_ids(1, E)[e]])) for e in range(E)]
                     for i, s in enumerate(sigs)]
        _CACHE[key] = (sigs, outs, mems, alone)
    return _CACHE[key]


# ---- 1. every member is its row alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["tensor", "counter"])
@pytest.mark.parametrize("name", MODELS)
def test_every_member_is_the_row_alone(name, mode):
    model, spec, _ = get_model(name)
    S, Ov, lens = _geom(spec)
    # the plan the docstring describes: Bw = 4, walks of 12 rows; FULL groups of 4, 4 and 2 entries, one ragged SHORT group of 3
    g = _lib.segment_groups(spec.tot_ds, lens, S, Ov, MAX_BATCH // E)
    assert g["batch"] == 4 and list(g["group_first"]) == [0, 4, 8, 10] and list(g["group_ragged"]) == [0, 0, 0, 1]
    assert len(g["row"]) == 13 and _sizer(model, spec, lens, MAX_BATCH, E)[1:] == (12, S)
    assert max(lens) % 4 != 0
    sigs, outs, mems, alone = _base(name, mode)
    for s, y, m in zip(sigs, outs, mems):
        assert y.shape == s.shape and m.shape == (E,) + tuple(s.shape)
        assert torch.isfinite(y).all() and torch.isfinite(m).all()
    _check(f"segments_var_ensemble.{name}.{mode}.member_vs_alone", [a for row in alone for a in row],
           [m[e] for m in mems for e in range(E)])


# ---- 2. E = 1 is ou_enhance_segments_var ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_one_member_is_the_var_call_bit_for_bit(name):
    model, spec, _ = get_model(name)
    _, _, lens = _geom(spec)
    sigs = _signals(spec, lens)
    ref = model.enhance_long_many(sigs, [_gen(300 + i) for i in range(len(sigs))], **_kw(spec, ALONE_BATCH))
    assert _sizer(model, spec, lens, ALONE_BATCH, 1)[1:] == _sizer(model, spec, lens, ALONE_BATCH, None)[1:]
    for stat in STATS:
        outs, mems = model.enhance_long_many_ensemble(sigs, 1, stat, rngs=[_gen(300 + i) for i in range(len(sigs))],
                                                      return_members=True, **_kw(spec, ALONE_BATCH))
        for r, y, m in zip(ref, outs, mems):
            assert torch.equal(y, r) and torch.equal(m[0], r), stat


# ---- 3. / 4. equal lengths and one row are ou_enhance_segments_ensemble --------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("rows", [2, 1])
def test_equal_lengths_are_the_segments_ensemble_bit_for_bit(name, rows):
    model, spec, _ = get_model(name)
    S, Ov, lens = _geom(spec)
    T = lens[0]
    x = torch.stack(_signals(spec, [T] * rows, seed=2700))
    ref, ref_mem = model.enhance_long_ensemble(x, E, "median", rng=_gen(9), return_members=True, **_kw(spec))
    noise = model.draw_noise_like_enhance(_gen(9), E * rows, T, N)  # what that call drew: (n_steps, E * C, T_pad)
    out, mem, (B, L) = _call(model, spec, list(x), E, "median", noise)
    assert torch.equal(out, ref) and torch.equal(mem.view(E, rows, T), ref_mem)
    need, Bs, Ls = c_size_t(), c_int32(), c_int32()
    _lib.check(model._L.ou_segments_ensemble_workspace_bytes(model._handle, rows, T, S, Ov, MAX_BATCH, E, ctypes.byref(need),
                                                             ctypes.byref(Bs), ctypes.byref(Ls)), model._handle)
    assert (B, L) == (Bs.value, Ls.value)


# ---- 5. ens_share = 0 is the var call on the replicated rows -------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_unshared_path_is_the_var_call_on_the_replicated_rows(name):
    model, spec, _ = get_model(name)
    S, Ov, lens = _geom(spec)
    lens, E2, mb = lens[:4], 2, 6
    sigs = _signals(spec, lens)
    g = _lib.segment_groups(spec.tot_ds, lens, S, Ov, mb // E2)
    assert g["batch"] == 3 and list(g["group_first"]) == [0, 3] and list(g["group_ragged"]) == [0, 1]
    g2 = _lib.segment_groups(spec.tot_ds, lens * E2, S, Ov, mb)
    assert g2["batch"] == 6 and list(g2["group_first"]) == [0, 6] and list(g2["group_ragged"]) == [0, 1]
    noise = _member_noise(model, spec, lens, E2, 500)
    # the var call on [rows, rows]: row e * C + c on the noise of member row e * C + c
    tr = (ctypes.c_int64 * (E2 * len(lens)))(*(lens * E2))
    plan = model._segments_plan(E2 * len(lens), max(lens), S, Ov, mb, t_raw=tr)
    rep = torch.stack([torch.nn.functional.pad(s, (0, max(lens) - s.shape[-1])) for s in sigs] * E2).contiguous()
    want = model._segments_run(plan, rep, N, model.diff_kwargs.epsilon, False, noise, None)
    torch.cuda.synchronize()
    model.set_option("ens_share", 0)
    try:
        _, mem, (B, _) = _call(model, spec, sigs, E2, "median", noise, max_batch=mb)
    finally:
        model.set_option("ens_share", 1)
    assert B == 6 and torch.equal(mem, want)
    _, mem_s, _ = _call(model, spec, sigs, E2, "median", noise, max_batch=mb)
    rows = [(r, lens[r % len(lens)]) for r in range(E2 * len(lens))]
    _check(f"segments_var_ensemble.{name}.shared_vs_unshared", [want[r, :n] for r, n in rows], [mem_s[r, :n] for r, n in rows])


# ---- 6. reduce and post ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat", STATS)
def test_out_is_the_reduce_of_the_members_and_tails_are_zero(stat):
    model, spec, _ = get_model("PP16m")
    _, _, lens = _geom(spec)
    sigs = _signals(spec, lens)
    C, lm = len(lens), max(lens)
    noise = _member_noise(model, spec, lens, E, 300)
    out, mem, _ = _call(model, spec, sigs, E, stat, noise)
    assert torch.isfinite(out).all() and torch.isfinite(mem).all()
    assert torch.equal(out, ensemble_reduce(mem.view(E, C, lm), stat, lens=lens))
    for c, n in enumerate(lens):
        assert not out[c, n:].any()
        for e in range(E):
            assert not mem[e * C + c, n:].any()
    assert float(mem.abs().max()) <= 1.0 and float(out.abs().max()) <= 1.0
    # other values behind the mix rows: the same bits
    out2, mem2, _ = _call(model, spec, sigs, E, stat, noise, tail=-3.0e4)
    assert torch.equal(out2, out) and torch.equal(mem2, mem)
    if stat == "median":  # the per-input draws of the base case: the same members through the Python method
        _, _, mems, _ = _base("PP16m", "tensor")
        for c, n in enumerate(lens):
            assert torch.equal(mem.view(E, C, lm)[:, c, :n], mems[c])


@pytest.mark.parametrize("name", MODELS)
def test_keep_rms_and_peak_guard_per_member(name):
    model, spec, _ = get_model(name)
    _, _, lens = _geom(spec)
    sigs = [s * g for s, g in zip(_signals(spec, lens), (0.02, 0.3, 0.1, 0.5, 0.05, 0.2))]  # a level of its own per row
    _, mems = model.enhance_long_many_ensemble(sigs, E, rngs=[CounterNoise(3, i) for i in range(len(sigs))], keep_rms=True,
                                               return_members=True, **_kw(spec))
    rms = lambda v: float(v.double().square().mean().sqrt())  # noqa: E731
    for s, m in zip(sigs, mems):
        for e in range(E):
            assert float(m[e].abs().max()) < 1.0  # (the peak guard did not divide)
            assert rms(m[e]) == pytest.approx(rms(s), rel=1e-5)  # (the tolerance of test_gpu_segments_var.py, reasoned there)
    loud = [s * 2000.0 for s in sigs]  # every RMS restore lands far above full scale: the guard divides by the member's own peak
    outs, mems = model.enhance_long_many_ensemble(loud, E, rngs=[CounterNoise(3, i) for i in range(len(sigs))], keep_rms=True,
                                                  return_members=True, **_kw(spec))
    for y, m in zip(outs, mems):
        assert float(m.abs().max()) <= 1.0 and float(y.abs().max()) <= 1.0


# ---- 7. repeatability and isolation -----------------------------------------------------------------------------------------------
def test_repeatable_and_leaves_the_other_entry_points_alone():
    model, spec, _ = get_model("PP16m")
    _, _, lens = _geom(spec)
    sigs = _signals(spec, lens)
    x = torch.stack(_signals(spec, [lens[0]] * 2, seed=2700))
    gens = lambda: [_gen(300 + i) for i in range(len(sigs))]  # noqa: E731
    many_before = model.enhance_long_many(sigs, gens(), **_kw(spec, ALONE_BATCH))
    many_stats = model.launch_stats()
    ens_before = model.enhance_long_ensemble(x, E, "median", rng=_gen(4), **_kw(spec))
    ens_stats = model.launch_stats()
    a = model.enhance_long_many_ensemble(sigs, E, "signal_median", rngs=gens(), return_members=True, **_kw(spec))
    b = model.enhance_long_many_ensemble(sigs, E, "signal_median", rngs=gens(), return_members=True, **_kw(spec))
    for k in range(len(sigs)):
        assert torch.equal(a[0][k], b[0][k]) and torch.equal(a[1][k], b[1][k])
    for r, y in zip(many_before, model.enhance_long_many(sigs, gens(), **_kw(spec, ALONE_BATCH))):
        assert torch.equal(r, y)
    assert model.launch_stats() == many_stats
    assert torch.equal(model.enhance_long_ensemble(x, E, "median", rng=_gen(4), **_kw(spec)), ens_before)
    assert model.launch_stats() == ens_stats
    assert model.options() == _lib.option_defaults()


# ---- 8. noise order -----------------------------------------------------------------------------------------------------------------
def test_shared_generator_advances_like_the_loop_over_the_inputs():
    model, spec, _ = get_model("PP16s")
    _, _, lens = _geom(spec)
    sigs = _signals(spec, lens[:4])
    ent = [torch.stack([sigs[0], sigs[0].flip(0)]), sigs[1], sigs[2], sigs[3]]  # a two-channel input and three mono ones
    g, g_ref = _gen(21), _gen(21)
    outs = model.enhance_long_many_ensemble(ent, E, rngs=g, **_kw(spec))
    for e in ent:
        model.advance_generator_like_enhance(g_ref, E * (e.shape[0] if e.ndim == 2 else 1), e.shape[-1], n_steps=N)
    assert torch.equal(g.get_state(), g_ref.get_state())
    assert [tuple(o.shape) for o in outs] == [tuple(e.shape) for e in ent]
    # per-input generators: every input gets what enhance_long_ensemble gives it alone from its generator
    outs, mems = model.enhance_long_many_ensemble(ent, E, "mean", rngs=[_gen(40 + i) for i in range(len(ent))], return_members=True,
                                                  **_kw(spec))
    refs = [model.enhance_long_ensemble(e, E, "mean", rng=_gen(40 + i), return_members=True, **_kw(spec)) for i, e in enumerate(ent)]
    assert [tuple(m.shape) for m in mems] == [tuple(r[1].shape) for r in refs]
    _check("segments_var_ensemble.PP16s.per_input_generators.members",
           [row for r in refs for row in r[1].reshape(-1, r[1].shape[-1])], [row for m in mems for row in m.reshape(-1, m.shape[-1])])
    _check("segments_var_ensemble.PP16s.per_input_generators.out", [r[0].flatten() for r in refs], [o.flatten() for o in outs])


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    model, spec, _ = get_model("PP16m")
    L, h = model._L, model._handle
    S, Ov, lens = _geom(spec)
    C, lm = len(lens), max(lens)
    sigs = _signals(spec, lens)
    noise = _member_noise(model, spec, lens, E, 300)
    _call(model, spec, sigs, E, "median", noise)  # a good call first: leaves the prepared workspace
    ws = model._ws
    small = model._private_workspace(4, S)  # prepared for another batch size
    torch.cuda.synchronize()
    stats0, word0 = model.launch_stats(), int(ws[:4].view(torch.int32).item())
    mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs]).contiguous()
    out = torch.empty(C, lm, device="cuda")
    mem = torch.empty(E * C, lm, device="cuda")
    sig = (ctypes.c_float * 3)(1.0, 0.5, 0.1)
    good = (ctypes.c_int64 * C)(*lens)

    def call(E_=E, stat=1, flags=0, noise_p=noise, mem_p=mem, warm=-1, max_batch=MAX_BATCH, ws_t=ws, ws_n=None, tr=good, C_=C,
             T_max=lm, seg=S):
        return L.ou_enhance_segments_var_ensemble(
            h, c_void_p(mix.data_ptr()), c_void_p(out.data_ptr()), c_void_p(mem_p.data_ptr()) if mem_p is not None else None,
            c_void_p(noise_p.data_ptr()) if noise_p is not None else None, C_, T_max, tr, E_, stat, seg, Ov, max_batch, N, 1.3, sig,
            warm, flags, c_void_p(ws_t.data_ptr()), c_size_t(ws_t.numel() if ws_n is None else ws_n), model._stream())

    def bad(rc, code=_lib.OU_EINVAL):
        assert rc == code and L.ou_last_error(h)

    bad(call(E_=0)); bad(call(E_=_lib.OU_MAX_ENSEMBLE + 1, max_batch=64))
    bad(call(E_=3, max_batch=2))  # E > max_batch
    many = 65535 // E + 1  # E * C > 65535 (decided from the counts alone: no row is looked at)
    bad(call(C_=many, tr=(ctypes.c_int64 * many)(*([lm] * many)), max_batch=64))
    bad(call(stat=3)); bad(call(stat=-1))
    bad(call(mem_p=None))
    bad(call(tr=None))
    for c, v in ((0, 0), (2, -5), (5, lm + 1)):
        t = list(lens)
        t[c] = v
        bad(call(tr=(ctypes.c_int64 * C)(*t)))
    bad(call(warm=0)); bad(call(warm=1))
    bad(call(flags=_lib.OU_ENH_USE_AUX_SIGNAL))
    bad(call(noise_p=None))  # tensor mode without a tensor
    # a segment too long for one pass: one row of 2^30 + 5 samples in windows of 2^30 (refused from the numbers alone)
    big = (1 << 30) + 5
    bad(call(C_=1, tr=(ctypes.c_int64 * 1)(big), T_max=big, seg=1 << 30, E_=1))
    bad(call(ws_t=small), _lib.OU_ENOMEM)  # the walk's workspace of another batch size: too small
    # large enough, never prepared by ou_workspace_init.  (Not torch.empty_like(ws): the caching allocator may hand back the
    # address of a freed workspace this handle once prepared for the same batch size, and the library knows workspaces by
    # address.  A view 256 bytes into a fresh block is an address no workspace ever started at.)
    bad(call(ws_t=torch.empty(ws.numel() + 256, dtype=ws.dtype, device=ws.device)[256:]))
    bad(call(ws_n=1 << 20), _lib.OU_ENOMEM)
    with model._counter_source(3, CounterNoise(3, 0).stream_ids(C)):  # n_streams = C != E * C
        bad(call(noise_p=None))
    with model._counter_source(3, CounterNoise(3, 0).stream_ids(C, E)):
        bad(call())  # a noise pointer while a source is set
    n, b, ln = c_size_t(), c_int32(), c_int32()
    for bad_e, mb in ((0, 12), (_lib.OU_MAX_ENSEMBLE + 1, 64), (3, 2)):
        bad(L.ou_segments_var_ensemble_workspace_bytes(h, C, good, S, Ov, mb, bad_e, ctypes.byref(n), ctypes.byref(b), ctypes.byref(ln)))
    torch.cuda.synchronize()
    assert model.launch_stats() == stats0 and int(ws[:4].view(torch.int32).item()) == word0
    assert call() == _lib.OU_OK  # and the same arguments without a fault are taken
    model._status(force=True)
    assert model.launch_stats()[0] > 0


# ---- 10. launches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_fewer_launches_than_the_calls_file_by_file(name):
    model, spec, _ = get_model(name)
    _, _, lens = _geom(spec)
    sigs = _signals(spec, lens)
    alone = 0
    for i, s in enumerate(sigs):
        model.enhance_long_ensemble(s, E, rng=CounterNoise(77, 5 + i), **_kw(spec))
        alone += model.launch_stats()[0]
    model.enhance_long_many_ensemble(sigs, E, rngs=[CounterNoise(77, 5 + i) for i in range(len(sigs))], **_kw(spec))
    together = model.launch_stats()[0]
    print(f"{name}: launches of the six enhance_long_ensemble calls {alone}, of the one call {together}")
    assert 0 < together < alone


# ---- 11. the CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_segment_ensemble_files_end_to_end(tmp_path):
    from open_universe_amd import audio as A
    from open_universe_amd.bin import enhance as cli

    model, spec, _ = get_model("PP16s")
    td = spec.tot_ds
    S, Ov, _ = _geom(spec)
    src = tmp_path / "in"
    src.mkdir()
    for i, T in enumerate((41 * td + 7, 9 * td, 20 * td + 100)):
        x = (synth_mix(spec, 1, T, seed=2800 + i) * 0.5).clamp(-1, 1)
        A.save(src / f"f{i}.wav", x, spec.fs)
    common = ["--segment-seconds", repr(S / spec.fs), "--segment-overlap", repr(Ov / spec.fs), "--segment-ensemble", str(E),
              "--noise", "counter", "--seed", "9", "--n_steps", str(N)]
    cli.main([str(src), str(tmp_path / "o1"), "--segment-ensemble-files", "1"] + common, model=model)
    cli.main([str(src), str(tmp_path / "o3"), "--segment-ensemble-files", "3"] + common, model=model)
    refs, outs = [], []
    for i in range(3):
        r, _ = A.load(tmp_path / "o1" / f"f{i}.wav")
        y, fs = A.load(tmp_path / "o3" / f"f{i}.wav")
        assert fs == spec.fs and y.shape == r.shape
        refs.append(r.flatten())
        outs.append(y.flatten())
    _check("segments_var_ensemble.cli", refs, outs)
