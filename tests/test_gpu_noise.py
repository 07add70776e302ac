"""GPU (-m gpu): counter-based sampler noise (ou_noise.hip, ou_set_noise_source, noise.CounterNoise).

  1. ou_noise_fill against the fp64 restatement noise.reference: |delta| <= 1e-5 (fp32 logf / log1pf / sqrtf / sincospif are
     within a few ulp on exact arguments and |z| < 5.9), repeatable, row-separable, zero behind a row's length;
  2. the wiring -- bit identity, no tolerance: a counter-mode call equals the tensor-mode call fed with the tensor that
     ou_noise_fill writes for the same seed / streams / draws / positions (ou_enhance, ou_enhance_var, warm start, keep_rms,
     ou_enhance_segments with one window and with several groups);
  3. scheduling independence: an utterance alone, as a row of a ragged batch, on a lane, through enhance_sharded -- the same
     noise bit for bit, outputs under the gates of test_gpu_ragged.py / test_gpu_lanes.py;
  4. segmented vs whole file under the gate of test_gpu_segments.py; the memory of enhance_long; the oracle on the filled noise;
     the C ABI's refusals; the tensor mode's launch count."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import restatement as O
from helpers import record, synth_mix, worst
from open_universe_amd import _lib
from open_universe_amd import noise as N
from open_universe_amd.noise import CounterNoise
from test_gpu_parity import get_model
from test_gpu_segments import GAP_GATE_DB, _si_sdr, _signal

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB


def _fill(model, streams, t0, lens, draw, cols=None, seed=SEED):
    return model.noise_fill(streams, t0, lens, seed, draw, cols)


def _tpad(spec, n):
    return n + (spec.tot_ds - n % spec.tot_ds)


def _noise_tensor(model, spec, ids, lens, n_steps, warm_start=None, seed=SEED):
    """What a counter-mode call of rows `ids` with raw lengths `lens` uses, as the (n, B, 1, T) tensor of the tensor mode:
    draw 0, then draw n + 1 for the absolute steps n = n_start .. N - 2; row b over its own padded length, 0 behind it."""
    n_start = 0 if warm_start is None else warm_start
    T = _tpad(spec, max(lens))
    tp = [_tpad(spec, n) for n in lens]
    draws = [0] + [n + 1 for n in range(n_start, n_steps - 1)]
    return torch.stack([_fill(model, ids, [0] * len(ids), tp, d, cols=T, seed=seed) for d in draws])[:, :, None, :]


def _tensor_mode(model, mix, noise, n_steps, t_raw=None, **kw):
    a = dict(use_aux_signal=False, keep_rms=False, warm_start=None)
    a.update(kw)
    return model._enhance(mix, n_steps, None, None, None, None, a["use_aux_signal"], a["keep_rms"], None, "median",
                          a["warm_start"], noise, t_raw=t_raw)


# ---- 1. the function ---------------------------------------------------------------------------------------------------------
def test_fill_against_the_fp64_reference():
    model, spec, _ = get_model("PP16s")
    cases = [(0, 1 << 20), (1, 1 << 20), (3, (1 << 20) - 5), (2, 777), ((1 << 32) + 7, 1 << 20), ((1 << 32) - 2, 1 << 19),
             ((1 << 40) + 1, 1 << 19), ((1 << 49) + 6, 1 << 18)]
    assert sum(n for _, n in cases) >= (1 << 22) and any(t % 4 for t, _ in cases) and any(t > 1 << 32 for t, _ in cases)
    worst_d, total = 0.0, 0
    for i, (t0, n) in enumerate(cases):
        stream, draw = (i << 16) | (i & 1), i % 5
        z = _fill(model, [stream], [t0], [n], draw)
        assert z.shape == (1, n) and z.dtype == torch.float32
        ref = N.reference(SEED, stream, draw, t0, n)
        d = float(np.abs(z[0].cpu().numpy().astype(np.float64) - ref).max())
        print(f"t0 = {t0}, n = {n}: max |fill - reference| = {d:.3e}")
        worst_d, total = max(worst_d, d), total + n
    print(f"ou_noise_fill vs noise.reference over {total} values: max |delta| = {worst_d:.3e}")
    assert worst_d <= 1e-5


def test_fill_is_repeatable_row_separable_and_zero_behind_the_length():
    model, spec, _ = get_model("PP16s")
    streams = [(4 << 16), (4 << 16) | 1, 9 << 16]
    t0 = [0, 5, (1 << 33) + 2]
    lens = [4000, 3001, 1234]
    cols = 4096
    a = _fill(model, streams, t0, lens, 2, cols)
    b = _fill(model, streams, t0, lens, 2, cols)
    assert torch.equal(a, b)
    for j in range(3):
        one = _fill(model, [streams[j]], [t0[j]], [lens[j]], 2, cols)
        assert torch.equal(one[0], a[j]), j
        assert not a[j, lens[j]:].any() and bool(a[j, :lens[j]].ne(0).all())
    assert not torch.equal(a[0, :3000], a[1, :3000])
    # position indexing on the device: a fill that starts at t0 is the slice of the fill that starts at 0 (odd offsets too)
    whole = _fill(model, [streams[0]], [0], [5000], 2)
    for off in (1, 2, 3, 4, 640, 1001):
        assert torch.equal(_fill(model, [streams[0]], [off], [3000], 2)[0], whole[0, off:off + 3000]), off
    # a row that does not start on a 16-byte boundary takes the scalar stores: the same values
    buf = torch.full((3, cols + 3), 7.0, device="cuda")
    model.noise_fill(streams, t0, lens, SEED, 2, cols, out=buf[:, 1:cols + 1])
    assert torch.equal(buf[:, 1:cols + 1], a) and bool((buf[:, 0] == 7).all()) and bool((buf[:, cols + 1:] == 7).all())
    # a width that is not a multiple of 4, and more rows than one launch carries
    odd = _fill(model, streams, t0, [1001, 1001, 1001], 2, 1001)
    assert torch.equal(odd, torch.stack([_fill(model, [s], [t], [1001], 2, 1001)[0] for s, t in zip(streams, t0)]))
    many = _fill(model, list(range(70)), [3] * 70, [257] * 70, 1, 260)
    assert torch.equal(many[66], _fill(model, [66], [3], [257], 1, 260)[0]) and not many[:, 257:].any()
    # every argument reaches the function
    assert not torch.equal(a, _fill(model, streams, t0, lens, 3, cols))
    assert not torch.equal(a, _fill(model, streams, t0, lens, 2, cols, seed=SEED + 1))
    assert not torch.equal(a, _fill(model, streams, t0, lens, 2, cols, seed=SEED + (1 << 32)))


def test_fill_refuses_bad_arguments():
    model, _, _ = get_model("PP16s")
    L = model._L
    out = torch.empty(2, 64, device="cuda")
    u64, i64 = ctypes.c_uint64 * 2, ctypes.c_int64 * 2
    call = lambda stride, cols, t0, ln, draw: L.ou_noise_fill(  # noqa: E731
        ctypes.c_void_p(out.data_ptr()), stride, cols, 2, u64(1, 2), i64(*t0), i64(*ln), 1, draw, model._stream())
    assert call(64, 64, (0, 0), (64, 10), 0) == _lib.OU_OK
    assert call(64, 64, (0, 0), (65, 10), 0) == _lib.OU_EINVAL   # longer than the row
    assert call(32, 64, (0, 0), (10, 10), 0) == _lib.OU_EINVAL   # stride below the width
    assert call(64, 64, (-1, 0), (10, 10), 0) == _lib.OU_EINVAL
    assert call(64, 64, (1 << 50, 0), (10, 10), 0) == _lib.OU_EINVAL
    assert call(64, 64, (0, 0), (10, 10), 1 << 16) == _lib.OU_EINVAL
    assert call(64, 64, (0, 0), (10, 10), -1) == _lib.OU_EINVAL
    torch.cuda.synchronize()


# ---- 2. the wiring: bit identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_rms", [False, True])
def test_wiring_ou_enhance(keep_rms):
    model, spec, _ = get_model("PP16s")
    B, T_raw, n_steps = 3, spec.tot_ds * 21 + 5, 4
    mix = synth_mix(spec, B, T_raw).cuda()
    src = CounterNoise(SEED, 12)
    got = model.enhance(mix, n_steps=n_steps, rng=src, keep_rms=keep_rms)
    ids = src.stream_ids(B)
    assert ids == [(12 << 16) | c for c in range(B)]
    noise = _noise_tensor(model, spec, ids, [T_raw] * B, n_steps)
    want = _tensor_mode(model, mix[:, None, :], noise, n_steps, keep_rms=keep_rms)[:, 0]
    assert torch.isfinite(got).all() and torch.equal(got, want)
    # ... and the same through the internal form that takes ids
    again = model._enhance(mix, n_steps, None, None, None, None, False, keep_rms, None, "median", None, None,
                           counter=(SEED, ids))
    assert torch.equal(again, got)
    # a wrong row, draw or seed is visible: the check above cannot pass by accident
    swapped = _noise_tensor(model, spec, ids[::-1], [T_raw] * B, n_steps)
    assert not torch.equal(_tensor_mode(model, mix[:, None, :], swapped, n_steps, keep_rms=keep_rms)[:, 0], got)


def test_wiring_warm_start():
    model, spec, _ = get_model("PP16s")
    B, T_raw, n_steps, k = 2, spec.tot_ds * 17 + 3, 5, 2
    mix = synth_mix(spec, B, T_raw).cuda()
    src = CounterNoise(SEED, 3)
    got = model.enhance(mix, n_steps=n_steps, rng=src, warm_start=k)
    noise = _noise_tensor(model, spec, src.stream_ids(B), [T_raw] * B, n_steps, warm_start=k)
    assert noise.shape[0] == n_steps - k  # draws 0, k + 1, .., N - 1
    want = _tensor_mode(model, mix[:, None, :], noise, n_steps, warm_start=k)[:, 0]
    assert torch.equal(got, want)
    # the draws are indexed by the ABSOLUTE step: the tensor of a cold start's first draws is a different call
    cold = _noise_tensor(model, spec, src.stream_ids(B), [T_raw] * B, n_steps)[:n_steps - k]
    assert not torch.equal(_tensor_mode(model, mix[:, None, :], cold, n_steps, warm_start=k)[:, 0], got)


@pytest.mark.parametrize("kw", [{}, {"keep_rms": True}, {"warm_start": 2}])
def test_wiring_ou_enhance_var(kw):
    model, spec, _ = get_model("PP16s")
    td = spec.tot_ds
    lens = [td * 23 + 7, td * 9, td * 14 + td // 2, 57, td * 23 + 7]  # one with T % tot_ds == 0, one below a block
    n_steps = 4
    sigs = [synth_mix(spec, 1, n, seed=1000 + i)[0].cuda() for i, n in enumerate(lens)]
    srcs = [CounterNoise(SEED, 100 + 3 * i) for i in range(len(lens))]
    got = model.enhance_many(sigs, srcs, n_steps=n_steps, **kw)
    ids = [s.stream_ids(1)[0] for s in srcs]
    noise = _noise_tensor(model, spec, ids, lens, n_steps, warm_start=kw.get("warm_start"))
    lm = max(lens)
    mix = torch.stack([torch.nn.functional.pad(s, (0, lm - s.shape[-1])) for s in sigs])[:, None, :]
    want = _tensor_mode(model, mix, noise, n_steps, t_raw=lens, **kw)
    for b, n in enumerate(lens):
        assert torch.equal(got[b], want[b, 0, :n]), b
    # one shared source: entry i is utterance stream + i
    shared = model.enhance_many(sigs, CounterNoise(SEED, 40), n_steps=n_steps, **kw)
    noise = _noise_tensor(model, spec, [(40 + i) << 16 for i in range(len(lens))], lens, n_steps,
                          warm_start=kw.get("warm_start"))
    want = _tensor_mode(model, mix, noise, n_steps, t_raw=lens, **kw)
    for b, n in enumerate(lens):
        assert torch.equal(shared[b], want[b, 0, :n]), b


def test_wiring_multichannel_entries_of_equal_length():
    """Entries of equal length take the plain path; a (C, L) entry's channel c is stream (utterance << 16) | c."""
    model, spec, _ = get_model("PP16s")
    n, n_steps = spec.tot_ds * 11 + 9, 3
    sigs = [synth_mix(spec, 2, n, seed=5).cuda(), synth_mix(spec, 1, n, seed=6)[0].cuda()]
    got = model.enhance_many(sigs, [CounterNoise(SEED, 7), CounterNoise(SEED, 2)], n_steps=n_steps)
    ids = [7 << 16, (7 << 16) | 1, 2 << 16]
    mix = torch.cat([sigs[0], sigs[1][None]])[:, None, :]
    want = _tensor_mode(model, mix, _noise_tensor(model, spec, ids, [n] * 3, n_steps), n_steps)
    assert torch.equal(got[0], want[:2, 0]) and torch.equal(got[1], want[2, 0])


@pytest.mark.parametrize("secs,segment_s,max_batch,windows,groups", [(2.0, 4.0, 8, 1, 1), (6.2, 1.0, 4, 7, 4)])
@pytest.mark.parametrize("keep_rms", [False, True])
def test_wiring_ou_enhance_segments(monkeypatch, secs, segment_s, max_batch, windows, groups, keep_rms):
    model, spec, _ = get_model("PP16s")
    C, T_raw, n_steps = 2, int(secs * spec.fs) + 11, 4
    plan = _lib.segment_plan(spec.tot_ds, T_raw, int(segment_s * spec.fs), int(0.125 * spec.fs))
    assert len(plan["starts"]) == windows and math.ceil(C * windows / max_batch) == groups
    x = torch.stack([_signal(spec.fs, T_raw, 1), _signal(spec.fs, T_raw, 2)])
    src = CounterNoise(SEED, 77)
    kw = dict(segment_s=segment_s, overlap_s=0.125, max_batch=max_batch, n_steps=n_steps, keep_rms=keep_rms)
    got = model.enhance_long(x, rng=src, **kw)
    T = _tpad(spec, T_raw)
    ids = src.stream_ids(C)
    noise = torch.stack([_fill(model, ids, [0, 0], [T, T], d) for d in range(n_steps)])  # (n_steps, C, T_pad), draws 0 .. N - 1
    monkeypatch.setattr(model, "draw_noise_like_enhance", lambda *a, **k: noise)
    want = model.enhance_long(x, rng=None, **kw)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    # the launch count is the tensor mode's: a fill stands where a gather stood
    n_tensor = model.launch_stats()
    model.enhance_long(x, rng=src, **kw)
    assert model.launch_stats() == n_tensor
    if windows == 1:  # ... and one window is the whole-file call
        whole = model.enhance(x, n_steps=n_steps, rng=src, keep_rms=keep_rms)
        assert torch.equal(got, whole) or min(_si_sdr(whole[c], got[c]) for c in range(C)) >= 100.0


def test_ensemble_members_draw_from_streams_of_their_own():
    model, spec, _ = get_model("PP16s")
    T_raw, n_steps = spec.tot_ds * 9 + 1, 3
    x = synth_mix(spec, 1, T_raw)[0].cuda()
    src = CounterNoise(SEED, 5)
    y = model.enhance(x, n_steps=n_steps, rng=src, ensemble=3, ensemble_stat="mean")
    ids = src.stream_ids(1, ensemble=3)
    assert len(set(ids)) == 3
    noise = _noise_tensor(model, spec, ids, [T_raw] * 3, n_steps)
    rows = _tensor_mode(model, x[None, None, :].repeat(3, 1, 1), noise, n_steps)[:, 0]
    assert not torch.equal(rows[0], rows[1]) and not torch.equal(rows[1], rows[2])
    # (the peak guard is applied per member before the reduction in both forms)
    assert torch.equal(y, rows.view(3, 1, 1, -1).mean(dim=0)[0, 0])
    with pytest.raises(ValueError, match="target"):
        model.enhance(x, n_steps=n_steps, rng=src, target=x)


# ---- 3. scheduling independence ----------------------------------------------------------------------------------------------
def _planes(model, B, T):
    """The two planes of the model's noise scratch as the last counter-mode call of (B, T) left them."""
    return model._noise_scratch[:2 * B * T * 4].view(torch.float32).view(2, B, T)


def test_scheduling_independence():
    """Utterance u = 5 of a set of 8: alone, as row 5 of a ragged batch, on lane 2 of 4 and through enhance_sharded -- the
    noise the call really used (read back from the scratch planes) is z(seed, u << 16, draw, t) bit for bit in all four; the
    outputs agree bit for bit where the call is the same call (alone / lane / sharded), >= 100 dB alone vs batched."""
    from open_universe_amd import distributed as D
    from open_universe_amd.lanes import LanePool

    model, spec, _ = get_model("PP16")
    secs = [1.3, 0.9, 1.0, 1.7, 0.6, 1.45, 2.0, 1.1]  # (1.0 s and 2.0 s: T % tot_ds == 0)
    lens = [int(round(s * spec.fs)) for s in secs]
    sigs = [synth_mix(spec, 1, n, seed=1000 + i)[0] for i, n in enumerate(lens)]
    u, n_steps, seed = 5, 3, 1028282
    Tu = _tpad(spec, lens[u])
    # what the last two steps that draw (steps N - 3 and N - 2: draws N - 2 and N - 1) must have used for utterance u
    want = {d & 1: _fill(model, [u << 16], [0], [Tu], d, seed=seed)[0] for d in (n_steps - 2, n_steps - 1)}

    def used(m, B, T, row):
        torch.cuda.synchronize()
        p = _planes(m, B, T)
        return all(torch.equal(p[k, row, :Tu], want[k]) for k in (0, 1))

    alone = model.enhance(sigs[u].cuda(), n_steps=n_steps, rng=CounterNoise(seed, u))
    assert used(model, 1, Tu, 0)
    batch = model.enhance_many([s.cuda() for s in sigs], [CounterNoise(seed, i) for i in range(8)], n_steps=n_steps)
    assert used(model, 8, _tpad(spec, max(lens)), u)
    fig = O.si_sdr(alone.cpu(), batch[u].cpu())
    print(f"utterance {u}: alone vs row {u} of a ragged batch of 8: {float(fig):.1f} dB (snr {fig.snr:.1f})")
    assert float(fig) >= 100.0 and fig.snr >= 100.0
    with LanePool(model, 4) as pool:
        assert pool.lanes == 4
        outs = {}
        for i in (3, 4, 5, 6):  # round robin: utterance 5 lands on lane 2
            lane, o = pool.submit(lambda m, i=i: m.enhance(sigs[i].cuda(), n_steps=n_steps, rng=CounterNoise(seed, i)))
            outs[i] = (lane, o)
        pool.synchronize()
        assert outs[u][0] == 2
        assert used(pool.models[2], 1, Tu, 0)
        on_lane = outs[u][1].clone()
    assert torch.equal(on_lane, alone)
    sharded = D.enhance_sharded(model, sigs, seed=seed, batch_size=1, n_steps=n_steps, noise="counter")
    assert torch.equal(sharded[u].cuda(), alone)
    # batched and in flight: the same rows as the batched call above, whatever lane a group runs on
    sh_b = D.enhance_sharded(model, sigs, seed=seed, batch_size=4, in_flight=2, n_steps=n_steps, noise="counter")
    figs = [O.si_sdr(sharded[i].cpu(), sh_b[i].cpu()) for i in range(8)]
    print(f"enhance_sharded counter mode, batch_size 1 vs 4 x 2 lanes: worst {float(worst(figs)):.1f} dB")
    assert float(worst(figs)) >= 100.0 and worst(figs).snr >= 100.0
    # generator mode is what it was: seed + index
    gen = D.enhance_sharded(model, sigs[:2], seed=seed, n_steps=n_steps)
    assert torch.equal(gen[1].cuda(), model.enhance(sigs[1].cuda(), n_steps=n_steps,
                                                    rng=D.utterance_generator(model.device, seed, 1)))


# ---- 4. segments, memory, oracle, ABI ------------------------------------------------------------------------------------------
def test_segmented_vs_whole_file_in_counter_mode():
    """The setting of test_gpu_segments.py (PP16, 60 s, 8 s windows, 1 s overlap, 4 steps), same gate."""
    model, spec, _ = get_model("PP16")
    x = _signal(spec.fs, 60 * spec.fs, 3)
    src = CounterNoise(SEED, 1)
    whole = model.enhance(x, n_steps=4, rng=src)
    y = model.enhance_long(x, segment_s=8.0, overlap_s=1.0, n_steps=4, rng=src)
    fig = _si_sdr(whole, y)
    print(f"PP16 60 s counter mode: segmented vs whole {fig:.2f} dB (gate {GAP_GATE_DB['PP16']})")
    assert y.shape == x.shape and torch.isfinite(y).all() and fig >= GAP_GATE_DB["PP16"]
    assert torch.equal(y, model.enhance_long(x, segment_s=8.0, overlap_s=1.0, n_steps=4, rng=src))


def test_enhance_long_memory_is_bounded_without_the_noise_tensor():
    """>= 64 windows, 8 steps: peak allocation above the baseline (input and workspace exist) < 4 C T_pad floats in counter
    mode -- the output and slack --; the generator mode holds the (8, C, T_pad) noise beside it, >= 8 C T_pad floats."""
    model, spec, _ = get_model("PP16s")
    C, T_raw, n_steps = 2, 70 * spec.fs + 123, 8
    kw = dict(segment_s=1.0, overlap_s=0.125, max_batch=16, n_steps=n_steps)
    plan = _lib.segment_plan(spec.tot_ds, T_raw, spec.fs, spec.fs // 8)
    assert len(plan["starts"]) >= 64
    unit = C * int(plan["T_pad"]) * 4
    x = torch.stack([_signal(spec.fs, T_raw, 1), _signal(spec.fs, T_raw, 2)])
    src = CounterNoise(SEED, 9)
    y0 = model.enhance_long(x, rng=src, **kw)  # (the workspace exists from here on)
    del y0

    def peak(rng):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = model.enhance_long(x, rng=rng, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(y).all()
        return torch.cuda.max_memory_allocated() - base

    p_counter = peak(src)
    p_generator = peak(torch.Generator(device="cuda").manual_seed(1))
    print(f"enhance_long {len(plan['starts'])} windows x {C} rows, 8 steps: peak above baseline {p_counter / unit:.2f} (counter) "
          f"/ {p_generator / unit:.2f} (generator) x C T_pad floats")
    assert p_counter < 4 * unit
    assert p_generator >= 8 * unit


def test_oracle_on_the_filled_noise():
    """The network did not change; one run of the oracle on the noise the counter mode uses (60 dB gate, helpers.record)."""
    model, spec, sd = get_model("PP16m")
    B, T_raw, n_steps = 2, 4000, 4
    mix = synth_mix(spec, B, T_raw)
    src = CounterNoise(SEED, 31)
    out = model.enhance(mix.cuda(), n_steps=n_steps, rng=src).cpu()
    noise = _noise_tensor(model, spec, src.stream_ids(B), [T_raw] * B, n_steps).cpu()
    ref = O.enhance(sd, spec.to_dict(), mix, n_steps=n_steps, noise=[noise[k] for k in range(n_steps)])
    record("noise.PP16m.counter_mode_vs_oracle", O.si_sdr(ref, out))


def test_c_abi_noise_source():
    model, spec, _ = get_model("PP16s")
    L, h = model._L, model._handle
    B, T_raw, n_steps = 2, spec.tot_ds * 10 + 3, 3
    T = _tpad(spec, T_raw)
    mix = synth_mix(spec, B, T_raw).cuda()
    out = torch.empty(B, T_raw, device="cuda")
    ws = model._workspace(B, T)
    need = ctypes.c_size_t()
    assert L.ou_noise_scratch_bytes(h, B, T, ctypes.byref(need)) == _lib.OU_OK and need.value == 2 * B * T * 4
    assert L.ou_noise_scratch_bytes(h, 0, T, ctypes.byref(need)) == _lib.OU_EINVAL
    scratch = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    dummy = torch.zeros(n_steps, B, T, device="cuda")
    ids = (ctypes.c_uint64 * 3)(11, 12, 13)

    def spec_of(n, buf, nbytes):
        s = _lib.NoiseSpec()
        s.seed, s.streams, s.n_streams = SEED, ids, n
        s.scratch, s.scratch_bytes = (buf.data_ptr() if buf is not None else None), nbytes
        return s

    def enhance(noise):
        return L.ou_enhance(h, ctypes.c_void_p(mix.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                            ctypes.c_void_p(noise.data_ptr()) if noise is not None else None, B, T_raw, n_steps, 1.3, None, -1,
                            0, ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(ws.numel()), model._stream())

    assert json.loads(L.ou_plan_json(h).decode())["noise_source"] == "tensor"
    try:
        assert L.ou_set_noise_source(h, ctypes.byref(spec_of(0, scratch, need.value))) == _lib.OU_EINVAL
        assert L.ou_set_noise_source(h, ctypes.byref(spec_of(2, scratch, 0))) == _lib.OU_EINVAL  # buffer without a size
        assert json.loads(L.ou_plan_json(h).decode())["noise_source"] == "tensor"
        assert L.ou_set_noise_source(h, ctypes.byref(spec_of(2, scratch, need.value))) == _lib.OU_OK
        assert json.loads(L.ou_plan_json(h).decode())["noise_source"] == "counter"
        assert enhance(dummy) == _lib.OU_EINVAL and b"must be NULL" in L.ou_last_error(h)  # never silently ignored
        assert enhance(None) == _lib.OU_OK
        torch.cuda.synchronize()
        n_counter = model.launch_stats()
        first = out.clone()
        noise = torch.stack([model.noise_fill([11, 12], [0, 0], [T, T], SEED, d) for d in range(n_steps)])
        assert L.ou_set_noise_source(h, ctypes.byref(spec_of(3, scratch, need.value))) == _lib.OU_OK
        assert enhance(None) == _lib.OU_EINVAL and b"n_streams" in L.ou_last_error(h)
        assert L.ou_set_noise_source(h, ctypes.byref(spec_of(2, scratch, need.value - 16))) == _lib.OU_OK
        assert enhance(None) == _lib.OU_ENOMEM
        assert L.ou_set_noise_source(h, ctypes.byref(spec_of(2, None, 0))) == _lib.OU_OK  # (enough for ou_enhance_segments)
        assert enhance(None) == _lib.OU_ENOMEM
    finally:
        assert L.ou_set_noise_source(h, None) == _lib.OU_OK
    assert json.loads(L.ou_plan_json(h).decode())["noise_source"] == "tensor"
    assert enhance(None) == _lib.OU_EINVAL and b"noise must be given" in L.ou_last_error(h)
    assert enhance(noise) == _lib.OU_OK
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    # the tensor mode enqueues no fill: the counter mode's count is exactly one fill per draw above it
    n_tensor = model.launch_stats()
    assert n_counter[0] == n_tensor[0] + n_steps and n_counter[1] == n_tensor[1]


def test_cli_noise_counter_end_to_end(tmp_path):
    from open_universe_amd import audio as A
    from open_universe_amd.bin import enhance as cli

    model, spec, _ = get_model("PP16s")
    src = tmp_path / "in"
    src.mkdir()
    lens = [3000, 5100, 2048]
    for i, n in enumerate(lens):
        A.save(src / f"f{i}.wav", (synth_mix(spec, 1, n, seed=50 + i) * 0.5).clamp(-1, 1), spec.fs)
    cli.main([str(src), str(tmp_path / "serial"), "--seed", "9", "--noise", "counter", "--n_steps", "3"], model=model)
    cli.main([str(src), str(tmp_path / "flying"), "--seed", "9", "--noise", "counter", "--n_steps", "3", "--in-flight", "2"],
             model=model)
    cli.main([str(src), str(tmp_path / "batched"), "--seed", "9", "--noise", "counter", "--n_steps", "3", "--batch-size", "2"],
             model=model)
    for k in range(len(lens)):
        x, _ = A.load(src / f"f{k}.wav")
        direct = model.enhance(x.cuda(), n_steps=3, rng=CounterNoise(9, k)).cpu()
        a, _ = A.load(tmp_path / "serial" / f"f{k}.wav")
        b, _ = A.load(tmp_path / "flying" / f"f{k}.wav")
        c, _ = A.load(tmp_path / "batched" / f"f{k}.wav")
        assert torch.equal(a, direct) and torch.equal(b, direct)
        fig = O.si_sdr(direct, c)  # (reduced-width model: the floor of test_gpu_ragged.py's small-model rows)
        assert float(fig) >= 80.0, (k, float(fig))
