"""GPU (-m gpu): ensembles inside the library -- ou_ensemble_reduce, ou_enhance_ensemble (Universe.enhance_ensemble,
enhance_many(ensemble=E)).

Yardsticks: the torch restatement of the reduce (tests/ensemble_ref.py, itself held against torch.median / signal_median / the
sort-based statement in test_ensemble_cpu.py); `enhance(ensemble=E)` -- the call on the replicated batch with the host-side
reduce -- for the plumbing (option ens_share = 0: same arithmetic, bit for bit); and for the shared conditioner (the default)
the project's gate where only the kernel selection differs: >= 100 dB SI-SDR per member (cf. exact batching in
test_gpu_ragged.py).  The measured minimum of every case is written to profiles/ensemble_observed.json."""
import ctypes
import json
import os
from ctypes import c_size_t, c_void_p

import pytest
import torch

import ensemble_ref as R
import restatement as O
from helpers import synth_mix
from open_universe_amd import _lib
from open_universe_amd.noise import CounterNoise
from open_universe_amd.universe import ensemble_reduce
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

E_LIST = [1, 2, 3, 4, 5, 8, 31, 32]
GATE_DB = 100.0
_OBSERVED = {}


def _observe(case, db):
    _OBSERVED[case] = round(float(db), 2)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "ensemble_observed.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(_OBSERVED)
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def _gen(seed):
    return torch.Generator(device="cuda:0").manual_seed(seed)


class _share:
    """`with _share(model, 0):` -- ens_share for the calls inside, back to the default behind them."""

    def __init__(self, model, v):
        self.model, self.v = model, v

    def __enter__(self):
        self.model.set_option("ens_share", self.v)

    def __exit__(self, *a):
        self.model.set_option("ens_share", 1)


# ---- 1. the reduce alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", E_LIST)
def test_reduce_kernels_against_the_restatement(E):
    for B in (1, 3):
        for cols in (1, 3, 64, 4097, 64161):
            for ties in (False, True):
                x = R.draw_members(E, B, cols, seed=E * 1000 + B * 10 + cols % 7 + ties, ties=ties)
                lens = [cols, max(1, cols // 2), 1][:B] if (cols + ties) % 2 else None
                if B == 1 and lens is not None:
                    lens = [max(1, cols - 2)]
                refs = {stat: R.reduce_ref(x, stat, lens) for stat in R.STATS if stat != "mean"}
                xv = x.clone()
                if lens is not None:
                    for b in range(B):
                        xv[:, b, lens[b]:] = 0
                m64 = xv.double().mean(dim=0)
                bound = R.mean_bound(xv, m64)
                for rs in (cols + 3, (cols + 8) // 4 * 4):  # rows off / on 16-byte boundaries: scalar and 16-byte accesses
                    buf = torch.full((E * B, rs), 9.0)
                    buf[:, :cols] = x.reshape(E * B, cols)
                    buf = buf.cuda()
                    mem = buf.view(E, B, rs)[:, :, :cols]
                    for stat in R.STATS:
                        outs = []
                        for rep in range(2):
                            full = torch.full((B, rs), 7.0, device="cuda:0")
                            out, pick = ensemble_reduce(mem, stat, lens, return_pick=True, out=full[:, :cols])
                            outs.append(out.cpu())
                            assert (full[:, cols:] == 7.0).all()  # nothing behind `cols` is touched
                        what = (E, B, cols, ties, rs, stat)
                        assert torch.equal(outs[0], outs[1]), what  # two runs: identical bits
                        got = outs[0]
                        for b in range(B):
                            n = cols if lens is None else lens[b]
                            assert not got[b, n:].any(), what  # zero from len[b] on
                        if stat == "mean":
                            assert ((got.double() - m64).abs() <= bound).all(), what
                        else:
                            assert torch.equal(got, refs[stat][0]), what  # bit-exact
                        if stat == "signal_median":
                            assert torch.equal(pick.cpu(), refs[stat][1]), what


# ---- 2. E = 1 is the plain call ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat", R.STATS)
def test_one_member_is_the_plain_call_bit_for_bit(stat):
    model, spec, sd = get_model("PP16m")
    td = spec.tot_ds
    mix = synth_mix(spec, 2, td * 11 + 5).cuda()
    # equal lengths: enhance, tensor noise from a generator and counter noise
    a = model.enhance(mix, n_steps=3, rng=_gen(11))
    b = model.enhance_ensemble(mix, 1, stat, n_steps=3, rng=_gen(11))
    assert torch.equal(a, b)
    a = model.enhance(mix, n_steps=3, rng=CounterNoise(5, 2))
    b, mem = model.enhance_ensemble(mix, 1, stat, n_steps=3, rng=CounterNoise(5, 2), return_members=True)
    assert torch.equal(a, b) and torch.equal(mem[0], b)
    # ragged: enhance_many
    sigs = [synth_mix(spec, 1, L, seed=50 + i)[0].cuda() for i, L in enumerate((td * 9 + 3, td * 4, td * 6 + 100))]
    a = model.enhance_many(sigs, _gen(3), n_steps=3)
    b = model.enhance_many(sigs, _gen(3), n_steps=3, ensemble=1, ensemble_stat=stat)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    a = model.enhance_many(sigs, CounterNoise(9, 4), n_steps=3)
    b = model.enhance_many(sigs, CounterNoise(9, 4), n_steps=3, ensemble=1, ensemble_stat=stat)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


# ---- 3. plumbing: ens_share = 0 is enhance(ensemble=E) ------------------------------------------------------------------------
def _members_by_enhance(model, mix, E, rng, **kw):
    """What enhance(ensemble=E) computes before its reduce: the plain call on the replicated batch, same draws."""
    rep = torch.stack([mix[:, None, :]] * E, dim=0).view(-1, 1, mix.shape[-1])
    y = model._enhance(rep, kw.get("n_steps", 3), None, None, None, None if isinstance(rng, CounterNoise) else rng, False,
                       kw.get("keep_rms", False), None, "median", kw.get("warm_start"), None,
                       counter=(rng.seed, rng.stream_ids(mix.shape[0], E)) if isinstance(rng, CounterNoise) else None)
    return y.view(E, mix.shape[0], mix.shape[-1])


def _check_reduced(out, ref, members, stat):
    if stat == "mean":
        m64 = members.double().mean(dim=0)
        assert ((out.double() - m64).abs() <= R.mean_bound(members, m64)).all()
    else:
        assert torch.equal(out, ref)


@pytest.mark.parametrize("E,B,kw", [(2, 1, {}), (3, 2, {}), (4, 1, dict(keep_rms=True)), (3, 2, dict(warm_start=1)),
                                    (4, 2, {}), (2, 1, dict(warm_start=1, keep_rms=True))])
@pytest.mark.parametrize("source", ["generator", "counter"])
def test_unshared_path_is_enhance_on_the_replicated_batch(E, B, kw, source):
    model, spec, sd = get_model("PP16m")
    mix = synth_mix(spec, B, spec.tot_ds * 10 + 77).cuda()
    rng = (lambda: _gen(21)) if source == "generator" else (lambda: CounterNoise(33, 7))
    want = _members_by_enhance(model, mix, E, rng(), n_steps=3, **kw)
    with _share(model, 0):
        for stat in R.STATS:
            out, mem = model.enhance_ensemble(mix, E, stat, n_steps=3, rng=rng(), return_members=True, **kw)
            assert torch.equal(mem, want), (stat, "members")
            ref = model.enhance(mix, n_steps=3, rng=rng(), ensemble=E, ensemble_stat=stat, **kw)
            _check_reduced(out.cpu(), ref.cpu(), mem.cpu(), stat)


# ---- 4. the shared conditioner (default) ---------------------------------------------------------------------------------------
def _check_shared_against_unshared(case, out_s, mem_s, out_u, mem_u, stat):
    """members >= 100 dB; mean / median 1-Lipschitz in the members; signal median = the restatement on the call's own members."""
    E = mem_s.shape[0]
    ms, mu = mem_s.cpu().reshape(E, -1, mem_s.shape[-1]), mem_u.cpu().reshape(E, -1, mem_u.shape[-1])
    os_, ou = out_s.cpu().reshape(-1, out_s.shape[-1]), out_u.cpu().reshape(-1, out_u.shape[-1])
    worst = min(float(O.si_sdr(mu[e, b], ms[e, b])) for e in range(E) for b in range(ms.shape[1]))
    _observe(case, worst)
    assert worst >= GATE_DB, (case, worst)
    if stat == "signal_median":
        ref, _, _ = R.reduce_ref(ms, stat)
        assert torch.equal(os_, ref)
        return worst
    dev = (ms.double() - mu.double()).abs().max(dim=0).values
    slack = 0.0
    if stat == "mean":  # both sides carry the rounding of their own sequential sum
        slack = R.mean_bound(ms, ms.double().mean(dim=0)) + R.mean_bound(mu, mu.double().mean(dim=0))
    assert ((os_.double() - ou.double()).abs() <= dev + slack).all(), case
    return worst


@pytest.mark.parametrize("E,B,kw", [(2, 1, {}), (4, 1, {}), (3, 2, {}), (8, 1, dict(keep_rms=True)), (3, 2, dict(warm_start=1))])
def test_shared_conditioner_replicates_and_stays_within_round_off(E, B, kw):
    model, spec, sd = get_model("PP16m")
    mix = synth_mix(spec, B, spec.tot_ds * 12 + 9).cuda()
    for stat in R.STATS:
        with _share(model, 0):
            out_u, mem_u = model.enhance_ensemble(mix, E, stat, n_steps=3, rng=CounterNoise(71, 3), return_members=True, **kw)
        out_s, mem_s = model.enhance_ensemble(mix, E, stat, n_steps=3, rng=CounterNoise(71, 3), return_members=True, **kw)
        # every tensor the score passes / the post step read per row: rows e B + b are row b
        names = ["cond.aux", "cond.latent", "mixn", "mel_scale"] + (["wav"] if "warm_start" in kw else [])
        j = 0
        while True:
            try:
                model.tensor(f"cond.c{j}")
            except KeyError:
                break
            names += [f"cond.c{j}", f"cond.sc{j}"]
            j += 1
        assert j >= 1
        for nm in names:
            t = model.tensor(nm)
            assert t.shape[0] == E * B
            t = t.view(E, B, -1)
            assert torch.equal(t, t[:1].expand_as(t)), nm
        tag = "".join(f".{k}" for k in kw)
        _check_shared_against_unshared(f"shared.PP16m.E{E}.B{B}{tag}.{stat}", out_s, mem_s, out_u, mem_u, stat)


# ---- 5. ragged ensembles --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat", R.STATS)
def test_ragged_ensembles_against_every_file_alone(stat):
    model, spec, sd = get_model("PP16m")
    td, E = spec.tot_ds, 3
    sigs = [synth_mix(spec, 1, td * 10 + 3, seed=60)[0].cuda(), synth_mix(spec, 2, td * 5 + 40, seed=61).cuda(),
            synth_mix(spec, 1, td * 7, seed=62)[0].cuda()]
    src = CounterNoise(17, 20)
    outs, mems = model.enhance_many(sigs, rngs=src, n_steps=3, ensemble=E, ensemble_stat=stat, return_members=True)
    for i, s in enumerate(sigs):
        assert outs[i].shape == s.shape and mems[i].shape == (E,) + tuple(s.shape)
        o1, m1 = model.enhance_ensemble(s, E, stat, n_steps=3, rng=src.at(i), return_members=True)
        assert o1.shape == s.shape
        _check_shared_against_unshared(f"ragged.PP16m.file{i}.{stat}", outs[i], mems[i], o1, m1, stat)
    # generators: entry i gets the draws enhance(entry_i, ensemble=E) makes alone, in serial-loop order
    g = _gen(5)
    alone = [model.enhance_ensemble(s, E, "median", n_steps=3, rng=g, return_members=True)[1] for s in sigs]
    _, mems = model.enhance_many(sigs, rngs=_gen(5), n_steps=3, ensemble=E, ensemble_stat="median", return_members=True)
    for i in range(len(sigs)):
        a, b = alone[i].cpu().reshape(-1, sigs[i].shape[-1]), mems[i].cpu().reshape(-1, sigs[i].shape[-1])
        worst = min(float(O.si_sdr(a[r], b[r])) for r in range(a.shape[0]))
        _observe(f"ragged_generator.PP16m.file{i}", worst)
        assert worst >= GATE_DB
    with pytest.raises(ValueError):
        model.enhance_many(sigs, rngs=src, n_steps=3, ensemble=E, pad_batch=True)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    model, spec, sd = get_model("PP16m")
    L, h = model._L, model._handle
    B, Traw = 2, spec.tot_ds * 6 + 1
    T = Traw + (spec.tot_ds - Traw % spec.tot_ds)
    mix = synth_mix(spec, B, Traw).cuda()
    model.enhance_ensemble(mix, 2, n_steps=3, rng=_gen(1))  # a good call first: leaves a prepared (2 B)-row workspace
    ws = model._ws
    small = model._private_workspace(B, T)  # prepared for B rows, not E * B (its init is the last thing enqueued here)
    torch.cuda.synchronize()
    stats0, word0 = model.launch_stats(), int(ws[:4].view(torch.int32).item())
    out = torch.empty(B, Traw, device="cuda:0")
    noise = torch.zeros(3, 2 * B, T, device="cuda:0")
    sig = (ctypes.c_float * 3)(1.0, 0.5, 0.1)

    def call(E=2, stat=1, flags=0, noise_p=noise, ws_t=ws):
        return L.ou_enhance_ensemble(h, c_void_p(mix.data_ptr()), c_void_p(out.data_ptr()), None,
                                     c_void_p(noise_p.data_ptr()) if noise_p is not None else None, B, Traw, None, E, stat, 3,
                                     1.3, sig, -1, flags, c_void_p(ws_t.data_ptr()), c_size_t(ws_t.numel()), model._stream())

    assert call(E=0) == _lib.OU_EINVAL and call(E=33) == _lib.OU_EINVAL
    assert call(stat=3) == _lib.OU_EINVAL and call(stat=-1) == _lib.OU_EINVAL
    assert call(flags=_lib.OU_ENH_USE_AUX_SIGNAL) == _lib.OU_EINVAL
    assert call(noise_p=None) == _lib.OU_EINVAL  # tensor mode without a tensor
    assert call(ws_t=small) == _lib.OU_EINVAL
    with model._counter_source(3, CounterNoise(3, 0).stream_ids(B), 2 * B, T):  # n_streams = B != E * B
        assert call(noise_p=None) == _lib.OU_EINVAL
    with model._counter_source(3, CounterNoise(3, 0).stream_ids(B, 2), 2 * B, T):
        assert call() == _lib.OU_EINVAL  # a noise pointer while a source is set
    n = c_size_t()
    assert L.ou_ensemble_workspace_bytes(h, B, T, 0, ctypes.byref(n)) == _lib.OU_EINVAL
    assert L.ou_ensemble_workspace_bytes(h, B, T, 33, ctypes.byref(n)) == _lib.OU_EINVAL
    torch.cuda.synchronize()
    assert model.launch_stats() == stats0 and int(ws[:4].view(torch.int32).item()) == word0
    mem = torch.zeros(2, 1, 8, device="cuda:0")
    for bad in (dict(E=0), dict(E=33), dict(stat=5)):
        a = dict(E=2, stat=1)
        a.update(bad)
        assert L.ou_ensemble_reduce(c_void_p(mem.data_ptr()), c_void_p(out.data_ptr()), a["E"], 1, 8, 8, None, a["stat"], None, 0,
                                    model._stream()) == _lib.OU_EINVAL
    assert call() == _lib.OU_OK  # and the same arguments without a fault are taken
    model._status(force=True)


# ---- 7. existing paths are untouched -----------------------------------------------------------------------------------------------
def test_plain_enhance_after_an_ensemble_call_is_unchanged():
    from open_universe_amd import UniverseGAN

    model, spec, sd = get_model("PP16m")
    fresh = UniverseGAN(spec, state_dict=sd, device="cuda:0")
    mix = synth_mix(spec, 1, spec.tot_ds * 16 + 11).cuda()
    want = fresh.enhance(mix, n_steps=4, rng=_gen(2))
    want_stats = fresh.launch_stats()
    model.enhance_ensemble(mix, 4, "signal_median", n_steps=4, rng=_gen(8))
    model.enhance_ensemble(mix, 1, "mean", n_steps=4, rng=_gen(8))  # (the same batch size as the plain call: shares its workspace)
    got = model.enhance(mix, n_steps=4, rng=_gen(2))
    assert model.launch_stats() == want_stats
    assert torch.equal(got, want)
    assert model.options() == _lib.option_defaults()
