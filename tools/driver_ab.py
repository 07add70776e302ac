#!/usr/bin/env python3
"""A/B of the enhance entry points between two builds of the library: same bits, same launches.

Every way into the sampler (ou_enhance, ou_enhance_var, ou_enhance_ensemble, ou_enhance_segments, ou_enhance_segments_var) is
called once on the reduced-width models of the GPU tests, 3 steps, fixed seeds, and one JSON line per call is printed: the
call's name, both counters of ou_launch_stats and the SHA-256 of the output bytes.  Run it once per library and compare the
files byte for byte:

    OU_LIBRARY=/path/to/parent/libouniverse.so timeout -k 10 600 python tools/driver_ab.py --out parent.json
    timeout -k 10 600 python tools/driver_ab.py --out branch.json && cmp parent.json branch.json

One process, all calls in a fixed order; needs a gfx950 device."""
import argparse
import ctypes
import hashlib
import json
import os
import sys
from ctypes import c_float, c_size_t, c_void_p

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import get_spec, synth_mix  # noqa: E402
from open_universe_amd import Universe, UniverseGAN, _lib, state_dict as S  # noqa: E402
from open_universe_amd.noise import CounterNoise  # noqa: E402

N = 3


def build(name):
    """As tests/test_gpu_parity.get_model."""
    spec = get_spec(name)
    sd = S.synthetic_state_dict(spec, seed=0)
    cls = UniverseGAN if spec.kind == "universe_gan" else Universe
    return cls(spec, state_dict=sd, device="cuda:0"), spec


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def digest(out):
    h = hashlib.sha256()
    for t in out if isinstance(out, (list, tuple)) else [out]:
        h.update(t.detach().to(torch.float32).cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def enhance_serial(model, mix, rng):
    """ou_enhance with OU_ENH_SERIAL (the flag has no keyword in Universe.enhance: graphed_enhance sets it)."""
    x = model._prep(mix)[None, None, :]
    L = x.shape[-1]
    T = L + (model.tot_ds - L % model.tot_ds)
    noise = torch.empty((N, 1, 1, T), dtype=torch.float32, device=model.device)
    for k in range(N):
        torch.randn((1, 1, T), generator=rng, out=noise[k])
    sigma = model._sigma_table(N)
    out = torch.empty(1, 1, L, dtype=torch.float32, device=model.device)
    ws = model._workspace(1, T)
    with torch.cuda.device(model.device):
        _lib.check(model._L.ou_enhance(
            model._handle, c_void_p(x.data_ptr()), c_void_p(out.data_ptr()), c_void_p(noise.data_ptr()), 1, L, N,
            float(model.diff_kwargs.epsilon), ctypes.cast(sigma.data_ptr(), ctypes.POINTER(c_float)), -1, _lib.OU_ENH_SERIAL,
            c_void_p(ws.data_ptr()), c_size_t(ws.numel()), model._stream()), model._handle)
    model._status()
    return out


def calls(model, spec):
    """-> (name, thunk) for every call of the comparison."""
    td = spec.tot_ds
    one = synth_mix(spec, 1, 23 * td + 5, seed=1500)[0].cuda()
    two = synth_mix(spec, 2, 19 * td + 11, seed=1600).cuda()
    ragged = [synth_mix(spec, 1, n, seed=1700 + i)[0].cuda() for i, n in enumerate([41 * td + 7, 57, 16 * td])]
    long3 = synth_mix(spec, 3, 70 * td + 3, seed=1800).cuda()
    six = [synth_mix(spec, 1, n, seed=2000 + i)[0].cuda()
           for i, n in enumerate([41 * td + 7, 9 * td, 57, 16 * td - 1, 16 * td, 70 * td + 3])]
    seg = dict(segment_s=16 * td / spec.fs, overlap_s=2 * td / spec.fs, max_batch=4, n_steps=N)

    yield "enhance.b1", lambda: model.enhance(one, n_steps=N, rng=gen(11))
    yield "enhance.b1.serial", lambda: enhance_serial(model, one, gen(11))
    yield "enhance.b1.warm_start", lambda: model.enhance(one, n_steps=N, rng=gen(12), warm_start=1)
    yield "enhance.b2.use_aux_signal", lambda: model.enhance(two, n_steps=N, use_aux_signal=True)
    yield "enhance_many.ragged.tensor", lambda: model.enhance_many(ragged, [gen(20 + i) for i in range(3)], n_steps=N)
    yield "enhance_many.ragged.counter", lambda: model.enhance_many(ragged, CounterNoise(31, 2), n_steps=N)
    for share in (1, 0):
        def with_share(fn, share=share):
            model.set_option("ens_share", share)
            try:
                return fn()
            finally:
                model.set_option("ens_share", 1)
        tag = f"enhance_ensemble.share{share}"
        yield tag + ".plain", lambda w=with_share: w(lambda: model.enhance_ensemble(two, 3, n_steps=N, rng=gen(40)))
        yield tag + ".plain.counter", lambda w=with_share: w(
            lambda: model.enhance_ensemble(two, 3, n_steps=N, rng=CounterNoise(41, 3)))
        yield tag + ".ragged", lambda w=with_share: w(
            lambda: model.enhance_many(ragged, [gen(50 + i) for i in range(3)], n_steps=N, ensemble=3))
    yield "enhance_ensemble.share1.ragged.warm_start", lambda: model.enhance_many(
        ragged, [gen(60 + i) for i in range(3)], n_steps=N, ensemble=3, ensemble_stat="mean", warm_start=1)
    for C in (1, 3):
        yield f"enhance_long.c{C}.tensor", lambda C=C: model.enhance_long(long3[:C], rng=gen(70 + C), **seg)
        yield f"enhance_long.c{C}.counter", lambda C=C: model.enhance_long(long3[:C], rng=CounterNoise(71, C), **seg)
    yield "enhance_long_many.six.tensor", lambda: model.enhance_long_many(six, [gen(80 + i) for i in range(6)], **seg)
    yield "enhance_long_many.six.counter", lambda: model.enhance_long_many(six, [CounterNoise(81, 5 + i) for i in range(6)], **seg)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--models", nargs="+", default=["PP16s", "PP24s"])
    args = ap.parse_args()
    lines = []
    for name in args.models:
        model, spec = build(name)
        for call, thunk in calls(model, spec):
            out = thunk()
            torch.cuda.synchronize()
            launches, convs = model.launch_stats()
            lines.append(json.dumps({"call": f"{name}.{call}", "launches": launches, "convs": convs, "sha256": digest(out)}))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
