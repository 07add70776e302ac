#!/usr/bin/env python3
"""A/B of the enhance entry points between two builds of the library: same bits, same launches.

Every way into the sampler -- the seven entry points ou_enhance, ou_enhance_var, ou_enhance_ensemble, ou_enhance_segments,
ou_enhance_segments_var, ou_enhance_segments_ensemble and ou_enhance_segments_var_ensemble -- is called on the reduced-width
models of the GPU tests, 3 steps, fixed seeds, and one JSON line per call is printed: the call's name, both counters of
ou_launch_stats, the SHA-256 of the
output bytes and `rng`, the SHA-256 of the end states (`get_state()`, concatenated) of the generators handed to the call (empty
for counter sources and calls without a generator).  The Python paths in front of the entry points are covered too: shared
generators, `pad_batch`, the `ensemble=` glue of `enhance`, noise handed over as a list or a tensor, `return_members`.  So the
tool also compares two versions of the Python front end on ONE library (the second use below).  The segmented entry points are
also called on edge shapes:
rows of 1, 2, 3 and 5 samples, of tot_ds + 1, 16 tot_ds + 2 and 33 tot_ds + 3, so that the longest row is 1, 2 and 3 past a
multiple of 4 -- the word-by-word head and tail of the 16-byte row moves and the guards of rows shorter than a quad.  The `opt.*`
calls repeat the batch-1, the ragged and the two-row call with one option off its default each, for the branches of the network
walk that the defaults never take, and one `layout` line per model holds workspace sizes and tensor offsets.  Behind the two
default models come the models of tests/snake_cases.py with Snake and with mixed ConvBlock activations (ou_enhance and a ragged
ou_enhance_var each, one `layout` line with the `.act` planes) and PP16s in every level-normalisation mode of
tests/norm_cases.py (normalization_norm max and 2-max, zero_mean false: ou_enhance and ou_enhance_segments each).  Every call
runs with the per-launch profile on, and its line carries `variants`: the SHA-256 of the variant codes of its profiled launches
(convs, fused bodies, GRU passes) in launch order -- which kernel took which layer, not how long it took.  Behind the calls of
the first model come the `forced` lines: `bench_conv` of one layer of each kind (k1, k3, k5, a down and an up rate-change conv)
at batch 1 and 4, one and five frames of the layer's level, with every code of FORCED as `cfg` -- the status (0, or the
exception a refusal raises) and the variant answered.  Run it once per library and compare the files byte for byte:

    OU_LIBRARY=/path/to/parent/libouniverse.so timeout -k 10 600 python tools/driver_ab.py --out parent.json
    timeout -k 10 600 python tools/driver_ab.py --out branch.json && cmp parent.json branch.json

    # two checkouts, one library:
    OU_LIBRARY=/path/to/libouniverse.so timeout -k 10 600 python <parent checkout>/tools/driver_ab.py --out parent.json

One process, all calls in a fixed order; needs a gfx950 device."""
import argparse
import hashlib
import json
import os
import sys
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import norm_cases  # noqa: E402
import snake_cases  # noqa: E402
from helpers import get_spec, synth_mix  # noqa: E402
from open_universe_amd import Universe, UniverseGAN, _lib, state_dict as S  # noqa: E402
from open_universe_amd.noise import CounterNoise  # noqa: E402
from open_universe_amd.universe import draw_noise  # noqa: E402

N = 3
# forced `cfg` codes of the `forced` lines: the launcher's choice, every LDS config, the first-generation family's requests, and
# one code of each register-direct family
FORCED = [-1] + list(range(8)) + list(range(105, 111)) + [223, 262, 322, 523, 613, 723, 813, 863]


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
    noise = draw_noise(model.tot_ds, [(1, L, rng)], N, device=model.device)
    out = torch.empty(1, 1, L, dtype=torch.float32, device=model.device)
    ws = model._workspace(1, noise.shape[-1])
    model._forward(model._L.ou_enhance, (x, out, noise), (1, L), N, model.diff_kwargs.epsilon, None, _lib.OU_ENH_SERIAL, ws)
    return out


def rng_digest(gens):
    h = hashlib.sha256()
    for g in gens:
        h.update(g.get_state().cpu().numpy().tobytes())
    return h.hexdigest() if gens else ""


def calls(model, spec):
    """-> (name, seeds, fn) for every call of the comparison: fn takes the generators made from `seeds` (none: a counter source,
    or no noise at all)."""
    td = spec.tot_ds
    one = synth_mix(spec, 1, 23 * td + 5, seed=1500)[0].cuda()
    two = synth_mix(spec, 2, 19 * td + 11, seed=1600).cuda()
    ragged = [synth_mix(spec, 1, n, seed=1700 + i)[0].cuda() for i, n in enumerate([41 * td + 7, 57, 16 * td])]
    long3 = synth_mix(spec, 3, 70 * td + 3, seed=1800).cuda()
    six = [synth_mix(spec, 1, n, seed=2000 + i)[0].cuda()
           for i, n in enumerate([41 * td + 7, 9 * td, 57, 16 * td - 1, 16 * td, 70 * td + 3])]
    seg = dict(segment_s=16 * td / spec.fs, overlap_s=2 * td / spec.fs, max_batch=4, n_steps=N)
    three, many6 = [20, 21, 22], [80 + i for i in range(6)]

    yield "enhance.b1", [11], lambda g: model.enhance(one, n_steps=N, rng=g[0])
    yield "enhance.b1.serial", [11], lambda g: enhance_serial(model, one, g[0])
    yield "enhance.b1.warm_start", [12], lambda g: model.enhance(one, n_steps=N, rng=g[0], warm_start=1)
    yield "enhance.b2.use_aux_signal", [], lambda g: model.enhance(two, n_steps=N, use_aux_signal=True)
    yield "enhance_many.ragged.tensor", three, lambda g: model.enhance_many(ragged, g, n_steps=N)
    yield "enhance_many.ragged.counter", [], lambda g: model.enhance_many(ragged, CounterNoise(31, 2), n_steps=N)
    for share in (1, 0):
        def with_share(fn, share=share):
            model.set_option("ens_share", share)
            try:
                return fn()
            finally:
                model.set_option("ens_share", 1)
        tag = f"enhance_ensemble.share{share}"
        yield tag + ".plain", [40], lambda g, w=with_share: w(lambda: model.enhance_ensemble(two, 3, n_steps=N, rng=g[0]))
        yield tag + ".plain.counter", [], lambda g, w=with_share: w(
            lambda: model.enhance_ensemble(two, 3, n_steps=N, rng=CounterNoise(41, 3)))
        yield tag + ".ragged", [50, 51, 52], lambda g, w=with_share: w(
            lambda: model.enhance_many(ragged, g, n_steps=N, ensemble=3))
    yield "enhance_ensemble.share1.ragged.warm_start", [60, 61, 62], lambda g: model.enhance_many(
        ragged, g, n_steps=N, ensemble=3, ensemble_stat="mean", warm_start=1)
    for C in (1, 3):
        yield f"enhance_long.c{C}.tensor", [70 + C], lambda g, C=C: model.enhance_long(long3[:C], rng=g[0], **seg)
        yield f"enhance_long.c{C}.counter", [], lambda g, C=C: model.enhance_long(long3[:C], rng=CounterNoise(71, C), **seg)
    yield "enhance_long_many.six.tensor", many6, lambda g: model.enhance_long_many(six, g, **seg)
    yield "enhance_long_many.six.counter", [], lambda g: model.enhance_long_many(six, [CounterNoise(81, 5 + i) for i in range(6)], **seg)

    ens = dict(seg, max_batch=12)
    two_long = long3[:2]

    def long_ensemble(share, mix, rng, stat, **kw):
        model.set_option("ens_share", share)
        try:
            return model.enhance_long_ensemble(mix, 3, ensemble_stat=stat, rng=rng, return_members=True, **ens, **kw)
        finally:
            model.set_option("ens_share", 1)
    yield "enhance_long_ensemble.share1.tensor.median", [90], lambda g: long_ensemble(1, two_long, g[0], "median")
    yield "enhance_long_ensemble.share0.tensor.median", [90], lambda g: long_ensemble(0, two_long, g[0], "median")
    yield "enhance_long_ensemble.share1.counter.mean", [], lambda g: long_ensemble(1, two_long, CounterNoise(91, 4), "mean")

    # rows with lengths of their own (groups of 12 // 3 = 4 entries: the windows of the two long rows, then the short rows as
    # ragged groups); results and members in one digest
    def long_many_ensemble(share, rngs):
        model.set_option("ens_share", share)
        try:
            res, mems = model.enhance_long_many_ensemble(six, 3, rngs=rngs, return_members=True, **ens)
            return list(res) + list(mems)
        finally:
            model.set_option("ens_share", 1)
    for share in (1, 0):
        yield f"enhance_long_many_ensemble.share{share}.tensor", many6, lambda g, share=share: long_many_ensemble(share, g)
        yield f"enhance_long_many_ensemble.share{share}.counter", [], lambda g, share=share: long_many_ensemble(
            share, [CounterNoise(95, 5 + i) for i in range(6)])

    # edge shapes (keep_rms: the post scale moves every row)
    edge = [1, 2, 3, 5, td + 1, 16 * td + 2, 33 * td + 3]
    for T in edge:
        mix = synth_mix(spec, 2, T, seed=2100).cuda()
        yield f"edge.enhance_long.t{T}", [100], lambda g, mix=mix: model.enhance_long(mix, rng=g[0], keep_rms=True, **seg)
        yield f"edge.enhance_long_ensemble.t{T}", [101], lambda g, mix=mix: long_ensemble(1, mix, g[0], "median", keep_rms=True)
    for n in (5, 6, 7):  # the longest row: tot_ds + 1, 16 tot_ds + 2, 33 tot_ds + 3
        rows = [synth_mix(spec, 1, T, seed=2200 + i)[0].cuda() for i, T in enumerate(edge[:n])]
        yield f"edge.enhance_long_many.max{edge[n - 1]}.tensor", [110 + i for i in range(n)], lambda g, rows=rows: (
            model.enhance_long_many(rows, g, keep_rms=True, **seg))
    yield "edge.enhance_long_many.counter", [], lambda g, rows=rows: model.enhance_long_many(
        rows, [CounterNoise(111, 9 + i) for i in range(len(rows))], keep_rms=True, **seg)

    # the Python paths in front of the entry points that the calls above do not reach
    yield "py.enhance_many.pad_batch.shared", [120], lambda g: model.enhance_many(ragged, g[0], pad_batch=True, n_steps=N)
    yield "py.enhance_many.ragged.shared", [121], lambda g: model.enhance_many(ragged, g[0], n_steps=N)
    for stat in ("mean", "median", "signal_median"):
        yield f"py.enhance.ensemble3.{stat}", [122], lambda g, stat=stat: model.enhance(
            two, n_steps=N, rng=g[0], ensemble=3, ensemble_stat=stat)
    T2 = two.shape[-1] + (td - two.shape[-1] % td)
    z = torch.randn((N, 2, 1, T2), generator=torch.Generator().manual_seed(123)).cuda()
    for tag, noise in (("list", list(z)), ("tensor", z)):
        yield f"py.enhance.noise_{tag}", [], lambda g, noise=noise: model._enhance(
            two, N, None, None, None, None, False, False, None, "median", None, noise)
    for tag, mix in (("t", one), ("bt", two)):
        yield f"py.enhance_ensemble.members.{tag}", [124], lambda g, mix=mix: model.enhance_ensemble(
            mix, 3, n_steps=N, rng=g[0], return_members=True)
    yield "py.enhance_long_many.shared", [125], lambda g: model.enhance_long_many(six, g[0], **seg)

    # the branches of the network walk (Runner::conv / block in ou_walk.cpp) that the default options never take: one option off
    # its default per call, reset afterwards
    def with_option(key, value, fn):
        default = model.get_option(key)
        model.set_option(key, value)
        try:
            return fn()
        finally:
            model.set_option(key, default)
    walk = [("rate_small", 0), ("fuse_upfir", 0), ("preact", 0)] + [("fuse", v) for v in (0, 2, 3)]
    walk += [("conv_direct", v) for v in range(5)] + [("wino", 0), ("split", 1), ("no_overlap", 1)]
    for key, value in walk:
        yield f"opt.{key}{value}.enhance.b1", [11], lambda g, k=key, v=value: with_option(
            k, v, lambda: model.enhance(one, n_steps=N, rng=g[0]))
        yield f"opt.{key}{value}.enhance_many.ragged.tensor", three, lambda g, k=key, v=value: with_option(
            k, v, lambda: model.enhance_many(ragged, g, n_steps=N))
    yield "opt.mask_fused0.enhance_many.ragged.tensor", three, lambda g: with_option(
        "mask_fused", 0, lambda: model.enhance_many(ragged, g, n_steps=N))
    # (rows 0 .. 3 of `six`: the windows of the long row, then the three short rows as one group of different lengths)
    yield "opt.mask_fused0.enhance_long_many.ragged_group", many6[:4], lambda g: with_option(
        "mask_fused", 0, lambda: model.enhance_long_many(six[:4], g, **seg))
    yield "opt.gru_bmax1.enhance.b2", [130], lambda g: with_option("gru_bmax", 1, lambda: model.enhance(two, n_steps=N, rng=g[0]))


WALK_TENSORS = ("mixn", "x", "cond.aux", "cond.latent", "cond.enc0.c1", "score.dec0.v", "score.gru")


def forced_lines(model, spec, name):
    """One line per (layer, B, frames, forced code): what a forced request reaches on a layer of each kind."""
    plan = json.loads(model._L.ou_plan_json(model._handle).decode())
    layers = {}
    for L in plan["convs"]:
        kind = ("down" if L["stride"] > 1 else "up" if L["up"] > 1 else "k%d" % L["KW"])
        if kind in ("k1", "k3", "k5", "down", "up") and (kind != "up" or L.get("fir_mode") == 2):
            layers.setdefault(kind, L)
    for kind in ("k1", "k3", "k5", "down", "up"):
        L = layers[kind]
        for B in (1, 4):
            for frames in (1, 5):
                Tin = frames * max(L["stride"], 1)
                for cfg in FORCED:
                    try:
                        _, used = model.bench_conv(L["name"], B, Tin, cfg=cfg, iters=1)
                        status = 0
                    except Exception as e:  # a refusal is a recorded answer
                        status, used = type(e).__name__, -1
                    torch.cuda.synchronize()
                    yield json.dumps({"call": f"{name}.forced.{kind}.b{B}.f{frames}.cfg{cfg}", "layer": L["name"], "status": status,
                                      "variant": used})


def layout(model, spec, names=WALK_TENSORS):
    """The workspace layout of a model as one record: ou_workspace_bytes at three shapes, and where `Universe.tensor` finds
    the tensors `names` of the walk after `enhance.b1` -- (byte offset into the workspace, C, T) each."""
    td = spec.tot_ds
    model.enhance(synth_mix(spec, 1, 23 * td + 5, seed=1500)[0].cuda(), n_steps=N, rng=gen(11))
    torch.cuda.synchronize()
    where = {}
    for name in names:
        t = model.tensor(name)
        where[name] = [t.data_ptr() - model._ws.data_ptr(), t.shape[1], t.shape[2]]
    return {"workspace_bytes": [model._workspace_bytes(B, n * td) for B, n in ((1, 23), (2, 19), (3, 41))], "tensors": where}


def build_case(cases, *key):
    """A model of tests/snake_cases.py or tests/norm_cases.py: the case's spec on the case's seeded weights."""
    spec = cases.spec_of(*key)
    cls = UniverseGAN if spec.kind == "universe_gan" else Universe
    return cls(spec, state_dict=cases.state_dict_of(*key), device="cuda:0"), spec


def snake_calls(model, spec):
    """Networks with Snake (and with mixed) ConvBlock activations: the batch-1 call and one ragged batch."""
    td = spec.tot_ds
    one = synth_mix(spec, 1, 23 * td + 5, seed=1500)[0].cuda()
    ragged = [synth_mix(spec, 1, n, seed=1700 + i)[0].cuda() for i, n in enumerate([41 * td + 7, 57, 16 * td])]
    yield "enhance.b1", [11], lambda g: model.enhance(one, n_steps=N, rng=g[0])
    yield "enhance_many.ragged.tensor", [20, 21, 22], lambda g: model.enhance_many(ragged, g, n_steps=N)


def norm_calls(model, spec):
    """The level normalisation modes: the cases' own batch (a smooth row and one with a spike, both on a DC offset) through
    `enhance`, and two such rows of 70 tot_ds + 3 samples through `enhance_long`."""
    td = spec.tot_ds
    mix = norm_cases.batch_mix(spec).cuda()
    long2 = synth_mix(spec, 2, 70 * td + 3, seed=1800) + norm_cases.DC
    long2[1] = norm_cases.with_spike(long2[1], 31 * td)
    long2 = long2.cuda()
    seg = dict(segment_s=16 * td / spec.fs, overlap_s=2 * td / spec.fs, max_batch=4, n_steps=N)
    yield "enhance.b2", [140], lambda g: model.enhance(mix, n_steps=N, rng=g[0])
    yield "enhance_long.c2.tensor", [141], lambda g: model.enhance_long(long2, rng=g[0], **seg)


def suites(models):
    """-> (name, build, calls, tensors of the layout line or None) for every model of the comparison"""
    for name in models:
        yield name, lambda name=name: build(name), calls, WALK_TENSORS
    # Snake activations: a plane of activated inputs per block (`.act`) in the workspace
    yield "snake.snake", lambda: build_case(snake_cases, "snake"), snake_calls, ("x", "score.enc0.act", "score.dec0.act", "score.gru")
    yield "snake.mixed", lambda: build_case(snake_cases, "mixed"), snake_calls, None
    for mode in norm_cases.MODES:  # max, 2max, keepmean (norm 2, zero_mean false)
        yield f"norm.PP16s.{mode}", lambda mode=mode: build_case(norm_cases, "PP16s", mode), norm_calls, None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--models", nargs="+", default=["PP16s", "PP24s"])
    args = ap.parse_args()
    lines = []
    for name, make, calls_of, tensors in suites(args.models):
        model, spec = make()
        for call, seeds, fn in calls_of(model, spec):
            gens = [gen(s) for s in seeds]
            model.profile(True)
            out = fn(gens)
            torch.cuda.synchronize()
            launches, convs = model.launch_stats()
            codes = [r[3] for r in model.profile_read(max_records=32768)]
            model.profile(False)
            variants = hashlib.sha256(",".join(map(str, codes)).encode()).hexdigest()
            lines.append(json.dumps({"call": f"{name}.{call}", "launches": launches, "convs": convs, "sha256": digest(out),
                                     "rng": rng_digest(gens), "variants": variants, "profiled": len(codes)}))
            print(lines[-1], flush=True)
        if name == args.models[0]:
            for line in forced_lines(model, spec, name):
                lines.append(line)
                print(line, flush=True)
        if tensors:
            lines.append(json.dumps({"call": f"{name}.layout", **layout(model, spec, tensors)}))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
