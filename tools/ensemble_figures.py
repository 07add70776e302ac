"""Figures of the ensemble call: `enhance(ensemble=E)` -- replicated batch, conditioner over E * B rows, host-side
reduce -- against `enhance_ensemble` (ou_enhance_ensemble) with ens_share 0 and 1, in ONE process on one box; and a ragged
directory: the serial `enhance(ensemble=4)` loop against `enhance_many(ensemble=4)` in groups.  The variants alternate inside
every repeat; one JSON line per figure (median and spread of the repeats, milliseconds per call).

  python tools/ensemble_figures.py single --config PP16 --seconds 4 --ensembles 2,4,8,16
  python tools/ensemble_figures.py dir    --config PP16 --files 32 --ensemble 4 --group-rows 8
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402

import open_universe_amd  # noqa: E402,F401
from open_universe_amd import Universe, state_dict as S  # noqa: E402
from open_universe_amd.noise import CounterNoise  # noqa: E402
from helpers import get_spec  # noqa: E402


def signal(fs, T, seed=0, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    t = torch.arange(T, device=device, dtype=torch.float64) / fs
    x = 0.1 * torch.sin(2 * math.pi * (150.0 + 35.0 * (seed % 9)) * t) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3 * t))
    return x.float() + 0.03 * torch.randn(T, device=device, generator=g)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(variants, warmup, repeats):
    """variants: {name: fn}.  Every repeat runs all of them once, in turn -> {name: (median ms, min, max)}."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(timed(fn))
    return {k: (round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["single", "dir"])
    ap.add_argument("--config", default="PP16")
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--ensembles", default="2,4,8,16")
    ap.add_argument("--stats", default="median,signal_median")
    ap.add_argument("--n-steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--ensemble", type=int, default=4)
    ap.add_argument("--group-rows", type=int, default=8)
    a = ap.parse_args()
    spec = get_spec(a.config)
    model = Universe(spec, state_dict=S.synthetic_state_dict(spec, seed=0), device="cuda:0")
    src = CounterNoise(5, 0)  # (no noise tensor on either side: the draws are not part of what is compared)

    def ens(x, E, stat, share):
        model.set_option("ens_share", share)
        try:
            return model.enhance_ensemble(x, E, stat, n_steps=a.n_steps, rng=src)
        finally:
            model.set_option("ens_share", 1)

    if a.what == "single":
        x = signal(spec.fs, int(round(a.seconds * spec.fs)))
        for E in [int(v) for v in a.ensembles.split(",")]:
            for stat in a.stats.split(","):
                res = alternate({
                    "enhance": lambda: model.enhance(x, n_steps=a.n_steps, rng=src, ensemble=E, ensemble_stat=stat),
                    "ensemble_share0": lambda: ens(x, E, stat, 0),
                    "ensemble_share1": lambda: ens(x, E, stat, 1),
                }, a.warmup, a.repeats)
                base = res["enhance"][0]
                print(json.dumps({"what": "single", "config": a.config, "seconds": a.seconds, "B": 1, "E": E, "stat": stat,
                                  "ms_median_min_max": res,
                                  "share0_vs_enhance": round(res["ensemble_share0"][0] / base, 4),
                                  "share1_vs_enhance": round(res["ensemble_share1"][0] / base, 4)}), flush=True)
        return
    # a ragged directory: lengths 1 .. 8 s from a seeded draw
    u = torch.rand(a.files, generator=torch.Generator().manual_seed(5))
    files = [signal(spec.fs, int(spec.fs * (1.0 + 7.0 * float(v))), seed=i) for i, v in enumerate(u)]
    E, per = a.ensemble, max(1, a.group_rows // a.ensemble)
    order = sorted(range(len(files)), key=lambda i: -files[i].shape[-1])

    def serial():
        for i, f in enumerate(files):
            model.enhance(f, n_steps=a.n_steps, rng=src.at(i), ensemble=E, ensemble_stat="median")

    def batched():
        for g0 in range(0, len(order), per):
            grp = order[g0:g0 + per]
            model.enhance_many([files[i] for i in grp], [src.at(i) for i in grp], n_steps=a.n_steps, ensemble=E,
                               ensemble_stat="median")

    res = alternate({"serial_enhance": serial, "enhance_many": batched}, 1, max(3, a.repeats // 2))
    secs = sum(f.shape[-1] for f in files) / spec.fs
    print(json.dumps({"what": "dir", "config": a.config, "files": a.files, "E": E, "member_rows_per_call": per * E,
                      "audio_seconds": round(secs, 1), "ms_median_min_max": res,
                      "utt_per_s": {k: round(a.files / (v[0] * 1e-3), 2) for k, v in res.items()},
                      "many_vs_serial": round(res["enhance_many"][0] / res["serial_enhance"][0], 4)}), flush=True)


if __name__ == "__main__":
    main()
