"""Figures of the ensemble of a long recording: `enhance_long_ensemble` (ou_enhance_segments_ensemble) against the
way without it -- E `enhance_long` calls, one per member on that member's stream ids, and `ensemble_reduce` over their outputs.

The two variants alternate inside every repeat, in ONE process on one box; counter noise on both sides (no noise tensor; a
member's noise does not depend on the grouping).  One JSON line per E: wall time per pass (median, min, max over the repeats,
ms), launches, workspace bytes, and the worst member-vs-loop SI-SDR / SNR.

  python tools/segment_ensemble_figures.py --config PP16 --steps 8 --seconds 60 --ensembles 4,8 --warmup 1 --repeats 7
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
import restatement as O  # noqa: E402
from open_universe_amd import Universe, UniverseGAN, state_dict as S  # noqa: E402
from open_universe_amd.noise import CounterNoise  # noqa: E402
from open_universe_amd.universe import ensemble_reduce  # noqa: E402
from helpers import get_spec  # noqa: E402


def signal(fs, T, seed=0, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    t = torch.arange(T, device=device, dtype=torch.float64) / fs
    x = 0.1 * torch.sin(2 * math.pi * (150.0 + 35.0 * (seed % 9)) * t) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3 * t))
    return x.float() + 0.03 * torch.randn(T, device=device, generator=g)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="PP16")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--segment", type=float, default=8.0)
    ap.add_argument("--overlap", type=float, default=1.0)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--ensembles", default="4,8")
    ap.add_argument("--stat", default="median")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    spec = get_spec(args.config)
    cls = UniverseGAN if spec.kind == "universe_gan" else Universe
    model = cls(spec, state_dict=S.synthetic_state_dict(spec, seed=0), device="cuda:0")
    kw = dict(segment_s=args.segment, overlap_s=args.overlap, max_batch=args.max_batch, n_steps=args.steps)
    x = signal(spec.fs, int(round(args.seconds * spec.fs)))[None, :]  # (1, T)
    segment, overlap = int(round(args.segment * spec.fs)), int(round(args.overlap * spec.fs))
    for E in [int(v) for v in args.ensembles.split(",")]:
        src = CounterNoise(3, 0)
        ids = src.stream_ids(1, E)
        peak = {}

        def loop():
            launches, mem = 0, []
            for e in range(E):  # member e alone: the row on that member's stream id
                mem.append(model._segments_call(x, segment, overlap, args.max_batch, args.steps, model.diff_kwargs.epsilon,
                                                False, None, (src.seed, [ids[e]])))
                launches += model.launch_stats()[0]
            mem = torch.stack(mem)
            peak["loop_ws"], peak["loop_launches"] = model._seg_ws[1].numel(), launches
            return ensemble_reduce(mem, args.stat), mem

        def one():
            r = model.enhance_long_ensemble(x, E, args.stat, rng=src, return_members=True, **kw)
            peak["one_ws"], peak["one_launches"] = model._seg_ws[1].numel(), model.launch_stats()[0]
            return r

        for _ in range(args.warmup):
            loop()
            one()
        ms = {"loop": [], "one": []}
        for _ in range(args.repeats):
            t, ref = timed(loop)
            ms["loop"].append(t)
            t, out = timed(one)
            ms["one"].append(t)
        figs = [O.si_sdr(ref[1][e].cpu(), out[1][e].cpu()) for e in range(E)]
        stat = lambda v: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]  # noqa: E731
        print(json.dumps({"E": E, "config": args.config, "steps": args.steps, "seconds": args.seconds, "segment_s": args.segment,
                          "max_batch": args.max_batch, "stat": args.stat,
                          "loop_ms": stat(ms["loop"]), "one_call_ms": stat(ms["one"]),
                          "speedup_median": round(statistics.median(ms["loop"]) / statistics.median(ms["one"]), 3),
                          "loop_workspace_bytes": peak["loop_ws"], "one_call_workspace_bytes": peak["one_ws"],
                          "loop_launches": peak["loop_launches"], "one_call_launches": peak["one_launches"],
                          "worst_member_vs_loop_si_sdr_db": round(min(float(f) for f in figs), 1),
                          "worst_member_vs_loop_snr_db": round(min(f.snr for f in figs), 1)}), flush=True)


if __name__ == "__main__":
    main()
