"""Figures of the segmented ensemble over files of different lengths: `enhance_long_many_ensemble`
(ou_enhance_segments_var_ensemble) against the file-by-file loop of `enhance_long_ensemble` (what `--segment-ensemble E` runs per
file) on the two sets of DESIGN 4.13:

  a: 16 files of 2-8 s plus one of 3 min          b: 8 files of 1-5 min

The two variants alternate inside every repeat, in ONE process on one handle; counter noise on both sides (no noise tensor, a
file's noise does not depend on the grouping).  One JSON line per (set, E): wall time per pass (median, min, max over the repeats,
ms), workspace bytes of both sides, launches (ou_launch_stats), and the worst file-vs-alone SI-SDR / SNR of the reduced outputs.

  python tools/segment_many_ensemble_figures.py --config PP16 --steps 8 --segment 8 --sets a,b --ensembles 4,8 --warmup 1 --repeats 5
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import open_universe_amd  # noqa: E402,F401
import restatement as O  # noqa: E402
from open_universe_amd import Universe, UniverseGAN, state_dict as S  # noqa: E402
from open_universe_amd.noise import CounterNoise  # noqa: E402
from helpers import get_spec  # noqa: E402
from segment_many_figures import set_seconds, signal, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="PP16")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--segment", type=float, default=8.0)
    ap.add_argument("--overlap", type=float, default=1.0)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--sets", default="a,b")
    ap.add_argument("--ensembles", default="4,8")
    ap.add_argument("--stat", default="median")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    spec = get_spec(args.config)
    cls = UniverseGAN if spec.kind == "universe_gan" else Universe
    model = cls(spec, state_dict=S.synthetic_state_dict(spec, seed=0), device="cuda:0")
    kw = dict(segment_s=args.segment, overlap_s=args.overlap, max_batch=args.max_batch, n_steps=args.steps)
    for which in args.sets.split(","):
        secs = set_seconds(which)
        sigs = [signal(spec.fs, int(round(s * spec.fs)), seed=i) for i, s in enumerate(secs)]
        srcs = lambda: [CounterNoise(3, i) for i in range(len(sigs))]  # noqa: E731
        for E in [int(v) for v in args.ensembles.split(",")]:
            peak = {}

            def loop():
                outs, launches, ws = [], 0, 0
                for x, g in zip(sigs, srcs()):
                    outs.append(model.enhance_long_ensemble(x, E, args.stat, rng=g, **kw))
                    ws = max(ws, model._seg_ws[1].numel())
                    launches += model.launch_stats()[0]
                peak["loop_ws"], peak["loop_launches"] = ws, launches
                return outs

            def many():
                outs = model.enhance_long_many_ensemble(sigs, E, args.stat, rngs=srcs(), **kw)
                peak["many_ws"], peak["many_launches"] = model._seg_ws[1].numel(), model.launch_stats()[0]
                return outs

            for _ in range(args.warmup):
                loop()
                many()
            ms = {"loop": [], "many": []}
            for _ in range(args.repeats):
                t, ref = timed(loop)
                ms["loop"].append(t)
                t, out = timed(many)
                ms["many"].append(t)
            figs = [O.si_sdr(r.cpu(), y.cpu()) for r, y in zip(ref, out)]
            del ref, out
            stat = lambda v: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]  # noqa: E731
            print(json.dumps({"set": which, "E": E, "stat": args.stat, "config": args.config, "steps": args.steps,
                              "segment_s": args.segment, "max_batch": args.max_batch, "files": len(sigs),
                              "audio_s": round(sum(secs), 1), "loop_ms": stat(ms["loop"]), "many_ms": stat(ms["many"]),
                              "loop_over_many_median": round(statistics.median(ms["loop"]) / statistics.median(ms["many"]), 3),
                              "loop_workspace_bytes": peak["loop_ws"], "many_workspace_bytes": peak["many_ws"],
                              "loop_launches": peak["loop_launches"], "many_launches": peak["many_launches"],
                              "worst_file_vs_alone_si_sdr_db": round(min(float(f) for f in figs), 1),
                              "worst_file_vs_alone_snr_db": round(min(f.snr for f in figs), 1)}), flush=True)


if __name__ == "__main__":
    main()
