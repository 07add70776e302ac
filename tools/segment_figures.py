"""Figures of the segmented enhance: segmented vs whole-file SI-SDR per overlap, wall time and workspace bytes of
`enhance_long` against one whole-file `enhance`, and a row past the length guard of `ou_enhance`.  One JSON line per figure.

  python tools/segment_figures.py gap  --config PP16 --seconds 60 --overlaps 0.25,0.5,1,2
  python tools/segment_figures.py time --config PP16 --seconds 600
  python tools/segment_figures.py long --config PP24 --seconds 1440
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402

import open_universe_amd  # noqa: E402,F401
from open_universe_amd import Universe, state_dict as S  # noqa: E402
from helpers import get_spec  # noqa: E402


def signal(fs, T, seed=0, device="cuda"):
    """AM tones + noise (the suite's synthetic input), drawn on the device: long rows without a host copy."""
    g = torch.Generator(device=device).manual_seed(seed)
    t = torch.arange(T, device=device, dtype=torch.float64) / fs
    x = 0.1 * torch.sin(2 * math.pi * 220.0 * t) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3 * t))
    x = x + 0.02 * torch.sin(2 * math.pi * 0.05 * t) * torch.sin(2 * math.pi * 700.0 * t)
    return (x.float() + 0.03 * torch.randn(T, device=device, generator=g))


def si_sdr(ref, est):
    ref = ref.double().flatten()
    est = est.double().flatten()
    a = (ref @ est) / (ref @ ref)
    e = a * ref - est
    return float(10 * torch.log10((a * ref).square().sum() / e.square().sum()))


def model_for(name):
    spec = get_spec(name)
    return Universe(spec, state_dict=S.synthetic_state_dict(spec, seed=0), device="cuda:0"), spec


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = fn()
    torch.cuda.synchronize()
    return y, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["gap", "time", "long"])
    ap.add_argument("--config", default="PP16")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--overlaps", default="0.25,0.5,1,2")
    ap.add_argument("--segment", type=float, default=Universe.SEGMENT_S)
    ap.add_argument("--n-steps", type=int, default=None)
    ap.add_argument("--max-batch", type=int, default=32)
    a = ap.parse_args()
    model, spec = model_for(a.config)
    T = int(round(a.seconds * spec.fs))
    x = signal(spec.fs, T)
    res = {"what": a.what, "config": a.config, "seconds": a.seconds, "segment_s": a.segment}
    if a.what == "gap":
        whole = model.enhance(x, n_steps=a.n_steps, rng=torch.Generator(device="cuda").manual_seed(5))
        for ov in [float(v) for v in a.overlaps.split(",")]:
            y = model.enhance_long(x, segment_s=a.segment, overlap_s=ov, n_steps=a.n_steps, max_batch=a.max_batch,
                                   rng=torch.Generator(device="cuda").manual_seed(5))
            print(json.dumps(dict(res, overlap_s=ov, si_sdr_vs_whole=round(si_sdr(whole, y), 2))), flush=True)
        return
    rng = lambda: torch.Generator(device="cuda").manual_seed(5)  # noqa: E731
    model.enhance_long(x[: spec.fs * 20], segment_s=a.segment, n_steps=a.n_steps, max_batch=a.max_batch, rng=rng())  # warm
    y, t_seg = timed(lambda: model.enhance_long(x, segment_s=a.segment, n_steps=a.n_steps, max_batch=a.max_batch, rng=rng()))
    y2 = model.enhance_long(x, segment_s=a.segment, n_steps=a.n_steps, max_batch=a.max_batch, rng=rng())
    res.update(segmented_s=round(t_seg, 3), segmented_ws_bytes=int(model._seg_ws[1].numel()),
               finite=bool(torch.isfinite(y).all()), peak=float(y.abs().max()), repeat_bit_identical=bool(torch.equal(y, y2)))
    if a.what == "time":
        yw, t_whole = timed(lambda: model.enhance(x, n_steps=a.n_steps, rng=rng()))
        B, Tp = 1, T + (spec.tot_ds - T % spec.tot_ds)
        res.update(whole_s=round(t_whole, 3), whole_ws_bytes=int(model._workspace_bytes(B, Tp)),
                   si_sdr_vs_whole=round(si_sdr(yw, y), 2))
    else:
        try:
            model.enhance(x, n_steps=a.n_steps, rng=rng())
            res["whole"] = "ran"
        except ValueError as e:
            res["whole"] = "refused: " + str(e)[:160]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
