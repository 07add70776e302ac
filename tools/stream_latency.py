"""Measure the streaming enhance: the time of one steady-state push that completes a window against
`ou_enhance` of the same (C, S) -- the floor: a window IS that call -- and the cost of the two stream kernels alone (a push
that completes no window runs the gather only; the difference of the two calls is gather + emit + the stitch's bookkeeping).
Writes profiles/stream_latency.json.  Single measurements (medians of `--reps` timed calls on an otherwise idle device).

    python tools/stream_latency.py [--model PP16] [--channels 1] [--segment-seconds 4] [--overlap-seconds 0.5] [--steps 8]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="PP16")
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--segment-seconds", type=float, default=4.0)
    ap.add_argument("--overlap-seconds", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_latency.json"))
    a = ap.parse_args()
    from helpers import get_spec, synth_mix
    from open_universe_amd import Universe, UniverseGAN, state_dict as S
    from open_universe_amd.noise import CounterNoise

    spec = get_spec(a.model)
    model = (UniverseGAN if spec.kind == "universe_gan" else Universe)(spec, state_dict=S.synthetic_state_dict(spec, seed=0),
                                                                        device="cuda:0")
    C = a.channels
    st = model.stream(channels=C, segment_s=a.segment_seconds, overlap_s=a.overlap_seconds, seed=1, n_steps=a.steps)
    Sg = st.latency_samples
    hop = Sg - (int(round(a.overlap_seconds * spec.fs)) // spec.tot_ds) * spec.tot_ds
    x = synth_mix(spec, C, Sg + hop * (a.reps + 3)).cuda()
    w = x[:, :Sg].contiguous()
    floor = lambda: model.enhance(w, n_steps=a.steps, rng=CounterNoise(1, stream=0))  # noqa: E731
    for _ in range(2):
        floor()
    t_floor = timed(floor, a.reps)
    st.push(x[:, :Sg])  # window 0, and the warm-up of the stream's own workspace
    st.push(x[:, Sg:Sg + hop])
    at = [Sg + hop]

    def window_push():
        st.push(x[:, at[0]:at[0] + hop])
        at[0] += hop

    t_push = timed(window_push, a.reps)
    st.flush()
    st.push(x[:, :16])
    t_ring = timed(lambda: st.push(x[:, :16]), a.reps)  # no window completes: one gather launch (ring update) and the host side
    st.close()
    res = {"model": a.model, "device": torch.cuda.get_device_name(0), "C": C, "S": Sg, "hop": hop, "n_steps": a.steps, "reps": a.reps,
           "ou_enhance_of_one_window_ms": t_floor, "push_completing_one_window_ms": t_push,
           "push_completing_no_window_ms": t_ring, "stream_over_floor_ms": t_push - t_floor,
           "note": "medians of single runs through the Python layer (the floor through Universe.enhance, which also pads a "
                   "full block and polls the status word); a push that completes a window = gather + ou_enhance + emit"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
