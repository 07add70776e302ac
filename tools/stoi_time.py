"""Call time of metrics.stoi (ou_stoi) on the device: B pairs of T samples at fs, both forms, device events around windows of
back-to-back calls (scratch allocation by torch's caching allocator included: it is what a caller of metrics.stoi pays), after a
warm-up of the same shape; si_sdr on the same rows beside it for scale.  Prints one JSON line.

  python tools/stoi_time.py [--pairs 16] [--seconds 4] [--fs 16000] [--calls 200] [--windows 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from open_universe_amd import metrics as M  # noqa: E402


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stoi_time.py needs a HIP device: a time taken anywhere else says nothing")
    T = int(args.seconds * args.fs)
    g = torch.Generator().manual_seed(0)
    t = torch.arange(T) / args.fs
    ref = torch.randn(args.pairs, T, generator=g) * (0.6 + 0.4 * torch.sin(2 * torch.pi * 3.0 * t))
    est = (ref + 0.3 * torch.randn(args.pairs, T, generator=g)).cuda()
    ref = ref.cuda()
    runs = {"stoi": lambda: M.stoi(est, ref, args.fs), "stoi_ext": lambda: M.stoi(est, ref, args.fs, extended=True),
            "si_sdr": lambda: M.si_sdr(est, ref)}
    out = {"pairs": args.pairs, "T": T, "fs": args.fs, "calls_per_window": args.calls, "windows": args.windows,
           "device": torch.cuda.get_device_name(0)}
    for name, fn in runs.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = [window_ms(fn, args.calls) for _ in range(args.windows)]
        out[name + "_ms_per_call"] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}
    out["stoi_first_row"] = float(runs["stoi"]()[0])
    out["stoi_ext_first_row"] = float(runs["stoi_ext"]()[0])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
