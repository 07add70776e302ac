"""Figures of the resampler: `audio.resample` / the per-file loop with the torch backend (pad + dense strided
conv1d + transpose copy + slice) against the library backend (ou_resample), in ONE process on one MI355X.  The variants
alternate inside every repeat; a timed block is `--inner` calls between two device synchronisations (one call of a 4 s file is
tens of microseconds: a block of one would time the clock), reported per call; one JSON line per figure with the median and
the spread of the repeats.  The first line is the box's device-to-device copy bandwidth.

  python tools/resample_rate.py [--repeats 25] [--warmup 5] [--inner 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import open_universe_amd  # noqa: E402,F401
from open_universe_amd import audio as A  # noqa: E402

PAIRS = [(44100, 16000), (16000, 44100), (48000, 16000), (16000, 48000)]


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def alternate(variants, warmup, repeats, inner):
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(timed(fn, inner))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in ms.items()}


def copy_bandwidth():
    a = torch.empty(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    ms = statistics.median(timed(lambda: b.copy_(a), 4) for _ in range(7))
    return 2 * a.numel() * 4 / (ms * 1e-3) / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_rate.py measures on a HIP device; none found")
    print(json.dumps({"figure": "copy_bandwidth_TB_per_s", "value": round(copy_bandwidth(), 3),
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    for fs, tfs in PAIRS:
        # one 4 s mono file
        x = 0.1 * torch.randn(1, 4 * fs, device="cuda", generator=g)
        res = alternate({"torch": lambda: A.resample(x, fs, tfs),
                         "library": lambda: A.resample(x, fs, tfs, backend="library")}, args.warmup, args.repeats, args.inner)
        print(json.dumps({"figure": "one_file_4s_mono", "fs_in": fs, "fs_out": tfs, **res}), flush=True)
        # 16 files of 2 - 8 s: the 16-call loop against one resample_many call
        secs = [2.0 + 6.0 * i / 15 for i in range(16)]
        files = [0.1 * torch.randn(1, int(s * fs), device="cuda", generator=g) for s in secs]
        res = alternate({"torch_loop_16": lambda: A.resample_many(files, fs, tfs),
                         "library_loop_16": lambda: [A.resample(f, fs, tfs, backend="library") for f in files],
                         "library_many_16": lambda: A.resample_many(files, fs, tfs, backend="library")},
                        args.warmup, args.repeats, max(1, args.inner // 4))
        print(json.dumps({"figure": "16_files_2_to_8s", "fs_in": fs, "fs_out": tfs, "audio_seconds": round(sum(secs), 1), **res}),
              flush=True)


if __name__ == "__main__":
    main()
