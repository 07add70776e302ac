"""Figures of the FLAC output path: 16 mono files of 4 s, 24 bit, at 16 kHz and at 24 kHz, content = an enhanced
batch of the synthetic full-width model (PP16 / PP24), encoded three ways in ONE process on one MI355X:
  1. numpy_loop   : audio.save_flac file by file (copy to the host, float64 quantisation, the numpy bit packer, Python CRCs)
  2. library_many : audio.flac_encode_many (one kernel launch, three device-to-host copies, ou_flac_assemble) + writing the files
  3. device_stage : ou_flac_encode_frames alone (no copy, no host stage)
Each is the best of `--repeats` after a warm-up, with a device synchronisation on both sides.  One JSON line.

  python tools/flac_encode_rate.py [--repeats 5] [--steps 4]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from helpers import get_spec, synth_mix  # noqa: E402
from open_universe_amd import Universe, UniverseGAN, audio as A, state_dict as S  # noqa: E402

FILES, SECONDS, BPS = 16, 4, 24


def best_ms(fn, repeats):
    fn()  # warm-up
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flac_encode_rate.py measures on a HIP device; none found")
    result = {"figure": "flac_encode_16_files_4s_mono_24bit", "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    for name in ("PP16", "PP24"):
        spec = get_spec(name)
        cls = UniverseGAN if spec.kind == "universe_gan" else Universe
        model = cls(spec, state_dict=S.synthetic_state_dict(spec, 0), device="cuda:0")
        n = SECONDS * spec.fs
        sigs = [synth_mix(spec, 1, n, seed=500 + i)[0].cuda() for i in range(FILES)]
        with torch.no_grad():
            enh = model.enhance_many(sigs, torch.Generator(device="cuda").manual_seed(1), n_steps=args.steps)
        enh = [e.reshape(1, -1)[:, :n].contiguous() for e in enh]
        peak = max(float(e.abs().max()) for e in enh)
        enh = [e * (0.5 / max(peak, 1e-9)) for e in enh]  # the level of a real result: half of full scale at the peak
        del model
        x = torch.stack([e[0] for e in enh])
        with tempfile.TemporaryDirectory() as tmp:
            paths_a = [os.path.join(tmp, f"a{i}.flac") for i in range(FILES)]
            paths_b = [os.path.join(tmp, f"b{i}.flac") for i in range(FILES)]

            def numpy_loop():
                for p, e in zip(paths_a, enh):
                    A.save_flac(p, e, spec.fs, BPS)

            t_numpy = best_ms(numpy_loop, args.repeats)
            t_lib = best_ms(lambda: A.save_flac_many(paths_b, enh, spec.fs, BPS), args.repeats)
            t_dev = best_ms(lambda: A._flac_encode_device(x, x.stride(0), [1] * FILES, [n] * FILES, BPS), args.repeats)
            same = all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(paths_a, paths_b))
            size = sum(os.path.getsize(b) for b in paths_b)
        result[f"fs_{spec.fs}"] = {"numpy_loop_ms": round(t_numpy, 3), "library_many_ms": round(t_lib, 3),
                                   "device_stage_ms": round(t_dev, 4), "ratio_numpy_over_library": round(t_numpy / t_lib, 1),
                                   "byte_identical": same, "stream_bytes": size, "pcm_bytes": FILES * n * 3}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
