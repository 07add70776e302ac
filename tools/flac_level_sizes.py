"""Sizes and times of the FLAC compression levels, in ONE process on one MI355X, for two contents of 16 mono files
of 4 s at 16 kHz, 24 bit:
  enhanced : the workload of tools/flac_encode_rate.py (an enhanced batch of the synthetic full-width model PP16)
  ar8      : the order-8 autoregressive, speech-like process of tests/flac_level_cases.py, a third of full scale at the peak
Per level 0, 1, 2: total bytes of the 16 streams, how many subframes took each form, audio.save_flac_many wall time and the
device stage alone (ou_flac_encode_frames_level, no copy, no host stage); each time is the best of `--repeats` after a warm-up,
with a device synchronisation on both sides.  Level 0's times in this run are the baseline of the other two.  One JSON line, also
written to profiles/flac_level_sizes.json.

  python tools/flac_level_sizes.py [--repeats 5] [--steps 4]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flac_level_cases as LC  # noqa: E402
from flac_encode_rate import best_ms  # noqa: E402
from helpers import get_spec, synth_mix  # noqa: E402
from open_universe_amd import Universe, UniverseGAN, audio as A, state_dict as S  # noqa: E402

FILES, SECONDS, BPS = 16, 4, 24


def contents(steps):
    spec = get_spec("PP16")
    n = SECONDS * spec.fs
    cls = UniverseGAN if spec.kind == "universe_gan" else Universe
    model = cls(spec, state_dict=S.synthetic_state_dict(spec, 0), device="cuda:0")
    sigs = [synth_mix(spec, 1, n, seed=500 + i)[0].cuda() for i in range(FILES)]
    with torch.no_grad():
        enh = model.enhance_many(sigs, torch.Generator(device="cuda").manual_seed(1), n_steps=steps)
    enh = [e.reshape(1, -1)[:, :n].contiguous() for e in enh]
    peak = max(float(e.abs().max()) for e in enh)
    del model
    full = 1 << (BPS - 1)
    ar = [torch.from_numpy(LC.from_ints(LC.ar8(n, 900 + i, full // 3), BPS)).cuda() for i in range(FILES)]
    return spec.fs, n, {"enhanced": [e * (0.5 / max(peak, 1e-9)) for e in enh], "ar8": ar}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flac_level_sizes.py measures on a HIP device; none found")
    result = {"figure": "flac_level_sizes_16_files_4s_mono_24bit", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "note": "one measurement"}
    fs, n, sets = contents(args.steps)
    result["fs"], result["pcm_bytes"] = fs, FILES * n * 3
    for name, sigs in sets.items():
        x = torch.stack([s[0] for s in sigs])
        rows = {}
        with tempfile.TemporaryDirectory() as tmp:
            paths = [os.path.join(tmp, f"f{i}.flac") for i in range(FILES)]
            for level in (0, 1, 2):
                streams, rec = A.flac_encode_many(sigs, fs, BPS, level=level, return_choices=True)
                rec = np.concatenate(rec)
                kinds = {LC.KINDS[k]: int((rec[:, 0] == k).sum()) for k in sorted(LC.KINDS)}
                t_many = best_ms(lambda: A.save_flac_many(paths, sigs, fs, BPS, level=level), args.repeats)
                t_dev = best_ms(lambda: A._flac_encode_device(x, x.stride(0), [1] * FILES, [n] * FILES, BPS, level), args.repeats)
                assert [open(p, "rb").read() for p in paths] == streams
                rows[f"level_{level}"] = {"stream_bytes": sum(len(s) for s in streams), "subframes": kinds,
                                          "partition_orders": np.bincount(rec[:, 2], minlength=7).tolist(),
                                          "save_flac_many_ms": round(t_many, 3), "device_stage_ms": round(t_dev, 4)}
        result[name] = rows
    line = json.dumps(result)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "flac_level_sizes.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
