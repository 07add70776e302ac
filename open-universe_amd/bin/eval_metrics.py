"""
`python -m open_universe_amd.bin.eval_metrics REF_DIR DEG_DIR --metrics lsd si-lsd si-sdr snr [sdr] [--intelligibility stoi stoi-ext] [--batch-size N] --result-dir OUT`

The scoring half of the reference's inference tooling (open_universe/bin/eval_metrics.py) for the metrics this library
computes on the device (open_universe_amd.metrics): every .wav / .flac below DEG_DIR is scored against the file with the same
relative path below REF_DIR.  Up to --batch-size pairs of one sample rate -- of any lengths -- share one library call per
metric (`metrics.evaluate_many`); every pair is scored as if it were alone.

`sdr` (the BSS-eval SDR, filter length 512) is computed when it is named; it is not among the defaults.
`--intelligibility stoi stoi-ext` adds STOI and / or extended STOI (`metrics.stoi`; default: neither): their columns follow
those of --metrics in the same two files.  `--metrics stoi` stays refused.

Nothing is resampled: a pair whose two sample rates differ is an error naming the pair.  Files are mono.

Written to OUT (default: the parent of DEG_DIR), as the reference writes them: `<name of DEG_DIR>.json` with one entry
{metric: value} per file, keyed by the relative path without its suffix, and `<name of DEG_DIR>_summary.json` with the mean of
every metric over the files, `<metric>_std` beside it, and "number", the count of files.
"""
import argparse
import json
import math
import sys
from pathlib import Path

from .. import metrics as M
from ..audio import load

SUFFIXES = (".wav", ".flac")


def find_pairs(ref_dir, deg_dir):
    """-> sorted list of (label, reference path, degraded path); label = relative path below DEG_DIR without the suffix.
    A degraded file without a reference of the same relative path (either suffix) is an error."""
    ref_dir, deg_dir = Path(ref_dir), Path(deg_dir)
    pairs = []
    for deg in sorted(p for p in deg_dir.rglob("*") if p.is_file() and p.suffix.lower() in SUFFIXES):
        rel = deg.relative_to(deg_dir)
        cands = [ref_dir / rel] + [ref_dir / rel.with_suffix(s) for s in SUFFIXES]
        ref = next((c for c in cands if c.is_file()), None)
        if ref is None:
            raise FileNotFoundError(f"{deg}: no reference {ref_dir / rel} (every metric here needs one)")
        pairs.append((rel.with_suffix("").as_posix(), ref, deg))
    if not pairs:
        raise FileNotFoundError(f"{deg_dir}: no .wav / .flac file")
    return pairs


def load_pair(label, ref_path, deg_path):
    """-> (fs, degraded (T,), reference (T',)); mono files of ONE sample rate."""
    deg, fs = load(deg_path)
    ref, fs_ref = load(ref_path)
    if deg.shape[0] > 1 or ref.shape[0] > 1:
        raise ValueError(f"{label}: expected mono data ({deg_path}: {deg.shape[0]} channels, {ref_path}: {ref.shape[0]})")
    if int(fs) != int(fs_ref):
        raise ValueError(f"{label}: {ref_path} is at {fs_ref} Hz and {deg_path} at {fs} Hz: nothing is resampled here, "
                         "bring the pair to one rate first")
    return int(fs), deg[0], ref[0]


def summarize(results):
    """{label: {metric: value}} -> {metric: mean, metric_std: population std, "number": files}; infinite values are left out of
    a metric's mean."""
    values = {}
    for res in results.values():
        for met, val in res.items():
            if isinstance(val, str) or math.isinf(val):
                continue
            values.setdefault(met, []).append(float(val))
    summary = {}
    for met, v in values.items():
        mean = sum(v) / len(v)
        summary[met] = mean
        summary[met + "_std"] = math.sqrt(sum((a - mean) ** 2 for a in v) / len(v))
    summary["number"] = len(results)
    return summary


def save_results(results, result_dir, name):
    result_dir = Path(result_dir)
    result_dir.mkdir(parents=True, exist_ok=True)
    results_path, summary_path = result_dir / f"{name}.json", result_dir / f"{name}_summary.json"
    with open(results_path, "w") as f:
        json.dump(results, f, indent=2)
    with open(summary_path, "w") as f:
        json.dump(summarize(results), f, indent=2)
    return results_path, summary_path


def evaluate_pairs(pairs, metric_names, batch_size=16, device="cuda:0", intelligibility=()):
    """Score the pairs in batches of one sample rate -> {label: {metric: value}} in the order of `pairs`."""
    names = M.check_score_names(metric_names)
    extra = M.check_intelligibility_names(intelligibility)
    results = {label: None for label, _, _ in pairs}
    pending = {}  # fs -> [(label, deg, ref)]

    def flush(fs):
        batch = pending.pop(fs, [])
        if batch:
            scores = M.evaluate_many([d.to(device) for _, d, _ in batch], [r.to(device) for _, _, r in batch], fs, names,
                                     intelligibility=extra)
            for (label, _, _), s in zip(batch, scores):
                results[label] = s

    for label, ref_path, deg_path in pairs:
        fs, deg, ref = load_pair(label, ref_path, deg_path)
        pending.setdefault(fs, []).append((label, deg, ref))
        if len(pending[fs]) >= batch_size:
            flush(fs)
    for fs in list(pending):
        flush(fs)
    return results


def main(argv=None):
    parser = argparse.ArgumentParser(description="Score enhanced files against their references on the device")
    parser.add_argument("ref_path", type=Path, help="Path to the reference (clean) audio folder")
    parser.add_argument("enhanced_path", type=Path, help="Path to the enhanced (degraded) audio folder")
    parser.add_argument("--metrics", nargs="+", default=list(M.AVAILABLE_METRICS),
                        help=f"Metrics to compute (default: {' '.join(M.AVAILABLE_METRICS)}; also: {' '.join(M.OPTIONAL_METRICS)})")
    parser.add_argument("--intelligibility", nargs="*", default=[], choices=list(M.INTELLIGIBILITY_METRICS),
                        help="STOI scores to add (default: none)")
    parser.add_argument("--batch-size", type=int, default=16, help="pairs per library call")
    parser.add_argument("--result-dir", "--result_dir", type=Path, default=None, help="where the two JSON files go")
    parser.add_argument("--device", default="cuda:0")
    args = parser.parse_args(argv)
    if args.batch_size < 1:
        parser.error("--batch-size must be at least 1")
    names = M.check_score_names(args.metrics)
    pairs = find_pairs(args.ref_path, args.enhanced_path)
    results = evaluate_pairs(pairs, names, args.batch_size, args.device, args.intelligibility)
    result_dir = args.enhanced_path.resolve().parent if args.result_dir is None else args.result_dir
    paths = save_results(results, result_dir, args.enhanced_path.resolve().name)
    print(f"{len(results)} files scored: {paths[0]}, {paths[1]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
