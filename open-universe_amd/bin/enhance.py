"""
`python -m open_universe_amd.bin.enhance <input> <output> [--model ...] [enhance arguments]`

The reference's inference script (open_universe/bin/enhance.py:83-192) on the MI355X-native model: enhance one audio
file or every .wav/.mp3/.flac below a folder (folder structure retained), channels of a file = batch of the
`enhance` call, resample to the model rate and back, ONE torch.Generator seeded with --seed shared by all files in
processing order (so a run is reproducible file by file, exactly like the reference), model-specific arguments
generated from the signature of `model.enhance`.

Extensions (not in the reference, whose loop is serial on one device, one file per `enhance` call):
* launched under `torch.distributed.run` with N processes, the files are sharded over the ranks (one GPU each, LPT by
  file size so the ranks finish together); rank 0 reads the checkpoint and the packed weights reach the other ranks
  with one broadcast (`inference_utils.load_model_sharded`).  Because the reference draws the noise of file k from the
  generator state left by files 0..k-1, a sharded run cannot reproduce the serial noise; with `--per-file-seed` (forced
  when N > 1) file k uses its own generator seeded with `seed + k` (k = index in the sorted file list), which makes the
  result of a file independent of how the list was sharded;
* `--batch-size K`: up to K files of the same sample rate -- of ANY lengths -- share
  one `enhance` call (`Universe.enhance_many`; the channels of a file stay rows of the batch).  Every row keeps the
  geometry of the call on that file alone (own padding, normalisation, conv zero padding, GRU length: exact batching,
  ou_enhance_var), and the noise is drawn file by file in processing order with the shapes of the serial loop, so the
  shared generator advances exactly as in the reference and every file gets the noise -- and, to fp32 round-off, the
  result -- it would get alone.  Files are read `--batch-window` ahead (default 4 K) and grouped by length inside the window
  (a call costs what its longest row costs); every file's generator starts from the state the shared generator has in front
  of that file in processing order, so the grouping does not change anybody's noise.  `--pad-batch` selects the reference's own batch semantics instead: right-zero-padded to
  the longest like `max_collator` (datasets/datamodule.py:24-42; no mask: the padding takes part in the normalisation,
  as in a reference batch).
"""
import argparse
import os
import sys
from pathlib import Path

import torch

from .. import inference_utils
from ..audio import AUDIO_SUFFIXES, can_decode, channels, load, resample, resample_many, save, save_flac_many


def handle_help(argv):
    """bin/enhance.py:36-57: defer --help until the model's own arguments are known."""
    if "--model" not in argv:
        return False
    for flag in ("--help", "-h"):
        if flag in argv:
            argv.remove(flag)
            return True
    return False


def find_files(path):
    """bin/enhance.py:60-74 (sorted, so that the processing order -- and with it the noise -- is deterministic)."""
    path = Path(path)
    if not path.is_dir():
        return [path], path.parent, False
    files = sorted(p for p in path.rglob("*") if p.suffix in AUDIO_SUFFIXES)
    return files, path, True


def plan_files(files, world, rank):
    """(index, path) pairs this rank processes: all of them in order for one process, else an LPT shard by file size
    (a proxy for the duration) -- the index k is what --per-file-seed adds to the seed."""
    todo = list(enumerate(files))
    if world <= 1:
        return todo
    from ..distributed import shard_utterances

    sizes = [os.path.getsize(p) for p in files]
    return [todo[i] for i in sorted(shard_utterances(sizes, world)[rank])]


def build_parser():
    parser = argparse.ArgumentParser(description="Enhance a file or a directory of audio files")
    parser.add_argument("input", type=Path, help="Path to an audio file or a folder of audio files")
    parser.add_argument("output", type=Path,
                        help="Output path for the enhanced files. In the case of a folder, the orignal structure is retained.")
    parser.add_argument("--model", type=str, default="line-corporation/open-universe:plusplus",
                        help="A checkpoint file (config.yaml beside it) or a Huggingface model id repo[:revision]")
    parser.add_argument("--hf-token", type=str, help="Huggingface access token")
    parser.add_argument("--model-strict", action="store_true",
                        help="Use strict policy to load the model. Can help uncover problems.")
    parser.add_argument("--seed", type=int, default=1028282, help="Set a deterministic seed to get reproducible results")
    parser.add_argument("--device", type=str, default="cuda:0", help="The device to use, e.g. cuda:0. Default: cuda:0.")
    parser.add_argument("--per-file-seed", action="store_true",
                        help="Seed the generator of file k with seed + k instead of sharing one generator across files "
                             "(always on when the files are sharded over several processes)")
    parser.add_argument("--noise", choices=("generator", "counter"), default="generator",
                        help="Where the sampler's noise comes from.  generator (default): torch.randn from the seeded generator, "
                             "as the reference draws it.  counter: a counter-based function of (--seed, file index in the sorted "
                             "list, channel, step, sample) evaluated on the device (an extension; the reference has no such "
                             "mode): a file's result then does not depend on batching, lanes, segmenting or sharding, and no "
                             "noise tensor is held in memory")
    parser.add_argument("--resampler", choices=("torch", "library"), default="torch",
                        help="What resamples a file to the model rate and back.  torch (default): a strided conv1d over the "
                             "dense windowed-sinc kernel.  library: the library's own kernel (ou_resample; an extension), the "
                             "same filter evaluated over the window's support only -- with --batch-size one launch per "
                             "window of files and per enhanced group instead of one chain of torch calls per file")
    parser.add_argument("--encoder", choices=("numpy", "library"), default="numpy",
                        help="What encodes a .flac output.  numpy (default): the host encoder, file by file.  library: the "
                             "library's own kernel (ou_flac_encode_frames; an extension) -- the results stay on the device, "
                             "every .flac output of a window, group or file is encoded in one call, and the files are byte "
                             "for byte those of the default.  .wav outputs are written as before")
    parser.add_argument("--flac-level", type=int, choices=(0, 1, 2), default=0,
                        help="Compression level of every .flac output, with either --encoder; .wav outputs ignore it.  0 "
                             "(default): fixed predictor of order 2, one Rice parameter per block.  1: constant subframes, "
                             "fixed orders 0-4, partitioned Rice.  2: level 1 plus an LPC candidate of order 8.  At levels 0 "
                             "and 1 the two encoders write identical files; at level 2 they may differ in the LPC subframes "
                             "(the last bits of the analysis), and both decode to the same samples")
    parser.add_argument("--batch-size", type=int, default=1,
                        help="Enhance up to this many consecutive files of equal sample rate (any lengths) in one call; "
                             "every file gets the result it would get alone")
    parser.add_argument("--batch-window", type=int, default=0,
                        help="With --batch-size: read this many files ahead and group them by length (longest first) -- a call "
                             "costs what its longest file costs.  Every file still gets the noise of the file-by-file loop "
                             "(its generator state is taken in processing order).  Default: 4 x batch-size; 1: files as they come")
    parser.add_argument("--in-flight", type=int, default=1,
                        help="Keep this many enhance calls in flight side by side on the device (one stream and workspace "
                             "each, 1..8): same result as the file-by-file loop, bit for bit, at a multiple of its "
                             "throughput (--batch-size reaches a higher rate, equal to fp32 round-off)")
    parser.add_argument("--segment-seconds", type=float, default=None,
                        help="Enhance every file longer than this many seconds in overlapping windows of this length "
                             "(Universe.enhance_long: bounded memory for recordings of any length; normalisation, mel scale, "
                             "noise and output level stay those of the whole file).  Takes --warm_start and --use_aux_signal "
                             "(every window starts from, or is, its own conditioner estimate); --segment-ensemble and "
                             "--segment-files N > 1 refuse them.  Off by default")
    parser.add_argument("--segment-overlap", type=float, default=None,
                        help="With --segment-seconds: overlap of consecutive windows in seconds (default 1.0)")
    parser.add_argument("--segment-files", type=int, default=1,
                        help="With --segment-seconds: enhance this many consecutive files of the sorted list in one call "
                             "(Universe.enhance_long_many: files of any lengths, long ones in windows, short ones as one "
                             "window each, the windows of all files share the window groups; every file gets the result "
                             "it would get alone).  Default 1: one file per call")
    parser.add_argument("--segment-ensemble", type=int, default=None,
                        help="With --segment-seconds: enhance every file as an ensemble of this many samples, reduced with "
                             "--ensemble_stat (Universe.enhance_long_ensemble: the windows of all members share the window "
                             "groups and the conditioner runs once per window).  Not with --ensemble or --segment-files > 1")
    parser.add_argument("--segment-ensemble-files", type=int, default=1,
                        help="With --segment-seconds and --segment-ensemble E: enhance this many consecutive files of the sorted "
                             "list in one call (Universe.enhance_long_many_ensemble: the windows of all files share the window "
                             "groups, all E members of a window in one group; every file gets the noise and, to round-off, the "
                             "result of the one-file-per-call loop).  Default 1: one file per call.  Not with --segment-files > 1")
    parser.add_argument("--stream", type=float, default=None, metavar="CHUNK_SECONDS",
                        help="With --segment-seconds: read every file in chunks of this many seconds and push them through a "
                             "streaming session (Universe.stream: every window of --segment-seconds is enhanced as an excerpt "
                             "of its own, crossfaded over --segment-overlap, on counter-based noise of --seed + file index; no "
                             "whole-file normalisation and no peak guard, so the result differs from the file-at-once forms).  "
                             "Not with --batch-size, --in-flight, --ensemble, --segment-ensemble, --segment-ensemble-files or "
                             "--segment-files > 1.  Off by default")
    parser.add_argument("--pad-batch", action="store_true",
                        help="With --batch-size: files of different lengths are zero-padded to the longest WITHOUT a mask "
                             "(the reference's batch semantics: the padding changes every result)")
    return parser


def group_files(todo, infos, batch_size, pad_batch=False):
    """Consecutive runs of `todo` (in processing order) that may share one enhance call: same sample rate (any number of
    samples: rows keep their own geometry, or are zero-padded with pad_batch), at most batch_size files.
    infos[k] = (fs, n_samples)."""
    groups, cur = [], []
    for item in todo:
        k = item[0]
        if cur:
            k0 = cur[0][0]
            same = infos[k][0] == infos[k0][0]
            if not same or len(cur) >= batch_size:
                groups.append(cur)
                cur = []
        cur.append(item)
    if cur:
        groups.append(cur)
    return groups


def check_segment_args(args, enhance_kwargs):
    """--segment-seconds / --segment-overlap: refused with what they cannot be combined with."""
    seg_ens = getattr(args, "segment_ensemble", None)
    if seg_ens is not None:
        if enhance_kwargs.get("ensemble") is not None:
            raise ValueError("--segment-ensemble cannot be combined with --ensemble (--segment-ensemble E is the ensemble of a "
                             "segmented file)")
        if args.segment_seconds is None:
            raise ValueError("--segment-ensemble needs --segment-seconds")
        if seg_ens < 1:
            raise ValueError("--segment-ensemble must be at least 1")
        if getattr(args, "segment_files", 1) > 1:
            raise ValueError("--segment-ensemble cannot be combined with --segment-files > 1 (one file per call)")
    ens_files = getattr(args, "segment_ensemble_files", 1)
    if ens_files != 1:
        if ens_files < 1:
            raise ValueError("--segment-ensemble-files must be at least 1")
        if args.segment_seconds is None or seg_ens is None:
            raise ValueError("--segment-ensemble-files needs --segment-seconds and --segment-ensemble")
        if getattr(args, "segment_files", 1) > 1:
            raise ValueError("--segment-ensemble-files cannot be combined with --segment-files > 1")
    if args.segment_seconds is None:
        if args.segment_overlap is not None:
            raise ValueError("--segment-overlap needs --segment-seconds")
        if getattr(args, "segment_files", 1) != 1:
            raise ValueError("--segment-files needs --segment-seconds")
        return
    if getattr(args, "segment_files", 1) < 1:
        raise ValueError("--segment-files must be at least 1")
    if not args.segment_seconds > 0:
        raise ValueError("--segment-seconds must be positive")
    ov = 1.0 if args.segment_overlap is None else args.segment_overlap
    if ov < 0 or 2 * ov > args.segment_seconds:
        raise ValueError("--segment-overlap must lie in [0, segment-seconds / 2]")
    if args.pad_batch:
        raise ValueError("--segment-seconds cannot be combined with --pad-batch")
    if args.batch_size > 1 or args.in_flight > 1:
        raise ValueError("--segment-seconds cannot be combined with --batch-size or --in-flight (--segment-files N puts N "
                         "files into one segmented call)")
    for key in ("ensemble", "target"):
        if enhance_kwargs.get(key) is not None:
            raise ValueError(f"--segment-seconds cannot be combined with --{key}")
    # --warm_start / --use_aux_signal: taken by the one-file-per-call form without an ensemble (enhance_long); the ensemble
    # and the multi-file forms of the CLI refuse them
    if seg_ens is not None or getattr(args, "segment_files", 1) > 1:
        form = "--segment-ensemble" if seg_ens is not None else "--segment-files > 1"
        if enhance_kwargs.get("warm_start") is not None:
            raise ValueError(f"{form} cannot be combined with --warm_start")
        if enhance_kwargs.get("use_aux_signal"):
            raise ValueError(f"{form} cannot be combined with --use_aux_signal")


def check_stream_args(args, enhance_kwargs):
    """--stream: refused with what it cannot be combined with."""
    if getattr(args, "stream", None) is None:
        return
    if args.segment_seconds is None:
        raise ValueError("--stream needs --segment-seconds (the window of the stream)")
    if not args.stream > 0:
        raise ValueError("--stream must be a positive number of seconds")
    if args.batch_size > 1 or args.in_flight > 1:
        raise ValueError("--stream cannot be combined with --batch-size or --in-flight (a stream is one file at a time)")
    if enhance_kwargs.get("ensemble") is not None:
        raise ValueError("--stream cannot be combined with --ensemble")
    if getattr(args, "segment_ensemble", None) is not None or getattr(args, "segment_ensemble_files", 1) != 1:
        raise ValueError("--stream cannot be combined with --segment-ensemble or --segment-ensemble-files")
    if getattr(args, "segment_files", 1) > 1:
        raise ValueError("--stream cannot be combined with --segment-files > 1")
    if enhance_kwargs.get("target") is not None:
        raise ValueError("--stream cannot be combined with --target")


def stream_file(model, audio, args, enhance_kwargs, k):
    """One file through a streaming session in chunks of --stream seconds: what comes out of the pushes and the flush, joined."""
    ov = 1.0 if args.segment_overlap is None else args.segment_overlap
    kw = {key: v for key, v in enhance_kwargs.items()
          if key in ("n_steps", "epsilon", "keep_rms", "warm_start", "use_aux_signal") and v is not None}
    rows = audio if audio.ndim == 2 else audio[None, :]
    n = max(1, int(round(args.stream * model.fs)))
    with model.stream(channels=rows.shape[0], segment_s=args.segment_seconds, overlap_s=ov,
                      seed=(args.seed + k) & ((1 << 63) - 1), **kw) as st:
        parts = [st.push(rows[:, i:i + n]) for i in range(0, rows.shape[1], n)]
        parts.append(st.flush(flat=False))
    enh = torch.cat(parts, dim=1)
    return enh if audio.ndim == 2 else enh[0]


def check_noise_args(args, enhance_kwargs):
    """--noise counter: refused with what it cannot be combined with."""
    if args.noise != "counter":
        return
    if enhance_kwargs.get("target") is not None:
        raise ValueError("--noise counter cannot be combined with --target (the oracle-score path draws from a generator)")
    if args.per_file_seed:
        raise ValueError("--per-file-seed selects generator seeds: with --noise counter file k is stream k of --seed already")
    if args.seed < 0:
        raise ValueError("--noise counter takes a non-negative --seed (it is the 64-bit key)")


def file_noise(args, k):
    """--noise counter: the source of file k of the sorted list -- key --seed, stream k -- whatever process, batch, lane or
    window the file ends up in (noise.plan_streams)."""
    from ..noise import plan_streams

    return plan_streams(k + 1, args.seed, [k])[k]


def enhance_file(model, audio, args, enhance_kwargs, rng):
    """One file of the serial loop: `enhance`, or `enhance_long` when --segment-seconds is set and the file is longer; with
    --segment-ensemble E every file goes through `enhance_long_ensemble` (a short file is one window)."""
    if args.segment_seconds is not None and getattr(args, "segment_ensemble", None) is not None:
        ov = 1.0 if args.segment_overlap is None else args.segment_overlap
        kw = {k: v for k, v in enhance_kwargs.items() if k in ("n_steps", "epsilon", "keep_rms") and v is not None}
        return model.enhance_long_ensemble(audio, args.segment_ensemble, enhance_kwargs.get("ensemble_stat") or "median",
                                           segment_s=args.segment_seconds, overlap_s=ov, rng=rng, **kw)
    if args.segment_seconds is not None and audio.shape[-1] > args.segment_seconds * model.fs:
        ov = 1.0 if args.segment_overlap is None else args.segment_overlap
        kw = {k: v for k, v in enhance_kwargs.items() if k in ("n_steps", "epsilon", "keep_rms")}
        if enhance_kwargs.get("warm_start") is not None:
            kw["warm_start"] = enhance_kwargs["warm_start"]
        if enhance_kwargs.get("use_aux_signal"):
            kw["use_aux_signal"] = True
        return model.enhance_long(audio, segment_s=args.segment_seconds, overlap_s=ov, rng=rng, **kw)
    try:
        return model.enhance(audio, **dict(enhance_kwargs, rng=rng))
    except ValueError as e:
        if "ou_enhance_segments" in str(e):
            raise ValueError(f"{e} -- this file is too long for one pass: run with --segment-seconds (e.g. 8)") from e
        raise


def main(argv=None, model=None):
    """`model`: an already-loaded model (tests); otherwise --model is loaded like the reference does."""
    argv = list(sys.argv[1:] if argv is None else argv)
    parser = build_parser()
    requires_help = handle_help(argv)
    args, _ = parser.parse_known_args(argv)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if model is None:
        device = args.device
        if world > 1:
            # one GPU per rank; ranks wrap around the visible devices when there are fewer GPUs than ranks
            device = f"cuda:{int(os.environ.get('LOCAL_RANK', rank)) % max(1, torch.cuda.device_count())}"
        if not device.startswith("cuda"):
            raise ValueError("Device name should be 'cuda:X' where X is an integer (this build has no CPU path). "
                             f"Provided {device}")
        if world > 1:
            from .. import distributed

            distributed.init()  # nccl (= RCCL) with one GPU per rank, gloo when ranks share a device
            model = inference_utils.load_model_sharded(args.model, device=device, strict=args.model_strict,
                                                       hf_token=args.hf_token)
        else:
            model = inference_utils.load_model(args.model, device=device, strict=args.model_strict,
                                               hf_token=args.hf_token)
    device = str(getattr(model, "device", args.device))

    inference_utils.add_enhance_arguments(model, parser)
    if requires_help:
        argv.append("--help")
    args = parser.parse_args(argv)
    enhance_kwargs = {}
    for group in parser._action_groups:
        if group.title == "enhance":
            enhance_kwargs = {a.dest: getattr(args, a.dest, None) for a in group._group_actions}

    check_stream_args(args, enhance_kwargs)
    check_segment_args(args, enhance_kwargs)
    check_noise_args(args, enhance_kwargs)
    if args.pad_batch and enhance_kwargs.get("ensemble") is not None:
        raise ValueError("--pad-batch cannot be combined with --ensemble (ensembles are batched exactly)")
    counter = args.noise == "counter"
    files, rel_path, dir_proc = find_files(args.input)
    # (counter mode: the file index is part of the noise function -- nothing to force for sharded runs, nothing to re-draw)
    per_file_seed = (args.per_file_seed or world > 1) and not counter
    rng = torch.Generator(device=device)
    rng.manual_seed(args.seed)

    undecodable = [str(p) for p in files if not can_decode(p)]
    if undecodable:
        # fail before the first file is enhanced, not in the middle of a directory (torchaudio is what the reference
        # decodes .mp3 / .flac with, bin/enhance.py:183)
        raise RuntimeError(f"{len(undecodable)} input file(s) need torchaudio to be decoded (.wav and .flac are read natively): "
                           + ", ".join(undecodable[:5]))
    todo = plan_files(files, world, rank)

    def out_path(path):
        if dir_proc:
            output_path = args.output / path.relative_to(rel_path)
            output_path.parent.mkdir(exist_ok=True, parents=True)
            return output_path
        if args.output.is_dir():
            return args.output / path.name
        return args.output

    done = []

    def write(outputs):
        """outputs: list of (output_path, enhanced tensor on the device, fs), written in this order"""
        if args.encoder == "library":
            flac = [o for o in outputs if Path(o[0]).suffix.lower() == ".flac"]
            for fs in dict.fromkeys(o[2] for o in flac):  # one encoder call per sample rate
                grp = [o for o in flac if o[2] == fs]
                save_flac_many([o[0] for o in grp], [o[1] for o in grp], fs, level=args.flac_level)
            outputs_host = [o for o in outputs if Path(o[0]).suffix.lower() != ".flac"]
        else:
            outputs_host = outputs
        for output_path, enh, fs in outputs_host:
            save(output_path, enh.cpu(), fs, flac_level=args.flac_level)
        done.extend(o[0] for o in outputs)

    if args.stream is not None:
        # --stream: one streaming session per file, fed in chunks; what the pushes and the flush return is the file's output
        for k, path in todo:
            audio, fs = load(path)
            with torch.no_grad():
                x = resample(audio.to(device), fs, model.fs, backend=args.resampler)
                enh = resample(stream_file(model, x, args, enhance_kwargs, k), model.fs, fs, backend=args.resampler)
            write([(out_path(path), enh, fs)])
        return done
    if args.batch_size <= 1 and args.in_flight > 1 and enhance_kwargs.get("target") is None \
            and getattr(model, "fork", None) is not None:
        # The serial loop below with K calls in flight: file k + K is read, resampled and enqueued while files k .. k + K - 1
        # are still on the device; a file is written when its lane comes round again.  The noise is drawn at enqueue time
        # in processing order, so the shared generator advances exactly as in the serial loop.
        from ..lanes import LanePool

        def finish(item):
            lane, output_path, enh, fs = item
            pool.wait(lane)
            write([(output_path, enh, fs)])

        # one call per file, batch size = its channel count: files that differ there put calls of different sizes in flight,
        # and the lanes then have to agree on how their GRU clusters share the device (headers only are read here)
        chans = {channels(path) for _, path in todo}
        mb = max(chans, default=1)
        with LanePool(model, min(int(args.in_flight), LanePool.MAX_LANES),
                      max_batch=mb if (len(chans) > 1 or mb > 1) else 0) as pool:
            pending = []
            for k, path in todo:
                output_path = out_path(path)
                audio, fs = load(path)
                audio = audio.to(device)
                if counter:
                    file_rng = file_noise(args, k)
                elif per_file_seed:
                    # a generator of its own per file: the draws of a call in flight must not see the next file's re-seed
                    file_rng = torch.Generator(device=device)
                    file_rng.manual_seed(args.seed + k)
                else:
                    file_rng = rng
                if len(pending) >= pool.lanes:
                    finish(pending.pop(0))

                def work(m, audio=audio, fs=fs, file_rng=file_rng):
                    with torch.no_grad():
                        x = resample(audio, fs, m.fs, backend=args.resampler)
                        return resample(m.enhance(x, **dict(enhance_kwargs, rng=file_rng)), m.fs, fs,
                                        backend=args.resampler)

                lane, enh = pool.submit(work, audio)
                pending.append((lane, output_path, enh, fs))
            for item in pending:
                finish(item)
        return done
    if args.segment_seconds is not None and args.segment_files > 1:
        # --segment-files N: N consecutive files per enhance_long_many call.  Every file gets the generator or counter source
        # the serial loop below would hand it (the shared generator advances file by file inside the call, in input order).
        ov = 1.0 if args.segment_overlap is None else args.segment_overlap
        kw = {key: v for key, v in enhance_kwargs.items() if key in ("n_steps", "epsilon", "keep_rms")}
        for g0 in range(0, len(todo), args.segment_files):
            grp = todo[g0:g0 + args.segment_files]
            with torch.no_grad():
                sigs, rates, rngs = [], [], []
                for k, path in grp:
                    audio, fs = load(path)
                    sigs.append(resample(audio.to(device), fs, model.fs, backend=args.resampler))
                    rates.append(fs)
                    if counter:
                        rngs.append(file_noise(args, k))
                    elif per_file_seed:
                        file_rng = torch.Generator(device=device)
                        file_rng.manual_seed(args.seed + k)
                        rngs.append(file_rng)
                enhs = model.enhance_long_many(sigs, rngs if rngs else rng, segment_s=args.segment_seconds, overlap_s=ov, **kw)
                outs = [resample(e, model.fs, fs, backend=args.resampler) for e, fs in zip(enhs, rates)]
            write([(out_path(path), enh, fs) for (k, path), enh, fs in zip(grp, outs, rates)])
        return done
    if args.segment_seconds is not None and getattr(args, "segment_ensemble_files", 1) > 1:
        # --segment-ensemble-files N: up to N consecutive files of one sample rate per enhance_long_many_ensemble call.  Every file
        # gets the generator or counter source the serial loop below would hand it (the shared generator advances file by file
        # inside the call, in input order).
        ov = 1.0 if args.segment_overlap is None else args.segment_overlap
        kw = {key: v for key, v in enhance_kwargs.items() if key in ("n_steps", "epsilon", "keep_rms") and v is not None}
        stat = enhance_kwargs.get("ensemble_stat") or "median"

        def run_group(grp):
            """grp: list of (k, path, audio at the model's rate, fs), one fs"""
            with torch.no_grad():
                rngs = []
                for k, _, _, _ in grp:
                    if counter:
                        rngs.append(file_noise(args, k))
                    elif per_file_seed:
                        file_rng = torch.Generator(device=device)
                        file_rng.manual_seed(args.seed + k)
                        rngs.append(file_rng)
                enhs = model.enhance_long_many_ensemble([a for _, _, a, _ in grp], args.segment_ensemble, stat,
                                                        rngs=rngs if rngs else rng, segment_s=args.segment_seconds,
                                                        overlap_s=ov, **kw)
                outs = [resample(e, model.fs, fs, backend=args.resampler) for e, (_, _, _, fs) in zip(enhs, grp)]
            write([(out_path(path), enh, fs) for (_, path, _, fs), enh in zip(grp, outs)])

        grp = []
        for k, path in todo:
            audio, fs = load(path)
            if grp and (fs != grp[0][3] or len(grp) >= args.segment_ensemble_files):  # a new sample rate ends a group
                run_group(grp)
                grp = []
            with torch.no_grad():
                grp.append((k, path, resample(audio.to(device), fs, model.fs, backend=args.resampler), fs))
        if grp:
            run_group(grp)
        return done
    if args.batch_size <= 1:
        for k, path in todo:
            output_path = out_path(path)
            audio, fs = load(path)
            audio = audio.to(device)
            if per_file_seed:
                rng.manual_seed(args.seed + k)
            with torch.no_grad():
                audio = resample(audio, fs, model.fs, backend=args.resampler)
                enh = enhance_file(model, audio, args, enhance_kwargs, file_noise(args, k) if counter else rng)
                enh = resample(enh, model.fs, fs, backend=args.resampler)
            write([(output_path, enh, fs)])
        return done

    # --batch-size: files are read in processing order into a window (one sample rate, --batch-window files), sorted by length
    # inside it and enhanced batch_size at a time
    if enhance_kwargs.get("target") is not None:
        raise ValueError("--batch-size cannot be combined with --target (one call per file needed)")
    # --ensemble E --batch-size K: every group is one enhance_many(ensemble=E) call (exact batching; the members are reduced
    # inside the library)
    ensemble = enhance_kwargs.get("ensemble")
    drop = ("rng", "target", "fake_score_snr") + (("ensemble", "ensemble_stat") if ensemble is None else ())
    kw = {key: v for key, v in enhance_kwargs.items() if key not in drop}

    window_size = max(1, args.batch_window if args.batch_window > 0 else 4 * args.batch_size)
    # Sorting a window by length needs a generator per file that starts where the serial loop's shared generator would stand
    # in front of that file: with per-file seeds by construction, with the shared generator by taking its state file by file
    # in processing order and advancing it by the file's draws (Universe.advance_generator_like_enhance).
    can_sort = counter or per_file_seed or hasattr(model, "advance_generator_like_enhance")
    if not can_sort:
        window_size = min(window_size, args.batch_size)

    def flush(window):
        """window: list of (k, path, audio, fs) with one fs, in processing order"""
        if not window:
            return
        fs = window[0][3]
        with torch.no_grad():
            items = []
            # (library resampler: the whole window in one launch; torch: file by file, as before)
            sigs = resample_many([a.to(device) for _, _, a, _ in window], fs, model.fs, backend=args.resampler)
            for (k, path, _, _), sig in zip(window, sigs):
                if counter:
                    g = file_noise(args, k)
                elif per_file_seed:
                    g = torch.Generator(device=device)
                    g.manual_seed(args.seed + k)
                elif can_sort:
                    g = torch.Generator(device=device)
                    g.set_state(rng.get_state())
                    # (with --ensemble E a file draws for its E * channels member rows)
                    model.advance_generator_like_enhance(rng, (sig.shape[0] if sig.ndim == 2 else 1) * int(ensemble or 1),
                                                         sig.shape[-1],
                                                         n_steps=kw.get("n_steps"), warm_start=kw.get("warm_start"),
                                                         use_aux_signal=bool(kw.get("use_aux_signal")))
                else:
                    g = None  # (a model without the hook: consecutive files, the shared generator drawn from in order)
                items.append((k, path, sig, g))
            order = sorted(range(len(items)), key=lambda i: (-items[i][2].shape[-1], i)) if can_sort else list(range(len(items)))
            results = {}
            for b0 in range(0, len(order), args.batch_size):
                grp = [items[i] for i in order[b0:b0 + args.batch_size]]
                rngs = [g for _, _, _, g in grp] if can_sort else rng
                enhs = model.enhance_many([sig for _, _, sig, _ in grp], rngs, pad_batch=args.pad_batch, **kw)
                outs = resample_many(list(enhs), model.fs, fs, backend=args.resampler)
                for (k, _, _, _), e in zip(grp, outs):
                    results[k] = e
        write([(out_path(path), results[k], fs) for k, path, _, _ in window])  # written in processing order

    window = []
    for k, path in todo:
        audio, fs = load(path)
        if window and (fs != window[0][3] or len(window) >= window_size):
            flush(window)
            window = []
        window.append((k, path, audio, fs))
    flush(window)
    return done


if __name__ == "__main__":
    main()
