"""
Scores of enhanced speech on the device: log-spectral distance (LSD, SI-LSD), SI-SDR, SNR, the BSS-eval SDR, STOI and extended
STOI, and the time-domain + multi-resolution spectral L1, through ou_lsd / ou_si_sdr / ou_sdr / ou_stoi / ou_spectral_mae of
the C ABI (include/ouniverse.h, "scoring").

Names and defaults follow the reference: `log_spectral_distance` / `LogSpectralDistance` (open_universe/metrics/lsd.py),
`Metrics` (metrics/wrapper.py), `MultiResL1SpecLoss` (losses/multires_stft.py).  Every function takes tensors on a HIP device
(there is no CPU path and no fallback) and returns one score per row; `evaluate_many` packs pairs of any lengths into one call
per metric, every row scored as if it were alone.  These are scores: nothing here is differentiable.

What the kernels do not cover raises NotImplementedError naming the argument (p != 2, a custom window, win_length != n_fft,
pad != 0); the metrics of the reference that need a model or a package (pesq-*, lps, dnsmos, plcmos) are refused by name.
`sdr` is computed here (`sdr`, and `evaluate_many` / bin/eval_metrics when it is named) from its definition: the package the
reference asks for it (fast_bss_eval) is not a dependency.  `Metrics` keeps the four names it had and refuses `sdr`.

`stoi` and `stoi-ext` are computed here too, from their definition (include/ouniverse.h; pystoi, which the reference asks, is
not a dependency): by `stoi(input, target, fs, extended)`, and by `evaluate_many(..., intelligibility=[...])` /
`eval_metrics --intelligibility` when they are named there (INTELLIGIBILITY_METRICS).  As names of `Metrics`, of
`check_metric_names` / `check_score_names` and of the `metrics=` argument they remain refused, with the message they always
had: one list of names for all scores is left to a later change.
"""
import ctypes

import torch

from . import _lib

#: metrics this module computes ("snr" is an extension: the plain signal-to-noise ratio with the clamp of si-sdr)
AVAILABLE_METRICS = ("lsd", "si-lsd", "si-sdr", "snr")
#: metrics `evaluate_many` and bin/eval_metrics compute when they are named explicitly (never by default, never by `Metrics`)
OPTIONAL_METRICS = ("sdr",)
#: the scores `stoi` computes; `evaluate_many(intelligibility=...)` and `eval_metrics --intelligibility` take these names
INTELLIGIBILITY_METRICS = ("stoi", "stoi-ext")
#: metrics of the reference (metrics/wrapper.py) that `Metrics` and `metrics=` refuse by name.  pesq-*, lps, dnsmos and plcmos
#: need an external model or package; `sdr` (OPTIONAL_METRICS) and `stoi` / `stoi-ext` (INTELLIGIBILITY_METRICS) are computed by
#: this module through entry points of their own and stay in this list only because those two callers keep their refusals
EXTERNAL_METRICS = ("pesq-wb", "pesq-nb", "stoi", "stoi-ext", "lps", "dnsmos", "plcmos", "sdr")
#: the filter length and clamp of the reference's `Metrics.sdr` (metrics/wrapper.py:179-195)
SDR_FILTER_LENGTH, SDR_CLAMP_DB = 512, 100.0


def _spec(n_fft, hop, eps=0.0, flags=0):
    return _lib.MetricsSpec(int(n_fft), int(hop), float(eps), int(flags))


def _specs_array(specs):
    return (_lib.MetricsSpec * max(len(specs), 1))(*specs)


def scratch_bytes(B, T_max, specs=()):
    """ou_metrics_scratch_bytes: pure host code; ValueError for a resolution the kernels refuse (n_fft odd or above the cap, hop < 1)."""
    L = _lib.load()
    n = ctypes.c_size_t()
    specs = list(specs)
    _lib.check(L.ou_metrics_scratch_bytes(int(B), int(T_max), _specs_array(specs) if specs else None, len(specs), ctypes.byref(n)))
    return n.value


def frames(T, hop):
    """ou_metrics_frames: frames of the centred STFT of T samples."""
    return int(_lib.load().ou_metrics_frames(int(T), int(hop)))


def _flatten(input, target, who):
    if input.shape != target.shape:
        raise ValueError(f"{who}: the shapes of the inputs should match, got {tuple(input.shape)} and {tuple(target.shape)}")
    if input.ndim < 1 or input.shape[-1] < 1:
        raise ValueError(f"{who}: the inputs need at least one sample")
    batch = input.shape[:-1]
    return input.reshape(-1, input.shape[-1]), target.reshape(-1, target.shape[-1]), batch


def _device_rows(x, y, who):
    if x.device.type != "cuda" or y.device != x.device:
        raise ValueError(f"{who} runs on a HIP device only: move both tensors to one (there is no CPU path and no fallback)")
    x = x.to(torch.float32)
    y = y.to(torch.float32)
    if x.stride(-1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    if y.stride(-1) != 1 or y.stride(0) != x.stride(0):
        y2 = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=x.device)
        y2.copy_(y)
        y = y2
    return x, y


class _Call:
    """Pointers of one ABI call on rows x, y (B, stride) with the lengths `lens`."""

    def __init__(self, x, y, lens, specs, nbytes=None):
        self.B = x.shape[0]
        self.lens = (ctypes.c_int64 * self.B)(*[int(n) for n in lens])
        self.x, self.y = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr())
        self.stride = int(x.stride(0)) if self.B > 1 else max(int(x.stride(0)), int(x.shape[1]))
        self.nbytes = scratch_bytes(self.B, max(int(n) for n in lens), specs) if nbytes is None else nbytes
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=x.device)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)

    def out(self, device):
        return torch.empty(self.B, dtype=torch.float32, device=device)


def _lsd_rows(x, y, lens, n_fft, hop, eps, scale_invariant, db):
    flags = (_lib.OU_MET_SCALE_INVARIANT if scale_invariant else 0) | (0 if db else _lib.OU_MET_NATURAL_LOG)
    spec = _spec(n_fft, hop, eps, flags)
    scratch_bytes(1, 1, [spec])  # the refusals of the resolution, before anything else
    short = [int(n) for n in lens if int(n) <= int(n_fft) // 2]
    if short:
        raise ValueError(f"log_spectral_distance: a signal of {short[0]} samples must exceed n_fft / 2 = {int(n_fft) // 2} "
                         "(the reflect padding of the centred STFT is undefined otherwise)")
    x, y = _device_rows(x, y, "log_spectral_distance")
    L = _lib.load()
    with torch.cuda.device(x.device):
        c = _Call(x, y, lens, [spec])
        out = c.out(x.device)
        _lib.check(L.ou_lsd(c.x, c.y, c.stride, c.lens, c.B, ctypes.byref(spec), ctypes.c_void_p(out.data_ptr()),
                            ctypes.c_void_p(c.scratch.data_ptr()), ctypes.c_size_t(c.nbytes), c.stream))
    return out


def _sdr_rows(x, y, lens, clamp_db):
    if not (float(clamp_db) > 0.0 and float(clamp_db) < float("inf")):
        raise ValueError(f"si_sdr / snr: clamp_db = {clamp_db!r} must be positive and finite")
    x, y = _device_rows(x, y, "si_sdr / snr")
    L = _lib.load()
    with torch.cuda.device(x.device):
        c = _Call(x, y, lens, [])
        a, b = c.out(x.device), c.out(x.device)
        _lib.check(L.ou_si_sdr(c.x, c.y, c.stride, c.lens, c.B, float(clamp_db), ctypes.c_void_p(a.data_ptr()),
                               ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(c.scratch.data_ptr()), ctypes.c_size_t(c.nbytes),
                               c.stream))
    return a, b


def sdr_scratch_bytes(B, T_max, filter_length=SDR_FILTER_LENGTH):
    """ou_sdr_scratch_bytes: pure host code; ValueError for a filter_length outside 1 .. 512."""
    n = ctypes.c_size_t()
    _lib.check(_lib.load().ou_sdr_scratch_bytes(int(B), int(T_max), int(filter_length), ctypes.byref(n)))
    return n.value


def _bss_sdr_rows(x, y, lens, filter_length, clamp_db):
    if int(filter_length) != filter_length:
        raise ValueError(f"sdr: filter_length = {filter_length!r} must be an integer")
    sdr_scratch_bytes(1, 1, filter_length)  # the refusal of the filter length, before anything else
    if not (float(clamp_db) > 0.0 and float(clamp_db) < float("inf")):
        raise ValueError(f"sdr: clamp_db = {clamp_db!r} must be positive and finite")
    x, y = _device_rows(x, y, "sdr")
    L = _lib.load()
    with torch.cuda.device(x.device):
        c = _Call(x, y, lens, [], sdr_scratch_bytes(x.shape[0], max(int(n) for n in lens), filter_length))
        out = c.out(x.device)
        _lib.check(L.ou_sdr(c.x, c.y, c.stride, c.lens, c.B, int(filter_length), float(clamp_db), ctypes.c_void_p(out.data_ptr()),
                            ctypes.c_void_p(c.scratch.data_ptr()), ctypes.c_size_t(c.nbytes), c.stream))
    return out


def stoi_scratch_bytes(B, T_max, fs):
    """ou_stoi_scratch_bytes: pure host code; ValueError for fs < 1 and for an fs whose 10 kHz resampling filter exceeds the caps
    of include/ouniverse.h (OU_STOI_MAX_TAPS, OU_STOI_MAX_TABLE_BYTES)."""
    n = ctypes.c_size_t()
    _lib.check(_lib.load().ou_stoi_scratch_bytes(int(B), int(T_max), int(fs), ctypes.byref(n)))
    return n.value


def _stoi_rows(x, y, lens, fs, extended):
    if int(fs) != fs:
        raise ValueError(f"stoi: fs = {fs!r} must be an integer")
    stoi_scratch_bytes(1, 1, fs)  # the refusal of the rate, before anything else
    x, y = _device_rows(x, y, "stoi")
    L = _lib.load()
    with torch.cuda.device(x.device):
        c = _Call(x, y, lens, [], stoi_scratch_bytes(x.shape[0], max(int(n) for n in lens), fs))
        out = c.out(x.device)
        _lib.check(L.ou_stoi(c.x, c.y, c.stride, c.lens, c.B, int(fs), 1 if extended else 0, ctypes.c_void_p(out.data_ptr()),
                             ctypes.c_void_p(c.scratch.data_ptr()), ctypes.c_size_t(c.nbytes), c.stream))
    return out


def _l1_rows(x, y, lens, window_sz, hop_sz, eps, time_domain_weight, scale_invariant):
    specs = [_spec(w, h) for w, h in zip(window_sz, hop_sz)]
    if len(specs) > _lib.OU_METRICS_MAX_SPECS:
        raise ValueError(f"MultiResL1SpecLoss: at most {_lib.OU_METRICS_MAX_SPECS} resolutions, got {len(specs)}")
    scratch_bytes(1, 1, specs)
    x, y = _device_rows(x, y, "MultiResL1SpecLoss")
    L = _lib.load()
    with torch.cuda.device(x.device):
        c = _Call(x, y, lens, specs)
        out = c.out(x.device)
        _lib.check(L.ou_spectral_mae(c.x, c.y, c.stride, c.lens, c.B, _specs_array(specs) if specs else None, len(specs),
                                    float(time_domain_weight), float(eps), _lib.OU_MET_SCALE_INVARIANT if scale_invariant else 0,
                                    ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(c.scratch.data_ptr()),
                                    ctypes.c_size_t(c.nbytes), c.stream))
    return out


def _lsd_unsupported(p, n_fft, win_length, window, pad, stft_kwargs):
    if p is None or p <= 0:
        raise ValueError(f"p must be a positive number, but got p={p}")  # lsd.py:92-93
    if p != 2:
        raise NotImplementedError(f"log_spectral_distance: p={p!r} is not implemented (the kernel computes p=2)")
    if window is not None:
        raise NotImplementedError("log_spectral_distance: a custom window is not implemented (the kernel applies the periodic Hann "
                                  "window of n_fft points)")
    if win_length is not None and int(win_length) != int(n_fft):
        raise NotImplementedError(f"log_spectral_distance: win_length={win_length!r} != n_fft={n_fft!r} is not implemented")
    if pad != 0:
        raise NotImplementedError(f"log_spectral_distance: pad={pad!r} is not implemented (pad=0 only)")
    if stft_kwargs:
        raise NotImplementedError(f"log_spectral_distance: the STFT arguments {sorted(stft_kwargs)} are not implemented")


def log_spectral_distance(input, target, p=2, db=True, n_fft=400, hop_length=160, eps=1e-7, win_length=None, window=None, pad=0,
                          scale_invariant=False, **stft_kwargs):
    """metrics/lsd.py:27-140 on the device: input, target [..., T] -> [...].  With `scale_invariant` the target is rescaled by
    sum(input target) / (sum(input^2) + eps) first."""
    _lsd_unsupported(p, n_fft, win_length, window, pad, stft_kwargs)
    x, y, batch = _flatten(input, target, "log_spectral_distance")
    return _lsd_rows(x, y, [x.shape[1]] * x.shape[0], n_fft, hop_length, eps, scale_invariant, db).reshape(batch)


class LogSpectralDistance(torch.nn.Module):
    """metrics/lsd.py:143-202 (its `eps` defaults to 1e-5, unlike the function's 1e-7)."""

    def __init__(self, p=2, db=True, n_fft=400, hop_length=160, win_length=None, window=None, pad=0, eps=1e-5, reduction="mean",
                 scale_invariant=False, **stft_kwargs):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("Only reduction=mean|sum|none are supported")
        _lsd_unsupported(p, n_fft, win_length, window, pad, stft_kwargs)
        self.p, self.db, self.n_fft, self.hop_length, self.eps = p, db, n_fft, hop_length, eps
        self.reduction, self.scale_invariant = reduction, scale_invariant

    def forward(self, input, target):
        dist = log_spectral_distance(input, target, p=self.p, db=self.db, n_fft=self.n_fft, hop_length=self.hop_length,
                                     eps=self.eps, scale_invariant=self.scale_invariant)
        if self.reduction == "mean":
            return dist.mean()
        if self.reduction == "sum":
            return dist.sum()
        return dist


class MultiResL1SpecLoss(torch.nn.Module):
    """losses/multires_stft.py:22-129 as a score: `forward(target, estimate)` -> the mean over the batch, `per_row` -> (B,)."""

    def __init__(self, window_sz=(512,), hop_sz=None, eps=1e-8, time_domain_weight=0.5, scale_invariant=False):
        super().__init__()
        window_sz = [int(w) for w in window_sz]
        assert all(w % 2 == 0 for w in window_sz)  # multires_stft.py:53
        self.window_sz = window_sz
        self.hop_sz = [w // 2 for w in window_sz] if hop_sz is None else [int(h) for h in hop_sz]
        if len(self.hop_sz) != len(self.window_sz):
            raise ValueError("MultiResL1SpecLoss: hop_sz needs one entry per window_sz")
        self.eps, self.time_domain_weight, self.scale_invariant = eps, time_domain_weight, scale_invariant

    def per_row(self, target, estimate, lengths=None):
        """(B, T) each -> (B,); `lengths`: the rows' own lengths (default: T for every row)."""
        assert target.shape == estimate.shape, (target.shape, estimate.shape)
        x, y, batch = _flatten(estimate, target, "MultiResL1SpecLoss")
        lens = [x.shape[1]] * x.shape[0] if lengths is None else [int(n) for n in lengths]
        return _l1_rows(x, y, lens, self.window_sz, self.hop_sz, self.eps, self.time_domain_weight,
                        self.scale_invariant).reshape(batch)

    def forward(self, target, estimate):
        return self.per_row(target, estimate).mean()


def si_sdr(input, target, clamp_db=100.0):
    """Scale-invariant SDR of `input` against `target` [..., T] -> [...], as metrics/wrapper.py:197-213 computes it
    (zero_mean=False, clamped to +-clamp_db)."""
    x, y, batch = _flatten(input, target, "si_sdr")
    return _sdr_rows(x, y, [x.shape[1]] * x.shape[0], clamp_db)[0].reshape(batch)


def snr(input, target, clamp_db=100.0):
    """10 log10(sum target^2 / sum (input - target)^2) [..., T] -> [...], with the clamp of `si_sdr`."""
    x, y, batch = _flatten(input, target, "snr")
    return _sdr_rows(x, y, [x.shape[1]] * x.shape[0], clamp_db)[1].reshape(batch)


def sdr(input, target, filter_length=SDR_FILTER_LENGTH, clamp_db=SDR_CLAMP_DB):
    """BSS-eval SDR of `input` against `target` [..., T] -> [...] with a distortion filter of `filter_length` taps (1 .. 512), as
    metrics/wrapper.py:179-195 asks fast_bss_eval for it (zero_mean=False, clamped to +-clamp_db): the share of `input` that lies
    in the span of `target` delayed by 0 .. filter_length - 1 samples, against the rest.  filter_length=1 is `si_sdr`."""
    x, y, batch = _flatten(input, target, "sdr")
    return _bss_sdr_rows(x, y, [x.shape[1]] * x.shape[0], filter_length, clamp_db).reshape(batch)


def stoi(input, target, fs, extended=False):
    """STOI (extended=False) or extended STOI of the estimate `input` against the clean `target` [..., T] -> [...], both at rate
    `fs`, from the definition in include/ouniverse.h (resampling to 10 kHz, silent-frame removal, one-third-octave bands,
    30-frame segments), as metrics/wrapper.py:116-128 asks pystoi for them.  A signal that ends with fewer than 30 frames
    scores 1e-5."""
    x, y, batch = _flatten(input, target, "stoi")
    return _stoi_rows(x, y, [x.shape[1]] * x.shape[0], fs, extended).reshape(batch)


def check_intelligibility_names(names):
    """The names `evaluate_many(intelligibility=...)` accepts, in order; ValueError for any other."""
    out = list(names or ())
    for n in out:
        if n not in INTELLIGIBILITY_METRICS:
            raise ValueError(f"intelligibility: {n!r} is not one of {', '.join(INTELLIGIBILITY_METRICS)}")
    return out


def check_metric_names(metrics):
    """The names `Metrics` accepts, in order; NotImplementedError for any other (metrics/wrapper.py:76-79)."""
    out = []
    for met in AVAILABLE_METRICS if metrics is None else metrics:
        if met in OPTIONAL_METRICS:
            raise NotImplementedError(f"Metric {met} is not supported by Metrics, which keeps to {', '.join(AVAILABLE_METRICS)}: "
                                      f"call metrics.{met}, or name it in evaluate_many(metrics=[...]) / eval_metrics --metrics")
        if met in EXTERNAL_METRICS:
            raise NotImplementedError(f"Metric {met} is not supported: it needs a model or a package that this library does not "
                                      f"carry (available: {', '.join(AVAILABLE_METRICS)})")
        if met not in AVAILABLE_METRICS:
            raise NotImplementedError(f"Metric {met} is not supported")
        out.append(met)
    return out


def check_score_names(metrics):
    """The names `evaluate_many` and bin/eval_metrics accept, in order: those of `Metrics` and, named explicitly, OPTIONAL_METRICS
    (None: the defaults of `Metrics`)."""
    if metrics is None:
        return check_metric_names(None)
    return [met if met in OPTIONAL_METRICS else check_metric_names([met])[0] for met in metrics]


def stft_setting(fs):
    """(n_fft, hop) of the LSD at sampling rate fs: 25 ms and 10 ms (metrics/wrapper.py:134-136)."""
    return int(0.025 * fs), int(0.01 * fs)


def pack_pairs(est_list, ref_list, device=None):
    """Pairs of 1-D signals of any lengths -> (est (B, stride), ref (B, stride), lengths): the shorter signal of a pair is
    zero-padded to the longer (metrics/wrapper.py:243-246), row b holds pair b in its first lengths[b] columns, the rest is 0."""
    est_list, ref_list = list(est_list), list(ref_list)
    if len(est_list) != len(ref_list):
        raise ValueError(f"evaluate_many: {len(est_list)} estimates for {len(ref_list)} references")
    if not est_list:
        raise ValueError("evaluate_many: no signals")
    for s in est_list + ref_list:
        if s.ndim != 1 or s.shape[0] < 1:
            raise ValueError("evaluate_many: signals are 1-D tensors with at least one sample")
    device = est_list[0].device if device is None else device
    lens = [max(int(e.shape[0]), int(r.shape[0])) for e, r in zip(est_list, ref_list)]
    stride = (max(lens) + 3) // 4 * 4
    x = torch.zeros((len(lens), stride), dtype=torch.float32, device=device)
    y = torch.zeros((len(lens), stride), dtype=torch.float32, device=device)
    for b, (e, r) in enumerate(zip(est_list, ref_list)):
        x[b, :e.shape[0]] = e.to(device=device, dtype=torch.float32)
        y[b, :r.shape[0]] = r.to(device=device, dtype=torch.float32)
    return x, y, lens


def unpack_scores(names, columns, n):
    """{name: (n,) sequence} -> n dicts {name: float}, names in the order asked for."""
    return [{name: float(columns[name][b]) for name in names} for b in range(n)]


def _score_rows(names, x, y, lens, fs):
    n_fft, hop = stft_setting(fs)
    cols = {}
    if "lsd" in names:
        cols["lsd"] = _lsd_rows(x, y, lens, n_fft, hop, 1e-7, False, True)
    if "si-lsd" in names:
        cols["si-lsd"] = _lsd_rows(x, y, lens, n_fft, hop, 1e-7, True, True)
    if "si-sdr" in names or "snr" in names:
        a, b = _sdr_rows(x, y, lens, 100.0)
        cols["si-sdr"], cols["snr"] = a, b
    if "sdr" in names:
        cols["sdr"] = _bss_sdr_rows(x, y, lens, SDR_FILTER_LENGTH, SDR_CLAMP_DB)
    return {k: v.tolist() for k, v in cols.items() if k in names}  # (the one host synchronisation per metric)


def evaluate_many(est_list, ref_list, fs, metrics=None, intelligibility=()):
    """Score pairs (estimate, reference) of 1-D signals of any lengths at rate fs: ONE library call per metric over all pairs,
    every pair scored as `Metrics(metrics)(fs, est, ref)` scores it alone.  -> one dict per pair.  `metrics` may also name
    "sdr" (OPTIONAL_METRICS): the BSS-eval SDR as `sdr` computes it, one ou_sdr call over all pairs.  `intelligibility` names
    scores of INTELLIGIBILITY_METRICS ("stoi", "stoi-ext"): their columns follow the others, one ou_stoi call per name over all
    pairs; anything else there is a ValueError."""
    names = check_score_names(metrics)
    extra = check_intelligibility_names(intelligibility)
    x, y, lens = pack_pairs(est_list, ref_list)
    cols = _score_rows(names, x, y, lens, fs)
    for name in extra:
        cols[name] = _stoi_rows(x, y, lens, fs, name == "stoi-ext").tolist()
    return unpack_scores(names + [n for n in extra if n not in names], cols, len(lens))


class Metrics:
    """metrics/wrapper.py:54-281 for the metrics this library computes: lsd, si-lsd, si-sdr (and snr)."""

    @classmethod
    def get_metric_names(cls):
        return list(AVAILABLE_METRICS)

    def __init__(self, metrics=None):
        self.metrics = check_metric_names(metrics)

    def __call__(self, fs, degraded, reference=None, skip_list=None, skip_unknown_metrics=True):
        """degraded, reference: (T,) or (B, T); the shorter is zero-padded to the longer.  -> dict, or list of dicts for 2-D
        input.  Without a reference nothing here can be computed: every metric of this class is intrusive ({} per signal)."""
        if degraded.ndim > 2 or degraded.ndim < 1:
            raise ValueError("The input should have 1 or 2 dimensions")
        single = degraded.ndim == 1
        if reference is None:
            return {} if single else [{} for _ in range(degraded.shape[0])]
        M = max(reference.shape[-1], degraded.shape[-1])
        degraded = torch.nn.functional.pad(degraded, (0, M - degraded.shape[-1]))
        reference = torch.nn.functional.pad(reference, (0, M - reference.shape[-1]))
        if reference.shape != degraded.shape:
            raise ValueError("The shapes of the inputs should match")
        names = [m for m in self.metrics if skip_list is None or m not in skip_list]
        x, y = degraded.reshape(-1, M), reference.reshape(-1, M)
        out = unpack_scores(names, _score_rows(names, x, y, [M] * x.shape[0], fs), x.shape[0]) if names else [{}] * x.shape[0]
        return out[0] if single else out
