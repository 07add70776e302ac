"""The reference's scores restated with torch.stft, for the tests of open_universe_amd.metrics: written once from the definitions
in metrics/lsd.py (log_spectral_distance through torchaudio.functional.spectrogram: centred, reflect padding, periodic Hann,
normalized="window", power 2), losses/multires_stft.py (torchaudio.transforms.Spectrogram: centred, constant padding, periodic
Hann, magnitude, hop = window / 2) and metrics/wrapper.py:197-213 (fast_bss_eval.si_sdr with zero_mean=False and clamp_db).
Every function works in the dtype it is given -- float64 is the reference, float32 the reference's own arithmetic -- on signals
of shape (T,) or (B, T) (all rows T long: ragged batches are scored row by row)."""
import numpy as np
import torch


def signals(lengths, seed=0, fs=16000):
    """Seeded pairs (estimate, reference) of the given lengths, float32: reference = noise + two sinusoids, estimate =
    0.7 reference + 0.05 fresh noise (so the scale-invariant forms differ visibly from the plain ones)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, T in enumerate(lengths):
        t = torch.arange(T, dtype=torch.float64) / fs
        ref = 0.1 * torch.randn(T, generator=g, dtype=torch.float64) + 0.5 * torch.sin(2 * np.pi * (220.0 + 30 * i) * t) + \
            0.25 * torch.sin(2 * np.pi * (1870.0 + 110 * i) * t + 0.3)
        est = 0.7 * ref + 0.05 * torch.randn(T, generator=g, dtype=torch.float64)
        out.append((est.to(torch.float32), ref.to(torch.float32)))
    return out


def _alpha(x, y, eps):
    return torch.sum(x * y, -1, keepdim=True) / (torch.sum(x ** 2, -1, keepdim=True) + eps)


def _stft(x, n_fft, hop, pad_mode):
    w = torch.hann_window(n_fft, periodic=True, dtype=x.dtype, device=x.device)
    s = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode=pad_mode, normalized=False,
                   onesided=True, return_complex=True)
    return s, w


def lsd(est, ref, n_fft=400, hop=160, eps=1e-7, scale_invariant=False, db=True, dtype=torch.float64):
    x, y = est.to(dtype), ref.to(dtype)
    if scale_invariant:
        y = _alpha(x, y, eps) * y

    def logpower(s):
        spec, w = _stft(s, n_fft, hop, "reflect")
        p = (spec / w.pow(2).sum().sqrt()).abs().pow(2)
        return 10 * torch.log10(p + eps) if db else torch.log(p + eps)

    d = logpower(x) - logpower(y)
    return torch.norm(d, p=2, dim=(-2, -1)) / (d.shape[-1] * d.shape[-2]) ** 0.5


def spectral_l1(est, ref, window_sz, hop_sz=None, eps=1e-8, time_domain_weight=0.5, scale_invariant=False, dtype=torch.float64):
    """Per row (the reference then takes the mean over the batch)."""
    x, y = est.to(dtype), ref.to(dtype)
    if scale_invariant:
        x = x * _alpha(x, y, eps)
    td = (x - y).abs().mean(-1)
    if not window_sz:
        return td
    hop_sz = [w // 2 for w in window_sz] if hop_sz is None else hop_sz
    sp = torch.zeros_like(td)
    for w, h in zip(window_sz, hop_sz):
        sp = sp + (_stft(x, w, h, "constant")[0].abs() - _stft(y, w, h, "constant")[0].abs()).abs().mean(dim=(-2, -1))
    return td * time_domain_weight + (1 - time_domain_weight) * sp / len(window_sz)


def _clamped_db(coh, clamp_db):
    e = 10.0 ** (-clamp_db / 10.0)
    e = e / (1.0 + e)
    coh = torch.clamp(coh, min=e, max=1 - e)
    return 10.0 * torch.log10(coh / (1 - coh))


def si_sdr(est, ref, clamp_db=100.0, dtype=torch.float64):
    x, y = est.to(dtype), ref.to(dtype)
    den = (x * x).sum(-1) * (y * y).sum(-1)
    coh = torch.where(den > 0, (x * y).sum(-1) ** 2 / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    return _clamped_db(coh, clamp_db)


def snr(est, ref, clamp_db=100.0, dtype=torch.float64):
    x, y = est.to(dtype), ref.to(dtype)
    s, n = (y * y).sum(-1), ((x - y) ** 2).sum(-1)
    coh = torch.where(s + n > 0, s / torch.where(s + n > 0, s + n, torch.ones_like(s)), torch.zeros_like(s))
    return _clamped_db(coh, clamp_db)


def ulp32(v):
    """One unit in the last place of the float64 value v rounded to float32."""
    return float(np.spacing(np.abs(np.float32(v))))


def gate(lib, f64, f32):
    """(|lib - f64|, the bound 4 max(|f32 - f64|, 1 ulp of f64 in fp32), their ratio to the UNscaled max(...))."""
    own = max(abs(float(f32) - float(f64)), ulp32(f64))
    err = abs(float(lib) - float(f64))
    return err, 4.0 * own, err / own
