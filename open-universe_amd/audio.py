"""Audio file I/O and resampling for the `enhance` CLI (the caller side of the hot path).

The reference CLI uses `torchaudio.load / save / functional.resample` (bin/enhance.py:77-80,180-192).  torchaudio
is used when it is installed; otherwise .wav files are read / written with the standard library + numpy, .flac files are
decoded by the native library (`ou_flac_decode`, csrc/ou_flac.cpp: every CRC of the stream and the MD5 of the decoded audio
are verified), and `resample` is restated from torchaudio's documented algorithm (`sinc_interp_hann`, lowpass_filter_width 6,
rolloff 0.99 -- the defaults the reference relies on).  .mp3 needs torchaudio.
"""
import ctypes
import hashlib
import math
import wave
from pathlib import Path

import numpy as np
import torch

AUDIO_SUFFIXES = [".wav", ".mp3", ".flac"]  # bin/enhance.py:33


def _torchaudio():
    try:
        import torchaudio  # noqa: F401

        return torchaudio
    except Exception:
        return None


def can_decode(path):
    """True when `load` can read this file here: anything with torchaudio, .wav / .flac without."""
    return _torchaudio() is not None or Path(path).suffix.lower() in (".wav", ".flac")


def _flac_info(raw):
    from . import _lib

    L = _lib.load()
    buf = (ctypes.c_uint8 * len(raw)).from_buffer_copy(raw)
    fs, ch, bps, total = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    md5 = (ctypes.c_uint8 * 16)()
    rc = L.ou_flac_info(buf, len(raw), ctypes.byref(fs), ctypes.byref(ch), ctypes.byref(bps), ctypes.byref(total), md5)
    if rc != 0:
        raise RuntimeError((L.ou_flac_last_error() or b"FLAC decoding failed").decode())
    return L, buf, fs.value, ch.value, bps.value, total.value, bytes(md5)


def _flac_channels(path):
    """Channel count of a FLAC file from its STREAMINFO block alone: the metadata block headers are walked with seeks, so
    neither the audio frames nor large metadata blocks (cover art) are read."""
    with open(path, "rb") as f:
        head = f.read(10)
        off = 0
        if head[:3] == b"ID3" and len(head) == 10:  # ID3v2 tag in front of the stream: sync-safe size
            sz = ((head[6] & 0x7F) << 21) | ((head[7] & 0x7F) << 14) | ((head[8] & 0x7F) << 7) | (head[9] & 0x7F)
            off = 10 + sz + (10 if head[5] & 0x10 else 0)
        f.seek(off)
        if f.read(4) != b"fLaC":
            raise RuntimeError("not a FLAC stream (no fLaC marker)")
        while True:
            h = f.read(4)
            if len(h) < 4:
                raise RuntimeError("FLAC: truncated metadata")
            last, typ, ln = h[0] & 0x80, h[0] & 0x7F, int.from_bytes(h[1:4], "big")
            if typ == 0:
                s = f.read(ln)
                if len(s) < 34 or ln < 34:
                    raise RuntimeError("FLAC: short STREAMINFO")
                return ((s[12] >> 1) & 7) + 1
            f.seek(ln, 1)
            if last:
                raise RuntimeError("FLAC: no STREAMINFO block")


def load_flac(path):
    """-> (float32 tensor (channels, T) in [-1, 1), sample rate): what torchaudio.load returns for a FLAC file (integer samples
    scaled by 2^-(bits - 1)).  Refuses a stream whose CRCs or whose MD5 signature of the decoded audio do not match."""
    raw = Path(path).read_bytes()
    try:
        L, buf, fs, ch, bps, total, md5 = _flac_info(raw)
        # STREAMINFO is untrusted input (36 bits of sample count x up to 8 channels): a frame of a few bytes can stand for a
        # whole block of 65 535 constant samples per channel, nothing can stand for more
        if total > max(1, len(raw)) * 16384:
            raise RuntimeError(f"FLAC: STREAMINFO claims {total} samples per channel, more than {len(raw)} bytes can encode")
        try:
            out = np.zeros((ch, max(total, 1)), dtype=np.int32)
        except MemoryError:
            raise RuntimeError(f"FLAC: cannot hold {ch} x {total} samples in memory") from None
        done = ctypes.c_int64()
        rc = L.ou_flac_decode(buf, len(raw), out.ctypes.data_as(ctypes.c_void_p), out.shape[1], ctypes.byref(done))
        if rc != 0:
            raise RuntimeError((L.ou_flac_last_error() or b"FLAC decoding failed").decode())
    except RuntimeError as e:
        raise RuntimeError(f"{path}: {e}") from None
    out = out[:, :done.value]
    if any(md5):  # MD5 of the interleaved little-endian samples, ceil(bits / 8) bytes each
        nb = (bps + 7) // 8
        inter = np.ascontiguousarray(out.T).astype("<i4")
        b = inter.view(np.uint8).reshape(-1, 4)[:, :nb] if nb < 4 else inter.view(np.uint8).reshape(-1, 4)
        if hashlib.md5(np.ascontiguousarray(b).tobytes()).digest() != md5:
            raise RuntimeError(f"{path}: FLAC MD5 signature of the decoded audio does not match the stream's")
    return torch.from_numpy(out.astype(np.float32) / float(1 << (bps - 1))), fs


def load(path):
    """-> (float32 tensor (channels, T) in [-1, 1], sample rate): torchaudio.load semantics."""
    ta = _torchaudio()
    if ta is not None:
        return ta.load(str(path))
    path = Path(path)
    if path.suffix.lower() == ".flac":
        return load_flac(path)
    if path.suffix.lower() != ".wav":
        raise RuntimeError(f"{path}: only .wav and .flac can be decoded without torchaudio")
    with open(path, "rb") as f:
        head = f.read(12)
        if head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise RuntimeError(f"{path}: not a RIFF/WAVE file")
        fmt = None
        data = None
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                break
            cid, size = ck[:4], int.from_bytes(ck[4:], "little")
            body = f.read(size + (size & 1))[:size]
            if cid == b"fmt ":
                fmt = body
            elif cid == b"data":
                data = body
        if fmt is None or data is None:
            raise RuntimeError(f"{path}: missing fmt / data chunk")
    tag = int.from_bytes(fmt[0:2], "little")
    ch = int.from_bytes(fmt[2:4], "little")
    fs = int.from_bytes(fmt[4:8], "little")
    bits = int.from_bytes(fmt[14:16], "little")
    if tag == 0xFFFE and len(fmt) >= 26:  # WAVE_FORMAT_EXTENSIBLE: sub-format GUID starts with the real tag
        tag = int.from_bytes(fmt[24:26], "little")
    if tag == 3 and bits == 32:
        x = np.frombuffer(data, dtype="<f4").astype(np.float32)
    elif tag == 3 and bits == 64:
        x = np.frombuffer(data, dtype="<f8").astype(np.float32)
    elif tag == 1 and bits == 16:
        x = np.frombuffer(data, dtype="<i2").astype(np.float32) / 32768.0
    elif tag == 1 and bits == 32:
        x = np.frombuffer(data, dtype="<i4").astype(np.float32) / 2147483648.0
    elif tag == 1 and bits == 24:
        b = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / 8388608.0
    elif tag == 1 and bits == 8:
        x = (np.frombuffer(data, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    else:
        raise RuntimeError(f"{path}: unsupported WAV encoding (format tag {tag}, {bits} bits)")
    n = (x.size // ch) * ch
    return torch.from_numpy(x[:n].reshape(-1, ch).T.copy()), fs


def channels(path):
    """Number of channels of an audio file from its header alone (no sample is decoded)."""
    ta = _torchaudio()
    if ta is not None:
        return int(ta.info(str(path)).num_channels)
    if Path(path).suffix.lower() == ".flac":
        try:
            return _flac_channels(path)
        except RuntimeError as e:
            raise RuntimeError(f"{path}: {e}") from None
    with open(path, "rb") as f:
        head = f.read(12)
        if head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise RuntimeError(f"{path}: not a RIFF/WAVE file")
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                raise RuntimeError(f"{path}: missing fmt chunk")
            cid, size = ck[:4], int.from_bytes(ck[4:], "little")
            if cid == b"fmt ":
                return int.from_bytes(f.read(4)[2:4], "little")
            f.seek(size + (size & 1), 1)


def save(path, audio, fs, flac_level=0):
    """audio: float tensor (channels, T).  Written as 32-bit float WAV (what torchaudio.save does for float32).  flac_level > 0:
    a .flac file comes from `save_flac` at that compression level, with or without torchaudio."""
    ta = _torchaudio()
    if ta is not None and not (flac_level and Path(path).suffix.lower() == ".flac"):
        return ta.save(str(path), audio, fs)
    path = Path(path)
    if path.suffix.lower() == ".flac":
        return save_flac(path, audio, fs, level=flac_level)
    if path.suffix.lower() != ".wav":
        raise RuntimeError(f"{path}: only .wav and .flac can be encoded without torchaudio")
    x = audio.detach().to(torch.float32).cpu().numpy()
    if x.ndim == 1:
        x = x[None]
    ch, n = x.shape
    payload = np.ascontiguousarray(x.T).astype("<f4").tobytes()
    fmt = (3).to_bytes(2, "little") + ch.to_bytes(2, "little") + int(fs).to_bytes(4, "little") + \
        (int(fs) * ch * 4).to_bytes(4, "little") + (ch * 4).to_bytes(2, "little") + (32).to_bytes(2, "little")
    fact = n.to_bytes(4, "little")
    body = b"WAVE" + b"fmt " + len(fmt).to_bytes(4, "little") + fmt + b"fact" + (4).to_bytes(4, "little") + fact + \
        b"data" + len(payload).to_bytes(4, "little") + payload
    with open(path, "wb") as f:
        f.write(b"RIFF" + len(body).to_bytes(4, "little") + body)


_kernel_cache = {}


def _sinc_kernel(orig, new, device, lowpass_filter_width=6, rolloff=0.99):
    """torchaudio.functional.resample's `sinc_interp_hann` kernel: (new, 1, 2*width + orig) and `width`."""
    key = (orig, new, str(device))
    if key not in _kernel_cache:
        base = min(orig, new) * rolloff
        width = math.ceil(lowpass_filter_width * orig / base)
        idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
        t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
        t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
        window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
        t = t * math.pi
        scale = base / orig
        k = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t) * window * scale
        _kernel_cache[key] = (k.to(torch.float32).to(device), width)
    return _kernel_cache[key]


_RESAMPLE_BACKENDS = ("torch", "library")
_table_cache = {}


def _resample_torch(audio, fs, target_fs):
    if fs == target_fs:
        return audio
    g = math.gcd(fs, target_fs)
    orig, new = fs // g, target_fs // g
    kernel, width = _sinc_kernel(orig, new, audio.device)
    shape = audio.shape
    x = audio.reshape(-1, shape[-1]).to(torch.float32)
    n, length = x.shape
    x = torch.nn.functional.pad(x, (width, width + orig))
    y = torch.nn.functional.conv1d(x[:, None], kernel, stride=orig)  # (n, new, frames)
    y = y.transpose(1, 2).reshape(n, -1)
    target_length = int(math.ceil(new * length / orig))
    return y[..., :target_length].reshape(shape[:-1] + (target_length,))


def _device_table(L, fs, target_fs, device):
    """The coefficient table of ou_resample on `device` (uploaded once per reduced rate pair and device) and its byte size."""
    from . import _lib

    g = math.gcd(fs, target_fs)
    key = (fs // g, target_fs // g, str(device))
    if key not in _table_cache:
        raw = _lib.resample_table(fs, target_fs)[2]
        _table_cache[key] = torch.from_numpy(raw).to(device)
    return _table_cache[key]


def _resample_rows(x, lens, fs, target_fs):
    """ONE ou_resample call: x (rows, stride) float32 on a HIP device, row b holding lens[b] samples -> ((rows, cols) tensor,
    output lengths); the columns behind a row's own output are zero."""
    from . import _lib

    L = _lib.load()
    rows = x.shape[0]
    out_lens = [int(L.ou_resample_length(fs, target_fs, int(n))) for n in lens]
    cols = max(out_lens)
    y = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
    if cols == 0:
        return y, out_lens
    if fs == target_fs:
        tab_ptr, tab_bytes = None, 0
    else:
        tab = _device_table(L, fs, target_fs, x.device)
        tab_ptr, tab_bytes = ctypes.c_void_p(tab.data_ptr()), tab.numel()
    with torch.cuda.device(x.device):
        _lib.check(L.ou_resample(ctypes.c_void_p(x.data_ptr()), x.stride(0), (ctypes.c_int64 * rows)(*[int(n) for n in lens]),
                                 ctypes.c_void_p(y.data_ptr()), y.stride(0), cols, rows, fs, target_fs, tab_ptr,
                                 ctypes.c_size_t(tab_bytes),
                                 ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
    return y, out_lens


def _check_backend(backend):
    if backend not in _RESAMPLE_BACKENDS:
        raise ValueError(f"resample: backend must be one of {_RESAMPLE_BACKENDS}, not {backend!r}")


def resample(audio, fs, target_fs, backend="torch"):
    """torchaudio.functional.resample(audio, fs, target_fs) with its default arguments (bin/enhance.py:77-80):
    polyphase windowed-sinc FIR.  backend "torch" (default): one strided conv1d over the dense kernel on the tensor's device.
    backend "library" (extension): the library's own kernel (ou_resample), which evaluates only the taps inside the window's
    support; the tensor must live on a HIP device (ValueError otherwise: there is no CPU path and no fallback)."""
    _check_backend(backend)
    fs, target_fs = int(fs), int(target_fs)
    if backend == "torch":
        return _resample_torch(audio, fs, target_fs)
    if audio.device.type != "cuda":
        raise ValueError("resample(backend='library') runs on a HIP device only: move the tensor there or use backend='torch'")
    if fs == target_fs:
        return audio
    shape = audio.shape
    x = audio.reshape(-1, shape[-1]).to(torch.float32).contiguous()
    y, out_lens = _resample_rows(x, [shape[-1]] * x.shape[0], fs, target_fs)
    return y.reshape(shape[:-1] + (out_lens[0] if out_lens else 0,))


def resample_many(signals, fs, target_fs, backend="torch"):
    """`resample` of a list of (T_i,) or (C_i, T_i) tensors of one rate -> list of the same shapes at the new rate.
    backend "library": ONE ou_resample call over all channel rows of all signals (gathered into one padded buffer on the
    device; the lengths travel as a host array), every row bit-identical to `resample(row, backend="library")`.
    backend "torch": the loop over `resample`."""
    _check_backend(backend)
    fs, target_fs = int(fs), int(target_fs)
    signals = list(signals)
    if backend == "torch":
        return [_resample_torch(s, fs, target_fs) for s in signals]
    if not signals:
        return []
    for s in signals:
        if s.device.type != "cuda":
            raise ValueError("resample_many(backend='library') runs on a HIP device only")
        if s.ndim not in (1, 2):
            raise ValueError("resample_many: signals are (T,) or (C, T) tensors")
    if fs == target_fs:
        return signals
    device = signals[0].device
    counts = [1 if s.ndim == 1 else s.shape[0] for s in signals]
    lens = [int(s.shape[-1]) for s, c in zip(signals, counts) for _ in range(c)]
    stride = (max(lens) + 3) // 4 * 4  # 16-byte aligned rows: the kernel then stages with 16-byte loads
    x = torch.empty((sum(counts), max(stride, 4)), dtype=torch.float32, device=device)
    r = 0
    for s, c in zip(signals, counts):
        x[r:r + c, :s.shape[-1]] = s.to(device=device, dtype=torch.float32).reshape(c, -1)
        r += c
    y, out_lens = _resample_rows(x, lens, fs, target_fs)
    out, r = [], 0
    for s, c in zip(signals, counts):
        o = y[r:r + c, :out_lens[r] if c else 0].clone()
        out.append(o[0] if s.ndim == 1 else o)
        r += c
    return out


# ---- FLAC encoder (the output side of a .flac input: the reference writes the enhanced file under the input's name with
# torchaudio.save, bin/enhance.py:77-80).  A plain, valid subset of the format, vectorised with numpy: independent channels,
# fixed block size, the order-2 fixed predictor, one Rice partition per subframe (verbatim where that is shorter), 24 bits per
# sample (float32 audio; 16 on request), STREAMINFO with the MD5 of the audio.  Compression ratio is not the point; any FLAC
# decoder reads the result, `load_flac` reads it back bit for bit (tests/test_audio_flac.py).
_CRC8 = None
_CRC16 = None


def _crc_tables():
    global _CRC8, _CRC16
    if _CRC8 is None:
        t8, t16 = [], []
        for i in range(256):
            c = i
            for _ in range(8):
                c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
            t8.append(c)
            c = i << 8
            for _ in range(8):
                c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
            t16.append(c)
        _CRC8, _CRC16 = t8, t16
    return _CRC8, _CRC16


def _crc8(b):
    t, _ = _crc_tables()
    c = 0
    for x in b:
        c = t[c ^ x]
    return c


def _crc16(b):
    _, t = _crc_tables()
    c = 0
    for x in b:
        c = ((c << 8) & 0xFFFF) ^ t[(c >> 8) ^ x]
    return c


def _bits_of(values, width):
    """(n,) non-negative ints -> (n, width) array of bits, MSB first"""
    v = np.asarray(values, dtype=np.uint64)[:, None]
    sh = np.arange(width - 1, -1, -1, dtype=np.uint64)[None, :]
    return ((v >> sh) & np.uint64(1)).astype(np.uint8)


def _utf8_number(n):
    if n < 0x80:
        return bytes([n])
    out, lead = [], 0
    nb = 2 if n < 0x800 else 3 if n < 0x10000 else 4 if n < 0x200000 else 5 if n < 0x4000000 else 6 if n < 0x80000000 else 7
    for _ in range(nb - 1):
        out.append(0x80 | (n & 0x3F))
        n >>= 6
    lead = ((0xFF << (8 - nb)) & 0xFF) | n
    return bytes([lead] + out[::-1])


def _subframe_bits(x, bps):
    """one channel of one block (int64) -> bit array: order-2 fixed predictor + one Rice partition, or verbatim"""
    n = len(x)
    two = np.uint64(1) << np.uint64(bps)
    verb = np.concatenate([np.array([0, 0, 0, 0, 0, 0, 1, 0], np.uint8), _bits_of((x.astype(np.int64) % int(two)).astype(np.uint64), bps).ravel()])
    if n < 3:
        return verb
    r = x[2:] - 2 * x[1:-1] + x[:-2]
    u = np.where(r >= 0, 2 * r, -2 * r - 1).astype(np.uint64)
    mean = float(u.mean()) if len(u) else 0.0
    k = int(max(0, min(14, math.floor(math.log2(mean + 1.0)))))
    q = (u >> np.uint64(k)).astype(np.int64)
    if int(q.max(initial=0)) > 4096:
        return verb
    lens = q + 1 + k
    total = int(lens.sum())
    if 8 + 2 * bps + 10 + total >= len(verb):
        return verb
    body = np.zeros(total, np.uint8)
    ends = np.cumsum(lens)
    body[ends - k - 1] = 1                                    # the terminating 1 of every unary part
    if k:
        low = _bits_of(u & np.uint64((1 << k) - 1), k)
        idx = (ends - k)[:, None] + np.arange(k)[None, :]
        body[idx.ravel()] = low.ravel()
    head = np.concatenate([np.array([0, 0, 0, 1, 0, 1, 0, 0], np.uint8),               # pad, fixed order 2, no wasted bits
                           _bits_of((x[:2].astype(np.int64) % int(two)).astype(np.uint64), bps).ravel(),
                           np.array([0, 0], np.uint8), np.zeros(4, np.uint8), _bits_of([k], 4).ravel()])
    return np.concatenate([head, body])


# ---- compression levels 1 and 2: per subframe the cheapest of constant / fixed 0-4 / (level 2) one LPC
# candidate of order 8, priced exactly in integers, then the best Rice partition order 0..6 for the winner; verbatim where that
# is not shorter.  Level 0 is `_subframe_bits` above.  A choice record is FLAC_CHOICE_WORDS int32: kind, order, partition order,
# precision, shift, subframe bits, then FLAC_CHOICE_COEFS coefficients (OU_FLAC_CHOICE_* of include/ouniverse.h).
FLAC_CHOICE_WORDS = 18
FLAC_CHOICE_COEFS = 12
FLAC_CONSTANT, FLAC_VERBATIM, FLAC_FIXED, FLAC_LPC = 0, 1, 2, 3
_FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))
_LPC_ORDER, _LPC_PRECISION, _LPC_MIN_BLOCK, _RICE_MAX_QUOTIENT = 8, 14, 64, 4096


def _rice_k(total, cnt):
    """the largest k <= 14 with (2^k - 1) cnt <= total"""
    k = 0
    while k < 14 and ((2 << k) - 1) * cnt <= total:
        k += 1
    return k


def _lpc_analysis(x):
    """one channel of one block (int64, n >= 64) -> (coefs, shift) or None.  Welch window, autocorrelation lags 0..8 and
    Levinson-Durbin in float64; the sums run in the order of the kernel (16 consecutive samples, a 64-wide butterfly, four
    partial sums), so the two usually agree to the last bit, which nothing depends on."""
    n = len(x)
    i = np.arange(4096, dtype=np.float64)
    z = (2.0 * i - float(n - 1)) / float(n + 1)
    xw = np.zeros(4096 + _LPC_ORDER, np.float64)
    xw[_LPC_ORDER:_LPC_ORDER + n] = x.astype(np.float64) * (1.0 - z * z)[:n]
    lane = np.arange(256)
    r = []
    for lag in range(_LPC_ORDER + 1):
        prod = (xw[_LPC_ORDER:] * xw[_LPC_ORDER - lag:4096 + _LPC_ORDER - lag]).reshape(256, 16)
        acc = np.zeros(256, np.float64)
        for j in range(16):
            acc = acc + prod[:, j]
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lane ^ o]
        t = 0.0
        for w in range(4):
            t = t + float(acc[64 * w])
        r.append(t)
    if not (math.isfinite(r[0]) and r[0] > 0.0):
        return None
    a, err = [0.0] * _LPC_ORDER, r[0]
    with np.errstate(all="ignore"):
        for m in range(_LPC_ORDER):
            acc = np.float64(r[m + 1])
            for j in range(m):
                acc = acc - np.float64(a[j]) * np.float64(r[m - j])
            kk = acc / np.float64(err)
            prev = list(a)
            for j in range(m):
                a[j] = float(np.float64(prev[j]) - kk * np.float64(prev[m - 1 - j]))
            a[m] = float(kk)
            err = float(np.float64(err) * (np.float64(1.0) - kk * kk))
            if not (math.isfinite(err) and err > 0.0):
                return None
    if not all(math.isfinite(v) for v in a):
        return None
    cmax = max(abs(v) for v in a)
    if cmax == 0.0:
        return None
    shift = min(15, max(0, (_LPC_PRECISION - 1) - math.frexp(cmax)[1]))
    return [int(np.rint(np.float64(v) * np.float64(2.0 ** shift))) for v in a], shift  # (a value of +-2^13 is refused later)


def _fold(r):
    return np.where(r >= 0, 2 * r, -2 * r - 1)


def _subframe_level(x, bps, level, override=None):
    """one channel of one block (int64) -> (bit array, choice record) at compression level 1 or 2"""
    n = len(x)
    two = 1 << bps
    rec = [0] * FLAC_CHOICE_WORDS
    # candidates in tie-break order: (kind, order, coefs, shift, residuals)
    cands = []
    for p in range(5):
        if n > p:
            r = x[p:].copy()
            for j, c in enumerate(_FIXED[p]):
                r = r - c * x[p - 1 - j:n - 1 - j]
            cands.append((FLAC_FIXED, p, (), 0, r))
    if level >= 2:
        lpc = None
        if override is not None:
            lpc = ([int(v) for v in override[0]], int(override[1]))
        elif n >= _LPC_MIN_BLOCK:
            lpc = _lpc_analysis(x)
        if lpc is not None:
            coefs, shift = lpc
            p = len(coefs)
            half = 1 << (_LPC_PRECISION - 1)
            if 1 <= p <= FLAC_CHOICE_COEFS and n > p and 0 <= shift <= 15 and all(-half <= c < half for c in coefs):
                pred = np.zeros(n - p, np.int64)
                for j, c in enumerate(coefs):
                    pred = pred + c * x[p - 1 - j:n - 1 - j]
                r = x[p:] - (pred >> shift)
                if int(np.abs(r).max(initial=0)) < (1 << 31):
                    cands.append((FLAC_LPC, p, tuple(coefs), shift, r))
    # stage 1 and stage 2, once for the candidates of level 1 and once for the lpc candidate, which wins only when it is
    # strictly shorter after its own partition search (so a level-2 subframe is never longer than the level-1 one)
    best, po, ks = None, 0, None  # best: (bits, candidate, u, head bits)
    for group in ([c for c in cands if c[0] == FLAC_FIXED], [c for c in cands if c[0] == FLAC_LPC]):
        gbest, gpo, gks = None, 0, None
        if group and group[0][0] == FLAC_FIXED and np.all(x == x[0]):
            gbest = (8 + bps, None, None, 0)
        for cand in group:
            kind, p, coefs, shift, r = cand
            u = _fold(r)
            cnt = n - p
            k = _rice_k(int(u.sum()), cnt)
            if int((u >> k).max(initial=0)) > _RICE_MAX_QUOTIENT:
                continue
            head = 8 + p * bps + (4 + 5 + p * _LPC_PRECISION if kind == FLAC_LPC else 0) + 2 + 4
            bits = head + 4 + cnt * (k + 1) + int((u >> k).sum())
            if gbest is None or bits < gbest[0]:
                gbest, gpo, gks = (bits, cand, u, head), 0, [k]
        if gbest is not None and gbest[1] is not None:
            bits, cand, u, head = gbest
            p = cand[1]
            for cpo in range(1, 7):
                if n % (1 << cpo) or (n >> cpo) < 16:
                    break
                size = n >> cpo
                total, kk = 4 << cpo, []
                for j in range(1 << cpo):
                    seg = u[max(j * size - p, 0):(j + 1) * size - p]
                    k = _rice_k(int(seg.sum()), len(seg))
                    if int((seg >> k).max(initial=0)) > _RICE_MAX_QUOTIENT:
                        break
                    kk.append(k)
                    total += len(seg) * (k + 1) + int((seg >> k).sum())
                if len(kk) == 1 << cpo and head + total < bits:
                    bits, gpo, gks = head + total, cpo, kk
            gbest = (bits, cand, u, head)
        if gbest is not None and (best is None or gbest[0] < best[0]):
            best, po, ks = gbest, gpo, gks
    wrapped = (x.astype(np.int64) % two).astype(np.uint64)
    if best is None or best[0] >= 8 + n * bps:
        rec[0], rec[5] = FLAC_VERBATIM, 8 + n * bps
        return np.concatenate([np.array([0, 0, 0, 0, 0, 0, 1, 0], np.uint8), _bits_of(wrapped, bps).ravel()]), rec
    bits, cand, u, head = best
    if cand is None:
        rec[0], rec[5] = FLAC_CONSTANT, bits
        return np.concatenate([np.zeros(8, np.uint8), _bits_of(wrapped[:1], bps).ravel()]), rec
    kind, p, coefs, shift, _ = cand
    rec[:6] = [kind, p, po, _LPC_PRECISION if kind == FLAC_LPC else 0, shift, bits]
    rec[6:6 + len(coefs)] = coefs
    parts = [_bits_of([(8 + p if kind == FLAC_FIXED else 31 + p) << 1], 8).ravel(), _bits_of(wrapped[:p], bps).ravel()]
    if kind == FLAC_LPC:
        parts += [_bits_of([_LPC_PRECISION - 1], 4).ravel(), _bits_of([shift], 5).ravel(),
                  _bits_of([c % (1 << _LPC_PRECISION) for c in coefs], _LPC_PRECISION).ravel()]
    parts.append(_bits_of([po], 6).ravel())  # coding method 0, the partition order
    size = n >> po
    idx = np.arange(p, n)
    part = idx // size
    kv = np.asarray(ks, np.int64)[part]
    pre = np.where((idx % size == 0) | (idx == p), 4, 0)
    pre[0] = 4
    lens = pre + (u >> kv) + 1 + kv
    ends = np.cumsum(lens)
    body = np.zeros(int(ends[-1]), np.uint8)
    body[ends - kv - 1] = 1
    for k in set(ks):
        if k:
            sel = kv == k
            at = (ends[sel] - k)[:, None] + np.arange(k)[None, :]
            body[at.ravel()] = _bits_of((u[sel] & ((1 << k) - 1)).astype(np.uint64), k).ravel()
    first = pre == 4
    at = (ends[first] - lens[first])[:, None] + np.arange(4)[None, :]
    body[at.ravel()] = _bits_of(kv[first].astype(np.uint64), 4).ravel()
    out = np.concatenate(parts + [body])
    assert len(out) == bits, (len(out), bits)
    return out, rec


def _level0_record(bits, n, bps):
    """the choice record of a level-0 subframe, read off its first byte"""
    rec = [0] * FLAC_CHOICE_WORDS
    rec[0], rec[5] = (FLAC_FIXED if bits[3] else FLAC_VERBATIM), len(bits)
    if bits[3]:
        rec[1] = 2
    return rec


def flac_encode(samples, fs, bps=24, block=4096, level=0, lpc_override=None, return_choices=False):
    """samples: int array (channels, T), values within bps bits -> the bytes of a FLAC stream.
    level: 0 (fixed order 2, one Rice parameter: the stream of earlier versions), 1 (constant, fixed orders 0-4, partitioned
    Rice) or 2 (level 1 plus an LPC candidate of order 8).  lpc_override: {(frame number, channel): (coefs, shift)} replaces
    the level-2 analysis of those subframes.  return_choices: also return one record per subframe in stream order, an int32
    array (subframes, FLAC_CHOICE_WORDS)."""
    x = np.asarray(samples, dtype=np.int64)
    ch, n = x.shape
    if level not in (0, 1, 2):
        raise ValueError("flac_encode: level is 0, 1 or 2")
    if level and block != 4096:
        raise ValueError("flac_encode: levels 1 and 2 use blocks of 4096")
    if not (1 <= ch <= 8) or bps not in (8, 16, 24) or not (0 < fs < (1 << 20)):
        raise ValueError("flac_encode: 1-8 channels, 8 / 16 / 24 bits per sample")
    records = []

    def sub(c, blk, fno):
        if level == 0:
            bits = _subframe_bits(blk, bps)
            records.append(_level0_record(bits, len(blk), bps))
            return bits
        bits, rec = _subframe_level(blk, bps, level, (lpc_override or {}).get((fno, c)))
        records.append(rec)
        return bits

    nb = (bps + 7) // 8
    inter = np.ascontiguousarray(x.T).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :nb]
    md5 = hashlib.md5(np.ascontiguousarray(inter).tobytes()).digest()
    frames, fno, sizes = [], 0, []
    ssc = {8: 1, 16: 4, 24: 6}[bps]
    for s0 in range(0, max(n, 1), block):
        blk = x[:, s0:s0 + block]
        bs = blk.shape[1]
        if bs == 0:
            break
        hdr = bytearray([0xFF, 0xF8, (7 << 4) | 0, ((ch - 1) << 4) | (ssc << 1)])   # 16-bit block size follows, rate from STREAMINFO
        hdr += _utf8_number(fno)
        hdr += (bs - 1).to_bytes(2, "big")
        hdr.append(_crc8(hdr))
        bits = np.concatenate([sub(c, blk[c], fno) for c in range(ch)])
        body = np.packbits(bits).tobytes()
        fr = bytes(hdr) + body
        fr += _crc16(fr).to_bytes(2, "big")
        frames.append(fr)
        sizes.append(len(fr))
        fno += 1
    si = bytearray()
    si += min(block, 65535).to_bytes(2, "big") * 2
    si += (min(sizes) if sizes else 0).to_bytes(3, "big") + (max(sizes) if sizes else 0).to_bytes(3, "big")
    v = (int(fs) << 44) | ((ch - 1) << 41) | ((bps - 1) << 36) | n
    si += v.to_bytes(8, "big") + md5
    out = b"fLaC" + bytes([0x80]) + len(si).to_bytes(3, "big") + bytes(si) + b"".join(frames)
    if return_choices:
        return out, np.array(records, dtype=np.int32).reshape(-1, FLAC_CHOICE_WORDS)
    return out


def save_flac(path, audio, fs, bits_per_sample=24, level=0):
    """audio: float tensor (channels, T) in [-1, 1] -> FLAC with `bits_per_sample` bits (round to nearest, clipped)."""
    x = audio.detach().to(torch.float64).cpu().numpy()
    if x.ndim == 1:
        x = x[None]
    full = float(1 << (bits_per_sample - 1))
    q = np.clip(np.rint(x * full), -full, full - 1).astype(np.int64)
    Path(path).write_bytes(flac_encode(q, int(fs), bits_per_sample, level=level))


# ---- the same stream from the device (ou_flac_encode_frames, csrc/ou_flac_encode.hip): quantisation, residuals, Rice codes and
# bit packing of all files of a call in one kernel per 64 files, CRC-16 / MD5 / STREAMINFO in the library's host stage
# (ou_flac_assemble).  Byte for byte what `flac_encode` writes for the samples `save_flac` would quantise (a NaN sample, which
# numpy leaves undefined, encodes as 0).
_pinned = {}


def _pinned_bytes(key, nbytes):
    """a pinned uint8 host buffer of at least `nbytes`, kept and grown per purpose"""
    buf = _pinned.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True)
        _pinned[key] = buf
    return buf[:nbytes]


def _flac_encode_device(x, stride, channels, lens, bits_per_sample, level=0, want_choices=False):
    """ONE ou_flac_encode_frames_level call over the rows of x (file f: channels[f] consecutive rows of lens[f] samples) ->
    (frames, frame_bytes, pcm, choices or None) uint8 / int32 / uint8 / int32 tensors on the device.  No synchronisation."""
    from . import _lib

    L = _lib.load()
    files = len(channels)
    ch = (ctypes.c_int32 * files)(*channels)
    ln = (ctypes.c_int64 * files)(*lens)
    fb, nf, pb = ctypes.c_size_t(), ctypes.c_int64(), ctypes.c_size_t()
    if L.ou_flac_encode_sizes(files, ch, ln, int(bits_per_sample), ctypes.byref(fb), ctypes.byref(nf), ctypes.byref(pb), None) != 0:
        raise ValueError((L.ou_flac_last_error() or b"ou_flac_encode_sizes failed").decode())
    frames = torch.empty(fb.value, dtype=torch.uint8, device=x.device)
    sizes = torch.empty(nf.value, dtype=torch.int32, device=x.device)
    pcm = torch.empty(pb.value, dtype=torch.uint8, device=x.device)
    choices, cb = None, ctypes.c_size_t(0)
    if want_choices:
        if L.ou_flac_encode_choices_bytes(files, ch, ln, ctypes.byref(cb)) != 0:
            raise ValueError((L.ou_flac_last_error() or b"ou_flac_encode_choices_bytes failed").decode())
        choices = torch.empty(cb.value // 4, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.ou_flac_encode_frames_level(ctypes.c_void_p(x.data_ptr()), int(stride), files, ch, ln, int(bits_per_sample),
                                           int(level), ctypes.c_void_p(frames.data_ptr()), ctypes.c_size_t(fb.value),
                                           ctypes.c_void_p(sizes.data_ptr()), ctypes.c_void_p(pcm.data_ptr()),
                                           ctypes.c_size_t(pb.value),
                                           ctypes.c_void_p(choices.data_ptr()) if want_choices else None, cb,
                                           ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    if rc != 0:
        msg = (L.ou_flac_last_error() or b"ou_flac_encode_frames_level failed").decode()
        raise (RuntimeError if rc == _lib.OU_EHIP else ValueError)(msg)
    return frames, sizes, pcm, choices


def _flac_assemble(frames, sizes, pcm, channels, lens, fs, bits_per_sample):
    """host copies of the three buffers (numpy uint8 / int32 / uint8) -> list of streams (ou_flac_assemble)"""
    from . import _lib

    L = _lib.load()
    files = len(channels)
    ch = (ctypes.c_int32 * files)(*channels)
    ln = (ctypes.c_int64 * files)(*lens)
    cap = (ctypes.c_int64 * files)()
    if L.ou_flac_encode_sizes(files, ch, ln, int(bits_per_sample), None, None, None, cap) != 0:
        raise ValueError((L.ou_flac_last_error() or b"ou_flac_encode_sizes failed").decode())
    out = np.empty(sum(cap), dtype=np.uint8)
    off = (ctypes.c_int64 * (files + 1))()
    rc = L.ou_flac_assemble(frames.ctypes.data_as(ctypes.c_void_p), sizes.ctypes.data_as(ctypes.c_void_p),
                            pcm.ctypes.data_as(ctypes.c_void_p), files, ch, ln, int(fs), int(bits_per_sample),
                            out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.nbytes), off)
    if rc != 0:
        raise ValueError((L.ou_flac_last_error() or b"ou_flac_assemble failed").decode())
    return [out[off[f]:off[f + 1]].tobytes() for f in range(files)]


def flac_encode_many(signals, fs, bits_per_sample=24, level=0, return_choices=False):
    """signals: list of (T_i,) or (C_i, T_i) float tensors on one HIP device, in [-1, 1] -> list of `bytes`, the FLAC streams
    `save_flac` would write (round to nearest even, clipped; 16 or 24 bits).  One device call over all channel rows of all
    signals, one device-to-host copy per buffer (into pinned memory), one ou_flac_assemble.  There is no CPU path and no
    fallback: ValueError for a CPU tensor.  level: 0, 1 or 2 as in `flac_encode` (levels 0 and 1 give its bytes; a level-2 stream
    is the one it writes with the device's coefficients as lpc_override).  return_choices: -> (streams, list of int32 arrays
    (subframes of the file, FLAC_CHOICE_WORDS))."""
    signals = list(signals)
    if level not in (0, 1, 2):
        raise ValueError("flac_encode_many: level is 0, 1 or 2")
    if not signals:
        return ([], []) if return_choices else []
    for s in signals:
        if s.device.type != "cuda":
            raise ValueError("flac_encode_many runs on a HIP device only: move the tensors there or use save_flac")
        if s.ndim not in (1, 2):
            raise ValueError("flac_encode_many: signals are (T,) or (C, T) tensors")
        if s.device != signals[0].device:
            raise ValueError("flac_encode_many: all signals must live on one device")
    device = signals[0].device
    channels = [1 if s.ndim == 1 else int(s.shape[0]) for s in signals]
    lens = [int(s.shape[-1]) for s in signals]
    if min(channels) < 1 or min(lens) < 1:
        raise ValueError("flac_encode_many: every signal needs at least one channel and one sample")
    if len(signals) == 1 and signals[0].dtype == torch.float32 and signals[0].stride(-1) == 1 and \
            (signals[0].ndim == 1 or channels[0] == 1 or signals[0].stride(0) >= lens[0]):
        x = signals[0].detach()  # the rows as they lie: no gather
        stride = lens[0] if x.ndim == 1 or channels[0] == 1 else x.stride(0)
    else:
        stride = (max(lens) + 3) // 4 * 4
        x = torch.empty((sum(channels), stride), dtype=torch.float32, device=device)
        r = 0
        for s, c in zip(signals, channels):
            x[r:r + c, :s.shape[-1]] = s.detach().to(torch.float32).reshape(c, -1)
            r += c
    frames, sizes, pcm, choices = _flac_encode_device(x, stride, channels, lens, bits_per_sample, level, return_choices)
    host = []
    for key, t in (("frames", frames), ("sizes", sizes), ("pcm", pcm)):
        h = _pinned_bytes(key, t.numel() * t.element_size())
        h.copy_(t.view(torch.uint8), non_blocking=True)
        host.append(h)
    torch.cuda.current_stream(device).synchronize()
    streams = _flac_assemble(host[0].numpy(), host[1].numpy().view(np.int32), host[2].numpy(), channels, lens, fs, bits_per_sample)
    if not return_choices:
        return streams
    rec = choices.cpu().numpy().reshape(-1, FLAC_CHOICE_WORDS)
    cuts = np.cumsum([0] + [c * ((n + 4095) // 4096) for c, n in zip(channels, lens)])
    return streams, [rec[cuts[i]:cuts[i + 1]].copy() for i in range(len(channels))]


def save_flac_many(paths, signals, fs, bits_per_sample=24, level=0):
    """`save_flac(path, signal, fs, bits_per_sample, level)` for every pair, encoded by ONE `flac_encode_many` call."""
    paths, signals = list(paths), list(signals)
    if len(paths) != len(signals):
        raise ValueError("save_flac_many: one path per signal")
    for path, data in zip(paths, flac_encode_many(signals, fs, bits_per_sample, level)):
        Path(path).write_bytes(data)
