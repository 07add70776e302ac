"""CPU: the host side of the scores (open_universe_amd.metrics, ou_lsd / ou_spectral_mae / ou_si_sdr, bin/eval_metrics): the
frame count, every refusal -- through Python and through the raw ABI, all decided before the first HIP call, so they are
answered on a machine without a device --, the metric names, the packing of ragged pairs and the CLI's pairing."""
import ctypes
import json
from ctypes import POINTER, byref, c_float, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

from open_universe_amd import _lib, audio, metrics as M
from open_universe_amd.bin import eval_metrics as CLI


@pytest.mark.parametrize("T", [201, 400, 159, 160, 161, 16000])
def test_frames_match_torch_stft(built_lib, T):
    for n_fft, hop in ((400, 160), (600, 240), (64, 32)):
        spec = torch.stft(torch.zeros(T), n_fft, hop_length=hop, window=torch.hann_window(n_fft), center=True,
                          pad_mode="constant", return_complex=True)
        assert built_lib.ou_metrics_frames(T, hop) == spec.shape[-1] == M.frames(T, hop)
    assert built_lib.ou_metrics_frames(T, 0) == -1 and built_lib.ou_metrics_frames(-1, 160) == -1


@pytest.mark.parametrize("n_fft,hop", [(2, 1), (6, 1), (30, 7), (402, 160), (1022, 256), (1024, 256), (404, 101), (412, 103),
                                       (64, 100), (1024, 300), (400, 43), (512, 1)])
def test_edge_resolutions_are_accepted_and_frames_match_torch_stft(built_lib, n_fft, hop):
    """The resolutions test_gpu_metrics.py adds (test_g / test_h / test_i), at rows of 16 and 17 frames and the shortest row."""
    assert M.scratch_bytes(130, 16 * hop, [_lib.MetricsSpec(n_fft, hop, 0.0, 0)]) > M.scratch_bytes(130, 16 * hop)
    for T in (n_fft // 2 + 1, 15 * hop + hop // 2, 16 * hop):
        spec = torch.stft(torch.zeros(T), n_fft, hop_length=hop, window=torch.hann_window(n_fft), center=True,
                          pad_mode="constant", return_complex=True)
        assert M.frames(T, hop) == spec.shape[-1]


def test_symbols_are_bound(built_lib):
    for name in ("ou_metrics_frames", "ou_metrics_scratch_bytes", "ou_lsd", "ou_spectral_mae", "ou_si_sdr"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(built_lib, name)
    assert ctypes.sizeof(_lib.MetricsSpec) == 16


# ---- the raw ABI: host buffers stand in for device memory -- a refusal touches none of them ----
class _Raw:
    def __init__(self, L, B=2, T=1000):
        self.L, self.B, self.T = L, B, T
        self.x = np.zeros((B, T), np.float32)
        self.out = np.full(B, 7.0, np.float32)
        self.scratch = np.zeros(64, np.uint8)
        self.lens = (c_int64 * B)(*([T] * B))

    def p(self, a):
        return c_void_p(a.ctypes.data)

    def lsd(self, n_fft=400, hop=160, lens=None, scratch_bytes=1 << 40, eps=1e-7, flags=0):
        spec = _lib.MetricsSpec(n_fft, hop, eps, flags)
        lens = self.lens if lens is None else (c_int64 * self.B)(*lens)
        return self.L.ou_lsd(self.p(self.x), self.p(self.x), self.T, lens, self.B, byref(spec), self.p(self.out),
                             self.p(self.scratch), c_size_t(scratch_bytes), None)

    def l1(self, windows=(64,), hops=None, scratch_bytes=1 << 40, lens=None, flags=0, eps=1e-8):
        hops = [w // 2 for w in windows] if hops is None else hops
        specs = (_lib.MetricsSpec * max(len(windows), 1))(*[_lib.MetricsSpec(w, h, 0.0, 0) for w, h in zip(windows, hops)])
        lens = self.lens if lens is None else (c_int64 * self.B)(*lens)
        return self.L.ou_spectral_mae(self.p(self.x), self.p(self.x), self.T, lens, self.B, specs, len(windows), 0.5, eps, flags,
                                     self.p(self.out), self.p(self.scratch), c_size_t(scratch_bytes), None)

    def sdr(self, clamp=100.0, scratch_bytes=1 << 40, lens=None):
        lens = self.lens if lens is None else (c_int64 * self.B)(*lens)
        return self.L.ou_si_sdr(self.p(self.x), self.p(self.x), self.T, lens, self.B, clamp, self.p(self.out), self.p(self.out),
                                self.p(self.scratch), c_size_t(scratch_bytes), None)


def _refused(L, code, want, *words):
    assert code == want, (code, L.ou_last_error(None))
    msg = L.ou_last_error(None).decode()
    for w in words:
        assert w in msg, msg
    return msg


def test_abi_refusals_launch_nothing(built_lib):
    L, r = built_lib, _Raw(built_lib)
    _refused(L, r.lsd(lens=[1000, 200]), _lib.OU_EINVAL, "len[1] = 200", "n_fft / 2 = 200")  # torch refuses the reflect pad too
    _refused(L, r.lsd(n_fft=401), _lib.OU_EINVAL, "n_fft = 401", "even")
    _refused(L, r.lsd(n_fft=_lib.OU_METRICS_MAX_NFFT + 2), _lib.OU_EINVAL, "OU_METRICS_MAX_NFFT = 1024")
    _refused(L, r.lsd(n_fft=0), _lib.OU_EINVAL, "n_fft = 0")
    _refused(L, r.lsd(hop=0), _lib.OU_EINVAL, "hop = 0")
    _refused(L, r.lsd(lens=[1000, 1001]), _lib.OU_EINVAL, "len[1]")  # behind the stride
    _refused(L, r.lsd(lens=[0, 1000]), _lib.OU_EINVAL, "len[0]")
    _refused(L, r.lsd(flags=4), _lib.OU_EINVAL, "flag")
    _refused(L, r.lsd(scratch_bytes=64), _lib.OU_ESHAPE, "ou_metrics_scratch_bytes asks for")
    _refused(L, r.l1(windows=(64, 255)), _lib.OU_EINVAL, "spec 1", "n_fft = 255")
    _refused(L, r.l1(windows=(64, 2048)), _lib.OU_EINVAL, "spec 1", "OU_METRICS_MAX_NFFT")
    _refused(L, r.l1(hops=[0]), _lib.OU_EINVAL, "hop = 0")
    _refused(L, r.l1(windows=(64,) * 9), _lib.OU_EINVAL, "n_spec")
    _refused(L, r.l1(flags=_lib.OU_MET_NATURAL_LOG), _lib.OU_EINVAL, "OU_MET_SCALE_INVARIANT")
    _refused(L, r.l1(scratch_bytes=0), _lib.OU_ESHAPE, "scratch")
    _refused(L, r.sdr(clamp=0.0), _lib.OU_EINVAL, "clamp_db")
    _refused(L, r.sdr(clamp=float("inf")), _lib.OU_EINVAL, "clamp_db")
    _refused(L, r.sdr(scratch_bytes=8), _lib.OU_ESHAPE, "scratch")
    _refused(L, r.sdr(lens=[1000, -1]), _lib.OU_EINVAL, "len[1]")
    assert (r.out == 7.0).all() and not r.scratch.any() and not r.x.any()
    n = c_size_t()
    bad = _lib.MetricsSpec(402, 0, 0.0, 0)
    _refused(L, L.ou_metrics_scratch_bytes(2, 1000, byref(bad), 1, byref(n)), _lib.OU_EINVAL, "hop = 0")
    _refused(L, L.ou_metrics_scratch_bytes(0, 1000, None, 0, byref(n)), _lib.OU_EINVAL, "B >= 1")


def test_scratch_bytes_grows_with_the_call(built_lib):
    s = [_lib.MetricsSpec(400, 160, 0.0, 0)]
    a, b, c = M.scratch_bytes(1, 16000, s), M.scratch_bytes(4, 16000, s), M.scratch_bytes(4, 64000, s)
    assert 0 < M.scratch_bytes(4, 16000) < a <= b < c  # (sections are aligned to 256 bytes)
    # the basis: 13 bin tiles x 2 x 100 k-steps x 64 lanes of doubles, whatever the batch
    assert a > 13 * 2 * 100 * 64 * 8 and b - a < 4 * 16000


def test_python_refusals(built_lib):
    x = torch.zeros(2, 1000)
    for kw, word in ((dict(p=1), "p=1"), (dict(window=torch.ones(400)), "window"), (dict(win_length=200), "win_length"),
                     (dict(pad=3), "pad=3"), (dict(onesided=False), "onesided")):
        with pytest.raises(NotImplementedError, match=word):
            M.log_spectral_distance(x, x, **kw)
        with pytest.raises(NotImplementedError, match=word):
            M.LogSpectralDistance(**kw)
    with pytest.raises(ValueError, match="positive"):
        M.log_spectral_distance(x, x, p=0)
    with pytest.raises(ValueError, match="n_fft = 401"):
        M.log_spectral_distance(x, x, n_fft=401)
    with pytest.raises(ValueError, match="OU_METRICS_MAX_NFFT"):
        M.log_spectral_distance(x, x, n_fft=1200, hop_length=480)
    with pytest.raises(ValueError, match="hop = 0"):
        M.log_spectral_distance(x, x, hop_length=0)
    with pytest.raises(ValueError, match="n_fft / 2 = 200"):
        M.log_spectral_distance(x[:, :200], x[:, :200])
    with pytest.raises(ValueError, match="shapes"):
        M.log_spectral_distance(x, x[:, :900])
    with pytest.raises(ValueError, match="spec 1: n_fft = 2048 exceeds OU_METRICS_MAX_NFFT"):
        M.MultiResL1SpecLoss(window_sz=[64, 2048]).per_row(x, x)
    with pytest.raises(ValueError, match="hop = 0"):
        M.MultiResL1SpecLoss(window_sz=[64], hop_sz=[0]).per_row(x, x)
    with pytest.raises(ValueError, match="clamp_db"):
        M.si_sdr(x, x, clamp_db=-1.0)
    with pytest.raises(AssertionError):
        M.MultiResL1SpecLoss(window_sz=[63])  # the reference's own assert
    # and with everything in order, a tensor that is not on a HIP device is refused: no CPU path, no fallback
    for call in (lambda: M.log_spectral_distance(x, x), lambda: M.si_sdr(x, x), lambda: M.snr(x, x),
                 lambda: M.MultiResL1SpecLoss()(x, x), lambda: M.Metrics()(16000, x, x)):
        with pytest.raises(ValueError, match="HIP device"):
            call()
    assert M.LogSpectralDistance().eps == 1e-5  # the class default differs from the function's 1e-7, as in the reference


def test_metric_names():
    assert M.Metrics.get_metric_names() == ["lsd", "si-lsd", "si-sdr", "snr"]
    assert M.Metrics().metrics == ["lsd", "si-lsd", "si-sdr", "snr"]
    assert M.Metrics(metrics=["si-sdr", "lsd"]).metrics == ["si-sdr", "lsd"]
    for name in ("pesq-wb", "pesq-nb", "stoi", "stoi-ext", "lps", "dnsmos", "plcmos", "sdr"):
        with pytest.raises(NotImplementedError, match=f"Metric {name} is not supported"):
            M.Metrics(metrics=["lsd", name])
    with pytest.raises(NotImplementedError, match="Metric mos is not supported"):
        M.Metrics(metrics=["mos"])
    x = torch.zeros(3, 500)
    assert M.Metrics()(16000, x) == [{}, {}, {}] and M.Metrics()(16000, x[0]) == {}  # no reference: nothing intrusive to compute
    with pytest.raises(ValueError, match="1 or 2 dimensions"):
        M.Metrics()(16000, x[None], x[None])
    assert M.stft_setting(16000) == (400, 160) and M.stft_setting(24000) == (600, 240)


def test_pack_and_unpack():
    g = torch.Generator().manual_seed(1)
    est = [torch.randn(n, generator=g) for n in (300, 1001, 7)]
    ref = [torch.randn(n, generator=g) for n in (310, 990, 7)]
    x, y, lens = M.pack_pairs(est, ref)
    assert lens == [310, 1001, 7] and x.shape == y.shape == (3, 1004) and x.dtype == torch.float32
    for b in range(3):
        ne, nr = est[b].shape[0], ref[b].shape[0]
        assert torch.equal(x[b, :ne], est[b]) and not x[b, ne:].any()  # the shorter of a pair is zero-padded to the longer
        assert torch.equal(y[b, :nr], ref[b]) and not y[b, nr:].any()
    with pytest.raises(ValueError, match="2 estimates for 3"):
        M.pack_pairs(est[:2], ref)
    with pytest.raises(ValueError, match="1-D"):
        M.pack_pairs([torch.zeros(2, 5)], [torch.zeros(5)])
    with pytest.raises(ValueError, match="no signals"):
        M.pack_pairs([], [])
    cols = {"lsd": [1.0, 2.0, 3.0], "snr": [4.0, 5.0, 6.0], "unused": [0, 0, 0]}
    assert M.unpack_scores(["snr", "lsd"], cols, 3) == [{"snr": 4.0, "lsd": 1.0}, {"snr": 5.0, "lsd": 2.0}, {"snr": 6.0, "lsd": 3.0}]
    with pytest.raises(NotImplementedError):
        M.evaluate_many(est, ref, 16000, metrics=["stoi"])


def _wav(path, n, fs):
    path.parent.mkdir(parents=True, exist_ok=True)
    audio.save(path, torch.linspace(-0.5, 0.5, n)[None], fs)


def test_cli_pairs_by_relative_path_and_refuses_a_rate_mismatch(tmp_path):
    ref, deg = tmp_path / "clean", tmp_path / "enh"
    _wav(ref / "a.wav", 500, 16000)
    _wav(ref / "spk" / "b.wav", 600, 16000)
    _wav(ref / "unused.wav", 100, 16000)
    _wav(deg / "a.wav", 480, 16000)
    _wav(deg / "spk" / "b.wav", 600, 16000)
    pairs = CLI.find_pairs(ref, deg)
    assert [(l, r.relative_to(ref).as_posix(), d.relative_to(deg).as_posix()) for l, r, d in pairs] == \
        [("a", "a.wav", "a.wav"), ("spk/b", "spk/b.wav", "spk/b.wav")]
    fs, d, r = CLI.load_pair(*pairs[0])
    assert fs == 16000 and d.shape == (480,) and r.shape == (500,)
    _wav(deg / "spk" / "c.wav", 100, 16000)
    with pytest.raises(FileNotFoundError, match="c.wav"):
        CLI.find_pairs(ref, deg)
    (deg / "spk" / "c.wav").unlink()
    # a pair at two rates: an error naming the pair, before anything is scored (nothing here needs a device)
    _wav(ref / "a.wav", 500, 8000)
    with pytest.raises(ValueError, match=r"a: .*8000 Hz.*16000 Hz"):
        CLI.main([str(ref), str(deg), "--metrics", "lsd", "--result-dir", str(tmp_path / "out")])
    assert not (tmp_path / "out").exists()
    with pytest.raises(NotImplementedError, match="pesq-wb"):
        CLI.main([str(ref), str(deg), "--metrics", "pesq-wb"])


def test_cli_summary_files(tmp_path):
    results = {"a": {"lsd": 1.0, "si-sdr": 10.0}, "spk/b": {"lsd": 3.0, "si-sdr": float("inf")}}
    s = CLI.summarize(results)
    assert s == {"lsd": 2.0, "lsd_std": 1.0, "si-sdr": 10.0, "si-sdr_std": 0.0, "number": 2}
    p, q = CLI.save_results(results, tmp_path / "out", "enh")
    assert p.name == "enh.json" and q.name == "enh_summary.json"
    assert json.load(open(p))["a"] == {"lsd": 1.0, "si-sdr": 10.0} and json.load(open(q))["number"] == 2
