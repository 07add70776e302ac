"""The library's resampler, host side (no GPU): plan, coefficient table and length helper of ou_resample against
`audio._sinc_kernel` / `audio.resample`, the refusals that are decided before any HIP call, and the CLI switch.

Definition and measuring stick: resample_reference.py (float64, numpy, dense kernel)."""
import ctypes

import numpy as np
import pytest
import torch

import resample_reference as R
from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli

# the longest support over the phases, from the dense float64 kernel (16 000 -> 16 001 and the other pairs that do not
# reduce the rate: 13)
EXPECTED_TAPS = {(44100, 16000): 34, (96000, 16000): 73, (16000, 44100): 13}


@pytest.mark.parametrize("fs_in,fs_out", R.PAIRS)
def test_plan_and_table_are_the_dense_kernel_over_its_support(built_lib, fs_in, fs_out):
    orig, new, base, width = R.geometry(fs_in, fs_out)
    plan = _lib.resample_plan(fs_in, fs_out)
    assert (plan["orig"], plan["new"], plan["width"]) == (orig, new, width)
    first, coef, raw = _lib.resample_table(fs_in, fs_out)
    taps = plan["taps"]
    assert raw.nbytes == plan["table_bytes"] == (taps + 1) * new * 4 and coef.shape == (taps, new)
    dense, w = A._sinc_kernel(orig, new, "cpu")
    if new > 4096:  # (the length check of this pair, while audio.resample finds its gigabyte of dense kernel in the cache)
        _check_lengths(built_lib, fs_in, fs_out)
    A._kernel_cache.pop((orig, new, "cpu"), None)  # (a gigabyte at 16 000 -> 16 001: not kept for the rest of the session)
    dense = dense[:, 0].numpy()
    L = 2 * width + orig
    assert w == width and dense.shape == (new, L)
    longest = 0
    for p0 in range(0, new, 1024):  # a slab of phases at a time
        ph = np.arange(p0, min(new, p0 + 1024))
        inside = np.abs(R.argument(fs_in, fs_out, ph)) < 6.0          # the support, from the definition
        d = dense[ph]
        count = inside.sum(axis=1)
        lo = inside.argmax(axis=1)
        assert (count >= 1).all() and (inside.cumsum(axis=1)[np.arange(len(ph)), lo + count - 1] == count).all()  # one run
        longest = max(longest, int(count.max()))
        assert np.array_equal(first[ph], lo - width)
        assert (np.abs(d[~inside]) < 1e-30).all()
        # the table's entries over the support are the dense kernel's, to one fp32 ulp (sin / cos of libm and of torch may
        # differ in the last float64 bit before the rounding); behind a phase's own support the table holds zeros
        t = np.arange(taps)[None, :]
        idx = np.minimum(lo[:, None] + t, L - 1)
        live = t < count[:, None]
        got = coef[:, ph].T
        want = d[np.arange(len(ph))[:, None], idx]
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32))
        assert (np.abs(got - want)[live] <= ulp[live]).all()
        assert not got[~live].any()
    assert taps == longest
    if (fs_in, fs_out) in EXPECTED_TAPS:
        assert taps == EXPECTED_TAPS[(fs_in, fs_out)]


@pytest.mark.parametrize("fs_in,fs_out", [(44100, 16000), (16000, 44100), (96000, 16000), (8000, 16000)])
def test_table_evaluation_equals_the_dense_float64_definition(built_lib, fs_in, fs_out):
    """The table read the way the kernel reads it (first[p], taps coefficients, ascending) in float64 against the dense
    definition: what the table leaves out is < 1e-30 per entry, so the two agree far beyond fp32 (> 250 dB)."""
    orig, new, _, _ = R.geometry(fs_in, fs_out)
    first, coef, _ = _lib.resample_table(fs_in, fs_out)
    taps = coef.shape[0]
    for n in (1, orig + 1, 1601):
        x = R.noise_rows(1, n, 3)[0].astype(np.float64)
        ref = R.resample64(x, fs_in, fs_out)
        j = np.arange(len(ref))
        f, p = j // new, j % new
        pos = (f * orig + first[p])[:, None] + np.arange(taps)[None, :]
        xv = np.where((pos >= 0) & (pos < n), x[np.clip(pos, 0, n - 1)], 0.0)
        y = (coef[:, p].T.astype(np.float64) * xv).sum(axis=1)
        assert R.snr_db(ref, y) > 250.0


def _check_lengths(L, fs_in, fs_out):
    orig, new, _, _ = R.geometry(fs_in, fs_out)
    for n in sorted({1, 2, orig - 1, orig, orig + 1, 1601, 4411} - {0}):
        want = A.resample(torch.zeros(n), fs_in, fs_out).shape[-1]
        assert L.ou_resample_length(fs_in, fs_out, n) == want == R.out_length(fs_in, fs_out, n), n


@pytest.mark.parametrize("fs_in,fs_out", R.PAIRS[:-1])  # (16 000 -> 16 001: inside the table test, which holds its dense kernel)
def test_length_helper_matches_audio_resample(built_lib, fs_in, fs_out):
    _check_lengths(built_lib, fs_in, fs_out)


def test_length_helper_edges(built_lib):
    assert built_lib.ou_resample_length(16000, 16000, 77) == 77 and built_lib.ou_resample_length(44100, 16000, 0) == 0
    assert built_lib.ou_resample_length(0, 16000, 5) == -1 and built_lib.ou_resample_length(16000, 16000, -1) == -1
    assert built_lib.ou_resample_tile(44100, 16000) > 0 and built_lib.ou_resample_tile(44100, 0) == -1


def test_default_backend_is_the_torch_path_bit_for_bit():
    x = torch.randn(2, 4411, generator=torch.Generator().manual_seed(1))
    for fs, tfs in ((44100, 16000), (16000, 44100), (16000, 16000)):
        a, b = A.resample(x, fs, tfs), A.resample(x, fs, tfs, backend="torch")
        assert a.dtype == b.dtype and torch.equal(a, b)
        many = A.resample_many([x, x[0, :1601]], fs, tfs)
        assert torch.equal(many[0], a) and torch.equal(many[1], A.resample(x[0, :1601], fs, tfs))
    with pytest.raises(ValueError):
        A.resample(x, 44100, 16000, backend="library")  # a CPU tensor: no CPU path, no fallback
    with pytest.raises(ValueError):
        A.resample_many([x], 44100, 16000, backend="library")
    with pytest.raises(ValueError):
        A.resample(x, 44100, 16000, backend="sox")


def test_refusals_decided_on_the_host(built_lib):
    """Every refusal of ou_resample is decided before the first HIP call: OU_EINVAL without a device (the pointers are host
    buffers standing in for device memory; a refused call never reads them)."""
    L = built_lib
    plan = _lib.resample_plan(44100, 16000)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    tb = plan["table_bytes"]

    def call(x_stride=441, lens=(441,), y_stride=160, cols=160, rows=1, fs_in=44100, fs_out=16000, table=ptr, nbytes=tb,
             x=ptr, y=ptr):
        arr = (ctypes.c_int64 * max(1, len(lens)))(*lens)
        return L.ou_resample(x, x_stride, arr, y, y_stride, cols, rows, fs_in, fs_out, table, ctypes.c_size_t(nbytes), None)

    assert call(fs_in=0) == _lib.OU_EINVAL and call(fs_out=-16000) == _lib.OU_EINVAL       # non-positive rates
    assert call(rows=0) == _lib.OU_EINVAL                                                  # rows < 1
    assert call(cols=159) == _lib.OU_EINVAL and b"160 output columns" in L.ou_last_error(None)  # a row that does not fit cols
    assert call(y_stride=159) == _lib.OU_EINVAL                                            # ... or cols that do not fit y_stride
    assert call(lens=(442,)) == _lib.OU_EINVAL and call(lens=(-1,)) == _lib.OU_EINVAL      # 0 <= len[b] <= x_stride
    assert call(nbytes=tb - 4) == _lib.OU_EINVAL and call(nbytes=tb + 4) == _lib.OU_EINVAL  # a wrong table size
    assert call(table=None) == _lib.OU_EINVAL and call(x=None) == _lib.OU_EINVAL and call(y=None) == _lib.OU_EINVAL
    big = 1 << 59
    assert call(x_stride=big, rows=4, lens=(1, 1, 1, 1)) == _lib.OU_EINVAL                  # rows * stride
    assert call(x_stride=big, lens=(big,), y_stride=1 << 60, cols=1 << 60) == _lib.OU_EINVAL  # new * len[b]
    # the host functions refuse the same way
    assert L.ou_resample_plan(0, 16000, None, None, None, None, None) == _lib.OU_EINVAL
    assert L.ou_resample_table(44100, 16000, ptr, ctypes.c_size_t(tb - 4)) == _lib.OU_EINVAL
    with pytest.raises(ValueError):
        _lib.resample_plan(44100, -1)


class _HalfModel:
    """enhance(mix) = 0.5 * mix, on the CPU: the script without a GPU (as test_cli_cpu.py does it)."""
    fs = 16000
    device = "cpu"

    class _KW(dict):
        pass

    diff_kwargs = _KW(n_steps=8, epsilon=1.3)

    def enhance(self, mix, n_steps: int = None, epsilon: float = None, rng: torch.Generator = None,
                keep_rms: bool = False) -> torch.Tensor:
        return 0.5 * mix

    def enhance_many(self, sigs, rngs, pad_batch=False, **kw):
        return [0.5 * s for s in sigs]


def test_cli_resampler_switch(tmp_path):
    parser = cli.build_parser()
    assert parser.parse_args(["a", "b"]).resampler == "torch"
    assert parser.parse_args(["a", "b", "--resampler", "library"]).resampler == "library"
    with pytest.raises(SystemExit):
        parser.parse_args(["a", "b", "--resampler", "sox"])
    src = tmp_path / "in"
    src.mkdir()
    g = torch.Generator().manual_seed(4)
    A.save(src / "a.wav", 0.1 * torch.randn(2, 1103, generator=g), 22050)
    A.save(src / "b.wav", 0.1 * torch.randn(1, 3000, generator=g), 22050)
    A.save(src / "c.wav", 0.1 * torch.randn(1, 800, generator=g), 16000)
    for extra in ([], ["--batch-size", "2"]):
        cli.main([str(src), str(tmp_path / "plain")] + extra, model=_HalfModel())
        cli.main([str(src), str(tmp_path / "torch"), "--resampler", "torch"] + extra, model=_HalfModel())
        for name in ("a.wav", "b.wav", "c.wav"):
            assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "torch" / name).read_bytes()
        # ... and they are what the resample -> enhance -> resample chain of the reference's loop gives
        x, fs = A.load(src / "b.wav")
        want = A.resample(0.5 * A.resample(x, fs, 16000), 16000, fs)
        assert torch.equal(A.load(tmp_path / "plain" / "b.wav")[0], want)
    # the library resampler has no CPU path: asked for on a CPU model it fails loudly instead of falling back
    with pytest.raises(ValueError):
        cli.main([str(src), str(tmp_path / "lib"), "--resampler", "library"], model=_HalfModel())
