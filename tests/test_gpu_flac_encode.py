"""GPU (-m gpu): the device FLAC encoder (ou_flac_encode_frames + ou_flac_assemble, audio.flac_encode_many / save_flac_many, the
CLI's --encoder library) against the numpy encoder.  Expected value everywhere: audio.flac_encode(q, fs, bps) of the
float64-quantised samples, compared with == on the bytes; then audio.load_flac of the result (every CRC and the MD5 verified by
the library's decoder) compared with q exactly.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import flac_encode_cases as C
from helpers import synth_mix
from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

FS = 16000


def _dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).cuda()  # (a copy: the shared cases are read-only)


def _check(x, bps, tmp_path, fs=FS, got=None):
    """x: float32 (C, T) -> the device encoder's stream equals the oracle's and decodes to the quantised samples"""
    want, q = C.oracle(x, fs, bps)
    if got is None:
        got, = A.flac_encode_many([_dev(x)], fs, bps)
    assert isinstance(got, bytes) and len(got) == len(want)
    if got != want:
        first = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"streams differ from byte {first} of {len(want)}")
    path = tmp_path / "x.flac"
    path.write_bytes(got)
    back, gfs = A.load_flac(path)
    assert gfs == fs and np.array_equal(np.rint(back.numpy().astype(np.float64) * (1 << (bps - 1))).astype(np.int64), q)
    return got


@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("n", [1, 2, 3, 4095, 4096, 4097, 8192])
def test_lengths(n, bps, tmp_path):
    _check(C.noise(n, 0.01, 40 + n % 7), bps, tmp_path)


@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("name", sorted(C.content_cases(24)))
def test_contents(name, bps, tmp_path):
    _check(C.content_cases(bps)[name], bps, tmp_path)


def test_the_content_set_reaches_every_k_and_both_verbatim_exits():
    """from the oracle's own streams, so the set cannot silently shrink"""
    seen = set()
    for x in C.content_cases(24).values():
        seen |= set(C.choices(C.quantise(x, 24), 24))
    assert {k for kind, k in seen if kind == "rice"} == set(range(15))
    assert {"quotient", "length"} <= {kind for kind, _ in seen}
    assert ("short", None) in C.choices(C.quantise(np.zeros((1, 4098), np.float32), 24), 24)  # n < 3: the lengths above


@pytest.mark.parametrize("margin", [1, 0, -1])
def test_fallback_inequality(margin, tmp_path):
    """a block whose Rice form is one bit shorter than, as long as and one bit longer than verbatim"""
    x = C.fallback_signal(C.FALLBACK_SEEDS[margin])
    assert C.fallback_margin(x) == margin
    kind = C.choices(C.quantise(x, C.FALLBACK_BPS), C.FALLBACK_BPS)[0][0]
    assert kind == ("rice" if margin > 0 else "length")
    _check(x, C.FALLBACK_BPS, tmp_path)


@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("ch", [1, 2, 8])
def test_channels(ch, bps, tmp_path):
    x = C.multichannel(ch, 4096 + 1501, 11 + ch)
    if ch > 1:
        bits = [C.subframe_choice(C.quantise(x, bps)[c, :4096], bps)[1] for c in range(ch)]
        assert any(b % 8 for b in np.cumsum(bits)[:-1])  # a subframe starts off a byte boundary
    _check(x, bps, tmp_path)


BATCH = [(1, 1), (2, 3), (1, 4097), (8, 12289), (2, 20000)]


@pytest.mark.parametrize("bps", [16, 24])
def test_batch_of_five(bps, tmp_path):
    sigs = [C.multichannel(ch, n, 20 + i) for i, (ch, n) in enumerate(BATCH)]
    got = A.flac_encode_many([_dev(x) for x in sigs], FS, bps)
    assert len(got) == len(sigs)
    for x, g in zip(sigs, got):
        assert g == A.flac_encode_many([_dev(x)], FS, bps)[0]  # its single-file call
        _check(x, bps, tmp_path, got=g)                        # and the oracle
    # a (T,) tensor is a mono file
    assert A.flac_encode_many([_dev(sigs[2][0])], FS, bps)[0] == got[2]


def test_batch_of_sixty_five_crosses_the_launch_chunk(tmp_path):
    sigs = [C.noise(700 + 53 * i, 2.0 ** (-4 - i % 9), 300 + i, ch=1 + i % 2) for i in range(65)]
    got = A.flac_encode_many([_dev(x) for x in sigs], FS, 24)
    for i in (0, 1, 31, 62, 63, 64):
        _check(sigs[i], 24, tmp_path, got=got[i])
    for i, (x, g) in enumerate(zip(sigs, got)):
        assert g == C.oracle(x, FS, 24)[0], i


def _raw(x, stride, channels, lens, bps, fill):
    """ou_flac_encode_frames as it is, on output buffers pre-filled with `fill` -> streams"""
    L = _lib.load()
    rc, fb, nf, pb, _ = C.sizes(L, channels, lens, bps)
    assert rc == 0
    frames = torch.full((fb,), fill, dtype=torch.uint8, device="cuda")
    sizes = torch.full((nf,), fill * 0x01010101 - (1 << 32 if fill >= 0x80 else 0), dtype=torch.int32, device="cuda")
    pcm = torch.full((pb,), fill, dtype=torch.uint8, device="cuda")
    ch, ln = C.c_arrays(channels, lens)
    rc = L.ou_flac_encode_frames(ctypes.c_void_p(x.data_ptr()), stride, len(channels), ch, ln, bps, ctypes.c_void_p(frames.data_ptr()),
                                 fb, ctypes.c_void_p(sizes.data_ptr()), ctypes.c_void_p(pcm.data_ptr()), pb,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, C.last_error(L)
    torch.cuda.synchronize()
    return A._flac_assemble(frames.cpu().numpy(), sizes.cpu().numpy(), pcm.cpu().numpy(), channels, lens, FS, bps)


@pytest.mark.parametrize("bps", [16, 24])
def test_isolation(bps):
    """garbage behind every row's length and between the rows of a padded stride, and whatever the output buffers held before,
    change no byte; two runs agree"""
    channels, lens = [2, 1, 3], [5000, 4096, 37]
    sigs = [C.multichannel(c, n, 60 + i) for i, (c, n) in enumerate(zip(channels, lens))]
    want = [C.oracle(x, FS, bps)[0] for x in sigs]
    stride = 5000 + 123
    rows = []
    for x in sigs:
        rows += list(x)
    outs = []
    for junk in (float("nan"), 3.0e38):
        x = torch.full((len(rows), stride), junk, dtype=torch.float32)
        if junk != junk:  # NaNs with the sign and payload bits set
            x = x.view(torch.int32).fill_(-1).view(torch.float32)
        for r, row in enumerate(rows):
            x[r, :len(row)] = torch.from_numpy(row)
        x = x.cuda()
        for fill in (0xFF, 0x00):
            outs.append(_raw(x, stride, channels, lens, bps, fill))
    outs.append(_raw(x, stride, channels, lens, bps, 0x00))
    for got in outs:
        assert got == want


def test_nan_encodes_as_zero(tmp_path):
    x = C.noise(300, 0.1, 1)
    x[0, [0, 17, 299]] = np.nan
    got, = A.flac_encode_many([_dev(x)], FS, 24)
    clean = x.copy()
    clean[np.isnan(clean)] = 0.0
    assert got == C.oracle(clean, FS, 24)[0]


def test_cli_library_encoder_writes_the_files_of_the_default(tmp_path):
    model, spec, _ = get_model("PP16s")
    src = tmp_path / "in"
    src.mkdir()
    shapes = [(1, 6000), (2, 7500), (1, 9000)]
    for i, (c, n) in enumerate(shapes):
        sig = torch.cat([synth_mix(spec, 1, n, seed=90 + 2 * i + ch) for ch in range(c)], dim=0)
        A.save(src / f"f{i}.flac", (sig * 0.5).clamp(-1, 1), FS)
    common = ["--seed", "9", "--noise", "counter", "--n_steps", "3"]
    for tag, extra in (("serial", []), ("batch", ["--batch-size", "3"])):
        cli.main([str(src), str(tmp_path / f"numpy_{tag}"), "--encoder", "numpy"] + extra + common, model=model)
        cli.main([str(src), str(tmp_path / f"library_{tag}"), "--encoder", "library"] + extra + common, model=model)
        for i, (c, n) in enumerate(shapes):
            a = (tmp_path / f"numpy_{tag}" / f"f{i}.flac").read_bytes()
            b = (tmp_path / f"library_{tag}" / f"f{i}.flac").read_bytes()
            assert a == b and len(a) > 42, (tag, i)
            got, fs = A.load(tmp_path / f"library_{tag}" / f"f{i}.flac")
            assert fs == FS and tuple(got.shape) == (c, n)
