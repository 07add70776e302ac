"""GPU (-m gpu): the compression levels of the device FLAC encoder (ou_flac_encode_frames_level, audio.flac_encode_many(level=),
the CLI's --flac-level) against the numpy encoder audio.flac_encode(level=).  Level 0: the bytes of ou_flac_encode_frames.
Level 1: == on the bytes and on the choice records.  Level 2: the stream decodes (every CRC and the MD5 verified) to the quantised
samples, the oracle handed the device's coefficients (lpc_override) gives == on the bytes, and no subframe is longer than its
level-1 form.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import flac_encode_cases as C
import flac_level_cases as LC
from helpers import synth_mix
from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

FS = LC.FS


def _dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).cuda()


def _decoded(stream, bps, tmp_path):
    path = tmp_path / "x.flac"
    path.write_bytes(stream)
    back, fs = A.load_flac(path)
    assert fs == FS
    return np.rint(back.numpy().astype(np.float64) * (1 << (bps - 1))).astype(np.int64)


def _same(got, want, what):
    if got != want:
        first = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError(f"{what}: streams of {len(got)} and {len(want)} bytes differ from byte {first}")


def _check(x, bps, tmp_path, got=None):
    """every level of one signal; got: {level: (stream, records)} from a batched call"""
    ch = x.shape[0]
    q = C.quantise(x, bps)
    lvl1 = None
    for level in (0, 1, 2):
        if got is None:
            (s,), (rec,) = A.flac_encode_many([_dev(x)], FS, bps, level=level, return_choices=True)
        else:
            s, rec = got[level]
        if level < 2:
            want, wrec, _ = LC.oracle(x, bps, level)
            _same(s, want, f"level {level}")
            assert np.array_equal(rec, wrec)
            if level == 0:
                assert s == A.flac_encode_many([_dev(x)], FS, bps)[0] == A.flac_encode(q, FS, bps)
            lvl1 = wrec
        else:
            assert np.array_equal(_decoded(s, bps, tmp_path), q)
            want, wrec, _ = LC.oracle(x, bps, 2, LC.override_from(rec, ch))
            _same(s, want, "level 2 with the device's coefficients")
            assert np.array_equal(rec, wrec)
            assert np.all(rec[:, 5] <= lvl1[:, 5])


@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("n", LC.LENGTHS)
def test_lengths(n, bps, tmp_path):
    _check(LC.content_cases(bps)["ar8_quiet"][:, :n], bps, tmp_path)


@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("name", sorted(LC.content_cases(24)))
def test_contents(name, bps, tmp_path):
    _check(LC.content_cases(bps)[name], bps, tmp_path)


@pytest.mark.parametrize("which", sorted(LC.TIE_SEEDS))
def test_ties(which, tmp_path):
    """two candidates, and two partition orders, at the same price (shown on the CPU: test_flac_level_cpu.py)"""
    _check(LC.tie_signal(which), LC.TIE_BPS, tmp_path)


@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("ch", [2, 8])
def test_channels(ch, bps, tmp_path):
    x = LC.multichannel(ch, 4096 + 48, bps, ch)
    _, rec, _ = LC.oracle(x, bps, 1)
    assert any(b % 8 for b in np.cumsum(rec[:ch, 5])[:-1])  # a subframe starts off a byte boundary
    _check(x, bps, tmp_path)


BATCH = [(1, 1), (2, 17), (1, 4097), (8, 8192 + 48), (2, 64)]


@pytest.mark.parametrize("bps", [16, 24])
def test_batch_of_five(bps, tmp_path):
    sigs = [LC.multichannel(ch, n, bps, 3 + i) for i, (ch, n) in enumerate(BATCH)]
    got = {lv: A.flac_encode_many([_dev(x) for x in sigs], FS, bps, level=lv, return_choices=True) for lv in (0, 1, 2)}
    for i, x in enumerate(sigs):
        for lv in (0, 1, 2):
            (s,), (rec,) = A.flac_encode_many([_dev(x)], FS, bps, level=lv, return_choices=True)
            assert s == got[lv][0][i] and np.array_equal(rec, got[lv][1][i]), (i, lv)  # its single-file call
        _check(x, bps, tmp_path, got={lv: (got[lv][0][i], got[lv][1][i]) for lv in (0, 1, 2)})


def test_batch_of_sixty_five_crosses_the_launch_chunk(tmp_path):
    names = sorted(LC.content_cases(24))
    sigs = [np.roll(LC.content_cases(24)[names[i % len(names)]], 31 * i, axis=1)[:, :300 + 53 * i].repeat(1 + i % 2, axis=0)
            for i in range(65)]
    dev = [_dev(x) for x in sigs]
    got = {lv: A.flac_encode_many(dev, FS, 24, level=lv, return_choices=True) for lv in (1, 2)}
    for i, x in enumerate(sigs):
        want, wrec, q = LC.oracle(x, 24, 1)
        assert got[1][0][i] == want and np.array_equal(got[1][1][i], wrec), i
        rec = got[2][1][i]
        assert got[2][0][i] == LC.oracle(x, 24, 2, LC.override_from(rec, x.shape[0]))[0], i
    for i in (0, 63, 64):
        (s,), (rec,) = A.flac_encode_many([dev[i]], FS, 24, level=2, return_choices=True)
        assert s == got[2][0][i] and np.array_equal(rec, got[2][1][i])
        assert np.array_equal(_decoded(s, 24, tmp_path), C.quantise(sigs[i], 24))


def _raw(x, stride, channels, lens, bps, level, fill):
    """ou_flac_encode_frames_level as it is, on output buffers pre-filled with `fill` -> (streams, records)"""
    L = _lib.load()
    rc, fb, nf, pb, _ = C.sizes(L, channels, lens, bps)
    assert rc == 0
    ch, ln = C.c_arrays(channels, lens)
    cb = ctypes.c_size_t()
    assert L.ou_flac_encode_choices_bytes(len(channels), ch, ln, ctypes.byref(cb)) == 0
    word = fill * 0x01010101 - (1 << 32 if fill >= 0x80 else 0)
    frames = torch.full((fb,), fill, dtype=torch.uint8, device="cuda")
    sizes = torch.full((nf,), word, dtype=torch.int32, device="cuda")
    pcm = torch.full((pb,), fill, dtype=torch.uint8, device="cuda")
    choices = torch.full((cb.value // 4,), word, dtype=torch.int32, device="cuda")
    rc = L.ou_flac_encode_frames_level(ctypes.c_void_p(x.data_ptr()), stride, len(channels), ch, ln, bps, level,
                                       ctypes.c_void_p(frames.data_ptr()), fb, ctypes.c_void_p(sizes.data_ptr()),
                                       ctypes.c_void_p(pcm.data_ptr()), pb, ctypes.c_void_p(choices.data_ptr()), cb.value,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, C.last_error(L)
    torch.cuda.synchronize()
    streams = A._flac_assemble(frames.cpu().numpy(), sizes.cpu().numpy(), pcm.cpu().numpy(), channels, lens, FS, bps)
    return streams, choices.cpu().numpy()


@pytest.mark.parametrize("level", [0, 1, 2])
def test_isolation(level):
    """garbage behind every row's length and between the rows of a padded stride, and whatever the output buffers held before,
    change no byte and no record; two runs agree"""
    bps = 24
    channels, lens = [2, 1, 3], [4096 + 48, 4096, 37]
    sigs = [LC.multichannel(c, n, bps, 5 + i) for i, (c, n) in enumerate(zip(channels, lens))]
    stride = 4096 + 48 + 123
    rows = []
    for x in sigs:
        rows += list(x)
    outs = []
    for junk in (float("nan"), 3.0e38):
        x = torch.full((len(rows), stride), junk, dtype=torch.float32)
        if junk != junk:
            x = x.view(torch.int32).fill_(-1).view(torch.float32)
        for r, row in enumerate(rows):
            x[r, :len(row)] = torch.from_numpy(row)
        x = x.cuda()
        for fill in (0xFF, 0x00):
            outs.append(_raw(x, stride, channels, lens, bps, level, fill))
    outs.append(_raw(x, stride, channels, lens, bps, level, 0x00))
    for streams, rec in outs[1:]:
        assert streams == outs[0][0] and np.array_equal(rec, outs[0][1])
    if level < 2:
        assert outs[0][0] == [LC.oracle(x, bps, level)[0] for x in sigs]
    if level == 0:
        assert outs[0][0] == A.flac_encode_many([_dev(x) for x in sigs], FS, bps)


def test_cli_flac_level(tmp_path):
    model, spec, _ = get_model("PP16s")
    src = tmp_path / "in"
    src.mkdir()
    shapes = [(1, 6000), (2, 7500), (1, 9000)]
    for i, (c, n) in enumerate(shapes):
        sig = torch.cat([synth_mix(spec, 1, n, seed=90 + 2 * i + ch) for ch in range(c)], dim=0)
        A.save(src / f"f{i}.flac", (sig * 0.5).clamp(-1, 1), FS)
    common = ["--seed", "9", "--noise", "counter", "--n_steps", "3"]

    def run(tag, extra):
        cli.main([str(src), str(tmp_path / tag)] + extra + common, model=model)
        return [(tmp_path / tag / f"f{i}.flac").read_bytes() for i in range(len(shapes))]

    parent = run("plain", [])
    assert run("lib0", ["--encoder", "library", "--flac-level", "0"]) == parent
    for tag, extra in (("serial", []), ("batch", ["--batch-size", "3"])):
        a = run(f"numpy1_{tag}", ["--encoder", "numpy", "--flac-level", "1"] + extra)
        b = run(f"library1_{tag}", ["--encoder", "library", "--flac-level", "1"] + extra)
        assert a == b and all(len(x) <= len(y) for x, y in zip(a, parent)), tag
    run("numpy2", ["--encoder", "numpy", "--flac-level", "2"])
    run("library2", ["--encoder", "library", "--flac-level", "2"])
    for i, (c, n) in enumerate(shapes):
        ref, _ = A.load(tmp_path / "plain" / f"f{i}.flac")
        for tag in ("numpy2", "library2", "library1_serial"):
            got, fs = A.load(tmp_path / tag / f"f{i}.flac")
            assert fs == FS and tuple(got.shape) == (c, n) and torch.equal(got, ref), (tag, i)
