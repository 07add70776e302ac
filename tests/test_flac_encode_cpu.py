"""CPU: the host side of the device FLAC encoder -- refusals of ou_flac_encode_sizes / ou_flac_encode_frames / ou_flac_assemble
(decided before any HIP call: this machine has no device and none is needed), the buffer sizes against their closed form,
ou_flac_assemble against streams of the numpy encoder (audio.flac_encode: frames, sizes and samples are cut out of its stream
and must come back as that stream, byte for byte), and the integer rule for the Rice parameter against the floating-point one of
audio._subframe_bits."""
import ctypes

import numpy as np
import pytest
import torch

import flac_encode_cases as C
from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli

NEW_SYMBOLS = ["ou_flac_encode_sizes", "ou_flac_encode_frames", "ou_flac_assemble"]


def test_symbols_are_exported(built_lib):
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(built_lib, name)


def test_sizes_against_the_closed_form(built_lib):
    for bps in (16, 24):
        channels, lens = [1, 2, 8, 3], [1, 4096, 4097, 20000]
        rc, fb, nf, pb, cap = C.sizes(built_lib, channels, lens, bps)
        assert rc == _lib.OU_OK
        blocks = [(n + 4095) // 4096 for n in lens]
        # one slot per block: header, `channels` verbatim subframes, CRC-16, rounded up to 16 bytes
        slot = [(16 + (c * (8 + 4096 * bps) + 7) // 8 + 2 + 15) // 16 * 16 for c in channels]
        assert slot == [C.slot_bytes(c, bps) for c in channels]
        assert fb == sum(b * s for b, s in zip(blocks, slot)) and nf == sum(blocks)
        assert pb == sum((c * n * (bps // 8) + 15) // 16 * 16 for c, n in zip(channels, lens))
        assert cap == [42 + b * C.frame_max(c, bps) for b, c in zip(blocks, channels)]
    assert C.sizes(built_lib, [1], [2 ** 36 - 1], 24)[0] == _lib.OU_OK


@pytest.mark.parametrize("channels,lens,bps,files,word", [
    ([1], [10], 24, 0, "files"),
    ([0], [10], 24, None, "channels"),
    ([9], [10], 24, None, "channels"),
    ([1, 2], [10, 0], 24, None, "len[1]"),
    ([1], [2 ** 36], 24, None, "len[0]"),
    ([1], [10], 8, None, "bits per sample"),
    ([1], [10], 20, None, "bits per sample"),
])
def test_refusals_of_every_call(built_lib, channels, lens, bps, files, word):
    L = built_lib
    n = len(channels) if files is None else files
    assert C.sizes(L, channels, lens, bps, files)[0] == _lib.OU_EINVAL
    assert word in C.last_error(L) and "ou_flac_encode_sizes" in C.last_error(L)
    ch, ln = C.c_arrays(channels, lens)
    # (a pointer that is never followed: the refusal comes before any HIP call, and this machine has no device to launch on)
    fake = ctypes.c_void_p(4096)
    assert L.ou_flac_encode_frames(fake, 1 << 40, n, ch, ln, bps, fake, 1 << 40, fake, fake, 1 << 40, None) == _lib.OU_EINVAL
    assert word in C.last_error(L) and "ou_flac_encode_frames" in C.last_error(L)
    buf = np.zeros(4096, np.uint8)
    off = (ctypes.c_int64 * 3)()
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.ou_flac_assemble(p, p, p, n, ch, ln, 16000, bps, p, buf.nbytes, off) == _lib.OU_EINVAL
    assert word in C.last_error(L) and "ou_flac_assemble" in C.last_error(L)


def test_refusals_of_the_device_call_alone(built_lib):
    L = built_lib
    ch, ln = C.c_arrays([2, 1], [100, 300])
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    _, fb, _, pb, _ = C.sizes(L, [2, 1], [100, 300], 24)
    call = lambda stride=300, frames=fake, fbytes=fb, sizes=fake, pcm=fake, pbytes=pb, x=fake: L.ou_flac_encode_frames(  # noqa: E731
        x, stride, 2, ch, ln, 24, frames, fbytes, sizes, pcm, pbytes, None)
    assert call(stride=299) == _lib.OU_EINVAL and "row_stride" in C.last_error(L)
    assert call(x=None) == _lib.OU_EINVAL and call(frames=None) == _lib.OU_EINVAL
    assert call(sizes=None) == _lib.OU_EINVAL and call(pcm=None) == _lib.OU_EINVAL
    assert call(frames=odd) == _lib.OU_EINVAL and "aligned" in C.last_error(L)
    assert call(pcm=odd) == _lib.OU_EINVAL
    assert call(stride=1 << 61) == _lib.OU_EINVAL and "overflows" in C.last_error(L)
    assert call(fbytes=fb - 1) == _lib.OU_ESHAPE and "ou_flac_encode_sizes" in C.last_error(L)
    assert call(pbytes=pb - 1) == _lib.OU_ESHAPE


def _cut(stream, q, bps):
    """the three buffers ou_flac_encode_frames would hand over, cut out of a stream of the numpy encoder (CRC-16 bytes blanked)"""
    ch, n = q.shape
    fsz = C.frame_sizes(q, bps)
    slot = C.slot_bytes(ch, bps)
    frames = np.full(len(fsz) * slot, 0xA5, np.uint8)
    at = 42
    for i, sz in enumerate(fsz):
        frames[i * slot:i * slot + sz - 2] = np.frombuffer(stream[at:at + sz - 2], np.uint8)
        at += sz
    assert at == len(stream)
    nb = bps // 8
    inter = np.ascontiguousarray(q.T).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :nb]
    pcm = np.full(C.pcm_bytes(ch, n, bps), 0x5A, np.uint8)
    pcm[:ch * n * nb] = inter.ravel()
    return frames, np.array(fsz, np.int32), pcm


def _assemble(L, parts, channels, lens, fs, bps, capacity=None):
    frames = np.concatenate([p[0] for p in parts])
    sizes = np.concatenate([p[1] for p in parts])
    pcm = np.concatenate([p[2] for p in parts])
    ch, ln = C.c_arrays(channels, lens)
    cap = sum(C.sizes(L, channels, lens, bps)[4]) if capacity is None else capacity
    out = np.zeros(max(cap, 1), np.uint8)
    off = (ctypes.c_int64 * (len(channels) + 1))()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = L.ou_flac_assemble(vp(frames), vp(sizes), vp(pcm), len(channels), ch, ln, fs, bps, vp(out), cap, off)
    return rc, [out[off[i]:off[i + 1]].tobytes() for i in range(len(channels))] if rc == 0 else None


@pytest.mark.parametrize("bps", [16, 24])
def test_assemble_gives_back_the_numpy_encoders_stream(built_lib, bps):
    fs = 16000
    n = 2 * 4096 + 1234  # 3 blocks
    sigs = [C.noise(n, 0.05, 5, ch=1), C.multichannel(2, n, 6)]
    streams, parts = [], []
    for x in sigs:
        s, q = C.oracle(x, fs, bps)
        streams.append(s)
        parts.append(_cut(s, q, bps))
    for i in range(2):  # each alone
        rc, got = _assemble(built_lib, [parts[i]], [i + 1], [n], fs, bps)
        assert rc == _lib.OU_OK and got == [streams[i]]
    rc, got = _assemble(built_lib, parts, [1, 2], [n, n], fs, bps)  # and both in one call
    assert rc == _lib.OU_OK and got == streams
    # exactly enough room passes, one byte less is OU_ESHAPE; a frame size the kernel cannot have written is OU_EINVAL
    need = len(streams[0]) + len(streams[1])
    assert _assemble(built_lib, parts, [1, 2], [n, n], fs, bps, capacity=need)[0] == _lib.OU_OK
    assert _assemble(built_lib, parts, [1, 2], [n, n], fs, bps, capacity=need - 1)[0] == _lib.OU_ESHAPE
    bad = [(parts[0][0], parts[0][1].copy(), parts[0][2])]
    bad[0][1][1] = C.frame_max(1, bps) + 1
    assert _assemble(built_lib, bad, [1], [n], fs, bps)[0] == _lib.OU_EINVAL
    for fs_bad in (0, 1 << 20):
        assert _assemble(built_lib, [parts[0]], [1], [n], fs_bad, bps)[0] == _lib.OU_EINVAL and "fs" in C.last_error(built_lib)


def test_assembled_stream_passes_the_decoder(built_lib, tmp_path):
    x = C.multichannel(2, 5000, 3)
    s, q = C.oracle(x, 22050, 24)
    rc, got = _assemble(built_lib, [_cut(s, q, 24)], [2], [5000], 22050, 24)
    assert rc == _lib.OU_OK
    (tmp_path / "a.flac").write_bytes(got[0])
    back, fs = A.load_flac(tmp_path / "a.flac")  # every CRC and the MD5 verified
    assert fs == 22050 and np.array_equal(back.numpy().astype(np.float64) * 2 ** 23, q)


def test_integer_rule_for_k_agrees_with_the_logarithm():
    """the largest k <= 14 with (2^k - 1) (n - 2) <= sum u  ==  clamp(floor(log2(mean(u) + 1)), 0, 14), on both sides of and on
    every boundary"""
    for n in (3, 4, 4096):
        m = n - 2
        for k in range(0, 16):
            edge = ((1 << k) - 1) * m
            for total in {max(edge - 1, 0), edge, edge + 1, edge + m - 1, edge + m // 2}:
                # residuals with this sum, spread as evenly as integers allow and, for the mean's summation order, as one spike
                even = np.full(m, total // m, np.uint64)
                even[:total % m] += np.uint64(1)
                spike = np.zeros(m, np.uint64)
                spike[m // 2] = total
                for u in (even, spike):
                    assert int(u.sum()) == total
                    assert C.integer_k(total, n) == C.log2_k(u), (n, k, total)


def test_cli_flag_and_cpu_tensors():
    parser = cli.build_parser()
    assert parser.parse_args(["a", "b"]).encoder == "numpy"
    assert parser.parse_args(["a", "b", "--encoder", "library"]).encoder == "library"
    with pytest.raises(SystemExit):
        parser.parse_args(["a", "b", "--encoder", "sox"])
    with pytest.raises(ValueError):  # no CPU path and no fallback
        A.flac_encode_many([torch.zeros(100)], 16000)
    with pytest.raises(ValueError):
        A.save_flac_many(["a.flac", "b.flac"], [torch.zeros(100)], 16000)
    assert A.flac_encode_many([], 16000) == []
