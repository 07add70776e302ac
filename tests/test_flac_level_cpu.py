"""CPU: compression levels 1 and 2 of the numpy FLAC encoder (audio.flac_encode(level=), the definition of what the device
writes) and the host side of ou_flac_encode_frames_level / ou_flac_encode_choices_bytes.  Every stream goes through the
library's decoder (every CRC and the MD5 verified) and comes back as the input samples; the choices are checked against an
independent restatement of the pricing rules (flac_level_cases.py) and the bytes against the bit-level test encoder
(flac_ref_encoder.py); the case list is shown to reach every subframe form, partition order, exit and tie of the contract."""
import ctypes

import numpy as np
import pytest
import torch

import flac_encode_cases as C
import flac_level_cases as LC
import flac_ref_encoder as R
from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli

BPS = (16, 24)


def _decode(stream, bps, tmp_path):
    (tmp_path / "x.flac").write_bytes(stream)
    back, fs = A.load_flac(tmp_path / "x.flac")
    assert fs == LC.FS
    return np.rint(back.numpy().astype(np.float64) * (1 << (bps - 1))).astype(np.int64)


def _frames_of(stream, q, bps, rec):
    """the frames of a stream, cut by the lengths its choice records promise"""
    ch, n = q.shape
    out, at = [], 42
    for fno in range((n + LC.BLOCK - 1) // LC.BLOCK):
        bits = int(sum(rec[fno * ch + c][5] for c in range(ch)))
        size = 4 + len(R.utf8_number(fno)) + 3 + (bits + 7) // 8 + 2
        out.append(stream[at:at + size])
        at += size
    assert at == len(stream)
    return out


def test_level_0_is_the_stream_it_was():
    for bps in BPS:
        for name in ("noise3", "kink", "zeros"):
            q = C.quantise(LC.content_cases(bps)[name], bps)
            assert A.flac_encode(q, LC.FS, bps, level=0) == A.flac_encode(q, LC.FS, bps)
        for name, x in C.content_cases(bps).items():
            q = C.quantise(x, bps)
            s, rec = A.flac_encode(q, LC.FS, bps, level=0, return_choices=True)
            assert s == A.flac_encode(q, LC.FS, bps), name
            want = [(A.FLAC_FIXED, 2) if kind == "rice" else (A.FLAC_VERBATIM, 0) for kind, _ in C.choices(q, bps)]
            assert [(int(r[0]), int(r[1])) for r in rec] == want and not rec[:, 2:5].any()


@pytest.mark.parametrize("bps", BPS)
@pytest.mark.parametrize("name", sorted(LC.content_cases(24)))
def test_streams_decode_lengths_fall_and_the_reference_encoder_agrees(name, bps, tmp_path):
    x = LC.content_cases(bps)[name]
    prev = None
    for level in (0, 1, 2):
        s, rec, q = LC.oracle(x, bps, level)
        assert np.array_equal(_decode(s, bps, tmp_path), q)
        if prev is not None:
            assert np.all(rec[:, 5] <= prev[:, 5])  # level 2 <= level 1 <= level 0, per subframe
        prev = rec
        if level == 0:
            continue
        # the same frames from the independent bit-level encoder; its header codes a block of <= 256 samples in 8 bits, ours
        # always in 16: there the bytes behind the header are compared
        for fr, ref, s0 in zip(_frames_of(s, q, bps, rec), LC.rebuild(q, bps, rec), range(0, q.shape[1], LC.BLOCK)):
            if q.shape[1] - s0 > 256:
                assert fr == ref
            else:
                assert fr[8:-2] == ref[7:-2]  # (frame numbers below 128: headers of 8 and 7 bytes)
        # every record is the cheapest by the restated rules
        for i, r in enumerate(rec):
            blk = q[0, i * LC.BLOCK:(i + 1) * LC.BLOCK]
            if r[0] in (A.FLAC_FIXED, A.FLAC_LPC):
                coefs = R.FIXED[int(r[1])] if r[0] == A.FLAC_FIXED else [int(v) for v in r[6:6 + r[1]]]
                per_po = [LC.price(blk, bps, coefs, int(r[4]), r[0] == A.FLAC_LPC, po) for po in LC.allowed_orders(len(blk))]
                assert per_po[int(r[2])] == r[5] == min(v for v in per_po if v is not None)
                assert [v for v in per_po if v is not None].index(r[5]) == [po for po, v in enumerate(per_po) if v is not None].index(int(r[2]))
            if level == 1:
                alive = {k: v for k, v in LC.fixed_prices(blk, bps).items() if v is not None}
                if r[0] == A.FLAC_FIXED:
                    assert f"fixed{int(r[1])}" == min(alive, key=lambda k: (alive[k], list(alive).index(k)))
                elif r[0] == A.FLAC_CONSTANT:
                    assert alive["constant"] == min(alive.values()) == r[5]


def test_the_case_list_reaches_everything_the_contract_names():
    seen, exits, lpc_po = set(), set(), set()
    for bps in BPS:
        for name, x in LC.content_cases(bps).items():
            for level in (1, 2):
                _, rec, q = LC.oracle(x, bps, level)
                for i, r in enumerate(rec):
                    seen.add((LC.KINDS[int(r[0])], int(r[1]), int(r[2])))
                    if r[0] == A.FLAC_VERBATIM and level == 1:
                        blk = q[0, i * LC.BLOCK:(i + 1) * LC.BLOCK]
                        exits.add("quotient" if all(v is None for v in LC.fixed_prices(blk, bps).values()) else "length")
    assert ("constant", 0, 0) in seen and exits == {"quotient", "length"}
    assert {o for k, o, _ in seen if k == "fixed"} == {0, 1, 2, 3, 4}
    assert {po for k, _, po in seen if k in ("fixed", "lpc")} == set(range(7))
    assert any(k == "lpc" for k, _, _ in seen)
    # the last block of 48 samples: orders 0 and 1 alone (divisibility); a block of 31 or 16: order 0 alone (the floor)
    assert LC.allowed_orders(48) == [0, 1] and LC.allowed_orders(4096) == list(range(7))
    assert LC.allowed_orders(32) == [0, 1] and LC.allowed_orders(16) == [0] and LC.allowed_orders(24) == [0]
    assert LC.content_cases(24)["zeros"].shape[1] % LC.BLOCK == 48
    _, rec, _ = LC.oracle(LC.content_cases(24)["tail"], 24, 1)
    assert rec[-1][0] == A.FLAC_FIXED and rec[-1][2] == 1  # partitions pay in the 48-sample block: order 1, the finest it may take


def test_ties_go_to_the_earlier_candidate_and_the_smaller_partition_order():
    x = LC.tie_signal("candidate")
    q = C.quantise(x, LC.TIE_BPS)[0]
    pr = LC.fixed_prices(q, LC.TIE_BPS)
    assert pr["fixed0"] == pr["fixed1"] == min(pr.values())
    _, rec, _ = LC.oracle(x, LC.TIE_BPS, 1)
    assert tuple(rec[0][:3]) == (A.FLAC_FIXED, 0, 0) and rec[0][5] == pr["fixed0"]
    x = LC.tie_signal("partition")
    q = C.quantise(x, LC.TIE_BPS)[0]
    _, rec, _ = LC.oracle(x, LC.TIE_BPS, 1)
    p = int(rec[0][1])
    assert LC.price(q, LC.TIE_BPS, R.FIXED[p], 0, False, 0) == LC.price(q, LC.TIE_BPS, R.FIXED[p], 0, False, 1) == rec[0][5]
    assert rec[0][0] == A.FLAC_FIXED and rec[0][2] == 0


def test_lpc_drop_rules_and_the_override(tmp_path):
    q = C.quantise(LC.content_cases(24)["ar8"][:, :LC.BLOCK], 24)
    s, rec = A.flac_encode(q, LC.FS, 24, level=2, return_choices=True)
    assert rec[0][0] == A.FLAC_LPC and rec[0][1] == 8 and rec[0][3] == 14 and 0 <= rec[0][4] <= 15
    # the override hands the same coefficients back: the same stream; other coefficients: another stream that still decodes
    assert A.flac_encode(q, LC.FS, 24, level=2, lpc_override=LC.override_from(rec, 1)) == s
    s2, rec2 = A.flac_encode(q, LC.FS, 24, level=2, lpc_override={(0, 0): ([4096, -2048], 12)}, return_choices=True)
    assert np.array_equal(_decode(s2, 24, tmp_path), q)
    level1 = A.flac_encode(q, LC.FS, 24, level=1, return_choices=True)
    assert rec2[0][5] <= level1[1][0][5]
    # dropped: a coefficient outside 14 bits; a residual outside 32 bits (shift 0, full-scale input); a degenerate analysis
    loud = np.full((1, 64), (1 << 23) - 1, np.int64)
    loud[0, ::2] = -(1 << 23)
    for x, ov in ((q, ([8192, 0, 0, 0, 0, 0, 0, 0], 13)), (q, ([-8193] + [0] * 7, 13)), (loud, ([8191] * 8, 0)),
                  (loud, ([-8192, 8191] * 4, 0))):
        s3, rec3 = A.flac_encode(x, LC.FS, 24, level=2, lpc_override={(0, 0): ov}, return_choices=True)
        assert (s3, rec3.tolist()) == tuple(v if i == 0 else v.tolist() for i, v in enumerate(
            A.flac_encode(x, LC.FS, 24, level=1, return_choices=True)))
    assert A._lpc_analysis(np.zeros(4096, np.int64)) is None                      # zero energy
    spike = C.quantise(LC.content_cases(24)["spike"][:, :LC.BLOCK], 24)[0]
    assert A._lpc_analysis(spike) is None                                         # every coefficient zero
    assert A.flac_encode(q[:, :63], LC.FS, 24, level=2) == A.flac_encode(q[:, :63], LC.FS, 24, level=1)  # n < 64: not built
    with pytest.raises(ValueError):
        A.flac_encode(q, LC.FS, 24, level=3)


def test_save_flac_passes_the_level_on(tmp_path):
    x = torch.from_numpy(np.array(LC.content_cases(24)["ar8_quiet"]))
    sizes = []
    for level in (0, 1, 2):
        A.save_flac(tmp_path / f"{level}.flac", x, LC.FS, level=level)
        data = (tmp_path / f"{level}.flac").read_bytes()
        assert data == LC.oracle(x.numpy(), 24, level)[0]
        sizes.append(len(data))
    A.save_flac(tmp_path / "d.flac", x, LC.FS)
    assert (tmp_path / "d.flac").read_bytes() == (tmp_path / "0.flac").read_bytes() and sizes[2] <= sizes[1] <= sizes[0]


def test_choices_bytes_closed_form_and_refusals(built_lib):
    L = built_lib
    for name in ("ou_flac_encode_choices_bytes", "ou_flac_encode_frames_level"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert A.FLAC_CHOICE_WORDS == 18 and A.FLAC_CHOICE_COEFS == 12
    channels, lens = [1, 2, 8, 3], [1, 4096, 4097, 20000]
    ch, ln = C.c_arrays(channels, lens)
    cb = ctypes.c_size_t()
    assert L.ou_flac_encode_choices_bytes(4, ch, ln, ctypes.byref(cb)) == _lib.OU_OK
    assert cb.value == 4 * A.FLAC_CHOICE_WORDS * sum(c * ((n + 4095) // 4096) for c, n in zip(channels, lens))
    assert L.ou_flac_encode_choices_bytes(4, ch, ln, None) == _lib.OU_EINVAL
    for bad_ch, bad_len, files, word in (([1], [10], 0, "files"), ([0], [10], 1, "channels"), ([9], [10], 1, "channels"),
                                          ([1], [0], 1, "len[0]"), ([1], [2 ** 36], 1, "len[0]")):
        bc, bl = C.c_arrays(bad_ch, bad_len)
        assert L.ou_flac_encode_choices_bytes(files, bc, bl, ctypes.byref(cb)) == _lib.OU_EINVAL
        assert word in C.last_error(L) and "ou_flac_encode_choices_bytes" in C.last_error(L)


@pytest.mark.parametrize("channels,lens,bps,files,word", [
    ([1], [10], 24, 0, "files"), ([0], [10], 24, None, "channels"), ([9], [10], 24, None, "channels"),
    ([1, 2], [10, 0], 24, None, "len[1]"), ([1], [2 ** 36], 24, None, "len[0]"), ([1], [10], 8, None, "bits per sample"),
    ([1], [10], 20, None, "bits per sample"),
])
def test_frames_level_refuses_what_encode_frames_refuses(built_lib, channels, lens, bps, files, word):
    L = built_lib
    n = len(channels) if files is None else files
    ch, ln = C.c_arrays(channels, lens)
    fake = ctypes.c_void_p(4096)  # never followed: the refusal comes before any HIP call
    for level in (0, 1, 2):
        assert L.ou_flac_encode_frames_level(fake, 1 << 40, n, ch, ln, bps, level, fake, 1 << 40, fake, fake, 1 << 40, None, 0,
                                             None) == _lib.OU_EINVAL
        assert word in C.last_error(L) and "ou_flac_encode_frames_level" in C.last_error(L)


def test_frames_level_refusals_of_its_own(built_lib):
    L = built_lib
    ch, ln = C.c_arrays([2, 1], [100, 5000])
    fake, odd, odd2 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4098)
    _, fb, _, pb, _ = C.sizes(L, [2, 1], [100, 5000], 24)
    cb = ctypes.c_size_t()
    assert L.ou_flac_encode_choices_bytes(2, ch, ln, ctypes.byref(cb)) == 0 and cb.value == 4 * 18 * 4

    def call(stride=5000, frames=fake, fbytes=fb, sizes=fake, pcm=fake, pbytes=pb, x=fake, level=1, choices=fake, cbytes=cb.value):
        return L.ou_flac_encode_frames_level(x, stride, 2, ch, ln, 24, level, frames, fbytes, sizes, pcm, pbytes, choices, cbytes, None)

    for level in (-1, 3):
        assert call(level=level) == _lib.OU_EINVAL and "level" in C.last_error(L)
    assert call(stride=4999) == _lib.OU_EINVAL and "row_stride" in C.last_error(L)
    assert call(x=None) == _lib.OU_EINVAL and call(frames=None) == _lib.OU_EINVAL
    assert call(sizes=None) == _lib.OU_EINVAL and call(pcm=None) == _lib.OU_EINVAL
    assert call(frames=odd) == _lib.OU_EINVAL and "aligned" in C.last_error(L)
    assert call(pcm=odd) == _lib.OU_EINVAL
    assert call(stride=1 << 61) == _lib.OU_EINVAL and "overflows" in C.last_error(L)
    assert call(fbytes=fb - 1) == _lib.OU_ESHAPE and call(pbytes=pb - 1) == _lib.OU_ESHAPE
    assert call(choices=odd2) == _lib.OU_EINVAL and "choices" in C.last_error(L)
    assert call(cbytes=cb.value - 1) == _lib.OU_ESHAPE and "ou_flac_encode_choices_bytes" in C.last_error(L)
    assert call(choices=odd2, level=0) == _lib.OU_EINVAL and call(cbytes=0, level=0) == _lib.OU_ESHAPE


def test_cli_flag_and_python_arguments():
    parser = cli.build_parser()
    assert parser.parse_args(["a", "b"]).flac_level == 0
    assert parser.parse_args(["a", "b", "--flac-level", "2"]).flac_level == 2
    with pytest.raises(SystemExit):
        parser.parse_args(["a", "b", "--flac-level", "3"])
    with pytest.raises(ValueError):
        A.flac_encode_many([torch.zeros(100)], 16000, level=1)  # no CPU path
    with pytest.raises(ValueError):
        A.flac_encode_many([], 16000, level=5)
    assert A.flac_encode_many([], 16000, level=2) == [] and A.flac_encode_many([], 16000, return_choices=True) == ([], [])
