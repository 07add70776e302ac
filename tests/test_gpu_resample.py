"""GPU (-m gpu): the library's resampler (ou_resample, audio.resample(backend="library"), audio.resample_many, the CLI's
--resampler library) against a float64 evaluation of the definition (resample_reference.py: numpy, dense kernel, no code
shared with the path under test).

Accuracy gate, measured in the test: d_ref = SNR of the existing fp32 path (audio.resample, default backend, on the CPU)
against the float64 evaluation; the library must reach d_ref - 6 dB against the same evaluation (one factor of two in error
amplitude for a different but fixed summation order and fused multiply-adds).  Both figures are recorded per case."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import resample_reference as R
import restatement as O
from helpers import gate, record, synth_mix
from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli
from test_gpu_parity import get_model

pytestmark = pytest.mark.gpu

MARGIN_DB = 6.0
# beyond the issue's eight pairs: a workgroup of 128 threads (the span of 1024 outputs of 192 000 -> 8 000 does not fit LDS) and a
# filter of 758 taps whose span fits no workgroup (1 MHz -> 16 kHz: one thread per output, no staging)
EXTRA_PAIRS = [(192000, 8000), (1000000, 16000)]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(fs_in, fs_out):
    return torch.from_numpy(_lib.resample_table(fs_in, fs_out)[2]).cuda()


def _call(x, lens, y, cols, fs_in, fs_out, table, nbytes=None):
    """ou_resample as it is: x (rows, x_stride), y (rows, y_stride) device tensors, table a device uint8 tensor or None"""
    L = _lib.load()
    rows = len(lens)
    return L.ou_resample(ctypes.c_void_p(x.data_ptr()), x.stride(0), (ctypes.c_int64 * rows)(*lens), ctypes.c_void_p(y.data_ptr()),
                         y.stride(0), cols, rows, fs_in, fs_out, None if table is None else ctypes.c_void_p(table.data_ptr()),
                         ctypes.c_size_t((0 if table is None else table.numel()) if nbytes is None else nbytes), _stream())


def _ragged(rows_np, fs_in, fs_out, pad_value=0.0, y_extra=0, y_fill=0.0, table=None):
    """One call over rows of their own lengths -> (y (rows, cols + y_extra) on the CPU, out lengths, cols)"""
    L = _lib.load()
    lens = [len(r) for r in rows_np]
    stride = max(4, (max(lens) + 3) // 4 * 4 + 4)
    x = torch.full((len(lens), stride), pad_value, dtype=torch.float32)
    for b, r in enumerate(rows_np):
        x[b, :len(r)] = torch.from_numpy(np.asarray(r, dtype=np.float32))
    out_lens = [int(L.ou_resample_length(fs_in, fs_out, n)) for n in lens]
    cols = max(1, max(out_lens))
    y = torch.full((len(lens), cols + y_extra), y_fill, dtype=torch.float32).cuda()
    xd = x.cuda()
    table = _table(fs_in, fs_out) if table is None else table
    assert _call(xd, lens, y, cols, fs_in, fs_out, table) == _lib.OU_OK, L.ou_last_error(None)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x) or pad_value != pad_value  # the input is left alone (NaN padding compares unequal)
    return y.cpu(), out_lens, cols


def _lengths(fs_in, fs_out):
    orig, new, _, width = R.geometry(fs_in, fs_out)
    if (fs_in, fs_out) == (16000, 16001):
        return [300]  # the 813 KB of coefficients: the out-of-LDS table path
    tile = int(_lib.load().ou_resample_tile(fs_in, fs_out))
    assert tile > 0
    # the launcher's own tile: a row whose last output is the last of a tile (or as close as the ratio allows), and the row
    # that just crosses into the next tile
    at_tile = [tile * orig // new, -(-tile * orig // new), -(-(tile + 1) * orig // new)]
    lens = [1, width - 1, orig - 1, orig, orig + 1, 4411, 1601] + at_tile
    return sorted({n for n in lens if n >= 1})


@pytest.mark.parametrize("fs_in,fs_out", R.PAIRS + EXTRA_PAIRS)
def test_accuracy_against_float64_within_6_db_of_the_fp32_conv(fs_in, fs_out):
    lens = _lengths(fs_in, fs_out)
    rows = []
    for i, n in enumerate(lens):
        rows += list(R.noise_rows(2, n, 100 + i))
    y, out_lens, _ = _ragged(rows, fs_in, fs_out)
    failures = []
    for i, n in enumerate(lens):
        x = np.stack(rows[2 * i:2 * i + 2])
        ref = np.stack([R.resample64(x[r], fs_in, fs_out) for r in range(2)])
        J = ref.shape[1]
        assert out_lens[2 * i] == out_lens[2 * i + 1] == J
        conv = A.resample(torch.from_numpy(x), fs_in, fs_out).numpy()
        assert conv.shape == ref.shape
        got = y[2 * i:2 * i + 2, :J].numpy()
        assert not y[2 * i:2 * i + 2, J:].any()
        d_ref, d_lib = R.snr_db(ref, conv), R.snr_db(ref, got)
        print(f"resample {fs_in}->{fs_out} n={n}: fp32 conv {d_ref:.1f} dB, library {d_lib:.1f} dB")
        tag = f"resample.{fs_in}_{fs_out}.n{n}"
        record(tag + ".fp32_conv_vs_f64", min(d_ref, 400.0))
        record(tag + ".library_vs_f64", min(d_lib, 400.0))
        if not d_lib >= d_ref - MARGIN_DB:
            failures.append((n, round(d_ref, 1), round(d_lib, 1)))
    A._kernel_cache.pop((R.geometry(fs_in, fs_out)[0], R.geometry(fs_in, fs_out)[1], "cpu"), None)
    assert not failures, failures


def test_public_backend_equals_the_raw_call_and_keeps_shapes():
    x = torch.from_numpy(R.noise_rows(3, 4411, 5)).cuda()
    for fs, tfs in ((44100, 16000), (16000, 44100)):
        raw, out_lens, _ = _ragged(list(x.cpu().numpy()), fs, tfs)
        y = A.resample(x, fs, tfs, backend="library")
        assert y.shape == (3, out_lens[0]) and y.is_cuda and torch.equal(y.cpu(), raw[:, :out_lens[0]])
        assert torch.equal(A.resample(x[0], fs, tfs, backend="library").cpu(), raw[0, :out_lens[0]])
        assert A.resample(x.reshape(3, 1, -1), fs, tfs, backend="library").shape == (3, 1, out_lens[0])
        many = A.resample_many([x[:2], x[2, :1601], x[1:2, :17]], fs, tfs, backend="library")
        assert [tuple(m.shape) for m in many] == [(2, out_lens[0]), (R.out_length(fs, tfs, 1601),), (1, R.out_length(fs, tfs, 17))]
        assert torch.equal(many[0].cpu(), raw[:2, :out_lens[0]])
        assert torch.equal(many[1], A.resample(x[2, :1601].contiguous(), fs, tfs, backend="library"))
        assert torch.equal(many[2], A.resample(x[1:2, :17].contiguous(), fs, tfs, backend="library"))
    assert A.resample(x, 16000, 16000, backend="library") is x


@pytest.mark.parametrize("fs_in,fs_out", [(44100, 16000), (16000, 44100)])
def test_ragged_batch_equals_row_by_row_bit_for_bit(fs_in, fs_out):
    lens = [1, 17, 440, 441, 442, 4411, 0, 3000]
    rows = [R.noise_rows(1, n, 40 + i)[0] if n else np.zeros(0, np.float32) for i, n in enumerate(lens)]
    table = _table(fs_in, fs_out)
    y, out_lens, cols = _ragged(rows, fs_in, fs_out, pad_value=123.0, y_extra=8, y_fill=777.0, table=table)
    assert (y[:, cols:] == 777.0).all()  # nothing behind `cols` is touched
    for b, n in enumerate(lens):
        assert not y[b, out_lens[b]:cols].any()  # zeroed up to cols; a zero-length row is all zero
        alone, ol, _ = _ragged([rows[b]], fs_in, fs_out, table=table)
        assert ol == [out_lens[b]] and torch.equal(alone[0, :ol[0]], y[b, :ol[0]]), (b, n)
        if n:
            assert y[b, :out_lens[b]].abs().max() > 0
    # nothing is read behind len[b]: NaN there changes no bit
    y_nan, _, _ = _ragged(rows, fs_in, fs_out, pad_value=float("nan"), y_extra=8, y_fill=777.0, table=table)
    assert torch.equal(y_nan, y)


def test_more_rows_than_one_launch_and_equal_rates():
    """65 rows: the launcher's second launch (64 rows per launch); equal rates: a copy with the same zeroing."""
    lens = [(37 * i) % 500 for i in range(65)]
    rows = [R.noise_rows(1, max(n, 1), 200 + i)[0][:n] for i, n in enumerate(lens)]
    y, out_lens, cols = _ragged(rows, 16000, 44100)
    for b in (0, 1, 63, 64):
        alone, ol, _ = _ragged([rows[b]], 16000, 44100)
        assert torch.equal(alone[0, :ol[0]], y[b, :ol[0]]) and not y[b, ol[0]:].any()
    y, out_lens, cols = _ragged(rows, 16000, 16000, pad_value=float("nan"), y_extra=4, y_fill=777.0)
    assert out_lens == lens and (y[:, cols:] == 777.0).all()
    for b, n in enumerate(lens):
        assert torch.equal(y[b, :n], torch.from_numpy(rows[b])) and not y[b, n:cols].any()


def test_repeatable_capturable_and_refusals_touch_nothing():
    fs_in, fs_out = 44100, 16000
    lens = [4411, 1601, 0, 17]
    stride = 4412
    x = torch.from_numpy(R.noise_rows(4, stride, 9)).cuda()
    table = _table(fs_in, fs_out)
    cols = R.out_length(fs_in, fs_out, 4411)
    y1 = torch.full((4, cols), 777.0).cuda()
    y2 = torch.full((4, cols), 555.0).cuda()
    assert _call(x, lens, y1, cols, fs_in, fs_out, table) == _lib.OU_OK
    assert _call(x, lens, y2, cols, fs_in, fs_out, table) == _lib.OU_OK
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)
    # captured on one stream (a serial chain: nothing forks) and replayed = the eager bits
    y3 = torch.full((4, cols), 333.0).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert _call(x, lens, y3, cols, fs_in, fs_out, table) == _lib.OU_OK
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _call(x, lens, y3, cols, fs_in, fs_out, table) == _lib.OU_OK
    y3.fill_(333.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y3, y1)
    # refusals with real device buffers: OU_EINVAL and the output keeps its canary
    canary = torch.full((4, cols), 777.0).cuda()
    bad = [
        lambda: _call(x, lens, canary, cols - 1, fs_in, fs_out, table),               # row 0 does not fit cols
        lambda: _call(x, lens, canary, cols + 1, fs_in, fs_out, table),               # cols does not fit y_stride
        lambda: _call(x, [4413, 1, 1, 1], canary, cols, fs_in, fs_out, table),        # len[b] > x_stride
        lambda: _call(x, lens, canary, cols, fs_in, fs_out, table, nbytes=table.numel() - 4),
        lambda: _call(x, lens, canary, cols, fs_in, fs_out, None),
        lambda: _call(x, lens, canary, cols, 0, fs_out, table),
        lambda: _call(x, lens, canary, cols, fs_in, 16001, table),                    # another pair's table size
    ]
    for k, f in enumerate(bad):
        assert f() == _lib.OU_EINVAL, k
    torch.cuda.synchronize()
    assert (canary == 777.0).all()


def _cli_files(tmp_path, spec):
    src = tmp_path / "in"
    src.mkdir()
    fs = 22050
    shapes = [(1, 8820), (2, 11025), (1, 13230)]  # 0.4, 0.5, 0.6 s; one stereo
    for i, (c, n) in enumerate(shapes):
        sig = torch.cat([synth_mix(spec, 1, n, seed=70 + 2 * i + ch) for ch in range(c)], dim=0)
        A.save(src / f"f{i}.wav", (sig * 0.5).clamp(-1, 1), fs)
    return src, fs, shapes


def test_cli_library_resampler_wiring_and_parity_with_the_default(tmp_path):
    model, spec, _ = get_model("PP16s")
    src, fs, shapes = _cli_files(tmp_path, spec)
    common = ["--seed", "9", "--noise", "counter", "--n_steps", "3"]
    cli.main([str(src), str(tmp_path / "lib"), "--batch-size", "4", "--resampler", "library"] + common, model=model)
    cli.main([str(src), str(tmp_path / "lib_serial"), "--resampler", "library"] + common, model=model)
    cli.main([str(src), str(tmp_path / "torch"), "--batch-size", "4", "--resampler", "torch"] + common, model=model)

    # the manual pipeline of the batched path, same counter sources: resample_many -> enhance_many -> resample_many
    audio = [A.load(src / f"f{i}.wav")[0].cuda() for i in range(len(shapes))]
    with torch.no_grad():
        sigs = A.resample_many(audio, fs, model.fs, backend="library")
        order = sorted(range(len(sigs)), key=lambda i: (-sigs[i].shape[-1], i))  # a window is enhanced longest first
        noise = [cli.file_noise(argparse.Namespace(seed=9), i) for i in range(len(sigs))]
        enh = model.enhance_many([sigs[i] for i in order], [noise[i] for i in order], n_steps=3)
        outs = A.resample_many(list(enh), model.fs, fs, backend="library")
    manual = {i: o.cpu() for i, o in zip(order, outs)}
    serial, default = [], []
    for i, (c, n) in enumerate(shapes):
        got, gfs = A.load(tmp_path / "lib" / f"f{i}.wav")
        assert gfs == fs and got.shape[0] == c and torch.equal(got, manual[i]), i
        ser, _ = A.load(tmp_path / "lib_serial" / f"f{i}.wav")
        tor, _ = A.load(tmp_path / "torch" / f"f{i}.wav")
        assert ser.shape == got.shape == tor.shape
        serial.append(min(float(O.si_sdr(got[ch], ser[ch])) for ch in range(c)))
        default.append(min(float(O.si_sdr(got[ch], tor[ch])) for ch in range(c)))
    # the serial path (resample(backend="library") per file) against the batched one: the ragged gate of test_gpu_ragged.py
    record("resample.cli.PP16s.serial_vs_batched", min(serial), 80)
    # against the default resampler: the project's parity tolerance (60 dB SI-SDR, tests/parity_gates.json)
    record("resample.cli.PP16s.library_vs_torch_resampler", min(default), 60)
    assert min(default) >= gate("resample.cli.PP16s.library_vs_torch_resampler", 60)
