"""GPU (-m gpu): ou_resample held sample by sample (resample_fp64.py): noise rows against the float64 evaluation of the dense kernel
at the chain bound (taps + 2) u A + 1/2 ulp, impulse rows against amplitude x the table's fp32 coefficient bit for bit, nothing
excluded, exactly 0 behind every row's own output length.  The ten pairs of test_gpu_resample.py's accuracy test reach every
kernel path; the row lengths sit around the launcher's tile and past two tiles; the impulse rows meet every phase and tap of
every table and both sides of the seam between tile 0 and tile 1 (test_resample_fp64_cpu.py asserts that, and that a dropped
seam tap is flagged).  The unaligned test takes the scalar staging loads (x off a 16-byte boundary, or x_stride % 4 != 0), which
have to give the bits of the 16-byte loads.

Every case logs the worst err / bound with its row and sample, the counts and the seconds to
build/observed/resample_fp64_observed.json (untracked) before it asserts; profiles/resample_fp64_observed.json is a committed
copy.

Measured on an MI355X (profiles/resample_fp64_observed.json), worst err / bound over the noise rows per kernel path:
resample_kernel<true> at 256 threads 0.275 (22 050 -> 24 000; the other six pairs 0.076 .. 0.272), at 128 threads 0.020
(192 000 -> 8 000, 291 taps), resample_kernel<false> 0.246 (16 000 -> 16 001), resample_direct_kernel 0.007 (1 MHz -> 16 kHz,
758 taps) -- the figures of the numpy restatement of test_resample_fp64_cpu.py to the last digit.  The impulse rows: every
sample of every pair equal (1 280 265 samples, 238 794 of them nonzero, at 16 000 -> 16 001).  The three layouts of the
unaligned test: equal bit for bit, with and without NaN around the rows."""
import json
import os
import time

import numpy as np
import pytest
import torch

import resample_fp64 as F
import resample_reference as R
from open_universe_amd import _lib
from test_gpu_resample import EXTRA_PAIRS, _call, _table

pytestmark = pytest.mark.gpu

_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed")
PAIRS = R.PAIRS + EXTRA_PAIRS
CANARY = 777.0


def _log(case, figures):
    try:
        os.makedirs(_OUT, exist_ok=True)
        path = os.path.join(_OUT, "resample_fp64_observed.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[case] = figures
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError as e:  # (the figures follow on stdout)
        print(f"resample_fp64_observed.json not written: {e}")


def _run(case, fs_in, fs_out, offset=0, stride_extra=0, pad_value=0.0):
    """One ragged call over the rows of `case`.  x starts `offset` floats into its allocation and its row stride is a multiple
    of 4 plus `stride_extra`; `pad_value` fills everything that is not a row's sample; y has 8 columns of canary behind `cols`.
    -> y (rows, cols + 8) on the CPU."""
    rows, lens, cols = case["rows"], case["lens"], case["cols"]
    stride = (max(lens) + 3) // 4 * 4 + 4 + stride_extra
    flat = torch.full((offset + len(rows) * stride + 4,), pad_value, dtype=torch.float32)
    x = flat[offset:offset + len(rows) * stride].view(len(rows), stride)
    for b, r in enumerate(rows):
        x[b, :len(r)] = torch.from_numpy(r)
    flat_d = flat.cuda()
    assert flat_d.data_ptr() % 16 == 0
    xd = flat_d[offset:offset + len(rows) * stride].view(len(rows), stride)
    y = torch.full((len(rows), cols + 8), CANARY, dtype=torch.float32).cuda()
    assert _call(xd, lens, y, cols, fs_in, fs_out, _table(fs_in, fs_out)) == _lib.OU_OK, _lib.load().ou_last_error(None)
    torch.cuda.synchronize()
    y = y.cpu()
    assert (y[:, cols:] == CANARY).all()  # nothing behind `cols` is touched
    return y


@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_noise_rows_within_the_chain_bound_sample_by_sample(fs_in, fs_out):
    t0 = time.time()
    P, case = F.pair(fs_in, fs_out), F.noise_case(fs_in, fs_out)
    assert case["out_lens"] == [int(_lib.load().ou_resample_length(fs_in, fs_out, n)) for n in case["lens"]]
    y = _run(case, fs_in, fs_out)
    rep = F.check_noise(f"noise.{fs_in}_{fs_out}", case, y[:, :case["cols"]])
    print(rep)
    _log(rep.name, dict(F.figures(rep, time.time() - t0), path=P.path, taps=P.taps, tile=P.tile, lens=sorted(set(case["lens"]))))
    assert rep.excluded == 0 and rep.checked == len(case["rows"]) * case["cols"]
    assert rep.ok(), str(rep)


@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_impulse_rows_give_the_table_bit_for_bit(fs_in, fs_out):
    t0 = time.time()
    P, case = F.pair(fs_in, fs_out), F.impulse_case(fs_in, fs_out)
    assert case["hits"].all()  # every phase meets every tap
    y = _run(case, fs_in, fs_out)
    rep = F.check_impulses(f"impulse.{fs_in}_{fs_out}", case, y[:, :case["cols"]])
    print(rep)
    _log(rep.name, dict(F.figures(rep, time.time() - t0), path=P.path, spacing=case["spacing"], seams=case["seams"],
                        nonzero=int((case["want"] != 0).sum())))
    assert rep.excluded == 0 and rep.checked == len(case["rows"]) * case["cols"]
    assert rep.ok(), str(rep)
    assert np.array_equal(y[:, :case["cols"]].double().numpy(), case["want"].numpy())  # ==: -0.0 equals 0.0


@pytest.mark.parametrize("fs_in,fs_out", [(44100, 16000), (16000, 44100), (192000, 8000)])
def test_unaligned_rows_take_the_scalar_loads_and_give_the_same_bits(fs_in, fs_out):
    """The same ragged call three ways: as everywhere else (16-byte loads), x 4 bytes into its allocation with an odd row stride,
    and an aligned x with x_stride % 4 == 2 (both: scalar staging loads).  A row's result depends on neither tiling nor batch
    (the kernel's header), so the outputs are equal bit for bit; NaN in every word that is not a row's sample changes none."""
    P, case = F.pair(fs_in, fs_out), F.noise_case(fs_in, fs_out)
    layouts = {"aligned": (0, 0), "base_plus_4_bytes_odd_stride": (1, 1), "aligned_base_stride_mod_4_is_2": (0, 2)}
    base = _run(case, fs_in, fs_out)
    figs, reports = {}, []
    for name, (offset, extra) in layouts.items():
        t0 = time.time()
        y = _run(case, fs_in, fs_out, offset, extra)
        y_nan = _run(case, fs_in, fs_out, offset, extra, pad_value=float("nan"))
        rep = F.check_noise(f"unaligned.{fs_in}_{fs_out}.{name}", case, y_nan[:, :case["cols"]])
        print(rep)
        same, same_nan = torch.equal(y, base), torch.equal(y_nan, base)
        figs[name] = dict(F.figures(rep, time.time() - t0), equals_aligned=same, nan_padding_changes_nothing=same_nan)
        reports.append((name, rep, same, same_nan))
    _log(f"unaligned.{fs_in}_{fs_out}", dict(figs, path=P.path))
    for name, rep, same, same_nan in reports:
        assert same and same_nan, name
        assert rep.excluded == 0 and rep.ok(), str(rep)
