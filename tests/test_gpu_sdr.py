"""GPU (-m gpu): the BSS-eval SDR of open_universe_amd.metrics.sdr (ou_sdr; csrc/ou_sdr.hip) against the float64 restatements of
tests/sdr_ref.py on the cases of tests/sdr_cases.py.

The gate of every gated case:  |library - sdr_lstsq| <= 4 d_ref + 1 fp32 ulp of the score,  d_ref = |sdr_lstsq - sdr_normal| of
that case.  The ulp is there because `out` is fp32; the factor 4 because the kernels do sdr_normal's arithmetic in the same
precision in another summation order and with another solver.  d_ref is 1e-15 .. 1e-11 dB on these cases (test_sdr_cpu.py
prints it), so this is a gate of one fp32 ulp.  Every case prints distance / bound and distance / d_ref before it asserts.

fast_bss_eval, the package the reference takes this number from, is not available to this project: nothing here compares
against a recording of it.

Shapes: every (L, T) of the case table -- T below, at and above L, one sample, rows of two to four correlation tiles, both
accumulator plans (L <= 256: one tile of 256 lags, L = 512: two) --, T around the correlation tile (found from the scratch
sizer), a ragged batch of five rows, and the clamp.  The edges (sdr_cases.edge): L = 255, 256, 257 and 511 -- either side of
the switch between the accumulator plans, and one below the cap -- at T = L + 1 and T = tile + 1, a coloured reference at
L = 257, T = 4097, and L = 64 at T = 65537 (32 correlation tiles).  Ragged calls of 130 rows (sdr_cases.MANY: launch groups
of 64, 64 and 2) at L = 64 and 257, one sample at rows 63, 64, 127 and 128, the one row of two tiles last or first.

Measured on an MI355X (DESIGN 4.21 has the table): distance / bound 0.007 .. 0.50 over the 33 gated cases and the 8 tile
cases -- the rounding of `out` to fp32 -- and every row of the ragged batch equal to the row scored alone; 0.02 .. 0.49 over
the 10 edge cases, 0.04 .. 0.45 over the rows of the 130-row calls, each of their rows equal to the row scored alone."""
import functools
import json

import numpy as np
import pytest
import torch

import sdr_cases as C
import sdr_ref as R
from open_universe_amd import audio, metrics as M
from open_universe_amd.bin import eval_metrics as CLI

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _score(case, **kw):
    est, ref = case.pair
    return float(M.sdr(_dev(est), _dev(ref), filter_length=case.L, **kw))


def _check(case, lib):
    dist, bound = abs(lib - case.lstsq), case.bound()
    print(f"{case}: lib {lib:.9g} lstsq {case.lstsq:.12g} dist {dist:.3g} bound {bound:.3g} dist/bound {dist / bound:.3f} "
          f"d_ref {case.d_ref:.3g} dist/d_ref {dist / case.d_ref if case.d_ref else float('inf'):.3g}")
    assert dist <= bound, (case, lib, case.lstsq, dist, bound)


@pytest.mark.parametrize("case", C.GATED, ids=repr)
def test_accuracy_gate(case):
    _check(case, _score(case))


@pytest.mark.parametrize("case", C.UNGATED, ids=repr)
def test_one_sample_scores_the_clamp(case):
    """T = 1: the estimate is a multiple of the reference whatever L is -- the ratio is infinite and the clamp answers."""
    assert _score(case) == pytest.approx(100.0, abs=R.ulp32(100.0))
    assert _score(case, clamp_db=20.0) == pytest.approx(20.0, abs=R.ulp32(20.0))


@pytest.mark.parametrize("T", [2, 5, 700, 4097, 8192])
def test_filter_length_one_is_si_sdr(T):
    est, ref = C.by_name(f"L1-T{T}").pair
    a, b = float(M.sdr(_dev(est), _dev(ref), filter_length=1)), float(M.si_sdr(_dev(est), _dev(ref)))
    print(f"T {T}: sdr(L=1) {a:.9g} si_sdr {b:.9g}")
    assert abs(a - b) <= R.ulp32(b)


@pytest.fixture(scope="module")
def ragged():
    """Five rows of lengths of their own in one (B, stride) buffer each, NaN behind every row."""
    lens = [c.T for c in C.RAGGED]
    stride = max(lens) + 4
    x = torch.full((len(lens), stride), float("nan"), device=DEV)
    y = torch.full((len(lens), stride), float("nan"), device=DEV)
    for b, c in enumerate(C.RAGGED):
        x[b, :c.T], y[b, :c.T] = _dev(c.pair[0]), _dev(c.pair[1])
    return x, y, lens


def test_rows_in_a_batch(ragged):
    """Each row of the ragged batch is bit for bit its own B = 1 call, two runs are bit-identical, the NaN behind the rows
    (and zeros in their place) change nothing, and every row holds the gate."""
    x, y, lens = ragged
    a = M._bss_sdr_rows(x, y, lens, C.RAGGED_L, 100.0)
    b = M._bss_sdr_rows(x, y, lens, C.RAGGED_L, 100.0)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    x0, y0 = torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)
    assert torch.equal(a, M._bss_sdr_rows(x0, y0, lens, C.RAGGED_L, 100.0))
    for i, c in enumerate(C.RAGGED):
        alone = M.sdr(x[i, :c.T], y[i, :c.T], filter_length=C.RAGGED_L)
        assert torch.equal(alone, a[i]), (c, float(alone), float(a[i]))
        _check(c, float(a[i]))


def _tile():
    """Samples per workgroup of the correlation kernel: the first length at which a row needs a second tile of partials."""
    lo, hi, base = 1, 1 << 20, M.sdr_scratch_bytes(1, 1, 512)
    assert M.sdr_scratch_bytes(1, hi, 512) > base
    while lo < hi:  # the last T that still costs `base`
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if M.sdr_scratch_bytes(1, mid, 512) == base else (lo, mid - 1)
    return lo


@pytest.mark.parametrize("L", [64, 512])
def test_tile_boundaries(L):
    tile = _tile()
    assert 512 <= tile <= 8192, tile  # (sdr_lstsq stays small)
    for T in (tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1):
        if L == 512 and T > tile + 1:
            continue
        case = C.Case(f"tile-L{L}-T{T}", L, T, 10.0, 500 + T % 7)
        assert case.cond <= C.COND_MAX and C.DB_MIN <= case.lstsq <= C.DB_MAX
        _check(case, _score(case))


@pytest.mark.parametrize("name", C.EDGE_NAMES)
def test_edge_accuracy_gate(name):
    """The accumulator-tile switch of sdr_corr_kernel -- L = 255 and 256 on one tile of 256 lags, 257 and 511 on two, where the
    `lag < L` guard of the write-out drops 255 and 1 lags of the second tile -- at T = L + 1 and one sample into a second
    correlation tile; a coloured reference on the two-tile path; and an SDR row of many tiles (32 at T = 65537), where the
    solver's ascending sum over tiles is long.  The gate of every other case."""
    case = C.edge(_tile())[name]
    _check(case, _score(case))


@functools.lru_cache(maxsize=None)
def _many_rows(k):
    """The 130 rows of C.MANY[k] in one (130, stride) buffer each, NaN behind every row; every distinct pair uploaded once."""
    many = C.MANY[k]
    lens = [c.T for c in many.cases]
    x = torch.full((len(lens), max(lens) + 4), float("nan"), device=DEV)
    y = torch.full_like(x, float("nan"))
    dev = {c.name: (_dev(c.pair[0]), _dev(c.pair[1])) for c in many.cases}
    for b, c in enumerate(many.cases):
        x[b, :c.T], y[b, :c.T] = dev[c.name]
    return x, y, lens


@pytest.mark.parametrize("k", range(len(C.MANY)), ids=[repr(m) for m in C.MANY])
def test_130_rows_in_one_call(k):
    """Rows 64 and up: 130 ragged rows are launch groups of 64, 64 and 2, so the second and third run with row0 = 64 and 128
    (signals, tsum, partial and out at row0 + block, the by-value lengths at the block), one sample at rows 63, 64, 127, 128.
    Per-group grid against per-call strides: with the longest row last, groups 0 and 1 run grids of one tile inside a tile
    stride of two; with it first, groups 1 and 2 do.  At L = 64 and at L = 257 (one and two accumulator tiles).  Two runs are
    bit-identical, zeros for the NaN behind the rows change nothing, EVERY row is bit for bit its own B = 1 call, and every
    row holds the gate or, at one sample, scores the clamp."""
    many = C.MANY[k]
    x, y, lens = _many_rows(k)
    assert _tile() < max(lens) and sorted(lens)[-2] <= _tile()  # the longest row alone reaches a second tile
    a = M._bss_sdr_rows(x, y, lens, many.L, 100.0)
    assert a.shape == (130,) and bool(torch.isfinite(a).all())
    assert torch.equal(a, M._bss_sdr_rows(x, y, lens, many.L, 100.0))
    assert torch.equal(a, M._bss_sdr_rows(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0), lens, many.L, 100.0))
    alone = torch.stack([M.sdr(x[i, :n], y[i, :n], filter_length=many.L) for i, n in enumerate(lens)])
    a, alone = a.cpu(), alone.cpu()
    differ = [(i, lens[i], float(a[i]), float(alone[i])) for i in range(len(lens)) if a[i] != alone[i]]
    assert not differ, (many, differ[:8])
    seen = set()
    for i, c in enumerate(many.cases):
        lib = float(a[i])
        if not c.gated:
            assert lib == pytest.approx(100.0, abs=R.ulp32(100.0)), (many, i, lib)
        elif c.name in seen:
            assert abs(lib - c.lstsq) <= c.bound(), (many, i, c, lib, c.lstsq)
        else:
            _check(c, lib)
            seen.add(c.name)


def test_clamp_and_degenerate_inputs():
    c = C.by_name("L17-T4097")  # about 35 dB
    est, ref = (_dev(a) for a in c.pair)
    zero = torch.zeros_like(ref)
    u100, u30 = R.ulp32(100.0), R.ulp32(30.0)
    assert float(M.sdr(ref, ref, filter_length=17)) == pytest.approx(100.0, abs=u100)
    assert float(M.sdr(ref, ref, filter_length=512)) == pytest.approx(100.0, abs=u100)
    assert float(M.sdr(zero, ref, filter_length=17)) == pytest.approx(-100.0, abs=u100)
    assert float(M.sdr(est, zero, filter_length=17)) == pytest.approx(-100.0, abs=u100)
    assert float(M.sdr(zero, zero, filter_length=17)) == pytest.approx(-100.0, abs=u100)
    assert c.lstsq > 34.0
    assert float(M.sdr(est, ref, filter_length=17, clamp_db=30.0)) == pytest.approx(30.0, abs=u30)
    assert float(M.sdr(-est, ref, filter_length=17, clamp_db=30.0)) == pytest.approx(30.0, abs=u30)
    assert abs(float(M.sdr(est, ref, filter_length=17, clamp_db=40.0)) - c.lstsq) <= c.bound()
    assert float(M.sdr(zero, ref, filter_length=17, clamp_db=30.0)) == pytest.approx(-30.0, abs=u30)


def test_scale_and_shape():
    c = C.by_name("L64-T700")
    est, ref = (_dev(a) for a in c.pair)
    base = float(M.sdr(est, ref, filter_length=64))
    for a, b in ((8.0, 1.0), (1.0, 0.125), (-4.0, 1024.0)):  # powers of two: every product scales exactly
        assert float(M.sdr(est * a, ref * b, filter_length=64)) == base
    both = M.sdr(torch.stack([est, ref])[None], torch.stack([ref, ref])[None], filter_length=64)
    assert both.shape == (1, 2) and float(both[0, 0]) == base and float(both[0, 1]) == pytest.approx(100.0, abs=1e-5)


def test_default_filter_and_evaluate_many():
    cases = [C.by_name(n) for n in ("L512-T700", "L512-T4097", "L512-T513")]
    est, ref = [_dev(c.pair[0]) for c in cases], [_dev(c.pair[1]) for c in cases]
    rows = M.evaluate_many(est, ref, 16000, metrics=["si-sdr", "sdr"])
    for c, row, e, r in zip(cases, rows, est, ref):
        assert list(row) == ["si-sdr", "sdr"]
        assert row["sdr"] == float(M.sdr(e, r)) and row["si-sdr"] == float(M.si_sdr(e, r))  # 512 taps by default
        _check(c, row["sdr"])
    assert list(M.evaluate_many(est, ref, 16000)[0]) == list(M.AVAILABLE_METRICS)  # not a default


def test_cli_writes_the_column(tmp_path):
    """eval_metrics --metrics si-sdr sdr --batch-size 4 on four small wav pairs: the sdr column is metrics.sdr per file."""
    g = torch.Generator().manual_seed(3)
    (tmp_path / "clean").mkdir()
    (tmp_path / "enh").mkdir()
    for i, n in enumerate((1200, 900, 1500, 700)):
        ref = 0.2 * torch.randn(n, generator=g)
        deg = 0.8 * ref + 0.02 * torch.randn(n, generator=g)
        audio.save(tmp_path / "clean" / f"f{i}.wav", ref[None], 16000)
        audio.save(tmp_path / "enh" / f"f{i}.wav", deg[None], 16000)
    assert CLI.main([str(tmp_path / "clean"), str(tmp_path / "enh"), "--metrics", "si-sdr", "sdr", "--batch-size", "4",
                     "--result-dir", str(tmp_path / "out")]) == 0
    res = json.load(open(tmp_path / "out" / "enh.json"))
    summary = json.load(open(tmp_path / "out" / "enh_summary.json"))
    assert sorted(res) == ["f0", "f1", "f2", "f3"] and summary["number"] == 4
    for i in range(4):
        deg, _ = audio.load(tmp_path / "enh" / f"f{i}.wav")
        ref, _ = audio.load(tmp_path / "clean" / f"f{i}.wav")
        assert list(res[f"f{i}"]) == ["si-sdr", "sdr"]
        assert res[f"f{i}"]["sdr"] == float(M.sdr(deg[0].to(DEV), ref[0].to(DEV)))
        assert res[f"f{i}"]["sdr"] >= res[f"f{i}"]["si-sdr"] - 1e-4  # 512 taps span the one of SI-SDR
    assert summary["sdr"] == pytest.approx(sum(res[f"f{i}"]["sdr"] for i in range(4)) / 4, abs=1e-9) and "sdr_std" in summary
