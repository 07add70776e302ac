"""CPU: the BSS-eval SDR (ou_sdr, metrics.sdr) without a device -- the two float64 restatements of tests/sdr_ref.py against each
other on every case of tests/sdr_cases.py, the facts the definition rests on (L = 1 is SI-SDR, scale invariance), that the gated
cases are well conditioned and away from the clamp, every refusal of the ABI (all decided before the first HIP call), the scratch
sizer, and the names `evaluate_many`, the CLI and `Metrics` accept."""
import ctypes
from ctypes import byref, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

import sdr_cases as C
import sdr_ref as R
from open_universe_amd import _lib, metrics as M
from open_universe_amd.bin import eval_metrics as CLI


def test_case_table_is_the_one_asked_for():
    assert len(C.CASES) == 37 and len({c.name for c in C.CASES}) == 37
    for L in C.FILTER_LENGTHS:
        want = {T for T in (1, 5, L - 1, L, L + 1, 700, 4097, 8192) if T >= 1}
        assert {c.T for c in C.CASES if c.L == L} == want
    assert [c.T for c in C.UNGATED] == [1] * 5  # one sample: the projection is the estimate itself
    assert sorted(c.T for c in C.RAGGED) == [5, 63, 65, 700, 4097] and C.COLOURED.pole == 0.9


@pytest.mark.parametrize("case", C.GATED, ids=repr)
def test_restatements_agree_and_the_case_can_be_gated(case):
    """d_ref, the distance of the two float64 routes, is computed here, and is small beside one fp32 ulp of the score: the gate
    of tests/test_gpu_sdr.py (4 d_ref + 1 ulp) is a gate of about one fp32 ulp."""
    print(f"{case}: lstsq {case.lstsq:.12f} normal {case.normal:.12f} d_ref {case.d_ref:.3g} cond {case.cond:.4g} "
          f"ulp32 {R.ulp32(case.lstsq):.3g}")
    assert np.isfinite(case.lstsq) and np.isfinite(case.normal)
    assert case.cond <= C.COND_MAX
    assert C.DB_MIN <= case.lstsq <= C.DB_MAX
    assert case.d_ref <= 1e-6 * max(1.0, abs(case.lstsq))  # float64 routes on cond <= 1e8: far inside this
    assert case.d_ref <= 0.01 * R.ulp32(case.lstsq)


def _can_be_gated(case):
    print(f"{case}: lstsq {case.lstsq:.12f} normal {case.normal:.12f} d_ref {case.d_ref:.3g} cond {case.cond:.4g} "
          f"ulp32 {R.ulp32(case.lstsq):.3g}")
    assert np.isfinite(case.lstsq) and np.isfinite(case.normal)
    assert case.cond <= C.COND_MAX
    assert C.DB_MIN <= case.lstsq <= C.DB_MAX
    assert case.d_ref <= 1e-6 * max(1.0, abs(case.lstsq))
    assert case.d_ref <= 0.01 * R.ulp32(case.lstsq)


@pytest.mark.parametrize("name", C.EDGE_NAMES)
def test_edge_cases_can_be_gated(built_lib, name):
    """The edge table (L = 255, 256, 257, 511 at T = L + 1 and one sample into a second correlation tile; a coloured reference
    at L = 257; 32 tiles at L = 64): every case is well conditioned and away from the clamp, as the table cases are."""
    tile = C.tile_from(M.sdr_scratch_bytes)
    case = C.edge(tile)[name]
    assert case.gated and case.L in C.EDGE_FILTER_LENGTHS + (64,)
    if name.endswith("tile+1"):
        assert case.T == tile + 1 and M.sdr_scratch_bytes(1, case.T, 512) > M.sdr_scratch_bytes(1, case.T - 1, 512)
    _can_be_gated(case)


def test_edge_table_is_the_one_asked_for(built_lib):
    tile = C.tile_from(M.sdr_scratch_bytes)
    E = C.edge(tile)
    assert {(c.L, c.T) for c in E.values()} == {(L, T) for L in (255, 256, 257, 511) for T in (L + 1, tile + 1)} | {
        (257, 4097), (64, 65537)}
    assert E["edge-coloured-L257-T4097"].pole == 0.9 and E["edge-coloured-L257-T4097"].cond > 100.0
    assert -(-65537 // tile) >= 32  # many tiles: the solver's ascending sum is long
    assert not {c.name for c in E.values()} & {c.name for c in C.CASES + [C.COLOURED]}


@pytest.mark.parametrize("many", C.MANY, ids=repr)
def test_rows_of_the_130_row_calls_can_be_gated(many):
    """130 rows: groups of 64, 64 and 2; one sample at the group borders; the one longest row first or last; every other row
    has a restatement the gate can be held against."""
    assert len(many.cases) == 130 and [many.cases[b].T for b in (63, 64, 127, 128)] == [1] * 4
    lens = [c.T for c in many.cases]
    assert lens.index(max(lens)) == many.longest_at and lens.count(max(lens)) == 1 and max(lens) == 4097
    assert {c.L for c in many.cases} == {many.L}
    distinct = {c.name: c for c in many.cases}
    assert len(distinct) <= 8  # the references are computed once per distinct pair
    for c in distinct.values():
        if c.gated:
            _can_be_gated(c)
    assert {(m.L, m.longest_at) for m in C.MANY} == {(64, 129), (64, 0), (257, 129), (257, 0)}


def test_target_ratios_are_covered():
    got = [c.lstsq for c in C.GATED]
    assert min(got) < -15.0 and max(got) > 33.0  # about -20 .. +35 dB
    assert C.COLOURED.cond > 100.0  # coloured: R is not near a multiple of the identity


@pytest.mark.parametrize("T", [2, 5, 700, 4097])
def test_filter_length_one_is_si_sdr(T):
    est, ref = C.by_name(f"L1-T{T}").pair
    assert R.sdr_normal(est, ref, 1) == pytest.approx(R.si_sdr(est, ref), abs=1e-12)
    assert R.sdr_lstsq(est, ref, 1) == pytest.approx(R.si_sdr(est, ref), abs=1e-12)


def test_scale_invariance():
    est, ref = C.by_name("L17-T700").pair
    base = R.sdr_normal(est, ref, 17)
    for a, b in ((8.0, 1.0), (1.0, 0.125), (-3.0, 1e3), (1e-3, -7.0)):
        e, r = est.astype(np.float64) * a, ref.astype(np.float64) * b
        assert R.sdr_normal(e, r, 17) == pytest.approx(base, abs=1e-10)
        assert R.sdr_lstsq(e, r, 17) == pytest.approx(base, abs=1e-10)


def test_more_taps_never_lower_the_score():
    est, ref = C.by_name("L64-T700").pair
    scores = [R.sdr_lstsq(est, ref, L) for L in (1, 2, 17, 64)]
    assert all(b >= a - 1e-10 for a, b in zip(scores, scores[1:]))  # the spans are nested


# ---- the raw ABI: host buffers stand in for device memory -- a refusal touches none of them ----
def test_symbols_are_bound(built_lib):
    for name in ("ou_sdr_scratch_bytes", "ou_sdr"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(built_lib, name)


def _call(L, B=2, T=1000, filter_length=512, clamp=100.0, scratch_bytes=1 << 40, lens=None):
    x = np.zeros((B, T), np.float32)
    out = np.full(B, 7.0, np.float32)
    scratch = np.zeros(64, np.uint8)
    lens = (c_int64 * B)(*([T] * B if lens is None else lens))
    p = lambda a: c_void_p(a.ctypes.data)
    rc = L.ou_sdr(p(x), p(x), T, lens, B, filter_length, clamp, p(out), p(scratch), c_size_t(scratch_bytes), None)
    assert (out == 7.0).all() and not scratch.any()
    return rc


def _refused(L, code, want, *words):
    assert code == want, (code, L.ou_last_error(None))
    msg = L.ou_last_error(None).decode()
    for w in words:
        assert w in msg, msg


def test_abi_refusals_launch_nothing(built_lib):
    L = built_lib
    _refused(L, _call(L, filter_length=0), _lib.OU_EINVAL, "filter_length = 0", "OU_SDR_MAX_FILTER = 512")
    _refused(L, _call(L, filter_length=513), _lib.OU_EINVAL, "filter_length = 513")
    _refused(L, _call(L, clamp=0.0), _lib.OU_EINVAL, "clamp_db")
    _refused(L, _call(L, clamp=-1.0), _lib.OU_EINVAL, "clamp_db")
    _refused(L, _call(L, clamp=float("inf")), _lib.OU_EINVAL, "clamp_db")
    _refused(L, _call(L, clamp=float("nan")), _lib.OU_EINVAL, "clamp_db")
    _refused(L, _call(L, lens=[1000, 0]), _lib.OU_EINVAL, "len[1]")
    _refused(L, _call(L, lens=[1001, 5]), _lib.OU_EINVAL, "len[0]")  # behind the stride
    _refused(L, _call(L, scratch_bytes=64), _lib.OU_ESHAPE, "ou_sdr_scratch_bytes asks for")
    _refused(L, _call(L, scratch_bytes=M.sdr_scratch_bytes(2, 1000, 512) - 1), _lib.OU_ESHAPE, "scratch")
    n = c_size_t()
    _refused(L, L.ou_sdr_scratch_bytes(2, 1000, 0, byref(n)), _lib.OU_EINVAL, "filter_length = 0")
    _refused(L, L.ou_sdr_scratch_bytes(2, 1000, 513, byref(n)), _lib.OU_EINVAL, "filter_length = 513")
    _refused(L, L.ou_sdr_scratch_bytes(0, 1000, 512, byref(n)), _lib.OU_EINVAL, "B >= 1")
    _refused(L, L.ou_sdr_scratch_bytes(2, 0, 512, byref(n)), _lib.OU_EINVAL, "T_max")


def test_scratch_sizer_is_monotone(built_lib):
    f = M.sdr_scratch_bytes
    for B, T, L in ((1, 1, 1), (3, 700, 17), (16, 64000, 512)):
        assert 0 < f(B, T, L) <= f(B + 1, T, L) and f(B, T, L) <= f(B, T + 1, L) <= f(B, 4 * T + 10000, L)
        if L < 512:
            assert f(B, T, L) <= f(B, T, L + 1)
    assert f(1, 1, 1) < f(64, 1, 1) and f(1, 1000, 512) < f(1, 100000, 512) and f(4, 64000, 1) < f(4, 64000, 512)
    # the partials: (rows, tiles, 2, L) doubles, whatever else there is
    assert f(16, 64000, 512) >= 16 * (64000 // 4096) * 2 * 512 * 8
    with pytest.raises(ValueError, match="filter_length = 513"):
        f(1, 1000, 513)


def test_names(built_lib):
    assert M.OPTIONAL_METRICS == ("sdr",) and "sdr" not in M.AVAILABLE_METRICS
    assert M.check_score_names(None) == list(M.AVAILABLE_METRICS)  # never a default
    assert M.check_score_names(["si-sdr", "sdr"]) == ["si-sdr", "sdr"]
    with pytest.raises(NotImplementedError, match="Metric stoi is not supported: it needs a model or a package"):
        M.check_score_names(["sdr", "stoi"])
    with pytest.raises(NotImplementedError, match="Metric sdr is not supported") as e:
        M.Metrics(metrics=["sdr"])
    assert "package" not in str(e.value) and "evaluate_many" in str(e.value)
    with pytest.raises(NotImplementedError, match="Metric sdr is not supported"):
        M.check_metric_names(["lsd", "sdr"])


def test_python_refusals_and_no_cpu_path(built_lib):
    x = torch.zeros(2, 1000)
    with pytest.raises(ValueError, match="filter_length = 0"):
        M.sdr(x, x, filter_length=0)
    with pytest.raises(ValueError, match="filter_length = 513"):
        M.sdr(x, x, filter_length=513)
    with pytest.raises(ValueError, match="integer"):
        M.sdr(x, x, filter_length=2.5)
    with pytest.raises(ValueError, match="clamp_db"):
        M.sdr(x, x, clamp_db=0.0)
    with pytest.raises(ValueError, match="shapes"):
        M.sdr(x, x[:, :900])
    # with everything in order, a tensor that is not on a HIP device is refused: no CPU path, no fallback
    with pytest.raises(ValueError, match="HIP device"):
        M.sdr(x, x)
    # evaluate_many accepts the name: it gets as far as the device check, where `stoi` is refused by name
    with pytest.raises(ValueError, match="HIP device"):
        M.evaluate_many([x[0]], [x[1]], 16000, metrics=["sdr"])
    with pytest.raises(NotImplementedError, match="stoi"):
        M.evaluate_many([x[0]], [x[1]], 16000, metrics=["sdr", "stoi"])


def test_cli_accepts_the_name(tmp_path):
    from open_universe_amd import audio

    for d in ("clean", "enh"):
        (tmp_path / d).mkdir()
        audio.save(tmp_path / d / "a.wav", torch.linspace(-0.5, 0.5, 500)[None], 16000)
    # the parser and the name check pass; scoring then asks for the device the files are to be moved to
    with pytest.raises((RuntimeError, AssertionError, ValueError)) as e:
        CLI.main([str(tmp_path / "clean"), str(tmp_path / "enh"), "--metrics", "si-sdr", "sdr", "--device", "cpu",
                  "--result-dir", str(tmp_path / "out")])
    assert "HIP device" in str(e.value)
    assert "sdr" in CLI.__doc__
