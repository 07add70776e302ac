"""CPU: STOI and extended STOI (ou_stoi, metrics.stoi) without a device -- the two float64 restatements of tests/stoi_ref.py
against each other on every case of tests/stoi_cases.py, the constants the definition rests on (filter lengths, band table),
the cut at 30 frames, identity and gain invariance, that the cases can be gated, every refusal of the ABI (all decided before the
first HIP call), the scratch sizer, and the names `evaluate_many`, the CLI and `Metrics` accept."""
import ctypes
import re
from ctypes import byref, c_int64, c_size_t, c_void_p
from pathlib import Path

import numpy as np
import pytest
import torch

import stoi_cases as C
import stoi_ref as R
from open_universe_amd import _lib, metrics as M
from open_universe_amd.bin import eval_metrics as CLI

TILE = 16
TABLE = C.table(TILE)
ROOT = Path(__file__).resolve().parent.parent


def test_tile_of_the_case_table(built_lib):
    assert int(built_lib.ou_stoi_frame_tile()) == TILE


@pytest.mark.parametrize("case", TABLE, ids=repr)
def test_restatements_agree(case):
    """d_ref, the distance of the two float64 routes, is computed here, and is small beside one fp32 ulp of the score: the gate
    of tests/test_gpu_stoi.py (4 d_ref + 1 ulp) is a gate of about one fp32 ulp."""
    for ext in (False, True):
        v, d = case.vec(ext), case.direct(ext)
        print(f"{case} {'estoi' if ext else 'stoi'}: vec {v.score:.15f} direct {d.score:.15f} d_ref {case.d_ref(ext):.3g} "
              f"frames {v.frames} margin {v.margin:.4g} / {d.margin:.4g} dB ulp32 {R.ulp32(v.score):.3g}")
        assert np.isfinite(v.score) and np.isfinite(d.score)
        assert v.frames == d.frames
        assert case.d_ref(ext) <= 1e-12
        if v.frames and np.isfinite(v.margin):
            assert abs(v.margin - d.margin) <= 1e-9
        if case.short:
            assert v.score == d.score == R.SHORT and v.frames < R.SEGMENT
        else:
            assert case.d_ref(ext) <= 0.01 * max(R.ulp32(v.score), 1e-9)


def _many_only():
    """The cases the 130-row calls add to the tables (the 16 kHz rows), once each."""
    known = {c.name for c in TABLE + C.EDGE}
    return list({c.name: c for m in C.MANY for c in m.cases if c.name not in known}.values())


@pytest.mark.parametrize("case", C.EDGE + _many_only(), ids=repr)
def test_edge_restatements_agree_and_the_case_can_be_gated(case):
    """The edge table and the rows of the 130-row calls, as test_restatements_agree holds the case table; and every case not
    built short is gated -- margin, at least 30 frames, both restatements on one frame count."""
    test_restatements_agree(case)
    assert case.gated == (not case.short), (case, case.margin, case.frames, case.direct().frames)
    if not case.short:
        assert case.margin >= C.MARGIN_MIN_DB and case.frames >= R.SEGMENT and case.direct().frames == case.frames


def test_edge_table_is_the_one_asked_for():
    E = {c.name: c for c in C.EDGE}
    assert len(E) == len(C.EDGE) and not set(E) & {c.name for c in TABLE}
    energy = lambda c: len(R.frame_starts(-(-c.T * R.ratio(c.fs)[0] // R.ratio(c.fs)[1])))  # frames before the silent ones go
    # the kept-frame scan walks chunks of 1024 energy frames: one short of a chunk, a chunk, one more, two chunks, one more
    assert [energy(E[f"mask-{e}"]) for e in (1023, 1024, 1025, 2048, 2049)] == [1023, 1024, 1025, 2048, 2049]
    assert [E[f"mask-{e}"].frames for e in (1023, 1024, 1025, 2048, 2049)] == [1022, 1023, 1024, 2047, 2048]  # none silent
    s = E["mask-silent-2100"]
    assert energy(s) == 2101 and s.T == C.length_for(2100) and s.frames < 2100 - 50
    for border in (C.MASK_CHUNK, 2 * C.MASK_CHUNK):  # silent hops on both sides of each chunk border
        assert {border - 2, border - 1, border, border + 1} <= set(s.silent_hops)
    # the segment tile: 45 frames are 16 segments, 46 are 17
    assert (E["segtile-45"].frames, E["segtile-46"].frames) == (C.SEG_TILE_FRAMES, C.SEG_TILE_FRAMES + 1) == (45, 46)
    assert not E["segtile-45"].silent_hops and not E["segtile-46"].silent_hops
    assert [R.ratio(E[f"fs-{fs}"].fs) for fs in (48000, 22050, 6000, 12000)] == [(5, 24), (200, 441), (5, 3), (5, 6)]
    assert all(E[f"fs-{fs}"].silent_hops and 60 <= E[f"fs-{fs}"].frames <= 75 for fs in (48000, 22050, 6000, 12000))
    lg = E["long-48000"]
    assert lg.fs == 48000 and lg.T == 14 * 48000 and energy(lg) > C.MASK_CHUNK + 30 and lg.frames > 1024
    assert {C.MASK_CHUNK - 1, C.MASK_CHUNK, C.MASK_CHUNK + 1} <= set(lg.silent_hops)


def test_the_130_row_calls_are_the_ones_asked_for():
    assert [(m.fs, m.longest_at) for m in C.MANY] == [(R.FS, 129), (R.FS, 0), (16000, 129), (16000, 0)]
    for m in C.MANY:
        lens = [c.T for c in m.cases]
        assert len(lens) == 130 and lens.index(max(lens)) == m.longest_at and lens.count(max(lens)) == 1
        assert {c.fs for c in m.cases} == {m.fs} and len({c.name for c in m.cases}) <= 12
        border = [m.cases[b] for b in (63, 64, 127, 128)]
        assert all(c.short for c in border) and 1 in {c.T for c in border} and {c.T for c in border} - {1}
        assert sum(not c.short for c in m.cases) > 80 and sum(c.short for c in m.cases) > 4
    assert max(c.T for c in C.MANY[0].cases) == C.length_for(60)


def test_the_cases_that_cannot_be_gated_are_the_ones_built_short():
    """`gated` is a condition on the inputs: a threshold margin of at least 1e-6 dB and at least 30 frames.  Every case that
    fails it was built to have fewer than 30 frames; no case fails it on the margin (they clear it by decibels)."""
    assert {c.name for c in TABLE if not c.gated} == {c.name for c in TABLE if c.short}
    assert all(c.margin >= 5.0 for c in TABLE)
    assert len({c.name for c in TABLE}) == len(TABLE)


def test_case_table_is_the_one_asked_for():
    frames = {c.name: c.frames for c in TABLE}
    assert [frames[f"frames-{j}"] for j in (28, 29, 30, 31)] == [28, 29, 30, 31]
    # one sample either side of a frame start: 256 + 128 k has k - 1 frames, 256 + 128 k + 1 has k
    assert (frames["start-k30"], frames["start-k30+1"], frames["start-k31"], frames["start-k31+1"]) == (29, 30, 30, 31)
    assert C.by_name("start-k30").T == 256 + 128 * 30 and C.by_name("start-k31+1").T == 256 + 128 * 31 + 1
    assert {frames[f"tile-{j}"] for j in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)} == {TILE - 1, TILE, TILE + 1, 2 * TILE + 1}
    assert frames["silent-leaves-30"] == 30 and frames["silent-leaves-29"] == 29
    assert frames["silent-leading"] == frames["silent-interior"] == 39 and frames["silent-trailing"] == 40  # of 45
    assert frames["silent-alternate"] == 39  # of 60: every third of 61 frames removed
    assert {C.by_name(f"fs-{fs}").fs for fs in (8000, 16000, 24000, 44100)} == {8000, 16000, 24000, 44100}
    assert all(35 <= frames[f"fs-{fs}"] <= 45 for fs in (8000, 16000, 24000, 44100))
    assert frames["one-sample"] == frames["T-255"] == 0 and frames["long-16000"] > 150
    assert len(C.RAGGED) == 6 and {c.fs for c in C.RAGGED} == {R.FS} and len({c.T for c in C.RAGGED}) == 6
    scores = [c.vec().score for c in TABLE if not c.short and not c.zero_clean]
    assert min(scores) < 0.5 and max(scores) > 0.99  # -5 .. 30 dB


def test_filter_lengths_and_band_table():
    assert [R.filter_half_length(*R.ratio(fs)) for fs in (8000, 16000, 24000, 48000, 44100)] == [182, 290, 435, 870, 15973]
    taps = [-(-(2 * R.filter_half_length(*R.ratio(fs)) + 1) // R.ratio(fs)[0]) for fs in (8000, 16000, 24000, 48000, 44100)]
    assert taps == [73, 117, 175, 349, 320]
    assert R.band_edges() == R.BANDS
    assert R.BANDS[0] == (7, 9) and R.BANDS[-1] == (174, 219) and all(a[1] == b[0] for a, b in zip(R.BANDS, R.BANDS[1:]))
    h = R.kaiser_filter_vec(5, 8)
    assert np.allclose(h, R.kaiser_filter_direct(5, 8), rtol=0, atol=1e-15)
    assert R.EPS == 2.0 ** -52 and list(R.frame_starts(256 + 128 * 3)) == [0, 128, 256] and list(R.frame_starts(256)) == []


def test_resamplers_agree_sample_by_sample():
    x = C.by_name("fs-44100").pair[1][:3000]
    for fs in (8000, 16000, 44100):
        a, b = R.resample_vec(x, fs), R.resample_direct(x, fs)
        assert a.shape == b.shape == (-(-3000 * R.ratio(fs)[0] // R.ratio(fs)[1]),)
        assert np.max(np.abs(a - b)) <= 5e-14  # taps x eps x sum |h| x max |x| = 320 x 1.1e-16 x 2 x 0.5


def test_below_thirty_frames_is_the_constant():
    X = np.abs(np.random.default_rng(0).standard_normal((15, 29)))
    for ext in (False, True):
        assert R.score_vec(X, X, ext) == R.score_direct(X, X, ext) == 1e-5
        assert R.score_vec(np.c_[X, X[:, :1]], np.c_[X, X[:, :1]], ext) == pytest.approx(1.0, abs=1e-12)


def test_identity_and_gain_invariance():
    est, ref = C.by_name("silent-interior").pair
    for route in (R.stoi_vec, R.stoi_direct):
        for ext in (False, True):
            assert route(ref, ref, R.FS, ext).score == pytest.approx(1.0, abs=1e-12)
        base = route(est, ref, R.FS).score
        for gain in (0.25, 3.0, 100.0):
            assert route(est.astype(np.float64) * gain, ref, R.FS).score == pytest.approx(base, abs=1e-12)


# ---- names and bindings ----
def test_names(built_lib):
    assert M.INTELLIGIBILITY_METRICS == ("stoi", "stoi-ext")
    assert M.OPTIONAL_METRICS == ("sdr",) and M.AVAILABLE_METRICS == ("lsd", "si-lsd", "si-sdr", "snr")
    assert "stoi" in M.EXTERNAL_METRICS and "stoi-ext" in M.EXTERNAL_METRICS
    with pytest.raises(NotImplementedError, match="Metric stoi is not supported: it needs a model or a package"):
        M.check_score_names(["si-sdr", "stoi"])
    with pytest.raises(NotImplementedError, match="stoi"):
        M.Metrics(metrics=["lsd", "stoi-ext"])
    assert M.check_score_names(None) == list(M.AVAILABLE_METRICS)
    assert M.check_intelligibility_names(["stoi-ext", "stoi"]) == ["stoi-ext", "stoi"] and M.check_intelligibility_names(()) == []
    x = torch.zeros(2, 1000)
    with pytest.raises(ValueError, match="pesq"):
        M.evaluate_many([x[0]], [x[1]], 16000, intelligibility=["pesq"])
    with pytest.raises(ValueError, match="sdr"):
        M.evaluate_many([x[0]], [x[1]], 16000, intelligibility=["stoi", "sdr"])
    with pytest.raises(NotImplementedError, match="stoi"):
        M.evaluate_many([x[0]], [x[1]], 16000, metrics=["stoi"])
    assert "intelligibility" in M.__doc__ and "stoi" in M.__doc__


def test_header_and_bindings(built_lib):
    header = (ROOT / "include" / "ouniverse.h").read_text()
    assert re.search(r"^int ou_stoi_scratch_bytes\(int32_t B, int64_t T_max, int32_t fs, size_t\* nbytes\);", header, re.M)
    assert re.search(r"^int ou_stoi\(const float\* est, const float\* ref, int64_t stride, const int64_t\* len_host, int32_t B, "
                     r"int32_t fs, int32_t extended,", header, re.M)
    assert re.search(r"^#define OU_ABI_VERSION 7 ", header, re.M) and _lib.OU_ABI_VERSION == 7
    for name in ("ou_stoi_scratch_bytes", "ou_stoi", "ou_stoi_frame_tile"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(built_lib, name)
    assert "ou_stoi(est, ref, stride, len_host, B, fs, extended, out, scratch, n, stream)" in (ROOT / "INTEGRATION.md").read_text()


# ---- the raw ABI: host buffers stand in for device memory -- a refusal touches none of them ----
def _call(L, B=2, T=1000, fs=16000, scratch_bytes=1 << 40, lens=None, extended=0):
    x = np.zeros((B, T), np.float32)
    out = np.full(B, 7.0, np.float32)
    scratch = np.zeros(64, np.uint8)
    lens = (c_int64 * max(B, 1))(*([T] * B if lens is None else lens))
    p = lambda a: c_void_p(a.ctypes.data)
    rc = L.ou_stoi(p(x), p(x), T, lens, B, fs, extended, p(out), p(scratch), c_size_t(scratch_bytes), None)
    assert (out == 7.0).all() and not scratch.any()
    return rc


def _refused(L, code, want, *words):
    assert code == want, (code, L.ou_last_error(None))
    msg = L.ou_last_error(None).decode()
    for w in words:
        assert w in msg, msg


def test_abi_refusals_launch_nothing(built_lib):
    L = built_lib
    _refused(L, _call(L, fs=0), _lib.OU_EINVAL, "fs = 0")
    _refused(L, _call(L, fs=-16000), _lib.OU_EINVAL, "fs = -16000")
    _refused(L, _call(L, fs=10001), _lib.OU_EINVAL, "fs = 10001", "OU_STOI_MAX_TAPS = 2048", "OU_STOI_MAX_TABLE_BYTES")
    _refused(L, _call(L, fs=1), _lib.OU_EINVAL, "fs = 1")
    _refused(L, _call(L, B=0), _lib.OU_EINVAL, "B must be at least 1")
    _refused(L, _call(L, lens=[1000, 0]), _lib.OU_EINVAL, "len[1]")
    _refused(L, _call(L, lens=[1001, 5]), _lib.OU_EINVAL, "len[0]")  # behind the stride
    for fs in (10000, 16000, 44100):
        _refused(L, _call(L, fs=fs, scratch_bytes=64), _lib.OU_ESHAPE, "ou_stoi_scratch_bytes asks for")
        _refused(L, _call(L, fs=fs, scratch_bytes=M.stoi_scratch_bytes(2, 1000, fs) - 1, extended=1), _lib.OU_ESHAPE, "scratch")
    n = c_size_t()
    _refused(L, L.ou_stoi_scratch_bytes(2, 1000, 0, byref(n)), _lib.OU_EINVAL, "fs = 0")
    _refused(L, L.ou_stoi_scratch_bytes(0, 1000, 16000, byref(n)), _lib.OU_EINVAL, "B >= 1")
    _refused(L, L.ou_stoi_scratch_bytes(2, 0, 16000, byref(n)), _lib.OU_EINVAL, "T_max")
    _refused(L, L.ou_stoi_scratch_bytes(1, 2 ** 31 - 1, 8000, byref(n)), _lib.OU_EINVAL, "at 10 kHz")  # 5 / 4 of 2^31 samples


def test_scratch_sizer(built_lib):
    """Pure host code: this test runs without a GPU.  Monotone in B and T; every rate of the header's list is accepted."""
    f = M.stoi_scratch_bytes
    for fs in (8000, 10000, 16000, 22050, 24000, 32000, 44100, 48000, 96000):
        for B, T in ((1, 1), (3, 700), (16, 64000)):
            assert 0 < f(B, T, fs) <= f(B + 1, T, fs) and f(B, T, fs) <= f(B, T + 1, fs) <= f(B, 4 * T + 10000, fs)
        assert f(1, 1, fs) < f(64, 100000, fs) and f(2, 1000, fs) < f(2, 1000000, fs)
    # the band values: (rows, 2 signals, 15 bands, frames) doubles, whatever else there is
    assert f(16, 64000, 16000) >= 16 * 2 * 15 * ((40000 - 256) // 128) * 8
    assert f(4, 40000, 10000) < f(4, 64000, 16000)  # the same 4 s: 16 kHz also holds the resampled signals and the table
    for fs in (0, -1, 10001, 7919):
        with pytest.raises(ValueError, match=f"fs = {fs}"):
            f(1, 1000, fs)


def test_python_refusals_and_no_cpu_path(built_lib):
    x = torch.zeros(2, 1000)
    with pytest.raises(ValueError, match="fs = 0"):
        M.stoi(x, x, 0)
    with pytest.raises(ValueError, match="integer"):
        M.stoi(x, x, 16000.5)
    with pytest.raises(ValueError, match="shapes"):
        M.stoi(x, x[:, :900], 16000)
    # with everything in order, a tensor that is not on a HIP device is refused: no CPU path, no fallback
    for ext in (False, True):
        with pytest.raises(ValueError, match="HIP device"):
            M.stoi(x, x, 16000, extended=ext)
    with pytest.raises(ValueError, match="HIP device"):
        M.evaluate_many([x[0]], [x[1]], 16000, metrics=["snr"], intelligibility=["stoi"])


def test_cli_accepts_the_option(tmp_path, monkeypatch):
    from open_universe_amd import audio

    monkeypatch.setattr(audio, "_torchaudio", lambda: None)  # the built-in WAV codec, whatever else this process has imported
    for d in ("clean", "enh"):
        (tmp_path / d).mkdir()
        audio.save(tmp_path / d / "a.wav", torch.linspace(-0.5, 0.5, 500)[None], 16000)
    args = [str(tmp_path / "clean"), str(tmp_path / "enh"), "--device", "cpu", "--result-dir", str(tmp_path / "out")]
    # the parser and the name checks pass; scoring then asks for the device the files are to be moved to
    with pytest.raises((RuntimeError, AssertionError, ValueError)) as e:
        CLI.main(args + ["--metrics", "si-sdr", "--intelligibility", "stoi"])
    assert "HIP device" in str(e.value)
    with pytest.raises(SystemExit):
        CLI.main(args + ["--intelligibility", "pesq"])
    with pytest.raises(NotImplementedError, match="Metric stoi is not supported"):
        CLI.main(args + ["--metrics", "stoi"])
    assert "--intelligibility" in CLI.__doc__
