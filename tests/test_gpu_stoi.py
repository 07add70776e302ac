"""GPU (-m gpu): STOI and extended STOI of open_universe_amd.metrics.stoi (ou_stoi; csrc/ou_stoi.hip) against the float64
restatements of tests/stoi_ref.py on the cases of tests/stoi_cases.py.

The gate of every gated case and both forms:  |library - stoi_vec| <= 4 d_ref + 1 fp32 ulp of the score,  d_ref = |stoi_vec -
stoi_direct| of that case.  The ulp is there because `out` is fp32; the factor 4 because the kernels do the restatements'
arithmetic in the same precision in another summation order.  d_ref is 0 .. 2e-16 on these cases (test_stoi_cpu.py prints it),
so this is a gate of one fp32 ulp.  Every case prints distance / bound before it asserts.

pystoi, the package the reference takes these numbers from, is not available to this project: nothing here compares against a
recording of it.

Shapes: the frame count round the cut of 30 and one sample either side of a frame start, frame counts round one, two and three
STFT frame tiles of the kernel (ou_stoi_frame_tile), silent stretches (leading, trailing, interior, every third frame, leaving
exactly 30 and 29 frames), 8, 16, 24 and 44.1 kHz, one sample, 255 samples, an all-zero clean signal, 3 s at 16 kHz, and a
ragged batch of six rows.  The edges (stoi_cases.EDGE): 1023, 1024, 1025, 2048 and 2049 energy frames with none silent and 2101
with silent stretches across frames 1024 and 2048 (the chunks of the kept-frame scan), 45 and 46 frames (the segment tile),
one second at 48, 22.05, 6 and 12 kHz, and 14 s at 48 kHz.  Ragged calls of 130 rows (stoi_cases.MANY: launch groups of 64, 64
and 2) at 10 and 16 kHz, one sample or a row below 30 frames at rows 63, 64, 127 and 128, the one longest row last or first;
`evaluate_many` on 70 pairs.

Measured on an MI355X (DESIGN 4.22 has the table): distance / bound 0.00 .. 0.49 over the 22 gated cases in both forms -- the
rounding of `out` to fp32 --, every below-30 case exactly float32(1e-5), and every row of the ragged batch equal to the row
scored alone; 0.01 .. 0.47 over the 13 edge cases in both forms, and each of the 130 rows equal to the row scored alone."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import stoi_cases as C
import stoi_ref as R
from open_universe_amd import _lib, audio, metrics as M
from open_universe_amd.bin import eval_metrics as CLI

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 16  # what the case table is built for; test_the_tile_is_the_one_the_cases_assume holds it against ou_stoi_frame_tile
TABLE = C.table(TILE)
GATED = [c for c in TABLE if not c.short]
SHORT = [c for c in TABLE if c.short]
FORMS = (False, True)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _score(case, extended):
    est, ref = case.pair
    return float(M.stoi(_dev(est), _dev(ref), case.fs, extended=extended))


def _check(case, extended, lib):
    assert case.gated, case
    want = case.vec(extended).score
    dist, bound = abs(lib - want), case.bound(extended)
    print(f"{case} {'estoi' if extended else 'stoi'}: lib {lib:.9g} vec {want:.12g} dist {dist:.3g} bound {bound:.3g} "
          f"dist/bound {dist / bound:.3f} d_ref {case.d_ref(extended):.3g} frames {case.frames} margin {case.margin:.3g} dB")
    assert dist <= bound, (case, extended, lib, want, dist, bound)


def test_the_tile_is_the_one_the_cases_assume():
    assert int(_lib.load().ou_stoi_frame_tile()) == TILE
    assert {f"tile-{TILE - 1}", f"tile-{TILE}", f"tile-{TILE + 1}", f"tile-{2 * TILE + 1}"} <= {c.name for c in TABLE}


@pytest.mark.parametrize("extended", FORMS, ids=("stoi", "estoi"))
@pytest.mark.parametrize("case", GATED, ids=repr)
def test_accuracy_gate(case, extended):
    _check(case, extended, _score(case, extended))


@pytest.mark.parametrize("extended", FORMS, ids=("stoi", "estoi"))
@pytest.mark.parametrize("case", SHORT, ids=repr)
def test_below_thirty_frames_scores_the_constant(case, extended):
    assert case.frames < R.SEGMENT and case.vec(extended).score == R.SHORT
    got = M.stoi(_dev(case.pair[0]), _dev(case.pair[1]), case.fs, extended=extended)
    assert got.dtype == torch.float32 and np.float32(got.item()) == np.float32(1e-5), (case, float(got))


@pytest.fixture(scope="module")
def ragged():
    """Six rows of lengths of their own in one (B, stride) buffer each, NaN behind every row."""
    lens = [c.T for c in C.RAGGED]
    stride = max(lens) + 4
    x = torch.full((len(lens), stride), float("nan"), device=DEV)
    y = torch.full((len(lens), stride), float("nan"), device=DEV)
    for b, c in enumerate(C.RAGGED):
        x[b, :c.T], y[b, :c.T] = _dev(c.pair[0]), _dev(c.pair[1])
    return x, y, lens


@pytest.mark.parametrize("extended", FORMS, ids=("stoi", "estoi"))
def test_rows_in_a_batch(ragged, extended):
    """Each row of the ragged batch is bit for bit its own B = 1 call, two runs are bit-identical, the NaN behind the rows
    (and zeros in their place) change nothing, and every row holds the gate or scores the constant."""
    x, y, lens = ragged
    a = M._stoi_rows(x, y, lens, R.FS, extended)
    b = M._stoi_rows(x, y, lens, R.FS, extended)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    x0, y0 = torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)
    assert torch.equal(a, M._stoi_rows(x0, y0, lens, R.FS, extended))
    for i, c in enumerate(C.RAGGED):
        alone = M.stoi(x[i, :c.T], y[i, :c.T], R.FS, extended=extended)
        assert torch.equal(alone, a[i]), (c, float(alone), float(a[i]))
        if c.short:
            assert np.float32(a[i].item()) == np.float32(1e-5)
        else:
            _check(c, extended, float(a[i]))


def test_rows_in_a_batch_at_another_rate():
    """The resampler's rows too: two rows of 16 kHz in one call against each alone."""
    cases = [C.by_name("fs-16000"), C.by_name("long-16000")]
    est, ref = [_dev(c.pair[0]) for c in cases], [_dev(c.pair[1]) for c in cases]
    x, y, lens = M.pack_pairs(est, ref)
    x[0, lens[0]:], y[0, lens[0]:] = float("nan"), float("nan")
    both = M._stoi_rows(x, y, lens, 16000, False)
    for i, c in enumerate(cases):
        assert torch.equal(both[i], M.stoi(est[i], ref[i], 16000)), c
        _check(c, False, float(both[i]))


@pytest.mark.parametrize("extended", FORMS, ids=("stoi", "estoi"))
@pytest.mark.parametrize("case", C.EDGE, ids=repr)
def test_edge_accuracy_gate(case, extended):
    """mask-*: more than 1024 energy frames in stoi_mask_kernel -- 1023, 1024, 1025, 2048 and 2049 frames with none silent,
    and 2101 with silent stretches across frames 1024 and 2048, so the scan's second and third chunks run with a carried base
    that is not the chunk's first frame and `src` is written past the first chunk.  segtile-*: the segment-tile border of
    stoi_seg_kernel, 45 frames (exactly one tile of 16 segments) and 46 (the first segment of a second).  fs-*: the resampling
    ratios 5/24 (48 kHz), 200/441 (22.05 kHz), 5/3 (6 kHz, up-sampling) and 5/6 (12 kHz); long-48000: 14 s at 48 kHz, a
    resampled row that needs a second mask chunk.  The gate of every other case."""
    _check(case, extended, _score(case, extended))


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


#: (index into C.MANY, extended): 10 kHz in both forms and both arrangements, 16 kHz in one form per arrangement
MANY_CALLS = [(0, False), (0, True), (1, False), (1, True), (2, False), (3, True)]


@pytest.mark.parametrize("k,extended", MANY_CALLS, ids=[f"{C.MANY[k]}-{'estoi' if e else 'stoi'}" for k, e in MANY_CALLS])
def test_130_rows_in_one_call(k, extended):
    """Rows 64 and up: 130 ragged rows are launch groups of 64, 64 and 2, so the second and third run with row0 = 64 and 128
    in every kernel (signals, res_*, energy, src, count, bands, partial and out at row0 + block, the by-value lengths at the
    block), one sample and a row below 30 frames at rows 63, 64, 127, 128.  Per-group grid against per-call strides: with the
    longest row last, groups 0 and 1 run grids sized by their own rows inside F, seg_stride and n10 of the call; with it first,
    groups 1 and 2 do.  At 16 kHz stoi_resample_kernel has its own row0 and res_* the call-wide n10 stride.  Two runs are
    bit-identical, zeros for the NaN behind the rows change nothing, EVERY row is bit for bit its own B = 1 call, and every row
    holds the gate or scores the constant."""
    many = C.MANY[k]
    x, y, lens = _many_rows(k)
    a = M._stoi_rows(x, y, lens, many.fs, extended)
    assert a.shape == (130,) and bool(torch.isfinite(a).all())
    assert torch.equal(a, M._stoi_rows(x, y, lens, many.fs, extended))
    assert torch.equal(a, M._stoi_rows(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0), lens, many.fs, extended))
    alone = torch.stack([M.stoi(x[i, :n], y[i, :n], many.fs, extended=extended) for i, n in enumerate(lens)])
    a, alone = a.cpu(), alone.cpu()
    differ = [(i, lens[i], float(a[i]), float(alone[i])) for i in range(len(lens)) if a[i] != alone[i]]
    assert not differ, (many, extended, differ[:8])
    seen = set()
    for i, c in enumerate(many.cases):
        lib = float(a[i])
        if c.short:
            assert np.float32(lib) == np.float32(1e-5), (many, i, c, lib)
        elif c.name in seen:
            assert c.gated and abs(lib - c.vec(extended).score) <= c.bound(extended), (many, i, c, lib)
        else:
            _check(c, extended, lib)
            seen.add(c.name)


def test_evaluate_many_on_70_pairs_is_the_per_pair_functions():
    """The wiring past one launch group: pack_pairs and the column unpacking are the only Python between `evaluate_many` and
    the calls, and 70 pairs put six of them behind row 64 (rows 64 and up of ou_si_sdr, ou_sdr and ou_stoi in one go)."""
    cases = C.MANY[0].cases[:70]
    dev = {c.name: (_dev(c.pair[0]), _dev(c.pair[1])) for c in cases}
    est, ref = [dev[c.name][0] for c in cases], [dev[c.name][1] for c in cases]
    rows = M.evaluate_many(est, ref, R.FS, metrics=["si-sdr", "sdr"], intelligibility=("stoi",))
    assert len(rows) == 70
    want = {name: {"si-sdr": float(M.si_sdr(e, r)), "sdr": float(M.sdr(e, r)), "stoi": float(M.stoi(e, r, R.FS))}
            for name, (e, r) in dev.items()}
    for i, (c, row) in enumerate(zip(cases, rows)):
        assert list(row) == ["si-sdr", "sdr", "stoi"]
        assert row == want[c.name], (i, c, row, want[c.name])


def test_identity_gain_and_shape():
    c = C.by_name("silent-interior")
    est, ref = (_dev(a) for a in c.pair)
    for ext in FORMS:
        assert float(M.stoi(ref, ref, R.FS, extended=ext)) == pytest.approx(1.0, abs=R.ulp32(1.0))
    base = float(M.stoi(est, ref, R.FS))
    assert float(M.stoi(est * 4.0, ref, R.FS)) == pytest.approx(base, abs=R.ulp32(base))  # c rescales the estimate
    both = M.stoi(torch.stack([est, ref])[None], torch.stack([ref, ref])[None], R.FS)
    assert both.shape == (1, 2) and float(both[0, 0]) == base


def test_evaluate_many_adds_the_columns():
    cases = [C.by_name(n) for n in ("frames-30", "silent-trailing", "frames-29")]
    est, ref = [_dev(c.pair[0]) for c in cases], [_dev(c.pair[1]) for c in cases]
    rows = M.evaluate_many(est, ref, R.FS, intelligibility=("stoi", "stoi-ext"))
    for c, row, e, r in zip(cases, rows, est, ref):
        assert list(row) == list(M.AVAILABLE_METRICS) + ["stoi", "stoi-ext"]
        assert row["stoi"] == float(M.stoi(e, r, R.FS)) and row["stoi-ext"] == float(M.stoi(e, r, R.FS, extended=True))
        assert row["si-sdr"] == float(M.si_sdr(e, r))
    assert list(M.evaluate_many(est, ref, R.FS)[0]) == list(M.AVAILABLE_METRICS)  # the default call is what it was
    assert list(M.evaluate_many(est, ref, R.FS, metrics=["snr"], intelligibility=["stoi-ext"])[0]) == ["snr", "stoi-ext"]


def test_cli_writes_both_columns(tmp_path, monkeypatch):
    """eval_metrics --metrics si-sdr --intelligibility stoi stoi-ext on two small wav pairs at 16 kHz."""
    monkeypatch.setattr(audio, "_torchaudio", lambda: None)  # the built-in WAV codec, whatever else this process has imported
    (tmp_path / "clean").mkdir()
    (tmp_path / "enh").mkdir()
    for i, name in enumerate(("fs-16000", "long-16000")):
        est, ref = C.by_name(name).pair
        audio.save(tmp_path / "clean" / f"f{i}.wav", torch.from_numpy(ref)[None], 16000)
        audio.save(tmp_path / "enh" / f"f{i}.wav", torch.from_numpy(est)[None], 16000)
    assert CLI.main([str(tmp_path / "clean"), str(tmp_path / "enh"), "--metrics", "si-sdr", "--intelligibility", "stoi", "stoi-ext",
                     "--batch-size", "2", "--result-dir", str(tmp_path / "out")]) == 0
    res = json.load(open(tmp_path / "out" / "enh.json"))
    summary = json.load(open(tmp_path / "out" / "enh_summary.json"))
    assert sorted(res) == ["f0", "f1"] and summary["number"] == 2
    for i in range(2):
        deg, _ = audio.load(tmp_path / "enh" / f"f{i}.wav")
        ref, _ = audio.load(tmp_path / "clean" / f"f{i}.wav")
        assert list(res[f"f{i}"]) == ["si-sdr", "stoi", "stoi-ext"]
        assert res[f"f{i}"]["stoi"] == float(M.stoi(deg[0].to(DEV), ref[0].to(DEV), 16000))
        assert res[f"f{i}"]["stoi-ext"] == float(M.stoi(deg[0].to(DEV), ref[0].to(DEV), 16000, extended=True))
        assert 0.0 < res[f"f{i}"]["stoi-ext"] < res[f"f{i}"]["stoi"] < 1.0
    assert summary["stoi"] == pytest.approx((res["f0"]["stoi"] + res["f1"]["stoi"]) / 2, abs=1e-9) and "stoi-ext_std" in summary


def test_abi_refusals_on_the_device():
    """A short scratch is OU_ESHAPE and a refused fs OU_EINVAL; neither launches anything: `out` keeps what it held."""
    L = _lib.load()
    c = C.by_name("frames-30")
    est, ref = (_dev(a)[None] for a in c.pair)
    out = torch.full((1,), 7.0, device=DEV)
    need = M.stoi_scratch_bytes(1, c.T, R.FS)
    scratch = torch.zeros(need, dtype=torch.uint8, device=DEV)
    lens = (ctypes.c_int64 * 1)(c.T)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(fs, nbytes):
        return L.ou_stoi(p(est), p(ref), c.T, lens, 1, fs, 0, p(out), p(scratch), ctypes.c_size_t(nbytes), stream)

    assert call(R.FS, need - 1) == _lib.OU_ESHAPE and b"ou_stoi_scratch_bytes asks for" in L.ou_last_error(None)
    assert call(0, need) == _lib.OU_EINVAL and b"fs = 0" in L.ou_last_error(None)
    assert call(10001, 1 << 40) == _lib.OU_EINVAL and b"OU_STOI_MAX_TAPS" in L.ou_last_error(None)
    torch.cuda.synchronize()
    assert float(out) == 7.0 and not bool(scratch.any())
    assert call(R.FS, need) == _lib.OU_OK
    torch.cuda.synchronize()
    assert float(out) == float(M.stoi(est[0], ref[0], R.FS))
