"""GPU (-m gpu): the scores of open_universe_amd.metrics (ou_lsd, ou_spectral_mae, ou_si_sdr; csrc/ou_metrics.hip) against the float64
restatement of tests/metrics_ref.py.

The gate of every figure:  |library - f64| <= 4 x max(|f32 - f64|, 1 ulp of the f64 value in fp32), f32 = the same restatement
evaluated in float32 on the same inputs (the reference's own agreement); the factor 4 stands for the other summation order (the
K order of the matrix pipe, per-workgroup partials).  The library's DFT runs in double (DESIGN 4.20 says why), so what is left
of its error is the rounding of the result to fp32: ratios up to 0.5.  Signals: seeded noise + two sinusoids, estimate = 0.7 reference + 0.05
noise.  Every case logs err / max(...) to build/observed/metrics_observed.json (untracked) before it asserts;
profiles/metrics_observed.json is a committed copy.

Lengths: 201 = the shortest the reflect padding allows at n_fft 400 (2 frames: a frame tile of two); 479 / 480 / 481 around
3 hops (480: 4 frames, the last one centred on the sample behind the row); 16000: 101 frames = 6 tiles of 16 and a last tile of
FIVE frames; 201 bins = 12 tiles of 16 and a tile of 9.

The shapes of test_g / test_h / test_i reach what those lengths and n_fft 400 / 600 / 64 / 256 / 512 do not: n_fft % 4 == 2
(Kpad != n_fft: the zero words of the frames, window and basis behind n_fft are live), n_fft / 4 rounded up = 1, 2, 3 mod 4
(the remainder loop behind the 4-deep MFMA pipeline), n_fft 2 (one k-step, two bins) and 1024 (the cap: all of the dynamic
LDS), hop 1, a hop above n_fft, hops that do not divide n_fft, rows of exactly 16 and 17 frames (a full frame tile; a full tile
and a tile of one), and 130 rows in one call (launches of 64, 64 and 2 rows, the longest row in the last one).

Measured on an MI355X (profiles/metrics_observed.json, `worst_ratio` = err / max(|f32 - f64|, 1 ulp), gate 4): test_g 0.025 ..
0.483 (worst: LSD at n_fft 1022), test_h 0.338 and 0.324, test_i 0.141 .. 0.498 (worst: the L1 of row 63), every one of the
130 rows equal to the row scored alone -- no higher than the 0.5 of the shapes above."""
import json
import os
import statistics

import pytest
import torch

import metrics_ref as R
from open_universe_amd import metrics as M

pytestmark = pytest.mark.gpu

_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed")
LENGTHS = (201, 400, 479, 480, 481, 16000)
L1_LENGTHS = (33, 512, 4001)
L1_WINDOWS = [64, 256, 512]
DEV = "cuda:0"


def _log(case, figures):
    try:
        os.makedirs(_OUT, exist_ok=True)
        path = os.path.join(_OUT, "metrics_observed.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[case] = figures
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError as e:  # (the figures follow on stdout)
        print(f"metrics_observed.json not written: {e}")


def _gate(case, rows):
    """rows: [(label, library value, f64, f32)]: log and print every figure, then assert every one."""
    figs = []
    for label, lib, f64, f32 in rows:
        err, bound, ratio = R.gate(lib, f64, f32)
        figs.append({"row": label, "lib": float(lib), "f64": float(f64), "f32_minus_f64": float(f32) - float(f64), "err": err,
                     "bound": bound, "ratio": ratio})
        print(f"{case} {label}: lib {float(lib):.9g} f64 {float(f64):.12g} err {err:.3g} bound {bound:.3g} err/own {ratio:.2f}")
    _log(case, {"worst_ratio": max(f["ratio"] for f in figs), "figures": figs})
    for f in figs:
        assert f["err"] <= f["bound"], f"{case} {f}"


@pytest.fixture(scope="module")
def pairs():
    return R.signals(LENGTHS, seed=0)


def _pack_nan(prs):
    """Pairs as a ragged batch on the device: one (B, stride) buffer each, filled with NaN behind every row -> (x, y, lengths)"""
    lens = [e.shape[0] for e, _ in prs]
    stride = max(lens) + 4
    x = torch.full((len(prs), stride), float("nan"), device=DEV)
    y = torch.full((len(prs), stride), float("nan"), device=DEV)
    for b, (e, r) in enumerate(prs):
        x[b, :e.shape[0]] = e.to(DEV)
        y[b, :r.shape[0]] = r.to(DEV)
    return x, y, lens


@pytest.fixture(scope="module")
def ragged(pairs):
    """The ragged batch on the device: rows of LENGTHS in one (B, stride) buffer filled with NaN behind every row."""
    return _pack_nan(pairs)


def _lsd_case(case, pairs, ragged, n_fft, hop, eps, si, db, keep=lambda T: True):
    x, y, lens = ragged
    idx = [i for i, T in enumerate(lens) if keep(T)]
    xs, ys, ls = x[idx], y[idx], [lens[i] for i in idx]
    lib = M._lsd_rows(xs, ys, ls, n_fft, hop, eps, si, db).cpu()
    rows = []
    for j, i in enumerate(idx):
        e, r = pairs[i]
        f64 = R.lsd(e, r, n_fft, hop, eps, si, db, torch.float64)
        f32 = R.lsd(e, r, n_fft, hop, eps, si, db, torch.float32)
        rows.append((f"T={lens[i]}", lib[j], f64, f32))
    _gate(case, rows)
    return lib


def test_a_lsd_and_si_lsd_16k(pairs, ragged):
    plain = _lsd_case("a_lsd_400_160", pairs, ragged, 400, 160, 1e-7, False, True)
    si = _lsd_case("a_si_lsd_400_160", pairs, ragged, 400, 160, 1e-7, True, True)
    assert (plain - si).abs().min() > 0.1  # 0.7 x the reference: 3 dB of level that the scale-invariant form takes out
    # the public function on whole rows is the same call
    e, r = pairs[-1]
    one = M.log_spectral_distance(e.to(DEV)[None], r.to(DEV)[None])
    assert one.shape == (1,) and one.cpu()[0] == plain[-1]
    assert M.LogSpectralDistance(eps=1e-7)(e.to(DEV)[None], r.to(DEV)[None]).cpu() == plain[-1]


@pytest.mark.parametrize("case,n_fft,hop,eps,si,db", [
    ("b_lsd_600_240", 600, 240, 1e-7, False, True),
    ("b_si_lsd_600_240", 600, 240, 1e-7, True, True),
    ("b_lsd_600_240_ln", 600, 240, 1e-7, False, False),
    ("b_si_lsd_400_160_ln_eps1e-5", 400, 160, 1e-5, True, False),
])
def test_b_lsd_24k_setting_and_natural_log(pairs, ragged, case, n_fft, hop, eps, si, db):
    """The 24 kHz setting on the rows with T >= 301, and db = False (both once with the class default eps of 1e-5)."""
    _lsd_case(case, pairs, ragged, n_fft, hop, eps, si, db, lambda T: T > n_fft // 2)  # n_fft 600: T >= 301


@pytest.mark.parametrize("tdw", [0.5, 0.0])
@pytest.mark.parametrize("si", [False, True])
def test_c_multires_l1(tdw, si):
    prs = R.signals(L1_LENGTHS, seed=1)
    x, y, lens = M.pack_pairs([e.to(DEV) for e, _ in prs], [r.to(DEV) for _, r in prs])
    loss = M.MultiResL1SpecLoss(window_sz=L1_WINDOWS, eps=1e-8, time_domain_weight=tdw, scale_invariant=si)
    lib = loss.per_row(y, x, lengths=lens).cpu()
    rows = []
    for b, (e, r) in enumerate(prs):
        f64 = R.spectral_l1(e, r, L1_WINDOWS, None, 1e-8, tdw, si, torch.float64)
        f32 = R.spectral_l1(e, r, L1_WINDOWS, None, 1e-8, tdw, si, torch.float32)
        rows.append((f"T={lens[b]}", lib[b], f64, f32))
    _gate(f"c_l1_tdw{tdw}_si{int(si)}", rows)
    e, r = prs[1]
    whole = loss(r.to(DEV)[None], e.to(DEV)[None])  # forward(target, estimate): the mean over the batch, here of one row
    assert whole.ndim == 0 and whole.cpu() == lib[1]
    # no resolution: the time-domain mean alone (multires_stft.py:107-108)
    td = M.MultiResL1SpecLoss(window_sz=[], scale_invariant=si).per_row(r.to(DEV)[None], e.to(DEV)[None]).cpu()
    _gate(f"c_l1_time_only_si{int(si)}", [("T=512", td[0], R.spectral_l1(e, r, [], None, 1e-8, 0.5, si, torch.float64),
                                           R.spectral_l1(e, r, [], None, 1e-8, 0.5, si, torch.float32))])


def test_d_si_sdr_and_snr(pairs, ragged):
    x, y, lens = ragged
    a, b = M._sdr_rows(x, y, lens, 100.0)
    a, b = a.cpu(), b.cpu()
    rows = []
    for i, (e, r) in enumerate(pairs):
        rows.append((f"si-sdr T={lens[i]}", a[i], R.si_sdr(e, r, 100.0, torch.float64), R.si_sdr(e, r, 100.0, torch.float32)))
        rows.append((f"snr T={lens[i]}", b[i], R.snr(e, r, 100.0, torch.float64), R.snr(e, r, 100.0, torch.float32)))
    _gate("d_si_sdr_snr", rows)
    r = pairs[-1][1].to(DEV)
    for clamp in (100.0, 30.0):  # identical signals: the clamp itself
        assert M.si_sdr(r, r, clamp_db=clamp).cpu().item() == pytest.approx(clamp, abs=1e-5)
        assert M.snr(r, r, clamp_db=clamp).cpu().item() == pytest.approx(clamp, abs=1e-5)
    z = torch.zeros_like(r)  # an all-zero estimate: finite
    assert M.si_sdr(z, r).cpu().item() == pytest.approx(-100.0, abs=1e-5)
    assert M.snr(z, r).cpu().item() == pytest.approx(0.0, abs=1e-5)
    assert torch.isfinite(M.si_sdr(z, z).cpu()).all() and torch.isfinite(M.snr(z, z).cpu()).all()
    assert torch.isfinite(M.log_spectral_distance(z, r).cpu()).all()


def test_e_rows_are_independent_and_runs_identical(pairs, ragged):
    x, y, lens = ragged
    calls = {
        "lsd": lambda x, y, l: M._lsd_rows(x, y, l, 400, 160, 1e-7, False, True),
        "si-lsd": lambda x, y, l: M._lsd_rows(x, y, l, 400, 160, 1e-7, True, True),
        "l1": lambda x, y, l: M._l1_rows(x, y, l, L1_WINDOWS, [32, 128, 256], 1e-8, 0.5, True),
        "si-sdr": lambda x, y, l: M._sdr_rows(x, y, l, 100.0)[0],
        "snr": lambda x, y, l: M._sdr_rows(x, y, l, 100.0)[1],
    }
    clean_x, clean_y = torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)
    for name, call in calls.items():
        first, second = call(x, y, lens).cpu(), call(x, y, lens).cpu()
        assert torch.isfinite(first).all(), name  # NaN behind every row's len: never read
        assert torch.equal(first, second), name  # two runs: bit-identical
        assert torch.equal(first, call(clean_x, clean_y, lens).cpu()), name  # what lies behind a row changes nothing
        for b, (e, r) in enumerate(pairs):  # every row = the same row alone, bit for bit
            alone = call(e.to(DEV)[None], r.to(DEV)[None], [lens[b]]).cpu()
            assert alone[0] == first[b], (name, lens[b], float(alone[0]), float(first[b]))


def test_evaluate_many_and_metrics_agree(pairs):
    est, ref = [e.to(DEV) for e, _ in pairs], [r.to(DEV)[: r.shape[0] - 3] for _, r in pairs]  # references 3 samples short
    many = M.evaluate_many(est, ref, 16000)
    assert [sorted(d) for d in many] == [["lsd", "si-lsd", "si-sdr", "snr"]] * len(pairs)
    m = M.Metrics()
    for b in (0, 3, 5):
        assert m(16000, est[b], ref[b]) == many[b]  # one pair alone: padded to the longer, scored the same, bit for bit
    two = M.Metrics(metrics=["si-sdr", "lsd"])(16000, torch.stack([est[5], est[5]]), torch.stack([pairs[5][1].to(DEV)] * 2))
    assert len(two) == 2 and two[0] == two[1] and list(two[0]) == ["si-sdr", "lsd"]


# (n_fft, hop): n_fft / 4 rounded up = 1, 2, 8, 101, 256, 256, 101, 103, 16; 2, 6, 30, 402 and 1022 leave zero words behind n_fft
G_SHAPES = [(2, 1), (6, 1), (30, 7), (402, 160), (1022, 256), (1024, 256), (404, 101), (412, 103), (64, 100)]


def _shape_lengths(n_fft, hop):
    """Ragged rows for one (n_fft, hop), every one above n_fft / 2: the shortest the reflect padding allows, exactly 16 frames,
    exactly 17 frames, and a few hops."""
    lens = [n_fft // 2 + 1, 15 * hop + hop // 2, 16 * hop, max(3 * hop + 1, n_fft // 2 + 3)]
    assert M.frames(lens[1], hop) == 16 and M.frames(lens[2], hop) == 17 and min(lens) > n_fft // 2
    return lens


@pytest.mark.parametrize("si", [False, True])
@pytest.mark.parametrize("n_fft,hop", G_SHAPES)
def test_g_lsd_at_the_edges_of_the_accepted_resolutions(n_fft, hop, si):
    prs = R.signals(_shape_lengths(n_fft, hop), seed=10 + n_fft)
    lib = _lsd_case(f"g_{'si_' if si else ''}lsd_{n_fft}_{hop}", prs, _pack_nan(prs), n_fft, hop, 1e-7, si, True)
    assert torch.isfinite(lib).all()


H_WINDOWS, H_HOPS = [2, 30, 1022, 1024], [1, 7, 256, 300]  # 7 does not divide 30, 256 not 1022, 300 not 1024
H_LENGTHS = (300, 1022, 4001)  # 300: shorter than half the largest window


@pytest.mark.parametrize("si", [False, True])
def test_h_multires_l1_smallest_and_largest_windows(si):
    prs = R.signals(H_LENGTHS, seed=4)
    x, y, lens = _pack_nan(prs)
    lib = M._l1_rows(x, y, lens, H_WINDOWS, H_HOPS, 1e-8, 0.5, si).cpu()
    rows = []
    for b, (e, r) in enumerate(prs):
        f64 = R.spectral_l1(e, r, H_WINDOWS, H_HOPS, 1e-8, 0.5, si, torch.float64)
        f32 = R.spectral_l1(e, r, H_WINDOWS, H_HOPS, 1e-8, 0.5, si, torch.float32)
        rows.append((f"T={lens[b]}", lib[b], f64, f32))
    _gate(f"h_l1_2_30_1022_1024_si{int(si)}", rows)


I_ROWS, I_GATED = 130, (0, 63, 64, 127, 128, 129)
I_LSD = (400, 43)  # hop 43: the rows of the first launch have one frame tile, the longest row of the call two
I_L1_HOPS = [43, 128, 1]  # of L1_WINDOWS; hop 1 at 512: 43 frame tiles in the first launch, 44 in the call


@pytest.fixture(scope="module")
def many():
    """130 rows in one call (launches of 64, 64 and 2 rows): lengths drawn from 201 ... 700, the longest row moved into the last
    launch and the shortest into the first, so the launches' grids differ from one another and from the call's tile stride."""
    lens = torch.randint(201, 701, (I_ROWS,), generator=torch.Generator().manual_seed(5)).tolist()
    i = lens.index(max(lens))
    lens[i], lens[I_ROWS - 1] = lens[I_ROWS - 1], lens[i]
    i = lens.index(min(lens))
    lens[i], lens[0] = lens[0], lens[i]
    tiles = lambda T, hop: (M.frames(T, hop) + 15) // 16
    for hop in (I_LSD[1], I_L1_HOPS[0], I_L1_HOPS[2]):
        assert tiles(max(lens[:64]), hop) < tiles(max(lens[128:]), hop) == tiles(max(lens), hop)
    assert min(lens[:64]) == min(lens) and min(lens) > I_LSD[0] // 2
    prs = R.signals(lens, seed=3)
    return prs, _pack_nan(prs)


_I_CALLS = {
    "lsd": lambda x, y, l: M._lsd_rows(x, y, l, I_LSD[0], I_LSD[1], 1e-7, False, True),
    "si-lsd": lambda x, y, l: M._lsd_rows(x, y, l, I_LSD[0], I_LSD[1], 1e-7, True, True),
    "l1": lambda x, y, l: M._l1_rows(x, y, l, L1_WINDOWS, I_L1_HOPS, 1e-8, 0.5, True),
    "si-sdr": lambda x, y, l: M._sdr_rows(x, y, l, 100.0)[0],
    "snr": lambda x, y, l: M._sdr_rows(x, y, l, 100.0)[1],
}
_I_REFS = {
    "lsd": lambda e, r, dt: R.lsd(e, r, I_LSD[0], I_LSD[1], 1e-7, False, True, dt),
    "si-lsd": lambda e, r, dt: R.lsd(e, r, I_LSD[0], I_LSD[1], 1e-7, True, True, dt),
    "l1": lambda e, r, dt: R.spectral_l1(e, r, L1_WINDOWS, I_L1_HOPS, 1e-8, 0.5, True, dt),
    "si-sdr": lambda e, r, dt: R.si_sdr(e, r, 100.0, dt),
    "snr": lambda e, r, dt: R.snr(e, r, 100.0, dt),
}


@pytest.mark.parametrize("name", list(_I_CALLS))
def test_i_130_rows_in_one_call_equal_every_row_alone(many, name):
    prs, (x, y, lens) = many
    call = _I_CALLS[name]
    whole = call(x, y, lens)
    alone = torch.cat([call(e.to(DEV)[None], r.to(DEV)[None], [lens[b]]) for b, (e, r) in enumerate(prs)])
    whole, alone = whole.cpu(), alone.cpu()
    _gate(f"i_130_rows_{name}", [(f"row {b} T={lens[b]}", whole[b], _I_REFS[name](*prs[b], torch.float64),
                                  _I_REFS[name](*prs[b], torch.float32)) for b in I_GATED])
    assert torch.isfinite(whole).all()  # NaN behind every row's len: never read
    differ = [(b, lens[b], float(whole[b]), float(alone[b])) for b in range(I_ROWS) if whole[b] != alone[b]]
    assert not differ, (name, differ[:8])  # every row = the same row alone, bit for bit


def _median_ms(fn, warmup=3, reps=15):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def test_f_timing_not_gated():
    """16 pairs of 4 s at 16 kHz, inputs already on the device on both sides: evaluate_many (lsd, si-lsd, si-sdr, snr; packing
    and the host read-back of the scores included) against the torch.stft restatement in float32 on the same device (one padded
    batch, the same four scores, the same read-back).  Logged, no ratio asserted."""
    prs = R.signals([64000] * 16, seed=2)
    est, ref = [e.to(DEV) for e, _ in prs], [r.to(DEV) for _, r in prs]
    xe, xr = torch.stack(est), torch.stack(ref)

    def torch_side():
        out = [R.lsd(xe, xr, 400, 160, 1e-7, False, True, torch.float32), R.lsd(xe, xr, 400, 160, 1e-7, True, True, torch.float32),
               R.si_sdr(xe, xr, 100.0, torch.float32), R.snr(xe, xr, 100.0, torch.float32)]
        return [o.tolist() for o in out]

    t_lib = _median_ms(lambda: M.evaluate_many(est, ref, 16000))
    t_torch = _median_ms(torch_side)
    x, y, lens = M.pack_pairs(est, ref)
    t_lsd = _median_ms(lambda: M._lsd_rows(x, y, lens, 400, 160, 1e-7, False, True))
    print(f"f_timing: evaluate_many {t_lib:.3f} ms, torch.stft fp32 {t_torch:.3f} ms, one ou_lsd call {t_lsd:.3f} ms")
    _log("f_timing_16x4s_16k", {"evaluate_many_ms": t_lib, "torch_stft_fp32_ms": t_torch, "ou_lsd_call_ms": t_lsd,
                                "note": "device-resident inputs on both sides, event timing, median of 15 after 3 warm-ups"})
    assert t_lib > 0 and t_torch > 0
