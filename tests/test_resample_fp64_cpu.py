"""CPU: the reference and the bounds of resample_fp64.py can be met, shown before anything runs on a device.  `restate` is a
numpy restatement of the kernels' order from the library's own table -- first[p], taps ascending, one rounding per tap (product
and add in float64, then rounded to fp32) -- and has to pass the very checks the library gets in test_gpu_resample_fp64.py: the
chain bound over the noise rows with nothing excluded, and the impulse rows bit for bit.

The same restatement with ONE seam error -- the last live tap dropped for the last output of tile 0, what a staged span one
sample short does -- has to be flagged by both checks.  Measured here on 44 100 -> 16 000 (that tap: -8.0e-6, 2.2e-5 of the
peak), on the two rows of 2 050 outputs: the intact restatement scores 139.7 and 139.4 dB against float64, the broken one 131.4
and 138.6 dB, beside the gate of test_gpu_resample.py at 6 dB under the fp32 conv's 139.7 and 139.5 dB: that gate passes the
second row and misses the first by 2.3 dB, and the same error in a row of 4 s (64 000 outputs) sits 15 dB further down, under
the rounding floor.  The chain bound flags the first row's sample at err / bound 2.4 whatever the row's length (in the second
row the lost product is smaller than the bound: the data hides it); the impulse row flags it whatever the data.  On
192 000 -> 8 000 the same tap is 3.1e-9: the dB figures do not move (130.3, 130.4), the chain bound passes, and the impulse row
alone flags it."""
import numpy as np
import pytest

import resample_fp64 as F
import resample_reference as R

PAIRS = R.PAIRS + [(192000, 8000), (1000000, 16000)]  # = the pairs of test_gpu_resample.py's accuracy test
EDGE = 1  # outputs at the edge of tile 0 that lose their last live tap


def restate(P, x, drop=None):
    """The kernels' arithmetic on the row x.  drop: outputs whose last live tap is left out (the broken restatement)."""
    xv = P.windows(np.asarray(x, dtype=np.float32))
    p = np.arange(xv.shape[0]) % P.new
    if drop is not None:
        drop = np.asarray([j for j in drop if j < xv.shape[0]], dtype=np.int64)
        xv[drop, P.last_live[p[drop]]] = 0
    acc = np.zeros(xv.shape[0], dtype=np.float32)
    for t in range(P.taps):
        acc = (P.coef[t, p].astype(np.float64) * xv[:, t].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def _run(P, case, drop=None):
    y = np.zeros((len(case["rows"]), case["cols"]), dtype=np.float32)
    for b, r in enumerate(case["rows"]):
        y[b, :case["out_lens"][b]] = restate(P, r, drop)
    return y


@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_paths_tiles_and_table_against_the_dense_kernel(built_lib, fs_in, fs_out):
    P = F.pair(fs_in, fs_out)
    assert P.tile == F.PATHS.get((fs_in, fs_out), F.DEFAULT_PATH)[1]
    # the table over every phase's support against the dense kernel of the reference: equal, or one fp32 ulp apart (the last
    # float64 bit of libm's and numpy's sin / cos before the one rounding), which the two spare u of the chain bound cover
    ph = np.arange(P.new) if P.new <= 4096 else np.arange(0, P.new, 7)
    dense = R.dense_rows(fs_in, fs_out, ph)
    idx = P.first[ph].astype(np.int64)[:, None] + P.width + np.arange(P.taps)[None, :]
    want = np.where(idx < dense.shape[1], dense[np.arange(len(ph))[:, None], np.minimum(idx, dense.shape[1] - 1)], 0.0)
    got = P.coef[:, ph].T.astype(np.float64)
    live = got != 0
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - want)[live] <= ulp[live]).all() and (np.abs(want[~live]) < 1e-30).all()
    print(f"table {fs_in}->{fs_out}: {int((got != want)[live].sum())} of {int(live.sum())} live coefficients one ulp from numpy's")


@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_restatement_meets_the_chain_bound_with_nothing_excluded(built_lib, fs_in, fs_out):
    P, case = F.pair(fs_in, fs_out), F.noise_case(fs_in, fs_out)
    rep = F.check_noise(f"restatement.noise.{fs_in}_{fs_out}", case, _run(P, case))
    print(rep)
    assert rep.excluded == 0 and rep.ok(), str(rep)
    assert rep.checked == len(case["rows"]) * case["cols"]


@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_comb_meets_every_phase_and_tap_and_restatement_is_exact(built_lib, fs_in, fs_out):
    P, case = F.pair(fs_in, fs_out), F.impulse_case(fs_in, fs_out)
    assert case["hits"].shape == (P.new, P.taps) and case["hits"].all(), int((~case["hits"]).sum())
    comb = case["rows"][0]
    assert comb[0] != 0 and comb[-1] != 0  # input sample 0 and sample len - 1
    assert sorted(j for j, _, _ in case["seams"]) == [P.tile - 1, P.tile - 1, P.tile, P.tile]
    assert all(case["out_lens"][1 + i] > P.tile for i in range(4))
    rep = F.check_impulses(f"restatement.impulse.{fs_in}_{fs_out}", case, _run(P, case))
    print(rep)
    assert rep.excluded == 0 and rep.ok(), str(rep)
    assert int((case["want"] != 0).sum()) > 0


def _broken(fs_in, fs_out):
    """The noise and impulse reports of the restatement with the last live tap of output tile - 1 dropped, and per noise row
    that reaches past tile 0 its dB against float64 (intact, broken)."""
    P, case, icase = F.pair(fs_in, fs_out), F.noise_case(fs_in, fs_out), F.impulse_case(fs_in, fs_out)
    drop = range(P.tile - EDGE, P.tile)
    good, bad = _run(P, case), _run(P, case, drop)
    rep = F.check_noise(f"broken.noise.{fs_in}_{fs_out}", case, bad)
    irep = F.check_impulses(f"broken.impulse.{fs_in}_{fs_out}", icase, _run(P, icase, drop))
    print(rep)
    print(irep)
    db = {}
    for b, J in enumerate(case["out_lens"]):
        if J > P.tile + P.new:
            ref = case["ref"][b, :J].numpy()
            db[b] = (R.snr_db(ref, good[b, :J]), R.snr_db(ref, bad[b, :J]))
            print(f"{fs_in}->{fs_out} row {b} ({J} outputs): intact {db[b][0]:.1f} dB, one seam tap dropped {db[b][1]:.1f} dB")
    return P, case, rep, icase, irep, db


def test_a_dropped_seam_tap_is_flagged_by_the_bound_and_by_the_impulse_rows(built_lib):
    P, case, rep, icase, irep, db = _broken(44100, 16000)
    assert rep.excluded == 0 and not rep.ok()
    flagged = rep.bad.reshape(len(case["rows"]), -1)
    assert flagged[:, P.tile - 1].any() and int(flagged.sum()) == int(flagged[:, P.tile - 1].sum())  # that sample, nothing else
    assert len(db) == 2 and all(bad < good for good, bad in db.values())
    # the row of the impulse under the last live tap of the last output of tile 0: that sample, nothing else
    iflag = irep.bad.reshape(len(icase["rows"]), -1)
    assert not irep.ok() and iflag[2, P.tile - 1] and int(iflag.sum()) == 1 + int(iflag[0].sum())


def test_a_dropped_tap_under_the_rounding_is_flagged_by_the_impulse_rows_alone(built_lib):
    """192 000 -> 8 000: the last live tap of output tile - 1 is 3.1e-9 (7.5e-8 of the peak): no check on noise can tell its
    loss from rounding -- the chain bound passes, the dB figures do not move -- and the impulse rows flag it."""
    P, case, rep, icase, irep, db = _broken(192000, 8000)
    assert abs(float(P.coef[P.last_live[(P.tile - 1) % P.new], (P.tile - 1) % P.new])) < 1e-8
    assert rep.ok() and all(abs(bad - good) < 0.05 for good, bad in db.values())
    assert not irep.ok() and irep.bad.reshape(len(icase["rows"]), -1)[2, P.tile - 1]
