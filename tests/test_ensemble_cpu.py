"""CPU: ensembles inside the library (ou_enhance_ensemble / ou_ensemble_reduce, ABI 7) -- the binding's declarations, the torch
restatement of the reduce kernels (tests/ensemble_ref.py) against torch.mean / torch.median / universe.signal_median and a
sort-based statement of the reference's signal median, and the CLI's --ensemble handling with --batch-size."""
import os
import re

import pytest
import torch

import ensemble_ref as R
from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli
from open_universe_amd.universe import signal_median

E_LIST = [1, 2, 3, 4, 5, 8, 31, 32]


def test_binding_declares_the_ensemble_entry_points(built_lib):
    assert _lib.OU_ABI_VERSION == 7
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ouniverse.h")).read()
    assert re.search(r"#define OU_ABI_VERSION 7\b", hdr) and re.search(r"#define OU_MAX_ENSEMBLE 32\b", hdr)
    assert _lib.OU_MAX_ENSEMBLE == 32
    assert (_lib.OU_ENS_MEAN, _lib.OU_ENS_MEDIAN, _lib.OU_ENS_SIGNAL_MEDIAN) == (0, 1, 2)
    for name in ("ou_ensemble_workspace_bytes", "ou_enhance_ensemble", "ou_ensemble_reduce"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(built_lib, name)
        assert getattr(built_lib, name).argtypes is not None
    assert "ens_share" in _lib.option_names() and _lib.option_defaults()["ens_share"] == 1.0
    # pure host function: histogram [B][E] + picks [B], int32
    assert built_lib.ou_ensemble_reduce_scratch_bytes(4, 3) >= (3 * 4 + 3) * 4


def sorted_signal_median(x):
    """The reference's signal median (utils/stats.py:22-66) stated with a sort: order the members of every sample ascending
    (stable: ties keep member order), find the POSITION in that order of the member whose index is nearest n / 2 (the first such
    position), count per input how often every position occurs, return the member numbered like the most frequent position."""
    n, B, S = x.shape
    order = x.sort(dim=0, stable=True).indices  # order[p, b, s] = member at position p
    dist = (order.double() - n / 2).abs()
    best = dist.min(dim=0).values
    pos = torch.full((B, S), n, dtype=torch.int64)
    for p in range(n - 1, -1, -1):  # descending: the first position with the smallest distance is written last
        pos = torch.where(dist[p] == best, torch.full_like(pos, p), pos)
    out = []
    for b in range(B):
        counts = torch.bincount(pos[b], minlength=n)
        first = int((counts == counts.max()).nonzero()[0])
        out.append(x[first, b])
    return torch.stack(out)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("E", E_LIST)
def test_reduce_restatement_agrees_with_torch_and_the_reference_semantics(E, ties):
    B, S = 3, 257
    x = R.draw_members(E, B, S, seed=100 + E, ties=ties)
    # mean: within the bound of a sequential fp32 sum of the float64 mean, and torch.mean inside the same bound
    m, _, _ = R.reduce_ref(x, "mean")
    m64 = x.double().mean(dim=0)
    assert ((m.double() - m64).abs() <= R.mean_bound(x, m64)).all()
    assert ((x.mean(dim=0).double() - m64).abs() <= R.mean_bound(x, m64)).all()
    # median: torch.median's lower median, bit for bit
    med, _, _ = R.reduce_ref(x, "median")
    assert torch.equal(med, x.median(dim=0).values)
    # signal median: the project's rank-counting form and the sort-based statement, bit for bit
    sm, pick, hist = R.reduce_ref(x, "signal_median")
    assert torch.equal(sm, signal_median(x))
    assert torch.equal(sm, sorted_signal_median(x))
    assert int(hist.sum()) == B * S and torch.equal(sm, x[pick, torch.arange(B)])
    # ranks are a permutation along the members
    assert torch.equal(R.ranks(x).sort(dim=0).values, torch.arange(E)[:, None, None].expand(E, B, S))


def test_reduce_restatement_ragged_lengths():
    E, B, S = 5, 3, 100
    x = R.draw_members(E, B, S, seed=7, ties=True)
    lens = [100, 37, 1]
    for stat in R.STATS:
        out, pick, _ = R.reduce_ref(x, stat, lens)
        for b, n in enumerate(lens):
            assert not out[b, n:].any()
            alone, _, _ = R.reduce_ref(x[:, b:b + 1, :n], stat)  # a row's own samples only
            assert torch.equal(out[b, :n], alone[0])


class _EnsModel:
    fs = 16000
    device = "cpu"
    tot_ds = 1

    class _KW(dict):
        pass

    diff_kwargs = _KW(n_steps=8, epsilon=1.3)

    def __init__(self):
        self.calls = []

    def enhance(self, mix, n_steps: int = None, epsilon: float = None, rng: torch.Generator = None, keep_rms: bool = False,
                ensemble: int = None, ensemble_stat: str = "median") -> torch.Tensor:
        self.calls.append(("enhance", tuple(mix.shape), ensemble, ensemble_stat))
        return 0.5 * mix

    def enhance_many(self, sigs, rngs, pad_batch=False, **kw):
        self.calls.append(("many", [tuple(s.shape) for s in sigs], kw.get("ensemble"), kw.get("ensemble_stat"), pad_batch))
        return [0.25 * s for s in sigs]

    def enhance_long(self, mix, **kw):
        self.calls.append(("long",))
        return mix

    def advance_generator_like_enhance(self, rng, channels, length, **kw):
        self.calls.append(("advance", channels, length))


def _three_files(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    A.save(src / "a.wav", torch.full((1, 1200), 0.25), 16000)
    A.save(src / "b.wav", torch.full((2, 800), 0.25), 16000)
    A.save(src / "c.wav", torch.full((1, 1000), 0.25), 16000)
    return src


def test_cli_ensemble_with_batch_size_goes_through_enhance_many(tmp_path):
    """--ensemble E --batch-size K: every group is ONE enhance_many(ensemble=E) call (refused before ABI 7)."""
    src = _three_files(tmp_path)
    m = _EnsModel()
    cli.main([str(src), str(tmp_path / "o"), "--ensemble", "3", "--ensemble_stat", "signal_median", "--batch-size", "2"], model=m)
    many = [c for c in m.calls if c[0] == "many"]
    assert len(many) == 2 and all(c[2] == 3 and c[3] == "signal_median" and c[4] is False for c in many)
    assert sorted(s for c in many for s in c[1]) == [(1, 1000), (1, 1200), (2, 800)]
    assert not [c for c in m.calls if c[0] == "enhance"]
    # the shared generator is advanced by the E * channels member rows of every file, in processing order
    assert [c for c in m.calls if c[0] == "advance"] == [("advance", 3, 1200), ("advance", 6, 800), ("advance", 3, 1000)]
    y, _ = A.load(tmp_path / "o" / "b.wav")
    assert torch.allclose(y, torch.full((2, 800), 0.0625))
    # with the counter-based noise too
    m = _EnsModel()
    cli.main([str(src), str(tmp_path / "o2"), "--ensemble", "2", "--batch-size", "4", "--noise", "counter"], model=m)
    assert [c[2] for c in m.calls if c[0] == "many"] == [2]
    # without --ensemble the batched path hands enhance_many no ensemble argument
    m = _EnsModel()
    cli.main([str(src), str(tmp_path / "o3"), "--batch-size", "2"], model=m)
    assert all(c[2] is None and c[3] is None for c in m.calls if c[0] == "many")
    # the serial loop keeps calling enhance
    m = _EnsModel()
    cli.main([str(src), str(tmp_path / "o4"), "--ensemble", "3"], model=m)
    assert [c[0] for c in m.calls] == ["enhance"] * 3 and all(c[2] == 3 for c in m.calls)


@pytest.mark.parametrize("extra", [["--segment-seconds", "2"], ["--pad-batch", "--batch-size", "2"], ["--pad-batch"]])
def test_cli_ensemble_refusals(tmp_path, extra):
    src = _three_files(tmp_path)
    m = _EnsModel()
    with pytest.raises(ValueError):
        cli.main([str(src), str(tmp_path / "o"), "--ensemble", "3"] + extra, model=m)
    assert m.calls == []
