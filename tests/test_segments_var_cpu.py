"""CPU: segmented enhance of rows with lengths of their own (Universe.enhance_long_many / ou_enhance_segments_var) -- the
library's window groups (ou_segment_groups), the refusals that are decided before any HIP call, and the CLI's --segment-files."""
import ctypes

import numpy as np
import pytest
import torch

from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli

TOT = 256
S, O, MAX_BATCH = 16 * TOT, 2 * TOT, 4
LENGTHS = [41 * TOT + 7, 9 * TOT, 57, 16 * TOT - 1, 16 * TOT, 70 * TOT + 3]


def _ceil(a, b):
    return -(-a // b)


def _even(n, max_batch):
    """batch size of a class of n entries: spread evenly over ceil(n / max_batch) groups"""
    return _ceil(n, _ceil(n, max_batch)) if n else 0


def test_groups_of_the_six_lengths(built_lib):
    g = _lib.segment_groups(TOT, LENGTHS, S, O, MAX_BATCH)
    plans = [_lib.segment_plan(TOT, t, S, O) for t in LENGTHS]
    n_win = [len(p["starts"]) for p in plans]
    assert n_win == [3, 1, 1, 1, 2, 5]  # 16 tot - 1 pads to S: one window; 16 tot pads to 17 tot: two, the second shifted
    assert plans[4]["starts"].tolist() == [0, TOT]
    # every (row, window) of the per-row plans exactly once, with the plan's length
    pairs = list(zip(g["row"].tolist(), g["window"].tolist()))
    assert sorted(pairs) == sorted((c, k) for c in range(len(LENGTHS)) for k in range(n_win[c]))
    for c, k, ln in zip(g["row"], g["window"], g["length"]):
        assert ln == plans[c]["lengths"][k]
    # class FULL first, row-major, then class SHORT in input order
    n_full = sum(n for n in n_win if n > 1)
    assert pairs[:n_full] == [(c, k) for c in (0, 4, 5) for k in range(n_win[c])]
    assert np.all(g["length"][:n_full] == S)
    assert pairs[n_full:] == [(1, 0), (2, 0), (3, 0)]
    assert g["length"][n_full:].tolist() == [10 * TOT, TOT, S]
    # one batch size, groups never mix classes, ragged exactly where the lengths of a group differ
    batch = g["batch"]
    assert batch == max(_even(n_full, MAX_BATCH), _even(3, MAX_BATCH)) == 4 and batch <= MAX_BATCH
    assert g["length_max"] == S
    first = g["group_first"].tolist()
    assert first == [0, 4, 8, 10]
    assert len(first) == _ceil(n_full, batch) + _ceil(3, batch)
    ends = first[1:] + [len(pairs)]
    for f, e, ragged in zip(first, ends, g["group_ragged"]):
        e = min(e, f + batch, n_full if f < n_full else len(pairs))
        assert 1 <= e - f <= batch
        assert (f < n_full) == (e <= n_full)  # one class per group
        assert bool(ragged) == (len(set(g["length"][f:e].tolist())) > 1)
    assert g["group_ragged"].tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("C,T_raw,max_batch", [(3, 41 * TOT + 7, 4), (3, 9 * TOT, 4), (1, 70 * TOT + 3, 4), (5, 57, 2),
                                               (2, 16 * TOT, 32)])
def test_equal_lengths_give_the_counts_of_the_single_length_call(built_lib, C, T_raw, max_batch):
    """batch = ceil(E / ceil(E / max_batch)) for E = C * n_win entries in row-major order (ou_enhance_segments' rule); the half
    that compares with ou_segments_workspace_bytes needs a handle and is in the GPU file."""
    p = _lib.segment_plan(TOT, T_raw, S, O)
    n_win = len(p["starts"])
    g = _lib.segment_groups(TOT, [T_raw] * C, S, O, max_batch)
    E = C * n_win
    assert len(g["row"]) == E
    assert g["batch"] == _even(E, max_batch)
    assert g["length_max"] == p["lengths"][0]
    assert list(zip(g["row"].tolist(), g["window"].tolist())) == [(c, k) for c in range(C) for k in range(n_win)]
    assert g["group_first"].tolist() == list(range(0, E, g["batch"]))
    assert not g["group_ragged"].any()


def test_counts_only_and_capacity(built_lib):
    tr = (ctypes.c_int64 * 6)(*LENGTHS)
    ne, ng, b, ln = (ctypes.c_int32() for _ in range(4))
    rc = built_lib.ou_segment_groups(TOT, 6, tr, S, O, MAX_BATCH, 0, None, None, None, None, None, ctypes.byref(ne),
                                     ctypes.byref(ng), ctypes.byref(b), ctypes.byref(ln))
    assert rc == 0 and (ne.value, ng.value, b.value, ln.value) == (13, 4, 4, S)
    row = (ctypes.c_int32 * 13)()
    rc = built_lib.ou_segment_groups(TOT, 6, tr, S, O, MAX_BATCH, 12, row, None, None, None, None, None, None, None, None)
    assert rc == _lib.OU_EINVAL


def test_group_refusals(built_lib):
    for lens, mb in (([100, 0], 4), ([100, -3], 4), ([100, 200], 0), ([], 4)):
        with pytest.raises(ValueError):
            _lib.segment_groups(TOT, lens, S, O, mb)
    with pytest.raises(ValueError):
        _lib.segment_groups(TOT, [100], TOT - 1, 0, 4)  # (the plan's own refusals)
    with pytest.raises(ValueError):
        _lib.segment_groups(TOT, [100], S, S, 4)


@pytest.mark.parametrize("t_raw,T_raw_max,max_batch,msg", [([100, 0], 100, 4, b"1 <= t_raw[c] <= T_raw_max"),
                                                           ([100, 200], 100, 4, b"1 <= t_raw[c] <= T_raw_max"),
                                                           ([100, 50], 200, 4, b"longest row"),
                                                           ([100, 50], 100, 0, b"max_batch")])
def test_enhance_refusals_come_before_any_hip_call(built_lib, t_raw, T_raw_max, max_batch, msg):
    """t_raw of 0, t_raw > T_raw_max, max != T_raw_max, max_batch < 1: the lengths are judged first, before the handle or any
    buffer is looked at -- so the refusal (and its message) can be had without a device: NULL handle, pointers to nowhere."""
    C = len(t_raw)
    tr = (ctypes.c_int64 * C)(*t_raw)
    dummy = ctypes.c_void_p(256)
    rc = built_lib.ou_enhance_segments_var(None, dummy, dummy, dummy, C, T_raw_max, tr, S, O, max_batch, 3, 1.0, None, -1, 0, dummy,
                                           ctypes.c_size_t(1 << 20), None)
    assert rc == _lib.OU_EINVAL
    assert msg in built_lib.ou_last_error(None)


class _Model:
    fs = 16000
    device = "cpu"

    class _KW(dict):
        pass

    diff_kwargs = _KW(n_steps=8, epsilon=1.3)

    def __init__(self):
        self.calls = []

    def enhance(self, mix, n_steps: int = None, epsilon: float = None, rng: torch.Generator = None, keep_rms: bool = False,
                ensemble: int = None, target: str = None, warm_start: int = None, use_aux_signal: bool = False) -> torch.Tensor:
        self.calls.append(("enhance", tuple(mix.shape), n_steps))
        return 0.5 * mix

    def enhance_long(self, mix, segment_s=8.0, overlap_s=1.0, max_batch=32, rng=None, n_steps=None, epsilon=None,
                     keep_rms=False):
        self.calls.append(("long", tuple(mix.shape), segment_s, overlap_s, n_steps))
        return 0.25 * mix

    def enhance_long_many(self, signals, rngs=None, segment_s=8.0, overlap_s=1.0, max_batch=32, n_steps=None, epsilon=None,
                          keep_rms=False):
        self.calls.append(("many", [tuple(s.shape) for s in signals], segment_s, overlap_s, n_steps,
                           len(rngs) if isinstance(rngs, list) else type(rngs).__name__))
        return [0.125 * s for s in signals]


def _three_files(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    A.save(src / "a_short.wav", torch.full((1, 16000), 0.25), 16000)  # 1 s
    A.save(src / "b_long.wav", torch.full((2, 48000), 0.25), 16000)   # 3 s, two channels
    A.save(src / "c_mid.wav", torch.full((1, 33000), 0.25), 16000)
    return src


def test_cli_segment_files_groups_the_sorted_list(tmp_path):
    src = _three_files(tmp_path)
    m = _Model()
    cli.main([str(src), str(tmp_path / "o"), "--segment-seconds", "2", "--segment-overlap", "0.5", "--segment-files", "2",
              "--n_steps", "4"], model=m)
    assert m.calls == [("many", [(1, 16000), (2, 48000)], 2.0, 0.5, 4, "Generator"), ("many", [(1, 33000)], 2.0, 0.5, 4, "Generator")]
    for name, shape in (("a_short.wav", (1, 16000)), ("b_long.wav", (2, 48000)), ("c_mid.wav", (1, 33000))):
        y, _ = A.load(tmp_path / "o" / name)
        assert torch.allclose(y, torch.full(shape, 0.25 * 0.125))
    # one CounterNoise source per file (file k of the sorted list = stream k), one generator per file with --per-file-seed
    for extra in (["--noise", "counter"], ["--per-file-seed"]):
        m = _Model()
        cli.main([str(src), str(tmp_path / "o2"), "--segment-seconds", "2", "--segment-files", "3"] + extra, model=m)
        assert m.calls == [("many", [(1, 16000), (2, 48000), (1, 33000)], 2.0, 1.0, 8, 3)]
    # the default is today's loop: one call per file
    m = _Model()
    cli.main([str(src), str(tmp_path / "o3"), "--segment-seconds", "2"], model=m)
    assert [c[0] for c in m.calls] == ["enhance", "long", "long"]


def test_cli_segment_files_needs_segment_seconds(tmp_path):
    src = _three_files(tmp_path)
    m = _Model()
    with pytest.raises(ValueError, match="--segment-seconds"):
        cli.main([str(src), str(tmp_path / "o"), "--segment-files", "2"], model=m)
    with pytest.raises(ValueError, match="--segment-files"):
        cli.main([str(src), str(tmp_path / "o"), "--segment-seconds", "2", "--segment-files", "0"], model=m)
    assert m.calls == []


@pytest.mark.parametrize("extra", [["--batch-size", "2"], ["--in-flight", "2"], ["--pad-batch"], ["--ensemble", "2"],
                                   ["--target", "t.wav"], ["--warm_start", "1"], ["--use_aux_signal", "1"]])
def test_cli_segment_files_refusals(tmp_path, extra):
    src = _three_files(tmp_path)
    m = _Model()
    with pytest.raises(ValueError):
        cli.main([str(src), str(tmp_path / "o"), "--segment-seconds", "2", "--segment-files", "2"] + extra, model=m)
    assert m.calls == []
