"""CPU: segmented enhance (Universe.enhance_long / ou_enhance_segments) -- the library's window plan, the crossfade weights,
the noise draws, and the CLI's --segment-seconds handling."""
import types

import numpy as np
import pytest
import torch

from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli
from open_universe_amd.universe import Universe

TOT = 256  # total down-sampling factor of the 16 kHz configurations
SEG, OV = 8 * 16000, 16000


def _lengths(tot, seg):
    return sorted({1, 2, tot - 1, tot, tot + 1, 3 * tot, 7 * tot - 1, seg - tot - 1, seg - tot, seg - 1, seg, seg + 1,
                   2 * seg, 5 * seg + 3, 12345678, 2 ** 26 + 7})


@pytest.mark.parametrize("tot,seg,ov", [(TOT, SEG, OV), (TOT, SEG, 0), (TOT, SEG, SEG // 2), (384, 8 * 24000, 24000),
                                        (TOT, 4 * TOT, TOT)])
def test_plan_tiles_the_padded_signal(tot, seg, ov):
    for T_raw in _lengths(tot, seg):
        p = _lib.segment_plan(tot, T_raw, seg, ov)
        T_pad = T_raw + (tot - T_raw % tot)
        assert p["T_pad"] == T_pad
        s, L, c0, c1 = p["starts"], p["lengths"], p["core_begin"], p["core_end"]
        n = len(s)
        assert n >= 1
        assert np.all(L % tot == 0) and np.all(L > 0) and np.all(L <= max(seg - seg % tot, T_pad if n == 1 else 0))
        assert np.all(s % tot == 0) and s[0] == 0 and np.all(s >= 0) and np.all(s + L <= T_pad)
        assert s[-1] + L[-1] == T_pad  # the windows cover [0, T_pad)
        assert np.all(np.diff(s) > 0) and np.all(s[1:] <= s[:-1] + L[:-1])  # no gap between windows
        assert c0[0] == 0 and c1[-1] == T_pad and np.array_equal(c0[1:], c1[:-1]) and np.all(c1 > c0)  # cores tile
        assert np.all(c0 >= s) and np.all(c1 <= s + L)  # a window's core lies inside it
        if T_pad <= seg - seg % tot:
            assert n == 1 and L[0] == T_pad
        else:
            assert np.all(L == seg - seg % tot) and p["overlap"] == ov - ov % tot


@pytest.mark.parametrize("T_raw", [1, TOT, 5 * TOT, SEG - TOT, SEG + 1, 3 * SEG + 77, 10 * SEG])
@pytest.mark.parametrize("ov", [0, TOT, OV, SEG // 2])
def test_crossfade_weights_sum_to_one(T_raw, ov):
    p = _lib.segment_plan(TOT, T_raw, SEG, ov)
    tot = np.zeros(p["T_pad"], dtype=np.float32)
    for k in range(len(p["starts"])):
        w = _lib.segment_weights(p, k)
        assert np.all(w >= 0) and np.all(w <= 1)
        s = p["starts"][k]
        tot[s:s + len(w)] += w
        # a window has weight >= 1/2 exactly on its core
        u = np.arange(s, s + len(w))
        core = (u >= p["core_begin"][k]) & (u < p["core_end"][k])
        assert np.all(w[core] >= 0.5) and np.all(w[~core] <= 0.5)
    assert np.array_equal(tot, np.ones_like(tot))  # exactly 1 in fp32 at every sample


def test_plan_of_a_very_long_signal_and_refusals():
    p = _lib.segment_plan(TOT, 2 ** 26 + 7, SEG, OV)
    n = len(p["starts"])
    assert p["overlap"] == OV - OV % TOT
    assert n == -(-(p["T_pad"] - SEG) // (SEG - p["overlap"])) + 1
    for bad in ((TOT, 100, TOT - 1, 0), (TOT, 100, SEG, SEG // 2 + TOT), (TOT, 0, SEG, OV),
                (TOT, 100, SEG, -TOT)):
        with pytest.raises(ValueError):
            _lib.segment_plan(*bad)


def test_noise_draws_advance_the_generator_like_enhance():
    stub = types.SimpleNamespace(diff_kwargs=types.SimpleNamespace(n_steps=5), tot_ds=TOT, device=torch.device("cpu"))
    g1 = torch.Generator().manual_seed(3)
    g2 = torch.Generator().manual_seed(3)
    noise = Universe.draw_noise_like_enhance(stub, g1, 2, 1000)
    T = 1000 + (TOT - 1000 % TOT)
    assert tuple(noise.shape) == (5, 2, T)
    # the values of enhance's draws, step by step ...
    for k in range(5):
        assert torch.equal(noise[k], torch.randn((2, 1, T), generator=g2)[:, 0])
    # ... and the generator state of advance_generator_like_enhance
    g3 = torch.Generator().manual_seed(3)
    Universe.advance_generator_like_enhance(stub, g3, 2, 1000)
    assert torch.equal(g1.get_state(), g3.get_state())


class _SegModel:
    fs = 16000
    device = "cpu"
    class _KW(dict):
        pass

    diff_kwargs = _KW(n_steps=8, epsilon=1.3)
    LIMIT = 40000  # samples: stands in for the length guard of ou_enhance

    def __init__(self):
        self.calls = []

    def enhance(self, mix, n_steps: int = None, epsilon: float = None, rng: torch.Generator = None,
                keep_rms: bool = False) -> torch.Tensor:
        if mix.shape[-1] > self.LIMIT:
            raise ValueError("input too long for one pass: ...; ou_enhance_segments enhances it in windows")
        self.calls.append(("enhance", tuple(mix.shape), n_steps))
        return 0.5 * mix

    def enhance_long(self, mix, segment_s=8.0, overlap_s=1.0, max_batch=32, rng=None, n_steps=None, epsilon=None,
                     keep_rms=False):
        self.calls.append(("long", tuple(mix.shape), segment_s, overlap_s, n_steps))
        return 0.25 * mix


def test_cli_segment_flags(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    A.save(src / "a_short.wav", torch.full((1, 16000), 0.25), 16000)   # 1 s
    A.save(src / "b_long.wav", torch.full((2, 48000), 0.25), 16000)    # 3 s
    m = _SegModel()
    cli.main([str(src), str(tmp_path / "o"), "--segment-seconds", "2", "--segment-overlap", "0.5", "--n_steps", "4"], model=m)
    assert m.calls == [("enhance", (1, 16000), 4), ("long", (2, 48000), 2.0, 0.5, 4)]
    y, _ = A.load(tmp_path / "o" / "b_long.wav")
    assert torch.allclose(y, torch.full((2, 48000), 0.0625))
    # off by default: every file takes enhance, and a file past the guard names the flag
    m = _SegModel()
    with pytest.raises(ValueError, match="--segment-seconds"):
        cli.main([str(src), str(tmp_path / "o2")], model=m)
    assert m.calls == [("enhance", (1, 16000), 8)]
    m = _SegModel()
    m.LIMIT = 10 ** 9
    cli.main([str(src), str(tmp_path / "o3")], model=m)
    assert [c[0] for c in m.calls] == ["enhance", "enhance"]


@pytest.mark.parametrize("extra", [["--pad-batch", "--batch-size", "2"], ["--batch-size", "2"], ["--in-flight", "2"],
                                   ["--segment-overlap", "1.5"], ["--segment-overlap", "-1"]])
def test_cli_segment_refusals(tmp_path, extra):
    src = tmp_path / "a.wav"
    A.save(src, torch.zeros(1, 1000), 16000)
    m = _SegModel()
    with pytest.raises(ValueError):
        cli.main([str(src), str(tmp_path / "o.wav"), "--segment-seconds", "2"] + extra, model=m)
    assert m.calls == []


def test_cli_overlap_needs_segment(tmp_path):
    src = tmp_path / "a.wav"
    A.save(src, torch.zeros(1, 1000), 16000)
    with pytest.raises(ValueError, match="--segment-seconds"):
        cli.main([str(src), str(tmp_path / "o.wav"), "--segment-overlap", "1"], model=_SegModel())
