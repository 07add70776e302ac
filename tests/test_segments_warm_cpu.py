"""CPU: warm start and the aux-signal exit in the segmented calls -- the ABI is unchanged, the CLI forwards the
options of the one-file-per-call form to `enhance_long` (and to `enhance` for a short file), the forms that keep refusing them
call nothing, and the long methods draw the planes `advance_generator_like_enhance` counts."""
import inspect
import os
import re
import types

import pytest
import torch

from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli
from open_universe_amd.universe import Universe

TOT = 256
CALLS = {  # name: arguments of the header's declaration
    "ou_enhance_segments": 17,
    "ou_enhance_segments_var": 18,
    "ou_enhance_segments_ensemble": 20,
    "ou_enhance_segments_var_ensemble": 21,
}


def test_the_abi_of_the_four_calls_is_unchanged(built_lib):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ouniverse.h")).read()
    assert re.search(r"#define OU_ABI_VERSION 7\b", hdr) and _lib.OU_ABI_VERSION == 7
    for name, n in CALLS.items():
        decl = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S).group(1)
        args = [a.strip() for a in decl.split(",")]
        assert len(args) == n == len(getattr(built_lib, name).argtypes), name
        assert args[-5:] == ["int32_t warm_start", "uint32_t flags", "void* ws", "size_t ws_bytes", "ou_stream_t stream"], name


class _Model:
    fs = 16000
    device = "cpu"

    class _KW(dict):
        pass

    diff_kwargs = _KW(n_steps=8, epsilon=1.3)

    def __init__(self):
        self.calls = []

    def enhance(self, mix, n_steps: int = None, epsilon: float = None, rng: torch.Generator = None, keep_rms: bool = False,
                use_aux_signal: bool = False, ensemble: int = None, ensemble_stat: str = "median",
                warm_start: int = None) -> torch.Tensor:
        self.calls.append(("enhance", tuple(mix.shape), warm_start, bool(use_aux_signal)))
        return 0.5 * mix

    def enhance_long(self, mix, **kw):
        self.calls.append(("long", tuple(mix.shape), kw))
        return 0.25 * mix

    def enhance_long_ensemble(self, mix, ensemble, ensemble_stat="median", **kw):
        self.calls.append(("long_ensemble", tuple(mix.shape), kw))
        return 0.125 * mix

    def enhance_long_many(self, sigs, rngs=None, **kw):
        self.calls.append(("long_many", kw))
        return list(sigs)


def _two_files(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    A.save(src / "a_short.wav", torch.full((1, 16000), 0.25), 16000)   # 1 s: one `enhance` call
    A.save(src / "b_long.wav", torch.full((2, 48000), 0.25), 16000)    # 3 s: `enhance_long`
    return src


def test_cli_forwards_warm_start(tmp_path):
    src = _two_files(tmp_path)
    m = _Model()
    cli.main([str(src), str(tmp_path / "o"), "--segment-seconds", "2", "--segment-overlap", "0.5", "--warm_start", "1"], model=m)
    assert [c[0] for c in m.calls] == ["enhance", "long"]
    assert m.calls[0] == ("enhance", (1, 16000), 1, False)
    kw = m.calls[1][2]
    assert kw["warm_start"] == 1 and "use_aux_signal" not in kw
    assert kw["segment_s"] == 2.0 and kw["overlap_s"] == 0.5 and isinstance(kw["rng"], torch.Generator)


def test_cli_forwards_use_aux_signal(tmp_path):
    src = _two_files(tmp_path)
    m = _Model()
    cli.main([str(src), str(tmp_path / "o"), "--segment-seconds", "2", "--use_aux_signal", "1"], model=m)
    assert [c[0] for c in m.calls] == ["enhance", "long"]
    assert m.calls[0] == ("enhance", (1, 16000), None, True)
    kw = m.calls[1][2]
    assert kw["use_aux_signal"] is True and "warm_start" not in kw


def test_cli_without_the_options_passes_neither(tmp_path):
    src = _two_files(tmp_path)
    m = _Model()
    cli.main([str(src), str(tmp_path / "o"), "--segment-seconds", "2"], model=m)
    assert m.calls[0] == ("enhance", (1, 16000), None, False)
    assert "warm_start" not in m.calls[1][2] and "use_aux_signal" not in m.calls[1][2]


@pytest.mark.parametrize("extra", [
    ["--segment-ensemble", "3", "--warm_start", "1"],
    ["--segment-ensemble", "3", "--use_aux_signal", "1"],
    ["--segment-files", "2", "--warm_start", "1"],
    ["--segment-files", "2", "--use_aux_signal", "1"],
])
def test_cli_forms_that_refuse_the_options_call_nothing(tmp_path, extra):
    src = _two_files(tmp_path)
    m = _Model()
    with pytest.raises(ValueError, match="warm_start|use_aux_signal"):
        cli.main([str(src), str(tmp_path / "o"), "--segment-seconds", "2"] + extra, model=m)
    assert m.calls == []
    assert "--warm_start" in cli.build_parser().format_help()  # the help of --segment-seconds says which forms take them


def test_the_long_methods_name_the_options_and_the_ensembles_do_not():
    for name in ("enhance_long", "enhance_long_many"):
        p = inspect.signature(getattr(Universe, name)).parameters
        assert p["warm_start"].default is None and p["use_aux_signal"].default is False, name
    for name in ("enhance_long_ensemble", "enhance_long_many_ensemble"):
        p = inspect.signature(getattr(Universe, name)).parameters
        assert "warm_start" not in p and "use_aux_signal" not in p, name
    with pytest.raises(ValueError, match="warm_start"):  # (what reaches **other is still refused)
        Universe._refuse_long_options("enhance_long_many_ensemble", {"warm_start": 1})


class _Drawer:
    """Universe.enhance_long / enhance_long_many on the CPU up to the library call: the draws are real, the call is recorded."""
    diff_kwargs = types.SimpleNamespace(n_steps=5, epsilon=1.3)
    tot_ds, fs, device = TOT, 16000, torch.device("cpu")
    _long_planes = staticmethod(Universe._long_planes)
    _refuse_long_options = staticmethod(Universe._refuse_long_options)
    _counter_plan = staticmethod(Universe._counter_plan)
    draw_noise_like_enhance = Universe.draw_noise_like_enhance
    advance_generator_like_enhance = Universe.advance_generator_like_enhance
    _long_rows = Universe._long_rows
    _segments_call = Universe._segments_call

    def __init__(self):
        self.runs = []

    def _begin(self, n_steps, epsilon, segment_s, overlap_s):
        return 5 if n_steps is None else n_steps, 1.3, int(segment_s * self.fs), int(overlap_s * self.fs)

    def _prep(self, x):
        return x.to(torch.float32).contiguous()

    def _segments_plan(self, C, T, segment, overlap, max_batch, ensemble=None, t_raw=None, warm_start=None, use_aux_signal=False):
        return ("plan", warm_start, use_aux_signal)

    def _segments_run(self, plan, x, n_steps, epsilon, keep_rms, noise, counter, members=None):
        self.runs.append((plan, None if noise is None else tuple(noise.shape)))
        return torch.zeros_like(x)


@pytest.mark.parametrize("mode,planes", [({}, 5), ({"warm_start": 0}, 5), ({"warm_start": 2}, 3), ({"warm_start": 4}, 1),
                                         ({"use_aux_signal": True}, 0), ({"warm_start": 2, "use_aux_signal": True}, 0)])
def test_the_draws_are_those_advance_generator_counts(mode, planes):
    C, T = 2, 1000
    Tp = T + (TOT - T % TOT)
    m = _Drawer()
    g, g_ref = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    Universe.enhance_long(m, torch.zeros(C, T), rng=g, **mode)
    Universe.advance_generator_like_enhance(m, g_ref, C, T, **mode)
    assert torch.equal(g.get_state(), g_ref.get_state())
    assert (not planes) == torch.equal(g.get_state(), torch.Generator().manual_seed(3).get_state())
    plan, shape = m.runs[0]
    assert plan == ("plan", mode.get("warm_start"), bool(mode.get("use_aux_signal")))
    assert shape == ((planes, C, Tp) if planes else None)
    # several inputs with one shared generator: input by input, each with the planes of the call on it alone
    lens = [700, 1000, 300]
    g, g_ref = torch.Generator().manual_seed(4), torch.Generator().manual_seed(4)
    Universe.enhance_long_many(m, [torch.zeros(n) for n in lens], g, **mode)
    for n in lens:
        Universe.advance_generator_like_enhance(m, g_ref, 1, n, **mode)
    assert torch.equal(g.get_state(), g_ref.get_state())
    assert m.runs[1][1] == ((planes, len(lens), 1, Tp) if planes else None)  # (draw_noise's own (n, rows, 1, T) layout)


@pytest.mark.parametrize("bad", [5, 6, -1])
def test_warm_start_outside_the_steps_is_refused_before_any_draw(bad):
    m = _Drawer()
    g = torch.Generator().manual_seed(3)
    with pytest.raises(ValueError, match="warm_start"):
        Universe.enhance_long(m, torch.zeros(1, 1000), rng=g, warm_start=bad)
    assert torch.equal(g.get_state(), torch.Generator().manual_seed(3).get_state()) and m.runs == []
