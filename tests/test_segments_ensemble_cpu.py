"""CPU: ensembles of segmented rows (ou_enhance_segments_ensemble, Universe.enhance_long_ensemble) -- the header and the binding
declare the two entry points (additive: the ABI number stays 7), and the CLI's --segment-ensemble with a fake model: one
`enhance_long_ensemble` call per file with the flag's arguments, and every refusal raises before any model call."""
import os
import re

import pytest
import torch

from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli

NEW = ("ou_segments_ensemble_workspace_bytes", "ou_enhance_segments_ensemble")


def test_header_and_binding_declare_the_entry_points(built_lib):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ouniverse.h")).read()
    assert re.search(r"#define OU_ABI_VERSION 7\b", hdr) and _lib.OU_ABI_VERSION == 7
    for name in NEW:
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(built_lib, name)
        assert getattr(built_lib, name).argtypes is not None
    # the argument lists of the header, counted: (h, C, T_raw, segment, overlap, max_batch, E, nbytes, batch, length) and
    # (h, mix, out, members, noise, C, T_raw, E, stat, segment, overlap, max_batch, n_steps, epsilon, sigma, warm_start, flags, ws,
    # ws_bytes, stream)
    for name, n in zip(NEW, (10, 20)):
        decl = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S).group(1)
        assert len(decl.split(",")) == n == len(getattr(built_lib, name).argtypes), name
    # the header says what grows with the recording
    doc = hdr[hdr.index("ensembles of segmented rows"):hdr.index("int ou_segments_ensemble_workspace_bytes(")]
    assert "REQUIRED" in doc and "GROWS WITH THE RECORDING" in doc


def test_the_model_has_the_method_and_enhance_long_points_to_it():
    from open_universe_amd.universe import Universe

    assert callable(getattr(Universe, "enhance_long_ensemble", None))
    with pytest.raises(ValueError, match="enhance_long_ensemble"):
        Universe._refuse_long_options("enhance_long", {"ensemble": 4})
    assert "enhance_long_ensemble" in Universe.enhance_long.__doc__


class _Model:
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
        self.calls.append(("many",))
        return [0.25 * s for s in sigs]

    def enhance_long(self, mix, **kw):
        self.calls.append(("long",))
        return mix

    def enhance_long_many(self, sigs, rngs=None, **kw):
        self.calls.append(("long_many",))
        return list(sigs)

    def enhance_long_ensemble(self, mix, ensemble, ensemble_stat="median", **kw):
        self.calls.append(("long_ensemble", tuple(mix.shape), ensemble, ensemble_stat, kw))
        return 0.125 * mix

    def advance_generator_like_enhance(self, rng, channels, length, **kw):
        self.calls.append(("advance", channels, length))


def _three_files(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    A.save(src / "a.wav", torch.full((1, 1200), 0.25), 16000)
    A.save(src / "b.wav", torch.full((2, 800), 0.25), 16000)
    A.save(src / "c.wav", torch.full((1, 1000), 0.25), 16000)
    return src


def test_cli_segment_ensemble_is_one_call_per_file(tmp_path):
    src = _three_files(tmp_path)
    m = _Model()
    cli.main([str(src), str(tmp_path / "o"), "--segment-seconds", "2", "--segment-ensemble", "3", "--ensemble_stat", "mean",
              "--segment-overlap", "0.5", "--n_steps", "5"], model=m)
    assert [c[0] for c in m.calls] == ["long_ensemble"] * 3
    assert [c[1] for c in m.calls] == [(1, 1200), (2, 800), (1, 1000)]
    for c in m.calls:
        assert c[2] == 3 and c[3] == "mean"
        kw = c[4]
        assert kw["segment_s"] == 2.0 and kw["overlap_s"] == 0.5 and kw["n_steps"] == 5
        assert isinstance(kw["rng"], torch.Generator)
        assert "ensemble" not in kw and "ensemble_stat" not in kw
    y, _ = A.load(tmp_path / "o" / "b.wav")
    assert torch.allclose(y, torch.full((2, 800), 0.03125))
    # the default statistic and the counter-based noise: file k gets its own source
    m = _Model()
    cli.main([str(src), str(tmp_path / "o2"), "--segment-seconds", "2", "--segment-ensemble", "2", "--noise", "counter"], model=m)
    assert [(c[0], c[2], c[3]) for c in m.calls] == [("long_ensemble", 2, "median")] * 3
    assert [c[4]["rng"].stream for c in m.calls] == [0, 1, 2]
    # without the flag nothing changes: short files go through `enhance`
    m = _Model()
    cli.main([str(src), str(tmp_path / "o3"), "--segment-seconds", "2"], model=m)
    assert [c[0] for c in m.calls] == ["enhance"] * 3


@pytest.mark.parametrize("extra", [
    ["--segment-ensemble", "3"],                                                     # needs --segment-seconds
    ["--segment-seconds", "2", "--segment-ensemble", "3", "--ensemble", "2"],        # refused with --ensemble
    ["--segment-ensemble", "3", "--ensemble", "2"],
    ["--segment-seconds", "2", "--segment-ensemble", "3", "--segment-files", "2"],   # the ragged form is out of scope
    ["--segment-seconds", "2", "--segment-ensemble", "0"],
    ["--segment-seconds", "2", "--segment-ensemble", "3", "--batch-size", "2"],      # (what --segment-seconds refuses anyway)
])
def test_cli_segment_ensemble_refusals(tmp_path, extra):
    src = _three_files(tmp_path)
    m = _Model()
    with pytest.raises(ValueError):
        cli.main([str(src), str(tmp_path / "o")] + extra, model=m)
    assert m.calls == []
