"""CPU: ensembles of segmented rows with lengths of their own (ou_enhance_segments_var_ensemble,
Universe.enhance_long_many_ensemble) -- the header and the binding declare the two entry points in the same argument order
(additive: the ABI number stays 7), and the CLI's --segment-ensemble-files with a fake model: the groups it forms, one noise
source per file, every refusal raises before any model call, and the default is still one `enhance_long_ensemble` call per file."""
import ctypes
import os
import re

import pytest
import torch

from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli

NEW = ("ou_segments_var_ensemble_workspace_bytes", "ou_enhance_segments_var_ensemble")
# C type of the header -> what the binding must declare in that place (pointers to device memory, handles and streams are void*)
_CT = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t,
       "double": ctypes.c_double, "const int64_t*": ctypes.POINTER(ctypes.c_int64), "size_t*": ctypes.POINTER(ctypes.c_size_t),
       "int32_t*": ctypes.POINTER(ctypes.c_int32), "const float* sigma_host": ctypes.POINTER(ctypes.c_float)}


def _header():
    return open(os.path.join(os.path.dirname(__file__), "..", "include", "ouniverse.h")).read()


def _decl(hdr, name):
    args = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S).group(1)
    return [" ".join(a.split()) for a in args.split(",")]


def test_header_declares_both_functions_and_the_abi_number_stays():
    hdr = _header()
    assert re.search(r"#define OU_ABI_VERSION 7\b", hdr) and _lib.OU_ABI_VERSION == 7
    for name in NEW:
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
    names = [a.split()[-1].lstrip("*") for a in _decl(hdr, NEW[0])]
    assert names == ["h", "C", "t_raw", "segment", "overlap", "max_batch", "E", "nbytes", "batch", "length"]
    names = [a.split()[-1].lstrip("*") for a in _decl(hdr, NEW[1])]
    assert names == ["h", "mix", "out", "members", "noise", "C", "T_raw_max", "t_raw", "E", "stat", "segment", "overlap",
                     "max_batch", "n_steps", "epsilon", "sigma_host", "warm_start", "flags", "ws", "ws_bytes", "stream"]
    doc = hdr[hdr.index("ensembles of segmented rows with lengths of their own"):hdr.index("int %s(" % NEW[0])]
    assert "MEMBER-MAJOR" in doc and "REQUIRED" in doc and "floor(max_batch / E)" in doc


def test_binding_has_the_argument_order_of_the_header(built_lib):
    hdr = _header()
    for name in NEW:
        fn = getattr(built_lib, name)
        decl = _decl(hdr, name)
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == len(decl), name
        for arg, got in zip(decl, fn.argtypes):
            ctype = arg.rsplit(" ", 1)[0]
            want = _CT.get(arg, _CT.get(ctype, ctypes.c_void_p))  # (sigma_host is the one typed float pointer of the binding)
            assert got is want, (name, arg, got)


def test_the_model_has_the_method_and_refuses_unknown_keywords():
    from open_universe_amd.universe import Universe

    assert callable(getattr(Universe, "enhance_long_many_ensemble", None))
    with pytest.raises(ValueError, match="warm_start"):
        Universe._refuse_long_options("enhance_long_many_ensemble", {"warm_start": 1})
    with pytest.raises(TypeError, match="segmnt_s"):
        Universe._refuse_long_options("enhance_long_many_ensemble", {"segmnt_s": 2.0})


class _Model:
    fs = 16000
    device = "cpu"
    tot_ds = 1

    class _KW(dict):
        pass

    diff_kwargs = _KW(n_steps=8, epsilon=1.3)

    def __init__(self):
        self.calls = []

    def enhance(self, mix, n_steps: int = None, epsilon: float = None, target: str = None, rng: torch.Generator = None,
                use_aux_signal: bool = False, keep_rms: bool = False, ensemble: int = None, ensemble_stat: str = "median",
                warm_start: int = None) -> torch.Tensor:
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

    def enhance_long_many_ensemble(self, sigs, ensemble, ensemble_stat="median", rngs=None, **kw):
        self.calls.append(("long_many_ensemble", [tuple(s.shape) for s in sigs], ensemble, ensemble_stat, rngs, kw))
        return [0.0625 * s for s in sigs]

    def advance_generator_like_enhance(self, rng, channels, length, **kw):
        self.calls.append(("advance", channels, length))


def _three_files(tmp_path, rates=(16000, 16000, 16000)):
    src = tmp_path / "in"
    src.mkdir()
    A.save(src / "a.wav", torch.full((1, 1200), 0.25), rates[0])
    A.save(src / "b.wav", torch.full((2, 800), 0.25), rates[1])
    A.save(src / "c.wav", torch.full((1, 1000), 0.25), rates[2])
    return src


SEG = ["--segment-seconds", "2", "--segment-ensemble", "3"]


def test_cli_groups_of_two_over_three_files(tmp_path):
    src = _three_files(tmp_path)
    m = _Model()
    cli.main([str(src), str(tmp_path / "o")] + SEG + ["--segment-ensemble-files", "2", "--ensemble_stat", "mean",
                                                      "--segment-overlap", "0.5", "--n_steps", "5"], model=m)
    assert [c[0] for c in m.calls] == ["long_many_ensemble"] * 2
    assert [c[1] for c in m.calls] == [[(1, 1200), (2, 800)], [(1, 1000)]]
    for c in m.calls:
        assert c[2] == 3 and c[3] == "mean"
        assert isinstance(c[4], torch.Generator)  # the shared generator: it advances file by file inside the call
        kw = c[5]
        assert kw["segment_s"] == 2.0 and kw["overlap_s"] == 0.5 and kw["n_steps"] == 5
        assert set(kw) <= {"segment_s", "overlap_s", "n_steps", "epsilon", "keep_rms"}
    assert m.calls[0][4] is m.calls[1][4]
    y, fs = A.load(tmp_path / "o" / "b.wav")
    assert fs == 16000 and torch.allclose(y, torch.full((2, 800), 0.25 * 0.0625))
    y, _ = A.load(tmp_path / "o" / "c.wav")
    assert torch.allclose(y, torch.full((1, 1000), 0.25 * 0.0625))


def test_cli_one_noise_source_per_file(tmp_path):
    src = _three_files(tmp_path)
    m = _Model()
    cli.main([str(src), str(tmp_path / "o")] + SEG + ["--segment-ensemble-files", "2", "--noise", "counter", "--seed", "11"],
             model=m)
    assert [c[0] for c in m.calls] == ["long_many_ensemble"] * 2
    got = [[(g.seed, g.stream) for g in c[4]] for c in m.calls]
    assert got == [[(11, 0), (11, 1)], [(11, 2)]]  # file index = stream, as the one-file-per-call loop hands them out
    assert all(c[3] == "median" for c in m.calls)
    # --per-file-seed: one generator per file, seeded seed + k as the serial loop re-seeds its generator
    m = _Model()
    cli.main([str(src), str(tmp_path / "o2")] + SEG + ["--segment-ensemble-files", "3", "--per-file-seed", "--seed", "5"], model=m)
    assert [c[1] for c in m.calls] == [[(1, 1200), (2, 800), (1, 1000)]]
    gens = m.calls[0][4]
    assert len(gens) == 3 and len({id(g) for g in gens}) == 3
    for k, g in enumerate(gens):
        assert torch.equal(g.get_state(), torch.Generator().manual_seed(5 + k).get_state())


def test_cli_a_new_sample_rate_ends_a_group(tmp_path):
    src = _three_files(tmp_path, rates=(16000, 8000, 8000))
    m = _Model()
    cli.main([str(src), str(tmp_path / "o")] + SEG + ["--segment-ensemble-files", "3"], model=m)
    assert [len(c[1]) for c in m.calls] == [1, 2]
    y, fs = A.load(tmp_path / "o" / "b.wav")
    assert fs == 8000 and y.shape == (2, 800)


@pytest.mark.parametrize("extra", [
    ["--segment-ensemble-files", "2"],                                                  # needs --segment-seconds and -ensemble
    ["--segment-seconds", "2", "--segment-ensemble-files", "2"],                        # needs --segment-ensemble
    ["--segment-ensemble", "3", "--segment-ensemble-files", "2"],                       # needs --segment-seconds
    SEG + ["--segment-ensemble-files", "2", "--segment-files", "2"],
    SEG + ["--segment-files", "2"],                                                     # (stays refused)
    SEG + ["--segment-ensemble-files", "2", "--batch-size", "2"],
    SEG + ["--segment-ensemble-files", "2", "--in-flight", "2"],
    SEG + ["--segment-ensemble-files", "2", "--batch-size", "2", "--pad-batch"],
    SEG + ["--segment-ensemble-files", "2", "--pad-batch"],
    SEG + ["--segment-ensemble-files", "2", "--ensemble", "2"],
    SEG + ["--segment-ensemble-files", "2", "--target", "t.wav"],
    SEG + ["--segment-ensemble-files", "2", "--warm_start", "1"],
    SEG + ["--segment-ensemble-files", "2", "--use_aux_signal", "1"],
    SEG + ["--segment-ensemble-files", "0"],
    SEG + ["--segment-ensemble-files", "-1"],
])
def test_cli_refusals_run_nothing(tmp_path, extra):
    src = _three_files(tmp_path)
    m = _Model()
    with pytest.raises(ValueError):
        cli.main([str(src), str(tmp_path / "o")] + extra, model=m)
    assert m.calls == []


def test_cli_default_is_one_enhance_long_ensemble_call_per_file(tmp_path):
    src = _three_files(tmp_path)
    for extra in ([], ["--segment-ensemble-files", "1"]):
        m = _Model()
        cli.main([str(src), str(tmp_path / "o")] + SEG + extra, model=m)
        assert [c[0] for c in m.calls] == ["long_ensemble"] * 3
        assert [c[1] for c in m.calls] == [(1, 1200), (2, 800), (1, 1000)]
