"""CPU: the streaming enhance's host side -- ou_stream_plan and ou_stream_emitted against the restatement of
tests/stream_ref.py and against ou_segment_plan where the header says they agree, the refusals that need no device, the ABI's
shape, and the CLI's argument refusals.  (What needs a handle -- the workspace size, the refusals about the model -- is held in
tests/test_gpu_stream.py.)"""
import ctypes
import re
import os

import numpy as np
import pytest
import torch

import stream_ref as R
from open_universe_amd import _lib
from open_universe_amd import audio as A
from open_universe_amd.bin import enhance as cli

TOT = 8
GEOMS = [(4 * TOT, TOT), (4 * TOT, 0), (4 * TOT, 2 * TOT), (2 * TOT, TOT), (5 * TOT + 3, TOT + 5), (6 * TOT, 3 * TOT)]


def _err():
    return _lib.load().ou_last_error(None).decode()


@pytest.mark.parametrize("segment,overlap", GEOMS)
def test_plan_properties_and_restatement(built_lib, segment, overlap):
    S, V = R.geometry(TOT, segment, overlap)
    for T in range(1, 4 * S + 2):
        p = _lib.stream_plan(TOT, T, segment, overlap)
        ref = R.plan(TOT, T, segment, overlap)
        for key in ("starts", "lengths", "core_begin", "core_end"):
            assert list(p[key]) == ref[key], (T, key)
        assert p["overlap"] == ref["overlap"] and p["T_pad"] == ref["T_pad"] == -(-T // TOT) * TOT
        s, L, n, Tp = p["starts"], p["lengths"], len(p["starts"]), p["T_pad"]
        # windows inside [0, T_pad), the first at 0, the last ending at T_pad, all of one length
        assert s[0] == 0 and s[-1] + L[-1] == Tp and all(0 <= s[k] and s[k] + L[k] <= Tp for k in range(n))
        assert (n == 1 and L[0] == Tp <= S) or (Tp > S and all(int(v) == S for v in L))
        # grid windows on the stride, only the last one may be shifted -- and then it starts before the grid would
        for k in range(n - 1):
            assert s[k] == k * (S - V)
        assert s[-1] <= (n - 1) * (S - V)
        # cores tile [0, T_pad), each inside its window
        assert p["core_begin"][0] == 0 and p["core_end"][-1] == Tp
        for k in range(n):
            assert s[k] <= p["core_begin"][k] < p["core_end"][k] <= s[k] + L[k]
            if k:
                assert p["core_begin"][k] == p["core_end"][k - 1]
        # crossfades as stated: [s_k + S - V, s_k + S) lies inside window k + 1 too, and its middle is the core boundary
        for k in range(n - 1):
            assert s[k + 1] <= s[k] + S - p["overlap"] and s[k] + S <= s[k + 1] + S
            assert p["core_end"][k] == s[k] + S - p["overlap"] + p["overlap"] // 2
        # the geometry of ou_segment_plan for a row whose padded length is this T_pad
        q = _lib.segment_plan(TOT, Tp - 1, segment, overlap)
        assert q["T_pad"] == Tp and q["overlap"] == p["overlap"]
        for key in ("starts", "lengths", "core_begin", "core_end"):
            assert list(q[key]) == list(p[key]), (T, key)


def test_plan_of_an_empty_stream(built_lib):
    p = _lib.stream_plan(TOT, 0, 4 * TOT, TOT)
    assert len(p["starts"]) == 0 and p["T_pad"] == 0


@pytest.mark.parametrize("segment,overlap", GEOMS)
def test_emitted_closed_form(built_lib, segment, overlap):
    S, V = R.geometry(TOT, segment, overlap)
    em = [_lib.stream_emitted(TOT, P, segment, overlap) for P in range(0, 5 * S)]
    assert em == [R.emitted(TOT, P, segment, overlap) for P in range(0, 5 * S)]
    assert all(a <= b for a, b in zip(em, em[1:])) and all(0 <= e <= P for P, e in enumerate(em))  # monotone, causal
    # once window k is complete everything below s_k + S - V is out
    for P, e in enumerate(em):
        if P >= S:
            k = (P - S) // (S - V)
            assert e == k * (S - V) + S - V
    # any split of the pushes sums to the same count, and the flush brings it to T
    g = torch.Generator().manual_seed(segment * 100 + overlap)
    for _ in range(50):
        T = int(torch.randint(1, 5 * S - 1, (1,), generator=g))
        cuts = sorted(set(int(v) for v in torch.randint(0, T + 1, (6,), generator=g)) | {0, T})
        total = sum(em[b] - em[a] for a, b in zip(cuts, cuts[1:]))
        assert total == em[T] and total + (T - em[T]) == T


def test_latency_is_one_window(built_lib):
    """A sample is emitted at the latest S samples after it arrived: sample u is out once P >= u + S."""
    for segment, overlap in GEOMS:
        S, V = R.geometry(TOT, segment, overlap)
        for u in range(0, 3 * S):
            P = next(P for P in range(u + 1, u + 2 * S + 2) if R.emitted(TOT, P, segment, overlap) > u)
            assert P - u <= S


@pytest.mark.parametrize("args,msg", [
    ((TOT, 10, 2 * TOT - 1, 0), "segment must be at least two total down-sampling factors (16 samples)"),
    ((TOT, 10, 4 * TOT, 3 * TOT), "overlap must lie in [0, segment / 2]"),
    ((TOT, 10, 4 * TOT, -1), "overlap must lie in [0, segment / 2]"),
    ((TOT, -1, 4 * TOT, TOT), "T >= 0"),
    ((0, 10, 4 * TOT, TOT), "tot_ds >= 1"),
])
def test_plan_refusals(built_lib, args, msg):
    n = ctypes.c_int32()
    rc = built_lib.ou_stream_plan(*args, 0, None, None, None, None, ctypes.byref(n), None, None)
    assert rc == _lib.OU_EINVAL and msg in _err()
    if args[1] >= 0:
        assert built_lib.ou_stream_emitted(args[0], args[1], args[2], args[3]) == -1 and msg in _err()


def test_plan_capacity(built_lib):
    starts = (ctypes.c_int64 * 1)()
    n = ctypes.c_int32()
    rc = built_lib.ou_stream_plan(TOT, 20 * TOT, 4 * TOT, TOT, 1, starts, None, None, None, ctypes.byref(n), None, None)
    assert rc == _lib.OU_EINVAL and "capacity" in _err() and n.value > 1


def test_refusals_that_need_no_device(built_lib):
    L = built_lib
    spec = _lib.StreamSpec()
    spec.C, spec.segment, spec.overlap, spec.n_steps = 0, 4 * TOT, TOT, 4
    out = ctypes.c_void_p()
    assert L.ou_stream_create(None, ctypes.byref(spec), None, 0, ctypes.byref(out)) == _lib.OU_EINVAL
    assert "C must be at least 1" in _err() and not out.value
    need = ctypes.c_size_t()
    assert L.ou_stream_workspace_bytes(None, 0, 4 * TOT, TOT, ctypes.byref(need)) == _lib.OU_EINVAL
    assert "C must be at least 1" in _err()
    # a push, a flush and a destroy on something that is not a live stream: refused by address, nothing is dereferenced
    junk = (ctypes.c_char * 512)()
    bogus = ctypes.cast(junk, ctypes.c_void_p)
    n_out = ctypes.c_int64(-7)
    assert L.ou_stream_push(bogus, None, 0, 0, None, 0, 0, ctypes.byref(n_out), None) == _lib.OU_EINVAL
    assert "ou_stream_push: not a live stream" in _err() and n_out.value == -7
    assert L.ou_stream_flush(bogus, None, 0, 0, ctypes.byref(n_out), None) == _lib.OU_EINVAL
    assert "ou_stream_flush: not a live stream" in _err()
    assert L.ou_stream_push(None, None, 0, 0, None, 0, 0, ctypes.byref(n_out), None) == _lib.OU_EINVAL
    L.ou_stream_destroy(bogus)
    assert "ou_stream_destroy: not a live stream" in _err()


def test_abi_is_additive_and_the_sizer_takes_no_length(built_lib):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ouniverse.h")).read()
    assert re.search(r"#define OU_ABI_VERSION 7\b", hdr) and _lib.OU_ABI_VERSION == 7
    names = ["ou_stream_plan", "ou_stream_emitted", "ou_stream_workspace_bytes", "ou_stream_create", "ou_stream_destroy",
             "ou_stream_push", "ou_stream_flush"]
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(built_lib, name)
    # the workspace cannot depend on the stream's length: the sizer is not told one
    decl = re.search(r"^int ou_stream_workspace_bytes\((.*?)\);", hdr, re.M | re.S).group(1)
    assert [a.strip() for a in decl.split(",")] == ["const ou_handle* h", "int32_t C", "int32_t segment", "int32_t overlap",
                                                    "size_t* nbytes"]
    assert "OU_STREAM_CLIP" in hdr and _lib.OU_STREAM_CLIP == 1


def test_kernels_are_in_the_library_and_in_make_check(built_lib):
    blob = open(_lib.lib_path(), "rb").read()
    assert b"stream_gather_kernel" in blob and b"stream_emit_kernel" in blob
    mk = open(os.path.join(os.path.dirname(_lib.lib_path()), "..", "csrc", "Makefile")).read()
    kernels = re.search(r"^KERNELS = (.*)$", mk, re.M).group(1).split()
    assert "ou_stream" in kernels and "check_spills.py $(KASM)" in mk  # every file of KERNELS goes through the spill check


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
        self.calls.append(("enhance",))
        return 0.5 * mix

    def stream(self, **kw):
        self.calls.append(("stream", kw))
        model = self

        class _S:
            def __enter__(self):
                return self

            def __exit__(self, *exc):
                model.calls.append(("close",))
                return False

            def push(self, x):
                model.calls.append(("push", tuple(x.shape)))
                return x[:, :0]

            def flush(self, flat=None):
                model.calls.append(("flush", flat))
                return torch.full((kw["channels"], 24000), 0.125)

        return _S()


@pytest.fixture(autouse=True)
def _builtin_wav_codec(monkeypatch):
    monkeypatch.setattr(A, "_torchaudio", lambda: None)  # the built-in WAV codec, whatever else this process has imported


def _file(tmp_path):
    src = tmp_path / "in.wav"
    A.save(src, torch.full((2, 24000), 0.25), 16000)  # 1.5 s, two channels
    return src


def test_cli_streams_a_file_in_chunks(tmp_path):
    m = _Model()
    out = tmp_path / "o.wav"
    cli.main([str(_file(tmp_path)), str(out), "--segment-seconds", "1", "--segment-overlap", "0.25", "--stream", "0.5",
              "--keep_rms", "1", "--seed", "9"], model=m)
    assert m.calls[0][0] == "stream"
    kw = m.calls[0][1]
    assert kw["channels"] == 2 and kw["segment_s"] == 1.0 and kw["overlap_s"] == 0.25 and kw["seed"] == 9 and kw["keep_rms"]
    assert [c for c in m.calls[1:]] == [("push", (2, 8000))] * 3 + [("flush", False), ("close",)]
    y, fs = A.load(out)
    assert fs == 16000 and tuple(y.shape) == (2, 24000) and torch.allclose(y, torch.full_like(y, 0.125), atol=1e-4)


@pytest.mark.parametrize("extra,msg", [
    (["--stream", "0.5"], "--stream needs --segment-seconds"),
    (["--stream", "0", "--segment-seconds", "1"], "--stream must be a positive number of seconds"),
    (["--stream", "0.5", "--segment-seconds", "1", "--batch-size", "2"], "--stream cannot be combined with --batch-size"),
    (["--stream", "0.5", "--segment-seconds", "1", "--in-flight", "2"], "--stream cannot be combined with --batch-size or --in-flight"),
    (["--stream", "0.5", "--segment-seconds", "1", "--ensemble", "2"], "--stream cannot be combined with --ensemble"),
    (["--stream", "0.5", "--segment-seconds", "1", "--segment-ensemble", "2"], "--stream cannot be combined with --segment-ensemble"),
    (["--stream", "0.5", "--segment-seconds", "1", "--segment-ensemble", "2", "--segment-ensemble-files", "2"],
     "--stream cannot be combined with --segment-ensemble or --segment-ensemble-files"),
    (["--stream", "0.5", "--segment-seconds", "1", "--segment-files", "2"], "--stream cannot be combined with --segment-files"),
])
def test_cli_refusals_call_nothing(tmp_path, extra, msg):
    m = _Model()
    with pytest.raises(ValueError) as e:
        cli.main([str(_file(tmp_path)), str(tmp_path / "o.wav"), "--segment-overlap", "0.25"][:2] + extra, model=m)
    assert msg in str(e.value) and m.calls == []


def test_cli_without_the_option_is_what_it_was(tmp_path):
    m = _Model()
    cli.main([str(_file(tmp_path)), str(tmp_path / "o.wav")], model=m)
    assert m.calls == [("enhance",)]
    assert cli.build_parser().parse_args(["a", "b"]).stream is None
