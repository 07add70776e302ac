"""GPU (-m gpu): snake_act_kernel through the stateless ou_snake_act, element by element against the float64 restatement of
tests/snake_fp64.py (itself held against the reference's Activation1d on the same inputs, tests/test_snake_cpu.py).

Allowance: the reference's own fp32 evaluation lies up to `max_rel` (tests/golden/snake_fp64_ref_error.json, relative to the
largest output magnitude of a tensor) from float64 on these inputs; the kernel sums in another order and its sinf differs from
the host's by an ulp or so, so it gets 4 x that, per tensor.  Every element of every tensor is compared, the zero tails of the
ragged batches included.  Observed figures: build/observed/snake_fp64_observed.json (untracked; profiles/snake_fp64_observed.json is a
committed copy)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import snake_fp64 as F
from open_universe_amd import _lib

pytestmark = pytest.mark.gpu
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "observed", "snake_fp64_observed.json")


def observe(section, key, value):
    try:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        old = json.load(open(OUT)) if os.path.exists(OUT) else {}
        old.setdefault(section, {})[key] = value
        with open(OUT, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError:
        pass


def snake_act(x, ea, eb, lens=None, stride=None):
    """ou_snake_act on the device: x (B, C, T) float32 numpy -> y numpy (the rows laid out `stride` apart)."""
    L = _lib.load()
    B, C, T = x.shape
    stride = T if stride is None else stride
    dev = torch.device("cuda:0")
    xd = torch.zeros(B * C, stride, dtype=torch.float32, device=dev)
    xd[:, :T] = torch.from_numpy(x).reshape(B * C, T).to(dev)
    yd = torch.full((B * C, stride), float("nan"), dtype=torch.float32, device=dev)
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)  # noqa: E731
    ead, ebd, upd, dnd = t(ea), t(eb), t(F.UP_K), t(F.DOWN_K)
    ln = None if lens is None else (ctypes.c_int32 * B)(*lens)
    ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())  # noqa: E731
    _lib.check(L.ou_snake_act(ptr(xd), ptr(yd), B, C, T, stride, ln, ptr(ead), ptr(ebd), ptr(upd), ptr(dnd),
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert np.isnan(y[:, T:]).all()  # nothing behind T is touched
    return y[:, :T].reshape(B, C, T)


def _tile():
    return _lib.load().ou_snake_tile()


def _groups():
    rec = F.ref_error()
    g = {}
    for case in F.cases(rec["tile"]):
        tag = case[0]
        key = tag.split(".", 1)[1] if not tag.startswith("ragged") else "ragged." + tag.rsplit(".", 1)[1]
        g.setdefault(key, []).append(case)
    return g


GROUPS = _groups()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_snake_act_against_float64(group):
    rec = F.ref_error()
    assert rec["tile"] == _tile(), "the cases were recorded for another tile: run tests/golden/make_golden_snake.py ref_error"
    allowed = F.KERNEL_FACTOR * rec["max_rel"]
    failures = []
    for tag, T, C, B, beta, lens in GROUPS[group]:
        x, la, lb = F.case_input(T, C, B, beta)
        ea, eb = F.exp32(la), F.exp32(lb)
        ref = F.snake_act(x, ea, eb, lens)
        # (odd T: rows that do not start on 16-byte boundaries, the scalar path; a padded stride: the vector path on the same data)
        for stride in (None, (T + 3) // 4 * 4 + 4):
            y = snake_act(x, ea, eb, lens, stride)
            assert np.isfinite(y).all(), tag
            err = F.rel_error(y, ref)
            name = tag + ("" if stride is None else ".padded")
            print(f"{name}: kernel {err:.3e}  reference fp32 {rec['cases'][tag]['ref_fp32']:.3e}  allowed {allowed:.3e}")
            observe("kernel_vs_float64", name, {"kernel": err, "reference_fp32": rec["cases"][tag]["ref_fp32"]})
            if lens is not None:
                for b, n in enumerate(lens):
                    assert not y[b, :, n:].any(), f"{name}: row {b} is not zero behind its end"
            if not err <= allowed:
                failures.append((name, err))
    observe("bound", "allowed", {"max_rel_reference_fp32": rec["max_rel"], "factor": F.KERNEL_FACTOR, "allowed": allowed})
    assert not failures, f"beyond {allowed:.3e}: {failures}"


@pytest.mark.parametrize("beta", [False, True])
def test_a_row_does_not_depend_on_its_batch(beta):
    """Bit for bit: a row of a batch of 3 against that row alone, whole rows and rows with lengths of their own."""
    tile = _tile()
    for T in (13, tile + 1, 2 * tile + 5):
        x, la, lb = F.case_input(T, 3, 3, beta)
        ea, eb = F.exp32(la), F.exp32(lb)
        full = snake_act(x, ea, eb)
        lens = [T, max(1, T - tile), max(1, T // 2)]
        rag = snake_act(x, ea, eb, lens)
        for b in range(3):
            assert np.array_equal(snake_act(x[b:b + 1], ea, eb).view(np.int32), full[b:b + 1].view(np.int32)), (T, b)
            alone = snake_act(np.ascontiguousarray(x[b:b + 1, :, :lens[b]]), ea, eb)
            assert np.array_equal(alone.view(np.int32), rag[b:b + 1, :, :lens[b]].view(np.int32)), (T, b)
            assert not rag[b, :, lens[b]:].any()
