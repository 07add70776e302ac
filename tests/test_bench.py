"""bench.py's options: a plain run times only the headline loop (`--full` adds every other leg), `--steps` is the number of
timed steps, and `--dump-outputs DIR` writes what the timed path returned in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_args_full_and_dump_outputs():
    a = bench.parse_args([])
    assert not a.full and a.dump_outputs is None and a.steps == 20 and a.warmup == 3
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "0", "--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d" and a.steps == 7 and a.warmup == 0


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_parse_args_refuses_no_timed_steps(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    x = torch.randn(3, 1000, generator=torch.Generator().manual_seed(1))
    bench.dump_outputs(str(tmp_path / "a"), x, 0, 1)
    a = np.load(tmp_path / "a" / "enhanced.npy")
    assert a.dtype == np.float32 and a.shape == (3, 1000) and np.array_equal(a, x.numpy())
    # beyond the limit: a fixed, seeded sample (the same elements every time), split between the ranks
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 1000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), x, 1, 2)
    b = np.load(tmp_path / "b" / "enhanced_rank1.npy")
    assert b.dtype == np.float32 and b.shape == (500,)
    assert np.array_equal(b, np.load(tmp_path / "c" / "enhanced_rank1.npy"))
    assert np.isin(b, x.numpy().ravel()).all()


def _bench(out_dir, steps, warmup, **env):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--batch", "2",
                        "--dump-outputs", str(out_dir)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return res, np.load(os.path.join(out_dir, "enhanced.npy"))


@pytest.mark.gpu
def test_timed_loop_runs_exactly_the_given_steps():
    calls = []
    dt, out = bench.timed_loop(lambda: calls.append(1) or len(calls), 5, 1, torch.device("cuda:0"))
    assert len(calls) == 5 and out == 5 and dt > 0


@pytest.mark.gpu
def test_bench_plain_run_headline_and_dump(tmp_path):
    """A plain run: the headline fields, none of the --full legs, and in DIR/enhanced.npy the enhanced batch (2 x 4 s at
    16 kHz) of call warmup + steps.  Every call draws fresh noise from one seeded generator, so the dump tells which call it
    came from: the same arguments give the same array; 1 + 3 and 2 + 2 calls give the same array (the last timed step, not a
    warm-up's); 1 + 2 calls give another one (--steps sets how many calls run)."""
    res, a = _bench(tmp_path / "a", 3, 1)
    assert res["unit"] == "x_realtime" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(2 * 4.0 / (res["ms_per_step"] * 1e-3), rel=1e-6)
    for k in ("roofline", "batch_sweep", "free_running", "sustained", "in_flight", "host_enqueue", "cpu_baseline"):
        assert k not in res, k
    assert a.dtype == np.float32 and a.shape == (2, 64000) and np.isfinite(a).all() and a.std() > 0
    _, a2 = _bench(tmp_path / "a2", 3, 1)
    assert np.array_equal(a, a2)
    _, b = _bench(tmp_path / "b", 2, 2)
    assert np.array_equal(a, b)
    # (and the OMP_NUM_THREADS override of the host-thread cap reaches the line)
    res_c, c = _bench(tmp_path / "c", 2, 1, OMP_NUM_THREADS="3")
    assert res_c["steps"] == 2 and res_c["host_threads_per_rank"] == 3
    assert c.shape == a.shape and not np.array_equal(a, c)
