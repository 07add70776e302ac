#!/usr/bin/env python
"""
bench.py -- headline benchmark of the `model.enhance` hot path on MI355X.

Metric (BASELINE.json): real-time factor (+ utterances/s) of UNIVERSE++ 16 kHz, 8-step enhance.
  step      = one `enhance` call over one batch of synthetic 4 s utterances (default batch 1 per GPU = configs[1])
  value     = whole-job audio seconds enhanced per wall second (inputs already resident in HBM), measured in the
              PRODUCT DEFAULT mode (`model.check_status = True`: the stream is synchronised and the device status word
              read after every call); with --full the free-running mode (no host sync inside the loop) is reported beside it
  roofline  = (--full) the dominant conv kernel (the one with the most device time per enhance among conv_direct_kernel,
              conv_mfma_kernel and conv_chain_kernel): algorithmic FLOPs of its launches / their device-side durations,
              against the fp32 MFMA peak (157.3 TFLOP/s) -- plus the HBM view, the other conv kernels and the
              whole-score-forward fractions (the unit of work is one score-network forward)
  cpu_baseline = (--full) the CPU oracle (plain-PyTorch restatement of the reference path) on the host's cores

Usage: python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
  A plain run sets up, warms up, times exactly K steps and prints the headline line (metric, value, unit, ms_per_step, ...).
  --full adds everything else the benchmark measures or checks: the free-running loop, per-rank times, the batch sweep, the
  sustained leg, the ragged-set leg, host enqueue / hipGraph times, the profiled roofline pass, the CPU baseline and the
  weight-broadcast / RCCL report.
  --dump-outputs DIR writes what the timed path returned in its last timed step as DIR/enhanced.npy (float32; rank r > 0:
  enhanced_rank<r>.npy); inputs, weights and noise are seeded, so two builds can be compared output for output.
  N > 1 without a launcher: the script re-executes itself under `torch.distributed.run` with N ranks (one per GPU);
  under a launcher (RANK / WORLD_SIZE set) it asserts WORLD_SIZE == N.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 = fp32 vector rate
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8 TB/s spec (6.29 TB/s measured copy ceiling)

# SURVEY.md 8(d) [probe]: algorithmic work of ONE score-network forward on a padded 4 s utterance, layer-granular
# accounting (every dense op reads its input once and writes its output once, folded weights read once per forward):
#   (GFLOP, activation MB per utterance, weight MB)
SCORE_FORWARD_WORK = {"PP16": (30.82, 421.8 + 90.3, 51.6), "OR16": (30.65, 421.9, 52.3), "PP24": (106.9, 998.6 + 216.8, 117.5)}


def synth_mix(fs, B, T, seed0):
    """x_i = 0.1 sin(2 pi f_i t)(0.5 + 0.5 sin(2 pi 3 t)) + 0.03 randn, f_i = 110 (1 + i mod 8)."""
    import math

    t = torch.arange(T) / fs
    out = []
    for i in range(B):
        g = torch.Generator().manual_seed(seed0 + i)
        f = 110.0 * (1 + (seed0 + i) % 8)
        out.append(0.1 * torch.sin(2 * math.pi * f * t) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3 * t))
                   + 0.03 * torch.randn(T, generator=g))
    return torch.stack(out)


def host_cpu_info():
    """lscpu's view of the host: model name, sockets, physical cores, logical CPUs."""
    import subprocess

    info = {"logical_cpus": os.cpu_count()}
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        kv = {}
        for line in out.splitlines():
            if ":" in line:
                k, v = line.split(":", 1)
                kv[k.strip()] = v.strip()
        info["model"] = kv.get("Model name")
        sockets = int(kv.get("Socket(s)", "0") or 0)
        cps = int(kv.get("Core(s) per socket", "0") or 0)
        info["sockets"] = sockets or None
        info["physical_cores"] = sockets * cps or None
        info["threads_per_core"] = int(kv.get("Thread(s) per core", "0") or 0) or None
    except Exception as e:  # lscpu missing: /proc/cpuinfo has the model at least
        info["lscpu_error"] = repr(e)[:100]
        try:
            for line in open("/proc/cpuinfo"):
                if line.startswith("model name"):
                    info["model"] = line.split(":", 1)[1].strip()
                    break
        except OSError:
            pass
    return info


class GpuSampler:
    """sclk / power of the device while a leg runs: a thread polling the amdgpu sysfs files (hwmon freq1_input, power1_average /
    power1_input) of the card; falls back to `rocm-smi --json` when sysfs has nothing to offer."""

    def __init__(self, period_s=0.25, device_index=0):
        import glob
        import threading

        self.period = period_s
        self.samples = []  # (t, sclk MHz or None, W or None)
        self._stop = threading.Event()
        self._freq, self._power = [], []
        # the sysfs card of THIS HIP device (a box exposes every GPU of the node under /sys/class/drm): match the PCI address
        want = None
        try:
            pr = torch.cuda.get_device_properties(device_index)
            want = f"{getattr(pr, 'pci_domain_id', 0):04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}"
        except Exception:
            pass
        self.card = None
        cards = []
        for card in sorted(glob.glob("/sys/class/drm/card[0-9]*/device")):
            try:
                if open(os.path.join(card, "vendor")).read().strip() != "0x1002":
                    continue
            except OSError:
                continue
            cards.append(card)
        match = [c for c in cards if want and os.path.basename(os.path.realpath(c)).lower().startswith(want)]
        for card in match or (cards if len(cards) == 1 else []):
            self._freq = sorted(glob.glob(os.path.join(card, "hwmon/hwmon*/freq1_input")))
            self._power = sorted(glob.glob(os.path.join(card, "hwmon/hwmon*/power1_average"))) or \
                sorted(glob.glob(os.path.join(card, "hwmon/hwmon*/power1_input")))
            if self._freq or self._power:
                self.card = f"{os.path.basename(os.path.dirname(card))} ({os.path.basename(os.path.realpath(card))})"
                break
        self.source = "sysfs hwmon" if (self._freq or self._power) else "rocm-smi"
        self._thread = threading.Thread(target=self._run, daemon=True)

    @staticmethod
    def _read(paths, scale):
        for p in paths:
            try:
                return float(open(p).read().strip()) * scale
            except (OSError, ValueError):
                continue
        return None

    def _smi(self):
        import subprocess

        try:
            out = subprocess.run(["rocm-smi", "-c", "-P", "--json"], capture_output=True, text=True, timeout=5).stdout
            d = json.loads(out)
            card = next(iter(d.values()))
            sclk = next((v for k, v in card.items() if "sclk" in k.lower() and "(" in str(v)), None)
            mhz = float(str(sclk).split("(")[1].split("M")[0]) if sclk else None
            pw = next((float(v) for k, v in card.items() if "power" in k.lower() and str(v).replace(".", "").isdigit()), None)
            return mhz, pw
        except Exception:
            return None, None

    def _run(self):
        t0 = time.perf_counter()
        while not self._stop.is_set():
            if self.source == "sysfs hwmon":
                mhz, w = self._read(self._freq, 1e-6), self._read(self._power, 1e-6)
            else:
                mhz, w = self._smi()
            self.samples.append((time.perf_counter() - t0, mhz, w))
            self._stop.wait(self.period)

    def __enter__(self):
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._thread.join(timeout=10)
        return False

    def summary(self):
        f = [m for _, m, _ in self.samples if m]
        w = [p for _, _, p in self.samples if p]
        out = {"source": self.source, "card": self.card, "samples": len(self.samples), "period_s": self.period}
        if f:
            out["sclk_MHz"] = {"min": min(f), "max": max(f), "mean": sum(f) / len(f), "first": f[0], "last": f[-1]}
        if w:
            out["power_W"] = {"min": min(w), "max": max(w), "mean": sum(w) / len(w)}
        out["trace_t_s_sclk_MHz_power_W"] = [[round(t, 2), m, p] for t, m, p in self.samples[:: max(1, len(self.samples) // 48)]]
        return out


def cpu_baseline_worker(model_name, n_steps, seconds, budget_s):
    """Runs in a child process: the oracle timed on the host cores.  The intra-op thread count is SWEPT (8 / 16 / 32 /
    64 / 128, capped by the logical CPUs): batch-1 convolutions of this size do not scale to a whole two-socket host --
    oversubscribed they run several times slower than on 8-16 threads -- and the best setting is what is reported, with
    the whole sweep beside it.  Bounded sample: one utterance; for more than 8 diffusion steps the cost is measured at 2
    and at 8 steps and extended linearly (one enhance = 1 conditioner pass + n score passes, all passes identical)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import restatement as O
    import open_universe_amd  # noqa: F401
    from open_universe_amd import config as C
    from open_universe_amd import state_dict as S

    spec = C.spec_from_config(C.builtin_config(model_name))
    sd = S.synthetic_state_dict(spec, seed=0)
    ncpu = os.cpu_count() or 1
    T = int(seconds * spec.fs)
    mix = synth_mix(spec.fs, 1, T, 1000)
    sdict = spec.to_dict()
    g = torch.Generator().manual_seed(1028282)

    def timed(n):
        t0 = time.time()
        O.enhance(sd, sdict, mix, n_steps=n, rng=g)
        return time.time() - t0

    n_meas = min(n_steps, 8)
    t_begin = time.time()
    cands = sorted({min(c, ncpu) for c in (8, 16, 32, 64, 128)})
    sweep = {}
    torch.set_num_threads(cands[0])
    timed(2)  # warm-up (allocator, oneDNN primitive caches)
    for c in cands:
        if sweep and time.time() - t_begin > 0.6 * budget_s:
            break
        torch.set_num_threads(c)
        timed(2)  # the thread pool of this setting
        # (the cheap settings twice, the faster run counts: a single sample flipped the choice between 8 and 16 threads from run
        # to run and moved the reported baseline by 30 %)
        sweep[c] = min(timed(n_meas), timed(n_meas)) if c <= 16 else timed(n_meas)
    best = min(sweep, key=sweep.get)
    torch.set_num_threads(best)
    times = [sweep[best]]
    while len(times) < 3 and time.time() - t_begin < budget_s:
        times.append(timed(n_meas))
    times.sort()
    med = times[0]  # the FASTEST run: the baseline gets the benefit of the doubt
    how = f"fastest of {len(times)} run(s) at the best thread count"
    if n_meas != n_steps:
        t2 = timed(2)
        per_step = max(0.0, (med - t2) / (n_meas - 2))
        med = t2 + per_step * (n_steps - 2)
        how += f" at {n_meas} steps, extended linearly to {n_steps} steps with the 2-step run ({per_step:.2f} s per step)"
    host = host_cpu_info()
    print("CPU_BASELINE_JSON " + json.dumps({
        "value": seconds / med,
        "unit": "x_realtime",
        "utterances_per_s": 1.0 / med,
        "cores": best,
        "cores_note": "torch intra-op threads of the best run of the sweep (the threads actually used); the host's sockets / "
                      "physical cores / logical CPUs are in `host`",
        "host": host,
        "kind": "port",
        "thread_sweep_s_per_enhance": {str(k): round(v, 3) for k, v in sweep.items()},
        "sample": f"1 utterance of {seconds:.0f} s, {model_name}, {n_steps} steps, {how} "
                  f"({med:.2f} s per enhance on {best} torch threads; {ncpu} logical CPUs; thread counts tried: "
                  f"{sorted(sweep)}); oracle/restatement.py (validated against the imported reference)",
    }))


def cpu_baseline(model_name, n_steps, seconds, budget_s=30.0, hard_limit_s=180.0):
    """Bounded CPU sample in a child process, so that a pathological host can never stall the GPU bench."""
    import subprocess

    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--model", model_name,
           "--n_steps", str(n_steps), "--seconds", str(seconds), "--cpu-budget", str(budget_s)]
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "OMP_NUM_THREADS"):
        env.pop(k, None)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=hard_limit_s, env=env)
        for line in r.stdout.splitlines():
            if line.startswith("CPU_BASELINE_JSON "):
                return json.loads(line[len("CPU_BASELINE_JSON "):])
        return {"value": None, "unit": "x_realtime", "cores": None, "kind": "port",
                "sample": "cpu baseline failed: " + (r.stderr or "")[-300:]}
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "x_realtime", "cores": None, "kind": "port",
                "sample": f"cpu baseline did not finish within {hard_limit_s:.0f} s (skipped)"}


# tools/ubench/xchg_latency.hip (profiles/r03_final_ubench_xchg_latency.txt): a bare all-gather step of 16 workgroups through
# L2 -- one store latency + one load latency, no compute -- takes 859 cycles of the 2.4 GHz shader clock
GRU_HANDOFF_FLOOR_US = 859 / 2400.0


def gru_roofline(gru_recs, args, ms_per_enhance):
    """The recurrence is latency-bound (T sequential steps, one L2 hand-off each), not MFMA- or HBM-bound: its figure of
    merit is microseconds per step against the measured floor of the hand-off itself."""
    if not gru_recs:
        return None
    n_prof = max(1, args.profile_steps)
    us = [1e3 * r[0] for r in gru_recs]
    steps = [r[3] - 1000 for r in gru_recs]
    per_step = sum(us) / sum(steps)
    return {"kernel": "ou::gru_ring_kernel (bidirectional GRU recurrence: a cluster of H / 8 workgroups per direction keeps W_hh in "
                      "registers, h is exchanged through L2 with {value, tag} granules)",
            "bound": "latency (one store + one load through L2 per time step)",
            "passes_per_enhance": len(gru_recs) // n_prof, "steps_per_pass": steps[0],
            "us_per_pass": sum(us) / len(us), "us_per_step": per_step,
            "handoff_floor_us_per_step": GRU_HANDOFF_FLOOR_US, "frac_of_floor": GRU_HANDOFF_FLOOR_US / per_step,
            "ms_per_enhance": sum(us) / 1e3 / n_prof, "share_of_enhance": sum(us) / 1e3 / n_prof / ms_per_enhance,
            "algorithmic_gflop_per_enhance": sum(r[1] for r in gru_recs) / n_prof / 1e9,
            "tflops": sum(r[1] for r in gru_recs) / (sum(us) * 1e-6) / 1e12,
            "method": "device-side first-block-start .. last-block-end of every GRU launch of the profiled pass (same stamps as "
                      "the conv launches); floor = tools/ubench/xchg_latency.hip (859 cycles at 2.4 GHz)"}


# --dump-outputs: at most this many bytes over all ranks (a larger output is cut to a fixed, seeded sample of its elements)
DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(dirname, out, rank, world):
    """What the timed path handed its caller in the last timed step (this rank's enhanced batch, (B, T)) as float32 .npy.
    Beyond DUMP_LIMIT_BYTES / world bytes per rank: the elements at a seeded random subset of flat indices (sorted), 1-D."""
    import numpy as np

    a = out.detach().to(torch.float32).cpu().contiguous()
    budget = DUMP_LIMIT_BYTES // world // 4
    if a.numel() > budget:
        idx = torch.randperm(a.numel(), generator=torch.Generator().manual_seed(0))[:budget].sort().values
        a = a.reshape(-1)[idx]
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "enhanced.npy" if rank == 0 else f"enhanced_rank{rank}.npy"), a.numpy())


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (enhance calls) of the headline loop")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also run every other leg (free-running loop, per-rank times, batch sweep, sustained, ragged sets, "
                         "host enqueue / hipGraph, profiled roofline pass, CPU baseline, weight-broadcast / RCCL report); "
                         "without it only the headline loop runs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the enhanced batch of the last timed step to DIR/enhanced.npy (float32)")
    ap.add_argument("--batch", type=int, default=1, help="utterances per GPU per step (configs[1]: 1)")
    ap.add_argument("--model", default="PP16", choices=["PP16", "OR16", "PP24"])
    ap.add_argument("--n_steps", type=int, default=8, help="diffusion steps")
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--varlen", action="store_true",
                    help="variable-length batch (configs[4]): lengths seconds*U(0.25,2) s, right-zero-padded to the batch "
                         "maximum like the reference's max_collator (datasets/datamodule.py:24-42)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--profile-steps", type=int, default=2, help="(--full) enhance calls of the profiled roofline pass")
    ap.add_argument("--share-devices", action="store_true",
                    help="allow more ranks than visible GPUs (ranks wrap around the devices, gloo rendezvous): "
                         "exercises the N > 1 path on a 1-GPU box; not a scaling measurement")
    ap.add_argument("--force-nccl", action="store_true",
                    help="create the nccl (= RCCL) process group even with ONE rank: communicator set-up, the environment RCCL "
                         "needs and the device-side weight broadcast then execute on a 1-GPU box exactly as on a node")
    ap.add_argument("--sustained-s", type=float, default=10.0,
                    help="(--full) length of the sustained leg (back-to-back free-running enhance calls with the device clock "
                         "and power sampled beside them); 0 = off")
    ap.add_argument("--in-flight", default="4",
                    help="(--full) lanes of the ragged-set leg (32 utterances of 32 different lengths through "
                         "distributed.enhance_sharded, serial loop vs K calls in flight); '' = off")
    ap.add_argument("--option", action="append", default=[], metavar="KEY=VALUE",
                    help="ou_set_option on every model of the run (tuning / A-B runs, e.g. --option split=0 --option no_overlap=1); "
                         "recorded in the line as `options`")
    ap.add_argument("--ragged-batch", default="8,16,32",
                    help="(--full) batch sizes of the ragged-set leg's exact-batching runs (ou_enhance_var); empty: skip")
    ap.add_argument("--batch-sweep", default="1,4,8,16",
                    help="(--full) also time these per-GPU batch sizes (short loops after the main one): one invocation gives the "
                         "utterances/s curve of configs[1] (batch 1) and of the batched throughput mode; '' = off")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-budget", type=float, default=30.0, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def timed_loop(step, steps, world, device):
    """EXACTLY `steps` steps bracketed by barrier + synchronize on both sides; MAX over ranks."""
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = None
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=device if torch.distributed.get_backend() == "nccl" else "cpu")
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tt.item())
    return dt, out


def per_rank_ms(step, steps, world, device):
    """Every rank's OWN time for `steps` steps (no barrier inside), gathered on all ranks: shows stragglers that the
    MAX-over-ranks figure hides."""
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    mine = 1e3 * (time.perf_counter() - t0) / steps
    if world == 1:
        return [mine]
    allv = [None] * world
    torch.distributed.all_gather_object(allv, mine)
    return [float(v) for v in allv]


def main():
    args = parse_args()
    if args.cpu_baseline_only:
        cpu_baseline_worker(args.model, args.n_steps, args.seconds, args.cpu_budget)
        return

    import open_universe_amd  # noqa: F401
    from open_universe_amd import Universe, UniverseGAN
    from open_universe_amd import config as C
    from open_universe_amd import distributed as D
    from open_universe_amd import state_dict as S

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started as plain `python bench.py --gpus N`: become the launcher of N ranks (one process per GPU)
        raise SystemExit(D.respawn_under_launcher(os.path.abspath(__file__), sys.argv[1:], args.gpus))

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback exists for the product path)")
    ndev = torch.cuda.device_count()
    if args.gpus > ndev and not args.share_devices:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but only {ndev} HIP device(s) visible "
                         "(--share-devices runs the ranks on shared GPUs for a functional check)")
    rank, local_rank, world = D.init(backend="nccl" if args.force_nccl else None, force=args.force_nccl)
    host_threads = D.cap_host_threads()  # one process per GPU: the ranks of a node share its host cores
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch exactly one rank per GPU")
    device = D.local_device(local_rank)
    torch.cuda.set_device(device)
    if world > 1:
        assert torch.distributed.get_world_size() == args.gpus
        devs = [None] * world
        torch.distributed.all_gather_object(devs, f"rank{rank}:cuda:{device.index}")
    else:
        devs = [f"rank0:cuda:{device.index}"]

    spec = C.spec_from_config(C.builtin_config(args.model))
    sd = S.synthetic_state_dict(spec, seed=0) if rank == 0 else None
    torch.cuda.synchronize()
    t_b0 = time.perf_counter()
    blob = D.broadcast_packed_weights(spec, sd, device)  # ONE broadcast (RCCL over xGMI); no collective in the loop
    torch.cuda.synchronize()
    t_pack_bcast = time.perf_counter() - t_b0
    bcast = None
    grouped = torch.distributed.is_initialized()
    if grouped and args.full:
        # the collective alone (the first call above also folds / packs on rank 0 and sets the communicator up)
        xb = blob if torch.distributed.get_backend() == "nccl" else blob.cpu()
        torch.distributed.barrier()
        torch.cuda.synchronize()
        t_b0 = time.perf_counter()
        torch.distributed.broadcast(xb, src=0)
        torch.cuda.synchronize()
        t_b = time.perf_counter() - t_b0
        # every rank must hold rank 0's bytes: compare a checksum of the blob across the ranks
        csum = [None] * world
        torch.distributed.all_gather_object(csum, (float(blob.double().sum().item()), int(blob.numel())))
        bcast = {"bytes": int(blob.numel() * 4), "seconds": t_b, "GBs": blob.numel() * 4 / t_b / 1e9,
                 "pack_plus_first_broadcast_s": t_pack_bcast, "identical_on_all_ranks": len(set(csum)) == 1,
                 "backend": torch.distributed.get_backend(), "ranks": world}
    # ranks, distinct physical GPUs (UUIDs), backend -- what a SCALE record has to prove
    rccl = D.rccl_report(device) if args.full else None
    cls = UniverseGAN if spec.kind == "universe_gan" else Universe
    forced = {}
    for kv in args.option:
        k, _, v = kv.partition("=")
        forced[k.strip()] = float(v)
    if forced:
        Universe.set_default_options(**forced)
    model = cls(spec, packed_weights=blob, device=device)

    T = int(args.seconds * spec.fs)
    lens = [T] * args.batch
    if args.varlen:
        g = torch.Generator().manual_seed(5 + rank)
        lens = sorted((int(T * (0.25 + 1.75 * float(u))) for u in torch.rand(args.batch, generator=g)), reverse=True)
        T = lens[0]
    mix = synth_mix(spec.fs, args.batch, T, 1000 + rank * args.batch)
    for i, n in enumerate(lens):
        mix[i, n:] = 0.0  # max_collator: right zero padding, no mask
    mix = mix.to(device)
    audio_s_per_step = sum(lens) / spec.fs
    rng = torch.Generator(device=device).manual_seed(1028282 + rank)

    def step():
        return model.enhance(mix, n_steps=args.n_steps, rng=rng)

    for _ in range(args.warmup):
        step()
    model.check_status = True   # product default: sync + device status word after every enhance
    dt, out = timed_loop(step, args.steps, world, device)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out, rank, world)
    assert torch.isfinite(out).all()
    launches = model.launch_stats()
    if args.full:
        model.check_status = False  # free-running: calls are only enqueued, status checked once afterwards
        dt_async, out = timed_loop(step, args.steps, world, device)
        model.check_status = True
        model._status()
        assert torch.isfinite(out).all()
        rank_ms = per_rank_ms(step, max(2, args.steps // 2), world, device)
    # ---- N > 1: the same loop on rank 0 ALONE (the other ranks wait at a barrier with idle GPUs) -- the one-GPU figure of THIS
    # invocation mode (same process layout, host-thread cap, backend), so that a multi-GPU record describes itself
    solo_ms = None
    if world > 1 and args.full:
        torch.cuda.synchronize()
        torch.distributed.barrier()
        if rank == 0:
            k = max(2, args.steps // 2)
            t0 = time.perf_counter()
            for _ in range(k):
                step()
            torch.cuda.synchronize()
            solo_ms = 1e3 * (time.perf_counter() - t0) / k
        torch.distributed.barrier()

    # ---- other per-GPU batch sizes, same model / length / step count (short loops; every rank takes part) ----
    batch_sweep = {}
    for bs in [int(b) for b in args.batch_sweep.split(",") if b.strip()] if args.full and not args.varlen else []:
        if bs == args.batch:
            batch_sweep[str(bs)] = {"ms_per_step": 1e3 * dt / args.steps,
                                    "utterances_per_s": args.steps * args.batch * world / dt, "steps": args.steps}
            continue
        mix_b = synth_mix(spec.fs, bs, T, 1000 + rank * bs).to(device)
        rng_b = torch.Generator(device=device).manual_seed(1028282 + rank)
        step_b = lambda: model.enhance(mix_b, n_steps=args.n_steps, rng=rng_b)  # noqa: E731
        step_b()
        k = max(3, args.steps // 2)
        dt_b, _ = timed_loop(step_b, k, world, device)
        batch_sweep[str(bs)] = {"ms_per_step": 1e3 * dt_b / k, "utterances_per_s": k * bs * world / dt_b, "steps": k}
    if args.full:
        step()  # back on the headline shape (workspace of the main configuration is current again)

    # ---- sustained rate: >= args.sustained_s of back-to-back free-running calls, per-window rates, sclk / power beside them
    sustained = None
    if args.full and rank == 0 and world == 1 and args.sustained_s > 0 and not args.varlen:
        model.check_status = False
        win = 100
        per_call = dt_async / args.steps
        n_calls = max(2 * win, int(args.sustained_s / per_call / win + 0.999) * win)
        marks = []
        with GpuSampler(device_index=device.index) as smp:
            torch.cuda.synchronize()
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record()
            t0 = time.perf_counter()
            for i in range(n_calls):
                step()
                if (i + 1) % win == 0:  # a window closes on the DEVICE: an event behind its last call
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    marks.append(e)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
        model.check_status = True
        model._status(force=True)
        ends = [ev0.elapsed_time(e) * 1e-3 for e in marks]
        wins = [ends[0]] + [ends[i] - ends[i - 1] for i in range(1, len(ends))]
        rates = [win * args.batch / w for w in wins]
        sustained = {"seconds": total, "calls": n_calls, "ms_per_step": 1e3 * total / n_calls,
                     "utterances_per_s": n_calls * args.batch / total, "window_calls": win,
                     "window_utterances_per_s": {"min": min(rates), "max": max(rates), "first": rates[0], "last": rates[-1]},
                     "vs_short_loop": (n_calls * args.batch / total) / (args.steps * args.batch / dt_async),
                     "device": smp.summary(),
                     "note": "free-running calls (no host sync inside the loop) for >= --sustained-s seconds; windows are closed by "
                             "events on the stream (device time); vs_short_loop = this rate / the free-running rate of the "
                             "--steps loop above; `device` = sclk / power of THIS GPU's sysfs card sampled beside the loop"}

    # ---- ragged utterance sets (the reference CLI's real workload): serial loop vs K calls in flight (lanes) -------------
    in_flight = None
    if args.full and rank == 0 and world == 1 and args.in_flight.strip() and not args.varlen and args.batch == 1:
        n_utt = 32
        gl = torch.Generator().manual_seed(17)
        lens = set()
        while len(lens) < n_utt:
            lens.add(int(spec.fs * args.seconds * (0.875 + 0.125 * float(torch.rand(1, generator=gl)))))
        lens = sorted(lens)
        lens = [lens[i] for i in torch.randperm(n_utt, generator=gl).tolist()]
        sigs = [synth_mix(spec.fs, 1, n, 2000 + i)[0].to(device) for i, n in enumerate(lens)]

        def rate(k):
            best = None
            for _ in range(2):  # (the first pass creates the lanes and their workspaces)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                o = D.enhance_sharded(model, sigs, seed=3, gather=False, in_flight=k, n_steps=args.n_steps)
                torch.cuda.synchronize()
                best = time.perf_counter() - t0
            return best, o

        t1, ref = rate(1)
        in_flight = {"utterances": n_utt, "lengths_s": [min(lens) / spec.fs, max(lens) / spec.fs], "all_lengths_different": True,
                     "serial": {"utterances_per_s": n_utt / t1, "ms_per_utterance": 1e3 * t1 / n_utt}}
        for k in [int(v) for v in args.in_flight.split(",") if v.strip()]:
            tk, ok_ = rate(k)
            in_flight[f"lanes_{k}"] = {"utterances_per_s": n_utt / tk, "ms_per_utterance": 1e3 * tk / n_utt,
                                       "real_time_factor": sum(lens) / spec.fs / tk,
                                       "bit_identical_to_serial": all(torch.equal(ref[i], ok_[i]) for i in ref)}
        # ... and the same set through EXACT batching (ou_enhance_var: every row keeps its own padding, statistics, conv zero
        # padding and GRU length -- the result of the file-by-file loop to fp32 round-off, at the batched kernels' rate)
        def snr_db(a, b):
            a, b = a.double(), b.double()
            return float(10 * torch.log10(a.square().sum() / (a - b).square().sum().clamp(min=1e-300)))

        for bs in [int(v) for v in args.ragged_batch.split(",") if v.strip()]:
            best, ob = None, None
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ob = D.enhance_sharded(model, sigs, seed=3, gather=False, batch_size=bs, n_steps=args.n_steps)
                torch.cuda.synchronize()
                best = time.perf_counter() - t0
            in_flight[f"exact_batch_{bs}"] = {"utterances_per_s": n_utt / best, "ms_per_utterance": 1e3 * best / n_utt,
                                              "real_time_factor": sum(lens) / spec.fs / best,
                                              "worst_row_snr_db_vs_serial": min(snr_db(ref[i], ob[i]) for i in ref)}
        in_flight["note"] = ("distributed.enhance_sharded on ONE GPU, 32 utterances of 32 different lengths: one call at a time vs K "
                             "calls in flight on K streams (open_universe_amd/lanes.py; every call the same launches as in the "
                             "serial loop) vs exact batching with per-row lengths (exact_batch_N: N utterances per ou_enhance_var "
                             "call, length-sorted neighbours; same per-utterance generators, plain SNR of the worst row against "
                             "the serial loop's output)")
        step()

    # ---- host side: time to ENQUEUE one enhance (no sync), eager walk of the network vs one hipGraph replay ----
    host_enqueue = None
    if args.full and rank == 0 and not args.varlen:
        model.check_status = False

        def enqueue_ms(fn, reps=10):
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            ts.sort()
            return 1e3 * ts[len(ts) // 2]

        host_enqueue = {"eager_ms": enqueue_ms(step)}

        def loop_ms(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / args.steps

        try:
            # the capturable form: one chain on one stream (OU_ENH_SERIAL); and, for the record, the eager call's own
            # fork / join structure captured as it is
            run = model.graphed_enhance(args.batch, T, n_steps=args.n_steps, serial=True)
            run(mix, rng=rng)
            host_enqueue["hipgraph_ms"] = enqueue_ms(lambda: run(mix, rng=rng))
            host_enqueue["hipgraph_ms_per_step"] = loop_ms(lambda: run(mix, rng=rng))
            run_fj = model.graphed_enhance(args.batch, T, n_steps=args.n_steps, serial=False)
            run_fj(mix, rng=rng)
            host_enqueue["hipgraph_forkjoin_ms_per_step"] = loop_ms(lambda: run_fj(mix, rng=rng))
            host_enqueue["note"] = ("eager_ms / hipgraph_ms: median host time of one enhance call returning without a sync (eager = "
                                    "Python + C walk of the network, ~400 launches; hipgraph = noise draws + one replay).  "
                                    "*_ms_per_step: free-running loops of args.steps calls.  hipgraph = the serial chain "
                                    "(OU_ENH_SERIAL) captured; hipgraph_forkjoin = the eager call's three side streams captured "
                                    "as graph edges -- slower than the chain, which is why graphed_enhance captures the chain")
        except Exception as e:  # capture support is a convenience, never the measured path
            host_enqueue["hipgraph_error"] = repr(e)[:300]
        model.check_status = True
        model._status(force=True)

    # ---- roofline of the dominant kernel: per-launch device-side timing (separate profiled pass, same workload) ----
    roofline = None
    if args.full and rank == 0:
        model.check_status = False
        model.profile(True)
        for _ in range(max(1, args.profile_steps)):
            step()
        torch.cuda.synchronize()
        recs = model.profile_read(max_records=32768)
        model.profile(False)
        # records: (ms, algorithmic flops, algorithmic bytes, variant); variant < 40: conv_mfma_kernel tile configs,
        # 40-49: rate_down_kernel,
        # 66 / 76 / 67 / 77: conv_direct2_kernel, 400 + 10 WK + KW: conv_direct2w_kernel, 600 / 700 + 10 TM + KW: conv_direct4w_kernel, other 50-99: conv_direct_kernel / conv_direct_strided_kernel variants,
        # 100-199: conv_chain_kernel (fused ConvBlock body), 200-299: conv_direct3_kernel (2xx: 200 + 10 TM + KW) /
        # conv_direct3s_kernel (260 + R), 500-599: conv_direct3w_kernel (500 + 10 TM + KW), 300-399: conv_direct4_kernel (300 + 10 TM + log2 WK), >= 1000: one GRU pass
        # (1000 + steps).
        gru_recs = [r for r in recs if r[3] >= 1000]
        recs = [r for r in recs if r[3] < 1000]
        split_launches = sum(1 for r in recs if 800 <= r[3] < 1000)  # conv_split_kernel launches of the timed configuration
        def executed_fraction(cfg):
            """MFMA multiply-adds a launch issues / its algorithmic ones: the minimal-filtering kernels (F(2, KW): KW + 1 products
            per pair of outputs instead of 2 KW) carry KW in their variant code."""
            if 400 <= cfg < 800:
                kw = cfg % 10
                return (kw + 1) / (2.0 * kw)
            if 800 <= cfg < 1000:  # conv_split_kernel: nothing on the f32 pipe (six bf16 products per MAC on the bf16 pipe)
                return 0.0
            if cfg == 193:  # conv_chainw_kernel, depth 3: k5, k3, k3
                return 14 / 22.0
            if cfg == 192:  # depth 2: k3, k3
                return 8 / 12.0
            return 1.0

        def summarise(rr):
            if not rr:
                return None
            ms_ = sum(r[0] for r in rr)
            fl_ = sum(r[1] for r in rr)
            by_ = sum(r[2] for r in rr)
            ex_ = sum(r[1] * executed_fraction(r[3]) for r in rr)
            bx_ = sum(r[1] * 6.0 for r in rr if 800 <= r[3] < 1000)
            return {"launches": len(rr) // max(1, args.profile_steps), "avg_launch_us": 1e3 * ms_ / len(rr),
                    "ms_per_enhance": ms_ / max(1, args.profile_steps),
                    "algorithmic_gflop_per_enhance": fl_ / max(1, args.profile_steps) / 1e9,
                    "algorithmic_GB_per_enhance": by_ / max(1, args.profile_steps) / 1e9,
                    "tflops": fl_ / (ms_ * 1e-3) / 1e12, "gbs": by_ / (ms_ * 1e-3) / 1e9,
                    "executed_tflops": ex_ / (ms_ * 1e-3) / 1e12,
                    "bf16_pipe_tflops": bx_ / (ms_ * 1e-3) / 1e12,
                    "algorithmic_bytes_per_launch": by_ / len(rr)}
        KERNELS = {
            "direct2": "ou::conv_direct2_kernel / conv_direct2w_kernel (register-direct split-K fp32-MFMA Conv1d, wide operand loads: "
                       "k3 / k5 layers; the w forms with minimal filtering F(2, 3) / F(2, 5): conv_direct2w_kernel on 64-column tiles, "
                       "conv_direct4w_kernel on 16 / 32-row tiles for the 401-frame levels)",
            "direct": "ou::conv_direct_kernel / conv_direct_strided_kernel (first-generation register-direct split-K, dword "
                      "operand loads: 1x1, phase-GEMM and rate-change convs of the 401-frame levels at batch 1 - 2)",
            "direct4": "ou::conv_direct4_kernel (wide-load split-K: 1x1, phase-GEMM and rate-change convs; 16x16x4 fp32 MFMA, "
                       "16-byte operand loads, LDS-staged epilogue with 16-byte stores)",
            "lds": "ou::conv_mfma_kernel (LDS-tiled fp32-MFMA implicit-GEMM Conv1d, wide levels / strided convs)",
            "rate": "ou::rate_down_kernel / rate_up_kernel (outermost rate-change convs with the anti-alias FIR fused, K = 64)",
            "chain": "ou::conv_chain_kernel (fused ConvBlock body, C = 32 / 64 levels)",
            "split": "ou::conv_split_kernel (stride-1 k3 / k5 convs on the BF16 matrix pipe: every fp32 operand as three bf16 pieces, "
                     "six piece products per fp32 product on v_mfma_f32_32x32x16_bf16, fp32 accumulate; 64 x 64 / 64 x 128 wave tiles, "
                     "activations split on the fly into LDS, weights pre-split as A fragments)",
            "direct3": "ou::conv_direct3_kernel / conv_direct3w_kernel / conv_direct3s_kernel (no-split-K throughput kernels: one "
                       "(16 TM) x 64 tile per wave over the whole reduction, 16x16x4 fp32 MFMA, register-direct operands, stores from "
                       "the accumulators; the w form with minimal filtering F(2, 3) / F(2, 5))",
        }
        # conv_direct2_kernel (8 / 4 K slices), its minimal-filtering form conv_direct2w_kernel, and conv_direct4w_kernel
        # (6xx / 7xx: the same layers on 16 / 32-row tiles where there are few columns)
        D2 = (66, 76, 67, 77) + tuple(range(400, 500)) + tuple(range(600, 800))
        groups = {"direct2": summarise([r for r in recs if r[3] in D2]),
                  "direct": summarise([r for r in recs if 50 <= r[3] < 100 and r[3] not in D2]),
                  "lds": summarise([r for r in recs if r[3] < 40]),
                  "rate": summarise([r for r in recs if 40 <= r[3] < 50]),
                  "chain": summarise([r for r in recs if 100 <= r[3] < 200]),
                  "direct3": summarise([r for r in recs if 200 <= r[3] < 300 or 500 <= r[3] < 600]),
                  "direct4": summarise([r for r in recs if 300 <= r[3] < 400]),
                  "split": summarise([r for r in recs if 800 <= r[3] < 1000])}
        groups = {k: v for k, v in groups.items() if v}
        fam = summarise([r for r in recs if (50 <= r[3] < 100 and r[3] not in D2) or 300 <= r[3] < 400 or 260 <= r[3] < 270])
        dom = max(groups, key=lambda k: groups[k]["ms_per_enhance"])  # the dominant kernel = most time per enhance
        gen = groups[dom]
        allconv = summarise(list(recs))
        traffic, traffic_note = None, "not collected (PMC passes are separate rocprofv3 runs)"
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        cfg_tag = f"{args.model}_b{args.batch}" + ("_varlen" if args.varlen else "") + (f"_n{args.n_steps}" if args.n_steps != 8 else "")
        if os.path.exists(tpath):
            with open(tpath) as f:
                tj = json.load(f)
            ent = tj.get("configs", {}).get(cfg_tag)
            if ent is not None:
                traffic = ent.get(dom + "_bytes_per_launch")
                traffic_note = (f"STATIC: copied from profiles/pmc_traffic.json [{cfg_tag}] -- separate rocprofv3 --pmc FETCH_SIZE / "
                                "WRITE_SIZE passes of this command, collected by tools/round_profile.sh in the evidence run of the "
                                "round on the box of the committed profiles/rNN_final_* files (profiles/rNN_final_box_health.txt); "
                                "not measured in THIS run: PMC passes need rocprofv3 around the process. "
                                + tj.get("note", ""))

        # whole score-network forward (the unit of work of SURVEY 8(d)): HIP events on the launch stream around
        # K calls of the operator seam score_model(x, sigma | cond)
        xin = torch.randn(args.batch, 1, T + (spec.tot_ds - T % spec.tot_ds), device=device)
        model.condition_model(xin)
        sig = torch.full((args.batch,), 0.5)
        for _ in range(2):
            model.score_model(xin, sig)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        K = 10
        e0.record()
        for _ in range(K):
            model.score_model(xin, sig)
        e1.record()
        torch.cuda.synchronize()
        fwd_ms = e0.elapsed_time(e1) / K
        gf, act_mb, w_mb = SCORE_FORWARD_WORK[args.model]
        scale = xin.shape[-1] / (4.0 * spec.fs + spec.tot_ds)
        fwd_flop = gf * 1e9 * scale * args.batch
        fwd_bytes = (act_mb * scale * args.batch + w_mb) * 1e6
        score_forward = {
            "ms": fwd_ms, "batch": args.batch,
            "algorithmic_gflop": fwd_flop / 1e9, "algorithmic_MB": fwd_bytes / 1e6,
            "compute_view": {"achieved_TFLOPs": fwd_flop / (fwd_ms * 1e-3) / 1e12, "peak": FP32_MFMA_PEAK_TFLOPS,
                             "frac": fwd_flop / (fwd_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS},
            "hbm_view": {"achieved_GBs": fwd_bytes / (fwd_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS,
                         "frac": fwd_bytes / (fwd_ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
            "method": f"HIP events on the launch stream around {K} score_model(x, sigma) calls (all launches of one "
                      "forward incl. the GRU pass, sigma embedding and FiLM table)",
        }
        roofline = {
            "kernel": KERNELS[dom],
            "bound": "mfma",
            "achieved": gen["tflops"],
            "peak": FP32_MFMA_PEAK_TFLOPS,
            "unit": "TFLOP/s",
            "frac": gen["tflops"] / FP32_MFMA_PEAK_TFLOPS,
            "executed": {"tflops": gen["executed_tflops"], "frac_of_peak": gen["executed_tflops"] / FP32_MFMA_PEAK_TFLOPS,
                         "note": "achieved / frac count ALGORITHMIC FLOPs (2 M Cin KW Nq per launch, SURVEY.md 8(d)); the "
                                 "minimal-filtering kernels (Winograd / Cook-Toom F(2, 3), F(2, 5): conv_direct2w / 3w / 4w, "
                                 "conv_chainw) issue 2/3 (k3) and 3/5 (k5) of them on the matrix pipe -- `executed` is what the "
                                 "pipe actually ran, the figure that cannot exceed its 157.3 TFLOP/s; conv_split_kernel runs on the "
                                 "BF16 pipe instead (six bf16 products per fp32 product: `bf16_pipe_tflops` = 6 x algorithmic, "
                                 "against 2 500 dense) and may exceed 157.3 algorithmic"},
            "traffic": traffic,
            "traffic_note": traffic_note,
            "launches": gen["launches"],
            "avg_launch_us": gen["avg_launch_us"],
            "algorithmic_bytes_per_launch": gen["algorithmic_bytes_per_launch"],
            "algorithmic_gflop_per_enhance": gen["algorithmic_gflop_per_enhance"],
            "conv_ms_per_enhance": gen["ms_per_enhance"],
            "hbm_view": {"achieved_GBs": gen["gbs"], "peak_GBs": HBM_PEAK_GBS, "frac": gen["gbs"] / HBM_PEAK_GBS,
                         "algorithmic_GB_per_enhance": gen["algorithmic_GB_per_enhance"]},
            "other_conv_kernels": {KERNELS[k]: {
                "achieved": v["tflops"], "frac": v["tflops"] / FP32_MFMA_PEAK_TFLOPS, "launches": v["launches"],
                "executed_tflops": v["executed_tflops"], "bf16_pipe_tflops": v["bf16_pipe_tflops"],
                "avg_launch_us": v["avg_launch_us"], "ms_per_enhance": v["ms_per_enhance"],
                "algorithmic_gflop_per_enhance": v["algorithmic_gflop_per_enhance"]} for k, v in groups.items() if k != dom},
            "all_conv_kernels": {"achieved": allconv["tflops"], "frac": allconv["tflops"] / FP32_MFMA_PEAK_TFLOPS,
                                 "executed_tflops": allconv["executed_tflops"],
                                 "launches": allconv["launches"], "ms_per_enhance": allconv["ms_per_enhance"],
                                 "algorithmic_gflop_per_enhance": allconv["algorithmic_gflop_per_enhance"]},
            "pointwise_family": None if not fam else {
                "what": "the 1x1 / phase-GEMM / rate-change convs, whichever kernel took them (conv_direct_kernel, "
                        "conv_direct_strided_kernel, conv_direct3s_kernel, conv_direct4_kernel)",
                "achieved": fam["tflops"], "frac": fam["tflops"] / FP32_MFMA_PEAK_TFLOPS, "launches": fam["launches"],
                "avg_launch_us": fam["avg_launch_us"], "ms_per_enhance": fam["ms_per_enhance"]},
            "gru": gru_roofline(gru_recs, args, 1e3 * dt / args.steps),
            "score_forward": score_forward,
            "method": f"device-side per-launch timing (first block start .. last block end on the 100 MHz s_memrealtime clock) of every conv launch, profiled pass of {args.profile_steps} "
                      "enhance calls right after the timed region, in the SAME mode as the timed calls (side streams inside the call: the "
                      "launches of the first score-encoder pass run beside the conditioner's and are timed as they run there; "
                      "profiles/*kstats*_serial.txt has the rocprofv3 averages of the same command as one serial chain); algorithmic FLOPs/bytes = reference (un-folded) "
                      "layer-granular accounting, SURVEY.md 8(d)",
        }

    if rank == 0:
        audio_s = args.steps * audio_s_per_step * world
        what = {"PP16": "UNIVERSE++ 16 kHz", "OR16": "UNIVERSE (original) 16 kHz", "PP24": "UNIVERSE++ 24 kHz"}[args.model]
        res = {
            "metric": f"real_time_factor (audio s / wall s), {what} {args.n_steps}-step enhance",
            "value": audio_s / dt,
            "unit": "x_realtime",
            "utterances_per_s": args.steps * args.batch * world / dt,
            "utterances_per_s_per_gpu": args.steps * args.batch / dt,
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic (seeded AM-sine + noise waveforms; seeded random weights with the reference key schema)",
            "config": {
                "workload": f"{what}, {args.n_steps} diffusion steps, batch={args.batch} utterance(s) of "
                            + (f"{min(lens)/spec.fs:.1f}-{max(lens)/spec.fs:.1f} s (variable length, right-zero-padded)"
                               if args.varlen else f"{args.seconds:.0f} s") + " per GPU per step",
                "network": args.model,  # PP16 = UNIVERSE++ 16 kHz, OR16 = UNIVERSE 16 kHz, PP24 = UNIVERSE++ 24 kHz
                "n_diffusion_steps": args.n_steps,
                "batch_per_gpu": args.batch,
                "samples_per_utterance": T,
                "parallelism": "utterances sharded across GPUs; packed weights broadcast once over RCCL; "
                               "no collective in the sampling loop",
                "devices": devs,
                "backend": torch.distributed.get_backend() if grouped else None,
                "launches_per_enhance": launches[0],
            },
            "options": {"forced": forced, "note": "ou_set_option values that differ from the defaults in this run (--option); the "
                                                  "library reads no environment variable"},
            "host_threads_per_rank": host_threads,
            "status_mode": "value / ms_per_step: product default (stream sync + device status read after every enhance)",
        }
        if args.full:
            res.update({
                "rank0_alone": None if solo_ms is None else {
                    "ms_per_step": solo_ms, "utterances_per_s": 1e3 * args.batch / solo_ms,
                    "per_gpu_rate_vs_rank0_alone": (args.steps * args.batch / dt) / (1e3 * args.batch / solo_ms),
                    "note": "the same loop on rank 0 while the other ranks wait at a barrier (their GPUs idle), same process layout "
                            "and host-thread cap: the one-GPU figure of this invocation mode; the ratio is the per-GPU rate of the "
                            "N-rank loop (MAX over ranks) over it"},
                "bf16_split_launches_per_enhance": split_launches // max(1, args.profile_steps),
                "dtype_note": "fp32 tensors and fp32 accumulation everywhere; the timed configuration (batch %d; from the kernel variants "
                              "recorded in the profiled pass) runs %s" % (
                    args.batch, "some of its k3 / k5 convs of the 256- / 512-channel levels on the BF16 matrix pipe with every fp32 operand as three "
                    "bf16 pieces and six piece products per fp32 product (conv_split_kernel, DESIGN.md 4.1f: fp32-class accuracy, measured "
                    "1 dB better than an fp32 fmaf chain against a double evaluation; option split = 0 keeps everything on the f32 MFMAs)"
                    if split_launches else
                    "every convolution on the f32-input MFMAs (exact fp32 products); from batch 16 -- the '16' entry of batch_sweep -- the "
                    "256- / 512-channel k3 / k5 convs go to conv_split_kernel (three bf16 pieces per fp32 operand on the BF16 pipe, "
                    "fp32-class accuracy, DESIGN.md 4.1f)"),
                "per_rank_ms_per_step": rank_ms,
                "rccl": rccl,
                "weight_broadcast": bcast,
                "batch_sweep": dict(batch_sweep, note="utterances/s of the whole job at other per-GPU batch sizes (same model, "
                                                      "length and step count; MAX over ranks like the headline)"),
                "free_running": {"value": audio_s / dt_async, "ms_per_step": 1e3 * dt_async / args.steps,
                                 "note": "model.check_status = False: no host sync inside the timed loop, status checked after it"},
                "host_enqueue": host_enqueue,
                "sustained": sustained,
                "in_flight": in_flight,
                "gru_exchange": dict(model.gru_exchange_stats(),
                                     note="hand-offs the GRU clusters had to repeat / waves that finished a pass with "
                                          "system-scope publishes (DESIGN.md 4.4), whole process; both 0 on a healthy device"),
                "roofline": roofline,
            })
            if not args.no_cpu_baseline:
                res["cpu_baseline"] = cpu_baseline(args.model, args.n_steps, args.seconds)
        print(json.dumps(res), flush=True)
    if grouped:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
