"""float64 definitions of the segmented-enhance operations (ou_segment.hip) for the tests, and the checks built on them.

Written from the definitions, not from the kernels: the segment plan and the crossfade of include/ouniverse.h (window k writes
[w_k, w_{k+1}) of the padded row, w_0 = 0, w_k = e_{k-1} - O, w_n = T_pad; on [w_k, e_{k-1}) it carries the weight
a(i) = 0.5 - 0.5 cos(pi (i + 0.5) / O) and the window in front 1 - a(i)), the pad split and the post step of universe.py as
DESIGN 4.9 / 4.17 restate them (pad = tot_ds - T % tot_ds, pad // 2 in front; statistics over the PADDED row; keep_rms and the
peak guard over the RAW row), utils/norm.py through tests/norm_cases.py.  pad_normalize, post, mel and mel_scale of
tests/small_fp64.py are reused with their `Report` / `ulp32`.

Every check takes the kernel's inputs from the GPU's own taps (teacher-forced), evaluates in float64, holds every element
against its bound and excludes none.  Bounds (kinds as in tests/small_fp64.py; u = 2^-24):

* statistics   the sums are double on the device: n 2^-52 relative.  mean, mix_rms: one rounding (the 1/2 ulp).  gain:
               norm_cases.stats_bounds (rounded mean, fl(x - mean), (float) sd, the division).  Fourth word: == 0.
* row scale    the frame energies of the whole normalised row: small_fp64.mel's chain bound with two more roundings per product
               (x - mean and * gain happen on the fly; the reference normalises unrounded), propagated to first order through
               sum mel^2, then small_fp64.mel_scale's statistic bound.
* gather       (x - mean) * gain: fl(x - mean) then one product: u (1 + u) |d g| + 1/2 ulp; exactly 0 behind the entry's length.
               Outside the raw row x is the 0 of the pad split.
* noise        exact copy, exactly 0 behind the entry's length.
* stitch       outside a crossfade an exact copy.  Inside: |d a| (|y_prev| + |y|) + u |1 - a| |y_prev| (the rounding of 1 - a)
               + u |(1 - a) y_prev| + u |a y| (the two products) + 1/2 ulp (the add).  d a = M_WEIGHT x e32, e32 = max |fp32 torch
               evaluation of a(i) - float64| over the ramp (the `library` kind: cosf).
* post         small_fp64.post on the stitched rows (the output of the identical call with keep_rms off and an idle guard).

The fp32 restatements (`*_fp32`, kernel order of operations, with the mutation switches `mut`) exist for
tests/test_seg_fp64_cpu.py: they pass every check, every mutant fails its own."""
import math

import numpy as np
import torch

import norm_cases as K
import small_fp64 as F
from open_universe_amd import _lib

U = F.U
# M of the crossfade weight = the next integer above twice the worst err / e32 over the cases of tests/test_gpu_seg_fp64.py
# (profiles/seg_fp64_observed.json, `lib_ratio`; err = what is left of |gpu - f64| after the final 1/2 ulp, over e32 (|y_prev| + |y|),
# so it still carries the three roundings of the blend: an upper estimate of the weight's own share).  Measured on an MI355X over
# the 34 cases with a stitch: 0.963 (PP16s, 58 tot_ds + 3 samples, O = 2 tot_ds, e32 = 1.30e-7) -> M = 2.
M_WEIGHT = 2
SENTINEL = 7.0  # what a destination word holds before the stitch in the restatement (the kernels find frame energies there)


# ---- geometry ---------------------------------------------------------------------------------------------------------------
class Row:
    """One long row of t_raw samples cut into windows of S with overlap O (samples; multiples of tot_ds)."""

    def __init__(self, t_raw, td, S, O):
        pad = td - t_raw % td
        self.t_raw, self.T_pad, self.pad_left, self.td = int(t_raw), int(t_raw + pad), int(pad // 2), td
        self.S_asked, self.O_asked = S, O
        p = _lib.segment_plan(td, t_raw, S, O)
        assert p["T_pad"] == self.T_pad
        self.starts = [int(v) for v in p["starts"]]
        self.n_win = len(self.starts)
        self.L = int(p["lengths"][0])
        self.O = int(p["overlap"])
        self.hop = self.L - self.O

    def window(self, k, mut=()):
        """-> (s, s_prev, w0, w1, e_prev) of window k in padded-row positions."""
        L, O, s = self.L, self.O, list(self.starts)
        if "no_shift" in mut:
            s[-1] = (self.n_win - 1) * self.hop
        sk, sp = s[k], (s[k - 1] if k else 0)
        w0 = 0 if k == 0 else sp + L - O
        w1 = self.T_pad if k == self.n_win - 1 else sk + L - O
        e_prev = 0 if k == 0 else sp + L
        if "w0_off" in mut and k:
            w0 += 1
        return sk, sp, w0, w1, e_prev

    def padded(self, x, dtype=torch.float64):
        xp = torch.zeros(self.T_pad, dtype=dtype)
        xp[self.pad_left: self.pad_left + self.t_raw] = x.reshape(-1)[: self.t_raw].to(dtype)
        return xp


def groups_alike(C, n_win, max_batch):
    """The groups of a call on C rows alike: entries (row, window) row-major, spread evenly over ceil(n / max_batch) groups.
    -> (Bw, [[(row, win)] per group])"""
    n = C * n_win
    g = -(-n // max_batch)
    Bw = -(-n // g)
    ents = [(c, k) for c in range(C) for k in range(n_win)]
    return Bw, [ents[i: i + Bw] for i in range(0, n, Bw)]


def groups_ragged(rows, td, S, O, max_batch):
    """ou_segment_groups for rows of their own lengths: -> (Bw, [[(row, win)] per group], [group is of class FULL])."""
    G = _lib.segment_groups(td, [r.t_raw for r in rows], S, O, max_batch)
    n_full = sum(r.n_win for r in rows if r.n_win > 1)
    ents = list(zip((int(v) for v in G["row"]), (int(v) for v in G["window"])))
    first = [int(v) for v in G["group_first"]]
    out, full = [], []
    for i, e0 in enumerate(first):
        is_full = e0 < n_full
        e1 = min(e0 + G["batch"], n_full if is_full else len(ents))
        out.append(ents[e0:e1])
        full.append(is_full)
    return int(G["batch"]), out, full


def last_group(geos, max_batch, ragged, E=1):
    """The group whose rows the taps hold after a call: -> (Bw, its real entries, all Bw slots (the fillers repeat the last real
    entry), the number of groups, T of its walk)."""
    if ragged:
        g0 = geos[0]
        Bw, groups, _ = groups_ragged(geos, g0.td, g0.S_asked, g0.O_asked, max_batch // E)
    else:
        Bw, groups = groups_alike(len(geos), geos[0].n_win, max_batch // E)
    real = groups[-1]
    return Bw, real, real + [real[-1]] * (Bw - len(real)), len(groups), max(geos[c].L for c, _ in real)


def weight(i, O, dtype=torch.float64, mut=()):
    """a(i) = 0.5 - 0.5 cos(pi (i + 0.5) / O); dtype float32: every operation rounded once, in that order."""
    i = torch.as_tensor(i).to(dtype)
    half, pi = torch.tensor(0.5, dtype=dtype), torch.tensor(math.pi, dtype=dtype)
    den = torch.tensor(float(O + 1 if "fade_plus1" in mut else O), dtype=dtype)
    arg = i if "no_half" in mut else i + half
    return half - half * torch.cos(pi * arg / den)


def weight_e32(O):
    i = torch.arange(O)
    return float((weight(i, O, torch.float32).double() - weight(i, O)).abs().max())


def dest_head(addr_words):
    """Words in front of the first 16-byte boundary of a destination that starts `addr_words` floats behind an aligned base."""
    return (4 - addr_words % 4) % 4


# ---- the case lists of the GPU tests -------------------------------------------------------------------------------------------
MODELS = ("PP16s", "PP24s")


def seg_so(td):
    return 16 * td, 2 * td


def lengths(td):
    return [1, 3, 16 * td - 1, 16 * td, 32 * td, 41 * td + 7, 30 * td + 2, 44 * td + 1, 58 * td + 3, 37 * td + 5]


def ragged_lengths(td):
    return [41 * td + 7, 9 * td, 57, 16 * td - 1, 16 * td, 70 * td + 3]


def ragged_multi(td):
    return [41 * td + 7, 16 * td, 70 * td + 3]


OVERLAP_EDGES = ("0", "S/2")      # with the length 58 td + 3: 4 and 7 windows
CARRY_LENGTH = lambda td: 58 * td + 3  # noqa: E731  (max_batch 4: groups of 4, 4, 2 entries; the last starts at row 1, window 3)
MULTI_BLOCK_ALIKE = 2 ** 18 + 5
MULTI_BLOCK_RAGGED = [2 ** 18 + 5, 57, 3 * 2 ** 18 - 1]
NORM_MODES = [(n, z) for n in ("2", "max", "2-max") for z in (True, False)]
DC = 0.02
LOUD, QUIET = 60.0, 0.06  # row 0 and row 1 of a case: 1e-3 apart; the loud one makes the peak guard divide under keep_rms


def case_mix(spec, lens, seed=0):
    """Rows of the given lengths: synth_mix on a DC offset, row 0 x LOUD, the others x QUIET."""
    from helpers import synth_mix

    rows = []
    for i, n in enumerate(lens):
        x = synth_mix(spec, 1, n, seed=7000 + seed + i)[0] + DC
        rows.append(x * (LOUD if i == 0 else QUIET))
    return rows


def coverage(td, C=2):
    """What the one-group lengths reach, from the lengths alone: residues of t_raw and pad_left modulo 4 and the stitch's
    destination heads (row c of the (C, t_raw) output starts c t_raw words behind its aligned base)."""
    S, O = seg_so(td)
    t4, p4, heads, wins = set(), set(), set(), set()
    for n in lengths(td):
        r = Row(n, td, S, O)
        t4.add(n % 4)
        p4.add(r.pad_left % 4)
        wins.add(r.n_win)
        for c in range(C):
            for k in range(r.n_win):
                _, _, w0, w1, _ = r.window(k)
                u0, u1 = max(w0, r.pad_left), min(w1, r.pad_left + r.t_raw)
                if u1 > u0:
                    heads.add(dest_head(c * n + u0 - r.pad_left))
    return t4, p4, heads, wins


# ---- statistics ------------------------------------------------------------------------------------------------------------
def check_stats(stats, mix_rows, td, level_db, norm="2", zero_mean=True, eps=1e-5, name="seg.stats"):
    """stats (C, 4) of the device against {mean removed, gain, mix_rms, 0} of every row in float64."""
    C = len(mix_rows)
    ref, bound = torch.zeros(C, 4, dtype=torch.float64), torch.zeros(C, 4, dtype=torch.float64)
    for c, x in enumerate(mix_rows):
        n = x.numel()
        xp = K.padded(x.double(), td)
        st = K.norm_stats(xp, norm, level_db, zero_mean, eps)
        _, rho = K.stats_bounds(xp, st, norm, zero_mean)
        dsum = xp.numel() * 2.0 ** -52
        rms = math.sqrt(float(x.double().square().mean()))
        ref[c] = torch.tensor([st["mean"], st["gain"], rms, 0.0], dtype=torch.float64)
        bound[c] = torch.tensor([dsum * abs(st["mean"]) if zero_mean else 0.0, rho * st["gain"], max(dsum * rms, 1e-300), 0.0])
        assert n >= 1
    return F.Report(name, stats.reshape(C, 4), ref, bound)


def stats_fp32(x, td, level_db, norm="2", zero_mean=True, eps=1e-5, mut=()):
    """The device's order in numpy: double sums, (float) mean over T_pad, sum of fl(x - mean)^2 plus the padding's term, (float)
    sd unbiased, the gain in fp32.  -> [mean removed, gain, mix_rms, 0] (float32)."""
    f = np.float32
    xr = x.numpy().astype(np.float32)
    n = xr.size
    pad = td - n % td
    Tp = n + pad
    s, sq = xr.astype(np.float64).sum(), (xr.astype(np.float64) ** 2).sum()
    mean = f(s / (n if "mean_traw" in mut else Tp))
    d = (xr - mean).astype(np.float64)
    ss = (d * d).sum()
    if "no_pad_term" not in mut:
        ss += (Tp - n) * float(f(0) - mean) ** 2
    sd = f(math.sqrt(ss / (Tp if "biased" in mut else Tp - 1)))
    mu = mean if zero_mean else f(0)
    mx = np.abs(xr - mu).max()
    if Tp > n:
        mx = max(mx, abs(f(0) - mu))
    gain = K.gain32(norm, level_db, sd, mx, eps)
    return torch.tensor(np.array([mu, gain, f(math.sqrt(sq / n)), 0], dtype=np.float32))


# ---- whole-row mel scale --------------------------------------------------------------------------------------------------------
def row_scale(x, geo, mean, gain, P, dtype=torch.float64):
    """1 / max(sqrt(mean over the frames of sum_m mel^2), 1e-5) of the whole normalised padded row.  -> (scale, bound)"""
    xn = ((geo.padded(x, dtype) - torch.tensor(float(mean), dtype=dtype)) * torch.tensor(float(gain), dtype=dtype))[None, None, :]
    mel, b = F.mel(xn, P, dtype)
    if dtype != torch.float64:
        e = (mel * mel).sum(1)  # (1, L)
        return 1.0 / max(math.sqrt(float(e.double().sum()) / e.shape[-1]), 1e-5), None
    b = b * ((P.n_fft + 5) / (P.n_fft + 3))  # the two roundings of the normalisation on the fly, per product
    ref, stat = F.mel_scale(mel)
    tot = float(mel.pow(2).sum())
    rel = float((mel.abs() * b).sum()) / max(tot, 1e-300)
    return float(ref), float(stat) + float(ref) * rel


def check_row_scale(scale, mix_rows, geos, stats, P, name="seg.row_scale"):
    C = len(mix_rows)
    ref, bound = torch.zeros(C, 1, dtype=torch.float64), torch.zeros(C, 1, dtype=torch.float64)
    for c in range(C):
        ref[c, 0], bound[c, 0] = row_scale(mix_rows[c], geos[c], stats[c, 0], stats[c, 1], P)
    return F.Report(name, scale.reshape(C, 1), ref, bound)


# ---- gathers ----------------------------------------------------------------------------------------------------------------------
def gather_input(mix_rows, geos, stats, entries, T, dtype=torch.float64, mut=()):
    """Row j: window `win` of row `row`, (x_padded - mean) * gain over the entry's length, 0 from there to T.
    -> (ref (n, 1, T), bound, lens)"""
    n = len(entries)
    ref, bound, lens = torch.zeros(n, 1, T, dtype=dtype), torch.zeros(n, 1, T, dtype=torch.float64), []
    for j, (c, k) in enumerate(entries):
        g = geos[c]
        sc = 0 if ("row0_stats" in mut and c == 1) else c
        mean, gain = (torch.tensor(float(stats[sc, i]), dtype=dtype) for i in (0, 1))
        xp = torch.zeros(g.T_pad + 2, dtype=dtype)
        pl = g.pad_left + (1 if "pad_plus" in mut else -1 if "pad_minus" in mut else 0)
        xp[1 + pl: 1 + pl + g.t_raw] = mix_rows[c].reshape(-1)[: g.t_raw].to(dtype)
        xp = xp[1: 1 + g.T_pad]
        s = g.starts[k]
        ln = g.L
        d = xp[s: s + ln] - mean
        ref[j, 0, :ln] = d * gain
        bound[j, 0, :ln] = U * (1 + U) * (d * gain).double().abs()
        if "no_tail_zero" in mut and ln < T:
            ref[j, 0, ln:] = (torch.zeros((), dtype=dtype) - mean) * gain
        lens.append(ln)
    return ref, bound, lens


def check_gather(mixn, mix_rows, geos, stats, entries, name="seg.gather"):
    n, T = len(entries), mixn.shape[-1]
    ref, bound, lens = gather_input(mix_rows, geos, stats, entries, T)
    return F.Report(name, mixn[:n], ref, bound, lens)


def gather_noise(noise, geos, entries, Bw, E, C, T):
    """z[m Bw + j][t] = noise[m C + row][s + t] below the entry's length, 0 from there to T (`entries`: all Bw slots).
    -> (ref (E Bw, 1, T), lens)"""
    ref, lens = torch.zeros(E * Bw, 1, T), []
    for m in range(E):
        for j, (c, k) in enumerate(entries):
            g = geos[c]
            ref[m * Bw + j, 0, : g.L] = noise[m * C + c, g.starts[k]: g.starts[k] + g.L]
            lens.append(g.L)
    return ref, lens


def check_noise(z, noise, geos, entries, Bw, E, C, name="seg.noise"):
    ref, lens = gather_noise(noise, geos, entries, Bw, E, C, z.shape[-1])
    return F.Report(name, z, ref, 0.0, lens)


# ---- crossfade stitch -----------------------------------------------------------------------------------------------------------
def stitch(geos, entries, y, carry, Bw, E, C, stride, M=None, dtype=torch.float64, mut=()):
    """The rows the last group's entries write.  y: (E Bw, 1, T) walk rows (member-major), carry: (E, 1, T) or None, the
    window in front of the group; `stride`: length of an output row.
    float64 (the reference): -> (ref, bound, seen, fade), each (E C, stride): value, bound, the element is written by one of
    the entries, e32 (|y_prev| + |y|) on the crossfades (0 elsewhere).
    float32 (the restatement): -> out (E C, stride) with SENTINEL where nothing was written."""
    M = M_WEIGHT if M is None else M
    f64 = dtype == torch.float64
    ref = torch.zeros(E * C, stride, dtype=dtype) if f64 else torch.full((E * C, stride), SENTINEL, dtype=dtype)
    bound, fade = torch.zeros(E * C, stride, dtype=torch.float64), torch.zeros(E * C, stride, dtype=torch.float64)
    seen = torch.zeros(E * C, stride, dtype=torch.int32)
    one = torch.ones((), dtype=dtype)
    for m in range(E):
        for j, (c, k) in enumerate(entries):
            g = geos[c]
            s, sp, w0, w1, e_prev = g.window(k, mut)
            u0, u1 = max(w0, g.pad_left, s), min(w1, g.pad_left + g.t_raw, s + g.L)
            if u1 <= u0:
                continue
            u = torch.arange(u0, u1)
            yk = y[m * Bw + j, 0].to(dtype)
            v = yk[u - s].clone()
            b = torch.zeros(u.numel(), dtype=torch.float64)
            fd = torch.zeros(u.numel(), dtype=torch.float64)
            if k > 0 and g.O > 0:
                if j > 0:
                    assert entries[j - 1] == (c, k - 1), "the row in front is not the window in front"
                    yp = y[m * Bw + j - 1, 0].to(dtype)
                else:
                    assert carry is not None, "the group's first entry needs the carry row"
                    yp = carry[m, 0].to(dtype)
                inside = u < e_prev
                ui = u[inside]
                a = weight(ui - w0, g.O, dtype, mut)
                p = yp[ui - sp]
                a1, a2 = (a, one - a) if "swap" in mut else (one - a, a)
                v[inside] = a1 * p + a2 * v[inside]
                if f64:
                    e32 = weight_e32(g.O)
                    w = p.abs() + yk[ui - s].abs()
                    b[inside] = M * e32 * w + U * (a1 * p).abs() * 2 + U * (a2 * yk[ui - s]).abs()
                    fd[inside] = e32 * w
            q = m * C + c
            lo, hi = u0 - g.pad_left, u1 - g.pad_left
            if f64:
                ref[q, lo:hi], bound[q, lo:hi], fade[q, lo:hi] = v, b, fd
            else:
                keep = _moved_words(q * stride + lo, hi - lo, mut)
                ref[q, lo:hi][keep] = v[keep]
            seen[q, lo:hi] += 1
    return (ref, bound, seen, fade) if f64 else ref


def _moved_words(addr, n, mut):
    """Which of the n destination words a 16-byte mover writes: all of them; the mutants drop the first / last of the words that
    go one by one (in front of the first 16-byte boundary and behind the last whole quad)."""
    keep = torch.ones(n, dtype=torch.bool)
    head = min(dest_head(addr), n)
    nq = (n - head) // 4
    singles = list(range(head)) + list(range(head + 4 * nq, n))
    if singles and "drop_first" in mut:
        keep[singles[0]] = False
    if singles and "drop_last" in mut:
        keep[singles[-1]] = False
    return keep


def check_stitch(out, geos, entries, y, carry, Bw, E, C, whole, tails=False, M=None, name="seg.stitch"):
    """out (E C, stride) of the device against the float64 stitch of the group's walk rows; `whole`: the group's entries have to
    cover every raw sample of every row (one group sees every window); `tails`: rows end at their own t_raw inside the stride,
    exactly 0 behind it.  Elements of earlier groups (not `seen`) cannot be held: they are not part of the report, and
    `excluded` counts nothing else."""
    stride = out.shape[-1]
    out = out.reshape(E * C, stride)
    ref, bound, seen, fade = stitch(geos, entries, y, carry, Bw, E, C, stride, M)
    assert int(seen.max()) <= 1, "two entries write one sample"
    held = seen.bool()
    for q in range(E * C):
        g = geos[q % C]
        if whole:
            assert bool(held[q, : g.t_raw].all()), "a raw sample no entry writes"
        if tails:
            held[q, g.t_raw:] = True  # ref = 0, bound = 0
    rep = F.Report(name, out[held].reshape(1, 1, -1), ref[held].reshape(1, 1, -1), bound[held].reshape(1, 1, -1))
    rep.held = int(held.sum())
    fd = fade[held]
    err = ((out[held].double() - ref[held]).abs() - 0.5 * F.ulp32(ref[held])).clamp(min=0)
    live = fd > 0
    rep.lib_ratio = float((err[live] / fd[live]).max()) if bool(live.any()) else 0.0
    rep.e32 = max([weight_e32(g.O) for g in geos if g.O > 0 and g.n_win > 1] or [0.0])
    rep.ref_peak = float(ref.abs().max())
    return rep


# ---- post step ----------------------------------------------------------------------------------------------------------------
def check_post(out, stitched, mix_rows, geos, E=1, name="seg.post"):
    """out (E C, stride) of the call with keep_rms against small_fp64.post of the stitched rows (member q: the mix of row q % C).
    -> (Report, [row divided], margin: the smallest |max|x| g - 1| of the reference over the bound's 8 u)"""
    C = len(mix_rows)
    stride = out.shape[-1]
    t_raw = [geos[q % C].t_raw for q in range(E * C)]
    mix = torch.zeros(E * C, 1, stride)
    for q in range(E * C):
        mix[q, 0, : t_raw[q]] = mix_rows[q % C]
    x = stitched.reshape(E * C, 1, stride)
    ref, bound, divided = F.post(x, mix, t_raw, [0] * (E * C), True)
    margin = float("inf")
    for q in range(E * C):
        n = t_raw[q]
        v = x[q, 0, :n].double()
        g = math.sqrt(float(mix[q, 0, :n].double().square().mean())) / max(math.sqrt(float(v.square().mean())), 1e-5)
        margin = min(margin, abs(float(v.abs().max()) * g - 1.0) / (8 * U))
    return F.Report(name, out.reshape(E * C, 1, stride), ref, bound, t_raw), divided, margin


def post_fp32(x, mix_rows, geos, E=1, mut=()):
    """The device's order: double sums, (float) rms, g = fl(mix_rms / max(x_rms, 1e-5)), the peak max|x| g in fp32, x g [/ peak]."""
    f = np.float32
    C = len(mix_rows)
    out = torch.zeros_like(x)
    for q in range(x.shape[0]):
        g_ = geos[q % C]
        n = g_.t_raw
        v = x[q, :n].numpy().astype(np.float32)
        mr = f(math.sqrt((mix_rows[q % C].numpy().astype(np.float64) ** 2).sum() / n))
        den = g_.T_pad if "rms_tpad" in mut else n
        xr = max(f(math.sqrt((v.astype(np.float64) ** 2).sum() / den)), f(1e-5))
        g = f(mr / xr)
        mxa = np.abs(v).max()
        mx = mxa if "guard_nogain" in mut else f(mxa * g)
        v = (v * g).astype(np.float32)
        if mx > f(1):
            v = (v / mx).astype(np.float32)
        out[q, :n] = torch.from_numpy(v)
    return out
