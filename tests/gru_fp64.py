"""float64 reference of the bidirectional GRU layers for the tests, written from the torch.nn.GRU definition:

    r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)        z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
    n = tanh(W_in x + b_in + r * (W_hn h + b_hn))     h' = (1 - z) * n + z * h            h0 = 0, gate order r, z, n

on the library's tap layout: the input projection `gx` is (B, 6H, T) with row dir * 3H + gate * H + unit and holds
W_ih x + b_ih + (b_hr, b_hz, 0) (the packer folds those biases into the projection and keeps b_hn apart); the output is
(B, 2H, T), forward units then backward units.  Three forms:

* `project`      gx from the layer's input tap;
* `step`         ONE step for all frames at once (teacher-forced: the previous state of every frame is given, so no error
                 accumulates and no dynamics enter -- valid for any weights, and an error shows at the frame and unit where
                 it was made);
* `free_run`     the plain recurrence (Python loop over the frames), for accumulated drift.

Per-row lengths: a row of `len` frames runs forward on [0, len), backward from len - 1 (from zero) and is exactly zero from
`len` on.

Tolerances.  Nothing absolute is fixed here.  Every check evaluates the same quantity from the same inputs twice on the CPU,
in float64 (the reference) and in fp32 torch, and takes e32 = max |fp32 - float64|.  A tap passes when, element by element,

    |tap - float64| <= M * e32 + 1/2 ulp(|tap|) [+ the input term below]

(1/2 ulp: the final rounding of the stored fp32 value, which the float64 reference does not have).  One M per form; they
live here so that the CPU sensitivity tests and the GPU tests share them.  M = twice the worst err / e32 ratio measured on an
MI355X over every case of tests/test_gpu_gru_fp64.py (profiles/gru_fp64_observed.json), rounded up to an integer; a ratio
above 8 is a finding, not a tolerance.

Input term (layers with the residual epilogue only).  Their tap holds out = (h + res) / sqrt(2), the previous state has to be
recovered from it, and a state recovered from a rounded value is not the state the kernel had.  With a = h + res:
|fl(a) - a| <= 1/2 ulp(a), |out - fl(a) s| <= 1/2 ulp(out), and the recovered value is rounded to fp32 once more (so that the
fp32 and the float64 evaluation read the same number): |h_rec - h| <= d := sqrt(2) * 1/2 ulp(out) + 1/2 ulp(sqrt(2) |out|) +
1/2 ulp(h_rec).  To first order the step moves by at most

    z d_u + |(1 - z)(1 - n^2) r| (|W_hn| d)_u + |(1 - z)(1 - n^2)(W_hn h + b_hn) r (1 - r)| (|W_hr| d)_u + |(h - n) z (1 - z)| (|W_hz| d)_u

which is evaluated in float64 per element and added to the bound (times 1 / sqrt(2) behind the residual)."""
import math

import torch

# one M per form (see above) = ceil(2 x worst measured ratio), profiles/gru_fp64_observed.json: projection 3.66 (PP24, 3 000
# frames, K = 768), step 4.57 (a first frame: h = 0, so e32 is a few 1e-8 and the hardware exp2 / rcp of the gates are what is
# left), free-running 2.58 (PP24, 3 000 frames)
M_PROJ = 8
M_STEP = 10
M_FREE = 6
M_CAP = 8  # a measured ratio above this is a finding to be explained, never a tolerance

SQRT2 = math.sqrt(2.0)
TAIL_Z = 1e4  # what gru_tail_fill_kernel puts into the z rows of gx behind a row's end (0 into the r and n rows)


def ulp32(x):
    """Spacing of the fp32 numbers at |x| (float64 tensor in, float64 tensor out)."""
    a = x.abs().to(torch.float32)
    # (a value that rounds up to the next binade gets that binade's spacing: the larger of the two, the safe side)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))).double() - a.double())


class Layer:
    """Weights of one bidirectional GRU layer as the packer lays them out: W (6H, I), folded bias (6H), W_hh (2, 3H, H),
    b_hn (2, H) -- fp32 values (the bias folded in double and rounded once, ou_model.cpp `pack` of GruL)."""

    def __init__(self, sd, prefix, layer):
        W, b, whh, bhn = [], [], [], []
        for sfx in ("", "_reverse"):
            k = f"_l{layer}{sfx}"
            w_ih, w_hh = sd[prefix + ".weight_ih" + k], sd[prefix + ".weight_hh" + k]
            b_ih, b_hh = sd[prefix + ".bias_ih" + k].double(), sd[prefix + ".bias_hh" + k].double()
            H = w_hh.shape[1]
            fold = b_ih.clone()
            fold[: 2 * H] += b_hh[: 2 * H]
            W.append(w_ih.float())
            b.append(fold.float())
            whh.append(w_hh.float())
            bhn.append(b_hh[2 * H:].float())
        self.H = H
        self.W, self.bias = torch.cat(W, 0), torch.cat(b, 0)
        self.whh, self.bhn = torch.stack(whh), torch.stack(bhn)


def _lens(lens, B, T):
    if lens is None:
        return torch.full((B,), T, dtype=torch.long)
    return torch.as_tensor(lens, dtype=torch.long)


def valid_mask(lens, B, T):
    """(B, 1, T) bool: frame t of row b lies inside the row."""
    return (torch.arange(T)[None, :] < _lens(lens, B, T)[:, None])[:, None, :]


def project(L, x, dtype=torch.float64):
    """gx = W_ih x + folded bias for both directions.  x: (B, I, T) -> (B, 6H, T)."""
    return torch.matmul(L.W.to(dtype), x.to(dtype)) + L.bias.to(dtype)[None, :, None]


def cell(whh, bhn, g, h, tanh=torch.tanh):
    """One GRU step of one direction.  whh (3H, H), bhn (H), g (..., 3H) projection, h (..., H) previous state -> (..., H)."""
    H = h.shape[-1]
    gh = h @ whh.T
    r = torch.sigmoid(g[..., :H] + gh[..., :H])
    z = torch.sigmoid(g[..., H:2 * H] + gh[..., H:2 * H])
    n = tanh(g[..., 2 * H:] + r * (gh[..., 2 * H:] + bhn))
    return (1 - z) * n + z * h


def step(L, gx, hprev, dtype=torch.float64, tanh=torch.tanh):
    """Teacher-forced: frame t of every (row, direction) from its given previous state.  gx (B, 6H, T), hprev (B, 2H, T)."""
    H = L.H
    out = []
    for d in range(2):
        g = gx[:, d * 3 * H:(d + 1) * 3 * H].to(dtype).transpose(1, 2)   # (B, T, 3H)
        h = hprev[:, d * H:(d + 1) * H].to(dtype).transpose(1, 2)        # (B, T, H)
        out.append(cell(L.whh[d].to(dtype), L.bhn[d].to(dtype), g, h, tanh).transpose(1, 2))
    return torch.cat(out, 1)


def shift_prev(h, lens=None):
    """Previous state of every frame from a (B, 2H, T) state tap: forward h[t - 1] (0 at t = 0), backward h[t + 1] (0 at the
    row's last frame len - 1; behind the row everything is 0 anyway)."""
    B, H2, T = h.shape
    H = H2 // 2
    prev = torch.zeros_like(h)
    prev[:, :H, 1:] = h[:, :H, :-1]
    prev[:, H:, :-1] = h[:, H:, 1:]
    ln = _lens(lens, B, T)
    for b in range(B):
        prev[b, H:, int(ln[b]) - 1:] = 0
        prev[b, :H, int(ln[b]):] = 0
    return prev


def free_run(L, gx, lens=None, dtype=torch.float64, bwd_start=None, hook=None, tanh=torch.tanh):
    """The recurrence itself.  gx (B, 6H, T) -> (B, 2H, T).  `bwd_start` (per row, default len - 1): frame at which the
    backward pass starts from zero; `hook(d, t, h_new, out)` may replace the state of a step (the CPU tests plant defects
    through these two; the product has neither)."""
    B, H6, T = gx.shape
    H = H6 // 6
    ln = _lens(lens, B, T)
    start = ln - 1 if bwd_start is None else torch.as_tensor(bwd_start, dtype=torch.long)
    out = torch.zeros(B, 2 * H, T, dtype=dtype)
    for d in range(2):
        whh, bhn = L.whh[d].to(dtype), L.bhn[d].to(dtype)
        g = gx[:, d * 3 * H:(d + 1) * 3 * H].to(dtype).permute(2, 0, 1).contiguous()  # (T, B, 3H)
        h = torch.zeros(B, H, dtype=dtype)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            live = ((t < ln) if d == 0 else (t <= start))[:, None]
            hn = cell(whh, bhn, g[t], h, tanh)
            if hook is not None:
                hn = hook(d, t, hn, out)
            h = torch.where(live, hn, h if d == 0 else torch.zeros_like(h))
            out[:, d * H:(d + 1) * H, t] = torch.where(live & (t < ln)[:, None], h, torch.zeros_like(h))
    return out


def free_run_aten_fp32(L, gx, lens=None):
    """The same recurrence through ATen's fp32 GRU: fed the gx tap through an identity input weight (exact in fp32), one
    direction and one row at a time (rows of different lengths)."""
    B, H6, T = gx.shape
    H = H6 // 6
    ln = _lens(lens, B, T)
    eye = torch.eye(3 * H)
    zero = torch.zeros(3 * H)
    out = torch.zeros(B, 2 * H, T)
    for d in range(2):
        b_hh = torch.cat([torch.zeros(2 * H), L.bhn[d]])
        flat = [eye, L.whh[d].contiguous(), zero, b_hh]
        for b in range(B):
            n = int(ln[b])
            x = gx[b, d * 3 * H:(d + 1) * 3 * H, :n].float().T[None]  # (1, n, 3H)
            if d:
                x = x.flip(1)
            y, _ = torch._VF.gru(x.contiguous(), torch.zeros(1, 1, H), flat, True, 1, 0.0, False, False, True)
            y = y[0].T
            out[b, d * H:(d + 1) * H, :n] = y.flip(1) if d else y
    return out


def residual(h, res, dtype=torch.float64):
    """The residual epilogue (h + res) / sqrt(2)."""
    return (h.to(dtype) + res.to(dtype)) / SQRT2


def undo_residual(out, res):
    """Previous-state source of a layer with the residual epilogue: h = sqrt(2) out - res in float64, rounded to fp32, and
    the bound d >= |h_rec - h_kernel| of the module docstring (float64)."""
    o = out.double()
    h = (o * SQRT2 - res.double()).float()
    d = SQRT2 * 0.5 * ulp32(o) + 0.5 * ulp32(o * SQRT2) + 0.5 * ulp32(h.double())
    return h, d


def _input_term(L, gx, hprev, dprev):
    """First-order bound of what an uncertainty `dprev` >= 0 of the previous state does to the step (module docstring)."""
    H = L.H
    out = []
    for d in range(2):
        W = L.whh[d].double()
        g = gx[:, d * 3 * H:(d + 1) * 3 * H].double().transpose(1, 2)
        h = hprev[:, d * H:(d + 1) * H].double().transpose(1, 2)
        dl = dprev[:, d * H:(d + 1) * H].double().transpose(1, 2)
        gh = h @ W.T
        aw = dl @ W.abs().T
        r = torch.sigmoid(g[..., :H] + gh[..., :H])
        z = torch.sigmoid(g[..., H:2 * H] + gh[..., H:2 * H])
        hn = gh[..., 2 * H:] + L.bhn[d].double()
        n = torch.tanh(g[..., 2 * H:] + r * hn)
        dn = ((1 - z) * (1 - n * n)).abs()
        t = z * dl + dn * r * aw[..., 2 * H:] + dn * (hn * r * (1 - r)).abs() * aw[..., :H] + ((h - n) * z * (1 - z)).abs() * aw[..., H:2 * H]
        out.append(t.transpose(1, 2))
    return torch.cat(out, 1)


class Report:
    """Outcome of one element-by-element check.  `bad`: bool tensor in the tap's shape; `ratio` = max (err - 1/2 ulp - input
    term) / e32, i.e. what M has to cover, `raw_ratio` = max err / e32; `worst` =
    location of the largest excess over the bound as a dict (row, dir, frame, unit -- or row, gx row, frame); `tail_bad` =
    elements behind a row's end that are not exactly what they have to be.  `excluded` is always 0: every element is either
    held against the bound or against an exact value."""

    def __init__(self, form, tap, ref, e32, M, slack, valid, tail_expect, H):
        self.form, self.H = form, H
        err = (tap.double() - ref).abs()
        v = valid.expand_as(err)
        self.e32 = float(e32)
        tol = M * self.e32 + slack
        self.err = float(err[v].max()) if v.any() else 0.0
        # what M has to cover: the error beyond the terms of the bound that are not multiples of e32
        net = float((err - slack)[v].clamp(min=0).max()) if v.any() else 0.0
        self.raw_ratio = self.err / self.e32 if self.e32 > 0 else (0.0 if self.err == 0 else float("inf"))
        self.ratio = net / self.e32 if self.e32 > 0 else (0.0 if net == 0 else float("inf"))
        self.bad = (err > tol) & v
        tail = ~v
        self.tail_bad = int(((tap.double() != tail_expect) & tail).sum())
        self.bad |= (tap.double() != tail_expect) & tail
        self.n_bad = int(self.bad.sum())
        self.checked = int(v.sum()) + int(tail.sum())
        self.excluded = tap.numel() - self.checked
        ex = torch.where(v, err - tol, torch.full_like(err, -float("inf")))
        if self.tail_bad:
            ex = torch.where(tail & (tap.double() != tail_expect), torch.full_like(err, float("inf")), ex)
        b, c, t = [int(i) for i in torch.unravel_index(ex.argmax(), ex.shape)]
        self.worst = {"row": b, "frame": t, "excess": float(ex[b, c, t]), "err": float(err[b, c, t]), "tol": float(tol[b, c, t])}
        if form == "proj":
            self.worst.update(dir=c // (3 * H), gate=(c // H) % 3, unit=c % H)
        else:
            self.worst.update(dir=c // H, unit=c % H)

    def where(self):
        """(rows, dirs, frames, units) that hold a flagged element, as sorted lists (state taps)."""
        idx = self.bad.nonzero()
        return (sorted(set(idx[:, 0].tolist())), sorted(set((idx[:, 1] // self.H).tolist())), sorted(set(idx[:, 2].tolist())),
                sorted(set((idx[:, 1] % self.H).tolist())))

    def summary(self):
        return {"form": self.form, "e32": self.e32, "err": self.err, "ratio": round(self.ratio, 3), "raw_ratio": round(self.raw_ratio, 3), "bad": self.n_bad,
                "tail_bad": self.tail_bad, "checked": self.checked, "excluded": self.excluded, "worst": self.worst}

    def ok(self):
        return self.n_bad == 0 and self.excluded == 0

    def __str__(self):
        w = self.worst
        m = f"{self.form}: err {self.err:.3e} e32 {self.e32:.3e} ratio {self.ratio:.2f} flagged {self.n_bad} of {self.checked}"
        if self.n_bad:
            m += (f"; worst at row {w['row']} dir {w['dir']} frame {w['frame']} unit {w['unit']} (16-unit workgroup "
                  f"{w['unit'] // 16}, 8-unit workgroup {w['unit'] // 8}): err {w['err']:.3e} > bound {w['tol']:.3e}")
        return m


def check_projection(L, x, gx, lens=None, ragged=False, M=None):
    """The gx tap against W_ih x + folded bias in float64; behind a row's end of a ragged call the exact tail fill."""
    M = M_PROJ if M is None else M
    B, _, T = gx.shape
    ref = project(L, x)
    e32 = (project(L, x, torch.float32).double() - ref).abs()
    valid = valid_mask(lens, B, T)
    e32 = e32[valid.expand_as(e32)].max()
    slack = 0.5 * ulp32(torch.maximum(ref.abs(), gx.double().abs()))
    tail = torch.zeros_like(ref)
    if ragged:
        H = L.H
        for d in range(2):
            tail[:, d * 3 * H + H: d * 3 * H + 2 * H] = TAIL_Z
    else:
        assert bool(valid.all())
    return Report("proj", gx, ref, e32, M, slack, valid, tail, L.H)


def check_step(L, gx, out, lens=None, res=None, M=None, tanh32=torch.tanh):
    """The output tap, teacher-forced: every frame from the tap's own neighbouring frame (the residual epilogue undone
    first, in float64) and the gx tap, against float64; exactly zero behind a row's end."""
    M = M_STEP if M is None else M
    B, _, T = out.shape
    valid = valid_mask(lens, B, T)
    extra = 0.0
    if res is None:
        hprev = shift_prev(out.float(), lens)
    else:
        h, d = undo_residual(out, res)
        hprev = shift_prev(h, lens)
        extra = _input_term(L, gx, hprev, shift_prev(d, lens)) / SQRT2
    ref = step(L, gx, hprev)
    r32 = step(L, gx, hprev, torch.float32)
    if res is not None:
        ref = residual(ref, res)
        r32 = residual(r32, res, torch.float32)
    e32 = (r32.double() - ref).abs()[valid.expand_as(ref)].max()
    slack = 0.5 * ulp32(torch.maximum(ref.abs(), out.double().abs())) + extra
    return Report("step", out, ref, e32, M, slack, valid, torch.zeros_like(ref), L.H)


def check_free(L, gx, out, lens=None, res=None, M=None):
    """The output tap against the free-running float64 recurrence from the gx tap.  Admissible only where two legitimate fp32
    evaluations (explicit, ATen) sit within 2 x of each other against float64 -- otherwise the dynamics amplify rounding
    and no bound exists; asserted here."""
    M = M_FREE if M is None else M
    B, _, T = out.shape
    valid = valid_mask(lens, B, T)
    ref = free_run(L, gx, lens)
    a = free_run(L, gx, lens, torch.float32)
    b = free_run_aten_fp32(L, gx, lens)
    if res is not None:
        ref, a, b = residual(ref, res), residual(a, res, torch.float32), residual(b, res, torch.float32)
    ea = float((a.double() - ref).abs()[valid.expand_as(ref)].max())
    eb = float((b.double() - ref).abs()[valid.expand_as(ref)].max())
    assert max(ea, eb) <= 2.0 * min(ea, eb), f"free-running comparison not admissible: fp32 explicit {ea:.3e} vs ATen {eb:.3e}"
    e32 = eb
    slack = 0.5 * ulp32(torch.maximum(ref.abs(), out.double().abs()))
    rep = Report("free", out, ref, e32, M, slack, valid, torch.zeros_like(ref), L.H)
    rep.e32_explicit, rep.e32_aten = ea, eb
    return rep
