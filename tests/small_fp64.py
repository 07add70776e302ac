"""float64 references of the small kernels of ou_small.hip for the tests, each written from the operation's definition on the
library's tap layout, each with a per-element bound.  The references are teacher-forced: they take the very inputs the kernel
read (the library's own intermediates), so an error shows at the element where it was made.

u = 2^-24 is the unit roundoff of fp32.  Three kinds of bound, none tuned:

* exact      the operation is a fixed sequence of single fp32 operations (one product, sequential adds): the tap has to equal
             the same sequence evaluated in fp32 torch, bit for bit (bound 0).
* chain      a sum of n products accumulated in fp32 in ANY order (a serial FMA chain, per-lane chains met by a butterfly,
             partial sums met in LDS): |gpu - f64| <= (n + 2) u A + 1/2 ulp(|gpu|), A = the float64 sum of the absolute values
             of the products (+ |bias|).  [Higham, Accuracy and Stability, (3.5): gamma_n A with gamma_n = n u / (1 - n u); the
             two spare u cover the bias add and 1 / (1 - n u) for n <= 2^10.]  Where an input of a product is itself one
             rounded fp32 operation of the tap (x * w_in, x * window, a PReLU product) n grows by one per such operation and
             the float64 reference uses the unrounded value.  Second stages propagate the first bound to first order.
* statistic  sums in double on the device; the bound is the fp32 rounding of the few scalars, propagated (docstrings).
* library    stages that call a math-library function (log10f, expf, sin): M x the error e32 = max |fp32 torch - f64| of the
             same stage from the same inputs evaluated on the CPU, + 1/2 ulp.  M = twice the worst err / e32 ratio measured on
             an MI355X over the cases of tests/test_gpu_small_fp64.py (profiles/small_fp64_observed.json), rounded up; a ratio
             above M_CAP is a finding, not a tolerance.

No element is excluded: every element of a tap is held against its bound or, behind a row's end, against exactly 0.

Parameters are the fp32 values the library holds, rebuilt by the packer's own formula (weight norm g v / |v| in double, rounded
once; the mel twiddles (float) cos / sin(2 pi i / N) in double); `Params.check_against_blob` holds them against the packed blob
where plan_json or the allocation order gives the offset.

Not verified against the blob (plan_json gives no offset and the allocation order does not pin them without restating the
whole layout): the conditioner's input conv (c_in_w, c_in_b) and the st convs' PReLU slopes (st_alpha) -- rebuilt by the same
formula as their verified score-network counterparts.  The FIR taps, biases and slopes ARE read from the blob at plan_json's
fir_off / fbias_off / a_off.

The Snake pair (cond.aux -> wav) and stft_forward / stft_inverse_frames are held at the `library` bound as whole stages
(sinf; sincospif twiddles, powf / log1pf / expm1f); stft_overlap_add at its chain bound from the GPU's own frames.
gru_tail_fill_kernel is held exactly by tests/test_gpu_gru_fp64.py
(ragged projection check).  upload_rows_kernel's table has no tensor name: it is seen only through the tails and row ends it
places.  out_conv_kernel's OUT_UPDATE WITH the noise term is never a call's last step and earlier steps leave no taps: the same
arithmetic is held through sampler_step_kernel.  init_x_kernel is held through score.in of a warm-started call (its x0 is
overwritten by the update).
Branches the shipped topologies (the cases of this module) do not reach, and where they are held instead -- the off-list
topologies of tests/offlist_cases.py, run by tests/test_gpu_offlist.py with the functions of this module: fir_kernel (the scalar
form takes only tap counts without a fir4_kernel instantiation; shipped: 5, 7, 9, 11, 17, all instantiated) at 13 and 15 taps on
both paths (cases r67, odd_pp, r27); out_conv_kernel's scalar path (T % 4 != 0) on whole rows of the models whose tot_ds is 21,
63 and 14 (odd_pp with KW 5, odd_or, r27); in_conv_kernel / out_conv_kernel with KW 1, 5 and 7 (one, odd_pp, kw7), OUT_SCORE and OUT_UPDATE;
film_kernel and sigma_embed_kernel with D / 64 = 1 and 16 (kw7, d1024) and the random-Fourier-feature MLP at n_rff 16 (odd_or);
sum_kernel with 2, 3 and 4 operands (one, odd_pp, r67 / odd_or)."""
import math

import torch

U = 2.0 ** -24

# M of the `library` bounds = ceil(2 x worst measured err / e32) over the 20 seam cases, profiles/small_fp64_observed.json
# (`lib_ratio`): simple embedding 1.00 (the kernel takes sin / cos of the fp32 phase in double: what is left is the phase's own
# fp32 rounding, the same as in the fp32 evaluation), random Fourier features + MLP 2.33 (OR16s, batch 3).
M_EMBED_SIMPLE = 2
M_EMBED_RFF = 5
M_CAP = 8  # a measured ratio above this is a finding to be explained, never a tolerance


def ulp32(x):
    """Spacing of the fp32 numbers at |x| (float64 in, float64 out)."""
    a = x.abs().to(torch.float32)
    return torch.nextafter(a, torch.full_like(a, float("inf"))).double() - a.double()


def valid_mask(lens, B, T):
    """(B, 1, T) bool: sample t of row b lies inside the row."""
    if lens is None:
        return torch.ones(B, 1, T, dtype=torch.bool)
    return (torch.arange(T)[None, :] < torch.as_tensor(lens, dtype=torch.long)[:, None])[:, None, :]


class Report:
    """Outcome of one element-by-element check: `ratio` = max err / bound over the elements inside their rows (what the
    a-priori bounds leave of their room; <= 1 passes), `tail_bad` = elements behind a row's end that are not exactly 0,
    `excluded` = elements held against nothing (always 0)."""

    def __init__(self, name, gpu, ref, bound, lens=None):
        gpu, ref = gpu.double(), ref.double()
        assert gpu.shape == ref.shape, (name, gpu.shape, ref.shape)
        if gpu.ndim < 3:
            gpu, ref = gpu.reshape(gpu.shape[0], 1, -1), ref.reshape(ref.shape[0], 1, -1)
        if not torch.is_tensor(bound):
            bound = torch.full_like(gpu, float(bound))
        else:
            bound = bound.double().reshape(gpu.shape) if bound.numel() == gpu.numel() else bound.double().expand_as(gpu)
        self.name = name
        valid = valid_mask(lens, gpu.shape[0], gpu.shape[-1]).expand_as(gpu)
        err = (gpu - ref).abs()
        err = torch.where(torch.isfinite(gpu), err, torch.full_like(err, float("inf")))
        tol = bound + 0.5 * ulp32(gpu) * (bound > 0)  # (exact operations: no final-rounding allowance either)
        self.bad = ((err > tol) & valid) | ((gpu != 0) & ~valid)
        self.tail_bad = int(((gpu != 0) & ~valid).sum())
        self.n_bad = int(self.bad.sum())
        # what is actually compared: inside the rows a finite reference against a finite bound, behind them the exact 0
        held = valid & torch.isfinite(ref) & torch.isfinite(bound)
        self.checked = int(held.sum()) + int((~valid).sum())
        self.excluded = gpu.numel() - self.checked
        self.err = float(err[valid].max()) if valid.any() else 0.0
        q = torch.where(valid, err / tol.clamp(min=1e-300), torch.zeros_like(err))
        q = torch.where(valid & (err == 0), torch.zeros_like(q), q)
        self.ratio = float(q.max())
        i = [int(v) for v in torch.unravel_index(torch.where(self.bad, torch.full_like(q, float("inf")), q).argmax(), q.shape)]
        self.worst = {"index": i, "gpu": float(gpu[tuple(i)]), "ref": float(ref[tuple(i)]), "err": float(err[tuple(i)]),
                      "bound": float(tol[tuple(i)])}

    def ok(self):
        return self.n_bad == 0 and self.excluded == 0

    def summary(self):
        return {"err": self.err, "ratio": round(self.ratio, 4), "bad": self.n_bad, "tail_bad": self.tail_bad, "checked": self.checked,
                "excluded": self.excluded, "worst": self.worst}

    def __str__(self):
        return (f"{self.name}: err {self.err:.3e}, err / bound {self.ratio:.3f}, flagged {self.n_bad} of {self.checked} "
                f"(tails {self.tail_bad}), excluded {self.excluded}; worst {self.worst}")


# ---- parameters ----------------------------------------------------------------------------------------------------------
def eff_weight(sd, p):
    """The packer's effective weight of a maybe-weight-normed layer: g v / |v| per output row in double, rounded once."""
    if p + ".weight_g" in sd:
        v = sd[p + ".weight_v"].double()
        g = sd[p + ".weight_g"].double().reshape(-1)
        nrm = v.reshape(v.shape[0], -1).pow(2).sum(1).sqrt()
        return (v * (g / nrm).reshape([-1] + [1] * (v.ndim - 1))).float()
    return sd[p + ".weight"].float()


class Params:
    """fp32 parameters of the small kernels of one model, as the library holds them."""

    def __init__(self, spec, sd):
        sp, cp = spec.score_prefix, "condition_model"
        s, c = spec.score, spec.cond
        self.spec = spec
        self.simple = s.time_embedding == "simple"
        self.D, self.n_rff = s.noise_cond_dim, s.n_rff
        if self.simple:
            self.sig_w, self.sig_b = sd[sp + ".sigma_block.weight"].float().reshape(()), sd[sp + ".sigma_block.bias"].float().reshape(())
        else:
            self.freq = sd[sp + ".sigma_block.freq"].float()
            self.mlp = [(sd[f"{sp}.sigma_block.layer{i}.prelu.weight"].float().reshape(()), sd[f"{sp}.sigma_block.layer{i}.lin.weight"].float(),
                         sd[f"{sp}.sigma_block.layer{i}.lin.bias"].float()) for i in (1, 2, 3)]
        self.s_in_w, self.s_in_b = eff_weight(sd, sp + ".input_conv")[:, 0, :], sd[sp + ".input_conv.bias"].float()
        self.c_in_w, self.c_in_b = eff_weight(sd, cp + ".input_conv")[:, 0, :], sd[cp + ".input_conv.bias"].float()
        n = len(s.rate_factors)
        nb = n + int(s.extra_conv_block)
        W, b = [], []
        for side, cnt in ((".encoder.cond_proj.", nb), (".decoder.noise_cond_proj.", nb)):
            for i in range(cnt):
                W.append(eff_weight(sd, f"{sp}{side}{i}"))
                b.append(sd[f"{sp}{side}{i}.bias"].float())
        self.film_w, self.film_b = torch.cat(W, 0), torch.cat(b, 0)
        self.out_w = eff_weight(sd, sp + ".output_conv.conv")[0]          # (C0, KW)
        self.out_b = sd[sp + ".output_conv.conv.bias"].float().reshape(())
        self.out_a = (sd[sp + ".prelu.weight"].float().reshape(()), sd[sp + ".output_conv.prelu.weight"].float().reshape(()))
        self.st_alpha = [sd[f"{cp}.encoder.st_convs.{i}.prelu.weight"].float().reshape(()) for i in range(n - 1)]
        self.st_rate = [int(math.prod(c.rate_factors[i:])) for i in range(n - 1)]
        tot = spec.tot_ds
        self.n_fft = c.n_mel_oversample * tot
        self.hop, self.mel_pad = tot, (self.n_fft - tot) // 2
        self.win = sd[cp + ".input_mel.mel_spec.spectrogram.window"].float()
        self.fb = sd[cp + ".input_mel.mel_spec.mel_scale.fb"].float()    # (n_freq, n_mels)
        i = torch.arange(self.n_fft, dtype=torch.float64)
        self.tc, self.ts = torch.cos(2 * math.pi * i / self.n_fft).float(), torch.sin(2 * math.pi * i / self.n_fft).float()
        self.level = torch.tensor(10.0 ** (spec.level_db / 20.0), dtype=torch.float64).float()
        self.edm = spec.edm_noise is not None

    def check_against_blob(self, blob, plan):
        """The rebuilt values are the blob's: the FiLM table at plan_json's offsets, and -- by the allocation order of
        ou_model.cpp (256-byte slots: sigma block, score input conv first; output conv, mel window, filterbank, twiddles right
        behind the FiLM bias) -- the rest."""
        a64 = lambda n: (n + 63) // 64 * 64
        def same(off, t):
            t = t.reshape(-1)
            assert torch.equal(blob[off: off + t.numel()], t), off
            return off + a64(t.numel())
        off = same(plan["film_w_off"], self.film_w)
        assert off == plan["film_b_off"] and self.film_w.shape[0] == plan["film_rows"]
        off = same(off, self.film_b)
        off = same(off, self.out_w)
        off = same(off, self.out_b)
        off = same(off, torch.stack(self.out_a))
        off = same(off, self.win)
        off = same(off, self.fb)
        same(off, torch.cat([self.tc, self.ts]))
        if self.simple:
            off = same(0, torch.stack([self.sig_w, self.sig_b]))
        else:
            off = same(0, torch.cat([self.freq] + [torch.cat([a.reshape(1), w.reshape(-1), b]) for a, w, b in self.mlp]))
        off = same(off, self.s_in_w)
        same(off, self.s_in_b)


def edm_coef(spec, sigma):
    """make_coef of ou_walk.cpp for per-row sigmas, in its fp32 arithmetic: dict of fp32 tensors (B,)."""
    s = torch.as_tensor(sigma, dtype=torch.float32)
    s2 = s * s
    if spec.edm_noise is None:
        one = torch.ones_like(s)
        return {"w_skip": 0 * one, "w_in": one, "w_out": one, "sigma_net": s, "sig2": s2}
    lvl = getattr(spec, "edm_data_level_db", None)
    sdv = 10.0 ** ((spec.level_db if lvl is None else lvl) / 20.0)
    sd2 = torch.tensor(sdv * sdv, dtype=torch.float64).float()
    sn2 = s2 + sd2
    sn = sn2.sqrt()
    return {"w_skip": sd2 / sn2, "w_in": 1.0 / sn, "w_out": (s * torch.tensor(sdv, dtype=torch.float64).float()) / sn,
            "sigma_net": torch.tensor(spec.edm_noise, dtype=torch.float32) * s, "sig2": s2}


def prelu(v, a):
    return torch.where(v >= 0, v, a * v)


def _taps(x, KW):
    """(B, C, T) -> (B, C, T, KW): sample t + k - (KW - 1) / 2 of the same row, 0 outside it."""
    pad = (KW - 1) // 2
    xp = torch.nn.functional.pad(x, (pad, KW - 1 - pad))
    return xp.unfold(-1, KW, 1)


# ---- exact operations ------------------------------------------------------------------------------------------------------
def s2d(x, alpha, R):
    """s2d_kernel: y[b, c R + k, q] = prelu(x[b, c, q R + k], alpha): one fp32 product per element -> exact."""
    B, C, T = x.shape
    v = prelu(x.float(), alpha.float())
    return v.view(B, C, T // R, R).permute(0, 1, 3, 2).reshape(B, C * R, T // R), 0.0


def sum_scaled(parts, scale):
    """sum_kernel: (((a + b) + c) + d) + e in fp32, then one product with fp32 `scale` -> exact."""
    v = parts[0].float().clone()
    for p in parts[1:]:
        v = v + p.float()
    return v * torch.tensor(scale, dtype=torch.float32), 0.0


def sum_scale_of(n_parts):
    """The host's scale of the conditioner's encoder sum: 1.0f / sqrtf((float) n)."""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n_parts), dtype=torch.float32).sqrt())


# ---- FMA chains --------------------------------------------------------------------------------------------------------------
def in_conv(x, w, bias, w_in=None, dtype=torch.float64):
    """in_conv_kernel: y[b, c, t] = sum_k w[c, k] (x[b, t + k - pad] w_in[b]) + bias[c], zero padding at the row's ends of the
    buffer.  chain bound with n = KW (+ 1 with w_in: the scaled sample is one rounded product; the reference scales exactly):
    (n + 2) u (sum_k |w x w_in| + |bias|)."""
    KW = w.shape[1]
    xs = x.to(dtype)
    if w_in is not None:
        xs = xs * w_in.to(dtype).view(-1, 1, 1)
    p = _taps(xs, KW) * w.to(dtype)[None, :, None, :]           # (B, 1 -> C, T, KW) products
    ref = p.sum(-1) + bias.to(dtype)[None, :, None]
    n = KW + (1 if w_in is not None else 0)
    bound = (n + 2) * U * (p.double().abs().sum(-1) + bias.double().abs()[None, :, None])
    return ref, bound


def in_conv_fp32(x, w, bias, w_in=None, hook=None):
    """The kernel's arithmetic in fp32 torch: taps k = 0 .. KW - 1 in that order by FMA (a * b + c rounded once, emulated in
    double: exact for fp32 operands), then + bias.  `hook(taps)` may damage the (B, 1, T, KW) window (CPU tests)."""
    xs = x.float() * w_in.float().view(-1, 1, 1) if w_in is not None else x.float()
    t = _taps(xs, w.shape[1])
    if hook is not None:
        t = hook(t)
    acc = torch.zeros(x.shape[0], w.shape[0], x.shape[-1])
    for k in range(w.shape[1]):
        acc = (w[None, :, None, k].double() * t[..., k].double() + acc.double()).float()
    return acc + bias.float()[None, :, None]


def film(g, W, b, dtype=torch.float64):
    """film_kernel: film[s, row] = sum_d W[row, d] g[s, d] + b[row]: 64 per-lane FMA chains of D / 64 terms met by a 6-stage
    butterfly = a sum of n = D products in some order: chain bound (D + 2) u (sum_d |W g| + |b|)."""
    g2 = g.to(dtype).reshape(g.shape[0], -1)
    ref = g2 @ W.to(dtype).T + b.to(dtype)
    bound = (W.shape[1] + 2) * U * (g2.double().abs() @ W.double().abs().T + b.double().abs())
    return ref, bound


def film_fp32(g, W, b, skip_stage=None, swap_rows=0):
    """The kernel's order: lane l chains d = l, l + 64, ... by FMA; butterfly over lane distances 32, 16, .., 1; + b.
    Damages for the CPU tests: one butterfly stage skipped (lane 0 then misses half the lanes); gamma / beta rows swapped
    (`swap_rows` = the first block's channel count C, from the spec)."""
    S, D = g.shape[0], W.shape[1]
    g2 = g.float().reshape(S, D)
    acc = torch.zeros(S, W.shape[0], 64)
    for i in range(D // 64):
        acc = (W[None, :, i * 64:(i + 1) * 64].double() * g2[:, None, i * 64:(i + 1) * 64].double() + acc.double()).float()
    for o in (32, 16, 8, 4, 2, 1):
        if o == skip_stage:
            continue
        acc = acc + acc[..., torch.arange(64) ^ o]
    out = acc[..., 0] + b.float()
    if swap_rows:  # (every block's rows are [gamma (C) | beta (C)]: the first block's halves exchanged)
        C = int(swap_rows)
        out = torch.cat([out[:, C:2 * C], out[:, :C], out[:, 2 * C:]], 1)
    return out


def out_conv_score(s, x, P, coef, dtype=torch.float64):
    """out_conv_kernel, OUT_SCORE.  v = prelu(prelu(s, a1), a2) (two rounded products on the negative side);
    net = sum_c sum_k w[c, k] v[c, t + k - pad] + bias: 8 per-wave FMA chains met in LDS by a tree = n = C KW products in some
    order, each carrying the two PReLU roundings: e_net = (C KW + 4) u (sum |w v| + |bias|).
    Plain model: score = net.  EDM: est = w_skip x + w_out net, score = (est - x) / sig2, every operation rounded once and the
    coefficients taken as make_coef's fp32 values with 1 ulp of slack each (their host arithmetic is rebuilt here, not read):
    |d score| <= [ |w_out| e_net + 3 u |w_skip x| + 3 u |w_out net| + u |est| + u |est - x| ] / sig2 + 2 u |score|
    -- the cancellation of est - x is bounded through these absolute terms, no element is masked."""
    a1, a2 = P.out_a
    C, KW = P.out_w.shape
    v = prelu(prelu(s.to(dtype), a1.to(dtype)), a2.to(dtype))
    p = _taps(v, KW) * P.out_w.to(dtype)[None, :, None, :]
    net = p.sum((-1, 1)) [:, None, :] + P.out_b.to(dtype)
    e_net = (C * KW + 4) * U * (p.double().abs().sum((-1, 1))[:, None, :] + P.out_b.double().abs())
    if not P.edm:
        return net, e_net
    ws, wo, s2 = (coef[k].to(dtype).view(-1, 1, 1) for k in ("w_skip", "w_out", "sig2"))
    xv = x.to(dtype)
    est = ws * xv + wo * net
    score = (est - xv) / s2
    bound = (wo.abs() * e_net + 3 * U * (ws * xv).abs() + 3 * U * (wo * net).abs() + U * est.abs() + U * (est - xv).abs()) / s2 \
        + 2 * U * score.abs()
    return score, bound.double()


def out_conv_fp32(s, x, P, coef, hook=None):
    """The kernel's arithmetic in fp32 torch (channel groups of C / 8 chained by FMA, the 8 partial sums as the kernel's tree).
    `hook(window)` may damage the (B, C, T, KW) window."""
    f = torch.float32
    a1, a2 = P.out_a
    C, KW = P.out_w.shape
    t = _taps(prelu(prelu(s.float(), a1), a2), KW)
    if hook is not None:
        t = hook(t)
    cpg = (C + 7) // 8
    part = []
    for gidx in range(8):
        acc = torch.zeros(s.shape[0], s.shape[-1])
        for c in range(gidx * cpg, min(C, (gidx + 1) * cpg)):
            for k in range(KW):
                acc = (P.out_w[c, k].double() * t[:, c, :, k].double() + acc.double()).float()
        part.append(acc)
    net = (((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7])) + P.out_b)[:, None, :]
    if not P.edm:
        return net
    ws, wo, s2 = (coef[k].to(f).view(-1, 1, 1) for k in ("w_skip", "w_out", "sig2"))
    est = ws * x.float() + wo * net
    return (est - x.float()) / s2


def _frames(x, P, L, shift=0):
    """(B, 1, T) -> (B, L, n_fft): frame f holds samples f hop + n - pad_left (+ shift), 0 outside the row's buffer."""
    T = x.shape[-1]
    xp = torch.nn.functional.pad(x[:, 0], (P.mel_pad + P.n_fft, P.n_fft + P.hop))
    start = P.n_fft + shift
    return xp[:, start: start + (L - 1) * P.hop + P.n_fft].unfold(-1, P.n_fft, P.hop)[:, :L]


def mel(x, P, dtype=torch.float64, shift=0):
    """mel_kernel: frame f, sample n: v = x[f hop + n - pad_left] win[n] (one rounded product); re_k = sum_n v cos[(k n) mod N],
    im_k = -sum_n v sin[...] (FMA chains of N terms; the tables are the packer's fp32 values); pw_k = re^2 + im^2;
    mel_m = sum_k pw_k fb[k, m] (FMA chain of n_freq terms).
    e_re = (N + 3) u sum_n |v cos| (e_im alike);  e_pw = 2 |re| e_re + 2 |im| e_im + 2 u pw (two products and an add, the
    squares of the errors dropped: first order);  bound = sum_k e_pw fb + (n_freq + 2) u sum_k pw fb   (fb >= 0)."""
    B, _, T = x.shape
    L = T // P.hop
    N, F = P.n_fft, P.fb.shape[0]
    v = _frames(x.to(dtype), P, L, shift) * P.win.to(dtype)                  # (B, L, N)
    idx = (torch.arange(F)[:, None] * torch.arange(N)[None, :]) % N         # (F, N)
    ct, st = P.tc.to(dtype)[idx].T.contiguous(), P.ts.to(dtype)[idx].T.contiguous()  # (N, F)
    re, im = v @ ct, -(v @ st)
    pw = re * re + im * im
    out = (pw @ P.fb.to(dtype)).transpose(1, 2)                              # (B, n_mels, L)
    if dtype != torch.float64:
        return out, None
    va = v.abs()
    e_re, e_im = (N + 3) * U * (va @ ct.abs()), (N + 3) * U * (va @ st.abs())
    e_pw = 2 * re.abs() * e_re + 2 * im.abs() * e_im + 2 * U * pw
    fb = P.fb.double()
    bound = (e_pw @ fb.abs() + (F + 2) * U * (pw @ fb.abs())).transpose(1, 2)
    return out, bound


def mel_scale(mel_tap, n_frames=None):
    """mel_scale_kernel (+ mel_kernel's frame energies): scale_b = 1 / max(sqrt(mean_f sum_m mel[b, m, f]^2), 1e-5) over the
    row's own frames, from the GPU's own mel tap.  Device arithmetic: every term mel^2 rounded (u), the frame's n_mels terms
    summed in fp32 by a block reduction ((n_mels + 2) u relative: all terms >= 0), frames summed in double, sqrt and the
    division rounded to fp32 once each, the square root halving the relative error of its argument:
    relative bound ((n_mels + 3) / 2 + 2) u."""
    B, n_mels, L = mel_tap.shape
    m = mel_tap.double()
    out = torch.zeros(B, 1, 1, dtype=torch.float64)
    for b in range(B):
        Lb = L if n_frames is None else int(n_frames[b])
        out[b] = 1.0 / max(math.sqrt(float(m[b, :, :Lb].pow(2).sum()) / Lb), 1e-5)
    return out, ((n_mels + 3) / 2 + 2) * U * out


# ---- statistics kernels ----------------------------------------------------------------------------------------------------
def norm_gain(level, sd, mx, norm, eps, dtype):
    """NormMode::gain (ou_kernels.h) of the unclamped 0-d tensors sd and mx, every operation once in `dtype`."""
    c = lambda v: torch.tensor(v, dtype=torch.float64).to(dtype)
    level = level.to(dtype)
    if norm == "max":
        return level / torch.maximum(mx, c(1e-5))
    if norm == "2-max":
        return torch.minimum(level / torch.maximum(sd, c(eps)), c(1.0) / torch.maximum(mx, c(eps)))
    return level / torch.maximum(sd, c(1e-5))


def pad_normalize(mix, t_raw, T_pad_max, level, tot_ds, dtype=torch.float64, std_den_off=1, norm="2", zero_mean=True, eps=1e-5):
    """pad_normalize_kernel / pad_normalize_var_kernel.  Row b: T_pad = t_raw + (tot_ds - t_raw % tot_ds), the samples at
    pad_left = (T_pad - t_raw) / 2, y = (x_padded - mean) * level / sd with mean over the PADDED signal and the unbiased sd
    (T_pad - 1) of it; zero from T_pad on (ragged batches).
    Device: sums in double (n 2^-53: negligible against u), mean rounded to fp32 (|d mean| <= u |mean|), d = fl(x - mean_f)
    (u |d|), sd from the d's in double: by the triangle inequality in l2 its relative error is at most u + u |mean| / sd
    sqrt(N / (N - 1)); then (float) sd, gain = fl(level / sd): rho = (3 u + 1.01 u |mean| / sd); y = fl(d * gain):
    |y - ref| <= G (u |mean| + |x - mean| (u + rho)) + 1/2 ulp(y),  G = level / sd.

    The other modes (NormMode, ou_kernels.h; `norm` "2" | "max" | "2-max", `zero_mean`, `eps` of the 2-max branch), as
    norm_cases.norm_stats states utils/norm.py: mu = mean if zero_mean else 0; sd unbiased around the row's own mean whatever
    zero_mean says; mx = max |x_padded - mu|; G = NormMode::gain(level, sd, mx); y = (x_padded - mu) G.  The same three
    sources of error, with rho the relative error of the device's gain as norm_cases.stats_bounds derives it:
      unclamped std branch   rho = rho_sd (there with one more u for fl(level), which this function is handed exactly: kept)
      max branch             rho = rho_max: the fp32 maximum of the d's is one of them (u, and the mean's u |mean| / mx), the
                             division u
      a clamp in force       the gain is fl(fl(level) / fl(clamp)), clamp = 1e-5, or eps under 2-max: rho = 3 u
      2-max                  the larger of its two candidates' rho, whichever the device took
      zero_mean true         |y - ref| <= G (u |mean| + |x - mean| (u + rho)) + 1/2 ulp(y)   as above
      zero_mean false        d = fl(x - 0) = x exactly and the padding is exactly 0:  |y - ref| <= |x| G rho + 1/2 ulp(y)
    (norm 2 with zero_mean keeps its own arithmetic and its 3 u above where the sd is not clamped.)
    Determinacy, asserted of the inputs in float64 from the reference alone (norm_cases.undetermined with the row's rho): no
    norm within rho of its clamp, and under 2-max the two candidate gains not within rho of each other -- elsewhere rounding
    would pick the branch (choose other inputs).
    With another dtype the arithmetic is the device's in that precision: the sums in double, every scalar rounded once."""
    import norm_cases as K

    norm = str(norm)
    plain = norm == "2" and zero_mean
    level_db = 20.0 * math.log10(float(level))  # (norm_stats takes dB; what it makes of this is fl(level) within 2^-52)
    B = mix.shape[0]
    ref = torch.zeros(B, 1, T_pad_max, dtype=dtype)
    bound = torch.zeros(B, 1, T_pad_max, dtype=torch.float64)
    lens = []
    for b in range(B):
        n = int(t_raw[b])
        pad = tot_ds - n % tot_ds
        Tp, pl = n + pad, pad // 2
        lens.append(Tp)
        xp = torch.zeros(Tp, dtype=dtype)
        xp[pl: pl + n] = mix[b].reshape(-1)[:n].to(dtype)
        st = K.norm_stats(xp, norm, level_db, zero_mean, eps)
        rho = K.stats_bounds(xp, st, norm, zero_mean)[1]
        why = K.undetermined(st, norm, rho, eps)
        assert why is None, f"row {b}: {why}: the gain's branch is not determined (choose other inputs)"
        if plain:
            mean = xp.double().sum() / Tp  # (the sum in double, as on the device; float64: the very sum this always was)
            if dtype != torch.float64:
                mean = mean.float()
            d = xp - mean
            sd = (d.double().pow(2).sum() / (Tp - std_den_off)).sqrt().to(dtype)
            if float(sd) > 1e-5:
                rho = 3 * U + 1.01 * U * float(mean.abs() / sd)
            G = level.to(dtype) / sd.clamp(min=1e-5)
            ref[b, 0, :Tp] = d * G
            bound[b, 0, :Tp] = float(G) * (U * float(mean.abs()) + d.double().abs() * (U + rho))
            continue
        if dtype == torch.float64:
            mean = torch.tensor(float(xp.mean()), dtype=dtype)
            mu = torch.tensor(st["mean"], dtype=dtype)
            sd, mx = torch.tensor(st["sd"], dtype=dtype), torch.tensor(st["mx"], dtype=dtype)
            if std_den_off != 1:
                sd = sd * math.sqrt((Tp - 1) / (Tp - std_den_off))
        else:
            mean = (xp.double().sum() / Tp).to(dtype)
            mu = mean if zero_mean else torch.zeros((), dtype=dtype)
            sd = ((xp - mean).double().pow(2).sum() / (Tp - std_den_off)).sqrt().to(dtype)
            mx = (xp - mu).abs().max()
        G = norm_gain(level, sd, mx, norm, eps, dtype)
        d = xp - mu
        ref[b, 0, :Tp] = d * G
        if zero_mean:
            bound[b, 0, :Tp] = float(G) * (U * float(mean.abs()) + d.double().abs() * (U + rho))
        else:
            bound[b, 0, :Tp] = float(G) * d.double().abs() * rho
    return ref, bound, lens


def post(x, mix, t_raw, pad_left, keep_rms, peak_guard=True, dtype=torch.float64, always_divide=False):
    """post_reg_kernel / post_kernel / post_var_kernel.  Row b: v = x[pad_left : pad_left + t_raw]; keep_rms: v *= g,
    g = mix_rms / max(x_rms, 1e-5) (mix_rms of the raw mix, computed here in float64 from the mix itself); peak guard:
    mx = max |v|, v /= mx where mx > 1; zero behind the row's t_raw (ragged batches).
    Device: both rms in double, rounded to fp32 once (u each), g = fl(mix_rms / x_rms) (u): 3 u; v = fl(x g): 4 u relative
    (0 without keep_rms: v = x exactly); mx is the maximum of those v's: within 4 u (0) of the true one; the division is
    rounded once (the 1/2 ulp): relative bound  r = 4 u (kept) + 4 u (divided) -- and 0 where neither applies (exact copy).
    A true mx within r of 1 would leave the branch to rounding: refused here (choose other inputs)."""
    B = x.shape[0]
    Tm = mix.shape[-1]
    ref = torch.zeros(B, 1, Tm, dtype=dtype)
    bound = torch.zeros(B, 1, Tm, dtype=torch.float64)
    divided = []
    for b in range(B):
        n, pl = int(t_raw[b]), int(pad_left[b])
        v = x[b, 0, pl: pl + n].to(dtype)
        r = 0.0
        if keep_rms:
            mix_rms = mix[b].reshape(-1)[:n].to(dtype).pow(2).mean().sqrt()
            x_rms = v.pow(2).mean().sqrt().clamp(min=1e-5)
            v = v * (mix_rms / x_rms)
            r += 4 * U
        mx = float(v.abs().max())
        assert abs(mx - 1.0) > 16 * U, "peak within rounding of 1: the branch is not determined"
        div = (peak_guard and mx > 1.0) or always_divide
        if div:
            v = v / v.abs().max()
            r += 4 * U if keep_rms else 0.0
            # (without keep_rms mx is exact and only the division rounds: the 1/2 ulp; give the bound a non-zero value so that
            # the final rounding is allowed for)
            r = max(r, 2.0 ** -60)
        divided.append(bool(div))
        ref[b, 0, :n] = v
        bound[b, 0, :n] = r * v.double().abs()
    return ref, bound, divided


# ---- math-library stages -----------------------------------------------------------------------------------------------------
def sigma_embed(sigma_net, P, dtype=torch.float64, swap_halves=False):
    """sigma_embed_kernel from the rows' fp32 sigma_net: ls = log10(sigma_net);
    simple:  f = 0.5 sigmoid(w ls + b), g = [sin(2 pi f k), cos(2 pi f k)], k < D / 2   (sigma_block.py:73-78)
    RFF:     [sin, cos](2 pi freq ls) -> 3 x (Linear -> PReLU)                         (sigma_block.py:50-57)
    `library` bound (module docstring): the fp32 evaluation is this function with dtype=torch.float32."""
    sn = sigma_net.to(dtype)
    ls = torch.log10(sn)
    two_pi = torch.tensor(2 * math.pi, dtype=dtype)
    if P.simple:
        f = 0.5 * torch.sigmoid(P.sig_w.to(dtype) * ls + P.sig_b.to(dtype))
        ph = (two_pi * f)[:, None] * torch.arange(P.D // 2, dtype=dtype)[None, :]
        halves = [torch.sin(ph), torch.cos(ph)]
        return torch.cat(halves[::-1] if swap_halves else halves, 1)
    ph = (two_pi * P.freq.to(dtype))[None, :] * ls[:, None]
    halves = [torch.sin(ph), torch.cos(ph)]
    h = torch.cat(halves[::-1] if swap_halves else halves, 1)
    for a, W, b in P.mlp:
        h = prelu(h @ W.to(dtype).T + b.to(dtype), a.to(dtype))
    return h


def check_sigma_embed(g_tap, sigma_net, P, M=None):
    """-> (Report, e32): the g tap (B, D, 1) against float64 at M e32 + 1/2 ulp."""
    M = (M_EMBED_SIMPLE if P.simple else M_EMBED_RFF) if M is None else M
    ref = sigma_embed(sigma_net, P)
    e32 = float((sigma_embed(sigma_net, P, torch.float32).double() - ref).abs().max())
    rep = Report("sigma_embed", g_tap.reshape(ref.shape), ref, torch.full_like(ref, M * e32))
    rep.e32 = e32
    rep.lib_ratio = float(((g_tap.reshape(ref.shape).double() - ref).abs() - 0.5 * ulp32(ref)).clamp(min=0).max()) / e32
    return rep


# ---- binomial FIR, sampler update ----------------------------------------------------------------------------------------------
INV_SQRT2 = float(torch.tensor(1.0 / math.sqrt(2.0), dtype=torch.float64).float())  # the host's kInvSqrt2 as fp32


def fir(x, taps, alpha=None, bias=None, res=None, res_scale=1.0, dtype=torch.float64, hook=None):
    """fir_kernel / fir4_kernel<NT>: y[c, t] = sum_j taps[j] a(x[c, t + j - r]) (+ bias[c]), a = PReLU(alpha) in the down-path
    (pre) form, identity in the up-path (post) form; zero padding at the row's ends; with a residual y = (y + res) * res_scale.
    chain bound e = (NT + 2 (+ 1 with the PReLU product)) u (sum |taps a(x)| + |bias|); the residual add and the scaling are one
    rounding each: (e + u |y + res|) res_scale + u |result| (+ 1/2 ulp).  `hook(window)` may damage the (B, C, T, NT) window."""
    NT = taps.numel()
    v = x.to(dtype)
    if alpha is not None:
        v = prelu(v, torch.as_tensor(alpha).to(dtype))
    w = _taps(v, NT)
    if hook is not None:
        w = hook(w)
    p = w * taps.to(dtype)
    if dtype == torch.float64:
        y = p.sum(-1)
    else:  # the kernel's serial FMA chain
        y = torch.zeros(x.shape)
        for j in range(NT):
            y = (taps[j].double() * w[..., j].double() + y.double()).float()
    A = p.double().abs().sum(-1)
    if bias is not None:
        y = y + bias.to(dtype)[None, :, None]
        A = A + bias.double().abs()[None, :, None]
    bound = (NT + 2 + (alpha is not None)) * U * A
    if res is not None:
        s = y + res.to(dtype)
        y = s * torch.tensor(res_scale, dtype=dtype)
        bound = (bound + U * s.double().abs()) * res_scale + U * y.double().abs()
    return y, bound


def sampler_update(x, score, c1, z=None, c2=0.0, score_bound=0.0, dtype=torch.float64):
    """sampler_step_kernel and out_conv_kernel's OUT_UPDATE epilogue: r = x + c1 * score (+ c2 * z), every operation rounded
    once, FMA contraction off in the build (were it on, the results would differ by at most the 1 ulp allowed here anyway):
    |r - ref| <= |c1| score_bound + u |c1 score| + u |x + c1 score| (+ u |c2 z| + u |r|) + 1/2 ulp.  c2 stands for beta * s_next
    in the fused form, where z * s_next is rounded first (one more u |c2 z|)."""
    t = torch.tensor(c1, dtype=dtype) * score.to(dtype)
    r = x.to(dtype) + t
    bound = abs(c1) * score_bound + U * t.double().abs() + U * r.double().abs()
    if z is not None:
        zt = torch.tensor(c2, dtype=dtype) * z.to(dtype)
        r = r + zt
        bound = bound + 2 * U * zt.double().abs() + U * r.double().abs()
    return r, bound


def init_x(noise, sigma, base=None):
    """init_x_kernel in its own fp32 arithmetic: fl(noise * sigma) (+ base): exact (1 ulp were FMA contraction on)."""
    v = noise.float() * torch.tensor(sigma, dtype=torch.float32)
    return v if base is None else base.float() + v


# ---- the cases of the GPU tests and the edge classes they have to hit -------------------------------------------------
MODELS = ("PP16s", "PP16m", "OR16s", "PP24s")
# (frames, batch) of the seam cases: T = frames * tot_ds.  1 frame: shorter than every tile; 3 / 33: odd lengths on the deepest
# level (a row ending inside a quad, 33 one past the 32-quotient tile of s2d); 16: T a multiple of the 256-sample tiles for
# tot_ds 160 and 240; 32: the s2d tile exactly.
SEAM_SHAPES = ((1, 1), (3, 3), (16, 1), (32, 3), (33, 3))
CASES = [(m, B, f) for m in MODELS for f, B in SEAM_SHAPES]
# ragged batches (frames per row; the samples are frames * tot_ds - 3): the short rows end inside a tile on every level
RAGGED = [(m, (33, 3, 1)) for m in MODELS]
# the stand-alone FIR passes (options fuse_upfir = 0, rate_small = 0) of the two anti-aliased topologies: frame counts at which
# the level lengths frames * (samples per frame of the level) are a multiple of the 1 024-sample tile or cross it by no more
# than the halo (205 frames: 1 025 and 4 100 samples on PP16's two deepest levels; 129 frames: 1 032 on PP24's deepest)
FIR_CASES = [("PP16s", B, f) for f, B in ((1, 1), (3, 3), (32, 1), (64, 3), (205, 3), (256, 1))] + \
            [("PP24s", B, f) for f, B in ((1, 1), (3, 3), (64, 1), (128, 3), (129, 3))]
FIR_RAGGED = [("PP16s", (205, 3, 1)), ("PP24s", (129, 3, 1))]
# a warm-started enhance of one step: ONE sigma shared by the rows of the batch (coefficient stride 0)
SHARED = [("PP16s", 3, 3), ("PP24s", 3, 16)]
PREPOST_T = (1, 1023, 1025, 65536, 65537)
# a ragged warm-started step: in_conv and out_conv of the score network with per-row lengths
RAGGED_STEP = [("PP16s", (33, 3, 1)), ("PP24s", (33, 3, 1))]
# cond.aux -> aux_to_wav() of the two topologies with the Snake decoupling layer
SNAKE_CASES = [(m, B, f) for m in ("PP16s", "PP24s") for f, B in SEAM_SHAPES]
# the STFT pair: (tag, n_fft, hop, window, transform, exponent, factor, T, B).  The four parameter sets of helpers.TRANSFORM_CASES
# (n_fft 510 > the 256-thread block and even, 256 even, 255 odd; `padded` differs from exp05 in the exponent and in the length
# CompressedMagSTFTPadded leaves: 1024 - 128), a T shorter than n_fft / 2, one frame only, batch 1 and 3.
STFT_CASES = [("exp05", 510, 128, "hann", "exponent", 0.5, 0.15, 1000, 3), ("log", 256, 64, "sqrthann", "log", 1.0, 0.5, 1000, 1),
              ("none_odd", 255, 85, "hamming", "none", 1.0, 1.0, 1000, 3), ("padded", 510, 128, "hann", "exponent", 0.667, 0.3, 896, 1),
              ("short", 510, 128, "hann", "exponent", 0.5, 0.15, 100, 3), ("short_odd", 255, 85, "hamming", "log", 1.0, 0.5, 60, 1)]

# what the GPU tests report per case list (the GPU file asserts it of every case it runs): the coverage test credits a kernel
# with a class only from lists whose test holds that kernel.  RAGGED-type lists give class (f) only where the kernel itself got
# the rows' lengths: with mask_fused = 0 the FIR pass runs without them (mask_tail_kernel zeroes behind it), so that list gives
# the FIR no (f).
REPORTED = {"CASES": ("in_conv", "out_conv", "mel", "s2d"), "RAGGED": ("in_conv", "mel", "s2d"), "RAGGED_STEP": ("in_conv", "out_conv"),
            "FIR_CASES": ("fir",), "FIR_RAGGED_MASKS": ("fir", "in_conv", "mel", "s2d"), "FIR_RAGGED_FUSED": ("fir", "in_conv", "mel", "s2d")}
GROUPS = {"CASES": CASES, "FIR_CASES": FIR_CASES}                     # (model, B, frames)
RAGGED_GROUPS = {"RAGGED": (RAGGED, True), "RAGGED_STEP": (RAGGED_STEP, True), "FIR_RAGGED_MASKS": (FIR_RAGGED, False),
                 "FIR_RAGGED_FUSED": (FIR_RAGGED, True)}              # (model, rows), kernel got the lengths


def family(key):
    """Kernel family of a report key of the GPU file / a tap of kernel_axes."""
    for f, pre in (("in_conv", ("cond.in", "score.in", "in_conv")), ("out_conv", ("out_conv",)), ("s2d", ("s2d",)), ("fir", ("fir",)),
                   ("mel", ("mel",))):
        if key.startswith(pre) and key != "mel_scale":
            return f
    return key
MAX_FRAMES = 256  # a class that only longer inputs reach is left out: a test case stays a few seconds at the most


def levels(plan, prefix):
    """samples per frame at the input of every rate-change conv of `prefix`'s encoder, from plan_json: [(m, fir_len)] in the
    order of the levels (the decoder's up-path FIRs run at the same lengths with the same tap counts, asserted)."""
    convs = {c["name"]: c for c in plan["convs"]}
    m, out, i = plan["tot_ds"], [], 0
    while f"{prefix}.encoder.ds_modules.{i}.rate_change_conv" in convs:
        c = convs[f"{prefix}.encoder.ds_modules.{i}.rate_change_conv"]
        out.append((m, c["fir_len"] if c["fir_mode"] == 1 else 0))
        m //= c["rate"]
        i += 1
    ups = [c for n, c in convs.items() if n.startswith(prefix + ".decoder.") and n.endswith("rate_change_conv")]
    assert sorted(c["fir_len"] for c in ups if c["fir_mode"] == 2) == sorted(n for _, n in out if n)
    return out


def kernel_axes(plan, spec):
    """Every checked tap of a model with its own time axis: {name: (samples per frame m, tile, halo, takes per-row lengths)}.
    Tiles and halos are the launch constants of ou_small.hip: in_conv 256 samples, halo (KW - 1) / 2; out_conv 64 quads = 256
    samples; s2d 32 quotients of R samples (halo: none; a crossing by up to 3 quotients counts); FIR 1 024, halo NT / 2;
    mel one block per frame."""
    td = plan["tot_ds"]
    pad = (spec.score.fb_kernel_size - 1) // 2
    ax = {"in_conv": (td, 256, pad, True), "out_conv": (td, 256, pad, True), "mel": (1, 1, 0, True)}
    for i, (m, _) in enumerate(levels(plan, "condition_model")[:-1]):
        ax[f"s2d{i}"] = (m, 32 * m, 3 * m, False)
    for i, (m, nt) in enumerate(levels(plan, spec.score_prefix)):
        if nt:
            ax[f"fir{i}.nt{nt}"] = (m, 1024, nt // 2, True)
    return ax


def classes_of(n, tile, halo, B, ragged=False):
    """Edge classes (a) .. (f) of the issue that a row of n elements in a batch of B meets."""
    hit = set()
    if n < tile:
        hit.add("a")
    if n % 4:
        hit.add("b")
    if n > tile and 0 < n % tile <= halo:
        hit.add("c")
    if n % tile == 0:
        hit.add("d")
    if B == 1:
        hit.add("e1")
    if B == 3:
        hit.add("e3")
    if ragged:
        hit.add("f")
    return hit


def reachable_classes(m, tile, halo, takes_lens):
    """What a call through the seams (n = frames * m, frames <= MAX_FRAMES) can meet, by number theory rather than by trying the
    classifier: the residues of n modulo tile are the multiples of g = gcd(m, tile)."""
    g = math.gcd(m, tile)
    out = {"e1", "e3"}
    if m < tile:
        out.add("a")                                       # one frame
    if m % 4:
        out.add("b")                                       # one frame
    if tile // g <= MAX_FRAMES:
        out.add("d")                                       # frames = tile / g
    if g <= halo and tile // g > 1:
        # smallest frames with residue g behind at least one whole tile: frames = inverse of (m / g) modulo (tile / g) (+ tile / g)
        q = tile // g
        f = pow(m // g, -1, q)
        if f * m <= tile:
            f += q
        if f <= MAX_FRAMES:
            out.add("c")
    if takes_lens:
        out.add("f")
    return out


# ---- Snake decoupling, STFT pair (stages with math-library calls: the `library` bound) -----------------------------------------
# M = ceil(2 x worst measured err / e32), profiles/small_fp64_observed.json (`lib_ratio` of the cases snake.* / stft.*):
# Snake 1.09 (PP16s, batch 3, 32 frames); forward STFT 1.63 (none_odd); inverse frames 4.32 (short: one frame, where the fp32
# torch evaluation sums its 2 x 254 terms blocked and the kernel in one serial FMA chain, so e32 is at its smallest).
M_SNAKE = 3
M_STFT_FWD = 4
M_STFT_INV = 9


def lib_report(name, gpu, ref, r32, M, lens=None):
    """Report at M e32 + 1/2 ulp, e32 = max |fp32 torch - f64| over the elements inside their rows; `lib_ratio` = what M covers."""
    gpu3 = gpu.reshape(ref.shape)
    valid = valid_mask(lens, ref.shape[0], ref.shape[-1]).expand_as(ref) if ref.ndim == 3 else torch.ones_like(ref, dtype=torch.bool)
    e32 = float((r32.double() - ref).abs()[valid].max())
    rep = Report(name, gpu3, ref, torch.full_like(ref, M * e32), lens)
    rep.e32 = e32
    net = ((gpu3.double() - ref).abs() - 0.5 * ulp32(ref))[valid].clamp(min=0).max()
    rep.lib_ratio = float(net) / e32 if e32 > 0 else (0.0 if float(net) == 0 else float("inf"))
    return rep


class SnakeParams:
    """signal_decoupling_layer as the packer holds it: alpha stored as exp(alpha) (fp32 exp on the host)."""

    def __init__(self, sd, p="signal_decoupling_layer"):
        self.alpha = torch.tensor([math.exp(float(a)) for a in sd[p + ".prelu.act.act.alpha"].float()], dtype=torch.float64).float()
        self.up = sd[p + ".prelu.act.upsample.kernel"].float()       # (2, 1, 15)
        self.down = sd[p + ".prelu.act.downsample.kernel"].float()   # (1, 1, 28)
        self.w, self.b = eff_weight(sd, p + ".conv"), sd[p + ".conv.bias"].float()


def snake(aux, S, dtype=torch.float64, hook=None):
    """snake_up_kernel + snake_down_conv_kernel: u[2 q + ph] = sum_k up[ph, k] aux[q + k - 7] (15 taps, zero padding);
    u += sin(alpha u)^2 / (alpha + 1e-9) (snake.py:59-62); d[t] = sum_k down[k] u[2 t + k - 13] (28 taps, zero padding);
    out[t] = sum_c sum_k3 w[c, k3] d_c[t + k3 - 1] + bias (zero padding).  The intermediate u has no tensor name and the stage
    calls sinf: `library` bound on aux -> wav as a whole.  `hook(u)` may damage the up-sampled signal (CPU tests)."""
    import torch.nn.functional as Fn

    B, C, T = aux.shape
    x = aux.to(dtype).reshape(B * C, 1, T)
    u = Fn.conv1d(Fn.pad(x, (7, 7)), S.up.to(dtype)).transpose(1, 2).reshape(B, C, 2 * T)
    a = S.alpha.to(dtype)[None, :, None]
    u = u + (1.0 / (a + torch.tensor(1e-9, dtype=dtype))) * torch.sin(u * a) ** 2
    if hook is not None:
        u = hook(u)
    d = Fn.conv1d(Fn.pad(u.reshape(B * C, 1, 2 * T), (13, 14)), S.down.to(dtype), stride=2).reshape(B, C, T)
    return Fn.conv1d(d, S.w.to(dtype), S.b.to(dtype), padding=1)


def _spec_compress(re, im, kind, e, factor):
    mag = torch.sqrt(re * re + im * im)
    if kind == "exponent":
        g = (1e-7 + mag) ** (e - 1.0) if e != 1.0 else torch.ones_like(mag)
        return re * g * factor, im * g * factor
    if kind == "log":
        g = torch.where(mag > 0, torch.log1p(mag) / mag.clamp(min=1e-300 if mag.dtype == torch.float64 else 1e-38), torch.zeros_like(mag))
        return re * (g * factor), im * (g * factor)
    return re, im


def _spec_expand(re, im, kind, e, factor):
    if kind == "none":
        return re, im
    re, im = re / factor, im / factor
    mag = torch.sqrt(re * re + im * im)
    if kind == "exponent":
        g = (1e-7 + mag) ** (1.0 / e - 1.0) if e != 1.0 else torch.ones_like(mag)
    else:
        g = torch.where(mag > 0, torch.expm1(mag) / mag.clamp(min=1e-300 if mag.dtype == torch.float64 else 1e-38), torch.zeros_like(mag))
    return re * g, im * g


def _twiddles(N, F, dtype):
    """cos / sin(2 pi (k n mod N) / N) as (N, F) matrices: the table is built in `dtype` (fp32: what a table of rounded entries
    costs), the index arithmetic is exact."""
    n = torch.arange(N, dtype=dtype)
    ang = 2 * math.pi * n / N
    idx = (torch.arange(F)[:, None] * torch.arange(N)[None, :]) % N
    return torch.cos(ang)[idx].T.contiguous(), torch.sin(ang)[idx].T.contiguous()


def stft_frames_count(T, N, hop):
    return 1 + (T + 2 * (N // 2) - N) // hop


def stft_forward(x, win, N, hop, kind, e, factor, dtype=torch.float64, shift=0):
    """stft_forward_kernel: centred frames (zero padding N / 2), v = x win; re_k = sum_n v cos(2 pi k n / N),
    im_k = -sum_n v sin(..); magnitude compression (dyn_range_comp.py:117-131); (B, [re | im] x F, frames).
    Twiddles by sincospif, compression by powf / log1pf: `library` bound on the whole kernel."""
    B, T = x.shape
    F_, nf = N // 2 + 1, stft_frames_count(T, N, hop)
    xp = torch.nn.functional.pad(x.to(dtype), (N // 2 + N, N // 2 + N + hop))
    fr = xp[:, N + shift:].unfold(-1, N, hop)[:, :nf] * win.to(dtype)
    ct, st = _twiddles(N, F_, dtype)
    re, im = _spec_compress(fr @ ct, -(fr @ st), kind, e, factor)
    return torch.cat([re, im], -1).transpose(1, 2).contiguous()


def stft_inverse_frames(spec, win, N, kind, e, factor, dtype=torch.float64):
    """stft_inverse_frames_kernel: expansion, then frames[b, f, n] = (re_0 (+ (-1)^n re_{N/2}) + 2 sum_{0 < k < N/2}
    (re_k cos(2 pi k n / N) - im_k sin(..))) / N * win[n] (c2r: the imaginary parts of DC and Nyquist ignored).  `library` bound."""
    B, C2, nf = spec.shape
    F_ = N // 2 + 1
    re, im = _spec_expand(spec[:, :F_].to(dtype).transpose(1, 2), spec[:, F_:].to(dtype).transpose(1, 2), kind, e, factor)  # (B, nf, F)
    ct, st = _twiddles(N, F_, dtype)                                                                                      # (N, F)
    kmax = F_ - 1 if N % 2 == 0 else F_
    acc = re[..., :1].expand(B, nf, N).clone()
    if N % 2 == 0:
        sign = torch.where(torch.arange(N) % 2 == 1, -1.0, 1.0).to(dtype)
        acc = acc + re[..., F_ - 1:F_] * sign
    s2 = re[..., 1:kmax] @ ct[:, 1:kmax].T - im[..., 1:kmax] @ st[:, 1:kmax].T
    return (acc + 2.0 * s2) / N * win.to(dtype)


def stft_overlap_add(frames, win, N, hop, length):
    """stft_overlap_add_kernel: y[t] = sum_f frames[f, t + N / 2 - f hop] / sum_f win[..]^2 where the envelope exceeds 1e-11,
    else exactly 0 (torch.istft, center=True, trimmed to `length`).  Sequential fp32 adds of n <= ceil(N / hop) frames and an
    FMA chain of as many squares, one division: chain bound
    ((n + 2) u sum |frames|) / env + |y| ((n + 2) u + u) + 1/2 ulp; bound 0 (exact) where the envelope is 0."""
    B, nf, _ = frames.shape
    total = (nf - 1) * hop + N + length
    acc = torch.zeros(B, total, dtype=torch.float64)
    ab = torch.zeros(B, total, dtype=torch.float64)
    env = torch.zeros(total, dtype=torch.float64)
    w2 = win.double() ** 2
    for f in range(nf):  # (frames, not samples)
        acc[:, f * hop: f * hop + N] += frames[:, f].double()
        ab[:, f * hop: f * hop + N] += frames[:, f].double().abs()
        env[f * hop: f * hop + N] += w2
    sl = slice(N // 2, N // 2 + length)
    acc, ab, env = acc[:, sl], ab[:, sl], env[sl]
    live = env.float() > 1e-11
    assert not bool(((env > 0) & (env < 1e-9)).any()), "an envelope at the kernel's threshold: the branch is not determined"
    n = -(-N // hop)
    safe = env.clamp(min=1e-30)
    y = torch.where(live, acc / safe, torch.zeros_like(acc))
    bound = torch.where(live, (n + 2) * U * ab / safe + y.abs() * (n + 3) * U, torch.zeros_like(acc))
    return y, bound
