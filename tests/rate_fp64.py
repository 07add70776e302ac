"""float64 references of the rate-change / 1x1 / phase-GEMM layers (all of Runner::conv outside Runner::body, ou_walk.cpp) for the
tests, written from the operation's definition on the library's tap layout, each with a per-element bound.  Teacher-forced like
tests/small_fp64.py and tests/conv_fp64.py, whose Report, ulp32, valid_mask, prelu, Epi, _epilogue, blocks_of and chain
convention are used, not copied: the reference of a layer takes the tap the kernel read.

The layers (blocks.py:205-227, condition.py:53-59, score.py:208):

    down   y = conv_{k=s=r}(FIR_{2r+1}(prelu(x))) + bias       conditioner: no FIR            {blk}.v (.fir) -> {blk}.h
    up     y = FIR_{2r+1}(convT_{k=s=r}(prelu(x))) + bias      conditioner: no FIR            previous .v -> {blk}.up (.upc)
           y = (y + res) / sqrt2   score decoder, res = the matching encoder .v; the bias is added AFTER the filter
    st     1x1 over the space-to-depth tensor, K = C R up to 5120, no prologue                cond.s2d{i} -> cond.st{i}
    sc     signal_cond_proj 1x1, no prologue                                                 cond.c{j} -> cond.sc{j}
    mel    Conv1d k3 over the mel frames, the input scaled by mel_scale[b]                    cond.mel, mel_scale -> cond.melconv

The FIR has 'same' zero padding at the ends of the row's buffer.  A transposed conv is r phase GEMMs: row co r + ph of the packed
weight gives sample q r + ph of channel co.

u = 2^-24.  Bound kinds, none tuned; which one a launch gets is `kind_of(variant code, layer, form)`:

* chain    one conv from the tap it read: (n + 2 + p) u A + 1/2 ulp, n = Cin KW (up convs: Cin per phase row), A = sum |w| |a| +
           |bias| in float64, p = 1 per rounded prologue product (PReLU, in_scale).  Every family's single-launch forms: the LDS
           conv_mfma_kernel (variant code < 40), conv_direct_kernel<1, ..> 6x / 7x and conv_direct_strided_kernel 9x,
           conv_direct3s_kernel 26x, conv_direct4_kernel 3xx, and rate_down_kernel 42 / rate_up_kernel 47 without a FIR.
           The residual of the score decoder is propagated exactly as conv_fp64._epilogue does.
* down_fir rate_down_kernel with its FIR (42 on a fir_mode 1 layer): the filtered tile lives in LDS only.  Composed in float64
           from {blk}.v: xf = FIR(prelu(x)), e1 = (ntaps + 2 + 1) u sum |f| |a| at the reference's xf, + u |xf| for its fp32
           rounding on the way through LDS; y = conv(xf) + bias, e = (n + 2) u (sum |w| |xf| + |bias|) + sum |w| (e1 + u |xf|).
* up_fir   rate_up_kernel with its FIR (47 on a fir_mode 2 layer) and the fused up-FIR epilogue of the first-generation kernel
           (6x / 7x with ConvArgs::fir): the phase-GEMM tile lives in LDS / registers only.  uu = convT(prelu(x)) (no bias),
           e1 = (Cin + 2 + 1) u sum |w| |a|, + u |uu|; y = FIR(uu) + bias, e = (ntaps + 2) u (sum |f| |uu| + |bias|) +
           sum |f| (e1 + u |uu|); then the residual step.
* folded   fir_fold = 3 (fir_mode 3: 3r-tap strided conv with left pad r; fir_mode 4: 3-tap phase GEMMs): the chain bound with
           n = Cin 3r / Cin 3 over the FOLDED weights, + u sum |W_folded| |a| for the packer's single rounding of each folded
           weight, against the UNFOLDED float64 definition.  The folded weights are rebuilt by the packer's formula
           (ou_model.cpp, CK_DOWN / CK_UP) and held bit for bit against the blob (`check_against_blob`).
* wino     the mel conv is a stride-1 k3 layer with Cin % 16 == 0, so at batch 1 the launcher gives it to conv_direct4w_kernel
           (613 / 623): conv_fp64's minimal-filtering bound with p = 1 for in_scale, U held against the blob at wu_off.
* exact    behind a row's own end in a ragged batch every element of every tap of the table is exactly 0 (Report's tails).
           {blk}.fir is the documented exception (down_path: not masked, its k = s = r reader has no halo): this module asserts
           nothing of that tap -- inside the rows it is held by tests/test_gpu_small_fp64.py -- and nothing behind its rows.

Variant codes 42 and 47 (40 + R, 45 + R with R = 2, the only instantiated rate) are no indices of kConvCfgs (ou_conv_mfma.hip:
eight slots, 0 .. 7), so a code below 40 always names the LDS kernel.

Whether a FIR rode along is not in the variant code of the first-generation kernel: the up path allocates {blk}.upc before it asks
the launcher, and only the unfused form writes it.  The GPU test fills that tap with a sentinel between two identical passes:
a tap that still holds the sentinel everywhere was not written (fused form, {blk}.up is held at the up_fir bound from the block's
input); otherwise it is held element-wise as the unfused conv's output (no bias, no residual) -- a partly written tap fails there.

What the bounds can NOT see.  A relative defect of the residual scale (0.7071 for 1/sqrt2: 161 u) shows where u n A < 161 u |res|:
on every up conv (n = 64 .. 768) for a sizeable residual, but the same few hundred u on the 5120-deep st convs (n u A ~ 5120 u A)
are not visible.  down_fir / up_fir: the propagated first-stage term sum |w| e1 is about ntaps / 2 times a single chain bound, so
one wrong FIR tap by a few u hides; a wrong halo frame, padding mode or phase order moves an output by a whole product and shows.
folded: one folded weight off by an ulp is invisible to the output bound (u sum |W| |a| is allowed for it) -- that is what the blob
identity holds instead.

Not reached by the shipped topologies: rate_up_kernel's scalar store loop (Tout % 4 != 0; padded lengths are multiples of tot_ds,
itself a multiple of 4).  rate_down_kernel / rate_up_kernel are built for R = 2 at 32 -> 64 and 48 -> 96 channels only, so an
odd tot_ds (no factor 2) or another width never reaches them: the loop runs in case r27 of tests/offlist_cases.py alone (rates
[2, 7] at 32 channels, T = 14, 42, 182: 2 modulo 4), where tests/test_gpu_offlist.py asserts that both kernels took the outermost
level of both networks -- with the FIR (score) and without (conditioner) -- and holds them with the bounds of this module; there
rate_down_kernel's rows also start 8 bytes off a 16-byte boundary.  The other off-list models (tot_ds 21, 63; rate factors 6, 7)
are held on whichever family takes their layers (tests/golden/offlist_variants.json).
conv_direct_strided_kernel with folded weights (G = 3) is not built: folded layers run on the LDS kernel.

No element is excluded: `excluded == 0` is asserted of every report.
"""
import torch
import torch.nn.functional as Fn

import conv_fp64 as C
from open_universe_amd import variants as V
import small_fp64 as F
from conv_fp64 import Epi, _epilogue
from small_fp64 import U, Report, prelu, valid_mask  # noqa: F401  (one convention, one implementation)


# ---- which family a variant code names ----------------------------------------------------------------------------------------
# (the mel conv is a stride-1 k3 layer: the minimal-filtering families of the body convs take it)
_FAMILIES = ("rate_down", "rate_up", "lds", "direct2", "direct", "strided", "direct3s", "direct4", "direct2w", "direct3w", "direct4w")


def family_of(cfg):
    """Kernel family of a variant code on a rate-change / 1x1 layer: the library's name, which has to be one such a layer can get."""
    fam = V.family_of(cfg)
    assert fam in _FAMILIES, f"variant code {cfg} is no rate-change / 1x1 family"
    return fam


def kind_of(cfg, fir_mode, fused_fir):
    """Bound kind of a launch: variant code, the layer's fir_mode (plan_json) and -- up convs -- whether the FIR rode along.
    40 + R / 45 + R (42, 47) do not collide with an index of kConvCfgs (0 .. 7): below 40 is the LDS kernel and nothing else."""
    fam = family_of(cfg)
    if fir_mode in (3, 4):
        assert fam in ("lds", "direct", "direct3s", "direct4", "strided"), (cfg, fir_mode)
        return "folded"
    if fam == "rate_down":
        return "down_fir" if fir_mode == 1 else "chain"
    if fam == "rate_up":
        return "up_fir" if fir_mode == 2 else "chain"
    if fused_fir:
        assert fam == "direct", (cfg, "only the first-generation kernel has the fused up-FIR epilogue")
        return "up_fir"
    return "chain"


# ---- parameters -----------------------------------------------------------------------------------------------------------------
class RateL:
    """One rate-change conv as the library holds it.  down: w (Cout, Cin, r); up: w (Cin, Cout, r) (ConvTranspose1d, weight norm
    over the input channels).  `f`: the FIR taps or None; `b`: the bias (added after the filter)."""

    def __init__(self, sd, q, tap, up):
        p = q + ".rate_change_conv"
        self.name, self.tap, self.up = p, tap, up
        self.w64 = C._eff_weight64(sd, p + ".conv")
        self.w = self.w64.float()
        self.r = self.w.shape[-1]
        self.Cin, self.Cout = (self.w.shape[0], self.w.shape[1]) if up else (self.w.shape[1], self.w.shape[0])
        self.aa = p + ".low_pass_filter.weights" in sd
        self.f = sd[p + ".low_pass_filter.weights"].float() if self.aa else None
        self.b = sd[p + (".bias" if self.aa else ".conv.bias")].float()
        self.alpha = sd[p + ".prelu.weight"].float().reshape(())

    def rows(self):
        """The packed GEMM rows of the unfolded layer, (M, Cin, KW): down (Cout, Cin, r); up row co r + ph = w[ci, co, ph]."""
        if not self.up:
            return self.w
        return self.w.permute(1, 2, 0).reshape(self.Cout * self.r, self.Cin, 1)

    def folded64(self, reverse_fir=False):
        """The packer's folded weights in double, its own summation order (ou_model.cpp CK_DOWN / CK_UP), before the rounding.
        down: W2[co, ci, k + j] += w[co, ci, k] f[j] (k ascending); up: W3[co r + ph, ci, dq + 1] += f[j] w[ci, co, pp] with
        s = ph + j - r, dq = floor(s / r) in -1 .. 1, pp = s - dq r (j ascending).  `reverse_fir`: the defect of the CPU tests."""
        r = self.r
        f = self.f.double().flip(0) if reverse_fir else self.f.double()
        if not self.up:
            W = torch.zeros(self.Cout, self.Cin, 3 * r, dtype=torch.float64)
            for k in range(r):
                W[..., k: k + 2 * r + 1] += self.w64[..., k: k + 1] * f
            return W
        W = torch.zeros(self.Cout, r, self.Cin, 3, dtype=torch.float64)
        wt = self.w64.permute(1, 2, 0)                                   # (Cout, r, Cin)
        for ph in range(r):
            for j in range(2 * r + 1):
                s = ph + j - r
                dq = -1 if s < 0 else (1 if s >= r else 0)
                W[:, ph, :, dq + 1] += f[j] * wt[:, s - dq * r, :]
        return W.reshape(self.Cout * r, self.Cin, 3)


class OneByOne:
    """st / sc / mel conv: fp32 effective weight (Cout, Cin, KW), bias."""

    def __init__(self, sd, p, tap, src, flat=False):
        self.name, self.tap, self.src = p, tap, src
        w64 = C._eff_weight64(sd, p)
        w = w64.float()
        self.w = w.reshape(w.shape[0], -1, 1) if flat else w    # st: (OC, C, R) == (OC, C R, 1), kk = ci R + k
        self.b = sd[p + ".bias"].float()
        self.KW = self.w.shape[-1]
        if self.KW in C.G:  # (the packer's transformed weights U = fl(G w) of a k3 / k5 layer, as conv_fp64.ConvP builds them)
            u = torch.zeros(*w64.shape[:2], self.KW + 1, dtype=torch.float64)
            for k in range(self.KW):
                u = u + C.G[self.KW][:, k] * w64[..., k:k + 1]
            self.U = u.float()


class RateParams:
    """The rate-change convs, st / sc / mel convs of one model in walk order, and the walk itself (`slots`)."""

    def __init__(self, spec, sd):
        self.spec = spec
        cp, sp = "condition_model", spec.score_prefix
        self.rate, self.one = {}, {}
        self.src, self.res = {}, {}
        prev = None
        for p, q, inp, fidx, add, c1n, vn, ex in C.blocks_of(spec):
            if q + ".rate_change_conv.conv.bias" in sd or q + ".rate_change_conv.bias" in sd:
                up = ".decoder." in q
                self.rate[p] = RateL(sd, q, p, up)
                self.src[p] = prev if up else vn
            if p == "cond.decin":
                prev = vn
            elif p.startswith(("cond.dec", "score.dec")):
                prev = vn
        n = len(spec.cond.rate_factors)
        ns = len(spec.score.rate_factors)
        nbs = ns + int(spec.score.extra_conv_block)
        # the first up conv of the score decoder reads the GRU's output (or, with an extra block, decoder block 0's)
        ups = [p for p in self.rate if p.startswith("score.dec")]
        if ups and not spec.score.extra_conv_block:
            self.src[ups[0]] = "score.gru"
        for p in ups:
            j = int(p[len("score.dec"):])
            self.res[p] = f"score.enc{nbs - 1 - j}.v"
        self.st_alpha = []
        for i in range(n - 1):
            self.one[f"cond.st{i}"] = OneByOne(sd, f"{cp}.encoder.st_convs.{i}.conv", f"cond.st{i}", f"cond.s2d{i}", flat=True)
            self.st_alpha.append(sd[f"{cp}.encoder.st_convs.{i}.prelu.weight"].float().reshape(()))
        for j in range(nbs):
            self.one[f"cond.sc{j}"] = OneByOne(sd, f"{sp}.decoder.signal_cond_proj.{j}", f"cond.sc{j}", f"cond.c{j}")
        self.one["cond.melconv"] = OneByOne(sd, cp + ".input_mel.conv", "cond.melconv", "cond.mel")
        self.body_C = {p: sd[q + ".conv1.conv.bias"].numel() for p, q, *_ in C.blocks_of(spec)}
        self.v_tap = {p: vn for p, q, i, f, a, c1n, vn, ex in C.blocks_of(spec)}
        self.slots = walk_slots(spec)

    def plan_name(self, key):
        """Name of the layer in plan_json."""
        if key in self.rate:
            return self.rate[key].name
        name = self.one[key].name
        return name[:-len(".conv")] if key.startswith("cond.st") else name

    def check_against_blob(self, blob, plan):
        """The rebuilt parameters are the library's, bit for bit, at plan_json's offsets: the packed rows (w_off; folded layers:
        the packer's formula), bias (b_off; fir_mode 2: fbias_off, the conv's own bias slot all 0), slope (a_off) and FIR taps
        (fir_off) of every rate-change conv; weight and bias of the st / sc / mel convs and the st convs' slopes."""
        convs = {c["name"]: c for c in plan["convs"]}

        def rows_of(L, Cin, KW, M):
            wk = blob[L["w_off"]: L["w_off"] + Cin * KW * L["Mp"]].view(Cin // L["CK"], KW, L["CK"], L["Mp"])[..., :M]
            return wk.permute(3, 0, 2, 1).reshape(M, Cin, KW)
        for key, rl in self.rate.items():
            L = convs[rl.name]
            mode = L["fir_mode"]
            assert (L["Cin"], L["Cout"], L["rate"], L["M"]) == (rl.Cin, rl.Cout, rl.r, rl.Cout * (rl.r if rl.up else 1)), rl.name
            assert (mode != 0) == rl.aa, rl.name
            W = rl.folded64().float() if mode in (3, 4) else rl.rows()
            assert L["KW"] == W.shape[-1], rl.name
            bad = first_wrong(rows_of(L, rl.Cin, L["KW"], L["M"]), W)
            assert bad is None, (rl.name, "packed weight differs from the packer's formula at (row, channel, tap)", bad)
            assert torch.equal(blob[L["a_off"]], rl.alpha), rl.name
            if mode == 2:
                assert not bool(blob[L["b_off"]: L["b_off"] + rl.Cout].any()), rl.name
                assert torch.equal(blob[L["fbias_off"]: L["fbias_off"] + rl.Cout], rl.b), rl.name
            else:
                assert torch.equal(blob[L["b_off"]: L["b_off"] + rl.Cout], rl.b), rl.name
            if mode in (1, 2):
                assert torch.equal(blob[L["fir_off"]: L["fir_off"] + 2 * rl.r + 1], rl.f), rl.name
        for key, ol in self.one.items():
            L = convs[self.plan_name(key)]
            Cout, Cin, KW = ol.w.shape
            assert (L["Cin"], L["Cout"], L["KW"]) == (Cin, Cout, KW), ol.name
            bad = first_wrong(rows_of(L, Cin, KW, Cout), ol.w)
            assert bad is None, (ol.name, "packed weight differs at (row, channel, tap)", bad)
            assert torch.equal(blob[L["b_off"]: L["b_off"] + Cout], ol.b), ol.name
            if L["KWP"]:
                bad = C.first_wrong_u(blob, L, ol)
                assert bad is None, (ol.name, "transformed weight differs from fl(G w) at blob offset", bad)
            if key.startswith("cond.st"):
                assert torch.equal(blob[L["a_off"]], self.st_alpha[int(key[len("cond.st"):])]), ol.name


def first_wrong(got, want):
    """(row, channel, tap) of the first element of `got` that is not `want`, or None."""
    ne = (got != want).reshape(-1)
    if not bool(ne.any()):
        return None
    return tuple(int(v) for v in torch.unravel_index(ne.int().argmax(), want.shape))


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
def _gemm(a, W, stride=1, pad=0, dtype=torch.float64):
    """conv of (B, Cin, T) with packed rows (M, Cin, KW): left pad `pad`, right pad so that T / stride columns come out."""
    KW = W.shape[-1]
    T = a.shape[-1]
    right = (T // stride - 1) * stride + KW - pad - T
    return Fn.conv1d(Fn.pad(a.to(dtype), (pad, max(right, 0))), W.to(dtype), stride=stride)


def _phases(y, r):
    """(B, Cout r, Q) phase rows -> (B, Cout, Q r): row co r + ph is sample q r + ph of channel co."""
    B, M, Q = y.shape
    return y.reshape(B, M // r, r, Q).permute(0, 1, 3, 2).reshape(B, M // r, Q * r)


def _fir(v, f, dtype=torch.float64):
    """y[c, t] = sum_j f[j] v[c, t + j - r], zeros outside the row's buffer."""
    B, Cc, T = v.shape
    r = (f.numel() - 1) // 2
    return Fn.conv1d(v.to(dtype).reshape(B * Cc, 1, T), f.to(dtype).reshape(1, 1, -1), padding=r).reshape(B, Cc, T)


def _mask(ref, e, lens):
    if lens is None:
        return ref, e
    m = valid_mask(lens, ref.shape[0], ref.shape[-1])
    return ref * m, e * m


def conv_1x1(x, ol, in_scale=None, lens=None, dtype=torch.float64, wino=False):
    """st / sc / mel conv from the tap it read -> (ref, bound).  chain, n = Cin KW, p = 1 with in_scale (one rounded product per
    operand; the reference scales exactly).  `wino`: the launch ran on a minimal-filtering family (4xx .. 7xx): conv_fp64's
    minimal-filtering bound, (n + 2) u A_uv + (p + t) u A_bt with n = (KW + 1) Cin over the transformed products."""
    Cout, Cin, KW = ol.w.shape
    a = x.to(dtype)
    p = 0
    if in_scale is not None:
        a = a * in_scale.to(dtype).reshape(-1, 1, 1)
        p = 1
    pad = (KW - 1) // 2
    bias = ol.b.to(dtype)[None, :, None]
    v = _gemm(a, ol.w, 1, pad, dtype) + bias
    if dtype != torch.float64:
        return v, None
    if wino:
        A_uv, A_bt = C.wino_abs(a, ol)
        return _mask(v, ((KW + 1) * Cin + 2) * U * (A_uv + bias.abs()) + (p + C.BT_ROUNDINGS[KW]) * U * A_bt, lens)
    A = _gemm(a.abs(), ol.w.abs(), 1, pad) + bias.abs()
    return _mask(v, (Cin * KW + 2 + p) * U * A, lens)


def down(x, rl, form, lens=None, dtype=torch.float64, hook=None, W=None):
    """The down rate-change conv -> (ref, bound), (B, Cout, T / r).  form:
    'conv'      from {blk}.v, PReLU in the conv, no FIR in the layer (conditioner)                       chain, p = 1
    'after_fir' from {blk}.fir (the FIR pass applied PReLU and filter), act = 0                         chain, p = 0
    'fused'     from {blk}.v, FIR inside the kernel (rate_down_kernel)                                  down_fir
    'folded'    from {blk}.v, the 3r-tap conv with left pad r over the folded weights                   folded
    The reference of 'folded' is the unfolded definition.  `hook(stage, tensor)` may damage an intermediate (CPU tests);
    `W`: other folded weights than the packer's (CPU tests: the emulation's arithmetic, dtype float32)."""
    r = rl.r
    hook = hook or (lambda stage, t: t)
    bias = rl.b.to(dtype)[None, :, None]
    n = rl.Cin * r
    if form == "after_fir":
        xf = x.to(dtype)
        v = _gemm(hook("fir", xf), rl.w, r, 0, dtype) + bias
        if dtype != torch.float64:
            return v, None
        return _mask(v, (n + 2) * U * (_gemm(xf.abs(), rl.w.abs(), r) + bias.abs()), lens)
    a = prelu(x.to(dtype), rl.alpha.to(dtype))
    if form == "conv":
        v = _gemm(a, rl.w, r, 0, dtype) + bias
        if dtype != torch.float64:
            return v, None
        return _mask(v, (n + 3) * U * (_gemm(a.abs(), rl.w.abs(), r) + bias.abs()), lens)
    if dtype != torch.float64 and form == "folded":  # (the emulation of the folded ALGORITHM)
        Wf = rl.folded64().float() if W is None else W
        return _gemm(a, Wf, r, r, dtype) + bias, None
    xf = hook("fir", _fir(a, rl.f, dtype))
    v = _gemm(xf, rl.w, r, 0, dtype) + bias
    if dtype != torch.float64:
        return v, None
    if form == "fused":
        e1 = (rl.f.numel() + 3) * U * _fir(a.abs(), rl.f.abs()) + U * xf.abs()
        e = (n + 2) * U * (_gemm(xf.abs(), rl.w.abs(), r) + bias.abs()) + _gemm(e1, rl.w.abs(), r)
    else:
        assert form == "folded", form
        Wa = rl.folded64().float().double().abs()
        S = _gemm(a.abs(), Wa, r, r)
        e = (rl.Cin * 3 * r + 3) * U * (S + bias.abs()) + U * S
    return _mask(v, e, lens)


def up(x, rl, form, res=None, lens=None, dtype=torch.float64, hook=None, W=None, bias_first=False):
    """The up rate-change conv -> (ref, bound), (B, Cout, T r).  form:
    'conv'     no FIR in the layer (conditioner): phase GEMMs + bias (+ residual)                       chain, n = Cin, p = 1
    'upc'      the unfused conv of an anti-aliased layer: phase GEMMs alone, no bias, no residual       chain, n = Cin, p = 1
    'fused'    FIR, bias and residual inside the kernel (rate_up_kernel, the fused up-FIR epilogue)    up_fir
    'folded'   3-tap phase GEMMs over the folded weights, bias, residual                                folded
    `hook(stage, tensor)`: stages 'gemm' (the phase rows (B, Cout r, Q) before they are interleaved) and 'u' (the up-sampled
    signal); `bias_first`: the bias added before the filter (both: defects of the CPU tests)."""
    r = rl.r
    hook = hook or (lambda stage, t: t)
    a = prelu(x.to(dtype), rl.alpha.to(dtype))
    bias = rl.b.to(dtype)[None, :, None]
    rows = rl.rows()
    ep = Epi(res=res)
    if dtype != torch.float64 and form == "folded":
        Wf = rl.folded64().float() if W is None else W
        v, _ = _epilogue(_phases(_gemm(a, Wf, 1, 1, dtype), r) + bias, None, ep, dtype)
        return v, None
    uu = hook("u", _phases(hook("gemm", _gemm(a, rows, 1, 0, dtype)), r))
    Au = _phases(_gemm(a.abs(), rows.abs()), r) if dtype == torch.float64 else None
    if form in ("conv", "upc"):
        if form == "upc":
            bias = torch.zeros_like(bias)
            ep = Epi()
        v = uu + bias
        e = (rl.Cin + 3) * U * (Au + bias.abs()) if Au is not None else None
    elif form == "fused":
        v = _fir(uu + bias, rl.f, dtype) if bias_first else _fir(uu, rl.f, dtype) + bias
        e = None
        if Au is not None:
            e1 = (rl.Cin + 3) * U * Au + U * uu.abs()
            e = (rl.f.numel() + 2) * U * (_fir(uu.abs(), rl.f.abs()) + bias.abs()) + _fir(e1, rl.f.abs())
    else:
        assert form == "folded", form
        v = _fir(uu, rl.f, dtype) + bias
        Wa = rl.folded64().float().double().abs()
        S = _phases(_gemm(a.abs(), Wa, 1, 1), r)
        e = (rl.Cin * 3 + 3) * U * (S + bias.abs()) + U * S
    v, e = _epilogue(v, e, ep, dtype)
    if dtype != torch.float64:
        return v, None
    return _mask(v, e, lens)


# ---- the walk and its pairing with the profile records ----------------------------------------------------------------------
def walk_slots(spec):
    """Every profiled launch of one conditioner pass and one score pass in the order the host enqueues them (run_condition,
    run_score_enc / run_score_dec; option no_overlap = 1): [(network, kind, key)], kind: 'body' (1 - 3 records of a ConvBlock),
    'rate' / 'conv' (one record of a layer of this module), 'gruproj' (one record), 'rec' (one record, variant >= 1000)."""
    c, s = spec.cond, spec.score
    n, ns = len(c.rate_factors), len(s.rate_factors)
    nb, nbs = n + int(c.extra_conv_block), ns + int(s.extra_conv_block)
    out = [("cond", "conv", "cond.melconv"), ("cond", "body", "cond.melblock")]
    for i in range(nb):
        out.append(("cond", "body", f"cond.enc{i}"))
        if i < n:
            out.append(("cond", "rate", f"cond.enc{i}"))
        if i < n - 1:
            out.append(("cond", "conv", f"cond.st{i}"))
    out += [("cond", "body", "cond.cb1"), ("cond", "gruproj", "cond.gru0"), ("cond", "rec", "cond.gru0"),
            ("cond", "gruproj", "cond.gru"), ("cond", "rec", "cond.gru"), ("cond", "body", "cond.cb2"), ("cond", "body", "cond.decin")]
    for j in range(nb):
        if not (c.extra_conv_block and j == 0):
            out.append(("cond", "rate", f"cond.dec{j}"))
        out += [("cond", "body", f"cond.dec{j}"), ("cond", "conv", f"cond.sc{j}")]
    for i in range(nbs):
        out.append(("score", "body", f"score.enc{i}"))
        if i < ns:
            out.append(("score", "rate", f"score.enc{i}"))
    out += [("score", "gruproj", "score.gru"), ("score", "rec", "score.gru")]
    for j in range(nbs):
        if not (s.extra_conv_block and j == 0):
            out.append(("score", "rate", f"score.dec{j}"))
        out.append(("score", "body", f"score.dec{j}"))
    return out


def _is_body(cfg):
    return not V.is_recurrence_record(cfg) and V.family_of(cfg) not in ("direct4", "direct3s", "rate_down", "rate_up")


def pair_walk(slots, records, flops_of, score_passes=1):
    """Walk order -> {(pass, key): variant code} for the 'rate' / 'conv' slots.  records: [(ms, flops, bytes, variant)] of one
    conditioner pass and `score_passes` score passes.  flops_of[(kind, key)]: algorithmic FLOPs of the slot (body: the three convs').
    The profile record carries no layer name and FLOPs collide (the first down conv and the last up conv have the same count), so
    the records are consumed strictly in walk order; the body records (1 - 3 per block, sums of its convs' FLOPs) and the
    recurrences (variant >= 1000) are the anchors.  A record that cannot be paired -- wrong FLOPs for its slot, a recurrence
    where a conv is due, records left over or missing -- fails."""
    seq = [(0, s) for s in slots if s[0] == "cond"]
    for k in range(score_passes):
        seq += [(k, s) for s in slots if s[0] == "score"]
    out, i = {}, 0
    for pas, (net, kind, key) in seq:
        assert i < len(records), (key, "the profile ended before this launch")
        cfg = records[i][3]
        if kind == "rec":
            assert V.is_recurrence_record(cfg), (key, i, "a recurrence is due here, the record says variant", cfg)
            i += 1
        elif kind == "gruproj":
            assert not V.is_recurrence_record(cfg), (key, i, cfg)
            i += 1
        elif kind == "body":
            fl = flops_of[(kind, key)]
            for pat in ([sum(fl)], [fl[0], fl[1] + fl[2]], list(fl)):
                got = records[i: i + len(pat)]
                if len(got) == len(pat) and all(_is_body(r[3]) and r[1] == f for r, f in zip(got, pat)) and \
                        all((V.family_of(r[3]) == "fused") == (len(pat) < 3 and k == len(pat) - 1) for k, r in enumerate(got)):
                    i += len(pat)
                    break
            else:
                raise AssertionError((key, i, "no body records here", [(r[1], r[3]) for r in records[i: i + 3]], fl))
        else:
            want = flops_of[(kind, key)]
            assert not V.is_recurrence_record(cfg) and records[i][1] == want, (key, i, "record", (records[i][1], cfg), "expected FLOPs", want)
            family_of(cfg)
            out[(pas, key)] = cfg
            i += 1
    assert i == len(records), ("records left over behind the walk", [(r[1], r[3]) for r in records[i: i + 4]])
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------
MODELS = ("PP16", "PP24")
# tag -> (options, model objects' fir_fold, families the case is about).  Which layers each family has to take in each case:
# tests/golden/rate_fp64_variants.json.
FAMILIES = {
    "default": (dict(), 0, ("rate_down", "rate_up", "direct4")),
    "d4_fir0": (dict(d4_fir=0), 0, ("direct4", "direct")),
    "d4_short0": (dict(d4_short=0), 0, ("direct4", "direct", "strided")),
    "gen1": (dict(conv_direct=3), 0, ("direct", "strided")),
    "gen1.unfused": (dict(conv_direct=3, fuse_upfir=0), 0, ("direct", "strided")),
    "direct3s": (dict(tile_min=0.01), 0, ("direct3s",)),
    "lds": (dict(conv_direct=0), 0, ("lds",)),
    "rate_small0": (dict(rate_small=0), 0, ("direct4", "direct", "strided")),
    "folded": (dict(), 3, ("lds", "direct4", "direct")),
}
FAMILIES.update({f"d4_force{s}": (dict(d4_force=s), 0, ("direct4",)) for s in (20, 21, 22, 23, 40, 41, 42, 43)})
# (frames, batch).  1 frame: PP16's level lengths 160, 80, 20, 5, 1 -- rate_down (64 output frames per block) one full and one
# partial block, rate_up with FIR (62 finished frames) 62 + 18, the deepest levels shorter than a conv_direct4 column tile; 3: odd
# deepest levels; 4: rate_down exactly full (PP16 320 = 5 x 64, PP24 480 = 15 x 32), rate_up without FIR exactly full; 13: 65 =
# 64 + 1 and 260 columns; 31: PP16's rate_up with FIR exactly full (2480 = 40 x 62: its last block ends on the row's last frame,
# its halo frame lies outside the signal); 64 / 65: the latent level on a 64-column tile and one past it.
DEFAULT_SHAPES = ((1, 1), (1, 4), (3, 4), (4, 1), (13, 1), (13, 4), (31, 1), (31, 4), (64, 4), (65, 1))
_SHAPES = {
    "default": DEFAULT_SHAPES,
    "d4_fir0": ((1, 1), (13, 1), (64, 4)), "d4_short0": ((1, 1), (13, 1), (64, 4)),
    "gen1": ((1, 1), (13, 4), (31, 1), (65, 1)), "gen1.unfused": ((1, 1), (13, 4), (31, 1), (65, 1)),
    "direct3s": ((13, 4), (31, 4), (64, 4), (65, 4)),
    "lds": ((1, 1), (13, 4), (31, 1), (65, 4)),
    "rate_small0": ((1, 1), (4, 4), (31, 1), (65, 4)),
    "folded": ((1, 1), (3, 4), (31, 1), (65, 4)),
}
CASES = [(tag, m, B, f) for tag in _SHAPES for m in MODELS for f, B in _SHAPES[tag] if not (tag == "folded" and m != "PP16")]
CASES += [(f"d4_force{s}", "PP16", B, f) for s in (20, 21, 22, 23) for f, B in ((1, 1), (13, 4), (65, 1))]
CASES += [(f"d4_force{s}", "PP24", 1, 13) for s in (20, 21, 22, 23)]
CASES += [(f"d4_force{s}", "PP16", 1, 13) for s in (40, 41, 42, 43)]
RAGGED = [(m, mf, rs) for m in MODELS for mf in (0, 1) for rs in (1, 0)]   # (model, mask_fused, rate_small)
RAGGED_ROWS = C.RAGGED_ROWS


def case_id(tag, name, B, frames):
    return f"{tag}.{name}.b{B}.f{frames}"
