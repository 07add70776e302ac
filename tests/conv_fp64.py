"""float64 references of the ConvBlock body convs (conv1 k5, conv2 k3, conv3 k3 of every block of both networks) for the tests,
written from the operation's definition on the library's tap layout, each with a per-element bound.  Teacher-forced like
tests/small_fp64.py (whose Report, ulp32, valid_mask, eff_weight, prelu, levels, classes_of and chain convention are used, not
copied): the reference of a conv takes the tap the kernel read and the taps of its epilogue operands.

One body conv, in the order every kernel family applies it (ou_kernels.h, "epi(v)"):

    a = prelu(x; alpha)            unless the producer stored x activated (ConvArgs::out_act, see `stores_activated`)
    v = sum_ci sum_k w[co, ci, k] a[ci, t + k - pad] + bias[co]                  zero padding at the row's ends
    v = (v + add) * 1/sqrt2        conv1 of the score decoder: add = cond.sc{j}
    v = gamma v + beta             conv1 of the score network: FiLM rows of sigma.film, gamma at [off + co], beta at [off + C + co]
    v = (v + hu) * 1/sqrt2         conv3: hu = the block's input at its own rate (.up, or the previous tap for a dir-0 block)
    v = prelu(v; alpha_next)       when the tap is stored activated

u = 2^-24.  Bound kinds, none tuned; which family takes which is `kind_of(variant code)`:

* chain  (LDS conv_mfma_kernel < 50, conv_direct 5x-7x, conv_direct2 66 / 67 / 76 / 77, conv_direct3 2xx; split-K partial sums
  are "any order"): the project's chain bound, e0 = (n + 2 + p) u A, n = Cin KW, A = sum |w| |a| + |bias| in float64 (a second
  conv with absolute values), p = 1 with the PReLU prologue (one rounded product per operand; the reference activates exactly).
  Epilogue, build with -ffp-contract=off so every operation rounds once, each step (v + o) * s: e <- (e + u |v + o|) s + u |result|;
  FiLM: e <- |gamma| e + u |gamma v| + u |gamma v + beta|; the activating store: e <- max(1, |alpha|) e + u |result|; + 1/2 ulp of the
  stored value (Report).  ROUTE: derived.
* minimal filtering  (conv_direct2w 4xx, conv_direct3w 5xx, conv_direct4w 6xx / 7xx, the fused body conv_chainw 19x): outputs
  in pairs, y[2p + j] = sum_x AT[j, x] sum_ci U_x[co, ci] V_x[ci, p], V = BT d, d = a[2p - pad .. 2p - pad + KW], U = G w.
      F(2,3)  G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]   BT = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]]
              AT = [[1,1,1,0],[0,1,-1,-1]]
      F(2,5)  G = [[1/2,0,0,0,0],[1/6]*5,[1/6,-1/6,1/6,-1/6,1/6],[16/15,8/15,4/15,2/15,1/15],[1/30,-1/15,2/15,-4/15,8/15],[0,0,0,0,1/2]]
              BT = [[2,-3,-4,3,2,0],[0,-2,1,5,2,0],[0,-2,5,-1,-2,0],[0,2,1,-2,-1,0],[0,1,-2,-1,2,0],[0,2,-3,-4,3,2]]
              AT = [[1,1,1,1,1,0],[0,1,-1,1/2,-2,1]]                       (ou_model.cpp store_conv, ou_dev.h wino_bt)
  U is G w of the double effective weight rounded ONCE by the packer (held bit for bit against the blob at plan_json's wu_off: `check_against_blob`), so
  U is exact data.  AT's entries are powers of two: y is a sum of n = (KW + 1) Cin products U V scaled exactly, accumulated in
  fp32 in some order (independent accumulators per x, A^T per wave, K slices met in LDS): the chain form over the TRANSFORMED
  products, (n + 2) u A_uv with A_uv = sum_x |AT[j, x]| sum_ci |U_x| |V_x| + |bias|.  The roundings of V itself are relative to
  A_bt = sum_x |AT[j, x]| sum_ci |U_x| (sum_i |BT[x, i]| |d_i|), the inner absolute sum, because V may cancel: the PReLU product
  of d (p) and wino_bt's t roundings along V's longest dependency (k3: one subtraction, t = 1; k5: nested fmaf,
  2 (X0 + X4) -> fmaf 3 (..) -> fmaf -4: an add, a subtraction inside the fmaf operand and
  two fmaf roundings, t = 4).  e0 = (n + 2) u A_uv + (p + t) u A_bt.  Rows of odd length: the last pair's second column lies behind the row
  (its window reads zeros there) and is not stored.  ROUTE: derived.  What this bound can NOT see: one U value off by an ulp moves
  an output by ~2 u |w a|, n times less than the bound allows -- that defect is held by the blob identity instead.
* bf16 split  (conv_split_kernel 8xx): a = ah + am + al and w = wh + wm + wl, bf16 pieces by round-to-nearest-even
  (ou_split_pack.h split3, the kernel's split_pair); the kernel keeps ah wh, ah wm, am wh, ah wl, am wm, al wh and drops am wl,
  al wm, al wl.  With |am| <= 2^-9 (1 + 2^-9) |a|, |al| <= 2^-18 (1 + 2^-9) |a| and the three-piece residual <= 2^-27 |a| the
  dropped part of a product is below (2 x 2^-27 + 2^-36 + 2 x 2^-27) (1 + 2^-8) |a w| < 1/2 u |a w|.  That part IS derived; what
  is not is the accumulation: 6 n piece products through 16-deep bf16 MFMAs whose internal order and rounding points are not
  documented -- the rigorous "any order" constant 6 n would be six times the chain bound and blind to a dropped smallest piece
  (2^-18 per product = 64 u).  ROUTE: M x e32, e32 = max |fp32 emulation - float64| of the SAME algorithm (`split_fp32`: the
  three pieces, the six kept products, accumulated in the kernel's documented order, one rounding per 16-deep instruction) from the same inputs with the same epilogue, + the derived 1/2 u A of
  the dropped products, + 1/2 ulp.  M_SPLIT below, from the measured ratios of profiles/conv_fp64_observed.json.
* fused body (19x): the convs composed in float64 from the block's input; every stage's own minimal-filtering bound at the
  reference's intermediate values, the previous stage's bound propagated to first order through the next conv:
  e_in = max(1, |alpha|) e_prev (the PReLU is Lipschitz), e0 += sum |w| e_in.  depth 3 (C = 32): .up -> .v (and the raw conv1
  result where it is a condition: cond.c{j}); depth 2 (C = 64): .c1 -> .v.  The interior taps (.c1 / .c2 of a depth-3 body, .c2
  of a depth-2 body) live in LDS only: NOT observable, nothing holds them element-wise but the composed output.
* exact: behind a row's own end in a ragged batch every element of every tap is exactly 0 (Report's tails), whichever of
  mask_fused 0 / 1 placed it.

In the default build conv_chainw_kernel is the only fused body and chainw_kind() refuses it whenever fuse_nc is set: option
fuse_nc 128 / 256 selects conv_chain_kernel variants that exist in `make EXPERIMENTS=1` builds only, so those two tile widths
are not reachable by this suite (the fused tile widths in use are conv_chainw's own 252 / 126 finished columns).

Sensitivity: a relative defect of the residual scale (0.7071 for 1/sqrt2: 161 u) shows where u n A < 161 u |hu| -- on the narrow
levels (n = 96 .. 480) for every sizeable hu, on the 512-channel levels only where the conv's products are small against hu.

No element is excluded: `excluded == 0` is asserted of every report.
"""
import math

import torch
import torch.nn.functional as Fn

import small_fp64 as F
from open_universe_amd.variants import family_of  # noqa: F401  (the one decoder; the body convs use its names as they are)
from small_fp64 import INV_SQRT2, U, Report, prelu, valid_mask  # noqa: F401  (one convention, one implementation)

# M of the bf16-split bound = ceil(2 x worst measured err / e32) over the split cases of tests/test_gpu_conv_fp64.py on an MI355X
# (profiles/conv_fp64_observed.json, `lib_ratio`); a ratio above small_fp64.M_CAP is a finding, not a tolerance.
# Measured over the split-kernel taps of the split cases: worst err / e32 3.21 (PP16, batch 1, 1 frame, cond.cb1.c2, 512
# channels k3, variant 923), median 1.36 -> M = ceil(2 x 3.21).  What M x e32 can see of a dropped smallest piece (2^-18 per
# product, 64 u, against a chain of 6 n / 16 roundings): a ratio of about 64 / sqrt(6 n / 16) -- 10.7 at n = 96, 7.5 at n = 192,
# 1.7 at n = 3 840: flagged on the narrow layers only.
M_SPLIT = 7

G = {3: torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64),
     5: torch.tensor([[1. / 2, 0, 0, 0, 0], [1. / 6] * 5, [1. / 6, -1. / 6, 1. / 6, -1. / 6, 1. / 6],
                      [16. / 15, 8. / 15, 4. / 15, 2. / 15, 1. / 15], [1. / 30, -1. / 15, 2. / 15, -4. / 15, 8. / 15],
                      [0, 0, 0, 0, 1. / 2]], dtype=torch.float64)}
BT = {3: torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64),
      5: torch.tensor([[2, -3, -4, 3, 2, 0], [0, -2, 1, 5, 2, 0], [0, -2, 5, -1, -2, 0], [0, 2, 1, -2, -1, 0], [0, 1, -2, -1, 2, 0],
                       [0, 2, -3, -4, 3, 2]], dtype=torch.float64)}
AT = {3: torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64),
      5: torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, .5, -2, 1]], dtype=torch.float64)}
BT_ROUNDINGS = {3: 1, 5: 4}


# ---- which family a variant code names, what its tap holds ------------------------------------------------------------------
_KIND = {"fused": ("fused",), "split": ("split",), "wino": ("direct2w", "direct3w", "direct4w"),
         "chain": ("lds", "rate_down", "rate_up", "direct", "direct2", "strided", "direct3", "direct3s")}


def kind_of(cfg):
    """Bound kind of a launch's variant code (open_universe_amd.variants.family_of: the library's own table)."""
    for kind, fams in _KIND.items():
        if family_of(cfg) in fams:
            return kind
    raise AssertionError(f"variant code {cfg} is no body-conv family")


def stores_activated(cfg, requested):
    """Does the tap hold prelu(y; alpha_next)?  `requested`: Runner::body asked for it (option preact, the tensor read by the next
    PReLU_Conv only).  The LDS kernels and the first-generation direct kernels have no activating epilogue (launch_conv /
    launch_conv_direct answer hipErrorNotSupported and the layer is launched again storing y); every other body family has."""
    kind_of(cfg)  # (a body-conv family at all)
    return bool(requested) and family_of(cfg) not in ("lds", "rate_down", "rate_up", "direct", "strided", "fused")


# ---- parameters -------------------------------------------------------------------------------------------------------------
def _eff_weight64(sd, p):
    """small_fp64.eff_weight before its final rounding (store_conv transforms this value): g v / |v| per output row in double."""
    if p + ".weight_g" in sd:
        v = sd[p + ".weight_v"].double()
        g = sd[p + ".weight_g"].double().reshape(-1)
        v2 = v.reshape(v.shape[0], -1).pow(2).T.contiguous()
        nrm = torch.zeros(v.shape[0], dtype=torch.float64)
        for row in v2:  # (the packer's own order: U = fl(G w) is compared bit for bit, so the double sum has to be its sum)
            nrm += row
        return v * (g / nrm.sqrt()).reshape([-1] + [1] * (v.ndim - 1))
    return sd[p + ".weight"].double()


class ConvP:
    """One PReLU_Conv as the library holds it: fp32 effective weight (Cout, Cin, KW), bias, the PReLU slope in front of it, and
    the packer's transformed weights U = fl(G w) (Cout, Cin, KW + 1)."""

    def __init__(self, sd, name):
        self.name = name
        w64 = _eff_weight64(sd, name + ".conv")
        self.w = w64.float()
        self.b = sd[name + ".conv.bias"].float()
        self.alpha = sd[name + ".prelu.weight"].float().reshape(())
        self.KW = self.w.shape[-1]
        # (the packer transforms the DOUBLE effective weight, taps ascending, and rounds once)
        u = torch.zeros(*w64.shape[:2], self.KW + 1, dtype=torch.float64)
        for k in range(self.KW):
            u = u + G[self.KW][:, k] * w64[..., k:k + 1]
        self.U = u.float()


class BlockP:
    def __init__(self, sd, name):
        self.name = name
        self.c = [ConvP(sd, f"{name}.conv{i}") for i in (1, 2, 3)]
        self.C = self.c[0].w.shape[0]


def blocks_of(spec):
    """Every ConvBlock of both networks in walk order (run_condition, run_score_enc / run_score_dec of ou_walk.cpp):
    [(tap prefix, state-dict prefix, input tap or None for '<prefix>.up', film index or None, cond add tap or None, c1 tap, v tap,
    c1 exported)]."""
    cp, sp = "condition_model", spec.score_prefix
    c, s = spec.cond, spec.score
    n = len(c.rate_factors)
    nb = n + int(c.extra_conv_block)
    out = [("cond.melblock", cp + ".input_mel.conv_block", "cond.melconv", None, None, None, None, False)]
    prev = "cond.in"
    for i in range(nb):
        out.append((f"cond.enc{i}", f"{cp}.encoder.ds_modules.{i}", prev, None, None, None, None, False))
        prev = f"cond.enc{i}.h" if i < n else f"cond.enc{i}.v"
    out.append(("cond.cb1", cp + ".encoder.conv_block1", "cond.enc_sum", None, None, None, None, False))
    out.append(("cond.cb2", cp + ".encoder.conv_block2", "cond.gru", None, None, None, "cond.latent", False))
    out.append(("cond.decin", cp + ".decoder.input_conv_block", "cond.latent", None, None, None, None, False))
    prev = "cond.decin.v"
    for j in range(nb):
        up = not (c.extra_conv_block and j == 0)
        v = "cond.aux" if j == nb - 1 else f"cond.dec{j}.v"
        out.append((f"cond.dec{j}", f"{cp}.decoder.up_modules.{j}", None if up else prev, None, None, f"cond.c{j}", v, True))
        prev = v
    ns = len(s.rate_factors)
    nbs = ns + int(s.extra_conv_block)
    prev = "score.in"
    for i in range(nbs):
        out.append((f"score.enc{i}", f"{sp}.encoder.ds_modules.{i}", prev, i, None, None, None, False))
        prev = f"score.enc{i}.h" if i < ns else f"score.enc{i}.v"
    prev = "score.gru"
    for j in range(nbs):
        up = not (s.extra_conv_block and j == 0)
        out.append((f"score.dec{j}", f"{sp}.decoder.up_modules.{j}", None if up else prev, nbs + j, f"cond.sc{j}", None, None, False))
        prev = f"score.dec{j}.v"
    return [(p, q, i, f, a, c1 or p + ".c1", v or p + ".v", ex) for p, q, i, f, a, c1, v, ex in out]


class ConvParams:
    """The body convs of one model and the FiLM row offsets of the score network's blocks."""

    def __init__(self, spec, sd):
        self.spec = spec
        self.walk = blocks_of(spec)
        self.blocks = {p: BlockP(sd, q) for p, q, *_ in self.walk}
        self.film_off, off = {}, 0
        for p, q, i, f, *_ in self.walk:
            if f is not None:
                self.film_off[p] = off
                off += 2 * self.blocks[p].C
        self.film_rows = off

    def check_against_blob(self, blob, plan):
        """The rebuilt weights are the library's: w (kernel layout at w_off and taps-innermost at wd_off), bias (b_off), slope
        (a_off) and the transformed weights U (wu_off) of every body conv, bit for bit; the FiLM row count."""
        convs = {c["name"]: c for c in plan["convs"]}
        assert self.film_rows == plan["film_rows"], (self.film_rows, plan["film_rows"])
        for bp in self.blocks.values():
            for cv in bp.c:
                L = convs[cv.name]
                Cout, Cin, KW = cv.w.shape
                Mp, CK, KWP = L["Mp"], L["CK"], L["KWP"]
                assert (L["Cin"], L["Cout"], L["KW"]) == (Cin, Cout, KW), cv.name
                assert torch.equal(blob[L["b_off"]: L["b_off"] + Cout], cv.b), cv.name
                assert torch.equal(blob[L["a_off"]], cv.alpha), cv.name
                # row = (chunk KW + tap) CK + l of channel ci = chunk CK + l, columns m < Mp (store_conv)
                wk = blob[L["w_off"]: L["w_off"] + Cin * KW * Mp].view(Cin // CK, KW, CK, Mp)[..., :Cout]
                assert torch.equal(wk.permute(3, 0, 2, 1).reshape(Cout, Cin, KW), cv.w), cv.name
                if KWP:
                    wd = blob[L["wd_off"]: L["wd_off"] + Cin * Mp * KWP].view(Cin, Mp, KWP)
                    assert torch.equal(wd[:, :Cout, :KW].permute(1, 0, 2), cv.w), cv.name
                    bad = first_wrong_u(blob, L, cv)
                    assert bad is None, (cv.name, "transformed weight differs from fl(G w) at blob offset", bad)


def first_wrong_u(blob, L, cv):
    """Blob offset of the first transformed weight that is not fl(G w), or None."""
    Cout, Cin, KW = cv.w.shape
    wu = blob[L["wu_off"]: L["wu_off"] + Cin * L["Mp"] * L["KWP"]].view(Cin, L["Mp"], L["KWP"])[:, :Cout, :KW + 1]
    ne = (wu != cv.U.permute(1, 0, 2)).reshape(-1)
    if not bool(ne.any()):
        return None
    ci, m, x = (int(v) for v in torch.unravel_index(ne.int().argmax(), (Cin, Cout, KW + 1)))
    return L["wu_off"] + (ci * L["Mp"] + m) * L["KWP"] + x


# ---- one conv ---------------------------------------------------------------------------------------------------------------
class Epi:
    """Epilogue operands of one body conv (CPU tensors) and what the reader does with the input."""

    def __init__(self, act=True, add=None, film=None, res=None, out_alpha=None):
        self.act, self.add, self.film, self.res, self.out_alpha = act, add, film, res, out_alpha


def _pairs(a, KW):
    """(B, C, T) -> (B, C, P, KW + 1): window d of output pair p, zeros outside the row."""
    T = a.shape[-1]
    pad = (KW - 1) // 2
    return Fn.pad(a, (pad, pad + 1 + T % 2)).unfold(-1, KW + 1, 2)


def _conv(a, w, dtype):
    return Fn.conv1d(a.to(dtype), w.to(dtype), padding=(w.shape[-1] - 1) // 2)


def wino_abs(a, cv):
    """The two absolute sums of the minimal-filtering bound without the bias, (B, Cout, T) float64 each:
    A_uv = sum_x |AT| sum_ci |U_x| |V_x| (what the accumulation's roundings are relative to) and
    A_bt = sum_x |AT| sum_ci |U_x| (sum_i |BT[x, i]| |d_i|) (what the roundings of d and of V = BT d are relative to)."""
    KW = cv.KW
    T = a.shape[-1]
    d = _pairs(a.double(), KW)
    out = []
    for v in ((d @ BT[KW].T).abs(), d.abs() @ BT[KW].abs().T):           # (B, Cin, P, KW + 1)
        Aj = torch.einsum("ocx,bcpx->bopx", cv.U.double().abs(), v) @ AT[KW].abs().T
        out.append(Aj.reshape(Aj.shape[0], Aj.shape[1], -1)[..., :T])
    return out


def wino_fp32(a, cv, U=None, hook=None):
    """fp32 emulation of the minimal-filtering arithmetic: V = BT d, per-x sums over the channels, A^T -- all in fp32.
    `hook(d)` may damage the (B, Cin, P, KW + 1) windows of the output pairs (CPU tests)."""
    KW = cv.KW
    T = a.shape[-1]
    d = _pairs(a.float(), KW)
    if hook is not None:
        d = hook(d.clone())
    V = d @ BT[KW].float().T
    M = torch.einsum("ocx,bcpx->bopx", (cv.U if U is None else U).float(), V)
    y = M @ AT[KW].float().T
    return y.reshape(y.shape[0], y.shape[1], -1)[..., :T]


def bf16_pieces(v):
    """split3 of ou_split_pack.h on a tensor: three fp32 tensors holding bf16 values, hi + mid + lo = v."""
    v = v.float()
    hi = v.bfloat16().float()
    r1 = v - hi
    mid = r1.bfloat16().float()
    lo = (r1 - mid).bfloat16().float()
    return hi, mid, lo


SPLIT_KEPT = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))  # (activation piece, weight piece): total order <= 2


def split_fp32(a, cv, kept=SPLIT_KEPT, x_pieces=3):
    """fp32 emulation of conv_split_kernel's arithmetic in the kernel's own summation order (ou_conv_split.hip, "Summation order
    per output"): channel chunks of 16 ascending, taps ascending, the kept piece products hi.hi first; one 16-deep instruction
    adds its 16 exact products to the fp32 accumulator with ONE rounding (emulated in double: the products are exact, their sum
    of 16 is exact in double to 2^-53).  A serial chain of Cin / 16 x KW x 6 rounded accumulations -- torch's blocked fp32 conv
    over the same products errs 6.6 times less on a 768-channel k5 layer and is NOT this algorithm.
    `x_pieces` < 3 drops the smallest activation piece(s) (CPU tests)."""
    ap, wp = bf16_pieces(a), bf16_pieces(cv.w)
    KW, T = cv.KW, a.shape[-1]
    pad = (KW - 1) // 2
    app = [Fn.pad(p, (pad, pad)).double() for p in ap]
    wpd = [p.double() for p in wp]
    acc = torch.zeros(a.shape[0], cv.w.shape[0], T)
    for cc in range(0, a.shape[1], 16):
        for k in range(KW):
            for i, j in kept:
                if i < x_pieces:
                    part = torch.einsum("bct,oc->bot", app[i][:, cc:cc + 16, k:k + T], wpd[j][:, cc:cc + 16, k])
                    acc = (acc.double() + part).float()
    return acc


def _epilogue(v, e, ep, dtype):
    """The kernels' epilogue in `dtype`; `e` (float64 bound so far, or None) is propagated as the module docstring says."""
    s2 = torch.tensor(INV_SQRT2, dtype=dtype)

    def scaled_add(v, e, o):
        s = v + o.to(dtype)
        r = s * s2
        if e is not None:
            e = (e + U * s.double().abs()) * INV_SQRT2 + U * r.double().abs()
        return r, e
    if ep.add is not None:
        v, e = scaled_add(v, e, ep.add)
    if ep.film is not None:
        ga, be = (t.to(dtype) for t in ep.film)
        gv = ga * v
        r = gv + be
        if e is not None:
            e = ga.double().abs() * e + U * gv.double().abs() + U * r.double().abs()
        v = r
    if ep.res is not None:
        v, e = scaled_add(v, e, ep.res)
    if ep.out_alpha is not None:
        v = prelu(v, ep.out_alpha.to(dtype))
        if e is not None:
            e = max(1.0, abs(float(ep.out_alpha))) * e + U * v.double().abs()
    return v, e


def body_conv(x, cv, ep, kind="chain", lens=None, e_in=None):
    """-> (ref, bound, extra): one body conv from the tap `x` the kernel read.  kind: chain / wino / split.  `e_in`: bound of x
    itself (fused bodies: the previous stage's), propagated through |w|.  Behind a row's end (lens) ref and bound are 0: Report
    holds those elements against exactly 0.  extra: {'e32': ..} for the split kind."""
    a = prelu(x.double(), cv.alpha.double()) if ep.act else x.double()
    p = 1 if ep.act else 0
    Cout, Cin, KW = cv.w.shape
    bias = cv.b.double()[None, :, None]
    v = _conv(a, cv.w, torch.float64) + bias
    extra = {}
    if kind == "wino":
        A_uv, A_bt = wino_abs(a, cv)
        A = A_uv + bias.abs()
        e = ((KW + 1) * Cin + 2) * U * A + (p + BT_ROUNDINGS[KW]) * U * A_bt
    else:
        A = _conv(a.abs(), cv.w.abs(), torch.float64) + bias.abs()
        e = (Cin * KW + 2 + p) * U * A
    if e_in is not None:
        e = e + _conv(e_in.double() * (max(1.0, abs(float(cv.alpha))) if ep.act else 1.0), cv.w.abs(), torch.float64)
    ref, e = _epilogue(v, e, ep, torch.float64)
    if kind == "split":
        a32 = prelu(x.float(), cv.alpha) if ep.act else x.float()
        r32, _ = _epilogue(split_fp32(a32, cv) + cv.b[None, :, None], None, ep, torch.float32)
        valid = valid_mask(lens, ref.shape[0], ref.shape[-1]).expand_as(ref)
        e32 = float((r32.double() - ref).abs()[valid].max())
        extra["e32"], extra["r32"] = e32, r32
        _, dropped = _epilogue(v, 0.5 * U * A, ep, torch.float64)   # the derived part, carried through the epilogue's scalings
        e = torch.full_like(ref, M_SPLIT * e32) + dropped
    if lens is not None:
        m = valid_mask(lens, ref.shape[0], ref.shape[-1])
        ref, e = ref * m, e * m
    return ref, e, extra


def split_report(name, gpu, ref, bound, extra, lens=None):
    """Report of a split-kind conv at its bound (M_SPLIT e32 + the derived part), with `e32` and `lib_ratio` as
    small_fp64.lib_report defines them (the figure M_SPLIT is taken from)."""
    rep = Report(name, gpu, ref, bound, lens)
    rep.e32 = extra["e32"]
    rep.lib_ratio = F.lib_report(name, gpu, ref, extra["r32"], 1, lens).lib_ratio
    return rep


def fused_body(x, bp, depth, ep1, res, lens=None):
    """conv_chainw_kernel: depth 3: conv1 (ep1: cond add, FiLM) -> conv2 -> conv3 from the block input x = hu; depth 2: conv2 ->
    conv3 from x = the .c1 tap.  -> (ref_v, bound_v, ref_c1, bound_c1) (c1: depth 3 only, the raw conv1 result)."""
    m = valid_mask(lens, x.shape[0], x.shape[-1]) if lens is not None else 1.0
    h, e, c1, e1 = x, None, None, None
    if depth == 3:
        h, e, _ = body_conv(x, bp.c[0], ep1, "wino", lens)
        c1, e1 = h, e
    h, e, _ = body_conv(h, bp.c[1], Epi(), "wino", lens, e_in=e)
    # (the kernel rounds the stage-2 result to fp32 before conv3 reads it, the float64 reference does not: one more u |h|)
    h3, e3, _ = body_conv(h, bp.c[2], Epi(res=res), "wino", lens, e_in=e + U * h.abs())
    return h3 * m, e3 * m, c1, e1


# ---- coarse check of today's suite ------------------------------------------------------------------------------------------
def snr_db(ref, got):
    """SNR over the whole tensor, what the parity tests assert >= 100 dB of."""
    n = float((ref.double() - got.double()).pow(2).sum())
    return float("inf") if n == 0 else 10.0 * math.log10(float(ref.double().pow(2).sum()) / n)


# ---- cases and coverage -------------------------------------------------------------------------------------------------------
MODELS = ("PP16", "PP24")
RAGGED_ROWS = (13, 4, 1)  # frames per row of the ragged batch (samples: frames * tot_ds - 3)
# column tiles of each family's launcher (conv_mfma configs 64 / 128; launch_conv_direct 32 tn; direct2w, direct3(w), direct4w
# 64-column tiles; conv_split BN 64 / 128; conv_chainw 126 / 252 finished columns)
FAMILY_TILES = {"lds": (64, 128), "direct": (32, 64), "direct2": (32, 64), "direct2w": (64,), "direct3": (64,), "direct3w": (64,),
                "direct4w": (64,), "split": (64, 128), "fused": (126, 252)}


def edge_classes(n, tile, halo, B):
    """small_fp64.classes_of (a .. e) + the pair-wise classes: 'odd' / 'even' row length, 'lt_halo' a row shorter than the halo."""
    hit = F.classes_of(n, tile, halo, B)
    hit.discard("e3")
    if B == 4:
        hit.add("e4")
    hit.add("odd" if n % 2 else "even")
    if n <= halo:
        hit.add("lt_halo")
    return hit


def reachable_within(m, tile, halo, frames, batches):
    """Every class whole batches of `batches` rows of f * m columns meet for f in `frames` (a class that only longer inputs
    reach is left out: a test case stays a few seconds)."""
    out = set()
    for f in frames:
        for B in batches:
            out |= edge_classes(f * m, tile, halo, B)
    return out


MAX_FRAMES = 65
# tag -> (options that bring the family onto the body convs at these small shapes, the families under test, batch sizes the
# family runs at, fewest frames at which it takes a layer).  Which (channels, kernel size) each family under test has to take in
# each case: tests/golden/conv_fp64_widths.json.
FAMILIES = {
    "lds": (dict(conv_direct=0, fuse=0), ("lds",), (1, 4), 1),
    "direct": (dict(conv_direct=1, fuse=0), ("direct",), (1, 4), 1),
    "direct2": (dict(conv_direct=4, fuse=0), ("direct2",), (1, 4), 1),
    "direct2.preact0": (dict(conv_direct=4, fuse=0, preact=0), ("direct2",), (4,), 13),
    # the default rule at batch 1: conv_direct4w 6xx on the short deep levels, conv_direct2w 4xx from rows of ~500 columns on
    "default": (dict(fuse=0), ("direct4w", "direct2w"), (1,), 1),
    "default.preact0": (dict(fuse=0, preact=0), ("direct4w", "direct2w"), (4,), 13),
    "direct3": (dict(tile_min=0.01, wino=0, fuse=0), ("direct3",), (4,), 13),
    "direct3w": (dict(tile_min=0.01, fuse=0), ("direct3w",), (4,), 13),
    "direct3w.preact0": (dict(tile_min=0.01, fuse=0, preact=0), ("direct3w",), (4,), 13),
    "split": (dict(split=1, fuse=0), ("split",), (1, 4), 1),
    "split.preact0": (dict(split=1, fuse=0, preact=0), ("split",), (4,), 13),
    "fuse3": (dict(fuse=3), ("fused",), (1, 4), 13),
    "fuse2": (dict(fuse=2), ("fused",), (1, 4), 13),
}
# (frames, batch): 1 frame: PP16's level lengths 1, 5, 20, 80, 160 (shorter than every tile, the deepest shorter than the halo);
# 3: odd deepest level; 13: 65 = 64 + 1 and 260 = 2 x 128 + 4; 26: 130 = 128 + 2; 32: 640 = 5 x 128; 64 / 65: the latent level
# on and one past a 64-column tile.  Every family runs all of them at the batch sizes it works at.
ALL_SHAPES = ((1, 1), (3, 4), (13, 1), (13, 4), (26, 1), (32, 1), (32, 4), (64, 1), (65, 4))
B4_SHAPES = ((13, 4), (26, 4), (32, 4), (64, 4), (65, 4))
_FUSE = ((13, 1), (13, 4), (32, 1), (52, 1), (63, 1))  # (52 / 63 frames: 80 f = 33 x 126 + 2 and 40 x 126, 160 f = 40 x 252)
_SHAPES = {"lds": ALL_SHAPES, "direct": ALL_SHAPES, "direct2": ALL_SHAPES, "split": ALL_SHAPES,
           "default": ((1, 1), (13, 1), (26, 1), (32, 1), (64, 1), (65, 1)), "direct3": B4_SHAPES, "direct3w": B4_SHAPES,
           "fuse3": _FUSE, "fuse2": _FUSE}
CASES = [(tag, m, B, f) for tag in FAMILIES for m in MODELS for f, B in _SHAPES.get(tag, ((13, 4),))
         if not (tag.startswith("fuse") and m != "PP16")]  # (conv_chainw_kernel: 32 / 64 channels -- PP24 has 48 / 96)
RAGGED = [(m, mf) for m in MODELS for mf in (0, 1)]


def case_id(tag, name, B, frames):
    return f"{tag}.{name}.b{B}.f{frames}"
