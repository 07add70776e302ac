"""Workspace poisoning: the helper, the calls and the case table of tests/test_gpu_ws_poison.py (tests/test_ws_poison_cpu.py
holds the table's coverage without a device).

ou_workspace_init clears the header of a workspace only (everything in front of `mel_scale`), and a buffer prepared for (B, T)
serves every shorter T: the body is never initialised, and every call finds in it what earlier calls left at other offsets.  A
call is right only if its result does not depend on that.  `poison(model, fill)` overwrites the body of every buffer a model
holds for its calls; a case runs one call once, then again after each fill, and every output has to come back bit for bit.

    zero     what a fresh allocation usually holds (and what hides a forgotten mask)
    nan      anything read and not discarded by a select shows
    finite   seeded uniform values in +-2^10: what a previous call realistically leaves, far above any rounding

The header (status words, coefficient rows, `stats`, `rows`, `lens`, both GRU exchange areas) is not touched: it continues
from call to call by design.

A case that may read stale words and cancel them arithmetically is listed in NAN_EXEMPT with the kernel, the line and the
operand; no case is exempt from `finite` or `zero`.
"""
import collections
import ctypes
import os
import re

import torch

import conv_fp64 as CF
import norm_cases
import offlist_cases
import seg_fp64 as SG
import seqmodel_cases
import snake_cases
from helpers import get_spec, synth_mix

FILLS = ("zero", "nan", "finite")
N_STEPS = 2
FRAMES = 13                 # the plain calls: 13 frames - 3 samples
RAGGED_ROWS = CF.RAGGED_ROWS  # frames per row (samples: frames * tot_ds - 3)
ENS = 3
ZOO = ("PP16s", "OR16s", "PP24s")
GAN = ("PP16s", "PP24s")    # models with the decoupling layer: warm start and the aux exit
# case id -> (fills the case runs, why): `nan` is the only fill a case may be spared, and only by name
NAN_EXEMPT = {}

Case = collections.namedtuple("Case", "id sect model call kw opts fns family kind")


# ---- the helper -----------------------------------------------------------------------------------------------------------------
_headers = {}  # (id(model), batch size) -> bytes in front of mel_scale


def header_bytes(model):
    """Byte offset of `mel_scale` in the workspace of the call that just returned (ou_tensor): what ou_workspace_init clears.
    The header's layout depends on the batch size alone: kept per (model, batch size)."""
    B = model._ws_key[0]
    key = (id(model), B)
    if key not in _headers:
        off, C, T = ctypes.c_size_t(), ctypes.c_int32(), ctypes.c_int32()
        rc = model._L.ou_tensor(model._handle, b"mel_scale", ctypes.byref(off), ctypes.byref(C), ctypes.byref(T))
        assert rc == 0 and off.value > 0 and off.value % 256 == 0, (rc, off.value)
        _headers[key] = off.value
    return _headers[key]


def _fill(buf, fill, seed):
    """Overwrite the uint8 tensor `buf` (a view whose start is 4-byte aligned)."""
    n = buf.numel() // 4
    words = buf[: 4 * n].view(torch.float32)
    if fill == "zero":
        buf.zero_()
    elif fill == "nan":
        buf.fill_(0xFF)  # every word 0xFFFFFFFF: a NaN as float, -1 as an integer
        words.fill_(float("nan"))
    elif fill == "finite":
        g = torch.Generator(device=buf.device).manual_seed(seed)
        words.copy_((torch.rand(n, generator=g, device=buf.device) * 2.0 - 1.0) * 1024.0)
    else:
        raise ValueError(fill)


def buffers(model):
    """[(uint8 tensor, header bytes)] of everything the model holds for its calls: the walk workspace in use (a captured
    graph's private one included, once adopted), the other cached walk workspaces, the segmented calls' workspace, the counter
    noise's scratch (no header).  A buffer held at a batch size whose header is not known yet is an error, not a buffer passed
    over: call header_bytes right after a call on that batch size."""
    header_bytes(model)
    out, seen = [], set()

    def add(ws, B, what):
        if ws is None or ws.data_ptr() in seen:
            return
        hdr = _headers.get((id(model), B))
        assert hdr is not None, f"{what}: a buffer for batch size {B} is held, the header of that batch size is not known"
        assert 0 < hdr < ws.numel(), (what, hdr, ws.numel())
        seen.add(ws.data_ptr())
        out.append((ws, hdr))
    add(model._ws, model._ws_key[0], "walk workspace")
    for B, ws in model._ws_cache.items():
        add(ws, B, "cached walk workspace")
    seg = getattr(model, "_seg_ws", None)
    if seg is not None:
        add(seg[1], seg[0], "segment workspace")
    scratch = model.__dict__.get("_noise_scratch")
    if scratch is not None:
        out.append((scratch, 0))
    return out


def poison(model, fill, seed=20260):
    """Overwrite the body (header excluded) of every buffer of `buffers(model)`.  -> a copy of the walk workspace in use as it
    stands after the fill (what an element the next call does not write still holds afterwards)."""
    torch.cuda.synchronize(model.device)
    for i, (ws, hdr) in enumerate(buffers(model)):
        _fill(ws[hdr:], fill, seed + i)
    torch.cuda.synchronize(model.device)
    return model._ws.clone()


# ---- models ---------------------------------------------------------------------------------------------------------------------
_models = {}


def spec_of(model):
    kind, name = model
    if kind == "zoo":
        return get_spec(name)
    if kind == "norm":
        return norm_cases.spec_of(*name)
    if kind == "snake":
        return snake_cases.spec_of(name)
    if kind == "seq":
        return seqmodel_cases.spec_of(name)
    if kind == "off":
        return offlist_cases.spec_of(name)
    raise KeyError(kind)


def get(model):
    """-> (model object, spec): the zoo's models are test_gpu_parity's (one object per process), the others are built here."""
    kind, name = model
    if kind == "zoo":
        from test_gpu_parity import get_model

        m, spec, _ = get_model(name)
        return m, spec
    if model not in _models:
        from open_universe_amd import Universe, UniverseGAN

        spec = spec_of(model)
        sd = {"norm": lambda: norm_cases.state_dict_of(*name), "snake": lambda: snake_cases.state_dict_of(name),
              "seq": lambda: seqmodel_cases.state_dict_of(name), "off": lambda: offlist_cases.state_dict_of(name)}[kind]()
        cls = UniverseGAN if spec.kind == "universe_gan" else Universe
        _models[model] = (cls(spec, state_dict=sd, device="cuda:0"), spec)
    return _models[model]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def row_sets(td):
    """name -> raw lengths of a ragged batch.  `rows`: the project's RAGGED_ROWS; `other`: other lengths under the same
    longest row; `mult`: one row whose length is a multiple of tot_ds (it pads by a whole block)."""
    return {"rows": [f * td - 3 for f in RAGGED_ROWS], "other": [13 * td - 3, 2 * td - 1, 7 * td - 3, 5],
            "mult": [13 * td - 3, 4 * td, td - 3], "b4": [13 * td - 3, 4 * td - 3, td - 3, 9 * td - 3]}


def padded(n, td):
    return n + (td - n % td)


def mix_of(spec, lens, seed=600):
    """(B, 1, max) rows of their own lengths, zeros behind."""
    lm = max(lens)
    sigs = [synth_mix(spec, 1, n, seed=seed + i)[0] for i, n in enumerate(lens)]
    return torch.stack([torch.nn.functional.pad(s, (0, lm - n)) for s, n in zip(sigs, lens)])[:, None, :].contiguous()


def noise_of(n, lens, td, E=1, seed=970):
    """(n, E * B, 1, T) member-major: N(0, 1) over every row's own padded length, zeros behind."""
    B, T = len(lens), padded(max(lens), td)
    nz = torch.zeros(n, E * B, 1, T)
    for q in range(E * B):
        Tq = padded(lens[q % B], td)
        nz[:, q, 0, :Tq] = torch.randn(n, Tq, generator=torch.Generator().manual_seed(seed + q))
    return nz


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ---- the calls ------------------------------------------------------------------------------------------------------------------
# run_*(model, spec, state, **kw) -> {"out": .., "members": .. (where the call has them), "frames": padded frames of every walk
# row the taps hold (ragged walks only), "cond_rows": rows of the conditioner's pass where they are not the walk's, "aux": the
# call ends at the conditioner's estimate (no score pass)}.  `state` lives as long as the
# case: what has to survive between the runs (a captured graph).
def run_plain(model, spec, state, B, frames=FRAMES, keep_rms=False, warm_start=None, use_aux=False, counter=False):
    td = spec.tot_ds
    lens = [frames * td - 3] * B
    mix = mix_of(spec, lens).cuda()
    if counter:
        from open_universe_amd.noise import CounterNoise

        return {"out": model.enhance(mix, n_steps=N_STEPS, rng=CounterNoise(77, stream=3), keep_rms=keep_rms)}
    n = 0 if use_aux else N_STEPS - (warm_start or 0)
    nz = noise_of(n, lens, td).cuda() if n else None
    return {"out": model._enhance(mix, N_STEPS, None, None, None, None, use_aux, keep_rms, None, "median", warm_start, nz),
            "aux": bool(use_aux)}


def run_var(model, spec, state, rows="rows", keep_rms=False, counter=False):
    td = spec.tot_ds
    lens = row_sets(td)[rows]
    mix = mix_of(spec, lens).cuda()
    kw = {"counter": (77, [(5 << 16) | b for b in range(len(lens))])} if counter else {}
    nz = None if counter else noise_of(N_STEPS, lens, td).cuda()
    out = model._enhance(mix, N_STEPS, None, None, None, None, False, keep_rms, None, "median", None, nz, t_raw=list(lens), **kw)
    return {"out": out, "frames": [padded(n, td) // td for n in lens], "cond_rows": len(lens)}


def run_ens(model, spec, state, B, stat="median", rows=None, keep_rms=False):
    td = spec.tot_ds
    lens = [FRAMES * td - 3] * B if rows is None else row_sets(td)[rows]
    B = len(lens)
    mix = mix_of(spec, lens).cuda()
    nz = noise_of(N_STEPS, lens, td, ENS).cuda()
    n_steps, eps = model._begin(N_STEPS, None)
    out, mem = model._ensemble_call(mix, ENS, stat, n_steps, eps, keep_rms, None, nz, None if rows is None else list(lens), None,
                                    True)
    share = int(model.get_option("ens_share")) != 0
    res = {"out": out, "members": mem, "cond_rows": B if share else ENS * B}
    if rows is not None:
        res["frames"] = [padded(n, td) // td for n in lens] * ENS
    return res


def seg_geometry(td, which):
    """The geometry of tests/seg_fp64.py / test_gpu_seg_fp64.py: -> (row lengths, max_batch)."""
    return {"one_window": ([FRAMES * td - 3] * 2, 32),            # T_pad = 13 tot_ds < S: the `enhance` result
            "carry": ([SG.CARRY_LENGTH(td)] * 2, 4),              # test_several_groups_with_a_carry
            # test_ragged_call: a FULL row and two SHORT ones, 16 tot_ds - 1 and 57 samples.  The SHORT group is the last one, so
            # the taps hold a ragged walk (one short row alone would fill its group with copies of itself: no tail to look at),
            # and its longest row is a whole window: every group of the call then walks one (batch, length), so what an earlier
            # group wrote lies under the same names and a tap no group writes still holds the fill afterwards
            "var": ([41 * td + 7, 16 * td - 1, 57], 32),
            "ens": ([41 * td + 7] * 2, 32),                       # test_ensemble_members
            "var_ens": ([41 * td + 7, 57, 16 * td - 1], 32)}[which]  # ... its ragged form, the last group as above


def seg_last_group(model, td, which):
    """What the taps hold after a segmented call (seg_fp64.last_group): -> (padded frames of every walk row of the last group,
    member-major, or None when its rows are alike; rows of its conditioner pass)."""
    Sg, Ov = SG.seg_so(td)
    lens, mb = seg_geometry(td, which)
    E = ENS if which in ("ens", "var_ens") else 1
    geos = [SG.Row(n, td, Sg, Ov) for n in lens]
    Bw, real, slots, n_groups, T = SG.last_group(geos, mb, which in ("var", "var_ens"), E)
    frames = [geos[c].L // td for c, _ in slots] * E
    assert max(frames) == T // td
    share = E > 1 and int(model.get_option("ens_share")) != 0
    return (frames if min(frames) < max(frames) else None), (Bw if share else E * Bw)


def run_seg(model, spec, state, which, keep_rms=False, warm_start=None, use_aux=False, counter=False):
    td = spec.tot_ds
    Sg, Ov = SG.seg_so(td)
    lens, mb = seg_geometry(td, which)
    rows = [r.cuda() for r in SG.case_mix(spec, lens)]
    kw = dict(segment_s=Sg / spec.fs, overlap_s=Ov / spec.fs, max_batch=mb, n_steps=N_STEPS, keep_rms=keep_rms)
    if counter:
        from open_universe_amd.noise import CounterNoise

        rng = CounterNoise(78, stream=1)
    else:
        rng = _gen(50)
    frames, cond_rows = seg_last_group(model, td, which)
    res = {"cond_rows": cond_rows, "aux": bool(use_aux)}
    if frames is not None:
        res["frames"] = frames
    if which == "var":
        outs = model.enhance_long_many(rows, rngs=rng, warm_start=warm_start, use_aux_signal=use_aux, **kw)
        res["out"] = torch.cat(outs)
    elif which == "var_ens":
        outs, mems = model.enhance_long_many_ensemble(rows, ENS, "median", rngs=rng, return_members=True, **kw)
        res.update(out=torch.cat(outs), members=torch.cat([m.reshape(-1) for m in mems]))
    elif which == "ens":
        res["out"], res["members"] = model.enhance_long_ensemble(torch.stack(rows), ENS, "median", rng=rng, return_members=True, **kw)
    else:
        res["out"] = model.enhance_long(torch.stack(rows), rng=rng, warm_start=warm_start, use_aux_signal=use_aux, **kw)
    return res


def run_graph(model, spec, state, B):
    """graphed_enhance(serial=True): captured once per case; a replay adopts the graph's private workspace, which is then the
    walk workspace `poison` reaches."""
    n = FRAMES * spec.tot_ds - 3
    if "run" not in state:
        state["run"] = model.graphed_enhance(B, n, n_steps=N_STEPS, serial=True)
    mix = mix_of(spec, [n] * B).cuda()
    return {"out": state["run"](mix, rng=_gen(11))}


def run_seam(model, spec, state, B, frames=FRAMES):
    """condition_model + score_model (the operator seams) as one call."""
    T = frames * spec.tot_ds
    x = mix_of(spec, [T] * B, seed=610).cuda() * 10.0
    model.condition_model(x)
    sig = torch.tensor([0.3, 1.7, 0.05, 4.0])[:B]
    xs = (torch.randn(B, 1, T, generator=torch.Generator().manual_seed(7)) * sig[:, None, None]).cuda()
    return {"out": model.score_model(xs, sig)}


RUNNERS = {"plain": run_plain, "var": run_var, "ens": run_ens, "seg": run_seg, "graph": run_graph, "seam": run_seam}


# ---- taps -----------------------------------------------------------------------------------------------------------------------
def tap_names(spec):
    """The names the fp64 tests enumerate: every block's .up / .c1 / .c2 / .v / .h (conv_fp64.blocks_of), the sandwich's
    blocks, cond.c{j}, cond.sc{j}, cond.in, score.in, mixn, x, wav.  -> (names, those every call has to have written)."""
    names, must = [], ["mixn", "x", "cond.in", "score.in"]
    for p, q, inp, f, add, c1n, vn, ex in CF.blocks_of(spec):
        names += [p + ".up", c1n, p + ".c2", vn, p + ".h"]
        must.append(vn)
    names += [f"score.cb{b}.{t}" for b in (1, 2) for t in ("c1", "c2", "v")]
    nb = len(spec.score.rate_factors) + int(spec.cond.extra_conv_block)
    for j in range(nb):
        names += [f"cond.c{j}", f"cond.sc{j}"]
        must += [f"cond.c{j}", f"cond.sc{j}"]
    names += must[:4] + ["wav"]
    return list(dict.fromkeys(names)), list(dict.fromkeys(must))


_PERSISTENT = re.compile(r"^cond\.(c\d+|sc\d+|aux|latent)$")


def read_taps(model, spec, cond_rows=None):
    """{name: (byte offset, rows, C, T)} of the named taps of the call that just returned (ou_tensor).  The conditioner's scratch
    taps have `cond_rows` rows where its pass ran fewer rows than the walk (a shared ensemble)."""
    rows_all = model._ws_key[0]
    out = {}
    for name in tap_names(spec)[0]:
        off, C, T = ctypes.c_size_t(), ctypes.c_int32(), ctypes.c_int32()
        if model._L.ou_tensor(model._handle, name.encode(), ctypes.byref(off), ctypes.byref(C), ctypes.byref(T)) != 0:
            continue
        rows = cond_rows if cond_rows and name.startswith("cond.") and not _PERSISTENT.match(name) else rows_all
        if off.value + 4 * rows * C.value * T.value <= model._ws.numel():
            out[name] = (off.value, rows, C.value, T.value)
    return out


def copy_taps(model, taps):
    return {name: model._ws[off: off + 4 * rows * C * T].clone() for name, (off, rows, C, T) in taps.items()}


def check_taps(model, spec, snapshot, base, fill, written, frames=None, cond_rows=None, aux=False):
    """The named taps of the last pass after a poisoned run against `base` = (read_taps, copy_taps) of the unpoisoned run.
    A tap the call did not write (an interior tap of a fused body, `wav` without a warm start) still holds the fill word for
    word: found under `nan` / `finite` (-> `written`, which the `zero` run, checked last, reads), and passed over.  One that was
    written has to hold the unpoisoned run's bits and, with `frames` (a ragged walk), exactly 0 from frames[b] * (T / longest)
    on.  -> {"compared": taps, "differ": [taps], "tail_elements": n, "tail_bad": {tap: non-zero elements}, "unwritten": [taps]}"""
    ws = model._ws
    taps = read_taps(model, spec, cond_rows)
    names, must = tap_names(spec)
    if aux:
        must = [n for n in must if n == "mixn" or n.startswith("cond.")]
    assert taps == base[0], "the two runs of one call laid their taps out differently"
    for name in must:
        assert name in taps, (name, "is no tap of this call")
    rep = {"compared": 0, "differ": [], "tail_elements": 0, "tail_bad": {}, "unwritten": []}
    fmax = max(frames) if frames is not None else None
    for name, (off, rows, C, T) in taps.items():
        got = ws[off: off + 4 * rows * C * T]
        if fill != "zero":
            if torch.equal(got, snapshot[off: off + 4 * rows * C * T]):
                assert name not in must, (name, "was not written by the call")
                rep["unwritten"].append(name)
                continue
            written.add(name)
        elif name not in written:
            continue
        rep["compared"] += 1
        if not torch.equal(got, base[1][name]):
            rep["differ"].append(name)
        if fmax is None:
            continue
        assert T % fmax == 0, (name, T, fmax)
        t = got.view(torch.float32).view(rows, C, T)
        per = T // fmax
        nbad = 0
        for b in range(rows):
            tail = t[b, :, frames[b] * per:]
            rep["tail_elements"] += tail.numel()
            nbad += int((tail != 0).sum())  # (a NaN is != 0)
        if nbad:
            rep["tail_bad"][name] = nbad
    return rep


# ---- the case table -------------------------------------------------------------------------------------------------------------
def _cases():
    out = []

    def add(id, sect, model, call, kw, fns, opts=None, family=None, kind=None):
        out.append(Case(id, sect, model, call, kw, opts or {}, tuple(fns), family, kind))

    # a. entry points
    for name in ZOO:
        m = ("zoo", name)
        for B in (1, 4):
            add(f"a.plain.{name}.b{B}", "a", m, "plain", dict(B=B), ["ou_enhance"])
            add(f"a.keep_rms.{name}.b{B}", "a", m, "plain", dict(B=B, keep_rms=True), ["ou_enhance"])
            add(f"a.counter.{name}.b{B}", "a", m, "plain", dict(B=B, counter=True), ["ou_enhance"])
            if name in GAN:
                add(f"a.warm.{name}.b{B}", "a", m, "plain", dict(B=B, warm_start=1), ["ou_enhance"])
                add(f"a.aux.{name}.b{B}", "a", m, "plain", dict(B=B, use_aux=True), ["ou_enhance"])
            add(f"a.graph.{name}.b{B}", "a", m, "graph", dict(B=B), ["ou_enhance"])
            for share in (0, 1):
                for stat in ("mean", "median", "signal_median"):
                    add(f"a.ens.{stat}.share{share}.{name}.b{B}", "a", m, "ens", dict(B=B, stat=stat), ["ou_enhance_ensemble"],
                        dict(ens_share=share))
        for rows in ("rows", "mult", "b4"):
            add(f"a.var.{rows}.{name}", "a", m, "var", dict(rows=rows), ["ou_enhance_var"])
            for share in (0, 1):
                add(f"a.ens_var.{rows}.share{share}.{name}", "a", m, "ens", dict(B=0, rows=rows), ["ou_enhance_ensemble"],
                    dict(ens_share=share))
        add(f"a.var.keep_rms.{name}", "a", m, "var", dict(rows="rows", keep_rms=True), ["ou_enhance_var"])
        add(f"a.var.counter.{name}", "a", m, "var", dict(rows="rows", counter=True), ["ou_enhance_var"])
        add(f"a.seg.one_window.{name}", "a", m, "seg", dict(which="one_window"), ["ou_enhance_segments"])
        add(f"a.seg.carry.{name}", "a", m, "seg", dict(which="carry", keep_rms=True), ["ou_enhance_segments"])
        add(f"a.seg.counter.{name}", "a", m, "seg", dict(which="carry", counter=True), ["ou_enhance_segments"])
        add(f"a.seg_var.{name}", "a", m, "seg", dict(which="var"), ["ou_enhance_segments_var"])
        add(f"a.seg_ens.{name}", "a", m, "seg", dict(which="ens"), ["ou_enhance_segments_ensemble"])
        add(f"a.seg_var_ens.{name}", "a", m, "seg", dict(which="var_ens"), ["ou_enhance_segments_var_ensemble"])
        if name in GAN:
            add(f"a.seg.warm.{name}", "a", m, "seg", dict(which="carry", warm_start=1), ["ou_enhance_segments"])
            add(f"a.seg_var.aux.{name}", "a", m, "seg", dict(which="var", use_aux=True), ["ou_enhance_segments_var"])
    # b. kernel families at full width
    for tag, (opts, want, batches, frames) in CF.FAMILIES.items():
        for name in CF.MODELS:
            if tag.startswith("fuse") and name != "PP16":
                continue
            m = ("zoo", name)
            for B in batches:
                add(f"b.plain.{tag}.{name}.b{B}", "b", m, "plain", dict(B=B, frames=frames), ["ou_enhance"], opts, tag)
            for mf in (0, 1):
                add(f"b.ragged.{tag}.mask_fused{mf}.{name}", "b", m, "var", dict(rows="rows"), ["ou_enhance_var"],
                    dict(opts, mask_fused=mf), tag)
    for name in CF.MODELS:
        m = ("zoo", name)
        for tag, opts, B in (("fir_alone", dict(fuse_upfir=0, rate_small=0), 1), ("gru_chunked", dict(gru_bmax=1), 4)):
            add(f"b.plain.{tag}.{name}.b{B}", "b", m, "plain", dict(B=B), ["ou_enhance"], opts, tag)
            for mf in (0, 1):
                add(f"b.ragged.{tag}.mask_fused{mf}.{name}", "b", m, "var", dict(rows="b4" if B == 4 else "rows"), ["ou_enhance_var"],
                    dict(opts, mask_fused=mf), tag)
    # c. the other model kinds
    kinds = [(("norm", ("PP16s", mode)), f"norm.{mode}") for mode in norm_cases.MODES]
    kinds += [(("snake", c), f"snake.{c}") for c in snake_cases.CASES]
    kinds += [(("seq", c), f"seq.{c}") for c in seqmodel_cases.CASES]
    kinds += [(("off", c), f"off.{c}") for c in ("r27", "odd_pp")]
    for m, kind in kinds:
        add(f"c.plain.{kind}", "c", m, "plain", dict(B=2, keep_rms=True), ["ou_enhance"], kind=kind)
        add(f"c.ragged.{kind}", "c", m, "var", dict(rows="rows", keep_rms=True), ["ou_enhance_var"], kind=kind)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
STEERING = ("fir_alone", "gru_chunked")               # (b): what conv_fp64.FAMILIES does not steer
KINDS = tuple(dict.fromkeys(c.kind for c in CASES if c.kind))
# f. call order through the header: PP16s, batch 4, every call at the same padded length
ORDER_CALLS = {
    "plain": ("plain", dict(B=4)),
    "ragged": ("var", dict(rows="b4")),
    "ragged_other": ("var", dict(rows="other")),
    "warm": ("plain", dict(B=4, warm_start=1)),
    "keep_rms": ("plain", dict(B=4, keep_rms=True)),
    "seam": ("seam", dict(B=4)),
}
ORDER_PAIRS = [(a, b) for a in ORDER_CALLS for b in ORDER_CALLS if a != b]
# e. inputs and outputs outside the rows
OUTSIDE = [(name, call) for name in ZOO for call in ("var", "ens_var")]


def declared_entry_points():
    """Every ou_enhance* function include/ouniverse.h declares."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ouniverse.h")
    with open(path) as f:
        return sorted(set(re.findall(r"^int (ou_enhance\w*)\(", f.read(), flags=re.M)))
