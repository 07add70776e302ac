"""
Host side of the drop-in `model` object returned by `inference_utils.load_model`.

Mirrors the inference surface of the reference's `Universe` / `UniverseGAN` LightningModule
(open_universe/networks/universe/universe.py:44-386, universe_gan.py:60-149): `.fs`, `.diff_kwargs`,
`.enhance(...)` (same signature + type hints: the reference CLI introspects them,
inference_utils/signature_to_parser.py:45), `.eval()`, `.to()`, `.condition_model(...)`,
`.score_model(...)`, `.aux_to_wav(...)`.

Everything numerical happens in libouniverse.so (HIP, gfx950) through the C ABI; this class only reshapes,
draws the noise with `torch.randn(generator=rng)` in the reference's order (so a shared generator advances
identically, bin/enhance.py:147-166) -- or, with `rng=noise.CounterNoise(..)`, hands the library a key and one stream id per row
and draws nothing (extension, noise.py) --, owns the device buffers (PyTorch = device memory + streams) and maps C
status codes to the reference's exception types.  No torch compute fallback exists: without the library or
without a GPU construction fails.
"""
import collections
import contextlib
import ctypes
import math
import weakref
from ctypes import byref, c_double, c_float, c_int32, c_size_t, c_void_p
from typing import Optional

import torch

from . import _lib
from .config import ModelSpec
from .noise import ENSEMBLE_SHIFT, CounterNoise, is_counter


def randn(x, sigma, rng=None):
    """universe.py:39-41 (kept for API parity; the product path passes raw normal draws to the C ABI)."""
    noise = torch.randn(x.shape, dtype=x.dtype, device=x.device, generator=rng)
    return noise * sigma[:, None, None]


def padded(n, tot_ds):
    """The length the network walks a signal of n samples at: the next multiple of tot_ds ABOVE n (`Universe.pad` gives a length
    that already is a multiple one whole block more)."""
    return n + (tot_ds - n % tot_ds)


def as_rows(s, who, prep, t="L"):
    """A (t,) or (C, t) signal as prepared (C, t) rows; `who`: the method named in the refusal."""
    if s.ndim not in (1, 2):
        raise ValueError(f"{who} takes ({t},) or (C, {t}) signals")
    return prep(s if s.ndim == 2 else s[None, :])


class Packed(collections.namedtuple("Packed", "dims chans lens batch")):
    """A list of (L,) / (C, L) signals as ONE batch (pack_rows): per entry its rank, channels (= rows) and length, and `batch`,
    the (sum C, longest L) tensor of all rows, right-padded with zeros."""
    __slots__ = ()

    @property
    def row_lens(self):
        """The length of every ROW of the batch (an entry's length, once per channel)."""
        return [n for c, n in zip(self.chans, self.lens) for _ in range(c)]

    def entries(self, rngs, own_length=True):
        """-> [(channels, length, generator)] for draw_noise; `rngs`: one generator per entry, or ONE for all (or None).
        own_length=False: every entry draws at the length of the longest (the rows of a plain batch)."""
        per_entry = isinstance(rngs, (list, tuple))
        return [(c, n if own_length else self.batch.shape[-1], rngs[i] if per_entry else rngs)
                for i, (c, n) in enumerate(zip(self.chans, self.lens))]


def pack_rows(signals, who, prep):
    """List of (L,) or (C, L) signals -> Packed; `prep`: what makes a signal float32, contiguous and on the right device."""
    rows = [as_rows(s, who, prep) for s in signals]
    lens = [int(r.shape[-1]) for r in rows]
    if min(lens) < 1:
        raise ValueError(f"{who}: empty input signal")
    batch = torch.cat([torch.nn.functional.pad(r, (0, max(lens) - n)) for r, n in zip(rows, lens)], dim=0)
    return Packed([s.ndim for s in signals], [int(r.shape[0]) for r in rows], lens, batch)


def unpack_rows(pk, out, members=None):
    """The inverse of pack_rows on a result: out (rows, L max) or (rows, 1, L max), members (E, rows, ..) likewise or None ->
    (list of per-entry outputs with the shape of their inputs, list of per-entry members (E,) + that shape -- empty without
    members).  Views, nothing is copied."""
    if out.ndim == 3:
        out, members = out[:, 0], (None if members is None else members[:, :, 0])
    res, mems, r0 = [], [], 0
    for nd, c, n in zip(pk.dims, pk.chans, pk.lens):
        o = out[r0:r0 + c, :n]
        res.append(o[0] if nd == 1 else o)
        if members is not None:
            m = members[:, r0:r0 + c, :n]
            mems.append(m[:, 0] if nd == 1 else m)
        r0 += c
    return res, mems


def draw_noise(tot_ds, entries, n, members=1, planes=None, device=None, discard=False):
    """Every `torch.randn` of the enhance methods.  `entries`: [(channels C_i, length L_i, generator g_i)], the inputs of one
    call; `n`: noise planes of the call (x0 first); `members`: E of an ensemble.  Performs, entry by entry and inside an entry
    plane by plane -- the order of the serial loop, so a generator shared by several entries ends where that loop leaves it --,
    the draws of the call on that entry ALONE: n times randn((E * C_i, 1, T_i), generator=g_i), T_i = padded(L_i).  (On the
    device the values of a draw depend on its shape: the shapes are part of the contract.)  Draw k of entry i lands member-major
    in plane k, columns [0, T_i) of the entry's rows: planes.view(n, E, rows, 1, T)[k, :, r_i : r_i + C_i, :, :T_i], rows = sum C_i,
    T = max T_i.  Where that block is contiguous -- one row, or ONE entry that is the whole plane: `enhance` at any batch size,
    `enhance_ensemble`, `draw_noise_like_enhance` -- the draw goes `out=` straight to its place, no temporary and no copy kernel;
    elsewhere it is drawn and copied.
    `planes`: None -- a new (n, E * rows, 1, T) float32 tensor on `device` is made, zeros where some T_i < T (what no draw covers
    stays 0), else uninitialised -- or any contiguous tensor of that many elements.  -> planes.
    discard=True: draw and drop (advance the generators, nothing is kept) -> None."""
    E = int(members)
    if len(entries) == 1 and not discard:  # the whole-plane case, nothing but the draws on its way (the host path of `enhance`)
        c, length, g = entries[0]
        rows, T = E * int(c), padded(int(length), tot_ds)
        slots = None
        if planes is None:
            planes = slots = torch.empty((n, rows, 1, T), dtype=torch.float32, device=device)
        elif planes.shape[-1] == T and planes.numel() == n * rows * T:
            slots = planes.view(n, rows, 1, T)
        if slots is not None:
            for k in range(n):
                torch.randn((rows, 1, T), generator=g, out=slots[k])
            return planes
    chans = [int(c) for c, _, _ in entries]
    Ts = [padded(int(length), tot_ds) for _, length, _ in entries]
    if discard:
        for (_, _, g), c, Ti in zip(entries, chans, Ts):
            for _ in range(n):
                torch.randn((E * c, 1, Ti), dtype=torch.float32, device=device, generator=g)
        return None
    if planes is None:
        make = torch.zeros if min(Ts) < max(Ts) else torch.empty
        planes = make((n, E * sum(chans), 1, max(Ts)), dtype=torch.float32, device=device)
    slots = planes.view(n, E, sum(chans), 1, planes.shape[-1])
    r0 = 0
    for (_, _, g), c, Ti in zip(entries, chans, Ts):
        for k in range(n):
            dst = slots[k, :, r0:r0 + c, :, :Ti]
            if dst.is_contiguous():
                torch.randn((E * c, 1, Ti), generator=g, out=dst.view(E * c, 1, Ti))
            else:
                dst.copy_(torch.randn((E * c, 1, Ti), dtype=torch.float32, device=planes.device, generator=g).view(E, c, 1, Ti))
        r0 += c
    return planes


_KEEP = object()  # (_forward: leave Universe._cond_key as it is)


class Universe:
    """MI355X-native stand-in for the reference's `Universe` / `UniverseGAN` inference object."""

    # Steering (tests / tuning only; the library reads no environment variable): options every NEW model object starts
    # with, and the live objects -- `set_default_options` reaches both, the way an environment variable used to.
    default_options = {}
    _live = weakref.WeakSet()
    # tools/ only (each sets it explicitly): before every call, OU_<OPTION>=value environment variables are translated into
    # ou_set_option calls -- the sweep scripts of earlier rounds steer that way.  The library itself reads no environment.
    steer_from_env = False

    def __init__(self, spec: ModelSpec, state_dict=None, device=None, packed_weights=None, fir_fold=0, split_copy=True):
        """`split_copy=False`: pack / expect a blob without the bf16-split weight copy (a quarter smaller: 486 instead of 648 MB
        for UNIVERSE++ 16 kHz) -- for models that never see a batch of 8 or more utterances per call."""
        if device is None:
            device = "cuda"
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(
                f"open_universe_amd runs on MI355X (HIP) only; device={device} requested. "
                "There is no CPU path -- use the reference implementation for CPU inference."
            )
        if not torch.cuda.is_available():
            raise RuntimeError("open_universe_amd: no HIP device visible (torch.cuda.is_available() is False)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._L = _lib.load()  # raises LibraryNotBuilt when the extension is missing
        self.spec = spec
        self.fs = spec.fs
        self.diff_kwargs = spec.diff_kwargs
        self.normalization_norm = 2 if spec.norm == "2" else spec.norm
        self.normalization_kwargs = {"ref": spec.norm_ref, "level_db": spec.level_db}
        if not spec.zero_mean:
            self.normalization_kwargs["zero_mean"] = False
        if spec.norm_eps != 1e-5:
            self.normalization_kwargs["eps"] = spec.norm_eps
        self.with_edm = spec.edm_noise is not None
        self.tot_ds = spec.tot_ds
        self.n_channels = spec.score.n_channels
        self.device = device
        # True: synchronise the stream and raise on a device-side timeout after every call (product default).
        # False: free-running -- the status word is still copied to pinned host memory after every call (async,
        # no host sync) and examined at the start of the next call, in synchronize() and in _status(force=True).
        self.check_status = True
        self._status_host = torch.zeros(64, dtype=torch.int32).pin_memory()
        self._status_np = self._status_host.numpy()  # (same pinned memory: read per call without building tensors)
        self._gru_recoveries_seen = {}   # workspace key -> recovery counter already acted upon
        self.gru_agent_scope = False     # True once the GRU publishes were switched to agent-scope stores for good
        self._status_event = None
        self._status_ws = None
        self.training = False
        self._fir_fold = int(fir_fold)
        self._split_copy = bool(split_copy)
        self._cfg = _lib.make_config(spec, self._fir_fold, self._split_copy)
        if packed_weights is None:
            if state_dict is None:
                raise ValueError("either state_dict or packed_weights is required")
            packed_weights, _ = _lib.pack_weights(spec, state_dict, self._fir_fold, self._split_copy)
        self._weights = packed_weights.to(device=device, dtype=torch.float32).contiguous()
        self._handle = c_void_p()
        with torch.cuda.device(device):
            _lib.check(self._L.ou_create(byref(self._cfg), c_void_p(self._weights.data_ptr()),
                                         c_size_t(self._weights.numel() * 4), device.index, byref(self._handle)))
        norm = _lib.norm_args(spec)
        if norm != (0, 1, 0.0):  # (every shipped config: the handle is never told, and is what it always was)
            _lib.check(self._L.ou_set_normalization(self._handle, *norm), self._handle)
        self._ws = None
        self._ws_key = None
        self._ws_cache = {}
        self._ws_need = {}
        self._cond_key = None
        self._sigma_cache = {}
        self._lanes = (1, 0)
        for k, v in type(self).default_options.items():
            self.set_option(k, v)
        Universe._live.add(self)
        self._env_seen = None
        self._sync_env()

    def _sync_env(self):
        if not Universe.steer_from_env:
            return
        import os

        snap = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("OU_")))
        if snap == self._env_seen:
            return
        self._env_seen = snap
        env = dict(snap)
        for key, dflt in _lib.option_defaults().items():
            v = env.get("OU_" + key.upper())
            if key in ("trace", "gru_ts", "ts", "no_overlap") and v is not None:
                v = "1" if v == "" or not v.lstrip("-").isdigit() else v  # (these used to be presence flags)
            self.set_option(key, dflt if v is None else float(v))
        _lib.check(self._L.ou_set_stamp_layer(self._handle, env.get("OU_CHAIN_TS", "").encode()), self._handle)

    # ---- steering through the C ABI (ou_set_option): tests force kernel families, tools sweep; never needed for normal use ----
    def set_option(self, key, value):
        """One typed option of this model's handle (keys: `_lib.option_names()`); takes effect from the next call on."""
        _lib.check(self._L.ou_set_option(self._handle, str(key).encode(), float(value)), self._handle)
        self._ws_need.clear()  # (options may change what a walk allocates)

    def get_option(self, key):
        v = c_double()
        _lib.check(self._L.ou_get_option(self._handle, str(key).encode(), byref(v)), self._handle)
        return v.value

    def options(self):
        return {k: self.get_option(k) for k in _lib.option_names()}

    def reset_options(self):
        _lib.check(self._L.ou_reset_options(self._handle), self._handle)
        self._ws_need.clear()

    @classmethod
    def set_default_options(cls, **kw):
        """Set options on every live model object AND on those created from now on (value None: back to the default)."""
        defaults = _lib.option_defaults()
        for k, v in kw.items():
            if v is None:
                Universe.default_options.pop(k, None)
            else:
                Universe.default_options[k] = v
            for m in list(Universe._live):
                m.set_option(k, defaults[k] if v is None else v)

    # ---- several enhance calls in flight in one process -----------------------------------------------------------
    def fork(self):
        """A second model object on the SAME packed weights (no copy) with a handle, workspace and status record of its
        own: what one lane of `LanePool` runs on.  A handle is not re-entrant; several handles side by side are fine."""
        twin = type(self)(self.spec, packed_weights=self._weights, device=self.device, fir_fold=self._fir_fold,
                          split_copy=self._split_copy)
        twin.check_status = self.check_status
        for k, v in self.options().items():  # a lane runs what its primary model would run
            twin.set_option(k, v)
        if self.gru_agent_scope:
            twin.gru_agent_scope = True
            _lib.check(twin._L.ou_set_gru_publish_mode(twin._handle, 1), twin._handle)
        return twin

    def set_lanes(self, lanes, lane, max_batch=0):
        """This object is lane `lane` of `lanes` models whose calls are in flight side by side on this device (one stream
        each): the library then sizes and places the GRU clusters of every lane so that all of them fit on the device
        together (include/ouniverse.h, ou_set_lanes).  `max_batch`: the largest batch size ANY lane of the pool will run
        when the calls differ in size (ou_set_lane_batch; 0 = every call's own size)."""
        _lib.check(self._L.ou_set_lanes(self._handle, int(lanes), int(lane)), self._handle)
        _lib.check(self._L.ou_set_lane_batch(self._handle, int(max_batch)), self._handle)
        self._lanes = (int(lanes), int(lane))

    def release_lanes(self):
        """Drop the forks (handles + workspaces) that `LanePool`s of this model created and kept for re-use."""
        for twin in self.__dict__.pop("_lane_forks", []):
            twin.reset_workspace()

    # ------------------------------------------------------------------------------------------------
    def __del__(self):
        try:
            if getattr(self, "_handle", None) is not None and self._handle.value:
                self._L.ou_destroy(self._handle)
                self._handle = c_void_p()
        except Exception:
            pass

    def eval(self, no_ema=False):
        """universe.py:864-865: inference always runs on the EMA weights (resolved at load time)."""
        return self

    def train(self, mode=True, no_ema=False):
        if mode:
            raise NotImplementedError("open_universe_amd implements the inference (enhance) path only")
        return self

    def to(self, *args, **kwargs):
        dev = kwargs.get("device", args[0] if args else None)
        if dev is not None and torch.device(dev).type != "cuda":
            raise RuntimeError("open_universe_amd models live on a HIP device; .to(cpu) is not supported")
        return self

    # ------------------------------------------------------------------------------------------------
    def _stream(self):
        return c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # workspaces kept alive, ONE per batch size (most recently used last): a buffer prepared by ou_workspace_init for
    # (B, T) serves every shorter length of the same batch size (include/ouniverse.h), so a directory of files of different
    # lengths runs on one buffer that grows to the longest file seen; a workspace costs an allocation plus the init
    WS_CACHE_ENTRIES = 4
    WS_CACHE_BYTES = 16 << 30

    def _workspace_bytes(self, B, T):
        n = self._ws_need.get((B, T))
        if n is None:
            c = c_size_t()
            _lib.check(self._L.ou_workspace_bytes(self._handle, B, T, byref(c)), self._handle)
            n = self._ws_need[(B, T)] = c.value
            if len(self._ws_need) > 4096:
                self._ws_need.clear()
        return n

    def _workspace(self, B, T, need=None):
        """`need`: bytes when the call wants more than the walk's own workspace for (B, T) (enhance_ensemble)."""
        key = (B, T)
        if self._ws_key == key and (need is None or self._ws.numel() >= need):
            return self._ws
        if need is None:
            need = self._workspace_bytes(B, T)
        cache = self._ws_cache
        ws = cache.get(B)
        if ws is None or ws.numel() < need:
            # free-running mode: the status copy of the previous call belongs to the workspace that is left now -- the next
            # call's copy would replace it unexamined
            if self._status_event is not None and not self.check_status:
                self._status_event.synchronize()
                self._raise_on_status()
            cache.pop(B, None)
            while cache and (len(cache) >= self.WS_CACHE_ENTRIES
                             or sum(w.numel() for w in cache.values()) + need > self.WS_CACHE_BYTES):
                cache.pop(next(iter(cache)))
            self._ws = ws = None
            try:
                ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            except torch.OutOfMemoryError:
                # give the idle workspaces (and the allocator's cached blocks) back and try once more
                cache.clear()
                torch.cuda.empty_cache()
                ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self._L.ou_workspace_init(self._handle, B, T, c_void_p(ws.data_ptr()),
                                                     c_size_t(need), self._stream()), self._handle)
        elif self._ws is not ws and self._status_event is not None and not self.check_status:
            self._status_event.synchronize()
            self._raise_on_status()
        cache.pop(B, None)
        cache[B] = ws  # most recently used last
        self._ws = ws
        self._ws_key = key
        self._cond_key = None
        return self._ws

    def _private_workspace(self, B, T):
        """A workspace of its own for a captured graph: never in the cache, so no eager call -- same batch size, longer
        signal -- can regrow or evict the buffer the graph's launches point into."""
        need = self._workspace_bytes(B, T)
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.ou_workspace_init(self._handle, B, T, c_void_p(ws.data_ptr()), c_size_t(need), self._stream()),
                       self._handle)
        return ws

    def _adopt_workspace(self, ws, B, T):
        """Make `ws` (prepared for at least (B, T)) the current workspace of this object."""
        if self._ws is ws and self._ws_key == (B, T):
            return
        if self._ws is not ws and self._status_event is not None and not self.check_status:
            # free-running mode: the pending status copy belongs to the workspace that is left now
            self._status_event.synchronize()
            self._raise_on_status()
        self._ws = ws
        self._ws_key = (B, T)
        self._cond_key = None

    def reset_workspace(self):
        """Drop every cached workspace: the next call allocates and initialises a fresh one (tests; after switching
        between kernel generations that lay the GRU exchange area out differently)."""
        if self._status_event is not None:
            # a status copy of an earlier call may still be pending: look at it while its workspace is still known
            self._status_event.synchronize()
            try:
                self._raise_on_status()
            finally:
                self._status_event = None
        self._ws_cache.clear()
        self._ws = None
        self._ws_key = None
        self._cond_key = None
        self._status_ws = None
        self.__dict__.pop("_noise_scratch", None)  # (the planes of the counter-based noise: re-made on demand)

    def _raise_on_status(self):
        self._status_event = None
        v = int(self._status_np[0])
        # word 20: waits the GRU clusters' safety net cut short by repeating a publish (0 on an idle device; a member that was
        # merely late -- starved by the kernels of other streams or lanes -- counts too); word 33: those among them where the
        # awaited granule was visible to a system-scope load / an atomic but not to the agent-scope load of the gather.  The
        # first time word 33 moves, the cheaper publish form has shown that it cannot be relied upon on this device / in this
        # process mix: switch to agent-scope (write-through) publishes for good -- +0.1 ms per GRU pass, no more recoveries.
        rec, lost = int(self._status_np[20]), int(self._status_np[33])
        if lost and not self.gru_agent_scope and not v:
            import warnings

            self.gru_agent_scope = True
            _lib.check(self._L.ou_set_gru_publish_mode(self._handle, 1), self._handle)
            warnings.warn(f"open_universe_amd: {lost} of {rec} repeated GRU hand-off(s) were publishes that an agent-scope load "
                          f"did not see (first event: {self._status_host[21:30].tolist()}); results are unaffected, the "
                          "recurrence kernels publish with agent-scope stores from now on", RuntimeWarning)
        if v:
            ws = self._status_ws if self._status_ws is not None else self._ws
            diag = ws[:256].view(torch.int32).cpu().tolist()  # who waited for what (see gru_ring_kernel)
            self._status_host.zero_()
            ws[:4].zero_()  # the device word is sticky until cleared
            ws[32 * 4:60 * 4].zero_()
            # [12..19]: reporting cluster / member / step / min tag seen / tag wanted / XCC / plain stores / block id;
            # [32] max tag seen, [36..]: (step << 8 | xcc now << 4 | xcc at the rendezvous) of every member of that cluster
            # that was itself stuck in a long wait (0xFFFFFFFF: slot not of this launch); [21..29]: first-recovery record
            members = [("-" if m == -1 else f"{(m & 0xFFFFFFFF) >> 8}@x{m & 0xFF:02x}") for m in diag[36:60]]
            if v & 16 and not v & ~16:
                # bit 16: the barrier of the fused deep-ConvBlock launch (conv_block3_kernel, OU_BLOCK3=1 only) ran out
                raise RuntimeError("device-side timeout in the fused ConvBlock launch's group barrier (status word 16, "
                                   "OU_BLOCK3=1); the output of that call is invalid and the workspace has to be "
                                   "re-initialised (Universe.reset_workspace())")
            raise RuntimeError(f"device-side timeout in the GRU cluster exchange (status word {v}, diagnostics "
                               f"{diag[8:20]}, max tag {diag[32] & 0xFFFFFFFF}, first recovery record {diag[21:30]}, "
                               f"members' waits {members}); the output of that call is invalid")

    def _poll_deferred_status(self):
        """Free-running mode: look at the status copy of an EARLIER call once its event has completed."""
        if self._status_event is not None and self._status_event.query():
            self._raise_on_status()

    def _status(self, force=False):
        """Called after every forward: enqueue the (async) copy of the device status word; in the default mode -- or
        with force=True -- wait for it and raise if a kernel flagged a timeout."""
        if self._ws is None:
            return
        st = torch.cuda.current_stream(self.device)
        if self._status_ws is not self._ws:
            self._status_ws = self._ws
            self._status_words = self._ws[:256].view(torch.int32)
        self._status_host.copy_(self._status_words, non_blocking=True)  # (on the current stream, behind the call's last kernel)
        ev = torch.cuda.Event()
        ev.record(st)
        self._status_event = ev
        if self.check_status or force:
            ev.synchronize()
            self._raise_on_status()

    def synchronize(self):
        """Wait for everything enqueued by this model and raise if any call since the last check timed out."""
        torch.cuda.current_stream(self.device).synchronize()
        if self._status_event is not None:
            self._raise_on_status()

    def gru_exchange_stats(self):
        """Health of the GRU clusters' L2 hand-offs on the current workspace: `recoveries` = publishes that had to be
        repeated by the safety net (each costs ~0.1 ms), `system_scope` = waves that finished their GRU pass with
        system-scope publishes after such a recovery (slower steps, no more recoveries).  Both 0 on a healthy device."""
        if self._ws is None:
            return {"recoveries": 0, "lost": 0, "system_scope": 0}
        d = self._ws[:256].view(torch.int32).cpu().tolist()
        # recoveries: waits cut short by the safety net (late members included); lost: publishes that really were invisible
        out = {"recoveries": int(d[20]), "lost": int(d[33]), "system_scope": int(d[31])}
        out["agent_scope_publishes"] = bool(self.gru_agent_scope)
        if d[21]:  # first recovery on this workspace: what three kinds of loads saw in the stale granule (gru_stale_probe)
            out["first_event"] = {"events": d[21], "cluster": (d[22] >> 16) & 0xFFFF, "member": (d[22] >> 8) & 0xFF,
                                  "wave": d[22] & 0xFF, "granule": d[23], "want": d[24], "sc1": d[25], "sc0sc1": d[26],
                                  "atomic": d[27], "sc1_after_inv": d[28], "step": (d[29] >> 16) & 0xFFFF,
                                  "xcc_at_rendezvous": (d[29] >> 8) & 0xFF, "xcc_now": d[29] & 0xFF}
        return out

    def tensor(self, name):
        """Debug: view of a named intermediate of the last call inside the workspace -> (B, C, T) tensor."""
        off, C, T = c_size_t(), c_int32(), c_int32()
        rc = self._L.ou_tensor(self._handle, name.encode(), byref(off), byref(C), byref(T))
        if rc != 0:
            raise KeyError(name)
        B = self._ws_key[0]
        n = B * C.value * T.value
        return self._ws[off.value: off.value + 4 * n].view(torch.float32).view(B, C.value, T.value)

    def launch_stats(self):
        a, b = c_int32(), c_int32()
        self._L.ou_launch_stats(self._handle, byref(a), byref(b))
        return a.value, b.value

    def profile(self, on):
        """Bracket every generic-conv launch of the following calls with HIP events (measurement only)."""
        _lib.check(self._L.ou_profile_enable(self._handle, int(bool(on))), self._handle)

    def profile_read(self, max_records=8192):
        """-> list of (ms, algorithmic_flops, algorithmic_bytes, tile_cfg) per conv launch since profile(True)."""
        ms = (c_float * max_records)()
        fl = (ctypes.c_double * max_records)()
        by = (ctypes.c_double * max_records)()
        cf = (c_int32 * max_records)()
        n = c_int32()
        _lib.check(self._L.ou_profile_read(self._handle, max_records, ms, fl, by, cf, byref(n)), self._handle)
        return [(ms[i], fl[i], by[i], cf[i]) for i in range(n.value)]

    def profile_read_ticks(self, max_records=32768):
        """-> list of (start, end, variant) per profiled launch: 10 ns ticks of the device's constant clock."""
        t0 = (ctypes.c_uint64 * max_records)()
        t1 = (ctypes.c_uint64 * max_records)()
        cf = (c_int32 * max_records)()
        n = c_int32()
        _lib.check(self._L.ou_profile_read_ticks(self._handle, max_records, t0, t1, cf, byref(n)), self._handle)
        return [(t0[i], t1[i], cf[i]) for i in range(n.value)]

    def bench_conv(self, layer, B, Tin, cfg=-1, sc=-1, with_res=False, iters=20):
        """Tuning aid: ms per launch of one packed conv layer (see ou_bench_conv)."""
        self._sync_env()
        ws = torch.empty(max(1 << 28, 64 * B * Tin * 4 * 64), dtype=torch.uint8, device=self.device)
        ms, used = c_float(), c_int32()
        _lib.check(self._L.ou_bench_conv(self._handle, layer.encode(), B, Tin, cfg, sc, int(with_res), iters,
                                         c_void_p(ws.data_ptr()), c_size_t(ws.numel()), self._stream(), byref(ms),
                                         byref(used)), self._handle)
        return ms.value, used.value

    def pad(self, x, pad=None):
        """universe.py:219-223."""
        if pad is None:
            pad = self.tot_ds - x.shape[-1] % self.tot_ds
        return torch.nn.functional.pad(x, (pad // 2, pad - pad // 2)), pad

    def unpad(self, x, pad):
        return x[..., pad // 2: -(pad - pad // 2)]

    def get_std_dev(self, time):
        """universe.py:380-386 (geometric schedule)."""
        s_min, s_max = self.diff_kwargs.sigma_min, self.diff_kwargs.sigma_max
        return s_min * (s_max / s_min) ** time

    # ---- operator seams (universe.py:314-316, 286) --------------------------------------------------
    def _sigma_table(self, n_steps):
        """The discretised schedule exactly as the reference builds it (universe.py:308-311): host arithmetic, done once per
        (n_steps, schedule)."""
        skey = (int(n_steps), float(self.diff_kwargs.sigma_min), float(self.diff_kwargs.sigma_max))
        sigma = self._sigma_cache.get(skey)
        if sigma is None:
            time = torch.linspace(0, 1, n_steps).to(torch.float32).flip(dims=[0])
            sigma = self.get_std_dev(time).to(torch.float32).contiguous()
            if len(self._sigma_cache) > 64:
                self._sigma_cache.clear()
            self._sigma_cache[skey] = sigma
        return sigma

    @staticmethod
    def _refuse_long_options(method, other):
        """enhance_long / enhance_long_many: the options of `enhance` that the segmented calls do not take, and typos."""
        for k in ("target", "ensemble", "fake_score_snr", "warm_start"):
            if other.get(k) is not None:
                hint = " (enhance_long_ensemble runs ensembles of long recordings)" if k == "ensemble" else ""
                raise ValueError(f"{method} does not take `{k}`{hint}")
        if other.get("use_aux_signal"):
            raise ValueError(f"{method} does not take `use_aux_signal`")
        unknown = set(other) - {"target", "ensemble", "fake_score_snr", "warm_start", "use_aux_signal", "ensemble_stat"}
        if unknown:
            raise TypeError(f"{method}() got unexpected keyword argument(s): {sorted(unknown)}")

    def _prep(self, x):
        if x.device != self.device:
            raise ValueError(f"input is on {x.device}, model on {self.device}")
        return x.to(torch.float32).contiguous()

    def condition_model(self, x, x_wav=None, train=False):
        """condition.py:346-377.  x: (B,1,T) normalised, T % tot_ds == 0.  Returns conditions or, with
        train=True, (conditions, aux_signal, latent) -- views into the workspace, valid until the next call."""
        self._sync_env()
        x = self._prep(x)
        if x.ndim != 3 or x.shape[1] != 1:
            raise ValueError("condition_model expects (B, 1, T)")
        B, _, T = x.shape
        if T % self.tot_ds:
            raise ValueError("the HIP conditioner needs T % tot_ds == 0 (enhance() pads accordingly)")
        ws = self._workspace(B, T)
        with torch.cuda.device(self.device):
            _lib.check(self._L.ou_condition(self._handle, c_void_p(x.data_ptr()), B, T, c_void_p(ws.data_ptr()),
                                            c_size_t(ws.numel()), self._stream()), self._handle)
        self._cond_key = (B, T)
        self._status()
        n_blocks = len(self.spec.score.rate_factors) + int(self.spec.cond.extra_conv_block)
        cond = [self.tensor(f"cond.c{j}") for j in range(n_blocks)]
        if train:
            return cond, self.tensor("cond.aux"), self.tensor("cond.latent")
        return cond

    def score_model(self, x, sigma, cond=None):
        """universe.py:197-209 / score.py:277-297: score(x, sigma | cond of the last condition_model call)."""
        self._sync_env()
        x = self._prep(x)
        B, _, T = x.shape
        if self._cond_key != (B, T):
            raise ValueError("score_model: call condition_model on a (B,1,T) input of the same shape first")
        sig = sigma.detach().to(torch.float32).cpu().contiguous()
        if sig.numel() != B:
            raise ValueError("sigma must have one entry per batch element")
        out = torch.empty_like(x)
        ws = self._ws
        with torch.cuda.device(self.device):
            _lib.check(self._L.ou_score(self._handle, c_void_p(x.data_ptr()),
                                        ctypes.cast(sig.data_ptr(), ctypes.POINTER(c_float)), c_void_p(out.data_ptr()),
                                        B, T, c_void_p(ws.data_ptr()), c_size_t(ws.numel()), self._stream()), self._handle)
        self._status()
        return out

    def aux_to_wav(self, y_aux=None):
        """universe_gan.py:145-149 on the aux signal of the last condition_model call."""
        if not self.spec.use_signal_decoupling:
            if y_aux is None:
                return self.tensor("cond.aux")
            return y_aux
        B, T = self._cond_key
        out = torch.empty(B, 1, T, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.ou_aux_to_wav(self._handle, c_void_p(out.data_ptr()), B, T, c_void_p(self._ws.data_ptr()),
                                             c_size_t(self._ws.numel()), self._stream()), self._handle)
        self._status()
        return out

    # ---- counter-based noise (noise.py; ou_set_noise_source) ------------------------------------------------------------
    @contextlib.contextmanager
    def _counter_source(self, seed, stream_ids, B=0, T=0):
        """The handle draws its noise from z(seed, stream_ids[row], draw, t) for the forward calls inside the `with` block and is
        back on the noise tensor (the default every other entry point expects) behind it.  (B, T) > 0: the call needs the
        two-plane scratch of ou_noise_scratch_bytes (ou_enhance / ou_enhance_var); ou_enhance_segments needs none."""
        n = len(stream_ids)
        spec = _lib.NoiseSpec()
        spec.seed = int(seed)
        spec.streams = (ctypes.c_uint64 * n)(*[int(v) for v in stream_ids])
        spec.n_streams = n
        if B and T:
            need = c_size_t()
            _lib.check(self._L.ou_noise_scratch_bytes(self._handle, int(B), int(T), byref(need)), self._handle)
            buf = self.__dict__.get("_noise_scratch")
            if buf is None or buf.numel() < need.value:  # kept and grown like the workspace
                self._noise_scratch = None
                buf = self._noise_scratch = torch.empty(need.value, dtype=torch.uint8, device=self.device)
            spec.scratch = buf.data_ptr()
            spec.scratch_bytes = buf.numel()
        _lib.check(self._L.ou_set_noise_source(self._handle, byref(spec)), self._handle)
        try:
            yield
        finally:
            self._L.ou_set_noise_source(self._handle, None)

    def noise_fill(self, streams, t0, lengths, seed, draw, cols=None, out=None):
        """z(seed, streams[j], draw, t0[j] + i) for i < lengths[j] (0 behind it) as a (rows, cols) float32 tensor on this
        model's device -- the library's own evaluation of the counter-based noise (ou_noise_fill), e.g. to hand the noise of a
        `CounterNoise` run to something that takes tensors."""
        n = len(streams)
        cols = int(max(lengths) if cols is None else cols)
        if out is None:
            out = torch.empty((n, cols), dtype=torch.float32, device=self.device)
        if out.shape != (n, cols) or out.dtype != torch.float32 or out.stride(1) != 1 or not out.is_cuda:
            raise ValueError("noise_fill: out must be a (rows, cols) float32 device tensor with unit column stride")
        with torch.cuda.device(self.device):
            _lib.check(self._L.ou_noise_fill(c_void_p(out.data_ptr()), out.stride(0), cols, n,
                                             (ctypes.c_uint64 * n)(*[int(v) for v in streams]),
                                             (ctypes.c_int64 * n)(*[int(v) for v in t0]),
                                             (ctypes.c_int64 * n)(*[int(v) for v in lengths]), int(seed), int(draw),
                                             self._stream()))
        return out

    # ---- what the enhance methods are arranged from (the Python side) ---------------------------------
    def _defaults(self, n_steps, epsilon):
        return (self.diff_kwargs.n_steps if n_steps is None else int(n_steps),
                self.diff_kwargs.epsilon if epsilon is None else epsilon)

    def _begin(self, n_steps=None, epsilon=None, segment_s=None, overlap_s=None):
        """What every enhance call starts with: environment steering (tools only), a look at the deferred status of an earlier
        call, the per-call defaults.  -> (n_steps, epsilon), with a window also (.., segment, overlap) in samples."""
        self._sync_env()
        self._poll_deferred_status()
        n_steps, epsilon = self._defaults(n_steps, epsilon)
        if segment_s is None:
            return n_steps, epsilon
        return n_steps, epsilon, int(round(float(segment_s) * self.fs)), int(round(float(overlap_s) * self.fs))

    @staticmethod
    def _lift(mix):
        """(T,) / (B, T) / (B, 1, T) -> ((B, 1, T), the rank to give back); `_lower` is the inverse."""
        x_ndim = mix.ndim
        if x_ndim == 1:
            mix = mix[None, None, :]
        elif x_ndim == 2:
            mix = mix[:, None, :]
        elif x_ndim > 3:
            raise ValueError("The input should have at most 3 dimensions")
        if mix.ndim == 3 and mix.shape[1] != 1:
            raise ValueError("enhance expects single-channel signals: (T,), (B,T) or (B,1,T)")
        return mix, x_ndim

    @staticmethod
    def _lower(x_ndim, x, members=None):
        """(B, 1, L) and, if any, the members (E, B, 1, L) back at the rank of the input."""
        if x_ndim == 1:
            return x[0, 0], (None if members is None else members[:, 0, 0])
        if x_ndim == 2:
            return x[:, 0, :], (None if members is None else members[:, :, 0, :])
        return x, members

    def _long_rows(self, mix, who):
        """The (T,) / (C, T) input of a segmented call as prepared (C, T) rows."""
        x = as_rows(mix, who, self._prep, "T")
        if x.shape[-1] < 1:
            raise ValueError(f"{who}: empty input signal")
        return x

    def _forward(self, fn, bufs, dims, n_steps, epsilon, warm_start, flags, ws, counter=None, scratch=(), cond_key=_KEEP):
        """The one call into a sampler entry point: fn(handle, *pointers of bufs (None: NULL), *dims, n_steps, epsilon, sigma table,
        warm_start, flags, workspace, its bytes, stream) on this model's device, inside the counter source `counter` = (seed,
        stream ids) if there is one -- `scratch` = (rows, T) where the call needs the two-plane noise scratch --, return code
        mapped to the reference's exceptions, `cond_key` recorded, status word polled."""
        sigma = self._sigma_table(n_steps)
        source = self._counter_source(counter[0], counter[1], *scratch) if counter is not None else contextlib.nullcontext()
        with torch.cuda.device(self.device), source:
            _lib.check(fn(self._handle, *[None if b is None else c_void_p(b.data_ptr()) for b in bufs], *dims, int(n_steps),
                          float(epsilon), ctypes.cast(sigma.data_ptr(), ctypes.POINTER(c_float)),
                          -1 if warm_start is None else int(warm_start), flags, c_void_p(ws.data_ptr()), c_size_t(ws.numel()),
                          self._stream()), self._handle)
        if cond_key is not _KEEP:
            self._cond_key = cond_key
        self._status()

    def _segments_sizer(self, sizer, *args):
        """A segment workspace sizer (ou_segments*_workspace_bytes) and the buffer it asks for: -> (ws, walk rows B, walk length L)."""
        need, B, L = c_size_t(), c_int32(), c_int32()
        _lib.check(sizer(self._handle, *args, byref(need), byref(B), byref(L)), self._handle)
        return self._segments_workspace(B.value, L.value, need.value), B.value, L.value

    # ---- the hot path ------------------------------------------------------------------------------
    def enhance(
        self,
        mix,
        n_steps: Optional[int] = None,
        epsilon: Optional[float] = None,
        target: Optional[torch.Tensor] = None,
        fake_score_snr: Optional[float] = None,
        rng: Optional[torch.Generator] = None,
        use_aux_signal: Optional[bool] = False,
        keep_rms: Optional[bool] = False,
        ensemble: Optional[int] = None,
        ensemble_stat: Optional[str] = "median",
        warm_start: Optional[int] = None,
    ) -> torch.Tensor:
        """Universe.enhance, universe.py:231-375 (same arguments, same return convention).

        Extension: `rng=noise.CounterNoise(seed, stream=u)` -- the noise comes from the counter-based function of noise.py
        instead of a generator: row (channel) c of the input draws from stream id `(u << 16) | c`, nothing is drawn or stored
        on the Python side and no generator advances.  With `ensemble=E` member e draws from the ids of the input plus
        `e << 48`, so the members differ as they do with a generator.  `target` (the oracle-score debug path, pure torch) keeps
        its generator and refuses a CounterNoise."""
        return self._enhance(mix, n_steps, epsilon, target, fake_score_snr, rng, use_aux_signal, keep_rms, ensemble,
                             ensemble_stat, warm_start, None)

    @torch.no_grad()
    def _enhance(self, mix, n_steps, epsilon, target, fake_score_snr, rng, use_aux_signal, keep_rms, ensemble,
                 ensemble_stat, warm_start, noise, t_raw=None, counter=None):
        """`t_raw`: per-row lengths of a batch whose rows are utterances of different lengths (enhance_many, exact
        batching -> ou_enhance_var); `mix` is then (B, 1, max length) and `noise` a (n, B, 1, T) tensor.
        `counter`: (seed, [one stream id per row]) -- counter-based noise (noise.py) instead of `noise` / `rng`."""
        n_steps, epsilon = self._begin(n_steps, epsilon)
        mix, x_ndim = self._lift(mix)
        if ensemble_stat not in ("mean", "median", "signal_median") and ensemble is not None:
            raise NotImplementedError()  # universe.py:368
        mix = self._prep(mix)
        if ensemble is not None:
            mix_shape = mix.shape
            if keep_rms and mix_shape[0] != 1:
                # universe.py:259 computes mix_rms before the replication (:261-264): the reference fails to
                # broadcast (B,1,1) against (E*B,1,T) at :354 for B > 1; same behaviour here.
                raise RuntimeError("keep_rms with ensemble is only defined for a single input signal (as in the reference)")
            mix = torch.stack([mix] * ensemble, dim=0).view((-1,) + mix_shape[1:])
        B, _, mix_len = mix.shape
        T = padded(mix_len, self.tot_ds)
        pad = T - mix_len
        if is_counter(rng):
            if target is not None:
                raise ValueError("`target` (the oracle-score path) draws from a torch.Generator: it does not take a CounterNoise")
            if noise is not None or counter is not None:
                raise ValueError("give either a CounterNoise or a noise tensor")
            counter = (rng.seed, rng.stream_ids(B if ensemble is None else B // int(ensemble), ensemble))
        if counter is not None and len(counter[1]) != B:
            raise ValueError("counter-based noise needs one stream id per row of the batch")

        if target is not None:
            x = self._enhance_with_oracle_score(mix, target, n_steps, epsilon, fake_score_snr, rng, pad)
        else:
            n_start = 0 if warm_start is None else int(warm_start)
            n_noise = 0 if use_aux_signal else n_steps - n_start
            if t_raw is not None:
                if ensemble is not None:
                    raise ValueError("per-row lengths and `ensemble` do not combine (call enhance per input)")
                noise_t = noise
                if counter is not None:
                    noise_t = None
                elif n_noise and (noise_t is None or tuple(noise_t.shape) != (n_noise, B, 1, T)):
                    raise ValueError(f"noise must be a tensor of shape {(n_noise, B, 1, T)}")
            elif counter is not None:
                noise_t = None  # the library fills one step's plane at a time (ou_set_noise_source)
            elif noise is None:
                # draw order of the reference: x0, then z_n for n = n_start .. N-2 (universe.py:326,330,338): the whole-plane case
                # of draw_noise -- n separate (B, 1, T) draws, each `out=` into its slice of the tensor the C ABI takes, no
                # temporaries, no copies -- queued BEFORE the host prepares the call (the device is idle meanwhile)
                # (n_noise <= 0: warm_start >= n_steps -- the C ABI refuses the call below)
                noise_t = draw_noise(self.tot_ds, [(B, mix_len, rng)], n_noise, device=self.device) if n_noise > 0 else None
            elif torch.is_tensor(noise):  # (all steps in one (n, B, 1, T) tensor: taken as it is)
                noise_t = self._prep(noise[:n_noise]) if n_noise else None
                if n_noise and tuple(noise_t.shape) != (n_noise, B, 1, T):
                    raise ValueError(f"noise must be a tensor of shape {(n_noise, B, 1, T)}")
            else:
                noise_t = torch.stack([self._prep(z) for z in noise[:n_noise]], dim=0) if n_noise else None
                if n_noise and noise_t.shape != (n_noise, B, 1, T):
                    raise ValueError(f"noise must be {n_noise} tensors of shape {(B, 1, T)}")
            out = torch.empty(B, 1, mix_len, dtype=torch.float32, device=self.device)
            ws = self._workspace(B, T)
            flags = (_lib.OU_ENH_KEEP_RMS if keep_rms else 0) | (_lib.OU_ENH_USE_AUX_SIGNAL if use_aux_signal else 0)
            fn, dims = self._L.ou_enhance, (B, mix_len)
            if t_raw is not None:
                if len(t_raw) != B:
                    raise ValueError("t_raw must have one entry per row of the batch")
                fn, dims = self._L.ou_enhance_var, (B, mix_len, (c_int32 * B)(*[int(v) for v in t_raw]))
            self._forward(fn, (mix, out, noise_t), dims, n_steps, epsilon, warm_start, flags, ws, counter, (B, T),
                          cond_key=(B, T) if t_raw is None else None)
            x = out

        if target is not None:
            if keep_rms:
                mix_rms = mix.square().mean(dim=(-2, -1), keepdim=True).sqrt()
                x_rms = x.square().mean(dim=(-2, -1), keepdim=True).sqrt().clamp(min=1e-5)
                x = x * (mix_rms / x_rms)
            scale = abs(x).max(dim=-1, keepdim=True).values
            x = torch.where(scale > 1.0, x / scale, x)

        if ensemble is not None:  # universe.py:359-368 (host-side glue over E replicas of the same utterance)
            x = x.view((-1,) + mix_shape)
            if ensemble_stat == "mean":
                x = x.mean(dim=0)
            elif ensemble_stat == "median":
                x = x.median(dim=0).values
            elif ensemble_stat == "signal_median":
                x = signal_median(x)
            else:
                raise NotImplementedError()
        return self._lower(x_ndim, x)[0]

    @torch.no_grad()
    def enhance_many(self, signals, rngs=None, pad_batch=False, n_steps=None, epsilon=None, use_aux_signal=False,
                     keep_rms=False, warm_start=None, ensemble=None, ensemble_stat="median", return_members=False, **other):
        """Several independent inputs in ONE `enhance` call (extension; the reference's CLI loops over files one by one,
        bin/enhance.py:173-192).  `signals`: list of (L,) or (C, L) tensors -- a (C, L) entry is a file whose channels
        are rows of the batch, as in the reference.  `rngs`: one generator per entry, ONE shared generator, or None -- or
        `noise.CounterNoise` objects (one per entry with one seed, or ONE shared: entry i is then utterance `stream + i`); channel
        c of an entry draws from stream id `(utterance << 16) | c`, and nothing is drawn here (no noise tensor exists).
        The noise of entry i is drawn from its generator entry by entry, step by step, with the shapes a call on that
        entry alone would use ((C_i, 1, T), x0 first) -- with a shared generator the draws come in exactly the order
        of the serial loop, so its state advances as the reference's does.
        pad_batch=False (default): EXACT batching -- entries may have any lengths, and every row is the signal it would be in
        a call of its own (own pad() split, own normalisation and mel norm, zero padding of every conv right behind its own
        last sample, GRU passes over its own frames: ou_enhance_var); the noise of entry i has the shape of that call,
        (C_i, 1, L_i + pad_i).  Agrees with the one-by-one loop to fp32 round-off (the kernels a batch selects differ).
        pad_batch=True: right-zero-padded to the longest entry like `max_collator` (datasets/datamodule.py:24-42);
        the reference has no mask, the padding takes part in the normalisation / mel norm / GRU; outputs are cropped.
        `ensemble=E` (with `ensemble_stat`): every entry is enhanced E times and reduced as `enhance(entry, ensemble=E)` does,
        all entries in one ou_enhance_ensemble call (exact batching only: refused with pad_batch=True).  With generators the
        noise of entry i is what `enhance(entry_i, ensemble=E, rng=..)` would draw alone ((E * C_i, 1, T_i) per step,
        member-major), in serial-loop order; with CounterNoise member e of a row draws from the row's id + (e << 48)
        (`stream_ids(C_i, E)`).  return_members=True (with `ensemble`): -> (results, members), members[i] of shape (E,) + the
        shape of entry i.
        Returns the list of enhanced signals, each with the shape of its input."""
        for k in ("target", "fake_score_snr"):
            if other.get(k) is not None:
                raise ValueError(f"enhance_many does not take `{k}` (call enhance per input)")
        unknown = set(other) - {"target", "fake_score_snr", "rng"}
        if unknown:  # (a typo must not change behaviour on the batched path only)
            raise TypeError(f"enhance_many() got unexpected keyword argument(s): {sorted(unknown)}")
        if other.get("rng") is not None:
            raise ValueError("enhance_many takes the generators as `rngs` (one per input, or one shared)")
        if not signals:
            return []
        pk = pack_rows(signals, "enhance_many", self._prep)
        n_steps = self._defaults(n_steps, None)[0]
        n_start = 0 if warm_start is None else int(warm_start)
        if n_start >= n_steps:
            raise ValueError("warm_start must be < n_steps")
        n_noise = 0 if use_aux_signal else n_steps - n_start
        counter = self._counter_plan(rngs, pk.chans)
        if ensemble is not None:
            return self._enhance_many_ensemble(pk, rngs, counter, int(ensemble), ensemble_stat, pad_batch, n_steps, epsilon,
                                               use_aux_signal, keep_rms, warm_start, n_noise, return_members)
        if return_members:
            raise ValueError("enhance_many: return_members needs `ensemble`")
        # exact batching of different lengths: per-row geometry through the whole path (t_raw -> ou_enhance_var), every entry
        # draws at its own padded length; otherwise one plain batch, every entry draws at the padded length of the longest
        ragged = not pad_batch and any(n != max(pk.lens) for n in pk.lens)
        extra = {} if counter is None else {"counter": counter}
        if ragged:
            extra["t_raw"] = pk.row_lens
        noise = None
        if counter is None and n_noise:
            noise = draw_noise(self.tot_ds, pk.entries(rngs, own_length=ragged), n_noise, device=self.device)
        out = self._enhance(pk.batch[:, None, :], n_steps, epsilon, None, None, None, use_aux_signal, keep_rms, None, "median",
                            warm_start, noise, **extra)
        return unpack_rows(pk, out)[0]

    # ---- ensembles inside the library (ou_enhance_ensemble) ---------------------------------------------------------------
    def _ensemble_call(self, mix, E, stat, n_steps, epsilon, keep_rms, warm_start, noise_t, t_raw, counter, return_members):
        """mix: (B, 1, L) prepared; noise_t: (n, E * B, 1, T) or None (counter: (seed, E * B member-major stream ids)).
        -> (out (B, 1, L), members (E, B, 1, L) or None)."""
        if stat not in _lib.ENSEMBLE_STATS:
            raise NotImplementedError()  # universe.py:368
        B, _, mix_len = mix.shape
        T = padded(mix_len, self.tot_ds)
        out = torch.empty(B, 1, mix_len, dtype=torch.float32, device=self.device)
        members = torch.empty(E, B, 1, mix_len, dtype=torch.float32, device=self.device) if return_members else None
        need = c_size_t()
        _lib.check(self._L.ou_ensemble_workspace_bytes(self._handle, B, T, E, byref(need)), self._handle)
        ws = self._workspace(E * B, T, need=need.value)
        rows_len = None if t_raw is None else (c_int32 * B)(*[int(v) for v in t_raw])
        self._forward(self._L.ou_enhance_ensemble, (mix, out, members, noise_t), (B, mix_len, rows_len, E, _lib.ENSEMBLE_STATS[stat]),
                      n_steps, epsilon, warm_start, _lib.OU_ENH_KEEP_RMS if keep_rms else 0, ws, counter, (E * B, T), cond_key=None)
        return out, members

    @torch.no_grad()
    def enhance_ensemble(self, mix, ensemble: int, ensemble_stat: str = "median", n_steps: Optional[int] = None,
                         epsilon: Optional[float] = None, rng=None, keep_rms: bool = False,
                         warm_start: Optional[int] = None, return_members: bool = False):
        """`enhance(mix, ensemble=E, ensemble_stat=..)` inside the library (extension, ou_enhance_ensemble): the conditioner runs
        once over the inputs instead of E times (option `ens_share`), the members are reduced on the device.  Input shapes and
        return convention of `enhance`; `rng`: a generator -- the draws are the (E * B, 1, T) shapes and order of
        `enhance(ensemble=E)`, so one seed gives both paths the same noise -- or a `CounterNoise` (member e of row b draws from
        the row's id + (e << 48)).  keep_rms restores every member to the RMS of its own input (for one input: the reference's
        result; the reference fails for more).  return_members=True: -> (result, members), members (E,) + the result's shape.
        Members agree with those of `enhance(ensemble=E)` to fp32 round-off (the conditioner's B-row pass may select other
        kernels); with `set_option("ens_share", 0)` bit for bit."""
        n_steps, epsilon = self._begin(n_steps, epsilon)
        E = int(ensemble)
        if not 1 <= E <= _lib.OU_MAX_ENSEMBLE:
            raise ValueError(f"enhance_ensemble: 1 <= ensemble <= {_lib.OU_MAX_ENSEMBLE}")
        mix, x_ndim = self._lift(mix)
        mix = self._prep(mix)
        B, _, mix_len = mix.shape
        n_noise = n_steps - (0 if warm_start is None else int(warm_start))
        counter, noise_t = None, None
        if is_counter(rng):
            counter = (rng.seed, rng.stream_ids(B, E))
        elif n_noise > 0:  # (n_noise <= 0: the C ABI refuses the call)
            noise_t = draw_noise(self.tot_ds, [(B, mix_len, rng)], n_noise, E, device=self.device)
        out, members = self._lower(x_ndim, *self._ensemble_call(mix, E, ensemble_stat, n_steps, epsilon, keep_rms, warm_start,
                                                                noise_t, None, counter, return_members))
        return (out, members) if return_members else out

    def _enhance_many_ensemble(self, pk, rngs, counter, E, stat, pad_batch, n_steps, epsilon, use_aux_signal, keep_rms,
                               warm_start, n_noise, return_members=False):
        """enhance_many(ensemble=E): all entries in one ou_enhance_ensemble call with per-row lengths."""
        if pad_batch:
            raise ValueError("enhance_many: `ensemble` runs with exact batching only (pad_batch=True is refused)")
        if use_aux_signal:
            raise ValueError("enhance_many: `ensemble` with use_aux_signal is refused (without noise all members are equal)")
        if not 1 <= E <= _lib.OU_MAX_ENSEMBLE:
            raise ValueError(f"enhance_many: 1 <= ensemble <= {_lib.OU_MAX_ENSEMBLE}")
        n_steps, epsilon = self._begin(n_steps, epsilon)
        noise_t = None
        if counter is not None:
            counter = (counter[0], [s + (e << ENSEMBLE_SHIFT) for e in range(E) for s in counter[1]])
        else:  # the draws of enhance(entry, ensemble=E) alone: (E * C_i, 1, T_i), member-major
            noise_t = draw_noise(self.tot_ds, pk.entries(rngs), n_noise, E, device=self.device)
        out, mem = self._ensemble_call(pk.batch[:, None, :], E, stat, n_steps, epsilon, keep_rms, warm_start, noise_t, pk.row_lens,
                                       counter, return_members)
        res, mems = unpack_rows(pk, out, mem)
        return (res, mems) if return_members else res

    @staticmethod
    def _counter_plan(rngs, channels):
        """`rngs` of enhance_many -> None (generators) or (seed, [stream id per row]) for CounterNoise sources: one per entry, or
        one shared (entry i = utterance stream + i); `channels[i]`: rows of entry i."""
        per_entry = isinstance(rngs, (list, tuple))
        srcs = list(rngs) if per_entry else [rngs]
        if not any(is_counter(g) for g in srcs):
            return None
        if not all(is_counter(g) for g in srcs):
            raise ValueError("enhance_many: CounterNoise sources and generators do not mix in one call")
        if per_entry:
            if len(srcs) != len(channels):
                raise ValueError("enhance_many: one CounterNoise per input (or one shared)")
            if len({g.seed for g in srcs}) != 1:
                raise ValueError("enhance_many: the CounterNoise sources of one call must share their seed")
        else:
            srcs = [rngs.at(i) for i in range(len(channels))]
        ids = [v for g, c in zip(srcs, channels) for v in g.stream_ids(c)]
        if len(set(ids)) != len(ids):
            raise ValueError("enhance_many: two rows of the call would draw the same noise (equal stream ids)")
        return srcs[0].seed, ids

    def advance_generator_like_enhance(self, rng, channels, length, n_steps=None, warm_start=None, use_aux_signal=False):
        """Advance `rng` by exactly the draws `enhance` makes for a (channels, length) input -- x0, then one z per noisy step
        (universe.py:326,330,338), each of shape (channels, 1, length + pad) -- without running anything.  For callers that
        re-order work but owe every input the noise of the serial loop: take `rng.get_state()` in front of an input, call this,
        and hand a generator restored to that state to the call that really processes the input (the CLI's length-sorted
        window, bin/enhance.py)."""
        n_steps = self.diff_kwargs.n_steps if n_steps is None else int(n_steps)
        n_noise = 0 if use_aux_signal else n_steps - (0 if warm_start is None else int(warm_start))
        draw_noise(self.tot_ds, [(int(channels), int(length), rng)], n_noise, device=self.device, discard=True)

    def draw_noise_like_enhance(self, rng, channels, length, n_steps=None, planes=None):
        """The noise `enhance` draws for a (channels, length) input -- x0, then one z per noisy step, each (channels, 1, length
        + pad) -- in ONE (n_steps, channels, length + pad) tensor, drawn in that order from `rng`.  `planes`: the number of
        draws where it is not n_steps (a warm start at step k draws n_steps - k)."""
        n_steps = self.diff_kwargs.n_steps if n_steps is None else int(n_steps)
        n = n_steps if planes is None else int(planes)
        return draw_noise(self.tot_ds, [(int(channels), int(length), rng)], n, device=self.device)[:, :, 0]

    @staticmethod
    def _long_planes(who, n_steps, warm_start, use_aux_signal):
        """Noise planes of a segmented call, as `enhance` counts them: n_steps - warm_start, none for the aux exit."""
        n_start = 0 if warm_start is None else int(warm_start)
        if not 0 <= n_start < n_steps:
            raise ValueError(f"{who}: warm_start must lie in [0, n_steps)")
        return 0 if use_aux_signal else n_steps - n_start

    # ---- recordings of any length: segmented enhance (ou_enhance_segments) ---------------------------------------------
    SEGMENT_S = 8.0
    OVERLAP_S = 1.0

    @torch.no_grad()
    def enhance_long(self, mix, segment_s: float = SEGMENT_S, overlap_s: float = OVERLAP_S, max_batch: int = 32,
                     rng: Optional[torch.Generator] = None, n_steps: Optional[int] = None, epsilon: Optional[float] = None,
                     keep_rms: Optional[bool] = False, warm_start: Optional[int] = None, use_aux_signal: bool = False,
                     **other) -> torch.Tensor:
        """`enhance` of a recording of any length in bounded memory (extension).  `mix`: (T,) or (C, T); rows are independent
        signals, as channels are everywhere else.  The signal is cut into windows of `segment_s` seconds that overlap by
        `overlap_s` seconds and run `max_batch` at a time through the walk of `enhance`; normalisation, mel scale, noise,
        keep_rms and the peak guard stay those of the whole file (include/ouniverse.h, ou_enhance_segments).  The noise is
        drawn exactly as `enhance` draws it for this input, so a shared generator advances identically -- as ONE (n_steps, C,
        T_pad) tensor, n_steps times the recording.  `rng=noise.CounterNoise(seed, u)` removes that tensor: every window's noise
        is computed at its offset from the counter-based function (row c: stream id (u << 16) | c), and the memory of the call is
        the workspace plus input and output.  A file that fits into one window gets the `enhance` result.  Workspace: ou_segments_workspace_bytes -- set by max_batch and segment_s.
        `warm_start=k` / `use_aux_signal=True` (UNIVERSE++ with the snake decoupling layer): every window starts at step k from
        its own conditioner estimate plus noise, or IS that estimate (no score pass); the draws are those of `enhance` with the
        same arguments -- n_steps - k planes, none for the aux exit, which leaves the generator where it was.
        Ensembles of long recordings: `enhance_long_ensemble` (`ensemble=` is refused here)."""
        self._refuse_long_options("enhance_long", other)
        n_steps, epsilon, segment, overlap = self._begin(n_steps, epsilon, segment_s, overlap_s)
        planes = self._long_planes("enhance_long", n_steps, warm_start, use_aux_signal)
        x = self._long_rows(mix, "enhance_long")
        C, T_raw = x.shape
        if is_counter(rng):
            noise, counter = None, (rng.seed, rng.stream_ids(C))
        else:
            noise, counter = (self.draw_noise_like_enhance(rng, C, T_raw, n_steps, planes) if planes else None), None
        out = self._segments_call(x, segment, overlap, max_batch, n_steps, epsilon, keep_rms, noise, counter, warm_start,
                                  use_aux_signal)
        return out if mix.ndim == 2 else out[0]

    def _segments_plan(self, C, T, segment, overlap, max_batch, ensemble=None, t_raw=None, warm_start=None, use_aux_signal=False):
        """What tells the four segmented entry points apart -- plain, `ensemble` = (E, stat), `t_raw` = a length per row, or both --,
        sized: -> (library function, its arguments between the noise pointer and n_steps, workspace, and the mode of the call:
        warm_start, use_aux_signal -- the sizers answer the same for every mode)."""
        geo = (segment, overlap, int(max_batch))
        if ensemble is not None and t_raw is not None:
            fn, sizer = self._L.ou_enhance_segments_var_ensemble, self._L.ou_segments_var_ensemble_workspace_bytes
            sized, dims = (C, t_raw) + geo + (ensemble[0],), (C, T, t_raw, ensemble[0], _lib.ENSEMBLE_STATS[ensemble[1]]) + geo
        elif ensemble is not None:
            fn, sizer = self._L.ou_enhance_segments_ensemble, self._L.ou_segments_ensemble_workspace_bytes
            sized, dims = (C, T) + geo + (ensemble[0],), (C, T, ensemble[0], _lib.ENSEMBLE_STATS[ensemble[1]]) + geo
        elif t_raw is not None:
            fn, sizer = self._L.ou_enhance_segments_var, self._L.ou_segments_var_workspace_bytes
            sized, dims = (C, t_raw) + geo, (C, T, t_raw) + geo
        else:
            fn, sizer = self._L.ou_enhance_segments, self._L.ou_segments_workspace_bytes
            sized, dims = (C, T) + geo, (C, T) + geo
        return fn, dims, self._segments_sizer(sizer, *sized)[0], warm_start, bool(use_aux_signal)

    def _segments_run(self, plan, x, n_steps, epsilon, keep_rms, noise, counter, members=None):
        """The call `plan` (_segments_plan) on the prepared (C, T) rows `x` -> out (C, T); `members`: the (E, C, T) tensor an
        ensemble writes its members to.  Noise as in `_segments_call`; no noise scratch (the library fills window by window)."""
        fn, dims, ws, warm_start, use_aux_signal = plan
        out = torch.empty(x.shape, dtype=torch.float32, device=self.device)
        flags = (_lib.OU_ENH_KEEP_RMS if keep_rms else 0) | (_lib.OU_ENH_USE_AUX_SIGNAL if use_aux_signal else 0)
        self._forward(fn, (x, out, noise) if members is None else (x, out, members, noise), dims, n_steps, epsilon, warm_start,
                      flags, ws, counter if noise is None else None)
        return out

    def _segments_call(self, x, segment, overlap, max_batch, n_steps, epsilon, keep_rms, noise, counter, warm_start=None,
                       use_aux_signal=False):
        """ou_enhance_segments of the prepared (C, T_raw) rows `x` on `noise` ((n_steps - (warm_start or 0), C, T_pad); None for
        the aux exit) or, with noise None, on the counter source `counter` = (seed, C stream ids).  (Also what the tests of
        enhance_long_ensemble run a single member row through, on that member's own noise or stream id.)"""
        plan = self._segments_plan(*x.shape, segment, overlap, max_batch, warm_start=warm_start, use_aux_signal=use_aux_signal)
        return self._segments_run(plan, x, n_steps, epsilon, keep_rms, noise, counter)

    @torch.no_grad()
    def enhance_long_ensemble(self, mix, ensemble: int, ensemble_stat: str = "median", segment_s: float = SEGMENT_S,
                              overlap_s: float = OVERLAP_S, max_batch: int = 32, rng=None, n_steps: Optional[int] = None,
                              epsilon: Optional[float] = None, keep_rms: bool = False, return_members: bool = False):
        """`enhance_ensemble` of a recording of any length (extension; ou_enhance_segments_ensemble).  `mix`: (T,) or (C, T), rows
        are independent signals.  Member e of row c is `enhance_long` of row c alone on that member's noise (to fp32 round-off:
        the kernels a group selects differ), the result is `ensemble_reduce` over the post-processed members of every row.  The
        windows of `enhance_long` run in groups of at most `max_batch` walk rows, all E members of a window in one group, and the
        conditioner runs once per window, not once per member (option `ens_share`).  `rng`: a generator -- the draws are those of
        `enhance(mix, ensemble=E)` for this input, n_steps draws of (E * C, 1, T_pad), so it ends where
        `advance_generator_like_enhance(rng, E * C, T)` ends -- or a `CounterNoise` (member e of row c: `stream_ids(C, E)`; no
        noise tensor exists then).  Memory: the workspace (set by max_batch and segment_s) plus the E member rows of every
        input row -- the one part that grows with the recording.  return_members=True: -> (result, members (E,) + mix.shape)."""
        n_steps, epsilon, segment, overlap = self._begin(n_steps, epsilon, segment_s, overlap_s)
        E = int(ensemble)
        if not 1 <= E <= _lib.OU_MAX_ENSEMBLE:
            raise ValueError(f"enhance_long_ensemble: 1 <= ensemble <= {_lib.OU_MAX_ENSEMBLE}")
        if ensemble_stat not in _lib.ENSEMBLE_STATS:
            raise NotImplementedError()  # universe.py:368
        x = self._long_rows(mix, "enhance_long_ensemble")
        C, T_raw = x.shape
        plan = self._segments_plan(C, T_raw, segment, overlap, max_batch, ensemble=(E, ensemble_stat))
        if is_counter(rng):
            noise, counter = None, (rng.seed, rng.stream_ids(C, E))
        else:
            noise, counter = self.draw_noise_like_enhance(rng, E * C, T_raw, n_steps), None
        members = torch.empty(E, C, T_raw, dtype=torch.float32, device=self.device)
        out = self._segments_run(plan, x, n_steps, epsilon, keep_rms, noise, counter, members)
        if mix.ndim == 1:
            out, members = out[0], members[:, 0]
        return (out, members) if return_members else out

    @torch.no_grad()
    def enhance_long_many(self, signals, rngs=None, segment_s: float = SEGMENT_S, overlap_s: float = OVERLAP_S,
                          max_batch: int = 32, n_steps: Optional[int] = None, epsilon: Optional[float] = None,
                          keep_rms: Optional[bool] = False, warm_start: Optional[int] = None, use_aux_signal: bool = False,
                          **other):
        """`enhance_long` of several independent inputs of ANY lengths in ONE call (extension; ou_enhance_segments_var).
        `signals`: list of (L,) or (C, L) tensors, channels are rows as in `enhance_many`.  Inputs longer than a window are cut
        into windows, shorter ones are one window each, and the windows of all rows share the window groups of `max_batch`;
        every row still gets what `enhance_long` gives it alone (whole-row normalisation, mel scale, noise, keep_rms and peak
        guard of its own; to fp32 round-off, since the kernels a group selects differ).  `rngs`: one generator per input, ONE
        shared generator (it advances input by input, as `enhance_long` draws for each), or None -- or `noise.CounterNoise`
        objects as in `enhance_many` (one per input with one seed, or one shared: input i is utterance `stream + i`).
        `warm_start` / `use_aux_signal`: as in `enhance_long`, for every input.
        Returns the list of enhanced signals, each with the shape of its input."""
        self._refuse_long_options("enhance_long_many", other)
        if not signals:
            return []
        n_steps, epsilon, segment, overlap = self._begin(n_steps, epsilon, segment_s, overlap_s)
        planes = self._long_planes("enhance_long_many", n_steps, warm_start, use_aux_signal)
        pk = pack_rows(signals, "enhance_long_many", self._prep)
        C, l_max = pk.batch.shape
        plan = self._segments_plan(C, l_max, segment, overlap, max_batch, t_raw=(ctypes.c_int64 * C)(*pk.row_lens),
                                   warm_start=warm_start, use_aux_signal=use_aux_signal)
        counter = self._counter_plan(rngs, pk.chans)
        noise = None
        if counter is None and planes:  # the draws of `enhance_long` on every input alone, input by input: (C_i, 1, T_i) per
            # step, x0 first
            noise = draw_noise(self.tot_ds, pk.entries(rngs), planes, device=self.device)
        return unpack_rows(pk, self._segments_run(plan, pk.batch, n_steps, epsilon, keep_rms, noise, counter))[0]

    @torch.no_grad()
    def enhance_long_many_ensemble(self, signals, ensemble: int, ensemble_stat: str = "median", rngs=None,
                                   segment_s: float = SEGMENT_S, overlap_s: float = OVERLAP_S, max_batch: int = 32,
                                   n_steps: Optional[int] = None, epsilon: Optional[float] = None, keep_rms: bool = False,
                                   return_members: bool = False, **other):
        """`enhance_long_ensemble` of several independent inputs of ANY lengths in ONE call (extension;
        ou_enhance_segments_var_ensemble).  `signals`: list of (L,) or (C, L) tensors, channels are rows as in `enhance_long_many`.
        The windows of all rows share the window groups of floor(max_batch / E) entries, all E members of a window in one group;
        every row still gets what `enhance_long_ensemble` gives it alone (to fp32 round-off, since the kernels a group selects
        differ).  `rngs`: one generator per input, ONE shared generator (it advances input by input: it ends where the loop of
        `advance_generator_like_enhance(g, E * C_i, L_i)` over the inputs leaves it), or None -- or `noise.CounterNoise` objects
        as in `enhance_long_many` (input i draws from `CounterNoise(seed, stream + i).stream_ids(C_i, E)`).  Returns the list of
        results, each with the shape of its input; return_members=True: -> (results, [members (E,) + that shape])."""
        self._refuse_long_options("enhance_long_many_ensemble", other)
        E = int(ensemble)
        if not 1 <= E <= _lib.OU_MAX_ENSEMBLE:
            raise ValueError(f"enhance_long_many_ensemble: 1 <= ensemble <= {_lib.OU_MAX_ENSEMBLE}")
        if ensemble_stat not in _lib.ENSEMBLE_STATS:
            raise NotImplementedError()  # universe.py:368
        if not signals:
            return ([], []) if return_members else []
        n_steps, epsilon, segment, overlap = self._begin(n_steps, epsilon, segment_s, overlap_s)
        pk = pack_rows(signals, "enhance_long_many_ensemble", self._prep)
        C, l_max = pk.batch.shape
        plan = self._segments_plan(C, l_max, segment, overlap, max_batch, ensemble=(E, ensemble_stat),
                                   t_raw=(ctypes.c_int64 * C)(*pk.row_lens))
        counter = self._counter_plan(rngs, pk.chans)
        noise = None
        if counter is not None:  # member e of a row: the row's id + (e << ENSEMBLE_SHIFT), member-major over all rows
            counter = (counter[0], [s + (e << ENSEMBLE_SHIFT) for e in range(E) for s in counter[1]])
        else:  # the draws of `enhance_long_ensemble` on every input alone, input by input: (E * C_i, 1, T_i) per step, x0 first,
            # each written straight into its member-major slice of the library's (n_steps, E * C, T_pad_max) tensor
            noise = draw_noise(self.tot_ds, pk.entries(rngs), n_steps, E, device=self.device)
        members = torch.empty(E, C, l_max, dtype=torch.float32, device=self.device)
        res, mems = unpack_rows(pk, self._segments_run(plan, pk.batch, n_steps, epsilon, keep_rms, noise, counter, members), members)
        return (res, mems) if return_members else res

    def _segments_workspace(self, B, L, need):
        """The workspace of enhance_long: one buffer kept for re-use (outside the per-batch-size cache of `enhance`)."""
        cur = getattr(self, "_seg_ws", None)
        if cur is None or cur[0] != B or cur[1].numel() < need:
            self._seg_ws = None
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self._L.ou_workspace_init(self._handle, B, L, c_void_p(ws.data_ptr()), c_size_t(need),
                                                     self._stream()), self._handle)
            cur = self._seg_ws = (B, ws)
        self._adopt_workspace(cur[1], B, L)
        return cur[1]

    # ---- streaming enhance --------------------------------------------------------------------
    def stream(self, channels=1, segment_s: float = SEGMENT_S, overlap_s: float = OVERLAP_S, seed=0, n_steps=None, epsilon=None,
               keep_rms=False, warm_start=None, use_aux_signal=False, clip=False):
        """An `EnhanceStream`: push chunks of a live signal of `channels` rows, get finished audio back (ou_stream_*).  Every
        window of `segment_s` seconds is the `enhance` call on that excerpt alone, with no peak guard, on counter-based noise of
        key `seed` (row c: stream ids from c << 32 on, one per window); consecutive windows are crossfaded over `overlap_s`.
        A stream is NOT `enhance_long` in pieces: it has no whole-row normalisation, mel scale or peak guard, so its result
        differs from that call's; `clip=True` clamps the output to [-1, 1]."""
        n_steps, epsilon, segment, overlap = self._begin(n_steps, epsilon, segment_s, overlap_s)
        return EnhanceStream(self, int(channels), segment, overlap, int(seed), n_steps, epsilon, bool(keep_rms), warm_start,
                             bool(use_aux_signal), bool(clip))

    # ---- hipGraph replay of the hot path ------------------------------------------------------------------------
    def graphed_enhance(self, batch, length, n_steps=None, epsilon=None, keep_rms=False, serial=True):
        """-> callable `run(mix, rng=None)` equivalent to `enhance(mix, n_steps, epsilon, rng=rng, keep_rms=keep_rms)`
        for inputs of shape (batch, length): ONE `ou_enhance` (pad .. peak guard, ~430 launches over the caller's stream
        and three side streams) is captured into a hipGraph once and replayed per call -- the host then enqueues one
        graph launch instead of walking the network (the GPU timeline is the same back-to-back sequence either way).
        The noise is still drawn per call with `torch.randn(generator=rng)` in the reference's order, into the static
        buffer the graph reads, so a shared generator advances exactly as in the eager path.  The library call is
        capturable by construction: no allocation, no host synchronisation, GRU exchange tags advance on the device."""
        n_steps = self.diff_kwargs.n_steps if n_steps is None else int(n_steps)
        epsilon = self.diff_kwargs.epsilon if epsilon is None else float(epsilon)
        if not serial:
            # Measured (profiles/r05_final_hwq_probe.txt): with GPU_MAX_HW_QUEUES below 4 the HIP runtime
            # SEGFAULTS replaying a captured graph that has this call's four-stream fork / join structure (round 4 recorded it
            # as a hang of bench.py); the eager call and the serial-chain capture are fine with 1, 2 or 4 queues.
            import os

            hwq = os.environ.get("GPU_MAX_HW_QUEUES")
            if hwq is not None and hwq.strip().isdigit() and int(hwq) < 4:
                raise RuntimeError(f"graphed_enhance(serial=False) captures four streams; GPU_MAX_HW_QUEUES={hwq} makes the HIP "
                                   "runtime crash when such a graph is replayed -- use serial=True (the default)")
        B, mix_len = int(batch), int(length)
        T = padded(mix_len, self.tot_ds)
        dev = self.device
        s_mix = torch.zeros(B, 1, mix_len, dtype=torch.float32, device=dev)
        s_noise = torch.zeros(n_steps, B, 1, T, dtype=torch.float32, device=dev)
        s_out = torch.empty(B, 1, mix_len, dtype=torch.float32, device=dev)
        sigma = self.get_std_dev(torch.linspace(0, 1, n_steps).to(torch.float32).flip(dims=[0])).to(torch.float32).contiguous()
        # the graph's launches carry this buffer's address: a workspace of the graph's own, outside the per-batch-size cache
        # (an eager call with the same B and a longer T regrows the cached one)
        ws = self._private_workspace(B, T)
        self._adopt_workspace(ws, B, T)
        # serial=True: capture the call as ONE chain on the capture stream.  The eager path forks three side streams inside
        # the call (mel branch, st convs, first score-encoder pass); captured, every fork / join becomes a cross-stream edge
        # of the graph, and such a graph replays SLOWER than the chain (measured, profiles/).
        flags = (_lib.OU_ENH_KEEP_RMS if keep_rms else 0) | (_lib.OU_ENH_SERIAL if serial else 0)

        def launch():
            _lib.check(self._L.ou_enhance(
                self._handle, c_void_p(s_mix.data_ptr()), c_void_p(s_out.data_ptr()), c_void_p(s_noise.data_ptr()), B,
                mix_len, n_steps, epsilon, ctypes.cast(sigma.data_ptr(), ctypes.POINTER(c_float)), -1, flags,
                c_void_p(ws.data_ptr()), c_size_t(ws.numel()), self._stream()), self._handle)

        with torch.cuda.device(dev):
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                launch()  # warm-up outside the capture (first-touch work, kernel attribute setup)
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                launch()
        self._cond_key = (B, T)

        def run(mix, rng=None):
            self._poll_deferred_status()
            x = self._prep(mix).reshape(B, 1, mix_len)
            self._adopt_workspace(ws, B, T)  # (eager calls on any shape in between are fine: the graph owns its workspace)
            s_mix.copy_(x)
            for n in range(n_steps):  # draw order of the reference: x0, z_0 .. z_{N-2}
                s_noise[n].copy_(torch.randn((B, 1, T), dtype=torch.float32, device=dev, generator=rng))
            graph.replay()
            self._status()
            out = s_out.clone()
            if mix.ndim == 1:
                return out[0, 0]
            if mix.ndim == 2:
                return out[:, 0, :]
            return out

        run.graph = graph
        return run

    def _enhance_with_oracle_score(self, mix, target, n_steps, epsilon, fake_score_snr, rng, pad):
        """Diagnostic mode of the reference (universe.py:278-298): the network is bypassed by the analytic
        score of a known target, so no kernel of this library is involved -- plain device tensor glue."""
        tot = self.tot_ds
        level = 10 ** (self.spec.level_db / 20.0)
        norm, zero_mean, eps = self.spec.norm, self.spec.zero_mean, self.spec.norm_eps

        def stats(t):  # utils/norm.py:22-44, 65-71: the model's normalization_norm, zero_mean and eps
            mean = t.mean(dim=(1, 2), keepdim=True) if zero_mean else torch.zeros_like(t[:, :1, :1])
            d = t - mean
            if norm == "2":
                return mean, level / d.std(dim=(1, 2), keepdim=True).clamp(min=1e-5)
            peak = d.abs().amax(dim=(1, 2), keepdim=True)
            if norm == "max":
                return mean, level / peak.clamp(min=1e-5)
            return mean, torch.minimum(level / d.std(dim=(1, 2), keepdim=True).clamp(min=eps), 1.0 / peak.clamp(min=eps))

        def padded(t):
            return torch.nn.functional.pad(t, (pad // 2, pad - pad // 2))

        # utils/norm.py:47-87: ref == "both" normalises the target by its own statistics, "noisy" by the mixture's
        mixp, tgt = padded(mix), padded(self._prep(target))
        m_mean, m_gain = stats(mixp)
        t_mean, t_gain = stats(tgt) if self.normalization_kwargs["ref"] == "both" else (m_mean, m_gain)
        mixp = (mixp - m_mean) * m_gain
        tgt = (tgt - t_mean) * t_gain
        score_snr = 5.0 if fake_score_snr is None else fake_score_snr
        delta_t = 1.0 / (n_steps - 1)
        gamma = (self.diff_kwargs.sigma_max / self.diff_kwargs.sigma_min) ** -delta_t
        eta = 1 - gamma ** epsilon
        beta = math.sqrt(1 - gamma ** (2 * (epsilon - 1.0)))
        time = torch.linspace(0, 1, n_steps).type_as(mixp).flip(dims=[0])
        sigma = self.get_std_dev(time)
        sigma = torch.broadcast_to(sigma[None, :], (mixp.shape[0], sigma.shape[0]))

        def score_wrapper(x, s):
            true_score = -(x - tgt) / s[:, None, None] ** 2
            noise_rms = (true_score ** 2).mean().sqrt() * 10 ** (-score_snr / 20.0)
            nz = torch.randn(true_score.shape, dtype=true_score.dtype, device=true_score.device, generator=rng)
            return true_score + nz * noise_rms

        x = randn(mixp, sigma[:, 0], rng=rng)
        for n in range(n_steps - 1):
            s_now, s_next = sigma[:, n], sigma[:, n + 1]
            score = score_wrapper(x, s_now)
            z = randn(x, s_next, rng=rng)
            x = x + s_now[..., None, None] ** 2 * eta * score + beta * z
        x = x + sigma[:, -1, None, None] ** 2 * score_wrapper(x, sigma[:, -1])
        x = x[..., pad // 2: -(pad - pad // 2)]
        return torch.nn.functional.pad(x, (0, mix.shape[-1] - x.shape[-1]))


class EnhanceStream:
    """A streaming enhance session on a model (`Universe.stream`): `.push(chunk)` returns the samples that became final with
    that chunk (possibly none), `.flush()` the rest, after which the stream starts over at position 0.  `latency_samples` = the
    window length S: the worst-case delay between a sample's arrival and its emission.  Usable as a context manager; the
    session owns its workspace (its size depends on the channels and the window, not on how long the stream runs).  The model's
    handle is not re-entrant: a stream and other calls on the model take turns."""

    ROW_ID_SPACING = 1 << 32  # noise stream id of row c: c * 2^32, + k for window k

    def __init__(self, model, channels, segment, overlap, seed, n_steps, epsilon, keep_rms, warm_start, use_aux_signal, clip):
        self._model = model
        self._session = c_void_p()
        L = self._L = model._L
        self.channels = channels
        self._segment, self._overlap = segment, overlap
        need = c_size_t()
        _lib.check(L.ou_stream_workspace_bytes(model._handle, channels, segment, overlap, byref(need)), model._handle)
        # (zeroed: `flush` reads the status word in front of it, also of a stream that never ran a window)
        self._ws = torch.zeros(need.value, dtype=torch.uint8, device=model.device)
        sigma = model._sigma_table(n_steps)
        spec = _lib.StreamSpec()
        spec.C, spec.segment, spec.overlap = channels, segment, overlap
        spec.n_steps, spec.epsilon = int(n_steps), float(epsilon)
        spec.sigma_host = ctypes.cast(sigma.data_ptr(), ctypes.POINTER(c_float))
        spec.warm_start = -1 if warm_start is None else int(warm_start)
        spec.enh_flags = (_lib.OU_ENH_KEEP_RMS if keep_rms else 0) | (_lib.OU_ENH_USE_AUX_SIGNAL if use_aux_signal else 0)
        spec.stream_flags = _lib.OU_STREAM_CLIP if clip else 0
        spec.seed = seed
        spec.ids = (ctypes.c_uint64 * channels)(*[c * self.ROW_ID_SPACING for c in range(channels)])
        _lib.check(L.ou_stream_create(model._handle, byref(spec), c_void_p(self._ws.data_ptr()), c_size_t(need.value),
                                      byref(self._session)), model._handle)
        tot = model.tot_ds
        self.latency_samples = segment - segment % tot
        self._pushed = 0

    def _out(self, n, flat):
        return torch.empty((self.channels, n) if not flat else (n,), dtype=torch.float32, device=self._model.device)

    def _live(self):
        if not self._session.value:
            raise ValueError("this EnhanceStream is closed")

    @torch.no_grad()
    def push(self, chunk):
        """chunk: (n,) for one channel or (channels, n), on the model's device -> the (.., n_out) samples that are final now."""
        self._live()
        m = self._model
        flat = chunk.ndim == 1
        x = as_rows(chunk, "EnhanceStream.push", m._prep, "n")
        if x.shape[0] != self.channels:
            raise ValueError(f"EnhanceStream.push: {x.shape[0]} rows for a stream of {self.channels} channels")
        n = x.shape[1]
        tot = m.tot_ds
        cap = (_lib.stream_emitted(tot, self._pushed + n, self._segment, self._overlap)
               - _lib.stream_emitted(tot, self._pushed, self._segment, self._overlap))
        out = self._out(cap, False)
        n_out = ctypes.c_int64()
        with torch.cuda.device(m.device):
            _lib.check(self._L.ou_stream_push(self._session, c_void_p(x.data_ptr()) if n else None, x.stride(0), n,
                                              c_void_p(out.data_ptr()) if cap else None, max(out.stride(0), cap), cap,
                                              byref(n_out), m._stream()), m._handle)
        m._cond_key = None  # (the handle ran other windows since any ou_condition)
        self._pushed += n
        assert n_out.value == cap
        return out[0] if flat else out

    @torch.no_grad()
    def flush(self, flat=None):
        """The rest of the stream, (channels, n_out) -- `(n_out,)` for one channel unless flat=False --; the stream then starts
        over.  Waits for the device and raises if a kernel of the stream's calls flagged a timeout."""
        self._live()
        m = self._model
        cap = self._pushed - _lib.stream_emitted(m.tot_ds, self._pushed, self._segment, self._overlap)
        out = self._out(cap, False)
        n_out = ctypes.c_int64()
        with torch.cuda.device(m.device):
            _lib.check(self._L.ou_stream_flush(self._session, c_void_p(out.data_ptr()) if cap else None, max(out.stride(0), cap),
                                               cap, byref(n_out), m._stream()), m._handle)
            m._cond_key = None
            self._pushed = 0
            torch.cuda.current_stream(m.device).synchronize()
            _lib.check(self._L.ou_check_device_status(m._handle, c_void_p(self._ws.data_ptr())), m._handle)
        assert n_out.value == cap
        return out[0] if (self.channels == 1 if flat is None else flat) else out

    def close(self):
        if self._session.value:
            self._L.ou_stream_destroy(self._session)
            self._session = c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class UniverseGAN(Universe):
    """UNIVERSE++ (universe_gan.py:60): same inference surface; aux_to_wav goes through the decoupling layer."""


def ensemble_reduce(members, stat="median", lens=None, return_pick=False, out=None):
    """The library's ensemble reduce on its own (ou_ensemble_reduce; extension): members (E, B, S) float32 on a HIP device,
    member-major, unit stride along S and rows one common stride apart (a view into a wider (E * B, row_stride) buffer is
    fine) -> (B, S) mean / median / signal median over the members; `lens`: valid samples per input (the rest of `out` is 0).
    return_pick=True (signal_median): -> (out, picked member per input).  `out`: a (B, S) view with the members' row stride."""
    E, B, S = members.shape
    rs = members.stride(1)
    if members.dtype != torch.float32 or not members.is_cuda or members.stride(2) != 1 or members.stride(0) != B * rs:
        raise ValueError("ensemble_reduce: members must be a float32 device tensor (E, B, S) with rows one stride apart")
    if stat not in _lib.ENSEMBLE_STATS:
        raise NotImplementedError()
    L = _lib.load()
    if out is None:
        out = torch.empty((B, rs), dtype=torch.float32, device=members.device)[:, :S]
    if out.shape != (B, S) or out.stride(0) != rs or out.stride(1) != 1:
        raise ValueError("ensemble_reduce: out must be a (B, S) view with the members' row stride")
    nb = L.ou_ensemble_reduce_scratch_bytes(E, B)
    scratch = torch.empty(nb, dtype=torch.uint8, device=members.device)
    len_arr = None if lens is None else (ctypes.c_int64 * B)(*[int(v) for v in lens])
    with torch.cuda.device(members.device):
        _lib.check(L.ou_ensemble_reduce(c_void_p(members.data_ptr()), c_void_p(out.data_ptr()), E, B, rs, S, len_arr,
                                        _lib.ENSEMBLE_STATS[stat], c_void_p(scratch.data_ptr()), c_size_t(nb),
                                        c_void_p(torch.cuda.current_stream(members.device).cuda_stream)))
    if return_pick:
        pick = scratch[B * E * 4:(B * E + B) * 4].view(torch.int32).to(torch.int64) if stat == "signal_median" else None
        return out, pick
    return out


def signal_median(signal):
    """utils/stats.py:22-66 semantics without the sort: for every (batch entry, sample) the reference looks up, in the
    ascending order of the n ensemble members, the POSITION of the member whose index is nearest to n/2 (first hit in
    rank order on a tie), histograms those positions per batch entry and returns member number argmax(histogram).
    Here the position of member c is obtained by counting the members that precede it ("x_j < x_c", ties broken by
    member index like a stable sort), and the histogram is one bincount over (batch entry, position) pairs."""
    shape = signal.shape
    x = signal.flatten(start_dim=2)  # (n, B, S)
    n, B, S = x.shape
    dist = (torch.arange(n, dtype=torch.float64) - n / 2).abs()
    cands = [c for c in range(n) if float(dist[c]) == float(dist.min())]
    pos = None
    for c in cands:
        before = (x < x[c]).sum(dim=0)
        if c > 0:
            before = before + (x[:c] == x[c]).sum(dim=0)
        pos = before if pos is None else torch.minimum(pos, before)  # (B, S): rank position, smaller wins a tie
    rows = torch.arange(B, device=x.device)[:, None] * n
    hist = torch.bincount((rows + pos).flatten(), minlength=B * n).view(B, n)
    pick = hist.argmax(dim=1)  # first maximum, like the reference's counts.argmax
    out = x[pick, torch.arange(B, device=x.device)]
    return out.reshape(shape[1:])
