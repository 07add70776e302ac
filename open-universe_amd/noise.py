"""
Counter-based sampler noise (extension; the reference draws its noise with `torch.randn` on the model's device).

The noise value of (seed, stream, draw, sample position) is a pure function -- DESIGN.md 4.10, include/ouniverse.h:

    z(seed, stream, draw, t)        standard normal, fp32 on the device

  * Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).  Key = (seed & 0xffffffff, seed >> 32).
    With the quad index q = t >> 2, the counter is
        c0 = q & 0xffffffff,   c1 = ((q >> 32) & 0xffff) | (draw << 16),   c2 = stream & 0xffffffff,   c3 = stream >> 32
    (q < 2^48, draw < 2^16).  One block (w0, w1, w2, w3) gives the four normals of the positions 4q .. 4q + 3.
  * word -> uniform in the open interval: u = ((w >> 8) + 0.5) * 2^-24.
  * Box-Muller on the two pairs: r = sqrt(-2 ln u(w0)), z(4q) = r cos(2 pi u(w1)), z(4q + 1) = r sin(2 pi u(w1)); the same with
    (w2, w3) for z(4q + 2), z(4q + 3).
  * draw: 0 = the initial draw (x0, or the warm-start noise), n + 1 = z_n of the ABSOLUTE step n.
  * t: position in the row's own padded signal.  stream: one 64-bit id per row, (utterance index << 16) | channel in this package.

So a file gets the same noise alone, as a row of a ragged batch, on a lane, on rank 3 of 8, or cut into windows, and nobody holds
a (n_steps, B, T) tensor of it: the library fills one step's plane at a time (ou_noise.hip).

`CounterNoise` is the value object the enhance entry points accept in place of a `torch.Generator`; `reference` is the same
function in numpy with fp64 arithmetic behind the integer part -- the yardstick of the tests, written from the definition above.
"""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MAX_DRAW = 1 << 16
MAX_POSITION = 1 << 50  # quad index < 2^48
CHANNEL_BITS = 16       # stream = (utterance index << 16) | channel
ENSEMBLE_SHIFT = 48     # ... | (ensemble member << 48)


class CounterNoise:
    """Noise source `z(seed, stream + row's own id, draw, t)` for `enhance(rng=...)`, `enhance_many(rngs=...)`, `enhance_long(rng=...)`,
    the lane pool and `distributed.enhance_sharded(noise="counter")`.

    `seed`: the 64-bit key.  `stream`: the utterance index of the input this object is handed to (an int < 2^32); channel c of
    that input draws from stream id `(stream << 16) | c`, member e of an `ensemble` from that id plus `e << 48`.  One object
    shared by the entries of `enhance_many` gives entry i the index `stream + i`.  Immutable and stateless: using it does not
    advance anything, and two calls with equal (seed, stream) see the same noise."""

    __slots__ = ("seed", "stream")

    def __init__(self, seed, stream=0):
        seed, stream = int(seed), int(stream)
        if not 0 <= seed < 1 << 64:
            raise ValueError("CounterNoise: seed must be in [0, 2^64)")
        if not 0 <= stream < 1 << 32:
            raise ValueError("CounterNoise: stream (the utterance index) must be in [0, 2^32)")
        object.__setattr__(self, "seed", seed)
        object.__setattr__(self, "stream", stream)

    def __setattr__(self, *_):
        raise AttributeError("CounterNoise is immutable")

    def __repr__(self):
        return f"CounterNoise(seed={self.seed}, stream={self.stream})"

    def __eq__(self, other):
        return isinstance(other, CounterNoise) and (self.seed, self.stream) == (other.seed, other.stream)

    def __hash__(self):
        return hash((self.seed, self.stream))

    def at(self, offset):
        """The source of the utterance `offset` entries further on."""
        return CounterNoise(self.seed, self.stream + int(offset))

    def stream_ids(self, channels, ensemble=None):
        """The 64-bit stream ids of the rows of ONE input with `channels` channels: channel c -> (stream << 16) | c; with
        `ensemble` = E the rows of member e (member-major, as `enhance` replicates the input) get `+ (e << 48)`."""
        channels = int(channels)
        if not 1 <= channels <= 1 << CHANNEL_BITS:
            raise ValueError(f"CounterNoise: 1 <= channels <= {1 << CHANNEL_BITS}")
        base = [(self.stream << CHANNEL_BITS) | c for c in range(channels)]
        if ensemble is None:
            return base
        if not 1 <= int(ensemble) <= 1 << (64 - ENSEMBLE_SHIFT):
            raise ValueError(f"CounterNoise: 1 <= ensemble <= {1 << (64 - ENSEMBLE_SHIFT)}")
        return [s + (e << ENSEMBLE_SHIFT) for e in range(int(ensemble)) for s in base]


def is_counter(rng):
    return isinstance(rng, CounterNoise)


def plan_streams(n_files, seed, indices=None):
    """The CLI's plan (`--noise counter`): file k of the sorted list is utterance k of key `seed`, whatever process, batch, lane
    or window it ends up in.  -> {k: CounterNoise(seed, k)} for `indices` (default: all of them)."""
    ks = range(int(n_files)) if indices is None else indices
    return {int(k): CounterNoise(seed, int(k)) for k in ks}


# ---- the function itself, in numpy (tests) --------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """The Philox4x32-10 block function.  counter: (..., 4) uint32, key: (..., 2) uint32 (broadcast) -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = k[..., 0], k[..., 1]
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for rnd in range(10):
        p0 = np.uint64(PHILOX_M0) * c0  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        if rnd < 9:
            k0 = (k0 + np.uint64(PHILOX_W0)) & mask
            k1 = (k1 + np.uint64(PHILOX_W1)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def reference(seed, stream, draw, t0, n):
    """z(seed, stream, draw, t) for t = t0 .. t0 + n - 1 as float64 (integer part exact, everything behind it in fp64)."""
    seed, stream, draw, t0, n = int(seed), int(stream), int(draw), int(t0), int(n)
    if not (0 <= seed < 1 << 64 and 0 <= stream < 1 << 64 and 0 <= draw < MAX_DRAW and t0 >= 0 and n >= 0
            and t0 + n <= MAX_POSITION):
        raise ValueError("noise.reference: argument out of range")
    if n == 0:
        return np.zeros(0, dtype=np.float64)
    q0, q1 = t0 >> 2, (t0 + n + 3) >> 2
    q = np.arange(q0, q1, dtype=np.uint64)
    ctr = np.empty((q.size, 4), dtype=np.uint64)
    ctr[:, 0] = q & np.uint64(0xFFFFFFFF)
    ctr[:, 1] = ((q >> np.uint64(32)) & np.uint64(0xFFFF)) | np.uint64(draw << 16)
    ctr[:, 2] = stream & 0xFFFFFFFF
    ctr[:, 3] = stream >> 32
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    u = ((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    z = np.empty((q.size, 4), dtype=np.float64)
    for p in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[:, p]))
        ang = 2.0 * np.pi * u[:, p + 1]
        z[:, p] = r * np.cos(ang)
        z[:, p + 1] = r * np.sin(ang)
    z = z.reshape(-1)
    lo = t0 - (q0 << 2)
    return z[lo:lo + n]
