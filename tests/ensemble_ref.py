"""Torch restatement of the library's ensemble reduce (csrc/ou_ensemble.hip; ou_ensemble_reduce in include/ouniverse.h), for the
tests.  members: (E, B, S) -- member-major as everywhere -- `lens`: valid samples per input or None.  Rank counting, as the
kernel does it:  rank(c) = #{j : x_j < x_c} + #{j < c : x_j == x_c}  (the stable ascending order)."""
import torch

STATS = ("mean", "median", "signal_median")


def ranks(x):
    """(E, B, S) -> integer ranks of the same shape (a permutation of 0 .. E - 1 along dim 0)."""
    E = x.shape[0]
    out = []
    for c in range(E):
        r = (x < x[c]).sum(dim=0)
        if c:
            r = r + (x[:c] == x[c]).sum(dim=0)
        out.append(r)
    return torch.stack(out)


def candidates(E):
    """Members whose index is nearest E / 2: one for even E, both neighbours for odd E."""
    return [E // 2] if E % 2 == 0 else ([0] if E == 1 else [(E - 1) // 2, (E + 1) // 2])


def reduce_ref(members, stat, lens=None):
    """-> (out (B, S) float32 with 0 from lens[b] on, pick (B,) int64 or None, hist (B, E) or None)."""
    x = members.to(torch.float32)
    E, B, S = x.shape
    lens = [S] * B if lens is None else [int(v) for v in lens]
    valid = torch.arange(S)[None, :] < torch.tensor(lens)[:, None]  # (B, S)
    pick = hist = None
    if stat == "mean":
        s = x[0].clone()
        for e in range(1, E):  # sequential fp32 sum in member order, then one division
            s = s + x[e]
        out = s / torch.tensor(float(E), dtype=torch.float32)
    elif stat == "median":
        r = ranks(x)
        out = torch.zeros(B, S)
        for c in range(E):
            out = torch.where(r[c] == (E - 1) // 2, x[c], out)
    elif stat == "signal_median":
        r = ranks(x)
        pos = None
        for c in candidates(E):
            pos = r[c] if pos is None else torch.minimum(pos, r[c])
        hist = torch.zeros(B, E, dtype=torch.int64)
        for b in range(B):
            hist[b] = torch.bincount(pos[b, :lens[b]], minlength=E)
        pick = torch.tensor([int((hist[b] == hist[b].max()).nonzero()[0]) for b in range(B)])  # first maximum
        out = x[pick, torch.arange(B)]
    else:
        raise NotImplementedError(stat)
    return torch.where(valid, out, torch.zeros(())), pick, hist


def mean_bound(members, mean):
    """Per-sample bound of a sequential fp32 sum plus one division against the float64 mean:
    (E - 1) 2^-24 sum_e |x_e| + 2^-24 |mean|."""
    E = members.shape[0]
    return (E - 1) * 2.0 ** -24 * members.double().abs().sum(dim=0) + 2.0 ** -24 * mean.double().abs()


def draw_members(E, B, S, seed, ties=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(E, B, S, generator=g)
    if ties:
        x = torch.round(x * 8) / 8  # quantised to 1/8: ties occur
    return x
