"""CPU: the pieces the enhance methods of Universe are arranged from -- `draw_noise` (every generator draw of those methods) and
`pack_rows` / `unpack_rows` -- on CPU tensors with CPU generators, against the loops they replaced written out naively here.
Smallest shapes that can go wrong: tot_ds 4; entries of 1, 2 and 1 channels; lengths 3 (shorter than a block), 16 (an exact
multiple: gets a whole extra block) and 9 (one past a multiple); 3 planes; ensembles of 1 and 3 members."""
import pytest
import torch

from open_universe_amd.universe import draw_noise, pack_rows, padded, unpack_rows

TOT = 4
CHANS = [1, 2, 1]
LENS = [3, 4 * TOT, 2 * TOT + 1]
N = 3
SENTINEL = -77.0


def gens(shared, seed=11):
    """-> (what a caller hands over: one generator per entry or ONE, the distinct generators among them)."""
    if shared:
        g = torch.Generator("cpu").manual_seed(seed)
        return g, [g]
    gs = [torch.Generator("cpu").manual_seed(seed + i) for i in range(len(CHANS))]
    return gs, gs


def entries(rngs):
    return [(c, n, rngs[i] if isinstance(rngs, list) else rngs) for i, (c, n) in enumerate(zip(CHANS, LENS))]


def naive(rngs, E):
    """The loop of enhance_many(ensemble=E) as it was spelled: per entry, per plane, a (E * C, 1, T_i) temporary scattered
    member-major into the zero-filled (n, E * B, 1, T) tensor."""
    B, T = sum(CHANS), max(n + (TOT - n % TOT) for n in LENS)
    exp = torch.zeros(N, E * B, 1, T)
    r0 = 0
    for i, (C, n) in enumerate(zip(CHANS, LENS)):
        g = rngs[i] if isinstance(rngs, list) else rngs
        Ti = n + (TOT - n % TOT)
        for k in range(N):
            d = torch.randn((E * C, 1, Ti), dtype=torch.float32, generator=g)
            exp[k].view(E, B, 1, T)[:, r0:r0 + C, :, :Ti] = d.view(E, C, 1, Ti)
        r0 += C
    return exp


def test_padded_length():
    assert [padded(n, TOT) for n in LENS] == [4, 20, 12]  # a multiple gets a whole block more, as `Universe.pad` gives it


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("E", [1, 3])
def test_planes_and_generator_state_are_those_of_the_serial_loop(E, shared):
    rngs, distinct = gens(shared)
    ref_rngs, ref_distinct = gens(shared)
    exp = naive(ref_rngs, E)
    got = draw_noise(TOT, entries(rngs), N, E, device="cpu")
    assert got.shape == (N, E * sum(CHANS), 1, 20) and got.dtype == torch.float32
    assert torch.equal(got, exp)
    # member-major: member e of entry i sits in rows e * B + r_i .., and what no draw covers is zero
    B = sum(CHANS)
    for e in range(E):
        assert not got[:, e * B, :, 4:].any() and got[:, e * B, :, :4].all()       # entry 0: T_0 = 4
        assert got[:, e * B + 1:e * B + 3].all()                                   # entry 1 is the longest: no zero
        assert not got[:, e * B + 3, :, 12:].any() and got[:, e * B + 3, :, :12].all()
    for g, r in zip(distinct, ref_distinct):
        assert torch.equal(g.get_state(), r.get_state())
    # draw and discard (advance_generator_like_enhance) ends where placing ends ...
    adv, adv_distinct = gens(shared)
    assert draw_noise(TOT, entries(adv), N, E, device="cpu", discard=True) is None
    for g, r in zip(adv_distinct, ref_distinct):
        assert torch.equal(g.get_state(), r.get_state())
    if shared:  # ... which for ONE generator is after E * C_i rows per entry, in entry order
        serial = torch.Generator("cpu").manual_seed(11)
        for C, n in zip(CHANS, LENS):
            for _ in range(N):
                torch.randn((E * C, 1, padded(n, TOT)), generator=serial)
        assert torch.equal(distinct[0].get_state(), serial.get_state())


def test_planes_handed_in_keep_their_zeros():
    """A caller's own (n, rows, T) tensor (the 3-D planes of enhance_long_many): filled in place, the same elements."""
    rngs, _ = gens(True)
    ref_rngs, _ = gens(True)
    mine = torch.zeros(N, sum(CHANS), 20)
    assert draw_noise(TOT, entries(rngs), N, planes=mine) is mine
    assert torch.equal(mine, naive(ref_rngs, 1)[:, :, 0])


@pytest.mark.parametrize("rows, E", [(1, 1), (3, 1), (2, 3)])
def test_one_entry_is_the_whole_plane(rows, E):
    """`enhance`, `enhance_ensemble`, `draw_noise_like_enhance`: n draws of (E * rows, 1, T) with `out=` into the planes."""
    L = 2 * TOT + 1
    T = padded(L, TOT)
    g, ref = torch.Generator("cpu").manual_seed(5), torch.Generator("cpu").manual_seed(5)
    planes = torch.full((N, E * rows, 1, T), SENTINEL)
    got = draw_noise(TOT, [(rows, L, g)], N, E, planes=planes)
    assert got is planes and not (planes == SENTINEL).any()
    exp = torch.empty(N, E * rows, 1, T)
    for k in range(N):
        torch.randn((E * rows, 1, T), generator=ref, out=exp[k])
    assert torch.equal(planes, exp)
    assert torch.equal(g.get_state(), ref.get_state())
    # made by the routine itself: the same tensor, and as (n, rows, T) what draw_noise_like_enhance hands out
    again = draw_noise(TOT, [(rows, L, torch.Generator("cpu").manual_seed(5))], N, E, device="cpu")
    assert again.shape == (N, E * rows, 1, T) and torch.equal(again, exp)
    assert again[:, :, 0].is_contiguous()


@pytest.mark.parametrize("E", [None, 3])
def test_pack_then_unpack_is_the_identity(E):
    sigs = [torch.arange(1.0, 4.0), torch.arange(1.0, 33.0).view(2, 16), torch.arange(1.0, 10.0)[None, :],
            torch.arange(1.0, 10.0, dtype=torch.float64)]
    pk = pack_rows(sigs, "who", lambda x: x.to(torch.float32).contiguous())
    assert pk.dims == [1, 2, 2, 1] and pk.chans == [1, 2, 1, 1] and pk.lens == [3, 16, 9, 9]
    assert pk.row_lens == [3, 16, 16, 9, 9]
    assert pk.batch.shape == (5, 16) and pk.batch.dtype == torch.float32 and pk.batch.is_contiguous()
    assert not pk.batch[0, 3:].any() and not pk.batch[3:, 9:].any()  # right-padded with zeros
    g = object()
    assert pk.entries(g) == [(1, 3, g), (2, 16, g), (1, 9, g), (1, 9, g)]
    assert pk.entries([0, 1, 2, 3], own_length=False) == [(1, 16, 0), (2, 16, 1), (1, 16, 2), (1, 16, 3)]
    members = None if E is None else torch.stack([(e + 1) * pk.batch for e in range(E)])
    for lift in (lambda t: t, lambda t: t.unsqueeze(-2)):  # (rows, L) of the segmented calls, (rows, 1, L) of the others
        res, mems = unpack_rows(pk, lift(pk.batch), None if E is None else lift(members))
        assert len(res) == len(sigs) and len(mems) == (0 if E is None else len(sigs))
        for i, (s, o) in enumerate(zip(sigs, res)):
            assert o.shape == s.shape and torch.equal(o, s.to(torch.float32))
            if E is not None:
                assert mems[i].shape == (E,) + s.shape
                assert all(torch.equal(mems[i][e], (e + 1) * s.to(torch.float32)) for e in range(E))
    with pytest.raises(ValueError, match=r"who takes \(L,\) or \(C, L\) signals"):
        pack_rows([torch.zeros(1, 1, 4)], "who", lambda x: x)
    with pytest.raises(ValueError, match="who: empty input signal"):
        pack_rows([torch.zeros(4), torch.zeros(0)], "who", lambda x: x)
