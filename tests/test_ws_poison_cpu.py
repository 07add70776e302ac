"""CPU: the coverage of the workspace-poison case table (tests/ws_poison.py).  A new ou_enhance* entry point, a new option set of
conv_fp64.FAMILIES or a new model kind without a poison case fails here."""
import conv_fp64 as CF
import norm_cases
import seqmodel_cases
import snake_cases
import ws_poison as W


def test_every_declared_entry_point_has_a_case():
    declared = W.declared_entry_points()
    assert "ou_enhance" in declared and "ou_enhance_segments_var_ensemble" in declared and len(declared) >= 7, declared
    driven = {fn for c in W.CASES for fn in c.fns}
    assert driven == set(declared), (sorted(set(declared) - driven), sorted(driven - set(declared)))


def test_every_entry_point_runs_on_every_zoo_model():
    for name in W.ZOO:
        driven = {fn for c in W.CASES if c.sect == "a" and c.model == ("zoo", name) for fn in c.fns}
        assert driven == set(W.declared_entry_points()), (name, driven)
        ids = {c.id for c in W.CASES if c.model == ("zoo", name)}
        for B in (1, 4):
            assert {f"a.plain.{name}.b{B}", f"a.keep_rms.{name}.b{B}", f"a.graph.{name}.b{B}"} <= ids
            for stat in ("mean", "median", "signal_median"):
                for share in (0, 1):
                    assert f"a.ens.{stat}.share{share}.{name}.b{B}" in ids
        for rows in ("rows", "mult"):
            assert f"a.var.{rows}.{name}" in ids and f"a.ens_var.{rows}.share0.{name}" in ids and f"a.ens_var.{rows}.share1.{name}" in ids
    for name in W.GAN:
        ids = {c.id for c in W.CASES}
        assert {f"a.warm.{name}.b1", f"a.aux.{name}.b4", f"a.seg.warm.{name}", f"a.seg_var.aux.{name}"} <= ids


def test_every_family_has_a_plain_and_a_ragged_case():
    for tag, (opts, want, batches, frames) in CF.FAMILIES.items():
        for name in CF.MODELS:
            if tag.startswith("fuse") and name != "PP16":
                continue
            plain = [c for c in W.CASES if c.family == tag and c.call == "plain" and c.model == ("zoo", name)]
            assert sorted(c.kw["B"] for c in plain) == sorted(batches), (tag, name)
            assert all(c.kw["frames"] == frames and c.opts == opts for c in plain), (tag, name)
            ragged = [c for c in W.CASES if c.family == tag and c.call == "var" and c.model == ("zoo", name)]
            assert sorted(c.opts["mask_fused"] for c in ragged) == [0, 1], (tag, name)
            assert all(dict(c.opts, mask_fused=None) == dict(opts, mask_fused=None) for c in ragged), (tag, name)
    assert {c.family for c in W.CASES if c.family} == set(CF.FAMILIES) | set(W.STEERING)
    for tag in W.STEERING:
        for name in CF.MODELS:
            calls = sorted(c.call for c in W.CASES if c.family == tag and c.model == ("zoo", name))
            assert calls == ["plain", "var", "var"], (tag, name, calls)
    chunked = [c for c in W.CASES if c.family == "gru_chunked"]
    assert all(c.opts["gru_bmax"] == 1 for c in chunked)
    assert all(c.kw.get("B") == 4 or len(W.row_sets(160)[c.kw["rows"]]) == 4 for c in chunked)


def test_every_model_kind_has_a_plain_and_a_ragged_case():
    kinds = [f"norm.{m}" for m in norm_cases.MODES] + [f"snake.{c}" for c in snake_cases.CASES]
    kinds += [f"seq.{c}" for c in seqmodel_cases.CASES] + ["off.r27", "off.odd_pp"]
    assert sorted(W.KINDS) == sorted(kinds)
    assert {"norm.max", "norm.2max", "norm.keepmean"} <= set(kinds)
    assert any(k.startswith("seq.sand") for k in kinds) and any(k.startswith("seq.none") for k in kinds)
    for k in kinds:
        calls = sorted(c.call for c in W.CASES if c.kind == k)
        assert calls == ["plain", "var"], (k, calls)
        W.spec_of(next(c.model for c in W.CASES if c.kind == k))  # (the configuration exists)


def test_the_table_itself():
    assert len({c.id for c in W.CASES}) == len(W.CASES)
    assert all(c.call in W.RUNNERS for c in W.CASES)
    # no case is spared `finite` or `zero`; what is spared `nan` is named with its reason
    for cid, (fills, why) in W.NAN_EXEMPT.items():
        assert cid in W.BY_ID and set(fills) == {"zero", "finite"} and len(why) > 20, cid
    assert len(W.ORDER_PAIRS) == 30 and len(set(W.ORDER_PAIRS)) == 30
    # the ragged row sets: the project's rows, and one row that is a multiple of tot_ds
    for td in (160, 240, 21):
        sets = W.row_sets(td)
        assert sets["rows"] == [f * td - 3 for f in CF.RAGGED_ROWS]
        assert any(n % td == 0 for n in sets["mult"]) and max(sets["mult"]) == max(sets["rows"])
        assert len({max(v) for v in sets.values()}) == 1  # (one padded length: the calls of (f) share a workspace)
    assert [W.padded(n, 160) for n in (157, 160, 1)] == [160, 320, 160]


def test_tap_names_are_the_fp64_tests():
    names, must = W.tap_names(W.spec_of(("zoo", "PP16s")))
    for n in ("mixn", "x", "wav", "cond.in", "score.in", "cond.c0", "cond.sc0", "score.enc0.up", "score.enc0.c1", "score.enc0.c2",
              "score.enc0.v", "score.enc0.h", "cond.aux"):
        assert n in names, n
    assert not any(n.endswith(".fir") for n in names)  # (the documented exception, rate_fp64.py)
    assert set(must) <= set(names)


def test_segmented_ragged_geometry_leaves_a_ragged_walk_in_the_taps():
    """The last group of the ragged segmented cases has rows of different lengths, and is as long as a full window: all groups
    of the call walk one length (tests/ws_poison.py, seg_geometry)."""
    import seg_fp64 as SG

    for td in (160, 240):
        Sg, Ov = SG.seg_so(td)
        for which, E in (("var", 1), ("var_ens", W.ENS)):
            lens, mb = W.seg_geometry(td, which)
            geos = [SG.Row(n, td, Sg, Ov) for n in lens]
            assert any(g.n_win > 1 for g in geos)  # a full row
            Bw, real, slots, n_groups, T = SG.last_group(geos, mb, True, E)
            ls = [geos[c].L for c, _ in slots]
            assert n_groups > 1 and T == Sg and min(ls) < max(ls), (which, td, ls)
