"""Variant codes are named once: csrc/ou_variants.h is the table, ou_variant_family reads it, open_universe_amd.variants.family_of
is the one Python decoder.  The expected names below are written out from the two decoders this replaced (tests/conv_fp64.py and
tests/rate_fp64.py before the table existed) -- not derived from the table."""
import json
import os
import re

from open_universe_amd import _lib, variants as V

_HERE = os.path.dirname(os.path.abspath(__file__))
# (42, 47, 91, 265, 320: rate_fp64's finer names; 1000 as a FORCED cfg reaches conv_split_kernel -- as a profile record it is a GRU pass)
EXPECTED = {0: "lds", 12: "lds", 42: "rate_down", 47: "rate_up", 61: "direct", 66: "direct2", 77: "direct2", 91: "strided",
            133: "fused", 192: "fused", 203: "direct3", 265: "direct3s", 320: "direct4", 443: "direct2w", 485: "direct2w",
            523: "direct3w", 613: "direct4w", 723: "direct4w", 803: "split", 875: "split", 925: "split", 1000: "split"}
# the names rate_fp64_variants.json is keyed by, with a code of each
GOLDEN_NAMES = {"lds": 1, "direct": 72, "direct2": 76, "strided": 91, "direct3s": 262, "direct4": 322, "rate_down": 42, "rate_up": 47,
                "direct2w": 483, "direct3w": 523, "direct4w": 613}


def test_family_of_names_every_listed_code():
    for code, name in EXPECTED.items():
        assert V.family_of(code) == name, code
    with open(os.path.join(_HERE, "golden", "rate_fp64_variants.json")) as f:
        golden = json.load(f)
    names = {fam for case in golden.values() for fam in case}
    assert names and names <= set(GOLDEN_NAMES), names - set(GOLDEN_NAMES)
    for name in names:
        assert V.family_of(GOLDEN_NAMES[name]) == name


def test_no_family_for_minus_one():
    assert _lib.load().ou_variant_family(-1) is None
    assert V.is_recurrence_record(1000) and V.is_recurrence_record(1401) and not V.is_recurrence_record(925)


def test_table_is_sorted_and_disjoint_but_for_the_documented_overlaps():
    src = open(os.path.join(_HERE, "..", "open-universe_amd", "csrc", "ou_variants.h")).read()
    rows = [(int(lo), 2 ** 31 - 1 if hi == "INT_MAX" else int(hi), name)
            for lo, hi, name in re.findall(r'^\s*\{(\d+),\s*(\d+|INT_MAX),\s*"(\w+)"\},', src, re.M)]
    assert len(rows) >= 15 and rows == sorted(rows, key=lambda r: r[0]) and all(lo < hi for lo, hi, _ in rows)
    overlaps = [(a[2], b[2]) for i, a in enumerate(rows) for b in rows[i + 1:] if b[0] < a[1]]
    assert overlaps == [("direct4", "block3"), ("split", "recurrence")]
    # the function reads this table: first range that holds the code
    L = _lib.load()
    for code in range(-2, 1200):
        want = next((name for lo, hi, name in rows if lo <= code < hi), None)
        got = L.ou_variant_family(code)
        assert (got.decode() if got else None) == want, code
