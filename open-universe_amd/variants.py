"""Variant codes -> kernel family names: the one Python decoder, over the library's table (csrc/ou_variants.h).

A variant code is what a conv launch answers with (the `cfg` of a profile record, `last_cfg` of bench_conv) and what a forced
`cfg` asks for.  The names are the finest partition anyone uses ("strided", "direct3s", "rate_down" and "rate_up" apart); coarser
users group names, nobody writes ranges."""
from . import _lib


def family_of(code):
    """Family name of a variant code; AssertionError for a code that names none."""
    name = _lib.load().ou_variant_family(int(code))
    assert name is not None, f"variant code {code} names no kernel family"
    return name.decode()


def is_recurrence_record(code):
    """Profile RECORDS from 1000 on are GRU passes of code - 1000 steps (kVarRecurrence), whatever family_of says about the same
    number as a forced cfg: 1000 .. 1099 reach conv_split_kernel there (the overlap ou_variants.h documents)."""
    return code >= 1000
