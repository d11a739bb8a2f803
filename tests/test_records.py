"""The host record <-> column format (gpu/records.py): what layout a list
of records gets, what ranks agree on, what the columns hold and that they
decode back.  Pure host logic: no kernel, no process group."""
import itertools

import pytest
import torch

from dampr_amd.gpu.engine import GpuRunner
from dampr_amd.gpu.records import (Layout, agree, build, classify, decode,
                                   decode_text)
from dampr_amd.gpu.stores import HostStore, decode_f64_sortable
from dampr_amd.runner import Graph

I64, F64 = torch.int64, torch.float64

# name -> (records, value dtype or "str", fkeys, keyed, str_table)
ROUND_TRIP = {
    "int_int": ([(3, 10), (1, 20), (2, -5)], I64, False, False, None),
    "int_mixed_vals": ([(1, 2), (2, 2.5), (3, -1)], F64, False, False, None),
    "float_keys": ([(1.5, 1), (-2.25, 2), (0.5, 3)], I64, True, False, None),
    "mixed_keys": ([(1, 1), (2.5, 2), (-3, 3)], I64, True, False, None),
    "str_keys": ([("b", 1), ("é", 2), ("a", 3), ("b", 4)], I64, False, False,
                 ("a", "b", "é")),
    "str_vals": ([(1, ""), (2, "héllo 世"), (3, "x")], "str", False, False,
                 None),
    "keyed_num": ([(1, (1, 10)), (2, (2, 20))], I64, False, True, None),
    "keyed_str": ([("a", ("a", "x")), ("b", ("b", "")), ("a", ("a", "ü"))],
                  "str", False, True, ("a", "b")),
    "i64_extremes": ([(-(1 << 63), 1), ((1 << 63) - 1, 2)], I64, False,
                     False, None),
    "zeros": ([(0.0, 1), (-0.0, 2), (1.5, 3)], I64, True, False, None),
}

NO_LAYOUT = {
    "bool_key": [(True, 1), (2, 2)],
    "bool_val": [(1, True), (2, 3)],
    "none_val": [(1, None), (2, 3)],
    "tuple_val": [(1, (2, 3)), (2, (2, 5))],
    "keyed_mixed": [(1, (1, "a")), (2, (2, 3))],
    "str_int_keys": [("a", 1), (2, 2)],
    "str_int_vals": [(1, "a"), (2, 2)],
    "tuple_key": [((1, 2), 3)],
}


@pytest.mark.parametrize("name", sorted(ROUND_TRIP))
def test_round_trip_and_metadata(name):
    recs, vdtype, want_fkeys, want_keyed, want_table = ROUND_TRIP[name]
    keys, vals, keyed, fkeys, table = build(
        recs, agree([classify(recs, True)]))
    assert keys.dtype == I64 and keys.numel() == len(recs)
    if vdtype == "str":
        assert vals.is_strvals
    else:
        assert vals.dtype == vdtype
    assert (fkeys, keyed, table) == (want_fkeys, want_keyed, want_table)
    got = list(decode(keys, vals, keyed, fkeys, table))
    assert got == recs
    # == does not tell 1 from 1.0, nor the value layouts apart
    want_types = [(float if fkeys else type(k),
                   float if vdtype == F64 else type(v[1] if keyed else v))
                  for k, v in recs]
    assert [(type(k), type(v[1] if keyed else v)) for k, v in got] \
        == want_types


def test_key_columns():
    def keys_of(name):
        recs = ROUND_TRIP[name][0]
        return build(recs, agree([classify(recs, True)]))[0]

    assert keys_of("int_int").tolist() == [3, 1, 2]
    assert keys_of("str_keys").tolist() == [1, 2, 0, 1]
    assert keys_of("i64_extremes").tolist() == [-(1 << 63), (1 << 63) - 1]
    # -0.0 and 0.0 are one key: one encoding, which decodes to +0.0
    zeros = keys_of("zeros")
    assert zeros[0] == zeros[1]
    back = decode_f64_sortable(zeros)
    assert back.tolist() == [0.0, 0.0, 1.5]
    assert not torch.signbit(back).any()
    # the encoding's unsigned order is the float order
    enc = keys_of("float_keys") ^ -(1 << 63)
    assert torch.argsort(enc).tolist() == [1, 2, 0]


def test_empty_records():
    keys, vals, keyed, fkeys, table = build([], agree([classify([], True)]))
    assert (keys.dtype, vals.dtype, keys.numel(), vals.numel()) \
        == (I64, I64, 0, 0)
    assert (keyed, fkeys, table) == (False, False, None)
    assert list(decode(keys, vals, keyed, fkeys, table)) == []


class _NeverRead(object):
    def __getitem__(self, i):
        raise AssertionError("the table was read")


def test_decode_leaves_the_table_alone_without_keys():
    empty = torch.zeros(0, dtype=I64)
    assert list(decode(empty, empty, str_table=_NeverRead())) == []


@pytest.mark.parametrize("name", sorted(NO_LAYOUT))
def test_no_columnar_layout(name):
    recs = NO_LAYOUT[name]
    assert agree([classify(recs, True)]) is None
    runner = GpuRunner("records-test", Graph(), device="cpu")
    store = runner._encode_or_host(list(recs))
    assert isinstance(store, HostStore) and list(store) == recs
    runner.pool.cleanup()


# -- agreement between ranks ------------------------------------------------

INTS = Layout("int", "int", False, None)
FLOATS = Layout("float", "float", False, None)
EMPTY = Layout("empty", "empty", None, None)
OBJ_KEYS = Layout("obj", "int", False, None)
OBJ_VALS = Layout("int", "obj", False, None)
KEYED = Layout("int", "int", True, None)
STR_A = Layout("str", "int", False, ("a", "c"))
STR_B = Layout("str", "int", False, ("b", "c"))
STR_VALS = Layout("int", "str", False, None)


@pytest.mark.parametrize("layouts, want", [
    ([INTS, EMPTY], INTS),
    ([EMPTY, EMPTY], INTS),                 # int keys, i64 values, not keyed
    ([EMPTY], INTS),
    ([INTS, FLOATS], FLOATS),
    ([INTS, Layout("float", "int", False, None)],
     Layout("float", "int", False, None)),  # key kinds [int, float]
    ([INTS, Layout("int", "float", False, None)],
     Layout("int", "float", False, None)),  # value kinds [int, float]
    ([STR_A, STR_B], Layout("str", "int", False, ("a", "b", "c"))),
    ([STR_A, EMPTY], STR_A),
    ([STR_A, INTS], None),                  # [str, int] keys
    ([STR_VALS, INTS], None),               # [str, int] values
    ([STR_VALS, EMPTY], STR_VALS),
    ([INTS, OBJ_KEYS, INTS], None),         # one obj anywhere
    ([INTS, EMPTY, OBJ_VALS], None),
    ([KEYED, INTS], None),                  # keyed on one rank only
    ([KEYED, EMPTY], KEYED),
    ([KEYED, KEYED], KEYED),
])
def test_agree_table(layouts, want):
    assert agree(layouts) == want


def test_string_ranks_share_the_union_table():
    a = [("pear", 1), ("apple", 2)]
    b = [("kiwi", 3), ("pear", 4), ("é", 5)]
    layout = agree([classify(a, False), classify(b, False)])
    assert layout.table == ("apple", "kiwi", "pear", "é")
    for recs in (a, b):
        keys, vals, keyed, fkeys, table = build(recs, layout)
        assert table == layout.table
        assert [table[i] for i in keys.tolist()] == [k for k, _ in recs]
        assert list(decode(keys, vals, keyed, fkeys, table)) == recs


def test_empty_rank_builds_the_agreed_columns():
    layout = agree([classify([], False), classify([(1.5, "x")], False)])
    keys, vals, keyed, fkeys, table = build([], layout)
    assert keys.numel() == 0 and vals.is_strvals and vals.numel() == 0
    assert (keyed, fkeys, table) == (False, True, None)


def test_int_rank_builds_float_columns_next_to_a_float_rank():
    a, b = [(1, 2), (3, 4)], [(0.5, 1.5)]
    layout = agree([classify(a, False), classify(b, False)])
    keys, vals, keyed, fkeys, table = build(a, layout)
    assert fkeys and vals.dtype == F64
    assert list(decode(keys, vals, keyed, fkeys, table)) \
        == [(1.0, 2.0), (3.0, 4.0)]


def test_keyed_string_values_need_the_flag():
    recs = [("a", ("a", "x")), ("b", ("b", "y"))]
    assert classify(recs, True) == Layout("str", "str", True, ("a", "b"))
    # more than one rank: the tuple values are objects, so host records
    local = classify(recs, False)
    assert local == Layout("str", "obj", False, ("a", "b"))
    assert agree([local]) is None
    assert agree([local, EMPTY]) is None


def test_classify_kinds():
    assert classify([], True) == EMPTY
    assert classify([(1, 2)], True) == INTS
    assert classify([(1, 2.0), (2.5, 3)], True) == FLOATS
    assert classify([(1, (1, 2))], False) == KEYED
    # a tuple value that does not repeat the key is an object
    assert classify([(1, (1, 2)), (2, (3, 4))], True) \
        == Layout("int", "obj", False, None)
    assert classify([(True, 1)], True).kkind == "obj"
    assert classify([(1, False)], True).vkind == "obj"


@pytest.mark.parametrize("three", [
    [INTS, FLOATS, EMPTY],
    [STR_A, STR_B, EMPTY],
    [STR_A, STR_B, Layout("str", "float", False, ("z",))],
    [KEYED, EMPTY, Layout("float", "int", True, None)],
    [KEYED, INTS, EMPTY],
    [STR_A, INTS, EMPTY],
    [INTS, OBJ_VALS, FLOATS],
    [EMPTY, EMPTY, EMPTY],
])
def test_agree_ignores_rank_order(three):
    results = [agree(list(p)) for p in itertools.permutations(three)]
    assert all(r == results[0] for r in results)


# -- text lines -------------------------------------------------------------

# recorded from GpuRunner._decode_store(TextSource(data)) before the line
# decoder moved to gpu/records.py
@pytest.mark.parametrize("data, want", [
    (b"", []),
    (b"a", [(0, "a")]),
    (b"a\n", [(0, "a")]),
    (b"a\n\nb", [(0, "a"), (2, ""), (3, "b")]),
    (b"\n", []),
    (b"\n\n", [(0, "")]),
    (b"a\n\n", [(0, "a")]),
    (b"x\r\ny\n", [(0, "x\r"), (3, "y")]),
    (b"ok\n\xff\xfe bad\nz", [(0, "ok"), (3, "�� bad"), (10, "z")]),
])
def test_decode_text(data, want):
    assert decode_text(data) == want
