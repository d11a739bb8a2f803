"""What the extension's host layer refuses, checked without a GPU.

Every wrapper takes its tensor arguments through the checked accessors of
ops/hip/host.h.  Here each wrapper is called with small, well-formed CPU
tensors in which ONE argument has ONE defect (wrong dtype, strided, one
entry short, a table that is no power of two) and must refuse with a
message that starts with that argument's parameter name.  Matching the name
is the point: without a GPU an unchecked wrapper raises too, but about the
missing device.  A form defect is reported before anything about devices,
which is what lets this run on CPU tensors; the well-formed call itself is
refused for being on the host, by name as well.
"""
import pytest
import torch

from dampr_amd.ops import native

I64, I32, U8, F64 = torch.int64, torch.int32, torch.uint8, torch.float64


@pytest.fixture(scope="module")
def ext():
    try:
        return native.get()
    except Exception as e:      # noqa: BLE001 - no toolchain on this machine
        pytest.skip("dampr_hip extension cannot be built here: {}".format(e))


def z(n, dtype=I64):
    return torch.zeros(n, dtype=dtype)


# text / arena columns shared by several wrappers
def _text():
    return ("text", z(40, U8))


def _tables():
    return [("cnt_keys", z(16)), ("cnt_vals", z(16)),
            ("dict_keys", z(16)), ("dict_vals", z(16))]


def _join_table(nxt=3):
    return [("t_keys", z(16)), ("t_head", z(17)), ("next", z(nxt))]


def _arena():
    return [("blob", z(20, U8)), ("offs", z(4))]       # 3 rows


KEY_GT = [0, 0, 0, 1, 0]         # key > 1 over i64
KEY_ISIN = [0, 0, 8, 3, 0]       # key isin a set of 3 non-zero members
STR_EQ = [1, 3, 4, 2, 0]         # value == a 2-byte constant
STR_ISIN = [1, 3, 8, 0, 0]       # value isin a string set
SVF_CONSTS = 2 * 8 * 8           # words of the string filter's constants


def _sv_set():
    # member blob, member offs (2 members), member hashes, slots, row hashes
    return [z(10, U8), z(3), z(2), z(16, I32), z(3)]


_TABLE_DEFECTS = {"cnt_keys": "dsp", "cnt_vals": "dsl",
                  "dict_keys": "dsp", "dict_vals": "dsl"}
_JOIN_DEFECTS = {"t_keys": "dsp", "t_head": "dsl"}

# wrapper -> (positional arguments as (name, value), {tensor argument:
# defects}).  d: wrong dtype, s: strided, l: one entry short (only where
# the host knows the length), p: not a power of two.
WRAPPERS = {
    "mark_counts": (lambda: [_text(), ("mode", 0)], {"text": "ds"}),
    "mark_positions": (
        lambda: [_text(), ("mode", 0), ("block_offsets", z(1, I32)),
                 ("out", z(4, I32))],
        {"text": "ds", "block_offsets": "dl", "out": "ds"}),
    "tfidf_count": (
        lambda: [_text(), ("nl_pos", z(4, I32)), ("tok_start", z(6, I32)),
                 ("seen_keys", z(16))] + _tables()
        + [("pos_base", 0), ("doc_base", 0)],
        dict(_TABLE_DEFECTS, text="ds", nl_pos="ds", tok_start="ds",
             seen_keys="dsp")),
    "tfidf_count_docs": (
        lambda: [_text()] + _tables()
        + [("pos_base", 0), ("fb_seen", z(16)), ("meta", z(3, I32)),
           ("ablate", 0)],
        dict(_TABLE_DEFECTS, text="ds", fb_seen="dsp", meta="dsl")),
    "table_merge": (
        lambda: [("in_keys", z(6)), ("in_vals", z(6)), ("keys", z(16)),
                 ("vals", z(16))],
        {"in_keys": "ds", "in_vals": "dsl", "keys": "dsp", "vals": "dsl"}),
    "table_put": (
        lambda: [("in_keys", z(6)), ("in_vals", z(6)), ("keys", z(16)),
                 ("vals", z(16))],
        {"in_keys": "ds", "in_vals": "dsl", "keys": "dsp", "vals": "dsl"}),
    "table_extract": (
        lambda: [("keys", z(16)), ("vals", z(16)), ("n_out", 3)],
        {"keys": "ds", "vals": "dsl"}),
    "table_lookup": (
        lambda: [("keys", z(16)), ("vals", z(16)), ("query", z(6))],
        {"keys": "dsp", "vals": "dsl", "query": "ds"}),
    "idf": (lambda: [("df", z(6)), ("total", 10.0)], {"df": "ds"}),
    "gather_tokens": (
        lambda: [_text(), ("packed", z(6)), ("offsets", z(6)),
                 ("total_bytes", 12)],
        {"text": "ds", "packed": "ds", "offsets": "dsl"}),
    "tsv_sizes": (
        lambda: [("lens", z(6)), ("df", z(6)), ("idf", z(6, F64))],
        {"lens": "ds", "df": "dsl", "idf": "dsl"}),
    "tsv_format": (
        lambda: [("blob", z(40, U8)), ("tok_off", z(6)), ("lens", z(6)),
                 ("df", z(6)), ("idf", z(6, F64)), ("row_off", z(6)),
                 ("total_bytes", 100)],
        {"blob": "ds", "tok_off": "dsl", "lens": "ds", "df": "dsl",
         "idf": "dsl", "row_off": "dsl"}),
    "rs_digit_fold": (lambda: [("keys", z(8))], {"keys": "ds"}),
    "rs_hist": (lambda: [("keys", z(8)), ("shift", 8), ("nblocks", 1)],
                {"keys": "ds"}),
    "rs_scatter": (
        lambda: [("keys", z(8)), ("payload", z(8, I32)),
                 ("scanned", z(256)), ("shift", 8), ("nblocks", 1),
                 ("out_k", z(8)), ("out_p", z(8, I32))],
        {"keys": "ds", "payload": "dsl", "scanned": "dsl", "out_k": "dsl",
         "out_p": "dsl"}),
    "seg_count": (lambda: [("keys", z(8))], {"keys": "ds"}),
    "seg_reduce_fused": (
        lambda: [("keys", z(8)), ("vals", z(8)), ("tile_base", z(1)),
                 ("op", 0), ("out_keys", z(3)), ("out_vals", z(3))],
        {"keys": "ds", "vals": "dsl", "tile_base": "dl", "out_keys": "dsl",
         "out_vals": "ds"}),
    "mp_merge": (
        lambda: [("ka", z(5)), ("pa", z(5, I32)), ("kb", z(3)),
                 ("pb", z(3, I32)), ("bias_signed", 1), ("out_k", z(8)),
                 ("out_p", z(8, I32))],
        {"ka": "ds", "pa": "dsl", "kb": "ds", "pb": "dsl", "out_k": "dsl",
         "out_p": "dsl"}),
    "hj_build": (
        lambda: [("keys_r", z(3))] + _join_table(),
        dict(_JOIN_DEFECTS, keys_r="ds", next="dsl")),
    "hj_count": (
        lambda: [("keys_l", z(5))] + _join_table() + [("left_outer", 0)],
        dict(_JOIN_DEFECTS, keys_l="ds", next="ds")),
    "hj_emit": (
        lambda: [("keys_l", z(5))] + _join_table()
        + [("offsets", z(5)), ("total", 4), ("left_outer", 0),
           ("track_matched", 0), ("nr", 3)],
        dict(_JOIN_DEFECTS, keys_l="ds", next="dsl", offsets="dsl")),
    "varlen_gather": (
        lambda: [("blob", z(40, U8)), ("src_off", z(4)), ("lens", z(4)),
                 ("new_offs", z(5)), ("out", z(20, U8))],
        {"blob": "ds", "src_off": "ds", "lens": "dsl", "new_offs": "dsl",
         "out": "ds"}),
    "sv_hash64": (
        lambda: _arena() + [("mask", 1), ("out", z(3))],
        {"blob": "ds", "offs": "ds", "out": "dsl"}),
    "sv_adjacent_eq": (
        lambda: _arena() + [("sorted_hash", z(3)), ("perm", z(3, I32)),
                            ("heads", z(3, U8)), ("n_mismatch", z(1))],
        {"blob": "ds", "offs": "ds", "sorted_hash": "dsl", "perm": "dsl",
         "heads": "dsl", "n_mismatch": "dl"}),
    "sv_lex_key": (
        lambda: _arena() + [("rows", z(2, I32)), ("d", 0), ("out", z(2))],
        {"blob": "ds", "offs": "ds", "rows": "ds", "out": "dsl"}),
    "sv_lex_refine": (
        lambda: [("grp_sorted", z(4)), ("key_sorted", z(4)),
                 ("heads", z(4, U8)), ("open", z(4, U8))],
        {"grp_sorted": "dsl", "key_sorted": "ds", "heads": "dsl",
         "open": "dsl"}),
    "filter_count": (
        lambda: [("keys", z(6)), ("vals", z(6)), ("prog", KEY_ISIN),
                 ("set_k", z(16))],
        {"keys": "ds", "vals": "dsl", "set_k": "dsp"}),
    "filter_scatter": (
        lambda: [("keys", z(6)), ("vals", z(6)), ("prog", KEY_ISIN),
                 ("block_off", z(1)), ("out_k", z(2)), ("out_v", z(2)),
                 ("set_k", z(16))],
        {"keys": "ds", "vals": "dsl", "block_off": "dl", "out_k": "ds",
         "out_v": "dsl", "set_k": "dsp"}),
    "set_build": (
        lambda: [("members", z(3)), ("table", z(16))],
        {"members": "ds", "table": "dsp"}),
    "sv_filter_count": (
        lambda: [("keys", z(3))] + _arena()
        + [("prog", KEY_ISIN + STR_ISIN), ("consts", z(SVF_CONSTS)),
           ("set_k", z(16)), ("sv_set", _sv_set())],
        {"keys": "dsl", "blob": "ds", "offs": "ds", "consts": "dsl",
         "set_k": "dsp", "sv_set[0]": "ds", "sv_set[1]": "ds",
         "sv_set[2]": "dsl", "sv_set[3]": "dsp", "sv_set[4]": "dsl"}),
    "sv_filter_scatter": (
        lambda: [("keys", z(3))] + _arena()
        + [("prog", KEY_GT + STR_EQ), ("consts", z(SVF_CONSTS)),
           ("block_off", z(1)), ("out_k", z(2)), ("out_src", z(2)),
           ("out_len", z(2))],
        {"keys": "dsl", "blob": "ds", "offs": "ds", "consts": "dsl",
         "block_off": "dl", "out_k": "ds", "out_src": "dsl",
         "out_len": "dsl"}),
    "sv_set_build": (
        lambda: [("hashes", z(3)), ("slots", z(16, I32))],
        {"hashes": "ds", "slots": "dsp"}),
}

# the entry points without a tensor argument
SCALAR_ONLY = {"rs_span", "tfidf_span_bytes", "filter_tile", "set_capacity",
               "sv_filter_tile", "sv_filter_max_const"}


def _spoil(t, defect):
    if defect == "d":       # i32 stands in for i64; i64 for i32, u8 and f64
        return t.to(I32 if t.dtype == I64 else I64)
    if defect == "s":       # same length, every other element of a buffer
        return torch.zeros(2 * t.numel(), dtype=t.dtype)[::2]
    if defect == "l":
        return t[:-1]
    assert defect == "p"
    return torch.zeros(t.numel() - 4, dtype=t.dtype)        # 16 -> 12


def _call(ext, name, args):
    return getattr(ext, name)(*[v for _n, v in args])


CASES = [(w, arg, d) for w, (_make, defects) in sorted(WRAPPERS.items())
         for arg, ds in sorted(defects.items()) for d in ds]


def test_every_export_is_covered(ext):
    exported = {n for n in dir(ext) if not n.startswith("_")}
    assert exported == set(WRAPPERS) | SCALAR_ONLY
    assert len(exported) == 38 and "seg_reduce" not in exported
    for name, (make, defects) in WRAPPERS.items():
        tensors = set()
        for arg, v in make():
            if torch.is_tensor(v):
                tensors.add(arg)
            elif isinstance(v, list) and v and torch.is_tensor(v[0]):
                tensors.update("{}[{}]".format(arg, i)
                               for i in range(len(v)))
        assert tensors == set(defects), name


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_well_formed_host_tensors_are_refused_as_host_tensors(ext, name):
    make, _defects = WRAPPERS[name]
    with pytest.raises(RuntimeError, match="expected a device tensor"):
        _call(ext, name, make())


@pytest.mark.parametrize("name,arg,defect", CASES)
def test_one_defect_is_refused_by_name(ext, name, arg, defect):
    make, _defects = WRAPPERS[name]
    args = make()
    base, _, idx = arg.partition("[")
    pos = [n for n, _v in args].index(base)
    if idx:                                  # an entry of a tensor list
        i = int(idx.rstrip("]"))
        args[pos][1][i] = _spoil(args[pos][1][i], defect)
    else:
        t = _spoil(args[pos][1], defect)
        assert defect != "s" or not t.is_contiguous()
        args[pos] = (base, t)
    with pytest.raises(RuntimeError) as e:
        _call(ext, name, args)
    msg = str(e.value)
    assert msg.startswith(arg), (name, arg, defect, msg.split("\n")[0])


@pytest.mark.parametrize("name,args,arg", [
    ("rs_hist", (z(8), 4, 1), "shift"),
    ("rs_hist", (z(8), 64, 1), "shift"),
    ("rs_hist", (z(8), 8, 2), "nblocks"),
    ("rs_scatter", (z(8), z(8, I32), z(512), 8, 2, z(8), z(8, I32)),
     "nblocks"),
    ("seg_reduce_fused", (z(8), z(8), z(1), 3, z(3), z(3)), "op"),
    ("seg_reduce_fused", (z(8), z(8, F64), z(1), 0, z(3), z(3)),
     "out_vals"),
    ("hj_emit", (z(5), z(16), z(17), z(3), z(5), -1, 0, 0, 3), "total"),
    ("gather_tokens", (z(40, U8), z(6), z(6), -1), "total_bytes"),
    ("tsv_format", (z(40, U8), z(6), z(6), z(6), z(6, F64), z(6), -1),
     "total_bytes"),
    ("table_extract", (z(16), z(16), -1), "n_out"),
])
def test_scalar_arguments_are_checked(ext, name, args, arg):
    with pytest.raises(RuntimeError) as e:
        getattr(ext, name)(*args)
    assert str(e.value).startswith(arg), str(e.value).split("\n")[0]
