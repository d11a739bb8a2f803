"""What the extension's checked host layer must go on accepting: the forms
its callers rely on (tests/test_ext_args.py covers what it refuses).  A
check that is too strict fails here, not somewhere inside the engine."""
import re

import numpy as np
import pytest
import torch

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif("not __import__('torch').cuda.is_available()",
                       reason="needs an MI355X"),
]

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
I64, I32, U8, F64 = torch.int64, torch.int32, torch.uint8, torch.float64


@pytest.fixture(scope="module")
def ext():
    from dampr_amd.ops import native
    return native.require()


@pytest.fixture(scope="module")
def oracle():
    from dampr_amd.gpu.backend import TorchOps
    return TorchOps()


@pytest.fixture(scope="module")
def hip():
    from dampr_amd.gpu.backend import HipOps
    return HipOps()


def z(n, dtype=I64):
    return torch.zeros(n, dtype=dtype, device=DEV)


def test_zero_rows_return_before_any_launch(ext):
    e, e32, e8, ef = z(0), z(0, I32), z(0, U8), z(0, F64)
    tab = [z(16), z(16)]
    tabs = tab + [z(16), z(16)]
    join = [z(16), z(17), z(1)]
    arena = [e8, z(1)]
    key_gt, str_eq = [0, 0, 0, 1, 0], [1, 3, 4, 2, 0]
    consts = z(2 * 8 * ext.sv_filter_max_const() // 8)
    assert ext.mark_counts(e8, 0).tolist() == [0]
    ext.mark_positions(e8, 0, z(1, I32), e32)
    ext.tfidf_count(e8, e32, e32, z(16), *tabs, 0, 0)
    ext.tfidf_count_docs(e8, *tabs, 0, z(16), z(4, I32), 0)
    ext.table_merge(e, e, *tab)
    ext.table_put(e, e, *tab)
    out_k, out_v, cursor = ext.table_extract(e, e, 0)
    assert out_k.numel() == 0 and cursor.tolist() == [0]
    assert ext.table_lookup(*tab, e).numel() == 0
    assert ext.idf(e, 3.0).numel() == 0
    ext.gather_tokens(e8, e, e, 0)
    sizes = ext.tsv_sizes(e, e, ef)
    ext.tsv_format(e8, e, e, e, ef, torch.cumsum(sizes, 0) - sizes, 0)
    assert ext.rs_digit_fold(e).tolist() == [-1, 0]
    assert ext.rs_hist(e, 0, 0).numel() == 0
    ext.rs_scatter(e, e32, e, 0, 0, z(0), z(0, I32))
    counts = ext.seg_count(e)
    ext.seg_reduce_fused(e, e, counts.to(I64), 0, z(0), z(0))
    ext.seg_reduce_fused(e, ef, counts.to(I64), 0, z(0), z(0, F64))
    ext.mp_merge(e, e32, e, e32, 1, z(0), z(0, I32))
    ext.hj_build(e, *join)
    counts = ext.hj_count(e, *join, 0)
    ext.hj_emit(e, *join, torch.cumsum(counts, 0) - counts, 0, 0, 0, 0)
    ext.varlen_gather(e8, e, e, z(1), z(0, U8))
    ext.sv_hash64(*arena, 1, z(0))
    ext.sv_adjacent_eq(*arena, e, e32, e8, z(1))
    ext.sv_lex_key(*arena, e32, 0, z(0))
    ext.sv_lex_refine(e, e, e8, z(0, U8))
    assert ext.filter_count(e, e, key_gt).numel() == 0
    ext.filter_scatter(e, e, key_gt, e, z(0), z(0))
    ext.set_build(e, z(16))
    assert ext.sv_filter_count(None, *arena, str_eq, consts).numel() == 0
    ext.sv_filter_scatter(e, *arena, key_gt + str_eq, consts, e, z(0), z(0),
                          z(0))
    ext.sv_set_build(e, z(16, I32))
    torch.cuda.synchronize()


def _span(ext):
    return ext.rs_span()


def _offset_view(t_cpu):
    """``t_cpu`` on the device as a contiguous view 3 entries into a larger
    buffer whose other entries are poison."""
    buf = torch.full((t_cpu.numel() + 5,), 77, dtype=t_cpu.dtype, device=DEV)
    view = buf[3:3 + t_cpu.numel()]
    view.copy_(t_cpu)
    assert view.storage_offset() == 3 and view.is_contiguous()
    return view


# one row, exactly one block, two blocks (RS_SPAN = SEG_SPAN = MP_TILE)
SIZES = ["1", "span", "span+1"]


def _n(ext, size):
    return {"1": 1, "span": _span(ext), "span+1": _span(ext) + 1}[size]


def _keys(n, seed, hi=1 << 62):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(-hi, hi, size=n, dtype=np.int64))


@pytest.mark.parametrize("size", SIZES)
def test_offset_views_sort(ext, oracle, size):
    from dampr_amd.gpu.relational import radix_sort_pairs
    n = _n(ext, size)
    keys = _keys(n, 1)
    payload = torch.arange(n, dtype=I32) * 3
    want_k, want_p = oracle.sort_pairs(keys, payload)
    kv, pv = _offset_view(keys), _offset_view(payload)
    got_k, got_p = radix_sort_pairs(kv, pv)
    assert torch.equal(got_k.cpu(), want_k)
    assert torch.equal(got_p.cpu(), want_p)
    assert torch.equal(kv.cpu(), keys) and torch.equal(pv.cpu(), payload)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("dtype", [I64, F64])
def test_offset_views_group_reduce(ext, oracle, size, dtype):
    from dampr_amd.gpu.relational import OP_SUM, group_reduce_sorted
    n = _n(ext, size)
    keys = torch.sort(_keys(n, 2, hi=40) ^ (-1 << 63)).values ^ (-1 << 63)
    vals = _keys(n, 3, hi=1000).to(dtype)       # f64 sums of ints are exact
    want_k, want_v = oracle.seg_reduce_sorted(keys, vals, "sum")
    got_k, got_v = group_reduce_sorted(_offset_view(keys),
                                       _offset_view(vals), OP_SUM)
    assert torch.equal(got_k.cpu(), want_k)
    assert torch.equal(got_v.cpu(), want_v)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("fkeys", [False, True])
def test_offset_views_merge(ext, hip, oracle, size, fkeys):
    n = _n(ext, size)
    runs = [_keys(n, 4), _keys(3, 5)]
    flip = (-1 << 63) if fkeys else 0           # fkeys merge as unsigned
    runs = [torch.sort(r ^ flip).values ^ flip for r in runs]
    want_k, want_p = oracle.merge_sorted_runs(runs, fkeys=fkeys)
    got_k, got_p = hip.merge_sorted_runs([_offset_view(r) for r in runs],
                                         fkeys=fkeys)
    assert torch.equal(got_k.cpu(), want_k)
    assert torch.equal(got_p.cpu(), want_p)


def _pairs(out_l, out_r):
    return sorted(zip(out_l.cpu().tolist(), out_r.cpu().tolist()))


# a 3-row build side against a 5-row probe that includes key 0
JOIN_R = torch.tensor([7, 0, 7], dtype=I64)
JOIN_L = torch.tensor([0, 7, 5, -3, 0], dtype=I64)


@pytest.mark.parametrize("how", ["inner", "left", "outer"])
def test_offset_views_join(oracle, how):
    from dampr_amd.gpu.relational import hash_join
    want = _pairs(*oracle.hash_join(JOIN_L, JOIN_R, how))
    got = _pairs(*hash_join(_offset_view(JOIN_L), _offset_view(JOIN_R), how))
    assert got == want and len(want) >= 4


@pytest.mark.parametrize("how", ["inner", "left", "outer"])
def test_strided_join_keys_are_normalised(oracle, how):
    from dampr_amd.gpu.relational import hash_join
    want = _pairs(*oracle.hash_join(JOIN_L, JOIN_R, how))
    left = torch.stack([JOIN_L, JOIN_L + 100], 1).to(DEV)[:, 0]
    right = torch.stack([JOIN_R, JOIN_R + 100], 1).to(DEV)[:, 0]
    assert not left.is_contiguous() and not right.is_contiguous()
    assert _pairs(*hash_join(left, right, how)) == want


def test_positions_on_a_small_text():
    """mark_counts hands back u32 counts and mark_positions takes i32
    offsets and an i32 result: both forms pass the u32 accessors."""
    from dampr_amd.gpu.tfidf import (MODE_NEWLINE, MODE_TOKEN_START,
                                     TfidfEngine)
    raw = (b"the quick brown fox\njumps over_the lazy dog 42 times\n\n"
           b"  and again, The END of it all; no newline at the end")[:100]
    assert len(raw) == 100
    text = torch.frombuffer(bytearray(raw), dtype=U8).to(DEV)
    eng = TfidfEngine(DEV, vocab_capacity=1 << 10,
                      fallback_seen_capacity=1 << 10)
    nl, n_nl = eng.positions(text, MODE_NEWLINE)
    assert nl.dtype == I32 and n_nl == raw.count(b"\n")
    assert nl.tolist() == [i for i, c in enumerate(raw) if c == 10]
    ts, n_tok = eng.positions(text, MODE_TOKEN_START)
    want = [m.start() for m in re.finditer(rb"\w+", raw, re.ASCII)]
    assert n_tok == len(want) and ts.tolist() == want
