"""GPU-side tests of the set membership filter: HipOps.filter_rows and
sv_filter_rows with isin / notin clauses (set_build / sv_set_build and the
probe in ops/hip/dampr_filter.hip, dampr_strfilter.hip, set_table.h) bit
for bit and in order against the TorchOps oracle, and isin pipelines on
cuda:0 that never take the host map.  Every shape is valid input."""
import collections

import numpy as np
import pytest
import torch

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif("not __import__('torch').cuda.is_available()",
                       reason="needs an MI355X"),
]

from dampr_amd import Dampr, funcs, keyhash  # noqa: E402
from dampr_amd.gpu import filters, relational  # noqa: E402
from dampr_amd.gpu.backend import HipOps, TorchOps  # noqa: E402
from dampr_amd.gpu.relational import FILTER_TILE  # noqa: E402
from dampr_amd.gpu.stores import StrTable, encode_f64_sortable  # noqa: E402
from dampr_amd.gpu.strvals import StrVals  # noqa: E402

DEV = "cuda:0"
T = FILTER_TILE
_I64_MIN = -(1 << 63)
_I64_MAX = (1 << 63) - 1
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 5 * T + 17]
SET_SIZES = [1, 2, 8, 9, 1000, 100_003]
ORDERS = ["strided", "consecutive", "random"]


@pytest.fixture(scope="module")
def hip():
    return HipOps()


def bits(x):
    return filters._f64_bits(x)


def check(hip, keys, vals, clauses, compiled=None):
    """HipOps on the device copies == TorchOps on the host columns: same
    rows, same order, same bits, same dtypes.  Returns rows kept."""
    want_k, want_v = TorchOps().filter_rows(keys, vals, clauses)
    got_k, got_v = hip.filter_rows(keys.to(DEV), vals.to(DEV),
                                   clauses if compiled is None else compiled)
    assert got_k.dtype == keys.dtype and got_v.dtype == vals.dtype
    assert got_k.device.type == "cuda" and got_v.device.type == "cuda"
    assert torch.equal(got_k.cpu(), want_k)
    assert torch.equal(got_v.cpu().view(torch.int64),
                       want_v.view(torch.int64))
    return want_k.numel()


def test_set_capacity_is_the_extensions(hip):
    for m in (0, 1, 8, 9, 1000):
        assert hip.ext.set_capacity(m) == filters.set_capacity(m)


# -- numeric sets ------------------------------------------------------------

def _i64_members(m, order, rng):
    if order == "strided":                  # share their 20 low bits
        return (np.arange(m, dtype=np.int64) - m // 2) << 20
    if order == "consecutive":
        return np.arange(m, dtype=np.int64) - m // 3
    out = np.unique(rng.integers(_I64_MIN, _I64_MAX, size=2 * m + 8,
                                 dtype=np.int64, endpoint=True))
    return rng.permutation(out)[:m]


def _column_around(members, n, rng):
    """n words, about half of them members, the rest near misses: a
    member with one bit flipped or moved by one, and zeros."""
    pick = members[rng.integers(0, members.size, size=n)]
    kind = rng.integers(0, 6, size=n)
    bit = np.int64(1) << rng.integers(0, 63, size=n).astype(np.int64)
    col = np.where(kind < 3, pick,
                   np.where(kind == 3, pick ^ bit,
                            np.where(kind == 4, pick + 1, 0)))
    return torch.from_numpy(col.astype(np.int64))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("m", SET_SIZES)
def test_i64_sets(hip, m, order):
    rng = np.random.default_rng(31 * m + len(order))
    members = _i64_members(m, order, rng)
    assert np.unique(members).size == m
    mt = torch.from_numpy(members)
    n_max = SIZES[-1]
    col = _column_around(members, n_max, rng)
    other = torch.from_numpy(rng.integers(-9, 9, size=n_max))
    for c in (0, 1):
        for op in ("isin", "notin"):
            clauses = [(c, "i64", op, mt, None)]
            compiled = hip.filter_compile(clauses, "numeric", DEV)
            for n in SIZES:
                k, v = (col, other) if c == 0 else (other, col)
                kept = check(hip, k[:n], v[:n], clauses, compiled)
                if n >= 64:
                    assert 0 < kept < n


def test_i64_special_members(hip):
    rng = np.random.default_rng(41)
    special = np.array([0, 1, -1, _I64_MIN, _I64_MAX, _I64_MIN + 1,
                        _I64_MAX - 1, 2, -2], dtype=np.int64)
    n = 5 * T + 17
    col = torch.from_numpy(special[rng.integers(0, special.size, size=n)])
    other = torch.arange(n, dtype=torch.int64)
    for present in ([0, 1, -1, _I64_MIN, _I64_MAX], [0], [1, -1],
                    [_I64_MIN], [_I64_MAX, 2], [_I64_MIN + 1, -2, 7]):
        mt = torch.tensor(present, dtype=torch.int64)
        for op in ("isin", "notin"):
            kept = check(hip, col, other, [(0, "i64", op, mt, None)])
            assert 0 < kept < n
            check(hip, other, col, [(1, "i64", op, mt, None)])


_F64_SPECIAL = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, 5e-324,
                         -5e-324, 2.2250738585072014e-308, 1.5, -1.5])


def _f64_column(n, rng):
    col = rng.integers(-40, 41, size=n).astype(np.float64) / 8.0
    col[rng.integers(0, n, size=n // 2)] = \
        _F64_SPECIAL[rng.integers(0, _F64_SPECIAL.size, size=n // 2)]
    return torch.from_numpy(col)


def _f64_members(values):
    """Members as the contract wants them: double bits, -0.0 as 0.0."""
    return torch.tensor(sorted({bits(float(x) + 0.0) for x in values}),
                        dtype=torch.int64)


@pytest.mark.parametrize("m", SET_SIZES)
def test_f64_and_fkey_sets(hip, m):
    rng = np.random.default_rng(51 + m)
    n_max = SIZES[-1]
    doubles = _f64_column(n_max, rng)
    ids = torch.arange(n_max, dtype=torch.int64)
    fill = (rng.permutation(4 * m + 64)[:m] - 2 * m) / 8.0
    with_zero = [0.0, np.inf, 5e-324, -1.5] + fill.tolist()
    no_zero = [-np.inf, -5e-324, 2.2250738585072014e-308] + \
        [x for x in fill.tolist() if x != 0.0]
    for values in (with_zero[:max(m, 1)], no_zero[:max(m, 1)]):
        mt = _f64_members(values)
        for op in ("isin", "notin"):
            vclause = [(1, "f64", op, mt, None)]
            kclause = [(0, "fkey", op, mt, None)]
            vcomp = hip.filter_compile(vclause, "numeric", DEV)
            kcomp = hip.filter_compile(kclause, "numeric", DEV)
            for n in SIZES:
                kept = check(hip, ids[:n], doubles[:n], vclause, vcomp)
                as_key = check(hip, encode_f64_sortable(doubles[:n]),
                               ids[:n], kclause, kcomp)
                assert as_key == kept
    # the rows the contract names, one by one
    rows = torch.tensor([np.nan, -0.0, 0.0, 5e-324, -5e-324, np.inf, 1.0],
                        dtype=torch.float64)
    ids = torch.arange(rows.numel())
    mt = _f64_members([-0.0, 5e-324, np.inf])
    got_k, _v = hip.filter_rows(ids.to(DEV), rows.to(DEV),
                                [(1, "f64", "isin", mt, None)])
    assert got_k.tolist() == [1, 2, 3, 5]
    got_k, _v = hip.filter_rows(ids.to(DEV), rows.to(DEV),
                                [(1, "f64", "notin", mt, None)])
    assert got_k.tolist() == [0, 4, 6]          # NaN is never a member


def test_table_past_one_l2(hip):
    """300_000 members: a table of 2**20 words, 8 MiB."""
    rng = np.random.default_rng(61)
    m, n = 300_000, (1 << 20) + 3
    assert filters.set_capacity(m) * 8 == 8 << 20
    members = _i64_members(m, "random", rng)
    col = _column_around(members, n, rng)
    other = torch.arange(n, dtype=torch.int64)
    mt = torch.from_numpy(members)
    kept = check(hip, other, col, [(1, "i64", "isin", mt, None)])
    assert n // 4 < kept < 3 * n // 4
    assert check(hip, col, other, [(0, "i64", "notin", mt, None)]) == n - kept


def test_programs_with_two_sets(hip):
    rng = np.random.default_rng(71)
    n = 5 * T + 17
    ikeys = torch.from_numpy(rng.integers(-50, 50, size=n))
    fvals = _f64_column(n, rng)
    kset = torch.tensor(sorted(set(range(-40, 45, 3)) | {0}))
    vset = _f64_members([0.0, 1.5, -1.5, 0.25, 0.5, -2.0, np.inf, 5e-324])
    eight = [(0, "i64", "ge", -45, 0), (1, "f64", "notin", vset, None),
             (0, "i64", "ne", 2, 0), (1, "f64", "ne", -1.0, 0.0),
             (0, "i64", "isin", kset, None), (1, "f64", "ge", -4.0, 0.0),
             (0, "i64", "lt", 44, 0), (1, "f64", "between", -4.5, 4.5)]
    kept = check(hip, ikeys, fvals, eight)
    assert 0 < kept < n
    fkeys = encode_f64_sortable(_f64_column(n, rng))
    ivals = torch.from_numpy(rng.integers(-50, 50, size=n))
    eight = [(0, "fkey", "isin", vset, None), (1, "i64", "le", 44, 0),
             (0, "fkey", "ne", 0.5, 0.0), (1, "i64", "ne", -2, 0),
             (0, "fkey", "between", -1.5, 2.0), (1, "i64", "gt", -45, 0),
             (1, "i64", "notin", kset, None), (1, "i64", "ne", 3, 0)]
    kept = check(hip, fkeys, ivals, eight)
    assert 0 < kept < n
    with pytest.raises(ValueError):
        hip.filter_rows(ikeys.to(DEV), fvals.to(DEV),
                        eight[:1] + [(0, "fkey", "notin", vset, None)])
    with pytest.raises(ValueError):
        hip.filter_rows(ikeys.to(DEV), ivals.to(DEV),
                        [(1, "f64", "isin", vset, None)])


def test_views_at_a_storage_offset(hip):
    rng = np.random.default_rng(72)
    n = T + 70
    kbase = torch.from_numpy(rng.integers(-50, 50, size=n)).to(DEV)
    vbase = _f64_column(n, rng).to(DEV)
    clauses = [(1, "f64", "notin", _f64_members([0.0, 1.5, np.inf]), None),
               (0, "i64", "isin", torch.arange(-30, 30, 2), None)]
    for ks, vs in ((kbase[3:], vbase[3:]), (kbase[1:-2], vbase[3:]),
                   (kbase[::2], vbase[1::2])):
        assert ks.numel() == vs.numel()
        want_k, want_v = TorchOps().filter_rows(ks.cpu(), vs.cpu(), clauses)
        got_k, got_v = hip.filter_rows(ks, vs, clauses)
        assert want_k.numel() > 0
        assert torch.equal(got_k.cpu(), want_k)
        assert torch.equal(got_v.cpu().view(torch.int64),
                           want_v.view(torch.int64))


def test_a_full_table_ends_the_probe(hip):
    """A table without an empty slot (no legal build makes one) gives an
    answer after ``capacity`` steps."""
    n = T + 5
    keys = torch.arange(n, dtype=torch.int64, device=DEV) % 11
    table = torch.full((16,), 7, dtype=torch.int64, device=DEV)
    prog = filters.filter_program(
        [(0, "i64", "isin", torch.tensor([7]), None)])
    counts = hip.ext.filter_count(keys, keys, prog, table, None)
    assert int(counts.sum()) == int((keys == 7).sum())


# -- string sets -------------------------------------------------------------

def host_sv(rows):
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(np.fromiter((len(r) for r in rows), dtype=np.int64,
                          count=len(rows)), out=offs[1:])
    blob = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    return StrVals(torch.from_numpy(blob), torch.from_numpy(offs))


def dev_sv(sv, shift):
    """``sv`` on the device with its blob a view ``shift`` bytes into a
    larger tensor (so its base is unaligned), the bytes around it set."""
    n = sv.blob.numel()
    big = torch.full((shift + n + 11,), 0xAA, dtype=torch.uint8, device=DEV)
    big[shift:shift + n] = sv.blob.to(DEV)
    return StrVals(big[shift:shift + n], sv.offs.to(DEV))


def sv_check(hip, keys, sv, clauses, compiled=None, shift=1):
    want_k, want_v = TorchOps().sv_filter_rows(keys, sv, clauses)
    got_k, got_v = hip.sv_filter_rows(
        keys.to(DEV), dev_sv(sv, shift),
        clauses if compiled is None else compiled)
    assert torch.equal(got_k.cpu(), want_k)
    assert torch.equal(got_v.offs.cpu(), want_v.offs)
    assert torch.equal(got_v.blob.cpu(), want_v.blob)
    assert int(got_v.offs[0]) == 0
    assert got_v.blob.numel() == int(got_v.offs[-1])
    return want_k.numel()


_LENS = [0, 1, 7, 8, 9, 15, 16, 17, 64, 65, 200]


def _pool(rng):
    """Candidate rows of every length in _LENS, several per length, plus
    the awkward neighbours of the members."""
    pool = []
    for ln in _LENS:
        for _ in range(4 if ln else 1):
            pool.append(bytes(rng.integers(97, 123, size=ln,
                                           dtype=np.uint8).tolist()))
    return pool


def _string_case(rng):
    pool = _pool(rng)
    long65 = pool[-6]
    long200 = pool[-1]
    assert len(long65) == 65 and len(long200) == 200
    members = [b"", b"ab", b"ab\0", b"abc", b"abcdefgh", b"abcdefghi",
               long65, long200] + pool[3::5]
    members = sorted(set(members))
    near = [b"a", b"ab\0\0", b"abd", b"abcdefg", b"abcdefgh\0", b"\0",
            long65[:64], long65[:64] + b"#", long200[:64] + b"?" * 136,
            long200[:199] + b"#", long200 + b"x"]
    rows = pool + near + members
    return members, rows


@pytest.mark.parametrize("n", SIZES)
def test_string_sets(hip, n):
    rng = np.random.default_rng(81)
    members, cand = _string_case(rng)
    assert b"" in members and b"ab" in members and b"ab\0" in members
    assert any(len(m) == 65 for m in members)
    assert any(len(m) == 200 for m in members)
    assert any(r not in members and r[:64] in {m[:64] for m in members}
               and len(r) > 64 for r in cand)
    rows = [cand[i] for i in rng.integers(0, len(cand), size=n)]
    if n:
        rows[0], rows[-1] = cand[-1], cand[5]   # the arena's edges, not b""
    sv = host_sv(rows)
    keys = torch.from_numpy(rng.integers(-5, 6, size=n))
    for op in ("isin", "notin"):
        clauses = [(1, "str", op, members, None)]
        kept = sv_check(hip, keys, sv, clauses, shift=1 + n % 5)
        if n >= 64:
            assert 0 < kept < n
        assert hip.sv_count_rows(dev_sv(sv, 3), clauses) == kept
    # beside comparison clauses and a key set
    kset = torch.tensor([-4, -1, 0, 2, 5])
    mixed = [(1, "str", "notin", members, None),
             (0, "i64", "isin", kset, None),
             (1, "str", "ge", b"ab", b""), (0, "i64", "ne", 2, 0)]
    sv_check(hip, keys, sv, mixed)


def test_string_sets_under_hash_collisions(hip):
    """hash_mask 0xF leaves 16 hash values for 100 members: chains as long
    as the table allows, and rows that share a member's hash without being
    one.  The oracle's bytes decide."""
    rng = np.random.default_rng(82)
    mask = 0xF
    words = sorted({bytes(rng.integers(97, 123, size=int(ln),
                                       dtype=np.uint8).tolist())
                    for ln in rng.integers(0, 24, size=400)})
    members, strangers = words[:100], words[100:]
    assert len(members) == 100 and len(strangers) > 100
    member_hashes = {keyhash.strmix64(m) & mask for m in members}
    assert any(keyhash.strmix64(s) & mask in member_hashes
               for s in strangers)
    n = 2 * T + 9
    rows = [words[i] for i in rng.integers(0, len(words), size=n)]
    sv = host_sv(rows)
    keys = torch.arange(n, dtype=torch.int64)
    for op in ("isin", "notin"):
        clauses = [(1, "str", op, members, None)]
        compiled = relational.filter_compile(clauses, "string", DEV,
                                             hash_mask=mask)
        assert compiled.sv_set.hash_mask == mask
        assert int(compiled.sv_set.hashes.max()) <= mask
        kept = sv_check(hip, keys, sv, clauses, compiled)
        assert 0 < kept < n


def test_string_table_ids_stay_on_device(hip):
    words = ["w{}".format(i) for i in range(500)] + ["", "w1" * 50]
    table = sorted(words, key=lambda s: s.encode("utf-8"))
    tbl = StrTable(StrVals.from_strings(table).to(DEV))
    members = [b"w7", b"", b"w499", b"nope", ("w1" * 50).encode(), b"w"]
    want = sorted(table.index(m.decode()) for m in members
                  if m.decode() in table)
    assert tbl.ids_of(members, hip) == want and len(want) == 4
    assert tbl.materialized is False


def test_row_count_guard_precedes_any_launch(hip):
    big = torch.empty(1 << 31, dtype=torch.int64, device="meta")
    with pytest.raises(OverflowError):
        hip.filter_rows(big, big,
                        [(0, "i64", "isin", torch.tensor([1]), None)])
    sv = StrVals(torch.empty(0, dtype=torch.uint8, device="meta"),
                 torch.empty((1 << 31) + 1, dtype=torch.int64,
                             device="meta"))
    with pytest.raises(OverflowError):
        hip.sv_filter_rows(big, sv, [(1, "str", "isin", [b"a"], None)])


# -- pipelines on cuda:0 -------------------------------------------------------

@pytest.fixture
def no_host_map(monkeypatch):
    from dampr_amd.gpu.engine import GpuRunner
    calls = []
    orig = GpuRunner._host_map

    def counting(self, stage, ins):
        calls.append(repr(stage))
        return orig(self, stage, ins)

    monkeypatch.setattr(GpuRunner, "_host_map", counting)
    yield calls
    assert calls == []


def _run(pm, name, **kw):
    from dampr_amd.gpu.engine import GpuRunner
    pm = pm.checkpoint()
    runner = GpuRunner(name, pm.pmer.graph, device=DEV, **kw)
    out = runner.run([pm.source])[0]
    return runner, out


def test_pipeline_isin_count(no_host_map):
    rng = np.random.default_rng(91)
    vals = rng.integers(-500, 500, size=200_000)
    members = set(range(-400, 400, 7)) | {2.5, 17.0, "x", 2 ** 70, True}
    runner, out = _run(
        Dampr.columns(vals).filter(funcs.isin(members)).count(),
        "isin_count")
    kept = [v for v in vals.tolist() if v in members]
    want = collections.Counter(kept)
    assert 0 < len(kept) < vals.size
    assert {k: v[1] for k, v in out.read()} == dict(want)
    assert runner.stats["filter_rows_in"] == vals.size
    assert runner.stats["filter_rows_kept"] == len(kept)


def _zipf_words(n, seed):
    rng = np.random.default_rng(seed)
    return ["w{}".format(int(z) % 3000) for z in rng.zipf(1.3, size=n)]


def test_pipeline_stop_words(no_host_map):
    words = _zipf_words(50_000, 92)
    stop = {"w{}".format(i) for i in range(1, 40)} | {"", "the", 3}
    runner, out = _run(
        Dampr.columns(words).filter(funcs.notin(stop)).count(),
        "isin_stop_words")
    want = collections.Counter(w for w in words if w not in stop)
    assert want and sum(want.values()) < len(words)
    assert {k: v[1] for k, v in out.read()} == dict(want)
    assert runner.stats["filter_rows_in"] == len(words)
    assert runner.stats["filter_rows_kept"] == sum(want.values())


def test_pipeline_wordcount_isin_keys(no_host_map):
    words = _zipf_words(50_000, 93)
    wanted = {"w{}".format(i) for i in range(0, 3000, 3)} | {"zz", 1.5}
    runner, out = _run(
        Dampr.columns(words).count().filter(funcs.isin(wanted,
                                                       on=funcs.fst)),
        "isin_wordcount")
    wc = collections.Counter(words)
    want = {w: c for w, c in wc.items() if w in wanted}
    assert want and len(want) < len(wc)
    assert isinstance(out.str_table, StrTable)
    assert out.str_table.materialized is False
    assert runner.stats["filter_rows_in"] == len(wc)
    assert runner.stats["filter_rows_kept"] == len(want)
    assert {k: v[1] for k, v in out.read()} == want


def test_pipeline_isin_sort_f64(no_host_map):
    rng = np.random.default_rng(94)
    vals = rng.integers(-80, 80, size=100_000) / 8.0
    vals[::1000] = np.nan
    vals[1::1000] = -0.0
    members = {0, 0.125, -2.5, 3, 2 ** 60 + 1, "a", float("inf")}
    runner, out = _run(
        Dampr.columns(vals).filter(funcs.isin(members)).sort_by(),
        "isin_sort_f64")
    want = np.sort(np.array([v for v in vals.tolist() if v in members]))
    got = np.array([v for _k, v in out.read()])
    assert 0 < want.size < vals.size
    assert got.size == want.size
    assert np.array_equal(got, want)
    assert runner.stats["filter_rows_kept"] == want.size
