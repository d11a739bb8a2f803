"""GPU-side tests of the row filter: HipOps.filter_rows (filter_count +
scan + filter_scatter, ops/hip/dampr_filter.hip) bit for bit and in order
against the TorchOps oracle, and filter pipelines on cuda:0 that never
take the host map.  Every shape is valid input."""
import collections

import numpy as np
import pytest
import torch

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif("not __import__('torch').cuda.is_available()",
                       reason="needs an MI355X"),
]

from dampr_amd import Dampr, funcs  # noqa: E402
from dampr_amd.gpu.backend import HipOps, TorchOps  # noqa: E402
from dampr_amd.gpu.relational import FILTER_TILE  # noqa: E402
from dampr_amd.gpu.stores import encode_f64_sortable  # noqa: E402

DEV = "cuda:0"
T = FILTER_TILE
_I64_MIN = -(1 << 63)
_I64_MAX = (1 << 63) - 1
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 5 * T + 17, (1 << 20) + 3]
OPS = ["gt", "ge", "lt", "le", "eq", "ne", "between"]


@pytest.fixture(scope="module")
def hip():
    return HipOps()


def check(hip, keys, vals, clauses):
    """HipOps on the device copies == TorchOps on the host columns: same
    rows, same order, same bits, same dtypes.  Returns rows kept."""
    want_k, want_v = TorchOps().filter_rows(keys, vals, clauses)
    got_k, got_v = hip.filter_rows(keys.to(DEV), vals.to(DEV), clauses)
    assert got_k.dtype == keys.dtype and got_v.dtype == vals.dtype
    assert got_k.device.type == "cuda" and got_v.device.type == "cuda"
    assert torch.equal(got_k.cpu(), want_k)
    assert torch.equal(got_v.cpu().view(torch.int64),
                       want_v.view(torch.int64))
    return want_k.numel()


def test_tile_constant(hip):
    assert hip.ext.filter_tile() == FILTER_TILE
    assert FILTER_TILE % 64 == 0


def _patterns(n, rng):
    """name -> bool[n]: which rows should pass."""
    i = np.arange(n)
    return {
        "all": np.ones(n, dtype=bool),
        "none": np.zeros(n, dtype=bool),
        "alternating": i % 2 == 0,
        "last_of_wave": i % 64 == 63,
        "p01": rng.random(n) < 0.01,
        "p50": rng.random(n) < 0.5,
        "p99": rng.random(n) < 0.99,
    }


@pytest.mark.parametrize("n", SIZES)
def test_selectivity_patterns(hip, n):
    """v > 0 over an i64 value column built to pass exactly the pattern's
    rows; random keys ride along."""
    rng = np.random.default_rng(1000 + n % 997)
    keys = torch.from_numpy(rng.integers(_I64_MIN, _I64_MAX, size=n,
                                         dtype=np.int64, endpoint=True))
    mag = rng.integers(1, 1 << 40, size=n, dtype=np.int64)
    for name, keep in _patterns(n, rng).items():
        vals = torch.from_numpy(np.where(keep, mag, -mag + 1))
        kept = check(hip, keys, vals, [(1, "i64", "gt", 0, 0)])
        assert kept == int(keep.sum()), name


def _i64_column(n, rng):
    special = np.array([_I64_MIN, _I64_MIN + 1, -1, 0, 1, _I64_MAX - 1,
                        _I64_MAX], dtype=np.int64)
    col = rng.integers(-5, 6, size=n, dtype=np.int64)
    col[rng.integers(0, n, size=n // 3)] = \
        special[rng.integers(0, special.size, size=n // 3)]
    return torch.from_numpy(col)


def _f64_column(n, rng):
    special = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, 5e-324,
                        -5e-324, 2.2250738585072014e-308, 1.5, -1.5])
    col = rng.integers(-4, 5, size=n).astype(np.float64) / 2.0
    col[rng.integers(0, n, size=n // 2)] = \
        special[rng.integers(0, special.size, size=n // 2)]
    return torch.from_numpy(col)


@pytest.mark.parametrize("op", OPS)
def test_i64_domain_bounds(hip, op):
    rng = np.random.default_rng(11)
    n = 5 * T + 17
    keys = _i64_column(n, rng)
    vals = _i64_column(n, rng)
    for a, b in ((_I64_MIN, _I64_MAX), (_I64_MAX, _I64_MIN), (0, 1),
                 (_I64_MIN + 1, _I64_MAX - 1)):
        check(hip, keys, vals, [(1, "i64", op, a, b)])
        check(hip, keys, vals, [(0, "i64", op, a, b)])


@pytest.mark.parametrize("op", OPS)
def test_f64_domain_specials(hip, op):
    rng = np.random.default_rng(12)
    n = 5 * T + 17
    keys = torch.arange(n, dtype=torch.int64)
    vals = _f64_column(n, rng)
    for a, b in ((0.0, 1.5), (-0.0, float("inf")), (float("nan"), 0.0),
                 (float("-inf"), 5e-324), (5e-324, float("nan")),
                 (-5e-324, 0.0)):
        check(hip, keys, vals, [(1, "f64", op, a, b)])


@pytest.mark.parametrize("op", OPS)
def test_fkey_domain_matches_f64(hip, op):
    """An encoded key column filters exactly as the doubles it encodes."""
    rng = np.random.default_rng(13)
    n = 5 * T + 17
    doubles = _f64_column(n, rng)
    keys = encode_f64_sortable(doubles)
    vals = torch.arange(n, dtype=torch.int64)
    for a, b in ((0.0, 1.5), (-0.0, float("inf")), (float("nan"), 0.0),
                 (float("-inf"), 5e-324), (-1.5, -5e-324)):
        kept = check(hip, keys, vals, [(0, "fkey", op, a, b)])
        _k, as_f64 = TorchOps().filter_rows(vals, doubles,
                                            [(1, "f64", op, a, b)])
        assert kept == as_f64.numel()


def test_clause_programs(hip):
    rng = np.random.default_rng(14)
    n = 5 * T + 17
    ikeys, ivals = _i64_column(n, rng), _i64_column(n, rng)
    fvals = _f64_column(n, rng)
    fkeys = encode_f64_sortable(_f64_column(n, rng))
    one = [(0, "i64", "ne", 0, 0)]
    two = [(0, "i64", "ge", -3, 0), (1, "f64", "lt", 1.0, 0.0)]
    eight_if = [(0, "i64", "ge", -4, 0), (1, "f64", "le", 1.5, 0.0),
                (0, "i64", "ne", 2, 0), (1, "f64", "ne", -1.0, 0.0),
                (0, "i64", "between", -4, 4), (1, "f64", "ge", -2.0, 0.0),
                (0, "i64", "lt", 5, 0), (1, "f64", "between", -1.5, 1.5)]
    eight_fi = [(0, "fkey", "ge", -2.0, 0.0), (1, "i64", "le", 4, 0),
                (0, "fkey", "ne", 0.5, 0.0), (1, "i64", "ne", -2, 0),
                (0, "fkey", "between", -1.5, 2.0), (1, "i64", "gt", -5, 0),
                (0, "fkey", "lt", 2.0, 0.0), (1, "i64", "eq", 3, 0)]
    assert check(hip, ikeys, ivals, one) > 0
    assert check(hip, ikeys, fvals, two) > 0
    assert check(hip, ikeys, fvals, eight_if) > 0
    assert check(hip, fkeys, ivals, eight_fi) > 0
    with pytest.raises(ValueError):
        hip.filter_rows(ikeys.to(DEV), ivals.to(DEV), eight_if + one)


def test_views_at_a_storage_offset(hip):
    """Contiguous views at a non-zero storage offset are read in place;
    strided views are made contiguous by the wrapper."""
    rng = np.random.default_rng(15)
    n = T + 70
    kbase, vbase = _i64_column(n, rng).to(DEV), _f64_column(n, rng).to(DEV)
    clauses = [(1, "f64", "ge", 0.0, 0.0), (0, "i64", "le", 3, 0)]
    for ks, vs in ((kbase[3:], vbase[3:]), (kbase[1:-2], vbase[3:]),
                   (kbase[::2], vbase[1::2])):
        assert ks.numel() == vs.numel()
        want_k, want_v = TorchOps().filter_rows(ks.cpu(), vs.cpu(), clauses)
        got_k, got_v = hip.filter_rows(ks, vs, clauses)
        assert want_k.numel() > 0
        assert torch.equal(got_k.cpu(), want_k)
        assert torch.equal(got_v.cpu().view(torch.int64),
                           want_v.view(torch.int64))


def test_row_count_guard_precedes_any_launch(hip):
    big = torch.empty(1 << 31, dtype=torch.int64, device="meta")
    with pytest.raises(OverflowError):
        hip.filter_rows(big, big, [(0, "i64", "gt", 0, 0)])


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


def test_pipeline_between_count(no_host_map):
    rng = np.random.default_rng(21)
    vals = rng.integers(-500, 500, size=200_000)
    runner, out = _run(
        Dampr.columns(vals).filter(funcs.between(-100, 250.5)).count(),
        "filter_between_count")
    kept = vals[(vals >= -100) & (vals <= 250)]
    uniq, counts = np.unique(kept, return_counts=True)
    got = {k: v[1] for k, v in out.read()}
    assert got == dict(zip(uniq.tolist(), counts.tolist()))
    assert runner.stats["filter_rows_in"] == vals.size
    assert runner.stats["filter_rows_kept"] == kept.size


def test_pipeline_wordcount_at_least_k(no_host_map):
    rng = np.random.default_rng(22)
    words = ["w{}".format(int(z) % 3000) for z in rng.zipf(1.3, size=50_000)]
    runner, out = _run(
        Dampr.columns(words).count().filter(funcs.ge(5, on=funcs.snd)),
        "filter_wordcount")
    wc = collections.Counter(words)
    want = {w: c for w, c in wc.items() if c >= 5}
    assert want and len(want) < len(wc)
    assert {k: v[1] for k, v in out.read()} == want
    assert runner.stats["filter_rows_in"] == len(wc)
    assert runner.stats["filter_rows_kept"] == len(want)


def test_pipeline_filter_sort_f64(no_host_map):
    rng = np.random.default_rng(23)
    vals = rng.standard_normal(100_000)
    vals[::1000] = np.nan
    vals[1::1000] = -0.0
    runner, out = _run(Dampr.columns(vals).filter(funcs.ge(0)).sort_by(),
                       "filter_sort_f64")
    want = np.sort(vals[vals >= 0])
    got = np.array([v for _k, v in out.read()])
    assert got.size == want.size
    assert np.array_equal(got, want)
    assert runner.stats["filter_rows_kept"] == want.size
