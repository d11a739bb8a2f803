"""Recognized filter predicates (funcs.gt/ge/lt/le/eq/ne/between): host
behaviour, DSL lowering, and the device engine's filter stage run on the
CPU backend (TorchOps, the oracle the HIP kernels are tested against in
test_gpu_filter.py).  Everything is exact equality."""
import collections
import math

import numpy as np
import pytest
import torch

from dampr_amd import Dampr, funcs, settings
from dampr_amd.dampr import ValueEmitter
from dampr_amd.gpu.engine import GpuRunner
from dampr_amd.gpu.stores import decode_f64_sortable
from dampr_amd.runner import MTRunner


@pytest.fixture
def host_map_calls(monkeypatch):
    """Counts GpuRunner._host_map calls."""
    calls = []
    orig = GpuRunner._host_map

    def counting(self, stage, ins):
        calls.append(repr(stage))
        return orig(self, stage, ins)

    monkeypatch.setattr(GpuRunner, "_host_map", counting)
    return calls


@pytest.fixture
def no_host_map(host_map_calls):
    """As host_map_calls; asserts on exit that the test never took it."""
    yield host_map_calls
    assert host_map_calls == []


def zipf_words(n, vocab, seed):
    rng = np.random.default_rng(seed)
    return ["w{}".format(int(z) % vocab) for z in rng.zipf(1.3, size=n)]


def dev_run(pm, **kw):
    """Run on the device engine's CPU backend: (runner, values)."""
    pm = pm.checkpoint()
    runner = GpuRunner("filter_test", pm.pmer.graph, device="cpu", **kw)
    out = runner.run([pm.source])[0]
    return runner, ValueEmitter(out).read()


def host_run(pm):
    return pm.run(runner=MTRunner, n_maps=2, n_reducers=2).read()


# ------------------------------------------------------------ predicates

_LAMBDAS = {
    "gt": lambda c: lambda x: x > c,
    "ge": lambda c: lambda x: x >= c,
    "lt": lambda c: lambda x: x < c,
    "le": lambda c: lambda x: x <= c,
    "eq": lambda c: lambda x: x == c,
    "ne": lambda c: lambda x: x != c,
}
_SAMPLES = [-3, 0, 2, 3, 7, 2.5, -0.0, 0.0, 3.0, float("inf"),
            float("-inf"), float("nan"), True, 2 ** 70]


@pytest.mark.parametrize("name", sorted(_LAMBDAS))
@pytest.mark.parametrize("c", [3, 2.5, float("nan"), 0])
def test_predicate_is_the_lambda(name, c):
    pred = getattr(funcs, name)(c)
    lam = _LAMBDAS[name](c)
    for v in _SAMPLES:
        assert pred(v) is lam(v), (name, c, v)
    on_fst = getattr(funcs, name)(c, on=funcs.fst)
    on_snd = getattr(funcs, name)(c, on=funcs.snd)
    ident = getattr(funcs, name)(c, on=funcs.identity)
    for v in _SAMPLES:
        assert on_fst((v, "x")) is lam(v)
        assert on_snd(("x", v)) is lam(v)
        assert ident(v) is lam(v)


def test_between_is_inclusive():
    pred = funcs.between(-0.5, 3)
    for v in _SAMPLES:
        assert pred(v) is (-0.5 <= v <= 3), v
    assert funcs.between(1, 3, on=funcs.snd)(("k", 3)) is True
    assert funcs.between(1, 3, on=funcs.fst)((0, "v")) is False


def test_predicate_carries_its_clause():
    assert funcs.filter_clause(funcs.gt(3)) == ("identity", "gt", (3,))
    assert funcs.filter_clause(funcs.between(1, 2.5, on=funcs.snd)) == \
        ("snd", "between", (1, 2.5))
    assert funcs.filter_clause(funcs.eq(True, on=funcs.fst)) == \
        ("fst", "eq", (True,))
    assert funcs.filter_clause(lambda x: x > 3) is None
    # a constant the device cannot compare: a working host predicate,
    # never a device clause
    p = funcs.ge("m")
    assert p("n") is True and p("a") is False
    assert funcs.filter_clause(p) is None
    with pytest.raises(TypeError):
        funcs.gt(3, on=len)


def test_dsl_records_specs():
    vals = np.arange(10)
    pm = Dampr.columns(vals).filter(funcs.gt(3)).filter(funcs.lt(8))
    assert pm.agg_specs == [("filter_clause", ("identity", "gt", (3,))),
                            ("filter_clause", ("identity", "lt", (8,)))]
    stage = pm.checkpoint().pmer.graph.stages[-1]
    assert stage.options["device_map"] == (
        "filter", (("identity", "gt", (3,)), ("identity", "lt", (8,))))
    # a plain lambda records None, and one opaque map hides the chain
    pm = Dampr.columns(vals).filter(lambda x: x > 3)
    assert pm.agg_specs == [None]
    mixed = pm.filter(funcs.lt(8)).checkpoint().pmer.graph.stages[-1]
    assert "device_map" not in (mixed.options or {})
    # host graphs get no extra stage
    host = Dampr.memory(list(range(10)))
    assert len(host.filter(funcs.gt(3)).count().pmer.graph.stages) == \
        len(host.filter(lambda x: x > 3).count().pmer.graph.stages)


# ------------------------------------------------------------- pipelines

def _ints(n=600, seed=3):
    return np.random.default_rng(seed).integers(-40, 60, size=n)


def _floats(n=400, seed=4):
    # multiples of 1/8 in [-2, 2): per-key sums are exact in any order
    return np.random.default_rng(seed).integers(-16, 16, size=n) / 8.0


def _pipelines():
    """name -> (device pipeline, host pipeline with the equivalent
    lambdas, rows into the filter, rows it keeps)."""
    v = _ints()
    vl = v.tolist()
    words = zipf_words(800, 60, 5)
    wc = collections.Counter(words)
    f = _floats()
    fl = f.tolist()
    fsum = collections.Counter(fl)
    cols, mem = Dampr.columns, Dampr.memory
    return {
        "filter": (
            cols(v).filter(funcs.gt(3)),
            mem(vl).filter(lambda x: x > 3),
            len(vl), sum(x > 3 for x in vl)),
        "filter_filter": (
            cols(v).filter(funcs.ge(-5)).filter(funcs.lt(20)),
            mem(vl).filter(lambda x: x >= -5).filter(lambda x: x < 20),
            len(vl), sum(-5 <= x < 20 for x in vl)),
        "count": (
            cols(v).filter(funcs.ne(7)).count(),
            mem(vl).filter(lambda x: x != 7).count(),
            len(vl), sum(x != 7 for x in vl)),
        "sort_by": (
            cols(v).filter(funcs.between(-10, 30)).sort_by(),
            mem(vl).filter(lambda x: -10 <= x <= 30).sort_by(lambda x: x),
            len(vl), sum(-10 <= x <= 30 for x in vl)),
        "len": (
            cols(v).filter(funcs.le(50)).len(),
            mem(vl).filter(lambda x: x <= 50).len(),
            len(vl), sum(x <= 50 for x in vl)),
        "topk": (
            cols(v).filter(funcs.lt(40)).topk(3),
            mem(vl).filter(lambda x: x < 40).topk(3),
            len(vl), sum(x < 40 for x in vl)),
        "mean": (
            cols(v).filter(funcs.gt(0)).mean(),
            mem(vl).filter(lambda x: x > 0).mean(),
            len(vl), sum(x > 0 for x in vl)),
        "wordcount_ge": (
            cols(words).count().filter(funcs.ge(2, on=funcs.snd)),
            mem(words).count().filter(lambda wc: wc[1] >= 2),
            len(wc), sum(c >= 2 for c in wc.values())),
        "float_keys_fst": (
            cols(f, keys=f).a_group_by().sum()
            .filter(funcs.lt(0.5, on=funcs.fst)),
            mem(fl).a_group_by(lambda x: x).sum()
            .filter(lambda kv: kv[0] < 0.5),
            len(fsum), sum(k < 0.5 for k in fsum)),
    }


_NAMES = ["filter", "filter_filter", "count", "sort_by", "len", "topk",
          "mean", "wordcount_ge", "float_keys_fst"]


@pytest.mark.parametrize("name", _NAMES)
def test_pipeline_matches_host_and_stays_on_device(name, no_host_map):
    dev_pm, host_pm, rows_in, rows_kept = _pipelines()[name]
    runner, got = dev_run(dev_pm)
    want = host_run(host_pm)
    assert want, "vacuous case"
    assert sorted(got) == sorted(want)
    if name == "sort_by":
        assert got == sorted(got)
    assert runner.stats["filter_rows_in"] == rows_in
    assert runner.stats["filter_rows_kept"] == rows_kept


def test_sink_after_filter(no_host_map, tmp_path):
    v = _ints()
    path = str(tmp_path / "sunk")
    runner, _ = dev_run(Dampr.columns(v).filter(funcs.gt(3)).sink(path))
    with open(tmp_path / "sunk" / "part-0") as fh:
        lines = fh.read().split()
    assert sorted(lines) == sorted(str(x) for x in v.tolist() if x > 3)
    assert runner.stats["filter_rows_in"] == v.size


def test_public_run_picks_device_engine(no_host_map):
    v = _ints()
    got = Dampr.columns(v).filter(funcs.gt(0)).count().run(device="cpu")
    want = collections.Counter(x for x in v.tolist() if x > 0)
    assert dict(got.read()) == dict(want)


# ------------------------------------------------------ constant folding

@pytest.mark.parametrize("pred", [
    funcs.gt(2.5), funcs.ge(2.5), funcs.lt(2.5), funcs.le(2.5),
    funcs.eq(2.5), funcs.ne(2.5), funcs.eq(3.0), funcs.ne(3.0),
    funcs.gt(-2.5), funcs.le(-2.5), funcs.between(-0.5, 2.5),
    funcs.between(2.5, -0.5), funcs.gt(True), funcs.eq(False),
    funcs.le((1 << 63) - 1), funcs.ge(-(1 << 63)), funcs.gt((1 << 63) - 1),
], ids=repr)
def test_i64_constant_folding(pred, no_host_map):
    vals = [-4, -3, -2, -1, 0, 1, 2, 3, 4, (1 << 63) - 1, -(1 << 63),
            (1 << 53) + 1]
    _r, got = dev_run(Dampr.columns(np.array(vals, dtype=np.int64))
                      .filter(pred))
    assert got == [v for v in vals if pred(v)]


_F64_ROWS = [float("nan"), -0.0, 0.0, float("inf"), float("-inf"), 1.5,
             -1.5, 5e-324, -5e-324, 3.0]


@pytest.mark.parametrize("name", ["gt", "ge", "lt", "le", "eq", "ne"])
@pytest.mark.parametrize("c", [0.0, -0.0, float("inf"), float("nan"), 3,
                               1.5, True], ids=repr)
def test_f64_ops(name, c, no_host_map):
    pred = getattr(funcs, name)(c)
    _r, got = dev_run(Dampr.columns(np.array(_F64_ROWS)).filter(pred))
    assert [repr(x) for x in got] == \
        [repr(v) for v in _F64_ROWS if pred(v)]


@pytest.mark.parametrize("lo,hi", [(-0.0, 1.5), (float("-inf"), 0),
                                   (1, float("nan")), (2, 1)])
def test_f64_between(lo, hi, no_host_map):
    pred = funcs.between(lo, hi)
    _r, got = dev_run(Dampr.columns(np.array(_F64_ROWS)).filter(pred))
    assert [repr(x) for x in got] == \
        [repr(v) for v in _F64_ROWS if pred(v)]


# -------------------------------------------------------------- fallbacks

def test_fallback_string_table_key(host_map_calls):
    words = zipf_words(300, 20, 6)
    wc = collections.Counter(words)
    for pred in (funcs.ne(3, on=funcs.fst), funcs.eq(3, on=funcs.fst)):
        del host_map_calls[:]
        runner, got = dev_run(Dampr.columns(words).count().filter(pred))
        assert sorted(got) == sorted(kv for kv in wc.items() if pred(kv))
        assert len(host_map_calls) == 1
        assert runner.stats["filter_rows_in"] == 0
    # ordering a str against an int: the host's TypeError
    with pytest.raises(TypeError):
        dev_run(Dampr.columns(words).count()
                .filter(funcs.ge(3, on=funcs.fst)))


def test_fallback_varlen_values(host_map_calls):
    words = zipf_words(200, 20, 7)
    _r, got = dev_run(Dampr.columns(words).filter(funcs.ne(3)))
    assert got == words
    assert len(host_map_calls) == 1


def test_fallback_nan_constant_on_i64(host_map_calls):
    v = _ints(100)
    _r, got = dev_run(Dampr.columns(v).filter(funcs.gt(float("nan"))))
    assert got == []
    _r, got = dev_run(Dampr.columns(v).filter(funcs.ne(float("nan"))))
    assert got == v.tolist()
    _r, got = dev_run(Dampr.columns(v).filter(funcs.lt(1 << 63)))
    assert got == v.tolist()
    assert len(host_map_calls) == 3


def test_fallback_big_int_on_f64(host_map_calls):
    rows = [2.0 ** 60, 2.0 ** 61, -1.0, float("nan")]
    c = 2 ** 60 + 1
    _r, got = dev_run(Dampr.columns(np.array(rows)).filter(funcs.gt(c)))
    assert got == [2.0 ** 61]
    _r, got = dev_run(Dampr.columns(np.array(rows)).filter(funcs.le(c)))
    assert got == [2.0 ** 60, -1.0]
    assert len(host_map_calls) == 2


def test_fallback_wrong_selector(host_map_calls):
    v = _ints(50)
    with pytest.raises(TypeError):                # int is not subscriptable
        dev_run(Dampr.columns(v).filter(funcs.gt(3, on=funcs.snd)))
    # identity on keyed records compares the (key, value) tuple
    _r, got = dev_run(Dampr.columns(v).count().filter(funcs.ne(3)))
    assert sorted(got) == sorted(collections.Counter(v.tolist()).items())
    assert len(host_map_calls) == 2


def test_fallback_mixed_input_kinds(host_map_calls):
    """An int column concatenated with a string column has no common
    value layout: the records reach the filter as a HostStore."""
    v = _ints(40)
    words = zipf_words(40, 10, 8)
    _r, got = dev_run(Dampr.columns(v).concat(Dampr.columns(words))
                      .filter(funcs.ne(3)))
    want = [x for x in v.tolist() + words if x != 3]
    assert sorted(map(repr, got)) == sorted(map(repr, want))
    assert any("_filter" in c for c in host_map_calls)


# ------------------------------------------------ chaining, store layout

def test_nine_chained_filters(no_host_map):
    v = _ints(2000)
    preds = [funcs.gt(-30), funcs.lt(50), funcs.ne(0), funcs.ne(1),
             funcs.ge(-29.5), funcs.le(48.5), funcs.ne(17), funcs.ne(2.5),
             funcs.between(-28, 47)]
    pm = Dampr.columns(v)
    host = Dampr.memory(v.tolist())
    for p in preds:
        pm = pm.filter(p)
    for lam in (lambda x: x > -30, lambda x: x < 50, lambda x: x != 0,
                lambda x: x != 1, lambda x: x >= -29.5,
                lambda x: x <= 48.5, lambda x: x != 17,
                lambda x: x != 2.5, lambda x: -28 <= x <= 47):
        host = host.filter(lam)
    stage = pm.checkpoint().pmer.graph.stages[-1]
    assert len(stage.options["device_map"][1]) == 9
    runner, got = dev_run(pm)
    want = host_run(host)
    assert want and sorted(got) == sorted(want)
    assert got == [x for x in v.tolist() if all(p(x) for p in preds)]
    assert runner.stats["filter_rows_in"] == v.size
    assert runner.stats["filter_rows_kept"] == len(got)


@pytest.fixture
def filter_stores(monkeypatch):
    """Captures each _map_filter call's input and output layout."""
    seen = []
    orig = GpuRunner._map_filter

    def snap(store):
        return {"meta": (store.partitioned, store.keyed, store.fkeys,
                         store.str_table, store.vdtype),
                "runs": {p: [(r.sorted, r.keys.clone(), r.vals.clone())
                             for r in runs]
                         for p, runs in store.items()}}

    def capturing(self, stage, spec, ins):
        before = snap(ins[0])
        out = orig(self, stage, spec, ins)
        seen.append((before, snap(out)))
        return out

    monkeypatch.setitem(GpuRunner._MAP_HANDLERS, "filter", capturing)
    return seen


def test_store_metadata_fkeys(filter_stores, no_host_map):
    f = _floats()
    _r, got = dev_run(Dampr.columns(f).a_group_by().sum()
                      .filter(funcs.eq(0.25, on=funcs.fst)), n_partitions=4)
    assert got == [(0.25, 0.25 * f.tolist().count(0.25))]
    (before, after), = filter_stores
    assert before["meta"][:3] == (True, True, True)
    assert after["meta"] == before["meta"]
    assert len(before["runs"]) == 4
    # only the partition holding 0.25 survives; nothing is left empty
    assert len(after["runs"]) == 1
    assert set(after["runs"]) < set(before["runs"])
    assert all(len(runs) for runs in after["runs"].values())


def test_store_metadata_str_table_sorted_runs(filter_stores, no_host_map):
    words = zipf_words(3000, 200, 9)
    wc = collections.Counter(words)
    _r, got = dev_run(Dampr.columns(words).count()
                      .filter(funcs.ge(3, on=funcs.snd)), n_partitions=4)
    assert sorted(got) == sorted(kv for kv in wc.items() if kv[1] >= 3)
    (before, after), = filter_stores
    assert before["meta"][3] is not None
    assert after["meta"][:3] == before["meta"][:3] == (True, True, False)
    assert after["meta"][3] is before["meta"][3]
    n_sorted = 0
    for p, runs in after["runs"].items():
        assert len(runs) == len(before["runs"][p])
        for (srt, k, _v), (srt0, _k0, _v0) in zip(runs, before["runs"][p]):
            assert srt is srt0
            if srt:
                n_sorted += 1
                assert bool((k[1:] > k[:-1]).all())
    assert n_sorted


def test_sorted_fkeys_runs_stay_sorted(filter_stores, no_host_map):
    f = _floats()
    dev_run(Dampr.columns(f).a_group_by().sum()
            .filter(funcs.between(-1, 1.5, on=funcs.fst)), n_partitions=2)
    (_before, after), = filter_stores
    for runs in after["runs"].values():
        for srt, k, _v in runs:
            assert srt
            d = decode_f64_sortable(k)
            assert bool((d[1:] > d[:-1]).all())
            assert bool(((d >= -1) & (d <= 1.5)).all())


def test_tiny_pool_spills(no_host_map, tmp_path):
    v = _ints(4000)
    old = settings.gpu_batch_records
    settings.gpu_batch_records = 512
    try:
        runner, got = dev_run(
            Dampr.columns(v).filter(funcs.gt(-20)).sort_by(),
            n_partitions=4, hbm_bytes=8192, host_bytes=8192,
            spill_dir=str(tmp_path))
    finally:
        settings.gpu_batch_records = old
    assert got == sorted(x for x in v.tolist() if x > -20)
    assert runner.stats["spilled_to_host_bytes"] > 0
    assert runner.stats["filter_rows_in"] == v.size
    assert runner.stats["filter_rows_kept"] == len(got)


def test_filtered_input_is_not_aliased(no_host_map):
    """The filter always makes new runs: a store shared with another
    consumer is untouched by it."""
    v = _ints(300)
    base = Dampr.columns(v).checkpoint(force=True)
    a = base.filter(funcs.gt(10))
    b = base.filter(funcs.le(10))
    ra, rb = Dampr.run(a, b, device="cpu")
    assert ra.read() == [x for x in v.tolist() if x > 10]
    assert rb.read() == [x for x in v.tolist() if x <= 10]


def test_rank_agreed_verdict_ignores_local_rows():
    """At world > 1 a rank without rows must reach the verdict of the
    ranks that hold some: it comes from metadata and constants alone."""
    from dampr_amd.gpu.filters import _filter_programs
    from dampr_amd.gpu.pool import DeviceRun
    from dampr_amd.gpu.stores import PartStore
    ok = [("snd", "ge", (2,))]
    only_f64 = [("snd", "gt", (float("nan"),))]
    only_i64 = [("snd", "lt", (2 ** 60 + 1,))]
    empty = PartStore(keyed=True)               # a reduce output: no vdtype
    full = PartStore(keyed=True)
    full[0] = [DeviceRun(torch.arange(3), torch.arange(3))]
    for store in (empty, full):
        assert set(_filter_programs(store, ok, rank_agreed=True)) == \
            {torch.int64, torch.float64}
        assert _filter_programs(store, only_f64, rank_agreed=True) is None
        assert _filter_programs(store, only_i64, rank_agreed=True) is None
    declared = PartStore(vdtype=torch.float64)
    assert set(_filter_programs(declared, [("identity", "gt", (0.5,))],
                                rank_agreed=True)) == {torch.float64}
    assert _filter_programs(declared, [("identity", "gt", (2 ** 60 + 1,))],
                            rank_agreed=True) is None
    # a single rank decides from the rows it holds
    assert _filter_programs(empty, only_f64) == {}
    assert set(_filter_programs(full, only_i64)) == {torch.int64}


# ---------------------------------------------------------------- backend

def test_torch_filter_rows_contract():
    from dampr_amd.gpu.backend import TorchOps
    from dampr_amd.gpu.stores import encode_f64_sortable
    ops = TorchOps()
    k = torch.arange(6, dtype=torch.int64)
    v = torch.tensor([1.5, float("nan"), -0.0, 0.0, 7.0, -2.0],
                     dtype=torch.float64)
    ok, ov = ops.filter_rows(k, v, [(1, "f64", "ge", 0.0, 0.0),
                                    (0, "i64", "ne", 4, 0)])
    assert ok.tolist() == [0, 2, 3] and ok.dtype == torch.int64
    assert ov.dtype == torch.float64
    assert [math.copysign(1, x) for x in ov.tolist()] == [1, -1, 1]
    ek = encode_f64_sortable(v)
    ok, ov = ops.filter_rows(ek, k, [(0, "fkey", "ne", 7.0, 0.0)])
    assert ov.tolist() == [0, 1, 2, 3, 5]
    ok, ov = ops.filter_rows(k[:0], v[:0], [(0, "i64", "gt", 0, 0)])
    assert ok.numel() == 0 and ov.dtype == torch.float64
    with pytest.raises(ValueError):
        ops.filter_rows(k, v, [(0, "i64", "gt", 0, 0)] * 9)
    with pytest.raises(ValueError):
        ops.filter_rows(k, v, [])


def test_oracle_and_encoders_refuse_the_same_programs():
    """The oracle backend and the kernels' program encoders share one
    validator: a malformed program raises the same exception type from
    both, for the numeric and for the string filter."""
    from dampr_amd.gpu import filters
    from dampr_amd.gpu.backend import TorchOps
    from dampr_amd.gpu.strvals import StrVals
    ops = TorchOps()
    k = torch.arange(3, dtype=torch.int64)
    sv = StrVals.from_strings(["a", "b", "c"])
    malformed = {
        "0 clauses": [],
        "9 clauses": [(0, "i64", "gt", 0, 0)] * 9,
        "str clause on column 0": [(0, "str", "eq", b"a", b"")],
        "f64 clause": [(1, "f64", "gt", 0.5, 0.0)],
        "65-byte constant": [(1, "str", "eq", b"x" * 65, b"")],
    }

    def raised(fn, *args):
        with pytest.raises(Exception) as exc:
            fn(*args)
        return type(exc.value)

    for name, prog in malformed.items():
        assert raised(ops.sv_filter_rows, k, sv, prog) is \
            raised(filters.sv_filter_program, prog, "cpu") is ValueError, name
        if name != "f64 clause":                # legal over numeric values
            assert raised(ops.filter_rows, k, k, prog) is \
                raised(filters.filter_program, prog) is ValueError, name
