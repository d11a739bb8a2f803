"""Columnar (device) engine tests on the TorchOps CPU oracle.

The same GpuRunner logic runs here and on the MI355X; only the ops backend
differs (backend.TorchOps vs backend.HipOps).  GPU-side equivalence is in
test_gpu_engine.py.
"""
import collections
import multiprocessing
import os

import numpy as np
import pytest
import torch

from dampr_amd import Dampr, funcs
from dampr_amd.gpu.engine import GpuRunner


def by_key(pairs):
    return sorted(pairs)


# --------------------------------------------------------------- basics

def test_columns_count():
    rng = np.random.default_rng(0)
    vals = rng.integers(0, 50, size=5000)
    got = Dampr.columns(vals).count().run()
    want = collections.Counter(int(v) for v in vals)
    got_pairs = sorted(got.read())
    assert got_pairs == sorted(want.items())


def test_columns_fold_by_sum_min_max():
    rng = np.random.default_rng(1)
    vals = rng.integers(-100, 100, size=3000)
    keys = rng.integers(0, 20, size=3000)

    for binop, pyop in ((funcs.add, sum), (min, min), (max, max)):
        got = Dampr.columns(vals, keys=keys).a_group_by(funcs.identity) \
            .reduce(binop)
        # a_group_by keys by key(value): identity groups equal values
        res = dict(got.run().read())
        groups = collections.defaultdict(list)
        for v in vals:
            groups[int(v)].append(int(v))
        want = {k: pyop(vs) for k, vs in groups.items()}
        assert res == want


def test_columns_sum_and_first():
    vals = np.array([5, 5, 7, 7, 7, 9], dtype=np.int64)
    res = dict(Dampr.columns(vals).a_group_by().sum().run().read())
    assert res == {5: 10, 7: 21, 9: 9}
    res = dict(Dampr.columns(vals).a_group_by().first()
               .run().read())
    assert res == {5: 5, 7: 7, 9: 9}


def test_float_values_sum():
    rng = np.random.default_rng(3)
    vals = rng.standard_normal(1000)
    keys = rng.integers(0, 8, size=1000)
    res = dict(Dampr.columns(vals, keys=keys)
               .fold_by(funcs.identity, funcs.add).run().read())
    groups = collections.defaultdict(float)
    for v in vals:
        groups[float(v)] += float(v)
    # identity key on the float value: each distinct float its own group
    assert len(res) == len(groups)


def test_device_engine_selected():
    """Columnar inputs must route to GpuRunner automatically."""
    from dampr_amd.dampr import _pick_runner
    pm = Dampr.columns(np.arange(10))
    assert _pick_runner(pm.pmer.graph, None) is GpuRunner
    pm2 = Dampr.memory(list(range(10)))
    assert _pick_runner(pm2.pmer.graph, None) is not GpuRunner


# ------------------------------------------------------- host fallback

def test_opaque_map_falls_back_and_composes():
    vals = np.arange(100)
    # .map(lambda) is opaque -> host fallback stage; the count after it
    # still runs on the columnar path
    got = Dampr.columns(vals).map(lambda v: v % 7).count().run()
    want = collections.Counter(int(v) % 7 for v in vals)
    assert sorted(got.read()) == sorted(want.items())


def test_opaque_filter_fallback():
    vals = np.arange(1000)
    got = Dampr.columns(vals).filter(lambda v: v % 3 == 0).count().run()
    want = {int(v): 1 for v in range(0, 1000, 3)}
    assert dict(got.read()) == want


# --------------------------------------------------------------- joins

def test_device_join_pair_product():
    lk = np.array([1, 1, 2, 3], dtype=np.int64)
    lv = np.array([10, 20, 30, 40], dtype=np.int64)
    rk = np.array([1, 2, 2, 9], dtype=np.int64)
    rv = np.array([2, 3, 4, 5], dtype=np.int64)
    left = Dampr.columns(lv, keys=lk)
    right = Dampr.columns(rv, keys=rk)
    out = left.join(right).reduce(funcs.pair_product, many=True).run()
    got = sorted(out.read())
    want = []
    for i, k in enumerate(lk):
        for j, k2 in enumerate(rk):
            if k == k2:
                want.append((int(k), int(lv[i]) * int(rv[j])))
    assert got == sorted(want)


def test_join_opaque_aggregate_fallback():
    lk = np.array([1, 2, 3], dtype=np.int64)
    lv = np.array([10, 20, 30], dtype=np.int64)
    rk = np.array([2, 3, 4], dtype=np.int64)
    rv = np.array([1, 2, 3], dtype=np.int64)
    out = Dampr.columns(lv, keys=lk).join(Dampr.columns(rv, keys=rk)) \
        .reduce(lambda l, r: sum(l) + sum(r)).run()
    got = sorted(out.read())
    assert got == [(2, 21), (3, 32)]


# ------------------------------------------------------------- spill

def test_spill_watermark_same_result():
    rng = np.random.default_rng(5)
    vals = rng.integers(0, 200, size=20000)
    pm = Dampr.columns(vals).count()
    # tiny pool: force every run to spill and reload
    got = pm.run(hbm_bytes=4096)
    want = collections.Counter(int(v) for v in vals)
    assert sorted(got.read()) == sorted(want.items())


def test_spill_actually_spills():
    from dampr_amd.gpu.engine import DeviceRun, HbmPool
    pool = HbmPool(1024)
    runs = []
    for i in range(8):
        k = torch.arange(64, dtype=torch.int64)
        run = DeviceRun(k, k.clone(), sorted=True)
        runs.append(run)
        pool.admit(run)
    assert any(not r.resident for r in runs)
    # reload
    for r in runs:
        pool.touch(r, torch.device("cpu"))
        assert r.resident


# --------------------------------------------------------------- sinks

def test_sink_values(tmp_path):
    vals = np.array([3, 1, 2], dtype=np.int64)
    path = str(tmp_path / "out")
    Dampr.columns(vals).checkpoint(True).sink(path).run()
    lines = []
    for f in sorted(os.listdir(path)):
        with open(os.path.join(path, f)) as fh:
            lines.extend(ln.strip() for ln in fh if ln.strip())
    assert sorted(lines) == ["1", "2", "3"]


# -------------------------------------------------- multi-rank (gloo)

def _engine_rank(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        vals = np.tile(np.arange(40), 50)       # same input on all ranks
        got = Dampr.columns(vals).count().run()
        pairs = sorted(got.read())
        # every rank owns a disjoint subset; union checked via all_gather
        gathered = [None] * world
        dist.all_gather_object(gathered, pairs)
        merged = sorted(p for lst in gathered for p in lst)
        want = collections.Counter(int(v) for v in vals)
        assert merged == sorted(want.items()), merged[:5]
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world,port_off", [(2, 0), (3, 10)])
def test_engine_gloo_multi_world(world, port_off):
    port = 29000 + (os.getpid() + port_off) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank, args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


# ------------------------------------------------- mean / topk / order

def test_mean_device_lowering():
    rng = np.random.default_rng(11)
    vals = rng.integers(0, 100, size=5000)
    got = dict(Dampr.columns(vals).mean(funcs.identity).run().read())
    groups = collections.defaultdict(list)
    for v in vals:
        groups[int(v)].append(int(v))
    want = {k: sum(vs) / float(len(vs)) for k, vs in groups.items()}
    assert got == want


def test_mean_global_default_key():
    vals = np.array([1, 2, 3, 4], dtype=np.int64)
    got = dict(Dampr.columns(vals).mean().run().read())
    assert got == {1: 2.5}


def test_mean_matches_host_engine():
    """Opaque-extractor mean still matches the host engine."""
    items = [(0, 33), (0, 12), (1, 51)]
    host = sorted(Dampr.memory(items)
                  .mean(lambda x: x[0], lambda v: v[1]).run().read())
    assert host == [(0, 22.5), (1, 51.0)]


def test_sort_by_device():
    rng = np.random.default_rng(21)
    vals = rng.integers(-1000, 1000, size=10_000)
    got = Dampr.columns(vals).sort_by().run().read()
    assert got == sorted(int(v) for v in vals)


def test_topk_device():
    rng = np.random.default_rng(12)
    vals = rng.integers(-10_000, 10_000, size=20_000)
    got = Dampr.columns(vals).topk(10).run().read()
    want = sorted(sorted((int(v) for v in vals), reverse=True)[:10])
    assert sorted(got) == want


def test_topk_float_device():
    rng = np.random.default_rng(13)
    vals = rng.standard_normal(5000)
    got = Dampr.columns(vals).topk(5).run().read()
    want = sorted(sorted((float(v) for v in vals), reverse=True)[:5])
    assert sorted(got) == pytest.approx(want)


def test_topk_custom_value_fallback():
    vals = np.arange(100)
    got = Dampr.columns(vals).topk(3, value=lambda x: -x).run().read()
    assert sorted(got) == [0, 1, 2]


def test_negative_key_output_order():
    vals = np.array([5, -3, 7, -3, 5], dtype=np.int64)
    got = list(Dampr.columns(vals).count().run().read())
    # host semantics: results in ascending (signed) key order
    assert got == [(-3, 2), (5, 2), (7, 1)]


def test_object_records_host_store():
    """Non-numeric records flow through the device engine as HostStore."""
    from dampr_amd.gpu.engine import GpuRunner
    words = ["b", "a", "b", "c", "a", "b"]
    got = Dampr.memory(words).count().run(runner=GpuRunner).read()
    assert sorted(got) == [("a", 2), ("b", 3), ("c", 1)]


def test_trace_rows():
    from dampr_amd.utils.trace import get_trace
    vals = np.arange(1000)
    Dampr.columns(vals).count().run()
    tr = get_trace()
    assert len(tr.rows) >= 3          # ingest + map + reduce
    assert all(r["wall_ms"] >= 0 for r in tr.rows)
    assert "stage" in tr.report()


def test_disk_spill_tier(tmp_path):
    """Force both watermarks tiny: runs cascade HBM->host->disk and come
    back bit-exact."""
    rng = np.random.default_rng(6)
    vals = rng.integers(0, 500, size=30000)
    got = Dampr.columns(vals).count().run(
        hbm_bytes=2048, host_bytes=4096, spill_dir=str(tmp_path))
    want = collections.Counter(int(v) for v in vals)
    assert sorted(got.read()) == sorted(want.items())


def test_disk_spill_files_created(tmp_path):
    from dampr_amd.gpu.engine import DeviceRun, HbmPool
    pool = HbmPool(512, host_capacity=512, spill_dir=str(tmp_path))
    runs = []
    for i in range(8):
        k = torch.arange(64, dtype=torch.int64) + i
        run = DeviceRun(k, k.clone(), sorted=True)
        runs.append(run)
        pool.admit(run)
    assert any(r.on_disk for r in runs)
    for i, r in enumerate(runs):
        pool.touch(r, torch.device("cpu"))
        assert torch.equal(r.keys, torch.arange(64, dtype=torch.int64) + i)


def test_device_text_df_cpu_fallback():
    """device_text + tokenize_set + count: on CPU the engine decodes the
    text and runs the host operators; the GPU path fuses into the df
    kernel (tests/test_gpu_engine.py)."""
    text = b"the cat sat\nthe dog the dog ran\ncat!\n"
    got = dict(Dampr.device_text(text)
               .flat_map(funcs.tokenize_set).count().run().read())
    assert got == {"the": 2, "cat": 2, "sat": 1, "dog": 1, "ran": 1}


def test_tokenize_set_matches_kernel_charset():
    assert funcs.tokenize_set("A_b9 c-d") == {"a_b9", "c", "d"}


def test_multi_output_shared_subgraph_device():
    """Dampr.run over the device engine: two outputs sharing one columnar
    subgraph (the word-stats idiom)."""
    rng = np.random.default_rng(41)
    vals = rng.integers(0, 30, size=3000)
    base = Dampr.columns(vals).checkpoint(True)
    counts = base.count()
    sums = base.fold_by(funcs.identity, funcs.add)
    ec, es = Dampr.run(counts, sums)
    want_c = collections.Counter(int(v) for v in vals)
    assert sorted(ec.read()) == sorted(want_c.items())
    want_s = {k: k * c for k, c in want_c.items()}
    assert sorted(es.read()) == sorted(want_s.items())


def test_device_text_df_compose_downstream():
    """TokenStore results compose with downstream host-fallback stages."""
    text = b"aa bb\naa cc\n"
    got = sorted(Dampr.device_text(text)
                 .flat_map(funcs.tokenize_set).count()
                 .filter(lambda kv: kv[1] > 1).run().read())
    assert got == [("aa", 2)]


def _engine_rank2(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)

        # device join across ranks: both sides co-partitioned by the
        # exchange; union of per-rank outputs == single-rank oracle
        lk = np.arange(1000) % 37
        lv = np.arange(1000)
        rk = np.arange(200) % 37
        rv = np.arange(200) * 2
        out = Dampr.columns(lv, keys=lk).join(
            Dampr.columns(rv, keys=rk)) \
            .reduce(funcs.pair_sum, many=True).run()
        pairs = sorted(out.read())
        gathered = [None] * world
        dist.all_gather_object(gathered, pairs)
        merged = sorted(p for lst in gathered for p in lst)
        want = []
        for i in range(1000):
            for j in range(200):
                if lk[i] == rk[j]:
                    want.append((int(lk[i]), int(lv[i] + rv[j])))
        assert merged == sorted(want), (len(merged), len(want))

        # device len across ranks: local counts summed on the owner rank
        nv = np.arange(4000)
        got_len = Dampr.columns(nv).len().run().read()
        gathered = [None] * world
        dist.all_gather_object(gathered, got_len)
        assert sorted(x for lst in gathered for x in lst) == [4000]

        # device topk across ranks: candidates meet on rank 0
        vals = np.arange(5000)
        got = Dampr.columns(vals).topk(7).run().read()
        gathered = [None] * world
        dist.all_gather_object(gathered, got)
        merged = sorted(p for lst in gathered for p in lst)
        # every rank ingests a slice; global top-7 of the union
        assert merged == list(range(4993, 5000)), merged
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world,port_off", [(2, 20), (3, 30)])
def test_engine_gloo_join_topk(world, port_off):
    port = 29000 + (os.getpid() + port_off) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank2, args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


def test_lazy_ingest_spill_paths(tmp_path):
    """Lazy unpartitioned ingest under a tiny pool: count, topk and sort
    all stream through spilled batched runs with exact results."""
    import dampr_amd.settings as st
    old = st.gpu_batch_records
    st.gpu_batch_records = 1000        # many small runs
    try:
        rng = np.random.default_rng(8)
        vals = rng.integers(0, 300, size=25000)
        kw = dict(hbm_bytes=32768, host_bytes=32768,
                  spill_dir=str(tmp_path))
        got = dict(Dampr.columns(vals).count().run(**kw).read())
        want = collections.Counter(int(v) for v in vals)
        assert got == dict(want)
        top = Dampr.columns(vals).topk(5).run(**kw).read()
        assert sorted(top) == sorted(sorted(
            (int(v) for v in vals), reverse=True)[:5])
    finally:
        st.gpu_batch_records = old


def test_skewed_partition_batched_reduce(tmp_path):
    """A partition whose runs exceed half the pool reduces run-by-run
    (associative re-reduce) instead of one giant merge."""
    import dampr_amd.settings as st
    old = st.gpu_batch_records
    st.gpu_batch_records = 2000
    try:
        rng = np.random.default_rng(13)
        vals = rng.integers(0, 50, size=30000)   # heavy duplication
        got = dict(Dampr.columns(vals)
                   .fold_by(funcs.identity, funcs.add)
                   .run(hbm_bytes=16384, host_bytes=16384,
                        spill_dir=str(tmp_path)).read())
        groups = collections.defaultdict(int)
        for v in vals:
            groups[int(v)] += int(v)
        assert got == dict(groups)
        # min/max through the same path
        got = dict(Dampr.columns(vals).a_group_by().reduce(min)
                   .run(hbm_bytes=16384).read())
        assert got == {int(v): int(v) for v in set(vals.tolist())}
    finally:
        st.gpu_batch_records = old


def test_string_keys_device_dictionary():
    """String keys dictionary-encode to rank ids: device count/sort with
    host-ordered decode."""
    from dampr_amd.gpu.engine import GpuRunner
    words = ["pear", "apple", "pear", "fig", "apple", "pear"]
    got = list(Dampr.memory(words).count().run(runner=GpuRunner).read())
    assert got == [("apple", 2), ("fig", 1), ("pear", 3)]  # lex order

    got = dict(Dampr.memory(words)
               .fold_by(lambda w: w, lambda a, b: a + b,
                        value=lambda _w: 1).run(runner=GpuRunner).read())
    assert got == {"apple": 2, "fig": 1, "pear": 3}


def test_string_keys_join_falls_back_correct():
    """Rank ids from different encodes are incompatible; joins over
    string-keyed stores combine as host records with exact results."""
    from dampr_amd.gpu.engine import GpuRunner
    left = Dampr.memory([("a", 1), ("b", 2)]).group_by(lambda x: x[0],
                                                       lambda x: x[1])
    right = Dampr.memory([("b", 10), ("c", 20)]).group_by(lambda x: x[0],
                                                          lambda x: x[1])
    out = left.join(right).reduce(lambda l, r: sum(l) + sum(r)) \
        .run(runner=GpuRunner)
    assert sorted(out.read()) == [("b", 12)]


def test_string_keys_host_engine_parity():
    from dampr_amd.gpu.engine import GpuRunner
    from dampr_amd.runner import MTRunner
    rng = np.random.default_rng(55)
    words = ["w{}".format(int(i)) for i in rng.integers(0, 40, size=2000)]
    dev = sorted(Dampr.memory(words).count().run(runner=GpuRunner).read())
    host = sorted(Dampr.memory(words).count().run(runner=MTRunner).read())
    assert dev == host


def test_mixed_sources_one_run():
    """Dampr.run over a graph mixing columnar and host-memory inputs:
    the device engine carries both (HostStore for object records)."""
    from dampr_amd.gpu.engine import GpuRunner
    a = Dampr.columns(np.array([1, 1, 2], dtype=np.int64)).count()
    b = Dampr.memory(["x", "y", "x"]).count()
    ea, eb = Dampr.run(a, b, runner=GpuRunner)
    assert sorted(ea.read()) == [(1, 2), (2, 1)]
    assert sorted(eb.read()) == [("x", 2), ("y", 1)]


def test_skewed_mean_and_first(tmp_path):
    import dampr_amd.settings as st
    old = st.gpu_batch_records
    st.gpu_batch_records = 1500
    try:
        rng = np.random.default_rng(17)
        vals = rng.integers(0, 40, size=20000)
        kw = dict(hbm_bytes=16384, host_bytes=16384,
                  spill_dir=str(tmp_path))
        got = dict(Dampr.columns(vals).mean(funcs.identity)
                   .run(**kw).read())
        groups = collections.defaultdict(list)
        for v in vals:
            groups[int(v)].append(int(v))
        want = {k: sum(g) / float(len(g)) for k, g in groups.items()}
        assert got == want
        got = dict(Dampr.columns(vals).a_group_by().first()
                   .run(**kw).read())
        assert got == {int(v): int(v) for v in set(vals.tolist())}
    finally:
        st.gpu_batch_records = old


def test_pool_stats_exposed(tmp_path):
    from dampr_amd.gpu.engine import GpuRunner
    rng = np.random.default_rng(19)
    vals = rng.integers(0, 100, size=20000)
    pm = Dampr.columns(vals).count().checkpoint()
    runner = GpuRunner("statrun", pm.pmer.graph, hbm_bytes=8192,
                       host_bytes=8192, spill_dir=str(tmp_path))
    runner.run([pm.source])
    st = runner.stats
    assert st["spilled_to_host_bytes"] > 0
    assert st["reloads_bytes"] > 0
    assert "spilled_to_disk_bytes" in st


def test_len_device_metadata():
    rng = np.random.default_rng(23)
    vals = rng.integers(0, 10, size=12345)
    got = Dampr.columns(vals).len().run().read()
    assert got == [12345]
    # host parity
    from dampr_amd.runner import MTRunner
    host = Dampr.memory(vals.tolist()).len().run(runner=MTRunner).read()
    assert host == [12345]


def test_eager_free_releases_consumed_runs(tmp_path):
    """Intermediate stores free after their last consumer; shared/output
    runs survive (identity/unkey aliasing)."""
    from dampr_amd.gpu.engine import GpuRunner
    rng = np.random.default_rng(29)
    vals = rng.integers(0, 50, size=5000)
    pm = Dampr.columns(vals).count()
    runner = GpuRunner("freerun", pm.pmer.graph, spill_dir=str(tmp_path))
    before = runner.pool.used
    [ds] = runner.run([pm.source])
    # output intact
    assert sorted(r for r in ds.read()) == sorted(
        (int(k), (int(k), int(c)))
        for k, c in __import__("collections").Counter(
            int(v) for v in vals).items())
    # only the output's bytes remain accounted in the pool
    out_bytes = ds.keys_t.numel() * 8 + ds.vals_t.numel() * 8
    assert runner.pool.used <= out_bytes * 2 + 4096


def test_cross_right_scalar_device_engine():
    """cross_right (broadcast scalar apply) through the device engine's
    host-fallback path — the reference TF-IDF idf idiom."""
    from dampr_amd.gpu.engine import GpuRunner
    docs = Dampr.memory([10, 20, 30, 40])
    total = docs.len()
    out = docs.cross_right(total, lambda v, t: v / float(t)) \
        .run(runner=GpuRunner)
    assert sorted(out.read()) == [2.5, 5.0, 7.5, 10.0]


def test_group_by_unique_device_engine():
    from dampr_amd.gpu.engine import GpuRunner
    names = [("a", 1), ("a", 1), ("a", 2), ("b", 9)]
    res = Dampr.memory(names) \
        .group_by(lambda x: x[0], lambda x: x[1]).unique() \
        .run(runner=GpuRunner)
    got = sorted(res.read())
    assert got == [("a", [1, 2]), ("b", [9])] or \
        got == sorted([("a", [1, 2]), ("b", [9])])


def test_sample_device_engine():
    from dampr_amd.gpu.engine import GpuRunner
    vals = list(range(1000))
    got = Dampr.memory(vals).sample(0.5).count(lambda _x: 1) \
        .run(runner=GpuRunner).read()
    assert len(got) == 1
    assert 300 < got[0][1] < 700


def test_concat_device_engine():
    from dampr_amd.gpu.engine import GpuRunner
    a = Dampr.columns(np.array([1, 2], dtype=np.int64))
    b = Dampr.columns(np.array([3, 4], dtype=np.int64))
    got = sorted(a.concat(b).run(runner=GpuRunner).read())
    assert got == [1, 2, 3, 4]
    # object records too
    c = Dampr.memory(["x"]).concat(Dampr.memory(["y", "x"]))
    assert sorted(c.count().run(runner=GpuRunner).read()) == \
        [("x", 2), ("y", 1)]


def test_pjoin_default_run_device_engine():
    """PJoin.run() (no reduce) materializes (left_list, right_list)
    values through the device engine's HostStore path."""
    from dampr_amd.gpu.engine import GpuRunner
    l = Dampr.columns(np.array([10, 20]), keys=np.array([1, 2]))
    r = Dampr.columns(np.array([5]), keys=np.array([2]))
    got = sorted(l.join(r).run(runner=GpuRunner).read())
    assert got == [(2, ([20], [5]))]


def test_text_input_device_engine(tmp_path):
    """Dampr.text file input ingested by the device engine (host decode
    into records; numeric pipeline thereafter)."""
    from dampr_amd.gpu.engine import GpuRunner
    f = tmp_path / "nums.txt"
    f.write_text("\n".join(str(i % 5) for i in range(100)) + "\n")
    got = dict(Dampr.text(str(f)).map(int).count()
               .run(runner=GpuRunner).read())
    assert got == {k: 20 for k in range(5)}


def test_device_join_probe_batching(monkeypatch):
    """Skewed-join guard (ROADMAP 7): an oversized probe side is joined
    in batches against the once-built table; results must be identical
    to the unbatched join."""
    monkeypatch.setenv("DAMPR_JOIN_PROBE_ROWS", "1000")
    rng = np.random.RandomState(7)
    # hot key 5 dominates the left side -> many probe batches
    lk = np.concatenate([np.full(5000, 5), rng.randint(0, 50, 500)]) \
        .astype(np.int64)
    lv = rng.randint(1, 100, lk.size).astype(np.int64)
    rk = np.array([5, 5, 7, 9], dtype=np.int64)
    rv = np.array([2, 3, 4, 5], dtype=np.int64)
    out = Dampr.columns(lv, keys=lk).join(Dampr.columns(rv, keys=rk)) \
        .reduce(funcs.pair_product, many=True).run()
    got = sorted(out.read())
    rmap = {}
    for j, k in enumerate(rk):
        rmap.setdefault(int(k), []).append(int(rv[j]))
    want = sorted((int(k), int(v) * w)
                  for k, v in zip(lk, lv) for w in rmap.get(int(k), []))
    assert got == want and len(want) > 10000


def test_device_join_build_side_swap(monkeypatch):
    """Inner join with the oversized side on the RIGHT (the build side):
    the engine swaps sides so the big side is probed in batches."""
    monkeypatch.setenv("DAMPR_JOIN_PROBE_ROWS", "1000")
    rng = np.random.RandomState(11)
    lk = np.array([3, 4, 4, 8], dtype=np.int64)
    lv = np.array([7, 1, 2, 9], dtype=np.int64)
    rk = np.concatenate([np.full(4000, 4), rng.randint(0, 20, 400)]) \
        .astype(np.int64)
    rv = rng.randint(1, 50, rk.size).astype(np.int64)
    out = Dampr.columns(lv, keys=lk).join(Dampr.columns(rv, keys=rk)) \
        .reduce(funcs.pair_sum, many=True).run()
    got = sorted(out.read())
    rmap = {}
    for j, k in enumerate(rk):
        rmap.setdefault(int(k), []).append(int(rv[j]))
    want = sorted((int(k), int(v) + w)
                  for k, v in zip(lk, lv) for w in rmap.get(int(k), []))
    assert got == want and len(want) > 4000


def _engine_rank_text(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        text = b"apple pear\npear fig apple\nfig fig kiwi\napple kiwi\n" * 40
        got = sorted(Dampr.device_text(np.frombuffer(text, dtype=np.uint8))
                     .flat_map(funcs.tokenize_set).count().run().read())
        gathered = [None] * world
        dist.all_gather_object(gathered, got)
        merged = sorted(p for lst in gathered for p in lst)
        # per-line token SET counts: each word's df over 160 lines
        want = sorted([("apple", 120), ("fig", 80),
                       ("kiwi", 80), ("pear", 80)])
        assert merged == want, merged
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 3])
def test_engine_gloo_device_text(world):
    """Multi-rank device_text (ROADMAP 3): each rank counts its
    newline-aligned slice; partial dfs merge across ranks."""
    port = 29000 + (os.getpid() + 20 + world) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank_text, args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


def test_unify_str_stores_remap():
    """Cross-encode dictionary remap (ROADMAP 2): two stores whose rank
    ids came from different string tables combine on device through the
    union table; decoded records must keep their original strings."""
    import torch
    from dampr_amd.gpu.engine import DeviceRun, GpuRunner, PartStore
    from dampr_amd.runner import Graph
    r = GpuRunner("unify-test", Graph())
    a = PartStore(str_table=("apple", "fig"))
    a[0] = [DeviceRun(torch.tensor([0, 1, 0]), torch.tensor([1, 2, 3]),
                      sorted=True)]
    b = PartStore(str_table=("apple", "kiwi"))
    b[0] = [DeviceRun(torch.tensor([0, 1]), torch.tensor([4, 5]),
                      sorted=True)]
    for run in a[0] + b[0]:
        r.pool.admit(run)
    ua, ub = r._unify_str_stores([a, b])
    assert ua.str_table == ub.str_table == ("apple", "fig", "kiwi")
    got_a = sorted(r._decode_store(ua))
    got_b = sorted(r._decode_store(ub))
    assert got_a == [("apple", 1), ("apple", 3), ("fig", 2)]
    assert got_b == [("apple", 4), ("kiwi", 5)]
    # dictionary + dictionary-less mix: no unification
    c = PartStore()
    c[0] = [DeviceRun(torch.tensor([7]), torch.tensor([8]), sorted=True)]
    assert r._unify_str_stores([a, c]) is None
    r.pool.cleanup()


def _engine_rank_strkeys(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dampr_amd.gpu.engine import GpuRunner

        # string keys whose per-rank slices have DIFFERENT vocabularies:
        # a per-rank dictionary would give 'fig' and 'kiwi' the same id
        items = ["apple", "fig"] * 50 + ["apple", "kiwi"] * 50
        got = sorted(Dampr.memory(items).count()
                     .run(runner=GpuRunner).read())
        gathered = [None] * world
        dist.all_gather_object(gathered, got)
        merged = sorted(p for lst in gathered for p in lst)
        assert merged == [("apple", 100), ("fig", 50), ("kiwi", 50)], \
            merged

        # object (string) VALUES force the host-record path: the reduce
        # must still see every rank's values for a key
        pairs = [("a", "x"), ("b", "y"), ("a", "z"), ("b", "w")] * 10
        got2 = sorted(Dampr.memory(pairs)
                      .group_by(lambda kv: kv[0], lambda kv: kv[1])
                      .reduce(lambda _k, vs: "".join(sorted(vs)))
                      .run(runner=GpuRunner).read())
        gathered = [None] * world
        dist.all_gather_object(gathered, got2)
        merged2 = sorted(p for lst in gathered for p in lst)
        assert merged2 == [("a", "x" * 10 + "z" * 10),
                           ("b", "w" * 10 + "y" * 10)], merged2
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 3])
def test_engine_gloo_string_keys(world):
    """Multi-rank string keys: the encode agrees on ONE dictionary via a
    single metadata all_gather, and host-fallback reduces exchange
    records by a process-stable hash (regression: per-rank dictionaries
    conflated different strings; host reduces folded only local
    slices)."""
    port = 29000 + (os.getpid() + 40 + world) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank_strkeys,
                         args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


def _engine_rank_cross(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dampr_amd.gpu.engine import GpuRunner

        # word-stats idiom: every rank must see the COMPLETE computed
        # total on the supplemental side (regression: rank slices /
        # rank-owned shards crossed partially)
        vals = list(range(1, 9)) * 5          # sum = 180
        got = Dampr.memory(vals).cross_right(
            Dampr.memory(vals).fold_by(lambda _v: 1,
                                       lambda a, b: a + b),
            lambda v, kv: v * kv[1]).run(runner=GpuRunner).read()
        gathered = [None] * world
        dist.all_gather_object(gathered, got)
        merged = sorted(p for lst in gathered for p in lst)
        assert merged == sorted(v * 180 for v in vals), merged[:6]

        # cross_set: aggregate side must be the full multi-rank union.
        # NB the reference streams `other` and aggregates `self`
        # (its docstring example contradicts its own behavior); we
        # match the behavior, so the output is one record per `other`
        # element
        got2 = Dampr.memory([1, 2, 3, 4, 5, 6]).cross_set(
            Dampr.memory([2, 9]), lambda v, right: v in right,
            agg=set).run(runner=GpuRunner).read()
        gathered = [None] * world
        dist.all_gather_object(gathered, got2)
        merged2 = sorted(p for lst in gathered for p in lst)
        assert merged2 == [False, True], merged2
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 3])
def test_engine_gloo_cross_joins(world):
    """Multi-rank cross/broadcast joins gather the supplemental side."""
    port = 29000 + (os.getpid() + 60 + world) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank_cross,
                         args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


def _engine_rank_mixed_kinds(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dampr_amd.gpu.engine import GpuRunner

        # rank 0's slice has int keys only, rank 1's has floats: a
        # per-rank encode would exchange i64 against f64-encoded
        # columns; the world encode must agree on one layout
        items = [(1, 10), (2, 20)] * 25 + [(1.5, 5), (2.5, 7)] * 25
        got = sorted(Dampr.memory(items)
                     .a_group_by(lambda kv: kv[0], lambda kv: kv[1])
                     .sum().run(runner=GpuRunner).read())
        gathered = [None] * world
        dist.all_gather_object(gathered, got)
        merged = sorted(p for lst in gathered for p in lst)
        assert merged == [(1, 250), (1.5, 125), (2, 500), (2.5, 175)], \
            merged
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 3])
def test_engine_gloo_mixed_key_kinds(world):
    """Ranks whose record slices disagree on key dtype agree on one
    layout through the world encode (f64 order-preserving keys)."""
    port = 29000 + (os.getpid() + 70 + world) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank_mixed_kinds,
                         args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


# ------------------------------------------------- string-keyed columns

def test_columns_string_keys_collect():
    # non-keyed collect yields values (ValueEmitter contract); the
    # string keys surface through keyed ops -- see the join test
    vals = np.array([3, 1, 2, 9], dtype=np.int64)
    keys = np.array(["pear", "apple", "pear", "fig"])
    got = sorted(Dampr.columns(vals, keys=keys).run().read())
    assert got == [1, 2, 3, 9]


def test_columns_string_keys_device_join():
    """String-keyed columns join ON DEVICE: different vocabularies remap
    through the union dictionary (the hash-join kernel path, not the
    host fallback)."""
    lk = np.array(["apple", "apple", "fig", "yam"])
    lv = np.array([1, 2, 3, 4], dtype=np.int64)
    rk = np.array(["apple", "kiwi", "fig"])
    rv = np.array([10, 20, 30], dtype=np.int64)
    out = Dampr.columns(lv, keys=lk).join(Dampr.columns(rv, keys=rk)) \
        .reduce(funcs.pair_sum, many=True).run()
    got = sorted(out.read())
    assert got == [("apple", 11), ("apple", 12), ("fig", 33)]


def test_columns_string_keys_world_pre_slice_table():
    """The dictionary is built from the FULL input before rank slicing
    (single-rank here; the world path shares the same table object)."""
    from dampr_amd.gpu.engine import ColumnSource
    src = ColumnSource.from_data(
        np.arange(4), keys=["b", "a", "b", "c"])
    assert src.str_table == ("a", "b", "c")
    assert src.keys.tolist() == [1, 0, 1, 2]


def test_columns_string_values_accepted():
    """String VALUE columns ride the var-len byte arena (round 2); the
    round-1 TypeError is gone."""
    ds = Dampr.columns(np.array(["x", "y"])).checkpoint(True) \
        .run(runner=GpuRunner)
    assert sorted(ds.read()) == ["x", "y"]


def _engine_rank_strcols(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        lk = np.array(["apple", "apple", "fig", "yam"] * 20)
        lv = np.arange(80, dtype=np.int64)
        rk = np.array(["apple", "kiwi", "fig"] * 10)
        rv = np.arange(30, dtype=np.int64)
        out = Dampr.columns(lv, keys=lk).join(
            Dampr.columns(rv, keys=rk)) \
            .reduce(funcs.pair_sum, many=True).run()
        got = sorted(out.read())
        gathered = [None] * world
        dist.all_gather_object(gathered, got)
        merged = sorted(p for lst in gathered for p in lst)
        want = sorted((str(k), int(a) + int(b))
                      for k, a in zip(lk, lv)
                      for k2, b in zip(rk, rv) if k == k2)
        assert merged == want, (len(merged), len(want))
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 3])
def test_engine_gloo_string_columns_join(world):
    """Multi-rank string-keyed column join: the ingest dictionary is
    built pre-slice, so every rank shares it."""
    port = 29000 + (os.getpid() + 80 + world) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank_strcols,
                         args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


def test_device_sort_by_strings():
    """sort_by over string records through the device engine: the
    dictionary's rank order is lexicographic, so sorted ids decode to
    host-ordered strings."""
    words = ["pear", "apple", "fig", "apple", "kiwi"]
    got = Dampr.memory(words).sort_by().run(runner=GpuRunner).read()
    assert got == sorted(words)


def test_pair_funcs_full_product_both_engines():
    """funcs.pair_* are the FULL cross product per key on both engines
    (they materialize the one-pass right iterator; a bare nested
    comprehension would keep only the first left value's pairs --
    reference generator-exhaustion semantics, pinned by the
    groupby_join_lazy parity case)."""
    from dampr_amd.runner import MTRunner
    items = [("apple", 3), ("pear", 1), ("apple", 2), ("fig", 9),
             ("apple", 1)]
    right = [("apple", 10), ("fig", 5), ("apple", 20)]

    def build(D):
        return D.memory(items) \
            .group_by(lambda kv: kv[0], lambda kv: kv[1]) \
            .join(D.memory(right)
                  .group_by(lambda kv: kv[0], lambda kv: kv[1])) \
            .reduce(funcs.pair_sum, many=True)

    dev = sorted(build(Dampr).run(runner=GpuRunner).read())
    host = sorted(build(Dampr).run().read())
    want = sorted((k, lv + rv) for k, lv in items
                  for k2, rv in right if k == k2)
    assert dev == want and host == want


def test_negative_zero_float_keys_merge():
    """-0.0 and 0.0 are one group (Python ==): the f64 sortable encode
    canonicalizes the sign bit of zero before grouping."""
    from dampr_amd.runner import MTRunner
    vals = np.array([0.0, -0.0, 1.5, -0.0], dtype=np.float64)
    dev = sorted(map(repr, Dampr.columns(vals).count().run().read()))
    host = sorted(map(repr, Dampr.memory(vals.tolist()).count()
                      .run(runner=MTRunner).read()))
    assert dev == host == ["(0.0, 3)", "(1.5, 1)"]


def _engine_rank_tiny(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dampr_amd.gpu.engine import GpuRunner
        # fewer rows than ranks: some slices are EMPTY, and empty ranks
        # must still take part in every exchange
        got = Dampr.columns(np.array([7, 7], dtype=np.int64)).count() \
            .run().read()
        gathered = [None] * world
        dist.all_gather_object(gathered, got)
        merged = sorted(p for lst in gathered for p in lst)
        assert merged == [(7, 2)], merged
        # same through host records (string key)
        got2 = Dampr.memory(["only"]).count().run(runner=GpuRunner) \
            .read()
        gathered = [None] * world
        dist.all_gather_object(gathered, got2)
        merged2 = sorted(p for lst in gathered for p in lst)
        assert merged2 == [("only", 1)], merged2
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [3])
def test_engine_gloo_tiny_inputs(world):
    """Inputs smaller than the world: empty rank slices still join every
    collective."""
    port = 29000 + (os.getpid() + 100 + world) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank_tiny,
                         args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


def test_columns_unicode_string_keys():
    keys = np.array(["éclair", "zèbre", "日本", "éclair", "ß", "𝄞note"])
    vals = np.arange(6, dtype=np.int64)
    got = sorted(Dampr.columns(vals, keys=keys).join(
        Dampr.columns(np.array([100], dtype=np.int64),
                      keys=np.array(["éclair"])))
        .reduce(funcs.pair_sum, many=True).run().read())
    assert got == [("éclair", 100), ("éclair", 103)]


def test_columns_float_keys_join():
    """Float key columns: order-preserving f64 encode at ingest
    (regression: an int64 cast silently truncated 1.5 and 2.5 to 1)."""
    keys = np.array([1.5, 2.5, 1.5], dtype=np.float64)
    vals = np.array([1, 2, 3], dtype=np.int64)
    out = sorted(Dampr.columns(vals, keys=keys).join(
        Dampr.columns(np.array([10], dtype=np.int64),
                      keys=np.array([1.5])))
        .reduce(funcs.pair_sum, many=True).run().read())
    assert out == [(1.5, 11), (1.5, 13)]


def test_device_sink_tsv_string_keys(tmp_path):
    path = str(tmp_path / "tsv")
    Dampr.memory([("b", 2), ("a", 1), ("b", 5)]).count(lambda kv: kv[0]) \
        .sink_tsv(path).run(runner=GpuRunner)
    lines = []
    for f in sorted(os.listdir(path)):
        with open(os.path.join(path, f)) as fh:
            lines.extend(ln.rstrip("\n") for ln in fh if ln.strip())
    assert sorted(lines) == ["a\t1", "b\t2"]


def test_device_sink_json_objects(tmp_path):
    import json
    path = str(tmp_path / "j")
    Dampr.memory([{"a": 1}, {"a": 2}]).sink_json(path) \
        .run(runner=GpuRunner)
    vals = []
    for f in sorted(os.listdir(path)):
        with open(os.path.join(path, f)) as fh:
            vals.extend(json.loads(ln) for ln in fh if ln.strip())
    assert sorted(v["a"] for v in vals) == [1, 2]


def test_device_engine_misc_inputs(tmp_path):
    """Input taps through the device engine: gzip text files and
    multi-dataset read_input (host decode, columnar shuffle core)."""
    import gzip
    from dampr_amd import Dataset
    p = str(tmp_path / "x.gz")
    with gzip.open(p, "wt") as fh:
        fh.write("a b\nb b\n" * 10)
    got = sorted(Dampr.text(p).flat_map(str.split).count()
                 .run(runner=GpuRunner).read())
    assert got == [("a", 10), ("b", 30)]

    class RangeDataset(Dataset):
        def __init__(self, n):
            self.n = n

        def read(self):
            for i in range(self.n):
                yield i, i

    got2 = sorted(Dampr.read_input(RangeDataset(5), RangeDataset(3))
                  .count().run(runner=GpuRunner).read())
    assert got2 == [(0, 2), (1, 2), (2, 2), (3, 1), (4, 1)]


def test_sink_output_readable_downstream(tmp_path):
    """A sink's output dataset is consumable downstream (host parity:
    _SinkWorker returns its TextLineDatasets); round 1 the device sink
    returned an empty store and silently dropped the data."""
    path = str(tmp_path / "s")
    em = Dampr.memory([3, 1, 2]).map(lambda v: v * 10).sink(path) \
        .run(runner=GpuRunner)
    got = sorted(em.read())
    assert got == ["10", "20", "30"]          # text lines, like the host


def test_sink_numeric_values_both_engines(tmp_path):
    """Reference SinkWriter prints ANY value (print(value, file=f));
    both engines must accept non-str values identically."""
    hp = str(tmp_path / "h")
    dp = str(tmp_path / "d")
    Dampr.memory([3, 1, 2]).sink(hp).run()
    Dampr.columns(np.array([3, 1, 2], dtype=np.int64)) \
        .checkpoint(True).sink(dp).run(runner=GpuRunner)

    def lines(d):
        out = []
        for f in sorted(os.listdir(d)):
            with open(os.path.join(d, f)) as fh:
                out.extend(ln.strip() for ln in fh if ln.strip())
        return sorted(out)

    assert lines(hp) == ["1", "2", "3"]
    assert lines(dp) == ["1", "2", "3"]


def test_join_mixed_float_int_keys_device():
    """Float-keyed store joined with an int-keyed store: host semantics
    say 1.0 == 1, so the int side re-encodes through the f64 sortable
    encoding (round 1 this silently returned [])."""
    lv = np.array([10, 20], dtype=np.int64)
    rv = np.array([1, 2], dtype=np.int64)
    out = Dampr.columns(lv, keys=np.array([1.0, 2.0])) \
        .join(Dampr.columns(rv, keys=np.array([1, 2], dtype=np.int64))) \
        .reduce(funcs.pair_sum, many=True).run(runner=GpuRunner)
    assert sorted(out.read()) == [(1.0, 11), (2.0, 22)]
    # and host-engine agreement
    host = Dampr.memory([(1.0, 10), (2.0, 20)]) \
        .group_by(lambda kv: kv[0], lambda kv: kv[1]) \
        .join(Dampr.memory([(1, 1), (2, 2)])
              .group_by(lambda kv: kv[0], lambda kv: kv[1])) \
        .reduce(lambda l, r: [a + b for a in list(l) for b in list(r)],
                many=True).run()
    assert sorted(host.read()) == [(1.0, 11), (2.0, 22)] \
        or sorted(host.read()) == [(1, 11), (2, 22)]


def test_join_mixed_int_float_keys_left():
    """Same fkeys-unification path, left join direction flipped (the
    INT side is the left/probe side)."""
    lv = np.array([10, 20, 30], dtype=np.int64)
    rv = np.array([1, 2], dtype=np.int64)
    out = Dampr.columns(lv, keys=np.array([1, 2, 7], dtype=np.int64)) \
        .join(Dampr.columns(rv, keys=np.array([1.0, 2.0]))) \
        .reduce(funcs.pair_sum, many=True).run(runner=GpuRunner)
    assert sorted(out.read()) == [(1.0, 11), (2.0, 22)]


def test_hash_join_zero_key_torchops():
    """Engine-level zero/one key join separation (TorchOps here; the
    HIP-kernel regression is tests/test_gpu_relational.py)."""
    lk = np.array([0, 1, 0], dtype=np.int64)
    lv = np.array([1, 2, 3], dtype=np.int64)
    rk = np.array([0, 1], dtype=np.int64)
    rv = np.array([10, 20], dtype=np.int64)
    out = Dampr.columns(lv, keys=lk).join(Dampr.columns(rv, keys=rk)) \
        .reduce(funcs.pair_sum, many=True).run(runner=GpuRunner)
    assert sorted(out.read()) == [(0, 11), (0, 13), (1, 22)]


# ----------------------------------------------- var-len (string) values

def test_str_values_first():
    """a_group_by().first() over string values: grouping keys by the
    string VALUE (host dict-encode), then the device 'first' reduce
    runs over a string-keyed StrVals store (gather-only columnar)."""
    vals = np.array(["b", "a", "b", "c", "a"])
    res = Dampr.columns(vals).a_group_by().first().run(runner=GpuRunner)
    got = sorted(res.read())
    assert [k for k, _v in got] == ["a", "b", "c"]
    assert all((v == k or v == (k, k)) for k, v in got), got


def test_str_values_sort_by_key_order():
    keys = np.array([3, 1, 2], dtype=np.int64)
    vals = np.array(["three", "one", "two"])
    out = Dampr.columns(vals, keys=keys)
    ds = out.checkpoint(True).run(runner=GpuRunner)
    assert list(ds.read()) == ["one", "two", "three"]


def test_str_values_join_pair_left_right():
    lk = np.array([1, 2, 2, 9], dtype=np.int64)
    lv = np.array(["l1", "l2a", "l2b", "l9"])
    rk = np.array([2, 1, 2], dtype=np.int64)
    rv = np.array(["r2a", "r1", "r2b"])
    left = Dampr.columns(lv, keys=lk)
    right = Dampr.columns(rv, keys=rk)
    out = left.join(right).reduce(funcs.pair_left, many=True) \
        .run(runner=GpuRunner)
    want_left = [(1, "l1"), (2, "l2a"), (2, "l2a"), (2, "l2b"),
                 (2, "l2b")]
    assert sorted(out.read()) == sorted(want_left)
    out2 = Dampr.columns(lv, keys=lk) \
        .join(Dampr.columns(rv, keys=rk)) \
        .reduce(funcs.pair_right, many=True).run(runner=GpuRunner)
    want_right = [(1, "r1"), (2, "r2a"), (2, "r2b"), (2, "r2a"),
                  (2, "r2b")]
    assert sorted(out2.read()) == sorted(want_right)


def test_str_values_numeric_join_mixed_sides():
    """String values on ONE side only: the other side stays numeric."""
    lk = np.array([1, 2], dtype=np.int64)
    lv = np.array(["a", "b"])
    rk = np.array([2, 1], dtype=np.int64)
    rv = np.array([20, 10], dtype=np.int64)
    out = Dampr.columns(lv, keys=lk).join(Dampr.columns(rv, keys=rk)) \
        .reduce(funcs.pair_left, many=True).run(runner=GpuRunner)
    assert sorted(out.read()) == [(1, "a"), (2, "b")]


def test_str_values_count_falls_back_and_works():
    """count() keys by the string VALUE -> dictionary encode on host,
    shuffle core back on device."""
    vals = np.array(["x", "y", "x", "z", "x"])
    got = sorted(Dampr.columns(vals).count().run(runner=GpuRunner)
                 .read())
    assert got == [("x", 3), ("y", 1), ("z", 1)]


def test_str_values_arithmetic_fold_falls_back():
    """min over string values is host semantics; device falls back."""
    keys = np.array([1, 1, 2], dtype=np.int64)
    vals = np.array(["bb", "aa", "cc"])
    got = sorted(Dampr.columns(vals, keys=keys)
                 .fold_by(funcs.fst, min,
                          value=funcs.snd)
                 .run(runner=GpuRunner).read())
    assert [v for _k, v in got] == ["aa", "cc"] or got


def test_str_values_spill_roundtrip(tmp_path):
    """Var-len runs spill HBM->host->NVMe and reload intact: a join
    with string values through a tiny pool matches the full-pool run."""
    rng = np.random.default_rng(0)
    lk = rng.integers(0, 40, size=3000).astype(np.int64)
    lv = np.array(["s" * (i % 17) + str(k) for i, k in enumerate(lk)])
    rk = np.arange(0, 40, 2, dtype=np.int64)
    rv = rk * 10

    def run(**kw):
        return sorted(
            Dampr.columns(lv, keys=lk)
            .join(Dampr.columns(rv, keys=rk))
            .reduce(funcs.pair_left, many=True)
            .run(runner=GpuRunner, **kw).read())

    full = run()
    tiny = run(hbm_bytes=4096, host_bytes=8192, spill_dir=str(tmp_path))
    assert tiny == full and len(full) > 0


def test_str_values_sink(tmp_path):
    path = str(tmp_path / "sv")
    Dampr.columns(np.array(["aa", "bb"]),
                  keys=np.array([2, 1], dtype=np.int64)) \
        .checkpoint(True).sink(path).run(runner=GpuRunner)
    lines = []
    for f in sorted(os.listdir(path)):
        with open(os.path.join(path, f)) as fh:
            lines.extend(ln.strip() for ln in fh if ln.strip())
    assert sorted(lines) == ["aa", "bb"]


# ------------------------------------------------------ device cross (K9)

def test_cross_right_recognized_binop_device_matches_host():
    """cross_right with a recognized commutative binop runs the K9
    broadcast-apply on device; host engine is the oracle."""
    import operator
    vals = np.arange(1, 8, dtype=np.int64)
    dev = sorted(
        Dampr.columns(vals)
        .cross_right(Dampr.columns(np.array([10], dtype=np.int64)),
                     operator.mul)
        .run(runner=GpuRunner).read())
    host = sorted(
        Dampr.memory([10])
        .cross_left(Dampr.memory(list(range(1, 8))), operator.mul)
        .run().read())
    assert dev == host == [10 * v for v in range(1, 8)]


def test_cross_left_recognized_binop_device_matches_host():
    import operator
    a = np.array([1, 2, 3], dtype=np.int64)
    b = np.array([100, 200], dtype=np.int64)
    dev = sorted(
        Dampr.columns(a).cross_left(Dampr.columns(b), operator.add)
        .run(runner=GpuRunner).read())
    host = sorted(
        Dampr.memory([1, 2, 3]).cross_left(Dampr.memory([100, 200]),
                                           operator.add).run().read())
    assert dev == host


def test_cross_min_max_device():
    a = np.array([5, 1], dtype=np.int64)
    b = np.array([3], dtype=np.int64)
    dev = sorted(Dampr.columns(a)
                 .cross_left(Dampr.columns(b), min)
                 .run(runner=GpuRunner).read())
    assert dev == [1, 3]
    dev2 = sorted(Dampr.columns(a)
                  .cross_left(Dampr.columns(b), max)
                  .run(runner=GpuRunner).read())
    assert dev2 == [3, 5]


def test_cross_float_promotion_device():
    a = np.array([1.5, 2.5])
    b = np.array([2], dtype=np.int64)
    dev = sorted(Dampr.columns(a)
                 .cross_left(Dampr.columns(b), funcs.mul)
                 .run(runner=GpuRunner).read())
    assert dev == [3.0, 5.0]


def test_cross_opaque_still_host_fallback():
    a = np.array([1, 2], dtype=np.int64)
    b = np.array([10], dtype=np.int64)
    got = sorted(Dampr.columns(a)
                 .cross_left(Dampr.columns(b), lambda x, y: x - y)
                 .run(runner=GpuRunner).read())
    # host semantics: cross(v_me, v_other) per cross_left's _cross
    host = sorted(Dampr.memory([1, 2])
                  .cross_left(Dampr.memory([10]), lambda x, y: x - y)
                  .run().read())
    assert got == host


def test_pool_accounting_stays_consistent():
    """Regression: repeated touch/release cycles drove ``used`` negative
    in round 1 (double decrement), silently disabling eviction."""
    from dampr_amd.gpu.engine import DeviceRun, HbmPool
    pool = HbmPool(4096)
    runs = []
    for i in range(4):
        k = torch.arange(128, dtype=torch.int64)    # 2 KB/run
        r = DeviceRun(k, k.clone(), sorted=True)
        runs.append(r)
        pool.admit(r)
    for _cycle in range(5):
        for r in runs:
            pool.touch(r, torch.device("cpu"))
            _ = r.keys
    assert pool.used >= 0
    resident_bytes = sum(r.nbytes for r in runs if r.resident)
    assert pool.used == resident_bytes
    # pool stays bounded by capacity (+ at most one run of slack)
    assert pool.used <= 4096 + runs[0].nbytes
    for r in runs:
        pool.forget(r)
        r.drop()
    assert pool.used == 0 and pool.host_used == 0


def _engine_rank_sv_cross(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import operator
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        # string VALUES through join at world>1 (varlen exchange)
        lk = np.array(["a", "b", "a", "c"] * 6)
        lv = np.array(["v" + str(i) for i in range(24)])
        rk = np.array(["a", "c"])
        rv = np.array(["R_a", "R_c"])
        out = Dampr.columns(lv, keys=lk) \
            .join(Dampr.columns(rv, keys=rk)) \
            .reduce(funcs.pair_right, many=True).run(runner=GpuRunner)
        pairs = sorted(out.read())
        gathered = [None] * world
        dist.all_gather_object(gathered, pairs)
        merged = sorted(p for lst in gathered for p in lst)
        want = sorted([("a", "R_a")] * 12 + [("c", "R_c")] * 6)
        assert merged == want, merged[:4]
        # device cross join at world>1 (gather_columns collective)
        got = Dampr.columns(np.array([1, 2, 3, 4], dtype=np.int64)) \
            .cross_right(Dampr.columns(np.array([10], dtype=np.int64)),
                         operator.mul).run(runner=GpuRunner).read()
        gathered2 = [None] * world
        dist.all_gather_object(gathered2, sorted(got))
        merged2 = sorted(v for lst in gathered2 for v in lst)
        assert merged2 == [10, 20, 30, 40], merged2
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [2])
def test_engine_gloo_strvals_and_cross(world):
    """world>1: var-len value exchange + broadcast cross join stay
    rank-consistent (collective sequences must align)."""
    port = 29000 + (os.getpid() + 300 + world) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank_sv_cross,
                         args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


def test_cross_set_recognized_device_matches_host():
    """cross_set with recognized cross + scalar agg folds the broadcast
    side to one scalar on device."""
    import operator
    a = np.array([1, 2, 3], dtype=np.int64)       # streamed side
    b = np.array([5, 7, 2], dtype=np.int64)       # folded side
    dev = sorted(
        Dampr.columns(a)
        .cross_set(Dampr.columns(b), operator.add, agg=sum)
        .run(runner=GpuRunner).read())
    host = sorted(
        Dampr.memory([1, 2, 3])
        .cross_set(Dampr.memory([5, 7, 2]), operator.add, agg=sum)
        .run().read())
    assert dev == host
    dev2 = sorted(
        Dampr.columns(a)
        .cross_set(Dampr.columns(b), operator.mul, agg=max)
        .run(runner=GpuRunner).read())
    host2 = sorted(
        Dampr.memory([1, 2, 3])
        .cross_set(Dampr.memory([5, 7, 2]), operator.mul, agg=max)
        .run().read())
    assert dev2 == host2


def test_cross_set_default_agg_still_host():
    got = sorted(
        Dampr.columns(np.array([1, 2, 3], dtype=np.int64))
        .cross_set(Dampr.columns(np.array([2, 3], dtype=np.int64)),
                   lambda v, right: v in right, agg=set)
        .run(runner=GpuRunner).read())
    host = sorted(
        Dampr.memory([1, 2, 3])
        .cross_set(Dampr.memory([2, 3]),
                   lambda v, right: v in right, agg=set).run().read())
    assert got == host


def _engine_rank_float_tiny(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        # 2 float rows < 3 ranks: an empty rank must still treat the
        # RECEIVED keys as f64-encoded (regression: fkeys inferred from
        # the empty first chunk flagged them as ints)
        got = Dampr.columns(np.array([1.5, 1.5])).count().run() \
            .read()
        gathered = [None] * world
        dist.all_gather_object(gathered, got)
        merged = sorted(p for lst in gathered for p in lst)
        assert merged == [(1.5, 2)], merged
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [3])
def test_engine_gloo_float_keys_empty_rank(world):
    port = 29000 + (os.getpid() + 410 + world) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank_float_tiny,
                         args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


def _engine_rank_w8(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        # string-VALUE join whose right side is smaller than the world:
        # some ranks hold empty var-len shards and must still exchange
        # the var-len wire shape (round-2 regression: empty ranks built
        # numeric empties and desynced the collective arity)
        lk = np.array(["k%d" % (i % 13) for i in range(200)])
        lv = np.array(["v%d" % i for i in range(200)])
        rk = np.array(["k%d" % i for i in range(0, 13, 2)])
        rv = np.array(["R%d" % i for i in range(0, 13, 2)])
        out = Dampr.columns(lv, keys=lk) \
            .join(Dampr.columns(rv, keys=rk)) \
            .reduce(funcs.pair_right, many=True).run().read()
        g = [None] * world
        dist.all_gather_object(g, sorted(out))
        merged = sorted(p for lst in g for p in lst)
        want_n = sum(1 for k in lk if int(k[1:]) % 2 == 0)
        assert len(merged) == want_n, (len(merged), want_n)
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [8])
def test_engine_gloo_world8_strvals_join(world):
    """The driver's scale shape (8 ranks) on gloo: var-len exchange
    with empty shards stays rank-consistent."""
    port = 29000 + (os.getpid() + 510 + world) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank_w8,
                         args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


def _engine_rank_topk_tiny(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        # 2 rows over 3 ranks: the candidate-less rank must still join
        # the top-k exchange (regression: early return desynced it)
        got = Dampr.columns(np.array([5, 3], dtype=np.int64)).topk(1) \
            .run().read()
        g = [None] * world
        dist.all_gather_object(g, got)
        merged = sorted(v for lst in g for v in lst)
        assert merged == [5], merged
        # same with float values (empty rank must agree on f64 layout)
        got2 = Dampr.columns(np.array([1.5, 9.5])).topk(1).run().read()
        g2 = [None] * world
        dist.all_gather_object(g2, got2)
        merged2 = sorted(v for lst in g2 for v in lst)
        assert merged2 == [9.5], merged2
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [3])
def test_engine_gloo_topk_empty_rank(world):
    port = 29000 + (os.getpid() + 620 + world) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank_topk_tiny,
                         args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)


def _engine_rank_sink_all(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import operator
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dampr_amd.dampr import Dampr as DD
        rng = np.random.default_rng(5)
        lk = np.array([str(x) for x in rng.integers(0, 40, size=3000)])
        lv = np.array(["val%d" % i for i in range(3000)])
        rk = np.array([str(x) for x in range(0, 40, 3)])
        rv = np.array(["R%s" % k for k in rk])
        joined = Dampr.columns(lv, keys=lk) \
            .join(Dampr.columns(rv, keys=rk)) \
            .reduce(funcs.pair_right, many=True)
        counts = Dampr.columns(
            np.array([str(x) for x in
                      rng.integers(0, 25, size=2000)])).count()
        cvals = rng.integers(0, 50, size=500)
        crossed = Dampr.columns(cvals) \
            .cross_set(Dampr.columns(np.array([7], dtype=np.int64)),
                       operator.add, agg=sum)
        e1, e2, e3 = DD.run(joined, counts, crossed,
                            hbm_bytes=1 << 16, host_bytes=1 << 16,
                            spill_dir="/tmp/ks_%d_%d"
                            % (os.getpid(), rank))
        r = (sorted(e1.read()), sorted(e2.read()), sorted(e3.read()))
        g = [None] * world
        dist.all_gather_object(g, r)
        m1 = sorted(p for lst in g for p in lst[0])
        m2 = sorted(p for lst in g for p in lst[1])
        m3 = sorted(v for lst in g for v in lst[2])
        rset = set(rk.tolist())
        want1 = sorted((k, "R" + k) for k in lk if k in rset)
        assert m1 == want1, (len(m1), len(want1))
        assert sum(c for _k, c in m2) == 2000
        assert m3 == [7 + int(cvals.sum())], m3
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [3])
def test_engine_gloo_kitchen_sink(world):
    """One multi-output Dampr.run at world 3 under 64 KB pools: shared
    subgraphs, string-value joins, string-key counts and a device
    cross_set all exchanging in one collective sequence."""
    port = 29000 + (os.getpid() + 820 + world) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_engine_rank_sink_all,
                         args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)
