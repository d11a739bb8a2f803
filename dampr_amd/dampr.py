"""The user-facing fluent DSL.

API parity with the reference's ``dampr/dampr.py`` (reference:
dampr.py:19-977): same classes (``Dampr``, ``PMap``, ``PReduce``,
``ARReduce``, ``PJoin``, ``ValueEmitter``), same methods and signatures,
same lazy-graph semantics — consecutive maps fuse into one stage and a stage
boundary appears only at ``checkpoint()`` (or the operators that imply one).

Additions over the reference:

* ``PJoin.outer_reduce`` — a *working* full outer join (the reference's
  OuterJoin is broken dead code).
* ``PMap.concat`` — declared but never implemented in the reference
  (disabled ``_test_concat``).
"""
import itertools
import json as json_mod
import os
import logging
import operator
import random
import sys

from . import funcs
from .base import (BlockMapper, Map, MapAllJoin, MapCrossJoin, Mapper,
                   ComposedMapper, ComposedStreamable, KeyedInnerJoin,
                   KeyedLeftJoin, KeyedOuterJoin, KeyedCrossJoin,
                   KeyedReduce, PartialReduceCombiner, Reduce, Reducer,
                   StreamMapper, StreamReducer, Streamable)
from .dataset import CatDataset, Chunker
from .inputs import MemoryInput, PathInput
from .runner import Graph, MTRunner, Source

log = logging.getLogger("dampr_amd")


class ValueEmitter(object):
    """Reads values out of a finished computation."""

    def __init__(self, dataset, run_root=None):
        self.dataset = dataset
        # run-scratch root, for pruning after a late delete()
        self.run_root = run_root

    def stream(self):
        for _k, v in self.dataset.read():
            yield v

    def read(self, k=None):
        if k is None:
            return list(self.stream())
        return list(itertools.islice(self.stream(), k))

    def __iter__(self):
        return self.stream()

    def delete(self):
        self.dataset.delete()
        # the run's tree is only dirs + this output now: prune bottom-up
        # (best-effort; shared parents with live files survive the rmdir)
        if self.run_root and os.path.isdir(self.run_root):
            for dirpath, _dirs, _files in sorted(
                    os.walk(self.run_root), key=lambda w: -len(w[0])):
                try:
                    os.rmdir(dirpath)
                except OSError:
                    pass


class PBase(object):
    def __init__(self, source, pmer):
        assert isinstance(source, Source)
        self.source = source
        self.pmer = pmer

    def run(self, name=None, **kwargs):
        """Evaluate the composed graph; returns a ValueEmitter.

        The engine is picked per graph: columnar inputs
        (``Dampr.columns``) run on the device engine (gpu/engine.py);
        everything else on the multi-process host engine.  Override with
        ``runner=`` (a runner class)."""
        if name is None:
            name = "dampr/{}".format(random.random())
        runner_cls = kwargs.pop("runner", None) or \
            _pick_runner(self.pmer.graph, self.pmer.runner)
        runner = runner_cls(name, self.pmer.graph, **kwargs)
        ds = runner.run([self.source])
        return ValueEmitter(
            ds[0], run_root=getattr(
                getattr(runner, "file_system", None), "path", None))

    def read(self, k=None, **kwargs):
        """run() followed by read()."""
        return self.run(**kwargs).read(k)


def _identity(k, v):
    yield k, v


def _pick_runner(graph, explicit):
    """Engine selection: explicit wins; columnar inputs get the device
    engine; everything else the multi-process host engine.  The check is
    a sentinel attribute, NOT an isinstance against gpu.engine — importing
    torch into the parent process would bloat every forked CPU worker."""
    if explicit is not None:
        return explicit
    if any(getattr(d, "dampr_columnar", False)
           for d in graph.inputs.values()):
        from .gpu.engine import GpuRunner
        return GpuRunner
    return MTRunner


class PMap(PBase):
    """A (possibly fused) chain of map operations."""

    def __init__(self, source, pmer, agg=None, agg_specs=None):
        super(PMap, self).__init__(source, pmer)
        self.agg = agg or []
        # device specs of pending (fusable) maps, parallel to ``agg``;
        # None for opaque lambdas
        self.agg_specs = agg_specs or []

    def run(self, name=None, **kwargs):
        if self.agg:
            return self.checkpoint().run(name, **kwargs)
        return super(PMap, self).run(name, **kwargs)

    # -- fusion ------------------------------------------------------------

    def _add_mapper(self, mapper, spec=None):
        assert isinstance(mapper, Streamable)
        return PMap(self.source, self.pmer, self.agg + [mapper],
                    self.agg_specs + [spec])

    def _add_map(self, f, spec=None):
        return self._add_mapper(Map(f), spec)

    def checkpoint(self, force=False, combiner=None, options=None):
        """Fuse the pending maps into one stage; shares the materialized
        result among downstream consumers."""
        if self.agg or force:
            aggs = self.agg[:] if self.agg else [Map(_identity)]
            if not self.agg:
                # pure materialization point: free on the device engine
                options = dict(options or {})
                options.setdefault("device_map", ("identity",))
            elif self._only_filters() and combiner is None:
                # a run of recognized predicates: one conjunction stage
                options = dict(options or {})
                options.setdefault(
                    "device_map",
                    ("filter", tuple(s[1] for s in self.agg_specs)))
            name = "Stage {}: %s" % " -> ".join(str(a) for a in aggs)
            source, pmer = self.pmer._add_mapper(
                [self.source], fuse(aggs), combiner=combiner, name=name,
                options=options)
            return PMap(source, pmer)
        return self

    def _only_filters(self):
        """Is every pending map a recognized filter predicate?"""
        return bool(self.agg_specs) and all(
            isinstance(s, tuple) and s[0] == "filter_clause"
            for s in self.agg_specs)

    def _filters_lowered(self):
        """This collection with pending recognized filters checkpointed
        into their own device filter stage, so the operator that follows
        sees nothing pending and keeps its device form.  Only on graphs
        with a columnar input (the sentinel ``_pick_runner`` reads); the
        host engine gets no extra stage."""
        if self._only_filters() and any(
                getattr(d, "dampr_columnar", False)
                for d in self.pmer.graph.inputs.values()):
            return self.checkpoint()
        return self

    # -- low/medium-level hooks ---------------------------------------------

    def custom_mapper(self, mapper, name=None, **options):
        """Attach a user Mapper instance directly (does not fuse)."""
        if isinstance(mapper, Streamable):
            return self._add_mapper(mapper)
        assert isinstance(mapper, Mapper)
        name = name or str(mapper)
        me = self.checkpoint()
        source, pmer = me.pmer._add_mapper([me.source], mapper, name=name,
                                           options=options)
        return PMap(source, pmer)

    def custom_reducer(self, reducer, name=None, **options):
        """Attach a user Reducer instance directly."""
        assert isinstance(reducer, Reducer)
        me = self.checkpoint(force=True)
        name = name or str(reducer)
        source, pmer = me.pmer._add_reducer([me.source], reducer, name=name,
                                            options=options)
        return PMap(source, pmer)

    def partition_map(self, f, **options):
        """Map over a whole partition iterator; runs on empty partitions
        too."""
        return self.custom_mapper(StreamMapper(f), **options)

    def partition_reduce(self, f, **options):
        """Reduce over a whole partition's (key, values) iterator; runs on
        empty partitions too."""
        return self.custom_reducer(StreamReducer(f), **options)

    # -- record-level operators ---------------------------------------------

    def map(self, f):
        """Map each value with f."""
        def _map(k, v):
            yield k, f(v)
        return self._add_map(_map)

    def map_values(self, f):
        """Map the second element of two-tuple values."""
        def _map_values(k, v):
            yield k, (v[0], f(v[1]))
        return self._add_map(_map_values)

    def map_keys(self, f):
        """Map the first element of two-tuple values."""
        def _map_keys(k, v):
            yield k, (f(v[0]), v[1])
        return self._add_map(_map_keys)

    def prefix(self, f):
        """value -> (f(value), value)."""
        def _prefix(k, v):
            yield k, (f(v), v)
        return self._add_map(_prefix)

    def suffix(self, f):
        """value -> (value, f(value))."""
        def _suffix(k, v):
            yield k, (v, f(v))
        return self._add_map(_suffix)

    def filter(self, f):
        """Keep values where f(value) is true.

        A predicate object from ``dampr_amd.funcs`` (``gt``, ``ge``,
        ``lt``, ``le``, ``eq``, ``ne``, ``between``, ``startswith``, each
        with an optional ``on=funcs.fst`` / ``funcs.snd``) is recognized:
        on the columnar engine a run of consecutive such filters evaluates
        as one conjunction in the device compaction kernels, and the
        ``count``, ``a_group_by``, ``sort_by``, ``mean``, ``len``, ``topk``
        or ``sink`` that follows keeps its device form.  Numeric constants
        compare against numeric columns; ``str`` constants (up to 64 UTF-8
        bytes) compare against string value columns byte-wise, which is
        Python's ``str`` order, and against string keys through their
        ranks.  A chain may mix both kinds.  ``funcs.isin(values)`` and
        ``funcs.notin(values)`` test membership in a set of ints, floats,
        bools and strs of any length: the kernels probe a device hash set,
        and a member of another kind than the column simply never matches,
        as in Python.  Any other callable, and any
        pairing of constant and column kinds that Python would not
        compare, runs on the host, record by record."""
        def _filter(k, v):
            if f(v):
                yield k, v
        clause = funcs.filter_clause(f) or funcs.filter_str_clause(f)
        return self._add_map(
            _filter, ("filter_clause", clause) if clause else None)

    def flat_map(self, f):
        """Map each value to an iterable and flatten.  Recognized
        ``funcs.tokenize_set`` marks the stage for the fused text
        document-frequency lowering on the device engine."""
        def _flat_map(k, v):
            for vi in f(v):
                yield k, vi
        spec = "flat_tokenize_set" if f is funcs.tokenize_set else None
        return self._add_map(_flat_map, spec)

    def sample(self, prob):
        """Uniformly keep each record with probability ``prob``."""
        assert 0 <= prob <= 1.0

        def _sample(k, v):
            if _get_rand().random() < prob:
                yield k, v
        return self._add_map(_sample)

    def inspect(self, prefix="", exit=False):
        """Debug passthrough that prints each value."""
        def _inspect(k, v):
            print("{}: {}".format(prefix, v))
            yield k, v
        ins = self._add_map(_inspect)
        if exit:
            ins.run()
            sys.exit(0)
        return ins

    # -- grouping -----------------------------------------------------------

    def group_by(self, key, vf=lambda x: x):
        """Group by key(value); general (non-associative) reductions."""
        def _group_by(_k, value):
            yield key(value), vf(value)
        pm = self._add_map(_group_by).checkpoint()
        return PReduce(pm.source, pm.pmer)

    def a_group_by(self, key=None, vf=None):
        """Group by key(value) for *associative* reductions: enables the
        map-side partial reduce (combiner), which is the fast path — on GPU
        it lowers to the device hash-combine kernel (K6).

        When ``key``/``vf`` are recognized named funcs (dampr_amd.funcs,
        e.g. the defaults) AND this PMap has no pending opaque maps, the
        stage carries a device spec so the columnar engine (gpu/engine.py)
        runs it on the CDNA4 kernels."""
        key = funcs.identity if key is None else key
        vf = funcs.identity if vf is None else vf

        def _a_group_by(_k, value):
            yield key(value), vf(value)
        kname = funcs.column_func_name(key)
        vname = funcs.column_func_name(vf)
        dev_map = None
        me = self._filters_lowered()
        if kname and vname and not me.agg:
            dev_map = ("kv", kname, vname)
        elif (kname == "identity" and vname == "one"
              and me.agg_specs == ["flat_tokenize_set"]):
            # text df idiom: flat_map(tokenize_set).count() fuses into
            # the one-pass doc-frequency kernel on TextSource inputs
            dev_map = ("text_df",)
        # No checkpoint: ARReduce attaches the combiner to this stage.
        return ARReduce(me._add_map(_a_group_by), device_map=dev_map)

    def fold_by(self, key, binop, value=None, **options):
        """a_group_by(key, value).reduce(binop)."""
        return self.a_group_by(key, value).reduce(binop, **options)

    def sort_by(self, key=None, **options):
        """Totally order the collection by key(value).  Recognized key
        funcs lower to the device radix sort (K3)."""
        key = funcs.identity if key is None else key

        def _sort_by(_k, value):
            yield key(value), value
        kname = funcs.column_func_name(key)
        me = self._filters_lowered()
        if kname and not me.agg:
            options = dict(options)
            options.setdefault("device_map", ("kv", kname, "identity"))
        return me._add_map(_sort_by).checkpoint(options=options)

    def count(self, key=None, **options):
        """Count occurrences by key(value)."""
        return self.a_group_by(key, funcs.one) \
                   .reduce(operator.add, **options)

    def mean(self, key=None, value=None, **options):
        """Mean of value(v) grouped by key(v).

        Recognized key/value funcs lower the whole chain to device: the
        segmented-reduce kernel computes sum and count, the average fuses
        into the same stage, and the trailing host ``_average`` map is
        tagged device-identity (the division already happened on device)."""
        key = funcs.one if key is None else key
        value = funcs.identity if value is None else value

        def _mean_binop(x, y):
            return x[0] + y[0], x[1] + y[1]

        def _average(x):
            return (x[0], x[1][0] / float(x[1][1]))

        me = self._filters_lowered()
        ar = me.a_group_by(key, lambda v: (value(v), 1))
        kname = funcs.column_func_name(key)
        vname = funcs.column_func_name(value)
        dev = None
        if kname and vname and ar._device_map is None and not me.agg:
            # a_group_by saw the opaque tuple lambda; re-tag with the
            # device form (plain value column; reduce computes the mean)
            ar._device_map = ("kv", kname, vname)
            dev = ("mean",)
        pm = ar._run(_mean_binop, dev, 1000, options)
        out = pm.map(_average)
        if dev is not None:
            return out.checkpoint(options={"device_map": ("identity",)})
        return out

    def len(self):
        """Number of records in the collection."""
        def _map_count(items):
            count = 0
            for _ in items:
                count += 1
            yield 1, count

        def _reduce_count(groups):
            count = 0
            seen = False
            for _k, counts in groups:
                seen = True
                for c in counts:
                    count += c
            if seen:
                yield 1, count

        me = self._filters_lowered()
        if me.agg:
            return self.partition_map(_map_count) \
                       .partition_reduce(_reduce_count) \
                       .map(lambda x: x[1])
        # no pending opaque maps: the device engine answers from run
        # lengths without reading any data
        me = me._add_mapper(StreamMapper(_map_count)) \
            .checkpoint(options={"device_map": ("len_local",)})
        source, pmer = me.pmer._add_reducer(
            [me.source], StreamReducer(_reduce_count),
            options={"device_reduce": ("sum",)})
        out = PMap(source, pmer).map(lambda x: x[1])
        return out.checkpoint(options={"device_map": ("unkey",)})

    def topk(self, k, value=None):
        """Top-k values ordered by value(x) (K11).

        ``value=None`` (natural order) on columnar inputs lowers to the
        device path: per-partition radix top-k candidates, single-partition
        final merge."""
        lowered = self._filters_lowered()
        device_ok = value is None and not lowered.agg
        if value is None:
            value = lambda x: x
        import heapq

        def map_topk(it):
            heap = []
            for x in it:
                heapq.heappush(heap, (value(x), x))
                if len(heap) > k:
                    heapq.heappop(heap)
            return ((1, x) for x in heap)

        def reduce_topk(it):
            candidates = (v for _k, vit in it for v in vit)
            for _score, x in heapq.nlargest(k, candidates):
                yield x, 1

        if not device_ok:
            return self.partition_map(map_topk) \
                       .partition_reduce(reduce_topk) \
                       .map(lambda x: x[0])
        me = lowered._add_mapper(StreamMapper(map_topk)) \
            .checkpoint(options={"device_map": ("topk_local", k)})
        source, pmer = me.pmer._add_reducer(
            [me.source], StreamReducer(reduce_topk),
            options={"device_reduce": ("topk_global", k)})
        out = PMap(source, pmer).map(lambda x: x[0])
        return out.checkpoint(options={"device_map": ("identity",)})

    # -- multi-graph operators ----------------------------------------------

    def join(self, other):
        """Reduce-side equi-join with another grouped computation."""
        assert isinstance(other, PBase)
        me = self.checkpoint(True)
        if isinstance(other, PMap):
            other = other.checkpoint(True)
        pmer = Dampr(me.pmer.graph.union(other.pmer.graph))
        return PJoin(me.source, pmer, other.source)

    def concat(self, other):
        """Concatenate two collections (new: the reference declares but
        never implements this)."""
        assert isinstance(other, PMap)
        me = self.checkpoint()
        other = other.checkpoint()
        pmer = Dampr(me.pmer.graph.union(other.pmer.graph))
        source, pmer = pmer._add_mapper(
            [me.source, other.source], Map(_identity),
            name="Stage {}: Concat", options={"concat": True})
        return PMap(source, pmer)

    def cross_left(self, other, cross, memory=False, **options):
        """Cross product; self is the left side.  When ``cross`` is a
        recognized commutative binop (funcs.CROSS_BINOPS) the columnar
        engine broadcasts the small side and fuses the apply on device
        (K9)."""
        def _cross(k1, v1, k2, v2):
            yield k1, cross(v2, v1)

        cname = funcs.cross_binop_name(cross)
        if cname:
            options = dict(options)
            options.setdefault("device_map", ("cross", cname))
        me = self.checkpoint()
        other = other.checkpoint()
        pmer = Dampr(me.pmer.graph.union(other.pmer.graph))
        source, pmer = pmer._add_mapper(
            [other.source, me.source], MapCrossJoin(_cross, cache=memory),
            combiner=None, name="Stage {}: Cross", options=options)
        return PMap(source, pmer)

    def cross_right(self, other, cross, memory=False):
        """Cross product; self is the right side.  With ``memory=True`` the
        small side is cached (GPU path: broadcast, K9)."""
        assert isinstance(other, PMap)
        cname = funcs.cross_binop_name(cross)
        kw = {"device_map": ("cross", cname)} if cname else {}
        return other.cross_left(self, lambda xi, yi: cross(yi, xi),
                                memory, **kw)

    def cross_set(self, other, cross, agg=None, **options):
        """Cross each value against the whole of ``other``, aggregated once
        by ``agg`` (default list).  With a recognized commutative
        ``cross`` (funcs.CROSS_BINOPS) AND a recognized scalar ``agg``
        (sum/min/max), the columnar engine folds the broadcast side to
        one scalar on device and fuses the apply (K9)."""
        def _cross(k1, v1, right):
            yield k1, cross(v1, right)

        cname = funcs.cross_binop_name(cross)
        aname = funcs.set_agg_name(agg) if agg is not None else None
        if cname and aname:
            options = dict(options)
            options.setdefault("device_map",
                               ("cross_set", cname, aname))
        if agg is None:
            agg = list

        def _aggregate(d):
            return agg(v for _k, v in d)

        me = self.checkpoint()
        other = other.checkpoint()
        pmer = Dampr(me.pmer.graph.union(other.pmer.graph))
        source, pmer = pmer._add_mapper(
            [other.source, me.source], MapAllJoin(_cross, _aggregate),
            combiner=None, name="Stage {}: CrossAll", options=options)
        return PMap(source, pmer)

    # -- caching and sinks --------------------------------------------------

    def cached(self, **options):
        """Materialize this subgraph in memory for reuse."""
        options["memory"] = True
        return self.checkpoint(options=options)

    def sink(self, path):
        """Write each value (assumed str) as a line into part files under
        ``path``; exempt from cleanup."""
        # No pending opaque maps -> the columnar engine can format the
        # value column on device (tfidf.py's tsv kernels are the model).
        me = self._filters_lowered()
        options = {"device_sink": "values"} if not me.agg else None
        aggs = me.agg[:] if me.agg else [Map(_identity)]
        name = "Stage {}: %s" % " -> ".join(str(a) for a in aggs)
        source, pmer = me.pmer._add_sink(
            [me.source], fuse(aggs), path=path, name=name,
            options=options)
        return PMap(source, pmer)

    def sink_tsv(self, path):
        """Format tuples as TSV lines, then sink."""
        return self.map(
            lambda x: u"\t".join(str(p) for p in x)).sink(path)

    def sink_json(self, path):
        """Serialize values as line-delimited JSON, then sink."""
        return self.map(json_mod.dumps).sink(path)


class ARReduce(object):
    """Associative reductions (map-side partial reduce enabled)."""

    def __init__(self, pmap, device_map=None):
        self.pmap = pmap
        self._device_map = device_map

    def _run(self, binop, dev_reduce, reduce_buffer, options):
        def _reduce(key, vs):
            acc = next(vs)
            for v in vs:
                acc = binop(acc, v)
            return acc

        options.update({"binop": binop, "reduce_buffer": reduce_buffer})
        if self._device_map is not None and dev_reduce is not None:
            options["device_map"] = self._device_map
        pm = self.pmap.checkpoint(
            True, combiner=PartialReduceCombiner(Reduce(_reduce)),
            options=options)
        red_opts = None
        if self._device_map is not None and dev_reduce is not None:
            red_opts = {"device_reduce": dev_reduce}
        return PReduce(pm.source, pm.pmer).reduce(_reduce,
                                                  options=red_opts)

    def reduce(self, binop, reduce_buffer=None, **options):
        """Reduce each group with an associative binop.  ``reduce_buffer``
        caps the map-side combine dictionary (distinct keys held in memory
        before a spill) — unlike the reference, it is honored (SURVEY.md
        §2.5); the default is ``settings.reduce_buffer``, a backstop
        under the RSS watermark so high-cardinality keys cannot grow an
        unbounded per-worker dict between amortized RSS checks.
        Recognized binops (operator.add, min, max — dampr_amd.funcs)
        lower to the device segmented-reduce kernel on the columnar
        engine."""
        name = funcs.binop_name(binop)
        return self._run(binop, (name,) if name else None, reduce_buffer,
                         options)

    def first(self, **options):
        """First value seen per key."""
        return self._run(lambda x, _y: x, ("first",), None, options)

    def sum(self, **options):
        """Sum of values per key."""
        return self._run(operator.add, ("sum",), None, options)


class PReduce(PBase):
    """General grouped reductions."""

    def reduce(self, f, options=None):
        """Reduce each group with ``f(key, iter values) -> value``."""
        source, pmer = self.pmer._add_reducer([self.source], KeyedReduce(f),
                                              options=options)
        return PMap(source, pmer)

    def unique(self, key=lambda x: x):
        """Distinct values per group, by key(value)."""
        def _uniq(_k, it):
            seen = set()
            out = []
            for v in it:
                fv = key(v)
                if fv not in seen:
                    seen.add(fv)
                    out.append(v)
            return out

        return self.reduce(_uniq)

    def join(self, other):
        """Join with another grouped computation."""
        assert isinstance(other, PBase)
        if isinstance(other, PMap):
            other = other.checkpoint(True)
        pmer = Dampr(self.pmer.graph.union(other.pmer.graph))
        return PJoin(self.source, pmer, other.source)

    def partition_reduce(self, f):
        source, pmer = self.pmer._add_reducer([self.source],
                                              StreamReducer(f))
        return PMap(source, pmer)


class PJoin(PBase):
    """Joins between two co-grouped computations (K8)."""

    def __init__(self, source, pmer, right):
        super(PJoin, self).__init__(source, pmer)
        self.right = right

    def run(self, name=None, **kwargs):
        return self.reduce(
            lambda l, r: (list(l), list(r))).run(name, **kwargs)

    def reduce(self, aggregate, many=False):
        """Inner join; aggregate(left_iter, right_iter).  ``many=True``
        flattens an iterable result into separate records.

        ``funcs.pair_sum/pair_product/pair_left/pair_right`` with
        ``many=True`` lower to the device hash-join kernel (K8) on the
        columnar engine."""
        def _reduce(_k, left, right):
            return aggregate(left, right)

        options = None
        pname = funcs.join_pair_name(aggregate)
        if pname and many:
            options = {"device_reduce": ("join", "inner"),
                       "device_join_pair": pname}
        source, pmer = self.pmer._add_reducer(
            [self.source, self.right], KeyedInnerJoin(_reduce, many),
            options=options)
        return PMap(source, pmer)

    def left_reduce(self, aggregate):
        """Left join; missing right groups get an empty iterator."""
        def _reduce(_k, left, right):
            return aggregate(left, right)

        source, pmer = self.pmer._add_reducer(
            [self.source, self.right], KeyedLeftJoin(_reduce))
        return PMap(source, pmer)

    def outer_reduce(self, aggregate):
        """Full outer join (new: the reference's outer join is broken dead
        code — reference: base.py:337-366)."""
        def _reduce(_k, left, right):
            return aggregate(left, right)

        source, pmer = self.pmer._add_reducer(
            [self.source, self.right], KeyedOuterJoin(_reduce))
        return PMap(source, pmer)

    def _cross(self, crosser):
        def _crossf(k1, v1, _k2, v2):
            return k1, crosser(v1, v2)

        source, pmer = self.pmer._add_reducer(
            [self.source, self.right], KeyedCrossJoin(_crossf))
        return PMap(source, pmer).map(lambda x: x[1])


class Dampr(object):
    """Entry points for building pipelines."""

    def __init__(self, graph=None, runner=None):
        self.graph = graph if graph is not None else Graph()
        self.runner = runner          # None = auto (see _pick_runner)

    @classmethod
    def memory(cls, items, partitions=50):
        """Pipeline over an in-memory list."""
        mi = MemoryInput(list(enumerate(items)), partitions)
        source, ng = Graph().add_input(mi)
        return PMap(source, cls(ng))

    @classmethod
    def device_text(cls, data):
        """Newline-delimited text for the device engine: a path, bytes,
        or a u8 numpy array.  ``device_text(p).flat_map(funcs.tokenize_set)
        .count()`` runs as the fused single-pass document-frequency kernel
        (the flagship TF-IDF path) on an MI355X; the same pipeline runs on
        the host fallback elsewhere."""
        from .gpu.engine import TextSource
        source, ng = Graph().add_input(TextSource(data))
        return PMap(source, cls(ng))

    @classmethod
    def columns(cls, vals, keys=None):
        """Pipeline over typed columns (numpy arrays / torch tensors of
        int64 or float64): records are (key_i, val_i), keys default to the
        row index.  Runs on the device engine — built-in ops (count, sum,
        fold_by with recognized binops, joins, first, ...) execute as
        gfx950 kernels over HBM-resident columns.

        ``keys`` may be int64, float64 (order-preserving IEEE encode at
        ingest), or a string array/list — strings dictionary-encode
        (sorted table, rank ids) and run on the same kernels; joins
        across different vocabularies remap through the union
        dictionary on device.

        ``vals`` may also be a string array/list: var-len values ride a
        device byte arena (blob + offsets) through partition, sort,
        spill, exchange and join — only keys compare on device
        (SURVEY.md §7).  Gather-only ops (first, sort_by, join with
        pair_left/pair_right) stay on the kernels; arithmetic folds
        over string values fall back to host records per stage.
        Keying by a string value (``count()``, ``a_group_by()``,
        ``sort_by()`` over a column of words) is a device path too: the
        column dictionary-encodes on device (string hash, radix sort,
        byte-verified segment heads; exact even under hash collisions)
        and only the distinct strings visit the host, to be ordered
        into the dictionary.  At world > 1 that stage still runs on
        host records.

        ``filter`` with a ``funcs`` predicate (``gt``, ``ge``, ``lt``,
        ``le``, ``eq``, ``ne``, ``between``; ``on=funcs.fst`` /
        ``funcs.snd`` for the key or value of grouped records) is a device
        stage as well: a stable compaction over int64, float64 and
        float-key columns that keeps the operator after it on the
        kernels, e.g. ``columns(v).filter(funcs.gt(0)).count()`` or
        ``columns(words).count().filter(funcs.ge(5, on=funcs.snd))``.
        With ``str`` constants (at most 64 UTF-8 bytes) the same
        predicates, and ``funcs.startswith``, filter a string value
        column by its bytes and a string key column by its keys' ranks:
        ``columns(words).filter(funcs.ge("m")).count()`` or
        ``columns(words).count().filter(funcs.startswith("m",
        on=funcs.fst))``.  A number against a string column or a string
        against a numeric one, longer string constants, constants an int
        column cannot hold (NaN, infinite, beyond 64 bits) and plain
        lambdas run that stage on host records.

        Numeric domain: typed columns use fixed-width i64/f64
        arithmetic — integer aggregates wrap at 64 bits, where the host
        engine's Python ints are arbitrary precision.  Pipelines whose
        sums exceed +/-2**63 belong on the host engine."""
        from .gpu.engine import ColumnSource
        src_obj = ColumnSource.from_data(vals, keys)
        source, ng = Graph().add_input(src_obj)
        return PMap(source, cls(ng))

    @classmethod
    def read_input(cls, *datasets):
        """Pipeline over custom Dataset/Chunker taps."""
        if len(datasets) == 1:
            ds = datasets[0]
        else:
            ds = CatDataset(list(datasets))
        source, ng = Graph().add_input(ds)
        return PMap(source, cls(ng))

    @classmethod
    def text(cls, fname, chunk_size=16 * 1024 ** 2, followlinks=False):
        """Pipeline over newline-delimited files/dirs/globs."""
        return cls.read_input(PathInput(fname, chunk_size, followlinks))

    @classmethod
    def json(cls, *args, **kwargs):
        """text() then json-decode each line."""
        return cls.text(*args, **kwargs).map(json_mod.loads)

    @classmethod
    def from_dataset(cls, dataset):
        """Pipeline over a raw stage-output dataset."""
        assert isinstance(dataset, Chunker)
        source, ng = Graph().add_input(dataset)
        return PMap(source, cls(ng))

    @classmethod
    def run(cls, *pmers, **kwargs):
        """Run several pipelines as ONE merged DAG; shared checkpointed
        subgraphs execute once.  Returns one ValueEmitter per input."""
        assert len(pmers) > 0, "Need at least one graph to run!"
        sources = []
        graph = None
        last = None
        for i, pmer in enumerate(pmers):
            if isinstance(pmer, PMap):
                pmer = pmer.checkpoint()
            elif isinstance(pmer, PJoin):
                pmer = pmer.reduce(lambda l, r: (list(l), list(r)))
            graph = pmer.pmer.graph if graph is None \
                else pmer.pmer.graph.union(graph)
            sources.append(pmer.source)
            last = pmer
        name = kwargs.pop("name", "dampr/{}".format(random.random()))
        runner_cls = kwargs.pop("runner", None) or \
            _pick_runner(graph, last.pmer.runner)
        runner = runner_cls(name, graph, **kwargs)
        ds = runner.run(sources)
        root = getattr(getattr(runner, "file_system", None), "path", None)
        return [ValueEmitter(d, run_root=root) for d in ds]

    def _add_mapper(self, *args, **kwargs):
        output, ng = self.graph.add_mapper(*args, **kwargs)
        return output, Dampr(ng)

    def _add_reducer(self, *args, **kwargs):
        output, ng = self.graph.add_reducer(*args, **kwargs)
        return output, Dampr(ng)

    def _add_sink(self, *args, **kwargs):
        output, ng = self.graph.add_sink(*args, **kwargs)
        return output, Dampr(ng)


def fuse(aggs):
    """Compose a fused mapper chain into a single Mapper."""
    if len(aggs) == 1:
        return aggs[0]
    s = aggs[1]
    for i in range(2, len(aggs)):
        s = ComposedStreamable(s, aggs[i])
    return ComposedMapper(aggs[0], s)


_RANDOM = None


def _get_rand():
    global _RANDOM
    if _RANDOM is None:
        import time
        _RANDOM = random.Random(time.time())
    return _RANDOM
