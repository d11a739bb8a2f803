"""The device dataflow engine: executes DSL plans (runner.Graph) over
columnar record batches resident in HBM.

Architecture (MI355X-first, no translation of the reference's process
pools):

* Records are **typed columns** — an i64 key column + an i64/f64 value
  column — not streams of pickled Python objects.  This is the layout the
  CDNA4 kernels (ops/hip/*.hip) operate on: radix sort (K2/K3), segmented
  reduce (K5/K7), hash join (K8), top-k (K11).  Pipelines over arbitrary
  Python objects belong to the host engine (runner.MTRunner), which is the
  complete, conformance-tested implementation of the same plans; pipelines
  over text use the tokenizer/string-dict specialization (gpu/tfidf.py).
* A stage lowers to device kernels when the DSL built it from *recognized*
  functions (dampr_amd.funcs); anything else falls back per-stage to the
  host operators with decode/encode at the boundary (SURVEY.md §7 "hard
  parts": opaque UDFs run on the host, the shuffle/sort/combine core stays
  on device).
* Out-of-core: runs live in an ``HbmPool`` with two watermarks; least
  recently used runs spill to pinned host memory and on to raw NVMe
  files, paging back when read — the reference's RSS-watermark spill
  files (dampr/memory.py, dataset.py:190-262) re-expressed over HBM →
  host → disk tiers.  The pool is the runs' one owner: the engine
  builds a run with ``_new_run`` (``DeviceRun`` + ``pool.admit``), reads
  it only through ``pool.columns(run, device)``, whose two references
  outlive a later eviction, asks ``run.n`` / ``nbytes`` / ``vdtype`` /
  ``has_sv`` for what a run on any tier holds, and gives it up with
  ``pool.free(run)``.  Pass-through stores share run objects, so a
  stage frees a consumed run only when no store outside the stage
  holds it (``_live_ids``, ``_free_consumed``).  Single-rank columnar
  ingest is *lazy*: batched
  unrouted runs, streamed run-by-run through record-wise stages; only
  key-colocating stages (reduce/join) route to hash partitions, and a
  skewed partition larger than half the pool reduces run-by-run with an
  associative re-reduce.  Only the active working set must be resident,
  so jobs scale past device memory.
* Multi-GPU: after every partitioning map stage the engine exchanges
  partitions to their owning rank over RCCL all-to-all (xGMI); partition p
  is owned by rank ``p % world`` (parallel/shuffle.py).

This module is the plan interpreter (``GpuRunner``).  The input, store and
result types live in gpu/stores.py and the tiered run storage
(``DeviceRun``, ``HbmPool``) in gpu/pool.py; both are re-exported here.
The host record <-> column format of the fallback boundary (classify,
agree across ranks, build, decode) lives in gpu/records.py.
"""
import logging
import os

import torch

from .. import settings
from ..runner import GMap, GReduce, GSink, RunnerBase
from . import records as record_format
from .backend import ops_for
from .filters import _filter_programs
from .pool import DeviceRun, HbmPool
from .stores import (ColumnDataset, ColumnSource, HostStore, PartStore,
                     SinkStore, StrTable, TextSource, TokenColumnDataset,
                     TokenStore, _cat_vals, _is_sv, _store_has_sv,
                     encode_f64_sortable)

__all__ = ["GpuRunner", "DeviceRun", "HbmPool", "PartStore", "ColumnSource",
           "TextSource"]

log = logging.getLogger("dampr_amd")

# elementwise pair ops shared by the cross maps and the join pair fold
_BINOPS = {"add": torch.add, "mul": torch.mul,
           "min": torch.minimum, "max": torch.maximum}


def _any_flag(ins, field):
    """Does any input store set this metadata flag?  A stage's inputs are
    stores, except that a text input reaches its first stage as the
    ``TextSource`` itself, which carries no store metadata."""
    return any(getattr(s, field) for s in ins
               if not isinstance(s, TextSource))


def _declared(ins, field, default=None):
    """The first value any input store declares for a metadata field
    (``vdtype``, ``str_table``).  Store metadata is identical on every
    rank, so e.g. a rank with no local rows builds its empty exchange
    columns with the value dtype the other ranks send."""
    return next((getattr(s, field) for s in ins
                 if not isinstance(s, TextSource)
                 and getattr(s, field) is not None), default)


def _extend_store(out, part):
    """Append ``part``'s runs to ``out``, partition by partition, and
    return ``out``; with no ``out`` yet (None), ``part`` becomes it."""
    if out is None:
        return part
    for q, runs in part.items():
        out.setdefault(q, []).extend(runs)
    return out


class GpuRunner(RunnerBase):
    """Interprets a runner.Graph over device columns.

    Stage dispatch: ``stage.options["device_map"] / ["device_reduce"]``
    descriptors (attached by the DSL when built from recognized funcs)
    select a handler from ``_MAP_HANDLERS`` / ``_REDUCE_HANDLERS`` that
    runs on the kernels; untagged stages run the host operators with a
    decode/encode boundary (records must stay numeric scalars).
    """

    def __init__(self, name, graph, device=None, n_partitions=None,
                 hbm_bytes=None, host_bytes=None, spill_dir=None):
        # note: RunnerBase.__init__ builds a /tmp FileSystem we don't use;
        # keep it for interface parity (sinks reuse its naming).
        super(GpuRunner, self).__init__(name, graph)
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.ops = ops_for(self.device)
        cap = hbm_bytes or settings.hbm_pool_mb * (1 << 20)
        host_cap = host_bytes if host_bytes is not None \
            else settings.host_pool_mb * (1 << 20)
        self.pool = HbmPool(cap, host_capacity=host_cap,
                            spill_dir=spill_dir)
        if torch.distributed.is_available() and \
                torch.distributed.is_initialized():
            self.world = torch.distributed.get_world_size()
            self.rank = torch.distributed.get_rank()
        else:
            self.world, self.rank = 1, 0
        self.exchanged_rows = 0
        # rows dictionary-encoded by the string-key kv map
        self._dict_encode_rows = 0
        # global uniques ranked on device by the string-key kv map
        self._str_rank_rows = 0
        # rows the device filter stages read and kept
        self._filter_rows_in = 0
        self._filter_rows_kept = 0
        # per-stage state set by run(): which inputs the running stage
        # consumes for the last time, and the ids of runs that stores
        # outside the stage still share
        self._consume_flags = None
        self._stage_live = frozenset()
        self._side_stream = (torch.cuda.Stream(device=self.device)
                             if self.device.type == "cuda" else None)
        # separate D2H stream: spills and prefetches use the DMA
        # engines in both directions concurrently with compute
        self.pool.spill_stream = (torch.cuda.Stream(device=self.device)
                                  if self.device.type == "cuda" else None)
        if n_partitions:
            self.n_partitions = n_partitions
        elif self.world == 1 and self._inputs_fit(cap):
            # single rank, everything resident: one partition means one
            # full-device sort/reduce per stage instead of 64 small ones
            # (the kernels are whole-device parallel; partitions exist
            # for out-of-core paging and the cross-rank exchange)
            self.n_partitions = 1
        else:
            self.n_partitions = settings.gpu_partitions

    def _inputs_fit(self, cap):
        total = 0
        for inp in self.graph.inputs.values():
            if isinstance(inp, ColumnSource):
                total += inp.keys.numel() * 8 + \
                    inp.vals.element_size() * inp.vals.numel()
            elif isinstance(inp, TextSource):
                total += inp.nbytes
            else:
                return False             # unknown size: keep partitions
        return total * 4 < cap           # headroom for intermediates

    # -- plan walk ---------------------------------------------------------

    def run(self, outputs, cleanup=True):
        from ..utils.trace import get_trace, trace_stage
        get_trace().clear()
        data = {}
        # consumer refcounts: a store is freed after its LAST consuming
        # stage (keeps true >HBM jobs from pinning dead intermediates)
        consumers = {}
        for stage in self.graph.stages:
            for src in stage.inputs:
                consumers[src] = consumers.get(src, 0) + 1
        for src in outputs:
            consumers[src] = consumers.get(src, 0) + 1
        for src, inp in self.graph.inputs.items():
            with trace_stage("ingest {}".format(src), self.device):
                data[src] = self._ingest(inp)
        for stage_id, stage in enumerate(self.graph.stages):
            log.info("[device] Stage %s/%s: %r", stage_id + 1,
                     len(self.graph.stages), stage)
            ins = [data[i] for i in stage.inputs]
            # consume-as-you-go: inputs whose LAST consumer is this
            # stage may free each partition right after it is reduced /
            # joined (out-of-core jobs would otherwise re-evict dead
            # partition data until stage-end cleanup)
            self._consume_flags = [
                cleanup and consumers.get(src, 0) ==
                stage.inputs.count(src) and src not in outputs
                for src in stage.inputs]
            self._stage_live = self._live_ids(data, set(stage.inputs))
            with trace_stage(repr(stage), self.device):
                if isinstance(stage, GMap):
                    out = self.run_map(stage, ins)
                elif isinstance(stage, GReduce):
                    out = self.run_reduce(stage, ins)
                elif isinstance(stage, GSink):
                    out = self.run_sink(stage, ins)
                else:
                    raise TypeError(stage)
            data[stage.output] = out
            if cleanup:
                for src in set(stage.inputs):
                    consumers[src] -= stage.inputs.count(src)
                    if consumers.get(src, 0) <= 0:
                        self._free_store(data.get(src),
                                         self._live_ids(data, {src}))
                        data[src] = PartStore()
        rets = []
        for source in outputs:
            store = data[source]
            rets.append(self._collect(store))
        st = self.pool.stats()
        st["exchanged_rows"] = self.exchanged_rows
        st["dict_encode_rows"] = self._dict_encode_rows
        st["dict_encode_host_batches"] = self.ops.dict_encode_host_batches
        st["str_rank_rows"] = self._str_rank_rows
        st["str_rank_rounds"] = self.ops.str_rank_rounds
        st["filter_rows_in"] = self._filter_rows_in
        st["filter_rows_kept"] = self._filter_rows_kept
        self.stats = st
        if st["spilled_to_host_bytes"] or st["exchanged_rows"]:
            log.info("[device] run stats: %s", st)
        self.pool.cleanup()
        return rets

    @staticmethod
    def _live_ids(data, sources):
        """ids of the runs held by the stores of ``data`` other than
        ``sources``.  Pass-through stages (identity/unkey/merges) share
        RUN objects between stores: a run is freed only when no other
        live source references it."""
        return {id(r) for k, v in data.items()
                if isinstance(v, PartStore) and k not in sources
                for runs in v.values() for r in runs}

    def _free_consumed(self, run):
        """Free a run the running stage has consumed, unless a store
        outside the stage still shares it."""
        if id(run) not in self._stage_live:
            self.pool.free(run)

    def _consume_partition(self, ins, p, flags=None):
        """Free partition ``p`` of fully-consumed input stores (their
        last consumer is the running stage) once its reduce/join is
        done — bounds the tier churn of >pool jobs.  (The reference
        deletes intermediates only after ALL outputs are known,
        runner.py:207-228; per-partition granularity is what lets a
        120 GB job fit a 24 GB pool without re-evicting dead data.)"""
        if flags is None:
            flags = self._consume_flags
        if not flags or len(flags) != len(ins):
            return
        for st, f in zip(ins, flags):
            if not f or not isinstance(st, PartStore):
                continue
            # a run two consumed inputs share is freed twice: pool.free
            # of a freed run does nothing
            for run in st.pop(p, []):
                self._free_consumed(run)

    def _free_store(self, store, live_ids=frozenset()):
        """Release a fully-consumed store's memory across all tiers
        (skipping runs still shared with live stores)."""
        if not isinstance(store, PartStore):
            return
        for part in list(store):
            kept = []
            for run in store[part]:
                if id(run) in live_ids:
                    kept.append(run)
                else:
                    self.pool.free(run)
            if kept:
                store[part] = kept
            else:
                del store[part]

    # -- ingest / collect --------------------------------------------------

    def _ingest(self, inp):
        """Input -> partition store.  ColumnSource goes straight to device;
        host Datasets/Chunkers decode through the numeric encoder."""
        if isinstance(inp, TextSource):
            if self.world > 1:
                # per-rank newline-aligned slice of the corpus; every
                # rank computes the identical boundaries (same input),
                # so slices partition the text exactly
                t = inp.text
                n = t.shape[0]

                def _align(b):
                    # first byte AFTER the next newline at/past b
                    import numpy as np
                    if b <= 0 or b >= n:
                        return min(max(b, 0), n)
                    nl = np.flatnonzero(t[b - 1:] == ord("\n"))
                    return (b - 1 + int(nl[0]) + 1) if nl.size else n

                lo, hi = map(_align, self._rank_slice(n))
                return TextSource(t[lo:hi].copy())
            return inp
        if isinstance(inp, ColumnSource):
            keys = inp.keys.to(self.device)
            vals = inp.vals.to(self.device)
            if self.world > 1:
                # each rank keeps an equal slice of the input
                lo, hi = self._rank_slice(keys.numel())
                keys, vals = keys[lo:hi], vals[lo:hi]
            if self.world > 1 or self.n_partitions == 1:
                return self._partition(keys, vals, fkeys=inp.fkeys,
                                       str_table=inp.str_table)
            # lazy ingest: batched unpartitioned runs as VIEWS of the
            # resident input — partitioning by the input keys is wasted
            # work when the first stage re-keys, and cloning would send
            # a full extra copy of the input through the spill tiers
            # (measured 2x tier traffic on a 120 GB job).  View runs
            # are NOT pool-admitted: the parent tensor is resident for
            # the stage regardless (ColumnSource holds it), so they are
            # never evicted and cost the pool nothing.
            store = PartStore(partitioned=False,
                              str_table=inp.str_table,
                              fkeys=inp.fkeys,
                              svals=_is_sv(vals),
                              vdtype=self._vdtype_of(vals))
            store[0] = []
            n = keys.numel()
            step = max(1, settings.gpu_batch_records)
            for lo in range(0, n, step):
                hi = min(lo + step, n)
                run = DeviceRun(keys[lo:hi], vals[lo:hi], sorted=False)
                store[0].append(run)
            return store
        # host dataset / chunker: stream records; numeric records become
        # columns, object records stay host-side (HostStore)
        records = self._host_records_of_input(inp)
        if self.world > 1:
            lo, hi = self._rank_slice(len(records))
            records = records[lo:hi]
        return self._encode_or_host(records)

    def _rank_slice(self, n):
        """``(lo, hi)``: this rank's equal share of ``n`` input rows."""
        return (n * self.rank // self.world,
                n * (self.rank + 1) // self.world)

    @staticmethod
    def _host_records_of_input(inp):
        from ..dataset import Chunker, Dataset
        if isinstance(inp, Dataset):
            return list(inp.read())
        if isinstance(inp, Chunker):
            out = []
            for c in inp.chunks():
                out.extend(c.read())
            return out
        raise TypeError("GPU engine cannot ingest {!r}".format(inp))

    def _encode_or_host(self, records):
        """Records -> partition store in the one columnar layout every
        rank agrees on, or the records themselves (``HostStore``) when
        there is none.  At world > 1 the ranks gather their local layouts
        in ONE collective before any tensor is built: a per-rank choice
        would desync the exchange collectives where branches differ.
        The host fallback is symmetric and issues no further collective
        (host reduces exchange via _host_exchange)."""
        # today's behaviour, kept as it is: only a single rank carries
        # string values under the keyed convention; at world > 1 such
        # records stay on the host (docs/ROADMAP.md)
        local = record_format.classify(
            records, keyed_str_values=self.world == 1)
        layouts = [local]
        if self.world > 1:
            import torch.distributed as dist
            layouts = [None] * self.world
            dist.all_gather_object(layouts, local)
        layout = record_format.agree(layouts)
        if layout is None:
            return HostStore(records)
        keys, vals, keyed, fkeys, table = record_format.build(records, layout)
        return self._partition(keys.to(self.device), vals.to(self.device),
                               keyed=keyed, fkeys=fkeys, str_table=table)

    def _collect(self, store):
        """Partition store -> one key-sorted ColumnDataset (the engine's
        MergeDataset analog: partitions are key-sorted, output is their
        merge)."""
        if isinstance(store, ColumnDataset):
            return store
        if isinstance(store, SinkStore):
            from ..dataset import cat_datasets
            return cat_datasets(store.datasets())
        if isinstance(store, HostStore):
            from ..dataset import MemoryDataset
            return MemoryDataset(sorted(store, key=lambda r: r[0]))
        if isinstance(store, TokenStore):
            return TokenColumnDataset(store, store.keyed)
        keyed, fkeys, tbl = store.keyed, store.fkeys, store.str_table
        sk, sv = self._merge_runs(
            [run for p in sorted(store) for run in store[p]], fkeys)
        if sk is None:
            sk = torch.zeros(0, dtype=torch.int64)
            sv = sk.clone()
        return ColumnDataset(sk, sv, keyed, fkeys, tbl)

    # -- ordering ----------------------------------------------------------

    _SIGN = -(1 << 63)

    def _sort(self, keys, payload=None, fkeys=False):
        """Key sort in *host* ascending order: signed for i64 keys, float
        ascending for f64-encoded keys (their encoding is already
        unsigned-ascending).  The backend sort is unsigned (built for
        hashes), so int keys are biased through the sign bit."""
        if fkeys:
            return self.ops.sort_pairs(keys, payload)
        sk, sp = self.ops.sort_pairs(keys ^ self._SIGN, payload)
        return sk ^ self._SIGN, sp

    # -- partitioning ------------------------------------------------------

    @staticmethod
    def _vdtype_of(vals):
        """Store-level value dtype of a value column (None: var-len)."""
        return None if _is_sv(vals) else vals.dtype

    def _empty(self, dtype=torch.int64):
        """A zero-row device column."""
        return torch.zeros(0, dtype=dtype, device=self.device)

    def _empty_vals(self, svals, vdtype):
        """A zero-row value column with a store's layout: the var-len
        arena, or a column of ``vdtype`` (i64 where none is declared).
        An empty rank's exchange columns must match the wire shape and
        dtype the other ranks send."""
        if svals:
            from .strvals import StrVals
            return StrVals.empty(self.device)
        return self._empty(vdtype or torch.int64)

    def _new_run(self, keys, vals, sorted):
        """A new pool-admitted run."""
        run = DeviceRun(keys, vals, sorted=sorted)
        self.pool.admit(run)
        return run

    def _partition(self, keys, vals, already_sorted=False, keyed=False,
                   fkeys=False, str_table=None):
        """Split columns into the partition store {p: [DeviceRun]} (K1+K2):
        partition ids, stable sort by id, slice contiguous segments."""
        P = self.n_partitions
        store = PartStore(keyed=keyed, fkeys=fkeys, str_table=str_table,
                          svals=_is_sv(vals), vdtype=self._vdtype_of(vals))
        if keys.numel() == 0 and self.world == 1:
            return store
        if P == 1 and self.world == 1:
            # no routing needed: one resident partition
            store[0] = [self._new_run(keys.contiguous(), vals.contiguous(),
                                      sorted=bool(already_sorted))]
            return store
        pid = self.ops.partition_of(keys, P)
        order = torch.argsort(pid, stable=True)
        keys, vals, pid = keys[order], vals[order], pid[order]
        if self.world > 1:
            keys, vals, pid = self._exchange(keys, vals, pid)
            # received rows arrive grouped by sender, not by partition:
            # restore pid order for the contiguous slicing below
            order = torch.argsort(pid, stable=True)
            keys, vals, pid = keys[order], vals[order], pid[order]
        self._slice_into(store, keys, vals, pid,
                         already_sorted=already_sorted)
        return store

    def _slice_into(self, store, keys, vals, pid, already_sorted=False):
        """Append contiguous partition slices of pid-ordered columns to
        ``store`` (this rank's owned partitions only at world > 1)."""
        P = self.n_partitions
        counts = torch.bincount(pid, minlength=P)
        offs = torch.cumsum(counts, 0) - counts
        counts_l = counts.tolist()
        offs_l = offs.tolist()
        for p in range(P):
            if self.world > 1 and p % self.world != self.rank:
                continue
            n = counts_l[p]
            if not n:
                continue
            o = offs_l[p]
            # clone, not view: spilled runs must release their HBM
            # (views pin the whole routed batch)
            k = keys[o:o + n].clone()
            v = vals[o:o + n].clone()
            # runs stay unsorted: consumers that need key order sort at
            # merge time, once per partition instead of once per
            # (run, partition) slice — thousands of tiny sorts otherwise
            store.setdefault(p, []).append(
                self._new_run(k, v, sorted=bool(already_sorted)))
        return store

    def _ensure_partitioned(self, store):
        """Route an unpartitioned store's runs to hash partitions, one
        run at a time (each run is bounded, so this streams through the
        pool).  At world > 1 the runs concatenate FIRST: run counts
        differ across ranks, and _partition exchanges — one collective
        per stage per rank is the invariant."""
        if not isinstance(store, PartStore) or store.partitioned:
            return store
        if self.world > 1:
            k, v = self._merge_runs(store.get(0, []), store.fkeys,
                                    need_sorted=False)
            if k is None:
                k = self._empty()
                v = self._empty_vals(store.svals, store.vdtype)
            return self._partition(k, v, keyed=store.keyed,
                                   fkeys=store.fkeys,
                                   str_table=store.str_table)
        out = None
        for run in store.get(0, []):
            k, v = self.pool.columns(run, self.device)
            out = _extend_store(out, self._partition(
                k, v, keyed=store.keyed, fkeys=store.fkeys,
                str_table=store.str_table))
        if out is None:
            out = PartStore(keyed=store.keyed, fkeys=store.fkeys,
                            str_table=store.str_table, svals=store.svals)
        return out

    def _exchange(self, keys, vals, pid):
        """RCCL all-to-all: route rows to the partition's owning rank
        (p % world); returns this rank's rows."""
        from ..parallel.shuffle import (exchange_columns,
                                        exchange_columns_varlen)
        self.exchanged_rows += keys.numel()
        if _is_sv(vals):
            return exchange_columns_varlen(keys, vals, pid, self.world)
        return exchange_columns(keys, vals, pid, self.world)

    def _merged_partition(self, stores, p, need_sorted=True):
        """All runs of partition p across input stores, merged
        key-sorted (``need_sorted=False`` skips the sort for consumers
        that re-key anyway, e.g. the kv map)."""
        return self._merge_runs(
            [run for store in stores for run in store.get(p, [])],
            any(s.fkeys for s in stores), need_sorted)

    def _merge_runs(self, runs, fkeys, need_sorted=True):
        """The rows of ``runs`` as one (keys, vals) pair, key-sorted
        unless ``need_sorted`` is off; (None, None) for no runs."""
        if not runs:
            return None, None
        cols = [self.pool.columns(run, self.device) for run in runs]
        ks = [k for k, _v in cols]
        vs = [v for _k, v in cols]
        all_sorted = all(run.sorted for run in runs)
        if len(ks) == 1 and (all_sorted or not need_sorted):
            return ks[0], vs[0]
        if not need_sorted:
            return torch.cat(ks), _cat_vals(vs)
        if all_sorted:
            # K4: merge-path k-way merge of already-sorted runs — one
            # log2(R)-deep pass tree instead of a full radix re-sort
            # (reference analog: heapq.merge, dataset.py:567-588)
            mk, perm = self.ops.merge_sorted_runs(ks, fkeys=fkeys)
            return mk, _cat_vals(vs)[perm]
        sk, sp = self._sort(torch.cat(ks), fkeys=fkeys)
        return sk, _cat_vals(vs)[sp.to(torch.int64)]

    def _all_rows(self, store):
        """All (keys, vals) rows of a store, concatenated on device."""
        ks, vs = [], []
        for p in sorted(store):
            k, v = self._merged_partition([store], p, need_sorted=False)
            if k is None:
                continue
            ks.append(k)
            vs.append(v)
        if not ks:
            return self._empty(), self._empty()
        return torch.cat(ks), _cat_vals(vs)

    def _parts(self, stores):
        ps = set()
        for s in stores:
            ps.update(s.keys())
        return sorted(ps)

    # -- map stage ---------------------------------------------------------

    def run_map(self, stage, ins):
        """Dispatch a map stage on its ``device_map`` descriptor; an
        untagged stage, or one fed host records, runs on the host."""
        spec = stage.options.get("device_map")
        if spec is None or any(isinstance(s, HostStore) for s in ins):
            return self._host_map(stage, ins)
        handler = self._MAP_HANDLERS.get(spec[0])
        if handler is None:
            raise ValueError("unknown device_map spec {!r}".format(spec))
        return handler(self, stage, spec, ins)

    def _batches(self, ins, consume=False):
        """Yield the inputs' (keys, vals) batches for a record-wise op:
        an unrouted store streams run by run, a routed one merged
        (unsorted) partition by partition.  With ``consume``, a batch's
        source runs are freed as soon as the caller asks for the next
        batch, for inputs whose last consumer is the running stage —
        the caller's output then never coexists with the whole input
        on >pool jobs."""
        flags = self._consume_flags if consume else None
        if not flags or len(flags) != len(ins):
            flags = [False] * len(ins)
        for store, f in zip(ins, flags):
            if isinstance(store, PartStore) and not store.partitioned:
                for run in store.get(0, []):
                    yield self.pool.columns(run, self.device)
                    if f:
                        self._free_consumed(run)
                if f:
                    store.pop(0, None)
            else:
                for p in self._parts([store]):
                    keys, vals = self._merged_partition(
                        [store], p, need_sorted=False)
                    if keys is None:
                        continue
                    yield keys, vals
                    self._consume_partition([store], p, flags=[f])

    def _count_batches(self, ins):
        """Upper bound on the batches ``_batches`` yields, computed
        WITHOUT consuming anything — the local term of the rank-agreed
        chunk count for the exchange pipeline."""
        c = 0
        for store in ins:
            if isinstance(store, PartStore) and not store.partitioned:
                c += len(store.get(0, []))
            elif isinstance(store, PartStore):
                c += len(self._parts([store]))
        return c

    def _map_kv(self, stage, spec, ins):
        """Emit (keyfn(v), valfn(v)) per record — the group_by/count map."""
        _kind, keyf, valf = spec
        if _any_flag(ins, "keyed"):
            # tuple-valued records (keyed convention): column funcs
            # don't apply — run the stage's Python mapper instead
            return self._host_map(stage, ins)
        if keyf == "identity" and any(_store_has_sv(s) for s in ins):
            # keying by a var-len VALUE needs a dictionary encode: on
            # device at world == 1 when every input is a string column;
            # otherwise the host path builds it (string-key ingest
            # re-enters the device path downstream)
            if self.world == 1 and valf in ("identity", "one") and all(
                    isinstance(s, PartStore)
                    and (_store_has_sv(s) or not len(s)) for s in ins):
                return self._map_kv_strkeys(valf, ins)
            return self._host_map(stage, ins)
        if self.world > 1:
            return self._kv_exchange(keyf, valf, ins)
        out = None
        for k, v in self._batches(ins, consume=True):
            nk = self._apply_colfunc(keyf, k, v)
            nv = self._apply_colfunc(valf, k, v)
            fkeys = nk.dtype == torch.float64
            if fkeys:
                nk = encode_f64_sortable(nk)
            out = _extend_store(out, self._partition(nk, nv, fkeys=fkeys))
        return out if out is not None else PartStore()

    def _map_kv_strkeys(self, valf, ins):
        """The kv map keyed by a var-len string VALUE (count, group,
        sort_by over a column of words), single rank.  Each batch
        dictionary-encodes on device (ops.dict_encode) into PROVISIONAL
        ids — positions in the concatenation of all batches' uniques —
        and is stored as an unrouted, pool-admitted run, so >pool jobs
        spill it.  After the last batch the uniques dedupe across
        batches on device, the U global uniques rank in byte order on
        device (ops.str_rank; UTF-8 byte order == Python str order), a
        device lut takes provisional id -> lexicographic rank, and the
        ``str_table`` is a lazy ``StrTable`` over the uniques gathered
        into rank order: nothing decodes on the host until keys are
        read.  That arena is O(U) bytes of device memory outside the
        pool's accounting until the first read.  Returns the unrouted
        string-keyed store ``_ensure_partitioned`` routes."""
        from .strvals import StrVals
        prov = PartStore(partitioned=False, svals=valf == "identity",
                         vdtype=None if valf == "identity"
                         else torch.int64)
        prov[0] = []
        uniqs = []
        base = 0
        for _k, v in self._batches(ins, consume=True):
            if v.numel() == 0:
                continue
            ids, uq = self.ops.dict_encode(v)
            self._dict_encode_rows += v.numel()
            prov[0].append(self._new_run(
                ids + base,
                v if valf == "identity" else torch.ones_like(ids),
                sorted=False))
            uniqs.append(uq)
            base += uq.numel()
        if not uniqs:
            return PartStore(vdtype=torch.int64)
        if len(uniqs) == 1:
            gids, guq = None, uniqs[0]
        else:
            gids, guq = self.ops.dict_encode(StrVals.cat(uniqs))
        from ..utils.trace import trace_stage
        n_uq = guq.numel()
        with trace_stage("  str_table: {} uniques ranked on device".format(
                n_uq)):
            rank = self.ops.str_rank(guq)
            self._str_rank_rows += n_uq
            order = torch.empty_like(rank)
            order[rank] = torch.arange(n_uq, dtype=torch.int64,
                                       device=rank.device)
            table = StrTable(guq.gather(order))
        lut = rank if gids is None else rank[gids]
        return self._rekeyed(prov, lut.__getitem__, fkeys=False,
                             str_table=table, consume=True)

    def _kv_exchange(self, keyf, valf, ins):
        """The kv map at world > 1, as a CHUNKED exchange pipeline: ranks
        agree on the chunk COUNT (one max-reduce; the collective
        sequence per stage stays identical on every rank), then per
        chunk: column funcs + partition routing on the compute stream,
        the data all-to-all on RCCL's comm stream.  Routing chunk i+1 is
        issued while chunk i's exchange is in flight (only the small
        counts collective syncs the host); received chunks slice into
        runs at the end.  (SURVEY §2.3 overlap; gloo executes the same
        sequence synchronously.)"""
        import torch.distributed as dist
        t = torch.tensor([self._count_batches(ins)])
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        n_chunks = int(t.item())
        # rank-deterministic empty-chunk layout (an empty rank must
        # match the others' collective dtypes)
        vd = _declared(ins, "vdtype", torch.int64)
        in_sv = any(_store_has_sv(s) for s in ins)
        # fkeys derives from world-agreed metadata, NOT from an observed
        # batch: a rank with zero local batches must still treat
        # RECEIVED keys as f64-encoded when the other ranks encode
        fkeys = (keyf == "identity" and vd == torch.float64) \
            or (keyf == "key" and _any_flag(ins, "fkeys"))
        it = self._batches(ins, consume=True)
        parts = []
        for _i in range(n_chunks):
            k, v = next(it, (None, None))
            if k is None:
                nk = self._empty()
                nv = self._empty_vals(in_sv, vd) if valf == "identity" \
                    else self._empty()
            else:
                nk = self._apply_colfunc(keyf, k, v)
                nv = self._apply_colfunc(valf, k, v)
                assert (nk.dtype == torch.float64) == fkeys, \
                    "kv key dtype disagrees with store metadata"
            if fkeys:
                nk = encode_f64_sortable(nk)
            pid = self.ops.partition_of(nk, self.n_partitions)
            order = torch.argsort(pid, stable=True)
            parts.append(self._exchange(nk[order], nv[order], pid[order]))
        rk = torch.cat([e[0] for e in parts]) if parts else self._empty()
        rv = _cat_vals([e[1] for e in parts]) if parts else self._empty()
        rp = torch.cat([e[2] for e in parts]) if parts else self._empty()
        out = PartStore(fkeys=bool(fkeys), svals=_is_sv(rv),
                        vdtype=self._vdtype_of(rv))
        order = torch.argsort(rp, stable=True)
        return self._slice_into(out, rk[order], rv[order], rp[order])

    def _map_identity(self, stage, spec, ins):
        return self._merge_stores(ins)

    def _map_unkey(self, stage, spec, ins):
        """Strip the keyed-reducer value convention: values become the
        bare aggregates (the host stage extracts x[1])."""
        merged = self._merge_stores(ins)
        if not isinstance(merged, PartStore):
            return self._host_map(stage, ins)
        out = PartStore(keyed=False, fkeys=merged.fkeys,
                        partitioned=merged.partitioned,
                        str_table=merged.str_table, svals=merged.svals)
        out.update(merged)
        return out

    def _map_len_local(self, stage, spec, ins):
        """Row count from run metadata: no data is read at all."""
        if any(not isinstance(s, PartStore) for s in ins):
            return self._host_map(stage, ins)
        total = sum(r.n for s in ins for runs in s.values() for r in runs)
        keys = torch.ones(1, dtype=torch.int64, device=self.device)
        vals = torch.tensor([total], dtype=torch.int64, device=self.device)
        if self.world > 1:
            return self._partition(keys, vals)
        store = PartStore()
        if total:
            store[0] = [self._new_run(keys, vals, sorted=True)]
        return store

    def _map_text_df(self, stage, spec, ins):
        """Fused one-pass document frequency over a text input."""
        src = ins[0]
        if not isinstance(src, TextSource) or self.device.type != "cuda":
            return self._host_map(stage, ins)
        from .tfidf import TfidfEngine, chunk_bounds
        if src.text_t is not None:
            text = src.text_t.to(self.device)
        else:
            text = torch.from_numpy(src.text).to(self.device)
        eng = TfidfEngine(self.device)
        eng.reset()
        bounds = chunk_bounds(text, 1 << 30)     # 1 GiB chunks
        for s0, e0 in zip(bounds, bounds[1:]):
            eng.count_chunk(text[s0:e0].contiguous(), pos_base=s0)
        keys, df = eng.extract()
        if self.world > 1:
            # ONE exchange of (key, df, token-bytes) partials routed
            # by key % world; each rank rebuilds its owned shard
            # (same pattern as bench.py's explicit pipeline)
            from ..parallel.shuffle import (all_reduce_scalar,
                                            exchange_keyed_payload)
            blob, lens = eng.token_strings_dev(keys, text)
            rk, rdf, rblob, rlens = exchange_keyed_payload(
                keys, df, blob, lens)
            eng.merge_exchanged(rk, rdf, rblob, rlens)
            keys, df = eng.extract()
            eng.n_docs = all_reduce_scalar(eng.n_docs, device=self.device)
            # received token strings live in the exchanged blob
            text = rblob
        return TokenStore(eng, keys, df, text)

    def _cross_operands(self, ins):
        """Front half of the K9 broadcast cross maps: ins[0] is the
        streamed (outer) side whose keys the output carries, ins[1] the
        broadcast side, gathered across ranks like the host supplemental
        path.  Returns (outer store, its keys, its vals, broadcast
        vals), or None when the stage has no columnar form."""
        if len(ins) != 2 \
                or any(not isinstance(s, PartStore) for s in ins) \
                or any(s.keyed for s in ins) \
                or any(_store_has_sv(s) for s in ins):
            return None
        other, me = ins
        ko, vo = self._all_rows(other)
        km, vm = self._all_rows(me)
        if self.world > 1:
            from ..parallel.shuffle import gather_columns
            km, vm = gather_columns(km, vm, device=self.device)
        return other, ko, vo, vm

    @staticmethod
    def _binop(opn, a, b):
        """``_BINOPS[opn]`` over two columns (or a column and a 0-dim
        scalar), promoted to a common dtype first."""
        if a.dtype != b.dtype:
            dt = torch.promote_types(a.dtype, b.dtype)
            a, b = a.to(dt), b.to(dt)
        return _BINOPS[opn](a, b)

    def _partition_like(self, other, keys, vals):
        """Route new columns whose keys come from ``other``'s rows."""
        return self._partition(keys, vals, fkeys=other.fkeys,
                               str_table=other.str_table)

    def _map_cross(self, stage, spec, ins):
        """K9 broadcast cross join: every streamed row against every
        broadcast row."""
        opn = spec[1]
        prepared = self._cross_operands(ins)
        if prepared is None:
            return self._host_map(stage, ins)
        other, ko, vo, vm = prepared
        n_o, m = ko.numel(), vm.numel()
        out_k = torch.repeat_interleave(ko, m) if m else self._empty()
        if n_o and m:
            # me value (v2) against other value (v1)
            out_v = self._binop(opn, vm.repeat(n_o),
                                torch.repeat_interleave(vo, m))
        else:
            out_v = self._empty()
        return self._partition_like(other, out_k, out_v)

    def _map_cross_set(self, stage, spec, ins):
        """K9 broadcast-set: fold the broadcast side to one scalar,
        apply cross(v_streamed, scalar) over the streamed side."""
        opn, aggn = spec[1], spec[2]
        prepared = self._cross_operands(ins)
        if prepared is None or prepared[3].numel() == 0:
            # (empty broadcast side) host semantics: sum() of nothing
            # is 0, min/max raise
            return self._host_map(stage, ins)
        other, ko, vo, vm = prepared
        scalar = {"sum": vm.sum, "min": vm.min, "max": vm.max}[aggn]()
        return self._partition_like(other, ko,
                                    self._binop(opn, vo, scalar))

    def _map_topk_local(self, stage, spec, ins):
        """Per-batch top-k candidates by value (K11); all candidates
        meet in partition 0 for the global pass."""
        if _any_flag(ins, "keyed") or any(_store_has_sv(s) for s in ins):
            return self._host_map(stage, ins)
        K = spec[1]
        cand_k, cand_v = [], []
        fkeys = False
        for _keys, vals in self._batches(ins):
            is_f = vals.dtype == torch.float64
            fkeys = fkeys or is_f
            sk, sp = self._sort(encode_f64_sortable(vals) if is_f else vals,
                                fkeys=is_f)
            top = min(K, sk.numel())
            cand_k.append(sk[-top:])
            cand_v.append(vals[sp.to(torch.int64)[-top:]])
        if cand_k:
            ck, cv = torch.cat(cand_k), torch.cat(cand_v)
        elif self.world == 1:
            return PartStore()
        else:
            # candidate-less rank (input shard smaller than the world)
            # must still join the exchange with the agreed layout, or
            # the collective sequence desyncs
            vd = _declared(ins, "vdtype", torch.int64)
            fkeys = vd == torch.float64
            ck, cv = self._empty(), self._empty_vals(False, vd)
        store = PartStore(fkeys=fkeys)
        if self.world > 1:
            ck, cv, _ = self._exchange(ck, cv, torch.zeros_like(ck))
            if self.rank != 0 or ck.numel() == 0:
                return store
        sk, sp = self._sort(ck, fkeys=fkeys)
        store[0] = [self._new_run(sk, cv[sp.to(torch.int64)], sorted=True)]
        return store

    def _map_filter(self, stage, spec, ins):
        """Keep the records that satisfy every recognized predicate of
        the stage (``spec[1]``: clauses of (selector, op, constants)).

        Record-wise and, the compaction being stable, order-preserving:
        the output keeps the input's metadata, every input run becomes
        one new run in the same partition with the same ``sorted`` flag,
        and runs that filter to nothing are dropped.  No exchange, so
        nothing here differs at world > 1 and an empty rank issues no
        collective.  Columns and comparison domains resolve on the host
        for the whole stage before any launch (``_filter_programs``);
        whatever does not resolve runs the stage's Python mapper.  Every
        program is compiled once, before the run loop
        (``ops.filter_compile``: the string constants' buffer, the device
        hash sets of ``isin`` / ``notin`` clauses, which live until the
        stage returns).  Runs of var-len string values go through
        ``ops.sv_filter_rows``, all others through ``ops.filter_rows``."""
        store = ins[0] if len(ins) == 1 else None
        if not isinstance(store, PartStore):
            return self._host_map(stage, ins)
        programs = _filter_programs(store, spec[1],
                                    rank_agreed=self.world > 1, ops=self.ops)
        if programs is None:
            return self._host_map(stage, ins)
        # the string kernels' constants and the set clauses' device hash
        # sets: built once a stage and program, dropped with ``programs``
        # when the stage returns
        programs = {
            vdt: [self.ops.filter_compile(
                chunk, "string" if vdt is None else "numeric", self.device)
                for chunk in chunks]
            for vdt, chunks in programs.items()}
        out = PartStore(keyed=store.keyed, fkeys=store.fkeys,
                        partitioned=store.partitioned,
                        str_table=store.str_table, svals=store.svals,
                        vdtype=store.vdtype)
        consume = bool(self._consume_flags and len(self._consume_flags) == 1
                       and self._consume_flags[0])
        for p in sorted(store):
            for run in store[p]:
                k, v = self.pool.columns(run, self.device)
                self._filter_rows_in += k.numel()
                # more than 8 clauses: successive applications
                rows = self.ops.sv_filter_rows if run.has_sv \
                    else self.ops.filter_rows
                for chunk in programs[run.vdtype]:
                    k, v = rows(k, v, chunk)
                self._filter_rows_kept += k.numel()
                if consume:
                    self._free_consumed(run)
                if k.numel():
                    # always a NEW run: pass-through stores share runs
                    out.setdefault(p, []).append(
                        self._new_run(k, v, sorted=run.sorted))
        if consume:
            store.clear()
        return out

    _MAP_HANDLERS = {
        "filter": _map_filter,
        "kv": _map_kv,
        "identity": _map_identity,
        "unkey": _map_unkey,
        "len_local": _map_len_local,
        "text_df": _map_text_df,
        "cross": _map_cross,
        "cross_set": _map_cross_set,
        "topk_local": _map_topk_local,
    }

    def _apply_colfunc(self, name, keys, vals):
        if name == "identity":
            return vals
        if name == "one":
            return torch.ones_like(keys)
        if name == "key":
            return keys
        raise ValueError("unknown column func {!r}".format(name))

    def _unify_str_stores(self, stores):
        """Cross-encode string keys (ROADMAP 2's remap): rank ids from
        different dictionaries are incompatible, so remap every run's
        key column through a device lut into the union table.  The lut
        is monotone (sorted table -> sorted union), so sorted runs stay
        sorted; hash ROUTING changes, so remapped stores come back
        unpartitioned and re-route in _ensure_partitioned.  Returns the
        unified store list, or None when any input has no dictionary
        (numeric/host/token stores: caller falls back to host records)."""
        tables = [s.str_table if isinstance(s, PartStore) else None
                  for s in stores]
        if any(t is None for t in tables):
            return None
        merged = tuple(sorted(set().union(*map(set, tables))))
        index = {t: i for i, t in enumerate(merged)}
        out = []
        for s, t in zip(stores, tables):
            if t == merged:
                out.append(s)
                continue
            lut = torch.tensor([index[x] for x in t], dtype=torch.int64,
                               device=self.device)
            out.append(self._rekeyed(s, lut.__getitem__, fkeys=False,
                                     str_table=merged))
        return out

    def _rekeyed(self, store, rekey, fkeys, str_table, consume=False):
        """An unrouted copy of ``store`` whose runs' key columns went
        through ``rekey`` (monotone, so sorted runs stay sorted).  With
        ``consume`` the caller owns ``store`` and gives it up: each new
        run takes over its source run's value column instead of cloning
        it, and the source run is freed."""
        ns = PartStore(keyed=store.keyed, fkeys=fkeys, partitioned=False,
                       str_table=str_table, svals=store.svals,
                       vdtype=store.vdtype)
        ns[0] = []
        for p in sorted(store):
            for run in store[p]:
                k, v = self.pool.columns(run, self.device)
                nr = DeviceRun(rekey(k), v if consume else v.clone(),
                               sorted=run.sorted)
                if consume:
                    self.pool.free(run)
                ns[0].append(nr)
                self.pool.admit(nr)
        if consume:
            store.clear()
        return ns

    def _unify_fkeys_stores(self, stores):
        """Mixed float-keyed and int-keyed inputs: the f64 side's keys are
        order-preserving encodings (encode_f64_sortable) while the int
        side's are raw i64 bit patterns, so comparisons AND hash routing
        would silently miss (1 != encode(1.0)).  Re-encode the int side
        through float64 (host semantics: 1 == 1.0).  Ints beyond 2^53
        lose precision here — the same contract as the mixed int+float
        record encode (records.build); such pipelines belong on
        the host engine.  Re-encoded stores come back unpartitioned
        (routing changed) and re-route in _ensure_partitioned."""
        if all(s.fkeys for s in stores) or not any(s.fkeys for s in stores):
            return stores
        return [s if s.fkeys else self._rekeyed(
                    s, lambda k: encode_f64_sortable(k.to(torch.float64)),
                    fkeys=True, str_table=s.str_table)
                for s in stores]

    def _as_host_records(self, stores):
        """Every store's records decoded into one HostStore (correct
        for any mix of layouts, slower)."""
        out = HostStore()
        for s in stores:
            out.extend(self._decode_store(s))
        return out

    def _merge_stores(self, stores):
        if len(stores) == 1:
            return stores[0]
        if any(not isinstance(s, PartStore) for s in stores):
            # HostStore / TokenStore / TextSource in the mix: only
            # PartStores share the run layout
            return self._as_host_records(stores)
        if any(s.str_table is not None for s in stores):
            uni = self._unify_str_stores(stores)
            if uni is None:
                # dictionary + dictionary-less mix
                return self._as_host_records(stores)
            stores = uni
        nonempty = [s for s in stores if len(s)]
        if any(_store_has_sv(s) for s in stores) and not all(
                _store_has_sv(s) for s in nonempty):
            # var-len + numeric value mix: no common column layout
            return self._as_host_records(stores)
        stores = self._unify_fkeys_stores(stores)
        if len({s.partitioned for s in stores}) > 1:
            # mixing hashed and unrouted partition-0 runs would corrupt
            # co-location: route everything first
            stores = [self._ensure_partitioned(s) for s in stores]
        out = PartStore(
            keyed=any(s.keyed for s in stores),
            fkeys=any(s.fkeys for s in stores),
            svals=any(s.svals for s in stores),
            partitioned=all(s.partitioned for s in stores),
            str_table=_declared(stores, "str_table"),
            vdtype=_declared(stores, "vdtype"))
        for s in stores:
            _extend_store(out, s)
        return out


    # -- reduce stage ------------------------------------------------------

    def run_reduce(self, stage, ins):
        """Co-locate the inputs' keys, then dispatch on the stage's
        ``device_reduce`` descriptor; stages with no columnar form run
        the host reducer."""
        spec = stage.options.get("device_reduce")
        routed = self._colocate(ins)
        if routed is None:
            return self._host_reduce(stage, ins)
        ins = routed
        if len(ins) == 1 and isinstance(ins[0], TokenStore) \
                and spec == ("sum",):
            ins[0].keyed = True        # keyed-reducer output convention
            return ins[0]
        if spec is None or self._reduce_needs_host(stage, spec[0], ins):
            return self._host_reduce(stage, ins)
        handler = self._REDUCE_HANDLERS.get(spec[0])
        if handler is None:
            raise ValueError(
                "unknown device_reduce spec {!r}".format(spec))
        return handler(self, stage, spec, ins)

    def _colocate(self, ins):
        """Make the inputs of a key-colocating stage comparable and
        co-partitioned: string keys remap into one union dictionary,
        int keys re-encode to match float-keyed inputs, and unrouted
        stores route to hash partitions.  Returns the new input list —
        every store then shares ``ins[0].str_table`` — or None when a
        dictionary-keyed input meets one without a dictionary (host
        records)."""
        if len(ins) > 1 and _declared(ins, "str_table") is not None:
            ins = self._unify_str_stores(ins)
            if ins is None:
                return None
        if len(ins) > 1 and all(isinstance(s, PartStore) for s in ins):
            ins = self._unify_fkeys_stores(ins)
        return [self._ensure_partitioned(s) for s in ins]

    @staticmethod
    def _reduce_needs_host(stage, kind, ins):
        if _any_flag(ins, "keyed") \
                or any(isinstance(s, HostStore) for s in ins):
            return True
        if not any(_store_has_sv(s) for s in ins):
            return False
        # var-len values: first/join(left|right) stay on device
        # (gather-only ops); arithmetic folds go to host records
        if kind == "join":
            return stage.options.get("device_join_pair") \
                not in ("left", "right")
        if kind != "first":
            return True
        # var-len + numeric mix can't share one value column
        svs = [_store_has_sv(s) for s in ins
               if isinstance(s, PartStore) and len(s)]
        return len(ins) > 1 and any(svs) and not all(svs)

    @staticmethod
    def _reduce_out(ins, keyed=True):
        """The empty output store of a reduce over co-located inputs."""
        return PartStore(keyed=keyed,
                         fkeys=any(s.fkeys for s in ins),
                         svals=any(_store_has_sv(s) for s in ins),
                         str_table=ins[0].str_table)

    def _reduce_partitions(self, ins, reduce_one, prefetch=False,
                           consume_empty=True):
        """Run ``reduce_one(p) -> (unique keys, aggregates)`` over every
        partition into a keyed output store, freeing each consumed
        input partition.  ``prefetch`` pages partition i+1 in on the
        side stream while partition i reduces; with ``consume_empty``
        off, a partition that reduced to nothing is left unconsumed."""
        out = self._reduce_out(ins)
        parts = self._parts(ins)
        for i, p in enumerate(parts):
            if prefetch:
                self._prefetch_partition(ins, parts, i + 1)
                self._wait_prefetch()
            uk, agg = reduce_one(p)
            if uk is not None or consume_empty:
                self._consume_partition(ins, p)
            if uk is None:
                continue
            out.setdefault(p, []).append(
                self._new_run(uk, agg, sorted=True))
        return out

    def _reduce_fold(self, stage, spec, ins):
        """sum / min / max per key."""
        return self._reduce_partitions(
            ins, lambda p: self._reduce_partition(ins, p, spec[0]),
            prefetch=True)

    def _reduce_mean(self, stage, spec, ins):
        def mean_of(p):
            uk, sm = self._reduce_partition(
                ins, p, "sum", vt=lambda v: v.to(torch.float64))
            if uk is None:
                return None, None
            _uk, c = self._reduce_partition(
                ins, p, "sum",
                vt=lambda v: torch.ones_like(v, dtype=torch.float64))
            return uk, sm / c

        return self._reduce_partitions(ins, mean_of, consume_empty=False)

    def _reduce_first(self, stage, spec, ins):
        """First value per key: stable sorts keep insertion order within
        equal keys, so the segment head is the first seen."""
        return self._reduce_partitions(
            ins, lambda p: self._reduce_partition(ins, p, "first"))

    def _reduce_topk_global(self, stage, spec, ins):
        K = spec[1]
        out = self._reduce_out(ins, keyed=False)
        ks, vs = [], []
        for p in self._parts(ins):
            keys, vals = self._merged_partition(ins, p)
            if keys is None:
                continue
            ks.append(keys)
            vs.append(vals)
        if not ks:
            return out
        keys = torch.cat(ks)
        vals = torch.cat(vs)
        sk, sp = self._sort(keys, fkeys=out.fkeys)
        top = min(K, sk.numel())
        out[0] = [self._new_run(
            sk[-top:].contiguous(),
            vals[sp.to(torch.int64)[-top:]].contiguous(), sorted=True)]
        return out

    def _reduce_join(self, stage, spec, ins):
        assert len(ins) == 2, "join takes two inputs"
        res = self._device_join(ins[0], ins[1], spec[1], stage)
        res.str_table = ins[0].str_table
        return res

    _REDUCE_HANDLERS = {
        "sum": _reduce_fold,
        "min": _reduce_fold,
        "max": _reduce_fold,
        "mean": _reduce_mean,
        "first": _reduce_first,
        "topk_global": _reduce_topk_global,
        "join": _reduce_join,
    }

    def _prefetch_partition(self, ins, parts, i):
        """Kick off async page-in of partition parts[i] on the side
        stream (no-op without a CUDA device)."""
        if self._side_stream is None or i >= len(parts):
            return
        nxt = parts[i]
        runs = [r for store in ins
                if isinstance(store, PartStore)
                for r in store.get(nxt, [])]
        self.pool.prefetch(runs, self.device, self._side_stream)

    def _wait_prefetch(self):
        if self._side_stream is not None:
            torch.cuda.current_stream(self.device).wait_stream(
                self._side_stream)

    def _first_sorted(self, keys, vals):
        """(unique_keys, first value per key) over a key-sorted column;
        stable sorts preserve insertion order within equal keys."""
        _seg, uk = self.ops.segment_ids(keys)
        flags = torch.ones_like(keys)
        flags[1:] = (keys[1:] != keys[:-1]).to(torch.int64)
        first_idx = torch.nonzero(flags.bool()).flatten()
        return uk, vals[first_idx]

    def _reduce_partition(self, ins, p, kind, vt=None):
        """One partition's reduce (kind: sum/min/max/first; ``vt``
        transforms the value column first).  A skewed partition whose
        runs exceed half the pool is reduced run-by-run and the partial
        aggregates re-reduced (associativity; "first" re-reduces in run
        order under stable sorts) — bounded memory instead of a giant
        merge (SURVEY §7 "skewed keys")."""
        def one(k_sorted, v):
            if kind == "first":
                return self._first_sorted(k_sorted, v)
            return self.ops.seg_reduce_sorted(k_sorted, v, kind)

        runs = [r for store in ins for r in store.get(p, [])]
        if not runs:
            return None, None
        fkeys = any(st.fkeys for st in ins)
        total = sum(r.nbytes for r in runs)
        if total <= self.pool.capacity // 2 or len(runs) == 1:
            keys, vals = self._merged_partition(ins, p)
            return one(keys, vt(vals) if vt else vals)
        pk, pv = [], []
        for run in runs:
            k, v = self.pool.columns(run, self.device)
            if not run.sorted:
                k, sp = self._sort(k, fkeys=fkeys)
                v = v[sp.to(torch.int64)]
            uk, agg = one(k, vt(v) if vt else v)
            pk.append(uk)
            pv.append(agg)
        keys = torch.cat(pk)
        vals = _cat_vals(pv)
        sk, sp = self._sort(keys, fkeys=fkeys)
        return one(sk, vals[sp.to(torch.int64)])

    def _device_join(self, left, right, how, stage):
        """Per-partition device hash join (K8); emits matched value pairs.
        The DSL's aggregate(left_vals, right_vals) runs per pair on the
        host only when not a recognized columnar op; the default device
        aggregate emits (key, (lv, rv)) as two columns folded into one
        f64/i64 value via the stage's pair op, or keeps lv when
        aggregate is 'left'."""
        pair_op = stage.options.get("device_join_pair", "pair_host")
        out = PartStore(
            keyed=True,
            fkeys=left.fkeys or right.fkeys,
            svals=(_store_has_sv(left) if pair_op == "left" else
                   _store_has_sv(right) if pair_op == "right" else
                   False))
        cap = int(os.environ.get("DAMPR_JOIN_PROBE_ROWS",
                                 settings.gpu_join_probe_rows))
        for p in self._parts([left, right]):
            # probe keys are CLUSTERED by their low bits (hash slot =
            # key & mask) rather than fully sorted: probes walk
            # L2-resident table regions (measured 3.5x over random
            # probing round 1) and the partial sort costs 2 radix
            # passes instead of up to 8
            lk, lv = self._merged_partition([left], p,
                                            need_sorted=False)
            rk, rv = self._merged_partition([right], p,
                                            need_sorted=False)
            if lk is None and rk is None:
                continue
            if lk is None:
                lk, lv = self._empty(), self._empty()
            if rk is None:
                rk, rv = self._empty(), self._empty()
            # skewed-join guard (ROADMAP 7): the table is built on the
            # RIGHT side, probes stream the LEFT.  Inner joins are
            # symmetric, so if the build side is the oversized one, swap
            # so the big side is probed in batches instead of blowing
            # out the table build.
            swap = (how == "inner" and rk.numel() > cap
                    and rk.numel() > lk.numel())
            if swap:
                lk, lv, rk, rv = rk, rv, lk, lv
            # probe through a low-bit-clustered VIEW of the keys; only
            # the (small) emitted index set maps back through the
            # permutation — the value column is never re-gathered
            perm = self.ops.probe_order(lk)
            probe_k = lk[perm] if perm is not None else lk
            # build the table ONCE; the skew guard probes in batches
            table = self.ops.hash_join_build(rk)
            # inner/left matches of a probe row are independent of every
            # other probe row, so probing distributes over contiguous
            # batches; full-outer tracks unmatched RIGHT rows across the
            # whole probe and must run in one piece.
            n = probe_k.numel()
            step = n if (how == "outer" or n <= cap) else cap
            for a in range(0, max(n, 1), max(step, 1)):
                b = min(n, a + max(step, 1))
                li, ri = self.ops.hash_join(probe_k[a:b], rk, how,
                                            table=table)
                li = torch.where(li >= 0, li + a, li)
                if perm is not None:
                    li = torch.where(
                        li >= 0, perm[torch.clamp(li, min=0)], li)
                if swap:
                    li, ri = ri, li
                    klk, krk, klv, krv = rk, lk, rv, lv
                else:
                    klk, krk, klv, krv = lk, rk, lv, rv
                keys = torch.where(li >= 0, klk[torch.clamp(li, min=0)],
                                   krk[torch.clamp(ri, min=0)])
                valid_l = li >= 0
                valid_r = ri >= 0
                if pair_op == "left":
                    merged = self._side_val(klv, li, valid_l)
                elif pair_op == "right":
                    merged = self._side_val(krv, ri, valid_r)
                else:
                    lvm = self._side_val(klv, li, valid_l)
                    rvm = self._side_val(krv, ri, valid_r)
                    merged = self._apply_pair_op(pair_op, lvm, rvm,
                                                 valid_l, valid_r)
                if keys.numel() == 0 and n > 0:
                    continue
                # emitted unsorted: consumers (collect/reduce) sort the
                # whole output once instead of per-batch sort + merge
                out.setdefault(p, []).append(self._new_run(
                    keys.contiguous(), merged.contiguous(), sorted=False))
            self._consume_partition([left, right], p)
        return out

    @staticmethod
    def _side_val(vcol, idx, valid):
        """One join side's matched values by row index; unmatched rows
        get the dtype's zero (numeric) or empty bytes (var-len)."""
        if _is_sv(vcol):
            from .strvals import StrVals
            if bool(valid.all()):
                return vcol.gather(idx)
            # append an empty row as the unmatched target
            ext = StrVals(vcol.blob,
                          torch.cat([vcol.offs, vcol.offs[-1:]]))
            nrow = vcol.numel()
            return ext.gather(
                torch.where(valid, idx, torch.full_like(idx, nrow)))
        if vcol.numel() == 0:           # empty side: all rows unmatched
            return torch.zeros(idx.numel(), dtype=vcol.dtype,
                               device=idx.device)
        return torch.where(valid, vcol[torch.clamp(idx, min=0)],
                           torch.zeros_like(idx))

    @staticmethod
    def _apply_pair_op(op, lv, rv, valid_l, valid_r):
        if op == "left":
            return lv
        if op == "right":
            return rv
        if op in ("sum", "mul"):
            return _BINOPS["add" if op == "sum" else op](lv, rv)
        raise ValueError(
            "join aggregate not columnar ({!r}); use funcs-recognized "
            "aggregates or the host engine".format(op))

    # -- sink --------------------------------------------------------------

    def run_sink(self, stage, ins):
        """Sink semantics match the host SinkWriter: one text line per
        record, value only, any value str-formatted (reference:
        dataset.py:277-278 prints the value).  Untagged sinks (pending
        format maps, e.g. sink_tsv's) run the mapper on host over the
        decoded records.  Returns a lazy view over the written part file
        so the sink's output is readable downstream, matching
        _SinkWorker (runner.py:278-298)."""
        import os
        path = stage.path
        os.makedirs(path, exist_ok=True)
        ds = self._collect(self._merge_stores(ins))
        fname = os.path.join(path, "part-{}".format(self.rank))
        if stage.options.get("device_sink") == "values":
            with open(fname, "w") as fh:
                for _kk, vv in ds.read():
                    fh.write("{}\n".format(vv))
        else:
            from ..dataset import MemoryDataset
            mem = MemoryDataset(list(ds.read()))
            with open(fname, "w") as fh:
                for _kk, vv in stage.mapper.map(mem):
                    fh.write("{}\n".format(vv))
        return SinkStore([fname])

    # -- host fallback -----------------------------------------------------

    def _decode_store(self, store):
        if isinstance(store, HostStore):
            return list(store)
        if isinstance(store, SinkStore):
            return [kv for ds in store.datasets() for kv in ds.read()]
        if isinstance(store, TextSource):
            return record_format.decode_text(store.text.tobytes())
        if isinstance(store, TokenStore):
            return list(TokenColumnDataset(store, store.keyed).read())
        records = []
        for p in sorted(store):
            keys, vals = self._merged_partition([store], p)
            if keys is not None:
                records.extend(record_format.decode(
                    keys, vals, store.keyed, store.fkeys, store.str_table))
        return records

    def _host_map(self, stage, ins):
        """Decode -> run the stage's (opaque) mapper on host -> re-encode.
        The shuffle core stays on device either side of this boundary.
        Input 0 is the primary dataset; the rest ride as supplemental
        dataset-lists (cross joins — reference: stagerunner.py:66-74).
        Concat stages treat every input as a primary."""
        from ..dataset import MemoryDataset
        if stage.options.get("concat"):
            out_records = []
            for store in ins:
                out_records.extend(stage.mapper.map(
                    MemoryDataset(self._decode_store(store))))
            return self._encode_or_host(out_records)
        primary = MemoryDataset(self._decode_store(ins[0]))
        supplemental = []
        for s in ins[1:]:
            recs = self._decode_store(s)
            if self.world > 1:
                # supplemental sides (cross/broadcast joins) must be
                # COMPLETE on every rank: computed stores are rank-owned
                # shards and raw inputs are rank slices, so gather the
                # union (the RCCL-bcast analog of K9's broadcast side)
                recs = self._host_gather(recs)
            supplemental.append([MemoryDataset(recs)])
        out_records = list(stage.mapper.map(primary, *supplemental))
        return self._encode_or_host(out_records)

    def _host_gather(self, recs):
        """Union of every rank's records, identical on all ranks (one
        collective; deterministic rank order)."""
        import torch.distributed as dist
        gathered = [None] * self.world
        dist.all_gather_object(gathered, recs)
        return [r for lst in gathered for r in lst]

    def _host_reduce(self, stage, ins):
        from ..dataset import MemoryDataset
        datasets = []
        for store in ins:
            recs = self._decode_store(store)
            if self.world > 1:
                recs = self._host_exchange(recs)
            recs.sort(key=lambda r: r[0])     # reducers need sorted streams
            datasets.append([MemoryDataset(recs)])
        out_records = list(stage.reducer.reduce(*datasets))
        return self._encode_or_host(out_records)

    def _host_exchange(self, recs):
        """Host-record analog of the column exchange (one collective per
        input store, deterministic across ranks): gather every rank's
        records, keep the keys this rank owns by the process-stable
        hash.  Without this, a multi-rank host-fallback reduce would
        silently fold only the local slice of each key's values."""
        import torch.distributed as dist
        from ..keyhash import stable_hash64
        gathered = [None] * self.world
        dist.all_gather_object(gathered, recs)
        return [r for lst in gathered for r in lst
                if stable_hash64(r[0]) % self.world == self.rank]
