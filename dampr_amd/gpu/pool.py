"""The device engine's three-tier run storage: ``DeviceRun`` (one spillable
(keys, vals) run), ``HbmPool`` (the two-watermark HBM -> pinned host -> NVMe
governor) and the recycled pinned staging buffers between the tiers.

The engine holds runs and talks to the pool: ``admit`` a new run,
``columns`` to read one (paged in from whatever tier holds it), ``free``
when its last consumer is done.  A run's row count, byte size and value
kind (``n``, ``nbytes``, ``vdtype``, ``has_sv``) are fixed when it is built
and readable on every tier without paging it in."""
import os

import torch

from .. import settings
from .stores import _is_sv
from .strvals import StrVals

class _PinnedPool(object):
    """Recycled pinned-host buffers for the spill tier: cudaHostAlloc of
    a multi-hundred-MB buffer costs tens of ms, and a >pool job spills
    hundreds of runs.  Power-of-two u8 buckets, views carved to size;
    a buffer with an in-flight H2D reload is only reused after its
    event completes."""

    def __init__(self, cap_bytes=192 << 30):
        import threading
        self.free = {}                 # bucket bytes -> [u8 base]
        self.free_bytes = 0
        self.cap = cap_bytes
        self._pending = []             # (base, bucket, event)
        self._lock = threading.Lock()  # IO threads stage into the pool

    @staticmethod
    def _bucket(nbytes):
        return 1 << max(12, int(nbytes - 1).bit_length())

    def _drain(self):
        still = []
        for base, b, evt in self._pending:
            if evt is not None and not evt.query():
                still.append((base, b, evt))
                continue
            if self.free_bytes + b <= self.cap:
                self.free.setdefault(b, []).append(base)
                self.free_bytes += b
        self._pending = still

    def get_like(self, t):
        """Pinned host tensor with t's shape/dtype."""
        return self.get(t.numel(), t.dtype)

    def get(self, numel, dtype):
        nbytes = numel * torch._utils._element_size(dtype)
        pin = torch.cuda.is_available()
        if nbytes == 0:
            return torch.empty(0, dtype=dtype, pin_memory=pin)
        with self._lock:
            self._drain()
            b = self._bucket(nbytes)
            lst = self.free.get(b)
            if lst:
                base = lst.pop()
                self.free_bytes -= b
            else:
                base = None
        if base is None:
            base = torch.empty(self._bucket(nbytes), dtype=torch.uint8,
                               pin_memory=pin)
        return base[:nbytes].view(dtype)

    def put(self, t, event=None):
        """Return a buffer; with ``event``, reuse waits for it (an
        async H2D may still be reading the pinned memory)."""
        if t is None or not isinstance(t, torch.Tensor) \
                or not t.is_pinned():
            return
        base = t
        while getattr(base, "_base", None) is not None:
            base = base._base
        nb = base.numel() * base.element_size()
        if base.dtype != torch.uint8 or nb != self._bucket(nb):
            return                     # not one of our bucket bases
        with self._lock:
            self._pending.append((base, nb, event))


_PIN = _PinnedPool()


def _copy_to_host(keys, vals, stream=None):
    """Copy a device (keys, vals) pair to host memory (pinned when the
    source is on a GPU); returns ((host keys, host vals), event).

    With ``stream`` the copies are non-blocking on that stream, ordered
    after the current stream's work; ``record_stream`` keeps the source
    tensors' memory from being reused until they land, and the returned
    event marks that point.  Without it the copies are synchronous and
    the event is None."""
    pin = keys.device.type == "cuda"

    def host(t):
        h = _PIN.get_like(t) if pin else torch.empty_like(t, device="cpu")
        h.copy_(t, non_blocking=stream is not None)
        if stream is not None:
            t.record_stream(stream)
        return h

    def pair():
        hk = host(keys)
        if _is_sv(vals):
            return hk, StrVals(host(vals.blob), host(vals.offs))
        return hk, host(vals)

    if stream is None:
        return pair(), None
    main = torch.cuda.current_stream(keys.device)
    with torch.cuda.stream(stream):
        # copies must see the producing kernels' writes
        stream.wait_stream(main)
        hp = pair()
        evt = torch.cuda.Event()
        evt.record(stream)
    return hp, evt


def _unpin(host_pair, event=None):
    """Give a host (keys, vals) pair's buffers back to ``_PIN``; with
    ``event``, their reuse waits for it."""
    hk, hv = host_pair
    _PIN.put(hk, event)
    if _is_sv(hv):
        _PIN.put(hv.blob, event)
        _PIN.put(hv.offs, event)
    else:
        _PIN.put(hv, event)


class DeviceRun(object):
    """One (keys, vals) run of a partition, spillable down the tier
    hierarchy HBM -> pinned host -> NVMe file (the reference's gzip-pickle
    /tmp spill files, dataset.py:119-188, re-expressed for 288 GB HBM +
    host DRAM + NVMe).

    Runs are immutable, so what the engine and the pool's accounting ask
    of a run is fixed at construction and stays the same on every tier
    and after ``drop()``: ``n`` rows, ``nbytes``, ``vdtype`` (the value
    column's dtype; None for a var-len ``StrVals`` column) and
    ``has_sv``."""

    __slots__ = ("keys", "vals", "sorted", "n", "nbytes", "vdtype",
                 "has_sv", "_blob", "_host", "_disk", "_evt", "_dfut",
                 "_lfut")

    def __init__(self, keys, vals, sorted=False):
        self.keys = keys
        self.vals = vals
        self.sorted = sorted
        self.n = keys.numel()
        self.has_sv = _is_sv(vals)
        if self.has_sv:
            self.vdtype = None
            self._blob = vals.blob.numel()     # spill-file layout
            self.nbytes = self.n * 8 + vals.nbytes
        else:
            self.vdtype = vals.dtype
            self._blob = 0
            self.nbytes = self.n * 8 + vals.element_size() * vals.numel()
        self._host = None
        self._disk = None
        self._evt = None           # in-flight async D2H spill marker
        self._dfut = None          # in-flight threaded disk WRITE
        self._lfut = None          # in-flight threaded disk READ-AHEAD

    @property
    def resident(self):
        return self.keys is not None

    @property
    def on_disk(self):
        return self._disk is not None

    @property
    def clean(self):
        """Resident with a (possibly in-flight) host copy."""
        return self.keys is not None and self._host is not None

    def _wait_spill(self):
        """Block until an in-flight async spill's D2H copies land."""
        if self._evt is not None:
            self._evt.synchronize()
            self._evt = None

    def _wait_io(self):
        """Join any threaded disk write/read touching this run."""
        if self._dfut is not None:
            self._dfut.result()
            self._dfut = None
        if self._lfut is not None:
            self._lfut.result()
            self._lfut = None

    def _stage_host(self):
        """IO-thread body: page the run's bytes from NVMe into pinned
        host buffers (read-ahead; the H2D happens at touch time).
        Joins a pending disk WRITE first (executor FIFO guarantees the
        write already started, so this cannot self-deadlock)."""
        self._wait_spill()
        if self._dfut is not None:
            self._dfut.result()
            self._dfut = None
        self._load_host()

    def drop(self):
        """Release storage on every tier (caller owns accounting and
        disk unlink).  Waits for in-flight spill DMA first — freeing a
        pinned buffer under an active copy corrupts host memory."""
        self._wait_spill()
        self._wait_io()
        if self._host is not None:
            _unpin(self._host)
        self.keys = None
        self.vals = None
        self._host = None

    def writeback_async(self, stream):
        """Copy HBM -> pinned host in the background WITHOUT evicting:
        runs are immutable, so the host copy never goes stale and a
        later eviction becomes a pointer drop instead of a synchronous
        (or burst-clustered) D2H on the critical path."""
        if stream is None or self.keys is None or self._host is not None \
                or self.keys.device.type != "cuda":
            return
        self._host, self._evt = _copy_to_host(self.keys, self.vals, stream)

    def spill_async(self, stream):
        """HBM -> pinned host on a dedicated D2H stream, overlapped
        with compute on the main stream.  Device tensors are released
        immediately (record_stream at copy time defers allocator reuse
        until the copies complete); host-side readers must
        _wait_spill().  A clean run already has its copy, so releasing
        the device tensors is the whole eviction."""
        if stream is None or self.keys is None \
                or self.keys.device.type != "cuda":
            return self.spill()
        self.writeback_async(stream)
        self.keys = None
        self.vals = None

    def spill(self):
        """HBM -> (pinned) host memory, synchronously."""
        if self._host is not None or self.keys is None:
            return
        self._host, _ = _copy_to_host(self.keys, self.vals)
        self.keys = None
        self.vals = None

    def spill_to_disk(self, path):
        """Host -> NVMe file (raw little-endian columns, no pickle)."""
        if self._host is None:
            return
        self._wait_spill()
        hk, hv = self._host
        with open(path, "wb") as fh:
            hk.numpy().tofile(fh)
            if self.has_sv:
                hv.offs.numpy().tofile(fh)
                hv.blob.numpy().tofile(fh)
            else:
                hv.numpy().tofile(fh)
        self._disk = path
        self._host = None
        _unpin((hk, hv))

    def _load_host(self):
        if self._host is None and self._disk is not None:
            def _readinto(fh, numel, dtype):
                t = _PIN.get(numel, dtype)
                if numel:
                    mv = memoryview(t.numpy()).cast("B")
                    got = fh.readinto(mv)
                    assert got == len(mv), "short spill-file read"
                return t

            with open(self._disk, "rb") as fh:
                hk = _readinto(fh, self.n, torch.int64)
                if self.has_sv:
                    ho = _readinto(fh, self.n + 1, torch.int64)
                    hb = _readinto(fh, self._blob, torch.uint8)
                    hv = StrVals(hb, ho)
                else:
                    hv = _readinto(fh, self.n, self.vdtype)
            self._unlink()
            self._host = (hk, hv)

    def _unlink(self):
        """Remove the spill file, if there is one."""
        if self._disk is not None:
            try:
                os.unlink(self._disk)
            except OSError:
                pass
            self._disk = None

    def load(self, device):
        if self.keys is None:
            self._wait_spill()
            self._wait_io()
            self._load_host()
            hk, hv = self._host
            self.keys = hk.to(device, non_blocking=True)
            self.vals = hv.to(device, non_blocking=True)
            self._host = None
            if torch.device(device).type == "cuda":
                evt = torch.cuda.Event()
                evt.record(torch.cuda.current_stream(device))
                _unpin((hk, hv), evt)
        return self


class HbmPool(object):
    """Two-watermark tier governor over run bytes (the reference's
    MemoryChecker/MaxMemoryWriter analog, memory.py:72-113, re-expressed
    over tiers): device-resident bytes above ``capacity`` spill to pinned
    host; host-resident bytes above ``host_capacity`` spill on to raw
    NVMe files under ``spill_dir``."""

    def __init__(self, capacity_bytes, host_capacity=None, spill_dir=None):
        import uuid
        self.capacity = capacity_bytes
        self.used = 0
        # ordered sets (insertion-ordered dicts): O(1) add/remove/contains
        # — a 2 TB job at 128 MB runs is ~16k live runs, list.remove per
        # touch would be O(n) scans on every access
        self._lru = {}                 # device-resident, insertion order
        self.host_capacity = (host_capacity
                              if host_capacity is not None
                              else float("inf"))
        self.host_used = 0
        self._host_lru = {}
        self.spill_dir = spill_dir or settings.spill_dir
        # dedicated D2H stream: evictions overlap main-stream compute
        # (set by the engine on CUDA devices; None = synchronous spill)
        self.spill_stream = None
        self._run_tag = "dampr_amd_{}".format(uuid.uuid4().hex[:10])
        self._file_ctr = 0
        self._disk_paths = []
        self.spilled_host = 0
        self.spilled_disk = 0
        self.reloaded = 0
        self.clean_bytes = 0       # resident runs with a host copy
        from collections import deque
        self._wb_queue = deque()   # writeback candidates, admit order
        self._io = None            # lazy ThreadPoolExecutor (NVMe IO)

    def _executor(self):
        if self._io is None:
            from concurrent.futures import ThreadPoolExecutor
            self._io = ThreadPoolExecutor(max_workers=2)
        return self._io

    def _next_path(self):
        os.makedirs(self.spill_dir, exist_ok=True)
        self._file_ctr += 1
        p = os.path.join(
            self.spill_dir,
            "{}_{}.run".format(self._run_tag, self._file_ctr))
        self._disk_paths.append(p)
        return p

    def cleanup(self):
        """Unlink any spill files still on disk (runs never paged back
        before the job finished)."""
        if self._io is not None:
            self._io.shutdown(wait=True)
            self._io = None
        for p in self._disk_paths:
            try:
                os.unlink(p)
            except OSError:
                pass
        self._disk_paths = []

    def stats(self):
        return {"hbm_used": self.used, "host_used": self.host_used,
                "spilled_to_host_bytes": self.spilled_host,
                "spilled_to_disk_bytes": self.spilled_disk,
                "reloads_bytes": self.reloaded}

    def admit(self, run):
        self.used += run.nbytes
        self._lru[run] = None
        self._wb_queue.append(run)
        self.balance()

    def prefetch(self, runs, device, stream):
        """Begin paging spilled runs back on a side HIP stream (overlaps
        the H2D copies with the current partition's compute).  The caller
        must make its stream wait on ``stream`` before consuming."""
        if stream is None:
            return
        main = torch.cuda.current_stream(device)
        # disk-resident runs: stage file -> pinned on the IO thread NOW
        # (the H2D happens at touch); host-resident runs take the H2D
        # side-stream path below
        for run in runs:
            if run.resident or run._lfut is not None:
                continue
            if run.on_disk or run._dfut is not None:
                run._lfut = self._executor().submit(run._stage_host)
        with torch.cuda.stream(stream):
            for run in runs:
                if run.resident or run._lfut is not None \
                        or run._dfut is not None or run.on_disk:
                    continue
                if run in self._host_lru:
                    del self._host_lru[run]
                    self.host_used -= run.nbytes
                self.reloaded += run.nbytes
                run.load(device)
                # tensors are allocated on the side stream but consumed
                # on the main stream: mark the cross-stream use so the
                # caching allocator does not reuse them early
                run.keys.record_stream(main)
                run.vals.record_stream(main)
                self.used += run.nbytes
                self._lru[run] = None
        # NOTE: no balance() here — eviction during an in-flight copy
        # could spill the very runs being loaded; the next touch() call
        # rebalances on the main stream.

    def touch(self, run, device):
        """Page the run in (if spilled) and refresh it to MRU.  ``used``
        counts every tracked resident run: a touched run stays tracked
        and evictable, there is no matching "done with it" call."""
        if not run.resident:
            if run in self._host_lru:
                del self._host_lru[run]
                self.host_used -= run.nbytes
            self.reloaded += run.nbytes
            run.load(device)
            self.used += run.nbytes
            self._lru[run] = None
            self._wb_queue.append(run)
            self.balance(exclude=run)
        elif run in self._lru:
            del self._lru[run]          # MRU refresh
            self._lru[run] = None
        return run

    def columns(self, run, device):
        """The run's (keys, vals) on ``device``: ``touch`` it, then hand
        out both references at once.  They stay valid when a later call
        evicts the run — eviction only drops the run's own references —
        so this is how the engine reads a run; reading ``run.keys``
        after another ``touch`` may find None."""
        self.touch(run, device)
        return run.keys, run.vals

    def forget(self, run):
        """Remove a run from all tier tracking (it is being freed)."""
        if run in self._lru:
            del self._lru[run]
            if run.resident:
                self.used -= run.nbytes
                if run.clean:
                    self.clean_bytes -= run.nbytes
        if run in self._host_lru:
            del self._host_lru[run]
            self.host_used -= run.nbytes

    def free(self, run):
        """Free a run on whatever tier holds it: out of the accounting,
        storage released (joins its in-flight spill and disk IO), spill
        file unlinked."""
        self.forget(run)
        run.drop()
        run._unlink()

    def balance(self, exclude=None):
        # background WRITEBACK above the half-full watermark: LRU runs
        # copy to pinned host while still resident (runs are immutable,
        # so the copy never goes stale); their later eviction is a
        # pointer drop.  Without this, a larger pool defers all D2H
        # into bursts that serialize against the reduce phase's
        # reloads (measured 2x wall at 120 GB with a 32 GB pool).
        if self.spill_stream is not None \
                and self.used > self.capacity // 2 \
                and self.clean_bytes * 2 < self.capacity:
            # FIFO candidate queue (admit order ~ LRU): O(1) amortized
            # — scanning the LRU dict would walk its clean prefix on
            # every admit
            wrote = 0
            while wrote < 4 and self._wb_queue \
                    and self.clean_bytes * 2 < self.capacity:
                r = self._wb_queue.popleft()
                if r is exclude:
                    self._wb_queue.append(r)
                    break
                if not r.resident or r._host is not None \
                        or r not in self._lru:
                    continue            # freed/evicted/already clean
                r.writeback_async(self.spill_stream)
                self.clean_bytes += r.nbytes
                wrote += 1
        while self.used > self.capacity and self._lru:
            victim = None
            for r in self._lru:
                if r is not exclude and r.resident:
                    victim = r
                    break
            if victim is None:
                return
            del self._lru[victim]
            self.used -= victim.nbytes
            if victim.clean:
                self.clean_bytes -= victim.nbytes
            victim.spill_async(self.spill_stream)
            self.spilled_host += victim.nbytes
            self.host_used += victim.nbytes
            self._host_lru[victim] = None
        while self.host_used > self.host_capacity and self._host_lru:
            v = next(iter(self._host_lru))
            del self._host_lru[v]
            self.host_used -= v.nbytes
            self.spilled_disk += v.nbytes
            path = self._next_path()
            if self.spill_stream is None:
                v.spill_to_disk(path)      # CPU/test path stays sync
            else:
                # NVMe writes ride an IO thread, overlapped with
                # compute; readers join via _wait_io
                v._dfut = self._executor().submit(v.spill_to_disk, path)
