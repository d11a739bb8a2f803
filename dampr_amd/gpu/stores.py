"""Columnar data types of the device engine: the inputs it ingests
(``ColumnSource``, ``TextSource``), the stores its stages hand to each
other (``PartStore``, ``TokenStore``, ``HostStore``, ``SinkStore``) and the
datasets it returns (``ColumnDataset``, ``TokenColumnDataset``).  Nothing
here needs a GPU."""
import collections.abc

import torch

_VAL_DTYPES = (torch.int64, torch.float64)


def _as_column(x, device=None, dtype=None):
    """device=None keeps a torch input where it lives (an HBM-resident
    tensor must not bounce through the host)."""
    if isinstance(x, torch.Tensor):
        t = x
    else:
        import numpy as np
        t = torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype not in _VAL_DTYPES:
        t = t.to(torch.float64 if t.is_floating_point() else torch.int64)
    if dtype is not None:
        t = t.to(dtype)
    return t if device is None else t.to(device)


def encode_f64_sortable(x):
    """Map float64 to i64 bit patterns whose unsigned order is the float
    order (IEEE trick): sortable keys for float group/sort/top-k columns.
    ``+ 0.0`` canonicalizes -0.0 to +0.0 first (Python == merges them as
    one group key; distinct bit patterns would split it) and leaves every
    other value, NaN included, unchanged."""
    b = (x + 0.0).view(torch.int64)
    sign_bit = -(1 << 63)
    return torch.where(b < 0, ~b, b ^ sign_bit)


def decode_f64_sortable(enc):
    """Inverse of encode_f64_sortable."""
    sign_bit = -(1 << 63)
    b = torch.where(enc < 0, enc ^ sign_bit, ~enc)
    return b.view(torch.float64)


class ColumnSource(object):
    """A device-columnar input: (keys i64, vals i64|f64).  String key
    arrays dictionary-encode at ingest (np.unique: sorted uniques +
    inverse ids, so rank order == lexicographic order); the table is
    built from the FULL input before any per-rank slicing, so every
    rank shares one dictionary."""

    dampr_columnar = True          # engine-selection sentinel (dampr.py)

    def __init__(self, keys, vals, str_table=None, fkeys=False):
        assert keys.dtype == torch.int64
        assert getattr(vals, "is_strvals", False) \
            or vals.dtype in _VAL_DTYPES
        assert keys.numel() == vals.numel()
        self.keys = keys
        self.vals = vals
        self.str_table = str_table
        # keys hold the f64 order-preserving encode (decoded on read)
        self.fkeys = fkeys

    @staticmethod
    def _is_str_array(x):
        import numpy as np
        if isinstance(x, np.ndarray):
            return x.dtype.kind in ("U", "S") or (
                x.dtype.kind == "O" and x.size
                and all(isinstance(e, str) for e in x.flat))
        return (isinstance(x, (list, tuple)) and len(x)
                and all(isinstance(e, str) for e in x))

    @classmethod
    def from_data(cls, vals, keys=None, device=None):
        import numpy as np
        if cls._is_str_array(vals):
            # var-len value arena: strings move as opaque bytes
            # addressed by row; only keys compare on device
            from .strvals import StrVals
            arr = np.asarray(vals)
            if arr.dtype.kind == "S":
                arr = arr.astype("U")
            v = StrVals.from_strings([str(s) for s in arr.flat],
                                     device=device)
        else:
            v = _as_column(vals, device)
        str_table = None
        fkeys = False
        if keys is None:
            k = torch.arange(v.numel(), dtype=torch.int64, device=v.device)
        elif (isinstance(keys, torch.Tensor)
              and keys.dtype.is_floating_point) or (
                  isinstance(keys, np.ndarray)
                  and keys.dtype.kind == "f"):
            # float keys: order-preserving f64 encode, NOT an int cast
            # (which would silently truncate 1.5 and 2.5 into key 1)
            kf = keys.to(torch.float64) if isinstance(keys, torch.Tensor) \
                else torch.from_numpy(keys.astype(np.float64))
            if kf.device != v.device:
                kf = kf.to(v.device)
            k = encode_f64_sortable(kf)
            fkeys = True
        elif cls._is_str_array(keys):
            arr = np.asarray(keys)
            if arr.dtype.kind == "S":
                arr = arr.astype("U")
            uniq, inv = np.unique(arr, return_inverse=True)
            str_table = tuple(str(u) for u in uniq)
            k = torch.from_numpy(inv.astype(np.int64))
            if device is not None or k.device != v.device:
                k = k.to(v.device)
        else:
            k = _as_column(keys, device, torch.int64)
            if k.device != v.device:
                k = k.to(v.device)
        return cls(k, v, str_table=str_table, fkeys=fkeys)


class TextSource(object):
    """Newline-delimited text input for the device engine: the
    ``device_text(...).flat_map(funcs.tokenize_set).count()`` idiom lowers
    onto the fused single-pass document-frequency kernel (gpu/tfidf.py)."""

    dampr_columnar = True

    def __init__(self, data):
        import numpy as np
        self.text_t = None             # device-resident u8 tensor, if given
        self._text_np = None
        if isinstance(data, torch.Tensor):
            assert data.dtype == torch.uint8
            self.text_t = data
        elif isinstance(data, str):
            with open(data, "rb") as fh:
                raw = fh.read()
            self._text_np = np.frombuffer(raw, dtype=np.uint8).copy()
        elif isinstance(data, bytes):
            self._text_np = np.frombuffer(data, dtype=np.uint8).copy()
        else:
            self._text_np = np.asarray(data, dtype=np.uint8)

    @property
    def nbytes(self):
        return (self.text_t.numel() if self.text_t is not None
                else self._text_np.nbytes)

    @property
    def text(self):
        """Host view (materialized on demand for fallback paths)."""
        if self._text_np is None:
            self._text_np = self.text_t.cpu().numpy()
        return self._text_np


class _StoreMeta(object):
    """Column metadata every stage output declares; the runner reads
    these as plain attributes.  The defaults describe a store with no
    columnar layout (``PartStore`` sets all of them per instance)."""

    keyed = False          # records follow the keyed-reducer convention
    fkeys = False          # key column is the f64 sortable encoding
    svals = False          # value column is a var-len byte arena
    str_table = None       # dictionary of string keys, if encoded
    vdtype = None          # value dtype every rank agrees on, if known
    partitioned = True     # runs are routed to hash partitions


class TokenStore(_StoreMeta):
    """Result of the fused text document-frequency stage: token-hash keys
    + counts, with the string dictionary needed to materialize tokens."""

    def __init__(self, engine, keys, vals, text_dev):
        self.engine = engine
        self.keys = keys
        self.vals = vals
        self.text_dev = text_dev


class TokenColumnDataset(object):
    """ColumnDataset analog whose keys decode to token strings via the
    device string dictionary."""

    def __init__(self, store, keyed):
        self.store = store
        self.keyed = keyed

    def read(self):
        st = self.store
        blob, lens = st.engine.token_strings(st.keys, st.text_dev)
        vals = st.vals.cpu().tolist()
        out = []
        pos = 0
        b = blob.tobytes()
        for i, ln in enumerate(lens):
            tok = b[pos:pos + int(ln)].decode("ascii")
            pos += int(ln)
            if self.keyed:
                out.append((tok, (tok, vals[i])))
            else:
                out.append((tok, vals[i]))
        out.sort(key=lambda r: r[0])
        return iter(out)

    def grouped_read(self):
        import itertools
        for key, group in itertools.groupby(self.read(),
                                            key=lambda p: p[0]):
            yield key, (v for _k, v in group)

    def delete(self):
        self.store = None

    def __iter__(self):
        return self.read()


class StrTable(collections.abc.Sequence):
    """Lazy, read-only dictionary of string keys: a Sequence over a
    ``StrVals`` arena whose row i is the string of key id i.  It stands
    wherever a ``str_table`` tuple does (``len``, indexing, slicing to a
    tuple, iteration, ``==`` against a tuple or another ``StrTable`` by
    contents), but the strings stay on the arena's device until someone
    reads keys: the first access that needs them does one copy to the
    host and one decode into a cached tuple, then drops the arena.
    ``len()`` does not materialise.

    Until that first read the arena is O(U) bytes of device memory that
    the HBM pool does not account for."""

    __slots__ = ("_sv", "_n", "_strs", "_enc")

    def __init__(self, sv):
        self._sv = sv
        self._n = sv.numel()
        self._strs = None
        self._enc = None

    @property
    def materialized(self):
        return self._strs is not None

    def _tuple(self):
        if self._strs is None:
            self._strs = tuple(self._sv.tolist())
            self._sv = None
        return self._strs

    def bounds(self, const_bytes, ops=None):
        """``(lo, hi)``: how many keys are smaller than ``const_bytes``,
        and how many are smaller or equal, as UTF-8 bytes (the order of
        the key ids).  Key ids are ranks, so ``[lo, hi)`` is the id range
        of the constant itself (empty when it is no key).  While the
        strings are on the device this counts there
        (``ops.sv_count_rows``) and does not materialise them; once they
        are on the host it bisects them."""
        if self._strs is None:
            if ops is None:
                from .backend import ops_for
                ops = ops_for(self._sv.device)
            c = bytes(const_bytes)
            return (ops.sv_count_rows(self._sv, [(1, "str", "lt", c, b"")]),
                    ops.sv_count_rows(self._sv, [(1, "str", "le", c, b"")]))
        if self._enc is None:
            self._enc = [s.encode("utf-8") for s in self._strs]
        return table_bounds(self._enc, const_bytes)

    def ids_of(self, members, ops=None):
        """The key ids of those of ``members`` (distinct UTF-8 ``bytes``)
        that are keys, ascending.  While the strings are on the device
        this is one string-set filter of ``(arange(U), arena)``
        (``ops.sv_filter_rows`` with an "isin" clause) whose surviving
        keys are the ids: no launch per member, and the table does not
        materialise.  Once they are on the host it bisects them."""
        members = [bytes(m) for m in members]
        if not members or not self._n:
            return []
        if self._strs is None:
            if ops is None:
                from .backend import ops_for
                ops = ops_for(self._sv.device)
            ids = torch.arange(self._n, dtype=torch.int64,
                               device=self._sv.device)
            kept, _sv = ops.sv_filter_rows(
                ids, self._sv, [(1, "str", "isin", members, None)])
            return kept.cpu().tolist()
        if self._enc is None:
            self._enc = [s.encode("utf-8") for s in self._strs]
        found = (table_bounds(self._enc, m) for m in members)
        return sorted(lo for lo, hi in found if hi > lo)

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        return self._tuple()[i]

    def __iter__(self):
        return iter(self._tuple())

    def __eq__(self, other):
        if isinstance(other, StrTable):
            return other is self or self._tuple() == other._tuple()
        if isinstance(other, tuple):
            return self._tuple() == other
        return NotImplemented

    def __repr__(self):
        return "StrTable({} keys, {})".format(
            self._n, "materialized" if self.materialized else "on device")


def table_bounds(sorted_bytes, const_bytes):
    """``StrTable.bounds`` over a sorted list of ``bytes`` keys."""
    import bisect
    c = bytes(const_bytes)
    return (bisect.bisect_left(sorted_bytes, c),
            bisect.bisect_right(sorted_bytes, c))


class PartStore(_StoreMeta, dict):
    """{partition -> [DeviceRun]} plus column metadata:

    * ``keyed``: output of a keyed reducer — records follow the host
      convention (k, (k, v)) at decode time (base.py KeyedReduce).
    * ``fkeys``: the key column is an order-preserving i64 encoding of
      float64 keys (encode_f64_sortable); decoded on read.
    """

    def __init__(self, keyed=False, fkeys=False, partitioned=True,
                 str_table=None, svals=False, vdtype=None):
        super(PartStore, self).__init__()
        self.keyed = keyed
        self.fkeys = fkeys
        # value columns are var-len byte arenas (StrVals).  Kept as a
        # STORE-level flag (not just per-run inspection) so an empty
        # rank's store still reports it: stage-dispatch guards must
        # agree across ranks or collective sequences desync.
        self.svals = svals
        # dictionary-encoded string keys: key column holds ranks into
        # this sorted tuple or StrTable (rank order == lexicographic
        # order, so sorted device output decodes to host-ordered
        # strings).  Cross-store
        # combinations remap ids into the union table on device
        # (_unify_str_stores); only dictionary + dictionary-less mixes
        # fall back to host records (_decode_store).
        self.str_table = str_table
        # False = runs in pseudo-partition 0, not yet routed by key hash
        # (lazy ingest: stages that need co-partitioned data call
        # _ensure_partitioned; record-wise maps stream run by run)
        self.partitioned = partitioned
        # value dtype of the numeric value column (None: var-len or
        # unknown).  Store metadata, so a rank holding no rows still
        # builds empty columns of the dtype the other ranks exchange.
        self.vdtype = vdtype


class HostStore(_StoreMeta, list):
    """Fallback record storage: a plain list of (k, v) Python records for
    stages whose outputs don't fit typed columns.  Downstream stages run
    on the host until records become numeric again (then they re-enter the
    columnar path via _encode_or_host)."""


class SinkStore(_StoreMeta):
    """A sink stage's output: lazy view over the durable text part
    files it wrote (host parity — _SinkWorker returns its
    TextLineDatasets, so a sink's output is readable downstream without
    re-materializing the sunk bytes; reference: the sink's
    TextLineDataset handles flow back as normal data,
    dampr/dataset.py:280-282, runner.py:195-197)."""

    def __init__(self, paths):
        self.paths = paths

    def datasets(self):
        from ..dataset import TextLineDataset
        return [TextLineDataset(p) for p in self.paths]


def _is_sv(x):
    """Is this value column a var-len byte arena (gpu.strvals.StrVals)?"""
    return getattr(x, "is_strvals", False)


def _cat_vals(vs):
    """Concatenate value columns (tensor or StrVals, never mixed)."""
    if len(vs) == 1:
        return vs[0]
    if any(_is_sv(v) for v in vs):
        from .strvals import StrVals
        assert all(_is_sv(v) for v in vs), \
            "mixed var-len and numeric value runs in one partition"
        return StrVals.cat(vs)
    return torch.cat(vs)


def _store_has_sv(store):
    if not isinstance(store, PartStore):
        return False
    return store.svals or any(
        r.has_sv for runs in store.values() for r in runs)


class ColumnDataset(object):
    """Dataset-duck-typed view over result columns: read() yields (k, v)
    Python scalars; columns() hands back the tensors for zero-copy
    composition.  ``keyed`` reproduces the host reducers' value
    convention (k, (k, v)); ``fkeys`` decodes float64 keys."""

    def __init__(self, keys, vals, keyed=False, fkeys=False,
                 str_table=None):
        self.keys_t = keys
        self.vals_t = vals
        self.keyed = keyed
        self.fkeys = fkeys
        self.str_table = str_table

    def columns(self):
        return self.keys_t, self.vals_t

    def read(self):
        from .records import decode      # records imports this module
        return iter(decode(self.keys_t, self.vals_t, self.keyed,
                           self.fkeys, self.str_table))

    def grouped_read(self):
        import itertools
        for key, group in itertools.groupby(self.read(), key=lambda p: p[0]):
            yield key, (v for _k, v in group)

    def delete(self):
        self.keys_t = self.vals_t = None

    def __iter__(self):
        return self.read()
