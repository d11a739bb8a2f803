"""Device-op backends for the columnar engine.

Two implementations of one small interface (sort, segmented reduce, hash
join, partition histogram):

* ``HipOps`` — the hand-written gfx950 kernels (ops/hip/*.hip) via the
  dampr_hip extension.  **The only backend allowed on a CUDA device**: if
  the extension is missing on a GPU box this raises instead of silently
  falling back to eager PyTorch.
* ``TorchOps`` — a plain-PyTorch oracle used (a) as the CPU reference the
  HIP kernels are numerics-tested against and (b) to run the full engine
  logic in the no-GPU CI (tests/, gloo world>1).

Pick with ``ops_for(device)``.
"""
import torch

from .filters import (FILTER_MAX_CLAUSES,  # noqa: F401 - re-exported
                      SET_OPS, SV_FILTER_MAX_CONST, _I64_MAX, _I64_MIN,
                      check_clauses, check_row_count)

OP_SUM, OP_MIN, OP_MAX = 0, 1, 2
_OP_IDS = {"sum": OP_SUM, "min": OP_MIN, "max": OP_MAX}


def ops_for(device):
    device = torch.device(device)
    if device.type == "cuda":
        return HipOps()
    return TorchOps()


def _dict_encode_host(sv):
    """Exact dictionary encode of a StrVals column on the host, over raw
    row BYTES (so rows that differ only in trailing NULs, or that are not
    valid UTF-8, stay distinct).  Returns CPU ``(ids i64[n], uniq
    StrVals[U])``; uniques come out in byte order."""
    import numpy as np
    from .strvals import StrVals
    n = sv.numel()
    if n == 0:
        return torch.zeros(0, dtype=torch.int64), StrVals.empty()
    data = sv.blob.cpu().numpy().tobytes()
    offs = sv.offs.cpu().numpy()
    rows = np.empty(n, dtype=object)
    rows[:] = [data[offs[i]:offs[i + 1]] for i in range(n)]
    uq, inv = np.unique(rows, return_inverse=True)
    lens = np.fromiter((len(b) for b in uq), dtype=np.int64, count=len(uq))
    uoffs = np.zeros(len(uq) + 1, dtype=np.int64)
    np.cumsum(lens, out=uoffs[1:])
    ublob = np.frombuffer(b"".join(uq), dtype=np.uint8).copy()
    ids = torch.from_numpy(np.ascontiguousarray(
        inv.reshape(-1).astype(np.int64)))
    return ids, StrVals(torch.from_numpy(ublob), torch.from_numpy(uoffs))


class _OpsBase(object):
    # batches dict_encode re-encoded exactly on the host (hash collision)
    dict_encode_host_batches = 0
    # refinement rounds str_rank ran on device, summed over its calls
    str_rank_rounds = 0

    def sort_pairs(self, keys, payload=None):
        raise NotImplementedError

    def str_rank(self, sv):
        """Byte-lexicographic rank of the rows of a var-len string column
        (StrVals): returns ``rank``, an i64 tensor of n entries on
        ``sv``'s device, where ``rank[i]`` is the number of rows of
        ``sv`` strictly smaller than row i.  Rows compare as unsigned
        bytes and a proper prefix is smaller; trailing and embedded NUL
        bytes are ordinary bytes (b"ab" < b"ab\\0", b"" < b"\\0").  For
        distinct rows ``rank`` is a permutation of [0, n); equal rows get
        equal ranks.  n == 0 returns an empty tensor; n >= 2**31 raises
        OverflowError.  For valid UTF-8 rows this is Python ``str``
        order."""
        raise NotImplementedError

    def dict_encode(self, sv):
        """Dictionary-encode a var-len string column (StrVals): returns
        ``(ids i64[n], uniq StrVals[U])`` with ids dense in [0, U) and
        ``uniq`` row i the string of id i.  The id order is unspecified."""
        raise NotImplementedError

    def seg_reduce_sorted(self, sorted_keys, vals, op="sum"):
        raise NotImplementedError

    def filter_rows(self, keys, vals, clauses):
        """Rows of (keys i64[n], vals i64|f64[n]) that satisfy EVERY
        clause: returns ``(keys', vals')`` holding the surviving rows in
        input order (a stable compaction), with exactly the inputs'
        dtypes and device.  ``clauses`` is a sequence of 1 to
        ``FILTER_MAX_CLAUSES`` resolved
        ``(col, domain, op, a, b)``:

        * ``col`` 0 reads the key column, 1 the value column;
        * ``domain`` "i64" compares the column as signed integers against
          int constants; "f64" (an f64 value column) compares IEEE
          doubles against float constants, so a NaN row fails everything
          but ``ne``; "fkey" (an i64 column holding
          ``encode_f64_sortable`` doubles) decodes each word, then
          compares as "f64";
        * ``op`` is gt/ge/lt/le/eq/ne against ``a``, or "between":
          ``a <= x <= b``.  ``b`` is ignored otherwise;
        * ``op`` "isin" / "notin" is a set clause
          ``(col, domain, op, members, None)``: ``members`` is a 1-D CPU
          i64 tensor of distinct words, the integers for "i64", the bit
          patterns of the doubles for "f64" / "fkey" with -0.0 given as
          0.0 and no NaN.  A row is a member when its value equals one:
          +-0.0 rows are the member 0.0, a NaN row is never a member
          ("isin" false, "notin" true).  At most one set clause per
          column; "f64" exactly over an f64 value column.

        ``clauses`` may also be what ``filter_compile`` made of such a
        sequence.  A malformed program raises ValueError.  n == 0 returns
        empty columns; n >= 2**31 rows, or a set of more than 2**30
        members, raises OverflowError before any launch."""
        raise NotImplementedError

    def sv_filter_rows(self, keys, svals, clauses):
        """``filter_rows`` over (keys i64[n], svals StrVals[n]): returns
        ``(keys', StrVals')`` holding the rows that satisfy EVERY clause,
        in input order, on the inputs' device.  The result's arena is
        fresh and compact: ``offs[0] == 0`` and
        ``blob.numel() == offs[-1]``.  ``clauses`` is a sequence of 1 to
        ``FILTER_MAX_CLAUSES`` resolved ``(col, domain, op, a, b)``, or
        what ``sv_filter_compile`` made of one:

        * ``col`` 0, ``domain`` "i64" or "fkey": a key clause, exactly as
          in ``filter_rows``;
        * ``col`` 1, ``domain`` "str": compares the row's bytes against
          ``bytes`` constants of at most ``SV_FILTER_MAX_CONST`` bytes in
          ``str_rank``'s order (unsigned bytes, a proper prefix is
          smaller, NUL is an ordinary byte).  ``op`` is gt/ge/lt/le/eq/ne
          against ``a``; "between": ``a <= row <= b``; or "startswith":
          ``a`` is a prefix of the row (the empty prefix keeps every
          row).  ``b`` is ignored unless the op is "between";
        * ``col`` 1, ``domain`` "str", ``op`` "isin" / "notin": a set
          clause ``(1, "str", op, members, None)`` with ``members`` a
          sequence of distinct ``bytes`` of any length; a row is a member
          when its bytes equal one's exactly.  A key set clause is as in
          ``filter_rows``.  At most one set clause per column.

        Any other clause, or a longer constant, raises ValueError.
        n == 0 returns empty columns; n >= 2**31 raises OverflowError
        before any launch."""
        raise NotImplementedError

    def sv_count_rows(self, svals, clauses):
        """How many rows of ``svals`` (StrVals[n]) satisfy EVERY clause:
        an int.  ``clauses`` as in ``sv_filter_rows``, "str" clauses
        only (there is no key column; a key clause raises ValueError).
        n == 0 returns 0; n >= 2**31 raises OverflowError before any
        launch."""
        raise NotImplementedError

    def filter_compile(self, clauses, values, device):
        """``clauses`` (resolved, for a "numeric" or "string" ``values``
        column) in a form that ``filter_rows`` / ``sv_filter_rows`` /
        ``sv_count_rows`` take in their place and reuse across calls on
        ``device``: the string kernels' constant buffer and the device
        hash sets of the set clauses are then built once per filter stage
        and program, not per run.  A set's tables are O(members) bytes of
        device memory that the HBM pool does not account for; they live
        as long as the compiled program does."""
        check_clauses(clauses, values, "filter_compile")
        return clauses

    def sv_filter_compile(self, clauses, device):
        """``filter_compile`` for a string value column."""
        return self.filter_compile(clauses, "string", device)

    def hash_join(self, keys_l, keys_r, how="inner", table=None):
        raise NotImplementedError

    def hash_join_build(self, keys_r):
        """Opaque reusable build-side state for batched probing."""
        return None

    def probe_order(self, keys):
        """Optional probe-locality permutation (None = keep order)."""
        return None

    def merge_sorted_runs(self, ks, fkeys=False):
        """K-way merge of key-sorted runs (K4).  ``ks`` is a list of
        runs each already in host-ascending order (signed for i64 keys,
        encoded-unsigned for fkeys).  Returns (merged_keys, perm) where
        perm indexes into the runs' concatenation.  Stable: ties keep
        run order, then within-run order."""
        raise NotImplementedError

    # shared helpers ------------------------------------------------------

    def partition_of(self, keys, n_partitions):
        """Partition id per key: hash-mix then mod (K1).  Must agree across
        backends so CPU tests predict device placement."""
        # splitmix64-style finalizer over the i64 bit pattern
        x = keys.to(torch.int64)
        x = x ^ (x >> 30)
        x = x * -4658895280553007687          # 0xbf58476d1ce4e5b9 as i64
        x = x ^ (x >> 27)
        x = x * -7723592293110705685          # 0x94d049bb133111eb as i64
        x = x ^ (x >> 31)
        return torch.remainder(x, n_partitions)

    def group_reduce(self, keys, vals, op="sum"):
        """Unsorted group-by reduce: sort then segmented reduce."""
        sk, sp = self.sort_pairs(keys)
        sv = vals[sp.to(torch.int64)]
        return self.seg_reduce_sorted(sk, sv, op)

    @staticmethod
    def segment_ids(sorted_keys):
        n = sorted_keys.numel()
        if n == 0:
            z = torch.zeros(0, dtype=torch.int64, device=sorted_keys.device)
            return z, sorted_keys
        flags = torch.ones(n, dtype=torch.int64, device=sorted_keys.device)
        flags[1:] = (sorted_keys[1:] != sorted_keys[:-1]).to(torch.int64)
        seg = torch.cumsum(flags, 0) - 1
        uniq = sorted_keys[flags.bool()]
        return seg, uniq


class HipOps(_OpsBase):
    """gfx950 HIP kernel backend (see gpu/relational.py docstrings for the
    kernel-level notes)."""

    def __init__(self):
        from ..ops import native
        self.ext = native.require()

    def sort_pairs(self, keys, payload=None):
        from .relational import radix_sort_pairs
        return radix_sort_pairs(keys, payload)

    def seg_reduce_sorted(self, sorted_keys, vals, op="sum"):
        from .relational import group_reduce_sorted
        return group_reduce_sorted(sorted_keys, vals, _OP_IDS[op])

    def filter_rows(self, keys, vals, clauses):
        from .relational import filter_rows
        return filter_rows(keys, vals, clauses)

    def sv_filter_rows(self, keys, svals, clauses):
        from .relational import sv_filter_rows
        return sv_filter_rows(keys, svals, clauses)

    def sv_count_rows(self, svals, clauses):
        from .relational import sv_count_rows
        return sv_count_rows(svals, clauses)

    def filter_compile(self, clauses, values, device):
        from .relational import filter_compile
        return filter_compile(clauses, values, device)

    def hash_join(self, keys_l, keys_r, how="inner", table=None):
        from .relational import hash_join
        return hash_join(keys_l, keys_r, how, table=table)

    def hash_join_build(self, keys_r):
        from .relational import hj_build_table
        return hj_build_table(keys_r)

    def dict_encode(self, sv):
        from .. import settings
        from .relational import dict_encode_strs
        ids, uniq, collided = dict_encode_strs(sv, settings.str_hash_mask)
        if collided:
            # two different strings share a 64-bit hash: this batch's
            # ids are invalid, re-encode it exactly (the batch tensors
            # are still live; nothing upstream restarts)
            self.dict_encode_host_batches += 1
            ids, uniq = _dict_encode_host(sv)
            dev = sv.blob.device
            ids, uniq = ids.to(dev), uniq.to(dev)
        return ids, uniq

    def str_rank(self, sv):
        from .relational import lex_rank_strs
        rank, rounds = lex_rank_strs(sv)
        self.str_rank_rounds += rounds
        return rank

    def probe_order(self, keys):
        """Permutation clustering probe keys by their low bits (hash
        slot = key & mask): probes then walk L2-resident table regions
        instead of random HBM lines.  Two low-byte passes give 64K-key
        clusters (~1 MB table window each)."""
        if keys.numel() < (1 << 20):
            return None
        from .relational import radix_sort_pairs
        _k, perm = radix_sort_pairs(keys, low_passes=2)
        return perm.to(torch.int64)

    def merge_sorted_runs(self, ks, fkeys=False):
        total = sum(k.numel() for k in ks)
        if total >= (1 << 31):      # u32 payload limit (same as sort)
            raise OverflowError("merge payload exceeds u32")
        dev = ks[0].device
        items = []
        base = 0
        for k in ks:
            p = torch.arange(base, base + k.numel(), dtype=torch.int32,
                             device=dev)
            items.append((k.contiguous(), p))
            base += k.numel()
        bias = 0 if fkeys else 1    # signed compare for raw i64 keys
        # pairwise merge tree over ADJACENT runs (keeps global stability)
        while len(items) > 1:
            nxt = []
            for a in range(0, len(items) - 1, 2):
                ka, pa = items[a]
                kb, pb = items[a + 1]
                n = ka.numel() + kb.numel()
                out_k = torch.empty(n, dtype=ka.dtype, device=dev)
                out_p = torch.empty(n, dtype=torch.int32, device=dev)
                self.ext.mp_merge(ka, pa, kb, pb, bias, out_k, out_p)
                nxt.append((out_k, out_p))
            if len(items) % 2:
                nxt.append(items[-1])
            items = nxt
        k, p = items[0]
        return k, p.to(torch.int64)


class TorchOps(_OpsBase):
    """Pure-torch oracle (CPU tests; never used on a CUDA device)."""

    def dict_encode(self, sv):
        ids, uniq = _dict_encode_host(sv)
        dev = sv.blob.device
        return ids.to(dev), uniq.to(dev)

    def str_rank(self, sv):
        """The exact host oracle: sort the rows' bytes, binary-search
        every row in the sorted list."""
        import numpy as np
        n = sv.numel()
        if n >= (1 << 31):
            raise OverflowError("str_rank: row count exceeds i32")
        dev = sv.blob.device
        if n == 0:
            return torch.zeros(0, dtype=torch.int64, device=dev)
        data = sv.blob.cpu().numpy().tobytes()
        offs = sv.offs.cpu().numpy()
        rows = np.empty(n, dtype=object)
        rows[:] = [data[offs[i]:offs[i + 1]] for i in range(n)]
        rank = np.searchsorted(np.sort(rows), rows, side="left")
        return torch.from_numpy(rank.astype(np.int64)).to(dev)

    def sort_pairs(self, keys, payload=None):
        n = keys.numel()
        if payload is None:
            payload = torch.arange(n, dtype=torch.int32, device=keys.device)
        if n <= 1:
            return keys.clone(), payload.clone()
        # unsigned order on the i64 bit pattern = flip sign bit, signed sort
        flipped = keys ^ _I64_MIN
        order = torch.argsort(flipped, stable=True)
        return keys[order], payload[order]

    def seg_reduce_sorted(self, sorted_keys, vals, op="sum"):
        seg, uniq = self.segment_ids(sorted_keys)
        n_seg = uniq.numel()
        if vals.dtype == torch.float64:
            init = {"sum": 0.0, "min": float("inf"),
                    "max": float("-inf")}[op]
        else:
            init = {"sum": 0, "min": _I64_MAX, "max": _I64_MIN}[op]
        out = torch.full((max(n_seg, 1),), init, dtype=vals.dtype,
                         device=vals.device)
        red = {"sum": "sum", "min": "amin", "max": "amax"}[op]
        out[:n_seg] = out[:n_seg].scatter_reduce(
            0, seg, vals, reduce=red, include_self=True)
        return uniq, out[:n_seg]

    @staticmethod
    def _numeric_mask(x, dom, op, a, b):
        """The oracle's keep mask of one numeric clause over column x."""
        from .stores import decode_f64_sortable
        if op in SET_OPS:
            # torch.isin over the decoded column: it takes +-0.0 as equal
            # and never matches NaN, which is the contract
            if dom != "i64":
                x = (decode_f64_sortable(x) if dom == "fkey" else x) + 0.0
                a = a.view(torch.float64)
            hit = torch.isin(x, a.to(x.device))
            return hit if op == "isin" else ~hit
        if dom == "i64":
            assert x.dtype == torch.int64
            a, b = int(a), int(b)
        else:
            x = decode_f64_sortable(x) if dom == "fkey" else x
            assert x.dtype == torch.float64
            a, b = float(a), float(b)
        if op == "between":
            return (x >= a) & (x <= b)
        return {"gt": torch.gt, "ge": torch.ge, "lt": torch.lt,
                "le": torch.le, "eq": torch.eq, "ne": torch.ne}[op](x, a)

    def filter_rows(self, keys, vals, clauses):
        """The oracle: a boolean mask per clause, ANDed, then indexed."""
        check_row_count("filter_rows", keys.numel())
        check_clauses(clauses, "numeric", "filter_rows", vals.dtype)
        mask = torch.ones(keys.numel(), dtype=torch.bool, device=keys.device)
        for col, dom, op, a, b in clauses:
            mask &= self._numeric_mask(vals if col else keys, dom, op, a, b)
        return keys[mask], vals[mask]

    def _sv_mask(self, keys, svals, clauses):
        """The oracle's keep mask: Python ``bytes`` comparisons (unsigned
        bytes, a proper prefix is smaller), row by row.  ``keys`` is None
        where there is no key column to read."""
        check_clauses(clauses, "string", "sv_filter_rows")
        if keys is None and any(c[0] == 0 for c in clauses):
            raise ValueError("sv_count_rows: a clause reads the key column")
        n = svals.numel()
        data = svals.blob.cpu().numpy().tobytes()
        offs = svals.offs.cpu().tolist()
        rows = [data[offs[i]:offs[i + 1]] for i in range(n)]
        mask = torch.ones(n, dtype=torch.bool)
        str_ops = {"gt": bytes.__gt__, "ge": bytes.__ge__,
                   "lt": bytes.__lt__, "le": bytes.__le__,
                   "eq": bytes.__eq__, "ne": bytes.__ne__,
                   "startswith": bytes.startswith}
        for col, dom, op, a, b in clauses:
            if dom == "str" and op in SET_OPS:
                members = set(bytes(m) for m in a)
                m = [(r in members) == (op == "isin") for r in rows]
                mask &= torch.tensor(m, dtype=torch.bool)
            elif dom == "str":
                a = bytes(a)
                if op == "between":
                    b = bytes(b)
                    m = [a <= r <= b for r in rows]
                else:
                    m = [str_ops[op](r, a) for r in rows]
                mask &= torch.tensor(m, dtype=torch.bool)
            else:
                mask &= self._numeric_mask(keys.cpu(), dom, op, a, b)
        return mask

    def sv_filter_rows(self, keys, svals, clauses):
        """The oracle: ``_sv_mask``, then index."""
        check_row_count("sv_filter_rows", keys.numel(), svals.numel())
        if svals.numel() != keys.numel():
            raise ValueError(
                "sv_filter_rows: keys and values differ in length")
        dev = keys.device
        mask = self._sv_mask(keys, svals, clauses).to(dev)
        idx = torch.nonzero(mask).flatten()
        return keys[idx], svals.gather(idx)

    def sv_count_rows(self, svals, clauses):
        check_row_count("sv_count_rows", svals.numel())
        return int(self._sv_mask(None, svals, clauses).sum().item())

    def merge_sorted_runs(self, ks, fkeys=False):
        keys = torch.cat(ks)
        ordk = (keys ^ _I64_MIN) if fkeys else keys
        perm = torch.argsort(ordk, stable=True)
        return keys[perm], perm

    def hash_join_build(self, keys_r):
        return self.sort_pairs(keys_r)

    def hash_join(self, keys_l, keys_r, how="inner", table=None):
        assert how in ("inner", "left", "outer")
        dev = keys_l.device
        # sort right side; binary-search each left key's run
        sr, pr = table if table is not None else self.sort_pairs(keys_r)
        fl = keys_l ^ _I64_MIN
        fr = sr ^ _I64_MIN
        lo = torch.searchsorted(fr, fl, side="left")
        hi = torch.searchsorted(fr, fl, side="right")
        counts = hi - lo
        matched_l = counts > 0
        if how in ("left", "outer"):
            counts = torch.where(matched_l, counts,
                                 torch.ones_like(counts))
        else:
            counts = torch.where(matched_l, counts,
                                 torch.zeros_like(counts))
        offs = torch.cumsum(counts, 0) - counts
        total = int(counts.sum().item())
        out_l = torch.empty(total, dtype=torch.int64, device=dev)
        out_r = torch.empty(total, dtype=torch.int64, device=dev)
        pos = torch.arange(total, device=dev)
        src = torch.repeat_interleave(
            torch.arange(keys_l.numel(), device=dev), counts)
        out_l[pos] = src
        within = pos - offs[src]
        has = matched_l[src]
        rr = torch.where(
            has, pr.to(torch.int64)[
                torch.clamp(lo[src] + within, max=max(sr.numel() - 1, 0))],
            torch.full_like(src, -1))
        out_r[pos] = rr
        if how == "outer" and keys_r.numel():
            m = torch.zeros(keys_r.numel(), dtype=torch.bool, device=dev)
            mr = out_r[out_r >= 0]
            m[mr] = True
            un = torch.nonzero(~m).flatten()
            if un.numel():
                out_l = torch.cat([out_l, torch.full_like(un, -1)])
                out_r = torch.cat([out_r, un])
        return out_l, out_r
