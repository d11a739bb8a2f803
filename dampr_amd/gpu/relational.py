"""Device relational ops over (u64-key, payload) columns: sort, group-by
reduce, join, top-k.

These are the GPU engine's building blocks for the DSL's ``group_by``,
``sort_by``, ``join``, ``filter`` and ``topk`` when keys/values lower to
device columns.  Keys are i64 words:
raw integers, sortable encodings of doubles, or the dense ids / byte-order
ranks that ``dict_encode_strs`` / ``lex_rank_strs`` give a string column.
Sort and merge carry an i32 row number as payload; the caller gathers its
device value columns (numeric tensors, or ``StrVals`` byte arenas) by it.

torch is the tensor layer (allocations, cumsum/nonzero metadata glue); all
per-record hot work is in the hand-written HIP kernels (ops/hip/), whose
wrappers check every argument's dtype, contiguity and length: the functions
here hand them contiguous tensors and take views at a storage offset as
they come.
"""
import collections

import torch

from ..ops import native
from .backend import OP_MAX, OP_MIN, OP_SUM     # noqa: F401 - re-exported
from .filters import (FILTER_DOMAINS, FILTER_OPS,  # noqa: F401 - re-exported
                      FILTER_TILE, SET_OPS, SV_FILTER_DOMAIN_STR,
                      SV_FILTER_OPS, SV_FILTER_TILE, NumFilterProgram,
                      SvFilterProgram, _I64_MAX, _I64_MIN, check_row_count,
                      filter_program, set_capacity, sv_filter_program)
from .stores import encode_f64_sortable     # noqa: F401 - sort_by/topk keys



def _pow2_at_least(n):
    return 1 << max(4, int(n - 1).bit_length())


def radix_sort_pairs(keys, payload=None, low_passes=None):
    """Stable LSD radix sort of int64-as-u64 keys; returns (keys, payload)
    sorted in unsigned key order.  Skips passes whose digit is constant.
    ``low_passes`` stops after that many ACTIVE low-byte passes — a
    partial sort that clusters keys by their low bits (hash-table probe
    locality wants slot-region grouping, not total order)."""
    ext = native.require()
    n = keys.numel()
    if payload is None:
        payload = torch.arange(n, dtype=torch.int32, device=keys.device)
    if n <= 1:
        return keys.clone(), payload.clone()
    RS_SPAN = ext.rs_span()
    nblocks = (n + RS_SPAN - 1) // RS_SPAN
    # The caller's tensors are read-only: the first executed pass scatters
    # out of them into an owned buffer, and later passes ping-pong between
    # two owned buffers (using the input as scratch would clobber it).
    src_k, src_p = keys.contiguous(), payload.contiguous()
    out_k, out_p = torch.empty_like(src_k), torch.empty_like(src_p)
    # one streaming read decides which byte passes are constant
    # (skippable): digit d is constant iff its byte of the AND-fold
    # equals its byte of the OR-fold.  Single host sync for the whole
    # sort; runs at read bandwidth (register fold + one atomic/wave).
    a, o = ext.rs_digit_fold(src_k).cpu().tolist()
    active = [((a >> (8 * b)) & 255) != ((o >> (8 * b)) & 255)
              for b in range(8)]
    n_done = 0
    for byte in range(8):
        if low_passes is not None and n_done >= low_passes:
            break
        shift = byte * 8
        if not active[byte]:
            continue                      # constant digit: skip pass
        hist = ext.rs_hist(src_k, shift, nblocks)
        scanned = torch.cumsum(hist, 0, dtype=torch.int64)
        scanned -= hist                # exclusive, fused i64 upcast
        ext.rs_scatter(src_k, src_p, scanned, shift, nblocks, out_k, out_p)
        n_done += 1
        if n_done == 1:
            src_k, src_p = out_k, out_p
            out_k, out_p = (torch.empty_like(src_k),
                            torch.empty_like(src_p))
        else:
            src_k, src_p, out_k, out_p = out_k, out_p, src_k, src_p
    if n_done == 0:
        return src_k.clone(), src_p.clone()
    return src_k, src_p


def _tile_offsets(counts):
    """A count pass's per-tile counts -> (exclusive i64 offsets for the
    second pass, total)."""
    scan = torch.cumsum(counts, 0, dtype=torch.int64)
    offsets = scan - counts
    return offsets, int(scan[-1].item())    # the call's one host sync


def group_reduce_sorted(sorted_keys, vals, op=OP_SUM):
    """Segmented reduce over a key-sorted column; returns (unique_keys,
    aggregates).  Fused form (K5+K7): per-tile segment-start counts +
    a tiny tile-base scan, then ONE pass that re-derives boundaries
    from neighbor keys, emits each segment head's key and folds values
    — no materialized per-element segment ids (the flags -> cumsum ->
    nonzero -> gather chain cost 4+ full-column passes and a host
    sync)."""
    ext = native.require()
    n = sorted_keys.numel()
    if n == 0:
        return sorted_keys, vals[:0]
    sorted_keys = sorted_keys.contiguous()
    vals = vals.contiguous()
    tile_base, n_seg = _tile_offsets(ext.seg_count(sorted_keys))
    if vals.dtype == torch.float64:
        init = {OP_SUM: 0.0, OP_MIN: float("inf"),
                OP_MAX: float("-inf")}[op]
        out = torch.full((n_seg,), init, dtype=torch.float64,
                         device=vals.device)
    else:
        init = {OP_SUM: 0, OP_MIN: _I64_MAX, OP_MAX: _I64_MIN}[op]
        out = torch.full((n_seg,), init, dtype=torch.int64,
                         device=vals.device)
    uniq = torch.empty(n_seg, dtype=torch.int64,
                       device=sorted_keys.device)
    ext.seg_reduce_fused(sorted_keys, vals, tile_base, op, uniq, out)
    return uniq, out


def group_sum(keys, vals):
    """Unsorted group-by-sum: radix sort then segmented reduce (the
    high-cardinality path; for low-cardinality the hash-combine table in
    tfidf.py is the faster route)."""
    sk, sp = radix_sort_pairs(keys)
    sv = vals[sp.to(torch.int64)]
    return group_reduce_sorted(sk, sv)


def hj_build_table(keys_r):
    """Build the chained hash table over the right side once; reusable
    across probe batches (the skew guard probes in chunks — rebuilding
    the table per chunk cost ~1.6 ms x batches at 25M rows)."""
    ext = native.require()
    keys_r = keys_r.contiguous()
    dev = keys_r.device
    nr = keys_r.numel()
    cap = _pow2_at_least(max(2 * nr, 16))
    t_keys = torch.zeros(cap, dtype=torch.int64, device=dev)
    # cap+1 heads: t_head[cap] is the dedicated zero-key chain (raw keys
    # include 0 — dictionary rank ids, int columns — and the open table
    # uses 0 as EMPTY; see hj_build_kernel)
    t_head = torch.full((cap + 1,), -1, dtype=torch.int64, device=dev)
    nxt = torch.empty(max(nr, 1), dtype=torch.int64, device=dev)
    ext.hj_build(keys_r, t_keys, t_head, nxt)
    return (t_keys, t_head, nxt, nr)


def hash_join(keys_l, keys_r, how="inner", table=None):
    """Equi-join on u64 keys.  Returns (l_idx, r_idx) int64 row-index pairs;
    for "left"/"outer", missing matches carry index -1.

    how: "inner" | "left" | "outer"; ``table`` reuses hj_build_table.
    """
    assert how in ("inner", "left", "outer")
    ext = native.require()
    keys_l = keys_l.contiguous()
    t_keys, t_head, nxt, nr = table or hj_build_table(keys_r)
    left_outer = 1 if how in ("left", "outer") else 0
    counts = ext.hj_count(keys_l, t_keys, t_head, nxt, left_outer)
    offsets = torch.cumsum(counts, 0) - counts
    total = int(counts.sum().item())
    out_l, out_r, matched = ext.hj_emit(
        keys_l, t_keys, t_head, nxt, offsets, total, left_outer,
        1 if how == "outer" else 0, nr)
    out_l, out_r = out_l[:total], out_r[:total]
    if how == "outer" and nr:
        un = torch.nonzero(matched[:nr] == 0).flatten()
        if un.numel():
            out_l = torch.cat([out_l, torch.full_like(un, -1)])
            out_r = torch.cat([out_r, un])
    return out_l, out_r


_U64 = (1 << 64) - 1


def dict_encode_strs(sv, hash_mask=None):
    """Dictionary-encode a var-len string column (gpu.strvals.StrVals) on
    device: hash every row (sv_hash64), radix-sort the hashes, mark
    segment heads over the sorted order with a byte compare of hash-equal
    neighbours (sv_adjacent_eq), scan the heads into dense ids and gather
    one row per segment.

    Returns ``(ids i64[n], uniq StrVals[U], collided)``: ids are dense in
    [0, U), ``uniq`` row i is the string of id i, and the id ORDER is
    hash order (unspecified to callers).  ``collided`` reports that two
    different strings shared a (masked) hash; the ids of such a batch are
    not a valid encoding and the caller must re-encode it exactly.
    ``hash_mask`` narrows the hash (tests force collisions with it)."""
    from .strvals import StrVals
    ext = native.require()
    n = sv.numel()
    dev = sv.blob.device
    if n == 0:
        return (torch.zeros(0, dtype=torch.int64, device=dev),
                StrVals.empty(dev), False)
    if n >= (1 << 31):                  # i32 sort payload
        raise OverflowError("dict_encode_strs: row count exceeds i32")
    mask = _U64 if hash_mask is None else int(hash_mask) & _U64
    blob, offs = sv.blob.contiguous(), sv.offs.contiguous()
    hashes = torch.empty(n, dtype=torch.int64, device=dev)
    ext.sv_hash64(blob, offs, mask, hashes)
    sorted_hash, perm = radix_sort_pairs(hashes)
    heads = torch.empty(n, dtype=torch.uint8, device=dev)
    n_mismatch = torch.zeros(1, dtype=torch.int64, device=dev)
    ext.sv_adjacent_eq(blob, offs, sorted_hash, perm, heads, n_mismatch)
    seg = torch.cumsum(heads, 0, dtype=torch.int64) - 1
    perm = perm.to(torch.int64)
    ids = torch.empty(n, dtype=torch.int64, device=dev)
    ids[perm] = seg
    uniq = sv.gather(perm[heads.bool()])
    return ids, uniq, bool(n_mismatch.item() > 0)


def _last_flag_pos(flags):
    """For every position of a bool column whose entry 0 is set, the
    position of the latest set entry at or before it (a running maximum
    over the set positions).  Done as a cumsum into segment numbers, a
    scatter of each set position into its segment's slot (unset entries
    all write one spare slot) and a gather back: torch.cummax measured
    5 ms over 2M entries on an MI355X, these kernels tens of
    microseconds."""
    m = flags.numel()
    pos = torch.arange(m, dtype=torch.int64, device=flags.device)
    seg = torch.cumsum(flags, 0, dtype=torch.int64) - 1
    slot = torch.where(flags, seg, torch.full_like(seg, m))
    tab = torch.empty(m + 1, dtype=torch.int64, device=flags.device)
    tab[slot] = pos
    return tab[seg]


def lex_rank_strs(sv):
    """Rank the rows of a var-len string column (gpu.strvals.StrVals) in
    byte-lexicographic order on device: returns ``(rank i64[n], rounds)``
    where ``rank[i]`` counts the rows strictly smaller than row i (rows
    compare as unsigned bytes, a proper prefix is smaller, equal rows
    share a rank) and ``rounds`` is the number of refinement rounds run.

    MSD refinement, 7 bytes a round.  ``cur`` holds the rows still
    undecided and ``grp`` the base rank of the group each belongs to (a
    group of m rows with base g owns ranks [g, g + m)).  Round d keys
    every undecided row by its window d (sv_lex_key, the twin of
    keyhash.lex_window_key), orders them by (grp, key) with two stable
    radix sorts, and sv_lex_refine marks the heads of the classes of
    equal (grp, key) and the rows still open: members of a class of two
    or more whose window did not reach the row's end.  A class's base is
    its group's base plus the class head's distance from the group head,
    and a class is open or closed as a whole, so an open class arrives
    complete, as one group, in round d + 1.  Every row's rank is written
    each round; an open row's is overwritten when a later round settles
    it.  An open row after round d is longer than 7(d + 1) bytes, so the
    loop runs at most max_len // 7 + 1 rounds.  Host syncs: the longest
    row once, then per round the open count and the radix sorts' digit
    folds."""
    ext = native.require()
    n = sv.numel()
    dev = sv.blob.device
    if n >= (1 << 31):                  # i32 row indices and sort payload
        raise OverflowError("lex_rank_strs: row count exceeds i32")
    rank = torch.zeros(n, dtype=torch.int64, device=dev)
    if n == 0:
        return rank, 0
    blob, offs = sv.blob.contiguous(), sv.offs.contiguous()
    max_rounds = int(sv.lens().max().item()) // 7 + 1
    cur = torch.arange(n, dtype=torch.int32, device=dev)
    grp = torch.zeros(n, dtype=torch.int64, device=dev)
    rounds = 0
    while cur.numel():
        if rounds >= max_rounds:
            raise RuntimeError(
                "lex_rank_strs: rows still undecided past the longest row "
                "(offsets not monotone?)")
        m = cur.numel()
        keys = torch.empty(m, dtype=torch.int64, device=dev)
        ext.sv_lex_key(blob, offs, cur, rounds, keys)
        keys, perm = radix_sort_pairs(keys)
        if rounds:
            # stable by group on top of the key order: (grp, key) order.
            # grp < 2**31, its constant high bytes are skipped passes
            grp, perm2 = radix_sort_pairs(grp[perm.to(torch.int64)])
            perm2 = perm2.to(torch.int64)
            keys, perm = keys[perm2], perm[perm2]
        rows = cur[perm.to(torch.int64)]
        heads = torch.empty(m, dtype=torch.uint8, device=dev)
        still = torch.empty(m, dtype=torch.uint8, device=dev)
        ext.sv_lex_refine(grp, keys, heads, still)
        base = grp + _last_flag_pos(heads.bool())
        if rounds:
            ghead = torch.ones(m, dtype=torch.bool, device=dev)
            ghead[1:] = grp[1:] != grp[:-1]
            base -= _last_flag_pos(ghead)
        rank[rows.to(torch.int64)] = base
        rounds += 1
        nxt = torch.nonzero(still).flatten()        # the round's host sync
        cur, grp = rows[nxt].contiguous(), base[nxt].contiguous()
    return rank, rounds


def set_table(members, device):
    """The device hash set of a numeric set clause's ``members`` (1-D CPU
    i64 tensor of distinct words): an i64 table of ``set_capacity(m)``
    words, EMPTY = 0, filled by set_build at splitmix64(word) & mask with
    linear probing.  The word 0 is not stored; the clause carries "zero
    is a member" as a flag.  8 * capacity device bytes that the HBM pool
    does not account for."""
    ext = native.require()
    table = torch.zeros(set_capacity(members.numel()), dtype=torch.int64,
                        device=device)
    if members.numel():
        ext.set_build(members.contiguous().to(device), table)
    return table


# The device form of a string set: the members' arena, their sv_hash64
# hashes under ``hash_mask``, and the i32 slot table (member index + 1 at
# hash & mask, linear probing).  O(members' bytes) of device memory that
# the HBM pool does not account for.
SvSetTable = collections.namedtuple(
    "SvSetTable", "blob offs hashes slots hash_mask")


def sv_set_table(members, device, hash_mask=None):
    """The device form of a string set clause's ``members`` (distinct
    ``bytes``).  ``hash_mask`` narrows the hashes as in
    ``dict_encode_strs`` (tests force collisions with it); the rows are
    hashed under the same mask when the set is probed."""
    import numpy as np
    ext = native.require()
    members = [bytes(m) for m in members]
    m = len(members)
    mask = _U64 if hash_mask is None else int(hash_mask) & _U64
    offs = np.zeros(m + 1, dtype=np.int64)
    np.cumsum([len(b) for b in members], out=offs[1:])
    blob = np.frombuffer(b"".join(members), dtype=np.uint8).copy()
    blob = torch.from_numpy(blob).to(device)
    offs = torch.from_numpy(offs).to(device)
    hashes = torch.empty(m, dtype=torch.int64, device=device)
    slots = torch.zeros(set_capacity(m), dtype=torch.int32, device=device)
    if m:
        ext.sv_hash64(blob, offs, mask, hashes)
        ext.sv_set_build(hashes, slots)
    return SvSetTable(blob, offs, hashes, slots, mask)


def filter_compile(clauses, values, device, hash_mask=None):
    """Compile resolved clauses for the filter kernels over a "numeric" or
    "string" ``values`` column on ``device``: the flat program, the string
    constants' buffer, and the device hash sets of the set clauses, built
    here once so every run of a filter stage reuses them.  Returns a
    ``NumFilterProgram`` / ``SvFilterProgram``, which passes through
    unchanged.  ``hash_mask``: see ``sv_set_table``."""
    if isinstance(clauses, (NumFilterProgram, SvFilterProgram)):
        return clauses
    if values == "string":
        p = sv_filter_program(clauses, device)
    else:
        p = NumFilterProgram(filter_program(clauses), None, None)
    return _with_sets(p, clauses, device, hash_mask)


def _with_sets(p, clauses, device, hash_mask=None):
    """The encoded program ``p`` of ``clauses`` with the device hash sets
    of its set clauses; ``p`` itself when it has none."""
    sets = {}
    for col, dom, op, a, _b in clauses:
        if op not in SET_OPS:
            continue
        if dom != "str":
            sets[col] = set_table(a, device)
            continue
        if hash_mask is None:
            from .. import settings
            hash_mask = settings.str_hash_mask
        sets[col] = sv_set_table(a, device, hash_mask)
    if not sets:
        return p
    if isinstance(p, SvFilterProgram):
        return p._replace(set_k=sets.get(0), sv_set=sets.get(1))
    return p._replace(set_k=sets.get(0), set_v=sets.get(1))


def _check_value_sets(prog, vals):
    """ValueError for a value-column set clause whose domain is not the
    value dtype's (the extension checks every clause; this one is part of
    the backends' shared contract)."""
    f64 = vals.dtype == torch.float64
    for i in range(0, len(prog), 5):
        col, dom, op = prog[i:i + 3]
        if col == 1 and op in SET_OPS.values() and \
                (dom == FILTER_DOMAINS["f64"]) != f64:
            raise ValueError("filter_rows: set domain does not match {} "
                             "values".format(vals.dtype))


def _sv_set_args(p, blob, offs):
    """The string kernels' set arguments for one run: the key set, and the
    string set with this run's row hashes (one sv_hash64 launch, read by
    both passes)."""
    if p.sv_set is None:
        return p.set_k, []
    t = p.sv_set
    row_hash = torch.empty(offs.numel() - 1, dtype=torch.int64,
                           device=offs.device)
    ext = native.require()
    ext.sv_hash64(blob, offs, t.hash_mask, row_hash)
    return p.set_k, [t.blob, t.offs, t.hashes, t.slots, row_hash]


def filter_rows(keys, vals, clauses):
    """Stable compaction of the rows of (keys, vals) that satisfy every
    clause: filter_count (survivors per tile), an exclusive scan of the
    tile counts, filter_scatter (each survivor to tile offset + wave
    prefix + its rank within the wave's ballot).  Output is in input
    order with the inputs' dtypes.  One host sync per call: the survivor
    total is read to allocate exact-size outputs (accepted; the engine
    needs the row count of every run anyway).  Non-contiguous inputs are
    made contiguous; a contiguous view at a storage offset (``t[3:]``) is
    read in place."""
    ext = native.require()
    n = keys.numel()
    check_row_count("filter_rows", n)
    p = clauses
    if not isinstance(p, NumFilterProgram):     # refuse before any launch
        p = NumFilterProgram(filter_program(clauses, vals.dtype), None, None)
    if n == 0:
        return keys.clone(), vals.clone()
    if p is clauses:
        _check_value_sets(p.prog, vals)
    else:
        p = _with_sets(p, clauses, keys.device)
    keys, vals = keys.contiguous(), vals.contiguous()
    offsets, total = _tile_offsets(
        ext.filter_count(keys, vals, p.prog, p.set_k, p.set_v))
    out_k = torch.empty(total, dtype=keys.dtype, device=keys.device)
    out_v = torch.empty(total, dtype=vals.dtype, device=vals.device)
    if total:
        ext.filter_scatter(keys, vals, p.prog, offsets, out_k, out_v,
                           p.set_k, p.set_v)
    return out_k, out_v


def sv_count_rows(sv, clauses):
    """How many rows of a StrVals column satisfy every (str) clause:
    sv_filter_count alone, its tile counts summed.  One host sync."""
    ext = native.require()
    n = sv.numel()
    check_row_count("sv_count_rows", n)
    p = filter_compile(clauses, "string", sv.blob.device)
    if p.n_key_clauses:
        raise ValueError("sv_count_rows: a clause reads the key column")
    if n == 0:
        return 0
    blob, offs = sv.blob.contiguous(), sv.offs.contiguous()
    set_k, sv_set = _sv_set_args(p, blob, offs)
    return _tile_offsets(ext.sv_filter_count(
        None, blob, offs, p.prog, p.consts, set_k, sv_set))[1]


def sv_filter_rows(keys, sv, clauses):
    """Stable compaction of the rows of (keys, StrVals) that satisfy every
    clause: sv_filter_count, an exclusive scan of the tile counts,
    sv_filter_scatter (each survivor's key, arena offset and length to
    its output slot), a scan of the surviving lengths into the new
    offsets, and varlen_gather for the bytes.  The result's arena is
    fresh and compact.  Two host syncs per call: the survivor total and
    the surviving byte total, each read to allocate exact-size outputs."""
    from .strvals import StrVals
    ext = native.require()
    n = keys.numel()
    check_row_count("sv_filter_rows", n, sv.numel())
    if sv.numel() != n:
        raise ValueError("sv_filter_rows: keys and values differ in length")
    dev = keys.device
    if n == 0:
        if not isinstance(clauses, SvFilterProgram):
            sv_filter_program(clauses, dev)     # still refuse a bad program
        return keys.clone(), StrVals.empty(dev)
    p = filter_compile(clauses, "string", dev)
    keys = keys.contiguous()
    blob, offs = sv.blob.contiguous(), sv.offs.contiguous()
    set_k, sv_set = _sv_set_args(p, blob, offs)
    offsets, total = _tile_offsets(      # host sync: rows kept
        ext.sv_filter_count(keys, blob, offs, p.prog, p.consts, set_k,
                            sv_set))
    out_k = torch.empty(total, dtype=torch.int64, device=dev)
    if total == 0:
        return out_k, StrVals.empty(dev)
    src = torch.empty(total, dtype=torch.int64, device=dev)
    lens = torch.empty(total, dtype=torch.int64, device=dev)
    ext.sv_filter_scatter(keys, blob, offs, p.prog, p.consts, offsets,
                          out_k, src, lens, set_k, sv_set)
    new_offs = torch.zeros(total + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=new_offs[1:])
    nbytes = int(new_offs[-1].item())       # host sync: bytes kept
    out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if nbytes:
        ext.varlen_gather(blob, src, lens, new_offs, out)
    return out_k, StrVals(out, new_offs)


def topk_by(values_u64, k, largest=True):
    """Top-k row indices ordered by a u64 sort column (K11 via the radix
    sort; the column is a key-encoded ordering, e.g. flipped-sign floats)."""
    keys = values_u64 if not largest else ~values_u64
    sk, sp = radix_sort_pairs(keys)
    return sp[:k].to(torch.int64)
