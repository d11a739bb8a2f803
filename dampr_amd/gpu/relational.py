"""Device relational ops over (u64-key, payload) columns: sort, group-by
reduce, join, top-k.

These are the GPU engine's building blocks for the DSL's ``group_by``,
``sort_by``, ``join`` and ``topk`` when keys/values lower to device columns
(SURVEY.md §2.4 K2/K3/K5/K7/K8/K11).  Keys are 64-bit (keyhash.key_hash64
for strings); payloads are row indices into host or device value arenas.

torch is the tensor layer (allocations, cumsum/nonzero metadata glue); all
per-record hot work is in the hand-written HIP kernels.
"""
import torch

from ..ops import native
from .filters import (FILTER_DOMAINS, FILTER_OPS,  # noqa: F401 - re-exported
                      FILTER_TILE, SV_FILTER_DOMAIN_STR, SV_FILTER_OPS,
                      SV_FILTER_TILE, SvFilterProgram, _I64_MAX, _I64_MIN,
                      check_row_count, filter_program, sv_filter_program)
from .stores import encode_f64_sortable     # noqa: F401 - sort_by/topk keys

OP_SUM, OP_MIN, OP_MAX = 0, 1, 2


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


def segment_ids(sorted_keys):
    """(seg_ids i64, unique_keys) for a key-sorted column."""
    n = sorted_keys.numel()
    if n == 0:
        return (torch.zeros(0, dtype=torch.int64,
                            device=sorted_keys.device), sorted_keys)
    flags = torch.ones(n, dtype=torch.int64, device=sorted_keys.device)
    flags[1:] = (sorted_keys[1:] != sorted_keys[:-1]).to(torch.int64)
    seg = torch.cumsum(flags, 0) - 1
    uniq = sorted_keys[flags.bool()]
    return seg, uniq


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
    prog = filter_program(clauses)
    if n == 0:
        return keys.clone(), vals.clone()
    keys, vals = keys.contiguous(), vals.contiguous()
    offsets, total = _tile_offsets(ext.filter_count(keys, vals, prog))
    out_k = torch.empty(total, dtype=keys.dtype, device=keys.device)
    out_v = torch.empty(total, dtype=vals.dtype, device=vals.device)
    if total:
        ext.filter_scatter(keys, vals, prog, offsets, out_k, out_v)
    return out_k, out_v


def sv_count_rows(sv, clauses):
    """How many rows of a StrVals column satisfy every (str) clause:
    sv_filter_count alone, its tile counts summed.  One host sync."""
    ext = native.require()
    n = sv.numel()
    check_row_count("sv_count_rows", n)
    p = sv_filter_program(clauses, sv.blob.device)
    if p.n_key_clauses:
        raise ValueError("sv_count_rows: a clause reads the key column")
    if n == 0:
        return 0
    return _tile_offsets(ext.sv_filter_count(
        None, sv.blob.contiguous(), sv.offs.contiguous(), p.prog,
        p.consts))[1]


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
    p = sv_filter_program(clauses, dev)
    if n == 0:
        return keys.clone(), StrVals.empty(dev)
    keys = keys.contiguous()
    blob, offs = sv.blob.contiguous(), sv.offs.contiguous()
    offsets, total = _tile_offsets(      # host sync: rows kept
        ext.sv_filter_count(keys, blob, offs, p.prog, p.consts))
    out_k = torch.empty(total, dtype=torch.int64, device=dev)
    if total == 0:
        return out_k, StrVals.empty(dev)
    src = torch.empty(total, dtype=torch.int64, device=dev)
    lens = torch.empty(total, dtype=torch.int64, device=dev)
    ext.sv_filter_scatter(keys, blob, offs, p.prog, p.consts, offsets,
                          out_k, src, lens)
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
