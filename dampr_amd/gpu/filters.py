"""The row filters' clause layer, from a DSL predicate to the kernels'
program: the constants both backends and both kernels agree on, the
validator for resolved clauses, the encoders of the extension's programs,
and the lowering of a filter stage against a store's metadata.

A resolved clause is ``(col, domain, op, a, b)`` as documented on
``_OpsBase.filter_rows`` / ``sv_filter_rows`` (gpu/backend.py).  Pure host
logic; nothing here launches a kernel.
"""
import collections
import math
import struct

import torch

from ..funcs import set_members_lower
from .stores import StrTable, _store_has_sv, table_bounds

_I64_MIN = -(1 << 63)
_I64_MAX = (1 << 63) - 1

# clauses one filter_rows / sv_filter_rows call takes (filter_clause.h
# FILTER_MAX_CLAUSES)
FILTER_MAX_CLAUSES = 8
# longest string constant of an sv_filter_rows clause, in bytes
# (dampr_strfilter.hip SVF_MAX_CONST)
SV_FILTER_MAX_CONST = 64
# rows one block of the filter kernels owns (compact.h COMPACT_TILE);
# tests/test_gpu_filter.py and tests/test_gpu_strfilter.py pin these and
# SV_FILTER_MAX_CONST to ext.filter_tile() / ext.sv_filter_tile() /
# ext.sv_filter_max_const()
FILTER_TILE = SV_FILTER_TILE = 4096

# filter_clause.h's clause encoding (FD_* / FO_*)
FILTER_DOMAINS = {"i64": 0, "f64": 1, "fkey": 2}
FILTER_OPS = {"gt": 0, "ge": 1, "lt": 2, "le": 3, "eq": 4, "ne": 5,
              "between": 6}
SV_FILTER_DOMAIN_STR = 3
SV_FILTER_OPS = dict(FILTER_OPS, startswith=7)
# set membership: the clause's constant is a set of members, probed in a
# device hash set (set_table.h)
SET_OPS = {"isin": 8, "notin": 9}
# members one set may hold (set_table.h SET_MAX_MEMBERS)
SET_MAX_MEMBERS = 1 << 30
_SV_CONST_WORDS = SV_FILTER_MAX_CONST // 8

# the (col, domain) pairs a program may hold, by kind of value column.  The
# key column is always i64 words: raw ints or encoded doubles.
_LEGAL = {
    "numeric": {(0, "i64"), (0, "fkey"), (1, "i64"), (1, "f64"),
                (1, "fkey")},
    "string": {(0, "i64"), (0, "fkey"), (1, "str")},
}


def set_capacity(m):
    """Slots of the device hash set of ``m`` members: the power of two that
    is at least 2 * m and at least 16 (set_table.h set_capacity_for;
    tests/test_gpu_isin.py pins the two together)."""
    return max(16, 1 << max(0, 2 * int(m) - 1).bit_length())


def check_clauses(clauses, values, what, vdtype=None):
    """Raise ValueError unless ``clauses`` is a program both backends take
    for a ``values`` ("numeric" or "string") value column: 1 to
    FILTER_MAX_CLAUSES resolved clauses, each a legal (col, domain) pair,
    every "str" comparison constant within SV_FILTER_MAX_CONST bytes, at
    most one set clause ("isin" / "notin") per column, a set's members in
    their domain's form (a 1-D CPU i64 tensor; for "str" a sequence of
    ``bytes``) and, where the value column's ``vdtype`` is known, a value
    set's domain "f64" exactly over f64 values.  A set of more than
    SET_MAX_MEMBERS members raises OverflowError.  ``what`` names the
    caller in the message."""
    if not 1 <= len(clauses) <= FILTER_MAX_CLAUSES:
        raise ValueError("{} takes 1..{} clauses, got {}".format(
            what, FILTER_MAX_CLAUSES, len(clauses)))
    set_cols = set()
    for col, dom, op, a, b in clauses:
        if (col, dom) not in _LEGAL[values]:
            raise ValueError("{}: {!r} clause on column {}".format(
                what, dom, col))
        if op in SET_OPS:
            if col in set_cols:
                raise ValueError("{}: two set clauses on column {}".format(
                    what, col))
            set_cols.add(col)
            if dom == "str":
                ok = all(isinstance(m, bytes) for m in a)
                m = len(a)
            else:
                ok = isinstance(a, torch.Tensor) and a.dim() == 1 and \
                    a.dtype == torch.int64 and a.device.type == "cpu"
                m = a.numel() if ok else 0
            if not ok:
                raise ValueError("{}: malformed members of a {!r} set".format(
                    what, dom))
            if m > SET_MAX_MEMBERS:
                raise OverflowError("{}: more than 2**30 set members".format(
                    what))
            if col == 1 and vdtype is not None and \
                    (dom == "f64") != (vdtype == torch.float64):
                raise ValueError("{}: {!r} set over {} values".format(
                    what, dom, vdtype))
            continue
        longest = max(len(a), len(b) if op == "between" else 0) \
            if dom == "str" else 0
        if longest > SV_FILTER_MAX_CONST:
            raise ValueError("{}: constant longer than {} bytes".format(
                what, SV_FILTER_MAX_CONST))


def check_row_count(what, *counts):
    """The kernels index rows with i32: refuse more before anything is
    launched or allocated."""
    if any(n >= (1 << 31) for n in counts):
        raise OverflowError("{}: row count exceeds i32".format(what))


# -- program encoders: resolved clauses -> what the extension takes -----------

def _f64_bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _encode_numeric(col, dom, op, a, b):
    if op in SET_OPS:
        # a: the count of non-zero members, which is what the table holds;
        # b: whether the word 0 (int 0, or +-0.0) is a member
        zero = bool((a == 0).any().item())
        return (int(col), FILTER_DOMAINS[dom], SET_OPS[op],
                a.numel() - zero, int(zero))
    if dom == "i64":
        a, b = int(a), int(b)
        if not (_I64_MIN <= a <= _I64_MAX and _I64_MIN <= b <= _I64_MAX):
            raise OverflowError("filter constant outside i64")
    else:
        a, b = _f64_bits(a), _f64_bits(b)
    return (int(col), FILTER_DOMAINS[dom], FILTER_OPS[op], a, b)


# A numeric clause program compiled for the filter kernels: the
# extension's 5 int64 per clause and the device hash sets of its set
# clauses, by column (None where the column has none).
NumFilterProgram = collections.namedtuple(
    "NumFilterProgram", "prog set_k set_v")


def filter_program(clauses, vdtype=None):
    """Flatten resolved clauses ``(col, domain, op, a, b)`` (the
    ``_OpsBase.filter_rows`` form) into the extension's 5 int64 per
    clause; f64 constants travel as their bit patterns, a set's members
    not at all (its clause says how many there are and whether 0 is
    one)."""
    check_clauses(clauses, "numeric", "filter_rows", vdtype)
    prog = []
    for clause in clauses:
        prog.extend(_encode_numeric(*clause))
    return prog


# A clause program compiled for the string-filter kernels: the extension's
# 5 int64 per clause and the device buffer of the string constants' words.
# Built once per filter stage, used for every run.  set_k: the key
# column's device hash set; sv_set: the value column's string set (a
# relational.SvSetTable); None where the program has none.
SvFilterProgram = collections.namedtuple(
    "SvFilterProgram", "prog consts n_key_clauses set_k sv_set",
    defaults=(None, None))


def sv_filter_program(clauses, device):
    """Compile resolved clauses (the ``_OpsBase.sv_filter_rows`` form) for
    ``device``.  A string constant is cut into 8-byte words, zero-padded,
    each packed big-endian (byte 0 most significant: unsigned word order
    is byte order); clause i's constants fill slots 2i and 2i + 1 of
    ``_SV_CONST_WORDS`` words each."""
    if isinstance(clauses, SvFilterProgram):
        return clauses
    check_clauses(clauses, "string", "sv_filter_rows")
    prog = []
    words = [0] * (2 * FILTER_MAX_CLAUSES * _SV_CONST_WORDS)
    n_key = 0
    for i, (col, dom, op, a, b) in enumerate(clauses):
        if dom != "str":
            prog.extend(_encode_numeric(col, dom, op, a, b))
            n_key += 1
            continue
        if op in SET_OPS:
            prog.extend((1, SV_FILTER_DOMAIN_STR, SET_OPS[op], 0, 0))
            continue
        consts = (bytes(a), bytes(b) if op == "between" else b"")
        for slot, c in enumerate(consts):
            base = (2 * i + slot) * _SV_CONST_WORDS
            for j in range(0, len(c), 8):
                w = int.from_bytes(c[j:j + 8].ljust(8, b"\0"), "big")
                words[base + j // 8] = w - (1 << 64) if w >> 63 else w
        prog.extend((1, SV_FILTER_DOMAIN_STR, SV_FILTER_OPS[op],
                     len(consts[0]), len(consts[1])))
    return SvFilterProgram(
        prog, torch.tensor(words, dtype=torch.int64, device=device), n_key)


# -- lowering: (selector, op, constants) -> resolved clauses ------------------

def _fold_i64(op, consts):
    """A predicate's (op, a, b) over an i64 column, or None when a
    constant has no integer form (NaN, infinite, outside i64).  Python
    compares int with float exactly, so a non-integral finite constant
    folds to the equivalent integer clause: ``v > 2.5`` is ``v >= 3``,
    ``v == 2.5`` never holds, ``v != 2.5`` always does."""
    cs = []
    for c in consts:
        if isinstance(c, float):
            if not math.isfinite(c):
                return None
            if c.is_integer():
                c = int(c)
        else:
            c = int(c)                               # bool -> int
        if isinstance(c, int) and not _I64_MIN <= c <= _I64_MAX:
            return None
        cs.append(c)
    if op == "between":
        lo, hi = cs
        return ("between",
                math.ceil(lo) if isinstance(lo, float) else lo,
                math.floor(hi) if isinstance(hi, float) else hi)
    c = cs[0]
    if isinstance(c, int):
        return (op, c, 0)
    if op in ("gt", "ge"):
        return ("ge", math.ceil(c), 0)
    if op in ("lt", "le"):
        return ("le", math.floor(c), 0)
    if op == "eq":
        return ("between", 1, 0)                     # never
    return ("between", _I64_MIN, _I64_MAX)           # ne: always


def _fold_f64(op, consts):
    """A predicate's (op, a, b) over doubles, or None when an int
    constant is not exactly a double (magnitude beyond 2**53)."""
    cs = []
    for c in consts:
        if not isinstance(c, float):
            c = int(c)
            if abs(c) > (1 << 53):
                return None
            c = float(c)
        cs.append(c)
    return (op, cs[0], cs[1] if len(cs) > 1 else 0.0)


_ALWAYS = ("between", _I64_MIN, _I64_MAX)


def _fold_rank(table, op, consts, ops):
    """A string predicate's (op, a, b) over the key ids of a string
    table.  Ids are the keys' ranks in byte order, so with lo(c) the
    number of keys below c and hi(c) the number at or below it, every
    comparison is an id range; ``startswith(p)`` is the range from lo(p)
    to below the first key past every extension of p: lo(succ(p)), succ
    being p without trailing 0xFF bytes and its last byte incremented
    (the table's end when nothing remains)."""
    if isinstance(table, StrTable):
        def bounds(c):
            return table.bounds(c, ops)
    else:
        enc = [s.encode("utf-8") for s in table]

        def bounds(c):
            return table_bounds(enc, c)
    cs = [c.encode("utf-8") for c in consts]
    if op == "between":
        return ("between", bounds(cs[0])[0], bounds(cs[1])[1] - 1)
    if op == "startswith":
        if not cs[0]:
            return _ALWAYS
        succ = cs[0].rstrip(b"\xff")
        upper = len(table) if not succ else \
            bounds(succ[:-1] + bytes([succ[-1] + 1]))[0]
        return ("between", bounds(cs[0])[0], upper - 1)
    lo, hi = bounds(cs[0])
    if op == "eq":
        return ("between", lo, hi - 1)
    if op == "ne":
        return ("ne", lo, 0) if hi > lo else _ALWAYS
    return {"gt": ("ge", hi, 0), "ge": ("ge", lo, 0),
            "lt": ("lt", lo, 0), "le": ("lt", hi, 0)}[op]


_NEVER = ("between", 1, 0)


def _set_words(dom, members, table=None, ops=None):
    """The members of a lowerable set (``set_members_lower``) that can
    equal a row of a ``dom`` column, in the column's form: a Python set of
    i64 words ("i64": the integers; "f64" / "fkey": the bits of the
    doubles, -0.0 as 0.0; "ids": the key ids of the ``str`` members in the
    string ``table``), or of UTF-8 ``bytes`` ("str").  A member that can
    never equal a row is dropped, which is exact: Python's ``in`` is
    ``==``, it compares int with float by value and a number with a
    ``str`` as unequal."""
    if dom in ("str", "ids"):
        enc = sorted(c.encode("utf-8") for c in members if type(c) is str)
        if dom == "str":
            return set(enc)
        if isinstance(table, StrTable):
            return set(table.ids_of(enc, ops))
        keys = [s.encode("utf-8") for s in table]
        return {lo for lo, hi in (table_bounds(keys, c) for c in enc)
                if hi > lo}
    words = set()
    for c in members:
        if type(c) is str:
            continue
        if dom == "i64":
            if isinstance(c, float):
                if not c.is_integer():        # also +-inf
                    continue
            c = int(c)
            if _I64_MIN <= c <= _I64_MAX:
                words.add(c)
            continue
        if not isinstance(c, float):
            c = int(c)
            try:
                f = float(c)
            except OverflowError:
                continue
            if int(f) != c:                   # no double equals it
                continue
            c = f
        words.add(_f64_bits(c + 0.0))         # -0.0 + 0.0 is 0.0
    return words


def _fold_sets(resolved):
    """One set clause per column: ``resolved`` with every column's set
    clauses (here still Python sets) folded into the first of them.
    isin(A) & isin(B) = isin(A & B); isin(A) & notin(B) = isin(A - B);
    notin(A) & notin(B) = notin(A | B).  An isin that folds to the empty
    set keeps nothing; a notin of the empty set drops out.  Members leave
    as the backends take them: a sorted 1-D i64 tensor, or a sorted list
    of ``bytes``."""
    folded = {}
    for col, dom, op, a, _b in resolved:
        if op not in SET_OPS:
            continue
        if col not in folded:
            folded[col] = (op, set(a))
            continue
        have_op, have = folded[col]
        if have_op == "isin":
            folded[col] = ("isin", have & a if op == "isin" else have - a)
        elif op == "isin":
            folded[col] = ("isin", a - have)
        else:
            folded[col] = ("notin", have | a)
    out = []
    for clause in resolved:
        col, dom, op = clause[:3]
        if op not in SET_OPS:
            out.append(clause)
            continue
        if col not in folded:
            continue                          # folded into an earlier one
        op, members = folded.pop(col)
        if not members:
            if op == "isin":
                out.append((0, "i64") + _NEVER)
            continue
        members = sorted(members)
        if dom != "str":
            members = torch.tensor(members, dtype=torch.int64)
        out.append((col, dom, op, members, None))
    # the key column is i64 words under every store: a clause over it that
    # always holds stands for a program whose clauses all dropped out
    return out or [(0, "i64") + _ALWAYS]


def _filter_programs(store, clauses, rank_agreed=False, ops=None):
    """Resolve a filter stage against ``store``: {value dtype: [chunks of
    at most FILTER_MAX_CLAUSES clauses]} for every value dtype its runs
    hold, or None when the stage has no device form (the caller runs it
    on host records).  A store of var-len string values has the one
    "dtype" None, and its chunks are ``ops.sv_filter_rows`` clauses;
    every other chunk is ``ops.filter_rows`` clauses.

    Selector -> column: on an unkeyed store records are bare values, so
    ``identity`` is the value column; on a keyed store records are
    (key, value), so ``fst`` is the key column and ``snd`` the value
    column.  Constant -> domain: numbers compare against numeric columns
    as folded by ``_fold_i64`` / ``_fold_f64``; ``str`` constants of at
    most SV_FILTER_MAX_CONST UTF-8 bytes compare against a var-len value
    column as "str" clauses, and against a string-table key column as
    i64 clauses on the key ids (``_fold_rank``; ``ops`` counts in a
    table that is still on the device).  Every other pairing goes to the
    host, which gives Python's answer or Python's TypeError.

    Set clauses (``isin`` / ``notin``; the constant is a frozenset) lower
    when ``funcs.set_members_lower`` takes the members.  Each resolves
    against its column by ``_set_words``; over a string-table key column
    the ``str`` members become key ids and the clause an i64 set clause.
    A member of another kind than the column is dropped, not sent to the
    host: ``3 in {"a"}`` is False, no TypeError.  ``_fold_sets`` then
    leaves at most one set clause per column, so a program carries at most
    two sets.

    ``rank_agreed`` (world > 1): the host path re-encodes its records
    with a collective, so every rank must take the same branch, also a
    rank that holds no rows.  The verdict then rests on store metadata
    and the constants alone: ``svals``, the string table (identical on
    every rank, so the folded ids agree), the declared ``vdtype``, or,
    where a store declares none (reduce outputs), both value dtypes."""
    if _store_has_sv(store):
        if not all(r.has_sv for runs in store.values() for r in runs):
            return None
        dtypes = {None}
    else:
        dtypes = {r.vdtype for runs in store.values() for r in runs}
        if rank_agreed:
            dtypes |= {store.vdtype} if store.vdtype is not None \
                else {torch.int64, torch.float64}
        if not dtypes <= {torch.int64, torch.float64}:
            return None
    for _sel, _op, consts in clauses:
        if any(type(c) is str and
               len(c.encode("utf-8")) > SV_FILTER_MAX_CONST for c in consts):
            return None
    members = {}                         # clause -> lowered set members
    for i, (_sel, op, consts) in enumerate(clauses):
        if op in SET_OPS:
            members[i] = set_members_lower(consts[0])
            if members[i] is None:
                return None
    programs = {}
    folded_keys = {}                     # one table lookup per clause
    for vdt in dtypes:
        resolved = []
        for i, (sel, op, consts) in enumerate(clauses):
            is_set = op in SET_OPS
            is_str = not is_set and type(consts[0]) is str
            if store.keyed and sel == "fst":
                if store.str_table is not None:
                    if is_set:
                        if i not in folded_keys:
                            folded_keys[i] = _set_words(
                                "ids", members[i], store.str_table, ops)
                        resolved.append((0, "i64", op, folded_keys[i], None))
                        continue
                    if not is_str:
                        return None
                    if i not in folded_keys:
                        folded_keys[i] = _fold_rank(store.str_table, op,
                                                    consts, ops)
                    resolved.append((0, "i64") + folded_keys[i])
                    continue
                col, dom = 0, "fkey" if store.fkeys else "i64"
            elif (sel == "snd") if store.keyed else (sel == "identity"):
                if vdt is None:
                    if is_set:
                        resolved.append((1, "str", op,
                                         _set_words("str", members[i]), None))
                        continue
                    if not is_str:
                        return None
                    cs = [c.encode("utf-8") for c in consts]
                    resolved.append((1, "str", op, cs[0],
                                     cs[1] if len(cs) > 1 else b""))
                    continue
                col, dom = 1, "i64" if vdt == torch.int64 else "f64"
            else:
                return None
            if is_str:
                return None
            if is_set:
                resolved.append((col, dom, op,
                                 _set_words(dom, members[i]), None))
                continue
            folded = (_fold_i64 if dom == "i64" else _fold_f64)(op, consts)
            if folded is None:
                return None
            resolved.append((col, dom) + folded)
        if members:
            resolved = _fold_sets(resolved)
        programs[vdt] = [resolved[i:i + FILTER_MAX_CLAUSES]
                         for i in range(0, len(resolved), FILTER_MAX_CLAUSES)]
    return programs
