"""The host record <-> column format: how a list of ``(k, v)`` Python
records becomes an i64 key column plus a value column, and back.  Int
keys stay i64, float (or mixed) keys take the f64 sortable encoding,
string keys become ranks into a sorted table, string values a ``StrVals``
arena, and reducer output ``(k, (k, v))`` stores ``v`` under a ``keyed``
flag.  Pure host logic in four steps: ``classify`` one rank's records,
``agree`` on the layout every rank shares (None: no columnar form),
``build`` the columns, ``decode`` them again."""
import collections

import numpy as np
import torch

from .stores import decode_f64_sortable, encode_f64_sortable

# kkind / vkind: "empty", "int", "float", "str" or "obj"; keyed: None for
# no records; table: the sorted distinct keys when they are strings
Layout = collections.namedtuple("Layout", "kkind vkind keyed table")


def _num(x):
    # bools stay Python objects: columnar i64 would decode True as 1
    # (repr-visible divergence from the host engine)
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def _int(x):
    return isinstance(x, int) and not isinstance(x, bool)


def _kind_of(xs):
    if not xs:
        return "empty"
    if all(_int(x) for x in xs):
        return "int"
    if all(_num(x) for x in xs):
        return "float"
    if all(isinstance(x, str) for x in xs):
        return "str"
    return "obj"


def classify(records, keyed_str_values):
    """The local ``Layout`` of a list of records.  Keyed means the host
    keyed-reducer convention, value = (key, scalar), where a string
    counts as a scalar only with ``keyed_str_values``."""
    if not records:
        return Layout("empty", "empty", None, None)
    keyed = all(
        isinstance(v, tuple) and len(v) == 2 and v[0] == k
        and (_num(v[1]) or (keyed_str_values and isinstance(v[1], str)))
        for k, v in records)
    ks = [k for k, _ in records]
    kkind = _kind_of(ks)
    return Layout(kkind, _kind_of([v[1] if keyed else v for _, v in records]),
                  keyed, tuple(sorted(set(ks))) if kkind == "str" else None)


def agree(layouts):
    """The one layout all of ``layouts`` (one per rank, any order) can
    build, or None when they have no common columnar form.  Empty ranks
    take what the others have, int and float promote to float, strings
    mix with nothing else, and string tables merge into their union: a
    per-rank table would give one id two meanings after an exchange."""
    kks = {m.kkind for m in layouts} - {"empty"}
    vks = {m.vkind for m in layouts} - {"empty"}
    keyeds = {m.keyed for m in layouts} - {None}
    if "obj" in kks | vks or len(keyeds) > 1 \
            or any("str" in s and len(s) > 1 for s in (kks, vks)):
        return None

    def common(kinds):
        return "str" if "str" in kinds else \
            "float" if "float" in kinds else "int"

    table = None
    if "str" in kks:
        table = tuple(sorted(set().union(*[m.table for m in layouts
                                           if m.table])))
    return Layout(common(kks), common(vks), keyeds == {True}, table)


def build(records, layout):
    """CPU columns of ``records`` in an agreed ``layout``:
    ``(keys i64, vals, keyed, fkeys, str_table)``.  Mixed int+float keys
    go through float64, so ints beyond 2^53 lose precision; such
    pipelines belong on the host engine."""
    ks = [k for k, _ in records]
    vs = [v[1] if layout.keyed else v for _, v in records]
    if layout.vkind == "str":
        from .strvals import StrVals
        vals = StrVals.from_strings(vs)
    else:
        vals = torch.from_numpy(np.asarray(
            vs, dtype=np.int64 if layout.vkind == "int" else np.float64))
    if layout.kkind == "str":
        # dictionary encoding: rank ids preserve lexicographic order
        rank = {t: i for i, t in enumerate(layout.table)}
        keys = torch.from_numpy(np.fromiter(
            (rank[k] for k in ks), dtype=np.int64, count=len(ks)))
    elif layout.kkind == "int":
        keys = torch.from_numpy(np.asarray(ks, dtype=np.int64))
    else:
        keys = encode_f64_sortable(
            torch.from_numpy(np.asarray(ks, dtype=np.float64)))
    return keys, vals, layout.keyed, layout.kkind == "float", layout.table


def decode(keys, vals, keyed=False, fkeys=False, str_table=None):
    """The records of a (keys, vals) column pair, in row order.  A lazy
    ``StrTable`` is first touched by the first key looked up in it.
    Both columns convert here, at once; what comes back is an iterator
    that only pairs them up, so the caller's ``list()`` or ``extend()``
    builds the one list of records there is (a list made here would be
    copied again: measured 15% on reading 2M string keys)."""
    if fkeys:
        keys = decode_f64_sortable(keys)
    kl = keys.cpu().tolist()
    if str_table is not None:
        kl = [str_table[i] for i in kl]
    vl = vals.cpu().tolist()
    if keyed:
        return ((k, (k, v)) for k, v in zip(kl, vl))
    return zip(kl, vl)


def decode_text(data):
    """``(byte offset, line)`` records of newline-delimited text bytes.
    The newline that ends the text starts no line, and an empty last
    line is dropped."""
    records = []
    pos = 0
    for line in data.split(b"\n"):
        if line or pos + len(line) < len(data):
            records.append((pos, line.decode("utf-8", "replace")))
        pos += len(line) + 1
    if records and pos - 1 >= len(data) and not records[-1][1]:
        records.pop()
    return records
