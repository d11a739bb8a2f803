"""Named, *recognizable* function objects used as DSL defaults.

The reference's API is lambda-everywhere (e.g. ``count(key=lambda x: x)``,
reference: dampr.py:439-448); opaque lambdas can only run on the host.  The
MI355X engine lowers a stage to device kernels when the functions it was
built from are these named objects (or a handful of stdlib ones:
``operator.add``, builtin ``min``/``max``) — identity-preserving `is`
checks, never bytecode inspection.  Users who pass their own callables get
the host path for that stage automatically; passing these (or just using
the DSL defaults) gets the device path.
"""
import operator


def identity(x):
    return x


def one(_x):
    return 1


def fst(x):
    return x[0]


def snd(x):
    return x[1]


add = operator.add
mul = operator.mul


# --- recognition tables ----------------------------------------------------

# binop -> segmented-reduce op name understood by the device backend
ASSOC_BINOPS = {
    add: "sum",
    operator.add: "sum",
    min: "min",
    max: "max",
}

# key/value extractors the columnar engine can apply without host trips
# (as kv extractors fst/snd await pair-column support in the engine; as
# predicate selectors, below, they pick the key or value column)
COLUMN_FUNCS = {
    identity: "identity",
    one: "one",
}


# --- filter predicates -------------------------------------------------------
# ``filter(funcs.gt(0))`` instead of ``filter(lambda x: x > 0)``: the same
# test on the host, and an object the DSL recognizes by type, so the
# columnar engine can evaluate it over the key or value column on device.

_SELECTORS = {identity: "identity", fst: "fst", snd: "snd"}

_COMPARE = {
    "gt": operator.gt,
    "ge": operator.ge,
    "lt": operator.lt,
    "le": operator.le,
    "eq": operator.eq,
    "ne": operator.ne,
}


class Predicate(object):
    """``on(v) OP constants`` as a callable.  ``on`` is ``identity`` (the
    record value; also the meaning of ``None``), ``fst`` or ``snd``; ``op``
    is one of gt/ge/lt/le/eq/ne/between/startswith/isin/notin.  Calling it
    runs the plain Python comparison, so every engine can use it as an
    opaque function; the device engine reads ``clause()`` (numeric
    constants, or a set) or ``str_clause()`` (string constants) instead."""

    __slots__ = ("on", "op", "constants")

    def __init__(self, op, constants, on=None):
        on = identity if on is None else on
        if _SELECTORS.get(on) is None:
            raise TypeError(
                "on= must be None, funcs.identity, funcs.fst or funcs.snd")
        assert op in ("between", "startswith", "isin", "notin") or \
            op in _COMPARE
        self.on = on
        self.op = op
        self.constants = tuple(constants)

    @property
    def selector(self):
        return _SELECTORS[self.on]

    def __call__(self, v):
        x = self.on(v)
        if self.op == "between":
            lo, hi = self.constants
            return lo <= x <= hi
        if self.op == "startswith":
            return x.startswith(self.constants[0])
        if self.op == "isin":
            return x in self.constants[0]
        if self.op == "notin":
            return x not in self.constants[0]
        return _COMPARE[self.op](x, self.constants[0])

    def clause(self):
        """``(selector, op, constants)`` for lowering, or None when a
        constant is not an int, float or bool (such a predicate still
        works as a host function).  A set predicate always has one: whether
        its members lower is decided against the column it selects
        (``set_members_lower``)."""
        if self.op in ("isin", "notin"):
            return (self.selector, self.op, self.constants)
        if self.op == "startswith" or \
                not all(isinstance(c, (int, float)) for c in self.constants):
            return None
        return (self.selector, self.op, self.constants)

    def str_clause(self):
        """``(selector, op, constants)`` for lowering over a string column,
        or None unless every constant is exactly a ``str`` that encodes to
        UTF-8 (a lone surrogate does not)."""
        for c in self.constants:
            if type(c) is not str:
                return None
            try:
                c.encode("utf-8", "strict")
            except UnicodeEncodeError:
                return None
        return (self.selector, self.op, self.constants)

    def __repr__(self):
        if self.op in ("isin", "notin"):
            return "{}(<{} members>, on={})".format(
                self.op, len(self.constants[0]), self.selector)
        return "{}({}, on={})".format(
            self.op, ", ".join(repr(c) for c in self.constants),
            self.selector)


def gt(c, on=None):
    """on(v) > c"""
    return Predicate("gt", (c,), on)


def ge(c, on=None):
    """on(v) >= c"""
    return Predicate("ge", (c,), on)


def lt(c, on=None):
    """on(v) < c"""
    return Predicate("lt", (c,), on)


def le(c, on=None):
    """on(v) <= c"""
    return Predicate("le", (c,), on)


def eq(c, on=None):
    """on(v) == c"""
    return Predicate("eq", (c,), on)


def ne(c, on=None):
    """on(v) != c"""
    return Predicate("ne", (c,), on)


def between(lo, hi, on=None):
    """lo <= on(v) <= hi (inclusive on both ends)"""
    return Predicate("between", (lo, hi), on)


def startswith(prefix, on=None):
    """on(v).startswith(prefix)"""
    return Predicate("startswith", (prefix,), on)


def isin(values, on=None):
    """on(v) in values (a set is taken of them, so they must hash)"""
    return Predicate("isin", (frozenset(values),), on)


def notin(values, on=None):
    """on(v) not in values"""
    return Predicate("notin", (frozenset(values),), on)


def set_members_lower(members):
    """The members of an isin / notin set as plain Python values, or None
    when the device cannot reproduce ``in`` for them.  ``in`` compares by
    identity before equality, which only the host can follow, so a set
    lowers only if every member is exactly an ``int``, ``float``, ``bool``
    or ``str`` (numpy integer and floating scalars count as their Python
    kinds), no member is NaN and every ``str`` encodes to UTF-8."""
    import numpy as np
    out = []
    for c in members:
        if isinstance(c, np.integer):
            c = int(c)
        elif isinstance(c, np.floating):
            c = float(c)
        if type(c) is str:
            try:
                c.encode("utf-8", "strict")
            except UnicodeEncodeError:
                return None
        elif type(c) is float:
            if c != c:
                return None
        elif type(c) not in (int, bool):
            return None
        out.append(c)
    return out


def filter_clause(f):
    """Device clause of a filter function, or None (opaque callable, or a
    predicate over constants the device cannot compare)."""
    if type(f) is Predicate:
        return f.clause()
    return None


def filter_str_clause(f):
    """Device clause of a filter function over a string column, or None
    (opaque callable, or a predicate whose constants are not all ``str``
    that encode to UTF-8)."""
    if type(f) is Predicate:
        return f.str_clause()
    return None


_TOKEN_RE = None


def tokenize_set(line):
    """Distinct ASCII word-tokens of a line, lowercased — the host mirror
    of the device tokenizer (ops/hip: is_word/lower_ascii).  Built-in so
    ``device_text(...).flat_map(funcs.tokenize_set).count()`` lowers to
    the fused single-pass document-frequency kernel."""
    global _TOKEN_RE
    if _TOKEN_RE is None:
        import re
        _TOKEN_RE = re.compile(r"[a-z0-9_]+")
    return set(_TOKEN_RE.findall(line.lower()))


# --- join pair aggregates ---------------------------------------------------
# PJoin.reduce(aggregate, many=True) aggregates the cartesian product of
# each key's (left values, right values).  These named per-pair forms let
# the device engine emit the product straight from the hash-join kernel.
#
# The right side is materialized first: the engines hand one-pass group
# iterators to aggregates (as the reference does), so a bare nested
# comprehension would exhaust `right` after the first left value and
# silently drop pairs.  These named funcs are defined as the FULL cross
# product — identical on the host path and the hash-join kernel.

def pair_sum(left, right):
    right = list(right)
    return [lv + rv for lv in left for rv in right]


def pair_product(left, right):
    right = list(right)
    return [lv * rv for lv in left for rv in right]


def pair_left(left, right):
    right = list(right)
    return [lv for lv in left for _rv in right]


def pair_right(left, right):
    right = list(right)
    return [rv for _lv in left for rv in right]


JOIN_PAIR_FUNCS = {
    pair_sum: "sum",
    pair_product: "mul",
    pair_left: "left",
    pair_right: "right",
}


# cross-join (K9) apply ops the device can fuse over the broadcast
# product; all COMMUTATIVE, so cross_left/cross_right share one table
# (cross_right wraps its lambda with swapped operands).
CROSS_BINOPS = {
    add: "add",
    operator.add: "add",
    mul: "mul",
    operator.mul: "mul",
    min: "min",
    max: "max",
}


# cross_set aggregate: the whole broadcast side folds to ONE scalar
SET_AGGS = {
    sum: "sum",
    min: "min",
    max: "max",
}


def set_agg_name(f):
    try:
        return SET_AGGS.get(f)
    except TypeError:
        return None


def cross_binop_name(f):
    try:
        return CROSS_BINOPS.get(f)
    except TypeError:
        return None


def join_pair_name(f):
    try:
        return JOIN_PAIR_FUNCS.get(f)
    except TypeError:
        return None


def binop_name(f):
    """Device op name for an associative binop, or None."""
    try:
        return ASSOC_BINOPS.get(f)
    except TypeError:
        return None


def column_func_name(f):
    try:
        return COLUMN_FUNCS.get(f)
    except TypeError:
        return None
