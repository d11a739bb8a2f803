"""tfidf_docs_kernel with span ownership: a wave owns a fixed byte span,
processes the documents that start in it and finds their boundaries in
the staged text.  Newlines around span edges, documents longer than a
span / a group / a stage, empty lines, missing newlines, odd lengths,
multi-chunk runs and random text against the exact CPU oracle, with the
kernel's own document count; plus a CPU model of the ownership rule."""
import random

import numpy as np
import pytest
import torch

HAVE_GPU = torch.cuda.is_available()


def gpu(fn):
    fn = pytest.mark.skipif(not HAVE_GPU, reason="needs an MI355X")(fn)
    return pytest.mark.gpu(fn)


DEV = torch.device("cuda:0") if HAVE_GPU else None
NL = ord("\n")


@pytest.fixture(scope="module")
def engine():
    from dampr_amd.gpu.tfidf import TfidfEngine
    return TfidfEngine(DEV, vocab_capacity=1 << 18)


@pytest.fixture(scope="module")
def span(engine):
    s = int(engine.ext.tfidf_span_bytes())
    assert s % 16 == 0 and 4096 <= s <= 8192
    return s


def _arr(data):
    if isinstance(data, str):
        data = data.encode()
    return np.frombuffer(bytes(data), dtype=np.uint8).copy()


def _n_docs(arr):
    """newlines + one unterminated tail line."""
    return int((arr == NL).sum()) + int(arr.size > 0 and arr[-1] != NL)


def _check(data, engine, limit=None, **kw):
    """dfs, materialised token strings and the document count equal the
    oracle's."""
    from dampr_amd.gpu.corpus import oracle_df
    from dampr_amd.gpu.tfidf import run_tfidf
    arr = _arr(data)
    if limit is not None:
        assert arr.size <= limit, (arr.size, limit)
    got = {t: v[0]
           for t, v in run_tfidf(arr, device=DEV, engine=engine,
                                 **kw).items()}
    assert got == oracle_df(arr)
    assert engine.n_docs == _n_docs(arr)
    return got


def _words(n_bytes, start=0, line=0):
    """Exactly n_bytes of distinct short tokens ("w0 w1 ..."), padded
    with commas; a newline every `line` bytes when line > 0."""
    out, k = [], start
    size = 0
    while size < n_bytes:
        tok = "w{} ".format(k)
        out.append(tok)
        size += len(tok)
        k += 1
    buf = bytearray("".join(out)[:n_bytes].encode())
    if buf and chr(buf[-1]).isalnum():
        buf[-1] = ord(",")                 # no cut token at the end
    if line:
        for p in range(line - 1, n_bytes, line):
            buf[p] = NL
    return bytes(buf)


# ------------------------------------------------------------ CPU-only


def _owned_docs(text, a, b):
    """Ownership rule as the kernel states it: skip to the first newline
    at a position >= a-1 (nothing when a == 0), run through the first
    newline at a position >= b-1 (or to n).  Returns doc start bytes."""
    n = len(text)
    if a >= n:
        return []
    start = 0
    if a > 0:
        p = text.find(b"\n", a - 1)
        if p < 0:
            return []
        start = p + 1
    if start >= min(b, n):
        return []
    e = text.find(b"\n", b - 1)
    end = n if e < 0 else e + 1            # one past the closing newline
    starts, s = [], start
    while s < min(end, n):
        starts.append(s)
        q = text.find(b"\n", s)
        s = n if q < 0 else q + 1
    return starts


def test_every_document_has_one_owner():
    rnd = random.Random(11)
    for span_bytes in (1, 2, 3, 5, 16, 48):
        for _ in range(150):
            n = rnd.randrange(0, 200)
            rate = rnd.choice([0.0, 0.02, 0.1, 0.5, 1.0])
            text = bytes(NL if rnd.random() < rate else ord("a")
                         for _ in range(n))
            want = [0] if n else []
            want += [i + 1 for i in range(n - 1) if text[i] == NL]
            got = []
            for a in range(0, n, span_bytes):
                got += _owned_docs(text, a, a + span_bytes)
            assert got == want, (span_bytes, text)
            assert len(got) == text.count(b"\n") + int(
                n > 0 and text[-1] != NL)


# ------------------------------------------------------------ GPU


@gpu
@pytest.mark.parametrize("edge", [1, 2])
def test_newline_swept_across_span_edge(engine, span, edge):
    # distinct tokens; the only newline near the edge is the swept one,
    # so a-1, a and b-1 each get to be the newline and the token that
    # straddles the edge belongs to one document
    base = bytearray(_words(3 * span + 40, line=200))
    at = edge * span
    for p in range(at - 64, at + 64):
        if base[p] == NL:
            base[p] = ord(" ")
    for p in range(at - 18, at + 19):
        text = bytearray(base)
        text[p] = NL
        _check(text, engine, limit=4 * span + 64)


@gpu
@pytest.mark.parametrize("length", ["S+1", "2S", "3S+7"])
def test_document_longer_than_a_span(engine, span, length):
    ln = {"S+1": span + 1, "2S": 2 * span, "3S+7": 3 * span + 7}[length]
    long_doc = b"dup " + _words(ln - 8, start=1000) + b" dup"
    assert len(long_doc) == ln and NL not in long_doc
    for pre in (b"", b"aa bb\ncc dup\n"):
        text = pre + long_doc + b"\ndd aa\nee dup\n"
        got = _check(text, engine, limit=4 * span + 64)
        assert got["dup"] == 2 + (1 if pre else 0)


@gpu
def test_document_longer_than_group_and_stage(engine, span):
    # GROUP_BYTES = 1024, STAGE_B + 16 = 2064: the same token at both
    # ends of the doc must dedupe across the restage
    for ln in [1025] + list(range(2047, 2066)) + [4100]:
        long_doc = b"dup " + _words(ln - 8, start=500) + b" dup"
        assert len(long_doc) == ln
        text = b"x dup\n" + long_doc + b"\ny dup\n"
        got = _check(text, engine, limit=4 * span + 64)
        assert got["dup"] == 3
    # at a stage offset other than the group start's
    text = _words(700, line=70) + b"dup " + _words(2100, start=900) \
        + b" dup\nz\n"
    _check(text, engine)


@gpu
def test_runs_of_empty_lines(engine, span):
    _check("\n" * 50 + "a b\n" + "\n" * 1500 + "b c\n\n\n", engine)
    # a run of empty lines across the first span edge, at each phase
    for lead in (span - 40, span - 1, span, span + 1):
        text = _words(lead, line=90) + b"\n" * 80 + b"a b\n\nb"
        got = _check(text, engine, limit=4 * span + 64)
        assert got["b"] == 2
    # a whole span of newlines between text
    text = b"a b\n" + b"\n" * (2 * span) + b"b c\n"
    _check(text, engine, limit=4 * span + 64)


@gpu
def test_only_newlines(engine, span):
    for n in (1, 2, 16, 17, 1024, 1025, span - 1, span, span + 1,
              3 * span + 5):
        assert _check(b"\n" * n, engine) == {}
        assert engine.n_docs == n


@gpu
def test_no_newline_at_all(engine, span):
    for n in (1, 15, 17, 100, 1023, 1024, 1025, 2064, 2065, span - 1,
              span, span + 1, 2 * span + 9, 4 * span + 63):
        text = b"dup " + _words(n - 4, start=7) if n > 8 else b"a" * n
        assert len(text) == n
        _check(text, engine, limit=4 * span + 64)
        assert engine.n_docs == 1


@gpu
def test_empty_text(engine):
    engine.reset()
    assert engine.count_chunk(torch.empty(0, dtype=torch.uint8,
                                          device=DEV)) == 0
    assert engine.n_docs == 0


@gpu
def test_no_trailing_newline(engine, span):
    for n in (span - 3, span, span + 5, 2 * span + 1, 3 * span + 33):
        text = bytearray(_words(n, line=97))
        if text[-1] == NL:
            text[-1] = ord("q")
        # last newline right before the final byte, and a longer tail
        _check(text, engine, limit=4 * span + 64)
        text[-2] = NL
        _check(text, engine)


@gpu
def test_odd_lengths(engine, span):
    for n in [1, 15, 17, 31, 33, 95, 1039, span + 7, 2 * span + 13]:
        for last in (b"a", b"\n", b" "):
            text = bytearray(_words(n, line=41))
            text[-1:] = last
            assert len(text) == n and n % 16
            _check(text, engine)
    for text in ("a", "\n", "a\n", "\na", "ab cd ef gh ij\n", "a" * 15,
                 "a" * 17, "a b c d e f g h\n"):
        _check(text, engine)


@gpu
def test_two_chunks_with_nonzero_pos_base(engine, span):
    from dampr_amd.gpu.tfidf import chunk_bounds
    # newline-terminated lines of distinct tokens: every token string of
    # the second chunk is materialised through pos_base
    text = _arr(_words(2 * span + 150, line=64))
    text[-1] = NL
    bounds = chunk_bounds(torch.from_numpy(text), span + 96)
    assert len(bounds) == 3 and bounds[1] > span
    _check(text, engine, limit=4 * span + 64, chunk_bytes=span + 96)
    # the same through count_chunk, with the per-chunk document counts
    engine.reset()
    t = torch.from_numpy(text).to(DEV)
    counts = [engine.count_chunk(t[s:e].contiguous(), pos_base=s)
              for s, e in zip(bounds, bounds[1:])]
    assert counts == [_n_docs(text[s:e])
                      for s, e in zip(bounds, bounds[1:])]
    assert engine.n_docs == _n_docs(text)


def _random_text(seed, n=64 * 1024):
    # test_gpu_tfidf_lanes._random_text's alphabet and newline rate
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"abA_0 ,\n", dtype=np.uint8)
    p = np.full(8, (1.0 - 1.0 / 40) / 7)
    p[7] = 1.0 / 40
    return alphabet[rng.choice(8, size=n, p=p)].copy()


@gpu
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_text(engine, seed):
    _check(_random_text(seed), engine)
