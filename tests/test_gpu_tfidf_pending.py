"""tfidf_docs_kernel's emit phases: the batched block-cache probe, the
global part (both table loads first, the slow probe loops when a loaded
word is not the key, the count add last) and the dict insert that
block-cache hits skip, with the block cache full.  The cases are those
a per-lane pending entry would also have to pass (last tokens of a text
or span, tokens that end on a window edge, several token ends per lane).
Every case is exact against ``corpus.oracle_df`` and checks each key's
token string through ``token_strings``; the CPU tests pin the shapes the
GPU cases rely on (distinct tokens per block, token ends on window edges).

A block is DOC_WAVES = 4 waves, a wave owns an 8 KiB span, so a text of at
most 32 KiB is one block and one of at most 8 KiB is one wave.  The block's
count cache has 1,024 slots."""
import functools

import numpy as np
import pytest
import torch

from dampr_amd import keyhash

HAVE_GPU = torch.cuda.is_available()


def gpu(fn):
    fn = pytest.mark.skipif(not HAVE_GPU, reason="needs an MI355X")(fn)
    return pytest.mark.gpu(fn)


DEV = torch.device("cuda:0") if HAVE_GPU else None
_MASK = (1 << 64) - 1
SPAN = 8192                     # DOC_SPAN; checked against the extension
BLOCK_BYTES = 4 * SPAN          # DOC_WAVES spans
CCACHE = 1024                   # block count-cache slots
DOC_SET = 256                   # per-wave dedupe set slots
WIN = 512                       # bytes per wave window
_AL = "abcdefghijklmnopqrstuvwxyz0123456789_"


@pytest.fixture(scope="module")
def engine():
    from dampr_amd.gpu.tfidf import TfidfEngine
    return TfidfEngine(DEV, vocab_capacity=1 << 18)


def _arr(data):
    if isinstance(data, str):
        data = data.encode()
    return np.frombuffer(bytes(data), dtype=np.uint8).copy()


@functools.lru_cache(maxsize=None)
def _want(text):
    """(oracle df, {key: (df, token bytes)}) of a text, computed once."""
    from dampr_amd.gpu.corpus import oracle_df
    df = oracle_df(_arr(text))
    keys = {(keyhash.tokmix64(t.encode()) or 1): (d, t.encode())
            for t, d in df.items()}
    assert len(keys) == len(df)
    return df, keys


def _keys_and_strings(engine, dev_text):
    keys, df = engine.extract()
    blob, lens = engine.token_strings(keys, dev_text)
    b = blob.tobytes()
    out, pos = {}, 0
    for k, d, ln in zip(keys.cpu().tolist(), df.cpu().tolist(),
                        lens.tolist()):
        out[int(k) & _MASK] = (int(d), b[pos:pos + int(ln)])
        pos += int(ln)
    return out


def _check(text, engine, **kw):
    """df per token and (df, lowercased string) per key, both exact."""
    from dampr_amd.gpu.tfidf import run_tfidf
    want_df, want_keys = _want(text)
    dev_text = torch.from_numpy(_arr(text)).to(DEV)
    got = {t: v[0] for t, v in run_tfidf(dev_text, device=DEV,
                                         engine=engine, **kw).items()}
    assert got == want_df
    assert _keys_and_strings(engine, dev_text) == want_keys
    return got


# ------------------------------------------------------------ inputs


def _tok79(i):
    """Distinct tokens of 7, 8 and 9 bytes."""
    return "w{:05d}".format(i) + "xyz"[:1 + i % 3]


def _two_pass_text(n_tok, per_line=12):
    """Every token in exactly two documents: once in index order, once in
    a stride order that never pairs the same neighbours."""
    toks = [_tok79(i) for i in range(n_tok)]
    second = [toks[(i * 7 + 3) % n_tok] for i in range(n_tok)]
    assert sorted(second) == sorted(toks)
    lines = [" ".join(p[i:i + per_line])
             for p in (toks, second) for i in range(0, n_tok, per_line)]
    return "\n".join(lines) + "\n"


@functools.lru_cache(maxsize=None)
def _one_block_text():
    return _two_pass_text(1800)


@functools.lru_cache(maxsize=None)
def _two_block_text():
    return _two_pass_text(3000)


def _tok2(i):
    return _AL[i // 37] + _AL[i % 37]          # 37^2 = 1,369 tokens


def _tok3(i):
    return _AL[i // 1296 % 36] + _AL[i // 36 % 36] + _AL[i % 36]


@functools.lru_cache(maxsize=None)
def _two_char_text():
    """`ab cd ef `: three token ends per 8-byte lane word."""
    toks = [_tok2(i) for i in range(37 * 37)]
    second = [toks[(i * 5 + 1) % len(toks)] for i in range(len(toks))]
    lines = [" ".join(p[i:i + 21]) for p in (toks, second)
             for i in range(0, len(toks), 21)]
    return "\n".join(lines) + "\n"


def _fill_lines(n_bytes, first=0):
    """n_bytes (a multiple of 64) of 64-byte lines of 3-byte tokens in
    4-byte cells, 16 new tokens per line; line k ends with a newline."""
    assert n_bytes % 64 == 0
    out = []
    for k in range(n_bytes // 64):
        cells = "".join(_tok3(first + 16 * k + j) + " " for j in range(16))
        out.append(cells[:-1] + "\n")
    return "".join(out)


def _pad_to(body, n, tail):
    """body, then spaces, then tail: exactly n bytes."""
    assert len(body) + len(tail) <= n
    return body + " " * (n - len(body) - len(tail)) + tail


@functools.lru_cache(maxsize=None)
def _drain_texts():
    """name -> text; each holds one token that occurs nowhere else, behind
    more than CCACHE distinct filler tokens."""
    fill = _fill_lines(5120)                    # 1,280 distinct tokens
    out = {}
    # the text ends in a token, no newline
    out["tail_no_newline"] = fill + "aa bb lastTOKEN_x1"
    # the unique token sits in the last window of the closing document
    out["closing_doc_last_window"] = (
        fill + " ".join(_tok3(i) for i in range(300)) + " closing_DOC9\n")
    # exactly one span and exactly three spans, with and without newline
    out["one_span"] = _pad_to(fill, SPAN, "spanEND_1\n")
    out["one_span_no_newline"] = _pad_to(fill, SPAN, "spanEND_2")
    three = fill + _fill_lines(2 * SPAN, first=2000)
    out["three_spans"] = _pad_to(three, 3 * SPAN, "spanEND_3\n")
    out["three_spans_no_newline"] = _pad_to(three, 3 * SPAN, "spanEND_4")
    return out


@functools.lru_cache(maxsize=None)
def _carry_text():
    """One wave (less than a span).  Six 1 KiB groups of filler fill the
    cache; groups start on multiples of 1,024, so windows start on
    multiples of 512.  Group 6 holds a token that ends on byte 511 of its
    first window with a separator behind it and the document going on
    (lane 0 emits it as a carry in the next window); group 7 is one
    512-byte document that ends in a token, its newline being the first
    byte of the next window and the last byte of the text (the group ends
    with a live token)."""
    fill = _fill_lines(6144)
    g6 = list(_fill_lines(1024, first=3000))
    # lines 7 and 8 of the group (bytes 448..575) become one document
    g6[511] = " "
    tok = "EDGE_carry_1"
    g6[448:576] = list(" " * 128)
    g6[512 - len(tok):512] = list(tok)
    g6[516:523] = list("after_7")
    g6[575] = "\n"
    tok2 = "edge_LIVE_2"
    g7 = "pre_a pre_b".ljust(512 - len(tok2)) + tok2 + "\n"
    return fill + "".join(g6) + g7, tok, tok2


@functools.lru_cache(maxsize=None)
def _many_blocks_text(reps):
    """A 24 KiB paragraph (1,536 distinct 7-byte tokens in 8-byte cells,
    each in two of its 96-byte documents) repeated `reps` times."""
    toks = ["p{:04d}qr".format(i) for i in range(1536)]
    cells = toks + [toks[(i * 11 + 5) % 1536] for i in range(1536)]
    lines = [" ".join(cells[i:i + 12]) for i in range(0, len(cells), 12)]
    para = "\n".join(lines) + "\n"
    assert len(para) == 24 * 1024
    return para * reps


@functools.lru_cache(maxsize=None)
def _three_chunk_text():
    """Three sections of equal length (about 9 KiB), one chunk each:
    `Word word WORD` spellings of shared tokens, and tokens that first
    occur in sections 2 and 3."""
    def spell(t, k):
        return (t, t.capitalize(), t.upper())[k % 3]
    secs = []
    for s in range(3):
        toks = ["shared{:03d}".format(i) for i in range(400)]
        toks += ["only{}_{:03d}".format(s, i) for i in range(500)]
        cells = [spell(t, i + s) for i, t in enumerate(toks)]
        lines = [" ".join(cells[i:i + 10])
                 for i in range(0, len(cells), 10)]
        sec = "\n".join(lines) + "\n"
        secs.append(sec)
    return "".join(secs), len(secs[0])


@functools.lru_cache(maxsize=None)
def _set_overflow_text():
    big = ["t{}".format(i) for i in range(600)]
    lines = ["x t1 t2", "y t599", " ".join(big + big[::-1]), "t0 z",
             "t300 t300 x"]
    return _fill_lines(5120) + "\n".join(lines) + "\n"


def _distinct_per_block(text):
    """Distinct lowercased tokens among the documents that start in each
    32 KiB block (the kernel's ownership rule)."""
    import re
    rx = re.compile(r"[^\w]+")
    blocks, pos = {}, 0
    for line in text.split("\n"):
        if pos < len(text):
            blocks.setdefault(pos // BLOCK_BYTES, set()).update(
                t for t in rx.split(line.lower()) if t)
        pos += len(line) + 1
    return [len(blocks.get(b, ()))
            for b in range((len(text) + BLOCK_BYTES - 1) // BLOCK_BYTES)]


# ------------------------------------------------------------ CPU-only


def test_cache_overflow_inputs():
    one = _one_block_text()
    assert len(one) <= BLOCK_BYTES
    assert _distinct_per_block(one) == [1800]
    assert {len(_tok79(i)) for i in range(1800)} == {7, 8, 9}
    assert all(d == 2 for d in _want(one)[0].values())
    two = _two_block_text()
    assert BLOCK_BYTES < len(two) <= 2 * BLOCK_BYTES
    per = _distinct_per_block(two)
    assert len(per) == 2 and min(per) > CCACHE
    df = _want(two)[0]
    assert len(df) == 3000 and all(d == 2 for d in df.values())
    # load of a 4,096-slot table
    assert 0.72 < len(df) / 4096.0 < 0.74


def test_two_char_inputs():
    text = _two_char_text()
    assert len(text) <= BLOCK_BYTES
    df = _want(text)[0]
    assert len(df) == 1369 > CCACHE
    assert all(len(t) == 2 and d == 2 for t, d in df.items())
    assert text.startswith("aa ab ac ")    # three ends in bytes 0..7


def test_drain_inputs():
    texts = _drain_texts()
    assert len(texts["one_span"]) == SPAN
    assert len(texts["one_span_no_newline"]) == SPAN
    assert len(texts["three_spans"]) == 3 * SPAN
    assert len(texts["three_spans_no_newline"]) == 3 * SPAN
    for name, text in texts.items():
        assert len(text) <= BLOCK_BYTES
        assert _distinct_per_block(text)[0] > CCACHE, name
        assert text.endswith("\n") == (not name.endswith("no_newline")
                                       and name != "tail_no_newline")
    for name, tok in [("tail_no_newline", "lasttoken_x1"),
                      ("closing_doc_last_window", "closing_doc9"),
                      ("one_span", "spanend_1"),
                      ("one_span_no_newline", "spanend_2"),
                      ("three_spans", "spanend_3"),
                      ("three_spans_no_newline", "spanend_4")]:
        text = texts[name]
        assert _want(text)[0][tok] == 1
        assert text.lower().count(tok) == 1
        # the unique token is the last one of the text
        assert text.lower().rstrip("\n").endswith(tok)


def test_carry_inputs():
    text, tok, tok2 = _carry_text()
    assert len(text) == 6144 + 1024 + 513 < SPAN
    assert _distinct_per_block(text[:6144]) == [1536]
    df = _want(text)[0]
    assert df[tok.lower()] == 1 and df[tok2.lower()] == 1
    # every newline before group 6 is at 63 mod 64: groups are 1 KiB
    nl = [i for i, c in enumerate(text[:6144]) if c == "\n"]
    assert nl == list(range(63, 6144, 64))
    e = text.index(tok) + len(tok) - 1
    assert e == 6144 + WIN - 1 and text[e + 1] == " "
    assert "\n" not in text[6144 + 448:e + 1 + 60]     # the doc goes on
    e2 = text.index(tok2) + len(tok2) - 1
    assert e2 == 7168 + WIN - 1 and text[e2 + 1] == "\n"
    assert e2 + 2 == len(text)
    assert "\n" not in text[7168:e2 + 1]


def test_many_blocks_inputs():
    for reps in (16, 86):
        text = _many_blocks_text(reps)
        assert len(text) == reps * 24 * 1024
        df = _want(text)[0]
        assert len(df) == 1536
        assert all(d == 2 * reps for d in df.values())
    assert len(_many_blocks_text(86)) >= 64 * BLOCK_BYTES
    assert min(_distinct_per_block(_many_blocks_text(16))) > CCACHE


def test_three_chunk_inputs():
    text, sec = _three_chunk_text()
    assert len(text) == 3 * sec and text[sec - 1] == "\n"
    df = _want(text)[0]
    assert df["shared007"] == 3 and df["only1_007"] == 1
    assert "only1_007" not in text[:sec].lower()
    assert "only2_007" not in text[:2 * sec].lower()
    assert {"Shared001", "SHARED002", "shared000"} <= set(text.split())
    assert min(_distinct_per_block(text)) > 0


def test_set_overflow_inputs():
    text = _set_overflow_text()
    assert len(text) <= BLOCK_BYTES
    assert _distinct_per_block(text)[0] > CCACHE
    assert max(len(set(l.split())) for l in text.split("\n")) > DOC_SET


# ------------------------------------------------------------ GPU


@gpu
def test_span_bytes(engine):
    assert engine.ext.tfidf_span_bytes() == SPAN


@gpu
@pytest.mark.parametrize("which", ["one_block", "two_blocks"])
def test_cache_overflow(engine, which):
    text = _one_block_text() if which == "one_block" else _two_block_text()
    got = _check(text, engine)
    assert all(d == 2 for d in got.values())


@gpu
def test_probe_chains_small_tables():
    from dampr_amd.gpu.tfidf import TfidfEngine
    small = TfidfEngine(DEV, vocab_capacity=1 << 12)
    assert small.cap == 4096
    got = _check(_two_block_text(), small)
    assert len(got) == 3000
    got = _check(_one_block_text(), small)
    assert len(got) == 1800


@gpu
def test_several_ends_per_lane(engine):
    got = _check(_two_char_text(), engine)
    assert len(got) == 1369


@gpu
@pytest.mark.parametrize("name", ["tail_no_newline",
                                  "closing_doc_last_window", "one_span",
                                  "one_span_no_newline", "three_spans",
                                  "three_spans_no_newline"])
def test_drain(engine, name):
    _check(_drain_texts()[name], engine)


@gpu
def test_window_edge_carry(engine):
    text, tok, tok2 = _carry_text()
    got = _check(text, engine)
    assert got[tok.lower()] == 1 and got[tok2.lower()] == 1


@gpu
@pytest.mark.parametrize("reps", [16, 86])
def test_many_blocks_same_keys(engine, reps):
    got = _check(_many_blocks_text(reps), engine)
    assert set(got.values()) == {2 * reps}


@gpu
def test_three_chunks(engine):
    text, sec = _three_chunk_text()
    one = _check(text, engine)
    assert _check(text, engine, chunk_bytes=sec) == one
    # chunk ends that fall inside a line move to the line's end
    assert _check(text, engine, chunk_bytes=sec - 17) == one


@gpu
def test_set_overflow_with_cache_full(engine):
    got = _check(_set_overflow_text(), engine)
    assert got["t1"] == 2 and got["t599"] == 2 and got["t300"] == 2
    assert got["t17"] == 1 and got["x"] == 2
