"""The overflow rerun of a chunk rolls back cnt_vals alone: the string
dict and cnt_keys keep what the failed pass left (valid occurrences and
keys the rerun counts again).  An engine with an 8-slot fallback seen
table makes the rerun reachable at test size."""
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
def span():
    from dampr_amd.ops import native
    return int(native.require().tfidf_span_bytes())


def _arr(data):
    if isinstance(data, str):
        data = data.encode()
    return np.frombuffer(bytes(data), dtype=np.uint8).copy()


def _n_docs(arr):
    """newlines + one unterminated tail line."""
    return int((arr == NL).sum()) + int(arr.size > 0 and arr[-1] != NL)


def _lines(n_bytes, seed=0):
    """Exactly n_bytes of short newline-terminated lines: a token of its
    own per line, tokens shared by many lines, one repeated in the line."""
    rnd = random.Random(seed)
    out, size, k = [], 0, 0
    while size < n_bytes:
        ln = "u{} s{} s{} c{} Common s{}\n".format(
            k, k % 89, rnd.randrange(40), rnd.randrange(7), k % 89)
        out.append(ln)
        size += len(ln)
        k += 1
    buf = bytearray("".join(out)[:n_bytes].encode())
    buf[-1] = NL
    return bytes(buf)


@gpu
def test_overflow_rerun_keeps_earlier_counts(span):
    """An 8-slot fallback seen table: a line of 300 distinct tokens
    overflows the 256-slot LDS set, fills the 8 slots and trips the probe
    bound (the designed error-flag path), so chunk 2 reruns on the general
    kernel with only cnt_vals rolled back.  Chunk 1's counts must
    survive, and chunk 2 must count once."""
    from dampr_amd.gpu.corpus import oracle_df
    from dampr_amd.gpu.tfidf import TfidfEngine, chunk_bounds
    eng = TfidfEngine(DEV, vocab_capacity=1 << 16, fallback_seen_capacity=8)
    c1 = _lines(3 * span, seed=6)
    wide = " ".join("wide{}".format(i) for i in range(300)) + " s1 Common\n"
    c2 = _lines(span + 500, seed=7) + wide.encode() + _lines(span, seed=8)
    text = _arr(c1 + c2)
    bounds = chunk_bounds(torch.from_numpy(text), len(c1))
    assert bounds == [0, len(c1), len(text)]
    t = torch.from_numpy(text).to(DEV)
    eng.reset()
    flags = []
    for s, e in zip(bounds, bounds[1:]):
        n = eng.count_chunk(t[s:e].contiguous(), pos_base=s)
        assert n == _n_docs(text[s:e])
        flags.append(eng._err.tolist()[0])
    assert flags == [0, 1]                     # chunk 2 took the rerun
    assert eng.n_docs == _n_docs(text)
    keys, df = eng.extract()
    blob, lens = eng.token_strings(keys, t)
    got, pos, b = {}, 0, blob.tobytes()
    for ln, d in zip(lens.tolist(), df.cpu().tolist()):
        got[b[pos:pos + ln].decode("ascii")] = d
        pos += ln
    want = oracle_df(text)
    assert got == want
    assert got["wide299"] == 1 and got["s1"] == want["s1"] > 2
