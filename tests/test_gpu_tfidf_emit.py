"""tfidf_docs_kernel's table walk and emit path: the length-mix table's
boundary (127 / 128 / 129, 255 / 256), unconditional table reads over all
256 byte values and over masked lanes, the one-multiply dedupe salt (many
docs per group, repeats inside a doc, set overflow into the global
fallback) and multi-chunk positions, all against the exact CPU oracle;
plus a Python model of the salt (CPU-only)."""
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
SALT_K = 0x9E3779B97F4A7C15     # DOC_SALT_K in dampr_tfidf.hip
DOC_SET = 256                   # per-wave dedupe set slots


@pytest.fixture(scope="module")
def engine():
    from dampr_amd.gpu.tfidf import TfidfEngine
    return TfidfEngine(DEV, vocab_capacity=1 << 18)


def _arr(data):
    if isinstance(data, str):
        data = data.encode()
    return np.frombuffer(bytes(data), dtype=np.uint8).copy()


def _dfs(arr, engine, **kw):
    from dampr_amd.gpu.tfidf import run_tfidf
    return {t: v[0]
            for t, v in run_tfidf(arr, device=DEV, engine=engine,
                                  **kw).items()}


def _oracle(arr):
    """corpus.oracle_df under the kernel's byte rule: a byte >= 0x80 is
    never a word character (and never a newline), so it stands for any
    ASCII separator.  ASCII text goes to the oracle unchanged."""
    from dampr_amd.gpu.corpus import oracle_df
    arr = np.where(arr >= 0x80, np.uint8(ord(" ")), arr).astype(np.uint8)
    return oracle_df(arr)


def _check(data, engine):
    arr = _arr(data)
    got = _dfs(arr, engine)
    assert got == _oracle(arr)
    return got


def _keys_and_strings(engine, dev_text):
    """{key: (df, token bytes)} of the engine's current tables."""
    keys, df = engine.extract()
    blob, lens = engine.token_strings(keys, dev_text)
    b = blob.tobytes()
    out, pos = {}, 0
    for k, d, ln in zip(keys.cpu().tolist(), df.cpu().tolist(),
                        lens.tolist()):
        out[int(k) & _MASK] = (int(d), b[pos:pos + int(ln)])
        pos += int(ln)
    return out


# ------------------------------------------------------------ CPU-only


def _salt(doc_id):
    """Model of the kernel's dedupe salt: doc_id * K mod 2^64."""
    return (doc_id * SALT_K) & _MASK


def _salt_block_ok(lo, hi):
    ids = np.arange(lo, hi, dtype=np.uint64)
    s = ids * np.uint64(SALT_K)                  # wraps mod 2^64
    assert int(s[0]) == _salt(lo) and int(s[-1]) == _salt(hi - 1)
    assert np.unique(s).size == s.size           # injective
    assert np.all(((s[1:] ^ s[:-1]) & np.uint64(0xFF)) != 0)


def test_salt_model():
    _salt_block_ok(0, 1 << 20)
    # the largest chunk-relative id: gs + ordinal < 2^31
    _salt_block_ok((1 << 31) - 1 - 4096, (1 << 31) + 4096)
    # the low byte is a bijection of doc_id mod 256: ids less than 256
    # apart never share a start slot of the 256-slot set
    for base in [0, 12345, (1 << 31) - 300]:
        low = {_salt(base + i) & (DOC_SET - 1) for i in range(DOC_SET)}
        assert len(low) == DOC_SET


def _boundary_tokens():
    # one token per length 1..300, unique after lowercasing and after the
    # dictionary's cut at 255 bytes: the length leads, then mixed-case
    # letters, digits and '_'
    fill = "aB3_Zq9Xy0_Km7"
    return [("{}x".format(ln) + fill * 22)[:ln] for ln in range(1, 301)]


def _boundary_text():
    seps = " ,;-\t"
    lines = []
    for i, tok in enumerate(_boundary_tokens()):
        # a varying run of separators in front moves the token starts over
        # every lane phase; the text is continuous, so long tokens cross
        # lane, 512-byte window and 2048-byte stage edges
        lines.append("".join(seps[(i + k) % 5] for k in range(i * 7 % 13))
                     + tok + " q")
    return "\n".join(lines) + "\n"


def test_boundary_text_shape():
    toks = _boundary_tokens()
    assert [len(t) for t in toks] == list(range(1, 301))
    assert len({t.lower()[:255] for t in toks}) == 300
    text = _boundary_text()
    # tokens of 127..129 and 255..256 bytes cross a 512-byte window edge,
    # and some token crosses a 2048-byte edge
    pos, spans = 0, {}
    for line, tok in zip(text.split("\n"), toks):
        s = pos + line.index(tok)
        spans[len(tok)] = (s, s + len(tok) - 1)
        pos += len(line) + 1
    assert any(a // 2048 != b // 2048 for a, b in spans.values())
    assert any(a // 512 != b // 512 for a, b in spans.values())


# ------------------------------------------------------------ GPU


@gpu
def test_length_table_boundary(engine):
    toks = _boundary_tokens()
    arr = _arr(_boundary_text())
    got = _dfs(arr, engine)
    # the string dictionary stores at most 255 bytes of a token
    want = {t[:255]: df for t, df in _oracle(arr).items()}
    assert got == want
    assert got["q"] == 300 and len(got) == 301
    for t in toks:
        assert got[t.lower()[:255]] == 1

    dev_text = torch.from_numpy(arr).to(DEV)
    engine.reset()
    engine.count_chunk(dev_text)
    ks = _keys_and_strings(engine, dev_text)
    want_keys = {(keyhash.tokmix64(t.lower().encode()) or 1):
                 (1, t.lower().encode()[:255]) for t in toks}
    want_keys[keyhash.tokmix64(b"q") or 1] = (300, b"q")
    assert ks == want_keys


@gpu
def test_multi_chunk_boundary_text(engine):
    arr = _arr(_boundary_text())
    dev_text = torch.from_numpy(arr).to(DEV)
    engine.reset()
    assert engine.count_chunk(dev_text) == 300
    one = _keys_and_strings(engine, dev_text)

    n = arr.size
    cuts = [0]
    for target in (n // 3, 2 * n // 3):
        cuts.append(target + int(np.nonzero(arr[target:] == 10)[0][0]) + 1)
    cuts.append(n)
    assert cuts == sorted(set(cuts)) and len(cuts) == 4
    engine.reset()
    docs = 0
    for s, e in zip(cuts, cuts[1:]):
        docs += engine.count_chunk(dev_text[s:e].contiguous(), pos_base=s)
    assert docs == 300
    assert _keys_and_strings(engine, dev_text) == one


@gpu
def test_all_byte_values(engine):
    rng = np.random.default_rng(10)
    arr = rng.integers(0, 256, size=64 * 1024, dtype=np.uint8)
    arr[rng.random(arr.size) < 1.0 / 40] = 10
    assert np.unique(arr).size == 256
    _check(arr, engine)


@gpu
def test_masked_lanes_short_docs(engine):
    # documents of 1..17 bytes: every group tail leaves masked lanes and
    # masked bytes inside the last lane
    body = "aB_9 xY,q7-Zz_0kL"
    lines = [body[(3 * i) % 5:][:1 + i % 17].ljust(1 + i % 17, "e")
             for i in range(3000)]
    assert {len(l) for l in lines} == set(range(1, 18))
    _check("\n".join(lines) + "\n", engine)
    _check("\n".join(lines), engine)            # unterminated tail


@gpu
def test_salt_one_token_docs(engine):
    # 512 docs per 1 KiB group all insert the same token: more pairs than
    # the set holds, so the salted keys also reach the fallback
    assert _check("a\n" * 4000, engine) == {"a": 4000}


@gpu
def test_salt_repeats_inside_a_doc(engine):
    got = _check("al_1 Be2 GAMMA d e5 " * 40 + "\n", engine)
    assert got == {"al_1": 1, "be2": 1, "gamma": 1, "d": 1, "e5": 1}


@gpu
def test_salt_same_tokens_many_docs(engine):
    toks = ["w{}".format(i) for i in range(12)]
    got = _check((" ".join(toks) + "\n") * 2000, engine)
    assert got == {t: 2000 for t in toks}


@gpu
def test_salt_one_byte_and_empty_docs(engine):
    got = _check("a\n\nb\n\n\na\nb\n" * 300 + "\n\nb", engine)
    assert got == {"a": 600, "b": 601}


@gpu
def test_set_overflow_document(engine):
    # 600 distinct tokens, each twice, in one document: more than the
    # per-wave set holds, so the tail goes through the global fallback
    big = ["t{}".format(i) for i in range(600)]
    lines = ["x t1 t2", "y t599", " ".join(big + big[::-1]), "t0 z",
             "t300 t300 x"]
    got = _check("\n".join(lines) + "\n", engine)
    assert len(big) > DOC_SET
    assert got["t1"] == 2 and got["t599"] == 2 and got["t300"] == 2
    assert got["t17"] == 1 and got["x"] == 2
