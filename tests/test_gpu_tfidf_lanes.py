"""tfidf_docs_kernel with several text bytes per lane: every lane phase,
dense token ends, many docs per lane, window/stage edges, long tokens and
random text against the exact CPU oracle, plus the tokmix join identity
the cross-lane stitch rests on (CPU-only)."""
import random

import numpy as np
import pytest
import torch

from dampr_amd import keyhash

HAVE_GPU = torch.cuda.is_available()


def gpu(fn):
    fn = pytest.mark.skipif(not HAVE_GPU, reason="needs an MI355X")(fn)
    return pytest.mark.gpu(fn)


DEV = torch.device("cuda:0") if HAVE_GPU else None
LANE = 8            # widest lane word the kernel is built with
STAGE = 2048        # staged segment bytes (+16 tail bytes)
_MASK = (1 << 64) - 1


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


def _check(data, engine):
    """dfs AND materialised token strings equal the oracle's."""
    from dampr_amd.gpu.corpus import oracle_df
    arr = _arr(data)
    got = _dfs(arr, engine)
    want = oracle_df(arr)
    assert got == want
    return got


# ------------------------------------------------------------ CPU-only


def _rotl(x, r):
    r &= 63
    return ((x << r) | (x >> (64 - r))) & _MASK if r else x


def _pre(data):
    """tokmix before the length finaliser."""
    return keyhash.tokmix64(data) ^ keyhash.splitmix64(len(data))


def test_tokmix_join_identity():
    rnd = random.Random(7)
    alphabet = b"abcXYZ_019"
    for n in [1, 2, 7, 8, 9, 63, 64, 65, 130, 200]:
        data = bytes(rnd.choice(alphabet) for _ in range(n))
        whole = _pre(data)
        for cut in range(n + 1):
            a, b = data[:cut], data[cut:]
            assert whole == _pre(a) ^ _rotl(_pre(b), len(a)), (n, cut)
    # associativity of the (g, len) join over three parts
    data = bytes(rnd.choice(alphabet) for _ in range(150))
    for i, j in [(0, 0), (3, 70), (64, 128), (65, 65), (149, 150)]:
        a, b, c = data[:i], data[i:j], data[j:]
        bc = _pre(b) ^ _rotl(_pre(c), len(b))
        assert _pre(data) == _pre(a) ^ _rotl(bc, len(a))


def _random_text(seed, n=64 * 1024):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"abA_0 ,\n", dtype=np.uint8)
    p = np.full(8, (1.0 - 1.0 / 40) / 7)
    p[7] = 1.0 / 40
    return alphabet[rng.choice(8, size=n, p=p)].copy()


def test_oracle_handles_random_alphabet():
    # oracle_df splits on "\n" only and lowercases; an independent
    # byte-walk tokenizer must agree on the random-test alphabet.
    from dampr_amd.gpu.corpus import oracle_df
    arr = _random_text(0, 8192)
    want = {}
    for line in bytes(arr).split(b"\n"):
        toks, cur = set(), b""
        for c in line + b" ":
            ch = bytes([c]).lower()
            if ch.isalnum() or ch == b"_":
                cur += ch
            elif cur:
                toks.add(cur.decode())
                cur = b""
        for t in toks:
            want[t] = want.get(t, 0) + 1
    assert oracle_df(arr) == want


# ------------------------------------------------------------ GPU


@gpu
def test_lane_phase_by_length(engine):
    # every start offset 0..15 x token length 1..40; each line is padded
    # to a multiple of 16 bytes so the offset IS the lane phase.
    pads = " ,;-"
    lines = []
    for off in range(16):
        for ln in range(1, 41):
            letter = chr(ord("a") + off)          # a..p, shared token is q
            tok = "".join(letter.upper() if i & 1 else letter
                          for i in range(ln))
            line = "".join(pads[(off + i) % 4] for i in range(off))
            line += tok + " q"
            line += " " * (-(len(line) + 1) % 16)
            lines.append(line)
    text = "\n".join(lines) + "\n"
    assert all((len(l) + 1) % 16 == 0 for l in lines)
    got = _check(text, engine)
    assert got["q"] == len(lines) == 640
    assert len(got) == 641


@gpu
def test_dense_token_ends(engine):
    letters = "abcdefghijklmnopqrstuvwxyz"
    lines = []
    for shift in range(8):
        # "a b c d " : four token ends in every 8-byte lane
        body = " ".join(letters[(shift + i) % 26] for i in range(150))
        lines.append(" " * shift + body)
        # mixed separators, 1- and 2-byte tokens
        seps = [",", ";", " ", "-", ", "]
        body = "".join(letters[(3 * i + shift) % 26] * (1 + i % 2)
                       + seps[(i + shift) % 5] for i in range(120))
        lines.append("," * shift + body + "a,b;c d")
    _check("\n".join(lines) + "\n", engine)


@gpu
@pytest.mark.parametrize("text", [
    "a\nb\na\n" * 200,
    "\n\n\n",
    "\n\n\na\n\n\n\nb\n\n",
    "ab\nab\nab\n",
    "ab ab ab\n",
    "a\n\nb\n" * 33 + "a",
], ids=["one_byte_docs", "empty_lines", "empty_around", "ab_x3_docs",
        "ab_x3_one_doc", "mixed_tail"])
def test_many_docs_per_lane(engine, text):
    got = _check(text, engine)
    if text == "ab\nab\nab\n":
        assert got == {"ab": 3}       # docs inside one lane salt apart
    if text == "ab ab ab\n":
        assert got == {"ab": 1}


def _edge_positions():
    # last byte of a lane, of a 4-byte-lane window, of an 8-byte-lane
    # window, of the staged 2048 bytes and of the stage incl. its tail
    return [LANE - 1, 64 * 4 - 1, 64 * LANE - 1, STAGE - 1, STAGE + 15]


def _line_with_ends(ends, length, live_tail):
    """A line of `length` bytes: 3-letter tokens ending exactly at each
    position in `ends`; with live_tail the line's last bytes are a token
    (so a doc ends with a live token)."""
    buf = bytearray(b" " * length)
    for k, p in enumerate(ends):
        if p < length:
            buf[p - 2:p + 1] = "e{}x".format(k % 10).encode()
    if live_tail:
        buf[length - 3:length] = b"end"
    return bytes(buf).decode()


@gpu
def test_tokens_end_on_lane_window_stage_edges(engine):
    ends = _edge_positions()
    # first doc starts at byte 0, so line offsets are stage offsets
    lines = [_line_with_ends(ends, STAGE + 100, False), "e0x e1x tail"]
    _check("\n".join(lines) + "\n", engine)
    # tokens CROSSING each edge by two bytes
    lines = [_line_with_ends([p + 2 for p in ends], STAGE + 100, False),
             "e3x q"]
    _check("\n".join(lines) + "\n", engine)


@gpu
@pytest.mark.parametrize("edge", _edge_positions())
def test_doc_ends_on_edge_with_live_token(engine, edge):
    # newline sits right after the edge byte; the token is live there
    lines = [_line_with_ends([], edge + 1, True), "end zz q",
             _line_with_ends([], edge + 1, True)]
    got = _check("\n".join(lines) + "\n", engine)
    assert got["end"] == 3


@gpu
@pytest.mark.parametrize("rem", [1, 7, 8, 9, 15])
def test_corpus_tail_without_newline(engine, rem):
    base = "alpha beta\ngamma delta_9 Alpha\n" * 40
    n = len(base) - 40
    while n % 16 != rem or not base[n - 1].isalnum():
        n += 1
    text = base[:n]
    assert len(text) % 16 == rem and not text.endswith("\n")
    _check(text, engine)


@gpu
def test_long_tokens(engine):
    # cross the rotation wrap (64), the dict length cap (255), a window
    # and a stage; each in two docs, mixed case, odd alignment.
    from dampr_amd.gpu.corpus import oracle_df
    lens = [63, 64, 65, 255, 256, 300, 600, 2500]
    toks = []
    for i, ln in enumerate(lens):
        a, b = chr(ord("a") + i), chr(ord("A") + i + 8)
        toks.append("".join(a if k % 3 else b for k in range(ln)))
    lines = ["x " + " ".join(toks), "pad,pad"]
    lines += ["-" * (i + 1) + t + " y" for i, t in enumerate(toks)]
    arr = _arr("\n".join(lines) + "\n")
    got = _dfs(arr, engine)
    # the string dictionary stores at most 255 bytes of a token
    want = {t[:255]: df for t, df in oracle_df(arr).items()}
    assert got == want
    for t in toks:
        assert got[t.lower()[:255]] == 2


@gpu
def test_keys_are_tokmix(engine):
    from dampr_amd.gpu.corpus import oracle_df
    text = ("Hello, WORLD! hello_world 123 foo-bar\n\n a b c d e f g h\n"
            + "z" * 70 + " tabs\tand spaces\nlast line no newline")
    arr = _arr(text)
    engine.reset()
    engine.count_chunk(torch.from_numpy(arr).to(DEV))
    keys, df = engine.extract()
    got = {int(k) & _MASK: int(v)
           for k, v in zip(keys.cpu().tolist(), df.cpu().tolist())}
    want = {(keyhash.tokmix64(t.encode()) or 1): d
            for t, d in oracle_df(arr).items()}
    assert got == want


@pytest.fixture(scope="module")
def random_runs(engine):
    """(text, single-chunk dfs) per seed, computed once and shared."""
    out = []
    for seed in range(5):
        arr = _random_text(seed)
        out.append((arr, _dfs(arr, engine)))
    return out


@gpu
def test_random_text_vs_oracle(random_runs):
    from dampr_amd.gpu.corpus import oracle_df
    for arr, got in random_runs:
        assert got == oracle_df(arr)


@gpu
def test_random_text_multi_chunk(engine, random_runs):
    for arr, one in random_runs:
        assert _dfs(arr, engine, chunk_bytes=10_007) == one
