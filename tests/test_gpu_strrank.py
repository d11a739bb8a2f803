"""GPU-side tests of the device lexicographic rank for string keys: the
sv_lex_key kernel bit for bit against keyhash.lex_window_key,
HipOps.str_rank exactly equal to the TorchOps oracle, and string-key
pipelines on cuda:0 whose dictionary stays a device-side StrTable until
keys are read.  Every shape is valid input."""
import collections

import numpy as np
import pytest
import torch

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif("not __import__('torch').cuda.is_available()",
                       reason="needs an MI355X"),
]

from dampr_amd import Dampr, funcs, keyhash, settings  # noqa: E402
from dampr_amd.gpu.stores import StrTable  # noqa: E402
from dampr_amd.gpu.strvals import StrVals  # noqa: E402

DEV = "cuda:0"
_U64 = (1 << 64) - 1


# -- sv_lex_key ----------------------------------------------------------------

_LENS = [0, 1, 6, 7, 8, 9, 13, 14, 15, 63, 64, 65, 513]
_WINDOWS = (0, 1, 2, 9, 73, 74)     # 73: last window of 513 bytes; 74: past


def _arena_rows():
    """Rows (bytes) of one arena: every length of _LENS starting at every
    byte alignment 0..7 (filler rows shift the running offset), empty
    rows first and last, random bytes with NULs, a couple of thousand
    short rows, and a last non-empty row of 513 bytes at an odd alignment
    that ends exactly at the end of the blob."""
    rng = np.random.default_rng(61)

    def rand(n):
        # a quarter of the bytes are NUL
        b = rng.integers(0, 256, size=n, dtype=np.uint8)
        b[rng.integers(0, 4, size=n) == 0] = 0
        return b.tobytes()

    rows = [b""]
    pos = 0
    placed = set()
    for ln in _LENS:
        for align in range(8):
            pad = (align - pos) % 8
            if pad:
                rows.append(rand(pad))
                pos += pad
            assert pos % 8 == align
            placed.add((ln, align))
            rows.append(rand(ln))
            pos += ln
    assert len(placed) == len(_LENS) * 8
    for _ in range(2000):
        rows.append(rand(int(rng.integers(0, 24))))
    pos = sum(len(r) for r in rows)
    if pos % 8 != 3:                    # odd alignment for the final row
        rows.append(rand((3 - pos) % 8))
    rows.append(rand(513))
    rows.append(b"")
    return rows


def _arena(rows, lead=0):
    """(blob, offs) on the device; ``lead`` > 0 makes the blob a view
    that starts ``lead`` bytes into its allocation (unaligned base)."""
    lens = np.fromiter((len(r) for r in rows), dtype=np.int64,
                       count=len(rows))
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    raw = np.frombuffer(b"\xff" * lead + b"".join(rows), dtype=np.uint8)
    blob = torch.from_numpy(raw.copy()).to(DEV)[lead:]
    assert blob.is_contiguous() and blob.numel() == int(offs[-1])
    return blob, torch.from_numpy(offs).to(DEV)


@pytest.fixture(scope="module")
def arena():
    rows = _arena_rows()
    assert rows[0] == b"" and rows[-1] == b"" and len(rows[-2]) == 513
    # a shuffled subset of the row indices, its length no multiple of 64,
    # that keeps the first row, the last row and the 513-byte tail row
    n = len(rows)
    pick = np.random.default_rng(62).permutation(n)[:n - 7]
    keep = np.array([0, n - 2, n - 1])
    pick = np.concatenate([pick[~np.isin(pick, keep)], keep])
    np.random.default_rng(63).shuffle(pick)
    assert len(pick) % 64 != 0 and len(pick) > 2000
    want = {d: [keyhash.lex_window_key(rows[i], d) for i in pick]
            for d in _WINDOWS}
    return rows, pick.astype(np.int32), want


@pytest.mark.parametrize("lead", [0, 5])
def test_sv_lex_key_bit_exact(arena, lead):
    from dampr_amd.ops import native
    ext = native.require()
    rows, pick, want = arena
    blob, offs = _arena(rows, lead)
    assert int(offs[-1]) == blob.numel()
    sel = torch.from_numpy(pick).to(DEV)
    for d in _WINDOWS:
        out = torch.empty(len(pick), dtype=torch.int64, device=DEV)
        ext.sv_lex_key(blob, offs, sel, d, out)
        got = [k & _U64 for k in out.cpu().tolist()]
        bad = [j for j, (g, w) in enumerate(zip(got, want[d])) if g != w]
        assert not bad, (d, len(bad), bad[:5],
                         [len(rows[pick[j]]) for j in bad[:5]])
    assert not any(want[74])
    assert any(want[73])


def test_sv_lex_refine_flags():
    from dampr_amd.ops import native
    # (grp, key) sorted; key low byte 8 = the row continues
    grp = [0, 0, 0, 0, 0, 5, 5, 5, 9]
    key = [0x107, 0x108, 0x108, 0x208, 0x303, 0x108, 0x303, 0x303, 0x108]
    hd = torch.empty(len(grp), dtype=torch.uint8, device=DEV)
    op = torch.empty(len(grp), dtype=torch.uint8, device=DEV)
    native.require().sv_lex_refine(
        torch.tensor(grp, dtype=torch.int64, device=DEV),
        torch.tensor(key, dtype=torch.int64, device=DEV), hd, op)
    assert hd.cpu().tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 1]
    assert op.cpu().tolist() == [0, 1, 1, 0, 0, 0, 0, 0, 0]


# -- HipOps.str_rank -------------------------------------------------------------

def _words(n, seed):
    """n distinct lowercase words, 3-12 letters."""
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        need = n - len(out)
        lens = rng.integers(3, 13, size=need)
        letters = rng.integers(97, 123, size=int(lens.sum()),
                               dtype=np.uint8).tobytes()
        pos = 0
        for ln in lens:
            out.add(letters[pos:pos + ln])
            pos += ln
    out = sorted(out)
    np.random.default_rng(seed + 1).shuffle(out)
    return out


def _small(n):
    rng = np.random.default_rng(n)
    return [b"t%d" % int(i) for i in rng.integers(0, 9, size=n)]


def _first_diff_pairs():
    base = b"0123456789abcdefghij"
    rows = []
    for at in (6, 7, 8, 13, 14):
        for tail in (b"", b"x", b"tail"):
            rows.append(base[:at] + b"A" + tail)
            rows.append(base[:at] + b"B" + tail)
    return rows


def _rand4(n, seed):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"\0ab\xfe", dtype=np.uint8)
    return [alphabet[rng.integers(0, 4, size=int(ln))].tobytes()
            for ln in rng.integers(0, 24, size=n)]


_P64 = b"p" * 64
_RANK_INPUTS = {
    "n0": [],
    "n1": [b"solo"],
    "n2_equal": [b"twin", b"twin"],
    "n63": _small(63),
    "n64": _small(64),
    "n65": _small(65),
    "n257": _small(257),
    "all_equal": [b"same word"] * 300,
    "distinct_1000": [b"d%d" % i for i in range(1000)],
    "trailing_nuls": [s for i in range(100)
                      for s in (b"nul%d" % i, b"nul%d\0" % i,
                                b"nul%d\0\0" % i)]
    + [b"ab", b"ab\0", b"ab\0\0", b"", b"\0"],
    "first_diff": _first_diff_pairs(),
    "long_shared_prefix": [_P64 + s for i in range(100)
                           for s in (b"%d" % i, b"%dy" % i, b"z")] * 2,
    "last_byte_513": [b"L" * 512 + bytes([i]) for i in (7, 0, 255, 128, 65)],
    "high_bytes": [bytes(r) for r in np.random.default_rng(64).choice(
        np.array([0x41, 0x7a, 0x80, 0xc3, 0xff, 0x00], dtype=np.uint8),
        size=(500, 9))] + [b"\x80", b"\x7f", b"\xff", b"A"],
    "rand4_3000": _rand4(3000, 65),
    "words_100k": _words(100_000, 66),
}
_DISTINCT = ("n1", "distinct_1000", "trailing_nuls", "first_diff",
             "last_byte_513", "words_100k")


def _sv(rows):
    lens = np.fromiter((len(r) for r in rows), dtype=np.int64,
                       count=len(rows))
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    blob = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    return StrVals(torch.from_numpy(blob), torch.from_numpy(offs))


@pytest.mark.parametrize("name", sorted(_RANK_INPUTS))
def test_hipops_str_rank(name):
    from dampr_amd.gpu.backend import HipOps, TorchOps
    rows = _RANK_INPUTS[name]
    sv = _sv(rows)
    ops = HipOps()
    rank = ops.str_rank(sv.to(DEV))
    assert rank.device.type == "cuda" and rank.dtype == torch.int64
    assert rank.shape == (len(rows),)
    want = TorchOps().str_rank(sv)
    assert torch.equal(rank.cpu(), want)
    if name in _DISTINCT:
        assert len(set(rows)) == len(rows)
        assert sorted(rank.cpu().tolist()) == list(range(len(rows)))
    if rows:
        assert 1 <= ops.str_rank_rounds <= max(map(len, rows)) // 7 + 1


def test_hipops_str_rank_row_count_overflow():
    from dampr_amd.gpu.backend import HipOps

    class Huge(object):
        """Stands for a column of 2**31 rows; only its row count is
        read before the refusal."""
        blob = torch.zeros(0, dtype=torch.uint8, device=DEV)

        def numel(self):
            return 1 << 31

    with pytest.raises(OverflowError):
        HipOps().str_rank(Huge())


# -- engine -----------------------------------------------------------------------

@pytest.fixture
def no_host_map(monkeypatch):
    from dampr_amd.gpu.engine import GpuRunner
    calls = []
    orig = GpuRunner._host_map

    def counting(self, stage, ins):
        calls.append(repr(stage))
        return orig(self, stage, ins)

    monkeypatch.setattr(GpuRunner, "_host_map", counting)
    yield calls
    assert calls == []


def zipf_words(n, vocab, seed):
    rng = np.random.default_rng(seed)
    return ["w{}".format(int(z) % vocab) for z in rng.zipf(1.3, size=n)]


def _run(pm, name, **kw):
    from dampr_amd.gpu.engine import GpuRunner
    pm = pm.checkpoint()
    runner = GpuRunner(name, pm.pmer.graph, device=DEV, **kw)
    return runner, runner.run([pm.source])[0]


def test_engine_sort_by_lazy_table(no_host_map):
    words = zipf_words(20_000, 3000, 70) + \
        ["", "é", "zz", "Zz", "日本", "a\0b"]
    runner, out = _run(Dampr.columns(words).sort_by(), "strrank_sort")
    assert isinstance(out.str_table, StrTable)
    assert out.str_table.materialized is False
    assert runner.stats["str_rank_rows"] == len(set(words))
    assert runner.stats["str_rank_rounds"] >= 1
    assert [v for _k, v in out.read()] == sorted(words)
    assert out.str_table.materialized is True


def test_engine_multi_batch(no_host_map):
    rng = np.random.default_rng(71)
    words = ["k{}".format(int(i)) for i in rng.integers(0, 12, size=101)]
    old = settings.gpu_batch_records
    settings.gpu_batch_records = 7
    try:
        runner, out = _run(Dampr.columns(words).count(), "strrank_batches",
                           n_partitions=4)
        got = {k: v[1] for k, v in out.read()}
    finally:
        settings.gpu_batch_records = old
    assert got == dict(collections.Counter(words))
    assert runner.stats["str_rank_rows"] == len(set(words))
    assert runner.stats["dict_encode_host_batches"] == 0


def test_engine_cross_vocabulary_join(no_host_map):
    left = zipf_words(5000, 80, 72)
    right = ["w{}".format(i) for i in range(40, 120)] * 2 + ["only_right"]
    out = Dampr.columns(left).count() \
        .join(Dampr.columns(right).count()) \
        .reduce(funcs.pair_sum, many=True).run(device=DEV)
    cl, cr = collections.Counter(left), collections.Counter(right)
    want = sorted((w, (w, cl[w], w, cr[w])) for w in cl if w in cr)
    assert want
    assert sorted(out.read()) == want


def test_engine_forced_collisions(no_host_map):
    words = zipf_words(1000, 50, 73)
    old = settings.str_hash_mask
    settings.str_hash_mask = 0x3
    try:
        runner, out = _run(Dampr.columns(words).count(), "strrank_coll")
        got = {k: v[1] for k, v in out.read()}
    finally:
        settings.str_hash_mask = old
    assert got == dict(collections.Counter(words))
    assert runner.stats["dict_encode_host_batches"] > 0
    assert runner.stats["str_rank_rows"] == len(set(words))
