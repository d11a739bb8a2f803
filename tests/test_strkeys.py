"""Keying by a string VALUE column (count / a_group_by / sort_by over
words) through the device engine's dictionary encode, on the CPU with the
TorchOps oracle backend: the strmix64 hash pins, the ``dict_encode``
contract, and whole pipelines that must never take the host map path."""
import collections

import numpy as np
import pytest
import torch

from dampr_amd import Dampr, funcs, keyhash, settings
from dampr_amd.gpu.backend import TorchOps
from dampr_amd.gpu.engine import GpuRunner
from dampr_amd.gpu.strvals import StrVals


# -- hash ------------------------------------------------------------------

def test_strmix64_pins():
    assert keyhash.strmix64(b"") == 0xe220a8397b1dcdaf
    assert keyhash.strmix64(b"a") == 0x2a4e8e0ec28bd6b5
    assert keyhash.strmix64(b"hello, world") == 0xfddf4f8349e88a81


def test_strmix64_trailing_nuls_differ():
    hs = {keyhash.strmix64(b) for b in (b"a", b"a\0", b"a\0\0")}
    assert len(hs) == 3


# -- TorchOps.dict_encode contract -------------------------------------------

def check_contract(ids, uniq, rows):
    """ids dense in [0, U), uniq distinct, uniq[ids[i]] == rows[i]."""
    ul = uniq.tolist()
    il = ids.cpu().tolist()
    assert ids.dtype == torch.int64
    assert len(il) == len(rows)
    assert len(ul) == len(set(ul)) == len(set(rows))
    assert all(0 <= i < len(ul) for i in il)
    assert [ul[i] for i in il] == list(rows)


_CONTRACT_INPUTS = {
    "n0": [],
    "n1": ["solo"],
    "all_equal": ["same"] * 37,
    "all_distinct": ["w{}".format(i) for i in range(300)],
    "empty_string": ["", "a", "", "b", ""],
    "utf8": ["naïve", "日本語", "naive", "日本", "日本語", "ü", "u"],
    "trailing_nuls": ["a", "a\0", "a\0\0", "a", "a\0", "\0", ""],
}


@pytest.mark.parametrize("name", sorted(_CONTRACT_INPUTS))
def test_torchops_dict_encode_contract(name):
    rows = _CONTRACT_INPUTS[name]
    ids, uniq = TorchOps().dict_encode(StrVals.from_strings(rows))
    check_contract(ids, uniq, rows)


# -- engine ------------------------------------------------------------------

@pytest.fixture
def no_host_map(monkeypatch):
    """Counts GpuRunner._host_map calls; the test asserts on exit that
    the string-key pipelines never took it."""
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


def test_count_zipf(no_host_map):
    words = zipf_words(20000, 3000, 0)
    got = dict(Dampr.columns(words).count().run(runner=GpuRunner).read())
    assert got == dict(collections.Counter(words))


def test_group_first(no_host_map):
    words = zipf_words(2000, 200, 1)
    res = Dampr.columns(words).a_group_by().first().run(runner=GpuRunner)
    got = sorted(res.read())
    assert [k for k, _v in got] == sorted(set(words))
    assert all(v == k for k, v in got)


def test_sort_by(no_host_map):
    words = zipf_words(3000, 500, 2) + ["", "é", "zz", "Zz", "日本"]
    got = list(Dampr.columns(words).sort_by().run(runner=GpuRunner).read())
    assert got == sorted(words)


def test_cross_vocabulary_join(no_host_map):
    """Two counts over different vocabularies join on the word: their
    dictionaries differ, so the join remaps through the union table
    (_unify_str_stores)."""
    left = zipf_words(1500, 80, 3)
    right = ["w{}".format(i) for i in range(40, 120)] * 2 + ["only_right"]
    out = Dampr.columns(left).count() \
        .join(Dampr.columns(right).count()) \
        .reduce(funcs.pair_sum, many=True).run(runner=GpuRunner)
    cl, cr = collections.Counter(left), collections.Counter(right)
    # a count's records are (word, n) values under the word as key, and
    # pair_sum adds the two sides' values: tuple concatenation, as on the
    # host engine
    want = sorted((w, (w, cl[w], w, cr[w])) for w in cl if w in cr)
    assert want
    assert sorted(out.read()) == want


def test_multi_batch_and_stats(no_host_map):
    """Words recur across 7-row batches: provisional ids dedupe across
    batches, and the runner reports what it encoded."""
    rng = np.random.default_rng(4)
    words = ["k{}".format(int(i)) for i in rng.integers(0, 12, size=101)]
    old = settings.gpu_batch_records
    settings.gpu_batch_records = 7
    try:
        pm = Dampr.columns(words).count().checkpoint()
        runner = GpuRunner("strkeys", pm.pmer.graph, n_partitions=4)
        out = runner.run([pm.source])[0]
        # raw reducer output: keyed convention (k, (k, v))
        got = {k: v[1] for k, v in out.read()}
    finally:
        settings.gpu_batch_records = old
    assert got == dict(collections.Counter(words))
    assert runner.stats["dict_encode_rows"] == len(words)
    assert runner.stats["dict_encode_host_batches"] == 0


def test_tiny_pool_spills(no_host_map, tmp_path):
    words = zipf_words(4000, 300, 5)
    old = settings.gpu_batch_records
    settings.gpu_batch_records = 512
    try:
        pm = Dampr.columns(words).sort_by().checkpoint()
        runner = GpuRunner("strkeys_pool", pm.pmer.graph, n_partitions=4,
                           hbm_bytes=8192, host_bytes=8192,
                           spill_dir=str(tmp_path))
        out = runner.run([pm.source])[0]
        got = list(out.read())
    finally:
        settings.gpu_batch_records = old
    assert [v for _k, v in got] == sorted(words)
    assert runner.stats["spilled_to_host_bytes"] > 0
    assert runner.stats["dict_encode_rows"] == len(words)


def test_empty_input_matches_host_path():
    got = list(Dampr.columns(np.array([], dtype="U1")).count()
               .run(runner=GpuRunner).read())
    assert got == []
