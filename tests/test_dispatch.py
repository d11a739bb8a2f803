"""Structure of the device engine's stage dispatch and of the shared text
chunking helper (CPU only; the lowerings themselves are covered by
test_engine.py and the GPU suites)."""
import pytest
import torch

from dampr_amd.gpu.engine import GpuRunner, PartStore
from dampr_amd.gpu.tfidf import chunk_bounds
from dampr_amd.runner import GMap, GReduce, Graph, Source

# every kind dampr.py can emit
MAP_KINDS = ["kv", "identity", "unkey", "len_local", "text_df", "cross",
             "cross_set", "topk_local"]
REDUCE_KINDS = ["sum", "min", "max", "mean", "first", "topk_global", "join"]


@pytest.mark.parametrize("kind", MAP_KINDS)
def test_map_table_has_handler(kind):
    assert callable(GpuRunner._MAP_HANDLERS[kind])


@pytest.mark.parametrize("kind", REDUCE_KINDS)
def test_reduce_table_has_handler(kind):
    assert callable(GpuRunner._REDUCE_HANDLERS[kind])


def test_unknown_kinds_raise():
    runner = GpuRunner("dispatch-test", Graph(), device="cpu")
    out = Source("out")
    with pytest.raises(ValueError, match="unknown device_map spec"):
        runner.run_map(
            GMap(out, [], None, options={"device_map": ("no_such_map",)}),
            [PartStore()])
    with pytest.raises(ValueError, match="unknown device_reduce spec"):
        runner.run_reduce(
            GReduce(out, [], None,
                    options={"device_reduce": ("no_such_reduce",)}),
            [PartStore()])
    runner.pool.cleanup()


def _u8(data):
    return torch.tensor(list(data), dtype=torch.uint8)


# Expected bounds follow the chunking rule by hand: the tentative end is
# min(prev + chunk_bytes, n); below n it moves to just after the first
# newline in text[end-1 : end+65536], or to n when there is none.
@pytest.mark.parametrize("data, chunk_bytes, want", [
    (b"", 4, [0]),                                   # empty text
    (b"ab\ncd\n", 6, [0, 6]),                        # chunk_bytes == n
    (b"ab\ncd\n", 100, [0, 6]),                      # chunk_bytes > n
    (b"ab\ncd\nef\n", 3, [0, 3, 6, 9]),              # end just after \n stays
    (b"abcd\nef\ngh", 2, [0, 5, 8, 10]),             # end falls mid-line
    (b"ab\ncdefgh", 2, [0, 3, 9]),                   # no later newline
])
def test_chunk_bounds(data, chunk_bytes, want):
    got = chunk_bounds(_u8(data), chunk_bytes)
    assert got == want
    assert got[0] == 0 and got[-1] == len(data)
    assert all(a < b for a, b in zip(got, got[1:]))
    assert all(data[b - 1:b] == b"\n" for b in got[1:-1])
