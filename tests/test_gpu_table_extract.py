"""table_extract compacts a table's live slots tile by tile with one
cursor add per tile: capacities around the 64-slot strip and the
4,096-slot tile, live fractions from none to all, the cursor's final
value, and an output shorter than the live count."""
import numpy as np
import pytest
import torch

HAVE_GPU = torch.cuda.is_available()


def gpu(fn):
    fn = pytest.mark.skipif(not HAVE_GPU, reason="needs an MI355X")(fn)
    return pytest.mark.gpu(fn)


DEV = torch.device("cuda:0") if HAVE_GPU else None
CAPS = [1, 63, 64, 65, 4095, 4096, 4097, 1 << 16]
FRACTIONS = ["none", "first", "last", "5%", "all"]


@pytest.fixture(scope="module")
def ext():
    from dampr_amd.ops import native
    return native.require()


def _table(cap, fraction, seed):
    """(keys, vals) i64 host arrays: distinct non-zero keys (sign bit
    included) in the live slots, positive values everywhere live."""
    rng = np.random.default_rng(seed)
    live = {"none": np.zeros(cap, bool),
            "first": np.arange(cap) == 0,
            "last": np.arange(cap) == cap - 1,
            "5%": rng.random(cap) < 0.05,
            "all": np.ones(cap, bool)}[fraction]
    pool = rng.permutation(2 * cap)[:cap].astype(np.int64) + 1
    pool[::2] *= -1                          # u64 keys with the top bit set
    keys = np.where(live, pool, 0).astype(np.int64)
    vals = np.where(live, rng.integers(1, 1 << 40, cap), 0).astype(np.int64)
    return keys, vals


def _pairs(keys, vals):
    k = torch.as_tensor(keys).cpu()
    v = torch.as_tensor(vals).cpu()
    order = torch.argsort(k)
    return k[order].tolist(), v[order].tolist()


@gpu
@pytest.mark.parametrize("cap", CAPS)
def test_extract_equals_nonzero(ext, cap):
    for i, fraction in enumerate(FRACTIONS):
        keys, vals = _table(cap, fraction, seed=cap + i)
        tk = torch.from_numpy(keys).to(DEV)
        tv = torch.from_numpy(vals).to(DEV)
        idx = torch.nonzero(tk).flatten()
        n_live = idx.numel()
        out_k, out_v, cursor = ext.table_extract(tk, tv, n_live)
        assert out_k.numel() == n_live and out_v.numel() == n_live
        assert int(cursor[0].item()) == n_live, (cap, fraction)
        assert _pairs(out_k, out_v) == _pairs(tk[idx], tv[idx]), \
            (cap, fraction)


@gpu
@pytest.mark.parametrize("cap", CAPS)
def test_short_output_is_filled_and_not_overrun(ext, cap):
    for i, fraction in enumerate(["5%", "all"]):
        keys, vals = _table(cap, fraction, seed=3 * cap + i)
        tk = torch.from_numpy(keys).to(DEV)
        tv = torch.from_numpy(vals).to(DEV)
        want = dict(zip(keys[keys != 0].tolist(), vals[keys != 0].tolist()))
        n_live = len(want)
        for n_out in sorted({0, n_live // 2, max(n_live - 1, 0)}):
            out_k, out_v, cursor = ext.table_extract(tk, tv, n_out)
            torch.cuda.synchronize()         # the call completes
            assert out_k.numel() == n_out and out_v.numel() == n_out
            assert int(cursor[0].item()) == n_live
            got_k, got_v = out_k.cpu().tolist(), out_v.cpu().tolist()
            # exactly n_out rows, each a live slot, none twice
            assert len(set(got_k)) == n_out
            assert all(want[k] == v for k, v in zip(got_k, got_v))
