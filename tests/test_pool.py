"""The tiered run storage (gpu/pool.py) on CPU, where spills are
synchronous: a run's metadata is fixed at construction and the same on
every tier, ``HbmPool.columns`` hands out references that outlive an
eviction, ``HbmPool.free`` leaves nothing behind on any tier, and the
pool's byte counters always equal the sums over the runs it tracks."""
import os

import pytest
import torch

from dampr_amd.gpu.pool import DeviceRun, HbmPool
from dampr_amd.gpu.strvals import StrVals

CPU = torch.device("cpu")
N = 64
KINDS = ("i64", "f64", "sv")


def _make(kind, i=0):
    """A 64-row run; ``i`` (one digit) varies the contents, not the size."""
    keys = torch.arange(N, dtype=torch.int64) * 3 + i
    if kind == "i64":
        vals = keys * 7 - 11
    elif kind == "f64":
        vals = keys.to(torch.float64) / 3 - 0.5
    else:
        # mixed lengths, multi-byte characters, empty strings
        vals = StrVals.from_strings(
            ["" if j % 5 == 0 else "é" * (j % 3) + "w" * (j % 7) + str(i)
             for j in range(N)])
    return DeviceRun(keys, vals, sorted=True)


def _copy(run):
    """Independent copies of a resident run's columns."""
    return run.keys.clone(), run.vals.clone()


def _same(got, want):
    gk, gv = got
    wk, wv = want
    if isinstance(wv, StrVals):
        return torch.equal(gk, wk) and torch.equal(gv.blob, wv.blob) \
            and torch.equal(gv.offs, wv.offs)
    return torch.equal(gk, wk) and gv.dtype == wv.dtype \
        and torch.equal(gv.view(torch.int64), wv.view(torch.int64))


def _meta(run):
    return run.n, run.nbytes, run.vdtype, run.has_sv


def _expected_meta(kind, run):
    if kind == "sv":
        return N, N * 8 + run.vals.blob.numel() + (N + 1) * 8, None, True
    return (N, N * 8 + N * 8,
            torch.int64 if kind == "i64" else torch.float64, False)


def _check_accounting(pool, live):
    resident = [r for r in live if r.resident]
    host = [r for r in live if not r.resident and not r.on_disk]
    assert pool.used == sum(r.nbytes for r in resident)
    assert pool.host_used == sum(r.nbytes for r in host)
    assert pool.clean_bytes == 0           # no writeback without a stream


@pytest.mark.parametrize("kind", KINDS)
def test_metadata_fixed_across_tiers(kind, tmp_path):
    run, filler = _make(kind, 1), _make(kind, 2)
    want = _expected_meta(kind, run)
    orig = _copy(run)
    assert _meta(run) == want                          # at construction
    pool = HbmPool(run.nbytes, spill_dir=str(tmp_path))
    pool.admit(run)
    pool.admit(filler)                                 # evicts ``run``
    assert not run.resident and not run.on_disk
    assert _meta(run) == want                          # on the host tier
    pool.host_capacity = run.nbytes - 1                # below one run
    pool.balance()
    spill_file, = os.listdir(str(tmp_path))
    assert run.on_disk
    assert _meta(run) == want                          # on disk
    got = pool.columns(run, CPU)           # ``filler`` takes its place
    assert run.resident and not run.on_disk
    assert spill_file not in os.listdir(str(tmp_path))
    assert _meta(run) == want                          # reloaded
    assert _same(got, orig)
    pool.free(run)
    assert _meta(run) == want                          # and after drop()
    pool.free(filler)
    pool.cleanup()


@pytest.mark.parametrize("kind", KINDS)
def test_columns_references_survive_eviction(kind):
    a, b = _make(kind, 1), _make(kind, 2)
    orig_a, orig_b = _copy(a), _copy(b)
    pool = HbmPool(a.nbytes)                           # room for one run
    pool.admit(a)
    pool.admit(b)
    cols_a = pool.columns(a, CPU)
    assert a.resident and not b.resident
    cols_b = pool.columns(b, CPU)                      # evicts ``a``
    assert not a.resident and a.keys is None and a.vals is None
    assert _same(cols_a, orig_a)
    assert _same(cols_b, orig_b)
    assert _same(pool.columns(a, CPU), orig_a)


def test_free_leaves_nothing_behind(tmp_path):
    runs = [_make(kind, i) for i, kind in enumerate(KINDS)]
    metas = [_meta(r) for r in runs]
    cap = max(r.nbytes for r in runs)
    pool = HbmPool(cap, host_capacity=cap, spill_dir=str(tmp_path))
    for r in runs:
        pool.admit(r)
    disk, host, resident = runs
    assert disk.on_disk and not disk.resident
    assert not host.resident and not host.on_disk
    assert resident.resident
    assert len(os.listdir(str(tmp_path))) == 1
    _check_accounting(pool, runs)
    for r in (host, disk, resident):
        pool.free(r)
        assert not r.resident and not r.on_disk
    assert pool.used == pool.host_used == pool.clean_bytes == 0
    assert os.listdir(str(tmp_path)) == []
    assert [_meta(r) for r in runs] == metas
    pool.free(disk)                        # freeing a freed run is a no-op
    assert pool.used == pool.host_used == pool.clean_bytes == 0
    pool.cleanup()
    assert os.listdir(str(tmp_path)) == []


def test_accounting_matches_tracked_runs(tmp_path):
    runs = [_make(KINDS[i % 3], i) for i in range(8)]
    origs = [_copy(r) for r in runs]
    cap = 2 * max(r.nbytes for r in runs)              # holds two runs
    pool = HbmPool(cap, host_capacity=cap, spill_dir=str(tmp_path))
    live = []

    def admit(i):
        pool.admit(runs[i])
        live.append(runs[i])

    def read(i):
        assert _same(pool.columns(runs[i], CPU), origs[i])

    def free(i):
        pool.free(runs[i])
        live.remove(runs[i])

    steps = [(admit, 0), (admit, 1), (admit, 2), (admit, 3), (read, 0),
             (free, 1), (admit, 4), (admit, 5), (read, 2), (read, 0),
             (free, 3), (admit, 6), (admit, 7), (read, 4), (free, 0),
             (read, 5), (read, 2), (read, 6), (read, 7), (read, 4)]
    for op, i in steps:
        op(i)
        _check_accounting(pool, live)
        assert pool.used <= cap + max(r.nbytes for r in runs)
    assert any(r.on_disk for r in live)
    assert any(not r.resident and not r.on_disk for r in live)
    for r in list(live):
        free(runs.index(r))
        _check_accounting(pool, live)
    assert pool.used == pool.host_used == 0
    assert os.listdir(str(tmp_path)) == []
