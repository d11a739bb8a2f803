"""Device set-membership filter at world > 1 (gloo, CPU): the filter stage
has no exchange of its own and building a set issues no collective, so a
rank whose rows all filter away must still walk the following stages'
collectives in step with the others."""
import collections
import multiprocessing
import os

import torch

from dampr_amd import Dampr, funcs, settings


def _columns():
    """Keys whose owning rank (partition % 2) is known, a distinct value
    per row, and the member set: the values of rank 1's rows, and
    strangers."""
    from dampr_amd.gpu.backend import TorchOps
    keys = torch.arange(400, dtype=torch.int64)
    owner = TorchOps().partition_of(keys, settings.gpu_partitions) % 2
    vals = keys * 3 - 100
    members = set(vals[owner == 1].tolist()) | {-5000, 2.5, "k", True}
    return keys.numpy(), vals.numpy(), owner.numpy(), members


def _filter_rank(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dampr_amd.gpu.engine import GpuRunner
        keys, vals, owner, members = _columns()
        pm = Dampr.columns(vals, keys=keys) \
            .filter(funcs.isin(members)).count()
        runner = GpuRunner("isin_dist", pm.pmer.graph, device="cpu")
        pairs = sorted(v for _k, v in runner.run([pm.source])[0].read())
        # this rank's ingest slice is the rows it owns
        mine = int((owner == rank).sum())
        assert runner.stats["filter_rows_in"] == mine
        assert runner.stats["filter_rows_kept"] == (0 if rank == 0 else mine)
        gathered = [None] * world
        dist.all_gather_object(gathered, pairs)
        merged = sorted(p for lst in gathered for p in lst)
        want = collections.Counter(
            v for v in vals.tolist() if v in members)
        assert merged == sorted(want.items()), merged[:5]
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:       # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


def test_isin_gloo_one_rank_filters_to_nothing():
    _k, vals, owner, members = _columns()
    assert (owner == 0).any() and (owner == 1).any()
    assert not any(v in members for v in vals[owner == 0].tolist())
    assert all(v in members for v in vals[owner == 1].tolist())
    world = 2
    port = 29000 + (os.getpid() + 570) % 900
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_filter_rank, args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    for rank, status in results:
        assert status == "ok", "rank {} failed:\n{}".format(rank, status)
