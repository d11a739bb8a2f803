#!/usr/bin/env python3
"""Flagship benchmark: TF-IDF over synthetic Zipf text (BASELINE.json
config 2), whole-node rows/sec.

One step = the complete TF-IDF job over this rank's resident corpus:
tokenize + hash + per-doc dedupe + df-count on device, the RCCL exchange of
(key, df, token-bytes) partials when world_size > 1, the idf epilogue, token
string materialization and the TSV sink.  Nothing is cached across steps
(tables are reset each step); data is synthetic (no network for datasets).

Run: python bench.py --gpus N --steps K --warmup W [--mb-per-gpu M]
                     [--dump-outputs DIR] [--full]
For N > 1 the driver launches via torch.distributed.run; ranks read
RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from the environment.

A plain run does only what the headline figure needs: set up, warm up,
time the steps, print the result line.  ``--dump-outputs DIR`` also
writes what the last timed step computed as DIR/<name>.npy (the corpus
is seeded, so two builds can be compared output for output).  ``--full``
adds the measurements that take runs of their own (the NVMe -> HBM
ingest probe).
"""
import argparse
import json
import os
import shutil
import tempfile
import time

import numpy as np
import torch

# --dump-outputs budget: 64 MB in all.  Row arrays are float64 (4 per
# row), the sink bytes float32 (4 B per byte).
DUMP_MAX_ROWS = 1 << 20          # 4 arrays x 8 B x 1M rows = 32 MiB
DUMP_MAX_SINK_BYTES = 6 << 20    # x 4 B = 24 MiB


def use_built_extension():
    """Run from a tree that was built elsewhere (another user's checkout,
    a read-only mount): the extension loader takes a lock file in its
    build directory on every start, which fails there although the
    library is complete.  If that directory is not writable (so nothing
    could be rebuilt in it anyway) and holds dampr_hip.so, hand that
    library to the loader as it is; anything else stays the loader's
    business (and its error)."""
    import importlib.machinery
    import importlib.util
    from dampr_amd.ops import native
    so = os.path.join(native.BUILD_DIR, "dampr_hip.so")
    if os.access(native.BUILD_DIR, os.W_OK) or not os.path.isfile(so):
        return
    spec = importlib.util.spec_from_file_location(
        "dampr_hip", so,
        loader=importlib.machinery.ExtensionFileLoader("dampr_hip", so))
    ext = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ext)
    native._EXT = ext


def dump_outputs(out_dir, suffix, keys, df, idf, sink_file):
    """Write the last timed step's outputs: the (key, df, idf) columns a
    caller of the pipeline receives and the TSV part file it sank.  u64
    keys are split into exact 32-bit halves; df (int64 < 2^53) and idf
    are exact in float64.  Outputs over the budget are cut to a fixed
    seeded row sample / byte prefix."""
    os.makedirs(out_dir, exist_ok=True)
    n = keys.numel()
    if n > DUMP_MAX_ROWS:
        rows = np.sort(np.random.default_rng(0).choice(
            n, DUMP_MAX_ROWS, replace=False))
        sel = torch.from_numpy(rows).to(keys.device)
        keys, df, idf = keys[sel], df[sel], idf[sel]
    k = keys.cpu().numpy().view(np.uint64)
    with open(sink_file, "rb") as fh:
        sink = np.frombuffer(fh.read(DUMP_MAX_SINK_BYTES), dtype=np.uint8)
    arrays = {
        "keys_hi": (k >> np.uint64(32)).astype(np.float64),
        "keys_lo": (k & np.uint64(0xFFFFFFFF)).astype(np.float64),
        "df": df.cpu().numpy().astype(np.float64),
        "idf": idf.cpu().numpy().astype(np.float64),
        "sink_tsv_bytes": sink.astype(np.float32),
    }
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, name + suffix + ".npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    # default = BASELINE.json config 2: "TF-IDF on 1 MI355X, 10 GB
    # synthetic text" (10240 MB per GPU; weak scaling adds 10 GB/rank)
    ap.add_argument("--mb-per-gpu", type=int,
                    default=int(os.environ.get("DAMPR_BENCH_MB", "10240")))
    ap.add_argument("--sink-dir", default=None,
                    help="where the TSV sink goes (default: a fresh "
                         "temporary directory, removed at the end)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as "
                         "DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline "
                         "figure (NVMe->HBM ingest probe)")
    ap.add_argument("--no-ingest-probe", action="store_true",
                    help="with --full: skip the NVMe->HBM ingest "
                         "measurement")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if not torch.cuda.is_available():
        raise SystemExit("bench.py requires an MI355X (no GPU visible)")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # modulo lets an N-rank run share fewer GPUs (RCCL smoke tests on a
    # 1-GPU box); on a full node it is the identity mapping
    dev_idx = local_rank % max(torch.cuda.device_count(), 1)
    dist_mode = world > 1
    if dist_mode:
        import torch.distributed as dist
        torch.cuda.set_device(dev_idx)
        dist.init_process_group("nccl")
    device = torch.device("cuda", dev_idx)
    torch.cuda.set_device(device)

    use_built_extension()
    from dampr_amd.gpu.corpus import synth_corpus_device
    from dampr_amd.gpu.tfidf import TfidfEngine
    if dist_mode:
        from dampr_amd.parallel.shuffle import (exchange_keyed_payload,
                                                all_reduce_scalar)
        import torch.distributed as dist

    # ---- setup (untimed): per-rank synthetic corpus, generated ON
    # DEVICE at HBM bandwidth (seconds even at 10+ GB, so the timed
    # region dominates the run's wall time), resident in HBM
    n_bytes = args.mb_per_gpu * (1 << 20)
    text = synth_corpus_device(n_bytes, device, vocab=100_000,
                               seed=1234 + rank)
    n = text.numel()
    line_bytes = 96                 # synth corpus: 12 words x 8 bytes
    docs_local = n // line_bytes
    eng = TfidfEngine(device)
    # a fixed path under a shared /tmp can belong to another user's run
    own_sink = args.sink_dir is None
    if own_sink:
        args.sink_dir = tempfile.mkdtemp(prefix="dampr_amd_bench_")
    else:
        shutil.rmtree(args.sink_dir, ignore_errors=True)

    # chunk bounds on line boundaries (count_chunk takes < 2 GiB); lines
    # are uniform so bounds land on multiples of line_bytes
    lines_per_chunk = (1 << 30) // line_bytes
    chunks = []
    lo = 0
    while lo < n:
        hi = min(lo + lines_per_chunk * line_bytes, n)
        chunks.append((lo, hi))
        lo = hi

    def step():
        eng.reset()
        for s, e in chunks:
            eng.count_chunk(text[s:e].contiguous(), pos_base=s)
        keys, df = eng.extract()
        if dist_mode:
            blob, lens = eng.token_strings_dev(keys, text)
            rk, rdf, rblob, rlens = exchange_keyed_payload(
                keys, df, blob, lens)
            eng.merge_exchanged(rk, rdf, rblob, rlens)
            keys, df = eng.extract()
            total_docs = all_reduce_scalar(eng.n_docs, device=device)
            src_text = rblob
        else:
            total_docs = eng.n_docs
            src_text = text
        idf = eng.idf(df, total_docs)
        eng.sink_tsv_device(args.sink_dir, rank, keys, df, idf, src_text)
        return keys, df, idf

    def barrier_sync():
        if dist_mode:
            dist.barrier()
        torch.cuda.synchronize(device)

    for _ in range(args.warmup):
        step()

    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    barrier_sync()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if dist_mode:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        total_docs_job = all_reduce_scalar(docs_local, device=device)
    else:
        total_docs_job = docs_local

    ms_per_step = elapsed * 1000.0 / args.steps
    rows_per_sec = total_docs_job * args.steps / elapsed
    gb_per_sec = (n * world / (1 << 30)) * args.steps / elapsed

    if args.dump_outputs:
        dump_outputs(args.dump_outputs,
                     "_rank{}".format(rank) if dist_mode else "",
                     *last,
                     os.path.join(args.sink_dir, "part-{}".format(rank)))

    # ---- explicit second metric (--full only): NVMe -> HBM ingest
    # bandwidth (the reference harness streams files from disk; the
    # headline metric processes the HBM-resident corpus, this reports
    # what staging it from disk costs).  Rank 0 only; capped probe bounds
    # wall time.
    ingest = None
    if args.full and rank == 0 and not args.no_ingest_probe:
        probe_bytes = min(n, 4 << 30)
        probe_path = os.path.join(args.sink_dir, "ingest_probe.bin")
        try:  # noqa: SIM105 — a probe failure must NOT lose the result
            with open(probe_path, "wb") as fh:
                step_b = 1 << 28
                for lo in range(0, probe_bytes, step_b):
                    hi = min(lo + step_b, probe_bytes)
                    fh.write(text[lo:hi].cpu().numpy().tobytes())
                fh.flush()
                os.fsync(fh.fileno())
            dst = torch.empty(probe_bytes, dtype=torch.uint8,
                              device=device)
            # double-buffered pinned staging: disk read of buffer A
            # overlaps the in-flight H2D of buffer B
            pins = [torch.empty(1 << 28, dtype=torch.uint8,
                                pin_memory=True) for _ in range(2)]
            evts = [torch.cuda.Event(), torch.cuda.Event()]
            for e in evts:
                e.record()
            torch.cuda.synchronize(device)
            t1 = time.perf_counter()
            with open(probe_path, "rb", buffering=0) as fh:
                lo = 0
                i = 0
                while lo < probe_bytes:
                    pin, evt = pins[i & 1], evts[i & 1]
                    evt.synchronize()     # buffer's last H2D done
                    got = fh.readinto(memoryview(pin.numpy()))
                    if not got:
                        break
                    dst[lo:lo + got].copy_(pin[:got], non_blocking=True)
                    evt.record()
                    lo += got
                    i += 1
            torch.cuda.synchronize(device)
            ingest = {
                "disk_to_hbm_gb_s":
                    probe_bytes / (1 << 30) / (time.perf_counter() - t1),
                "probe_gib": probe_bytes / (1 << 30),
            }
            del dst, pins
        except Exception as e:     # noqa: BLE001 — probe is auxiliary
            ingest = {"error": str(e)[:200]}
        finally:
            try:
                os.unlink(probe_path)
            except OSError:
                pass

    if own_sink:
        shutil.rmtree(args.sink_dir, ignore_errors=True)

    if rank == 0:
        n_gpus = world if dist_mode else args.gpus
        print(json.dumps({
            "metric": "tfidf_rows_per_sec",
            "value": rows_per_sec,
            "unit": "rows/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "int64-exact",
            "data": "synthetic",
            "config": {
                "model": "tfidf-docfreq",
                "corpus_mb_per_gpu": args.mb_per_gpu,
                "vocab": 100_000,
                "global_batch": total_docs_job,
                "seq_len": line_bytes,
                "parallelism": "dp{}".format(n_gpus),
                "gb_per_sec_ingest": gb_per_sec,
                "ingest_probe": ingest,
            },
        }))

    if dist_mode:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
