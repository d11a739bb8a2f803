"""String row filter through the device engine, and the string-filter
kernels alone.

* ``--mode pipeline`` (default): a Zipf word column (``--rows`` 10M over a
  ``--vocab`` of about 100k words, ``bench_strkeys``'s generator) through

    value_between   ``columns(words).filter(funcs.between("m", "t")).count()``
    table_key_ge    ``columns(words).count().filter(funcs.ge("m", on=fst))``

  Uses only the public DSL and predicates that are plain host functions
  on a commit without the string lowering, so the same file run there
  gives the baseline (the filter stage is then a host map over decoded
  records).  ``ColumnSource`` construction is outside the timed window;
  each timed run covers ingest through the synchronised end of ``run()``.
* ``--mode kernel``: ``HipOps.sv_filter_rows`` alone over the same column
  already on the device, for ``between``, ``ge`` and ``startswith``.  GB/s
  is against the bytes the passes must move: offsets and arena read by
  both passes (8 B + the row per row, twice), 8 B of key read and 24 B
  written per survivor, then the gather's 24 B read per survivor and the
  surviving bytes read and written.

Run on a GPU box:
    python benchmarks/bench_strfilter.py [--mode kernel] [--rows 10000000]
Prints one JSON line: per point the median of ``--runs`` after
``--warmup``.
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import torch

from bench_strkeys import zipf_words
from dampr_amd import Dampr, funcs


def timed(fn, runs, warmup):
    times = []
    out = None
    for i in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1000.0)
    return times, out


def bench_pipeline(args, device):
    words = zipf_words(args.rows, args.vocab, 0)
    wc = None if args.no_check else collections.Counter(words.tolist())
    pipelines = (
        ("value_between",
         Dampr.columns(words).filter(funcs.between("m", "t")).count(),
         lambda w: "m" <= w <= "t"),
        ("table_key_ge",
         Dampr.columns(words).count().filter(funcs.ge("m", on=funcs.fst)),
         lambda w: w >= "m"),
    )
    points = []
    for name, pm, keep in pipelines:
        times, out = timed(lambda: pm.run(device=device), args.runs,
                           args.warmup)
        point = {"pipeline": name, "ms": statistics.median(times),
                 "runs_ms": times}
        t0 = time.perf_counter()
        got = dict(out.read())
        point["read_ms"] = (time.perf_counter() - t0) * 1000.0
        point["uniques_kept"] = len(got)
        if wc is not None:
            assert got == {w: c for w, c in wc.items() if keep(w)}, \
                "{}: mismatch against collections.Counter".format(name)
            point["checked"] = True
        points.append(point)
    return {"metric": "strfilter_pipeline_ms", "unit": "ms",
            "value": points[0]["ms"], "rows": args.rows,
            "vocab": args.vocab, "points": points, "device": device}


def bench_kernel(args, device):
    from dampr_amd.gpu.backend import HipOps
    from dampr_amd.gpu.strvals import StrVals
    hip = HipOps()
    words = zipf_words(args.rows, args.vocab, 0)
    sv = StrVals.from_strings(words.tolist(), device=device)
    n = sv.numel()
    keys = torch.arange(n, dtype=torch.int64, device=device)
    blob_n = int(sv.blob.numel())
    points = []
    for name, clause in (("between", (1, "str", "between", b"m", b"t")),
                         ("ge", (1, "str", "ge", b"m", b"")),
                         ("startswith", (1, "str", "startswith", b"m", b""))):
        prog = hip.sv_filter_compile([clause], torch.device(device))
        times, (out_k, out_v) = timed(
            lambda: hip.sv_filter_rows(keys, sv, prog), args.runs,
            args.warmup)
        kept = int(out_k.numel())
        kept_bytes = int(out_v.blob.numel())
        nbytes = 2 * (8 * n + blob_n) + 32 * kept + 24 * kept + \
            2 * kept_bytes
        ms = statistics.median(times)
        points.append({"clause": name, "rows_kept": kept,
                       "bytes_kept": kept_bytes, "ms": ms, "runs_ms": times,
                       "bytes_moved": nbytes, "gbps": nbytes / ms / 1e6})
    return {"metric": "strfilter_rows_ms", "unit": "ms",
            "value": points[0]["ms"], "rows": n, "blob_bytes": blob_n,
            "points": points, "device": device}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("pipeline", "kernel"),
                    default="pipeline")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-check", action="store_true",
                    help="skip the (untimed) comparison with a Python "
                         "oracle")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_strfilter.py measures the GPU engine and "
                         "needs a GPU")
    device = "cuda:0"
    res = (bench_pipeline if args.mode == "pipeline" else bench_kernel)(
        args, device)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
