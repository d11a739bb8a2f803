"""Row filter through the device engine, and the filter kernels alone.

* ``--mode pipeline`` (default): ``Dampr.columns(vals).filter(P).count()``
  over ``--rows`` i64 values drawn uniformly from [0, 2**20), with the
  predicate ``v > c`` and c chosen so that about 1%, 50% and 99% of the
  rows pass.  Uses only the public DSL: where ``funcs.gt`` exists the
  predicate is ``funcs.gt(c)``, otherwise the equivalent lambda, so the
  same file run on a commit without recognized predicates gives the
  baseline (there the filter, and the count after it, are host stages:
  pick a ``--rows`` it can finish).  ``ColumnSource`` construction is
  outside the timed window; each timed run covers ingest through the
  synchronised end of ``run()``.
* ``--mode kernel``: ``HipOps.filter_rows`` against the torch-eager
  boolean-mask form (``m = v > c; k[m], v[m]``) on the same device and the
  same inputs, three selectivities, i64 and f64 values.  The three are
  timed interleaved (torch, hip, torch again): the two torch series are
  the same code, so their difference is the run-to-run spread a hip/torch
  difference has to exceed.  GB/s is against the bytes the two passes must
  move: predicate column read twice, keys read once, 16 B written per
  survivor.

Run on a GPU box:
    python benchmarks/bench_filter.py [--mode kernel] [--rows 100000000]
Prints one JSON line: per point the median of ``--runs`` after
``--warmup``.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import numpy as np
import torch

from dampr_amd import Dampr, funcs

SELECTIVITIES = (0.01, 0.50, 0.99)
VALUE_RANGE = 1 << 20


def threshold(sel):
    """c such that ``v > c`` passes a fraction ``sel`` of uniform
    [0, VALUE_RANGE) integers."""
    return int(round(VALUE_RANGE * (1.0 - sel))) - 1


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
    rng = np.random.default_rng(0)
    vals = rng.integers(0, VALUE_RANGE, size=args.rows, dtype=np.int64)
    recognized = hasattr(funcs, "gt")
    points = []
    for sel in SELECTIVITIES:
        c = threshold(sel)
        pred = funcs.gt(c) if recognized else (lambda x, c=c: x > c)
        pm = Dampr.columns(vals).filter(pred).count()
        times, out = timed(lambda: pm.run(device=device), args.runs,
                           args.warmup)
        point = {"selectivity": sel, "constant": c,
                 "ms": statistics.median(times), "runs_ms": times}
        if not args.no_check:
            kept = vals[vals > c]
            uniq, counts = np.unique(kept, return_counts=True)
            assert dict(out.read()) == dict(zip(uniq.tolist(),
                                                counts.tolist())), \
                "count mismatch against numpy"
            point["rows_kept"] = int(kept.size)
            point["checked"] = True
        points.append(point)
    return {"metric": "filter_pipeline_ms", "unit": "ms",
            "value": points[1]["ms"], "rows": args.rows,
            "predicate": "funcs.gt" if recognized else "lambda",
            "points": points, "device": device}


def bench_kernel(args, device):
    from dampr_amd.gpu.backend import HipOps
    hip = HipOps()
    rng = np.random.default_rng(1)
    n = args.rows
    keys = torch.arange(n, dtype=torch.int64, device=device)
    ivals = torch.from_numpy(
        rng.integers(0, VALUE_RANGE, size=n, dtype=np.int64)).to(device)
    points = []
    for dtype, vals in (("i64", ivals), ("f64", ivals.to(torch.float64))):
        for sel in SELECTIVITIES:
            c = threshold(sel)
            const = c if dtype == "i64" else float(c)
            clauses = [(1, dtype, "gt", const, 0)]

            def torch_form():
                m = vals > const
                return keys[m], vals[m]

            def hip_form():
                return hip.filter_rows(keys, vals, clauses)

            series = {"torch_a": [], "hip": [], "torch_b": []}
            outs = {}
            for i in range(args.warmup + args.runs):
                for name, fn in (("torch_a", torch_form), ("hip", hip_form),
                                 ("torch_b", torch_form)):
                    t, outs[name] = timed(fn, 1, 0)
                    if i >= args.warmup:
                        series[name].extend(t)
            assert torch.equal(outs["hip"][0], outs["torch_a"][0])
            assert torch.equal(outs["hip"][1], outs["torch_a"][1])
            kept = int(outs["hip"][0].numel())
            nbytes = 24 * n + 16 * kept
            med = {k: statistics.median(v) for k, v in series.items()}
            torch_ms = min(med["torch_a"], med["torch_b"])
            points.append({
                "dtype": dtype, "selectivity": sel, "rows_kept": kept,
                "hip_ms": med["hip"], "torch_a_ms": med["torch_a"],
                "torch_b_ms": med["torch_b"],
                "torch_spread_ms": abs(med["torch_a"] - med["torch_b"]),
                "hip_gbps": nbytes / med["hip"] / 1e6,
                "torch_gbps_same_bytes": nbytes / torch_ms / 1e6,
                "speedup_vs_torch": torch_ms / med["hip"],
                "runs_ms": series})
    return {"metric": "filter_kernel_ms", "unit": "ms",
            "value": points[1]["hip_ms"], "rows": n, "points": points,
            "device": device}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("pipeline", "kernel"),
                    default="pipeline")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-check", action="store_true",
                    help="skip the (untimed) comparison with numpy")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_filter.py measures the GPU engine and "
                         "needs a GPU")
    device = "cuda:0"
    if args.mode == "pipeline":
        res = bench_pipeline(args, device)
    else:
        res = bench_kernel(args, device)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
