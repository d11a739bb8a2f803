"""Word count over a string VALUE column through the device engine:
``Dampr.columns(words).count().run(device=...)`` — keying by a string
value, i.e. the dictionary encode of the column plus the usual
sort/segmented-reduce.

Uses only the public DSL, so the same file runs on a commit that still
takes the per-record host path for this case (the baseline to compare
against: run this script there, same arguments).

* default: a Zipf word column (``--rows`` 10M over a ``--vocab`` of about
  100k words).  ``ColumnSource.from_data`` (host arena construction,
  identical whatever path the engine takes) happens once, outside the
  timed window; each timed run covers ingest (H2D of the arena) through
  the synchronised end of ``run()``.
* ``--mode sort_distinct``: ``sort_by()`` over ``--rows`` DISTINCT strings
  (U == N), the case the host sort of the uniques dominates.

Run on a GPU box:
    python benchmarks/bench_strkeys.py [--rows 10000000] [--trace]
Prints one JSON line (median of ``--runs`` after ``--warmup``, and
``read_ms``: the first ``out.read()`` of the last run, which pays for any
key decoding the engine deferred); with ``--trace`` also the per-stage
timings of the last run.
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

import numpy as np
import torch

from dampr_amd import Dampr


def make_vocab(n, seed):
    """n distinct lowercase words, 3-12 letters."""
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        need = n - len(out)
        lens = rng.integers(3, 13, size=need)
        letters = rng.integers(97, 123, size=int(lens.sum()),
                               dtype=np.uint8).tobytes().decode("ascii")
        pos = 0
        for ln in lens:
            out.add(letters[pos:pos + ln])
            pos += ln
    return np.array(sorted(out))


def zipf_words(rows, vocab, seed):
    rng = np.random.default_rng(seed)
    idx = (rng.zipf(1.3, size=rows) - 1) % vocab
    return make_vocab(vocab, seed + 1)[idx]


def timed_runs(pm, device, runs, warmup):
    times = []
    out = None
    for i in range(warmup + runs):
        if device.startswith("cuda"):
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pm.run(device=device)
        if device.startswith("cuda"):
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i >= warmup:
            times.append(dt)
    return times, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("count", "sort_distinct"),
                    default="count")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-check", action="store_true",
                    help="skip the (untimed) comparison with a Python "
                         "oracle")
    ap.add_argument("--trace", action="store_true",
                    help="print per-stage timings of the last run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_strkeys.py measures the GPU engine and "
                         "needs a GPU")
    device = "cuda:0"

    if args.mode == "count":
        words = zipf_words(args.rows, args.vocab, 0)
        pm = Dampr.columns(words).count()
    else:
        words = make_vocab(args.rows, 2)
        np.random.default_rng(3).shuffle(words)
        pm = Dampr.columns(words).sort_by()
    src = next(iter(pm.pmer.graph.inputs.values()))
    blob_bytes = int(src.vals.blob.numel())
    offs_bytes = int(src.vals.offs.numel()) * 8

    times, out = timed_runs(pm, device, args.runs, args.warmup)
    res = {"metric": "strkeys_{}_ms".format(args.mode),
           "value": statistics.median(times) * 1000.0, "unit": "ms",
           "rows": args.rows, "runs_ms": [t * 1000.0 for t in times],
           "rows_per_sec": args.rows / statistics.median(times),
           "blob_bytes": blob_bytes, "offs_bytes": offs_bytes,
           "device": device}
    # first read of the last run's result, outside the timed window: key
    # decoding deferred to the read (the lazy string table) shows up here
    t0 = time.perf_counter()
    records = list(out.read())
    res["read_ms"] = (time.perf_counter() - t0) * 1000.0
    if args.mode == "count":
        got = dict(records)
        res["uniques"] = len(got)
        if not args.no_check:
            assert got == dict(collections.Counter(words.tolist())), \
                "count mismatch against collections.Counter"
            res["checked"] = True
    else:
        got = records
        res["uniques"] = len(got)
        if not args.no_check:
            assert got == sorted(words.tolist()), \
                "sort_by mismatch against sorted()"
            res["checked"] = True
    print(json.dumps(res))
    if args.trace:
        from dampr_amd.utils.trace import get_trace
        print(get_trace().report())


if __name__ == "__main__":
    main()
