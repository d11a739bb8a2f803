"""Set membership filter (``funcs.isin`` / ``funcs.notin``) through the
device engine, and its kernels alone.

* ``--mode pipeline`` (default): ``Dampr.columns(v).filter(isin(S)).count()``
  over ``--rows`` i64 values and over ``--words`` Zipf words.  Uses only the
  public DSL: where ``funcs.isin`` exists the predicate is that, otherwise
  the equivalent lambda, so the same file run on a commit without it gives
  the baseline (there the filter, and the count after it, are host stages:
  pick sizes it can finish).
* ``--mode kernel``: ``HipOps.filter_rows`` with one ``isin`` clause over
  ``--rows`` i64 rows against the torch-eager form
  (``m = torch.isin(v, members); k[m], v[m]``) on the same tensors, for
  sets of 8, 4096, 2**20 and 2**24 members (the last a 256 MiB table) and
  members chosen so that about 1 % and 50 % of the rows pass: the members
  are every ``stride``-th integer of the value range, strided ids as a
  group-by would hand over.  The three are timed interleaved (torch, hip,
  torch again): the two torch series are the same code, so their
  difference is the spread a hip/torch difference has to exceed.  GB/s is
  against the bytes the passes must move: predicate column read twice,
  keys read once, 16 B written per survivor, and one 8 B table word per
  probe step of both passes.  The steps are counted on the host: the
  built table is copied back and a sample of the rows walked through it.
  ``set_build_ms`` is the upload of the members and ``set_build``;
  ``host_fold_ms`` the lowering of the Python set (``_set_words`` and the
  tensor), measured up to 2**20 members.  Then ``sv_filter_rows`` over
  ``--words`` Zipf words against sets of 100 and 50_000 words, with
  filtering the decoded column through a Python set as the only reference
  there is.

Run on a GPU box:
    python benchmarks/bench_isin.py [--mode kernel] [--rows 100000000]
Prints one JSON line: per point the median of ``--runs`` after
``--warmup``; every timed call includes its host sync.
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

SET_SIZES = (8, 4096, 1 << 20, 1 << 24)
STRIDES = ((0.01, 100), (0.50, 2))
WORD_SETS = (100, 50_000)
VOCAB = 200_000
_M64 = (1 << 64) - 1


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


def zipf_words(n, seed):
    rng = np.random.default_rng(seed)
    vocab = np.array(["w{}".format(i) for i in range(VOCAB)], dtype=object)
    return vocab[rng.zipf(1.3, size=n) % VOCAB].tolist()


def word_members(m):
    """m words of the vocabulary, the frequent ones included."""
    return {"w{}".format(i) for i in range(0, 3 * m, 3)}


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def probe_steps(table, rows):
    """Mean table words one probe of set_has_u64 reads, over ``rows`` (a
    CPU sample of the column) and the built ``table`` (copied back)."""
    tab = table.cpu().numpy().view(np.uint64)
    mask = np.uint64(tab.size - 1)
    w = rows.numpy().view(np.uint64)
    w = w[w != 0]                       # the word 0 reads no table word
    with np.errstate(over="ignore"):
        slot = _splitmix64(w) & mask
    steps = np.zeros(w.size, dtype=np.int64)
    live = np.arange(w.size)
    while live.size:
        steps[live] += 1
        cur = tab[slot[live]]
        done = (cur == w[live]) | (cur == 0)
        live = live[~done]
        slot[live] = (slot[live] + np.uint64(1)) & mask
    return float(steps.sum()) / max(rows.numel(), 1)


def bench_kernel(args, device):
    from dampr_amd.gpu import filters
    from dampr_amd.gpu.backend import HipOps
    from dampr_amd.gpu.strvals import StrVals
    hip = HipOps()
    rng = np.random.default_rng(1)
    n = args.rows
    keys = torch.arange(n, dtype=torch.int64, device=device)
    unit = torch.from_numpy(rng.random(n))          # one draw for all points
    points = []
    for m in SET_SIZES:
        for sel, stride in STRIDES:
            span = m * stride
            vals = (unit * span).to(torch.int64).clamp_(0, span - 1)
            sample = vals[:1 << 20].clone()
            vals = vals.to(device)
            members = torch.arange(m, dtype=torch.int64) * stride
            clauses = [(1, "i64", "isin", members, None)]
            fold_ms = None
            if m <= 1 << 20:
                pyset = frozenset(members.tolist())
                t0 = time.perf_counter()
                folded = filters._set_words("i64", pyset)
                torch.tensor(sorted(folded), dtype=torch.int64)
                fold_ms = (time.perf_counter() - t0) * 1000.0
                del pyset, folded
            build, prog = timed(
                lambda: hip.filter_compile(clauses, "numeric", device),
                args.runs, args.warmup)
            dev_members = members.to(device)

            def torch_form():
                keep = torch.isin(vals, dev_members)
                return keys[keep], vals[keep]

            def hip_form():
                return hip.filter_rows(keys, vals, prog)

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
            steps = probe_steps(prog.set_v, sample)
            nbytes = 24 * n + 16 * kept + 2 * 8 * steps * n
            med = {k: statistics.median(v) for k, v in series.items()}
            torch_ms = min(med["torch_a"], med["torch_b"])
            points.append({
                "members": m, "stride": stride, "selectivity": sel,
                "table_bytes": 8 * prog.set_v.numel(), "rows_kept": kept,
                "probe_steps_per_row": steps, "bytes_moved": nbytes,
                "hip_ms": med["hip"], "torch_a_ms": med["torch_a"],
                "torch_b_ms": med["torch_b"],
                "torch_spread_ms": abs(med["torch_a"] - med["torch_b"]),
                "hip_gbps": nbytes / med["hip"] / 1e6,
                "speedup_vs_torch": torch_ms / med["hip"],
                "set_build_ms": statistics.median(build),
                "host_fold_ms": fold_ms, "runs_ms": series})
            del vals, outs, prog
    del keys, unit
    words = zipf_words(args.words, 2)
    sv = StrVals.from_strings(words).to(device)
    wkeys = torch.arange(len(words), dtype=torch.int64, device=device)
    word_points = []
    for m in WORD_SETS:
        wanted = word_members(m)
        clauses = [(1, "str", "isin",
                    sorted(w.encode("utf-8") for w in wanted), None)]
        build, prog = timed(
            lambda: hip.filter_compile(clauses, "string", device),
            args.runs, args.warmup)
        times, out = timed(lambda: hip.sv_filter_rows(wkeys, sv, prog),
                           args.runs, args.warmup)
        t0 = time.perf_counter()
        ref = [w for w in words if w in wanted]
        py_ms = (time.perf_counter() - t0) * 1000.0
        assert out[1].tolist() == ref, "mismatch against the Python set"
        word_points.append({
            "members": m, "rows_kept": len(ref),
            "hip_ms": statistics.median(times), "runs_ms": times,
            "python_set_ms": py_ms,
            "set_build_ms": statistics.median(build)})
    return {"metric": "isin_kernel_ms", "unit": "ms",
            "value": points[3]["hip_ms"], "rows": n, "points": points,
            "words": len(words), "word_points": word_points,
            "device": device}


def bench_pipeline(args, device):
    recognized = hasattr(funcs, "isin")
    rng = np.random.default_rng(0)
    vals = rng.integers(0, 1 << 20, size=args.rows, dtype=np.int64)
    wanted = frozenset(range(0, 1 << 20, 2))
    pred = funcs.isin(wanted) if recognized else (lambda x: x in wanted)
    pm = Dampr.columns(vals).filter(pred).count()
    times, out = timed(lambda: pm.run(device=device), args.runs, args.warmup)
    ints = {"rows": args.rows, "members": len(wanted),
            "ms": statistics.median(times), "runs_ms": times}
    if not args.no_check:
        uniq, counts = np.unique(vals[vals % 2 == 0], return_counts=True)
        assert dict(out.read()) == dict(zip(uniq.tolist(), counts.tolist()))
        ints["checked"] = True
    words = zipf_words(args.words, 2)
    stop = frozenset(word_members(WORD_SETS[0]))
    pred = funcs.notin(stop) if recognized else (lambda w: w not in stop)
    pm = Dampr.columns(words).filter(pred).count()
    times, out = timed(lambda: pm.run(device=device), args.runs, args.warmup)
    strs = {"rows": len(words), "members": len(stop),
            "ms": statistics.median(times), "runs_ms": times}
    if not args.no_check:
        import collections
        want = collections.Counter(w for w in words if w not in stop)
        assert dict(out.read()) == dict(want)
        strs["checked"] = True
    return {"metric": "isin_pipeline_ms", "unit": "ms", "value": ints["ms"],
            "predicate": "funcs.isin" if recognized else "lambda",
            "ints": ints, "words": strs, "device": device}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("pipeline", "kernel"),
                    default="pipeline")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--words", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-check", action="store_true",
                    help="skip the (untimed) comparison with numpy")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_isin.py measures the GPU engine and needs "
                         "a GPU")
    device = "cuda:0"
    if args.mode == "pipeline":
        res = bench_pipeline(args, device)
    else:
        res = bench_kernel(args, device)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
