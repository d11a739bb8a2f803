"""Word count that keeps the words seen at least k times, without leaving
the device engine: the string column dictionary-encodes and counts on the
kernels, and the recognized predicate ``funcs.ge(k, on=funcs.snd)`` filters
the (word, count) records with the stable compaction kernels.  The lambda
``lambda wc: wc[1] >= k`` gives the same records through the per-record
host map.  Runs on CPU too (pure-torch oracle backend).

Usage: python examples/filter_device.py [k]
"""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import numpy as np

from dampr_amd import Dampr, funcs


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rng = np.random.default_rng(0)
    words = np.array(["w%d" % (z % 20_000)
                      for z in rng.zipf(1.3, size=1_000_000)])

    frequent = Dampr.columns(words).count() \
        .filter(funcs.ge(k, on=funcs.snd)).run("frequent-words")
    pairs = frequent.read()
    print("words seen at least {} times: {}".format(k, len(pairs)))
    print("most frequent:", sorted(pairs, key=lambda wc: -wc[1])[:5])

    # filters before the aggregate lower too: a conjunction in one pass,
    # and the count after it stays on the kernels
    amounts = rng.integers(-1000, 1000, size=5_000_000)
    hist = Dampr.columns(amounts) \
        .filter(funcs.gt(0)).filter(funcs.ne(500)).count().run("positive")
    print("distinct positive amounts:", len(hist.read()))


if __name__ == "__main__":
    main()
