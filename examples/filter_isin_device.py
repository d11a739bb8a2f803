"""A stop-word filter without leaving the device engine: drop a set of
words from a word column before counting it, then keep a wanted set of
the (word, count) records.  ``funcs.notin`` / ``funcs.isin`` probe a device
hash set in the filter kernels: the words' bytes against a string set, the
string keys as integer ids against a numeric one.  The equivalent lambdas
give the same records through the per-record host map.  Runs on CPU too
(pure-torch oracle backend).  The result is checked against Python sets.

Usage: python examples/filter_isin_device.py [n_words]
"""
import collections
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import numpy as np

from dampr_amd import Dampr, funcs


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    rng = np.random.default_rng(0)
    words = ["w%d" % (z % 20_000) for z in rng.zipf(1.3, size=n)]
    # the 50 most frequent words and a few that never occur; a number in
    # the set is no error, it just never equals a word
    stop = {"w%d" % i for i in range(1, 51)} | {"the", "of", "", 7}
    wanted = {"w%d" % i for i in range(0, 20_000, 5)}

    counted = Dampr.columns(np.array(words)) \
        .filter(funcs.notin(stop)).count() \
        .filter(funcs.isin(wanted, on=funcs.fst)).run("stop-words")
    got = dict(counted.read())

    kept = collections.Counter(w for w in words if w not in stop)
    want = {w: c for w, c in kept.items() if w in wanted}
    assert got == want, "device filter disagrees with Python sets"
    print("{} words, {} after the stop list, {} distinct wanted words "
          "(checked against Python sets)".format(
              n, sum(kept.values()), len(got)))
    print("most frequent:", sorted(got.items(), key=lambda wc: -wc[1])[:5])


if __name__ == "__main__":
    main()
