"""Filters over words without leaving the device engine: keep a range or
a prefix of a word column before counting it, or keep some of the
(word, count) records after.  ``str`` constants in the recognized
predicates (``funcs.ge``, ``between``, ``startswith``, ...) compare
against string values byte-wise on the string-filter kernels, and against
string keys as integer comparisons on their ranks.  The equivalent lambdas
give the same records through the per-record host map.  Runs on CPU too
(pure-torch oracle backend).

Usage: python examples/filter_words_device.py [prefix]
"""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import numpy as np

from dampr_amd import Dampr, funcs


def main():
    prefix = sys.argv[1] if len(sys.argv) > 1 else "w12"
    rng = np.random.default_rng(0)
    words = np.array(["w%d" % (z % 20_000)
                      for z in rng.zipf(1.3, size=1_000_000)])

    # filter the values, then count the survivors
    ranged = Dampr.columns(words) \
        .filter(funcs.between("w2", "w5")).filter(funcs.ne("w3")) \
        .count().run("ranged-words")
    print("distinct words in [w2, w5] but w3:", len(ranged.read()))

    # count, then filter the (word, count) records by key and by value
    picked = Dampr.columns(words).count() \
        .filter(funcs.startswith(prefix, on=funcs.fst)) \
        .filter(funcs.ge(5, on=funcs.snd)).run("picked-words")
    pairs = picked.read()
    print("words starting with {!r} seen at least 5 times: {}".format(
        prefix, len(pairs)))
    print("most frequent:", sorted(pairs, key=lambda wc: -wc[1])[:5])


if __name__ == "__main__":
    main()
