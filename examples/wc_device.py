"""Word count over a string column on the device engine.

The words are the VALUES of the column, so count() keys by a string value:
the engine dictionary-encodes the column on device (hash, radix sort,
byte-verified segment heads), and the count itself is the usual radix
sort + segmented reduce over the ids.  Runs on CPU too (oracle backend).

Usage: python examples/wc_device.py [text-file]
"""
import os
import re
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import numpy as np

from dampr_amd import Dampr


def main(fname):
    if fname is not None:
        with open(fname, encoding="utf-8", errors="replace") as fh:
            words = np.array([w for w in re.split(r"[^\w]+", fh.read().lower())
                              if w])
    else:
        rng = np.random.default_rng(0)
        vocab = np.array(["word%d" % i for i in range(5000)])
        words = vocab[(rng.zipf(1.3, size=1_000_000) - 1) % vocab.size]

    col = Dampr.columns(words)
    counts = col.count().run("wc-device")
    top = sorted(counts.read(), key=lambda kv: (-kv[1], kv[0]))[:10]
    print("{} words, {} distinct".format(words.size, len(counts.read())))
    for word, n in top:
        print("{:>10}  {}".format(n, word))

    # the same column, totally ordered, and one representative per word
    first = col.sort_by().run("sorted").read()[:3]
    print("first words in order:", first)
    groups = col.a_group_by().first().run("distinct")
    print("distinct via group/first:", len(groups.read()))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
