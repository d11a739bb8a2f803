#!/usr/bin/env python3
"""Record the reference library's outputs for tests/test_reference_parity.py.

    python oracle/record_parity.py /path/to/reference/checkout

Imports the reference ``dampr`` package from the given checkout (it is
executed, never copied), runs every case of the parity test module over
it and writes the results to tests/golden/reference_parity.json.  Rerun
it whenever a case is added or changed there.
"""
import importlib
import importlib.util
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_lib(ref_root):
    sys.path.insert(0, ref_root)
    try:
        dampr = importlib.import_module("dampr")
        base = importlib.import_module("dampr.base")
        utils = importlib.import_module("dampr.utils")
    finally:
        sys.path.remove(ref_root)
    return types.SimpleNamespace(Dampr=dampr.Dampr, Map=base.Map,
                                 Reduce=base.Reduce,
                                 filter_by_count=utils.filter_by_count,
                                 Indexer=utils.Indexer)


def main(argv):
    if len(argv) != 2 or not os.path.isdir(os.path.join(argv[1], "dampr")):
        raise SystemExit(__doc__)
    sys.path.insert(0, ROOT)
    spec = importlib.util.spec_from_file_location(
        "test_reference_parity",
        os.path.join(ROOT, "tests", "test_reference_parity.py"))
    cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cases)
    with tempfile.TemporaryDirectory() as tmp:
        out = cases.record(reference_lib(os.path.abspath(argv[1])), tmp)
    os.makedirs(os.path.dirname(cases.GOLDEN), exist_ok=True)
    with open(cases.GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", cases.GOLDEN)


if __name__ == "__main__":
    main(sys.argv)
