#!/usr/bin/env python
"""Record what handle construction decides for every configuration of tests/init_cases.py: tensor tables, parameter counts, device
bytes, the SHA-256 of the initial variables, gradient bucket ranges and the carried state's width.

The result is the fixture tests/golden/init_tables.json, which tests/test_gpu_init_tables.py compares exactly.  It pins a refactor of
Model::init, so it is recorded from the commit BEFORE the change (a checkout of that commit, this tool and tests/init_cases.py copied
in), on a whole MI355X and with the environment the tests see:

    python tools/record_init_tables.py --commit <hash of the recorded commit> --out tests/golden/init_tables.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--commit", required=True, help="hash of the commit the library under record was built from")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    from tests.init_cases import CASES, SEED, describe
    doc = {"recorded_from_commit": a.commit, "command": "python tools/record_init_tables.py --commit %s --out %s" % (a.commit, a.out),
           "seed": SEED, "cases": {}}
    for name, kw in CASES:
        doc["cases"][name] = describe(kw)
        print("%-32s %12d bytes" % (name, doc["cases"][name]["device_bytes"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
