#!/usr/bin/env python
"""Record what the training step's drivers compute for every call sequence of tests/step_cases.py: the losses of every call as fp32
bit patterns, the SHA-256 of variables, optimizer state and gradients, the recurrence launch counts of a profiled pass.

The result is the fixture tests/golden/step_fixture.json, which tests/test_gpu_step_fixture.py compares exactly.  It pins a refactor of
Model::d_backward / Model::g_backward, so it is recorded from the commit BEFORE the change (that commit's library, this tool,
tests/step_cases.py and tests/test_gpu_step_fixture.py added), on a whole MI355X:

    python tools/record_step_fixture.py --commit <hash of the recorded commit> --out tests/golden/step_fixture.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--commit", required=True, help="hash of the commit the library under record was built from")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    from tests.step_cases import GROUPS, group_cases, run_group
    doc = {"recorded_from_commit": a.commit, "command": "python tools/record_step_fixture.py --commit %s --out %s" % (a.commit, a.out),
           "cases": {}}
    failed = []
    for group in GROUPS:
        t0 = time.time()
        got = run_group(group)
        doc["cases"].update(got)
        for name, rec in sorted(got.items()):
            if "error" in rec:
                failed.append(name)
                print("%s FAILED:\n%s" % (name, rec["error"]), flush=True)
        print("%-24s %2d cases %6.1f s" % (group, len(got), time.time() - t0), flush=True)
        if len(got) < len(group_cases(group)):
            sys.exit("stopped: a case of group %s ended in a library or device error" % group)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    if failed:
        sys.exit("not a usable fixture: %d case(s) failed: %s" % (len(failed), ", ".join(failed)))


if __name__ == "__main__":
    main()
