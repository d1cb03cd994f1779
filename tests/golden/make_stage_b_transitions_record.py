#!/usr/bin/env python3
"""Writes tests/golden/stage_b_transitions_record.json: the SHA-256 digest of every output array (z, status, resid, pivots,
active, primal write-back) of every run of every scenario of tests/stage_b_transitions.py, and nothing else.

The record pins the outputs of the Stage B pivot loop ACROSS commits: it is written on an MI355X from a build of the commit
BEFORE a change to the loop, and tests/test_gpu_stage_b_transitions.py compares the working tree's build with it bit for bit.
From a checkout of that commit, build its library (csrc/build.sh with QPN_OUT=<path>), then in the working tree:

    QPN_HIP_LIB=<path of that library> python tests/golden/make_stage_b_transitions_record.py --commit <that commit's hash>

The record names the commit it was written from.  An existing record is not overwritten without --force."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stage_b_cases as S  # noqa: E402
import stage_b_transitions as T  # noqa: E402

RECORD = os.path.join(HERE, "stage_b_transitions_record.json")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", required=True, help="the commit whose build (QPN_HIP_LIB) is recorded")
    ap.add_argument("--out", default=RECORD)
    ap.add_argument("--force", action="store_true", help="overwrite an existing record")
    a = ap.parse_args()
    if os.path.exists(a.out) and not a.force:
        sys.exit(f"{a.out} exists: a record is written once, from the commit before a change (--force overwrites it)")
    import qpn_amd
    from qpn_amd import _lib
    engine = qpn_amd.default_engine(0)
    cases = {}
    for name in T.SCENARIOS:
        for label, w, out, max_pivots in T.run_scenario(engine, name):
            cases[f"{name}/{label}"] = S.digests(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:                                  # a case per line
        f.write('{"source": "tests/golden/make_stage_b_transitions_record.py", "commit": %s, "cases": {\n' % json.dumps(a.commit))
        f.write(",\n".join(f" {json.dumps(k)}: {json.dumps(cases[k], sort_keys=True)}" for k in sorted(cases)))
        f.write("\n}}\n")
    print("wrote", a.out, "from", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
