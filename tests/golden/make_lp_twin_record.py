#!/usr/bin/env python3
"""Writes tests/golden/lp_twin_record.json: what the numpy twins of the three LP entries (polyhedra_host.solve_lps_host,
issubset_pairs_host, implicit_bounds_host) answer on the seeded families of the GPU suites -- the shapes, seeds and variants of
the ..._equals_the_twin_bit_for_bit family tests of tests/test_gpu_lp.py, test_gpu_subset_pairs.py and test_gpu_implicit_bounds.py.
For every output array the dtype, the shape and the SHA-256 of its C-contiguous bytes; the status / how histograms in clear, so
that a mismatch can be read.

The record pins the twin ACROSS commits: it is written from the polyhedra_host.py of the commit BEFORE a change to the twin and
tests/test_lp_host.py recomputes it with the working tree's.  From a checkout of that commit's file:

    git show <parent>:quadraticprogramnetworks.jl_amd/polyhedra_host.py > /tmp/parent_polyhedra_host.py
    python tests/golden/make_lp_twin_record.py --twin /tmp/parent_polyhedra_host.py

(the twins need numpy alone; before the twins had a module of their own the file was polyhedra.py).  Without --twin it reads the
working tree's polyhedra_host.py.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import implicit_cases  # noqa: E402
import lp_cases  # noqa: E402
import subset_cases  # noqa: E402

RECORD = os.path.join(HERE, "lp_twin_record.json")
TWIN = os.path.join(ROOT, "quadraticprogramnetworks.jl_amd", "polyhedra_host.py")
LP_SHAPES = [(1, 1), (3, 2), (2, 3), (5, 2), (16, 8)]
SUBSET_SHAPES = [(1, 1, 1), (3, 2, 2), (5, 4, 2), (16, 16, 8)]
IB_SHAPES = [(1, 1), (3, 2), (8, 4), (16, 8)]
CUT = dict(max_iters=1)
HISTOGRAMS = ("status", "how")


def load_twin(path=TWIN):
    spec = importlib.util.spec_from_file_location("lp_twin_under_record", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def colmajor(A):
    return np.ascontiguousarray(np.swapaxes(np.asarray(A, dtype=np.float64), -1, -2))


def digest(out):
    """-> dict(outputs = {name: dict(dtype, shape, sha256)}, histograms = {name: {code: count}})."""
    rec = dict(outputs={}, histograms={})
    for k in sorted(out):
        a = np.ascontiguousarray(out[k])
        rec["outputs"][k] = dict(dtype=str(a.dtype), shape=list(a.shape), sha256=hashlib.sha256(a.tobytes()).hexdigest())
        if k in HISTOGRAMS:
            codes, counts = np.unique(a, return_counts=True)
            rec["histograms"][k] = {str(int(c)): int(n) for c, n in zip(codes, counts)}
    return rec


def record(twin):
    """The record of one twin module: {case name: digest}."""
    cases = {}
    for shape in LP_SHAPES:
        seeds = list(range(40, 56))
        A, l, u, cost, poly_of, obj_row, obj_sign = lp_cases.family_batch(shape, seeds)
        Ac = colmajor(A)
        for tag, opts in (("default", None), ("max_iters=1", CUT)):
            cases[f"solve_lps {shape} cost {tag}"] = digest(twin.solve_lps_host(Ac, l, u, np.arange(len(seeds), dtype=np.int32), cost=cost, opts=opts))
            cases[f"solve_lps {shape} rows {tag}"] = digest(
                twin.solve_lps_host(Ac, l, u, poly_of[:64], obj_row=obj_row[:64], obj_sign=obj_sign[:64], opts=opts))
    for shape in SUBSET_SHAPES:
        A1, l1, u1, A2, l2, u2 = subset_cases.family_batch(shape, range(48))
        pi = np.concatenate([np.arange(48), [0, 0]]).astype(np.int32); pj = np.concatenate([np.arange(48), [1, 2]]).astype(np.int32)
        for tag, opts in (("default", None), ("max_iters=1", CUT)):
            cases[f"issubset_pairs {shape} {tag}"] = digest(
                twin.issubset_pairs_host(colmajor(A1), l1, u1, colmajor(A2), l2, u2, pi, pj, opts=opts))
    for shape in IB_SHAPES:
        A, l, u = implicit_cases.family_batch(shape, range(50))
        for tag, kw in (("default", {}), ("all_extremes", dict(all_extremes=True)), ("max_iters=1", dict(opts=CUT))):
            cases[f"implicit_bounds {shape} {tag}"] = digest(twin.implicit_bounds_host(colmajor(A), l, u, **kw))
    return cases


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--twin", default=TWIN, help="the polyhedra_host.py to record (default: the working tree's)")
    ap.add_argument("--out", default=RECORD)
    a = ap.parse_args()
    cases = record(load_twin(a.twin))
    with open(a.out, "w") as f:                                  # a case per line
        f.write('{"source": "tests/golden/make_lp_twin_record.py", "cases": {\n')
        f.write(",\n".join(f" {json.dumps(k)}: {json.dumps(cases[k], sort_keys=True)}" for k in sorted(cases)))
        f.write("\n}}\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
