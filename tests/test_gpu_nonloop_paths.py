"""The code of the fused 32-class kernel (csrc/qpn_avi_schur.hip) outside the Stage B pivot loop, bit for bit: the reuse body's
loads -- the LDS-DMA of Ad with its immediate offsets -- and replay, the c sweep, the read-back, the post-check and the stores.
The batches are those of tests/nonloop_cases.py (its docstring lists them); n = m = 32, resident handles.

* Ad layout: 4 160 nodes (the mixed, staggered instantiations) and 64 nodes (the plain ones) whose Ad holds distinct integers.
  Reuse, mixed and streamed sweeps are compared with a handle whose crash cache is off -- it stages Ad through registers, not by
  LDS-DMA -- and with a fresh handle's filling sweep: all six output arrays equal.
* parameter counts 0, 1, 7, 8, 9, 16, with w shared and with one strided row per node: the two must differ (unless p = 0), and a
  repeated sweep must repeat its bits.
* check paths: bounds infinite on one side, both sides, neither; all multipliers zero and exactly one nonzero multiplier in
  each tile column; check_tol = 0 turns a solved node's status into QPN_FAILURE and changes nothing else.
* every run against tests/golden/nonloop_paths_record.json, SHA-256 digests of the six arrays written by
  tests/golden/make_nonloop_paths_record.py from a build of the commit BEFORE this code was rewritten."""
import json
import os

import numpy as np
import pytest

import crash_mix_rule as rule
import nonloop_cases as NC

pytestmark = pytest.mark.gpu

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nonloop_paths_record.json")
_record = {}


def _golden():
    if not _record:
        _record.update(json.load(open(RECORD))["cases"])
    return _record


def _same(a, b, what):
    for k in NC.KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


def _against_record(name, runs):
    for label, out in runs:
        assert NC.digests(out) == _golden()[f"{name}/{label}"], f"{name}/{label}: not the bits of the record"


@pytest.mark.parametrize("cnt", NC.LAYOUT_COUNTS)
def test_ad_layout(engine, cnt):
    assert rule.mixed(cnt) == (cnt == 4160) and not rule.mixed(4096)
    A = NC.layout_records(cnt)[3]
    flat = np.transpose(A[0], (1, 0)).ravel() * 2.0 ** 8            # column-major, node 0: the running index + 1
    assert np.array_equal(flat, np.arange(1, 1025, dtype=np.float64))
    name = f"layout_{cnt}"
    runs = dict(NC.run_layout(engine, cnt))
    for s in range(3):
        ref = runs[f"sweep {s}/off"]
        assert not np.any(ref["status"] == -1)
        assert np.count_nonzero(ref["status"] == NC.SUCCESS) >= cnt // 2
        assert np.count_nonzero(ref["z"][:, NC.N:]) >= cnt // 2     # multipliers: the c sweep's result matters
        for other in ("stream", "plain", "fresh"):
            _same(runs[f"sweep {s}/{other}"], ref, f"{name} sweep {s}: {other} against QPN_OPT_CRASH_CACHE = 0")
    _against_record(name, list(runs.items()))


@pytest.mark.parametrize("p", NC.PARAM_COUNTS)
def test_parameter_counts(engine, p):
    runs = NC.run_params(engine, p)
    out = dict(runs)
    assert np.all(out["shared/fill"]["status"] == NC.SUCCESS)
    _same(out["shared/reuse"], out["shared/fill"], f"p = {p}: reuse against fill")
    _same(out["rows/reuse again"], out["rows/reuse"], f"p = {p}: the sweep repeated")
    assert np.array_equal(out["rows/reuse"]["z"], out["shared/fill"]["z"]) == (p == 0)
    _against_record(f"params_{p}", runs)


def test_check_paths(engine):
    runs = NC.run_checks(engine)
    out = dict(runs)
    fill, reuse, strict = out["fill"], out["reuse"], out["reuse, check_tol 0"]
    _same(reuse, fill, "checks: reuse against fill")
    assert np.all(fill["status"] == NC.SUCCESS)
    lam = fill["z"][:, NC.N:]
    i0, i1, i2 = (NC.CHECK_SPECIALS[k] for k in ("feasible", "row_reg_1", "row_reg_5"))
    assert np.count_nonzero(lam[i0]) == 0
    assert list(np.flatnonzero(lam[i1])) == [5] and list(np.flatnonzero(lam[i2])) == [21]
    l, u = NC.check_records()[5:7]
    both = np.isinf(l).all(axis=1) & np.isinf(u).all(axis=1)
    assert both.sum() >= 10 and np.count_nonzero(lam[both]) == 0
    for side in (np.isinf(l).all(axis=1) & ~both, np.isinf(u).all(axis=1) & ~both, ~np.isinf(l).any(axis=1) & ~np.isinf(u).any(axis=1)):
        assert side.sum() >= 10 and np.count_nonzero(lam[side]) > 0
    # check_tol = 0: a residual of one ulp is a violation -- the status flips where there is one, nothing else moves
    assert np.count_nonzero(strict["status"] == NC.FAILURE) >= 1
    assert np.all((strict["status"] == NC.FAILURE) | (strict["status"] == NC.SUCCESS))
    for k in NC.KEYS:
        if k != "status":
            assert np.array_equal(strict[k], reuse[k]), k
    _against_record("checks", runs)
