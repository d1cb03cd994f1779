"""Every exit and join of the Stage B pivot loop of the fused 32-class kernel (csrc/qpn_avi_schur.hip), in every instantiation
that shares the loop.  The classes and the batches are those of tests/stage_b_cases.py (its docstring lists them;
tests/test_stage_b_cases_host.py shows without a GPU that every class is what it says).  Each scenario is checked three ways:

* against the CPU oracle, with the bars of the parity tests: status, pivots and active masks equal, primals to 1e-9, residuals
  to 1e-8, the primal write-back equal to z;
* the special nodes show their class's marker in the GPU's own outputs (at the parameters the classes are built for);
* bit for bit against tests/golden/stage_b_paths_record.json, SHA-256 digests of every output array, written by
  tests/golden/make_stage_b_paths_record.py from a build of the commit BEFORE the loop's scalar side was rewritten: a rewrite
  of the loop's control flow may not change a single bit of any output.

Scenarios: 96 nodes of n = m = 32 through a resident handle (a filling sweep and two reuse sweeps; symmetric records, and the
same with one Qd made asymmetric), n = m = 16, the ragged (20, 12), explicit-M batches of N = 64 and N = 40, the pivot budget,
and 4 224 nodes of n = m = 32 -- just above the 4 096 resident wavefronts: the staggered, mixed instantiations -- with the crash
cache streamed (QPN_OPT_LLC_BUDGET_MB = -1) and not (0)."""
import json
import os

import numpy as np
import pytest

import stage_b_cases as S

pytestmark = pytest.mark.gpu

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_b_paths_record.json")
_record = {}


def _golden():
    if not _record:
        _record.update(json.load(open(RECORD))["cases"])
    return _record


@pytest.mark.parametrize("name", list(S.SCENARIOS))
def test_stage_b_paths(engine, oracle, name):
    kind, cnt, n, m, seed = S.SCENARIOS[name]
    recs, where = S.scenario_records(name)
    # the oracle sees every node of a small batch; of the large one the special nodes and the first 64
    idx = np.arange(cnt) if cnt <= 1000 else np.unique(np.concatenate([np.arange(64), np.array(sorted(where.values()))]))
    runs = S.run_scenario(engine, name)
    assert len(runs) >= 2
    for label, w, out, max_pivots in runs:
        tag = f"{name}/{label}"
        ref = S.oracle_solve(oracle, recs, w, idx, max_pivots)
        assert np.array_equal(out["status"][idx], ref["status"]), tag
        assert np.array_equal(out["pivots"][idx], ref["pivots"]), (tag, idx[out["pivots"][idx] != ref["pivots"]])
        ok = ref["status"] == S.SUCCESS
        assert ok.sum() >= 10, tag
        assert np.array_equal(out["active"][idx][ok], ref["active"][ok]), tag
        err = np.max(np.abs(out["z"][idx][ok] - ref["z"][ok]))
        assert err <= 1e-9, (tag, err)
        assert np.max(out["resid"][idx][ok]) <= 1e-8, tag
        solved = out["status"] == S.SUCCESS
        assert np.array_equal(out["x_out"][solved, :n], out["z"][solved, :n]), tag
        if max_pivots:
            i = where["many"]
            assert out["status"][i] == S.MAX_ITERS and out["pivots"][i] == max_pivots, tag
            assert set(np.unique(out["status"])) >= {S.SUCCESS, S.MAX_ITERS}, tag
        if w is S.W0:
            for cls, i in where.items():
                if max_pivots and cls in ("many", "flips", "free_pair"):
                    continue                            # (longer than the budget, or possibly so)
                rec, meta = S.special(cls, n, m)
                S.check_marker(cls, rec, meta, out, i, n)
        assert S.digests(out) == _golden()[tag], f"{tag}: not the bits of the record"
