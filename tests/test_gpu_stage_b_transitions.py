"""The batch of tests/stage_b_transitions.py -- every ordered pair of iteration kinds of the Stage B pivot loop, that is every
hand-over of the state the loop carries from one iteration into the next -- through the instantiations of the fused 32-class
kernel that share the loop (csrc/qpn_avi_schur.hip): a resident handle with a filling sweep and two reuse sweeps, n = m = 16,
the ragged (20, 12), explicit M of N = 64, the pivot budget, and 4 224 nodes -- the staggered, mixed instantiations of the
bench -- with the crash cache streamed and not.  tests/test_stage_b_transitions_host.py shows without a GPU that the batch takes
the pairs.  Each scenario is checked

* against the CPU oracle with the bars of tests/test_gpu_stage_b_paths.py: status, pivots and active masks equal, primals to
  1e-9, residuals to 1e-8, the primal write-back equal to z;
* bit for bit against tests/golden/stage_b_transitions_record.json, SHA-256 digests of every output array, written by
  tests/golden/make_stage_b_transitions_record.py from a build of the commit BEFORE the loop's carried state was moved."""
import json
import os

import numpy as np
import pytest

import stage_b_cases as S
import stage_b_transitions as T

pytestmark = pytest.mark.gpu

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_b_transitions_record.json")
_record = {}


def _golden():
    if not _record:
        _record.update(json.load(open(RECORD))["cases"])
    return _record


@pytest.mark.parametrize("name", list(T.SCENARIOS))
def test_stage_b_transitions(engine, oracle, name):
    kind, _, n, m, seed = T.SCENARIOS[name]
    recs, names = T.scenario_records(name)
    idx = np.arange(len(names))                         # the oracle sees the batch; the padding of the large launches is pinned by the record
    runs = T.run_scenario(engine, name)
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
            assert set(np.unique(out["status"][idx])) >= {S.SUCCESS, S.MAX_ITERS}, tag
            assert np.all(out["pivots"][idx][ref["status"] == S.MAX_ITERS] == max_pivots), tag
        assert S.digests(out) == _golden()[tag], f"{tag}: not the bits of the record"
