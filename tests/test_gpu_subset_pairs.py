"""qpn_issubset_pairs (csrc/qpn_lp.hip) against its numpy twin polyhedra.issubset_pairs_host, bit for bit on every output, in every
kernel class and both memory modes; its argument errors; and the host functions that use it -- issubset_batch, remove_subsets_many,
solve() end to end -- against the emptiness queries they built before (an engine wrapper that hides issubset_pairs)."""
from __future__ import annotations

import numpy as np
import pytest

import lp_cases
import subset_cases
from subset_cases import BY_OPTIMUM, BY_POINT, EMPTY, FAILURE, HOLDS, UNBOUNDED

pytestmark = pytest.mark.gpu


def _both_modes(engine, A1, l1, u1, A2, l2, u2, pi, pj, **kw):
    """The kernel in host and in device mode against the twin.  -> the twin's answer."""
    import torch
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    pi = np.asarray(pi, np.int32); pj = np.asarray(pj, np.int32)
    host = (colmajor(A1), l1, u1, colmajor(A2), l2, u2)
    want = polyhedra.issubset_pairs_host(*host, pi, pj, **kw)
    subset_cases.same_bits(engine.issubset_pairs(*host, pi, pj, **kw), want, "host mode")
    dv = f"cuda:{engine.device}"
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dv)
    i = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dv)
    got = engine.issubset_pairs(*(f(a) for a in host), i(pi), i(pj), **kw)
    assert all(hasattr(v, "cpu") for v in got.values())
    subset_cases.same_bits(got, want, "device mode")
    return want


def _family_pairs(shape):
    """Seeds 0..47 pair by pair, plus piece 0 as P1 against the second pieces 1 and 2: 50 pairs, a first piece shared by three of
    them, and a last workgroup of the wavefront class with two of its four pairs."""
    batch = subset_cases.family_batch(shape, range(48))
    pi = np.concatenate([np.arange(48), [0, 0]]); pj = np.concatenate([np.arange(48), [1, 2]])
    return batch, pi, pj


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 2, 2), (5, 4, 2), (16, 16, 8)])
def test_the_family_equals_the_twin_bit_for_bit(engine, shape):
    batch, pi, pj = _family_pairs(shape)
    assert engine.lp_kernel_class(shape[0], shape[2]) == 0
    want = _both_modes(engine, *batch, pi, pj)
    seen = set(want["how"].tolist())
    assert {HOLDS} < seen <= {HOLDS, BY_POINT, BY_OPTIMUM, UNBOUNDED, EMPTY}
    if shape == (16, 16, 8):
        assert seen == {HOLDS, BY_POINT, BY_OPTIMUM, UNBOUNDED, EMPTY} and want["iters"].max() > 3 and want["lps"].max() > 3
        cut = _both_modes(engine, *batch, pi, pj, opts=dict(max_iters=1))
        assert subset_cases.ITER_LIMIT in cut["how"].tolist()


def _class_shapes(engine):
    """(the largest wave-class r1, the smallest workgroup-class r1, the smallest workspace-class r1) at d = 24, 24, 128."""
    r0 = max(r for r in range(1, 200) if engine.lp_kernel_class(r, 24) == 0)
    r2 = min(r for r in range(1, 1025) if engine.lp_kernel_class(r, 128) == 2)
    return (r0, 24), (r0 + 1, 24), (r2, 128)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_class_boundaries_equal_the_twin_bit_for_bit(engine, which):
    r1, d = _class_shapes(engine)[which]
    r2 = 4
    assert engine.lp_kernel_class(r1, d) == which and (which == 0 or engine.lp_kernel_class(r1 - 1, d) == which - 1)
    A1, l1, u1 = lp_cases.bounded_batch(17 + which, 3, r1, d)
    A1[2, 1:, 0] = 0.0                                            # x_0 in row 0 alone, open below: that row has no minimum
    l1[2] = A1[2] @ np.ones(d) - 1.0; u1[2] = l1[2] + 2.0; l1[2, 0] = -np.inf
    A2, l2, u2 = lp_cases.bounded_batch(27 + which, 3, r2, d)
    centre = np.linalg.lstsq(A1[0], 0.5 * (l1[0] + u1[0]), rcond=None)[0]
    A2[0] = A1[0, [5, 0, 7, 2]]; l2[0] = l1[0, [5, 0, 7, 2]] - 0.5; u2[0] = u1[0, [5, 0, 7, 2]] + 0.5       # P1[0] widened: holds
    l2[0, 1] = -np.inf
    l2[1] = A2[1] @ centre; u2[1] = np.inf                        # every row cuts P1[0] through its centre: refuted
    A2[2] = 0.0; A2[2, :, 0] = [1.0, -1.0, 2.0, 1.0]              # bounds on x_0 alone, far out
    l2[2] = [-1e3, -np.inf, -2e3, -np.inf]; u2[2] = [np.inf, 1e3, np.inf, 1e3]
    pi = [0, 0, 1, 2, 0, 2]; pj = [0, 1, 1, 2, 2, 0]
    want = _both_modes(engine, A1, l1, u1, A2, l2, u2, pi, pj)
    how = want["how"].tolist()
    assert how[0] == HOLDS and how[1] in (BY_POINT, BY_OPTIMUM) and how[3] == UNBOUNDED
    assert set(how) - {BY_POINT, BY_OPTIMUM} == {HOLDS, UNBOUNDED} and set(how) & {BY_POINT, BY_OPTIMUM}
    assert want["iters"].max() > 3
    assert want["lps"][0] == 1                                    # the widened copy: every bound P1's own


def test_different_rows_and_pack_sizes(engine):
    """r1 != r2 and B1 != B2; pieces of one pack read in place by several pairs."""
    A1, l1, u1, _, _, _ = subset_cases.family_batch((12, 9, 6), range(7))
    _, _, _, A2, l2, u2 = subset_cases.family_batch((12, 5, 6), range(30, 33))
    A2[1, 0] = A1[3, 4]; l2[1, 0] = l1[3, 4]; u2[1, 0] = u1[3, 4]
    pi = np.repeat(np.arange(7), 3); pj = np.tile(np.arange(3), 7)
    want = _both_modes(engine, A1, l1, u1, A2, l2, u2, pi, pj)
    assert len(set(want["how"].tolist())) >= 2
    back = _both_modes(engine, A2, l2, u2, A1, l1, u1, pj, pi)                         # the packs the other way round: r1 = 5, r2 = 12
    assert back["lps"].max() > 1


def test_argument_errors(engine):
    import torch
    from qpn_amd.engine import QpnError, colmajor
    A1, l1, u1, A2, l2, u2 = subset_cases.family_batch((3, 2, 2), [0, 1, 2])
    host = (colmajor(A1), l1, u1, colmajor(A2[:2]), l2[:2], u2[:2])
    i32 = lambda a: np.array(a, np.int32)
    for pi, pj in (([0, 3, 1], [0, 0, 0]), ([0, -1, 1], [0, 0, 0]), ([0, 1, 1], [0, 2, 0]), ([0, 1, 1], [0, -1, 0])):
        with pytest.raises(QpnError, match="bad argument|out of range"):
            engine.issubset_pairs(*host, i32(pi), i32(pj))
    # the same indices in device arrays: that pair alone fails, with zeros
    dv = f"cuda:{engine.device}"
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dv)
    want = _both_modes(engine, A1, l1, u1, A2[:2], l2[:2], u2[:2], [0, 2], [0, 1])
    got = engine.issubset_pairs(*(f(a) for a in host), f(i32([0, 3, -1, 1, 2])), f(i32([0, 0, 1, 2, 1])))
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert got["how"][1:4].tolist() == [FAILURE] * 3 and got["bound"][1:4].tolist() == [-1] * 3
    for k in ("sub", "val", "lps", "iters"):
        assert not got[k][1:4].any()
    for k in subset_cases.OUTPUTS:
        assert np.array_equal(got[k][[0, 4]], want[k])
    # sizes beyond the limits
    z = lambda b, r, d: (np.zeros((b, d, r)), np.zeros((b, r)), np.ones((b, r)))
    for r1, r2, d in ((1025, 2, 2), (2, 1025, 2), (2, 2, 257)):
        with pytest.raises(QpnError, match="size"):
            engine.issubset_pairs(*z(1, r1, d), *z(1, r2, d), i32([0]), i32([0]))
    # inconsistent shapes
    for bad in ((host[0], l1[:2], u1) + host[3:], host[:3] + (colmajor(np.zeros((2, 2, 3))), l2[:2], u2[:2]), host[:5] + (u2,)):
        with pytest.raises(QpnError, match="inconsistent shapes"):
            engine.issubset_pairs(*bad, i32([0]), i32([0]))
    with pytest.raises(QpnError, match="inconsistent shapes"):
        engine.issubset_pairs(*host, i32([0, 1]), i32([0]))
    # no pairs
    assert engine.issubset_pairs(*host, i32([]), i32([]))["sub"].shape == (0,)


# ---- the host functions on the pair route against the emptiness queries -------------------------------------------------------
class _WithoutPairs:
    """The engine without issubset_pairs: the host functions take the route they took before."""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        if name == "issubset_pairs":
            raise AttributeError(name)
        return getattr(self._eng, name)


def _node_solves(engine):
    return sum(v for k, v in engine.calls.items() if k.startswith("qpn_solve_nodes") or k == "qpn_solve_avi_batch")


def test_issubset_batch_on_the_pair_route(engine):
    from qpn_amd import polyhedra
    pairs = []
    for shape in [(1, 1, 1), (3, 2, 2), (5, 4, 2), (16, 16, 8)]:
        (A1, l1, u1, A2, l2, u2), pi, pj = _family_pairs(shape)
        first = [(A1[k], l1[k], u1[k]) for k in range(48)]; second = [(A2[k], l2[k], u2[k]) for k in range(48)]
        pairs += [(first[a], second[b]) for a, b in zip(pi, pj)]
    n0, s0 = engine.calls["qpn_issubset_pairs"], _node_solves(engine)
    got = polyhedra.issubset_batch(pairs, engine)
    assert engine.calls["qpn_issubset_pairs"] - n0 == 4 and _node_solves(engine) == s0        # a call per pair of shapes, no node solve
    want = polyhedra.issubset_batch(pairs, _WithoutPairs(engine))
    assert engine.calls["qpn_issubset_pairs"] - n0 == 4 and _node_solves(engine) > s0
    assert np.array_equal(got, want) and got.any() and not got.all()
    assert np.array_equal(polyhedra.issubset_batch_chunked(pairs, engine, chunk_bytes=4000), want)
    assert engine.calls["qpn_issubset_pairs"] - n0 > 8


def test_remove_subsets_many_keeps_the_same_lists(engine):
    from qpn_amd import algorithm, examples, polyhedra
    seen = []
    orig = algorithm.remove_subsets_many

    def recording(lists, eng, *a, **k):
        seen.append([None if polys is None else list(polys) for polys in lists])
        return orig(lists, eng, *a, **k)
    algorithm.remove_subsets_many = recording
    try:
        ret = algorithm.solve(examples.setup("synthetic_pairs", pairs=12, n=8, m=8), engine=engine)
    finally:
        algorithm.remove_subsets_many = orig
    assert ret["solved"] and seen
    n0 = engine.calls["qpn_issubset_pairs"]
    for prefilter in (True, False):
        for lists in seen:
            got = polyhedra.remove_subsets_many(lists, engine, prefilter=prefilter)
            want = polyhedra.remove_subsets_many(lists, _WithoutPairs(engine), prefilter=prefilter)
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert (g is None and w is None) or [id(P) for P in g] == [id(P) for P in w]
    assert engine.calls["qpn_issubset_pairs"] > n0


def test_solve_end_to_end_with_and_without_the_entry(engine):
    from qpn_amd import algorithm, examples
    n0 = engine.calls["qpn_issubset_pairs"]
    on = algorithm.solve(examples.setup("robust_avoid_simple", seed=1), engine=engine)
    assert engine.calls["qpn_issubset_pairs"] > n0
    off = algorithm.solve(examples.setup("robust_avoid_simple", seed=1), engine=_WithoutPairs(engine))
    assert on["solved"] and off["solved"]
    assert np.max(np.abs(on["x_opt"] - off["x_opt"])) <= 1e-9
