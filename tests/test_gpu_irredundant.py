"""qpn_irredundant_bounds (csrc/qpn_lp.hip) against its numpy twin polyhedra_host.irredundant_bounds_host, bit for bit on every output,
in every kernel class and both memory modes; its argument errors; and polyhedra.irredundant_batch and solve() with
QPNetOptions.irredundant_pieces on the HIP engine against the same on the twin engine."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import irredundant_cases as ic

pytestmark = pytest.mark.gpu


def _both_modes(engine, A, l, u, **kw):
    """The kernel in host and in device mode against the twin.  -> the twin's answer."""
    import torch
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    host = (colmajor(A), l, u)
    want = polyhedra.irredundant_bounds_host(*host, **kw)
    ic.same_bits(engine.irredundant_bounds(*host, **kw), want, "host mode")
    dv = f"cuda:{engine.device}"
    got = engine.irredundant_bounds(*(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dv) for a in host), **kw)
    assert all(hasattr(v, "cpu") for v in got.values())
    ic.same_bits(got, want, "device mode")
    return want


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (8, 4), (16, 8)])
def test_the_planted_family_equals_the_twin_bit_for_bit(engine, shape):
    """50 polyhedra: the last workgroup of the wavefront class holds two of its four."""
    from qpn_amd import _lib
    n0 = engine.calls["qpn_irredundant_bounds"]
    A, l, u = ic.planted_batch(shape, range(50))
    r = A.shape[1]
    assert engine.lp_kernel_class(r, shape[1]) == 0
    want = _both_modes(engine, A, l, u)
    assert engine.calls["qpn_irredundant_bounds"] == n0 + 2
    assert np.all(want["status"] == _lib.IB_OK) and np.all(np.isinf(want["ur"][:, r - 3:])) and np.array_equal(want["ur"][:, :r - 3], u[:, :r - 3])
    cut = _both_modes(engine, A, l, u, opts=dict(max_iters=1))
    if shape == (16, 8):
        assert _lib.IB_ITER_LIMIT in cut["status"] and want["iters"].max() > 3


def _class_shapes(engine):
    """(tests/test_gpu_implicit_bounds.py's, stated again) the largest wave-class r, the smallest workgroup-class r, the smallest
    workspace-class r, at d = 24, 24, 128."""
    r0 = max(r for r in range(1, 200) if engine.lp_kernel_class(r, 24) == 0)
    r2 = min(r for r in range(1, 1025) if engine.lp_kernel_class(r, 128) == 2)
    return (r0, 24), (r0 + 1, 24), (r2, 128)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_class_boundaries_equal_the_twin_bit_for_bit(engine, which):
    from qpn_amd import _lib
    r, d = _class_shapes(engine)[which]
    assert engine.lp_kernel_class(r, d) == which and (which == 0 or engine.lp_kernel_class(r - 1, d) == which - 1)
    A, l, u = ic.one_sided_batch(17 + which, 2, r, d)
    want = _both_modes(engine, A, l, u)
    assert np.all(want["status"] == _lib.IB_OK) and np.all(want["lps"] == 1 + r) and want["iters"].max() > 3
    implied = ic.implied_rows(r, d)
    assert np.all(np.isinf(want["ur"][:, implied]))                                  # the rows made to be implied go
    seen = set(want["how"][:, :, 1].ravel().tolist())
    assert {_lib.RED_KEPT_BY_OPTIMUM, _lib.RED_REMOVED} <= seen


def test_the_hand_cases_equal_the_twin_bit_for_bit(engine):
    from qpn_amd import _lib
    A, l, u = ic.hand_batch()
    want = _both_modes(engine, A, l, u)
    assert want["status"].tolist() == [_lib.IB_OK] * 4 + [_lib.IB_EMPTY] * 2
    seen = set(want["how"].ravel().tolist())
    assert seen == {_lib.RED_UNDECIDED, _lib.RED_NONE, _lib.RED_KEPT_EQUALITY, _lib.RED_REMOVED_ZERO_ROW, _lib.RED_KEPT_UNBOUNDED,
                    _lib.RED_KEPT_BY_OPTIMUM, _lib.RED_REMOVED}
    cut = _both_modes(engine, A, l, u, opts=dict(max_iters=1))
    k = list(ic.HAND).index("one side")
    assert cut["status"][k] == _lib.IB_ITER_LIMIT and cut["fail_row"][k] == 3
    assert np.array_equal(cut["lr"][k], l[k]) and np.array_equal(cut["ur"][k], u[k]) and np.all(cut["how"][k] == _lib.RED_UNDECIDED)


def test_the_projected_pieces_equal_the_twin_bit_for_bit(engine):
    """project_cases' pieces up to 130 rows (irredundant_cases.pieces: the 1101-row piece is beyond the kernel's limits and stands
    here as its first step's input), one call per piece; two of them are empty."""
    from qpn_amd import _lib
    classes, status = set(), []
    for name, A, l, u in ic.pieces():
        classes.add(engine.lp_kernel_class(*A.shape))
        status.append(int(_both_modes(engine, A[None], l[None], u[None])["status"][0]))
    assert classes == {0, 1} and status.count(_lib.IB_EMPTY) == 2 and status.count(_lib.IB_OK) == len(status) - 2


def test_more_workspace_jobs_than_one_chunk_holds(engine):
    """The launcher's second launch: the two workspace-class polytopes of the boundary test, repeated until they pass the 256 MiB
    chunk; every job answers what the twin answers for its polytope."""
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    r, d = _class_shapes(engine)[2]
    A, l, u = ic.one_sided_batch(19, 2, r, d)
    want = polyhedra.irredundant_bounds_host(colmajor(A), l, u)
    slice_bytes = 8 * (((r + 1) | 1) * d + (r + 1) + 5 * d + 8 * r + 8) + 4 * (r + d)
    assert slice_bytes > 156 << 10
    reps = ((256 << 20) // slice_bytes) // 2 + 3                                      # 2 reps jobs: the chunk and a few more
    got = engine.irredundant_bounds(np.tile(colmajor(A), (reps, 1, 1)), np.tile(l, (reps, 1)), np.tile(u, (reps, 1)))
    assert 2 * reps > (256 << 20) // slice_bytes
    ic.same_bits(got, {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in want.items()}, "two launches")


def test_argument_errors_and_edge_cases(engine):
    from qpn_amd import polyhedra
    from qpn_amd._lib import MEM_HOST
    from qpn_amd.engine import QpnError, colmajor
    for r, d in ((1025, 2), (2, 257)):                                               # sizes beyond the limits
        with pytest.raises(QpnError, match="size"):
            engine.irredundant_bounds(np.zeros((1, d, r)), np.zeros((1, r)), np.ones((1, r)))
    A, l, u = ic.planted_batch((3, 2), range(4))
    for bad in ((colmajor(A), l[:3], u), (colmajor(A), l, u[:, :2]), (colmajor(A)[0], l, u)):
        with pytest.raises(QpnError, match="inconsistent shapes"):
            engine.irredundant_bounds(*bad)
    got = engine.irredundant_bounds(np.zeros((0, 2, 3)), np.zeros((0, 3)), np.zeros((0, 3)))   # no polyhedron
    assert got["status"].shape == (0,) and got["lr"].shape == (0, 3) and got["how"].shape == (0, 3, 2)
    # the optional outputs left out: the others are those of the full call
    want = polyhedra.irredundant_bounds_host(colmajor(A), l, u)
    r = A.shape[1]
    Ac = np.ascontiguousarray(colmajor(A)); status = np.full(4, -7, np.int32); lr = np.zeros((4, r)); ur = np.zeros((4, r))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = engine.lib.qpn_irredundant_bounds(engine.ctx, 4, r, 2, p(Ac), p(l), p(u), 1e-8, None, p(status), None, p(lr), p(ur), None, None, None,
                                           None, MEM_HOST)
    assert rc == 0
    assert np.array_equal(status, want["status"]) and lr.tobytes() == want["lr"].tobytes() and ur.tobytes() == want["ur"].tobytes()
    # a required output missing
    assert engine.lib.qpn_irredundant_bounds(engine.ctx, 4, r, 2, p(Ac), p(l), p(u), 1e-8, None, p(status), None, None, p(ur), None, None, None,
                                             None, MEM_HOST) != 0


# ---- the front end and solve() on the HIP engine against the same on the twin engine ----------------------------------------------
def _key(p):
    return tuple((a.dtype.str, a.shape, a.tobytes()) for a in (*(np.asarray(v) for v in p.vectorize()), *p.open_bounds()))


def test_irredundant_batch_on_the_hip_engine(engine):
    from qpn_amd import polyhedra
    items = [(A, l, u) for _, A, l, u in ic.pieces()] + [ic.planted(8, 4, s)[:3] for s in range(6)] + [ic.HAND[k] for k in ic.HAND]
    n0 = engine.calls["qpn_irredundant_bounds"]
    got = polyhedra.irredundant_batch(items, engine)
    assert engine.calls["qpn_irredundant_bounds"] - n0 == len({np.atleast_2d(A).shape for A, _, _ in items})   # one call per shape
    want = polyhedra.irredundant_batch(items, ic.red_twin_engine())
    assert len(got) == len(want) == len(items)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is items[k]) == (w is items[k]), k
        if g is not items[k]:
            assert _key(g) == _key(w), k
    assert sum(g is not p for g, p in zip(got, items)) >= 12


def test_solve_with_irredundant_pieces_on_the_hip_engine(engine):
    from qpn_amd import algorithm, examples
    n0 = engine.calls["qpn_irredundant_bounds"]
    off = algorithm.solve(examples.setup("robust_avoid_simple", seed=1), engine=engine)
    assert engine.calls["qpn_irredundant_bounds"] == n0                              # off: the entry is not called
    on = algorithm.solve(examples.setup("robust_avoid_simple", seed=1, irredundant_pieces=True), engine=engine)
    assert engine.calls["qpn_irredundant_bounds"] > n0
    want = algorithm.solve(examples.setup("robust_avoid_simple", seed=1, irredundant_pieces=True), engine=ic.red_twin_engine())
    assert on["solved"] and off["solved"] and want["solved"]
    print("x_opt on the HIP engine - on the twin engine:", float(np.max(np.abs(on["x_opt"] - want["x_opt"]))),
          " on - off:", float(np.max(np.abs(on["x_opt"] - off["x_opt"]))))
    assert sorted(on["Sol"]) == sorted(want["Sol"])
    rows_on = rows_off = 0
    for pid in sorted(want["Sol"]):
        a, b = on["Sol"][pid], want["Sol"][pid]
        assert (a is None) == (b is None)
        if a is not None:
            assert [_key(p) for p in a] == [_key(p) for p in b], pid                 # the same pieces in the same order
            rows_on += sum(len(p) for p in a); rows_off += sum(len(p) for p in off["Sol"][pid])
    assert rows_on < rows_off
    assert on["x_opt"].tobytes() == want["x_opt"].tobytes()
    assert np.max(np.abs(on["x_opt"] - off["x_opt"])) <= 1e-9
