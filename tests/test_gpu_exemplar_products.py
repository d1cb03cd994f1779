"""qpn_exemplar_products (csrc/qpn_lp.hip) against its numpy twin polyhedra.exemplar_products_host, bit for bit
on every output, in every kernel class and both memory modes, on the cut polyhedra of tests/products_cases.py; against
qpn_exemplar_polys on the stacked polyhedra; its closure test, its argument errors and its bad factors; and the host functions that
use it -- combine_at with route="products" against route="polyhedron", solve() end to end with qp_processing.EMPTINESS_ROUTE switched."""
from __future__ import annotations

import numpy as np
import pytest

import exemplar_cases
import goldenio as G
import products_cases
from exemplar_cases import FAILURE, TOL
from products_cases import POINT_TOL

pytestmark = pytest.mark.gpu

INF = np.inf
NOT_NEAR = 6
OUTPUTS = ("near",) + exemplar_cases.OUTPUTS


def _same_bits(got, want, what):
    exemplar_cases.same_bits(got, want, what)
    g = got["near"].cpu().numpy() if hasattr(got["near"], "cpu") else np.asarray(got["near"])
    assert g.dtype == np.uint8 and np.array_equal(g, want["near"]), (what, "near", g, want["near"])


def _dev(engine, a, dtype):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=f"cuda:{engine.device}")


def _both_modes(engine, pool, piece_row, factors, n, point=None, point_of=None, want=None, device_twin=False, **kw):
    """The kernel in host and in device mode against the twin (`want`: a twin answer the caller has).  -> the twin's answer."""
    from qpn_amd import polyhedra
    A, l, u, ol, oh = pool
    if want is None:
        want = polyhedra.exemplar_products_host(A, l, u, ol, oh, piece_row, factors, n, point=point, point_of=point_of, device=device_twin, **kw)
    if not device_twin:
        _same_bits(engine.exemplar_products(A, l, u, ol, oh, piece_row, factors, n, point=point, point_of=point_of, **kw), want, "host mode")
    f, b, i = (lambda a: _dev(engine, a, np.float64)), (lambda a: _dev(engine, a, np.uint8)), (lambda a: _dev(engine, a, np.int32))
    got = engine.exemplar_products(f(A), f(l), f(u), b(ol), b(oh), i(piece_row), i(factors), n, point=f(point), point_of=i(point_of), **kw)
    assert all(hasattr(v, "cpu") for v in got.values()) and sorted(got) == sorted(OUTPUTS)
    _same_bits(got, want, "device mode")
    return want


@pytest.mark.parametrize("shape", [(3, 2), (8, 4), (24, 8)])
def test_the_family_equals_the_twin_and_the_polyhedron_entry_bit_for_bit(engine, shape):
    """50 cut products, the five kinds and k = 1, 2, 3, 5 mixed; the same question as ONE polyhedron each through
    qpn_exemplar_polys: two GPU entries, one LP."""
    from qpn_amd.engine import colmajor
    n, d = shape
    assert engine.lp_kernel_class(2 * n + 1, d + 1) == 0
    c = products_cases.cut_batch(shape, 50)
    n0 = engine.calls["qpn_exemplar_products"]
    want = _both_modes(engine, c["pool"], c["piece_row"], c["factors"], n, tol=TOL)
    assert engine.calls["qpn_exemplar_products"] == n0 + 2
    assert np.array_equal(want["how"], c["how"]) and np.array_equal(want["empty"].astype(bool), c["empty"]) and want["near"].all()
    A, l, u, ol, oh = c["whole"]
    exemplar_cases.same_bits(engine.exemplar_polys(colmajor(A), l, u, ol, oh, tol=TOL), want, "qpn_exemplar_polys on the stacked rows")
    cut = _both_modes(engine, c["pool"], c["piece_row"], c["factors"], n, tol=TOL, opts=dict(max_iters=1))
    if shape == (24, 8):
        assert want["iters"].max() > 20
        assert np.all(cut["how"] == exemplar_cases.ITER_LIMIT) and np.all(cut["iters"] == 1) and cut["near"].all() and not cut["lam"].any()


def _class_shapes(engine):
    """tests/test_gpu_exemplar.py's: (the largest wave-class n, the smallest workgroup-class n) at d = 12 and the smallest
    workspace-class n at d = 24; the class of a job is that of its slack LP, 2 n + 1 rows in d + 1 variables."""
    n0 = max(n for n in range(1, 120) if engine.lp_kernel_class(2 * n + 1, 13) == 0)
    n2 = min(n for n in range(1, 512) if engine.lp_kernel_class(2 * n + 1, 25) == 2)
    return (n0, 12), (n0 + 1, 12), (n2, 24)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_class_boundaries_equal_the_twin_bit_for_bit(engine, which):
    n, d = _class_shapes(engine)[which]
    cls = lambda n: engine.lp_kernel_class(2 * n + 1, d + 1)
    assert cls(n) == which and (which == 0 or cls(n - 1) == which - 1) and (which != 0 or cls(n + 1) == 1)
    c = products_cases.cut_batch((n, d), 3 if which == 2 else 5, first=2 if which == 2 else 0, ks=(3,))
    assert ((c["factors"] >= 0).sum(1) == 3).all()
    want = _both_modes(engine, c["pool"], c["piece_row"], c["factors"], n, tol=TOL)
    assert np.array_equal(want["how"], c["how"]) and want["iters"].min() > 3 and want["near"].all()


def test_workspace_class_runs_a_second_chunk(engine):
    """More products of the workspace class than one chunk of the workspace holds.  A job takes its slice (more than 156 KiB in this
    class) and its region (the rows of its slack LP, (2 n + 1) (d + 1) + 2 (2 n + 1) doubles, and the n int32 of its row map) and a
    chunk is 256 MiB, so the count below is more than a chunk holds and the launcher's second chunk runs.  The pool holds five cut
    polyhedra, one of each kind, asked in turn: the twin solves five, every job equals its own."""
    from qpn_amd import polyhedra
    n, d = _class_shapes(engine)[2]
    region_bytes = ((2 * n + 1) * (d + 1) + 2 * (2 * n + 1)) * 8 + 4 * n
    count = (256 << 20) // ((156 << 10) + region_bytes) + 5
    assert engine.lp_kernel_class(2 * n + 1, d + 1) == 2 and 500 < count < 1000
    c = products_cases.cut_batch((n, d), 5, first=10, ks=(3,))
    five = polyhedra.exemplar_products_host(*c["pool"], c["piece_row"], c["factors"], n, tol=TOL)
    assert np.array_equal(five["how"], c["how"])
    t = np.arange(count) % 5
    want = {k: np.ascontiguousarray(v[t]) for k, v in five.items()}
    _both_modes(engine, c["pool"], c["piece_row"], np.ascontiguousarray(c["factors"][t]), n, want=want, tol=TOL)


def test_near_and_not_near_products_in_one_call(engine):
    """The `fat` polyhedra of a batch at their own point and at a point 0.01 beyond one bound (margins of 1e-3 against point_tol =
    1e-6), the other kinds at their own point -- which `gap` puts 1 beyond the upper bound of its row 0, and the thin kinds on a
    bound; two points with point_of choosing between them; and NULL points."""
    shape = (8, 4)
    n, d = shape
    c = products_cases.cut_batch(shape, 20)
    A, l, u, _, _ = c["whole"]
    points, point_of, factors, rows = [], [], [], []
    for t in range(20):
        kind = exemplar_cases.KINDS[t % 5]
        x0 = products_cases.plant_x0(t, n, d, kind)
        factors.append(c["factors"][t]); point_of.append(len(points)); points.append(x0); rows.append(1 if kind == "gap" else -1)
        if kind == "fat":
            p, row = products_cases.closure_points(A[t], l[t], u[t], x0)
            factors.append(c["factors"][t]); point_of.append(len(points)); points.append(p); rows.append(row)
    factors = np.array(factors, np.int32); points = np.array(points); point_of = np.array(point_of, np.int32); rows = np.array(rows)
    want = _both_modes(engine, c["pool"], c["piece_row"], factors, n, point=points, point_of=point_of, point_tol=POINT_TOL, tol=TOL)
    off = rows >= 0
    assert off.sum() == 8 and np.array_equal(want["near"], (~off).astype(np.uint8)) and np.array_equal(want["row"][off], rows[off])
    assert np.all(want["how"][off] == NOT_NEAR) and not want["iters"][off].any() and np.isnan(want["eps"][off]).all()
    assert not want["x"][off].any() and not want["lam"][off].any() and want["iters"][~off].min() > 0
    # two points, point_of choosing: the first fat polyhedron's own point and its point beyond the bound
    fat0 = 1                                      # (product 0 is the first fat polyhedron at its own point, product 1 beyond the bound)
    assert rows[0] == -1 and rows[1] >= 0
    two = points[[fat0 - 1, fat0]]
    pick = (np.arange(len(factors)) % 2).astype(np.int32)
    same = np.ascontiguousarray(np.repeat(factors[fat0][None], len(factors), axis=0))
    got = _both_modes(engine, c["pool"], c["piece_row"], same, n, point=two, point_of=pick, point_tol=POINT_TOL, tol=TOL)
    assert np.array_equal(got["near"], (1 - pick).astype(np.uint8)) and np.all(got["row"][pick == 1] == rows[fat0])
    # NULL points: no closure test
    none = _both_modes(engine, c["pool"], c["piece_row"], factors, n, tol=TOL)
    assert none["near"].all() and none["iters"].min() > 0


def test_argument_errors_null_flags_and_bad_factors(engine):
    from qpn_amd import polyhedra
    from qpn_amd.engine import QpnError
    c = products_cases.cut_batch((3, 2), 10)
    pool, pr, fac, n = c["pool"], c["piece_row"], c["factors"], c["n"]
    A, l, u, ol, oh = pool
    # sizes beyond the limits
    one = lambda d: (np.zeros((1, d)), np.zeros(1), np.ones(1), None, None, np.array([0, 1], np.int32))
    for args in ((*one(2), np.zeros((1, 1), np.int32), 512), (*one(256), np.zeros((1, 1), np.int32), 1), (*one(2), np.zeros((1, 33), np.int32), 1)):
        with pytest.raises(QpnError, match="size"):
            engine.exemplar_products(*args)
    # inconsistent shapes
    for bad in ((A, l[:3], u, ol, oh, pr, fac, n), (A, l, u, ol[:4], oh, pr, fac, n), (A[0], l, u, ol, oh, pr, fac, n), (A, l, u, ol, oh, pr, fac[0], n)):
        with pytest.raises(QpnError, match="inconsistent shapes"):
            engine.exemplar_products(*bad)
    for kw in (dict(point=np.zeros((1, 2))), dict(point=np.zeros((1, 3)), point_of=np.zeros(10, np.int32)),
               dict(point=np.zeros((1, 2)), point_of=np.zeros(9, np.int32))):
        with pytest.raises(QpnError, match="inconsistent shapes"):
            engine.exemplar_products(*pool, pr, fac, n, **kw)
    # host factors out of range, rows that do not add up, a point_of out of range: an argument error
    pieces = len(pr) - 1
    for value in (pieces, -2):
        f = fac.copy(); f[3, np.nonzero(f[3] >= 0)[0][0]] = value
        with pytest.raises(QpnError, match="bad argument"):
            engine.exemplar_products(*pool, pr, f, n)
    with pytest.raises(QpnError, match="bad argument"):
        engine.exemplar_products(*pool, pr, fac, n + 1)
    with pytest.raises(QpnError, match="bad argument"):
        engine.exemplar_products(*pool, pr, fac, n, point=np.zeros((1, 2)), point_of=np.ones(10, np.int32))
    # no product
    got = engine.exemplar_products(*pool, pr, np.zeros((0, 3), np.int32), n)
    assert got["near"].shape == (0,) and got["lam"].shape == (0, 7)
    # null flags mean closed: the answer of zero flags, and of one array alone
    zero = np.zeros_like(ol)
    closed = _both_modes(engine, (A, l, u, None, None), pr, fac, n, tol=TOL)
    _same_bits(closed, polyhedra.exemplar_products_host(A, l, u, zero, zero, pr, fac, n, tol=TOL), "zero flags")
    assert np.all(closed["row"] == -1) and not closed["empty"][c["how"] == exemplar_cases.EMPTY_OPEN].any()
    _both_modes(engine, (A, l, u, ol, None), pr, fac, n, tol=TOL)
    _both_modes(engine, (A, l, u, None, oh), pr, fac, n, tol=TOL)
    # device arrays: a factor of `pieces` and one of -2, a point_of out of range: those products alone fail, with zeros
    f = fac.copy()
    f[3, np.nonzero(f[3] >= 0)[0][0]] = pieces; f[6, np.nonzero(f[6] >= 0)[0][0]] = -2
    good = polyhedra.exemplar_products_host(*pool, pr, fac, n, tol=TOL)
    got = _both_modes(engine, pool, pr, f, n, device_twin=True, tol=TOL)
    rest = np.delete(np.arange(10), [3, 6])
    exemplar_cases.same_bits({k: np.ascontiguousarray(got[k][rest]) for k in exemplar_cases.OUTPUTS},
                             {k: np.ascontiguousarray(good[k][rest]) for k in exemplar_cases.OUTPUTS}, "the rest")
    assert np.all(got["how"][[3, 6]] == FAILURE) and not got["near"][[3, 6]].any() and not got["x"][[3, 6]].any() and not got["lam"][[3, 6]].any()
    x0 = np.zeros((1, 2))
    pof = np.zeros(10, np.int32); pof[2] = 1; pof[8] = -1
    got = _both_modes(engine, pool, pr, fac, n, point=x0, point_of=pof, device_twin=True, point_tol=1e3, tol=TOL)     # (every product is near)
    assert np.all(got["how"][[2, 8]] == FAILURE) and np.array_equal(np.delete(got["how"], [2, 8]), np.delete(good["how"], [2, 8]))


# ---- the host functions on the products route against the polyhedron route --------------------------------------------------------
def _node_solves(engine):
    return sum(v for k, v in engine.calls.items() if k.startswith("qpn_solve_nodes") or k == "qpn_solve_avi_batch")


def _counts(engine):
    return engine.calls["qpn_exemplar_products"], engine.calls["qpn_exemplar_polys"], engine.calls["qpn_solve_lps"], _node_solves(engine)


def test_combine_at_on_the_kink_by_products_equals_the_polyhedron_route(engine):
    """tests/test_level_batch.py's hand-worked kink: route="products" returns the pieces of route="polyhedron", the same rows, bounds
    and flags in the same order, with the closure and the emptiness tests on qpn_exemplar_products alone."""
    from qpn_amd.programs import Poly
    from qpn_amd.qp_processing import combine_at
    R1 = Poly(np.array([[0.0, 1.0], [1.0, 0.0]]), [0.0, -INF], [0.0, 0.0])
    R2 = Poly(np.array([[1.0, -1.0], [0.0, 1.0]]), [0.0, 0.0], [0.0, INF])
    S1 = Poly(np.array([[0.0, 1.0], [1.0, 0.0]]), [0.0, -INF], [0.0, 0.0])
    S2 = Poly(np.array([[1.0, 0.0], [0.0, 1.0]]), [0.0, 0.0], [0.0, 0.0])
    want = combine_at([[R1], [R2]], [[S1], [S2]], np.zeros(2), engine, route="polyhedron")
    before = _counts(engine)
    out = combine_at([[R1], [R2]], [[S1], [S2]], np.zeros(2), engine, route="products")
    after = _counts(engine)
    assert after[0] > before[0] and after[1:] == before[1:]
    assert len(out) == len(want) >= 2
    for P, Q in zip(out, want):
        for a, b in zip(P.vectorize() + (P.open_lo, P.open_hi), Q.vectorize() + (Q.open_lo, Q.open_hi)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    inside = lambda pt: any(P.contains(np.array(pt, float), tol=1e-9) for P in out)
    assert inside((0.0, 0.0)) and inside((-1.0, 0.0)) and not inside((1.0, 1.0)) and not inside((1.0, 0.5)) and not inside((-1.0, 1.0))


def test_reference_end_to_end_cases_on_the_products_route(engine, monkeypatch):
    """tests/test_gpu_host_logic.py's test_reference_end_to_end_cases_on_gpu with qp_processing.EMPTINESS_ROUTE = "products": the same
    assertions, and every combine_many asks its questions of qpn_exemplar_products alone."""
    from qpn_amd import algorithm, examples, qp_processing
    from qpn_amd.qp_processing import local_recipe_count
    assert qp_processing.EMPTINESS_ROUTE == "nodes"
    monkeypatch.setattr(qp_processing, "EMPTINESS_ROUTE", "products")
    inner = qp_processing.combine_many
    ran = []

    def counted(jobs, x, eng, **kw):
        before = _counts(engine)
        out = inner(jobs, x, eng, **kw)
        ran.append(tuple(a - b for a, b in zip(_counts(engine), before)))
        return out

    monkeypatch.setattr(qp_processing, "combine_many", counted)
    c = G.load("simple_bilevel_cases.json")
    assert len(c["w"]) == 8
    for w, xs, min_pieces in zip(c["w"], c["accepted_xy"], c["min_pieces_root_graph"]):
        net = examples.setup("simple_bilevel", gen_solution_map=True)
        ret = algorithm.solve(net, np.array(list(w) + c["x0"], float), engine=engine)
        assert ret["solved"], ret
        assert any(np.allclose(ret["x_opt"], list(w) + list(xy), atol=c["atol"]) for xy in xs), (w, ret["x_opt"])
        assert len(ret["Sol"][2]) >= min_pieces, (w, len(ret["Sol"][2]))
        assert local_recipe_count(net, 2, ret["x_opt"], ret["Sol"], engine=engine) >= min_pieces, w
    print("combine_many calls (exemplar_products, exemplar_polys, solve_lps, node solves):", ran)
    assert ran and all(ex == 0 and lp == 0 and nodes == 0 for _, ex, lp, nodes in ran)
    assert any(pr >= 1 for pr, _, _, _ in ran)
