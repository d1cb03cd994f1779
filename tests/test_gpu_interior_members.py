"""Interior members of polyhedra with the node records made on the MI355X: qpn_assemble_interior_nodes
against its numpy twin bit for bit, qpn_interior_members against solve_nodes over the twin's records in every size class of the
node solver, qpn_members_outside against its twin, both memory modes; remove_subsets_many and solve() with and without the new
entries.  The CPU side is tests/test_interior_members_host.py."""
import numpy as np
import pytest

from qpn_amd import algorithm, examples, polyhedra
from qpn_amd.engine import QpnError, colmajor

pytestmark = pytest.mark.gpu

INF = np.inf
DELTA = 1e-2


def polys(seed, B, r, d, n_eq, one_sided=0.0, ragged=True):
    """B polyhedra of r rows in d variables with a common interior point each: up to n_eq equality rows (fewer on some items
    when ragged), the other rows two-sided, or with probability one_sided open on one side; a few rows open on both."""
    g = np.random.default_rng(seed)
    A = g.standard_normal((B, r, d))
    s = np.einsum("brd,bd->br", A, g.standard_normal((B, d)))
    l = s - g.uniform(0.2, 1.0, (B, r)); u = s + g.uniform(0.2, 1.0, (B, r))
    for b in range(B):
        k = n_eq - (b % 3 if ragged and n_eq >= 2 else 0)
        E = g.choice(r, k, replace=False) if k else []
        l[b, E] = u[b, E] = s[b, E]
        for i in range(r):
            if i in E:
                continue
            v = g.uniform()
            if v < one_sided / 2:
                l[b, i] = -INF
            elif v < one_sided:
                u[b, i] = INF
            elif ragged and v > 0.97:
                l[b, i] = -INF; u[b, i] = INF
    return A, l, u


def to_dev(engine, *arrs):
    import torch
    return tuple(torch.as_tensor(np.ascontiguousarray(a), device=f"cuda:{engine.device}") for a in arrs)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


# (r, d, equality rows, share of one-sided rows): from one row in one variable to 256 rows in 128
ASSEMBLE = [(1, 1, 0, 0.0), (1, 1, 1, 0.0), (3, 2, 1, 0.5), (10, 6, 2, 0.3), (24, 20, 3, 0.0), (64, 64, 32, 0.0), (70, 5, 4, 0.6),
            (130, 9, 0, 1.0), (300, 40, 20, 0.9), (256, 128, 10, 1.0)]


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("r,d,n_eq,one_sided", ASSEMBLE)
def test_assembly_equals_the_numpy_twin(engine, r, d, n_eq, one_sided, dev):
    B = 5
    A, l, u = polys(r * 1000 + d, B, r, d, n_eq, one_sided, ragged=(r, d) != (64, 64))
    ne, nlo, nhi = polyhedra.interior_member_counts(l, u)
    if (r, d) == (64, 64):
        assert (ne, nlo, nhi) == (32, 32, 32)                   # the traced shape: records of (97, 64)
    want = polyhedra.interior_member_records(A, l, u, DELTA)
    args = (colmajor(A), l, u)
    got = engine.assemble_interior_nodes(*(to_dev(engine, *args) if dev else args), DELTA, ne, nlo, nhi)
    for name, w, g in zip(("Qc", "qd", "Ac", "l", "u"), want, got[:5]):
        g = host(g)
        assert g.shape == w.shape and np.array_equal(g, w), name
    assert not host(got[5]).any()


# (r, d, equality rows, one-sided share) -> the class of the record (nf, mp) in the node solver
SOLVE = {"32-class": (10, 6, 2, 0.3), "33-48": (24, 20, 3, 0.0), "49-64": (30, 40, 2, 0.0), "65-128 (97, 64)": (64, 64, 32, 0.0),
         "above 128": (256, 128, 10, 1.0)}
WANT_MAX = {"32-class": (1, 32), "33-48": (33, 48), "49-64": (49, 64), "65-128 (97, 64)": (65, 128), "above 128": (129, 1024)}


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("cls", list(SOLVE))
def test_members_equal_solve_nodes_on_the_twin_records(engine, cls, dev):
    r, d, n_eq, one_sided = SOLVE[cls]
    B = 6 if cls == "above 128" else 40
    A, l, u = polys(7 + r, B, r, d, n_eq, one_sided, ragged=cls != "65-128 (97, 64)")
    i0, i1 = np.nonzero(l[1] != u[1])[0][:2]                 # one empty item: two of its inequality rows say a'x >= 1 and a'x <= 0
    A[1, i1] = A[1, i0]; l[1, i0] = 1.0; u[1, i0] = INF; l[1, i1] = -INF; u[1, i1] = 0.0
    ne, nlo, nhi = polyhedra.interior_member_counts(l, u)
    Qc, qd, Ac, ll, uu = polyhedra.interior_member_records(A, l, u, DELTA)
    nf, mp = qd.shape[1], ll.shape[1]
    lo_, hi_ = WANT_MAX[cls]
    assert lo_ <= max(nf, mp) <= hi_, (nf, mp)
    if cls == "65-128 (97, 64)":
        assert (nf, mp) == (97, 64)
    rec = (Qc, np.zeros((B, 1, nf)), qd, Ac, np.zeros((B, 1, mp)), ll, uu, np.zeros(1))
    args = (colmajor(A), l, u)
    if dev:
        rec = to_dev(engine, *rec); args = to_dev(engine, *args)
    res = engine.solve_nodes(*rec)
    st = host(res["status"]); z = host(res["z"])
    want_ok = (st == 1) & (z[:, d] <= 1e-6)
    x, ok, status = (host(a) for a in engine.interior_members(*args, DELTA, ne, nlo, nhi))
    assert np.array_equal(status, st)
    assert np.array_equal(ok.astype(bool), want_ok)
    assert np.array_equal(x[want_ok], z[want_ok, :d])        # bit for bit
    assert want_ok.sum() >= B - 1 and not want_ok[1]         # the empty item has no member, the others do
    for b in np.nonzero(want_ok)[0]:                         # a member: on its equality rows, inside the others
        ax = A[b] @ x[b]
        eq = l[b] == u[b]
        assert np.max(np.abs(ax[eq] - l[b][eq]), initial=0.0) <= 1e-7
        assert np.all(ax[~eq] >= l[b][~eq] - 1e-7) and np.all(ax[~eq] <= u[b][~eq] + 1e-7)


@pytest.mark.parametrize("dev", [False, True])
def test_item_beyond_the_capacities_is_flagged_not_cut_short(engine, dev):
    B, r, d = 6, 9, 4
    A, l, u = polys(5, B, r, d, 2, 0.3, ragged=False)
    l[3, :5] = u[3, :5] = np.where(np.isfinite(l[3, :5]), l[3, :5], 0.0)      # item 3: five equality rows, the others have two
    others = np.arange(B) != 3
    ne, nlo, nhi = polyhedra.interior_member_counts(l[others], u[others])
    assert polyhedra.interior_member_counts(l, u)[0] == 5 > ne == 2
    args = (colmajor(A), l, u)
    if dev:
        args = to_dev(engine, *args)
    Qc, qd, Ac, ll, uu, flag = (host(a) for a in engine.assemble_interior_nodes(*args, DELTA, ne, nlo, nhi))
    assert flag.tolist() == [0, 0, 0, 1, 0, 0]
    # the flagged item's record is the one of a polyhedron without rows; the others are what the twin makes of them
    l2, u2 = l.copy(), u.copy()
    l2[3] = -INF; u2[3] = INF
    for w, g in zip(polyhedra.interior_member_records(A, l2, u2, DELTA), (Qc, qd, Ac, ll, uu)):
        assert np.array_equal(g, w)
    x, ok, status = (host(a) for a in engine.interior_members(*args, DELTA, ne, nlo, nhi))
    assert ok.tolist() == [1, 1, 1, 0, 1, 1]
    for b in np.nonzero(others)[0]:
        ax = A[b] @ x[b]
        eq = l[b] == u[b]
        assert np.max(np.abs(ax[eq] - l[b][eq])) <= 1e-7 and np.all(ax[~eq] >= l[b][~eq] - 1e-7) and np.all(ax[~eq] <= u[b][~eq] + 1e-7)


def test_size_limits(engine):
    A, l, u = polys(1, 1, 4, 3, 0)
    with pytest.raises(QpnError, match="size"):
        engine.interior_members(colmajor(A), l, u, DELTA, 600, 300, 300)


OUTSIDE = [(1, 1, 3), (9, 6, 5), (64, 64, 6), (70, 12, 4), (200, 128, 3), (256, 128, 2), (33, 40, 7)]


@pytest.mark.parametrize("order", ["by_member", "by_piece"])
@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("rj,d,Bj", OUTSIDE)
def test_members_outside_equals_the_numpy_twin(engine, rj, d, Bj, dev, order):
    g = np.random.default_rng(rj * 100 + d)
    A = g.standard_normal((Bj, rj, d))
    Bi = 37
    X = g.standard_normal((Bi, d))
    X[1] = X[0] + 1e-7 * g.standard_normal(d)                   # members next to the one the bounds are built around
    ax = np.einsum("jrd,d->jr", A, X[0])
    wide = g.uniform(0.0, 3.0, (Bj, rj)) * (g.uniform(size=(Bj, rj)) < 0.9)       # a tenth of the rows pass through X[0] itself
    lj = ax - wide; uj = ax + wide
    lj[g.uniform(size=lj.shape) < 0.2] = -INF; uj[g.uniform(size=uj.shape) < 0.2] = INF
    pi = np.repeat(np.arange(Bi), Bj).astype(np.int32); pj = np.tile(np.arange(Bj), Bi).astype(np.int32)
    if order == "by_piece":                                     # runs of pairs over one piece: the kernel's tiles of 16, and their tails
        pi, pj = np.tile(np.arange(Bi), Bj).astype(np.int32), np.repeat(np.arange(Bj), Bi).astype(np.int32)
    t = 1e-5
    Ajc = colmajor(A)
    want = polyhedra.members_outside_host(Ajc, lj, uj, X, pi, pj, t)
    args = (Ajc, lj, uj, X, pi, pj)
    got = host(engine.members_outside(*(to_dev(engine, *args) if dev else args), t))
    print(f"rj={rj} d={d}: {len(pi)} pairs, {int(want.sum())} refuted")
    assert got.dtype == np.uint8 and np.array_equal(got, want)           # every pair: the operation order is the same
    assert 0 < want.sum() < len(want)


def test_members_outside_index_out_of_range(engine):
    A = np.eye(2)[None]; lj = np.zeros((1, 2)); uj = np.ones((1, 2)); X = np.full((2, 2), 0.5)
    Ajc = colmajor(A)
    good = (np.array([0, 1], np.int32), np.array([0, 0], np.int32))
    assert engine.members_outside(Ajc, lj, uj, X, *good, 1e-5).tolist() == [0, 0]
    for pi, pj in ((np.array([0, 2], np.int32), good[1]), (good[0], np.array([0, -1], np.int32))):
        with pytest.raises(QpnError):
            engine.members_outside(Ajc, lj, uj, X, pi, pj, 1e-5)
        # device index arrays are not read back: such a pair answers 1 ("not settled here"), the others are answered
        out = engine.members_outside(*to_dev(engine, Ajc, lj, uj, X, pi, pj), 1e-5)
        assert host(out).tolist() == [0, 1]


class Hidden:
    """The engine without the three new methods: polyhedra.py takes the route it took before them."""

    def __init__(self, engine):
        self._engine = engine

    def __getattr__(self, name):
        if name in ("assemble_interior_nodes", "interior_members", "members_outside"):
            raise AttributeError(name)
        return getattr(self._engine, name)


def test_remove_subsets_many_keeps_the_same_lists(engine):
    seen = []
    orig = algorithm.remove_subsets_many

    def recording(lists, eng, *a, **k):
        seen.append([None if p is None else list(p) for p in lists])
        return orig(lists, eng, *a, **k)
    algorithm.remove_subsets_many = recording
    try:
        ret = algorithm.solve(examples.setup("synthetic_pairs", pairs=12, n=8, m=8), engine=engine)
    finally:
        algorithm.remove_subsets_many = orig
    assert ret["solved"] and seen
    asked = 0
    for lists in seen:
        engine.calls.clear()
        got = polyhedra.remove_subsets_many(lists, engine)
        used = engine.calls["qpn_interior_members"], engine.calls["qpn_members_outside"]
        want = polyhedra.remove_subsets_many(lists, Hidden(engine))
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert (g is None and w is None) or [id(P) for P in g] == [id(P) for P in w]
        if any(p is not None and len(p) >= 2 for p in lists):
            assert used[0] >= 1 and used[1] >= 1
            asked += 1
    assert asked >= 1


def _solve_both(engine, net_of):
    engine.calls.clear()
    new = algorithm.solve(net_of(), engine=engine)
    calls = engine.calls["qpn_interior_members"]
    engine.calls.clear()
    old = algorithm.solve(net_of(), engine=Hidden(engine))
    assert engine.calls["qpn_interior_members"] == 0
    assert new["solved"] and old["solved"]
    assert np.max(np.abs(new["x_opt"] - old["x_opt"])) <= 1e-9
    assert calls > 0
    return calls


def test_solve_synthetic_pairs_with_and_without_the_new_route(engine):
    _solve_both(engine, lambda: examples.setup("synthetic_pairs", pairs=40, n=16, m=16))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_solve_robust_avoid_simple_with_and_without_the_new_route(engine, seed):
    _solve_both(engine, lambda: examples.setup("robust_avoid_simple", seed=seed))
