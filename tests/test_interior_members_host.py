"""Interior members of polyhedra with the records made by the engine, host side; the `-m gpu` twin is
tests/test_gpu_interior_members.py.

What is pinned here:
* polyhedra.interior_member_records (the numpy twin of qpn_assemble_interior_nodes, and the route of engines without it) equals
  a slow per-item construction written from the math of the record: ne = 0, nlo = 0, nhi = 0, rows infinite on both sides,
  ragged class counts inside one batch (idle slots), d = 1;
* remove_subsets_many on an engine that has interior_members and members_outside (a spy built from the two twins over the
  oracle engine) keeps exactly the lists it keeps on the plain oracle engine, calls the two methods, and asks no member query
  through solve_nodes;
* polyhedra.members_outside_host (the numpy twin of qpn_members_outside) against a.x computed exactly (fractions.Fraction) on
  seeded Gaussian pieces, and on hand-made members on a bound and beyond it."""
from fractions import Fraction

import numpy as np
import pytest

import qpn_amd  # noqa: F401
from qpn_amd import algorithm, examples, polyhedra
from qpn_amd.programs import Poly

INF = np.inf
DELTA = 1e-2


def slow_records(A, l, u, delta, ne, nlo, nhi):
    """The record of every item, element by element, in the MATH layout: Qd [nf, nf], qd, Ad [mp, nf], l, u [mp]."""
    B, r, d = A.shape
    nf = d + 1 + ne
    mi = nlo + nhi
    mp = max(16, (mi + 15) // 16 * 16)
    out = []
    for b in range(B):
        E = [i for i in range(r) if np.isfinite(l[b, i]) and l[b, i] == u[b, i]]
        LO = [i for i in range(r) if i not in E and np.isfinite(l[b, i])]
        HI = [i for i in range(r) if i not in E and np.isfinite(u[b, i])]
        assert len(E) <= ne and len(LO) <= nlo and len(HI) <= nhi
        Qd = np.zeros((nf, nf)); qd = np.zeros(nf); Ad = np.zeros((mp, nf)); lo = np.full(mp, -INF); hi = np.full(mp, INF)
        for c in range(d + 1):
            Qd[c, c] = delta
        qd[d] = 1.0
        for k in range(ne):
            if k < len(E):
                for c in range(d):
                    Qd[d + 1 + k, c] = A[b, E[k], c]           # the equality row: a' x = l
                    Qd[c, d + 1 + k] = -A[b, E[k], c]          # ... and -a mu in x's stationarity
                qd[d + 1 + k] = -l[b, E[k]]
            else:
                Qd[d + 1 + k, d + 1 + k] = 1.0                 # an idle multiplier: 1 * mu = 0
        for s, i in enumerate(LO):
            Ad[s, :d] = A[b, i]; Ad[s, d] = 1.0; lo[s] = l[b, i]
        for s, i in enumerate(HI):
            Ad[nlo + s, :d] = A[b, i]; Ad[nlo + s, d] = -1.0; hi[nlo + s] = u[b, i]
        out.append((Qd, qd, Ad, lo, hi))
    return out


def seeded_polyhedra(seed, B, r, d, kind):
    """B polyhedra of r rows in d variables around a common point.  kind: "mixed" (ragged counts of every class, some rows
    infinite on both sides), "no_eq", "no_lo" (no row has a finite lower bound unless it is an equality), "no_hi"."""
    g = np.random.default_rng(seed)
    A = g.standard_normal((B, r, d))
    s = np.einsum("brd,bd->br", A, g.standard_normal((B, d)))
    l = s - g.uniform(0.2, 1.0, (B, r)); u = s + g.uniform(0.2, 1.0, (B, r))
    for b in range(B):
        for i in range(r):
            what = g.integers(0, 5) if kind == "mixed" else {"no_eq": 1, "no_lo": 2, "no_hi": 3}[kind] * int(g.integers(0, 2))
            if what == 0 and kind == "mixed":
                l[b, i] = u[b, i] = s[b, i]
            elif what == 2:
                l[b, i] = -INF
            elif what == 3:
                u[b, i] = INF
            elif what == 4:
                l[b, i] = -INF; u[b, i] = INF
    if kind == "no_lo" or kind == "no_hi":                     # (a few equality rows: the only finite lower / upper bounds)
        l[:, 0] = u[:, 0] = s[:, 0]
        if kind == "no_lo":
            l[:, 1:] = -INF
        else:
            u[:, 1:] = INF
    return A, l, u


@pytest.mark.parametrize("seed,B,r,d,kind", [(1, 6, 9, 4, "mixed"), (2, 5, 7, 1, "mixed"), (3, 4, 6, 3, "no_eq"), (4, 4, 6, 3, "no_lo"),
                                             (5, 4, 6, 3, "no_hi"), (6, 3, 40, 5, "mixed"), (7, 2, 1, 1, "no_eq")])
def test_records_equal_a_slow_construction(seed, B, r, d, kind):
    A, l, u = seeded_polyhedra(seed, B, r, d, kind)
    ne, nlo, nhi = polyhedra.interior_member_counts(l, u)
    if kind == "no_eq":
        assert ne == 0
    if kind == "no_lo":
        assert nlo == 0 and ne > 0
    if kind == "no_hi":
        assert nhi == 0 and ne > 0
    if kind == "mixed" and B > 2 and r > 5:
        eq = np.isfinite(l) & (l == u)
        assert len(set(eq.sum(1).tolist())) > 1                # ragged: some item has idle multiplier slots
        assert np.any(np.isinf(l) & np.isinf(u))               # rows infinite on both sides
    Qc, qd, Ac, ll, uu = polyhedra.interior_member_records(A, l, u, DELTA)
    nf = d + 1 + ne
    mp = max(16, (nlo + nhi + 15) // 16 * 16)
    assert Qc.shape == (B, nf, nf) and qd.shape == (B, nf) and Ac.shape == (B, nf, mp) and ll.shape == uu.shape == (B, mp)
    for b, (Qd, q, Ad, lo, hi) in enumerate(slow_records(A, l, u, DELTA, ne, nlo, nhi)):
        # the twin packs the ABI layout (column-major per item): Qc[b] = Qd', Ac[b] = Ad'
        assert np.array_equal(Qc[b], Qd.T) and np.array_equal(qd[b], q) and np.array_equal(Ac[b], Ad.T)
        assert np.array_equal(ll[b], lo) and np.array_equal(uu[b], hi)


def make_spy():
    from oracle_engine import OracleEngine

    class Spy(OracleEngine):
        """The oracle engine with the two new methods, each built from its numpy twin."""

        def __init__(self):
            super().__init__()
            self.member_solves = 0                              # solve_nodes calls over interior-member records

        def solve_nodes(self, Qc, *a, **k):
            if np.asarray(Qc)[0, 0, 0] == DELTA:                # (a member record starts with delta; an emptiness query's Q is I)
                self.member_solves += 1
            return OracleEngine.solve_nodes(self, Qc, *a, **k)

        def interior_members(self, Ac, l, u, delta, ne, nlo, nhi):
            A = np.swapaxes(np.asarray(Ac), 1, 2)
            assert (ne, nlo, nhi) == polyhedra.interior_member_counts(l, u)
            Qc, qd, Arec, ll, uu = polyhedra.interior_member_records(A, l, u, delta)
            B, nf = qd.shape
            mp = ll.shape[1]
            res = OracleEngine.solve_nodes(self, Qc, np.zeros((B, 1, nf)), qd, Arec, np.zeros((B, 1, mp)), ll, uu, np.zeros(1))
            st = np.asarray(res["status"]); z = np.asarray(res["z"])
            d = A.shape[2]
            return z[:, :d].copy(), ((st == 1) & (z[:, d] <= 1e-6)).astype(np.uint8), st.astype(np.int32)

        def members_outside(self, Ajc, lj, uj, X, pi, pj, t):
            return polyhedra.members_outside_host(Ajc, lj, uj, X, pi, pj, t)

    return Spy()


def level_lists(engine, **net):
    """The lists remove_subsets_many is given by the levels of one solve()."""
    seen = []
    orig = algorithm.remove_subsets_many

    def recording(lists, eng, *a, **k):
        seen.append([None if polys is None else list(polys) for polys in lists])
        return orig(lists, eng, *a, **k)
    algorithm.remove_subsets_many = recording
    try:
        ret = algorithm.solve(examples.setup("synthetic_pairs", **net), engine=engine)
    finally:
        algorithm.remove_subsets_many = orig
    assert ret["solved"]
    return seen


def test_spy_engine_keeps_the_same_lists_without_member_solves():
    from oracle_engine import OracleEngine
    box = lambda lo, hi: Poly(np.eye(2), [lo, lo], [hi, hi])
    hand = [[box(-1, 1), box(-2, 2), box(0, 3)], [box(0, 1)], [box(0, 1), box(0, 1)],
            [Poly(np.array([[1.0, 0.0], [0.0, 1.0]]), [0.0, 0.0], [0.0, 1.0]), box(-1, 1), box(2, 3)]]     # (a segment inside a box)
    levels = [hand] + level_lists(OracleEngine(), pairs=6, n=4, m=6)
    assert sum(1 for lists in levels for polys in lists if polys is not None and len(polys) >= 2) >= 3
    for lists in levels:
        plain, spy = OracleEngine(), make_spy()
        want = polyhedra.remove_subsets_many(lists, plain)
        got = polyhedra.remove_subsets_many(lists, spy)
        assert len(want) == len(got)
        for w, g in zip(want, got):
            assert (w is None and g is None) or [id(P) for P in w] == [id(P) for P in g]
        if any(polys is not None and len(polys) >= 2 for polys in lists):
            assert spy.calls["interior_members"] >= 1 and spy.calls["members_outside"] >= 1
        assert spy.member_solves == 0
    # the plain engine's members come through solve_nodes, as before
    plain = make_spy()
    plain.interior_members = None; plain.members_outside = None
    polyhedra.remove_subsets_many(hand, plain)
    assert plain.member_solves >= 1


def test_interior_members_batch_through_the_engine_method():
    """interior_members_batch on an engine with interior_members: the same members as on the plain engine, bit for bit."""
    from oracle_engine import OracleEngine
    A, l, u = seeded_polyhedra(11, 7, 8, 4, "mixed")
    trips = [(A[b], l[b], u[b]) for b in range(7)]
    trips.append((np.array([[1.0, 0, 0, 0], [1.0, 0, 0, 0]]), np.array([1.0, -INF]), np.array([INF, 0.0])))      # empty
    want = polyhedra.interior_members_batch(trips, OracleEngine())
    spy = make_spy()
    got = polyhedra.interior_members_batch(trips, spy)
    assert spy.calls["interior_members"] >= 2 and spy.member_solves == 0      # (one call per size; every look at the attribute counts too)
    assert got[-1] is None and want[-1] is None and any(x is not None for x in want)
    for a, b in zip(want, got):
        assert (a is None and b is None) or np.array_equal(a, b)


def exact_outside(Ajc, lj, uj, X, pi, pj, t, band):
    """Per pair: the verdict from a.x computed exactly (Fraction), and whether some row's exact a.x lies within
    band * (1 + |bound|) of a threshold (such a pair may be left out of the comparison)."""
    F = Fraction
    verdict = np.zeros(len(pi), bool); near = np.zeros(len(pi), bool)
    Bj, d, rj = Ajc.shape
    for q, (i, j) in enumerate(zip(pi, pj)):
        for row in range(rj):
            ax = sum((F(float(Ajc[j, c, row])) * F(float(X[i, c])) for c in range(d)), F(0))
            for bound, sign in ((lj[j, row], -1), (uj[j, row], 1)):
                if not np.isfinite(bound):
                    continue
                thr = F(float(bound)) + sign * F(float(t))
                if sign * (ax - thr) > 0:
                    verdict[q] = True
                if abs(ax - thr) <= F(band) * (1 + abs(F(float(bound)))):
                    near[q] = True
    return verdict, near


@pytest.mark.parametrize("seed,Bj,rj,d", [(21, 5, 9, 6), (22, 3, 70, 12), (23, 4, 1, 1), (24, 6, 33, 40)])
def test_members_outside_host_against_exact_arithmetic(seed, Bj, rj, d):
    g = np.random.default_rng(seed)
    A = g.standard_normal((Bj, rj, d))
    Bi = 7
    X = g.standard_normal((Bi, d))
    # bounds around the members' own values, so that both verdicts occur
    ax = np.einsum("jrd,d->jr", A, X[0])
    lj = ax - g.uniform(0.0, 2.0, (Bj, rj)); uj = ax + g.uniform(0.0, 2.0, (Bj, rj))
    lj[g.uniform(size=lj.shape) < 0.2] = -INF; uj[g.uniform(size=uj.shape) < 0.2] = INF
    pi = np.repeat(np.arange(Bi), Bj).astype(np.int32); pj = np.tile(np.arange(Bj), Bi).astype(np.int32)
    t = 1e-5
    Ajc = np.ascontiguousarray(np.swapaxes(A, 1, 2))
    got = polyhedra.members_outside_host(Ajc, lj, uj, X, pi, pj, t).astype(bool)
    want, near = exact_outside(Ajc, lj, uj, X, pi, pj, t, 1e-9)
    print(f"seed {seed}: {len(pi)} pairs, {int(near.sum())} within the band, {int(want.sum())} refuted")
    assert int(near.sum()) == 0                                  # continuous random data: no pair sits on a threshold
    assert np.array_equal(got, want)
    assert want.any() and not want.all()


def test_members_outside_host_on_a_bound_and_beyond():
    t = 1e-5
    # one piece: 0 <= x1 <= 1, x2 <= 2 (column-major: Ajc[piece, column, row])
    A = np.array([[[1.0, 0.0], [0.0, 1.0]]])
    Ajc = np.ascontiguousarray(np.swapaxes(A, 1, 2))
    lj = np.array([[0.0, -INF]]); uj = np.array([[1.0, 2.0]])
    X = np.array([[1.0, 2.0],                # on two bounds: not refuted
                  [0.0, 0.0],                # on the lower bound: not refuted
                  [1.0 + 2 * t, 0.0],        # beyond the upper bound by 2 t: refuted
                  [-2 * t, 0.0],             # beyond the lower bound by 2 t: refuted
                  [0.5, 2.0 + 2 * t],        # beyond the second row's upper bound: refuted
                  [0.5, -1e9]])              # the second row has no lower bound: not refuted
    pi = np.arange(6, dtype=np.int32); pj = np.zeros(6, np.int32)
    got = polyhedra.members_outside_host(Ajc, lj, uj, X, pi, pj, t)
    assert got.dtype == np.uint8 and got.tolist() == [0, 0, 1, 1, 1, 0]


def test_pairs_asked_in_slices_give_the_same_lists(monkeypatch):
    """remove_subsets_many asks its (member, piece) pairs in slices of PAIR_CHUNK: slices that cut through a list, and through the
    pairs of one second piece, keep the lists of one slice."""
    npairs = lambda lists: sum(len(p) * (len(p) - 1) for p in lists if p is not None)
    box = lambda lo, hi: Poly(np.eye(2), [lo, lo], [hi, hi])
    lists = [[box(-i, i) for i in (3, 1, 2, 5, 4, 1)], [box(0, 1)], [box(0, 1), box(2, 3), box(0, 3), box(1, 2)], None,
             [Poly(np.eye(3), [0, 0, 0], [1, 1, i]) for i in (2, 1, 3)]]
    assert npairs(lists) == 30 + 12 + 6
    want = polyhedra.remove_subsets_many(lists, make_spy())
    for chunk in (1, 7):
        monkeypatch.setattr(polyhedra, "PAIR_CHUNK", chunk)
        spy = make_spy()
        got = polyhedra.remove_subsets_many(lists, spy)
        assert [g if g is None else [id(P) for P in g] for g in got] == [w if w is None else [id(P) for P in w] for w in want]
        assert spy.calls["members_outside"] > 2
