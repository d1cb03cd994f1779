"""Test double: the oracle engine plus the six polyhedral entries, each served by its numpy twin (qpn_amd.polyhedra_host), with a
log of the calls it received.  TEST INFRASTRUCTURE ONLY: it lets the front ends of qpn_amd.polyhedra take every route the HIP
engine takes, without a GPU, and pins which calls they make and in which order."""
from __future__ import annotations

import numpy as np

from oracle_engine import OracleEngine
from qpn_amd import polyhedra_host as twin


def _shapes(args):
    return [f"{a.dtype}{list(a.shape)}" for a in args if isinstance(a, np.ndarray)]


class TwinEngine(OracleEngine):
    """log: [(method, dtype and shape of each of its array arguments)] in the order of the calls, solve_nodes included."""

    def __init__(self):
        super().__init__()
        self.log = []

    def _note(self, method, *args):
        self.log.append([method, _shapes(args)])

    def solve_nodes(self, Qc, Rc, qd, Ac, Bc, l, u, w, **kw):
        self._note("solve_nodes", Qc, Rc, qd, Ac, Bc, l, u, w)
        return OracleEngine.solve_nodes(self, Qc, Rc, qd, Ac, Bc, l, u, w, **kw)

    def solve_lps(self, Ac, l, u, poly_of, cost=None, obj_row=None, obj_sign=None, opts=None):
        self._note("solve_lps", Ac, l, u, poly_of, cost, obj_row, obj_sign)
        return twin.solve_lps_host(Ac, l, u, poly_of, cost=cost, obj_row=obj_row, obj_sign=obj_sign, opts=opts)

    def issubset_pairs(self, A1c, l1, u1, A2c, l2, u2, pi, pj, tol=1e-6, opts=None):
        assert pi.dtype == np.int32 and pj.dtype == np.int32
        self._note("issubset_pairs", A1c, l1, u1, A2c, l2, u2, pi, pj)
        return twin.issubset_pairs_host(A1c, l1, u1, A2c, l2, u2, pi, pj, tol=tol, opts=opts)

    def implicit_bounds(self, Ac, l, u, tol=1e-4, all_extremes=False, opts=None):
        self._note("implicit_bounds", Ac, l, u)
        return twin.implicit_bounds_host(Ac, l, u, tol=tol, all_extremes=all_extremes, opts=opts)

    def exemplar_polys(self, Ac, l, u, open_lo=None, open_hi=None, tol=1e-2, slack_cap=1.0, opts=None):
        assert open_lo.dtype == np.uint8 and open_hi.dtype == np.uint8
        self._note("exemplar_polys", Ac, l, u, open_lo, open_hi)
        return twin.exemplar_polys_host(Ac, l, u, open_lo, open_hi, tol=tol, slack_cap=slack_cap, opts=opts)

    def interior_members(self, Ac, l, u, delta, ne, nlo, nhi):
        """The records of the twin through the oracle's node solver (tests/test_interior_members_host.py's spy, stated again)."""
        self._note("interior_members", Ac, l, u)
        assert (ne, nlo, nhi) == twin.interior_member_counts(l, u)
        A = np.swapaxes(np.asarray(Ac), 1, 2)
        Qc, qd, Arec, ll, uu = twin.interior_member_records(A, l, u, delta)
        B, nf = qd.shape
        mp = ll.shape[1]
        res = OracleEngine.solve_nodes(self, Qc, np.zeros((B, 1, nf)), qd, Arec, np.zeros((B, 1, mp)), ll, uu, np.zeros(1))
        st = np.asarray(res["status"]); z = np.asarray(res["z"])
        d = A.shape[2]
        return z[:, :d].copy(), ((st == 1) & (z[:, d] <= 1e-6)).astype(np.uint8), st.astype(np.int32)

    def members_outside(self, Ajc, lj, uj, X, pi, pj, t):
        self._note("members_outside", Ajc, lj, uj, X, pi, pj)
        return twin.members_outside_host(Ajc, lj, uj, X, pi, pj, t)
