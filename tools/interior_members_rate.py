"""Rates of the interior-member queries of remove_subsets on one GPU, at the traced shape: polyhedra of
64 rows in 64 variables with 32 equality rows, records of (nf, mp) = (97, 64).

  records_host   the route before qpn_interior_members: numpy records (polyhedra.interior_member_records) + host-mode solve_nodes
  members_host   qpn_interior_members in host mode (the polyhedra go up, members / ok / status come down)
  members_dev    qpn_interior_members in device mode (polyhedra resident, members stay on the device)
  assemble_dev   qpn_assemble_interior_nodes alone in device mode: the bytes it writes over its time

The three routes alternate, `--rounds` times; every time is a host clock around a call that ends in a synchronise.  The bytes
moved per query are computed from the shapes.  Prints one JSON line per measurement.
usage: python tools/interior_members_rate.py [--queries 20000] [--rounds 3]"""
import argparse
import time

import numpy as np

from rate_common import emit, on_device, polyhedra, qpn_amd
from qpn_amd.engine import colmajor

DELTA = 1e-2


def queries(B, r=64, d=64, n_eq=32, seed=0):
    g = np.random.default_rng(seed)
    A = g.standard_normal((B, r, d))
    s = np.einsum("brd,bd->br", A, g.standard_normal((B, d)))
    l = s - g.uniform(0.2, 1.0, (B, r)); u = s + g.uniform(0.2, 1.0, (B, r))
    l[:, :n_eq] = u[:, :n_eq] = s[:, :n_eq]
    return A, l, u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    eng = qpn_amd.default_engine(0)
    B = a.queries
    A, l, u = queries(B)
    r, d = A.shape[1:]
    ne, nlo, nhi = polyhedra.interior_member_counts(l, u)
    nf = d + 1 + ne
    mp = max(16, -(-(nlo + nhi) // 16) * 16)
    N = nf + mp
    rec_bytes = 8 * (nf * nf + nf + nf * mp + 2 * mp)
    emit(what="bytes_per_query", r=r, d=d, nf=nf, mp=mp, polyhedron=8 * (r * d + 2 * r), record=rec_bytes,
         records_host_up=rec_bytes + 8 * (nf + mp + 1), records_host_down=8 * N + 4 + 8 + 4 + N,
         members_host_up=8 * (r * d + 2 * r), members_host_down=8 * d + 1 + 4, members_dev_pcie=0,
         assembly_hbm_written=rec_bytes + 1, assembly_hbm_read=8 * (r * d + 2 * r))

    def records_host():
        Qc, qd, Ac, ll, uu = polyhedra.interior_member_records(A, l, u, DELTA)
        res = eng.solve_nodes(Qc, np.zeros((B, 1, nf)), qd, Ac, np.zeros((B, 1, mp)), ll, uu, np.zeros(1))
        st = np.asarray(res["status"]); z = np.asarray(res["z"])
        return z[:, :d], (st == 1) & (z[:, d] <= 1e-6)

    def members_host():
        x, ok, _ = eng.interior_members(colmajor(A), l, u, DELTA, ne, nlo, nhi)
        return x, ok.astype(bool)

    Ad, ld, ud = on_device(eng, (colmajor(A), l, u))

    def members_dev():
        x, ok, _ = eng.interior_members(Ad, ld, ud, DELTA, ne, nlo, nhi)
        torch.cuda.synchronize()
        return x, ok

    def assemble_dev():
        out = eng.assemble_interior_nodes(Ad, ld, ud, DELTA, ne, nlo, nhi)
        torch.cuda.synchronize()
        return out

    routes = dict(records_host=records_host, members_host=members_host, members_dev=members_dev, assemble_dev=assemble_dev)
    small = slice(0, min(B, 256))
    A_, l_, u_ = A, l, u
    A, l, u, B = A_[small], l_[small], u_[small], A_[small].shape[0]          # warm: module loads, first launches
    x0, ok0 = records_host()
    x1, ok1 = members_host()
    same = bool(np.array_equal(ok0, ok1) and np.array_equal(x0[ok0], x1[ok1]))
    A, l, u, B = A_, l_, u_, A_.shape[0]
    for f in (members_dev, assemble_dev):
        f()
    emit(what="routes_agree_bitwise", queries=int(small.stop), same=same, members=int(ok0.sum()))
    for rnd in range(a.rounds):
        for name, f in routes.items():
            t0 = time.perf_counter()
            out = f()
            dt = time.perf_counter() - t0
            line = dict(what=name, round=rnd, queries=B, seconds=dt, queries_per_s=B / dt)
            if name == "assemble_dev":
                line["written_GB_per_s"] = B * (rec_bytes + 1) / dt / 1e9
            else:
                line["members"] = int(np.asarray(out[1].cpu() if hasattr(out[1], "cpu") else out[1]).sum())
            del out
            emit(**line)


if __name__ == "__main__":
    main()
