"""qpn_convexity_nodes (csrc/qpn_convexity.hip) against answers known by construction.

test_gpu_convexity compares the kernel with a float64 restatement that decides the rank by a threshold of its own, and leaves
out every node whose singular values come near that threshold: exactly dependent rows -- an implicit equality arrives as two
opposing rows -- are such nodes.  Here the rank is known (tests/convexity_cases.py), the truth is a longdouble enclosure of
lambda_min(Z' S Z) (tests/convexity_ref.py), and EVERY node is compared, from host and from device inputs:

    null_dim == n - rank,   convex == (truth > -tol),   min_eig == +inf where n - rank = 0,   otherwise
    dist(min_eig, [lam_lo, lam_hi]) <= max(16 E_ref, 64 eps) |S|_2,
    E_ref = the worst distance of the float64 restatement WITH THE RANK GIVEN (convexity_ref.plain64) over |S|_2 on the same cell

(cell = row family x shape; convexity_ref.accuracy_bar), never more than test_gpu_convexity's 1e-9 max(1, |S|_2).  The measured
tallies are in profiles/convexity_accuracy.txt.
"""
import numpy as np
import pytest

import convexity_cases as CC
import convexity_ref as CR

pytestmark = pytest.mark.gpu

# (shape, row family) -> factor where the global 16 does not hold, with the reason; none needed so far
FACTORS = {}
SHAPES = [s for s, _ in CC.SHAPES]


def _run(engine, Qc, Ac, eq, mode):
    if mode == "host":
        return tuple(np.asarray(a) for a in engine.convexity_nodes(Qc, Ac, eq, tol=CC.TOL))
    import torch
    out = engine.convexity_nodes(*(torch.tensor(a, device="cuda:0") for a in (Qc, Ac, eq)), tol=CC.TOL)
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in out)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_node_against_its_truth(engine, shape, capsys):
    nodes = CC.all_cases()[shape]
    truths = [CC.truth(c) for c in nodes]
    e_ref = {}
    for c, t in zip(nodes, truths):
        e_ref[c["family"]] = max(e_ref.get(c["family"], 0.0), t["e64"])
    Qc, Ac, eq = CC.stack(nodes)
    fails, tally, compared = [], {}, 0
    for mode in ("host", "device"):
        cvx, lam, nd = _run(engine, Qc, Ac, eq, mode)
        for i, (c, t) in enumerate(zip(nodes, truths)):
            compared += 1
            where = f"{shape} {mode} [{i}] {c['family']}/{c['hessian']} variant {c['variant']} scale 2^{c['scale']} rank {c['rank']}"
            row = tally.setdefault(c["family"], [0, 0.0, 0, 0.0])       # nodes, worst error over |S|_2, null_dim misses, worst error at S = 0
            row[0] += 1
            if nd[i] != t["d"]:
                row[2] += 1
                fails.append(f"{where}: null_dim {nd[i]}, true {t['d']} (min_eig {lam[i]:.6e}, truth [{float(t['lo']):.6e}, {float(t['hi']):.6e}])")
                continue
            if t["d"] == 0:
                if not (np.isinf(lam[i]) and lam[i] > 0 and cvx[i] == 1):
                    fails.append(f"{where}: min_eig {lam[i]}, convex {cvx[i]} on a node without a null space")
                continue
            if cvx[i] != int(t["hi"] > -CC.TOL):
                fails.append(f"{where}: convex {cvx[i]}, truth [{float(t['lo']):.9e}, {float(t['hi']):.9e}], min_eig {lam[i]:.9e}")
            bar = CR.accuracy_bar(e_ref[c["family"]], t["snorm"], FACTORS.get((shape, c["family"]), CR.FACTOR))
            assert bar <= CR.OLD_BAR * max(1.0, t["snorm"]), where
            err = CR.dist(lam[i], t["lo"], t["hi"])
            if t["snorm"] > 0:
                row[1] = max(row[1], err / t["snorm"])
            else:
                row[3] = max(row[3], err)
            if not err <= bar:
                fails.append(f"{where}: min_eig {lam[i]:.17e} is {err:.2e} from [{float(t['lo']):.17e}, {float(t['hi']):.17e}], bar {bar:.2e}")
    with capsys.disabled():
        print()
        for f, (cnt, e, miss, e0) in tally.items():
            er = e_ref[f]
            ratio = f"{e / er:8.2f}" if er > 0 else "       -"
            print(f"[convexity {shape[0]}x{shape[1]} {CC.cvx_class(*shape):6s}] {f:11s} nodes {cnt:3d}  null_dim misses {miss:2d}  kernel {e:.2e}  "
                  f"E_ref {er:.2e}  ratio {ratio}  bar {max(FACTORS.get((shape, f), CR.FACTOR) * er, CR.FLOOR):.2e}  (x |S|_2)"
                  + (f"  S = 0: off by {e0:.1e}" if e0 else ""))
    assert not fails, "\n".join(fails[:12]) + (f"\n... {len(fails)} in all" if len(fails) > 12 else "")
    # nothing was skipped: every built node was compared, in both modes
    assert compared == 2 * len(nodes) == sum(r[0] for r in tally.values())


def test_row_limit(engine):
    """m = 1024 is the last accepted row count."""
    from qpn_amd.engine import QpnError
    Qc = np.eye(4)[None].copy()
    Ac = np.zeros((1, 4, 1024)); Ac[0, 2, 1023] = 1.0; Ac[0, 2, 0] = -1.0
    eq = np.zeros((1, 1024), np.uint8); eq[0, [0, 1023]] = 1
    cvx, lam, nd = (np.asarray(a) for a in engine.convexity_nodes(Qc, Ac, eq, tol=CC.TOL))
    assert nd[0] == 3 and cvx[0] == 1 and lam[0] == pytest.approx(2.0, abs=1e-14)
    with pytest.raises(QpnError):
        engine.convexity_nodes(Qc, np.zeros((1, 4, 1025)), np.zeros((1, 1025), np.uint8), tol=CC.TOL)


def test_second_chunk_of_the_global_class(engine):
    """Two distinct (16, 1024) nodes tiled on the device to one node more than a launch of the global class takes: every copy
    answers bit for bit as in the two-node call, in the second launch (first > 0) as in the first."""
    import torch
    n, m = 16, 1024
    assert CC.cvx_class(n, m) == "global"
    nodes = CC.all_cases()[(n, m)]
    pick = [next(c for c in nodes if c["family"] == "wide" and c["rank"] == n - 1 and c["scale"] == 0),
            next(c for c in nodes if c["family"] == "dup_neg" and c["variant"] == 1 and c["scale"] == 0)]
    count = CC.cvx_chunk(n, m) + 1
    assert count * CC.slice_bytes(n, m, CC.CVX_GROUP) > CC.GLOBAL_CHUNK_BYTES >= (count - 1) * CC.slice_bytes(n, m, CC.CVX_GROUP)
    assert 2 < count < 5000
    two = [torch.tensor(a, device="cuda:0") for a in CC.stack(pick)]
    c2, l2, n2 = engine.convexity_nodes(*two, tol=CC.TOL)
    assert n2.cpu().tolist() == [1, n - pick[1]["rank"]]
    idx = torch.arange(count, device="cuda:0") % 2
    idx[-1] = 0                                            # (count is odd or even: the node of the second launch is node 0's copy ...)
    idx[-2] = 1                                            # (... and the last of the first launch node 1's)
    ct, lt, nt = engine.convexity_nodes(*(a[idx].contiguous() for a in two), tol=CC.TOL)
    torch.cuda.synchronize()
    assert torch.equal(ct, c2[idx]) and torch.equal(nt, n2[idx])
    assert torch.equal(lt.view(torch.int64), l2[idx].view(torch.int64))


def test_pinned_leaf_end_to_end(engine):
    from qpn_amd import algorithm
    from qpn_amd.qp_processing import check_qp_convexity
    from test_convexity_host import _leaf
    net = _leaf(pinned=True)
    pid = next(iter(net.qps))
    qp = net.qps[pid]
    cons = [net.constraints[c].poly for c in qp.constraint_indices]
    A = np.vstack([P.A for P in cons]); l = np.concatenate([P.l for P in cons]); u = np.concatenate([P.u for P in cons])
    lam, nd = check_qp_convexity(qp.f.Q, A, l, u, net.decision_inds(pid), pid, engine=engine)
    assert nd == 1 and lam == pytest.approx(2.0, abs=1e-14)
    off = algorithm.solve(_leaf(pinned=True), engine=engine)
    net.set_options(check_convexity=True)
    before = engine.calls["qpn_convexity_nodes"]
    on = algorithm.solve(net, engine=engine)
    assert engine.calls["qpn_convexity_nodes"] > before
    assert on["solved"] == off["solved"]
    key = "x_opt" if off["solved"] else "x_fail"
    assert np.array_equal(on[key], off[key])


def test_dense_pin_of_the_negative_direction(engine):
    """n = 40, Q = U diag(1, ..., 1, -1) U': pinned by the two opposing dense rows +-u_40' x >= 0 the node is convex on what is
    left (Z' (Q + Q') Z = 2 I); without the pin it is not."""
    from qpn_amd.qp_processing import NonConvexQPError, check_qp_convexity
    n = 40
    g = np.random.Generator(np.random.Philox(key=[9, n]))
    U, R = np.linalg.qr(g.standard_normal((n, n)))
    lam = np.ones(n); lam[-1] = -1.0
    Q = (U * lam) @ U.T
    Q = 0.5 * (Q + Q.T)
    u40 = U[:, -1]
    box = (np.eye(n), -np.ones(n), np.ones(n))
    A = np.vstack([box[0], u40[None], u40[None]])
    l = np.concatenate([box[1], [0.0, -np.inf]]); u = np.concatenate([box[2], [np.inf, 0.0]])
    assert np.all(l < u)
    got, nd = check_qp_convexity(Q, A, l, u, range(n), 7, engine=engine)
    assert nd == n - 1 and got == pytest.approx(2.0, abs=1e-12)
    with pytest.raises(NonConvexQPError) as ei:
        check_qp_convexity(Q, *box, range(n), 7, engine=engine)
    assert ei.value.pid == 7 and ei.value.min_eig == pytest.approx(-2.0, abs=1e-12)
