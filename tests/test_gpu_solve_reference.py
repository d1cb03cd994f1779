"""Every route of qpn_solve_nodes*, qpn_solve_nodes_h and qpn_solve_avi_batch against planted, exactly known solutions.

The other solve tests compare with the CPU oracle, which shares the kernels' pivot rule and was written with them; here the
truth is the exact solution of the rounded data (tests/solve_ref.py: longdouble refinement, proved by a certificate), over
condition numbers up to 1e6, a spectrum below the fused kernels' decline threshold, asymmetric and nearly symmetric Hessians,
weakly active rows, no and min(n, m) active rows and badly scaled rows (tests/solve_cases.py), on the smallest shapes at which
each kernel's tiling can go wrong.  Per node: status SUCCESS, active[] equal to the masks of the truth wherever an error of the
bar's size cannot move them, and

    error <= max(16 E_ref, 64 eps),   E_ref = the CPU oracle's worst error against the truth on the same cell and family

(solve_ref.accuracy_bar; 16: blocked elimination in another summation order, reciprocals good to 10 ulp instead of 0.5).  The
resident n = m = 32 cells check the crash-cache reuse sweep and the mixed launch against a SECOND planted solution installed by
Nodes.update -- an exactly known answer, not the recompute path -- and read Nodes.info(): symmetric bit, cache-valid bit, declines.
The measured tallies are in profiles/planted_solve_accuracy.txt.
"""
import numpy as np
import pytest

import solve_cases as SC
import solve_ref as SR

pytestmark = pytest.mark.gpu

# (cell, family) -> factor where the global 16 does not hold, with the reason; none needed so far
FACTORS = {}


def _abi(nodes):
    from qpn_amd.engine import colmajor
    Q, R, qd, A, B, l, u = SC.stack(nodes)
    return [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u]


def _np(res):
    return {k: np.asarray(v) for k, v in res.items() if v is not None}


class _Cell:
    """The checks of one cell: every run is compared with its truths and with the oracle's error on the same nodes."""

    def __init__(self, cell, oracle):
        self.cell, self.oracle = cell, oracle
        self.runs = []                                    # (where, nodes, truths, outputs)
        self.e_ref = {}
        self.notes = []

    def oracle_on(self, nodes, truths, w):
        """The oracle's errors on these nodes enter E_ref (and it has to solve every one of them)."""
        ref = SC.oracle_solve(self.oracle, nodes, w)
        assert np.all(ref["status"] == 1), f"{self.cell}: the oracle does not solve its own reference cases"
        for i, (c, (zt, info)) in enumerate(zip(nodes, truths)):
            e = SR.node_error(ref["z"][i], zt, c["rec"][0].shape[0], SC.row_norm(c))
            self.e_ref[c["family"]] = max(self.e_ref.get(c["family"], 0.0), e)
        return ref

    def planted(self, where, nodes, res):
        truths = [SC.truth(c) for c in nodes]
        self.oracle_on(nodes, truths, nodes[0]["w"])
        self.runs.append((where, nodes, truths, _np(res)))

    def per_node_w(self, where, nodes, W, res):
        """A sweep with one w per node: the truth by certificate, from the active set the oracle's answer claims."""
        ref = SC.oracle_solve(self.oracle, nodes, W)
        truths = [SC.truth_from_solution(c, W[i], ref["z"][i]) for i, c in enumerate(nodes)]
        self.oracle_on(nodes, truths, W)
        self.runs.append((where, nodes, truths, _np(res)))

    def finish(self, capsys):
        fails, tally = [], {}
        factor = {f: v for (c, f), v in FACTORS.items() if c == self.cell}
        for where, nodes, truths, res in self.runs:
            t = {}
            fails += SC.check_against_truth(nodes, truths, res, f"{self.cell} {where}", t, self.e_ref, factor)
            for f, (e, cnt) in t.items():
                a = tally.setdefault(f, [0.0, 0])
                a[0] = max(a[0], e); a[1] += cnt
        with capsys.disabled():
            print(f"\n[solve {self.cell}] runs: " + ", ".join(r[0] for r in self.runs))
            for f, (e, cnt) in sorted(tally.items()):
                if f == "mask-unsafe":
                    print(f"[solve {self.cell}]   masks not compared on {cnt} nodes of per-node-w sweeps (a row near a threshold)")
                    continue
                er = self.e_ref[f]
                print(f"[solve {self.cell}]   {f:9s} nodes {cnt:5d}  kernel {e:.2e}  E_ref {er:.2e}  ratio {e / max(er, 1e-300):7.2f}  "
                      f"bar {SR.accuracy_bar(er, factor.get(f, SR.FACTOR)):.2e}")
            for note in self.notes:
                print(f"[solve {self.cell}]   {note}")
        assert not fails, "\n".join(fails[:12]) + (f"\n... {len(fails)} in all" if len(fails) > 12 else "")
        # no case was skipped: every node of every run was compared
        assert sum(t[1] for f, t in tally.items() if f != "mask-unsafe") == sum(len(r[1]) for r in self.runs)


def _n_axis(nodes, n):
    """axis nodes with a diagonal below the decline threshold 1e-4 max(1, max |M|)."""
    return sum(c["family"] == "axis" and np.diag(c["rec"][0]).min() < 1e-4 for c in nodes)


def _handle_sweeps(engine, ck, nodes, n, m, p, where, second=None):
    """One upload and its sweeps: the shared w of the plant, (after Nodes.update of qd, l, u) the second plant, and one w per
    node; x_out equals z[:, :n] bit for bit in each.  -> Nodes.info() after the sweeps, and before the update."""
    h = engine.upload_nodes(*_abi(nodes))
    try:
        x = np.zeros((len(nodes), n + 2))
        res = _np(h.solve(nodes[0]["w"], x_out=x))
        assert np.array_equal(x[:, :n], res["z"][:, :n]) and np.all(x[:, n:] == 0), f"{where}: x_out"
        ck.planted(f"{where} handle", nodes, res)
        mid = h.info()
        if second is not None:
            Q, R, qd, A, B, l, u = SC.stack(second)
            for f, a in (("qd", qd), ("l", l), ("u", u)):
                h.update(f, a)
            assert h.info()["crash_cached"] == mid["crash_cached"], "an update of qd, l, u dropped the crash cache"
            x = np.zeros((len(nodes), n))
            res = _np(h.solve(second[0]["w"], x_out=x))
            assert np.array_equal(x, res["z"][:, :n]), f"{where}: x_out, second plant"
            ck.planted(f"{where} handle second-plant", second, res)
            nodes = second
        W = SC.per_node_params(ck.cell, nodes)
        x = np.zeros((len(nodes), n))
        res = _np(h.solve(W, x_out=x))
        assert np.array_equal(x, res["z"][:, :n]), f"{where}: x_out, per-node w"
        ck.per_node_w(f"{where} handle per-node-w", nodes, W, res)
        engine.synchronize()
        return h.info(), mid
    finally:
        h.close()


def test_f32_call(engine, oracle, capsys):
    ck = _Cell("f32_call", oracle)
    for n, m, p, nodes in SC.cell_cases("f32_call"):
        assert SC.route_of(n, m) == "fused32"
        ck.planted(f"({n},{m}) per-call", nodes, engine.solve_nodes(*_abi(nodes), nodes[0]["w"]))
    ck.finish(capsys)


def test_f32_handle_sym(engine, oracle, capsys):
    ck = _Cell("f32_handle_sym", oracle)
    (n, m, p, nodes), = SC.cell_cases("f32_handle_sym")
    info, mid = _handle_sweeps(engine, ck, nodes, n, m, p, f"({n},{m})", second=SC.second_plants("f32_handle_sym"))
    assert mid["symmetric"] and mid["crash_cached"] and not mid["crash_refused"], mid      # sweep 1 filled the cache
    assert info["symmetric"] and info["crash_cached"] and not info["crash_refused"], info  # ... and the later ones reused it
    # the axis nodes' diagonals are below the decline threshold: the fused kernel hands them to the general kernel
    assert info["decline_state"] == 3 and info["declined"] >= _n_axis(nodes, n) > 0, info
    ck.notes.append(f"info: {info}; axis nodes {_n_axis(nodes, n)}; reuse sweep checked against the second plant")
    ck.finish(capsys)


def test_f32_handle_gen(engine, oracle, capsys):
    ck = _Cell("f32_handle_gen", oracle)
    (n, m, p, nodes), = SC.cell_cases("f32_handle_gen")
    info, _ = _handle_sweeps(engine, ck, nodes, n, m, p, f"({n},{m}) skew+nearsym")
    assert not info["symmetric"] and not info["crash_cached"] and info["crash_refused"], info
    # one nearly symmetric record in an otherwise symmetric batch switches the whole handle
    sym = SC.cell_cases("f32_handle_sym")[0][3]
    near = next(c for c in nodes if c["family"] == "nearsym")
    mixed = [dict(c, w=near["w"]) for c in sym[:12]]
    for c in mixed:                                       # (the same records under this batch's w: planted again)
        c.pop("_truth", None)
    rng = np.random.default_rng(5)
    mixed = [SC.replant(rng, c) for c in mixed] + [near]
    info2, _ = _handle_sweeps(engine, ck, mixed, n, m, p, f"({n},{m}) symmetric+1 nearsym")
    assert not info2["symmetric"] and not info2["crash_cached"], info2
    ck.notes.append(f"info: {info}; with one nearsym record: {info2}")
    ck.finish(capsys)


def test_f32_mixed(engine, oracle, capsys):
    """64 distinct planted nodes tiled to 4 160 (more than the resident set): sweep 1 fills the crash cache, sweep 2 -- after
    Nodes.update to the second plant -- is the mixed reuse / recompute launch.  The truth is computed for the 64 only."""
    ck = _Cell("f32_mixed", oracle)
    (n, m, p, nodes), = SC.cell_cases("f32_mixed")
    second = SC.second_plants("f32_mixed")
    reps = SC.RESIDENT // len(nodes) + 1
    assert len(nodes) == 64 and reps * len(nodes) > SC.RESIDENT
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1)))
    h = engine.upload_nodes(*[tile(a) for a in _abi(nodes)])
    try:
        for sweep, cases in enumerate((nodes, second)):
            if sweep:
                Q, R, qd, A, B, l, u = SC.stack(second)
                for f, a in (("qd", qd), ("l", l), ("u", u)):
                    h.update(f, tile(a))
                assert h.info()["crash_cached"]
            res = _np(h.solve(cases[0]["w"]))
            # every copy of a node is compared with its truth: the worst copy per node goes into the check
            truths = [SC.truth(c) for c in cases]
            zt = np.stack([np.asarray(t[0]) for t in truths])
            err = np.abs(res["z"].reshape(reps, len(cases), n + m).astype(np.longdouble) - zt[None]).max(axis=2)
            worst = err.argmax(axis=0)
            pick = worst * len(cases) + np.arange(len(cases))
            assert np.all(res["status"] == 1)
            act = res["active"].reshape(reps, len(cases), n + m)
            assert np.all(act == act[0][None]), "copies of one node carry different masks"
            ck.planted(f"sweep {sweep + 1} ({'fill' if not sweep else 'mixed reuse, second plant'}), worst of {reps} copies",
                       cases, {k: res[k][pick] for k in ("z", "status", "active")})
        engine.synchronize()
        info = h.info()
    finally:
        h.close()
    assert info["symmetric"] and info["crash_cached"] and info["sweeps"] >= 2, info
    assert info["decline_state"] == 3 and info["declined"] >= reps * _n_axis(nodes, n) > 0, info
    ck.notes.append(f"{reps * len(nodes)} nodes; info: {info}")
    ck.finish(capsys)


@pytest.mark.parametrize("cell", ["s48", "wg", "wg2", "big2"])
def test_fused_class(engine, oracle, cell, capsys):
    """Per shape: one per-call launch over every family (the general variants), and a resident handle over the symmetric
    families (the variants that skip the mirrored tile; big2: Stage B by block principal pivoting) with its sweeps."""
    ck = _Cell(cell, oracle)
    for n, m, p, nodes in SC.cell_cases(cell):
        assert SC.route_of(n, m) == SC.ROUTE[cell]
        ck.planted(f"({n},{m}) per-call", nodes, engine.solve_nodes(*_abi(nodes), nodes[0]["w"]))
        sym = [c for c in nodes if c["family"] in SC.SYMMETRIC]
        info, _ = _handle_sweeps(engine, ck, sym, n, m, p, f"({n},{m})")
        assert info["symmetric"], info
        if cell != "big2":                                # (the big2 route has no decline count: it always runs the gated launch)
            na = _n_axis(sym, n)
            assert info["decline_state"] == (3 if na else info["decline_state"]) and info["declined"] >= na, info
            ck.notes.append(f"({n},{m}): declined {info['declined']}, axis nodes below the threshold {na}")
            assert na > 0
    ck.finish(capsys)


def test_general(engine, oracle, capsys):
    from qpn_amd import _lib
    ck = _Cell("general", oracle)
    for n, m, p, nodes in SC.cell_cases("general"):
        assert SC.route_of(n, m) == "general"
        ck.planted(f"({n},{m}) per-call", nodes, engine.solve_nodes(*_abi(nodes), nodes[0]["w"]))
    # a fused shape on the general route (QPN_OPT_MID_ROUTE = 0) ...
    n, m, p, nodes = SC.cell_cases("s48")[1]
    assert SC.route_of(n, m, mid_route=0) == "general"
    engine.set_option(_lib.OPT_MID_ROUTE, 0)
    try:
        res = engine.solve_nodes(*_abi(nodes), nodes[0]["w"])
    finally:
        engine.set_option(_lib.OPT_MID_ROUTE, 1)
    ck.planted(f"({n},{m}) mid-route 0", nodes, res)
    # ... and a fused shape under a pivot budget of n + 40 (it stays on its fused route; the budget is Lemke's)
    n, m, p, nodes = SC.cell_cases("wg")[2]
    assert SC.route_of(n, m, max_pivots=n + 40) == "wg"
    o = engine.default_opts()
    o.max_pivots = n + 40
    ck.planted(f"({n},{m}) budget n+40", nodes, engine.solve_nodes(*_abi(nodes), nodes[0]["w"], opts=o))
    ck.finish(capsys)


def test_explicit_M(engine, oracle, capsys):
    """qpn_solve_avi_batch on the assembled blocks: small (matrix-core) and large node-shaped items."""
    import problems as P
    from qpn_amd.engine import colmajor
    ck = _Cell("explicit_M", oracle)
    for n, m, p, nodes in SC.cell_cases("explicit_M"):
        M, q, lo, hi, kind = P.reduced_blocks(*SC.stack(nodes), nodes[0]["w"])
        ck.planted(f"({n},{m}) assembled blocks", nodes, engine.solve_avi_batch(colmajor(M), q, lo, hi, kind=kind))
    ck.finish(capsys)


def test_bpp_multipliers_as_accurate_as_lemke(engine, oracle, capsys):
    """Regression: Stage B by block principal pivoting (resident symmetric records of the big2 class) reads S(:, A) as the rows A
    of the computed S = Ad (H^-1 Ad') and factors its lower triangle, i.e. it solved with a SYMMETRISED S, while the read-back
    x = -(W lambda + h) uses the W of the same factorisation: the computed S is symmetric only to cond(H) eps, so the active rows
    missed their bounds by |S - S'| |lambda|.  At cond(H) = 1e4 the symmetric handle was 8 - 10 x worse than the Lemke kernel on
    the SAME S and c (5.6e-10 and 7.4e-10 against 5.5e-11 and 1.0e-10 on the (129, 16) and (130, 96) shapes below) and missed
    the accuracy bar.  Fixed by one refinement step on the rows of S itself (schur_big_bpp); block pivoting is now at 1 - 3e-12.
    Both routes read the same S and c and share the read-back, and cond(S_AA) <= 1e2 here: block pivoting may differ from
    Lemke's pivots by rounding, a factor 4 at the most."""
    lines = []
    for n, m, p, nodes in SC.cell_cases("big2")[:2]:
        k1e4 = [c for c in nodes if c["family"] == "k1e4"]
        h = engine.upload_nodes(*_abi(k1e4))
        try:
            assert h.info()["symmetric"]
            o = engine.default_opts()
            o.max_pivots = 100_000                        # a caller-set budget is Lemke's to count: no block pivoting
            lemke = _np(h.solve(k1e4[0]["w"], opts=o))
            bpp = _np(h.solve(k1e4[0]["w"]))
        finally:
            h.close()
        assert np.all(lemke["status"] == 1) and np.all(bpp["status"] == 1)
        for i, c in enumerate(k1e4):
            zt = SC.truth(c)[0]
            el, eb = SR.node_error(lemke["z"][i], zt, n), SR.node_error(bpp["z"][i], zt, n)
            lines.append(f"[solve bpp] ({n},{m}) k1e4 [{i}]: Lemke {el:.2e}  block pivoting {eb:.2e}  ratio {eb / el:.2f}")
            assert eb <= max(4 * el, SR.FLOOR), lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines))
