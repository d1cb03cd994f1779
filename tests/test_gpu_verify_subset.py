"""qpn_verify_nodes_subset_h on the GPU (Nodes.verify_subset, csrc/qpn_verify.hip <LIST = true>): the accept gate
over a listed part of a resident handle.

The contract: slot s of solution, path and lambda equals, bit for bit, what Nodes.verify returns on the SAME handle for node
idx[s] given the same xd and w rows and the same tol.  Every comparison here is np.array_equal against that full call; the full
call itself is checked against an independent reference in test_gpu_verify_reference.py.  Records and points: the cells of
tests/verify_cases.py (every kernel and hand-over of the file), synthetic.synth_nodes for the small and empty shapes.
  * the route matrix: a permutation of all nodes and a scattered, non-monotone third, each as a device and as a host list;
  * mid_overflow (more nodes with k > 32 than verify_wide_node has slots): flags and paths equal, multipliers that differ pass
    the certificate of the reference;
  * one node at three points in one call, every node twice (count = 2 batch);
  * m = 0, p = 0, a shared w, tol = 1e-6;
  * arguments: count 0, bad host lists (QPN_ERR_ARG, outputs untouched), bad entries of a device list (path 6, zeros);
  * level_batch.SUBSET_VERIFY_ROUTE through process_level on this engine: one subset call, the same results.
No m == 0 reference goes through Engine.verify_nodes on device memory (include/qpn_hip.h: a null Ad there is a load from 0)."""
import numpy as np
import pytest
import torch

import verify_cases as VC
import verify_ref as VR

pytestmark = pytest.mark.gpu
TOL = 1e-4
SENT = -7.25


def _upload(engine, recs):
    from qpn_amd.engine import colmajor
    Q, R, qd, A, B, l, u = recs[:7]
    return engine.upload_nodes(colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u)


class _Batch:
    """Records on a resident handle, the points (xd, w) and the full call's answer at them (host arrays, computed once)."""

    def __init__(self, engine, recs, xd, w, tol=TOL):
        self.recs, self.xd, self.w, self.tol = recs, np.ascontiguousarray(xd), np.ascontiguousarray(w), tol
        self.nodes = _upload(engine, recs)
        self.batch = self.nodes.batch
        self.full = self.verify(self.xd, self.w)

    def verify(self, xd, w):
        return tuple(np.array(a) for a in self.nodes.verify(xd, w, tol=self.tol))

    def rows(self, idx):
        return self.w if self.w.ndim == 1 else self.w[idx]

    def subset(self, idx, xd=None, w=None, device=True):
        idx = np.asarray(idx, dtype=np.int32)
        xd = self.xd[idx] if xd is None else xd
        w = self.rows(idx) if w is None else w
        if device:
            t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")
            out = self.nodes.verify_subset(t(idx, torch.int32), t(xd, torch.float64), t(w, torch.float64), tol=self.tol)
            return tuple(a.cpu().numpy() for a in out)
        return tuple(np.array(a) for a in self.nodes.verify_subset(idx, xd, w, tol=self.tol))

    def close(self):
        self.nodes.close()


def _assert_slots(got, full, idx, what):
    for name, g, f in zip(("solution", "lambda", "path"), got, full):
        assert g.shape[0] == len(idx), f"{what}: {name} has {g.shape[0]} slots for {len(idx)} entries"
        bad = [s for s in range(len(idx)) if not np.array_equal(g[s], f[idx[s]])]
        assert not bad, f"{what}: {name} differs from the full call in slots {bad[:8]} ({len(bad)} in all)"


def _permutation(batch, seed):
    return np.random.default_rng(seed).permutation(batch).astype(np.int32)


def _scattered(batch, seed):
    """A third of the nodes, the first and the last among them, in an order that is not monotone."""
    rng = np.random.default_rng(seed)
    mid = rng.choice(np.arange(1, batch - 1), size=max(batch // 3 - 2, 1), replace=False)
    idx = np.concatenate([[batch - 1], mid, [0]]).astype(np.int32)
    assert np.any(np.diff(idx) > 0) and np.any(np.diff(idx) < 0)
    return idx


@pytest.fixture(scope="module")
def cells(engine):
    made = {}

    def get(cell):
        if cell not in made:
            recs = VC.stack(VC.cell_cases(cell))
            made[cell] = _Batch(engine, recs, recs[7], recs[8])
        return made[cell]
    yield get
    for b in made.values():
        b.close()


# ---- 1. the route matrix ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [c for c in VC.CELLS if c != "mid_overflow"])
def test_route_matrix(cells, cell):
    b = cells(cell)
    for name, idx in (("permutation", _permutation(b.batch, 3)), ("scattered third", _scattered(b.batch, 4))):
        for device in (True, False):
            got = b.subset(idx, device=device)
            _assert_slots(got, b.full, idx, f"{cell}, {name}, {'device' if device else 'host'} list")
            paths = set(got[2].tolist())
            assert paths & {1, 2, 3} and paths & {0, 4, 5}, f"{cell}, {name}: the listed nodes' paths {sorted(paths)} do not cover both sides"


# ---- 2. more flagged nodes than slots ---------------------------------------------------------------------------------
def test_mid_overflow(cells):
    b = cells("mid_overflow")
    assert b.batch == 280 > VC.MID_SLOTS
    idx = _permutation(b.batch, 5)
    for device in (True, False):
        sol, lam, path = b.subset(idx, device=device)
        assert np.array_equal(sol, b.full[0][idx]) and np.array_equal(path, b.full[2][idx])
        Q, R, qd, A, B, l, u, xd, w = b.recs
        differ = 0
        for s, i in enumerate(idx):
            if sol[s] == 1 and not np.array_equal(lam[s], b.full[1][i]):
                differ += 1
                ref = VR.verify_reference(*[a[i] for a in b.recs], tol=TOL)
                ok, msg = VR.certificate(lam[s], ref, A[i], int(path[s]), TOL, Qd=Q[i], R=R[i], xd=xd[i], w=w[i], qd=qd[i])
                assert ok, f"slot {s} (node {i}): multipliers differ from the full call's and fail the certificate: {msg}"
        print(f"[verify subset mid_overflow, {'device' if device else 'host'}] accepted slots with other multipliers: {differ}")


# ---- 3. duplicates, count > batch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["node32_full", "node64", "wide_fast"])
def test_one_node_at_three_points(cells, cell):
    b = cells(cell)
    node = int(np.flatnonzero(b.full[0] == 1)[0])              # a node the full call accepts at its own point
    pts = np.stack([b.xd[node], b.xd[node] * (1.0 - 1e-2), b.xd[node] + 0.05])
    idx = np.array([node, 3, node, node], dtype=np.int32)
    xd = np.stack([pts[0], b.xd[3], pts[1], pts[2]])
    want = []                                                  # the full call with slot s's row in its node's place
    for s in range(4):
        x_full = b.xd.copy()
        x_full[idx[s]] = xd[s]
        want.append(b.verify(x_full, b.w))
    assert want[0][0][node] == 1 and len({tuple(np.concatenate([[f[0][node], f[2][node]], f[1][node]])) for f in want[0:1] + want[2:]}) > 1
    for device in (True, False):
        got = b.subset(idx, xd=xd, device=device)
        for s in range(4):
            for g, f in zip(got, want[s]):
                assert np.array_equal(g[s], f[idx[s]]), f"{cell}: slot {s} (node {idx[s]}) differs from the full call at its row"


@pytest.mark.parametrize("cell", ["node32", "mid_slots", "wide_pivoted"])
def test_every_node_twice(cells, cell):
    b = cells(cell)
    idx = np.concatenate([_permutation(b.batch, 6), _permutation(b.batch, 7)])
    assert len(idx) == 2 * b.batch
    for device in (True, False):
        _assert_slots(b.subset(idx, device=device), b.full, idx, f"{cell}, every node twice")


# ---- 4. small and empty shapes ----------------------------------------------------------------------------------------
def _synth(engine, n, m, p, cnt, shared_w=False, seed=21):
    """Records of synthetic.synth_nodes with qd and three lower bounds re-made so that the point x is optimal by construction
    (rows 0 .. 2 sit at their lower bound with multipliers in [0.5, 2], q~ = Ad' lambda); every other node is then moved off it."""
    from qpn_amd import synthetic as P
    Q, R, qd, A, B, l, u = P.synth_nodes(40, cnt, n, m, p=p)
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(p) if shared_w else rng.standard_normal((cnt, p))
    xd = 0.1 * rng.standard_normal((cnt, n))
    k = min(3, m)
    for i in range(cnt):
        lam = rng.uniform(0.5, 2.0, k)
        l[i, :k] = A[i, :k] @ xd[i]
        qd[i] = -(Q[i] @ xd[i] + R[i] @ (w if shared_w else w[i])) + A[i, :k].T @ lam
    xd[1::2] += 0.05
    return _Batch(engine, (Q, R, qd, A, B, l, u), xd, w)


def test_no_rows(engine):
    b = _synth(engine, 5, 0, 2, 24)
    try:
        assert set(b.full[2].tolist()) == {1} and set(b.full[0].tolist()) == {0, 1}
        for idx in (_permutation(24, 1), _scattered(24, 2)):
            for device in (True, False):
                _assert_slots(b.subset(idx, device=device), b.full, idx, "(5, 0), p = 2")
    finally:
        b.close()


@pytest.mark.parametrize("shared_w", [False, True])
def test_no_parameters_and_shared_w(engine, shared_w):
    b = _synth(engine, 12, 16, 8 if shared_w else 0, 40, shared_w=shared_w)
    try:
        assert len(set(b.full[0].tolist())) == 2
        for idx in (_permutation(40, 1), _scattered(40, 2)):
            for device in (True, False):
                _assert_slots(b.subset(idx, device=device), b.full, idx, f"(12, 16), {'shared w' if shared_w else 'p = 0'}")
    finally:
        b.close()


def test_nondefault_tol(engine):
    """tol = 1e-6 reaches the subset's :119 test as it reaches the full call's: the planted residuals of
    test_verify_nondefault_tol give paths 2, 2, 3, 3, 4."""
    rng = np.random.default_rng(5)
    cases = [VC.make_case(rng, 12, 16, 6, "generic", rperp=r) for r in (0.0, 3e-7, 1e-5, 1e-5, 3e-4)]
    recs = VC.stack(cases)
    b = _Batch(engine, recs, recs[7], recs[8], tol=1e-6)
    try:
        assert list(b.full[2]) == [2, 2, 3, 3, 4]
        idx = np.array([4, 2, 0, 3, 1, 2], dtype=np.int32)
        for device in (True, False):
            got = b.subset(idx, device=device)
            _assert_slots(got, b.full, idx, "tol = 1e-6")
            assert list(got[2]) == [4, 3, 2, 3, 2, 3]
    finally:
        b.close()


# ---- 5. arguments -----------------------------------------------------------------------------------------------------
def _raw(engine, nodes, idx, xd, w, sol, lam, path, tol=TOL):
    """The entry point itself on caller-made outputs; returns its code."""
    from qpn_amd import _lib
    from qpn_amd.engine import _ptr
    dev = isinstance(sol, torch.Tensor)
    engine._bind_stream(dev)
    rc = engine.lib.qpn_verify_nodes_subset_h(engine.ctx, nodes.h, len(idx), _ptr(idx), _ptr(xd), _ptr(w), w.shape[-1], float(tol),
                                              _ptr(sol), _ptr(lam), _ptr(path), _lib.MEM_DEVICE if dev else _lib.MEM_HOST)
    if dev:
        torch.cuda.synchronize()
    return rc


def test_count_zero_and_bad_host_lists(cells, engine):
    b = cells("node32")
    m = b.recs[5].shape[1]
    # count = 0: nothing is touched (device outputs: nothing is launched either)
    sol = torch.full((4,), -9, dtype=torch.int32, device="cuda:0"); path = sol.clone()
    lam = torch.full((4, m), SENT, dtype=torch.float64, device="cuda:0")
    empty = torch.zeros((0,), dtype=torch.int32, device="cuda:0")
    assert _raw(engine, b.nodes, empty, torch.zeros((0, 12), dtype=torch.float64, device="cuda:0"),
                torch.zeros((0, b.w.shape[1]), dtype=torch.float64, device="cuda:0"), sol, lam, path) == 0
    assert bool((sol == -9).all()) and bool((path == -9).all()) and bool((lam == SENT).all())
    s0, l0, p0 = b.subset(np.zeros(0, np.int32), device=False)
    assert s0.shape == (0,) and p0.shape == (0,) and l0.shape == (0, m)
    # a host list with a bad entry: QPN_ERR_ARG before anything is staged, the outputs stay
    for bad in ([3, -1, 5, 20], [3, b.batch, 5, 20]):
        idx = np.array(bad, dtype=np.int32)
        sol = np.full(4, -9, np.int32); path = sol.copy(); lam = np.full((4, m), SENT)
        good = np.clip(idx, 0, b.batch - 1)
        assert _raw(engine, b.nodes, idx, np.ascontiguousarray(b.xd[good]), np.ascontiguousarray(b.w[good]), sol, lam, path) == -1
        assert np.all(sol == -9) and np.all(path == -9) and np.all(lam == SENT)
    from qpn_amd.engine import QpnError
    with pytest.raises(QpnError, match="qpn_verify_nodes_subset_h"):
        b.subset(np.array([0, b.batch], np.int32), xd=b.xd[:2], w=b.w[:2], device=False)
    with pytest.raises(QpnError):
        b.subset(np.array([0, 1], np.int32), xd=b.xd[:3], w=b.w[:2], device=False)          # xd rows != count
    # the handle is as usable as before
    idx = _scattered(b.batch, 8)
    _assert_slots(b.subset(idx, device=False), b.full, idx, "after the errors")


@pytest.mark.parametrize("cell", ["node32", "node64", "mid_slots", "wide_fast"])
def test_bad_entries_of_a_device_list(cells, cell):
    b = cells(cell)
    m = b.recs[5].shape[1]
    idx = _scattered(b.batch, 9).copy()
    good = idx.copy()
    bad_slots = [1, len(idx) // 2, len(idx) - 2]
    for s, v in zip(bad_slots, (-1, b.batch, 2 ** 31 - 1)):
        idx[s] = v
    sol, lam, path = b.subset(idx, xd=b.xd[good], w=b.w[good], device=True)
    keep = np.setdiff1d(np.arange(len(idx)), bad_slots)
    assert np.all(sol[bad_slots] == 0) and np.all(path[bad_slots] == 6) and np.all(lam[bad_slots] == 0.0)
    assert lam.shape == (len(idx), m)
    _assert_slots((sol[keep], lam[keep], path[keep]), b.full, good[keep], f"{cell}: the slots beside the bad entries")
    # nothing is left behind: a handle of another shape class verifies as before
    other = cells("node64" if cell != "node64" else "wide_fast")
    for a, f in zip(other.verify(other.xd, other.w), other.full):
        assert np.array_equal(a, f)
    i2 = _scattered(other.batch, 10)
    _assert_slots(other.subset(i2), other.full, i2, f"another handle after the bad list of {cell}")


# ---- 6. the host loop -------------------------------------------------------------------------------------------------
def test_process_level_takes_the_route(engine):
    import test_verify_subset_host as H
    from qpn_amd import level_batch
    which = [1, 4]

    def two_sweeps(route):
        net, followers, x = H._net()
        assert level_batch.SUBSET_VERIFY_ROUTE is False
        level_batch.SUBSET_VERIFY_ROUTE = route
        try:
            r1 = level_batch.process_level(net, followers, x, {}, engine=engine)
            assert all(r["solution"] for r in r1)
            before = dict(engine.calls)
            r2 = level_batch.process_level(net, followers, H._moved(net, followers, x, which), {}, engine=engine)
        finally:
            level_batch.SUBSET_VERIFY_ROUTE = False
        made = {k: engine.calls[k] - before.get(k, 0) for k in ("qpn_verify_nodes_subset_h", "qpn_verify_nodes_h", "qpn_verify_nodes")}
        return r1, r2, made

    _, off, made_off = two_sweeps(False)
    first, on, made_on = two_sweeps(True)
    assert made_off == {"qpn_verify_nodes_subset_h": 0, "qpn_verify_nodes_h": 1, "qpn_verify_nodes": 0}
    assert made_on == {"qpn_verify_nodes_subset_h": 1, "qpn_verify_nodes_h": 0, "qpn_verify_nodes": 0}
    H._same(on, off)
    for k in range(len(on)):
        assert (on[k] is first[k]) == (k not in which)
