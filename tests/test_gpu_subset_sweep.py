"""qpn_solve_nodes_subset_h on the GPU (Nodes.solve_subset, csrc/qpn_subset.hip): a sweep over a chosen part of a
resident handle's nodes, compact inputs and outputs.

Every comparison is with Nodes.solve over the same handle (or a twin made from the same records) given w_full with
w_full[idx[s]] = w[s], and is array_equal -- not close -- on z, status, resid, pivots, active and the x scatter buffer
([count, n + 3] with three sentinel columns that have to stay).  Records: synthetic.synth_nodes with a random B (the crash
cache tests' records), asymmetric Qd / equality rows added where a case needs them.
  * 32-class, symmetric: fresh handle (the subset call comes first and fills no crash cache), cache filled (the reuse path),
    asymmetric Qd (the general variants), other shapes; (5, 0) has no rows and takes the general route: the fallback;
  * mixed launch (kResidentMI355X + 64 nodes), with the schedule on: `sweeps` and `scheduled` stay, a full sweep afterwards
    equals the one of a twin handle that never saw a subset call;
  * the mid classes; the fallback of large records (a full sweep: the handle's state is what a full sweep leaves);
  * decliners (equality rows) through the gated general launch, info() unchanged with and without a census;
  * warm hints in the 32-class and at (64, 64) after set_warm();
  * arguments: count 0 / batch, shared w, host and device memory, max_pivots, bad host lists (QPN_ERR_ARG, outputs untouched),
    bad entries of a device list (those slots FAILURE and zeros, the rest equal);
  * level_batch.SUBSET_SWEEP_ROUTE through solve_level: x_opt bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("z", "status", "resid", "pivots", "active")
SENTINEL = -7.25
RESIDENT = 16 * 256                       # kResidentMI355X (csrc/qpn_internal.h)
FAILURE = 4                               # QPN_FAILURE
_RECORDS = {}


def _records(n, m, p, cnt, asym=False, eq=()):
    """(abi records, w_full [cnt, p]) of a shape, built once.  asym: Qd + a skew part (the handle takes the general variants);
    eq: nodes that get an equality row (the fused kernels decline them)."""
    key = (n, m, p, cnt, asym, tuple(eq))
    if key not in _RECORDS:
        from qpn_amd import synthetic
        from qpn_amd.engine import colmajor
        Q, R, qd, A, B, l, u = synthetic.synth_nodes(0, cnt, n, m, p)
        rng = np.random.default_rng([7, n, m, cnt])
        B = 0.1 * rng.standard_normal((cnt, m, p))
        if asym:
            S = rng.standard_normal((cnt, n, n))
            Q = Q + 0.05 * (S - np.swapaxes(S, 1, 2)) / np.sqrt(n)
        u = u.copy()
        for k in eq:
            u[k, 2] = l[k, 2]
        w = synthetic.shared_params(p)[None, :] + 0.05 * rng.standard_normal((cnt, p))
        _RECORDS[key] = ([colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u], w)
    return _RECORDS[key]


def _np(res):
    return {k: v.cpu().numpy() if hasattr(v, "cpu") else np.array(v) for k, v in res.items() if v is not None}


def _t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def _full(nodes, w, device=True, warm=None, opts=None):
    """Nodes.solve with every output and the primal blocks scattered into an iterate of their own."""
    n = nodes.n
    if device:
        x = torch.full((nodes.batch, n + 3), SENTINEL, dtype=torch.float64, device="cuda:0")
        out = _np(nodes.solve(_t(w), x_out=x, opts=opts, warm=None if warm is None else _t(warm)))
        torch.cuda.synchronize()
        out["x"] = x.cpu().numpy()
    else:
        x = np.full((nodes.batch, n + 3), SENTINEL)
        out = _np(nodes.solve(w, x_out=x, opts=opts, warm=warm))
        out["x"] = x
    return out


def _subset(nodes, idx, w, device=True, warm=None, opts=None):
    """Nodes.solve_subset: w (and warm) are the compact rows."""
    idx = np.asarray(idx, dtype=np.int32)
    n = nodes.n
    if device:
        x = torch.full((idx.size, n + 3), SENTINEL, dtype=torch.float64, device="cuda:0")
        out = _np(nodes.solve_subset(_t(idx, torch.int32), _t(w), x_out=x, opts=opts, warm=None if warm is None else _t(warm)))
        torch.cuda.synchronize()
        out["x"] = x.cpu().numpy()
    else:
        x = np.full((idx.size, n + 3), SENTINEL)
        out = _np(nodes.solve_subset(idx, w, x_out=x, opts=opts, warm=warm))
        out["x"] = x
    return out


def _assert_rows(sub, full, idx, what, slots=None):
    """Slot s of the subset call == node idx[s] of the full sweep, on every output; slots: the slots to look at (all)."""
    idx = np.asarray(idx)
    slots = np.arange(idx.size) if slots is None else np.asarray(slots)
    for k in KEYS + ("x",):
        assert np.array_equal(sub[k][slots], full[k][idx[slots]], equal_nan=True), f"{what}: {k} differs"
    assert np.all(sub["x"][:, nodes_n(sub):] == SENTINEL), f"{what}: the columns of x beyond n were written"


def nodes_n(out):
    return out["x"].shape[1] - 3


def _scattered(batch, count, seed=3):
    """count distinct nodes, the first and the last among them, in non-monotone order."""
    rng = np.random.default_rng([seed, batch, count])
    mid = np.sort(rng.permutation(np.arange(1, batch - 1))[:count - 2])
    idx = np.concatenate([[batch - 1], mid, [0]]).astype(np.int32)          # down, up through the middle, down again
    assert np.unique(idx).size == count and np.any(np.diff(idx) < 0) and np.any(np.diff(idx) > 0)
    return idx


# ---- the 32-class ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_32_class_fresh_handle_then_reuse(engine, device):
    abi, w = _records(32, 32, 4, 96)
    idx = _scattered(96, 7)
    nodes = engine.upload_nodes(*abi)
    try:
        before = nodes.info()
        assert before["symmetric"] and not before["crash_cached"]
        first = _subset(nodes, idx, w[idx], device)                 # nothing is cached yet: the subset call fills nothing
        engine.synchronize()
        assert nodes.info() == before and not nodes.info()["crash_cached"]
        full = _full(nodes, w, device)
        assert np.all(full["status"] == 1) and nodes.info()["crash_cached"]
        _assert_rows(first, full, idx, "fresh handle")
        engine.synchronize()
        before = nodes.info()                                       # (the census has arrived: no node declines)
        assert before["decline_state"] == 2
        again = _subset(nodes, idx, w[idx], device)                 # the reuse path, no general launch, no workspace
        _assert_rows(again, full, idx, "cache filled")
        engine.synchronize()
        assert nodes.info() == before
    finally:
        nodes.close()


def test_32_class_general_variants(engine):
    abi, w = _records(32, 32, 4, 96, asym=True)
    idx = _scattered(96, 7)
    nodes = engine.upload_nodes(*abi)
    try:
        assert not nodes.info()["symmetric"]
        full = _full(nodes, w)
        assert np.all(full["status"] == 1)
        _assert_rows(_subset(nodes, idx, w[idx]), full, idx, "asymmetric Qd")
    finally:
        nodes.close()


@pytest.mark.parametrize("n,m", [(16, 16), (5, 0), (1, 32)])
def test_32_class_other_shapes(engine, n, m):
    abi, w = _records(n, m, 4, 40)
    idx = _scattered(40, 7)
    nodes = engine.upload_nodes(*abi)
    try:
        sub = _subset(nodes, idx, w[idx])                           # ((5, 0): the general route, i.e. the fallback)
        full = _full(nodes, w)
        assert np.all(full["status"] == 1)
        _assert_rows(sub, full, idx, f"({n}, {m})")
        _assert_rows(_subset(nodes, idx, w[idx], device=False), full, idx, f"({n}, {m}) host")
    finally:
        nodes.close()


def test_mixed_launch_and_handle_state(engine):
    """Beyond the resident set a reuse sweep is a mixed launch and the handle keeps a schedule: the subset call runs under its
    list all the same and leaves schedule, statistics and sweep count alone."""
    batch = RESIDENT + 64
    abi, w = _records(32, 32, 4, batch)
    idx = np.arange(0, batch, 13, dtype=np.int32)
    a, b = engine.upload_nodes(*abi), engine.upload_nodes(*abi)
    try:
        for h in (a, b):
            h.set_schedule(16)
        full = _full(a, w)
        twin = _full(b, w)
        assert np.all(full["status"] == 1) and a.info()["crash_cached"]
        engine.synchronize()
        before = a.info()
        assert before["sweeps"] == 1 and before["scheduled"]
        sub = _subset(a, idx, w[idx])
        _assert_rows(sub, full, idx, "mixed launch")
        engine.synchronize()
        assert a.info() == before
        w2 = w * 1.01
        after, twin2 = _full(a, w2), _full(b, w2)
        for k in KEYS + ("x",):
            assert np.array_equal(twin[k], full[k]) and np.array_equal(after[k], twin2[k]), f"twin handle: {k} differs"
        engine.synchronize()
        assert a.info() == b.info() and a.info()["sweeps"] == 2
    finally:
        a.close(); b.close()


# ---- the mid classes and the fallback ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(48, 48), (64, 64), (97, 64), (128, 128)])
def test_mid_classes(engine, n, m):
    abi, w = _records(n, m, 4, 24)
    idx = _scattered(24, 5)
    nodes = engine.upload_nodes(*abi)
    try:
        before = nodes.info()
        sub = _subset(nodes, idx, w[idx])                           # before any census: the workspace of the general launch is carved
        engine.synchronize()
        assert nodes.info() == before
        full = _full(nodes, w)
        assert np.all(full["status"] == 1)
        _assert_rows(sub, full, idx, f"({n}, {m}) first")
        engine.synchronize()
        nodes.info()
        _assert_rows(_subset(nodes, idx, w[idx]), full, idx, f"({n}, {m}) after the census")
        _assert_rows(_subset(nodes, idx, w[idx], device=False), full, idx, f"({n}, {m}) host")
    finally:
        nodes.close()


def test_fallback_route_of_large_records(engine):
    abi, w = _records(136, 40, 4, 6)
    idx = np.array([4, 1], dtype=np.int32)
    a, b = engine.upload_nodes(*abi), engine.upload_nodes(*abi)
    try:
        sub = _subset(a, idx, w[idx])
        w_full = np.zeros_like(w); w_full[idx] = w[idx]             # rows that no subset call has written are zero
        full = _full(b, w_full)
        _assert_rows(sub, full, idx, "(136, 40)")
        assert np.all(sub["status"] == 1)
        engine.synchronize()
        assert a.info() == b.info()                                 # the state of a handle after one full sweep
    finally:
        a.close(); b.close()


# ---- decliners ---------------------------------------------------------------------------------------------------------------------
def test_decliners_take_the_general_launch(engine):
    abi, w = _records(32, 32, 4, 96, eq=(5, 9))
    idx = np.array([40, 5, 95, 0, 17], dtype=np.int32)              # node 5 listed, node 9 not
    fresh, known = engine.upload_nodes(*abi), engine.upload_nodes(*abi)
    try:
        full = _full(known, w)
        engine.synchronize()
        before = known.info()
        assert before["decline_state"] == 3 and before["declined"] == 2 and np.all(full["status"] == 1)
        sub = _subset(known, idx, w[idx])
        _assert_rows(sub, full, idx, "census taken")
        engine.synchronize()
        assert known.info() == before
        before = fresh.info()
        assert before["decline_state"] == 0
        sub = _subset(fresh, idx, w[idx])
        _assert_rows(sub, full, idx, "no census")
        engine.synchronize()
        assert fresh.info() == before
        # the census of the next full sweep counts both decliners: the subset call left nothing behind in the counter
        _full(fresh, w)
        engine.synchronize()
        assert fresh.info()["declined"] == 2
    finally:
        fresh.close(); known.close()


# ---- warm hints --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(32, 32), (64, 64)])
def test_warm_hint(engine, n, m):
    abi, w = _records(n, m, 4, 48)
    idx = _scattered(48, 7)
    nodes = engine.upload_nodes(*abi)
    try:
        nodes.set_warm(1)                                           # (changes nothing at (32, 32))
        cold = _full(nodes, w)
        assert np.all(cold["status"] == 1)
        w2 = w * 1.001
        warm = _full(nodes, w2, warm=cold["z"])
        sub = _subset(nodes, idx, w2[idx], warm=cold["z"][idx])
        _assert_rows(sub, warm, idx, f"warm ({n}, {m})")
        assert np.any(sub["pivots"] == 0), "no listed node accepted its hint"
        _assert_rows(_subset(nodes, idx, w2[idx], device=False, warm=cold["z"][idx]), warm, idx, f"warm ({n}, {m}) host")
    finally:
        nodes.close()


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_counts_shared_w_and_budget(engine, device):
    abi, w = _records(32, 32, 4, 96)
    nodes = engine.upload_nodes(*abi)
    try:
        full = _full(nodes, w, device)
        # count == 0: nothing happens
        none = _subset(nodes, np.zeros(0, np.int32), np.zeros((0, 4)), device)
        assert none["status"].shape == (0,) and none["z"].shape == (0, 64)
        # count == batch, the identity list
        every = np.arange(96, dtype=np.int32)
        _assert_rows(_subset(nodes, every, w, device), full, every, "identity list")
        # one shared w (stride_w == 0)
        idx = _scattered(96, 7)
        shared = _full(nodes, w[0], device)
        _assert_rows(_subset(nodes, idx, w[0], device), shared, idx, "shared w")
        # a pivot budget: the nodes that stop at it are the same ones, with the same bits
        o = engine.default_opts()
        o.max_pivots = max(1, int(np.median(full["pivots"])))       # about half of the nodes need more
        capped = _full(nodes, w, device, opts=o)
        print("max_pivots =", o.max_pivots, ": statuses", np.unique(capped["status"], return_counts=True))
        assert np.any(capped["status"] != full["status"]), "the budget stopped no node: the case shows nothing"
        _assert_rows(_subset(nodes, idx, w[idx], device, opts=o), capped, idx, "max_pivots")
        # only the statuses
        if device:
            only = nodes.solve_subset(_t(idx, torch.int32), _t(w[idx]), want=())
            assert only["z"] is None and np.array_equal(only["status"].cpu().numpy(), full["status"][idx])
        else:
            only = nodes.solve_subset(idx, w[idx], want=())
            assert only["z"] is None and np.array_equal(only["status"], full["status"][idx])
    finally:
        nodes.close()


def test_bad_host_list_is_an_argument_error(engine):
    from qpn_amd.engine import QpnError
    abi, w = _records(32, 32, 4, 96)
    nodes = engine.upload_nodes(*abi)
    try:
        for bad in ([3, 8, 3, 20], [3, 96, 5, 20], [3, -1, 5, 20]):
            idx = np.array(bad, dtype=np.int32)
            out = dict(status=np.full(4, -9, np.int32), z=np.full((4, 64), SENTINEL), resid=np.full(4, SENTINEL),
                       pivots=np.full(4, -9, np.int32), active=np.full((4, 64), 9, np.uint8))
            x = np.full((4, 35), SENTINEL)
            with pytest.raises(QpnError):
                nodes.solve_subset(idx, w[:4], out=out, x_out=x)
            assert np.all(out["status"] == -9) and np.all(out["z"] == SENTINEL) and np.all(out["resid"] == SENTINEL)
            assert np.all(out["pivots"] == -9) and np.all(out["active"] == 9) and np.all(x == SENTINEL)
        with pytest.raises(QpnError):
            nodes.solve_subset(np.arange(97, dtype=np.int32) % 96, np.zeros((97, 4)))       # count > batch
        # the handle is as usable as before
        idx = _scattered(96, 7)
        _assert_rows(_subset(nodes, idx, w[idx], device=False), _full(nodes, w, device=False), idx, "after the errors")
    finally:
        nodes.close()


def test_bad_entries_of_a_device_list(engine):
    abi, w = _records(32, 32, 4, 96)
    nodes = engine.upload_nodes(*abi)
    try:
        full = _full(nodes, w)
        idx = np.array([95, 30, 7, 96, 30, 0, 61], dtype=np.int32)   # slot 3 out of range; slots 1 and 4 name node 30
        wq = w[np.minimum(idx, 95)]
        sub = _subset(nodes, idx, wq)
        good = [0, 2, 5, 6]
        _assert_rows(sub, full, idx, "good slots", slots=good)
        # of the two slots that name node 30 one claimed it and is solved, the other is the repeated entry
        lost = [s for s in (1, 4) if sub["status"][s] == FAILURE]
        assert len(lost) == 1
        won = 5 - lost[0]
        _assert_rows(sub, full, idx, "the claimant", slots=[won])
        for s in (3, lost[0]):
            assert sub["status"][s] == FAILURE and sub["resid"][s] == 0 and sub["pivots"][s] == 0
            assert np.all(sub["z"][s] == 0) and np.all(sub["active"][s] == 0) and np.all(sub["x"][s, :32] == 0)
    finally:
        nodes.close()


# ---- the host loop -----------------------------------------------------------------------------------------------------------------
def test_solve_level_route(engine):
    from qpn_amd import examples, level_batch
    net = examples.setup("synthetic_pairs", pairs=12, n=8, m=8)
    leaves = sorted(i for i in net.qps if not net.network_edges[i])
    assert len(leaves) == 12
    settled = set(leaves[::2]) | {leaves[1]}                        # 5 players left
    assert len(leaves) - len(settled) == 5
    x = 0.1 * np.random.default_rng(5).standard_normal(net.num_vars)
    assert level_batch.SUBSET_SWEEP_ROUTE is False
    off = level_batch.solve_level(net, leaves, x, engine=engine, settled=settled)
    calls = engine.calls["qpn_solve_nodes_subset_h"] if hasattr(engine, "calls") else None
    level_batch.SUBSET_SWEEP_ROUTE = True
    try:
        on = level_batch.solve_level(net, leaves, x, engine=engine, settled=settled)
    finally:
        level_batch.SUBSET_SWEEP_ROUTE = False
    if calls is not None:
        assert engine.calls["qpn_solve_nodes_subset_h"] == calls + 1
    assert np.array_equal(on, off) and not np.array_equal(on, x)
