"""Host buffers against device buffers: every C-ABI entry point that takes a `mem` argument gives bitwise the same outputs for
the same inputs passed as numpy arrays (QPN_MEM_HOST, staged through the context's workspace) and as torch device tensors
(QPN_MEM_DEVICE, handed to the kernels as they are), on every route and size class.  A `mem` that is neither is refused, and so
is a device tensor that is not what the header declares for its argument."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if isinstance(a, np.ndarray) else a


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _same(h, d, what):
    if isinstance(h, dict):
        assert h.keys() == d.keys(), what
        for k in h:
            _same(h[k], d[k], f"{what}[{k}]")
    elif isinstance(h, (tuple, list)):
        assert len(h) == len(d), what
        for i, (a, b) in enumerate(zip(h, d)):
            _same(a, b, f"{what}[{i}]")
    elif isinstance(h, np.ndarray):
        b = np.ascontiguousarray(_np(d))
        assert h.shape == b.shape and h.dtype == b.dtype, what
        assert np.ascontiguousarray(h).tobytes() == b.tobytes(), what
    else:
        assert h == d, what


def _both(fn, *args, what="", **kw):
    """fn on host arrays, then on device copies of the same arrays; the outputs must agree bit for bit."""
    import torch
    h = fn(*args, **kw)
    d = fn(*(_dev(a) for a in args), **{k: _dev(v) for k, v in kw.items()})
    torch.cuda.synchronize()
    _same(h, d, what or getattr(fn, "__name__", "call"))
    return h


def _records(count, n, m, p=8, first=0, per_item_w=False):
    from qpn_amd import synthetic as S
    from qpn_amd.engine import colmajor
    Q, R, qd, A, B, l, u = S.synth_nodes(first, count, n, m, p)
    w = np.random.default_rng(n * 1000 + m).standard_normal((count, p)) if per_item_w else S.shared_params(p)
    return [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u, w]


def _kkt(engine, n, m, count=32):
    Mc, q, lo, hi, kind = engine.assemble_nodes(*_records(count, n, m))
    return Mc, q, lo, hi, kind


@pytest.mark.parametrize("n, m", [(16, 16), (40, 40)])         # N <= 64 and N > 64 (the large-item workspace)
def test_solve_and_check_avi_batch(engine, n, m):
    Mc, q, lo, hi, kind = _kkt(engine, n, m)
    for k in (None, kind[0], kind):
        _both(engine.solve_avi_batch, Mc, q, lo, hi, kind=k, what=f"solve_avi_batch kind {None if k is None else k.ndim}")
    _both(engine.solve_avi_batch, Mc, q, lo, hi, kind=kind, want_active=False, what="solve_avi_batch no active")
    z0 = np.random.default_rng(1).uniform(-0.5, 0.5, q.shape)
    r = _both(engine.solve_avi_batch, Mc, q, lo, hi, z0=z0, kind=kind, what="solve_avi_batch z0")
    for want_r in (True, False):
        _both(engine.check_avi_batch, Mc, q, lo, hi, r["z"], kind=kind, want_r=want_r, what=f"check_avi_batch r={want_r}")
    _, res = engine.check_avi_batch(Mc, q, lo, hi, r["z"], kind=kind)
    for shift in (0, 4):
        _both(engine.comp_indices, r["z"], res, lo, hi, shift=shift, what=f"comp_indices shift {shift}")


@pytest.mark.parametrize("m, p, per_item_w", [(8, 0, False), (0, 6, False), (8, 6, False), (8, 6, True)])
def test_assemble_nodes(engine, m, p, per_item_w):
    _both(engine.assemble_nodes, *_records(16, 12, m, p, per_item_w=per_item_w), what=f"assemble_nodes m={m} p={p}")


def _masks(rng, rows, N):
    return rng.choice(np.array([1, 2, 4, 3, 5], np.uint8), size=(rows, N), p=[0.3, 0.3, 0.2, 0.1, 0.1])


def test_recipes_and_pieces(engine):
    rng = np.random.default_rng(5)
    n, m, p, nodes = 6, 4, 3, 4
    N = n + m
    _both(engine.recipes_from_masks, _masks(rng, 1, N)[0], what="recipes_from_masks")
    masks = _masks(rng, nodes, N)
    totals = [engine.recipes_from_masks(mk, count=0)[1] for mk in masks]
    offsets = np.concatenate([[0], np.cumsum([min(t, 5) for t in totals])]).astype(np.int64)
    K, node_of = _both(lambda mk: engine.recipes_batch(mk, offsets), masks, what="recipes_batch")
    rec = _records(nodes, n, m, p)[:7]
    for no, KK in ((node_of, K), (None, K[:nodes])):
        tag = "node_of" if no is not None else "one per node"
        _both(engine.local_pieces, *rec, KK, node_of=no, what=f"local_pieces {tag}")
        _both(engine.reduced_pieces, *rec, KK, node_of=no, what=f"reduced_pieces {tag}")


def test_assemble_pools(engine):
    """Both forms; one M shared by the batch and one M per item."""
    rng = np.random.default_rng(9)
    n_i, m_i, p = [2, 3], [2, 1], 2
    nd, sn, sm = 5, 5, 3
    dpos = rng.permutation(nd).astype(np.int32)
    sh = dict(Qd=(nd, sn), Qp=(p, sn), qd=(sn,), Ad=(nd, sm), Bp=(p, sm), l=(sm,), u=(sm,), w=(p,))
    blocks = {k: rng.standard_normal(s) for k, s in sh.items()}
    blocks["l"], blocks["u"] = -rng.random(sm), rng.random(sm)
    order = ["Qd", "Qp", "qd", "Ad", "Bp", "l", "u", "w"]
    for form in ("reduced", "reference"):
        call = lambda *a: engine.assemble_pools(n_i, m_i, dpos, nd, *a, form=form)      # noqa: E731
        _both(call, *(blocks[k] for k in order), what=f"pools {form} single")
        batch = dict(blocks, qd=rng.standard_normal((3, sn)), w=rng.standard_normal((3, p)))
        _both(call, *(batch[k] for k in order), what=f"pools {form} shared M")
        per = dict(batch, Qd=rng.standard_normal((3, nd, sn)), Ad=rng.standard_normal((3, nd, sm)),
                   l=-rng.random((3, sm)), u=rng.random((3, sm)))
        _both(call, *(per[k] for k in order), what=f"pools {form} per-item M")


def _solve_x(engine, rec, n, **kw):
    import torch
    batch = rec[2].shape[0]
    xh = np.full((batch, n + 3), 7.0)
    h = engine.solve_nodes(*rec, x_out=xh, **kw)
    xd = torch.full((batch, n + 3), 7.0, dtype=torch.float64, device=DEV)
    d = engine.solve_nodes(*(_dev(a) for a in rec), x_out=xd, **{k: _dev(v) for k, v in kw.items()})
    torch.cuda.synchronize()
    return h, d, xh, xd


# the routes of qpn_solve_nodes: the 32 class, mid (one wavefront <= 48, one workgroup <= 128), big2, general (N <= 64 and > 64)
@pytest.mark.parametrize("n, m", [(16, 16), (40, 40), (80, 80), (160, 32), (16, 0), (80, 0)])
def test_solve_nodes_routes(engine, n, m):
    rec = _records(48, n, m, per_item_w=True)
    h, d, xh, xd = _solve_x(engine, rec, n)
    _same(h, d, f"solve_nodes {n}x{m}")
    _same(xh, xd, f"solve_nodes {n}x{m} x_out")
    if m == 16:
        z0 = np.random.default_rng(2).uniform(-0.5, 0.5, h["z"].shape)
        h, d, xh, xd = _solve_x(engine, rec, n, z0=z0)
        _same(h, d, "solve_nodes z0")
        _same(xh, xd, "solve_nodes z0 x_out")


@pytest.mark.parametrize("n, m", [(16, 16), (48, 48), (80, 80)])        # the verify classes: <= 32, <= 64, wide
def test_verify_nodes(engine, n, m):
    rec = _records(32, n, m)
    z = engine.solve_nodes(*rec)["z"]
    xd = z[:, :n].copy()
    _both(engine.verify_nodes, *rec[:7], xd, rec[7], what=f"verify_nodes {n}x{m}")


@pytest.mark.parametrize("n, m", [(16, 16), (80, 80)])
def test_nodes_handle_host_and_device_w(engine, n, m):
    import torch
    rec = _records(32, n, m, per_item_w=True)
    nodes = engine.upload_nodes(*rec[:7])
    try:
        for w in (rec[7], rec[7][0]):
            for _ in range(2):           # the second sweep runs on what the first learned about declines
                xh = np.zeros((32, n))
                h = nodes.solve(w, x_out=xh)
                xd = torch.zeros((32, n), dtype=torch.float64, device=DEV)
                d = nodes.solve(_dev(w), x_out=xd)
                torch.cuda.synchronize()
                _same(h, d, "Nodes.solve")
                _same(xh, xd, "Nodes.solve x_out")
            _same(nodes.verify(h["z"][:, :n].copy(), w), nodes.verify(_dev(h["z"][:, :n].copy()), _dev(w)), "Nodes.verify")
    finally:
        nodes.close()


@pytest.mark.parametrize("n, m", [(16, 0), (16, 8), (160, 40)])        # m = 0, m > 0, the HBM-workspace class
def test_convexity_nodes(engine, n, m):
    from qpn_amd.engine import colmajor
    g = np.random.default_rng(n + m)
    G = g.standard_normal((8, n, n))
    Qc = colmajor(G + np.swapaxes(G, 1, 2))
    Ac = g.standard_normal((8, n, m))
    eq = (g.random((8, m)) < 0.5).astype(np.uint8)
    _both(engine.convexity_nodes, Qc, Ac, eq, what=f"convexity {n}x{m}")


def test_order_then_solve(engine):
    rec = _records(64, 16, 16)
    piv = engine.solve_nodes(*rec)["pivots"]
    try:
        engine.order_nodes_by_pivots(piv)
        h = engine.solve_nodes(*rec)
        engine.order_nodes_by_pivots(_dev(piv))
        d = engine.solve_nodes(*(_dev(a) for a in rec))
        _same(h, d, "solve after order_nodes_by_pivots")
    finally:
        engine.set_node_order(None)


def _bad_mem_calls(engine, nodes):
    rec = _records(4, 8, 4, 3)
    Mc, q, lo, hi, kind = engine.assemble_nodes(*rec)
    z = np.zeros_like(q)
    masks = np.ones((2, 12), np.uint8)
    K = np.ones((2, 12), np.uint8)
    ones = lambda *s: np.ones(s)     # noqa: E731
    return {
        "solve_avi_batch": lambda: engine.solve_avi_batch(Mc, q, lo, hi, kind=kind),
        "check_avi_batch": lambda: engine.check_avi_batch(Mc, q, lo, hi, z, kind=kind),
        "comp_indices": lambda: engine.comp_indices(z, z, lo, hi),
        "assemble_nodes": lambda: engine.assemble_nodes(*rec),
        "recipes_from_masks": lambda: engine.recipes_from_masks(masks[0]),
        "recipes_batch": lambda: engine.recipes_batch(masks, np.array([0, 1, 2], np.int64)),
        "local_pieces": lambda: engine.local_pieces(*rec[:7], K[:2]),
        "reduced_pieces": lambda: engine.reduced_pieces(*rec[:7], K[:2]),
        "assemble_pools": lambda: engine.assemble_pools([1], [1], [0], 1, ones(1, 1), ones(0, 1), ones(1), ones(1, 1),
                                                        ones(0, 1), -ones(1), ones(1), ones(0)),
        "solve_nodes": lambda: engine.solve_nodes(*rec),
        "solve_nodes_h": lambda: nodes.solve(rec[7]),
        "verify_nodes": lambda: engine.verify_nodes(*rec[:7], np.zeros((4, 8)), rec[7]),
        "verify_nodes_h": lambda: nodes.verify(np.zeros((4, 8)), rec[7]),
        "order_nodes_by_pivots": lambda: engine.order_nodes_by_pivots(np.zeros(4, np.int32)),
        "convexity_nodes": lambda: engine.convexity_nodes(rec[0], rec[3], np.ones((4, 4), np.uint8)),
    }


@pytest.mark.parametrize("entry", ["solve_avi_batch", "check_avi_batch", "comp_indices", "assemble_nodes", "recipes_from_masks",
                                   "recipes_batch", "local_pieces", "reduced_pieces", "assemble_pools", "solve_nodes",
                                   "solve_nodes_h", "verify_nodes", "verify_nodes_h", "order_nodes_by_pivots", "convexity_nodes"])
def test_unknown_mem_kind_is_refused(engine, monkeypatch, entry):
    """include/qpn_hip.h: `mem` is QPN_MEM_HOST or QPN_MEM_DEVICE; anything else is QPN_ERR_ARG, and nothing is launched."""
    from qpn_amd import engine as E
    nodes = engine.upload_nodes(*_records(4, 8, 4, 3)[:7])
    try:
        calls = _bad_mem_calls(engine, nodes)
        monkeypatch.setattr(E, "MEM_HOST", 2)
        with pytest.raises(E.QpnError, match="bad argument.*bad mem kind"):
            calls[entry]()
    finally:
        monkeypatch.undo()
        nodes.close()
        engine.set_node_order(None)


def _typed_device_args(engine):
    """case -> (entry point, a well-formed device tensor for the argument, the call with that argument replaced)."""
    import torch
    zeros = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=DEV)     # noqa: E731
    n, m, N = 8, 4, 12
    rec = [_dev(a) for a in _records(4, n, m, 3)[:7]]
    Mc, q = zeros(4, N, N), zeros(4, N)
    K, masks, kind = (zeros(4, N, dt=torch.uint8) for _ in range(3))
    idx = zeros(4, dt=torch.int32)
    return {
        "local_pieces: K": ("qpn_local_pieces", K, lambda a: engine.local_pieces(*rec, a, node_of=idx)),
        "local_pieces: node_of": ("qpn_local_pieces", idx, lambda a: engine.local_pieces(*rec, K, node_of=a)),
        "reduced_pieces: K": ("qpn_reduced_pieces", K, lambda a: engine.reduced_pieces(*rec, a, node_of=idx)),
        "reduced_pieces: node_of": ("qpn_reduced_pieces", idx, lambda a: engine.reduced_pieces(*rec, K, node_of=a)),
        "recipes_from_masks: mask": ("qpn_recipes_from_masks", masks[0], lambda a: engine.recipes_from_masks(a)),
        "recipes_batch: masks": ("qpn_recipes_batch", masks, lambda a: engine.recipes_batch(a, np.arange(5, dtype=np.int64))),
        "solve_avi_batch: kind": ("qpn_solve_avi_batch", kind, lambda a: engine.solve_avi_batch(Mc, q, q, q, kind=a)),
        "check_avi_batch: kind": ("qpn_check_avi_batch", kind, lambda a: engine.check_avi_batch(Mc, q, q, q, q, kind=a)),
        "recipe_filter: masks": ("qpn_recipe_filter", masks, lambda a: engine.recipe_filter(a, K, idx, idx)),
        "recipe_filter: K": ("qpn_recipe_filter", K, lambda a: engine.recipe_filter(masks, a, idx, idx)),
        "recipe_filter: vrow_of": ("qpn_recipe_filter", idx, lambda a: engine.recipe_filter(masks, K, a, idx)),
        "recipe_filter: first_of": ("qpn_recipe_filter", idx, lambda a: engine.recipe_filter(masks, K, idx, a)),
        "order_nodes_by_pivots: pivots": ("qpn_order_nodes_by_pivots", idx, lambda a: engine.order_nodes_by_pivots(a)),
        "set_node_order: order": ("qpn_set_node_order", idx, lambda a: engine.set_node_order(a)),
    }


@pytest.mark.parametrize("case", ["local_pieces: K", "local_pieces: node_of", "reduced_pieces: K", "reduced_pieces: node_of",
                                  "recipes_from_masks: mask", "recipes_batch: masks", "solve_avi_batch: kind", "check_avi_batch: kind",
                                  "recipe_filter: masks", "recipe_filter: K", "recipe_filter: vrow_of", "recipe_filter: first_of",
                                  "order_nodes_by_pivots: pivots", "set_node_order: order"])
def test_mistyped_device_argument_is_refused(engine, case):
    """A device tensor goes to the kernels as a raw address, so every method refuses one that is not what include/qpn_hip.h
    declares -- another integer type, a strided view, another GPU's memory -- before the library is called.  Each bad tensor
    is zeros over at least the bytes of the well-formed one."""
    import torch
    from qpn_amd.engine import QpnError
    entry, good, call = _typed_device_args(engine)[case]
    bad = [torch.zeros(good.shape, dtype=torch.int64, device=DEV),
           torch.zeros((*good.shape[:-1], 2 * good.shape[-1]), dtype=good.dtype, device=DEV)[..., ::2]]
    assert bad[1].shape == good.shape and not bad[1].is_contiguous()
    if torch.cuda.device_count() >= 2:
        bad.append(good.to("cuda:1"))
    before = engine.calls[entry]
    try:
        for a in bad:
            with pytest.raises(QpnError, match=f"{case} must be a contiguous"):
                call(a)
        assert engine.calls[entry] == before
    finally:
        engine.set_node_order(None)
