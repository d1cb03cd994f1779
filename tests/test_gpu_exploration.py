"""QPNetOptions.exploration_vertices on the MI355X: qpn_multiplier_vertices and qpn_recipe_filter against their numpy twins
(level_batch.multiplier_vertices_host, recipe_filter_host) in every size class and both memory modes, the statuses, and the
counterexample of tests/test_exploration_host.py on the HIP engine."""
import numpy as np
import pytest

from exploration_cases import X0, counterexample_net, degenerate_case
from qpn_amd import algorithm, examples
from qpn_amd import level_batch as lb

pytestmark = pytest.mark.gpu


def _cases(seed, n, m, batch, kind):
    rng = np.random.default_rng(seed)
    cs = [degenerate_case(rng, n, m, kind) for _ in range(batch)]
    return (np.stack([c[0] for c in cs]), np.stack([c[1] for c in cs]), np.stack([c[2] for c in cs]), np.stack([c[3] for c in cs]))


def _same(engine, Ac, g, cls, lam, V, max_bases, dev=False):
    tv, tc, ts = lb.multiplier_vertices_host(Ac, g, cls, lam, V, max_bases=max_bases)
    if dev:
        import torch
        to = lambda a: torch.as_tensor(a, device=f"cuda:{engine.device}")
        kv, kc, ks = engine.multiplier_vertices(to(Ac), to(g), to(cls), to(lam), V, max_bases=max_bases)
        kv, kc, ks = kv.cpu().numpy(), kc.cpu().numpy(), ks.cpu().numpy()
    else:
        kv, kc, ks = engine.multiplier_vertices(Ac, g, cls, lam, V, max_bases=max_bases)
    assert np.array_equal(kc, tc) and np.array_equal(ks, ts)
    for b in range(len(tc)):
        c = int(tc[b])
        assert np.allclose(kv[b, :c], tv[b, :c], rtol=1e-9, atol=1e-9 * max(1.0, np.max(np.abs(tv[b, :c]), initial=0.0)))
    return tc, ts


SMALL = [(1, 1, 5, 4, 16), (3, 5, 40, 8, 64), (2, 9, 9, 12, 256), (32, 32, 9, 6, 40), (20, 60, 5, 6, 40), (100, 128, 3, 4, 16),
         (64, 200, 2, 3, 8)]
LARGE = [(300, 512, 1, 2, 4), (512, 512, 1, 2, 3)]       # the global class at the entry's limit: one shape and mode each


@pytest.mark.parametrize("shape,kind,dev", [(s_, k, d) for s_ in SMALL for k in ("lp", "mixed", "dependent") for d in (False, True)]
                         + [(s_, "lp", False) for s_ in LARGE])
def test_kernel_matches_twin(engine, shape, kind, dev):
    n, m, batch, V, mb = shape
    Ac, g, cls, lam = _cases(n * 1000 + m, n, m, batch, kind)
    tc, ts = _same(engine, Ac, g, cls, lam, V, mb, dev)
    assert np.all(ts != lb.MV_EMPTY)


def test_kernel_results_do_not_depend_on_the_batch(engine):
    Ac, g, cls, lam = _cases(7, 4, 10, 12, "mixed")
    v_all, c_all, s_all = engine.multiplier_vertices(Ac, g, cls, lam, 8)
    for b in (0, 5, 11):
        v1, c1, s1 = engine.multiplier_vertices(Ac[b:b + 1], g[b:b + 1], cls[b:b + 1], lam[b:b + 1], 8)
        assert np.array_equal(v1[0], v_all[b]) and c1[0] == c_all[b] and s1[0] == s_all[b]


def test_kernel_statuses(engine):
    Ac = np.array([[[1.0, 1.0], [0.0, 0.0]]]); g = np.array([[1.0, 1.0]])
    _, s = _same(engine, Ac, g, np.zeros((1, 2), np.uint8), np.array([[0.5, 0.5]]), 4, 16)
    assert s[0] == lb.MV_EMPTY
    cls = np.array([[lb.MV_FREE, lb.MV_FREE, lb.MV_GE]], np.uint8)
    _, s = _same(engine, np.ones((1, 1, 3)), np.array([[1.0]]), cls, np.array([[0.5, 0.5, 0.0]]), 4, 16)
    assert s[0] == lb.MV_NO_VERTEX
    simplex = (np.ones((1, 1, 6)), np.array([[1.0]]), np.zeros((1, 6), np.uint8), np.full((1, 6), 1 / 6))
    c, s = _same(engine, *simplex, 10, 640)
    assert s[0] == lb.MV_COMPLETE and c[0] == 6
    c, s = _same(engine, *simplex, 4, 640)
    assert s[0] == lb.MV_VERTEX_BUDGET and c[0] == 4
    c, s = _same(engine, *simplex, 10, 3)
    assert s[0] == lb.MV_BASIS_BUDGET and c[0] == 3


@pytest.mark.parametrize("dev", [False, True])
def test_recipe_filter_matches_twin(engine, dev):
    rng = np.random.default_rng(3)
    rows, N = 9, 6
    masks = (rng.integers(1, 16, size=(rows, N)) << 4).astype(np.uint8)
    first = np.array([0, 0, 0, 3, 3, 5, 5, 5, 5], np.int32)
    K = (rng.integers(5, 9, size=(500, N))).astype(np.uint8)
    vrow = rng.integers(0, rows, size=500).astype(np.int32)
    want = lb.recipe_filter_host(masks, K, vrow, first)
    if dev:
        import torch
        to = lambda a: torch.as_tensor(a, device=f"cuda:{engine.device}")
        got = engine.recipe_filter(to(masks), to(K), to(vrow), to(first)).cpu().numpy()
    else:
        got = engine.recipe_filter(masks, K, vrow, first)
    assert np.array_equal(got, want) and 0 < want.sum() < 500


@pytest.mark.parametrize("max_pieces", [64, None])
def test_counterexample_on_the_hip_engine(engine, max_pieces):
    net, _, _ = counterexample_net()
    r = algorithm.solve(net, X0, engine=engine)
    assert r["solved"] and np.max(np.abs(r["x_opt"] - X0)) <= 1e-9
    net, _, _ = counterexample_net(exploration_vertices=3, max_pieces=max_pieces)
    r = algorithm.solve(net, X0, engine=engine)
    assert r["solved"] and np.max(np.abs(r["x_opt"] - np.array([-1.0, 1.0, 1.0]))) <= 1e-6


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_robust_avoid_simple_with_exploration(engine, seed):
    """Config 2 with exploration_vertices = 10: a solved answer passes the checks of test_config2_end_to_end; whether it is
    solved and whether it differs from the default is printed (-s)."""
    net = examples.setup("robust_avoid_simple", seed=seed, exploration_vertices=10, num_projections=5)
    r = algorithm.solve(net, engine=engine)
    ref = algorithm.solve(examples.setup("robust_avoid_simple", seed=seed, num_projections=5), engine=engine)
    print(f"seed {seed}: solved={r['solved']} default solved={ref['solved']}"
          + (f" max|x - x_default|={np.max(np.abs(r['x_opt'] - ref['x_opt'])):.3g}" if r["solved"] and ref["solved"] else ""))
    if not r["solved"]:
        return
    x = r["x_opt"]
    again = algorithm.solve(examples.setup("robust_avoid_simple", seed=seed, exploration_vertices=10, num_projections=5), x,
                            engine=engine)
    assert again["solved"] and np.max(np.abs(again["x_opt"] - x)) <= 1e-9
    for con in net.constraints.values() if isinstance(net.constraints, dict) else net.constraints:
        A, l, u = con.poly.vectorize()
        ax = A @ x
        assert np.all(ax >= l - 1e-6) and np.all(ax <= u + 1e-6)
