"""Inner-node records made on the MI355X from a static store, a pool of child pieces and column maps:
qpn_assemble_parent_nodes against its numpy twin bit for bit in both memory modes and both forms, its argument errors and bad
items, solve_nodes / verify_nodes over the device-made records, and solve() with level_batch.PARENT_RECORDS_ROUTE on and off.
The CPU side (the twin against today's host code, the wiring through a spy engine) is tests/test_parent_records_host.py."""
import numpy as np
import pytest

from qpn_amd import algorithm, examples, level_batch
from qpn_amd.engine import QpnError
from qpn_amd.level_batch import assemble_parent_records_host, parent_batches

import parent_cases as PC

pytestmark = pytest.mark.gpu

NAMES = ("Qc", "Rc", "qd", "Ac", "Bc", "l", "u", "err")


def to_dev(engine, args):
    import torch
    return tuple(torch.as_tensor(np.ascontiguousarray(a), device=f"cuda:{engine.device}") if isinstance(a, np.ndarray) else a for a in args)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same_bits(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(engine, args, dev):
    want = assemble_parent_records_host(*args)
    got = engine.assemble_parent_nodes(*(to_dev(engine, args) if dev else args))
    for name, w, g in zip(NAMES, want, got):
        assert same_bits(host(g), w), name
    return want


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c[0])
def test_entry_equals_the_twin_on_the_host_cases(engine, case, form, dev):
    net, items = PC.build(case)
    spy = PC.TwinEngine()
    parent_batches(net, items, spy, form)
    assert spy.args
    for args in spy.args:
        assert not check(engine, args, dev)[7].any()


# (form, items, parents, n0, mb, ps, p, pieces, rows, eqs, c, slots, base_eq): one item; 70 items over 3 parents (more items than
# a workgroup has lanes in a wavefront, more than one parent), rows on both sides of the padding; all 8 slots; the mid-size
# shape: 32 base rows and a 64-row piece with 32 equalities, form 1 -> n = 64, m = 64
DIRECT = [(0, 1, 1, 3, 4, 1, 2, 3, 5, 1, 3, 1, True), (1, 1, 1, 3, 4, 1, 2, 3, 5, 1, 3, 1, True),
          (0, 70, 3, 5, 7, 2, 3, 10, 6, 2, 4, 2, True), (1, 70, 3, 5, 7, 2, 3, 10, 6, 2, 4, 2, True),
          (1, 9, 2, 4, 3, 1, 1, 5, 3, 3, 2, 8, True), (0, 9, 2, 4, 3, 1, 1, 5, 3, 0, 2, 8, False),
          (1, 3, 1, 32, 32, 4, 8, 2, 64, 32, 40, 1, False), (0, 3, 1, 32, 32, 4, 8, 2, 64, 32, 40, 1, False)]


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("spec", DIRECT, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_entry_equals_the_twin_on_direct_calls(engine, spec, dev):
    args = PC.random_call(sum(spec), *spec)
    if spec[3] == 32 and spec[0] == 1:
        assert (args[1], args[2]) == (32, 64)                       # the free block is 64 wide over 64 rows
    want = check(engine, args, dev)
    assert not want[7].any() and len(want[7]) == spec[1]


def test_argument_errors_and_the_empty_call(engine):
    args = list(PC.random_call(5, 1, 4, 2, 3, 4, 1, 2, 3, 5, 1, 3, 2))
    out = engine.assemble_parent_nodes(*[a[:0] if k >= 18 else a for k, a in enumerate(args)])          # no items: fine, and empty
    assert host(out[0]).shape == (0, 3 + args[1], 3 + args[1]) and host(out[7]).shape == (0,)
    for k, v in ((2, 1024), (3, 0), (0, 2)):                         # n + m beyond the solver's limit; p = 0; no such form
        bad = list(args); bad[k] = v
        with pytest.raises(QpnError):
            engine.assemble_parent_nodes(*bad)
    bad = list(args); bad[20] = bad[20][:, :7]                      # seven slots
    with pytest.raises(QpnError):
        engine.assemble_parent_nodes(*bad)
    bad = list(to_dev(engine, args)); bad[13] = args[13]            # host and device buffers in one call
    with pytest.raises(QpnError):
        engine.assemble_parent_nodes(*bad)
    check(engine, tuple(args), False)                               # ... and the context is fine afterwards


def test_bad_items_leave_their_neighbours_intact(engine):
    net, items = PC.build(PC.CASES[1])
    spy = PC.TwinEngine()
    parent_batches(net, items, spy, 1)
    base = PC.biggest_call(spy)
    codes = set()
    for name, edit, code in PC.bad_edits(base):
        a = tuple(edit([np.array(v) if isinstance(v, np.ndarray) else v for v in base]))
        want = assemble_parent_records_host(*a)
        assert want[7][0] == code and not want[7][1:].any(), name
        got = engine.assemble_parent_nodes(*to_dev(engine, a))      # device arrays: err tells, the records are the twin's
        for nm, w, g in zip(NAMES, want, got):
            assert same_bits(host(g), w), (name, nm)
        with pytest.raises(QpnError):                               # host arrays: an argument error
            engine.assemble_parent_nodes(*a)
        codes.add(code)
    assert codes == {1, 2, 3, 4, 5}
    check(engine, base, True)


def test_solve_and_verify_take_the_device_made_records(engine):
    """solve_nodes and verify_nodes over the records as the entry left them in device memory answer bit for bit what they answer
    over the host-made records."""
    net, x, S = PC.kinked_pairs()
    leaders = sorted(net.network_depth_map[1])
    items = [(pid, [P]) for pid in leaders for P in S[sorted(net.network_edges[pid])[0]]]
    for form in (0, 1):
        recs = [level_batch.node_record(net, pid, ch) for pid, ch in items]
        want = level_batch.batch_records([level_batch.free_equalities(r) for r in recs] if form else recs)
        got, rest = parent_batches(net, items, engine, form)
        assert rest == [] and len(got) == len(want)
        for g, w in zip(got, want):
            assert g.where == w.where and hasattr(g.dev[0], "is_cuda")
            xd, wv = w.gather(x)
            if form:
                z0 = np.zeros((len(w), w.n + w.m)); z0[:, :w.nx] = xd
                a = engine.solve_nodes(w.Qc, w.Rc, w.qd, w.Ac, w.Bc, w.l, w.u, wv, z0=z0)
                b = g.solve(engine, wv, z0)
                assert same_bits(a["status"], b["status"]) and same_bits(a["z"], b["z"])
            else:
                a = engine.verify_nodes(w.Qc, w.Rc, w.qd, w.Ac, w.Bc, w.l, w.u, xd, wv, tol=1e-4)
                b = g.verify(engine, xd, wv, 1e-4)
                for u, v in zip(a, b):
                    assert same_bits(np.ascontiguousarray(u), np.ascontiguousarray(v))
            for name in ("Qc", "Rc", "qd", "Ac", "Bc", "l", "u"):                    # the one download fills the record arrays
                assert same_bits(getattr(g, name), getattr(w, name)), name


class Recorder:
    """The engine, with the statuses of every solve_nodes / verify_nodes call kept in call order."""

    def __init__(self, engine):
        self._e, self.log = engine, []

    def __getattr__(self, name):
        return getattr(self._e, name)

    def solve_nodes(self, *a, **k):
        res = self._e.solve_nodes(*a, **k)
        self.log.append(("solve", host(res["status"]).tobytes()))
        return res

    def verify_nodes(self, *a, **k):
        res = self._e.verify_nodes(*a, **k)
        self.log.append(("verify", host(res[0]).tobytes(), host(res[2]).tobytes()))
        return res


def _both_routes(engine, make, x0=None):
    out = []
    for route in ("host", "device"):
        level_batch.PARENT_RECORDS_ROUTE = route
        try:
            rec = Recorder(engine)
            before = engine.calls["qpn_assemble_parent_nodes"]
            ret = algorithm.solve(make(), x0, engine=rec) if x0 is not None else algorithm.solve(make(), engine=rec)
            out.append((ret, rec.log, engine.calls["qpn_assemble_parent_nodes"] - before))
        finally:
            level_batch.PARENT_RECORDS_ROUTE = "host"
    (a, la, na), (b, lb, nb) = out
    assert a["solved"] and b["solved"]
    assert same_bits(a["x_opt"], b["x_opt"])
    assert la == lb and len(la) > 0                                 # every sweep's statuses, bit for bit
    assert na == 0 and nb > 0
    return a, b


def test_solve_golden_cases_with_the_route_on(engine):
    import goldenio as G
    c = G.load("simple_bilevel_cases.json")
    for w in c["w"]:
        a, b = _both_routes(engine, lambda: examples.setup("simple_bilevel", gen_solution_map=True), np.array(list(w) + c["x0"], float))
        assert len(a["Sol"][2]) == len(b["Sol"][2])


def test_solve_twenty_pairs_with_the_route_on(engine):
    _both_routes(engine, lambda: examples.setup("synthetic_pairs", pairs=20, n=6, m=8))
