"""qpn_project_pieces (local_pieces_kernel + project_pieces_kernel, csrc/qpn_project.hip) on the HIP engine over the cases of
tests/project_cases.py: bit for bit against the CPU twin (level_batch.project_pieces_host) over the whole arrays, device mode
against host mode, as SETS against the LP reference with the constants fixed on the CPU, the cap rule (flag 4, all fill, and the
context still good afterwards), a call that the ABI splits into chunks, pieces that are not degenerate against
qpn_reduced_pieces, the host-side refusals, and solve() through the one call per round.  CPU side: tests/test_project_pieces_host.py."""
import numpy as np
import pytest

import project_cases as pc
import reduced_cases as rc

pytestmark = pytest.mark.gpu

NAMES = ("Ar", "lr", "ur", "rows", "flags")
INF = np.inf


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda:0")


def _host(out):
    return [a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a) for a in out]


def _same_bits(want, got, what):
    for nm, a, b in zip(NAMES, want, got):
        a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, nm, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (what, nm, np.argwhere(~((a == b) | ((a != a) & (b != b))))[:4].tolist())


def _both_modes(engine, c):
    """engine.project_pieces on host arrays and on device tensors; the two bit-equal.  -> the host-mode output."""
    import torch
    got = _host(engine.project_pieces(*c["args"], c["K"], c["node_of"], cap=c["cap"]))
    gd = engine.project_pieces(*[_dev(a) for a in c["args"]], _dev(c["K"]), _dev(c["node_of"]), cap=c["cap"])
    torch.cuda.synchronize()
    _same_bits(got, _host(gd), "device mode vs host mode")
    return got


@pytest.mark.parametrize("name", pc.CASES)
def test_project_pieces_equals_the_twin_and_is_the_projection(engine, oracle, name):
    """Per case: every output equals the twin's bit for bit over the WHOLE arrays (the fill beyond rows[t] included), device mode
    equals host mode, and the rows pass the set-level check with the constants fixed on the CPU."""
    c = pc.case(name)
    got = _both_modes(engine, c)
    _same_bits(pc.twin_output(name), got, "twin vs engine")
    worst, least = pc.check_projection(got, pc.points(name))
    print(f"{name}: rows {got[3].tolist()}, worst inside violation {worst:.3e} (TAU_IN {pc.TAU_IN:.2e}), smallest outside {least:.3e}")


def test_cap_overflow_gives_flag_4_and_the_context_stays_good(engine, oracle):
    """(64, 65, 2) (b) at cap = 194 < the 1101 rows its step makes: flag 4, rows 0, all fill, in both modes -- and the next call
    on the same context is right."""
    c = pc.case(pc.OVERFLOW)
    got = _both_modes(engine, c)
    assert got[4].tolist() == [4] and got[3].tolist() == [0]
    assert not got[0].any() and np.all(got[1] == -INF) and np.all(got[2] == INF)
    _same_bits(pc.twin_output(pc.OVERFLOW), got, "twin vs engine")
    after = pc.case("5-6-3")
    _same_bits(pc.twin_output("5-6-3"), _host(engine.project_pieces(*after["args"], after["K"], after["node_of"], cap=after["cap"])),
               "the call after an overflow")


def test_project_pieces_in_chunks(engine, oracle):
    """cap = 2^18 at (5, 6, 3): one piece's rows take 59 MB of the workspace, so the ABI serves 13 pieces in two chunks (seven fit
    512 MiB); device mode, checked there.  Every piece equals the small-cap call on its rows, and nothing but fill lies beyond."""
    import torch
    c = pc.case("5-6-3")
    reps = 5
    K = np.concatenate([c["K"]] * reps)[:13]; node_of = np.concatenate([c["node_of"]] * reps)[:13]
    want = pc.twin_output("5-6-3")
    cap = 1 << 18
    Ar, lr, ur, rows, flags = engine.project_pieces(*[_dev(a) for a in c["args"]], _dev(K), _dev(node_of), cap=cap)
    torch.cuda.synchronize()
    assert tuple(Ar.shape) == (13, 8, cap)
    small = c["cap"]
    k = len(c["K"])
    for t in range(13):
        got = [Ar[t:t + 1, :, :small], lr[t:t + 1, :small], ur[t:t + 1, :small], rows[t:t + 1], flags[t:t + 1]]
        _same_bits([a[t % k:t % k + 1] for a in want], _host(got), f"piece {t}")
    assert not bool(Ar[:, :, small:].any()) and bool((lr[:, small:] == -INF).all()) and bool((ur[:, small:] == INF).all())
    del Ar, lr, ur
    torch.cuda.empty_cache()


def test_project_pieces_equals_reduced_pieces_where_nothing_is_degenerate(engine, oracle):
    """Pieces without a leftover column: the first n + 2m rows are qpn_reduced_pieces' output bit for bit, the rest is fill."""
    shape = (5, 6, 3)
    n, m, p = shape
    c = rc.case(shape, "gauss")
    want = _host(engine.reduced_pieces(*c["args"], c["K"], c["node_of"]))
    got = _host(engine.project_pieces(*c["args"], c["K"], c["node_of"]))
    cap0 = n + 2 * m
    assert got[0].shape[2] > cap0 and not want[4].any()
    _same_bits(want, [got[0][:, :, :cap0], got[1][:, :cap0], got[2][:, :cap0], got[3], got[4]], "reduced vs project")
    assert not got[0][:, :, cap0:].any() and np.all(got[1][:, cap0:] == -INF) and np.all(got[2][:, cap0:] == INF)
    # and without node_of piece t reads record t
    two = _host(engine.project_pieces(*c["args"], c["K"][[0, len(c["K"]) - 1]], None))
    assert c["node_of"][0] == 0 and c["node_of"][-1] == 1
    for a, b in zip(two, got):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[len(c["K"]) - 1].tobytes()


def test_project_pieces_refusals(engine):
    """What the entry refuses on the host, before anything is launched."""
    from qpn_amd.engine import QpnError
    from qpn_amd._lib import MEM_HOST
    import ctypes as C

    def zeros(n, m, p):
        return (np.zeros((1, n, n)), np.zeros((1, p, n)), np.zeros((1, n)), np.zeros((1, n, m)), np.zeros((1, p, m)),
                np.zeros((1, m)), np.zeros((1, m)), np.zeros((1, n + m), np.uint8), np.zeros(1, np.int32))

    with pytest.raises(QpnError, match="cap < n \\+ 2m"):
        engine.project_pieces(*zeros(5, 6, 3), cap=16)
    with pytest.raises(QpnError, match="n \\+ m <= 512"):
        engine.project_pieces(*zeros(257, 256, 1))
    with pytest.raises(QpnError, match="bad tolerance"):
        engine.project_pieces(*zeros(5, 6, 3), tol=-1.0)
    # a cap of which not even one piece fits the workspace: QPN_ERR_SIZE, straight at the ABI (no output of that size is made)
    Q, R, q, A, B, l, u, K, no = zeros(5, 6, 3)
    one = np.zeros(1); i1 = np.zeros(1, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    rc_ = engine.lib.qpn_project_pieces(engine.ctx, 1, 1, 5, 6, 3, ptr(Q), ptr(R), ptr(q), ptr(A), ptr(B), ptr(l), ptr(u), ptr(no), ptr(K),
                                        1e-9, 1 << 30, ptr(one), ptr(one), ptr(one), ptr(i1), ptr(i1), MEM_HOST)
    assert engine.lib.qpn_strerror(rc_).decode() == "problem size not supported"
    rc_ = engine.lib.qpn_project_pieces(engine.ctx, 1, 1, 5, 6, 3, ptr(Q), ptr(R), ptr(q), ptr(A), ptr(B), ptr(l), ptr(u), ptr(no), ptr(K),
                                        1e-9, 16, ptr(one), ptr(one), ptr(one), ptr(i1), ptr(i1), MEM_HOST)
    assert engine.lib.qpn_strerror(rc_).decode() == "bad argument"


@pytest.mark.parametrize("max_pieces", [64, None])
def test_solve_takes_the_one_call_per_round(engine, oracle, max_pieces):
    """Config 2, seed 1, through solve() on the HIP engine, capped (the host reader) and with every solution graph (the device
    reader): it ends solved, at the oracle engine's point (1e-8) as tests/test_config2_end_to_end.py asks of it; its flagged pieces
    went through qpn_project_pieces, and qpn_local_pieces was not called for any of them."""
    from oracle_engine import OracleEngine
    from qpn_amd import algorithm, examples

    def run(eng):
        net = examples.setup("robust_avoid_simple", seed=1)
        net.options.max_pieces = max_pieces
        ret = algorithm.solve(net, engine=eng)
        assert ret["solved"]
        return ret["x_opt"]
    before = dict(engine.calls)
    xh = run(engine)
    assert engine.calls["qpn_project_pieces"] - before.get("qpn_project_pieces", 0) >= 1
    assert engine.calls["qpn_local_pieces"] - before.get("qpn_local_pieces", 0) == 0
    xo = run(OracleEngine())
    assert np.max(np.abs(xh - xo)) <= 1e-8
