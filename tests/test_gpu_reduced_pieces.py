"""qpn_reduced_pieces (local_pieces_kernel + reduce_pieces_kernel) on the HIP engine, in every size class of its strided loops and
on degenerate pieces: its output checked as SETS against the elimination-free reference of tests/reduced_cases.py with the
constants fixed on the CPU, bit for bit against the CPU twin over the whole arrays, device mode against host mode, the flags of
constructed degenerate pieces, a record index out of range, and the host-side refusals.  CPU side of the same cases:
tests/test_reduced_pieces_host.py."""
import numpy as np
import pytest

import reduced_cases as rc

pytestmark = pytest.mark.gpu

NAMES = ("Ar", "lr", "ur", "rows", "flags")


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda:0")


def _host(out):
    return [a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a) for a in out]


def _same_bits(want, got, what):
    for nm, a, b in zip(NAMES, want, got):
        a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, nm)
        assert a.tobytes() == b.tobytes(), (what, nm, np.argwhere(~((a == b) | ((a != a) & (b != b))))[:4].tolist())


def _both_modes(engine, args, K, node_of):
    """engine.reduced_pieces on host arrays and on device tensors; the two bit-equal.  -> the host-mode output."""
    import torch
    got = _host(engine.reduced_pieces(*args, K, node_of))
    gd = engine.reduced_pieces(*[_dev(a) for a in args], _dev(K), _dev(node_of))
    torch.cuda.synchronize()
    _same_bits(got, _host(gd), "device mode vs host mode")
    return got


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_reduced_pieces_are_the_reference_sets_and_equal_the_twin(engine, oracle, case):
    """Per shape and kind: the pieces let in the reference's inside points (TAU_IN, measured on the CPU twin) and keep out its
    outside and off-manifold points; every output equals the twin's bit for bit over the WHOLE arrays -- beyond rows[t] the
    kernel writes zeros into Ar and (-inf, +inf) into lr, ur, as include/qpn_hip.h states --; device mode equals host mode."""
    shape, kind = case
    c = rc.case(shape, kind)
    assert len(c["K"]) <= 8
    rc.check_balance(shape, c["points"])
    got = _both_modes(engine, c["args"], c["K"], c["node_of"])
    worst = rc.check_pieces(got, c["points"])
    print(f"{rc.case_id(case)}: {len(c['K'])} pieces, worst inside violation {worst:.3e} (TAU_IN {rc.TAU_IN:.2e})")
    _same_bits(rc.twin_output(shape, kind), got, "twin vs engine")
    cap = shape[0] + 2 * shape[1]
    for t, r in enumerate(got[3]):                                    # the fill, stated on its own
        assert not got[0][t][:, r:].any() and np.all(got[1][t][r:] == -np.inf) and np.all(got[2][t][r:] == np.inf)
        assert 0 <= r <= cap


@pytest.mark.parametrize("shape", rc.FLAG_SHAPES, ids=str)
def test_flags_of_degenerate_pieces(engine, oracle, shape):
    """Flags as constructed (reduced_cases.degenerate) and equal to the twin's; the pieces next to the degenerate ones are clear
    and pass the set-level check.  A flagged piece's output is incomplete by the header: only its flag is asserted."""
    from oracle_engine import OracleEngine
    d = rc.degenerate(shape)
    got = _both_modes(engine, d["args"], d["K"], d["node_of"])
    assert got[4].tolist() == d["flags"].tolist(), list(zip(d["names"], got[4].tolist()))
    want = OracleEngine().reduced_pieces(*d["args"], d["K"], d["node_of"])
    assert np.array_equal(want[4], got[4]) and np.array_equal(want[3], got[3])
    for t, pts in d["points"].items():
        rc.check_piece(got[0][t], got[1][t], got[2][t], got[3][t], pts)


def test_reduced_pieces_bad_node_index(engine, oracle):
    """node_of outside 0 .. nodes-1: an argument error for host arrays; for DEVICE arrays (which the host does not read) the piece
    comes back empty -- rows = 0, flags = 0, the fill everywhere -- and the pieces next to it are what they are without it."""
    import torch
    from qpn_amd.engine import QpnError
    c = rc.case((5, 6, 3), "gauss")
    K = c["K"][[0, 1, len(c["K"]) - 1, 2]]
    good = np.array([c["node_of"][0], 0, c["node_of"][-1], 0], np.int32)
    bad = good.copy(); bad[1] = rc.NODES; bad[3] = -1
    with pytest.raises(QpnError):
        engine.reduced_pieces(*c["args"], K, bad)
    ref = _host(engine.reduced_pieces(*c["args"], K, good))
    got = engine.reduced_pieces(*[_dev(a) for a in c["args"]], _dev(K), _dev(bad))
    torch.cuda.synchronize()
    got = _host(got)
    for t in (1, 3):
        assert got[3][t] == 0 and got[4][t] == 0
        assert not got[0][t].any() and np.all(got[1][t] == -np.inf) and np.all(got[2][t] == np.inf)
    for t in (0, 2):
        for nm, a, b in zip(NAMES, ref, got):
            assert a[t].tobytes() == b[t].tobytes(), (nm, t)
        assert got[3][t] == 11


def test_reduced_pieces_refusals(engine):
    """Sizes and tolerances the entry refuses on the host, before anything is launched (qpn_capi.hip: pieces_check, then the
    tolerance and the LDS budget, all ahead of the staging)."""
    from qpn_amd.engine import QpnError

    def zeros(n, m, p):
        return (np.zeros((1, n, n)), np.zeros((1, p, n)), np.zeros((1, n)), np.zeros((1, n, m)), np.zeros((1, p, m)),
                np.zeros((1, m)), np.zeros((1, m)), np.zeros((1, n + m), np.uint8), np.zeros(1, np.int32))

    with pytest.raises(QpnError, match="n \\+ m <= 512"):
        engine.reduced_pieces(*zeros(257, 256, 1))
    with pytest.raises(QpnError, match="too many parameters"):       # 61448 bytes of LDS, the limit is 61440
        engine.reduced_pieces(*zeros(256, 256, 3457))
    with pytest.raises(QpnError, match="bad tolerance"):
        engine.reduced_pieces(*zeros(5, 6, 3), tol=float("nan"))
    with pytest.raises(QpnError, match="bad tolerance"):
        engine.reduced_pieces(*zeros(5, 6, 3), tol=-1.0)
