"""The labelled walk and the batch of tests/stage_b_transitions.py through the CPU oracle: the walk is the oracle's on every
node, the batch takes every ordered pair of iteration kinds that the module writes down, and at n = m = 32 those pairs include
every hand-over of loop-carried state that the Stage B pivot loop of csrc/qpn_avi_schur.hip has.  A batch that lost a
transition fails here, before it fails to test anything on the device."""
import numpy as np
import pytest

import stage_b_cases as S
import stage_b_lemke as L
import stage_b_transitions as T


@pytest.mark.parametrize("n,m", T.SHAPES)
def test_the_labelled_walk_is_the_oracles_on_every_node(oracle, n, m):
    o = oracle.default_opts()
    recs, names = T.batch(n, m)
    assert len(names) <= 300
    wks = T.walks(n, m, o.piv_tol, o.feas_tol)
    for label, w, mp in T.runs(n):
        ref = S.oracle_solve(oracle, recs, w, max_pivots=mp)
        for i, nm in enumerate(names):
            wk = wks[label][i]
            if wk is None:
                assert nm == "equal"                    # (declined: not a node of this loop)
                continue
            assert (wk["status"], wk["pivots"]) == (ref["status"][i], ref["pivots"][i] - n), (label, nm)
            # one name per iteration that pivots, and one for the exit that is no pivot of its own
            extra = 1 if wk["kinds"] and wk["kinds"][-1] in ("exit_ray", "exit_budget") else 0
            assert len(wk["kinds"]) == wk["pivots"] + extra, (label, nm)
            assert all(T.base(k) not in T.EXITS for k in wk["kinds"][:-1]), (label, nm)
            if mp == 0:
                # ... and it is the walk of tests/stage_b_lemke.py: same status, count and flips
                ref_wk = L.walk(*(c[i] for c in recs), w, o.piv_tol, o.feas_tol)
                assert (wk["status"], wk["pivots"], wk["flips"]) == (ref_wk["status"], ref_wk["pivots"], ref_wk["flips"]), (label, nm)
                flips = [+1 if k == "flip_up" else -1 for k in map(T.base, wk["kinds"]) if k.startswith("flip")]
                assert flips == wk["flips"], (label, nm)
        if mp == 0:
            assert (ref["status"] == S.SUCCESS).sum() >= len(names) - 2, label      # all but `ray` solve (`equal` by the general route)


@pytest.mark.parametrize("n,m", T.SHAPES)
def test_the_batch_covers_every_pair_that_is_written_down(oracle, n, m):
    o = oracle.default_opts()
    got = T.covered(n, m, o.piv_tol, o.feas_tol)
    want = set(T.COVERED[(n, m)])
    assert len(want) == len(T.COVERED[(n, m)])
    assert want <= got, sorted(want - got)
    assert got <= want, ("pairs the constant does not name", sorted(got - want))


def test_the_one_sided_nodes_solve_and_hand_an_infinite_limit_on(oracle):
    """Ids 9000 .. 9059 with a third of the rows bounded below only and a third above only all solve at the shared parameters, and
    reach `one-sided d_k leaves` followed by both kinds of p_k pivot at n = m = 32 and n = m = 16 (one of them at (20, 12))."""
    o = oracle.default_opts()
    for n, m in T.SHAPES:
        recs, names = T.batch(n, m)
        idx = [i for i, nm in enumerate(names) if nm.startswith("one_sided_")]
        assert len(idx) == T.NATURAL
        ref = S.oracle_solve(oracle, recs, T.WS, np.array(idx))
        assert np.all(ref["status"] == S.SUCCESS), (n, m)
        got = set()
        for i in idx:
            got |= T.pairs_of([T.base(k) for k in T.walks(n, m, o.piv_tol, o.feas_tol)["ws"][i]["kinds"]])
        want = {("d_one", "p_lo"), ("d_one", "p_hi")} if m >= 16 else {("d_one", "p_lo")}
        assert want <= got, (n, m, sorted(want - got))


def test_the_pairs_at_32_hold_every_hand_over_of_carried_state():
    pairs = {(T.base(a), T.base(b)) for a, b in T.COVERED[(32, 32)]}
    P_, D_, F_ = ("p_lo", "p_hi"), ("d_two", "d_one", "d_free"), ("flip_up", "flip_dn")

    def some(As, Bs):
        return any((a, b) in pairs for a in As for b in Bs)

    for a in P_:
        for b in P_:
            assert (a, b) in pairs, (a, b)                       # p -> p in all four sign combinations
    assert some(P_, D_) and some(D_, P_) and some(D_, D_)
    assert some(("d_one",), P_)                                  # the infinite limit of a one-sided pair handed to a p_k pivot
    assert some(D_, ("flip_up",)) and some(D_, ("flip_dn",))     # d -> flip in both directions
    assert some(F_, P_) and some(F_, D_)
    assert some(("first",), P_)
    assert any("+tie" in a or "+tie" in b for a, b in T.COVERED[(32, 32)])     # a tie-break row choice
    # each exit, behind some iteration -- but for `exit_art_flip`, which no node can take (docstring of
    # tests/stage_b_transitions.py: a row always blocks the artificial variable in the only iteration in which it is nonbasic),
    # and `exit_fail`, which no well-posed node takes
    for x in ("exit_art_leaves", "exit_ray", "exit_budget"):
        assert any(b == x for _, b in pairs), x
    assert not any(b in ("exit_art_flip", "exit_fail") for _, b in pairs)
