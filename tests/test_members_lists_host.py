"""The list-wise member prefilter of remove_subsets_many, host side; the `-m gpu` twin is
tests/test_gpu_members_lists.py.

What is pinned here:
* polyhedra.members_outside_lists_host (the numpy twin of qpn_members_outside_lists, and its normative statement) gives, pair
  for pair, what polyhedra.members_outside_host gives on the enumerated ordered pairs masked by ok: lists of every length
  around a word's edge mixed in one call and interleaved in the pack, a pack that holds only part of its lists' pieces,
  members that are not ok, positions without a member, infinite bounds; undecided is the recount of the zero bits, padding
  bits are 0; a member on a bound, at bound +- t and one ulp beyond;
* every kind of bad item: the device-mode outputs, and that the host-mode rules raise;
* remove_subsets_many with REFUTE_ROUTE = "lists" on a spy engine served by the twins keeps the lists the "pairs" route and
  the route without engine help keep, makes no members_outside call and one members_outside_lists call per pack, and forms no
  matrix for a list with nothing undecided; with the route at its default no members_outside_lists call is made."""
import numpy as np
import pytest

import qpn_amd  # noqa: F401
from qpn_amd import polyhedra

import members_lists_cases as cases
from members_lists_cases import ListsSpy

INF = np.inf


@pytest.mark.parametrize("rj,d", cases.SHAPES)
def test_twin_equals_the_pairwise_twin_on_the_enumerated_pairs(rj, d):
    case = cases.make_case(100 + rj, cases.LENGTHS, rj, d)
    assert len(set(case["list_of"][:20].tolist())) > 3                      # interleaved in the pack
    assert np.any(case["list_mem"] == -1) and np.any(case["ok"] == 0)
    assert np.any(np.isinf(case["lj"])) and np.any(np.isinf(case["uj"]))
    bits, und = polyhedra.members_outside_lists_host(*cases.args_of(case), case["t"])
    ones, zeros = cases.check_against_pairs(case, bits, und)
    assert ones > 100 and zeros > 100                                       # both verdicts occur
    # the host-mode rules accept what the device-mode rules accept here, with the same answer
    b2, u2 = polyhedra.members_outside_lists_host(*cases.args_of(case), case["t"], strict=True)
    assert np.array_equal(b2, bits) and np.array_equal(u2, und)


def test_a_pack_that_holds_part_of_its_lists():
    whole = cases.make_case(7, (33, 5, 70), 9, 4, share=1.0)
    part = cases.make_case(7, (33, 5, 70), 9, 4, share=0.4)
    assert len(part["list_of"]) < len(whole["list_of"]) and np.array_equal(part["list_mem"], whole["list_mem"])
    bits, und = polyhedra.members_outside_lists_host(*cases.args_of(part), part["t"])
    cases.check_against_pairs(part, bits, und)


def test_members_on_a_bound_and_beyond():
    """One piece 0 <= x <= 1 (and a row without bounds), t = 1/4: exactly representable, so every sum is exact."""
    t = 0.25
    up = np.nextafter
    xs = [0.5, 1.0, 1.25, up(1.25, 2.0), 0.0, -0.25, up(-0.25, -1.0), 7.0, 0.5]
    X = np.array([[x, 3.0] for x in xs])
    k = len(xs)
    Ajc = np.array([[[1.0, 0.0], [0.0, 1.0]]])                               # [1, d = 2, rj = 2]: rows x0 and x1
    lj = np.array([[0.0, -INF]]); uj = np.array([[1.0, INF]])
    ok = np.ones(k, np.uint8)
    bits, und = polyhedra.members_outside_lists_host(Ajc, lj, uj, X, ok, [0, k], np.arange(k), [0], [k - 1], [0, 1], t)
    flags, pad = cases.unpack(bits, [0, 1], 0, k)
    #                on l<x<u  on u   u + t  beyond  on l   l - t  beyond  far   own
    assert flags.tolist() == [False, False, False, True, False, False, True, True, False] and not pad.any()
    assert und.tolist() == [5]


def test_small_case_and_the_device_mode_rules_for_bad_items():
    bits, und = cases.run_small()
    assert bits.tolist() == [0b10, 0b110, 0b100] and und.tolist() == [0, 0, 1]
    # a bad list_of: segment 0, undecided 0; its neighbours intact
    for a in (-1, 2, 1 << 30):
        bits, und = cases.run_small(list_of=np.array([0, a, 1], np.int32))
        assert bits.tolist() == [0b10, 0, 0b100] and und.tolist() == [0, 0, 1]
    # a bad self_pos: segment 0, undecided k - 1
    for sp in (-1, 3, 1 << 30):
        bits, und = cases.run_small(self_pos=np.array([0, sp, 1], np.int32))
        assert bits.tolist() == [0b10, 0, 0b100] and und.tolist() == [0, 2, 1]
    # a segment shorter than the list needs (here: none at all)
    bits, und = cases.run_small(word_ptr=np.array([0, 1, 1, 2], np.int64))
    assert bits.tolist() == [0b10, 0b100] and und.tolist() == [0, 2, 1]
    # a segment longer than the list needs: the rest is 0
    bits, und = cases.run_small(word_ptr=np.array([0, 1, 4, 5], np.int64))
    assert bits.tolist() == [0b10, 0b110, 0, 0, 0b100] and und.tolist() == [0, 0, 1]
    # a segment that is not inside bits: nothing of it is written, the piece counts as one with too short a segment
    bits, und = cases.run_small(word_ptr=np.array([0, 1, -1, 1], np.int64))
    assert bits.tolist() == [0b10] and und.tolist() == [0, 2, 2]
    # a list whose list_ptr entries decrease or leave list_mem is a bad list
    bits, und = cases.run_small(list_ptr=np.array([0, 6, 5], np.int32))
    assert bits.tolist() == [0, 0, 0] and und.tolist() == [0, 0, 0]
    # a list_mem entry outside [-1, Bi): that position answers 1 -- but never the piece's own
    for m in (5, -2, 1 << 30):
        mem = np.arange(5, dtype=np.int32); mem[2] = m
        bits, und = cases.run_small(list_mem=mem)
        assert bits.tolist() == [0b10, 0b110, 0b101] and und.tolist() == [0, 0, 0]
    # no member (-1), or a member that is not ok: refutes nothing
    mem = np.arange(5, dtype=np.int32); mem[3] = -1
    bits, und = cases.run_small(list_mem=mem)
    assert bits.tolist() == [0b10, 0b100, 0b100] and und.tolist() == [0, 1, 1]
    okf = np.ones(5, np.uint8); okf[4] = 0
    bits, und = cases.run_small(ok=okf)
    assert bits.tolist() == [0b10, 0b010, 0] and und.tolist() == [0, 1, 2]
    # no lists at all: every segment 0, nothing undecided
    bits, und = cases.run_small(list_ptr=np.array([0], np.int32), list_mem=np.zeros(0, np.int32))
    assert bits.tolist() == [0, 0, 0] and und.tolist() == [0, 0, 0]
    # no pieces
    c = cases.small()
    bits, und = polyhedra.members_outside_lists_host(np.zeros((0, 1, 1)), np.zeros((0, 1)), np.zeros((0, 1)), c["X"], c["ok"], c["list_ptr"],
                                                     c["list_mem"], np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.int64), 1e-5)
    assert bits.shape == (0,) and und.shape == (0,)


@pytest.mark.parametrize("over", [
    dict(list_of=np.array([0, 2, 1], np.int32)), dict(list_of=np.array([-1, 1, 1], np.int32)),
    dict(self_pos=np.array([2, 0, 1], np.int32)), dict(self_pos=np.array([0, 0, -1], np.int32)),
    dict(list_mem=np.array([0, 1, 2, 3, 5], np.int32)), dict(list_mem=np.array([0, -2, 2, 3, 4], np.int32)),
    dict(list_ptr=np.array([0, 3, 2], np.int32)), dict(list_ptr=np.array([1, 2, 5], np.int32)),
    dict(word_ptr=np.array([0, 1, 0, 1], np.int64)), dict(word_ptr=np.array([0, 1, 1, 2], np.int64)),
    dict(word_ptr=np.array([1, 2, 3, 4], np.int64))])
def test_host_mode_rules_raise(over):
    with pytest.raises(ValueError, match="members_outside_lists"):
        cases.run_small(strict=True, **over)


def test_remove_subsets_many_on_the_lists_route(monkeypatch):
    from oracle_engine import OracleEngine
    from twin_engine import TwinEngine
    lists = cases.subset_lists(5)
    plain = polyhedra.remove_subsets_many(lists, OracleEngine())
    assert any(len(k) < len(p) for k, p in zip(plain, lists) if p is not None)       # something IS removed
    pairs = TwinEngine()
    assert cases.kept_ids(polyhedra.remove_subsets_many(lists, pairs)) == cases.kept_ids(plain)
    assert any(m == "members_outside" for m, _ in pairs.log)
    spy = ListsSpy().watch(monkeypatch)
    monkeypatch.setattr(polyhedra, "REFUTE_ROUTE", "lists")
    got = polyhedra.remove_subsets_many(lists, spy)
    assert cases.kept_ids(got) == cases.kept_ids(plain)
    assert spy.count("members_outside") == 0
    packs = spy.count("interior_members")                                   # one pack per interior_members call
    assert packs >= 1 and spy.count("members_outside_lists") == packs
    # a matrix is formed only for a list that left something undecided: never for the separate boxes
    assert spy.matrices and cases.SEPARATE not in spy.matrices
    assert len(spy.matrices) < sum(1 for p in lists if p is not None and len(p) >= 2)
    assert [id(P) for P in got[-3]] == [id(P) for P in lists[-3]] and got[-3] is not lists[-3]
    # pieces of two sizes: two packs, two calls
    wide = [cases.box([0, 0], [1, 1]), cases.box([0.2, 0.2], [0.8, 0.8]), cases.box([5, 5], [6, 6])]
    spy2 = ListsSpy().watch(monkeypatch)
    kept = polyhedra.remove_subsets_many(lists + [wide], spy2)
    assert spy2.count("members_outside_lists") == spy2.count("interior_members") == packs + 1
    assert [id(P) for P in kept[-1]] == [id(wide[0]), id(wide[2])]
    # an engine without the method keeps today's route under "lists"
    old = TwinEngine()
    assert cases.kept_ids(polyhedra.remove_subsets_many(lists, old)) == cases.kept_ids(plain)
    assert any(m == "members_outside" for m, _ in old.log)


def test_default_route_makes_no_lists_call(monkeypatch):
    assert polyhedra.REFUTE_ROUTE == "pairs"
    spy = ListsSpy().watch(monkeypatch)
    lists = cases.subset_lists(6)
    polyhedra.remove_subsets_many(lists, spy)
    assert spy.count("members_outside_lists") == 0 and spy.count("members_outside") >= 1 and not spy.matrices


def test_unknown_route_is_refused(monkeypatch):
    monkeypatch.setattr(polyhedra, "REFUTE_ROUTE", "both")
    with pytest.raises(ValueError, match="REFUTE_ROUTE"):
        polyhedra.remove_subsets_many(cases.subset_lists(6), ListsSpy())
