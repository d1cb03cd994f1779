"""The list-wise member prefilter on the MI355X: qpn_members_outside_lists against its numpy twin, bit for
bit on `bits` and `undecided`, in both memory modes -- the shapes of the CPU side, piece sizes on either side of the LDS budget,
lists that span several workgroups and several visits of one workgroup, no pieces and no lists; the argument errors of host
mode and the bad items of device mode beside intact neighbours; remove_subsets_many and solve() on both routes.  The CPU
side (the twin against the pairwise twin, the call pattern) is tests/test_members_lists_host.py."""
import numpy as np
import pytest

from qpn_amd import algorithm, examples, polyhedra
from qpn_amd.engine import QpnError

import members_lists_cases as cases

pytestmark = pytest.mark.gpu


def to_dev(engine, *arrs):
    import torch
    return tuple(torch.as_tensor(np.ascontiguousarray(a), device=f"cuda:{engine.device}") for a in arrs)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same_as_twin(engine, case, dev):
    want_bits, want_und = polyhedra.members_outside_lists_host(*cases.args_of(case), case["t"])
    args = cases.args_of(case)
    bits, und = engine.members_outside_lists(*(to_dev(engine, *args) if dev else args), case["t"])
    if dev:
        assert hasattr(bits, "cpu") and hasattr(und, "cpu")
    bits, und = host(bits), host(und)
    assert bits.dtype == np.uint32 and und.dtype == np.int32
    assert np.array_equal(und, want_und)
    assert np.array_equal(bits, want_bits)
    ones = int(np.unpackbits(want_bits.view(np.uint8)).sum())
    print(f"Bj={len(und)} words={len(bits)} refuted={ones} undecided={int(want_und.sum())}")
    return ones, int(want_und.sum())


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("rj,d", cases.SHAPES)
def test_entry_equals_the_numpy_twin(engine, rj, d, dev):
    ones, zeros = same_as_twin(engine, cases.make_case(100 + rj, cases.LENGTHS, rj, d), dev)
    assert ones > 100 and zeros > 100


# the piece (A, l, u) goes into LDS while 8 rj (d + 2) <= 78 KiB = 79 872 bytes: (128, 76) is exactly that, (128, 77) the first
# size beyond it, (1024, 40) far beyond: the last two read the piece from global memory
@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("rj,d,lens", [(128, 76, (33, 5, 40)), (128, 77, (33, 5, 40)), (1024, 40, (33, 5))])
def test_either_side_of_the_lds_budget(engine, rj, d, lens, dev):
    ones, zeros = same_as_twin(engine, cases.make_case(rj + d, lens, rj, d), dev)
    assert ones > 20 and zeros > 20


def test_lds_and_global_paths_give_the_same_bits(engine):
    """The same members against the same rows: once as pieces of 76 columns (LDS), once with a 77th column of zeros (global)."""
    a = cases.make_case(5, (33, 70), 128, 76)
    b = dict(a)
    Bj, Bi = a["Ajc"].shape[0], a["X"].shape[0]
    b["Ajc"] = np.ascontiguousarray(np.concatenate([a["Ajc"], np.zeros((Bj, 1, 128))], axis=1))
    b["X"] = np.ascontiguousarray(np.concatenate([a["X"], np.ones((Bi, 1))], axis=1))
    ra = engine.members_outside_lists(*cases.args_of(a), a["t"])
    rb = engine.members_outside_lists(*cases.args_of(b), b["t"])
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[0].any()


@pytest.mark.parametrize("dev", [False, True])
def test_a_list_over_several_workgroups(engine, dev):
    """A list of 2 500 (79 words: three chunks of 32) of which the pack holds a few pieces: the grid gives each piece many
    workgroups, and `undecided` is summed over them."""
    case = cases.make_case(3, (2500, 40), 9, 4, share=0.004)
    assert 4 <= len(case["list_of"]) <= 32 and np.any(case["list_of"] == 0)
    ones, zeros = same_as_twin(engine, case, dev)
    assert ones > 1000 and zeros > 1000


def test_a_list_over_several_visits_of_one_workgroup(engine):
    """2 100 pieces in one pack: one workgroup per piece, which walks the list's 66 words in three visits."""
    case = cases.make_case(4, (2100,), 2, 1, holes=False)
    ones, zeros = same_as_twin(engine, case, True)
    assert ones > 10000 and zeros > 10000


def test_no_pieces_and_no_lists(engine):
    c = cases.small()
    none = dict(c, Ajc=np.zeros((0, 1, 1)), lj=np.zeros((0, 1)), uj=np.zeros((0, 1)), list_of=np.zeros(0, np.int32),
                self_pos=np.zeros(0, np.int32), word_ptr=np.zeros(1, np.int64))
    nolist = dict(c, list_ptr=np.array([0], np.int32), list_mem=np.zeros(0, np.int32))
    for dev in (False, True):
        for case in (none, nolist):
            args = [case[k] for k in cases.ARGS]
            bits, und = engine.members_outside_lists(*(to_dev(engine, *args) if dev else args), 1e-5)
            want = polyhedra.members_outside_lists_host(*args, 1e-5)
            assert np.array_equal(host(bits), want[0]) and np.array_equal(host(und), want[1])
            assert not host(bits).any() and not host(und).any()


def run_small(engine, dev, **over):
    c = cases.small(**over)
    args = [c[k] for k in cases.ARGS]
    bits, und = engine.members_outside_lists(*(to_dev(engine, *args) if dev else args), 1e-5)
    return host(bits), host(und), polyhedra.members_outside_lists_host(*args, 1e-5)


BAD_ITEMS = [dict(list_of=np.array([0, 2, 1], np.int32)), dict(list_of=np.array([0, -1, 1], np.int32)),
             dict(list_of=np.array([0, 1 << 30, 1], np.int32)),
             dict(self_pos=np.array([0, 3, 1], np.int32)), dict(self_pos=np.array([0, -1, 1], np.int32)),
             dict(self_pos=np.array([0, 1 << 30, 1], np.int32)),
             dict(word_ptr=np.array([0, 1, 1, 2], np.int64)),
             dict(list_mem=np.array([0, 1, 5, 3, 4], np.int32)), dict(list_mem=np.array([0, 1, -2, 3, 4], np.int32)),
             dict(list_mem=np.array([0, 1, 1 << 30, 3, 4], np.int32))]


def test_argument_errors_and_bad_items(engine):
    for dev in (False, True):
        bits, und, want = run_small(engine, dev)
        assert bits.tolist() == [0b10, 0b110, 0b100] and und.tolist() == [0, 0, 1] and np.array_equal(bits, want[0])
        # a segment longer than its list needs is legal in both modes: the rest is written 0
        bits, und, want = run_small(engine, dev, word_ptr=np.array([0, 1, 4, 5], np.int64))
        assert bits.tolist() == [0b10, 0b110, 0, 0, 0b100] and und.tolist() == [0, 0, 1]
        # offsets that do not bound their buffers are refused in either mode, before anything is launched
        for over in (dict(word_ptr=np.array([0, 1, -1, 1], np.int64)), dict(word_ptr=np.array([1, 2, 3, 4], np.int64)),
                     dict(list_ptr=np.array([0, 6, 5], np.int32)), dict(list_ptr=np.array([0, 2, 6], np.int32)),
                     dict(list_ptr=np.array([1, 2, 5], np.int32))):
            with pytest.raises(QpnError):
                run_small(engine, dev, **over)
    for over in BAD_ITEMS:
        with pytest.raises(QpnError):                                       # host mode: an index out of range is an error
            run_small(engine, False, **over)
        bits, und, want = run_small(engine, True, **over)                    # device mode: the item answers, its neighbours are intact
        assert np.array_equal(bits, want[0]) and np.array_equal(und, want[1]), over
        assert bits[0] == 0b10 and und[0] == 0
    # beyond the limits
    c = cases.small()
    with pytest.raises(QpnError, match="size"):
        engine.members_outside_lists(np.ones((3, 1, 4097)), np.zeros((3, 4097)), np.ones((3, 4097)), *[c[k] for k in cases.ARGS[3:]], 1e-5)


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


def both_routes(engine, make, x0=None):
    out = []
    for route in ("pairs", "lists"):
        polyhedra.REFUTE_ROUTE = route
        try:
            rec = Recorder(engine)
            before = engine.calls["qpn_members_outside_lists"], engine.calls["qpn_members_outside"]
            ret = algorithm.solve(make(), x0, engine=rec) if x0 is not None else algorithm.solve(make(), engine=rec)
            out.append((ret, rec.log, engine.calls["qpn_members_outside_lists"] - before[0], engine.calls["qpn_members_outside"] - before[1]))
        finally:
            polyhedra.REFUTE_ROUTE = "pairs"
    (a, la, na, pa), (b, lb, nb, pb) = out
    assert a["solved"] and b["solved"]
    assert a["x_opt"].tobytes() == b["x_opt"].tobytes()
    assert la == lb and len(la) > 0                                 # every sweep's statuses, bit for bit
    assert na == 0 and pb == 0                                      # each route makes only its own calls
    return pa, nb


def test_remove_subsets_many_keeps_the_same_lists_on_both_routes(engine):
    seen = []
    orig = algorithm.remove_subsets_many

    def recording(lists, eng, *a, **k):
        seen.append([None if p is None else list(p) for p in lists])
        return orig(lists, eng, *a, **k)
    algorithm.remove_subsets_many = recording
    try:
        ret = algorithm.solve(examples.setup("synthetic_pairs", pairs=12, n=8, m=8), engine=engine)
    finally:
        algorithm.remove_subsets_many = orig
    assert ret["solved"] and seen
    levels = [cases.subset_lists(5)] + seen
    asked = 0
    for lists in levels:
        want = cases.kept_ids(polyhedra.remove_subsets_many(lists, engine))
        engine.calls.clear()
        polyhedra.REFUTE_ROUTE = "lists"
        try:
            got = cases.kept_ids(polyhedra.remove_subsets_many(lists, engine))
        finally:
            polyhedra.REFUTE_ROUTE = "pairs"
        assert got == want
        assert engine.calls["qpn_members_outside"] == 0
        if any(p is not None and len(p) >= 2 for p in lists):
            assert engine.calls["qpn_members_outside_lists"] == engine.calls["qpn_interior_members"] >= 1
            asked += 1
    assert asked >= 2
    assert any(len(k) < len(p) for k, p in zip(polyhedra.remove_subsets_many(levels[0], engine), levels[0]) if p is not None)


def test_solve_golden_cases_on_both_routes(engine):
    import goldenio as G
    c = G.load("simple_bilevel_cases.json")
    assert len(c["w"]) == 8
    for w in c["w"]:
        both_routes(engine, lambda: examples.setup("simple_bilevel", gen_solution_map=True), np.array(list(w) + c["x0"], float))


def test_solve_twenty_pairs_on_both_routes(engine):
    pa, nb = both_routes(engine, lambda: examples.setup("synthetic_pairs", pairs=20, n=6, m=8))
    assert pa > 0 and nb > 0


def test_solve_an_uncapped_net_on_both_routes(engine):
    """max_pieces=None: every local recipe becomes a piece, so the lists are long."""
    longest = []
    orig = algorithm.remove_subsets_many

    def recording(lists, eng, *a, **k):
        longest.append(max([len(p) for p in lists if p is not None], default=0))
        return orig(lists, eng, *a, **k)
    algorithm.remove_subsets_many = recording
    try:
        pa, nb = both_routes(engine, lambda: examples.setup("synthetic_pairs", pairs=40, n=16, m=16, max_pieces=None))
    finally:
        algorithm.remove_subsets_many = orig
    print(f"longest list per level: {longest}")
    assert pa > 0 and nb > 0 and max(longest) >= 64
