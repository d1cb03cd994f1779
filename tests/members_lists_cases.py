"""Seeded inputs of the list-wise member prefilter (qpn_members_outside_lists), shared by
tests/test_members_lists_host.py and tests/test_gpu_members_lists.py, and a spy engine served by the numpy twins."""
from __future__ import annotations

import numpy as np

from qpn_amd import polyhedra
from qpn_amd.programs import Poly
from twin_engine import TwinEngine

INF = np.inf
LENGTHS = (1, 2, 16, 17, 31, 32, 33, 65, 100)                 # a word's edge on either side, one piece alone, several words
SHAPES = ((1, 1), (5, 3), (63, 7), (64, 64), (65, 9), (257, 12))      # (rj, d): around the 64-row chunk, d % 4 = 0 .. 3, several chunks
ARGS = ("Ajc", "lj", "uj", "X", "ok", "list_ptr", "list_mem", "list_of", "self_pos", "word_ptr")


def make_case(seed, lens, rj, d, share=1.0, holes=True):
    """One call's arguments (dict over ARGS, plus t): lists of the lengths `lens`, their pieces interleaved in the pack in a
    seeded order; share < 1 keeps only that share of the pieces in the pack (the others' matrices sit in another pack: their
    members still stand in the lists).  Every piece's bounds are drawn around the members of a random third of its list, a dozen
    in a long list (its own among them), so that both verdicts occur in every list; a fifth of the bounds is infinite; with `holes`, a tenth of the
    positions has no member (-1) and a seventh of the members is not ok."""
    g = np.random.default_rng(seed)
    lens = list(lens)
    ptr = np.zeros(len(lens) + 1, np.int64); ptr[1:] = np.cumsum(lens)
    total = int(ptr[-1])
    Bi = total + 3
    X = g.standard_normal((Bi, d))
    rows = g.permutation(Bi)[:total]
    list_mem = rows.astype(np.int32)
    ok = np.ones(Bi, np.uint8)
    if holes:
        list_mem[g.random(total) < 0.1] = -1
        ok[g.random(Bi) < 0.15] = 0
    order = g.permutation(total)
    order = order[:max(1, int(round(share * total)))]
    la = np.searchsorted(ptr, order, side="right") - 1          # the list of each piece of the pack
    sp = order - ptr[la]
    Bj = len(order)
    A = g.standard_normal((Bj, rj, d))
    lj = np.empty((Bj, rj)); uj = np.empty((Bj, rj))
    for j in range(Bj):
        k = lens[la[j]]
        inside = np.nonzero(g.random(k) < min(1 / 3, 12 / k))[0].tolist() + [int(sp[j])]
        ax = A[j] @ X[rows[ptr[la[j]] + np.array(inside)]].T    # [rj, members inside]
        lj[j] = ax.min(1) - 1e-3; uj[j] = ax.max(1) + 1e-3
    lj[g.random((Bj, rj)) < 0.2] = -INF; uj[g.random((Bj, rj)) < 0.2] = INF
    kk = np.array([lens[a] for a in la], np.int64)
    word_ptr = np.zeros(Bj + 1, np.int64); word_ptr[1:] = np.cumsum(-(-kk // 32))
    return dict(Ajc=np.ascontiguousarray(np.swapaxes(A, 1, 2)), lj=lj, uj=uj, X=X, ok=ok, list_ptr=ptr.astype(np.int32),
                list_mem=list_mem, list_of=la.astype(np.int32), self_pos=sp.astype(np.int32), word_ptr=word_ptr, t=1e-5)


def args_of(case):
    return [case[k] for k in ARGS]


def unpack(bits, word_ptr, j, k):
    """The k bits of piece j's segment, and the rest of the segment (padding) as one array of bits."""
    seg = np.ascontiguousarray(np.asarray(bits)[int(word_ptr[j]):int(word_ptr[j + 1])], dtype="<u4")
    flat = np.unpackbits(seg.view(np.uint8), bitorder="little").astype(bool)
    return flat[:k], flat[k:]


def by_pairs(case):
    """What the entry has to give, from polyhedra.members_outside_host on the enumerated ordered pairs, masked by ok:
    [(flags [k] bool, undecided)] per piece of the pack."""
    ptr, mem = case["list_ptr"].astype(np.int64), case["list_mem"].astype(np.int64)
    out = []
    pi, pj, where = [], [], []
    for j in range(len(case["list_of"])):
        a, sp = int(case["list_of"][j]), int(case["self_pos"][j])
        for s in range(int(ptr[a + 1] - ptr[a])):
            m = int(mem[ptr[a] + s])
            if s != sp and m >= 0:
                pi.append(m); pj.append(j); where.append((j, s))
    verdict = polyhedra.members_outside_host(case["Ajc"], case["lj"], case["uj"], case["X"], np.array(pi, np.int64), np.array(pj, np.int64),
                                             case["t"]).astype(bool)
    verdict &= case["ok"][np.array(pi, np.int64)].astype(bool)
    flags = [np.zeros(int(ptr[a + 1] - ptr[a]), bool) for a in case["list_of"]]
    for (j, s), v in zip(where, verdict):
        flags[j][s] = v
    for j, f in enumerate(flags):
        out.append((f, len(f) - 1 - int(f.sum())))
    return out


def check_against_pairs(case, bits, undecided):
    bits = np.asarray(bits); undecided = np.asarray(undecided)
    assert bits.dtype == np.uint32 and bits.shape == (int(case["word_ptr"][-1]),)
    assert undecided.dtype == np.int32 and undecided.shape == (len(case["list_of"]),)
    both = [0, 0]
    for j, (want, und) in enumerate(by_pairs(case)):
        got, pad = unpack(bits, case["word_ptr"], j, len(want))
        assert np.array_equal(got, want), f"piece {j}"
        assert not pad.any(), f"piece {j}: padding bits set"
        assert int(undecided[j]) == und == int(np.sum(~got)) - 1, f"piece {j}"
        both[0] += int(want.sum()); both[1] += und
    return both


def small(**over):
    """Three pieces (rj = 1, d = 1) of two lists: list 0 = rows (0, 1), list 1 = rows (2, 3, 4); piece x in [0, 1]."""
    c = dict(Ajc=np.ones((3, 1, 1)), lj=np.zeros((3, 1)), uj=np.ones((3, 1)), X=np.array([[0.5], [5.0], [0.5], [5.0], [9.0]]),
             ok=np.ones(5, np.uint8), list_ptr=np.array([0, 2, 5], np.int32), list_mem=np.arange(5, dtype=np.int32),
             list_of=np.array([0, 1, 1], np.int32), self_pos=np.array([0, 0, 1], np.int32), word_ptr=np.array([0, 1, 2, 3], np.int64))
    c.update(over)
    return c


def run_small(strict=False, **over):
    c = small(**over)
    return polyhedra.members_outside_lists_host(*[c[k] for k in ARGS], 1e-5, strict=strict)


def box(lo, hi):
    lo = np.asarray(lo, dtype=np.float64); hi = np.asarray(hi, dtype=np.float64)
    return Poly(np.eye(len(lo)), lo, hi)


def subset_lists(seed, count=6, d=3):
    """Lists of boxes for remove_subsets_many: per list a few seeded boxes, and of some of them a strictly smaller box inside
    (a true subset), a duplicate, and a neighbour that shares a face (merely touching); then a list of separate boxes (nothing
    is left undecided there) of a length no other list has, a single piece and an absent list."""
    g = np.random.default_rng(seed)
    lists = []
    for n in range(count):
        polys = []
        for b in range(int(g.integers(2, 6))):
            lo = g.uniform(-3, 3, d); hi = lo + g.uniform(0.5, 2.0, d)
            polys.append(box(lo, hi))
            what = int(g.integers(0, 4))
            if what == 0:
                polys.append(box(lo + 0.1, hi - 0.1))
            elif what == 1:
                polys.append(box(lo, hi))
            elif what == 2:
                shift = np.zeros(d); shift[0] = hi[0] - lo[0]
                polys.append(box(lo + shift, hi + shift))
        order = g.permutation(len(polys))
        lists.append([polys[i] for i in order])
    apart = [box(np.full(d, 1.5 * i - 9), np.full(d, 1.5 * i - 8)) for i in range(SEPARATE)]
    return lists + [apart, [box(np.zeros(d), np.ones(d))], None]


SEPARATE = 13                                                   # the length of the list of separate boxes


def kept_ids(kept):
    return [None if polys is None else [id(P) for P in polys] for polys in kept]


class ListsSpy(TwinEngine):
    """The twin engine with members_outside_lists served by its numpy twin (host-mode rules: a bad index raises); it also
    records the list lengths for which polyhedra forms a refutation matrix (watch())."""

    def __init__(self):
        super().__init__()
        self.matrices = []

    def members_outside_lists(self, Ajc, lj, uj, X, ok, list_ptr, list_mem, list_of, self_pos, word_ptr, t):
        assert list_ptr.dtype == np.int32 and list_mem.dtype == np.int32 and list_of.dtype == np.int32
        assert self_pos.dtype == np.int32 and word_ptr.dtype == np.int64 and np.asarray(ok).dtype == np.uint8
        self._note("members_outside_lists", Ajc, lj, uj, X, ok, list_ptr, list_mem, list_of, self_pos, word_ptr)
        return polyhedra.members_outside_lists_host(Ajc, lj, uj, X, ok, list_ptr, list_mem, list_of, self_pos, word_ptr, t, strict=True)

    def watch(self, monkeypatch):
        orig = polyhedra._refuted_matrix

        def counted(k, cols, segs):
            self.matrices.append(k)
            return orig(k, cols, segs)
        monkeypatch.setattr(polyhedra, "_refuted_matrix", counted)
        return self

    def count(self, method):
        return sum(1 for m, _ in self.log if m == method)
