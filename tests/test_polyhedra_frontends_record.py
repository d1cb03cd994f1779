"""The batch front ends of polyhedra.py against tests/golden/polyhedra_frontend_record.json: what they answered, and which engine
calls they made in which order, at the commit before the host layer was last edited (tests/golden/make_polyhedra_frontend_record.py
holds the cases and writes the record).  On the GPU the same cases run through the HIP engine and are compared with the twin engine
of tests/twin_engine.py."""
import importlib.util
import os

import numpy as np
import pytest

import qpn_amd  # noqa: F401
from qpn_amd import polyhedra
from qpn_amd.programs import Poly

import goldenio

NODE_TOL = 1e-9                                  # HIP node solver against the oracle's (tests/test_polyhedra.py's bound)


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_polyhedra_frontend_record",
                                                  os.path.join(goldenio.GOLD, "make_polyhedra_frontend_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_front_ends_answer_and_call_what_the_recorded_commit_did(maker):
    want = goldenio.load("polyhedra_frontend_record.json")["cases"]
    got = maker.record(polyhedra)
    assert sorted(got) == sorted(want) and len(want) == 42
    for name in sorted(want):
        assert got[name].get("raised") == want[name].get("raised"), name
        assert got[name].get("calls") == want[name].get("calls"), name            # the same calls in the same order
        assert got[name].get("result") == want[name].get("result"), name          # dtype, shape and bytes of every array


def test_the_record_mixes_shapes_and_reaches_every_route(maker):
    """What the record is for: every batch packs at least two shapes, the chunked call makes three chunks or more, and the items
    beyond the kernels' limits reach the routes they fall back to."""
    want = goldenio.load("polyhedra_frontend_record.json")["cases"]
    packs = lambda name, method: [args[0] for m, args in want[name]["calls"] if m == method]
    for name, method in (("issubset_batch [twin]", "issubset_pairs"), ("interior_members_batch [twin]", "interior_members"),
                         ("implicit_bounds_batch route=polyhedron [twin]", "implicit_bounds"), ("implicit_bounds_batch route=jobs [twin]", "solve_lps"),
                         ("exemplar_slack_batch route=polyhedron [twin]", "exemplar_polys"), ("exemplar_slack_batch route=None [twin]", "solve_lps"),
                         ("remove_subsets_many prefilter=True [twin]", "members_outside")):
        assert len({s.split(", ", 1)[1] for s in packs(name, method)}) >= 2, name   # ("float64[k, d, r]" -> "d, r]")
    assert len(packs("issubset_batch_chunked [twin]", "issubset_pairs")) >= len(packs("issubset_batch [twin]", "issubset_pairs")) + 2
    methods = lambda name: [m for m, _ in want[name]["calls"]]
    assert "solve_nodes" in methods("issubset_batch beyond [twin]")
    assert methods("exemplar_slack_batch beyond route=polyhedron [twin]")[-1] == "solve_lps"
    assert methods("implicit_bounds_batch beyond route=polyhedron [twin]")[-2:] == ["solve_nodes", "solve_lps"]
    assert want["implicit_bounds_batch empty route=polyhedron [twin]"]["raised"] == "RuntimeError: Empty set (polyhedron 9)"


def test_the_slack_rows_of_a_pack_are_the_rows_of_its_members_stacked(maker):
    """exemplar_rows writes the slack LP once: what _exemplar_slack_lps sends for a pack is what the twin expands per polyhedron."""
    for shape in ((1, 1), (3, 2), (16, 8)):
        A, l, u = (np.stack(v) for v in zip(*[maker.lp_cases.family_case(s, shape=shape)[:3] for s in range(6)]))
        pack = polyhedra.exemplar_rows(A, l, u, 0.5)
        for b in range(6):
            for got, want in zip(pack, polyhedra.exemplar_rows(A[b], l[b], u[b], 0.5)):
                assert got[b].dtype == want.dtype and got[b].shape == want.shape and got[b].tobytes() == want.tobytes()


def _same(got, want, tol, what):
    """got == want: None where None, arrays of one dtype and shape; integers and flags equal, floats bit-equal (tol = 0, NaN in the
    same places) or within tol."""
    if want is None or got is None:
        assert got is None and want is None, what
    elif isinstance(want, Poly):
        _same(got.vectorize(), want.vectorize(), tol, what)
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), what
        for k, (g, w) in enumerate(zip(got, want)):
            _same(g, w, tol, (what, k))
    else:
        g, w = np.asarray(got), np.asarray(want)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
        if tol == 0 or w.dtype.kind != "f":
            assert np.array_equal(g, w, equal_nan=w.dtype.kind == "f"), (what, g, w)
        else:
            with np.errstate(invalid="ignore"):
                assert np.all((g == w) | (np.isnan(g) & np.isnan(w)) | (np.abs(g - w) <= tol)), (what, g, w)


@pytest.mark.gpu
def test_the_hip_engine_answers_what_the_twin_engine_answers(engine, maker):
    """The cases of the record through the HIP engine, host arrays in: bit-equal to the twin engine's answers where the floats come
    from an LP entry (the kernels are bit-equal to the twins), within NODE_TOL where they come from the node solver (the oracle's
    under the twin engine); verdicts, None-ness and error texts equal everywhere.  The batches with an item beyond the kernels'
    limits stay with the record: their fallback is host routing, and the shapes are none the HIP entries take."""
    from twin_engine import TwinEngine
    for name, call, beyond, exact in maker.cases(polyhedra):
        if beyond:
            continue
        want, got = maker.answer(call, TwinEngine()), maker.answer(call, engine)
        assert got.get("raised") == want.get("raised"), name
        if "raised" in want:
            continue
        if isinstance(exact, list):                              # (empty, example, eps) of exemplar_slack_batch, item by item
            (e_g, x_g, eps_g), (e_w, x_w, eps_w) = got["result"], want["result"]
            _same(e_g, e_w, 0, name)
            for b, p in enumerate(exact):
                has_open = hasattr(p, "open_bounds") and bool(np.any(p.open_bounds()))
                _same([x_g[b], eps_g[b]], [x_w[b], eps_w[b]], NODE_TOL if has_open else 0, (name, b))
        else:
            _same(got["result"], want["result"], 0 if exact else NODE_TOL, name)
