"""level_batch.solution_pieces against the record of the commit before its three bodies became one pipeline
(tests/golden/solution_pieces_record.json, written by tests/golden/make_solution_pieces_record.py from that commit's file): the
pieces of every item Poly by Poly, the warnings, `truncated`, the exceptions and the engine's call counts, on small levels under
every setting of max_pieces, _chunk and exploration_vertices and on both oracle engines."""
import collections
import importlib.util
import json
import os

import pytest

import goldenio


@pytest.fixture(scope="module")
def recomputed():
    spec = importlib.util.spec_from_file_location("make_solution_pieces_record", os.path.join(goldenio.GOLD, "make_solution_pieces_record.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    stats = collections.Counter()
    return mk.record(mk.load_pipeline(), stats), stats


def test_the_cases_reach_every_branch(recomputed):
    """Without these the record proves nothing: the routes can differ only where pieces are flagged, merged, missed by the point,
    kept as a fallback, cut by the cap, filtered against an earlier product, or spread over several rounds."""
    _, stats = recomputed
    for what in ("flagged", "merge candidates", "non-members", "fallbacks", "cuts by the cap", "items with several products",
                 "uncapped items over several rounds"):
        assert stats[what] >= 1, what


def test_solution_pieces_equal_the_record(recomputed):
    (got, lists), _ = recomputed
    record = goldenio.load("solution_pieces_record.json")
    want = record["cases"]
    assert sorted(got) == sorted(want)
    # an item's Polys by their digests, whatever number the list has on either side
    polys = lambda entry, table: [None if g is None else table[g] for g in entry.get("polys", [])]
    for case in sorted(want):
        assert polys(got[case], lists) == polys(want[case], record["polys"]), case
        rest = lambda entry: {k: v for k, v in entry.items() if k != "polys"}
        assert json.loads(json.dumps(rest(got[case]))) == rest(want[case]), case


def test_an_item_with_more_recipes_than_an_int64_holds_keeps_its_first_pieces(recomputed):
    """64 weakly active rows, 2^64 recipes: the cap's first recipes are expanded, and the warning names the count."""
    (got, _), _ = recomputed
    for cap in (2, 3, 64):
        entry = got[f"counterexample d=64 max_pieces={cap} chunk=None E=0 [oracle]"]
        assert entry["pieces"] == [cap] and "18446744073709551616 local recipes" in entry["warnings"][0]
