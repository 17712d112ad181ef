"""Subset analyses, pinned to the reference (no GPU): the oracle run on a
subset's samples only (tests/subset_cases.py) equals what the reference itself
computes on the kept tables of every subset -- build_graph + SampleSimilarity
over the tables whose two samples are both kept, as after make_subset
(tests/golden/subsets.json, captured by tests/golden/make_golden_subsets.py) --
and a subset's result is not a restriction of the full run's."""
import json
import os

import pytest

import subset_cases as sc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "subsets.json")


@pytest.fixture(scope="module")
def recorded():
    from test_oracle_golden_ties import load_ties
    d = json.load(open(GOLDEN))
    fx = next(f for f in load_ties()[3] if f["name"] == d["fixture"])
    assert fx["samples"] == d["samples"] and len(fx["samples"]) == 4
    assert [tuple(s) for s in d["settings"]] == sc.SUBSET_SETTINGS
    return d, fx


@pytest.mark.parametrize("top,keep", sc.SUBSET_SETTINGS)
def test_oracle_on_the_subset_is_the_reference_on_the_kept_tables(recorded, top, keep):
    d, fx = recorded
    exp = d["expected"][f"{top}-{keep}"]
    subsets = sc.all_subsets(4)
    assert sorted(exp) == sorted(sc.subset_key(ids) for ids in subsets) and len(subsets) == 11
    samples = fx["samples"]
    for ids in subsets:
        want, got = exp[sc.subset_key(ids)], sc.oracle_subset(samples, fx["hits"], ids, top, keep)
        assert got["sample_count"] == want["sample_count"] == len(ids), ids
        assert sorted([samples.index(s), g] for s, g in got["valid"]) == want["valid"], ids
        assert got["sums"] == want["sums"], ids
        if want["matrix"] is None:
            assert got["matrix"] is None, ids
        else:
            assert [samples.index(s) for s in got["matrix"]["labels"]] == want["matrix"]["labels"], ids
            assert got["matrix"]["values"] == want["matrix"]["values"], ids


def test_full_set_subset_is_the_recorded_full_run(recorded):
    """The subset of all four samples is the run post_alignment_ties.json records."""
    d, fx = recorded
    for top, keep in sc.SUBSET_SETTINGS:
        full, sub = fx["expected"][f"{top}-{keep}"], d["expected"][f"{top}-{keep}"][sc.subset_key(range(4))]
        assert sub["sample_count"] == full["sample_count"]
        assert sub["valid"] == sorted([fx["samples"].index(s), g] for s, g in full["valid"])
        assert sub["matrix"]["values"] == full["matrix"]["values"]


def test_recorded_subsets_are_no_restriction_of_the_full_run(recorded):
    """With keep_all the fixture's full run has 2 ideal components; subsets
    have their own (4 over samples 0, 1, 2): a subset's valid nodes are not
    the full run's valid nodes of its samples, and its distances are not the
    full matrix's entries."""
    exp = recorded[0]["expected"]["3-True"]
    full = exp[sc.subset_key(range(4))]
    assert len(full["valid"]) == 8 and len(exp["0-1-2"]["valid"]) == 12
    assert [v for v in full["valid"] if v[0] in (0, 1, 2)] != exp["0-1-2"]["valid"]
    sub = exp["0-1-2"]["matrix"]
    assert sub["labels"] == [0, 1, 2] and full["matrix"]["labels"] == [0, 1, 2, 3]
    assert sub["values"] != [row[:3] for row in full["matrix"]["values"][:3]]
