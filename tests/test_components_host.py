"""The per-component restatement (tests/component_oracle.py) against the
reference's own recorded output, the clique cases the GPU tests rely on, and
bootstrap_weights. No GPU."""
import numpy as np
import pytest

import component_oracle as co
import post_cases as pc
from test_oracle_golden_ties import COLS, FIX, SETTINGS

PARAMS = [(fx, top, keep) for fx in FIX for top, keep in SETTINGS]
IDS = [f"{fx['name']}-n{top}-{keep}" for fx, top, keep in PARAMS]


@pytest.mark.parametrize("fx,top,keep", PARAMS, ids=IDS)
def test_helper_on_recorded_reference(fx, top, keep):
    """Over the reference's own tables, edges and nodes of every recorded
    setting: the helper's sums, added over the components, are the recorded
    restricted sums, and its members are the recorded valid nodes."""
    exp = fx["expected"][f"{top}-{keep}"]
    samples = fx["samples"]
    tables = {tuple(k.split("|")): [dict(zip(COLS, r)) for r in rows] for k, rows in exp["tables"].items()}
    nodes, edges = co.index_nodes(samples, [tuple(n) for n in exp["nodes"]],
                                  [(tuple(u), tuple(v)) for u, v in exp["edges"]])
    t = co.ComponentTables(co.records_from_tables(samples, tables), nodes, edges, exp["sample_count"], len(samples))
    ix = {s: i for i, s in enumerate(samples)}
    want = {tuple(sorted((ix[a], ix[b]))): tuple(v) for (a, b), v in
            ((k.split("|"), v) for k, v in exp["sums"].items())}
    assert t.pair_sums() == want
    members = sorted(v for c in t.members for v in c)
    assert members == sorted((ix[s], g) for s, g in exp["valid"])
    assert all(len(c) == exp["sample_count"] for c in t.members)
    assert [c[0] for c in t.members] == sorted(c[0] for c in t.members)
    # all-ones weights give the pair sums; the identity each component's row
    C = t.n_components
    num, den = t.resample(np.ones((1, C), dtype=np.uint16))
    assert {(a, b): (int(num[0, co.pair_index(a, b)]), int(den[0, co.pair_index(a, b)])) for a, b in want} == want
    if C:
        num, den = t.resample(np.eye(C, dtype=np.uint16))
        assert (num == t.num).all() and (den == t.den).all()


@pytest.mark.parametrize("S", [3, 4, 6])
def test_clique_cases_exercise_the_attribution_rule(S):
    """cliques_case(S): 25 ideal components; 25 counted sums-only records
    whose endpoints lie in two different ideal components (only the
    attribution rule places them); every (component, pair) denominator at
    least 29, so a replicate with a non-zero row has no zero denominator."""
    case = pc.cliques_case(S)
    t = co.from_case(case)
    assert t.n_components == 25 and t.sample_count == S
    assert t.crossing == 25
    assert int(t.den.min()) >= 29 and t.den.shape == (25, S * (S - 1) // 2)
    # the crossing records are sums-only ones, and each lands in the component
    # of its higher-sample endpoint
    comp_of = {v: i for i, c in enumerate(t.members) for v in c}
    crossing = [(k, u, v) for k, u, v, _, _ in case.recs
                if k != pc.NODE_ONLY and u in t.valid and v in t.valid and comp_of[u] != comp_of[v]]
    assert len(crossing) == 25 and all(k == pc.SUM_ONLY for k, _, _ in crossing)
    # the same tables whatever the record order, and their sum is the case's own expectation
    assert t.pair_sums() == {k: tuple(v) for k, v in case.expected()["sums"].items()}
    t2 = co.from_case(case.permuted(5))
    assert (t2.num == t.num).all() and (t2.den == t.den).all() and t2.members == t.members


def test_distance_forms_agree_below_2_to_53():
    t = co.from_case(pc.cliques_case(3))
    W = np.random.default_rng(0).integers(1, 9, size=(3, t.n_components))
    a, b = t.distances(W, [2, 0, 1]), t.distances(W, [2, 0, 1], exact=True)
    assert np.array_equal(a, b) and a.shape == (3, 3, 3) and (np.diagonal(a, axis1=1, axis2=2) == 0).all()
    z = t.distances(np.zeros((1, t.n_components), dtype=np.uint16), [0, 1, 2])
    assert np.isnan(z[0][~np.eye(3, dtype=bool)]).all()


def test_bootstrap_weights():
    from rna_clique_amd.similarity import bootstrap_weights
    w = bootstrap_weights(257, 40, seed=3)
    assert w.shape == (40, 257) and w.dtype == np.uint16
    assert (w.sum(axis=1, dtype=np.int64) == 257).all()
    assert np.array_equal(w, bootstrap_weights(257, 40, seed=3))
    assert not np.array_equal(w, bootstrap_weights(257, 40, seed=4))
    assert np.array_equal(w.astype(np.int64),
                          np.random.default_rng(3).multinomial(257, np.full(257, 1 / 257), size=40))
    assert bootstrap_weights(0, 5).shape == (5, 0)
