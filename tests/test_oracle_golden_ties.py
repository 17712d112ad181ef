"""The post-alignment oracle and its vectorised restatement reproduce the
reference's own outputs on tests/golden/post_alignment_ties.json: tie-heavy
groups of up to 16 HSPs, top_matches 1, 3 and 5, several rows and edges per
item, duplicates at the nlargest threshold (cases: tests/post_cases.py,
captured by tests/golden/make_golden.py --only ties). Also: the shared case
generator produces the inputs that the GPU tests rely on."""
import itertools
import json
import os

import pytest

import post_cases as pc
from oracle import post_oracle as po
from test_oracle_golden import FAST_COLS, _fast_rows

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "post_alignment_ties.json")


def load_ties():
    d = json.load(open(GOLDEN))
    assert d["id_format"] == pc.ID_FORMAT
    return pc.TABLE_COLUMNS, pc.HSP_COLUMNS, [tuple(s) for s in d["settings"]], [pc.unpack_fixture(f) for f in d["fixtures"]]


COLS, HC, SETTINGS, FIX = load_ties()
PARAMS = [(fx, top, keep) for fx in FIX for top, keep in SETTINGS]
IDS = [f"{fx['name']}-n{top}-{keep}" for fx, top, keep in PARAMS]


def fixture_hits(fx):
    return fx["hits"]


def oracle_mismatches(fx, top, keep, oracle=po):
    """Messages where `oracle`.run_pipeline differs from the recorded
    reference output (tables with labels, order and every column; edges;
    sample count; valid nodes; sums; matrix). Empty = equal."""
    exp = fx["expected"][f"{top}-{keep}"]
    assert not any(k != "matrix" for k in exp["errors"])
    res = oracle.run_pipeline(fx["samples"], fixture_hits(fx), po.default_parse_id, top, keep)
    msgs = []
    for key, rows in exp["tables"].items():
        t1, t2 = key.split("|")
        got = [[r["label"]] + [r[c] for c in COLS[1:]] for r in res["tables"][(t1, t2)]]
        if got != rows:
            msgs.append(f"table {key}")
    if sorted(sorted([list(u), list(v)]) for u, v in res["edges"]) != exp["edges"]:
        msgs.append("edges")
    if res["sample_count"] != exp["sample_count"]:
        msgs.append("sample_count")
    if sorted([list(x) for x in res["valid"]]) != exp["valid"]:
        msgs.append("valid")
    for key, v in exp["sums"].items():
        if list(res["sums"][tuple(key.split("|"))]) != v:
            msgs.append(f"sums {key}")
    if exp["matrix"] is None:
        try:
            po.distance_matrix(fx["samples"], res["sums"])
            msgs.append("matrix where the reference raises")
        except po.NoIdealComponentsError:
            pass
    else:
        try:
            labels, mat = po.distance_matrix(fx["samples"], res["sums"])
            if labels != exp["matrix"]["labels"] or mat != exp["matrix"]["values"]:
                msgs.append("matrix")
        except po.NoIdealComponentsError:
            msgs.append("no matrix")
    return msgs


def test_fixture_file_is_current_and_small():
    """The file holds exactly the generator's cases (so the GPU tests, which
    rebuild the transcripts from it, and make_golden.py agree) and stays under
    the 1 MiB limit for committed files."""
    assert os.path.getsize(GOLDEN) < 1 << 20
    cases = pc.fixture_cases()
    assert [fx["name"] for fx in FIX] == [c.name for c in cases]
    assert SETTINGS == pc.FIXTURE_SETTINGS
    for fx, c in zip(FIX, cases):
        assert fx["samples"] == c.samples
        assert fixture_hits(fx) == c.hits
        assert fx["transcripts"] == c.transcripts
    # the shapes the issue asks for: 2, 3 and 4 samples, 300-600 HSPs each,
    # one case with groups of at least 12 HSPs
    fam = cases[:3]
    assert [len(c.samples) for c in fam] == [2, 3, 4]
    assert all(300 <= c.n_hsps() <= 600 for c in fam)
    assert max(pc.largest_group(c) for c in fam) >= 12


@pytest.mark.parametrize("fx,top,keep", PARAMS, ids=IDS)
def test_oracle_matches_reference_on_ties(fx, top, keep):
    assert oracle_mismatches(fx, top, keep) == []


@pytest.mark.parametrize("fx,top,keep", PARAMS, ids=IDS)
def test_fast_match_table_matches_reference_on_ties(fx, top, keep):
    from oracle import post_fast as pf
    exp = fx["expected"][f"{top}-{keep}"]
    hits = fixture_hits(fx)
    cmp_cols = ["label"] + [c for c in COLS[1:] if c in FAST_COLS or c == "sstrand"]
    for t1, t2 in itertools.combinations(fx["samples"], 2):
        fwd = pf.rows_from_dicts(hits.get((t2, t1), []), po.default_parse_id)
        rev = pf.rows_from_dicts(hits.get((t1, t2), []), po.default_parse_id)
        got = _fast_rows(pf.match_table(fwd, rev, top, keep))
        want = [dict(zip(COLS, r)) for r in exp["tables"][f"{t1}|{t2}"]]
        assert [[r[c] for c in cmp_cols] for r in got] == [[r[c] for c in cmp_cols] for r in want], (t1, t2)


def test_fixtures_catch_a_strict_threshold(monkeypatch):
    """Sensitivity of the fixtures: an oracle whose nlargest(keep="all")
    threshold uses > instead of >= (dropping the rows that tie with the n-th
    largest) disagrees with the recorded reference output."""
    real = po.highest_bitscores

    def strict(rows, n=1, key=("qgene",), keep="all"):
        out = real(rows, n, key, keep)
        if keep != "all":
            return out
        groups = {}
        for r in rows:
            groups.setdefault(tuple(r[k] for k in key), []).append(r["bitscore"])
        thr = {k: sorted(v, reverse=True)[n - 1] for k, v in groups.items() if len(v) > n}
        return [r for r in out if tuple(r[k] for k in key) not in thr or r["bitscore"] > thr[tuple(r[k] for k in key)]]

    monkeypatch.setattr(po, "highest_bitscores", strict)
    failing = [i for (fx, top, keep), i in zip(PARAMS, IDS) if oracle_mismatches(fx, top, keep)]
    assert failing, "no fixture notices a strict threshold"
    assert any("threshold-duplicates" in i for i in failing)


def test_tie_order_quirk_recorded():
    """Q2: the reference orders tied rows of a group of at most top_matches
    HSPs by numpy's quicksort, which is not stable where numpy uses its SIMD
    sorting networks. The file is recorded with those switched off (ties in
    frame order, the oracle's rule) and names the setting whose tables the
    capturing machine's SIMD sort changes."""
    q = json.load(open(GOLDEN))["reference_quirks"]["Q2_unstable_tie_order"]
    assert q["recorded_with"].startswith("NPY_DISABLE_CPU_FEATURES=")
    assert "family-s0-3x15x2x2 5-True" in q["tables_differ_with_simd_sort"]


def test_small_group_ties_stay_in_frame_order():
    """The smallest input that shows Q2: a group of four rows, two tied
    pairs, top_matches 5. Tied rows stay in frame order (a SIMD quicksort in
    the reference's sort_values branch gives 3, 2, 1, 0 here)."""
    rows = [{"qgene": 10, "bitscore": b, "label": i} for i, b in enumerate([250.5, 250.5, 401.5, 401.5])]
    for n in (4, 5):
        assert [r["label"] for r in po.highest_bitscores(rows, n)] == [2, 3, 0, 1]
    assert [r["label"] for r in po.highest_bitscores(rows, 3)] == [2, 3, 0, 1]   # the partition branch agrees


def test_reference_outputs_have_the_intended_shapes():
    """What the recorded reference tables themselves contain: items with more
    than 2 rows and with 2 edges (keep_all), a placing-path case without
    either, top_matches settings that change the table."""
    def prof(name, key):
        fx = next(f for f in FIX if f["name"] == name)
        tabs = {k: [dict(zip(COLS, r)) for r in rows] for k, rows in fx["expected"][key]["tables"].items()}
        return pc.item_profile(tabs)
    for fx in FIX[:3]:
        assert prof(fx["name"], "3-True")["over_rows"] > 0
        assert prof(fx["name"], "3-False")["max_rows"] == 1
    assert prof("tie-across-genes", "1-True")["over_edges"] >= 3
    p = prof("placing-keep-all", "5-True")
    assert p["over_rows"] == 0 and p["over_edges"] == 0 and p["both"] >= 3
    thr = next(f for f in FIX if f["name"] == "threshold-duplicates")["expected"]
    assert len({json.dumps(thr[k]["tables"]) for k in ("1-True", "3-True", "5-True")}) == 3


# --- the generator itself ---------------------------------------------------

TOPS = (1, 2, 3, 5)


@pytest.mark.parametrize("shape", list(pc.FAMILY_SHAPES))
def test_family_shapes_force_their_paths(shape):
    """Every parametrised shape: with keep_all some item has more than 2 rows
    (the RBH step's full second pass), without it none has more than 2 rows or
    more than 1 edge (the placing kernel), and there is an ideal component at
    every setting. A seed or generator change that loses this fails here."""
    case = pc.family_shape_case(shape)
    assert pc.family_shape_case(shape).hits == case.hits   # deterministic
    for top in TOPS:
        for keep in (True, False):
            res = po.run_pipeline(case.samples, case.hits, po.default_parse_id, top, keep)
            p = pc.item_profile(res["tables"])
            assert res["valid"], (top, keep)
            if keep:
                assert p["over_rows"] > 0
            else:
                assert p["over_rows"] == 0 and p["over_edges"] == 0
    ns, nf, ni, _ = pc.FAMILY_SHAPES[shape]
    assert all(len(t) == (nf + 3) * ni for t in case.transcripts.values())   # silent genes included
    if shape == "large-groups":
        assert pc.largest_group(case) >= 12
    if shape == "spans-blocks":
        assert nf > 256
    if shape == "many-pairs":
        assert ns * (ns - 1) // 2 * nf <= 256


def test_unhit_sample_does_not_count():
    case = pc.family_case(3, 3, 12, 2, 2, p_empty=0.0, unhit_sample=True)
    assert len(case.samples) == 4 and len(case.transcripts[case.samples[3]]) > 0
    res = po.run_pipeline(case.samples, case.hits, po.default_parse_id, 2, True)
    assert res["sample_count"] == 3 and res["valid"]


def test_crafted_cases_force_their_paths():
    tie, place, thr = (pc.CRAFTED[k]() for k in ("tie-across-genes", "placing-keep-all", "threshold-duplicates"))
    for top in TOPS:
        r = po.run_pipeline(tie.samples, tie.hits, po.default_parse_id, top, True)
        assert pc.item_profile(r["tables"])["over_edges"] >= 3
        r = po.run_pipeline(tie.samples, tie.hits, po.default_parse_id, top, False)
        assert pc.item_profile(r["tables"])["max_rows"] == 1
        r = po.run_pipeline(place.samples, place.hits, po.default_parse_id, top, True)
        p = pc.item_profile(r["tables"])
        assert p["over_rows"] == 0 and p["over_edges"] == 0 and p["both"] >= 3
    for top_n in (2, 3, 5):
        assert pc.threshold_groups(thr, top_n) >= 1
    sizes = {len([h for h in rows if po.default_parse_id(h["qseqid"])[1] == g])
             for rows in thr.hits.values() for g in {po.default_parse_id(h["qseqid"])[1] for h in rows}}
    for top_n in (2, 3, 5):
        assert top_n in sizes and top_n + 1 in sizes
    for c in (tie, place, thr):
        assert 30 <= c.n_hsps() <= 400


def test_cases_convert_to_engine_records():
    """Every HSP case converts to HSP_DTYPE arrays (bit scores exact in
    tenths, transcripts found in the explicit lists), search by search."""
    cases = [pc.family_shape_case(s) for s in pc.FAMILY_SHAPES] + pc.fixture_cases() + \
        [pc.family_case(3, 3, 12, 2, 2, p_empty=0.0, unhit_sample=True)]
    for c in cases:
        arrays = c.hsp_arrays()
        assert sum(len(a) for a in arrays.values()) == c.n_hsps()
        for (q, s), a in arrays.items():
            rows = c.hits[(c.samples[q], c.samples[s])]
            assert [int(x) / 10.0 for x in a["bits10"]] == [h["bitscore"] for h in rows]
            assert all(c.transcripts[c.samples[q]][int(t)][0] == po.default_parse_id(h["qseqid"])[1]
                       for t, h in zip(a["q_tx"], rows))


def test_graph_cases_are_honest():
    """Every record case: records build (pair = single-shard pair_order index,
    a != b for edges, one graph record per undirected edge -- asserted by
    GraphCase.records()), node records sit where the issue puts them, the
    orders of one graph agree, and the large sums behave as described."""
    from rna_clique_amd import _native as nat
    cases = pc.graph_cases()
    for c in cases.values():
        arr = c.records()
        assert len(arr) == len(c.recs)
        edge = arr["pair"] != nat.RC_NODE_ONLY
        assert (arr["a"][edge] < arr["b"][edge]).all()
    assert sorted(len(c.recs) for n, c in cases.items() if "-first" in n) == [0, 1, 63, 64, 65, 257]
    for a, b in (("chain-ascending", "chain-permuted"), ("chain-ascending", "chain-descending"),
                 ("star-ascending", "star-permuted"), ("cliques3-pair-major", "cliques3-permuted"),
                 ("cliques4-pair-major", "cliques4-permuted"), ("cliques6-pair-major", "cliques6-permuted")):
        assert cases[a].expected() == dict(cases[b].expected())
        assert sorted(cases[a].recs) == sorted(cases[b].recs) and cases[a].recs != cases[b].recs
    e = cases["chain-ascending"].expected()
    assert (e["components"], e["ideal_components"], e["nodes"]) == (1, 0, 40000)
    for S in (3, 4, 6):
        arr = cases[f"cliques{S}-permuted"].records()
        pairs = (arr["pair"] & 0x7FFFFFFF).reshape(-1)[:len(arr) // 64 * 64].reshape(-1, 64)
        assert ((pairs != pairs[:, :1]).any(1)).mean() > 0.9     # almost every wave mixes pairs
        e = cases[f"cliques{S}-permuted"].expected()
        assert e["ideal_components"] == 25 and e["components"] == 100
        # sums-only records between ideal cliques count in the filtered sums
        plain = pc.cliques_case(S, extras=False).expected()
        assert sum(v[1] for v in e["sums"].values()) > sum(v[1] for v in plain["sums"].values())
    arr = cases["node-only-extra-sample"].records()
    assert all(arr["pair"][i] == nat.RC_NODE_ONLY for i in (0, 64, len(arr) - 1))
    assert cases["node-only-extra-sample"].expected()["ideal_components"] == 0
    assert cases["node-only-extra-sample-count3"].expected()["ideal_components"] == 30
    e = cases["large-sums"].expected()
    assert e["sums"][(0, 1)][0] > 2 ** 32 and e["sums"][(0, 1)] == e["usums"][(0, 1)]
