"""Consensus trees, conflicts and midpoint rooting of rna_clique_amd/tree.py
against tests/consensus_oracle.py, and the oracle against independent facts
(no GPU: the trees are nj_oracle's)."""
import functools
import re

import numpy as np
import pytest

import consensus_oracle as co
import nj_cases as nc
import nj_oracle as no
import treecheck
from rna_clique_amd.tree import (NJTree, SplitCensus, SplitTree, compatible, conflicts, consensus_splits,
                                 consensus_tree, midpoint_newick)

METHODS = ("strict", "majority", "greedy")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _replicates(n, R, rel=0.3):
    """R jittered replicates of one additive tree, nj_oracle's trees of them
    and the oracle's census (computed once, read-only)."""
    D = nc.additive(n, seed=n)[0]
    Ds = np.stack([nc.jitter(D, seed=100 * n + r, rel=rel) for r in range(R)])
    trees = no.nj_batch(Ds)
    masks, counts, ids, nv = co.census(trees[2], trees[3])
    census = SplitCensus(co.census_words(masks, n), counts, ids, nv)
    for a in trees + (census.splits, counts, ids):
        a.setflags(write=False)
    return trees, masks, census


# ---------------------------------------------------------------------------
# a small Newick reader (labels are the leaf positions, or quoted strings)
# ---------------------------------------------------------------------------

_TOKEN = re.compile(r"\s*('(?:[^']|'')*'|[(),:;]|[^\s(),:;']+)")


def parse_newick(text):
    """Nested nodes {"kids": [...], "label": str, "length": float or None}."""
    tokens = _TOKEN.findall(text)
    pos = 0

    def node():
        nonlocal pos
        me = {"kids": [], "label": "", "length": None}
        if tokens[pos] == "(":
            pos += 1
            me["kids"].append(node())
            while tokens[pos] == ",":
                pos += 1
                me["kids"].append(node())
            assert tokens[pos] == ")"
            pos += 1
        if tokens[pos] not in "(),:;":
            t = tokens[pos]
            me["label"] = t[1:-1].replace("''", "'") if t.startswith("'") else t
            pos += 1
        if tokens[pos] == ":":
            me["length"] = float(tokens[pos + 1])
            pos += 2
        return me
    root = node()
    assert tokens[pos] == ";" and pos == len(tokens) - 1
    return root


def leaves_below(node):
    if not node["kids"]:
        return frozenset([node["label"]])
    return frozenset().union(*(leaves_below(k) for k in node["kids"]))


def unrooted_splits(root, labels):
    """The non-trivial bipartitions of a parsed tree, as treecheck writes
    them; and {split: (label, length) of the node below its edge}."""
    out = {}

    def visit(node):
        for k in node["kids"]:
            visit(k)
        if node["kids"] and node is not root:
            s = treecheck._split(leaves_below(node), labels)
            if s is not None:
                out.setdefault(s, []).append((node["label"], node["length"]))
    visit(root)
    return out


def depths(node, above=0.0):
    """{leaf label: summed length from `node`}."""
    if not node["kids"]:
        return {node["label"]: above}
    out = {}
    for k in node["kids"]:
        out.update(depths(k, above + k["length"]))
    return out


def _labels(n):
    return [f"s{b}" for b in range(n)]


def _sets(masks, labels):
    return {frozenset(labels[b] for b in range(len(labels)) if m >> b & 1) for m in masks}


# ---------------------------------------------------------------------------
# the oracle against independent facts
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", (5, 8, 33))
def test_oracle_rf_is_treecheck_rf(n):
    trees, _, _ = _replicates(n, 12)
    labels = _labels(n)
    sets = [no.split_sets(trees[2][r], labels) for r in range(12)]
    pw = co.rf_pairwise(trees[2], trees[3])
    to0 = co.rf_to_ref(trees[2][0], trees[2], trees[3])
    for a in range(12):
        assert to0[a] == treecheck.robinson_foulds(sets[a], sets[0])
        for b in range(12):
            assert pw[a, b] == treecheck.robinson_foulds(sets[a], sets[b])
    assert (pw == pw.T).all() and not pw.diagonal().any() and (n == 5 or pw.max() > 0)


def test_oracle_census_counts_what_support_counts():
    trees, masks, census = _replicates(33, 24)
    counts, nv = no.support_counts(census.splits, trees[2], trees[3])
    assert nv == census.n_valid == 24 and np.array_equal(counts, census.counts)
    assert census.ids[0].tolist() == list(range(30))   # the first tree opens the numbering
    first = [int(np.flatnonzero(census.ids.ravel() == k)[0]) for k in range(len(masks))]
    assert first == sorted(first)


def test_fits_is_compatible():
    rng = np.random.default_rng(5)
    n = 9
    seen = set()
    for _ in range(400):
        a, b = (int(x) & ~1 for x in rng.integers(2, 1 << n, size=2))
        if a and b:
            assert compatible(a, b) == co.fits(a, b, n)
            seen.add(compatible(a, b))
    assert seen == {True, False}


# ---------------------------------------------------------------------------
# consensus
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,R", [(5, 7), (8, 64), (33, 64), (65, 24)])
def test_consensus_splits_follow_the_oracle(n, R):
    _, masks, census = _replicates(n, R)
    got = {}
    for method in METHODS:
        for thr in ((0.5, 0.75) if method == "majority" else (0.5,)):
            idx = consensus_splits(census, method, thr)
            assert idx.tolist() == co.consensus_splits(masks, census.counts, census.n_valid, n, method, thr)
            got[method, thr] = set(idx.tolist())
    assert got["greedy", 0.5] >= got["majority", 0.5] >= got["majority", 0.75] >= got["strict", 0.5]
    major = [masks[k] for k in sorted(got["majority", 0.5])]
    assert all(co.fits(a, b, n) for a in major for b in major)
    if n >= 33:
        assert len(masks) > n - 3 and len(got["majority", 0.5]) < n - 3 < len(masks)
        assert len(got["greedy", 0.5]) > len(got["majority", 0.5])


def test_threshold_range():
    _, _, census = _replicates(8, 64)
    for bad in (0.49, 1.0, -1, 2):
        with pytest.raises(ValueError):
            consensus_splits(census, "majority", bad)
    with pytest.raises(ValueError):
        consensus_splits(census, "median")


@pytest.mark.parametrize("n,R", [(8, 64), (33, 64), (65, 24)])
@pytest.mark.parametrize("method", METHODS)
def test_consensus_tree_follows_the_oracle(n, R, method):
    trees, masks, census = _replicates(n, R)
    labels = _labels(n)
    chosen = co.consensus_splits(masks, census.counts, census.n_valid, n, method)
    tree = consensus_tree(census, labels, trees[1], trees[0], method)
    assert tree.split_masks() == [masks[k] for k in chosen]
    assert tree.support.tolist() == [int(census.counts[k]) / census.n_valid for k in chosen]
    mean, leaf = co.mean_lengths(census.ids, trees[0], trees[1], trees[3], chosen, n)
    assert np.array_equal(_bits(tree.lengths), _bits(mean)) and np.array_equal(_bits(tree.leaf_lengths), _bits(leaf))
    # the Newick text nests every split under its smallest superset
    root = parse_newick(tree.newick())
    got = unrooted_splits(root, labels)
    assert set(got) == _sets(tree.split_masks(), labels) == set(tree.splits_as_sets())
    for s, (m, k) in zip(tree.splits_as_sets(), zip(tree.split_masks(), chosen)):
        (label, length), = got[s]
        assert label == str(int(round(100.0 * int(census.counts[k]) / census.n_valid)))
        assert np.float64(length).view(np.uint64) == _bits(mean)[chosen.index(k)]
    nest = co.nesting(tree.split_masks())

    def check(node, above):
        low = []
        for k in node["kids"]:
            below = leaves_below(k)
            low.append(min(labels.index(x) for x in below))
            if k["kids"]:
                m = sum(1 << labels.index(x) for x in below)
                assert nest[m] == above
                check(k, m)
            else:
                assert k["length"] == leaf[labels.index(k["label"])]
        assert low == sorted(low)
    check(root, None)
    assert root["kids"][0]["label"] == labels[0] and root["label"] == ""
    assert not chosen or re.search(r"\)\d", tree.newick()) is not None
    assert re.search(r"\)\d", tree.newick(support=False)) is None


@pytest.mark.parametrize("n", (4, 8, 33))
def test_consensus_of_copies_is_the_tree(n):
    """R copies of one tree: every method gives that tree, with support 1
    and its own lengths bit for bit."""
    j, le, s, v = no.nj(nc.noisy_additive(n, seed=n)[0])
    R = 5
    trees = tuple(np.stack([a] * R) for a in (j, le, s)) + (np.ones(R, dtype=np.uint8),)
    masks, counts, ids, nv = co.census(trees[2], trees[3])
    assert masks == co.ints(s) and counts.tolist() == [R] * (n - 3) and nv == R
    census = SplitCensus(co.census_words(masks, n), counts, ids, nv)
    one = NJTree(_labels(n), j, le, s)
    for method in METHODS:
        tree = consensus_tree(census, _labels(n), trees[1], trees[0], method)
        assert np.array_equal(tree.splits, s) and tree.support.tolist() == [1.0] * (n - 3)
        # five equal values added one by one, divided once (the sum may round)
        want = np.array([sum([x] * R, 0.0) / R for x in one.split_lengths()])
        assert np.array_equal(_bits(tree.lengths), _bits(want))
    # one copy and two ((x + x) / 2 is exact): its own lengths as bits
    for copies in (1, 2):
        few = SplitCensus(census.splits, np.full(n - 3, copies, dtype=np.uint32), ids[:copies], copies)
        tree = consensus_tree(few, _labels(n), trees[1][:copies], trees[0][:copies])
        assert np.array_equal(_bits(tree.lengths), _bits(one.split_lengths()))
        assert np.array_equal(_bits(tree.leaf_lengths), _bits(one.leaf_lengths()))
        assert tree.support.tolist() == [1.0] * (n - 3)
    got = unrooted_splits(parse_newick(tree.newick()), _labels(n))
    assert set(got) == set(one.splits_as_sets()) == set(unrooted_splits(parse_newick(one.newick()), _labels(n)))


def test_split_and_leaf_lengths_of_an_nj_tree():
    n = 8
    j, le, s, _ = no.nj(nc.noisy_additive(n, seed=3)[0])
    tree = NJTree(_labels(n), j, le, s)
    sl, ll = tree.split_lengths(), tree.leaf_lengths()
    assert sl.shape == (n - 3,) and ll.shape == (n,)
    edges = {c: length for c, _, length in co.nj_edges(j, le)}
    assert sl.tolist() == [edges[n + t] for t in range(n - 3)] and ll.tolist() == [edges[b] for b in range(n)]


def _five_leaf_census():
    """Three topologies over 5 leaves, in 2, 2 and 1 replicates, as splits
    without position 0."""
    A = [0b00110, 0b11000]      # {1,2}, {3,4}
    B = [0b01010, 0b10100]      # {1,3}, {2,4}
    C = [0b11000, 0b11100]      # {3,4}, {2,3,4}
    reps = [A, A, B, B, C]
    splits = np.array([[[m] for m in t] for t in reps], dtype=np.uint64)
    return co.census(splits, np.ones(5, dtype=np.uint8)), splits


def test_hand_built_five_leaves():
    (masks, counts, ids, nv), _ = _five_leaf_census()
    assert masks == [0b00110, 0b11000, 0b01010, 0b10100, 0b11100] and counts.tolist() == [2, 3, 2, 2, 1]
    census = SplitCensus(co.census_words(masks, 5), counts, ids, nv)
    labels = list("abcde")
    # majority: only {d,e} (3 of 5); {b,c} ties with {b,d} and {c,e} at 2 of 5, below the half
    major = consensus_tree(census, labels)
    assert major.split_masks() == [0b11000] and major.support.tolist() == [0.6]
    assert major.newick() == "(a,b,c,(d,e)60);"
    assert consensus_splits(census, "strict").tolist() == []
    assert consensus_tree(census, labels, method="strict").newick() == "(a,b,c,d,e);"
    # greedy: {d,e}, then of the tied 2/5 splits the lowest number that fits, {b,c}
    greedy = consensus_tree(census, labels, method="greedy")
    assert greedy.split_masks() == [0b00110, 0b11000] and greedy.newick() == "(a,(b,c)40,(d,e)60);"
    ids_, freq = conflicts(census, greedy)
    assert ids_.tolist() == [2, 2] and freq.tolist() == [0.4, 0.4]
    want = co.conflicts(masks, counts, nv, 5, greedy.split_masks())
    assert np.array_equal(ids_, want[0]) and np.array_equal(freq, want[1])
    # a tie at exactly half is not a majority: the tree is a star there
    half = SplitCensus(census.splits[:1], np.array([2], dtype=np.uint32), ids[:4, :1], 4)
    assert consensus_tree(half, labels).newick() == "(a,b,c,d,e);"
    assert consensus_tree(half, labels, method="greedy").newick() == "(a,(b,c)50,d,e);"


def test_split_tree_rejects_what_is_no_tree():
    labels = list("abcde")
    for bad in ([[0b00110], [0b01100]], [[0b00111]], [[0b100010]], [[0b00010]], [[0b11110]], [[0b00110], [0b00110]]):
        with pytest.raises(ValueError):
            SplitTree(labels, np.array(bad, dtype=np.uint64))
    t = SplitTree(["a b", "it's", "c", "d", "e", "f"], np.array([[0b000110], [0b001110], [0b110000]], dtype=np.uint64))
    assert t.newick() == "('a b',(('it''s',c),d),(e,f));"
    root = parse_newick(t.newick())
    assert set(unrooted_splits(root, t.labels)) == set(t.splits_as_sets())


@pytest.mark.parametrize("n,R", [(8, 64), (33, 64)])
def test_conflicts_follow_the_oracle(n, R):
    trees, masks, census = _replicates(n, R)
    ref = NJTree(_labels(n), trees[0][0], trees[1][0], trees[2][0])
    for tree in (ref, consensus_tree(census, _labels(n))):
        ids, freq = conflicts(census, tree)
        want = co.conflicts(masks, census.counts, census.n_valid, n, tree.split_masks())
        assert np.array_equal(ids, want[0]) and np.array_equal(freq, want[1])
    ids, _ = conflicts(census, ref)
    assert (ids >= 0).any()
    for k, x in zip(ids, ref.split_masks()):
        assert k < 0 or not compatible(x, masks[k])


# ---------------------------------------------------------------------------
# midpoint rooting
# ---------------------------------------------------------------------------

def _check_midpoint(tree, edges, labels):
    n = len(labels)
    i, j, longest, path, sums, k = co.midpoint(n, edges)
    root = parse_newick(midpoint_newick(tree))
    assert len(root["kids"]) == 2 and root["length"] is None and root["label"] == ""
    sides = [depths(kid, kid["length"]) for kid in root["kids"]]
    assert (labels[i] in sides[0]) != (labels[j] in sides[0])
    length = {frozenset((u, v)): w for u, v, w in edges}
    total = sum(abs(length[frozenset(e)]) for e in zip(path, path[1:]))
    bound = 2 * n * 2.0 ** -52 * total
    for side in sides:
        assert abs(max(side.values()) - 0.5 * longest) <= bound
    for leaf in (labels[i], labels[j]):
        assert abs((sides[0] if leaf in sides[0] else sides[1])[leaf] - 0.5 * longest) <= bound
    # the two halves of the divided edge
    a, b = sums[k - 1], sums[k]
    assert sorted(kid["length"] for kid in root["kids"]) == sorted([0.5 * longest - a, b - 0.5 * longest])
    # unrooted again: the original splits, the divided one once on each side of the root at most
    got = unrooted_splits(root, labels)
    assert set(got) == set(tree.splits_as_sets())
    assert sum(len(v) > 1 for v in got.values()) <= 1 and all(len(v) <= 2 for v in got.values())
    return root, got


@pytest.mark.parametrize("n", (4, 5, 8, 33))
def test_midpoint_of_nj_trees(n):
    j, le, s, _ = no.nj(nc.additive(n, seed=n)[0])
    labels = _labels(n)
    tree = NJTree(labels, j, le, s, support=np.linspace(0.1, 0.9, n - 3))
    root, got = _check_midpoint(tree, co.nj_edges(j, le), labels)
    for split, t in zip(tree.splits_as_sets(), range(n - 3)):
        assert {label for label, _ in got[split]} == {str(int(round(100.0 * tree.support[t])))}
    assert re.search(r"\)\d", midpoint_newick(tree, support=False)) is None


def test_midpoint_of_a_consensus_tree():
    trees, masks, census = _replicates(33, 64)
    labels = _labels(33)
    tree = consensus_tree(census, labels, trees[1], trees[0])
    n, m = 33, len(tree.splits)
    edges = [(b, n + (m if tree._leaf_parent[b] < 0 else int(tree._leaf_parent[b])), float(tree.leaf_lengths[b]))
             for b in range(n)]
    edges += [(n + i, n + (m if tree._parent[i] < 0 else int(tree._parent[i])), float(tree.lengths[i]))
              for i in range(m)]
    _check_midpoint(tree, edges, labels)
    with pytest.raises(ValueError):
        midpoint_newick(consensus_tree(census, labels))   # no lengths


def _hand_tree(lengths):
    """((a:l0,b:l1):l4,c:l2,(d:l3,e:l5):l6) as an NJTree over a..e."""
    l0, l1, l2, l3, l4, l5, l6 = lengths
    joins = [[0, 1, -1], [3, 4, -1], [5, 2, 6]]
    le = [[l0, l1, 0.0], [l3, l5, 0.0], [l4, l2, l6]]
    splits = [[0b11100], [0b11000]]
    return NJTree(list("abcde"), joins, le, np.array(splits, dtype=np.uint64), support=[0.5, 1.0])


def test_midpoint_hand_built():
    # the longest path: a - e = 3 + 1 + 2 + 4 = 10; the root 5 from a, on the edge above (d, e)
    tree = _hand_tree([3.0, 1.0, 1.0, 0.5, 1.0, 4.0, 2.0])
    assert tree.newick() == "((a:3.0,b:1.0)50:1.0,c:1.0,(d:0.5,e:4.0)100:2.0);"
    # the divided edge's label, 100, stands on both of its halves
    assert midpoint_newick(tree) == "(((a:3.0,b:1.0)50:1.0,c:1.0)100:1.0,(d:0.5,e:4.0)100:1.0);"
    root = parse_newick(midpoint_newick(tree))
    assert depths(root)["a"] == depths(root)["e"] == 5.0
    # exactly on a node: a - e = 4 + 1 + 2 + 3 = 10, the half at the inner node above (a, b): no edge is divided
    on = _hand_tree([5.0, 1.0, 1.0, 0.5, 1.0, 2.0, 2.0])
    assert midpoint_newick(on) == "(a:5.0,b:1.0,(c:1.0,(d:0.5,e:2.0)100:2.0)50:1.0);"
    # a negative branch is used as it is: a - e = 3 - 0.5 + 2 + 4 = 8.5, the root 4.25 from a
    neg = _hand_tree([3.0, 1.0, 1.0, 0.5, -0.5, 4.0, 2.0])
    assert midpoint_newick(neg) == "(((a:3.0,b:1.0)50:-0.5,c:1.0)100:1.75,(d:0.5,e:4.0)100:0.25);"
    root = parse_newick(midpoint_newick(neg))
    assert depths(root)["a"] == depths(root)["e"] == 4.25 and len(root["kids"]) == 2
    _check_midpoint(neg, co.nj_edges(neg.joins, neg.lengths), neg.labels)
    # ties: a - e and b - e both 10 -> the lowest i
    tie = _hand_tree([3.0, 3.0, 1.0, 0.5, 1.0, 4.0, 2.0])
    assert co.midpoint(5, co.nj_edges(tie.joins, tie.lengths))[:3] == (0, 4, 10.0)
    _check_midpoint(tie, co.nj_edges(tie.joins, tie.lengths), tie.labels)


def test_midpoint_needs_a_positive_path():
    for lengths in ([0.0] * 7, [-1.0] * 7):
        with pytest.raises(ValueError):
            midpoint_newick(_hand_tree(lengths))
        assert co.midpoint(5, co.nj_edges(_hand_tree(lengths).joins, _hand_tree(lengths).lengths))[5] is None
