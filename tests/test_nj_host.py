"""CPU: the neighbour-joining specification (tests/nj_oracle.py) against the
independent helper tests/treecheck.py and the true trees, its invariants, and
tree.NJTree's Newick output read back by a small parser."""
import numpy as np
import pytest

import nj_cases as nc
import nj_oracle as no
from treecheck import nj_splits, robinson_foulds, tree_splits

SIZES = (4, 5, 16, 33, 65, 129)


def _labels(n):
    return [f"T{i}" for i in range(n)]


@pytest.mark.parametrize("n", SIZES)
def test_oracle_agrees_with_treecheck_and_the_true_tree(n):
    D, parent, leaves = nc.noisy_additive(n, seed=n)
    labels = _labels(n)
    joins, lengths, splits, valid = no.nj(D)
    assert valid == 1
    got = no.split_sets(splits, labels)
    assert got == nj_splits(D, labels)
    truth = tree_splits(parent, leaves, dict(zip(leaves, labels)))
    assert len(truth) == n - 3 and robinson_foulds(got, truth) == 0


def _check_tree(n, joins, lengths, splits):
    """N - 3 distinct non-trivial splits on the side without position 0; the
    joins use every node below 2N - 3 exactly once as a child."""
    masks = no.split_ints(splits)
    assert len(masks) == n - 3 == len(set(masks))
    for m in masks:
        assert not m & 1 and m < 1 << n and 2 <= bin(m).count("1") <= n - 2
    assert joins.shape == (n - 2, 3) and (joins[:-1, 2] == -1).all()
    kids = joins[joins >= 0].tolist()
    assert sorted(kids) == list(range(2 * n - 3))
    for t in range(n - 2):
        assert all(c < n + t for c in joins[t])   # children exist before their parent
    # the split of join t is the leaf set below node n + t
    below = {i: 1 << i for i in range(n)}
    for t in range(n - 2):
        below[n + t] = 0
        for c in joins[t]:
            if c >= 0:
                below[n + t] |= below[int(c)]
    full = (1 << n) - 1
    for t in range(n - 3):
        b = below[n + t]
        assert masks[t] == (b ^ full if b & 1 else b)
    assert below[2 * n - 3] == full
    assert np.isfinite(lengths).all() and (lengths[:-1, 2] == 0.0).all()


@pytest.mark.parametrize("n", (3,) + SIZES)
def test_oracle_invariants_on_tie_heavy_input(n):
    for D in (nc.additive(n, seed=n, integer=True)[0], nc.all_equal(n), nc.additive(n, seed=n + 7)[0]):
        joins, lengths, splits, valid = no.nj(D)
        assert valid == 1
        _check_tree(n, joins, lengths, splits)


def test_additive_lengths_are_the_branch_lengths():
    # a quartet ((0,1),(2,3)) with pendant edges 1, 2, 3, 4 and inner edge 5
    D = np.array([[0, 3, 9, 10], [3, 0, 10, 11], [9, 10, 0, 7], [10, 11, 7, 0]], dtype=np.float64)
    joins, lengths, splits, valid = no.nj(D)
    # after the first join, leaf 3 (the last slot) has moved into slot 1
    assert joins.tolist() == [[0, 1, -1], [4, 3, 2]]
    assert lengths.tolist() == [[1.0, 2.0, 0.0], [5.0, 4.0, 3.0]]
    assert no.split_ints(splits) == [0b1100]


@pytest.mark.parametrize("n", (4, 33, 65))
def test_lower_triangle_and_diagonal_are_ignored(n):
    D = nc.noisy_additive(n, seed=n + 1)[0]
    a, b = no.nj(D), no.nj(nc.with_garbage(D, seed=n))
    assert b[3] == 1
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], no.nj(np.triu(D, 1))[:3]))


def test_non_finite_matrix_is_invalid():
    D = nc.noisy_additive(6, seed=3)[0]
    for bad in (np.nan, np.inf, -np.inf):
        E = D.copy()
        E[1, 4] = bad
        joins, lengths, splits, valid = no.nj(E)
        assert valid == 0 and (joins == -1).all() and np.isnan(lengths).all() and not splits.any()
    with pytest.raises(ValueError):
        no.nj(np.zeros((2, 2)))


def test_non_metric_input_gives_negative_lengths():
    joins, lengths, splits, valid = no.nj(nc.random_symmetric(16, seed=16))
    assert valid == 1 and lengths.min() < 0
    _check_tree(16, joins, lengths, splits)


# ---------------------------------------------------------------------------
# Newick
# ---------------------------------------------------------------------------

def _parse_newick(text):
    """(children, label, length) nested tuples of one Newick tree: quoted
    labels with '' for a quote, lengths after ':'."""
    pos = 0

    def label():
        nonlocal pos
        if pos < len(text) and text[pos] == "'":
            out = []
            pos += 1
            while True:
                if text[pos] == "'":
                    if text[pos + 1:pos + 2] == "'":
                        out.append("'")
                        pos += 2
                        continue
                    pos += 1
                    return "".join(out)
                out.append(text[pos])
                pos += 1
        start = pos
        while pos < len(text) and text[pos] not in "():;,":
            pos += 1
        return text[start:pos]

    def node():
        nonlocal pos
        kids = []
        if text[pos] == "(":
            pos += 1
            while True:
                kids.append(node())
                if text[pos] == ",":
                    pos += 1
                    continue
                assert text[pos] == ")"
                pos += 1
                break
        name = label()
        length = None
        if pos < len(text) and text[pos] == ":":
            pos += 1
            start = pos
            while text[pos] not in "(),;":
                pos += 1
            length = float(text[start:pos])
        return kids, name, length

    root = node()
    assert text[pos:] == ";"
    return root


def _walk(tree, first):
    """{canonical split: (internal label, length)} and {leaf: length}."""
    leaves_of = {}

    def collect(n):
        kids, name, _ = n
        s = frozenset([name]) if not kids else frozenset().union(*(collect(k) for k in kids))
        leaves_of[id(n)] = s
        return s
    everything = collect(tree)
    splits, leaf_len = {}, {}

    def visit(n, is_root):
        kids, name, length = n
        if not kids:
            leaf_len[name] = length
        elif not is_root:
            s = leaves_of[id(n)]
            splits[everything - s if first in s else s] = (name, length)
        for k in kids:
            visit(k, False)
    visit(tree, True)
    return splits, leaf_len, everything


@pytest.mark.parametrize("n,labels", [
    (3, ["a", "b", "c"]),
    (7, ["plain", "two words", "it's", "a_b", "x(1)", "semi;colon", "co:lon,comma"]),
    (33, None),
])
def test_newick_round_trip(n, labels):
    from rna_clique_amd.tree import NJTree
    labels = labels or _labels(n)
    D = nc.noisy(nc.random_symmetric(n, seed=n), seed=n)   # negative and long-fraction lengths
    joins, lengths, splits, _ = no.nj(D)
    support = np.linspace(0.0, 1.0, n - 3) if n > 3 else np.zeros(0)
    tree = NJTree(labels, joins, lengths, splits, support)
    assert set(tree.splits_as_sets()) == no.split_sets(splits, labels) and len(tree.splits_as_sets()) == n - 3
    text = tree.newick()
    root = _parse_newick(text)
    assert len(root[0]) == 3 and root[2] is None   # unrooted: a trifurcation at the last join
    got, leaf_len, everything = _walk(root, labels[0])
    assert everything == frozenset(labels)
    want_sets = tree.splits_as_sets()
    assert set(got) == set(want_sets)
    # every branch length reads back bit for bit, on the branch it belongs to
    for t in range(n - 2):
        for c, length in zip(joins[t], lengths[t]):
            if c < 0:
                continue
            if c < n:
                back = leaf_len[labels[c]]
            else:
                s = want_sets[c - n]
                back = got[s][1]
                assert got[s][0] == str(int(round(100.0 * support[c - n])))
            assert np.float64(back).tobytes() == np.float64(length).tobytes()
    # without support: no internal labels, the same topology
    bare, _, _ = _walk(_parse_newick(tree.newick(support=False)), labels[0])
    assert set(bare) == set(want_sets) and all(v[0] == "" for v in bare.values())
    assert NJTree(labels, joins, lengths, splits).newick() == tree.newick(support=False)


def test_tree_rejects_fewer_than_three_labels():
    from rna_clique_amd.tree import NJTree
    with pytest.raises(ValueError):
        NJTree(["a", "b"], np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 1)))
