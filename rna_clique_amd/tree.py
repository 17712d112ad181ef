"""Neighbour-joining trees as the engine returns them (rc_nj,
rc_resample_trees): joins, branch lengths and splits, with Newick output.

The reference's tutorial ends in Biopython's DistanceTreeConstructor().nj and
a Newick file (docs/tutorials/reads2tree/make_tree.py); NJTree.newick() writes
that unrooted tree, the last join as a trifurcation, which is what Biopython's
nj returns before rooting.
"""
from __future__ import annotations

import re
from collections import namedtuple

import numpy as np

# Arrays of a batch of trees: joins (R, N-2, 3) int32, lengths (R, N-2, 3)
# float64, splits (R, N-3, W) uint64, valid (R,) uint8; support (n_ref,) uint32
# or None, n_valid int.
NJResult = namedtuple("NJResult", "joins lengths splits valid support n_valid")

_PLAIN = re.compile(r"^[^\s()\[\]':;,_]+$")


def split_words(n):
    """64-bit words of a split over n positions."""
    return (n + 63) // 64


def _quote(label):
    s = str(label)
    if _PLAIN.match(s):
        return s
    return "'" + s.replace("'", "''") + "'"


class NJTree:
    """One neighbour-joining tree over `labels` (matrix order).

    joins (N-2, 3): children of internal node N + t (leaves are 0..N-1), the
    third -1 except in the last join, which joins the three remaining nodes;
    lengths: the children's branch lengths; splits (N-3, W) uint64: the leaves
    under join t as a bitmask over label positions, on the side without
    position 0; support: None or one value per split (join order)."""

    def __init__(self, labels, joins, lengths, splits, support=None):
        self.labels = list(labels)
        n = len(self.labels)
        if n < 3:
            raise ValueError("a tree needs at least 3 samples")
        self.joins = np.asarray(joins, dtype=np.int32).reshape(n - 2, 3)
        self.lengths = np.asarray(lengths, dtype=np.float64).reshape(n - 2, 3)
        self.splits = np.asarray(splits, dtype=np.uint64).reshape(n - 3, split_words(n))
        self.support = None if support is None else np.asarray(support, dtype=np.float64).reshape(n - 3)

    def split_masks(self):
        """The splits as Python ints (bit b = labels[b])."""
        return [sum(int(x) << (64 * w) for w, x in enumerate(row)) for row in self.splits]

    def splits_as_sets(self):
        """The non-trivial bipartitions as frozensets of labels, each on the
        side without the first label, in join order."""
        n = len(self.labels)
        return [frozenset(self.labels[b] for b in range(n) if m >> b & 1) for m in self.split_masks()]

    def newick(self, support=True):
        """The unrooted tree in Newick format. Lengths are written with repr
        (they read back exactly); an internal node's label is its support as
        an integer percentage when the tree has support values; labels that
        need it are quoted."""
        n = len(self.labels)
        text = {i: _quote(l) for i, l in enumerate(self.labels)}
        for t in range(n - 2):
            kids = [f"{text.pop(int(c))}:{float(l)!r}" for c, l in zip(self.joins[t], self.lengths[t]) if c >= 0]
            label = ""
            if support and self.support is not None and t < n - 3:
                label = str(int(round(100.0 * float(self.support[t]))))
            text[n + t] = "(" + ",".join(kids) + ")" + label
        return text[2 * n - 3] + ";"

    def __repr__(self):
        return f"NJTree({len(self.labels)} leaves{', support' if self.support is not None else ''})"
