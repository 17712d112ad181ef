"""Python handle over one native engine (one GPU).

Thin wrapper: inputs are copied into the engine, all compute runs in
librcgpu.so (hand-written HIP for gfx950), results come back as numpy arrays.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat


class Engine:
    """One engine = one device. Samples are numbered in the order they are
    added (the reference's `inputs` order)."""

    def __init__(self, top_matches=1, keep_all=True, evalue=1e-99, word_size=28,
                 xdrop_half=108, device=0, shard_rank=0, shard_count=1, symmetric=False,
                 dust=None):
        """dust: None = the default (rc_default_opts), False = off, or
        (level, window, linker)."""
        L = nat.lib()
        o = nat.RcOpts()
        L.rc_default_opts(ctypes.byref(o))
        o.top_matches = int(top_matches)
        o.keep_all = 1 if keep_all else 0
        o.evalue = float(evalue)
        o.word_size = int(word_size)
        o.xdrop_half = int(xdrop_half)
        o.device = int(device)
        o.shard_rank = int(shard_rank)
        o.shard_count = int(shard_count)
        o.symmetric = 1 if symmetric else 0
        if dust is False:
            o.dust_level = 0
        elif dust is not None:
            o.dust_level, o.dust_window, o.dust_linker = (int(v) for v in dust)
        self.symmetric = bool(symmetric)
        self.dust = (o.dust_level, o.dust_window, o.dust_linker) if o.dust_level else None
        h = ctypes.c_void_p()
        nat.check(L.rc_create(ctypes.byref(o), ctypes.byref(h)))
        self._h = h
        self.labels = []
        self.n_tx = []
        self.bases = []      # each sample's sequence length (resident or not)
        self.resident = []
        self.shard_count = int(shard_count)

    def close(self):
        if getattr(self, "_h", None):
            nat.lib().rc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------- inputs
    def add_sample(self, label, seq, tx_offsets, gene, iso):
        """seq None: a sample this engine does not align (a sharded run holds
        only the samples of its own pairs) -- its transcripts and genes still
        count for the graph and the e-value statistics."""
        seq = None if seq is None else np.ascontiguousarray(seq, dtype=np.uint8)
        offs = np.ascontiguousarray(tx_offsets, dtype=np.uint64)
        gene = np.ascontiguousarray(gene, dtype=np.int32)
        iso = np.ascontiguousarray(iso, dtype=np.int32)
        n_tx = len(gene)
        if len(offs) != n_tx + 1 or len(iso) != n_tx:
            raise ValueError("tx_offsets must have n_tx + 1 entries, iso n_tx")
        sid = ctypes.c_int32()
        P = ctypes.POINTER
        nat.check(nat.lib().rc_add_sample(
            self._h, str(label).encode(), None if seq is None else seq.ctypes.data_as(ctypes.c_char_p),
            offs.ctypes.data_as(P(ctypes.c_uint64)), gene.ctypes.data_as(P(ctypes.c_int32)),
            iso.ctypes.data_as(P(ctypes.c_int32)), n_tx, ctypes.byref(sid)))
        self.labels.append(str(label))
        self.n_tx.append(n_tx)
        self.bases.append(int(offs[-1]) if n_tx else 0)
        self.resident.append(seq is not None)
        return sid.value

    def add_hsps(self, q, s, hsps):
        arr = np.ascontiguousarray(hsps, dtype=nat.HSP_DTYPE)
        nat.check(nat.lib().rc_add_hsps(self._h, int(q), int(s),
                                        arr.ctypes.data_as(ctypes.c_void_p), len(arr)))

    # ------------------------------------------------------------- phases
    def upload(self):
        nat.check(nat.lib().rc_upload(self._h))

    def run(self):
        nat.check(nat.lib().rc_run(self._h))

    def align(self):
        nat.check(nat.lib().rc_align(self._h))

    def finish(self):
        nat.check(nat.lib().rc_finish(self._h))

    def pair_order(self):
        """The engine's pair numbering [(a, b), ...], a < b: shard by shard,
        subject-major inside a shard (rc_pair_order; one shard: (0,1), (0,2),
        (1,2), (0,3), ...)."""
        n = len(self.labels)
        m = n * (n - 1) // 2
        pa, pb = np.zeros(max(m, 1), dtype=np.int32), np.zeros(max(m, 1), dtype=np.int32)
        nat.check(nat.lib().rc_pair_order(self._h, pa.ctypes.data_as(ctypes.c_void_p),
                                          pb.ctypes.data_as(ctypes.c_void_p)))
        return list(zip(pa[:m].tolist(), pb[:m].tolist()))

    def owned_pairs(self):
        """(a, b) pairs whose tables this shard holds."""
        first, last = self.shard_pairs()
        return self.pair_order()[first:last]

    def shard_pairs(self):
        """[first, last) of this shard's sample pairs in pair_order()."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        nat.check(nat.lib().rc_shard_pairs(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def local_edge_count(self):
        n = ctypes.c_uint64()
        nat.check(nat.lib().rc_export_edges(self._h, None, 0, ctypes.byref(n), 0))
        return n.value

    @staticmethod
    def edge_record_size():
        return int(nat.lib().rc_edge_record_size())

    def export_edges(self, out=None):
        """This shard's graph edges as opaque records: into `out` (a uint8
        tensor: CUDA, written device-to-device, or CPU) or a new host uint8
        array."""
        L = nat.lib()
        n = ctypes.c_uint64()
        nat.check(L.rc_export_edges(self._h, None, 0, ctypes.byref(n), 0))
        rs = self.edge_record_size()
        if out is not None:
            if out.numel() < n.value * rs:
                raise ValueError("edge buffer too small")
            if n.value:
                nat.check(L.rc_export_edges(self._h, ctypes.c_void_p(out.data_ptr()), n.value,
                                            ctypes.byref(n), 1 if out.is_cuda else 0))
            return n.value
        buf = np.zeros(n.value * rs, dtype=np.uint8)
        if n.value:
            nat.check(L.rc_export_edges(self._h, buf.ctypes.data_as(ctypes.c_void_p), n.value,
                                        ctypes.byref(n), 0))
        return buf

    def set_sample_count(self, sample_count):
        """The ideal-component test's sample count (0: from the graph)."""
        nat.check(nat.lib().rc_set_sample_count(self._h, int(sample_count)))

    def import_edges(self, buf, n=None):
        """All shards' edges (host uint8 array, or CUDA tensor + record count)
        -> graph, ideal filter, pair sums."""
        L = nat.lib()
        rs = self.edge_record_size()
        if isinstance(buf, np.ndarray):
            buf = np.ascontiguousarray(buf, dtype=np.uint8)
            if len(buf) % rs:
                raise ValueError("edge buffer size is not a multiple of the record size")
            nat.check(L.rc_import_edges(self._h, buf.ctypes.data_as(ctypes.c_void_p), len(buf) // rs, 0))
        else:
            n = buf.numel() // rs if n is None else int(n)
            nat.check(L.rc_import_edges(self._h, ctypes.c_void_p(buf.data_ptr()), n, 1))

    def import_edge_parts(self, buf, counts, stride):
        """import_edges from blocks: block r starts at record r * stride of
        `buf` (a CUDA uint8 tensor or host uint8 array) and holds counts[r]
        records -- e.g. an all-gather's padded receive buffer as it is."""
        L = nat.lib()
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        if not isinstance(buf, np.ndarray) and not buf.is_cuda:
            buf = buf.numpy()
        if isinstance(buf, np.ndarray):
            buf = np.ascontiguousarray(buf, dtype=np.uint8)
            ptr, dev = buf.ctypes.data_as(ctypes.c_void_p), 0
        else:
            ptr, dev = ctypes.c_void_p(buf.data_ptr()), 1
        nat.check(L.rc_import_edge_parts(self._h, ptr, c.ctypes.data_as(ctypes.c_void_p), len(c), int(stride), dev))

    def trim(self):
        """Free the alignment working set of a finished run (rc_trim): rows,
        HSPs and edges stay; the next align() allocates it again."""
        nat.check(nat.lib().rc_trim(self._h))

    # ------------------------------------------------------------- results
    def _sized(self, fn, dtype, *args):
        n = ctypes.c_uint64()
        nat.check(fn(self._h, *args, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=dtype)
        if n.value:
            nat.check(fn(self._h, *args, out.ctypes.data_as(ctypes.c_void_p), n.value,
                         ctypes.byref(n)))
        return out

    def hsps(self, q, s):
        return self._sized(nat.lib().rc_hsps, nat.HSP_DTYPE, int(q), int(s))

    def pair_rows(self, s1, s2):
        return self._sized(nat.lib().rc_pair_rows, nat.ROW_DTYPE, int(s1), int(s2))

    def edges(self):
        return self._sized(nat.lib().rc_edges, nat.EDGE_DTYPE)

    def ideal_nodes(self):
        L = nat.lib()
        n = ctypes.c_uint64()
        nat.check(L.rc_ideal_nodes(self._h, None, None, 0, ctypes.byref(n)))
        s = np.zeros(n.value, dtype=np.int32)
        g = np.zeros(n.value, dtype=np.int32)
        nat.check(L.rc_ideal_nodes(self._h, s.ctypes.data_as(ctypes.c_void_p),
                                   g.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
        return s, g

    def stats(self):
        st = nat.RcStats()
        nat.check(nat.lib().rc_graph_stats(self._h, ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in nat.RcStats._fields_ if k != "pad"}

    def pair_sums(self, unfiltered=False):
        """(num, den) int64 N x N: sums of nident and of length - gaps over the
        rows of each pair's gene matches table inside ideal components, or
        over all of them (unfiltered=True)."""
        n = len(self.labels)
        num = np.zeros((n, n), dtype=np.int64)
        den = np.zeros((n, n), dtype=np.int64)
        fn = nat.lib().rc_pair_sums_unfiltered if unfiltered else nat.lib().rc_pair_sums
        nat.check(fn(self._h, num.ctypes.data_as(ctypes.c_void_p), den.ctypes.data_as(ctypes.c_void_p)))
        return num, den

    def distance(self, order=None):
        """Distances with rows/columns in `order` (default: every sample in
        sorted label order, similarity_computer.py:220; a subset of the
        samples gives their matrix only). Raises NativeError(RC_E_NO_IDEAL)
        when a pair has no ideal rows."""
        n = len(self.labels)
        if order is None:
            order = sorted(range(n), key=lambda i: self.labels[i])
        order = np.ascontiguousarray(order, dtype=np.int32)
        m = len(order)
        out = np.zeros((m, m), dtype=np.float64)
        nat.check(nat.lib().rc_distance_subset(self._h, order.ctypes.data_as(ctypes.c_void_p), m,
                                               out.ctypes.data_as(ctypes.c_void_p)))
        return [self.labels[i] for i in order], out

    # ------------------------------------------- components and resampling
    def ideal_components(self):
        """(sample, gene) int32 arrays of shape (C, S): the members of every
        ideal component, components in ascending order of their lowest
        (sample id, gene id) node -- not the reference's enumeration order --
        and ascending sample within a component."""
        L = nat.lib()
        c, sc = ctypes.c_uint64(), ctypes.c_int32()
        nat.check(L.rc_ideal_components(self._h, None, None, 0, ctypes.byref(c), ctypes.byref(sc)))
        s = np.zeros((c.value, sc.value), dtype=np.int32)
        g = np.zeros((c.value, sc.value), dtype=np.int32)
        if s.size:
            nat.check(L.rc_ideal_components(self._h, s.ctypes.data_as(ctypes.c_void_p),
                                            g.ctypes.data_as(ctypes.c_void_p), s.size, ctypes.byref(c),
                                            ctypes.byref(sc)))
        return s, g

    def component_sums(self):
        """(num, den) int64 arrays of shape (C, P): each ideal component's
        share of every pair's restricted sums, pairs in pair_order()
        numbering. A table row belongs to the component of its higher
        sample's gene; the sum over the components is pair_sums()."""
        L = nat.lib()
        c, p = ctypes.c_uint64(), ctypes.c_uint64()
        nat.check(L.rc_component_sums(self._h, None, None, 0, ctypes.byref(c), ctypes.byref(p)))
        num = np.zeros((c.value, p.value), dtype=np.int64)
        den = np.zeros((c.value, p.value), dtype=np.int64)
        if num.size:
            nat.check(L.rc_component_sums(self._h, num.ctypes.data_as(ctypes.c_void_p),
                                          den.ctypes.data_as(ctypes.c_void_p), num.size, ctypes.byref(c),
                                          ctypes.byref(p)))
        return num, den

    def n_components(self):
        c, p = ctypes.c_uint64(), ctypes.c_uint64()
        nat.check(nat.lib().rc_component_sums(self._h, None, None, 0, ctypes.byref(c), ctypes.byref(p)))
        return c.value

    # ------------------------------------------------------ component census
    def components(self):
        """One row per connected component of the graph, ideal or not, in
        ascending order of its lowest (sample id, gene id) node: a dict of
        root_sample, root_gene, samples (int32) and nodes, edges (int64)
        arrays of length K (rc_components; census.ComponentTable derives the
        rest)."""
        L = nat.lib()
        k = ctypes.c_uint64()
        nat.check(L.rc_components(self._h, None, None, None, None, None, 0, ctypes.byref(k)))
        out = {"root_sample": np.zeros(k.value, dtype=np.int32), "root_gene": np.zeros(k.value, dtype=np.int32),
               "nodes": np.zeros(k.value, dtype=np.int64), "edges": np.zeros(k.value, dtype=np.int64),
               "samples": np.zeros(k.value, dtype=np.int32)}
        if k.value:
            nat.check(L.rc_components(self._h, *(a.ctypes.data_as(ctypes.c_void_p) for a in out.values()),
                                      k.value, ctypes.byref(k)))
        return out

    def component_members(self):
        """(sample, gene) int32 arrays: every graph node, sorted by
        (component, sample id, gene id). Component c of components() owns
        [off[c], off[c] + nodes[c]), off the exclusive prefix sum of nodes."""
        L = nat.lib()
        n = ctypes.c_uint64()
        nat.check(L.rc_component_members(self._h, None, None, 0, ctypes.byref(n)))
        s = np.zeros(n.value, dtype=np.int32)
        g = np.zeros(n.value, dtype=np.int32)
        if n.value:
            nat.check(L.rc_component_members(self._h, s.ctypes.data_as(ctypes.c_void_p),
                                             g.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
        return s, g

    # ------------------------------------ arguments of the replicate analyses
    @staticmethod
    def _weights(weights):
        """Per-component weights as a contiguous uint16 (R, C) array."""
        w = np.asarray(weights)
        if w.ndim != 2:
            raise ValueError("weights must have shape (replicates, components)")
        if w.dtype != np.uint16:
            if w.dtype.kind not in "iu":
                raise TypeError("weights must be integers")
            if w.size and (w.min() < 0 or w.max() > 65535):
                raise ValueError("weights must lie in 0..65535")
        return np.ascontiguousarray(w, dtype=np.uint16)

    def _order(self, order):
        """Sample ids as an int32 array; default: sorted label order."""
        if order is None:
            order = sorted(range(len(self.labels)), key=lambda i: self.labels[i])
        return np.ascontiguousarray(order, dtype=np.int32)

    @staticmethod
    def _matrices(matrices):
        """Distance matrices (R, N, N) or (N, N) as float64 (R, N, N)."""
        d = np.ascontiguousarray(matrices, dtype=np.float64)
        if d.ndim == 2:
            d = d[None]
        if d.ndim != 3 or d.shape[1] != d.shape[2]:
            raise ValueError("matrices must have shape (replicates, N, N)")
        return d

    def resample(self, weights, order=None, sums=False, *, allow_nan=False):
        """Replicate distance matrices from per-component weights (R, C),
        integers in 0..65535: replicate r's sums are sum_c weights[r, c] *
        component_sums()[c]. Returns (labels, ndarray (R, M, M)) in `order`
        (default: that of distance()), plus (num, den) int64 (R, P) when
        `sums`. Raises NativeError(RC_E_NO_IDEAL) when a replicate has a pair
        without rows, unless allow_nan (its entries are then NaN). A bootstrap over components draws
        each row from a multinomial (similarity.bootstrap_weights); a
        delete-one jackknife or a block deletion is a 0/1 matrix."""
        w, order = self._weights(weights), self._order(order)
        n = len(self.labels)
        m, r = len(order), w.shape[0]
        p = n * (n - 1) // 2
        out = np.zeros((r, m, m), dtype=np.float64)
        num = np.zeros((r, p), dtype=np.int64) if sums else None
        den = np.zeros((r, p), dtype=np.int64) if sums else None
        vp = ctypes.c_void_p
        code = nat.lib().rc_resample(
            self._h, w.ctypes.data_as(vp), r, w.shape[1], order.ctypes.data_as(vp), m, out.ctypes.data_as(vp),
            num.ctypes.data_as(vp) if sums else None, den.ctypes.data_as(vp) if sums else None)
        if not (allow_nan and code == nat.RC_E_NO_IDEAL):
            nat.check(code)
        labels = [self.labels[i] for i in order]
        return (labels, out, (num, den)) if sums else (labels, out)

    # ------------------------------------------------ neighbour-joining trees
    @staticmethod
    def _nj_buffers(r, m, ref_splits):
        from .tree import split_words
        w = split_words(m)
        ref = None
        if ref_splits is not None:
            ref = np.ascontiguousarray(ref_splits, dtype=np.uint64).reshape(-1, w)
        bufs = {"joins": np.zeros((r, max(m - 2, 0), 3), dtype=np.int32),
                "lengths": np.zeros((r, max(m - 2, 0), 3), dtype=np.float64),
                "splits": np.zeros((r, max(m - 3, 0), w), dtype=np.uint64), "valid": np.zeros(r, dtype=np.uint8),
                "support": None if ref is None else np.zeros(len(ref), dtype=np.uint32)}
        return ref, bufs

    @staticmethod
    def _nj_args(ref, bufs, n_valid):
        vp = ctypes.c_void_p
        ptr = lambda a: None if a is None else a.ctypes.data_as(vp)   # noqa: E731
        return (ptr(bufs["joins"]), ptr(bufs["lengths"]), ptr(bufs["splits"]), ptr(bufs["valid"]), ptr(ref),
                0 if ref is None else len(ref), ptr(bufs["support"]), ctypes.byref(n_valid))

    def nj(self, matrices, ref_splits=None, *, allow_nan=False):
        """Neighbour-joining trees of distance matrices (R, N, N) or (N, N),
        of which only the part above the diagonal is read (rc_nj; the engine
        may be in any state). Returns tree.NJResult: joins, lengths, splits
        and valid with a leading replicate axis, and with `ref_splits`
        (n_ref, W) uint64 the number of valid trees that have each of them.
        Raises NativeError(RC_E_NO_IDEAL) when a matrix has a non-finite
        entry, unless allow_nan (that tree is then flagged in `valid`)."""
        from .tree import NJResult
        d = self._matrices(matrices)
        r, m = d.shape[0], d.shape[1]
        ref, bufs = self._nj_buffers(r, m, ref_splits)
        nv = ctypes.c_uint32()
        code = nat.lib().rc_nj(self._h, d.ctypes.data_as(ctypes.c_void_p), r, m, *self._nj_args(ref, bufs, nv))
        if code in (nat.RC_OK, nat.RC_E_NO_IDEAL):
            self._trees = (r, m)   # the trees now on the device (split_census, tree_rf)
        if not (allow_nan and code == nat.RC_E_NO_IDEAL):
            nat.check(code)
        return NJResult(n_valid=nv.value, **bufs)

    def resample_trees(self, weights, order=None, ref_splits=None, *, allow_nan=False):
        """The neighbour-joining tree of every replicate of resample(weights,
        order): the matrices stay on the device (rc_resample_trees). Returns
        (labels, tree.NJResult); split bit b stands for labels[b]. Raises
        NativeError(RC_E_NO_IDEAL) when a replicate has a pair without rows,
        unless allow_nan (that tree is then flagged in `valid`)."""
        from .tree import NJResult
        w, order = self._weights(weights), self._order(order)
        m, r = len(order), w.shape[0]
        ref, bufs = self._nj_buffers(r, m, ref_splits)
        nv = ctypes.c_uint32()
        vp = ctypes.c_void_p
        code = nat.lib().rc_resample_trees(self._h, w.ctypes.data_as(vp), r, w.shape[1], order.ctypes.data_as(vp), m,
                                           *self._nj_args(ref, bufs, nv))
        if code in (nat.RC_OK, nat.RC_E_NO_IDEAL):
            self._trees = (r, m)   # the trees now on the device (split_census, tree_rf)
        if not (allow_nan and code == nat.RC_E_NO_IDEAL):
            nat.check(code)
        return [self.labels[i] for i in order], NJResult(n_valid=nv.value, **bufs)

    # ------------------------------------ split census and tree distances
    def _tree_shape(self):
        """(replicates, samples) of the trees on the device; without any, the
        library's own error (RC_E_STATE)."""
        n = ctypes.c_uint64()
        nat.check(nat.lib().rc_split_census(self._h, None, None, None, 0, ctypes.byref(n), None))
        return self._trees

    def split_census(self):
        """The census of the splits of the last nj() / resample_trees() trees,
        counted on the device (rc_split_census): tree.SplitCensus(splits (K, W)
        uint64, counts (K,) uint32, ids (R, N-3) int32, n_valid). The distinct
        splits are numbered in ascending order of their first occurrence
        (replicate-major, then join order); counts[k] is the number of valid
        trees that have split k; ids[r, t] is the number of split t of tree r,
        -1 in an invalid tree."""
        from .tree import SplitCensus, split_words
        L = nat.lib()
        r, m = self._tree_shape()
        k, nv = ctypes.c_uint64(), ctypes.c_uint32()
        nat.check(L.rc_split_census(self._h, None, None, None, 0, ctypes.byref(k), ctypes.byref(nv)))
        splits = np.zeros((k.value, split_words(m)), dtype=np.uint64)
        counts = np.zeros(k.value, dtype=np.uint32)
        ids = np.zeros((r, m - 3), dtype=np.int32)
        vp = ctypes.c_void_p
        nat.check(L.rc_split_census(self._h, splits.ctypes.data_as(vp), counts.ctypes.data_as(vp),
                                    ids.ctypes.data_as(vp), k.value, ctypes.byref(k), ctypes.byref(nv)))
        return SplitCensus(splits, counts, ids, nv.value)

    def tree_rf(self, ref_splits=None, pairwise=False):
        """Robinson-Foulds distances of the last nj() / resample_trees() trees
        (rc_tree_rf): (to_ref, pairwise). to_ref (R,) uint32: the distance of
        every tree to the tree of the distinct splits `ref_splits` (n_ref, W)
        uint64, None without them; pairwise (R, R) uint32 when asked for, else
        None. Entries of an invalid tree are 0xFFFFFFFF."""
        from .tree import split_words
        r, m = self._tree_shape()
        ref = to_ref = pw = None
        if ref_splits is not None:
            ref = np.ascontiguousarray(ref_splits, dtype=np.uint64).reshape(-1, split_words(m))
            to_ref = np.zeros(r, dtype=np.uint32)
        if pairwise:
            pw = np.zeros((r, r), dtype=np.uint32)
        vp = ctypes.c_void_p
        ptr = lambda a: None if a is None else a.ctypes.data_as(vp)   # noqa: E731
        nat.check(nat.lib().rc_tree_rf(self._h, ptr(ref), 0 if ref is None else len(ref), ptr(to_ref), ptr(pw)))
        return to_ref, pw

    # ------------------------------------------------- principal coordinates
    @staticmethod
    def _pcoa_buffers(r, m, k):
        k = m if k is None else int(k)
        # the library checks the arguments; the buffers only have to exist
        kk = min(max(k, 0), max(m, 0))
        bufs = {"values": np.zeros((r, m), dtype=np.float64), "vectors": np.zeros((r, m, kk), dtype=np.float64),
                "sweeps": np.zeros(r, dtype=np.int32), "valid": np.zeros(r, dtype=np.uint8)}
        return k, bufs, [a.ctypes.data_as(ctypes.c_void_p) for a in bufs.values()]

    def pcoa(self, matrices, k=None, *, max_sweeps=0, allow_nan=False):
        """Principal coordinates of distance matrices (R, N, N) or (N, N), of
        which only the part above the diagonal is read (rc_pcoa; the engine
        may be in any state; N <= 128, else pcoa.pcoa_eigh on the host).
        Returns pcoa.PCoAEigen: values (R, N) descending, the first k (default
        N) unit eigenvectors (R, N, k), sweeps and valid. Raises
        NativeError(RC_E_NO_IDEAL) when a matrix has a non-finite entry, unless
        allow_nan (that replicate is then NaN and flagged in `valid`), and
        NativeError(RC_E_LIMIT) when one has not converged in max_sweeps
        (0 = the default, 30) sweeps."""
        from .pcoa import PCoAEigen
        d = self._matrices(matrices)
        r, m = d.shape[0], d.shape[1]
        k, bufs, ptrs = self._pcoa_buffers(r, m, k)
        code = nat.lib().rc_pcoa(self._h, d.ctypes.data_as(ctypes.c_void_p), r, m, k, int(max_sweeps), *ptrs)
        if not (allow_nan and code == nat.RC_E_NO_IDEAL):
            nat.check(code)
        return PCoAEigen(**bufs)

    def resample_pcoa(self, weights, order=None, k=None, *, max_sweeps=0, allow_nan=False):
        """The principal coordinates of every replicate of resample(weights,
        order): the matrices stay on the device (rc_resample_pcoa). Returns
        (labels, pcoa.PCoAEigen); row i of a replicate's vectors stands for
        labels[i]. Errors as pcoa(); RC_E_NO_IDEAL: a replicate has a pair
        without rows."""
        from .pcoa import PCoAEigen
        w, order = self._weights(weights), self._order(order)
        m, r = len(order), w.shape[0]
        k, bufs, ptrs = self._pcoa_buffers(r, m, k)
        vp = ctypes.c_void_p
        code = nat.lib().rc_resample_pcoa(self._h, w.ctypes.data_as(vp), r, w.shape[1], order.ctypes.data_as(vp), m,
                                          k, int(max_sweeps), *ptrs)
        if not (allow_nan and code == nat.RC_E_NO_IDEAL):
            nat.check(code)
        return [self.labels[i] for i in order], PCoAEigen(**bufs)

    # --------------------------------------------------------- group tests
    @staticmethod
    def _group_args(r, m, labels, perm_labels, method, perm_stats):
        """The label arrays as the library reads them (it checks them), the
        output buffers and the tail of rc_group_test's arguments."""
        from .groups import method_code
        code = method_code(method)
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.ndim != 1 or len(lab) != m:
            raise ValueError("one label per sample")
        perms = np.zeros((0, m), dtype=np.int32) if perm_labels is None else \
            np.ascontiguousarray(perm_labels, dtype=np.int32)
        if perms.size == 0:
            perms = perms.reshape(0, m)
        if perms.ndim != 2 or perms.shape[1] != m:
            raise ValueError("perm_labels must have shape (permutations, N)")
        p = len(perms)
        bufs = {"stat": np.zeros(r, dtype=np.float64), "n_ge": np.zeros(r, dtype=np.uint32),
                "total": np.zeros(r, dtype=np.float64), "within": np.zeros(r, dtype=np.float64),
                "perm_stat": np.zeros((r, p), dtype=np.float64) if perm_stats else None,
                "valid": np.zeros(r, dtype=np.uint8)}
        vp = ctypes.c_void_p
        ptr = lambda a: None if a is None else a.ctypes.data_as(vp)   # noqa: E731
        n_groups = int(lab.max()) + 1 if len(lab) else 0
        tail = (ptr(lab), n_groups, ptr(perms) if p else None, p, code, *(ptr(a) for a in bufs.values()))
        return (lab, perms), n_groups, bufs, tail

    @staticmethod
    def _group_result(method, m, n_groups, perms, bufs):
        from .groups import GroupTestResult
        return GroupTestResult.from_counts(method, m, n_groups, len(perms), bufs["stat"], bufs["n_ge"], bufs["total"],
                                           bufs["within"], bufs["valid"], bufs["perm_stat"])

    def group_test(self, matrices, labels, perm_labels=None, method="permanova", *, perm_stats=False,
                   allow_nan=False):
        """PERMANOVA ("permanova") or ANOSIM ("anosim") of distance matrices
        (R, N, N) or (N, N), of which only the part above the diagonal is read
        (rc_group_test; the engine may be in any state; N <= 128, else
        groups.group_test_host). labels (N,): group numbers 0..a-1
        (groups.encode_grouping), 2 <= a < N; perm_labels (P, N): rearrangements
        of labels (groups.permuted_labels), the same rows for every matrix;
        none: the statistics only. Returns groups.GroupTestResult with one
        entry per matrix, and the permutations' statistics with perm_stats.
        Raises NativeError(RC_E_NO_IDEAL) when a matrix has a non-finite
        entry, unless allow_nan (that replicate is then NaN and flagged in
        `valid`)."""
        d = self._matrices(matrices)
        r, m = d.shape[0], d.shape[1]
        (lab, perms), n_groups, bufs, tail = self._group_args(r, m, labels, perm_labels, method, perm_stats)
        code = nat.lib().rc_group_test(self._h, d.ctypes.data_as(ctypes.c_void_p), r, m, *tail)
        if not (allow_nan and code == nat.RC_E_NO_IDEAL):
            nat.check(code)
        return self._group_result(method, m, n_groups, perms, bufs)

    def resample_group_test(self, weights, labels, perm_labels=None, order=None, method="permanova", *,
                            perm_stats=False, allow_nan=False):
        """The group test of every replicate of resample(weights, order): the
        matrices stay on the device (rc_resample_group_test). labels[i] is the
        group of sample order[i]; an order that names some of the samples tests
        their sub-matrix. Returns (labels of the samples, GroupTestResult).
        Errors as group_test(); RC_E_NO_IDEAL: a replicate has a pair without
        rows."""
        w, order = self._weights(weights), self._order(order)
        m, r = len(order), w.shape[0]
        (lab, perms), n_groups, bufs, tail = self._group_args(r, m, labels, perm_labels, method, perm_stats)
        vp = ctypes.c_void_p
        code = nat.lib().rc_resample_group_test(self._h, w.ctypes.data_as(vp), r, w.shape[1], order.ctypes.data_as(vp),
                                                m, *tail)
        if not (allow_nan and code == nat.RC_E_NO_IDEAL):
            nat.check(code)
        return [self.labels[i] for i in order], self._group_result(method, m, n_groups, perms, bufs)

    # ------------------------------------------------------------ PERMDISP
    @classmethod
    def _dispersion_args(cls, r, m, labels, perm_labels, perm_stats):
        """_group_args for rc_group_dispersion: no method, and the observed
        distances (r, m) before `valid`."""
        (lab, perms), _, bufs, tail = cls._group_args(r, m, labels, perm_labels, "permanova", perm_stats)
        bufs["dist"] = np.zeros((r, m), dtype=np.float64)
        tail = (*tail[:4], *tail[5:10], bufs["dist"].ctypes.data_as(ctypes.c_void_p), tail[10])
        return lab, perms, bufs, tail

    @staticmethod
    def _dispersion_result(lab, perms, bufs):
        from .groups import DispersionResult
        return DispersionResult.from_counts(lab, len(perms), bufs["stat"], bufs["n_ge"], bufs["total"], bufs["within"],
                                            bufs["dist"], bufs["valid"], bufs["perm_stat"])

    def group_dispersion(self, matrices, labels, perm_labels=None, *, perm_stats=False, allow_nan=False):
        """PERMDISP (centroid form) of distance matrices (R, N, N) or (N, N):
        do the groups spread equally about their centroids? (rc_group_dispersion;
        the engine may be in any state; N <= 128, else groups.dispersion_host).
        labels, perm_labels, allow_nan and the errors as group_test(). Returns
        groups.DispersionResult with one entry per matrix."""
        d = self._matrices(matrices)
        r, m = d.shape[0], d.shape[1]
        lab, perms, bufs, tail = self._dispersion_args(r, m, labels, perm_labels, perm_stats)
        code = nat.lib().rc_group_dispersion(self._h, d.ctypes.data_as(ctypes.c_void_p), r, m, *tail)
        if not (allow_nan and code == nat.RC_E_NO_IDEAL):
            nat.check(code)
        return self._dispersion_result(lab, perms, bufs)

    def resample_group_dispersion(self, weights, labels, perm_labels=None, order=None, *, perm_stats=False,
                                  allow_nan=False):
        """PERMDISP of every replicate of resample(weights, order): the
        matrices stay on the device (rc_resample_group_dispersion). Arguments
        as resample_group_test(). Returns (labels of the samples,
        DispersionResult)."""
        w, order = self._weights(weights), self._order(order)
        m, r = len(order), w.shape[0]
        lab, perms, bufs, tail = self._dispersion_args(r, m, labels, perm_labels, perm_stats)
        vp = ctypes.c_void_p
        code = nat.lib().rc_resample_group_dispersion(self._h, w.ctypes.data_as(vp), r, w.shape[1],
                                                      order.ctypes.data_as(vp), m, *tail)
        if not (allow_nan and code == nat.RC_E_NO_IDEAL):
            nat.check(code)
        return [self.labels[i] for i in order], self._dispersion_result(lab, perms, bufs)

    # ------------------------------------------------------- the Mantel test
    @staticmethod
    def _mantel_args(r, m, other, perms, method, perm_stats):
        """Y and the permutations as the library reads them (it checks them),
        the output buffers and the tail of rc_mantel's arguments."""
        from .mantel import method_code
        code = method_code(method)
        y = np.ascontiguousarray(other, dtype=np.float64)
        if y.shape != (m, m):
            raise ValueError("Y must be a square matrix of the samples of X")
        pm = np.zeros((0, m), dtype=np.int32) if perms is None else np.ascontiguousarray(perms, dtype=np.int32)
        if pm.size == 0:
            pm = pm.reshape(0, m)
        if pm.ndim != 2 or pm.shape[1] != m:
            raise ValueError("perms must have shape (permutations, N)")
        p = len(pm)
        bufs = {"stat": np.zeros(r, dtype=np.float64), "n_ge": np.zeros(r, dtype=np.uint32),
                "n_le": np.zeros(r, dtype=np.uint32), "n_abs_ge": np.zeros(r, dtype=np.uint32),
                "perm_stat": np.zeros((r, p), dtype=np.float64) if perm_stats else None,
                "valid": np.zeros(r, dtype=np.uint8)}
        vp = ctypes.c_void_p
        ptr = lambda a: None if a is None else a.ctypes.data_as(vp)   # noqa: E731
        tail = (ptr(y), ptr(pm) if p else None, p, code, *(ptr(a) for a in bufs.values()))
        return (y, pm), bufs, tail

    @staticmethod
    def _mantel_result(method, m, pm, bufs):
        from .mantel import MantelResult
        return MantelResult.from_counts(method, m, len(pm), bufs["stat"], bufs["n_ge"], bufs["n_le"], bufs["n_abs_ge"],
                                        bufs["valid"], bufs["perm_stat"])

    def mantel(self, matrices, other, perms=None, method="pearson", *, perm_stats=False, allow_nan=False):
        """The Mantel test of distance matrices X (R, N, N) or (N, N) against
        one matrix `other` (N, N): the correlation ("pearson" or "spearman")
        of the entries above the diagonal, and how many of the permutations
        perms (P, N; mantel.permutations) of X's rows and columns reach it
        (rc_mantel; the engine may be in any state; 3 <= N <= 128, else
        mantel.mantel_host). Returns mantel.MantelResult with one entry per
        matrix. Raises NativeError(RC_E_NO_IDEAL) when a matrix of X has a
        non-finite entry, unless allow_nan (that replicate is then NaN and
        flagged in `valid`)."""
        d = self._matrices(matrices)
        r, m = d.shape[0], d.shape[1]
        (y, pm), bufs, tail = self._mantel_args(r, m, other, perms, method, perm_stats)
        code = nat.lib().rc_mantel(self._h, d.ctypes.data_as(ctypes.c_void_p), r, m, *tail)
        if not (allow_nan and code == nat.RC_E_NO_IDEAL):
            nat.check(code)
        return self._mantel_result(method, m, pm, bufs)

    def resample_mantel(self, weights, other, perms=None, order=None, method="pearson", *, perm_stats=False,
                        allow_nan=False):
        """The Mantel test of every replicate of resample(weights, order)
        against `other`, whose rows and columns stand for the samples of
        `order`: the replicate matrices stay on the device
        (rc_resample_mantel). Returns (labels of the samples, MantelResult).
        Errors as mantel(); RC_E_NO_IDEAL: a replicate has a pair without
        rows."""
        w, order = self._weights(weights), self._order(order)
        m, r = len(order), w.shape[0]
        (y, pm), bufs, tail = self._mantel_args(r, m, other, perms, method, perm_stats)
        vp = ctypes.c_void_p
        code = nat.lib().rc_resample_mantel(self._h, w.ctypes.data_as(vp), r, w.shape[1], order.ctypes.data_as(vp), m,
                                            *tail)
        if not (allow_nan and code == nat.RC_E_NO_IDEAL):
            nat.check(code)
        return [self.labels[i] for i in order], self._mantel_result(method, m, pm, bufs)

    def dust_mask(self, s):
        """DUST mask of sample s (uint8 per base, 1 = masked query base)."""
        return self._sized(nat.lib().rc_dust_mask, np.uint8, int(s))

    def dust_masks(self, samples, out=None):
        """The DUST masks of resident samples, computed in a pass of their own
        (before align): uint64 words, ceil(bases / 64) per sample in the given
        order (rc_dust_masks). Into `out` (a CUDA uint64/int64 tensor, device
        to device) or a new host array."""
        L = nat.lib()
        ss = np.ascontiguousarray(list(samples), dtype=np.int32)
        sp = ss.ctypes.data_as(ctypes.c_void_p)
        n = ctypes.c_uint64()
        nat.check(L.rc_dust_masks(self._h, sp, len(ss), None, 0, ctypes.byref(n), 0))
        if out is not None:
            if out.numel() < n.value:
                raise ValueError("mask buffer too small")
            nat.check(L.rc_dust_masks(self._h, sp, len(ss), ctypes.c_void_p(out.data_ptr()), n.value,
                                      ctypes.byref(n), 1))
            return n.value
        buf = np.zeros(n.value, dtype=np.uint64)
        nat.check(L.rc_dust_masks(self._h, sp, len(ss), buf.ctypes.data_as(ctypes.c_void_p), n.value,
                                  ctypes.byref(n), 0))
        return buf

    def set_dust_masks(self, samples, bits):
        """Masks for these samples (layout of dust_masks; a host uint64 array
        or a CUDA tensor): align copies them instead of running DUST on them."""
        L = nat.lib()
        ss = np.ascontiguousarray(list(samples), dtype=np.int32)
        sp = ss.ctypes.data_as(ctypes.c_void_p)
        if isinstance(bits, np.ndarray):
            b = np.ascontiguousarray(bits, dtype=np.uint64)
            nat.check(L.rc_set_dust_masks(self._h, sp, len(ss), b.ctypes.data_as(ctypes.c_void_p), len(b), 0))
        else:
            nat.check(L.rc_set_dust_masks(self._h, sp, len(ss), ctypes.c_void_p(bits.data_ptr()), bits.numel(), 1))

    def timings(self):
        t = nat.RcTiming()
        nat.check(nat.lib().rc_timings(self._h, ctypes.byref(t)))
        return {k: getattr(t, k) for k, _ in nat.RcTiming._fields_}
