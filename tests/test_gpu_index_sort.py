"""The main index's sort (sort.hip os_index_sort: global passes on the top G
k-mer bits, range offsets, the range-local LDS sort with the bucket entries,
the oversized-range fallbacks), called through the probe library
(tests/index_sort_probe.hip, built with the product's own sort.hip and
kernels.hip) and compared with integer-exact numpy references.

The contract pinned here is the one of tests/test_gpu_index_kernels.py: the
entries (k-mer << 32 | position) stably sorted on the bits [32, 64) -- so
positions ascend per k-mer -- and bucket[x] = first entry whose top `bits`
bits are >= x, bucket[2^bits] = n. Every assertion is whole-array equality
(np.array_equal plus a message); there are no tolerances. Sizes derive from the
compiled geometry: T keys per global-pass tile, CAP keys a range-local
workgroup holds, LIST oversized ranges the device list holds.

The references themselves are checked on the CPU (the tests without the gpu
marker). The last tests run the engine end to end with RC_INDEX_CAP.
"""
import numpy as np
import pytest

import index_sort_probe as isp
from oracle import index_probe as ip
from oracle.parity import full_check

gpu = pytest.mark.gpu

T, CAP, LIST, GMAX = isp.geometry()
U64 = np.uint64
# (G, bits): bits - G in {0, 4, 10}; G in {0, 5, 9, 10, 18}: no, one and two
# global passes ((18, 28) is a 1 GiB table and is left to the benchmark
# configurations; G = 0 needs bits > 0)
GB = [(5, 5), (9, 9), (10, 10), (18, 18),
      (0, 4), (5, 9), (9, 13), (10, 14), (18, 22),
      (0, 10), (5, 15), (9, 19), (10, 20)]
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


@pytest.fixture(scope="module")
def probe():
    with isp.Probe() as p:
        yield p


def keys_of(kmers):
    """(k-mer << 32 | input index): a loss of stability shows in the positions."""
    kmers = np.asarray(kmers, dtype=U64)
    return (kmers << U64(32)) | np.arange(kmers.shape[0], dtype=U64)


def uniform(n, seed, G=0, r=None):
    """n random k-mers; with r, all in range r of the top G bits."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    if r is not None:
        k = (k >> U64(G)) | (U64(r) << U64(32 - G)) if G else k
    return k


def check(probe, keys, G, bits, cap=0, what=""):
    ent, bucket, info = probe.sort(keys, G, bits, cap)
    want = isp.ref_entries(keys)
    isp.assert_same(ent, want, f"{what} entries (n={len(keys)}, G={G}, bits={bits}, cap={cap})")
    isp.assert_same(bucket, isp.ref_bucket(want, bits), f"{what} bucket (n={len(keys)}, G={G}, bits={bits}, cap={cap})")
    return info


# ------------------------------------------------------------------------
# the references, on the CPU
# ------------------------------------------------------------------------

def test_reference_entries_are_stable_on_the_kmer():
    keys = np.array([(7 << 32) | 5, (3 << 32) | 9, (7 << 32) | 1, (3 << 32) | 2, (0xFFFFFFFF << 32) | 0], dtype=U64)
    want = np.array([(3 << 32) | 9, (3 << 32) | 2, (7 << 32) | 5, (7 << 32) | 1, (0xFFFFFFFF << 32) | 0], dtype=U64)
    assert np.array_equal(isp.ref_entries(keys), want)
    # positions in input order = ascending positions: the stable sort is the full sort
    k = keys_of(uniform(5000, 1) >> U64(22))
    assert np.array_equal(isp.ref_entries(k), np.sort(k))


def test_reference_bucket_by_definition():
    ent = isp.ref_entries(keys_of(np.array([0, 0, 1 << 28, 5 << 28, 5 << 28, 15 << 28], dtype=U64)))
    b = isp.ref_bucket(ent, 4)
    assert b.tolist() == [0, 2, 3, 3, 3, 3, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 6]
    rng = np.random.default_rng(3)
    ent = isp.ref_entries(keys_of(rng.integers(0, 1 << 32, size=300, dtype=np.uint64)))
    b = isp.ref_bucket(ent, 9)
    top = (ent >> U64(64 - 9)).astype(np.int64)
    for x in range((1 << 9) + 1):
        assert b[x] == int((top < x).sum())
    assert isp.ref_bucket(np.zeros(0, dtype=U64), 5).tolist() == [0] * 33


def test_engine_choice_of_global_bits():
    assert isp.choice(1_600_000_000) == (28, GMAX)      # the C3 tile: two 9-bit passes
    assert isp.choice((CAP // 2) << GMAX) == (28, GMAX)
    assert isp.choice(((CAP // 2 + 1) << GMAX)) == (28, -1)   # larger: the four 8-bit passes stay
    assert isp.choice(3_100_000_000, cap=64) == (28, -1)      # ... whatever RC_INDEX_CAP says
    assert isp.choice(CAP // 2) == (16, 0)              # one range: no global pass
    assert isp.choice(CAP // 2 + 1)[1] == 1
    bits, G = isp.choice(3_000_000)
    assert bits == 22 and (3_000_000 >> G) <= CAP // 2 < (3_000_000 >> (G - 1))
    assert isp.choice(50_000, cap=2) == (16, 15)        # RC_INDEX_CAP: ranges of one key on average
    assert isp.choice(65_536, cap=2) == (16, 16)        # ... but never more global bits than bucket bits


# ------------------------------------------------------------------------
# the sort
# ------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("G,bits", GB)
def test_sizes_and_pass_counts(probe, G, bits):
    for n in SIZES:
        info = check(probe, keys_of(uniform(n, 100 + n)), G, bits)
        if G >= 5 or n <= CAP:
            assert info == dict(ranges=0, keys=0, whole=False)


@gpu
@pytest.mark.parametrize("m", [CAP - 1, CAP, CAP + 1])
def test_one_range_at_the_local_capacity(probe, m):
    G, bits, r = 9, 19, 37
    k = np.concatenate([uniform(m, 5, G, r), uniform(3000, 6)])
    k = k[(k >> U64(32 - G) != r) | (np.arange(k.shape[0]) < m)]   # the rest stays out of range r
    info = check(probe, keys_of(np.random.default_rng(7).permutation(k)), G, bits)
    assert info == (dict(ranges=1, keys=m, whole=False) if m > CAP else dict(ranges=0, keys=0, whole=False))


@gpu
def test_oversized_range_of_one_kmer_keeps_positions_ascending(probe):
    G, bits = 9, 13
    k = np.concatenate([np.full(3 * CAP, 0xA5A5A5A5, dtype=U64), uniform(2 * T, 8)])
    keys = keys_of(np.random.default_rng(9).permutation(k))
    ent, _, _ = probe.sort(keys, G, bits)
    run = ent[(ent >> U64(32)) == U64(0xA5A5A5A5)]
    assert run.shape[0] >= 3 * CAP and np.all(np.diff((run & U64(0xFFFFFFFF)).astype(np.int64)) > 0)
    info = check(probe, keys, G, bits)
    assert info["ranges"] == 1 and info["keys"] >= 3 * CAP and not info["whole"]


@gpu
@pytest.mark.parametrize("G,bits", [(9, 19), (18, 22), (0, 10)])
def test_ninety_percent_in_one_range(probe, G, bits):
    n = 200_000
    rng = np.random.default_rng(11)
    k = np.where(rng.random(n) < 0.9, uniform(n, 12, max(G, 2), 3), uniform(n, 13))
    info = check(probe, keys_of(k), G, bits)
    assert info["ranges"] == 1 and info["keys"] >= int(0.85 * n) and not info["whole"]


@gpu
@pytest.mark.parametrize("G,bits", [(9, 13), (18, 22), (10, 10)])
@pytest.mark.parametrize("where", ["first", "last"])
def test_keys_in_the_first_or_last_range_only(probe, G, bits, where):
    r = 0 if where == "first" else (1 << G) - 1
    check(probe, keys_of(uniform(5000, 14, G, r)), G, bits, what=where)
    # and the extreme k-mers themselves
    check(probe, keys_of(np.full(100, 0 if where == "first" else 0xFFFFFFFF, dtype=U64)), G, bits, what=where)


@gpu
def test_many_empty_ranges(probe):
    check(probe, keys_of(uniform(1000, 15)), 18, 22)
    check(probe, keys_of(uniform(40, 16, 9, 300)), 18, 18)


@gpu
@pytest.mark.parametrize("nbig", [LIST, LIST + 1])
def test_list_of_oversized_ranges_and_its_overflow(probe, nbig):
    """cap = 16: nbig ranges of 17 keys, the others of at most 16. The list
    holds LIST ranges; one more and the whole index takes the 8-bit passes."""
    G, bits, cap = 9, 13, 16
    parts = [uniform(17 if r < nbig else (r % 17), 1000 + r, G, 2 * r + 1) for r in range(200)]
    keys = keys_of(np.random.default_rng(17).permutation(np.concatenate(parts)))
    info = check(probe, keys, G, bits, cap)
    if nbig <= LIST:
        assert info == dict(ranges=nbig, keys=17 * nbig, whole=False)
    else:
        assert info == dict(ranges=nbig, keys=keys.shape[0], whole=True)


@gpu
def test_one_handle_three_sizes():
    """Stale look-back granules of a larger sort, then of either digit width
    (the fallback's 8-bit passes share the status table with the 9-bit ones)."""
    with isp.Probe() as p:
        check(p, keys_of(uniform(3 * T + 17, 18)), 18, 22)
        check(p, keys_of(uniform(100, 19)), 9, 13)
        check(p, keys_of(np.concatenate([uniform(2 * CAP, 20, 5, 9), uniform(T + 1, 21)])), 5, 9)
        check(p, keys_of(uniform(T + 1, 22)), 10, 14)


# ------------------------------------------------------------------------
# through the fill: the counted path and the ambiguity path
# ------------------------------------------------------------------------

def _transcripts(seed, n_tx, amb):
    rng = np.random.default_rng(seed)
    lens = rng.integers(10, 900, size=n_tx)
    lens[:3] = [15, 16, 17]
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(lens.sum()))].copy()
    # a repeat: the same 300 bases in many transcripts, and a poly-A run
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    for t in range(5, n_tx, 7):
        if lens[t] >= 300:
            seq[starts[t]:starts[t] + 300] = seq[starts[4]:starts[4] + 300] if lens[4] >= 300 else ord("A")
    seq[starts[-1]:starts[-1] + lens[-1]] = ord("A")
    if amb:
        seq[rng.integers(0, seq.shape[0], size=seq.shape[0] // 200)] = ord("N")
    return seq, starts, lens


@gpu
@pytest.mark.parametrize("amb", [False, True])
@pytest.mark.parametrize("cap", [0, 64, 5])
def test_index_through_the_fill(probe, amb, cap):
    """build_index_of's sequence: the fill fused with the global passes'
    histograms (no ambiguity codes) or count, scan and plain fill (ambiguity),
    then the sort with the engine's bits and G; cap as RC_INDEX_CAP sets it
    (64: some oversized ranges, 5: more than the list holds)."""
    seq, starts, lens = _transcripts(23, 150, amb)
    ent, bucket, bits, G, info = probe.index(seq, starts, lens, amb, cap)
    want = ip.ref_entries(seq, starts, lens, amb=amb)
    assert (bits, G) == isp.choice(want.shape[0], cap)
    isp.assert_same(ent, want, f"entries (amb={amb}, cap={cap}, G={G})")
    isp.assert_same(bucket, isp.ref_bucket(want, bits), f"bucket (amb={amb}, cap={cap}, G={G})")
    if cap:
        assert info["ranges"] > 0 and info["whole"] == (cap == 5)


# ------------------------------------------------------------------------
# through the engine
# ------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("cap", [None, "4", "600"])
def test_engine_parity_with_index_cap(native, monkeypatch, cap):
    """A small aligned run, bit-exact against the oracle with the default
    capacity, with RC_INDEX_CAP tiny (the whole-index fallback) and with one
    that leaves a few oversized ranges (the ranged fallback)."""
    if cap:
        monkeypatch.setenv("RC_INDEX_CAP", cap)
    from rna_clique_amd.engine import Engine
    from rna_clique_amd.simulate import simulate
    samples, _ = simulate(4, 120, seed=12, p_iso2=0.2, indel_rate=0.003, p_revcomp=0.5, polya=(0.3, 10, 40))
    with Engine(device=0) as eng:
        for s in samples:
            eng.add_sample(s.name, s.seq, s.tx_offsets, s.gene, s.iso)
        eng.run()
        msgs, summary = full_check(eng, samples)
        tm = eng.timings()
    assert not msgs, "\n".join(msgs[:10])
    assert summary["hsps"] > 0 and summary["ideal_nodes"] > 0
    if cap:
        assert tm["index_fb_ranges"] > 0 and tm["index_fb_keys"] > 0
