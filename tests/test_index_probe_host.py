"""Host side of the index kernel probe (no GPU): the probe library builds for
gfx950 and exports its C ABI, every numpy reference of oracle/index_probe.py
equals a brute-force pure-Python restatement on tiny inputs, and the
comparison the GPU tests use (whole-array equality) reports every kind of
damage a sort or bucket fill could do while leaving the array sorted."""
import ctypes
import os
import random

import numpy as np
import pytest

from oracle import index_probe as ip

MASK64 = (1 << 64) - 1
AMBIG = [ord("N"), ord("n"), ord("U"), 0x00, 0xFF]


# ------------------------------------------------------------------------
# the probe builds here
# ------------------------------------------------------------------------

def test_probe_builds_for_gfx950_and_exports_its_abi():
    path = ip.build_probe()
    assert path == ip.LIB and os.path.exists(path)
    # ctypes binds with RTLD_NOW: an unresolved project symbol fails the load
    L = ctypes.CDLL(path)
    missing = [s for s in ip.SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    with open(path, "rb") as f:
        assert b"gfx950" in f.read()


def test_probe_geometry_is_host_only_and_sane():
    tile, seg, per = ip.geometry()
    assert tile >= 64 and tile % 64 == 0
    assert seg >= 1 and seg & (seg - 1) == 0
    assert per >= 1


def test_probe_compiles_the_product_sources_unchanged():
    """The wrapper units only include the product source and add accessors."""
    for path, src in zip(ip.WRAPPERS, ip.PRODUCT_SOURCES):
        with open(path) as f:
            code = [ln for ln in f.read().splitlines() if ln.strip() and not ln.lstrip().startswith("//")]
        assert code[0] == f'#include "{src}"', path
        assert not any("__global__" in ln or "#define" in ln for ln in code), path


def test_probe_is_not_part_of_the_product():
    from rna_clique_amd import build
    assert "index_probe.hip" not in build.SOURCES
    pkg = os.path.join(ip.ROOT, "rna_clique_amd")
    for name in os.listdir(pkg):
        if name.endswith(".py"):
            with open(os.path.join(pkg, name)) as f:
                assert "index_probe" not in f.read(), name


# ------------------------------------------------------------------------
# brute-force restatements
# ------------------------------------------------------------------------

def _random_seq(rng, n, amb_rate=0.0):
    out = bytearray(rng.choice(b"ACGTacgt") for _ in range(n))
    for i in range(n):
        if rng.random() < amb_rate:
            out[i] = rng.choice(AMBIG)
    return bytes(out)


def _code(c):
    ch = chr(c)
    return "ACGT".index(ch.upper()) if ch in "ACGTacgt" else None


def _brute_entries(seq, tx_start, tx_len, amb):
    ents = []
    for s, ln in zip(tx_start, tx_len):
        for o in range(ln - 15):
            w = seq[s + o:s + o + 16]
            assert len(w) == 16
            codes = [_code(c) for c in w]
            if None in codes:
                assert amb
                continue
            key = sum(c << (2 * i) for i, c in enumerate(codes))
            ents.append((key << 32) | (s + o))
    return sorted(ents)


def _layout(rng, lens):
    """Transcripts of the given lengths back to back, the last ending at total."""
    start, p = [], 0
    for ln in lens:
        start.append(p)
        p += ln
    return start, p


@pytest.mark.parametrize("seed", range(4))
def test_ref_sort_equals_python_sorted(seed):
    rng = random.Random(seed)
    for n in (0, 1, 2, 17, 200):
        # few distinct k-mers, so equal sort keys with different low bits occur
        keys = [(rng.randrange(5) << 56) | (rng.randrange(3) << 32) | rng.randrange(1 << 32) for _ in range(n)]
        a = np.array(keys, dtype=np.uint64)
        for bb in (32, 40, 56):
            want = sorted(keys, key=lambda k: k >> bb)   # sorted() is stable
            assert ip.ref_sort(a, bb).tolist() == want
        assert ip.ref_sort(a, 0).tolist() == sorted(keys)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("amb", [False, True])
def test_ref_entries_equals_window_loop(seed, amb):
    rng = random.Random(100 + seed)
    lens = [0, 15, 16, 17, 40, 0, 33, 16]
    rng.shuffle(lens)
    start, total = _layout(rng, lens)
    seq = bytearray(_random_seq(rng, total, amb_rate=0.06 if amb else 0.0))
    if amb:
        seq[start[lens.index(40)]] = ord("N")                 # first base of a transcript
        seq[start[lens.index(33)] + 32] = 0xFF                # last base of a transcript
    want = _brute_entries(bytes(seq), start, lens, amb)
    got = ip.ref_entries(bytes(seq), start, lens, amb=amb)
    assert got.dtype == np.uint64 and got.tolist() == want
    if not amb:
        # without ambiguous bytes the two modes agree
        assert ip.ref_entries(bytes(seq), start, lens, amb=True).tolist() == want


def test_ref_entries_refuses_ambiguous_bytes_without_amb():
    with pytest.raises(ValueError):
        ip.ref_entries(b"ACGTNACGTACGTACGTACGT", [0], [21])


def test_ref_entries_known_values():
    # poly-A: key 0; poly-T: key 2^32 - 1; base i sits at bits 2i..2i+1
    assert ip.ref_entries(b"A" * 17, [0], [17]).tolist() == [0, 1]
    assert ip.ref_entries(b"t" * 16, [0], [16]).tolist() == [0xFFFFFFFF << 32]
    assert ip.ref_entries(b"C" + b"A" * 14 + b"G", [0], [16]).tolist() == [(1 | (2 << 30)) << 32]
    assert ip.ref_entries(b"A" * 15, [0], [15]).shape == (0,)


@pytest.mark.parametrize("seed", range(3))
def test_ref_bucket_equals_linear_scan(seed):
    rng = random.Random(200 + seed)
    for bits in (1, 4, 6):
        for n in (0, 1, 5, 60):
            ents = sorted(rng.randrange(1 << 64) for _ in range(n))
            if n == 5:
                ents = sorted((1 << 64) - 1 - rng.randrange(3) for _ in range(n))   # all in the last bucket
            want = []
            for x in range((1 << bits) + 1):
                i = 0
                while i < n and (ents[i] >> (64 - bits)) < x:
                    i += 1
                want.append(i)
            got = ip.ref_bucket(np.array(ents, dtype=np.uint64), bits)
            assert got.dtype == np.uint32 and got.tolist() == want
            assert got[0] == 0 and got[-1] == n


def _brute_pack(seq):
    total = len(seq)
    nw = (total + 31) // 32 + 2
    F, AF, RC, ARC = ([0] * nw for _ in range(4))
    for p, c in enumerate(seq):
        code = _code(c)
        F[p // 32] |= (code or 0) << (2 * (p % 32))
        AF[p // 32] |= (3 if code is None else 0) << (2 * (p % 32))
    # the reverse strand, written 5' to 3': base q pairs with forward base total - 1 - q
    for q in range(nw * 32):
        if q < total:
            code = _code(seq[total - 1 - q])
            rc, arc = 3 - (code or 0), (3 if code is None else 0)
        else:
            rc, arc = 3, 0
        RC[q // 32] |= rc << (2 * (q % 32))
        ARC[q // 32] |= arc << (2 * (q % 32))
    return F, AF, RC, ARC


@pytest.mark.parametrize("total", [0, 1, 31, 32, 33, 64, 97])
def test_ref_pack_equals_base_loop(total):
    rng = random.Random(300 + total)
    seq = _random_seq(rng, total, amb_rate=0.1)
    got = ip.ref_pack(seq)
    want = _brute_pack(seq)
    assert ip.pack_words(total) == len(want[0])
    for g, w, name in zip(got, want, ("F", "AF", "RC", "ARC")):
        assert g.dtype == np.uint64 and g.tolist() == w, name


def test_ref_pack_known_values():
    F, AF, RC, ARC = ip.ref_pack(b"ACGTN")
    assert F.tolist() == [0b00_11_10_01_00, 0, 0] and AF.tolist() == [0b11 << 8, 0, 0]
    # reverse complement of ACGTN is NACGT (N pairs with code 3), then all ones
    assert RC[0] == (MASK64 & ~0b11_11_11_11_11) | 0b11_10_01_00_11 and RC[1] == MASK64 and RC[2] == MASK64
    assert ARC.tolist() == [0b11, 0, 0]


# ------------------------------------------------------------------------
# the checker is sensitive
# ------------------------------------------------------------------------

def _expected_index():
    rng = random.Random(7)
    unit = _random_seq(rng, 3)
    seq = (unit * 40)[:100] + _random_seq(rng, 150)   # a tandem repeat: many equal k-mers
    return ip.ref_entries(seq, [0, 100], [100, 150])


def test_assert_same_accepts_equal_arrays():
    want = _expected_index()
    ip.assert_same(want.copy(), want, "index")


def test_assert_same_reports_adjacent_swap_within_one_kmer():
    want = _expected_index()
    kmer = want >> np.uint64(32)
    i = int(np.flatnonzero(kmer[1:] == kmer[:-1])[0])
    got = want.copy()
    got[i], got[i + 1] = want[i + 1], want[i]
    # still sorted by k-mer, same multiset: only whole-array equality sees it
    assert np.all(np.diff((got >> np.uint64(32)).astype(np.int64)) >= 0)
    assert np.array_equal(np.sort(got), np.sort(want))
    assert not np.array_equal(got, want)
    with pytest.raises(AssertionError, match=f"first at {i}"):
        ip.assert_same(got, want, "index")


def test_assert_same_reports_entry_overwritten_by_neighbour():
    want = _expected_index()
    i = want.shape[0] // 2
    got = want.copy()
    got[i] = want[i - 1]
    assert got.shape == want.shape and np.all(got[1:] >= got[:-1])   # same length, still sorted
    assert not np.array_equal(got, want)
    with pytest.raises(AssertionError, match=f"1 of {want.shape[0]} differ, first at {i}"):
        ip.assert_same(got, want, "index")


def test_assert_same_reports_bucket_boundary_off_by_one():
    want = ip.ref_bucket(_expected_index(), 16)
    x = int(np.flatnonzero(np.diff(want.astype(np.int64)) > 0)[0]) + 1   # a boundary with entries before it
    got = want.copy()
    got[x] -= 1
    assert np.all(np.diff(got.astype(np.int64)) >= 0) and got[0] == want[0] and got[-1] == want[-1]
    assert not np.array_equal(got, want)
    with pytest.raises(AssertionError, match=f"first at {x}"):
        ip.assert_same(got, want, "bucket")


def test_assert_same_reports_shape_and_dtype():
    want = _expected_index()
    with pytest.raises(AssertionError, match="shape"):
        ip.assert_same(want[:-1], want, "index")
    with pytest.raises(AssertionError, match="dtype"):
        ip.assert_same(want.astype(np.int64), want, "index")
