"""GPU: the seed index kernels one by one -- the 2-bit pack, the 16-mer fill,
the onesweep radix sort, the fused fill-and-histogram kernel and the bucket
table -- each called through the probe library (oracle/index_probe.hip, built
with the product's own sort.hip and kernels.hip) and compared with the
integer-exact host references of oracle/index_probe.py.

The contract pinned here: the index is the stable sort of
(k-mer << 32 | position) on the bits [bb, 64), plus the bucket table over it.
Every assertion is whole-array equality with the reference (assert_same is
np.array_equal plus a message); there are no tolerances. All sizes derive from
the compiled geometry (T = OS_TILE, S = OS_SEG, P = BF_PER).

Not covered here, and left to the end-to-end parity tests: the engine's own
orchestration (which fill path it picks, tile reuse, the second stream), the
engine's choice of the bucket `bits` (28 at full size: a 1 GiB table does not
belong in a test; 16, 17 and 22 run the same kernel). The sort's key-generator
first pass is not covered either: the engine no longer uses it. The look-back
epoch tag wraps only after 2^31 passes; forcing that is out of scope, and no
test touches the epoch.
"""
import functools

import numpy as np
import pytest

from oracle import index_probe as ip

pytestmark = pytest.mark.gpu

T, S, P = ip.geometry()
BIG = 5 * S * T + T // 2 + 1          # several tiles per look-back chain
U64 = np.uint64
AMBIG = np.frombuffer(b"NnU\x00\xff", dtype=np.uint8)
ACGT = np.frombuffer(b"ACGTacgt", dtype=np.uint8)


@pytest.fixture(scope="module")
def probe():
    with ip.Probe() as p:
        yield p


# ------------------------------------------------------------------------
# sort
# ------------------------------------------------------------------------

SORT_SIZES = [1, 2, 63, 64, 65, S - 1, S, S + 1, T - 1, T, T + 1, S * T - 1, S * T, S * T + 1, BIG]
# the other distributions at the sizes where they differ: within one wave,
# just past one tile, just past one tile per segment, several tiles per chain
DIST_SIZES = [65, T + 1, S * T + 1, BIG]
DISTS = ["equal", "extremes", "skew90", "top_byte", "low_byte", "sorted", "reverse", "flat_digits"]


def make_keys(dist, n, bb, seed):
    """n keys whose sorted field (the bits [bb, 64)) follows `dist`. For
    bb = 32 the low 32 bits are the input index, so a loss of stability shows."""
    rng = np.random.default_rng(seed)
    width = 64 - bb
    full = (1 << width) - 1

    def rand(m):
        return rng.integers(0, full, size=m, dtype=np.uint64, endpoint=True)

    if dist == "uniform":
        v = rand(n)
    elif dist == "equal":            # every sorted bit equal (bb = 32: one k-mer)
        v = np.full(n, 0x5AC3F00D5AC3F00D & full, dtype=U64)
    elif dist == "extremes":         # digits 0 and 255 in every pass
        v = np.where(rng.random(n) < 0.5, U64(0), U64(full)).astype(U64)
    elif dist == "skew90":           # one digit group owns almost every tile of the later passes
        v = np.where(rng.random(n) < 0.9, U64(0x3C3C3C3C3C3C3C3C & full), rand(n)).astype(U64)
    elif dist == "top_byte":         # only the top sorted byte varies
        v = (rng.integers(0, 256, size=n, dtype=np.uint64) << U64(width - 8)) | U64(0x00A5A5A5A5A5A5A5 & (full >> 8))
    elif dist == "low_byte":         # only the lowest sorted byte varies
        v = rng.integers(0, 256, size=n, dtype=np.uint64) | U64(0x7E7E7E7E7E7E7E00 & full)
    elif dist == "sorted":
        v = np.sort(rand(n))
    elif dist == "reverse":
        v = np.sort(rand(n))[::-1].copy()
    elif dist == "flat_digits":      # every digit uniform over 256 values: each tile writes many short runs
        v = np.zeros(n, dtype=U64)
        blocks = (n + 255) // 256
        for p in range(width // 8):
            d = rng.permuted(np.tile(np.arange(256, dtype=np.uint64), (blocks, 1)), axis=1).reshape(-1)[:n]
            v |= d << U64(8 * p)
    else:
        raise ValueError(dist)
    keys = v << U64(bb)
    if bb == 32:
        keys |= np.arange(n, dtype=U64)
    return keys


def check_sort(probe, dist, n, bb, seed):
    keys = make_keys(dist, n, bb, seed)
    got = probe.sort(keys, bb)
    ip.assert_same(got, ip.ref_sort(keys, bb), f"sort {dist} n={n} bb={bb}")


@pytest.mark.parametrize("bb", [32, 0])
@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_uniform(probe, n, bb):
    check_sort(probe, "uniform", n, bb, seed=n)


@pytest.mark.parametrize("bb", [32, 0])
@pytest.mark.parametrize("n", DIST_SIZES)
@pytest.mark.parametrize("dist", DISTS)
def test_sort_distributions(probe, dist, n, bb):
    check_sort(probe, dist, n, bb, seed=n + 1)


def test_sort_empty(probe):
    for bb in (32, 0):
        assert probe.sort(np.zeros(0, dtype=U64), bb).shape == (0,)


def test_sort_state_reuse():
    """One handle, many sorts: sizes up and down, bb alternating, skewed and
    uniform keys alternating. The look-back table is zeroed only when it grows,
    so later sorts meet the stale granules of earlier ones, told apart by the
    epoch tag alone. The epoch advances by one per pass and by nothing else."""
    plan = [("uniform", BIG, 32), ("skew90", 1, 0), ("skew90", T + 1, 0), ("skew90", BIG, 32),
            ("uniform", S - 1, 0), ("extremes", S * T + 1, 32), ("flat_digits", BIG, 0), ("equal", 2, 32),
            ("equal", T, 32), ("uniform", BIG - T, 0), ("skew90", BIG + S * T + 3, 32),   # the table grows here
            ("uniform", BIG, 0), ("top_byte", BIG, 32), ("uniform", 65, 32)]
    with ip.Probe() as p:
        assert p.epoch == 0
        passes = 0
        for i, (dist, n, bb) in enumerate(plan):
            keys = make_keys(dist, n, bb, seed=1000 + i)
            got = p.sort(keys, bb)
            ip.assert_same(got, ip.ref_sort(keys, bb), f"sort #{i} {dist} n={n} bb={bb}")
            passes += (64 - bb) // 8
            assert p.epoch == passes


# ------------------------------------------------------------------------
# index entries
# ------------------------------------------------------------------------

SPECIAL_LENS = [0, 15, 16, 17, 79, 80, 81]   # 0, 0, 1, 2, 64, 65, 66 windows


def make_seq(rng, lens):
    """ACGT in mixed case, by transcript in turn: random; random with a poly-A
    tail; a tandem repeat of period 1 to 3 (many equal k-mers); random."""
    parts = []
    for t, ln in enumerate(lens):
        kind = t % 4
        s = rng.choice(ACGT, size=ln)
        if kind == 1:
            s[ln - ln // 3:] = rng.choice(np.frombuffer(b"Aa", dtype=np.uint8), size=ln // 3)
        elif kind == 2:
            period = 1 + (t // 4) % 3
            unit = rng.choice(ACGT, size=period)
            s = np.tile(unit, ln // period + 1)[:ln]
            s = s ^ (rng.integers(0, 2, size=ln, dtype=np.uint8) << np.uint8(5))   # case only
        parts.append(s.astype(np.uint8))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def layout(lens):
    lens = np.asarray(lens, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]) if lens.shape[0] else np.zeros(0, dtype=np.int64)
    return start, lens, int(lens.sum())


def entry_count(lens):
    return int(np.maximum(np.asarray(lens, dtype=np.int64) - 15, 0).sum())


def index_lens(case, rem, rng):
    """Transcript lengths of an index case; the last transcript is stretched
    so that it ends exactly at a total with total % 32 == rem."""
    if case == "below_64S":          # n < 64 S: the small-n branch of the fused fill's segment arithmetic
        lens = SPECIAL_LENS + [3 * S + 160]
    elif case == "above_64S":        # n a little above 64 S: the one-division shortcut, segments of 64+ entries
        lens = SPECIAL_LENS + [64 * S + 30 - entry_count(SPECIAL_LENS) + 15]
    elif case == "straddle":         # a few tiles; 64-window chunks straddle segment boundaries
        lens = [700, 16] + SPECIAL_LENS + [int(x) for x in rng.integers(200, 3000, size=24)] + [15, 16, 900]
    elif case == "tiles":            # several tiles per segment
        lens = list(SPECIAL_LENS)
        while entry_count(lens) < 5 * S * T - 3000:
            lens.append(int(rng.integers(300, 3000)))
        lens += [16, 0]
        lens.append(BIG - entry_count(lens) + 15)   # n = BIG, plus the stretch
    else:
        raise ValueError(case)
    lens[-1] += (rem - sum(lens)) % 32
    return lens


@functools.lru_cache(maxsize=None)
def index_case(case, rem):
    rng = np.random.default_rng([ord(c) for c in case] + [rem])
    lens = index_lens(case, rem, rng)
    start, lens, total = layout(lens)
    seq = make_seq(rng, lens)
    want = ip.ref_entries(seq, start, lens)
    for a in (seq, start, lens, want):
        a.setflags(write=False)
    return seq, start, lens, want


def straddles(lens, n):
    """Whether some transcript's 64-window chunk lies across a segment boundary."""
    seg = (n + S - 1) // S
    off = 0
    for ln in lens:
        w = max(int(ln) - 15, 0)
        for o0 in range(0, w, 64):
            if (off + o0) // seg != (off + min(o0 + 63, w - 1)) // seg:
                return True
        off += w
    return False


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("rem", [0, 1, 31])
@pytest.mark.parametrize("case", ["below_64S", "above_64S", "straddle", "tiles"])
def test_index_entries(probe, case, rem, path):
    seq, start, lens, want = index_case(case, rem)
    n, total = want.shape[0], seq.shape[0]
    # the inputs are what the case names
    assert total % 32 == rem and start[-1] + lens[-1] == total and n == entry_count(lens)
    if case == "below_64S":
        assert n < 64 * S and (n + S - 1) // S < 64
    elif case == "above_64S":
        assert 64 * S < n <= 64 * S + 96
    elif case == "straddle":
        assert n > 2 * T and straddles(lens, n)
    else:
        assert n >= 5 * S * T and straddles(lens, n)
    got = probe.index(seq, start, lens, path)
    ip.assert_same(got, want, f"index {case} total%32={rem} path={path}")


@pytest.mark.parametrize("path", [0, 1, 2])
def test_index_without_windows(probe, path):
    """No transcript, and transcripts all shorter than the word: an empty index."""
    rng = np.random.default_rng(5)
    assert probe.index(np.zeros(0, dtype=np.uint8), [], [], path).shape == (0,)
    start, lens, total = layout([15, 0, 3])
    assert probe.index(make_seq(rng, lens), start, lens, path).shape == (0,)
    # one transcript of exactly 16 bases: one entry
    start, lens, total = layout([16])
    seq = make_seq(rng, lens)
    ip.assert_same(probe.index(seq, start, lens, path), ip.ref_entries(seq, start, lens, amb=True), "one window")


def amb_case(name):
    """(seq, start, lens) of an ambiguity case."""
    rng = np.random.default_rng([ord(c) for c in name])
    if name == "small":
        lens = SPECIAL_LENS + [40, 200]
    else:
        lens = SPECIAL_LENS + [int(x) for x in rng.integers(200, 2500, size=70)] + [40, 16, 777]
    start, lens, total = layout(lens)
    seq = make_seq(rng, lens)
    if name in ("rate_0.002", "rate_0.05"):
        seq[rng.random(total) < float(name[5:])] = ord("N")
    elif name in ("other_bytes", "small"):
        hit = rng.random(total) < 0.01
        seq[hit] = rng.choice(AMBIG, size=int(hit.sum()))
        long_t = len(SPECIAL_LENS) + 1   # 200 bases or more in both cases
        for j, b in enumerate(AMBIG):   # every byte kind at least once
            seq[start[long_t] + 20 + 31 * j] = b
    elif name == "edges":
        seq[start[8]] = ord("N")                       # first base of a transcript
        seq[start[9] + lens[9] - 1] = ord("N")         # last base of a transcript
        seq[start[10]:start[10] + lens[10]] = ord("N")   # a transcript of N alone: no entry
        seq[start[4]] = ord("N")                       # first base of the 64-window transcript
        seq[start[6] + lens[6] - 1] = ord("n")         # last base of the 66-window transcript
        seq[total - 1] = ord("N")                      # the last base of all
    elif name != "none":
        raise ValueError(name)
    return seq, start, lens


@pytest.mark.parametrize("name", ["rate_0.002", "rate_0.05", "edges", "other_bytes", "small"])
def test_index_entries_ambiguity_path(probe, name):
    seq, start, lens = amb_case(name)
    want = ip.ref_entries(seq, start, lens, amb=True)
    assert 0 < want.shape[0] < entry_count(lens)   # some windows are left out, not all
    got = probe.index(seq, start, lens, 2)
    ip.assert_same(got, want, f"index amb {name}")


def test_index_ambiguity_path_without_ambiguous_bytes(probe):
    seq, start, lens = amb_case("none")
    want = ip.ref_entries(seq, start, lens)
    assert want.shape[0] == entry_count(lens)
    p1 = probe.index(seq, start, lens, 1)
    p2 = probe.index(seq, start, lens, 2)
    ip.assert_same(p2, want, "index amb none, path 2")
    ip.assert_same(p1, want, "index amb none, path 1")
    ip.assert_same(p2, p1, "path 2 against path 1")


# ------------------------------------------------------------------------
# bucket table
# ------------------------------------------------------------------------

BUCKET_NS = [0, 1, P - 1, P, P + 1, 256 * P - 1, 256 * P, 256 * P + 1, 100003]
BUCKET_BITS = [16, 17, 22]


def bucket_entries(kind, n, bits, seed):
    """n sorted entries whose top `bits` bits follow `kind`."""
    rng = np.random.default_rng(seed)
    nb = 1 << bits
    low = rng.integers(0, (1 << (64 - bits)) - 1, size=n, dtype=np.uint64, endpoint=True)
    i = np.arange(n, dtype=np.uint64)
    if kind == "first":
        top = np.zeros(n, dtype=U64)
    elif kind == "last":
        top = np.full(n, nb - 1, dtype=U64)
    elif kind == "one_each":     # entry i in bucket i; more entries than buckets: one or two in every bucket
        top = i if n <= nb else i * U64(nb) // U64(n)
    elif kind == "gaps":         # a few occupied buckets, long empty runs between and around them
        k = max(1, min(n, 7))
        centers = np.sort(rng.integers(1, nb - 1, size=k, dtype=np.uint64))
        top = centers[(i * U64(k) // U64(max(n, 1))).astype(np.int64)]
    else:
        raise ValueError(kind)
    return np.sort((top << U64(64 - bits)) | low)


@pytest.mark.parametrize("bits", BUCKET_BITS)
@pytest.mark.parametrize("n", BUCKET_NS)
@pytest.mark.parametrize("kind", ["first", "last", "one_each", "gaps"])
def test_bucket_table(probe, kind, n, bits):
    ent = bucket_entries(kind, n, bits, seed=n + bits)
    got = probe.bucket(ent, bits)
    ip.assert_same(got, ip.ref_bucket(ent, bits), f"bucket {kind} n={n} bits={bits}")


@pytest.mark.parametrize("bits", BUCKET_BITS)
def test_bucket_table_of_an_index(probe, bits):
    seq, start, lens, want = index_case("straddle", 1)
    ent = probe.index(seq, start, lens, 0)
    ip.assert_same(ent, want, "index")
    ip.assert_same(probe.bucket(ent, bits), ip.ref_bucket(want, bits), f"bucket of an index, bits={bits}")


# ------------------------------------------------------------------------
# pack
# ------------------------------------------------------------------------

@pytest.mark.parametrize("amb_rate", [0.0, 0.05])
@pytest.mark.parametrize("total", [1, 31, 32, 33, 64, 4097])
def test_pack(probe, total, amb_rate):
    rng = np.random.default_rng(total)
    seq = make_seq(rng, [total])
    hit = rng.random(total) < amb_rate
    seq[hit] = rng.choice(AMBIG, size=int(hit.sum()))
    if amb_rate:
        seq[0] = 0xFF
        seq[-1] = ord("N")
    got = probe.pack(seq)
    for g, w, name in zip(got, ip.ref_pack(seq), ("F", "AF", "RC", "ARC")):
        ip.assert_same(g, w, f"pack {name} total={total}")
