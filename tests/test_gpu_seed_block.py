"""The seed kernel (seed.hip) at the sizes where its workgroup shape decides a
path: B threads per gene (RC_SEED_BLOCK), word items per round, hits per chunk
(B x RC_HBATCH), seeds per sort chunk and per LDS pass (RC_SEED_CAP).

B is a build constant; the cases are defined by it, so each is built for
B = 128 and B = 256 and holds whichever the library was built with (and for a
round of 256 items at either). Every test builds a few small samples, runs one
engine and compares every HSP of both directed searches, then the tables,
edges and distances, bit for bit with the C oracle (the pattern of
tests/test_gpu_align_cases.py).

A gene's word items are 2 strands x the words at stride word_size - 15 of each
isoform, so their number is even: the item-round cases sit at B - 2, B, B + 2,
2 B and 2 B + 2 items (B - 1, B + 1 and 2 B + 1 do not exist).
"""
import functools
import itertools
import zlib

import numpy as np
import pytest

import align_cases as ac
from oracle.parity import INT_FIELDS, full_check

pytestmark = pytest.mark.gpu

W = 28
S = W - 15          # the query stride
SEED_CAP = 512      # seeds of one LDS pass (RC_SEED_CAP)
HB_MAX = 8          # the largest RC_HBATCH that fits: a chunk holds at most B x HB_MAX hits
BLOCKS = (128, 256)
KNOBS = ("RC_SHARE", "RC_WIN_WORDS", "RC_RESUME", "RC_LATER", "RC_LATER_ROWS", "RC_LATER_CAP")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ------------------------------------------------------------------ helpers


def _rng(*key):
    return np.random.default_rng(zlib.crc32("|".join(str(k) for k in key).encode()))


def items_of(length):
    """Word items of one transcript (engine.hip: the word-item prefix)."""
    return 2 * ((length - 16) // S + 1) if length >= 16 else 0


def length_for(items):
    assert items % 2 == 0 and items > 0
    return 16 + S * (items // 2 - 1)


def substitute(seq, at, k=0):
    """seq with another base at every position of `at` (k picks which)."""
    c = ac.codes(seq).copy()
    at = np.asarray(at, dtype=np.int64)
    c[at] = (c[at] + 1 + k % 3) % 4
    return _ACGT[c].tobytes()


def mutated(rng, seq, rate):
    return substitute(seq, np.flatnonzero(rng.random(len(seq)) < rate), int(rng.integers(0, 3)))


def exact_runs(a, b, least=W):
    """Maximal exact runs of at least `least` bases on the main diagonal."""
    n = min(len(a), len(b))
    eq = np.frombuffer(a[:n], dtype=np.uint8) == np.frombuffer(b[:n], dtype=np.uint8)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], eq.astype(np.int8), [0]))))
    return int(np.sum(edges[1::2] - edges[0::2] >= least))


class Corpus:
    """samples[k] holds genes[g][k]: the isoforms (bytes) of gene g in sample k."""

    def __init__(self, genes, names):
        from rna_clique_amd.simulate import Sample
        self.names = []
        self.samples = []
        n_samples = len(genes[0])
        for k in range(n_samples):
            txs, gid, iso = [], [], []
            for g, per_sample in enumerate(genes):
                for i, t in enumerate(per_sample[k]):
                    txs.append(t)
                    gid.append(g)
                    iso.append(i + 1)
                    if k == 0:
                        self.names.append(f"{names[g]}/iso{i + 1}")
            offs = np.zeros(len(txs) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(t) for t in txs])
            self.samples.append(Sample(f"S{k}", np.frombuffer(b"".join(txs), dtype=np.uint8).copy(), offs,
                                       np.array(gid, dtype=np.int32), np.array(iso, dtype=np.int32),
                                       1.0 + np.arange(len(txs)) / 8.0))

    def case_of(self, t):
        return self.names[t]


def _run(cor, **kw):
    from rna_clique_amd.engine import Engine
    eng = Engine(device=0, **kw)
    for s in cor.samples:
        eng.add_sample(s.name, s.seq, s.tx_offsets, s.gene, s.iso)
    eng.run()
    return eng


def _rows(arr, base_q, base_s):
    """{query transcript: [record]} of one directed search, in output order."""
    out = {}
    for h in arr:
        out.setdefault(int(h["q_tx"]) - base_q, []).append(
            (int(h["s_tx"]) - base_s, *(int(h[f]) for f in INT_FIELDS)))
    return out


def check(eng, cor, **params):
    """Every HSP of every directed search against the oracle, named by case;
    then tables, edges, ideal nodes, sums and distances. Returns the number of
    oracle HSPs."""
    from oracle.align import OracleDB
    db = OracleDB(cor.samples)
    n = 0
    for q, s in itertools.permutations(range(len(cor.samples)), 2):
        ora = db.align(q, s, params.get("word_size", 28), params.get("xdrop_half", 108),
                       params.get("evalue", 1e-99), eng.symmetric, eng.dust)
        n += len(ora)
        want = _rows(ora, db.tx_base[q], db.tx_base[s])
        got = _rows(eng.hsps(q, s), 0, 0)
        for t in sorted(set(want) | set(got)):
            assert got.get(t, []) == want.get(t, []), \
                (f"search {q}->{s}, {cor.case_of(t)}: GPU {got.get(t, [])} vs oracle {want.get(t, [])} "
                 f"(s_tx, {', '.join(INT_FIELDS)})")
    msgs, _ = full_check(eng, cor.samples, check_hsps=False, **params)
    assert not msgs, "\n".join(msgs[:10])
    tm = eng.timings()
    assert tm["defer_length"] == 0 and tm["defer_gaveup"] == 0
    return n


def _setenv(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in KNOBS
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------ 1. item-round seams


@functools.lru_cache(maxsize=None)
def item_seam_corpus(B):
    """One gene per item count around a round of B items, and a gene of three
    isoforms whose items straddle both seams away from an isoform boundary.
    Samples 1 and 2 hold copies 2 % and 4 % diverged."""
    counts = (B - 2, B, B + 2, 2 * B, 2 * B + 2)
    genes, names = [], []
    for n in counts:
        rng = _rng("items", B, n)
        g = ac.rnd(rng, length_for(n))
        genes.append([[g], [mutated(rng, g, 0.02)], [mutated(rng, g, 0.04)]])
        names.append(f"items{n}")
    # isoform boundaries at items B - 100 and B + 20; the seams B and 2 B fall inside isoforms 2 and 3
    rng = _rng("iso3", B)
    isos = [ac.rnd(rng, length_for(n)) for n in (B - 100, 120, B)]
    genes.append([isos, [mutated(rng, t, 0.02) for t in isos], [mutated(rng, t, 0.04) for t in isos]])
    names.append("iso3")
    return Corpus(genes, names), counts


@pytest.mark.parametrize("B", BLOCKS)
def test_item_round_seams(native, monkeypatch, B):
    _setenv(monkeypatch, {})
    cor, counts = item_seam_corpus(B)
    for s in cor.samples:
        lens = np.diff(s.tx_offsets.astype(np.int64))
        assert tuple(items_of(int(x)) for x in lens[:5]) == counts
        iso = [items_of(int(x)) for x in lens[5:]]
        assert iso[0] < B < iso[0] + iso[1] < 2 * B < sum(iso) and iso[0] + iso[1] != B
    with _run(cor) as eng:
        assert check(eng, cor) >= 2 * 3 * len(counts)
        assert eng.timings()["big_passes"] == 0


# ------------------------------------------------------------------ 2, 5. D(p) across a seam; the reverse pass


@functools.lru_cache(maxsize=None)
def lookback_corpus(B):
    """Gene 0 of sample 0: B + 20 words per strand, a poly-A stretch whose DUST
    mask ends just before word B (item B: the first of the second round), so
    that D(p) of word B looks back over masked words of the round before.
    Sample 1's gene 0 shares only the 90 bases around it: the exact run is
    found by word B alone, and only if its D(p) is right (a smaller one calls
    the hit non-canonical and the run is lost). Gene 1: the run whose only
    aligned word of the lower sample is DUST-masked (a reverse-only seed of
    shared searches)."""
    from oracle.align import OracleDB
    n = B + 20
    L = length_for(2 * n)
    p = S * B
    dust = [c for c in ac.seed_cases(W) if c.cls == "seed_dust"]
    assert len(dust) == 1
    for end in range(p - 12, p + 1):   # where the poly-A ends: the mask's own end is DUST's business
        rng = _rng("lookback", B)
        a = bytearray(ac.rnd(rng, L))
        a[p - 50:end] = b"A" * (end - (p - 50))
        a[p - 51:p - 50], a[end:end + 1] = b"C", b"G"
        a = bytes(a)
        b = bytearray(ac.rnd(rng, L))
        b[p - 60:p + 30] = a[p - 60:p + 30]
        b[p - 61:p - 60] = ac.other(rng, a[p - 61:p - 60])
        b[p + 30:p + 31] = ac.other(rng, a[p + 30:p + 31])
        cor = Corpus([[[a], [bytes(b)]], [[dust[0].a], [dust[0].b]]], ["lookback", dust[0].name])
        mask = OracleDB(cor.samples).dust_mask(0)[:L]
        usable = [not mask[S * w:S * w + 16].any() for w in range(n)]
        if usable[B] and not usable[B - 1]:
            return cor, usable
    raise AssertionError("no poly-A placement masks word B - 1 and leaves word B usable")


def _lookback_facts(B):
    cor, usable = lookback_corpus(B)
    assert items_of(int(cor.samples[0].tx_offsets[1])) == 2 * (B + 20)
    # the oracle masks the words before item B: its previous usable word lies
    # at least three words back, in the round before
    back = next(k for k in range(1, B + 1) if usable[B - k])
    assert usable[B] and back >= 3
    # the shared run reaches further left of word B than one stride, less than D(p)
    assert S < 60 < back * S
    return cor


@pytest.mark.parametrize("B", BLOCKS)
def test_dust_lookback_across_seam(native, monkeypatch, B):
    _setenv(monkeypatch, {})
    cor = _lookback_facts(B)
    with _run(cor, evalue=10.0) as eng:
        assert eng.dust is not None
        # (the search 0 -> 1 finds gene 0's run alone: gene 1's only word there is masked)
        assert check(eng, cor, evalue=10.0) >= 3
        assert any(int(h["q_tx"]) == 0 for h in eng.hsps(0, 1)) and eng.timings()["big_passes"] == 0


@pytest.mark.parametrize("share", ["1", "0"])
@pytest.mark.parametrize("B", BLOCKS)
def test_reverse_pass(native, monkeypatch, B, share):
    """The same corpus through the reverse pass (shared searches: the lower
    sample's masked word leaves the run to the reverse search) and with every
    search run on its own."""
    _setenv(monkeypatch, {} if share == "1" else {"RC_SHARE": "0"})
    cor = _lookback_facts(B)
    with _run(cor, evalue=10.0) as eng:
        assert check(eng, cor, evalue=10.0) >= 3
        assert share == "0" or eng.timings()["reverse_seeds"] > 0


# ------------------------------------------------------------------ 3. hit-chunk seams


@functools.lru_cache(maxsize=None)
def hit_chunk_corpus(B):
    """One 950-base gene in enough samples 0.3 % apart that sample 0's one item
    round finds more than B x HB_MAX hits: previous-word hit lists straddle
    the chunks."""
    rng = _rng("chunks", B)
    g = ac.rnd(rng, 950)
    per_copy = items_of(950) // 2
    copies = -(-B * HB_MAX // per_copy) + 3
    genes = [[[g]] + [[mutated(rng, g, 0.003)] for _ in range(copies)]]
    return Corpus(genes, ["gene950"])


@pytest.mark.parametrize("B", BLOCKS)
def test_hit_chunk_seams(native, monkeypatch, B):
    _setenv(monkeypatch, {})
    cor = hit_chunk_corpus(B)
    q = cor.samples[0].seq.tobytes()
    assert items_of(len(q)) <= 256
    hits = sum(q[p:p + 16] == s.seq.tobytes()[p:p + 16] for s in cor.samples[1:] for p in range(0, len(q) - 15, S))
    assert hits > B * HB_MAX
    with _run(cor) as eng:
        assert check(eng, cor) >= len(cor.samples) * (len(cor.samples) - 1)
        assert eng.timings()["big_passes"] == 0


# ------------------------------------------------------------------ 4. sort paths and pass overflow


def _runs_copy(rng, g, runs, k, step=40):
    """A transcript sharing exactly `runs` exact runs (>= W bases) with g: g's
    first runs x step bases with another base at every step-th position (offset
    by k, so that two copies share less than either shares with g), the rest
    random."""
    n = runs * step
    head = substitute(g[:n], np.arange(k % 11, n, step), k)
    tail = ac.rnd(rng, len(g) - n)
    if tail:
        tail = ac.other(rng, g[n:n + 1]) + tail[1:]
    return head + tail


@functools.lru_cache(maxsize=None)
def seed_count_corpus(total, per_sample):
    """Sample 0's gene and subject samples that share `total` seeds with it in
    all, at most `per_sample` each (the first pass of sample 0's gene holds
    them all)."""
    rng = _rng("seeds", total, per_sample)
    g = ac.rnd(rng, per_sample * 40 + 20)
    left, copies = total, []
    while left:
        r = min(left, per_sample)
        copies.append([_runs_copy(rng, g, r, len(copies))])
        left -= r
    return Corpus([[[g]] + copies], [f"seeds{total}"])


def _check_seed_count(cor, total):
    q = cor.samples[0].seq.tobytes()
    assert sum(exact_runs(q, s.seq.tobytes()) for s in cor.samples[1:]) == total


@pytest.mark.parametrize("total", sorted({B + d for B in BLOCKS for d in (-1, 1)} | {2 * B + 1 for B in BLOCKS}))
def test_seed_sort_paths(native, monkeypatch, total):
    """Seeds of one (gene, pass) one short of a sort chunk of B, one past it,
    one past two chunks (a merge round) and one past the LDS pass (B = 256:
    2 B + 1 = RC_SEED_CAP + 1): that pass overflows and runs again over half
    the subject samples; no single sample overflows."""
    _setenv(monkeypatch, {})
    cor = seed_count_corpus(total, 30)
    _check_seed_count(cor, total)
    with _run(cor, dust=False) as eng:
        assert check(eng, cor) >= len(cor.samples) - 1
        assert eng.timings()["big_passes"] == 0


def test_seed_pass_overflow_one_sample(native, monkeypatch):
    """RC_SEED_CAP + 1 seeds against a single subject sample: the pass halves
    its subject range down to that sample, which takes the global-memory pass."""
    _setenv(monkeypatch, {})
    cor = seed_count_corpus(SEED_CAP + 1, SEED_CAP + 1)
    assert len(cor.samples) == 2
    _check_seed_count(cor, SEED_CAP + 1)
    with _run(cor, dust=False) as eng:
        assert check(eng, cor) >= 2
        assert eng.timings()["big_passes"] > 0
