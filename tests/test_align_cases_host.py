"""The hand-built alignment cases (tests/align_cases.py) on the CPU: the C
oracle against the declared properties and against the second statement of
the extension (tests/extend_trace.py), for every case in every placement. No
GPU: this file says which edge each input lands on, and that the two CPU
implementations agree there, before tests/test_gpu_align_cases.py puts the
same corpora through the kernels.

Per corpus, both directed searches of the C oracle (DUST off, no e-value cut
to speak of) must equal, HSP for HSP and in order, what extend_trace derives
from the sequences alone: seeds from 16-mer hits (exact_runs), containment
and MAX_HSP in seed order, the greedy extension with canonical roles, the
purge (search_pair), the cut from orc_threshold. Eight fields per HSP:
qstart, qend, sstart, send, score_half, mismatch, gaps, gapopen (and the
strand and both transcripts).
"""
import functools

import numpy as np
import pytest

import align_cases as ac
from extend_trace import DMAX, codes, exact_runs, greedy_trace, is_maximal_run, revcomp_codes, search_pair

LOOSE = 10.0        # an e-value that cuts nothing a seed of 16 or more can produce here
FIELDS = ("qstart", "qend", "sstart", "send", "score_half", "mismatch", "gaps", "gapopen")


def _tx(sample, t):
    return sample.seq[int(sample.tx_offsets[t]):int(sample.tx_offsets[t + 1])].tobytes()


def expected_records(q, s, W, X, swap, thr):
    """Records (strand, *FIELDS) of oriented-query/subject transcript pair
    (bytes q, s), plus strand then minus, from extend_trace alone."""
    out = []
    qc, sc = codes(q), codes(s)
    for strand, qo in ((0, qc), (1, revcomp_codes(qc))):
        kept, _ = search_pair(qo, sc, W, X, swap)
        for b in kept:
            if b.score_half >= thr:
                out.append((strand, *b.record(len(q), strand), b.score_half, b.mismatch, b.gaps, b.gapopen))
    return out


def oracle_records(db, hsps, base_q, base_s):
    """{local query transcript: [(local subject transcript, strand, *FIELDS)]} in the oracle's order."""
    out = {}
    for h in hsps:
        out.setdefault(int(h["q_tx"]) - base_q, []).append(
            (int(h["s_tx"]) - base_s, int(h["strand"]), *(int(h[f]) for f in FIELDS)))
    return out


@functools.lru_cache(maxsize=None)
def _oracle(corpus_key, W=28, X=108, evalue=LOOSE):
    from oracle.align import OracleDB
    cor = _corpus(corpus_key)
    db = OracleDB(cor.samples)
    return db, {(q, s): oracle_records(db, db.align(q, s, W, X, evalue, False, None), db.tx_base[q], db.tx_base[s])
                for q, s in ((0, 1), (1, 0))}


def _corpus(key):
    if key == "short":
        return ac.short_corpus()
    if key == "long":
        return ac.long_corpus()
    return ac.seed_corpus(int(key))


def _threshold(cor, q, t, evalue):
    """The cut of directed search q -> 1 - q for query transcript t."""
    from oracle.align import lib
    subj = cor.samples[1 - q]
    qlen = int(cor.samples[q].tx_offsets[t + 1] - cor.samples[q].tx_offsets[t])
    return int(lib().orc_threshold(qlen, int(subj.tx_offsets[-1]), subj.n_tx, evalue))


def check_transcripts(key, ts, W=28, X=108, evalue=LOOSE):
    """Oracle == extend_trace for transcripts ts of corpus `key`, both directed
    searches; no HSP joins two cases. Returns the number of HSPs compared."""
    cor = _corpus(key)
    _, ora = _oracle(key, W, X, evalue)
    n = 0
    for q in (0, 1):
        for t in ts:
            got = ora[(q, 1 - q)].get(t, [])
            assert all(g[0] == t for g in got), f"{cor.case_of(t)}: an HSP joins it to {sorted({cor.case_of(g[0]) for g in got})[:5]}"
            want = expected_records(_tx(cor.samples[q], t), _tx(cor.samples[1 - q], t), W, X, q == 1,
                                    _threshold(cor, q, t, evalue))
            assert [g[1:] for g in got] == want, f"{cor.case_of(t)}, search {q}->{1 - q}: oracle vs extend_trace"
            n += len(want)
    return n


def _entries(key, cls):
    cor = _corpus(key)
    return [t for t, (c, p) in enumerate(cor.entries) if c.cls == cls]


def _prop(box, path):
    if path == "box":
        return (box.qa, box.qb, box.sa, box.sb)
    obj, attr = path.split(".")
    return getattr(getattr(box, obj), attr)


def check_declared(key, cls, W=28):
    """What each case of the class declares, on the placement "asis" (search
    0 -> 1, plus strand): the seed is a maximal exact run and the first in seed
    order; the HSP count before any cut; the trace's properties."""
    cor = _corpus(key)
    _, ora = _oracle(key, W)
    seen = 0
    for t, (c, p) in enumerate(cor.entries):
        if c.cls != cls:
            continue
        if c.single:   # one HSP in every placement and in both searches
            for q in (0, 1):
                assert len(ora[(q, 1 - q)].get(t, [])) == 1, cor.case_of(t)
        if p != "asis":
            continue
        seen += 1
        a, b = codes(c.a), codes(c.b)
        runs = exact_runs(a, b, W)
        if c.seed is not None:
            assert is_maximal_run(a, b, c.seed) and c.seed in runs, c.name
        kept, boxes = search_pair(a, b, W)
        if c.hsps is not None:
            assert len(kept) == c.hsps, (c.name, len(kept))
            assert len([g for g in ora[(0, 1)].get(t, []) if g[1] == 0]) == c.hsps, c.name
        if c.props:
            assert c.seed is not None and runs[0] == c.seed, c.name
            for path, want in c.props.items():
                got = _prop(boxes[0], path)
                if isinstance(want, tuple) and want[0] in ("ge", "le"):
                    assert (got >= want[1]) if want[0] == "ge" else (got <= want[1]), (c.name, path, got)
                else:
                    assert got == want, (c.name, path, got, want)
    assert seen
    return seen


# ------------------------------------------------------------------ the short corpus

SHORT_CLASSES = ("band", "gap", "span", "repeat", "xdrop", "ends", "residue", "early_stop", "seed_run", "seed_N",
                 "seed_end", "seed_dust", "seed_pair", "seed_box", "max_hsp", "evalue")


def test_every_class_is_in_the_short_corpus():
    cor = ac.short_corpus()
    assert {c.cls for c, _ in cor.entries} == set(SHORT_CLASSES)
    assert {p for _, p in cor.entries} == set(ac.PLACEMENTS)
    assert max(len(_tx(s, t)) for s in cor.samples for t in range(s.n_tx)) < 1500
    names = [c.name for c, p in cor.entries if p == "asis"]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("cls", SHORT_CLASSES)
def test_short_case_class(cls):
    """The class's cases: declared properties on the placement as built, and
    oracle == extend_trace in all four placements and both directed searches."""
    ts = _entries("short", cls)
    n = check_transcripts("short", ts)
    if cls == "evalue":
        return   # declared against the default cut: test_evalue_cut_each_direction
    check_declared("short", cls)
    assert n > 0


def test_no_hsp_joins_two_cases():
    for key in ("short", "long", "16", "64"):
        _, ora = _oracle(key)
        for recs in ora.values():
            for t, got in recs.items():
                assert all(g[0] == t for g in got), _corpus(key).case_of(t)


def test_band_edges_differ():
    """+31 is the band's last diagonal and -32 its first: four insertions of 8
    are stopped (the next diagonal would be +32) where four deletions of 8 go
    through, and the straddling pairs fall on opposite sides."""
    by = {c.name: c for c, p in ac.short_corpus().entries if p == "asis"}

    def first(name):
        c = by[name]
        kept, boxes = search_pair(codes(c.a), codes(c.b))
        return len(boxes), boxes[0].right

    for inside, outside, edge in (("band_ins_8887", "band_ins_8888", "hi"), ("band_ins_16_15", "band_ins_16_16", "hi"),
                                  ("band_del_8888", "band_del_88881", "lo"), ("band_del_16_16", "band_del_16_17", "lo")):
        (n_in, t_in), (n_out, t_out) = first(inside), first(outside)
        assert (n_in, n_out) == (1, 2)
        assert getattr(t_in, edge + "_edge") and t_in.end == "ends" and t_out.end == "xdrop"
        assert (t_in.kmax, t_out.kmax) == (31, 31) if edge == "hi" else (t_in.kmin, t_out.kmin) == (-32, -32)
    # the same gaps with the roles swapped reach the other edge
    c = by["band_ins_8888"]
    kept, boxes = search_pair(codes(c.b), codes(c.a))
    assert len(boxes) == 1 and boxes[0].right.kmin == -32 and boxes[0].right.lo_edge


def test_window_spans():
    """Live spans of 31, 32 and 33 diagonals against either edge of the band
    (the 32-lane window holds 32), and spans past 40 from homopolymers and
    tandem repeats of period 2 and 3, right and left of the seed, one with an
    N inside; copy numbers differ by even and by odd counts."""
    by = {c.name: c for c, p in ac.short_corpus().entries if p == "asis"}
    spans = {}
    for name, c in by.items():
        if c.cls in ("span", "repeat"):
            kept, boxes = search_pair(codes(c.a), codes(c.b))
            spans[name] = max(max(b.left.span, b.right.span) for b in boxes)
    assert sorted(spans[n] for n in spans if n.startswith("span_")) == [31, 31, 32, 32, 33, 33]
    for side in ("right", "left"):
        for name in ("homopolymer_22_2", "homopolymer_22_2_N", "tandem2_11_1", "tandem2_11_1_N", "tandem3_8_1"):
            assert spans[f"{name}_{side}"] > 40, (name, side, spans[f"{name}_{side}"])
        assert spans[f"homopolymer_2_13_{side}"] == 23 and 32 < spans[f"tandem2_2_11_{side}"] <= 40


def test_xdrop_boundaries():
    """score < best - X is strict, and tested after the slide: 27 mismatches
    leave exactly best - 108 (live), so a block of 28 is crossed and 29 is not;
    22 gap bases are crossed (21 leave -105) and 23 are not."""
    names = {c.name for c, p in ac.short_corpus().entries}
    for side in ("right", "left"):
        assert {f"mismatch_block_28_{side}", f"mismatch_block_29_{side}"} <= names
    rng = np.random.default_rng(5)
    u = rng.integers(0, 4, 100).astype(np.uint8)
    for m, crossed in ((27, True), (28, True), (29, False)):
        a = np.concatenate([np.zeros(m, np.uint8), u])
        b = np.concatenate([np.ones(m, np.uint8), u])
        r, tr = greedy_trace(a, b)
        assert (r.i == m + 100) == crossed and (r.d == m if crossed else r.score == 0)


def test_transcript_starts_cover_every_residue():
    """The staging code computes (start & 31) + length: the "residue" cases
    put a transcript start at every residue mod 32, in both samples."""
    cor = ac.short_corpus()
    ts = _entries("short", "residue")
    assert ts == list(range(ts[0], ts[0] + 32))
    for s in cor.samples:
        assert {int(s.tx_offsets[t]) % 32 for t in ts} == set(range(32))


def test_evalue_cut_each_direction():
    """At the default e-value the shared exact run of thr/2 - 1, thr/2 and
    thr/2 + 1 bases (thr: the forward or the reverse search's cut, which differ
    because the two transcripts' lengths do) is reported exactly by the
    searches whose cut it meets; some case passes one way and is cut the other."""
    cor = ac.short_corpus()
    _, ora = _oracle("short", 28, 108, 1e-99)
    split, at_cut = 0, set()
    for t, (c, p) in enumerate(cor.entries):
        if c.cls != "evalue":
            continue
        for which, thr in zip("ab", c.props["cuts"]):
            if c.props["score"] == thr:
                at_cut.add((which, p))
        a_in = 0 if p in ("asis", "rc") else 1
        got_a = len(ora[(a_in, 1 - a_in)].get(t, []))
        got_b = len(ora[(1 - a_in, a_in)].get(t, []))
        assert (got_a, got_b) == (int(c.passes[0]), int(c.passes[1])), (cor.case_of(t), c.passes)
        split += c.passes[0] != c.passes[1]
    assert split > 0
    # a score exactly AT the cut, for either transcript as query, in every placement
    assert at_cut == {(w, p) for w in "ab" for p in ac.PLACEMENTS}
    # and the whole corpus at the default cut
    check_transcripts("short", range(len(cor.entries)), evalue=1e-99)


def test_max_hsp_binds():
    by = {c.name: c for c, p in ac.short_corpus().entries if p == "asis"}
    for n in (8, 9, 12):
        c = by[f"max_hsp_{n}"]
        runs = exact_runs(codes(c.a), codes(c.b), 28)
        assert len(runs) == n
        diags = sorted(x - y for x, y, _ in runs)
        assert min(np.diff(diags)) > 64
        kept, boxes = search_pair(codes(c.a), codes(c.b))
        assert len(kept) == len(boxes) == 8


# ------------------------------------------------------------------ seeds at other word sizes


@pytest.mark.parametrize("W", [16, 17, 29, 64])
def test_seed_cases_word_size(W):
    cor = ac.seed_corpus(W)
    n = check_transcripts(str(W), range(len(cor.entries)), W=W)
    for cls in ("seed_run", "seed_N", "seed_end", "seed_pair") + (("seed_dust",) if W >= 23 else ()):
        check_declared(str(W), cls, W)
    phases = {c.seed[0] % (W - 15) for c, p in cor.entries if c.cls == "seed_run" and c.seed}
    assert phases == set(range(W - 15)) and n > 0


@pytest.mark.parametrize("W", [28, 29, 64])
def test_dust_masks_one_search_only(W):
    """With DUST the "seed_dust" run is found by the search whose query is b
    and not by the one whose query is a (its only aligned word is masked): the
    seed that shared searches get from the reverse pass alone."""
    from oracle.align import OracleDB
    cor = _corpus("short" if W == 28 else str(W))
    (t,) = [t for t, (c, p) in enumerate(cor.entries) if c.cls == "seed_dust" and p == "asis"]
    db = OracleDB(cor.samples)
    for q, want in ((0, 0), (1, 1)):
        hs = db.align(q, 1 - q, W, 108, LOOSE, False, (20, 64, 1))
        assert sum(int(h["q_tx"]) - db.tx_base[q] == t for h in hs) == want, (W, q)


@pytest.mark.parametrize("X", [0, 1, 20, 1000])
def test_short_corpus_other_xdrop(X):
    cor = ac.short_corpus()
    ts = [t for t, (c, p) in enumerate(cor.entries) if c.cls not in ("seed_run", "residue")]
    assert check_transcripts("short", ts, X=X) > 0


# ------------------------------------------------------------------ the long corpus


def test_long_corpus():
    """The DMAX pair stops at d = 4096 differences with bases left, its twin
    ends at the transcripts' end with 4095; identical transcripts on either
    side of the bit score's switch to %5.3le (99 999 bits)."""
    from oracle.align import lib
    cor = ac.long_corpus()
    by = {c.name: c for c, p in cor.entries}
    r, tr = greedy_trace(codes(by["dmax"].a)[60:], codes(by["dmax"].b)[60:])
    assert tr.end == "dmax" and r.d == DMAX and tr.steps == DMAX and 60 + r.i < len(by["dmax"].a) - 500
    r, tr = greedy_trace(codes(by["dmax_minus_one"].a)[60:], codes(by["dmax_minus_one"].b)[60:])
    assert r.d == DMAX - 1 and tr.kernel_steps == DMAX - 1 and 60 + r.i == len(by["dmax_minus_one"].a)
    assert check_transcripts("long", range(len(cor.entries))) > 0
    for cls in ("dmax", "bits"):
        check_declared("long", cls)
    bits = {n: int(lib().orc_bits10(2 * n)) for n in (54100, 54150, 54151, 54200)}
    assert bits == {54100: 999040, 54150: 999970, 54151: 1000000, 54200: 1001000}
    assert {c.name for c, p in cor.entries if c.cls == "bits"} == {f"bits_{n}" for n in bits}
    assert max(len(_tx(s, t)) for s in cor.samples for t in range(s.n_tx)) > 50000


# ------------------------------------------------------------------ the second implementation, pinned


def test_extend_trace_random_pairs_against_oracle():
    """300 random pairs with substitutions and indels (fixed seed): every HSP
    of both directed searches equals extend_trace's."""
    from rna_clique_amd.simulate import Sample
    rng = np.random.default_rng(20261020)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    txs = [[], []]
    for n in range(300):
        L = int(rng.integers(60, 420))
        a = rng.integers(0, 4, L)
        b = []
        sub, indel = rng.choice([0.02, 0.06, 0.12]), rng.choice([0.0, 0.01, 0.04])
        for v in a:
            u = rng.random()
            if u < indel / 2:
                continue
            if u < indel:
                b.extend(rng.integers(0, 4, int(rng.integers(1, 9))))
            b.append((v + rng.integers(1, 4)) % 4 if rng.random() < sub else v)
        b = np.array(b, dtype=np.int64)
        if n % 3 == 0:
            b = (3 - b)[::-1]
        txs[n % 2].append(acgt[a].tobytes())
        txs[1 - n % 2].append(acgt[b].tobytes())
    from oracle.align import OracleDB, lib
    samples = [ac._sample(f"R{i}", txs[i]) for i in (0, 1)]
    assert isinstance(samples[0], Sample)
    cor = ac.Corpus(samples, [(ac.Case(f"random_{t}", "random", b"", b""), "asis") for t in range(300)])
    db = OracleDB(samples)
    total = 0
    for X in (108, 30):
        for q in (0, 1):
            ora = oracle_records(db, db.align(q, 1 - q, 28, X, LOOSE, False, None), db.tx_base[q], db.tx_base[1 - q])
            for t in range(300):
                got = ora.get(t, [])
                assert all(g[0] == t for g in got)
                subj = samples[1 - q]
                thr = int(lib().orc_threshold(len(txs[q][t]), int(subj.tx_offsets[-1]), 300, LOOSE))
                want = expected_records(txs[q][t], txs[1 - q][t], 28, X, q == 1, thr)
                assert [g[1:] for g in got] == want, (cor.case_of(t), q, X)
                total += len(want)
    assert total > 800
