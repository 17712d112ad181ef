"""Hand-built inputs for the alignment kernels: each case is a pair of
transcripts that lands on one edge of the spec in the header of
oracle/align_oracle.c (the band -32..+31, the 32-lane window, the X-drop
comparison, the DMAX cap, transcript ends, MAX_HSP, the e-value cut, the
bit-score print rule), with the property it must show on the CPU.

TEST INFRASTRUCTURE ONLY. tests/test_align_cases_host.py checks every case
against the C oracle and against tests/extend_trace.py without a GPU;
tests/test_gpu_align_cases.py runs the corpora through the engine.

A case is built as (a, b): `a` for the lower-numbered sample, whose sequence
takes the first role of the greedy step (spec 4b). Every case is placed four
ways -- as built, with the samples swapped (the roles swap: an insertion
becomes a deletion and the band's two edges change places), with b
reverse-complemented (minus strand: the walk starts from the other end), and
both -- so the declared property is asserted for the placement "asis" and the
other three are checked HSP for HSP against the oracle and the trace.
All filler comes from generators seeded by the case's name and placement:
each placement is its own draw of the case, and no two transcripts of
different cases or placements are related.
"""
from __future__ import annotations

import dataclasses
import functools
import zlib

import numpy as np

from extend_trace import codes, search_pair

PLACEMENTS = ("asis", "swap", "rc", "swaprc")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
U = 220   # a unique exact block that passes the default e-value cut on its own (2 U >= 384)


def revcomp(seq: bytes) -> bytes:
    return seq.translate(_RC)[::-1]


_SALT = "asis"   # the placement being built: each one is its own draw of every case


def _rng(name):
    return np.random.default_rng(zlib.crc32(f"{name}|{_SALT}".encode()))


def _salted(salt, fn, *args):
    global _SALT
    old, _SALT = _SALT, salt
    try:
        return fn(*args)
    finally:
        _SALT = old


def rnd(rng, n) -> bytes:
    return _ACGT[rng.integers(0, 4, int(n))].tobytes()


def other(rng, seq: bytes) -> bytes:
    """A sequence that differs from seq at every base."""
    c = codes(seq)
    return _ACGT[(c + rng.integers(1, 4, len(c))) % 4].tobytes()


def differing(rng, n, first_not=b"", last_not=b"") -> bytes:
    """n random bases whose first / last base avoid the given ones (so that the
    exact runs on either side stay maximal)."""
    s = bytearray(rnd(rng, n))
    if n:
        while bytes(s[:1]) in first_not or (n == 1 and bytes(s[:1]) in last_not):
            s[0] = _ACGT[rng.integers(0, 4)]
        while n > 1 and bytes(s[-1:]) in last_not:
            s[-1] = _ACGT[rng.integers(0, 4)]
    return bytes(s)


@dataclasses.dataclass
class Case:
    name: str
    cls: str                      # the class of section "case builders" it belongs to
    a: bytes
    b: bytes
    seed: tuple | None = None     # (x, y, len) on (a, b), plus strand: a maximal exact run
    hsps: int | None = None       # HSPs of search a -> b as built, before any e-value cut
    single: bool = False          # exactly one HSP, in every placement
    # properties of the declared seed's HSP as built: "left.kmax", "right.end", ... ->
    # value, or ("ge", v) / ("le", v); "box" -> (qa, qb, sa, sb)
    props: dict = dataclasses.field(default_factory=dict)
    # e-value cases: does the one HSP pass the cut when a / b is the query?
    passes: tuple | None = None


@dataclasses.dataclass
class Deferred:
    """A case whose content depends on the e-value thresholds, which depend on
    every transcript's length: the lengths are fixed first."""
    name: str
    cls: str
    la: int
    lb: int
    build: object                 # (name, thr_a, thr_b) -> Case, thr_x: cut when x is the query


def place(case, placement):
    """(transcript of sample 0, transcript of sample 1)."""
    a, b = case.a, case.b
    if placement in ("rc", "swaprc"):
        if placement == "rc":
            b = revcomp(b)
        else:
            a = revcomp(a)
    return (a, b) if placement in ("asis", "rc") else (b, a)


# --------------------------------------------------------------------------
# band and window


def rnd2(rng, n, letters) -> bytes:
    return np.frombuffer(letters, dtype=np.uint8)[rng.integers(0, 2, int(n))].tobytes()


ZONE = 30


def _blocks(name, cls, gaps, side, block=150, **kw):
    """Exact blocks with a gap after each but the last; side "ins": the extra
    bases are in a (diagonals walk up), "del": in b (down). The seed is the
    first block. The gaps are drawn from G and T, the 30 bases of a block next
    to a gap from A and C: on no diagonal of the band does a gap base match,
    so a gap of g costs exactly 5 g."""
    rng = _rng(name)
    blocks = [rnd2(rng, ZONE, b"AC") + rnd(rng, block - 2 * ZONE) + rnd2(rng, ZONE, b"AC")
              for _ in range(len(gaps) + 1)]
    long = bytearray(blocks[0])
    for g, nxt in zip(gaps, blocks[1:]):
        long += rnd2(rng, g, b"GT") + nxt
    short = b"".join(blocks)
    a, b = (bytes(long), short) if side == "ins" else (short, bytes(long))
    return Case(name, cls, a, b, seed=(0, 0, block), **kw)


def band_cases():
    out = []
    R = "right."
    # +31 is the last diagonal of the band, +32 is outside; -32 is inside, -33 outside
    out.append(_blocks("band_ins_8887", "band", [8, 8, 8, 7], "ins", single=True, hsps=1,
                       props={R + "kmax": 31, R + "hi_edge": True}))
    out.append(_blocks("band_ins_8888", "band", [8, 8, 8, 8], "ins", hsps=2,
                       props={R + "kmax": 31, R + "end": "xdrop", "box": (0, 624, 0, 600)}))
    out.append(_blocks("band_ins_16_15", "band", [16, 15], "ins", single=True, hsps=1,
                       props={R + "kmax": 31, R + "hi_edge": True}))
    out.append(_blocks("band_ins_16_16", "band", [16, 16], "ins", hsps=2,
                       props={R + "kmax": 31, R + "end": "xdrop", "box": (0, 316, 0, 300)}))
    out.append(_blocks("band_ins_16_14", "band", [16, 14], "ins", single=True, hsps=1,
                       props={R + "kmax": ("le", 31)}))
    out.append(_blocks("band_del_8888", "band", [8, 8, 8, 8], "del", hsps=1,
                       props={R + "kmin": -32, R + "lo_edge": True}))
    out.append(_blocks("band_del_88881", "band", [8, 8, 8, 8, 1], "del", hsps=2,
                       props={R + "kmin": -32, R + "end": "xdrop"}))
    out.append(_blocks("band_del_16_16", "band", [16, 16], "del", hsps=1,
                       props={R + "kmin": -32, R + "lo_edge": True}))
    out.append(_blocks("band_del_16_17", "band", [16, 17], "del", hsps=2,
                       props={R + "kmin": -32, R + "end": "xdrop", "box": (0, 300, 0, 316)}))
    out.append(_blocks("band_del_16_15", "band", [16, 15], "del", single=True, hsps=1,
                       props={R + "kmin": ("ge", -32)}))
    # one gap of g: the drop is 5 g against X = 108. The test comes after the
    # slide, so the last gap base is free of it: 21 gap bases leave -105 (live),
    # the 22nd lands on the match and slides; a gap of 23 is dropped at -110
    for side in ("ins", "del"):
        for g in (21, 22):
            out.append(_blocks(f"gap{g}_{side}", "gap", [g], side, block=250, single=True, hsps=1,
                               props={"box": (0, 500 + g, 0, 500) if side == "ins" else (0, 500, 0, 500 + g)}))
        # (the second block's HSP may share an end point with this one and be purged)
        out.append(_blocks(f"gap23_{side}", "gap", [23], side, block=250, props={"box": (0, 250, 0, 250)}))
    return out


def _repeat(name, unit, na, nb, side, n_at=None, tail=60):
    """A unique block next to a tandem repeat with na copies in a, nb in b,
    then a shared tail at which both transcripts end: only the repeat's ties
    spread the live diagonals. side: the repeat right or left of the unique
    block. n_at: an N at that base of a's repeat."""
    rng = _rng(name)
    u, t = rnd(rng, U), rnd(rng, tail)
    ra, rb = bytearray(unit * na), unit * nb
    if n_at is not None:
        ra[n_at] = ord("N")
    a = u + bytes(ra) + t
    b = u + rb + t
    if side == "left":
        a, b = a[::-1], b[::-1]
    return Case(name, "repeat", a, b)


def repeat_cases():
    """Every run stays under 28 bases, so that the repeats of different cases
    and placements cannot seed each other."""
    out = []
    for side in ("right", "left"):
        out.append(_repeat(f"homopolymer_22_2_{side}", b"A", 22, 2, side))
        out.append(_repeat(f"homopolymer_2_13_{side}", b"C", 2, 13, side))
        out.append(_repeat(f"tandem2_11_1_{side}", b"AC", 11, 1, side))
        out.append(_repeat(f"tandem2_2_11_{side}", b"AG", 2, 11, side))
        out.append(_repeat(f"tandem3_8_1_{side}", b"ACG", 8, 1, side))
        out.append(_repeat(f"tandem3_2_8_{side}", b"CAT", 2, 8, side))
        out.append(_repeat(f"homopolymer_22_2_N_{side}", b"G", 22, 2, side, n_at=9))
        out.append(_repeat(f"tandem2_11_1_N_{side}", b"CT", 11, 1, side, n_at=11))
    return out


def span_case(name, side, gaps, delta):
    """Gaps walk the alignment to diagonal +sum(gaps) (side "ins") or
    -sum(gaps) ("del"); then a homopolymer with delta more copies on the OTHER
    side brings it back, and its ties spread the live diagonals by delta either
    way: 2 delta + 1 of them unless the band's edge cuts some off. Both
    transcripts end with the shared tail, so nothing else widens the span."""
    rng = _rng(name)
    c = _blocks(name, "span", gaps, side)
    sp, t = rnd(rng, 19) + b"C", b"G" + rnd(rng, 120)
    more, fewer = sp + b"A" * (4 + delta) + t, sp + b"A" * 4 + t
    c.a += fewer if side == "ins" else more
    c.b += more if side == "ins" else fewer
    return c


def span_cases():
    """Live spans of exactly 31, 32 and 33 diagonals (the 32-lane window holds
    32), against either edge of the band: from +16, 16 ties either way are
    diagonals 0..+32, of which +32 is outside (32 live); from -16 they are
    -32..0, all inside (33 live); from -17, -33 is outside (32 live)."""
    out = []
    for name, side, gaps, delta, span, lo, hi in (
            ("span_31_up", "ins", [8, 8], 15, 31, 1, 31), ("span_32_up", "ins", [8, 8], 16, 32, 0, 31),
            ("span_33_up", "ins", [8, 7], 16, 33, -1, 31), ("span_31_down", "del", [8, 8], 15, 31, -31, -1),
            ("span_33_down", "del", [8, 8], 16, 33, -32, 0), ("span_32_down", "del", [8, 9], 16, 32, -32, -1)):
        c = span_case(name, side, gaps, delta)
        c.hsps, c.single = 1, True
        c.props = {"right.span": span, "right.end": "ends", **({"right.kmax": hi} if side == "ins" else {"right.kmin": lo})}
        out.append(c)
    return out


# --------------------------------------------------------------------------
# X-drop


def _mismatch_block(name, m, side):
    rng = _rng(name)
    u1, u2 = rnd(rng, U), rnd(rng, U)
    a = u1 + rnd2(rng, 64, b"AC")[:m] + u2
    b = u1 + rnd2(rng, 64, b"GT")[:m] + u2
    if side == "left":
        a, b = a[::-1], b[::-1]
    return Case(name, "xdrop", a, b)


def xdrop_cases():
    """The longest pure-mismatch block an extension crosses and one base more,
    for the right and for the left extension; the boundary is found with the
    trace (4 m against X = 108: m = 27 is crossed, the comparison is strict).
    The block is drawn from A and C on one side and from G and T on the other:
    nothing in it matches on any diagonal, and a detour of k diagonals (10 k)
    pairs at most k block bases with flank bases (6 k to gain)."""
    out = []
    for side in ("right", "left"):
        n = {m: len(search_pair(codes(c.a), codes(c.b))[0])
             for m in range(24, 33) for c in [_mismatch_block(f"mismatch_block_{m}_{side}", m, side)]}
        edge = max(m for m in n if n[m] == 1)
        assert all(n[m] == (1 if m <= edge else 2) for m in n), n
        for m in (edge, edge + 1):
            c = _mismatch_block(f"mismatch_block_{m}_{side}", m, side)
            c.hsps = 1 if m == edge else 2
            c.single = m == edge
            out.append(c)
    return out


# --------------------------------------------------------------------------
# ends


def end_cases():
    out = []
    for n in (28, 29, 32, 33, 63, 64, 65, 300):
        s = rnd(_rng(f"identical_{n}"), n)
        out.append(Case(f"identical_{n}", "ends", s, s, seed=(0, 0, n), single=True, hsps=1,
                        props={"box": (0, n, 0, n), "right.end": "ends", "left.end": "ends"}))
    for name, lo in (("prefix", 0), ("suffix", 240), ("infix", 120)):
        s = rnd(_rng(name), 500)
        out.append(Case(name, "ends", s, s[lo:lo + 260], seed=(lo, 0, 260), single=True, hsps=1,
                        props={"box": (lo, lo + 260, 0, 260)}))

    def parts(name):
        rng = _rng(name)
        u, fa, fb = rnd(rng, U), rnd(rng, 90), rnd(rng, 131)
        fb = other(rng, fa[:1]) + fb[1:]
        return u, fa, fb, fa[::-1], fb[::-1], rnd(rng, 80)

    u, fa, fb, ga, gb, x = parts("seed_at_base_0")
    out.append(Case("seed_at_base_0", "ends", u + fa, u + fb, seed=(0, 0, U), props={"left.kernel_steps": 0}))
    u, fa, fb, ga, gb, x = parts("seed_at_last_base")
    out.append(Case("seed_at_last_base", "ends", ga + u, gb + u, seed=(90, 131, U), props={"right.kernel_steps": 0}))
    u, fa, fb, ga, gb, x = parts("query_end_only")
    out.append(Case("query_end_only", "ends", ga + u, gb + u + x, seed=(90, 131, U), props={"right.kernel_steps": 0}))
    u, fa, fb, ga, gb, x = parts("subject_end_only")
    out.append(Case("subject_end_only", "ends", ga + u + x, gb + u, seed=(90, 131, U), props={"right.kernel_steps": 0}))
    # transcript starts at every residue mod 32 of the packed array: eight
    # identical pairs of 201 bases, four placements each, are 32 consecutive
    # transcripts of either sample, and 201 = 9 (mod 32) is a unit mod 32
    for r in range(8):
        s = rnd(_rng(f"residue_{r}"), 201)
        out.append(Case(f"residue_{r}", "residue", s, s, seed=(0, 0, 201), single=True, hsps=1))
    return out


def early_stop_cases(flank=True):
    """A long exact block, one mismatch, then k matching bases at the very end
    of both transcripts. Crossing the mismatch costs 4 and the k bases pay 2 k:
    k = 1 loses, k = 2 ties (the result stays before the mismatch; the bound
    of the live diagonal equals best exactly), k = 3 wins by 2. In every one a
    walk that stops when no bound exceeds best takes one step. flank: unrelated
    bases on the block's other side (else the transcripts begin with it)."""
    out = []
    for side in ("right", "left"):
        for k in (1, 2, 3):
            rng = _rng(f"early_stop_{side}_{k}_{flank}")
            u, t = rnd(rng, U), rnd(rng, 3)[:k]
            x = rnd(rng, 1)
            fa, fb = (rnd(rng, 35), rnd(rng, 47)) if flank else (b"", b"")
            a = fa + u + x + t
            b = fb + u + other(rng, x) + t
            seed, ext = (len(fa), len(fb), U), "right"
            if side == "left":
                a, b = a[::-1], b[::-1]
                seed, ext = (1 + k, 1 + k, U), "left"
            reach = 1 + k if k == 3 else 0
            out.append(Case(f"early_stop_{side}_{k}" + ("" if flank else "_bare"), "early_stop", a, b, seed=seed,
                            hsps=1, single=True,
                            props={ext + ".kernel_steps": 1, ext[0] + "ext.i": reach, ext[0] + "ext.j": reach}))
    return out


# --------------------------------------------------------------------------
# seeds, for a word size W


def _run_pair(rng, x, y, run, la, lb):
    """a and b with the exact run `run` at a[x:], b[y:] and nothing else in common
    on that diagonal's neighbourhood: the bases next to the run differ."""
    n = len(run)
    pa, pb = rnd(rng, x), rnd(rng, y)
    if x and y:
        pb = pb[:-1] + other(rng, pa[-1:])
    sa, sb = rnd(rng, la - x - n), rnd(rng, lb - y - n)
    if sa and sb:
        sb = other(rng, sa[:1]) + sb[1:]
    return pa + run + sa, pb + run + sb


def seed_cases(W):
    """Exact runs of W - 1, W and W + 1 at every phase x mod (W - 15) of the
    query stride; runs cut by an N; runs touching a transcript end; two runs on
    one diagonal a mismatch apart. (Both strands come with the placements.)"""
    s = W - 15
    out = []
    x0 = s * -(-24 // s)
    for ph in range(s):
        for n in (W - 1, W, W + 1):
            name = f"w{W}_run{n}_phase{ph}"
            rng = _rng(name)
            x, y = x0 + ph, 31 + (ph * 7) % 23
            a, b = _run_pair(rng, x, y, rnd(rng, n), x + n + 40, y + n + 33)
            out.append(Case(name, "seed_run", a, b, seed=(x, y, n) if n >= W else None,
                            hsps=1 if n >= W else 0, single=n >= W))
    for n, at, hs in ((2 * W - 1, W - 1, 0), (2 * W, W - 1, 1), (2 * W, W, 1), (2 * W + 1, W, 1)):
        # an N at base `at` of a's copy of a run of n bases leaves exact runs of
        # at | n - at - 1 bases: no seed, one, one, two seeds (one HSP: the
        # first one's extension crosses the N)
        name = f"w{W}_run{n}_N_at_{at}"
        rng = _rng(name)
        a, b = _run_pair(rng, 30, 44, rnd(rng, n), 30 + n + 25, 44 + n + 25)
        a = a[:30 + at] + b"N" + a[30 + at + 1:]
        out.append(Case(name, "seed_N", a, b, hsps=hs, single=hs == 1))
    for n in (W - 1, W, W + 1):
        for end in ("start", "end"):
            name = f"w{W}_run{n}_at_{end}"
            rng = _rng(name)
            a, b = _run_pair(rng, 0, 0, rnd(rng, n), n + 50, n + 61)
            seed = (0, 0, n)
            if end == "end":
                a, b = a[::-1], b[::-1]
                seed = (50, 61, n)
            out.append(Case(name, "seed_end", a, b, seed=seed if n >= W else None,
                            hsps=1 if n >= W else 0, single=n >= W))
    if W >= 23:
        # an exact run of W bases holds one aligned word of either transcript:
        # a's in its last 16 bases (x = 1 mod the stride), b's in its first 16
        # (y = 0). A×9 inside a's word and past b's is DUST-masked, so with DUST
        # the search with a as query finds no seed and the one with b does:
        # as built a reverse-only seed of shared searches (swapped, forward-only)
        name = f"w{W}_run{W}_dust_masks_one_word"
        rng = _rng(name)
        run = bytearray(rnd(rng, W))
        lo = max(16, s - 1)
        at = lo + (W - lo - 9) // 2
        run[at - 1:at + 10] = b"C" + b"A" * 9 + b"G"
        a, b = _run_pair(rng, 2 * s + 1, 3 * s, bytes(run), 2 * s + 1 + W + 37, 3 * s + W + 48)
        out.append(Case(name, "seed_dust", a, b, seed=(2 * s + 1, 3 * s, W), hsps=1, single=True))
    name = f"w{W}_two_runs_one_mismatch"
    rng = _rng(name)
    r1, r2, x = rnd(rng, W + 10), rnd(rng, W + 10), rnd(rng, 1)
    a, b = _run_pair(rng, 26, 39, r1 + x + r2, 26 + 2 * W + 21 + 30, 39 + 2 * W + 21 + 30)
    b = b[:39 + W + 10] + other(rng, x) + b[39 + W + 11:]
    out.append(Case(name, "seed_pair", a, b, seed=(26, 39, W + 10), hsps=1, single=True))
    return out


def _box_seed(name, inside, tries=200):
    """a = P R M R' x ..., b = P R M R' y ...: the diagonal-0 HSP ends after R'
    (R without its last base r). The run a's first R against b's second copy
    lies inside that box when y != r, and sticks out by the one base r when
    y = r. Found by search over the filler: the box of the first HSP must end
    exactly there."""
    for t in range(tries):
        rng = _rng(f"{name}_{t}")
        p, r, m = rnd(rng, 120), rnd(rng, 31), rnd(rng, 80)
        x = other(rng, r[-1:])
        y = r[-1:] if not inside else other(rng, r[-1:])
        if y == x:
            continue
        body = p + r + m + r[:-1]
        a = body + x + rnd(rng, 40)
        b = body + y + rnd(rng, 55)
        kept, boxes = search_pair(codes(a), codes(b))
        e = len(body)
        if (boxes[0].qa, boxes[0].qb, boxes[0].sa, boxes[0].sb) != (0, e, 0, e):
            continue
        if len(boxes) == (1 if inside else 2) and len(kept) == len(boxes):
            return Case(name, "seed_box", a, b, seed=(0, 0, e), hsps=len(boxes), single=inside)
    raise AssertionError(name)


def box_seed_cases():
    return [_box_seed("second_seed_inside_box", True), _box_seed("second_seed_out_by_one", False)]


# --------------------------------------------------------------------------
# MAX_HSP


def max_hsp_case(n, block=60, spacer=70):
    """n exact blocks, contiguous in b and `spacer` bases apart in a: each on
    its own diagonal, more than 64 from every other, so no extension joins two."""
    name = f"max_hsp_{n}"
    rng = _rng(name)
    blocks = [rnd(rng, block) for _ in range(n)]
    a = bytearray()
    for i, bl in enumerate(blocks):
        a += bl
        if i + 1 < n:
            a += differing(rng, spacer, first_not=blocks[i + 1][:1], last_not=bl[-1:])
    return Case(name, "max_hsp", bytes(a), b"".join(blocks), seed=(0, 0, block), hsps=min(n, 8))


# --------------------------------------------------------------------------
# e-value cut


def _evalue_case(which, delta):
    """One HSP whose score is thr - 2, thr or thr + 2, thr = the cut of the
    search with a (or b) as query. An exact run of n bases scores 2 n; an odd
    score takes two runs with one extra base of a between them (2 n - 5), so
    the middle case sits exactly AT the cut whatever its parity."""
    def build(name, thr_a, thr_b, la=300, lb=1400, tries=300):
        target = (thr_a if which == "a" else thr_b) + 2 * delta
        n = target // 2 if target % 2 == 0 else (target + 5) // 2
        n2 = 0 if target % 2 == 0 else 20
        for t in range(tries):
            rng = _rng(f"{name}_{t}")
            x, y = 20 + int(rng.integers(0, la - n - 45)), 20 + int(rng.integers(0, lb - n - 45))
            run = rnd(rng, n)
            if n2:   # the extra base differs from both of its neighbours' partners
                extra = differing(rng, 1, first_not=run[n - n2:n - n2 + 1], last_not=run[n - n2 - 1:n - n2])
                a, b = _run_pair(rng, x, y, run, la - 1, lb)
                a = a[:x + n - n2] + extra + a[x + n - n2:]
            else:
                a, b = _run_pair(rng, x, y, run, la, lb)
            kept, boxes = search_pair(codes(a), codes(b))
            if len(boxes) == 1 and (boxes[0].qa, boxes[0].qb, boxes[0].score_half) == (x, x + n + (1 if n2 else 0), target):
                return Case(name, "evalue", a, b, seed=(x, y, n - n2), hsps=1, single=True,
                            passes=(target >= thr_a, target >= thr_b), props={"score": target, "cuts": (thr_a, thr_b)})
        raise AssertionError(name)
    return Deferred(f"evalue_{which}_{delta:+d}", "evalue", 300, 1400, build)


def evalue_cases():
    return [_evalue_case(w, d) for w in ("a", "b") for d in (-1, 0, 1)]


# --------------------------------------------------------------------------
# corpora


@dataclasses.dataclass
class Corpus:
    samples: list
    entries: list                 # transcript t of either sample: (Case, placement)

    def case_of(self, t):
        c, p = self.entries[t]
        return f"{c.name}[{p}]"

    def name_messages(self, msgs):
        """Parity messages with the case of the first differing transcript."""
        import re
        out = []
        for m in msgs:
            hit = re.search(r"GPU \[(\d+), (\d+),.* vs oracle \[(\d+), (\d+),", m)
            if hit:
                n = len(self.entries)
                tx = sorted({int(g) % n for g in hit.groups()})
                m += "  <- " + ", ".join(self.case_of(t) for t in tx)
            out.append(m)
        return out


def _sample(name, txs):
    from rna_clique_amd.simulate import Sample
    offs = np.zeros(len(txs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(t) for t in txs])
    n = len(txs)
    return Sample(name, np.frombuffer(b"".join(txs), dtype=np.uint8).copy(), offs,
                  np.arange(n, dtype=np.int32), np.ones(n, dtype=np.int32), 1.0 + np.arange(n) / 8.0)


def build_corpus(make_cases, placements=PLACEMENTS, evalue=1e-99):
    """Two samples; case c in placement p is transcript t of both (gene t).
    make_cases() is called once per placement (its own draw of every case).
    Deferred cases get the thresholds of the finished corpus: every length is
    known before their content is chosen."""
    from oracle.align import lib
    drawn = {p: _salted(p, make_cases) for p in placements}
    n = len(drawn[placements[0]])
    assert all([c.name for c in drawn[p]] == [c.name for c in drawn[placements[0]]] for p in placements)
    plan = [(drawn[p][i], p) for i in range(n) for p in placements]
    lens = [[], []]
    for c, p in plan:
        la, lb = (c.la, c.lb) if isinstance(c, Deferred) else (len(c.a), len(c.b))
        a_in = 0 if p in ("asis", "rc") else 1
        lens[a_in].append(la)
        lens[1 - a_in].append(lb)
    dblen, dbn = [sum(lens[0]), sum(lens[1])], len(plan)
    txs, entries = [[], []], []
    for c, p in plan:
        if isinstance(c, Deferred):
            a_in = 0 if p in ("asis", "rc") else 1
            thr_a = int(lib().orc_threshold(c.la, dblen[1 - a_in], dbn, evalue))
            thr_b = int(lib().orc_threshold(c.lb, dblen[a_in], dbn, evalue))
            c = c.build(f"{c.name}_{p}", thr_a, thr_b)
        t0, t1 = place(c, p)
        txs[0].append(t0)
        txs[1].append(t1)
        entries.append((c, p))
    assert [len(t) for t in txs[0]] == lens[0] and [len(t) for t in txs[1]] == lens[1]
    return Corpus([_sample("S0", txs[0]), _sample("S1", txs[1])], entries)


def short_cases(amb=True):
    cases = (band_cases() + span_cases() + repeat_cases() + xdrop_cases() + end_cases() +
             early_stop_cases() + early_stop_cases(False) + seed_cases(28) + box_seed_cases() +
             [max_hsp_case(n) for n in (8, 9, 12)] + evalue_cases())
    return [c for c in cases if amb or isinstance(c, Deferred) or b"N" not in c.a + c.b]


@functools.lru_cache(maxsize=None)
def short_corpus(amb=True):
    """Every transcript under 1.5 kb: whole-transcript staging. amb False
    leaves out the cases that hold an N: one N anywhere puts a whole engine on
    its ambiguous-base kernels, so the plain ones need a corpus without. Read
    only."""
    return build_corpus(functools.partial(short_cases, amb))


def step_count_cases():
    """Pairs whose every extension ends at a transcript end with few live
    diagonals: nothing outgrows the 32-lane window, every search has one seed,
    so the engine's step counter is the sum of the traces' kernel_steps."""
    return early_stop_cases(False) + [c for c in end_cases() if c.name in ("identical_64", "identical_300")]


@functools.lru_cache(maxsize=None)
def step_count_corpus():
    return build_corpus(step_count_cases, placements=("asis", "swap"))


@functools.lru_cache(maxsize=None)
def seed_corpus(W):
    return build_corpus(functools.partial(seed_cases, W))


# ---- long corpus: windowed staging cannot be avoided

DMAX_LEN = 17500


def _dmax_pair(name, length):
    """60 exact bases, then a mismatch at every fourth base."""
    rng = _rng(name)
    a = np.frombuffer(rnd(rng, DMAX_LEN), dtype=np.uint8).copy()
    b = a.copy()
    pos = np.arange(60, DMAX_LEN, 4)
    b[pos] = np.frombuffer(other(rng, a[pos].tobytes()), dtype=np.uint8)
    return Case(name, "dmax", a[:length].tobytes(), b[:length].tobytes(), seed=(0, 0, 60))


# the extension of the full pair stops at DMAX = 4096 differences (base 16 444);
# cut before the 4096th mismatch, the twin ends at the transcripts' end one short
DMAX_TWIN_LEN = 60 + 4 * 4095


def long_cases():
    out = [(_dmax_pair("dmax", DMAX_LEN), ("asis", "rc")),
           (_dmax_pair("dmax_minus_one", DMAX_TWIN_LEN), ("asis",))]
    # the bit-score print rule switches to %5.3le past 99 999 bits: between raw
    # scores 108 300 and 108 302 half-units, identical transcripts of 54 150 and
    # 54 151 bases (99 997.2 and 99 999.05 bits)
    for n in (54100, 54150, 54151, 54200):
        s = rnd(_rng(f"bits_{n}"), n)
        out.append((Case(f"bits_{n}", "bits", s, s, seed=(0, 0, n), single=True, hsps=1,
                         props={"box": (0, n, 0, n)}), ("asis",)))
    return out


@functools.lru_cache(maxsize=None)
def long_corpus():
    """Transcripts of 16 to 54 kb: windowed staging. The cases are placed as
    listed (not four ways): the DMAX pair on both strands. Read only."""
    txs, entries = [[], []], []
    for i, (_, ps) in enumerate(long_cases()):
        for p in ps:
            c = _salted(p, long_cases)[i][0]
            t0, t1 = place(c, p)
            txs[0].append(t0)
            txs[1].append(t1)
            entries.append((c, p))
    return Corpus([_sample("L0", txs[0]), _sample("L1", txs[1])], entries)
