"""A second, plain statement of the greedy X-drop extension (spec items 4 and
4b in the header of oracle/align_oracle.c), with a trace of what the walk did.

TEST INFRASTRUCTURE ONLY. Written from the spec text as the furthest-reaching
form of Zhang et al. (2000): after d differences the frontier R[k] is the
furthest base i of the first sequence reached on diagonal k = i - j, the score
of a point is i + j - 6 d half-units (match +2, mismatch -4, gap -5), and a
diagonal is dropped when its score falls more than X below the best seen. It
shares no code with the C oracle or the kernels: a step is a handful of numpy
operations over the 64 diagonals of the band, and a slide is a table lookup
(the length of the exact run that starts at each point of each diagonal).

It serves two ends: it says, without a GPU, which kernel path an input must
take (how wide the live band grows, whether it touches the band's edges, why
the walk ends), and it checks the C oracle's extension independently.
"""
from __future__ import annotations

import dataclasses

import numpy as np

BAND_LO, BAND_HI = -32, 31        # the band is not symmetric: 64 diagonals
NB = BAND_HI - BAND_LO + 1
DMAX = 4096                       # cap on differences
X_DEFAULT = 108
MATCH, MISMATCH, GAP = 2, 4, 5    # half-units; a difference costs 6 on i + j

END_XDROP, END_SEQ, END_DMAX = "xdrop", "ends", "dmax"


@dataclasses.dataclass
class Ext:
    score: int = 0
    i: int = 0
    j: int = 0
    d: int = 0
    gaps: int = 0
    gapopens: int = 0

    def astuple(self):
        return (self.score, self.i, self.j, self.d, self.gaps, self.gapopens)


@dataclasses.dataclass
class Trace:
    span: int = 1          # most diagonals between the lowest and highest live one in a step
    kmin: int = 0          # lowest diagonal ever live
    kmax: int = 0          # highest diagonal ever live
    lo_edge: bool = False  # diagonal -32 was live
    hi_edge: bool = False  # diagonal +31 was live
    steps: int = 0         # greedy steps taken (the last one may leave nothing live)
    end: str = END_SEQ
    best_step: int = 0     # step of the reported result
    # the early-stop edge: the smallest (bound - best) over live diagonals after
    # any step, bound = the score if every remaining base of the diagonal matched
    min_slack: int | None = None
    # steps a walk takes that also stops as soon as no live diagonal's bound
    # exceeds best (the kernels' early stop; the result is the same), and none
    # at all when the first slide uses up either sequence
    kernel_steps: int = 0


def codes(seq):
    """ASCII bytes / str -> codes 0..3 (ACGT, either case), 4 for anything else."""
    lut = np.full(256, 4, dtype=np.uint8)
    for v, c in enumerate(b"ACGT"):
        lut[c] = lut[c | 0x20] = v
    if isinstance(seq, str):
        seq = seq.encode()
    return lut[np.frombuffer(bytes(seq), dtype=np.uint8)]


def revcomp_codes(c):
    c = np.asarray(c, dtype=np.uint8)[::-1]
    return np.where(c < 4, 3 - c, 4).astype(np.uint8)


def _runs(a, b):
    """run[l, i]: length of the exact run starting at (i, i - k), k = l + BAND_LO;
    0 outside either sequence. Non-ACGT never matches."""
    na, nb = len(a), len(b)
    i = np.arange(na + 1)
    j = i[None, :] - (np.arange(NB)[:, None] + BAND_LO)
    ok = (i[None, :] < na) & (j >= 0) & (j < nb)
    ap = np.append(a, 4)
    bv = np.append(b, 5)[np.clip(j, 0, nb)]
    eq = ok & (ap[None, :] == bv) & (ap[None, :] < 4)
    # distance to the next non-match on the row
    stop = np.where(eq, na + 1, i[None, :])
    nxt = np.minimum.accumulate(stop[:, ::-1], axis=1)[:, ::-1]
    return (nxt - i[None, :]).astype(np.int64)


_CACHE = {}


def greedy_trace(a, b, X=X_DEFAULT):
    """Extend from (0, 0) over code arrays a (first role: a gap that consumes a
    base of `a` alone is an insertion, diagonal + 1) and b. Returns (Ext, Trace).
    Results are remembered by content: the two directed searches of a pair
    walk the same sequences (spec 4b)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    key = (a.tobytes(), b.tobytes(), X)
    if key not in _CACHE:
        if len(_CACHE) > 20000:
            _CACHE.clear()
        _CACHE[key] = _greedy_trace(a, b, X)
    e, t = _CACHE[key]
    return dataclasses.replace(e), dataclasses.replace(t)


def _greedy_trace(a, b, X):
    na, nb = len(a), len(b)
    run = _runs(a, b)
    lanes = np.arange(NB)
    k = lanes + BAND_LO
    z = -BAND_LO
    R = np.full(NB, -1, dtype=np.int64)
    G = np.zeros(NB, dtype=np.int64)       # gap bases on the path to the frontier
    O = np.zeros(NB, dtype=np.int64)       # gap openings on it
    E = np.zeros(NB, dtype=np.int64)       # the path ends in: 0 a pair, 1 insertion, 2 deletion
    R[z] = run[z, 0]
    best = Ext(MATCH * int(R[z]), int(R[z]), int(R[z]))
    tr = Trace()
    neg = np.int64(-1)
    stopped = int(R[z]) >= min(na, nb)
    for d in range(1, DMAX + 1):
        tr.steps = d
        j = R - k
        # the three ways onto diagonal k with one more difference
        c_mis = np.where((R >= 0) & (R < na) & (j < nb), R + 1, neg)
        Rl, Gl, Ol, El = (np.concatenate(([v0], v[:-1])) for v, v0 in ((R, -1), (G, 0), (O, 0), (E, 0)))
        c_ins = np.where((Rl >= 0) & (Rl < na), Rl + 1, neg)
        Rr, Gr, Or, Er = (np.concatenate((v[1:], [v0])) for v, v0 in ((R, -1), (G, 0), (O, 0), (E, 0)))
        c_del = np.where((Rr >= 0) & (Rr - (k + 1) < nb), Rr, neg)
        # furthest wins; equal reach: mismatch, then insertion, then deletion
        ni = c_mis.copy()
        ng, no, ne = G.copy(), O.copy(), np.zeros(NB, dtype=np.int64)
        t = c_ins > ni
        ni = np.where(t, c_ins, ni)
        ng = np.where(t, Gl + 1, ng)
        no = np.where(t, Ol + (El != 1), no)
        ne = np.where(t, 1, ne)
        t = c_del > ni
        ni = np.where(t, c_del, ni)
        ng = np.where(t, Gr + 1, ng)
        no = np.where(t, Or + (Er != 2), no)
        ne = np.where(t, 2, ne)
        cand = (ni >= 0) & (ni - k >= 0)
        s = np.where(cand, run[lanes, np.clip(ni, 0, na)], 0)
        ni = ni + s
        ne = np.where(s > 0, 0, ne)
        score = MATCH * ni - k - 6 * d
        live = cand & (score >= best.score - X)
        dropped = bool((cand & ~live).any())
        R = np.where(live, ni, neg)
        G, O, E = ng, no, ne
        if live.any():
            ls = np.where(live, score, np.iinfo(np.int64).min)
            bl = int(np.argmax(ls))                       # first of the equals: lowest diagonal
            if int(ls[bl]) > best.score:
                best = Ext(int(ls[bl]), int(R[bl]), int(R[bl] - k[bl]), d, int(G[bl]), int(O[bl]))
                tr.best_step = d
            kl = k[live]
            lo, hi = int(kl.min()), int(kl.max())
            tr.span = max(tr.span, hi - lo + 1)
            tr.kmin, tr.kmax = min(tr.kmin, lo), max(tr.kmax, hi)
            tr.lo_edge |= lo == BAND_LO
            tr.hi_edge |= hi == BAND_HI
            rem = np.minimum(na - R, nb - (R - k))
            slack = int((score + MATCH * rem)[live].max()) - best.score
            tr.min_slack = slack if tr.min_slack is None else min(tr.min_slack, slack)
            if not stopped:
                tr.kernel_steps = d
                stopped = slack <= 0
        else:
            if not stopped:
                tr.kernel_steps = d
            tr.end = END_XDROP if dropped else END_SEQ
            break
    else:
        tr.end = END_DMAX
    return best, tr


@dataclasses.dataclass
class Box:
    """An HSP in oriented query/subject coordinates (half-open) and its fields."""
    qa: int
    qb: int
    sa: int
    sb: int
    score_half: int
    mismatch: int
    gaps: int
    gapopen: int
    nident: int
    left: Trace = None      # the two extensions' traces and results
    right: Trace = None
    lext: Ext = None
    rext: Ext = None

    def record(self, Lq, strand):
        """(qstart, qend, sstart, send) as BLAST prints them: 1-based, closed, the
        query on its forward strand, the subject running backwards on minus."""
        if not strand:
            return self.qa + 1, self.qb, self.sa + 1, self.sb
        return Lq - self.qb + 1, Lq - self.qa, self.sb, self.sa + 1


def rebuild_hsp(q, s, seed, X=X_DEFAULT, swap=False):
    """The HSP of seed (x, y, len) between oriented query codes q and subject
    codes s. Canonical roles (spec 4b): the lower-numbered sample's sequence
    takes the first role; swap = the query's sample is the higher-numbered one.
    The left extension walks the reversed sequences from the base before the
    seed."""
    x, y, ln = seed
    q = np.asarray(q, dtype=np.uint8)
    s = np.asarray(s, dtype=np.uint8)

    def ext(qa, sa):
        if swap:
            r, t = greedy_trace(sa, qa, X)
            r.i, r.j = r.j, r.i
            return r, t
        return greedy_trace(qa, sa, X)

    r, tr = ext(q[x + ln:], s[y + ln:])
    l, tl = ext(q[:x][::-1], s[:y][::-1])
    d, g = l.d + r.d, l.gaps + r.gaps

    def ident(e):   # aligned pairs = (i + j - gaps) / 2, of which d - gaps mismatch
        return (e.i + e.j - e.gaps) // 2 - (e.d - e.gaps)

    return Box(x - l.i, x + ln + r.i, y - l.j, y + ln + r.j, l.score + MATCH * ln + r.score,
               d - g, g, l.gapopens + r.gapopens, ln + ident(l) + ident(r), tl, tr, l, r)


def is_maximal_run(q, s, seed):
    """seed (x, y, len) is an exact ACGT run that no base extends on either side."""
    x, y, ln = seed
    q = np.asarray(q)
    s = np.asarray(s)
    if x < 0 or y < 0 or x + ln > len(q) or y + ln > len(s):
        return False
    if not ((q[x:x + ln] == s[y:y + ln]) & (q[x:x + ln] < 4)).all():
        return False
    left = x > 0 and y > 0 and q[x - 1] == s[y - 1] and q[x - 1] < 4
    right = x + ln < len(q) and y + ln < len(s) and q[x + ln] == s[y + ln] and q[x + ln] < 4
    return not left and not right


def exact_runs(q, s, W):
    """Every maximal exact ACGT run of at least W bases (W >= 16) between code
    arrays q and s, as (x, y, len) sorted by (x, y): the seeds of spec 2 when
    no query word is masked. From 16-mer hits merged along their diagonals."""
    K = 16
    q = np.asarray(q, dtype=np.uint8)
    s = np.asarray(s, dtype=np.uint8)
    nq, ns = len(q) - K + 1, len(s) - K + 1
    if nq <= 0 or ns <= 0:
        return []

    def words(c, n):
        v = np.zeros(n, dtype=np.uint64)
        bad = np.zeros(n, dtype=bool)
        for t in range(K):
            v |= c[t:t + n].astype(np.uint64) << np.uint64(2 * t)
            bad |= c[t:t + n] > 3
        return v, bad

    qv, qbad = words(q, nq)
    sv, sbad = words(s, ns)
    spos = np.flatnonzero(~sbad)
    order = np.argsort(sv[spos], kind="stable")
    spos, skey = spos[order], sv[spos][order]
    qpos = np.flatnonzero(~qbad)
    lo = np.searchsorted(skey, qv[qpos], "left")
    hi = np.searchsorted(skey, qv[qpos], "right")
    cnt = hi - lo
    if not cnt.sum():
        return []
    i = np.repeat(qpos, cnt)
    j = spos[np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
    o = np.lexsort((i, i - j))
    i, j = i[o], j[o]
    brk = np.ones(len(i), dtype=bool)
    brk[1:] = ((i - j)[1:] != (i - j)[:-1]) | (i[1:] != i[:-1] + 1)
    st = np.flatnonzero(brk)
    ln = np.diff(np.append(st, len(i))) + K - 1
    runs = [(int(i[a]), int(j[a]), int(n)) for a, n in zip(st, ln) if n >= W]
    return sorted(runs)


MAX_HSP = 8


def search_pair(q, s, W=28, X=X_DEFAULT, swap=False):
    """Spec 3 and the purge of spec 5 for one (oriented query, subject)
    transcript pair: seeds in (x, y) order, each one not inside a box found so
    far extended, at most MAX_HSP boxes; then HSPs that share a start or an end
    point with a kept one of higher score (earlier on ties) go. No e-value cut.
    Returns (kept boxes in the order found, all boxes)."""
    boxes = []
    for x, y, ln in exact_runs(q, s, W):
        if len(boxes) >= MAX_HSP:
            break
        if any(b.qa <= x and x + ln <= b.qb and b.sa <= y and y + ln <= b.sb for b in boxes):
            continue
        boxes.append(rebuild_hsp(q, s, (x, y, ln), X, swap))
    order = sorted(range(len(boxes)), key=lambda n: (-boxes[n].score_half, n))
    kept = []
    for n in order:
        b = boxes[n]
        if not any((b.qa, b.sa) == (boxes[m].qa, boxes[m].sa) or (b.qb, b.sb) == (boxes[m].qb, boxes[m].sb)
                   for m in kept):
            kept.append(n)
    return [boxes[n] for n in sorted(kept)], boxes
