// The full-band extension of seed-and-extend (the pass order: align.hip):
//
//   extend_kernel        one wave per search (the full band, seeds by
//                        selection, purge, cuts): what the row kernels and
//                        the later-seed rounds cannot take.
//
// Host entry point: launch_extend_retry.
//
// Semantics: oracle/align_oracle.c ("RC-megablast v1"), bit for bit.
#include "align_common.h"
#include "launch.h"

namespace rcg {

constexpr int EWAVES = EBLOCK / 64;
#ifndef EXT_MIN_WAVES
#define EXT_MIN_WAVES 8
#endif
constexpr int STAGE_BASES = 8192;                 // staged transcript length limit

// wave-uniform copies (SGPR) of values the compiler cannot prove uniform
// (LDS and vector-memory loads at a uniform address)
__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t rfl(uint64_t v)
{
    return ((uint64_t)rfl((uint32_t)(v >> 32)) << 32) | rfl((uint32_t)v);
}


// ------------------------------------------------------------------------
// extension
// ------------------------------------------------------------------------

struct ExtRes {
    int score, i, j, d, g, o;
};

// Max over the wave: DPP inside rows of 16 (xor 1, xor 2, half-row mirror,
// row mirror), then the four row maxima through readlane. No LDS round trips.
__device__ __forceinline__ int wave_max(int v)
{
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, false));  // row_mirror
    const int a = max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16));
    const int b = max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48));
    return max(a, b);
}

// lane l <- lane l-1 (lane 0 gets `edge`) / lane l <- lane l+1 (lane 63 gets
// `edge`): gfx9-family DPP wavefront shifts, one VALU op each.
__device__ __forceinline__ int from_lower(int v, int edge)
{
    return __builtin_amdgcn_update_dpp(edge, v, 0x138, 0xF, 0xF, false);   // wave_shr:1
}
__device__ __forceinline__ int from_upper(int v, int edge)
{
    return __builtin_amdgcn_update_dpp(edge, v, 0x130, 0xF, 0xF, false);   // wave_shl:1
}

// 32 bases starting at base p of a packed array viewed as dwords (16 bases
// each): three dword loads and two funnel shifts (v_alignbit_b32).
template <typename PT>
__device__ __forceinline__ uint64_t win3(const uint32_t *__restrict__ a, PT p)
{
    const PT i = p >> 4;
    const uint32_t sh = ((uint32_t)p & 15u) * 2u;
    const uint32_t w0 = a[i], w1 = a[i + 1], w2 = a[i + 2];
    const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh);
    const uint32_t hi = __builtin_amdgcn_alignbit(w2, w1, sh);
    return ((uint64_t)hi << 32) | lo;
}

// Matching bases walking forward from (pa, pb) (BACK = false) or backwards
// from (pa - 1, pb - 1) (BACK = true; the window ending at p is read at p - 32
// and the first mismatch is its highest differing base), at most maxn.
template <bool AMB, bool BACK, typename PT>
__device__ __forceinline__ int slide(const uint32_t *A, const uint32_t *AM, PT pa, const uint32_t *B,
                                     const uint32_t *BM, PT pb, int maxn)
{
    int n = 0;
    while (n < maxn) {
        const PT qa = BACK ? pa - (PT)(n + 32) : pa + (PT)n;
        const PT qb = BACK ? pb - (PT)(n + 32) : pb + (PT)n;
        uint64_t x = win3(A, qa) ^ win3(B, qb);
        if (AMB) x |= win3(AM, qa) | win3(BM, qb);
        if (x == 0) {
            n += 32;
            continue;
        }
        n += (BACK ? __builtin_clzll(x) : __builtin_ctzll(x)) >> 1;
        return n < maxn ? n : maxn;
    }
    return maxn > 0 ? maxn : 0;
}

// Greedy X-drop extension (oracle/align_oracle.c greedy_ext), one diagonal per
// lane of the wave. A / B: oriented query and subject; the walk starts at
// (pa, pb) forward, or at (pa - 1, pb - 1) backwards. Branch-free step; the
// per-lane gap state G | O << 13 | E << 26 travels in one register. Stops as
// soon as no live diagonal can still beat the best score (score + 2 x bases
// left on the shorter side <= best): the result is unchanged.
template <bool AMB, bool BACK, typename PT>
__device__ __forceinline__ ExtRes ext_wave(const uint32_t *A, const uint32_t *AM, PT pa, int alen,
                                           const uint32_t *B, const uint32_t *BM, PT pb, int blen, int X,
                                           int lane, uint32_t &steps, uint32_t &edge)
{
    constexpr int EBIT = 26, OBIT = 13;
    constexpr int GMASK = 8191;
    const int k = lane + BAND_LO;
    int r0 = 0;
    if (lane == -BAND_LO) r0 = slide<AMB, BACK, PT>(A, AM, pa, B, BM, pb, min(alen, blen));
    r0 = __builtin_amdgcn_readlane(r0, -BAND_LO);
    ExtRes best = {2 * r0, r0, r0, 0, 0, 0};
    if (min(alen, blen) - r0 <= 0) return best;
    int R = lane == -BAND_LO ? r0 : -1;
    int goe = 0;
    for (int d = 1; d <= DMAX; ++d) {
        steps++;
        const int Rl = from_lower(R, -1), Rr = from_upper(R, -1);
        const int gl = from_lower(goe, 0), gr = from_upper(goe, 0);
        // candidates; ties prefer mismatch, then insertion, then deletion
        const int cm = (R >= 0 && R < alen && R - k < blen) ? R + 1 : -1;
        const int ci = (Rl >= 0 && Rl < alen) ? Rl + 1 : -1;
        const int cd = (Rr >= 0 && Rr - (k + 1) < blen) ? Rr : -1;
        int ni = max(max(cm, ci), cd);
        const bool fm = ni >= 0 && cm == ni, fi = !fm && ci == ni;
        const int gi = (gl & ~(3 << EBIT)) + 1 + ((((gl >> EBIT) & 3) == 1) ? 0 : (1 << OBIT)) + (1 << EBIT);
        const int gd = (gr & ~(3 << EBIT)) + 1 + ((((gr >> EBIT) & 3) == 2) ? 0 : (1 << OBIT)) + (2 << EBIT);
        int ng = fm ? (goe & ~(3 << EBIT)) : (fi ? gi : gd);
        int score = INT_MIN, bound = INT_MIN;
        if (ni >= 0) {
            const int ja = ni - k;
            const int m = min(alen - ni, blen - ja);
            const int s = slide<AMB, BACK, PT>(A, AM, BACK ? pa - (PT)ni : pa + (PT)ni, B, BM,
                                               BACK ? pb - (PT)ja : pb + (PT)ja, m);
            ni += s;
            if (s > 0) ng &= ~(3 << EBIT);
            score = 2 * ni - k - 6 * d;
            if (score < best.score - X) ni = -1;
            bound = score + 2 * (m - s);
        }
        R = ni;
        goe = ng;
        const bool live = ni >= 0;
        if (!__ballot(live)) break;
        // the 64-diagonal band binds (spec 3): a live diagonal at its edge
        if (__ballot(live && (lane == 0 || lane == BAND - 1))) edge = 1;
        if (__ballot(live && score > best.score)) {
            // (score, lowest lane) as one key: score * 64 + (63 - lane)
            const int mk = wave_max(live ? score * 64 + (63 - lane) : INT_MIN);
            const int bl = 63 - (mk & 63);
            best.score = mk >> 6;
            best.i = __builtin_amdgcn_readlane(R, bl);
            best.j = best.i - (bl + BAND_LO);
            best.d = d;
            const int bg = __builtin_amdgcn_readlane(goe, bl);
            best.g = bg & GMASK;
            best.o = (bg >> OBIT) & GMASK;
        }
        if (!__ballot(live && bound > best.score)) break;
    }
    return best;
}

// Both extensions of one seed (x, y, len): right from its end, left from its
// start. swap (spec 4b): the query is the higher-numbered sample, so the
// greedy primitive runs with the subject in the first role and its end
// point is swapped back.
template <bool AMB, typename PT>
__device__ __forceinline__ void extend_seed(const uint32_t *QO, const uint32_t *QOM, PT qo, const uint32_t *TF,
                                            const uint32_t *TFM, PT tf, int Lq, int Lt, int x, int y, int len, int X,
                                            int lane, uint32_t &steps, uint32_t &eg, bool swap, ExtRes &r, ExtRes &l)
{
    if (!swap) {
        r = ext_wave<AMB, false, PT>(QO, QOM, qo + (PT)(x + len), Lq - (x + len), TF, TFM, tf + (PT)(y + len),
                                     Lt - (y + len), X, lane, steps, eg);
        l = ext_wave<AMB, true, PT>(QO, QOM, qo + (PT)x, x, TF, TFM, tf + (PT)y, y, X, lane, steps, eg);
    } else {
        r = ext_wave<AMB, false, PT>(TF, TFM, tf + (PT)(y + len), Lt - (y + len), QO, QOM, qo + (PT)(x + len),
                                     Lq - (x + len), X, lane, steps, eg);
        l = ext_wave<AMB, true, PT>(TF, TFM, tf + (PT)y, y, QO, QOM, qo + (PT)x, x, X, lane, steps, eg);
        int t = r.i;
        r.i = r.j;
        r.j = t;
        t = l.i;
        l.i = l.j;
        l.j = t;
    }
}

// Shared searches: one directed search of a candidate on one wave, in the
// forward search's coordinates (query = the lower sample, which is also the
// first role of spec 4b). The search's seeds (dbit) are taken in ITS order
// -- forward: (x, y); reverse: (y, x) on the plus strand, (y + len, x + len)
// descending on the minus strand -- by selection: the next seed extended is
// the first in that order outside every box so far (a seed inside a box
// stays inside as boxes are added, so this is the sequential rule of spec 3).
template <bool AMB, typename PT>
__device__ __forceinline__ void process_search(const uint32_t *QO, const uint32_t *QOM, PT qo, const uint32_t *TF,
                                               const uint32_t *TFM, PT tf, int Lq, int Lt, const GSeed *sd, int ns,
                                               int X, int lane, uint32_t dbit, int strand, int &bqa, int &bqb,
                                               int &bsa, int &bsb, int &bsc, int &bd, int &bg, int &bo, int &bni,
                                               int &nh, uint32_t &steps, uint32_t &exts, uint32_t &edges,
                                               uint32_t &capped, bool swap, const int *fx = nullptr, int e = -1)
{
    nh = 0;
    if (fx) {
        // the search's first seed (always extended, spec 3) was extended by
        // the row kernel: its HSP as first_finish_kernel builds it
        constexpr int OBIT = 13, GMASK = 8191;
        const GSeed s0 = sd[e];
        const int x = (int)s0.x, y = (int)s0.y, len = (int)(s0.len & SEED_LEN);
        const int rsc = fx[FX_R], ri = fx[FX_R + 1], rj = fx[FX_R + 2], rd = fx[FX_R + 3], rgo = fx[FX_R + 4];
        const int lsc = fx[FX_L], lI = fx[FX_L + 1], lJ = fx[FX_L + 2], ld = fx[FX_L + 3], lgo = fx[FX_L + 4];
        if (lane == 0) {
            bqa = x - lI; bqb = x + len + ri; bsa = y - lJ; bsb = y + len + rj;
            bsc = lsc + 2 * len + rsc;
            bd = ld + rd; bg = (lgo & GMASK) + (rgo & GMASK); bo = ((lgo >> OBIT) & GMASK) + ((rgo >> OBIT) & GMASK);
            bni = len + (lI + lJ - 2 * ld + (lgo & GMASK)) / 2 + (ri + rj - 2 * rd + (rgo & GMASK)) / 2;
        }
        nh = 1;
    }
    for (;;) {
        unsigned long long bk = ~0ull;
        int bi = 0;
        for (int c0 = 0; c0 < ns; c0 += 64) {
            const int i = c0 + lane;
            if (i >= ns) continue;
            const GSeed g = sd[i];
            if (!(g.len & dbit)) continue;
            const uint32_t x = g.x, y = g.y, len = g.len & SEED_LEN;
            bool in = false;
            for (int h = 0; h < nh; h++) {
                const int qa = __builtin_amdgcn_readlane(bqa, h), qb = __builtin_amdgcn_readlane(bqb, h);
                const int sa = __builtin_amdgcn_readlane(bsa, h), sb = __builtin_amdgcn_readlane(bsb, h);
                in = in || (qa <= (int)x && (int)(x + len) <= qb && sa <= (int)y && (int)(y + len) <= sb);
            }
            if (in) continue;
            const unsigned long long key =
                dbit == SEED_F ? ((unsigned long long)x << 32) | y
                               : (strand ? ((unsigned long long)(uint32_t)~(y + len) << 32) | (uint32_t)~(x + len)
                                         : ((unsigned long long)y << 32) | x);
            if (key < bk) {
                bk = key;
                bi = i;
            }
        }
        unsigned long long m = bk;
        for (int o = 32; o; o >>= 1) {
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(m >> 32), o);
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)m, o);
            const unsigned long long v = ((unsigned long long)hi << 32) | lo;
            m = v < m ? v : m;
        }
        if (m == ~0ull) break;
        if (nh >= MAX_HSP) {   // MAX_HSP binds (spec 3): a seed outside every box remains
            capped++;
            break;
        }
        const int src = __ffsll((unsigned long long)__ballot(bk == m)) - 1;
        const int si = __shfl(bi, src);
        const GSeed g = sd[si];
        const int x = (int)g.x, y = (int)g.y, len = (int)(g.len & SEED_LEN);
        uint32_t eg = 0;
        ExtRes r, l;
        extend_seed<AMB, PT>(QO, QOM, qo, TF, TFM, tf, Lq, Lt, x, y, len, X, lane, steps, eg, swap, r, l);
        exts += 2;
        edges += eg;
        if (lane == nh) {
            bqa = x - l.i; bqb = x + len + r.i; bsa = y - l.j; bsb = y + len + r.j;
            bsc = l.score + 2 * len + r.score;
            bd = l.d + r.d; bg = l.g + r.g; bo = l.o + r.o;
            bni = len + (l.i + l.j - 2 * l.d + l.g) / 2 + (r.i + r.j - 2 * r.d + r.g) / 2;
        }
        nh++;
    }
}

// One candidate (all its seeds) on one wave. QO: oriented query (its base u at
// qo + u), TF: subject forward (base v at tf + v); right extensions walk
// forward from the seed end, left extensions backwards from the seed start.
template <bool AMB, typename PT>
__device__ __forceinline__ void process_candidate(const uint32_t *QO, const uint32_t *QOM, PT qo, const uint32_t *TF,
                                                  const uint32_t *TFM, PT tf, int Lq, int Lt, const GSeed *sd,
                                                  int ns, int X, int lane, int &bqa, int &bqb, int &bsa, int &bsb,
                                                  int &bsc, int &bd, int &bg, int &bo, int &bni, int &nh,
                                                  uint32_t &steps, uint32_t &exts, uint32_t &edges, uint32_t &capped,
                                                  bool swap)
{
    nh = 0;
    int next = ns;   // the first seed not examined (MAX_HSP reached before it)
    for (int c0 = 0; c0 < ns && next == ns; c0 += 64) {
        // lane i holds seed c0 + i; the loop broadcasts them with readlane
        int sx = 0, sy = 0, sl = 0;
        if (c0 + lane < ns) {
            const GSeed g = sd[c0 + lane];
            sx = (int)g.x;
            sy = (int)g.y;
            sl = (int)(g.len & SEED_LEN);
        }
        const int nc = min(ns - c0, 64);
        for (int si = 0; si < nc; si++) {
            if (nh >= MAX_HSP) {
                next = c0 + si;
                break;
            }
            const int x = __builtin_amdgcn_readlane(sx, si), y = __builtin_amdgcn_readlane(sy, si);
            const int len = __builtin_amdgcn_readlane(sl, si);
            const bool inside = lane < nh && bqa <= x && x + len <= bqb && bsa <= y && y + len <= bsb;
            if (__ballot(inside)) continue;
            uint32_t eg = 0;
            ExtRes r, l;
            extend_seed<AMB, PT>(QO, QOM, qo, TF, TFM, tf, Lq, Lt, x, y, len, X, lane, steps, eg, swap, r, l);
            exts += 2;
            edges += eg;
            if (lane == nh) {
                bqa = x - l.i; bqb = x + len + r.i; bsa = y - l.j; bsb = y + len + r.j;
                bsc = l.score + 2 * len + r.score;
                bd = l.d + r.d; bg = l.g + r.g; bo = l.o + r.o;
                bni = len + (l.i + l.j - 2 * l.d + l.g) / 2 + (r.i + r.j - 2 * r.d + r.g) / 2;
            }
            nh++;
        }
    }
    // MAX_HSP binds (spec 3) when a seed past the cap lies outside every box
    for (int i = next; i < ns; i++) {
        const GSeed g = sd[i];
        const int x = (int)g.x, y = (int)g.y, len = (int)(g.len & SEED_LEN);
        if (!__ballot(lane < nh && bqa <= x && x + len <= bqb && bsa <= y && y + len <= bsb)) {
            capped++;
            break;
        }
    }
}

constexpr int SPAD = 32;                               // front pad of staged sequences (bases)
constexpr int SW2 = (STAGE_BASES + SPAD) / 32 + 3;     // u64 words per staged sequence

// stage bases [pos, pos + L) of a packed global array at LDS base SPAD
__device__ __forceinline__ void stage_seq(uint64_t *dst, const uint64_t *src, uint64_t pos, int L, int lane)
{
    const int nw = (L >> 5) + 3;
    for (int w = lane; w < nw; w += 64) dst[w] = w ? win<uint64_t>(src, pos + 32 * (uint64_t)(w - 1)) : 0ull;
}

template <bool AMB>
__global__ __launch_bounds__(EBLOCK, EXT_MIN_WAVES) void extend_kernel(Db db, ExtParams P)
{
    constexpr int NA = AMB ? 4 : 2;
    __shared__ uint64_t stg[EWAVES][NA][SW2];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t total = db.total;
    const uint64_t nwaves = (uint64_t)gridDim.x * EWAVES;
    uint64_t li = (uint64_t)blockIdx.x * EWAVES + wid;
    // the searches the row kernels and first_finish_kernel (or the later-seed
    // rounds) left: candidate slots P.defer[0, *P.defer_count)
    const uint64_t n_work = (uint64_t)*P.defer_count;
    // candidate slots are wave-uniform: keep them (and what is loaded through
    // them) in scalar registers
    auto locate = [&](uint64_t l) -> uint64_t { return rfl((uint64_t)P.defer[l]); };
    const Cand *__restrict__ cands = P.cands;
    const TxInfo *__restrict__ txs = db.tx;
    uint32_t steps = 0, exts = 0, ncands = 0, edges = 0, capped = 0;
    for (; li < n_work; li += nwaves) {
        const uint64_t ci = locate(li);
        const Cand cd = cands[ci];
        const TxInfo qt = txs[cd.q_gtx], st = txs[cd.s_gtx];
        const int Lq = (int)qt.len, Lt = (int)st.len;
        const int strand = cd.strand;
        const int ns = (int)cand_seeds(cd);
        const GSeed *sd = P.seeds + cd.seed_off;
        ncands++;
        int bqa = 0, bqb = 0, bsa = 0, bsb = 0, bsc = 0, bd = 0, bg = 0, bo = 0, bni = 0, nh = 0;
        // oriented query: q (forward array) or revcomp(q) (reverse-complement array)
        const uint64_t *QA = strand ? db.RC : db.F;
        const uint64_t *QAM = strand ? db.ARC : db.AF;
        const uint64_t q0 = strand ? total - qt.start - (uint64_t)Lq : qt.start;
        // spec 4b: the lower-numbered sample in the greedy's first role
        const bool swap = qt.sample > st.sample;
        // shared searches: this work item is one directed search of the candidate
        const uint32_t dbit = P.dir ? SEED_R : SEED_F;
        // its first seed's extension from the row kernel, when that finished
        // (a search deferred for a seed outside the first box, not for a
        // sub-band overflow): the search starts with that HSP
        const int *fx0 = nullptr;
        int e0 = -1;
        if (P.share) {
            const bool second = P.dir == 1 && cd.e1 != SEED_NONE;
            const int *fx = (second ? P.cand_box2 : P.cand_box) + ci * BOX_REC;
            if (fx[FX_STATUS] >= 0) {
                fx0 = fx;
                e0 = (int)(second ? cd.e1 : cd.e0);
            }
        }
        if (Lq + SPAD <= STAGE_BASES && Lt + SPAD <= STAGE_BASES) {
            uint64_t *QO = stg[wid][0], *TF = stg[wid][1];
            stage_seq(QO, QA, q0, Lq, lane);
            stage_seq(TF, db.F, st.start, Lt, lane);
            const uint32_t *QOM = nullptr, *TFM = nullptr;
            if (AMB) {
                stage_seq(stg[wid][2], QAM, q0, Lq, lane);
                stage_seq(stg[wid][3], db.AF, st.start, Lt, lane);
                QOM = reinterpret_cast<const uint32_t *>(stg[wid][2]);
                TFM = reinterpret_cast<const uint32_t *>(stg[wid][3]);
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            if (P.share)
                process_search<AMB, uint32_t>(reinterpret_cast<const uint32_t *>(QO), QOM, (uint32_t)SPAD,
                                              reinterpret_cast<const uint32_t *>(TF), TFM, (uint32_t)SPAD, Lq, Lt,
                                              sd, ns, P.xdrop, lane, dbit, strand, bqa, bqb, bsa, bsb, bsc, bd, bg,
                                              bo, bni, nh, steps, exts, edges, capped, swap, fx0, e0);
            else
                process_candidate<AMB, uint32_t>(reinterpret_cast<const uint32_t *>(QO), QOM, (uint32_t)SPAD,
                                                 reinterpret_cast<const uint32_t *>(TF), TFM, (uint32_t)SPAD, Lq, Lt,
                                                 sd, ns, P.xdrop, lane, bqa, bqb, bsa, bsb, bsc, bd, bg, bo, bni, nh,
                                                 steps, exts, edges, capped, swap);
        } else if (P.share) {
            process_search<AMB, int64_t>(reinterpret_cast<const uint32_t *>(QA),
                                         reinterpret_cast<const uint32_t *>(QAM), (int64_t)q0,
                                         reinterpret_cast<const uint32_t *>(db.F),
                                         reinterpret_cast<const uint32_t *>(db.AF), (int64_t)st.start, Lq, Lt, sd,
                                         ns, P.xdrop, lane, dbit, strand, bqa, bqb, bsa, bsb, bsc, bd, bg, bo, bni,
                                         nh, steps, exts, edges, capped, swap, fx0, e0);
        } else {
            // global arrays carry two zero words in front, so backward windows
            // of the first transcript stay in bounds (positions may go to -32)
            process_candidate<AMB, int64_t>(reinterpret_cast<const uint32_t *>(QA),
                                            reinterpret_cast<const uint32_t *>(QAM), (int64_t)q0,
                                            reinterpret_cast<const uint32_t *>(db.F),
                                            reinterpret_cast<const uint32_t *>(db.AF), (int64_t)st.start, Lq, Lt,
                                            sd, ns, P.xdrop, lane, bqa, bqb, bsa, bsb, bsc, bd, bg, bo, bni, nh,
                                            steps, exts, edges, capped, swap);
        }
        // purge HSPs with common endpoints: by (score desc, index asc)
        int rank = 0;
        for (int j = 0; j < nh; j++) {
            const int sj = __builtin_amdgcn_readlane(bsc, j);
            if (lane < nh && (sj > bsc || (sj == bsc && j < lane))) rank++;
        }
        bool kept = false;
        for (int rr = 0; rr < nh; rr++) {
            const uint64_t m = __ballot(lane < nh && rank == rr);
            const int i = __ffsll((unsigned long long)m) - 1;
            const int qa = __builtin_amdgcn_readlane(bqa, i), sa = __builtin_amdgcn_readlane(bsa, i);
            const int qb = __builtin_amdgcn_readlane(bqb, i), sb2 = __builtin_amdgcn_readlane(bsb, i);
            const bool conflict = kept && lane < nh && ((bqa == qa && bsa == sa) || (bqb == qb && bsb == sb2));
            if (!__ballot(conflict) && lane == i) kept = true;
        }
        // e-value cut of each direction: query->subject (query length, subject
        // DB) and the mirrored one (subject length, query sample's DB)
        const int thr_f = P.thr[(size_t)st.sample * (size_t)(P.max_len + 1) + (size_t)Lq];
        const int thr_r = P.thr[(size_t)qt.sample * (size_t)(P.max_len + 1) + (size_t)Lt];
        // shared searches: the forward item applies the forward cut, the
        // reverse item the reverse one (its records go to the _r arrays)
        const bool pf = (!P.share || !P.dir) && bsc >= thr_f, pr = (P.sym || (P.share && P.dir)) && bsc >= thr_r;
        const bool out = kept && (pf || pr);
        const uint64_t om = __ballot(out);
        const int nout = __popcll(om);
        uint32_t obase = 0;
        if (nout > 1 && lane == 0) {
            const unsigned long long b = atomicAdd(P.ovf_count, (unsigned long long)(nout - 1));
            if (b + (nout - 1) > P.ovf_cap) atomicOr(P.status, ST_OVERFLOW);
            obase = (uint32_t)b;
        }
        obase = __builtin_amdgcn_readlane(obase, 0);
        if (out) {
            const int rk = __popcll(om & ((1ull << lane) - 1ull));
            DHsp h;
            h.q_tx = cd.q_gtx;
            h.s_tx = cd.s_gtx;
            if (!strand) {
                h.qstart = bqa + 1; h.qend = bqb; h.sstart = bsa + 1; h.send = bsb;
            } else {
                h.qstart = Lq - bqb + 1; h.qend = Lq - bqa; h.sstart = bsb; h.send = bsa + 1;
            }
            h.gaps = bg;
            h.gapopen = bo;
            h.mismatch = bd - bg;
            h.nident = bni;
            h.length = bni + (bd - bg) + bg;
            h.score_half = bsc;
            h.bits10 = P.bits10[bsc];
            h.strand = strand | (pf ? HSP_FWD : 0) | (pr ? HSP_REV : 0) | (lane << HSP_IDX_SHIFT);
            if (rk == 0) (P.share && P.dir ? P.cand_hsp_r : P.cand_hsp)[ci] = h;
            else if ((uint64_t)obase + (rk - 1) < P.ovf_cap) P.ovf[obase + rk - 1] = h;
        }
        if (lane == 0) {
            (P.share && P.dir ? P.cand_nh_r : P.cand_nh)[ci] = (uint8_t)nout;
            (P.share && P.dir ? P.cand_ovf_r : P.cand_ovf)[ci] = obase;
        }
    }
    if (lane == 0 && P.counters) {
        atomicAdd(&P.counters[DC_STEPS - DC_COUNTERS], (unsigned long long)steps);
        atomicAdd(&P.counters[DC_EXTS - DC_COUNTERS], (unsigned long long)exts);
        atomicAdd(&P.counters[DC_CANDS - DC_COUNTERS], (unsigned long long)ncands);
        if (edges) atomicAdd(&P.counters[DC_BAND_BOUND - DC_COUNTERS], (unsigned long long)edges);
        if (capped) atomicAdd(&P.counters[DC_MAXHSP - DC_COUNTERS], (unsigned long long)capped);
    }
}

// extend_kernel over the searches the row kernels left (B.defer, and for
// shared searches the reverse ones, B.defer_r)
static void extend_lists(bool amb, const Db &db, const ExtParams &B, hipStream_t st)
{
    for (int dir = 0; dir < (B.share ? 2 : 1); dir++) {
        ExtParams W3 = B;
        W3.dir = dir;
        if (dir) {
            W3.defer = B.defer_r;
            W3.defer_count = B.defer_r_count;
        }
        if (amb) {
            auto kern = extend_kernel<true>;
            hipLaunchKernelGGL(kern, dim3(resident_blocks(kern, 0)), dim3(EBLOCK), 0, st, db, W3);
        } else {
            auto kern = extend_kernel<false>;
            hipLaunchKernelGGL(kern, dim3(resident_blocks(kern, 0)), dim3(EBLOCK), 0, st, db, W3);
        }
    }
}

// The extend_kernel launches over the searches launch_extend_rows deferred
// (sub-band overflow, seeds outside the first box; without the windowed
// kernel transcripts longer than the row staging slot): after it, or again
// after the HSP overflow buffer overflowed (only extend_kernel writes it; the
// row kernels' results, first_finish_kernel's and the defer lists stand).
// The deferred counts stay on the device: the list launches read them.
void launch_extend_retry(bool amb, const Db &db, const ExtParams &P, hipStream_t st)
{
    if (P.n_cand == 0) return;
    ExtParams W = P;
    W.list = nullptr;
    W.list_n = nullptr;
    W.resume = nullptr;
    extend_lists(amb, db, W, st);
}

}  // namespace rcg
