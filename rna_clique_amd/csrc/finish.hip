// What follows the row kernels of the extension, one thread per candidate or
// search (the pass order: align.hip):
//
//   first_finish_kernel  one thread per candidate: a search whose seeds all
//                        lie in the first seed's box is done (cuts, record).
//   later_round_kernel   the other searches, one seed per round: the next
//   later_finish_kernel  seed outside every box goes to the 64-lane rows;
//                        then purge and cuts, one thread per search.
//
// Host entry points: launch_first_finish, launch_later_round,
// launch_later_finish.
//
// Semantics: oracle/align_oracle.c ("RC-megablast v1"), bit for bit.
#include "device.h"
#include "launch.h"

#include <algorithm>
#include <climits>

namespace rcg {

// The candidates' first-seed extensions -> box; the other seeds of the
// candidate are checked against it (spec 3: a seed inside a found HSP box is
// not extended). All inside: the candidate has this one HSP -- e-value cuts of
// both directions, HSP record. Otherwise extend_kernel redoes the candidate
// whole (the defer list it runs next). One thread per candidate.
__global__ __launch_bounds__(256) void first_finish_kernel(ExtParams P)
{
    constexpr int OBIT = 13, GMASK = 8191;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < P.n_cand;
         li += (uint64_t)gridDim.x * blockDim.x) {
        int lo = 0, hi = NSHARD;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (P.shard_prefix[mid] <= li) lo = mid; else hi = mid;
        }
        const uint64_t ci = (uint64_t)lo * P.cand_cap + (li - P.shard_prefix[lo]);
        if (!P.share && P.cand_box[ci * BOX_REC + FX_STATUS] < 0) continue;   // deferred by the row kernel
        const Cand cd = P.cands[ci];
        // shared searches: each directed search of the candidate on its own --
        // its first seed's box (cand_box, or cand_box2 when the reverse
        // search's first seed is another seed), its own seeds, its own cut.
        // Both searches' containment tests share one pass over the seeds.
        const int ndir = P.share ? 2 : 1;
        bool live[2] = {false, false};
        int bqa[2] = {0, 0}, bqb[2] = {0, 0}, bsa[2] = {0, 0}, bsb[2] = {0, 0}, ex[2] = {-1, -1};
        const int *fxd[2] = {nullptr, nullptr};
        // each live search's HSP fields from its box, computed (and the bit
        // score and cut loads issued) before the pass over the seeds, so that
        // they are not round trips of their own after it
        int bsc[2] = {0, 0}, bd[2] = {0, 0}, bg[2] = {0, 0}, bo[2] = {0, 0}, bni[2] = {0, 0}, b10[2] = {0, 0};
        const int thr_f = P.thr[(size_t)cd.ssam * (size_t)(P.max_len + 1) + (size_t)cd.Lq];
        const int thr_r = P.thr[(size_t)cd.qsam * (size_t)(P.max_len + 1) + (size_t)cd.Lt];
        for (int dir = 0; dir < ndir; dir++) {
            if (P.share && !((cd.dflags >> dir) & 1)) {   // this search found no seed here
                (dir ? P.cand_nh_r : P.cand_nh)[ci] = 0;
                (dir ? P.cand_ovf_r : P.cand_ovf)[ci] = 0;
                continue;
            }
            const bool second = dir == 1 && cd.e1 != SEED_NONE;
            fxd[dir] = (second ? P.cand_box2 : P.cand_box) + ci * BOX_REC;
            if (fxd[dir][FX_STATUS] < 0) {   // (shared searches) the row kernel gave it up
                if (P.why) atomicAdd(&P.why[1], 1ull);
                const unsigned long long di = atomicAdd(dir ? P.defer_r_count : P.defer_count, 1ull);
                (dir ? P.defer_r : P.defer)[di] = (uint32_t)ci;
                continue;
            }
            ex[dir] = (int)(second ? cd.e1 : cd.e0);
            const GSeed s0 = P.seeds[cd.seed_off + ex[dir]];
            const int *fx = fxd[dir];
            const int x = (int)s0.x, y = (int)s0.y, len = (int)(s0.len & SEED_LEN);
            bqa[dir] = x - fx[FX_L + 1];
            bqb[dir] = x + len + fx[FX_R + 1];
            bsa[dir] = y - fx[FX_L + 2];
            bsb[dir] = y + len + fx[FX_R + 2];
            live[dir] = true;
            const int rsc = fx[FX_R], ri = fx[FX_R + 1], rj = fx[FX_R + 2], rd = fx[FX_R + 3], rgo = fx[FX_R + 4];
            const int lsc = fx[FX_L], lI = fx[FX_L + 1], lJ = fx[FX_L + 2], ld = fx[FX_L + 3], lgo = fx[FX_L + 4];
            const int lg = lgo & GMASK, lo2 = (lgo >> OBIT) & GMASK, rg = rgo & GMASK, ro = (rgo >> OBIT) & GMASK;
            bsc[dir] = lsc + 2 * len + rsc;
            bd[dir] = ld + rd;
            bg[dir] = lg + rg;
            bo[dir] = lo2 + ro;
            bni[dir] = len + (lI + lJ - 2 * ld + lg) / 2 + (ri + rj - 2 * rd + rg) / 2;
            b10[dir] = P.bits10[bsc[dir]];
        }
        // the other seeds of each live search inside its box? (four seeds'
        // loads in flight at a time)
        bool in0 = live[0], in1 = live[1];
        const GSeed *const sp = P.seeds + cd.seed_off;
        const uint32_t ns = cand_seeds(cd);
        for (uint32_t i0 = 0; i0 < ns && (in0 || in1); i0 += 4) {
            GSeed s4[4];
#pragma unroll
            for (int k = 0; k < 4; k++) s4[k] = i0 + k < ns ? sp[i0 + k] : GSeed{0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i = (int)(i0 + k);
                if (i >= (int)ns) break;
                const int sl = (int)(s4[k].len & SEED_LEN), sx = (int)s4[k].x, sy = (int)s4[k].y;
                // without shared searches every seed is the one search's
                const bool f = !P.share || (s4[k].len & SEED_F), r = P.share && (s4[k].len & SEED_R);
                if (in0 && f && i != ex[0])
                    in0 = bqa[0] <= sx && sx + sl <= bqb[0] && bsa[0] <= sy && sy + sl <= bsb[0];
                if (in1 && r && i != ex[1])
                    in1 = bqa[1] <= sx && sx + sl <= bqb[1] && bsa[1] <= sy && sy + sl <= bsb[1];
            }
        }
        for (int dir = 0; dir < ndir; dir++) {
            if (!live[dir]) continue;
            DHsp *const hsp_out = dir ? P.cand_hsp_r : P.cand_hsp;
            uint8_t *const nh_out = dir ? P.cand_nh_r : P.cand_nh;
            uint32_t *const ovf_out = dir ? P.cand_ovf_r : P.cand_ovf;
            if (!(dir ? in1 : in0)) {
                if (P.why) atomicAdd(&P.why[2], 1ull);
                const unsigned long long di = atomicAdd(dir ? P.defer_r_count : P.defer_count, 1ull);
                (dir ? P.defer_r : P.defer)[di] = (uint32_t)ci;
                continue;
            }
            const bool pf = (!P.share || dir == 0) && bsc[dir] >= thr_f;
            const bool pr = (P.sym || (P.share && dir == 1)) && bsc[dir] >= thr_r;
            if (pf || pr) {
                DHsp h;
                h.q_tx = cd.q_gtx;
                h.s_tx = cd.s_gtx;
                if (!cd.strand) {
                    h.qstart = bqa[dir] + 1; h.qend = bqb[dir]; h.sstart = bsa[dir] + 1; h.send = bsb[dir];
                } else {
                    h.qstart = cd.Lq - bqb[dir] + 1; h.qend = cd.Lq - bqa[dir];
                    h.sstart = bsb[dir]; h.send = bsa[dir] + 1;
                }
                h.gaps = bg[dir];
                h.gapopen = bo[dir];
                h.mismatch = bd[dir] - bg[dir];
                h.nident = bni[dir];
                h.length = bni[dir] + bd[dir];
                h.score_half = bsc[dir];
                h.bits10 = b10[dir];
                h.strand = cd.strand | (pf ? HSP_FWD : 0) | (pr ? HSP_REV : 0);
                hsp_out[ci] = h;
            }
            nh_out[ci] = (uint8_t)((pf || pr) ? 1 : 0);
            ovf_out[ci] = 0;
        }
    }
}

// HSP box of a seed (x, y, len) from its row-kernel results (cand_box
// record): what process_search builds from extend_seed's two results
__device__ __forceinline__ void box_from_fx(const int *fx, int x, int y, int len, int *b)
{
    constexpr int OBIT = 13, GMASK = 8191;
    const int rsc = fx[FX_R], ri = fx[FX_R + 1], rj = fx[FX_R + 2], rd = fx[FX_R + 3], rgo = fx[FX_R + 4];
    const int lsc = fx[FX_L], lI = fx[FX_L + 1], lJ = fx[FX_L + 2], ld = fx[FX_L + 3], lgo = fx[FX_L + 4];
    const int lg = lgo & GMASK, lo = (lgo >> OBIT) & GMASK, rg = rgo & GMASK, ro = (rgo >> OBIT) & GMASK;
    b[LB_QA] = x - lI;
    b[LB_QB] = x + len + ri;
    b[LB_SA] = y - lJ;
    b[LB_SB] = y + len + rj;
    b[LB_SC] = lsc + 2 * len + rsc;
    b[LB_D] = ld + rd;
    b[LB_G] = lg + rg;
    b[LB_O] = lo + ro;
    b[LB_NI] = len + (lI + lJ - 2 * ld + lg) / 2 + (ri + rj - 2 * rd + rg) / 2;
}

// A search the later-seed rounds cannot take: extend_kernel runs it whole
// (from its first seed's HSP)
__device__ __forceinline__ void later_full(const LaterParams &L, int dir, uint64_t ci)
{
    const unsigned long long i = atomicAdd(&L.full_n[dir], 1ull);
    (dir ? L.full1 : L.full0)[i] = (uint32_t)ci;
    if (L.counters) atomicAdd(&L.counters[LC_WHOLE], 1ull);
}

// One round of the later-seed rounds, one thread per active search: take the
// result of the seed the previous round extended (round 0: the first seed's,
// from cand_box / cand_box2) as the search's next HSP, then pick the next seed
// as process_search does -- the first in the search's order outside every box
// so far -- and list it for the row kernels as a candidate record whose e0 is
// that seed. A search with no such seed is finished; one at MAX_HSP HSPs with
// such a seed is finished and MAX_HSP-bound (spec 3).
__device__ __forceinline__ bool later_step(const ExtParams &P, const LaterParams &L, uint64_t s, uint32_t &bi_out)
{
    const int dir = s >= L.n0 ? 1 : 0;
    const uint64_t ci = dir ? L.defer1[s - L.n0] : L.defer0[s];
    if (s >= L.n_cap) {   // (round 0 only: past the states' capacity)
        later_full(L, dir, ci);
        return false;
    }
    int *const st = L.state + s * LATER_REC;
    const Cand cd = P.cands[ci];
    const GSeed *const sd = P.seeds + cd.seed_off;
    int nh;
    uint32_t last;   // the seed extended last
    if (L.round == 0) {
        const bool second = dir == 1 && cd.e1 != SEED_NONE;
        const int *fx = (second ? P.cand_box2 : P.cand_box) + ci * BOX_REC;
        st[LS_CAPPED] = 0;
        st[LS_PEND] = -1;
        if (fx[FX_STATUS] < 0) {   // the row kernels gave its first seed up
            st[LS_STATE] = LATER_FULL;
            later_full(L, dir, ci);
            return false;
        }
        last = second ? cd.e1 : cd.e0;
        const GSeed g = sd[last];
        box_from_fx(fx, (int)g.x, (int)g.y, (int)(g.len & SEED_LEN), st + LS_BOX);
        nh = 1;
    } else {
        nh = st[LS_STATE];
        const int w = st[LS_PEND];
        const int *fx = L.box_in + (size_t)w * BOX_REC;
        if (fx[FX_STATUS] < 0) {   // the row kernels gave this seed up
            st[LS_STATE] = LATER_FULL;
            later_full(L, dir, ci);
            return false;
        }
        last = L.vc_in[w].e0;
        const GSeed g = sd[last];
        box_from_fx(fx, (int)g.x, (int)g.y, (int)(g.len & SEED_LEN), st + LS_BOX + nh * LB_N);
        nh++;
    }
    // the next seed: the search's own seeds, in its order, outside every box
    // (the boxes in registers; an unused one is empty)
    int qa[MAX_HSP], qb[MAX_HSP], sa[MAX_HSP], sb[MAX_HSP];
#pragma unroll
    for (int h = 0; h < MAX_HSP; h++) {
        const int *b = st + LS_BOX + h * LB_N;
        const bool u = h < nh;
        qa[h] = u ? b[LB_QA] : INT_MAX;
        qb[h] = u ? b[LB_QB] : INT_MIN;
        sa[h] = u ? b[LB_SA] : INT_MAX;
        sb[h] = u ? b[LB_SB] : INT_MIN;
    }
    const uint32_t dbit = dir ? SEED_R : SEED_F;
    const uint32_t ns = cand_seeds(cd);
    unsigned long long bk = ~0ull;
    uint32_t bi = 0;
    // the forward search's order is the seeds' (x, y) order: the seeds before
    // the last one extended were inside a box when it was picked, and boxes
    // only grow, so they still are (the reverse order is another permutation)
    for (uint32_t i = dir ? 0u : last + 1u; i < ns; i++) {
        const GSeed g = sd[i];
        if (!(g.len & dbit)) continue;
        const int x = (int)g.x, y = (int)g.y, len = (int)(g.len & SEED_LEN);
        bool in = false;
#pragma unroll
        for (int h = 0; h < MAX_HSP; h++)
            in = in || (qa[h] <= x && x + len <= qb[h] && sa[h] <= y && y + len <= sb[h]);
        if (in) continue;
        const unsigned long long key =
            !dir ? ((unsigned long long)g.x << 32) | g.y
                 : (cd.strand ? ((unsigned long long)(uint32_t)~(g.y + (uint32_t)len) << 32) |
                                    (uint32_t)~(g.x + (uint32_t)len)
                              : ((unsigned long long)g.y << 32) | g.x);
        if (key < bk) {
            bk = key;
            bi = i;
        }
    }
    st[LS_STATE] = nh;
    if (bk == ~0ull) return false;   // every seed inside a box: finished
    if (nh >= MAX_HSP) {             // MAX_HSP binds
        st[LS_CAPPED] = 1;
        return false;
    }
    if (bi >= SEED_NONE) {           // past the record's 16-bit seed field
        st[LS_STATE] = LATER_FULL;
        later_full(L, dir, ci);
        return false;
    }
    bi_out = bi;   // (its record goes out once the wave has its work slots)
    return true;
}

__global__ __launch_bounds__(256) void later_round_kernel(ExtParams P, LaterParams L)
{
    const uint64_t n = L.round == 0 ? L.n_search : (uint64_t)*L.act_in_n;
    const int lane = threadIdx.x & 63;
    // whole waves iterate together (the work slots are allocated per wave)
    for (uint64_t b0 = blockIdx.x * (uint64_t)blockDim.x; b0 < n; b0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t li = b0 + threadIdx.x;
        uint64_t s = 0;
        uint32_t bi = 0;
        bool emit = false;
        if (li < n) {
            s = L.round == 0 ? li : (uint64_t)L.act_in[li];
            emit = later_step(P, L, s, bi);
        }
        const uint64_t m = __ballot(emit);
        if (!m) continue;
        const int cnt = __popcll(m);
        const int leader = __ffsll((unsigned long long)m) - 1;
        unsigned long long wb = 0, ab = 0;
        if (lane == leader) {
            wb = atomicAdd(L.work_n, (unsigned long long)cnt);
            ab = atomicAdd(L.act_out_n, (unsigned long long)cnt);
        }
        wb = (unsigned long long)__shfl((long long)wb, leader);
        ab = (unsigned long long)__shfl((long long)ab, leader);
        if (emit) {
            const int rk = __popcll(m & ((1ull << lane) - 1ull));
            const uint64_t w = wb + rk;
            const int dir = s >= L.n0 ? 1 : 0;
            const uint64_t ci = dir ? L.defer1[s - L.n0] : L.defer0[s];
            Cand v = P.cands[ci];
            v.e0 = (uint16_t)bi;
            v.e1 = SEED_NONE;
            L.vc[w] = v;
            L.list[w] = (uint32_t)w;
            L.state[s * LATER_REC + LS_PEND] = (int)w;
            L.act_out[ab + rk] = (uint32_t)s;
        }
    }
}

// The searches the rounds finished, one thread each: extend_kernel's end of a
// search -- purge of HSPs with a common end point, by (score desc, index
// asc), then the direction's e-value cut -- and its records: the first in
// cand_hsp (_r), the others in the overflow buffer (one atomic per wave).
__global__ __launch_bounds__(256) void later_finish_kernel(ExtParams P, LaterParams L)
{
    const uint64_t n = L.n_search < L.n_cap ? L.n_search : L.n_cap;
    const int lane = threadIdx.x & 63;
    for (uint64_t b0 = blockIdx.x * (uint64_t)blockDim.x; b0 < n; b0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s = b0 + threadIdx.x;
        const int *const st = L.state + s * LATER_REC;
        const int nh = s < n ? st[LS_STATE] : -1;
        const bool live = nh >= 0;
        const int dir = s >= L.n0 ? 1 : 0;
        uint64_t ci = 0;
        Cand cd{};
        int qa[MAX_HSP], qb[MAX_HSP], sa[MAX_HSP], sb[MAX_HSP], sc[MAX_HSP];
        uint32_t outm = 0, pfm = 0, prm = 0;
        bool capped = false;
        if (live) {
            ci = dir ? L.defer1[s - L.n0] : L.defer0[s];
            cd = P.cands[ci];
            capped = st[LS_CAPPED] != 0;
#pragma unroll
            for (int h = 0; h < MAX_HSP; h++) {
                const int *b = st + LS_BOX + h * LB_N;
                const bool u = h < nh;
                qa[h] = u ? b[LB_QA] : 0;
                qb[h] = u ? b[LB_QB] : 0;
                sa[h] = u ? b[LB_SA] : 0;
                sb[h] = u ? b[LB_SB] : 0;
                sc[h] = u ? b[LB_SC] : INT_MIN;
            }
            // purge: in (score desc, index asc) order, an HSP sharing its start
            // or its end point with one kept before it goes
            uint32_t kept = 0, done = 0;
            for (int rr = 0; rr < nh; rr++) {
                int i = -1, bs = INT_MIN;
#pragma unroll
                for (int h = 0; h < MAX_HSP; h++)
                    if (h < nh && !((done >> h) & 1u) && (i < 0 || sc[h] > bs)) {
                        i = h;
                        bs = sc[h];
                    }
                done |= 1u << i;
                bool conflict = false;
#pragma unroll
                for (int h = 0; h < MAX_HSP; h++)
                    conflict = conflict || (((kept >> h) & 1u) && ((qa[h] == qa[i] && sa[h] == sa[i]) ||
                                                                   (qb[h] == qb[i] && sb[h] == sb[i])));
                if (!conflict) kept |= 1u << i;
            }
            const int thr_f = P.thr[(size_t)cd.ssam * (size_t)(P.max_len + 1) + (size_t)cd.Lq];
            const int thr_r = P.thr[(size_t)cd.qsam * (size_t)(P.max_len + 1) + (size_t)cd.Lt];
#pragma unroll
            for (int h = 0; h < MAX_HSP; h++) {
                const bool pf = (!P.share || !dir) && sc[h] >= thr_f;
                const bool pr = (P.sym || (P.share && dir)) && sc[h] >= thr_r;
                if (((kept >> h) & 1u) && (pf || pr)) {
                    outm |= 1u << h;
                    pfm |= (pf ? 1u : 0u) << h;
                    prm |= (pr ? 1u : 0u) << h;
                }
            }
        }
        // overflow slots of HSPs 2.. of the wave's searches: one atomic
        const int nout = __popc(outm);
        const uint32_t need = nout > 1 ? (uint32_t)(nout - 1) : 0u;
        uint32_t incl = need;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
            if (lane >= o) incl += v;
        }
        const uint32_t tot = (uint32_t)__shfl((int)incl, 63);
        unsigned long long wb = 0;
        if (lane == 63 && tot) {
            wb = atomicAdd(P.ovf_count, (unsigned long long)tot);
            if (wb + tot > P.ovf_cap) atomicOr(P.status, ST_OVERFLOW);
        }
        wb = (unsigned long long)__shfl((long long)wb, 63);
        if (P.counters) {
            const uint64_t cm = __ballot(capped);
            if (lane == 0 && cm) atomicAdd(&P.counters[DC_MAXHSP - DC_COUNTERS], (unsigned long long)__popcll(cm));
        }
        if (!live) continue;
        const uint32_t obase = need ? (uint32_t)(wb + incl - need) : 0u;
        DHsp *const hsp_out = dir ? P.cand_hsp_r : P.cand_hsp;
        int rk = 0;
        for (int h = 0; h < nh; h++) {
            if (!((outm >> h) & 1u)) continue;
            const int *b = st + LS_BOX + h * LB_N;
            DHsp o;
            o.q_tx = cd.q_gtx;
            o.s_tx = cd.s_gtx;
            if (!cd.strand) {
                o.qstart = b[LB_QA] + 1; o.qend = b[LB_QB]; o.sstart = b[LB_SA] + 1; o.send = b[LB_SB];
            } else {
                o.qstart = cd.Lq - b[LB_QB] + 1; o.qend = cd.Lq - b[LB_QA]; o.sstart = b[LB_SB]; o.send = b[LB_SA] + 1;
            }
            const int bd = b[LB_D], bg = b[LB_G], bni = b[LB_NI];
            o.gaps = bg;
            o.gapopen = b[LB_O];
            o.mismatch = bd - bg;
            o.nident = bni;
            o.length = bni + (bd - bg) + bg;
            o.score_half = b[LB_SC];
            o.bits10 = P.bits10[b[LB_SC]];
            o.strand = cd.strand | (((pfm >> h) & 1u) ? HSP_FWD : 0) | (((prm >> h) & 1u) ? HSP_REV : 0) |
                       (h << HSP_IDX_SHIFT);
            if (rk == 0) hsp_out[ci] = o;
            else if ((uint64_t)obase + (rk - 1) < P.ovf_cap) P.ovf[obase + rk - 1] = o;
            rk++;
        }
        (dir ? P.cand_nh_r : P.cand_nh)[ci] = (uint8_t)nout;
        (dir ? P.cand_ovf_r : P.cand_ovf)[ci] = obase;
    }
}

// One thread per candidate (the caller has checked P.n_cand != 0)
void launch_first_finish(const ExtParams &P, hipStream_t st)
{
    const uint64_t g = std::min<uint64_t>((P.n_cand + 255) / 256, 65536);
    hipLaunchKernelGGL(first_finish_kernel, dim3((unsigned)g), dim3(256), 0, st, P);
}

// One round of the later seeds, one thread per search (the caller has checked
// L.n_search != 0)
void launch_later_round(const ExtParams &P, const LaterParams &L, hipStream_t st)
{
    const uint64_t g = std::min<uint64_t>((L.n_search + 255) / 256, 8192);
    hipLaunchKernelGGL(later_round_kernel, dim3((unsigned)g), dim3(256), 0, st, P, L);
}

// The searches the later-seed rounds finished: purge, cuts, records (again
// after an HSP overflow-buffer retry: the search states stand)
void launch_later_finish(const ExtParams &P, const LaterParams &L, hipStream_t st)
{
    const uint64_t n = std::min(L.n_search, L.n_cap);
    if (!n) return;
    uint64_t g = (n + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(later_finish_kernel, dim3((unsigned)g), dim3(256), 0, st, P, L);
}

}  // namespace rcg
