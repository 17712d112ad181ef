// Seeds of seed-and-extend (the BLAST+ replacement):
//
//   seed_kernel          one workgroup per query gene: 16-mer lookups at
//                        stride W-15 on both strands of every isoform,
//                        canonical maximal exact runs >= W (seeds), sorted per
//                        candidate (query tx, strand, subject tx); candidates
//                        grouped by subject sample.
//   rs_range_kernel      each query gene's range of the reverse-only seeds.
//
// Host entry points: launch_seed, launch_seed_big, launch_rs_range.
//
// Semantics: oracle/align_oracle.c ("RC-megablast v1"), bit for bit.
#include "device.h"
#include "launch.h"

#include <algorithm>
#include <type_traits>

namespace rcg {

// Threads per query gene (one workgroup) and word items per round of the
// lookup -> hits -> test chain. A C3 gene has ~146 word items, ~176 seeds and
// ~16 candidates: most of 256 lanes idle in every phase, and what a CU can
// hold is workgroups (registers, LDS), so smaller workgroups put more genes'
// dependent chains in flight. Items per round are kept apart from the threads
// (IPT items per thread, their loads in flight together) so that a typical
// gene still takes one round. r19 (profiles/r19_seed_block, C3 seed kernel per
// step, both passes): 256 threads at 5 workgroups per CU 65.8 ms; 128 threads
// with 256 items per round at 8 per CU 56.5 (4 hits per lane 57.9); 128 items
// per round at 8 per CU 58.8, at 10 per CU (96 VGPRs, 4 hits per lane) 57.3;
// 64 threads at 8 per CU (two waves per SIMD) 65.6.
#ifndef RC_SEED_BLOCK
#define RC_SEED_BLOCK 128
#endif
#ifndef RC_SEED_ITEMS
#define RC_SEED_ITEMS 256
#endif
constexpr int SBLOCK = RC_SEED_BLOCK;
constexpr int SITEMS = RC_SEED_ITEMS;
constexpr int IPT = SITEMS / SBLOCK;   // word items per thread per round
static_assert(SBLOCK == 64 || SBLOCK == 128 || SBLOCK == 256, "RC_SEED_BLOCK: whole waves, a power of two (bitonic chunks)");
static_assert(SITEMS % SBLOCK == 0 && SITEMS <= 256, "RC_SEED_ITEMS: a multiple of the block; item slots are 8-bit (hq_k)");
// Seed kernel occupancy (r04, profiles/r04_i, C3 seed kernel per step):
// 1024-seed LDS passes at 4 workgroups per CU 79.5 ms; 512-seed passes at 5
// (96 VGPRs, 28 KB LDS) 70.7; 6 (2 hits per lane) 74.7; 256-seed passes at
// 7 or 8: 92 / 98 (more passes halve their subject range). C3v: 103-104 ms
// at 4 and 5 alike.
// RC_SEED_WAVES and RC_SEED_REV_WAVES are the launch bound's waves per SIMD,
// which the compiler lowers to what the LDS lets a CU hold: a CU holds
// 4 x waves / (SBLOCK / 64) workgroups, so 4 waves of 128-thread workgroups
// are 8 per CU (128 VGPRs, no scratch; 20.3 KB of LDS each: 8 need <= 20 480 B).
#ifndef RC_SEED_CAP
#define RC_SEED_CAP 512
#endif
#ifndef RC_SEED_WAVES
#define RC_SEED_WAVES (RC_SEED_BLOCK == 256 ? 5 : 4)
#endif
constexpr int SEED_CAP = RC_SEED_CAP;   // seeds of one pass in LDS (a power of two: the bitonic sort pads to one)
static_assert((SEED_CAP & (SEED_CAP - 1)) == 0, "RC_SEED_CAP must be a power of two");
// Hits per lane per batch of the forward pass (their loads in flight
// together; r05 at C3: 3 / 4 / 6 / 7 -> 59.1 / 58.3 / 56.6 / 71.4 ms, 7 no
// longer fits 5 workgroups' LDS; C3v 86.3 -> 84.6 ms at 6)
#ifndef RC_HBATCH
#define RC_HBATCH 6
#endif
constexpr int HBATCH = RC_HBATCH;
// The reverse pass (REV) keeps no seeds in LDS and finds few hits (the
// near-mask index is small): its own instantiation, without the seed and
// per-sample arrays and with fewer hits per lane, runs more workgroups per CU
// (7 waves per SIMD: 7 of 256 threads, 14 of 128).
#ifndef RC_SEED_REV_WAVES
#define RC_SEED_REV_WAVES 7
#endif
#ifndef RC_REV_HBATCH
#define RC_REV_HBATCH 2
#endif
#ifndef RC_PASS_SAMPLES
#define RC_PASS_SAMPLES 256
#endif
constexpr int PASS_SAMPLES = RC_PASS_SAMPLES;                // subject samples of one seed pass (per-sample counts in LDS)

// Oriented query geometry. strand 0: q; strand 1: revcomp(q).
struct QGeo {
    uint64_t qs;   // forward start
    int Lq;
};

__device__ __forceinline__ uint64_t qfwd_pos(const QGeo &q, int strand, uint64_t total, int u)
{
    return strand ? (total - q.qs - (uint64_t)q.Lq + (uint64_t)u) : (q.qs + (uint64_t)u);
}
// walk leftwards from oriented position x (x-1, x-2, ...) as a forward walk
__device__ __forceinline__ uint64_t qrev_pos(const QGeo &q, int strand, uint64_t total, int x)
{
    return strand ? (q.qs + (uint64_t)q.Lq - (uint64_t)x) : (total - q.qs - (uint64_t)x);
}

// ------------------------------------------------------------------------
// seeds
// ------------------------------------------------------------------------

// Exclusive scan of one value per thread over a SBLOCK-thread block (wsum: a
// slot per wave).
__device__ __forceinline__ uint32_t block_exscan(uint32_t v, uint32_t *wsum, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < SBLOCK / 64; i++) {
        const uint32_t w = wsum[i];
        if (i < wid) before += w;
        tot += w;
    }
    __syncthreads();
    total = tot;
    return before + x - v;
}

// last k with pre[k] <= h over an SITEMS + 1 prefix table (the word a hit belongs to)
__device__ __forceinline__ int run_of(const uint32_t *pre, uint32_t h)
{
    int lo = 0, hi = SITEMS;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= h) lo = mid; else hi = mid;
    }
    return lo;
}

// Query word at oriented position p of a transcript (forward start qs,
// length Lq): usable for seeding unless its 16 bases hold an ambiguous base or
// a DUST-masked one (spec 1, 1b; the mask is over forward positions)
template <bool AMB>
__device__ __forceinline__ bool word_usable(const Db &db, uint64_t qs, int Lq, int strand, int p, uint64_t total)
{
    if (AMB) {
        const QGeo qg = {qs, Lq};
        const uint64_t *QM = strand ? db.ARC : db.AF;
        if (win(QM, qfwd_pos(qg, strand, total, p)) & 0xFFFFFFFFull) return false;
    }
    if (db.dmask) {
        const int64_t f = (int64_t)qs + (strand ? (int64_t)(Lq - p - W16) : (int64_t)p);
        if (win_bits(db.dmask, f) & 0xFFFFull) return false;
    }
    return true;
}

// BIG = false: one workgroup per query gene, the seeds of a pass in LDS; a
// (gene, subject sample) pass that alone overflows LDS is put on P.big_list.
// BIG = true: one workgroup per big_list entry, that single pass with its
// seeds in global scratch (P.big_cap per workgroup); an entry that overflows
// even that goes to P.big_retry (the host doubles big_cap).
// ISOG (with BIG = false): one workgroup per gene of P.iso_list -- the genes
// with more than ISO_LDS isoforms, whose isoform tables are read from HBM; the
// plain launch leaves them to it (so its own code has no such path).
template <bool AMB, bool BIG, bool ISOG, bool REV>
__global__ __launch_bounds__(SBLOCK, REV ? RC_SEED_REV_WAVES : RC_SEED_WAVES) void seed_kernel(Db db, Index ix,
                                                                                          SeedParams P)
{
    static_assert(!(REV && BIG), "the reverse pass has no global-memory passes");
    constexpr int HB = REV ? RC_REV_HBATCH : HBATCH;   // hits per lane per batch
    constexpr bool LSEEDS = !BIG && !REV;             // the pass's seeds in LDS
    const uint64_t big_e = BIG ? P.big_list[blockIdx.x] : 0ull;
    const uint32_t g = BIG ? P.gene_begin + (uint32_t)(big_e >> 16)
                           : (ISOG ? P.iso_list[blockIdx.x] : P.gene_begin + blockIdx.x);
    if (g >= P.gene_end) return;
    const int tid = threadIdx.x;

    using SegIdx = typename std::conditional<BIG, uint32_t, uint16_t>::type;
    __shared__ LSeed seeds_lds[LSEEDS ? SEED_CAP : 1];
    const uint32_t cap = BIG ? P.big_cap : (REV ? 0u : (uint32_t)SEED_CAP);
    LSeed *const seeds = BIG ? P.big_seeds + (size_t)blockIdx.x * cap : seeds_lds;
    __shared__ uint32_t it_lo[SITEMS], it_pre[SITEMS + 1], it_info[SITEMS];
    __shared__ uint32_t it_key[SITEMS];
    __shared__ uint32_t it_d[SITEMS];   // D(p): distance to the previous usable query word (spec 2)
    __shared__ __attribute__((aligned(16))) uint32_t hq_pos[SBLOCK / 64][64 * HB];   // per-wave queue of hits for the full test
    __shared__ uint8_t hq_k[SBLOCK / 64][64 * HB];
    __shared__ uint64_t iso_start[ISO_LDS];
    __shared__ uint32_t iso_len[ISO_LDS], iso_gtx[ISO_LDS], iso_pre[ISO_LDS + 1];
    __shared__ uint16_t it_iso[SITEMS];   // isoform of each word item (it_info: p | strand << 24)
    // What only the candidate phase of a pass needs lives in arrays that are
    // dead once the pass's hits are tested (workgroups per CU are what moves
    // this kernel, and LDS is one of their two limits): the segment tables in
    // the hit queue, the per-sample counts and their prefix (by subject
    // sample - T0; the prefix's entries [0, T1 - T0) only) in it_key and
    // it_d, the first candidates' subject transcripts in it_lo, it_pre and
    // it_info. Too small for that (a build knob moved), they get their own.
    constexpr bool SEG_ALIAS = LSEEDS && sizeof(hq_pos) >= (SEED_CAP + 2) * sizeof(SegIdx) + SEED_CAP;
    constexpr bool TCNT_ALIAS = !REV && SITEMS >= PASS_SAMPLES;
    __shared__ SegIdx seg_own[LSEEDS && !SEG_ALIAS ? SEED_CAP + 1 : 1];
    __shared__ __attribute__((aligned(16))) uint8_t segT_own[LSEEDS && !SEG_ALIAS ? SEED_CAP : 4];
    __shared__ uint32_t tcnt_own[REV || TCNT_ALIAS ? 1 : PASS_SAMPLES], tpre_own[REV || TCNT_ALIAS ? 1 : PASS_SAMPLES];
    SegIdx *const seg_lds = SEG_ALIAS ? reinterpret_cast<SegIdx *>(&hq_pos[0][0]) + SEED_CAP / sizeof(SegIdx) : seg_own;
    uint8_t *const segT_lds = SEG_ALIAS ? reinterpret_cast<uint8_t *>(&hq_pos[0][0]) : segT_own;
    uint32_t *const tcnt = TCNT_ALIAS ? it_key : tcnt_own;
    uint32_t *const tpre = TCNT_ALIAS ? it_d : tpre_own;
    SegIdx *const seg_begin = BIG ? reinterpret_cast<SegIdx *>(P.big_seg + (size_t)blockIdx.x * (cap + 1)) : seg_lds;
    uint8_t *const seg_T = BIG ? P.big_segT + (size_t)blockIdx.x * cap : segT_lds;
    __shared__ uint32_t wsum[SBLOCK / 64];
    __shared__ uint32_t sh_nseed, sh_flags, sh_rs0, sh_rs1;
    __shared__ unsigned long long sh_sbase, sh_cbase, sh_lbase;

    // shared searches: the forward pass finds this query's seeds (its usable
    // words, as its own search does); each seed also records whether the
    // reverse search (query = the subject) has a usable word in it (SEED_R)
    const uint64_t *const dm = P.share ? db.dmask : nullptr;
    const int Q = db.gene_sample[g];
    const uint32_t t0 = db.gene_tx_off[g];
    const uint32_t niso = db.gene_tx_off[g + 1] - t0;
    const int N = db.n_samples;
    const uint64_t total = db.total;
    const int stride = P.stride;
    const uint32_t shard = blockIdx.x % NSHARD;
    const int xb = P.xbits;
    if (niso > P.max_iso) {
        if (tid == 0) atomicOr(P.status, ST_GENE_LIMIT);
        return;
    }
    // a gene's isoform tables: in LDS, or -- more than ISO_LDS isoforms (rare:
    // real assemblies have genes with hundreds) -- read from HBM (transcript
    // table and the host's word-item prefix); a block-uniform branch
    const bool isog = BIG ? niso > (uint32_t)ISO_LDS : ISOG;
    if (!BIG && !ISOG && niso > (uint32_t)ISO_LDS) return;   // the ISOG launch takes this gene
    // subject samples of this query sample in this shard (spec 5b: the
    // higher-numbered ones only, the pair's other direction is the mirror
    // image): its row of tmask; tm holds the bits of the current pass's
    // samples [T0, T0 + PASS_SAMPLES) (pass_mask)
    const uint64_t *const tmrow = P.tmask + (size_t)Q * (size_t)P.tmw;
    __shared__ uint64_t tm[4];   // (in LDS: the kernel's scalar registers already spill)
    auto pass_mask = [&](int T0) {   // the caller synchronises before tm is read
        if (tid < 4) {
            const int b = T0 + 64 * tid, wi = b >> 6, sh = b & 63;
            const uint64_t lo = wi < P.tmw ? tmrow[wi] : 0ull, hi = wi + 1 < P.tmw ? tmrow[wi + 1] : 0ull;
            tm[tid] = (lo >> sh) | ((hi << 1) << (63 - sh));
        }
    };
    auto in_mask = [&](int T, int T0) { return ((tm[(T - T0) >> 6] >> ((T - T0) & 63)) & 1ull) != 0; };
    // passes run over the span [T0, Tr) of the subject samples (a contiguous
    // position range, so hits are filtered by position; the query's own
    // sample, inside the span when both directions are searched, is filtered
    // out by position too), halved [T0, T1) while their seeds overflow the
    // pass capacity; the seed test drops any other sample outside the mask
    int T0, Tr;
    if (BIG) {
        T0 = (int)(big_e & 0xFFFFu);
        Tr = T0 + 1;
    } else {
        T0 = P.trange[2 * Q];
        Tr = P.trange[2 * Q + 1];
        if (P.sym || P.share) T0 = max(T0, Q + 1);
    }
    int T1 = min(Tr, T0 + PASS_SAMPLES);
    pass_mask(T0);
    const uint32_t qpb0 = (uint32_t)db.sample_pos_begin[Q], qpb1 = (uint32_t)db.sample_pos_begin[Q + 1];
    // the reverse pass's seeds of this gene's transcripts: [sh_rs0, sh_rs1) of
    // rs_key (rs_range_kernel), loaded beside the isoform tables
    if (P.rs_n && tid < 2) (tid ? sh_rs1 : sh_rs0) = P.rs_range[2 * (size_t)(g - P.gene_begin) + tid];
    // (the word-item prefix of the gene's isoforms comes from the host's
    // table, P.iso_pre_g: gene g's niso + 1 entries start at t0 + g)
    const uint32_t *const gpre = P.iso_pre_g + t0 + g;
    if (!isog) {
        for (uint32_t i = tid; i <= niso; i += SBLOCK) {
            if (i < niso) {
                const IsoRec r = db.giso[t0 + i];
                iso_gtx[i] = r.gtx;
                iso_start[i] = r.start;
                iso_len[i] = r.len;
            }
            iso_pre[i] = gpre[i];
        }
        __syncthreads();
    }
    auto I_gtx = [&](uint32_t i) -> uint32_t { return isog ? db.giso[t0 + i].gtx : iso_gtx[i]; };
    auto I_start = [&](uint32_t i) -> uint64_t { return isog ? (uint64_t)db.giso[t0 + i].start : iso_start[i]; };
    auto I_len = [&](uint32_t i) -> int { return isog ? (int)db.giso[t0 + i].len : (int)iso_len[i]; };
    auto I_pre = [&](uint32_t i) -> uint32_t { return isog ? gpre[i] : iso_pre[i]; };
    const uint32_t n_items = I_pre(niso);
#ifdef RC_ROW_TIMING
    unsigned long long tph[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tc = __builtin_readcyclecounter();
    auto tick = [&](int i) {
        const unsigned long long t = __builtin_readcyclecounter();
        tph[i] += t - tc;
        tc = t;
    };
#define SEED_TICK(i) tick(i)
#else
#define SEED_TICK(i) ((void)0)
#endif
    const uint32_t gl = g - P.gene_begin;

    if (P.rs_n) __syncthreads();   // sh_rs0 / sh_rs1
    SEED_TICK(8);
    while (T0 < Tr) {
        if (tid == 0) {
            sh_nseed = 0;
            sh_flags = 0;
        }
        __syncthreads();
        if (P.rs_n && sh_rs1 > sh_rs0) {
            // reverse-only seeds (SEED_R, no usable word of this query inside)
            // with a subject in this pass's samples
            for (uint32_t i = sh_rs0 + (uint32_t)tid; i < sh_rs1; i += SBLOCK) {
                const LSeed sd = P.rs_rec[P.rs_idx[i]];
                const int T = db.tx[key_gtx(sd.k1, xb)].sample;
                if (T < T0 || T >= T1 || !in_mask(T, T0)) continue;
                const uint32_t slot = atomicAdd(&sh_nseed, 1u);
                if (slot < cap) seeds[slot] = sd;
                else atomicOr(&sh_flags, 1u);
            }
            __syncthreads();
        }
        // words p of the oriented query at stride s, one per thread; hits are
        // the entries of the word's bucket with its key and a position in the
        // subject samples [T0, T1) (samples are contiguous in position)
        const uint32_t pb0 = (uint32_t)db.sample_pos_begin[T0], pb1 = (uint32_t)db.sample_pos_begin[T1];
        // canonical pre-test by sequence: a hit whose s bases before it match
        // (inside both transcripts) extends left past p - s: not canonical
        const bool fast = stride <= 32;
        const bool lpre = !AMB && stride >= 1 && stride < W16;
        for (uint32_t ib = 0; ib < n_items; ib += SITEMS) {
            // IPT word items per thread: item slot e * SBLOCK + tid of the round
            uint32_t lo[IPT], cnt[IPT], info[IPT], key[IPT], ii[IPT], D[IPT];
            bool ok[IPT];
            int p[IPT], strand[IPT];
            // the word's k-mer and its bucket are loaded together with its DUST
            // usability, in flight across the D(p) barriers below (every item
            // of the thread at once)
#pragma unroll
            for (int e = 0; e < IPT; e++) {
                const uint32_t it = ib + (uint32_t)(e * SBLOCK + tid);
                lo[e] = cnt[e] = info[e] = key[e] = ii[e] = 0;
                ok[e] = false;
                p[e] = strand[e] = 0;
                if (it < n_items) {
                    uint32_t i2 = 0;
                    if (!isog) {
                        while (i2 + 1 < niso && iso_pre[i2 + 1] <= it) i2++;
                    } else {
                        uint32_t lo2 = 0, hi2 = niso;   // last isoform with pre <= it
                        while (hi2 - lo2 > 1) {
                            const uint32_t mid = (lo2 + hi2) >> 1;
                            if (gpre[mid] <= it) lo2 = mid; else hi2 = mid;
                        }
                        i2 = lo2;
                    }
                    ii[e] = i2;
                    const uint32_t pre0 = I_pre(i2);
                    const uint32_t rem = it - pre0;
                    const uint32_t ns = (I_pre(i2 + 1) - pre0) >> 1;
                    strand[e] = rem >= ns ? 1 : 0;
                    p[e] = (int)(rem - (strand[e] ? ns : 0)) * stride;
                    info[e] = (uint32_t)p[e] | ((uint32_t)strand[e] << 24);
                    const QGeo qg = {I_start(i2), I_len(i2)};
                    const uint64_t qp = qfwd_pos(qg, strand[e], total, p[e]);
                    const uint64_t *QA = strand[e] ? db.RC : db.F;
                    key[e] = (uint32_t)win(QA, qp);
                    ok[e] = word_usable<AMB>(db, qg.qs, qg.Lq, strand[e], p[e], total);
                    if (ok[e]) {
                        const uint32_t b = key[e] >> (32 - ix.bits);
                        lo[e] = ix.bucket[b];
                        cnt[e] = ix.bucket[b + 1];
                    }
                }
            }
            // D(p): the previous usable word of the same isoform and strand is
            // item it - k (p - k s), in this round's LDS or (before the round's
            // first item) looked up again
#pragma unroll
            for (int e = 0; e < IPT; e++) it_d[e * SBLOCK + tid] = ok[e] ? 1u : 0u;
            __syncthreads();
#pragma unroll
            for (int e = 0; e < IPT; e++) {
                const int slot = e * SBLOCK + tid;
                D[e] = (uint32_t)p[e] + 1u;   // none: every hit is canonical
                if (ok[e]) {
                    for (int k = 1; p[e] - k * stride >= 0; k++) {
                        const bool u = slot - k >= 0 ? it_d[slot - k] != 0
                                                     : word_usable<AMB>(db, I_start(ii[e]), I_len(ii[e]), strand[e],
                                                                        p[e] - k * stride, total);
                        if (u) {
                            D[e] = (uint32_t)(k * stride);
                            break;
                        }
                    }
                }
            }
            __syncthreads();
            SEED_TICK(9);
            // the bucket of the key's top bits: entries are ascending (k-mer,
            // position) and the subject samples a contiguous position range:
            // two lower bounds in the bucket leave exactly the key's entries
            // in [pb0, pb1). Both searches of every item of the thread step
            // together, their loads in flight at once.
            uint32_t b0[IPT], n0[IPT], b1[IPT], n1[IPT];
#pragma unroll
            for (int e = 0; e < IPT; e++) {
                cnt[e] -= lo[e];
                b0[e] = b1[e] = lo[e];
                n0[e] = n1[e] = ok[e] ? cnt[e] : 0u;
            }
            for (;;) {
                uint32_t left = 0;
#pragma unroll
                for (int e = 0; e < IPT; e++) left |= n0[e] | n1[e];
                if (!left) break;
                uint64_t e0[IPT], e1[IPT];
#pragma unroll
                for (int e = 0; e < IPT; e++) {
                    e0[e] = n0[e] ? ix.ent[b0[e] + (n0[e] >> 1)] : 0ull;
                    e1[e] = n1[e] ? ix.ent[b1[e] + (n1[e] >> 1)] : 0ull;
                }
#pragma unroll
                for (int e = 0; e < IPT; e++) {
                    const uint64_t K0 = ((uint64_t)key[e] << 32) | pb0, K1 = ((uint64_t)key[e] << 32) | pb1;
                    const uint32_t h0 = n0[e] >> 1, h1 = n1[e] >> 1;
                    if (n0[e]) {
                        if (e0[e] < K0) { b0[e] += h0 + 1; n0[e] -= h0 + 1; } else n0[e] = h0;
                    }
                    if (n1[e]) {
                        if (e1[e] < K1) { b1[e] += h1 + 1; n1[e] -= h1 + 1; } else n1[e] = h1;
                    }
                }
            }
            SEED_TICK(0);
            uint32_t nh_round = 0;
#pragma unroll
            for (int e = 0; e < IPT; e++) {
                const int slot = e * SBLOCK + tid;
                if (ok[e]) {
                    lo[e] = b0[e];
                    cnt[e] = b1[e] - b0[e];
                } else {
                    lo[e] = cnt[e] = key[e] = 0;
                    }
                it_d[slot] = D[e];
                it_lo[slot] = lo[e];
                it_info[slot] = info[e];
                it_iso[slot] = (uint16_t)ii[e];
                it_key[slot] = key[e];
                // the hits' prefix in item order: slots [e SBLOCK, (e + 1) SBLOCK) after the earlier ones
                uint32_t tot;
                it_pre[slot] = nh_round + block_exscan(cnt[e], wsum, tot);
                nh_round += tot;
            }
            if (tid == 0) it_pre[SITEMS] = nh_round;
            __syncthreads();
            SEED_TICK(1);
            const uint32_t nh = it_pre[SITEMS];
            const int lane = tid & 63, wid = tid >> 6;
            uint32_t *wqp = hq_pos[wid];
            uint8_t *wqk = hq_k[wid];
            for (uint32_t hb0 = 0; hb0 < nh; hb0 += SBLOCK * HB) {
                // pass A: HB hits per lane with their loads in flight
                // together; drop other keys, other samples and hits the
                // sequence pre-test proves non-canonical (the s bases before
                // them equal and unambiguous, no transcript start in
                // (pos - s, pos]: the full test below would reject them)
                uint32_t hk[HB];
                uint64_t hev[HB], hsw[HB], hsm[HB], hbw[HB];
                bool live[HB];
#pragma unroll
                for (int j = 0; j < HB; j++) {
                    const uint32_t h = hb0 + (uint32_t)j * SBLOCK + (uint32_t)tid;
                    live[j] = h < nh;
                    hk[j] = live[j] ? (uint32_t)run_of(it_pre, h) : 0u;
                    hev[j] = live[j] ? ix.ent[it_lo[hk[j]] + (h - it_pre[hk[j]])] : 0ull;
                }
                // Hit-list pre-test (stride < 16, no ambiguity codes): item k-1
                // is the word at p - s of the same isoform and strand, and its
                // hit list is exactly its k-mer's entries in [pb0, pb1), in
                // position order. The s bases before a hit at pos match (same
                // transcript, no start in (pos - s, pos]) iff pos - s is in that
                // list: the entry's 16-mer covers them and the base at pos.
                // The chunk's positions go to LDS (the queue's space) and each
                // hit binary-searches its previous word's list there; hits whose
                // previous list is not wholly in this chunk take the sequence
                // pre-test.
                constexpr uint32_t HCHUNK = SBLOCK * HB;
                uint32_t *chk = &hq_pos[0][0];
                if (lpre) {
                    __syncthreads();   // the previous chunk's queue is consumed
#pragma unroll
                    for (int j = 0; j < HB; j++)
                        if (live[j]) chk[(uint32_t)j * SBLOCK + (uint32_t)tid] = (uint32_t)hev[j];
                    __syncthreads();
                }
                SEED_TICK(5);
#pragma unroll
                for (int j = 0; j < HB; j++) {
                    const uint32_t pos = (uint32_t)hev[j];
                    live[j] = live[j] && (uint32_t)(hev[j] >> 32) == it_key[hk[j]] && pos >= pb0 && pos < pb1 &&
                              (pos < qpb0 || pos >= qpb1);
                    hsw[j] = hsm[j] = hbw[j] = 0;
                    bool decided = false;
                    if (lpre && live[j] && hk[j] > 0 && it_d[hk[j]] == (uint32_t)stride &&
                        (int)(it_info[hk[j]] & 0xFFFFFFu) >= stride) {
                        const uint32_t a = it_pre[hk[j] - 1], b = it_pre[hk[j]];
                        if (a >= hb0 && b <= hb0 + HCHUNK) {
                            const uint32_t tgt = pos - (uint32_t)stride;
                            uint32_t lo = a - hb0, n = b - a;
                            while (n) {
                                const uint32_t half = n >> 1;
                                if (chk[lo + half] < tgt) {
                                    lo += half + 1;
                                    n -= half + 1;
                                } else {
                                    n = half;
                                }
                            }
                            const bool found = pos >= (uint32_t)stride && lo < b - hb0 && chk[lo] == tgt;
                            hsw[j] = found ? 0ull : ~0ull;
                            decided = true;
                        }
                    }
                    if (decided) {
                    } else if (live[j] && fast && it_d[hk[j]] == (uint32_t)stride &&
                               (int)(it_info[hk[j]] & 0xFFFFFFu) >= stride) {
                        // (the 32 query bases before the word are read here, by
                        // the few hits that need them, not kept per item in LDS)
                        const uint32_t inf = it_info[hk[j]], qi = it_iso[hk[j]];
                        const int qst = (int)(inf >> 24);
                        const QGeo qg = {I_start(qi), I_len(qi)};
                        const int64_t qp = (int64_t)qfwd_pos(qg, qst, total, (int)(inf & 0xFFFFFFu));
                        hsw[j] = win_s(db.F, (int64_t)pos - 32) ^ win_s(qst ? db.RC : db.F, qp - 32);
                        if (AMB) hsm[j] = win_s(db.AF, (int64_t)pos - 32) | win_s(qst ? db.ARC : db.AF, qp - 32);
                        hbw[j] = win_bits(db.txstart, (int64_t)pos - 63);
                    } else {
                        hsw[j] = ~0ull;
                    }
                }
                if (lpre) __syncthreads();   // every wave is done with chk before the queue reuses it
                uint32_t qn = 0;
#pragma unroll
                for (int j = 0; j < HB; j++) {
                    if (live[j] && (((hsw[j] | hsm[j]) >> (64 - 2 * stride)) == 0) && ((hbw[j] >> (64 - stride)) == 0))
                        live[j] = false;
                    const uint64_t m = __ballot(live[j]);
                    if (live[j]) {
                        const uint32_t q = qn + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                        wqp[q] = (uint32_t)hev[j];
                        wqk[q] = (uint8_t)hk[j];
                    }
                    qn += (uint32_t)__popcll(m);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                SEED_TICK(6);
                // pass B: the full canonical test and the seed of each queued hit
                for (uint32_t q = (uint32_t)lane; q < qn; q += 64) {
                    const uint32_t pos = wqp[q];
                    const int k = wqk[q];
                    const uint32_t inf = it_info[k];
                    const int p = (int)(inf & 0xFFFFFFu);
                    const uint32_t ii = it_iso[k];
                    const int strand = (int)(inf >> 24);
                    QGeo qg = {I_start(ii), I_len(ii)};
                    const uint64_t *QA = strand ? db.RC : db.F;
                    const uint64_t *QAM = strand ? db.ARC : db.AF;
                    const uint64_t qp = qfwd_pos(qg, strand, total, p);
                    // the transcript lookup and the 32-base windows on both sides
                    // of the word (query and subject) are independent: all their
                    // loads go out together, the bounds are applied afterwards
                    TxInfo st;
                    const uint32_t stx = tx_of_pos(db, ix, pos, st);
                    uint64_t xl = 0, xr = 0, xr2 = 0;   // xr2: the next 32 bases right (exact runs are long)
                    if (fast) {
                        xl = win_s(QA, (int64_t)qp - 32) ^ win_s(db.F, (int64_t)pos - 32);
                        xr = win(QA, qp + W16) ^ win(db.F, (uint64_t)pos + W16);
                        xr2 = win(QA, qp + W16 + 32) ^ win(db.F, (uint64_t)pos + W16 + 32);
                        if (AMB) {
                            xl |= win_s(QAM, (int64_t)qp - 32) | win_s(db.AF, (int64_t)pos - 32);
                            xr |= win(QAM, qp + W16) | win(db.AF, (uint64_t)pos + W16);
                            xr2 |= win(QAM, qp + W16 + 32) | win(db.AF, (uint64_t)pos + W16 + 32);
                        }
                    }
                    // (pos in [pb0, pb1): st.sample is in [T0, T1))
                    if (!in_mask(st.sample, T0)) continue;
                    const int off = (int)(pos - (uint32_t)st.start);
                    const int Dp = (int)it_d[k];
                    const int maxl = min(min(p, off), Dp);
                    int l;
                    if (fast && (xl || maxl <= 32)) {
                        // matching bases leftwards from (p - 1, pos - 1): the
                        // highest differing base of the windows ending there
                        l = min(xl ? (int)(__builtin_clzll(xl) >> 1) : 32, maxl);
                    } else {
                        const uint64_t *QL = strand ? db.F : db.RC;
                        const uint64_t *QLM = strand ? db.AF : db.ARC;
                        l = lcp<AMB>(QL, QLM, qrev_pos(qg, strand, total, p), db.RC, db.ARC,
                                     total - st.start - (uint64_t)off, maxl);
                    }
                    if (l >= Dp) continue;   // not canonical: a usable word lies in [x, p)
                    const int maxr = min(qg.Lq - p - W16, (int)st.len - off - W16);
                    int r;
                    if (fast && xr) {
                        r = min((int)(__builtin_ctzll(xr) >> 1), max(maxr, 0));
                    } else if (fast && xr2) {
                        r = min(32 + (int)(__builtin_ctzll(xr2) >> 1), max(maxr, 0));
                    } else {
                        const int r0 = fast ? min(64, max(maxr, 0)) : 0;
                        r = r0 + lcp64<AMB>(QA, QAM, qp + (uint64_t)(W16 + r0), db.F, db.AF,
                                            st.start + (uint64_t)(off + W16 + r0), maxr - r0);
                    }
                    const int len = l + W16 + r;
                    if (len < P.word) continue;
                    if (REV) {
                        // the reverse pass: only runs the forward pass cannot see
                        // go on -- no usable aligned word of the subject (the
                        // forward query, oriented by the strand) inside -- as
                        // SEED_R seeds of the forward candidate (subject tx,
                        // strand, this tx) in its coordinates
                        const int La = (int)st.len, ya = off - l, pb = p - l;
                        const int xa = strand ? La - ya - len : ya;
                        bool fwd = false;
                        for (int u = (xa + stride - 1) / stride * stride; !fwd && u + W16 <= xa + len; u += stride)
                            fwd = word_usable<AMB>(db, st.start, La, strand, u, total);
                        if (fwd) continue;
                        LSeed sd;
                        sd.k1 = seed_key(P.tx_pos[stx], (uint32_t)strand, I_gtx(ii), (uint32_t)xa, xb);
                        sd.y = (uint32_t)(strand ? qg.Lq - pb - len : pb);
                        sd.len = (uint32_t)len | SEED_R;
                        const unsigned long long k = atomicAdd(P.rseed_n, 1ull);
                        if (k < P.rseed_cap) {
                            P.rseeds[k] = sd;
                            P.rseed_gene[k] = db.tx_gene[stx];
                        }
                        continue;
                    }
                    uint32_t dfl = 0u;
                    if (P.share) {
                        // the reverse search (query = the subject, oriented by the
                        // strand): an aligned word of it in the run's span there,
                        // unmasked. Without DUST one always exists (a run of W =
                        // s + 15 bases holds an aligned word). Runs of the reverse
                        // search with no usable word of this query inside come
                        // from the reverse pass (P.rs_*).
                        bool okR = !dm;
                        if (dm) {
                            const int y = off - l, Lt = (int)st.len;
                            const int r0 = strand ? Lt - y - len : y;   // the run in the reverse query's orientation
                            for (int pp = (r0 + stride - 1) / stride * stride; !okR && pp + W16 <= r0 + len;
                                 pp += stride) {
                                const int64_t f = (int64_t)st.start + (strand ? (int64_t)(Lt - pp - W16) : (int64_t)pp);
                                okR = (win_bits(dm, f) & 0xFFFFull) == 0;
                            }
                        }
                        dfl = SEED_F | (okR ? SEED_R : 0u);
                    }
                    const uint32_t slot = atomicAdd(&sh_nseed, 1u);
                    if (slot < cap) {
                        LSeed sd;
                        sd.k1 = seed_key(ii, (uint32_t)strand, stx, (uint32_t)(p - l), xb);
                        sd.y = (uint32_t)(off - l);
                        sd.len = (uint32_t)len | dfl;
                        seeds[slot] = sd;
                    } else {
                        atomicOr(&sh_flags, 1u);
                    }
                }
                __builtin_amdgcn_wave_barrier();
                SEED_TICK(7);
            }
            __syncthreads();
        }
        if (REV) {   // the reverse pass keeps no seeds of its own: on to the next subject samples
            T0 = T1;
            T1 = min(Tr, T0 + PASS_SAMPLES);
            if (T0 < Tr) {
                pass_mask(T0);
                __syncthreads();
            }
            continue;
        }
        if (sh_flags & 1u) {   // too many seeds: fewer subject samples per pass
            if (T1 - T0 == 1) {
                // one subject sample alone overflows: the global-memory pass
                // takes (gene, T0); its groups stay empty here
                if (tid == 0) {
                    const uint64_t e = ((uint64_t)gl << 16) | (uint64_t)T0;
                    const unsigned long long k = atomicAdd(BIG ? P.big_retry_n : P.big_n, 1ull);
                    if (k < P.big_list_cap) (BIG ? P.big_retry : P.big_out)[k] = e;
                    else atomicOr(P.status, ST_BIG_LIST_FULL);
                }
                T0 = T1;
                T1 = min(Tr, T0 + PASS_SAMPLES);
                pass_mask(T0);
                __syncthreads();
                continue;
            }
            T1 = T0 + (T1 - T0) / 2;
            __syncthreads();
            continue;
        }
        SEED_TICK(2);
        const uint32_t nseed = sh_nseed;
        // the pass's seed and candidate slots are claimed as soon as their
        // counts are known; the atomics' round trips run under the sort and
        // the segment scan (the results are only read by thread 0, later)
        unsigned long long sb_claim = 0, cb_claim = 0;
        if (tid == 0 && nseed) sb_claim = atomicAdd(&P.seed_count[shard], (unsigned long long)nseed);
        // sort by (k1, y). Chunks of SBLOCK seeds: one per thread, bitonic in
        // registers -- partners within the wave by lane exchange, the few
        // stages across waves through the chunk's LDS. Then (LDS pass) merge
        // rounds of sorted runs: each seed's place is its index in its run plus
        // its rank in the partner run (a binary search there), all reads before
        // a barrier, then written in place. Global-memory passes (BIG): one
        // bitonic network over the whole pass instead.
        auto seed_gt = [](const LSeed &a, const LSeed &b) { return (a.k1 > b.k1) || (a.k1 == b.k1 && a.y > b.y); };
        uint32_t np2 = 1;
        if (!BIG || nseed <= SBLOCK) {
            const uint32_t nch = (nseed + SBLOCK - 1) / SBLOCK;
            for (uint32_t c = 0; c < nch; c++) {
                LSeed *cs = seeds + (size_t)c * SBLOCK;
                const uint32_t cn = min(nseed - c * (uint32_t)SBLOCK, (uint32_t)SBLOCK);
                uint32_t cp2 = 1;
                while (cp2 < cn) cp2 <<= 1;
                LSeed v = {~0ull, 0xFFFFFFFFu, 0u};
                if ((uint32_t)tid < cn) v = cs[tid];
                for (uint32_t kk = 2; kk <= cp2; kk <<= 1) {
                    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                        LSeed o;
                        if (j >= 64) {
                            __syncthreads();
                            if ((uint32_t)tid < cp2) cs[tid] = v;
                            __syncthreads();
                            o = (uint32_t)tid < cp2 ? cs[tid ^ j] : v;
                        } else {
                            const int jj = (int)j;
                            o.k1 = ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v.k1 >> 32), jj) << 32) |
                                   (uint32_t)__shfl_xor((int)(uint32_t)v.k1, jj);
                            o.y = (uint32_t)__shfl_xor((int)v.y, jj);
                            o.len = (uint32_t)__shfl_xor((int)v.len, jj);
                        }
                        const bool gt = seed_gt(v, o);
                        const bool want_min = ((tid & j) == 0) == ((tid & kk) == 0);
                        if (gt == want_min) v = o;
                    }
                }
                __syncthreads();
                if ((uint32_t)tid < cn) cs[tid] = v;
            }
            __syncthreads();
            if (!BIG) {
                constexpr int MPT = SEED_CAP / SBLOCK;   // seeds per thread in a merge round
                for (uint32_t w = SBLOCK; w < nseed; w <<= 1) {
                    LSeed mv[MPT];
                    uint32_t mdst[MPT];
#pragma unroll
                    for (int m = 0; m < MPT; m++) {
                        const uint32_t i = (uint32_t)(m * SBLOCK + tid);
                        mdst[m] = ~0u;
                        if (i >= nseed) continue;
                        mv[m] = seeds[i];
                        const uint32_t a0 = i / (2 * w) * (2 * w), b0 = a0 + w;
                        if (b0 >= nseed) {   // a run without a partner stays
                            mdst[m] = i;
                            continue;
                        }
                        const bool inA = i < b0;
                        // partner run [p0, p1): A's seeds go before equal B seeds
                        const uint32_t p0 = inA ? b0 : a0, p1 = inA ? min(b0 + w, nseed) : b0;
                        uint32_t lo = p0, n = p1 - p0;
                        while (n) {
                            const uint32_t h = n >> 1;
                            const LSeed &o = seeds[lo + h];
                            const bool before = inA ? seed_gt(mv[m], o) : !seed_gt(o, mv[m]);
                            if (before) {
                                lo += h + 1;
                                n -= h + 1;
                            } else {
                                n = h;
                            }
                        }
                        mdst[m] = a0 + (i - (inA ? a0 : b0)) + (lo - p0);
                    }
                    __syncthreads();
#pragma unroll
                    for (int m = 0; m < MPT; m++)
                        if (mdst[m] != ~0u) seeds[mdst[m]] = mv[m];
                    __syncthreads();
                }
            }
        } else {
            while (np2 < nseed) np2 <<= 1;
        }
        for (uint32_t i = nseed + tid; i < np2; i += SBLOCK) {
            seeds[i].k1 = ~0ull;
            seeds[i].y = 0xFFFFFFFFu;
        }
        if (np2 > 1) __syncthreads();
        for (uint32_t kk = 2; kk <= np2; kk <<= 1) {
            for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < np2; i += SBLOCK) {
                    const uint32_t ixj = i ^ j;
                    if (ixj > i) {
                        LSeed a = seeds[i], b = seeds[ixj];
                        const bool up = (i & kk) == 0;
                        if (seed_gt(a, b) == up) {
                            seeds[i] = b;
                            seeds[ixj] = a;
                        }
                    }
                }
                __syncthreads();
            }
        }
        SEED_TICK(3);
        // candidates (segments of equal (iso, strand, gtx)), block-parallel
        uint32_t nseg = 0;
        for (uint32_t c0 = 0; c0 < nseed; c0 += SBLOCK) {
            const uint32_t i = c0 + tid;
            const uint32_t f = (i < nseed && (i == 0 || (seeds[i].k1 >> xb) != (seeds[i - 1].k1 >> xb))) ? 1u : 0u;
            uint32_t tot;
            const uint32_t pos = nseg + block_exscan(f, wsum, tot);
            if (f) seg_begin[pos] = (SegIdx)i;
            nseg += tot;
        }
        if (tid == 0) {
            seg_begin[nseg] = (SegIdx)nseed;
            if (nseg) cb_claim = atomicAdd(&P.cand_count[shard], (unsigned long long)nseg);
        }
        const int NT = T1 - T0;   // <= PASS_SAMPLES: counts by T - T0
        for (int T = tid; T < NT; T += SBLOCK) tcnt[T] = 0;
        __syncthreads();
        // the subject transcript of segment tid is kept for the candidate
        // write in the word-item arrays (free after the hits; tile positions
        // are < 2^32)
        for (uint32_t sg = tid; sg < nseg; sg += SBLOCK) {
            const uint32_t gtx = key_gtx(seeds[seg_begin[sg]].k1, xb);
            const TxInfo st = db.tx[gtx];
            if (sg == (uint32_t)tid) {
                it_lo[tid] = (uint32_t)st.start;
                it_pre[tid] = st.len;
                it_info[tid] = (uint32_t)st.sample;
            }
            const int T = st.sample - T0;
            seg_T[sg] = (uint8_t)T;
            atomicAdd(&tcnt[T], 1u);
        }
        __syncthreads();
        for (int c0 = 0, before = 0; c0 < NT; c0 += SBLOCK) {   // (uniform: NT is the block's)
            uint32_t tot;
            const int T = c0 + tid;
            const uint32_t v = T < NT ? tcnt[T] : 0u;
            const uint32_t pre = (uint32_t)before + block_exscan(v, wsum, tot);
            if (T < NT) tpre[T] = pre;
            before += (int)tot;
        }
        if (tid == 0) {
            sh_sbase = sb_claim;
            sh_cbase = cb_claim;
            if (sb_claim + nseed > P.seed_cap || cb_claim + nseg > P.cand_cap) atomicOr(P.status, ST_OVERFLOW);
        }
        __syncthreads();
        const bool room = sh_sbase + nseed <= P.seed_cap && sh_cbase + nseg <= P.cand_cap;
        const uint64_t sbase = (uint64_t)shard * P.seed_cap + sh_sbase;
        const uint64_t cbase = (uint64_t)shard * P.cand_cap + sh_cbase;
        if (room) {
            for (uint32_t i = tid; i < nseed; i += SBLOCK) {
                GSeed gs;
                gs.x = key_x(seeds[i].k1, xb);
                gs.y = seeds[i].y;
                gs.len = seeds[i].len;
                P.seeds[sbase + i] = gs;
            }
            // rounds of SBLOCK candidates (uniform: the list2 append is a block scan)
            for (uint32_t c0 = 0; c0 < nseg; c0 += SBLOCK) {
                const uint32_t sg = c0 + tid;
                uint32_t want = 0;
                uint64_t cslot = 0;
                if (sg < nseg) {
                    const uint32_t b0 = seg_begin[sg], b1 = seg_begin[sg + 1];
                    const uint64_t k1 = seeds[b0].k1;
                    const uint32_t gtx = key_gtx(k1, xb);
                    const int T = seg_T[sg];   // - T0
                    uint32_t rk = 0;   // rank among earlier candidates of the same sample
                    if (T1 - T0 == 1) {
                        rk = sg;
                    } else {
                        // four samples per dword: bytes equal to T are the zero
                        // bytes of w ^ T x 0x01010101
                        const uint32_t pat = 0x01010101u * (uint32_t)T;
                        const uint32_t *const w4 = reinterpret_cast<const uint32_t *>(seg_T);
                        auto zb = [](uint32_t x) {
                            return (uint32_t)__builtin_popcount(~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
                        };
                        const uint32_t nf = sg >> 2;
                        for (uint32_t q = 0; q < nf; q++) rk += zb(w4[q] ^ pat);
                        if (sg & 3u) rk += zb((w4[nf] ^ pat) | (0xFFFFFFFFu << (8u * (sg & 3u))));
                    }
                    Cand c;
                    c.seed_off = (uint32_t)(sbase + b0);
                    c.q_gtx = I_gtx(key_iso(k1, xb));
                    c.s_gtx = gtx;
                    c.seed_lo = (uint16_t)(b1 - b0);
                    c.seed_hi = (uint16_t)((b1 - b0) >> 16);
                    c.strand = (uint8_t)key_strand(k1, xb);
                    c.dflags = 1;
                    c.e0 = 0;
                    c.e1 = SEED_NONE;
                    if (P.share) {
                        // each search's first seed: forward (x, y) order is the
                        // sorted order; reverse order is (y, x) on the plus strand,
                        // (y + len, x + len) descending on the minus strand (the
                        // reverse query is the subject's reverse complement there)
                        int fF = -1, fR = -1;
                        uint64_t bk = ~0ull;
                        for (uint32_t i = b0; i < b1; i++) {
                            const uint32_t sl = seeds[i].len;
                            if ((sl & SEED_F) && fF < 0) fF = (int)(i - b0);
                            if (sl & SEED_R) {
                                const uint32_t sx = key_x(seeds[i].k1, xb), sy = seeds[i].y, ln = sl & SEED_LEN;
                                const uint64_t key = c.strand ? ((uint64_t)~(sy + ln) << 32) | (uint32_t)~(sx + ln)
                                                              : ((uint64_t)sy << 32) | sx;
                                if (key < bk) {
                                    bk = key;
                                    fR = (int)(i - b0);
                                }
                            }
                        }
                        // e0 / e1 are 16-bit seed indices (SEED_NONE reserved)
                        if (fF >= (int)SEED_NONE || fR >= (int)SEED_NONE) atomicOr(P.status, ST_SEED_INDEX);
                        c.dflags = (uint8_t)((fF >= 0 ? 1 : 0) | (fR >= 0 ? 2 : 0));
                        c.e0 = (uint16_t)(fF >= 0 ? fF : fR);
                        c.e1 = (fF >= 0 && fR >= 0 && fR != fF) ? (uint16_t)fR : SEED_NONE;
                        want = c.e1 != SEED_NONE ? 1u : 0u;
                    }
                    const uint32_t qi = key_iso(k1, xb);
                    const uint64_t qstart = I_start(qi);
                    const int qlen = I_len(qi);
                    c.q0 = (uint32_t)(c.strand ? total - qstart - (uint64_t)qlen : qstart);
                    TxInfo st;
                    if (c0 == 0) {
                        st.start = it_lo[tid];
                        st.len = it_pre[tid];
                        st.sample = (int)it_info[tid];
                    } else {
                        st = db.tx[gtx];
                    }
                    c.s0 = (uint32_t)st.start;
                    c.Lq = (int32_t)qlen;
                    c.Lt = (int32_t)st.len;
                    c.qsam = (uint16_t)Q;
                    c.ssam = (uint16_t)st.sample;
                    c.pad0 = 0;
                    c.pad1 = 0;
                    cslot = cbase + tpre[T] + rk;
                    P.cands[cslot] = c;
                }
                if (P.share) {
                    uint32_t tot;
                    const uint32_t pos = block_exscan(want, wsum, tot);
                    if (tot) {
                        if (tid == 0) sh_lbase = atomicAdd(P.list2_n, (unsigned long long)tot);
                        __syncthreads();
                        if (want) P.list2[sh_lbase + pos] = (uint32_t)cslot;
                        __syncthreads();
                    }
                }
            }
        }
        for (int T = T0 + tid; T < T1; T += SBLOCK) {
            const size_t gi = (size_t)gl * (size_t)N + (size_t)T;
            P.gc_off[gi] = (uint32_t)(cbase + tpre[T - T0]);
            P.gc_cnt[gi] = tcnt[T - T0];
        }
        T0 = T1;
        T1 = min(Tr, T0 + PASS_SAMPLES);
        if (T0 < Tr) {   // (no next pass: no mask to load, nothing to wait for)
            pass_mask(T0);
            __syncthreads();
        }
        SEED_TICK(4);
    }
#ifdef RC_ROW_TIMING
    if (tid == 0 && P.prof)
        for (int i = 0; i < 10; i++) atomicAdd(&P.prof[i], tph[i]);
#endif
#undef SEED_TICK
}

// Reverse-only seeds of each query gene of [g0, g1): the lower bounds of g
// and g + 1 in rs_key (sorted by forward gene), one thread per gene (instead
// of a dependent binary search at the start of every seed workgroup).
__global__ void rs_range_kernel(const uint32_t *__restrict__ rs_key, uint32_t rs_n, uint32_t g0, uint32_t g1,
                                uint32_t *__restrict__ out)
{
    const uint64_t n = (uint64_t)(g1 - g0) * 2;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t key = g0 + (uint32_t)(i >> 1) + (uint32_t)(i & 1);
        uint32_t lo = 0, m = rs_n;
        while (m) {
            const uint32_t h = m >> 1;
            if (rs_key[lo + h] < key) {
                lo += h + 1;
                m -= h + 1;
            } else {
                m = h;
            }
        }
        out[i] = lo;
    }
}

void launch_rs_range(const uint32_t *rs_key, uint32_t rs_n, uint32_t g0, uint32_t g1, uint32_t *out, hipStream_t st)
{
    const uint64_t n = (uint64_t)(g1 - g0) * 2;
    if (!n) return;
    const uint64_t g = std::min<uint64_t>((n + 255) / 256, 65536);
    hipLaunchKernelGGL(rs_range_kernel, dim3((unsigned)g), dim3(256), 0, st, rs_key, rs_n, g0, g1, out);
}

template <bool AMB, bool REV>
static void launch_seed_t(const Db &db, const Index &ix, const SeedParams &P, uint32_t n, hipStream_t st)
{
    hipLaunchKernelGGL((seed_kernel<AMB, false, false, REV>), dim3(n), dim3(SBLOCK), 0, st, db, ix, P);
    if (P.iso_n)   // the run's genes with more than ISO_LDS isoforms
        hipLaunchKernelGGL((seed_kernel<AMB, false, true, REV>), dim3(P.iso_n), dim3(SBLOCK), 0, st, db, ix, P);
}

void launch_seed(bool amb, const Db &db, const Index &ix, const SeedParams &P, hipStream_t st)
{
    const uint32_t n = P.gene_end - P.gene_begin;
    if (n == 0) return;
    if (P.rev)
        (amb ? launch_seed_t<true, true> : launch_seed_t<false, true>)(db, ix, P, n, st);
    else
        (amb ? launch_seed_t<true, false> : launch_seed_t<false, false>)(db, ix, P, n, st);
}

// the global-memory passes of the (gene, sample) entries P.big_list[0, n)
void launch_seed_big(bool amb, const Db &db, const Index &ix, const SeedParams &P, uint32_t n, hipStream_t st)
{
    if (n == 0) return;
    if (amb)
        hipLaunchKernelGGL((seed_kernel<true, true, false, false>), dim3(n), dim3(SBLOCK), 0, st, db, ix, P);
    else
        hipLaunchKernelGGL((seed_kernel<false, true, false, false>), dim3(n), dim3(SBLOCK), 0, st, db, ix, P);
}

}  // namespace rcg
