// The seed index's radix sort, hand-written for gfx950 (replaces rocPRIM's
// onesweep in the index build).
//
// Keys are the index entries (k-mer << 32 | position), sorted stably on the
// key bits [bb, 64) -- the k-mer (bb = 32) for the main index, all 64 bits for
// the reverse pass's near-mask index -- by least-significant-digit passes of 8
// bits. One launch per pass (onesweep: decoupled look-back), with the array
// cut into OS_SEG segments that are independent look-back chains:
//
//   * segments: pass 0's input in OS_SEG equal ranges; pass p's input (pass
//     p-1's output) in the ranges of pass p-1's digit groups (256 / OS_SEG
//     consecutive digits each). A digit's output range is then the segments'
//     shares one after another, so the pass stays stable, and the counts that
//     place them -- how many keys of segment s have digit d -- are counted for
//     every pass before the first (seg_hist_kernel: one read of the keys).
//   * tiles of OS_TILE keys within a segment, taken from a counter in
//     round-robin order over the segments (tile j of every segment, then tile
//     j + 1): a tile's look-back predecessor was taken OS_SEG tiles earlier,
//     so the look-back finds a published prefix after few steps (one chain over
//     the whole array left every tile walking back over the tiles in flight).
//   * each wave ranks its keys stably by digit: item j of lane l is key
//     j * 64 + l of the wave's slice, matched against the wave's other lanes
//     by 8 ballots (one per digit bit) and counted in the wave's own LDS
//     histogram, so equal digits keep their input order;
//   * the tile's per-digit counts are published to the look-back table as
//     {tag, count} granules (agent-scope 64-bit stores; the tag carries the
//     pass's epoch, so the table needs no clearing between passes) and each
//     digit's exclusive prefix over the segment's earlier tiles is summed back
//     to a tile whose inclusive prefix is published;
//   * the keys go to LDS in digit order and leave in runs per digit, each run
//     to consecutive global slots.
//
// The main index (os_index_sort) does not run four such passes. It partitions
// the entries on their top G k-mer bits by one or two passes of up to 9 bits
// (the same kernel with 512 digits), finds the 2^G ranges' offsets by binary
// search, and one workgroup per range then sorts the range's remaining k-mer
// bits in LDS and writes the range's bucket entries (range_local_kernel).
// Ranges past the workgroup's capacity are listed for the host, which sorts
// each with the 8-bit passes; more of them than the list holds and the whole
// index is sorted by the 8-bit passes.
#include "device.h"
#include "launch.h"

#include <algorithm>
#include <functional>
#include <type_traits>
#include <utility>

namespace rcg {

namespace {
#ifndef OS_BLOCK_M
#define OS_BLOCK_M 512
#endif
#ifndef OS_ITEMS_M
#define OS_ITEMS_M 16
#endif
#ifndef OS_MINB
#define OS_MINB 2                              // workgroups per CU
#endif
constexpr int OS_BLOCK = OS_BLOCK_M;           // 8 waves
constexpr int OS_WAVES = OS_BLOCK / 64;
constexpr int OS_ITEMS = OS_ITEMS_M;           // keys per thread
constexpr int OS_TILE = OS_BLOCK * OS_ITEMS;   // 8192 keys, 64 KB of LDS
constexpr int RADIX = 256;                     // 8-bit digits (RB = 8); the index's global passes: RB = 9
constexpr int HIST_BLOCK = 256;
constexpr int HIST_MAXP = 8;
#ifndef OS_SEG_M
#define OS_SEG_M 8
#endif
constexpr int OS_SEG = OS_SEG_M;               // look-back chains per pass (power of 2)
static_assert(OS_SEG >= 1 && OS_SEG <= 16 && (OS_SEG & (OS_SEG - 1)) == 0,
              "seg_hist_kernel holds 8 passes x OS_SEG x 256 counters in LDS (<= 128 KB)");
constexpr int OS_SEG_LOG2 = OS_SEG >= 16 ? 4 : OS_SEG >= 8 ? 3 : OS_SEG >= 4 ? 2 : OS_SEG >= 2 ? 1 : 0;
// A pass of RB-bit digits (R = 2^RB of them).
// scratch (u32 words): per pass the segment histograms H[S][R], segment
// bases SB[S][R], digit bases [R], segment offsets [S + 1], tile bases
// [S + 1]; tile counters; then the claim order of the current pass
template <int RB>
struct Rx {
    static constexpr int R = 1 << RB;
    static constexpr int GSH = RB - OS_SEG_LOG2;   // a digit's group (the next pass's segment): digit >> GSH
    static constexpr uint64_t PASS_WORDS = 2 * OS_SEG * R + R + 2 * 64 + 2;
    static constexpr uint64_t FIXED_WORDS = HIST_MAXP * PASS_WORDS + HIST_MAXP;
};
// the digits of a sort's passes: pass p sorts on (key >> shift[p]) & mask[p]
struct PassBits {
    int np;
    int shift[HIST_MAXP];
    uint32_t mask[HIST_MAXP];
};
// 8-bit passes over the bits [bb, eb)
inline PassBits byte_passes(int bb, int eb)
{
    PassBits B{};
    B.np = (eb - bb + 7) / 8;
    for (int p = 0; p < B.np; p++) {
        B.shift[p] = bb + 8 * p;
        B.mask[p] = 255u;
    }
    return B;
}
}   // namespace

typedef __attribute__((address_space(1))) unsigned long long gu64;

struct PassTab {
    uint32_t *H, *SB, *base, *segoff, *tbase;
};
template <int RB>
__host__ __device__ inline PassTab pass_tab(uint32_t *scratch, int p)
{
    constexpr int R = Rx<RB>::R;
    uint32_t *q = scratch + (uint64_t)p * Rx<RB>::PASS_WORDS;
    return {q, q + OS_SEG * R, q + 2 * OS_SEG * R, q + 2 * OS_SEG * R + R, q + 2 * OS_SEG * R + R + 64};
}

// Segment histograms of every pass, one read of the keys: pass 0 counts digit
// 0 per input segment (index / segsize), pass p >= 1 counts digit p per digit
// group of digit p - 1. Per-block LDS tables (np * S * 256 u32, dynamic),
// added to H at the end.
template <int RB>
__global__ __launch_bounds__(HIST_BLOCK) void seg_hist_kernel(const uint64_t *__restrict__ keys, uint64_t n,
                                                              PassBits B, uint64_t segsize, uint32_t *scratch)
{
    extern __shared__ uint32_t h[];
    constexpr int R = Rx<RB>::R, GSH = Rx<RB>::GSH;
    const int tab = OS_SEG * R, np = B.np;
    for (int i = threadIdx.x; i < np * tab; i += HIST_BLOCK) h[i] = 0;
    __syncthreads();
    // 8 keys per thread in flight at a time (coalesced: key q of a thread is
    // HIST_BLOCK apart), then their counts
    constexpr int HQ = 8;
    const uint64_t stride = (uint64_t)gridDim.x * HIST_BLOCK * HQ;
    for (uint64_t i0 = (uint64_t)blockIdx.x * HIST_BLOCK * HQ + threadIdx.x; i0 < n; i0 += stride) {
        uint64_t kk[HQ];
#pragma unroll
        for (int q = 0; q < HQ; q++) {
            const uint64_t i = i0 + (uint64_t)q * HIST_BLOCK;
            kk[q] = i < n ? keys[i] : 0ull;
        }
#pragma unroll
        for (int q = 0; q < HQ; q++) {
            const uint64_t i = i0 + (uint64_t)q * HIST_BLOCK;
            if (i >= n) break;
            uint32_t prev = (uint32_t)(i / segsize);
            for (int p = 0; p < np; p++) {
                const uint32_t d = (uint32_t)(kk[q] >> B.shift[p]) & B.mask[p];
                atomicAdd(&h[p * tab + (p ? (prev >> GSH) : prev) * R + d], 1u);
                prev = d;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < np * tab; i += HIST_BLOCK)
        if (h[i]) atomicAdd(&pass_tab<RB>(scratch, i / tab).H[i % tab], h[i]);
}

// Every pass's tables from the histograms (one block, thread d = digit):
// digit bases, segment bases SB[s][d] = base[d] + sum_{s' < s} H[s'][d],
// segment offsets (pass 0: equal ranges; pass p: pass p-1's digit groups),
// tile bases (segment-major tile numbering).
template <int RB>
__global__ __launch_bounds__(Rx<RB>::R) void seg_scan_kernel(uint32_t *scratch, int np, uint64_t n, uint64_t segsize)
{
    constexpr int RADIX = Rx<RB>::R, OS_GSH = Rx<RB>::GSH;
    __shared__ uint32_t s[RADIX];
    const int d = threadIdx.x;
    for (int p = 0; p < np; p++) {
        const PassTab T = pass_tab<RB>(scratch, p);
        uint32_t tot = 0;
        for (int g = 0; g < OS_SEG; g++) tot += T.H[g * RADIX + d];
        s[d] = tot;
        __syncthreads();
        for (int o = 1; o < RADIX; o <<= 1) {
            const uint32_t v = d >= o ? s[d - o] : 0u;
            __syncthreads();
            s[d] += v;
            __syncthreads();
        }
        const uint32_t base = s[d] - tot;
        T.base[d] = base;
        uint32_t acc = base;
        for (int g = 0; g < OS_SEG; g++) {
            T.SB[g * RADIX + d] = acc;
            acc += T.H[g * RADIX + d];
        }
        __syncthreads();
        if (d == 0) {
            const PassTab Q = pass_tab<RB>(scratch, p > 0 ? p - 1 : 0);
            uint32_t tb = 0;
            for (int g = 0; g <= OS_SEG; g++) {
                uint64_t off;
                if (g == OS_SEG) off = n;
                else if (p == 0) off = std::min<uint64_t>((uint64_t)g * segsize, n);
                else off = Q.base[g << OS_GSH];
                T.segoff[g] = (uint32_t)off;
            }
            for (int g = 0; g < OS_SEG; g++) {
                T.tbase[g] = tb;
                tb += (T.segoff[g + 1] - T.segoff[g] + OS_TILE - 1) / OS_TILE;
            }
            T.tbase[OS_SEG] = tb;
        }
        __syncthreads();
    }
}

// The claim order of pass p's tiles: tile j of every segment (in segment
// order) before tile j + 1 of any. order[position] = segment-major tile id.
template <int RB>
__global__ void tile_order_kernel(const uint32_t *scratch, int p, uint32_t *order, uint32_t tmax)
{
    const PassTab T = pass_tab<RB>(const_cast<uint32_t *>(scratch), p);
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= tmax || g >= T.tbase[OS_SEG]) return;
    int sg = 0;
    while (sg + 1 < OS_SEG && T.tbase[sg + 1] <= g) sg++;
    const uint32_t j = g - T.tbase[sg];
    uint32_t pos = 0;
    for (int q = 0; q < OS_SEG; q++) {
        const uint32_t nt = T.tbase[q + 1] - T.tbase[q];
        pos += std::min(nt, j) + (q < sg && nt > j ? 1u : 0u);
    }
    order[pos] = g;
}

// The index fill (kernels.hip kmer_fill_kernel, no ambiguity codes: entry
// koff[t] + o is window o of transcript t) with the sort's segment
// histograms counted on the way, so the sort does not read the keys to count
// them. Wave per transcript, grid-stride; per-block LDS tables.
template <int RB>
__global__ __launch_bounds__(1024) void kmer_fill_hist_kernel(const TxInfo *__restrict__ tx, uint32_t n_tx,
                                                             const uint64_t *__restrict__ F,
                                                             const uint64_t *__restrict__ out_off,
                                                             uint64_t *__restrict__ ent, PassBits B, uint64_t segsize,
                                                             uint32_t *scratch)
{
    extern __shared__ uint32_t h[];
    constexpr int RADIX = Rx<RB>::R, OS_GSH = Rx<RB>::GSH;
    const int tab = OS_SEG * RADIX, np = B.np;
    for (int i = threadIdx.x; i < np * tab; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t wpb = blockDim.x >> 6, nwave = gridDim.x * wpb;
    for (uint32_t t = blockIdx.x * wpb + (threadIdx.x >> 6); t < n_tx; t += nwave) {
        const TxInfo ti = tx[t];
        const int64_t nwin = (int64_t)ti.len - W16 + 1;
        const uint64_t base = out_off[t];
        for (int64_t o0 = 0; o0 < nwin; o0 += 64) {
            // the segment of the 64 entries: one division per wave (a segment
            // holds at least 64 entries once n >= 64 OS_SEG)
            const uint64_t i0 = base + (uint64_t)o0;
            const uint32_t s0 = (uint32_t)(i0 / segsize);
            const uint64_t nb = (uint64_t)(s0 + 1) * segsize;
            const int64_t o = o0 + lane;
            if (o >= nwin) continue;
            const uint64_t p = ti.start + (uint64_t)o;
            const uint32_t key = (uint32_t)win(F, p);
            const uint64_t i = base + (uint64_t)o;
            if (ent) ent[i] = ((uint64_t)key << 32) | p;   // null: the first pass generates the keys itself
            uint32_t prev = segsize >= 64 ? s0 + (i >= nb ? 1u : 0u) : (uint32_t)(i / segsize);
            for (int q = 0; q < np; q++) {
                const uint32_t d = (key >> (B.shift[q] - 32)) & B.mask[q];   // the passes sort k-mer bits
                atomicAdd(&h[q * tab + (q ? (prev >> OS_GSH) : prev) * RADIX + d], 1u);
                prev = d;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < np * tab; i += blockDim.x)
        if (h[i]) atomicAdd(&pass_tab<RB>(scratch, i / tab).H[i % tab], h[i]);
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Pass 0 without the entry array: key i of the fill order is window
// i - koff[t] of tile transcript t (koff[t] <= i < koff[t + 1]), so the first
// pass computes it from the packed sequence instead of reading 8 bytes the
// fill would have written (transcripts without ambiguity codes).
struct KeyGen {
    const TxInfo *tx;
    const uint64_t *koff;   // n_tx + 1 entries
    const uint64_t *F;
    uint32_t n_tx;
    uint32_t *tile_tx;      // per pass-0 tile: its first transcript
};

// the transcript of entry i: last t with koff[t] <= i (binary search)
__device__ __forceinline__ uint32_t gen_tx_of(const uint64_t *koff, uint32_t n_tx, uint64_t i)
{
    uint32_t lo = 0, hi = n_tx;   // koff[lo] <= i < koff[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (koff[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// the first transcript of every pass-0 tile (one thread per tile)
__global__ void gen_tile_tx_kernel(const uint32_t *scratch, KeyGen G, uint32_t tmax)
{
    const PassTab T = pass_tab<8>(const_cast<uint32_t *>(scratch), 0);
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= tmax || g >= T.tbase[OS_SEG]) return;
    int sg = 0;
    while (sg + 1 < OS_SEG && T.tbase[sg + 1] <= g) sg++;
    const uint64_t t0 = (uint64_t)T.segoff[sg] + (uint64_t)(g - T.tbase[sg]) * OS_TILE;
    G.tile_tx[g] = gen_tx_of(G.koff, G.n_tx, t0);
}

#ifdef OS_STATS
__device__ unsigned long long os_stats[4];   // look-back loads, not-ready polls, tiles
#endif

// One tile: load; the tile's digit counts (LDS atomics) published at once;
// waves 0-3 then walk the look-back (one digit per thread) while waves 4-7
// rank their keys, and rank theirs after it; the keys go to LDS in digit
// order and out in runs.
// RB = 9 (512 digits, the digit (key >> shift) & dmask): every thread of the
// block walks the look-back, so the ranking follows it; the per-wave counts
// (<= 1024) are held in 16 bits and the digits' global offsets in 32 (mod
// 2^32: n < 2^32), which keeps two workgroups on a CU (78 KB of LDS each).
template <bool GEN, int RB>
__global__ __launch_bounds__(OS_BLOCK, OS_MINB * OS_WAVES / 4) void onesweep_kernel(const uint64_t *__restrict__ in,
                                                                     uint64_t *__restrict__ out, int shift,
                                                                     uint32_t dmask, const uint32_t *scratch, int p,
                                                                     const uint32_t *__restrict__ order,
                                                                     gu64 *status, uint32_t epoch, uint32_t *tile_ctr,
                                                                     uint64_t n_all, KeyGen G)
{
    constexpr int RADIX = Rx<RB>::R;
    static_assert(OS_BLOCK >= RADIX && OS_TILE <= 65536 && OS_ITEMS % 2 == 0, "one look-back thread per digit; 16-bit ranks");
    using hist_t = std::conditional_t<RB == 8, uint32_t, uint16_t>;
    using goff_t = std::conditional_t<RB == 8, uint64_t, uint32_t>;
    __shared__ uint64_t s_keys[OS_TILE];
    __shared__ hist_t s_hist[OS_WAVES * RADIX];
    __shared__ uint32_t s_cnt[RADIX];
    __shared__ uint32_t s_start[RADIX];
    __shared__ goff_t s_goff[RADIX];
    __shared__ uint32_t s_wsum[RADIX / 64];
    __shared__ uint32_t s_tile;
    constexpr int GTX = 64;   // GEN: the tile's transcripts staged (first entry, start); more: searched in HBM
    __shared__ uint64_t s_gk[GEN ? GTX + 1 : 1], s_gs[GEN ? GTX : 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const PassTab T = pass_tab<RB>(const_cast<uint32_t *>(scratch), p);
    if (tid == 0) {
        const uint32_t c = atomicAdd(tile_ctr, 1u);
        s_tile = c < T.tbase[OS_SEG] ? order[c] : 0xFFFFFFFFu;
    }
    for (int i = tid; i < OS_WAVES * RADIX; i += OS_BLOCK) s_hist[i] = 0;
    if (tid < RADIX) s_cnt[tid] = 0;
    __syncthreads();
    const uint32_t tile = s_tile;   // segment-major tile id (look-back index)
    if (tile == 0xFFFFFFFFu) return;
    int sg = 0;
    while (sg + 1 < OS_SEG && T.tbase[sg + 1] <= tile) sg++;
    const uint32_t tj = tile - T.tbase[sg];   // the tile's index within its segment
    const uint64_t t0 = (uint64_t)T.segoff[sg] + (uint64_t)tj * OS_TILE;
    const uint64_t n = std::min<uint64_t>(t0 + OS_TILE, T.segoff[sg + 1]);   // keys [t0, n)
    const uint64_t wbase = t0 + (uint64_t)w * (64 * OS_ITEMS) + (uint64_t)lane;
    uint64_t k[OS_ITEMS];
    if constexpr (GEN) {
        // the tile's transcripts from its first: their first entries and starts
        const uint32_t tf = G.tile_tx[tile];
        for (int q = tid; q <= GTX; q += OS_BLOCK) {
            const uint32_t t = tf + (uint32_t)q;
            s_gk[q] = t <= G.n_tx ? G.koff[t] : ~0ull;
            if (q < GTX) s_gs[q] = t < G.n_tx ? G.tx[t].start : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < OS_ITEMS; j++) {
            const uint64_t i = wbase + (uint64_t)j * 64;
            uint64_t key = 0;
            if (i < n) {
                uint64_t st, k0;
                if (s_gk[GTX] > i) {   // among the staged transcripts: last q with first entry <= i
                    int lo = 0, hi = GTX;
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (s_gk[mid] <= i) lo = mid; else hi = mid;
                    }
                    st = s_gs[lo];
                    k0 = s_gk[lo];
                } else {
                    const uint32_t t = gen_tx_of(G.koff, G.n_tx, i);
                    st = G.tx[t].start;
                    k0 = G.koff[t];
                }
                const uint64_t pos = st + (i - k0);
                key = ((uint64_t)(uint32_t)win(G.F, pos) << 32) | pos;
            }
            k[j] = key;
        }
    } else {
#pragma unroll
        for (int j = 0; j < OS_ITEMS; j++) {
            const uint64_t i = wbase + (uint64_t)j * 64;
            k[j] = i < n ? in[i] : 0ull;
        }
    }
    // the tile's digit counts
#pragma unroll
    for (int j = 0; j < OS_ITEMS; j++)
        if (wbase + (uint64_t)j * 64 < n) atomicAdd(&s_cnt[(uint32_t)(k[j] >> shift) & dmask], 1u);
    __syncthreads();
    const uint64_t gt_mask = lane == 63 ? 0ull : ~0ull << (lane + 1);
    hist_t *hw = s_hist + w * RADIX;
    uint32_t r[OS_ITEMS / 2];   // two 16-bit ranks per register (a rank < OS_TILE)
    // stable rank of each key among the wave's keys of its digit
    auto rank = [&]() {
#pragma unroll
        for (int j = 0; j < OS_ITEMS; j++) {
            const bool valid = wbase + (uint64_t)j * 64 < n;
            const uint32_t d = (uint32_t)(k[j] >> shift) & dmask;
            uint64_t peers = __ballot(valid);
#pragma unroll
            for (int b = 0; b < RB; b++) {
                const bool bit = (d >> b) & 1u;
                const uint64_t m = __ballot(bit);
                peers &= bit ? m : ~m;
            }
            const uint32_t old = hw[d];
            const uint32_t rk = old + lanes_below(peers);
            if (j & 1) r[j >> 1] |= rk << 16;
            else r[j >> 1] = rk;
            if (valid && (peers & gt_mask) == 0) hw[d] = (hist_t)(old + (uint32_t)__popcll(peers));
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
        }
    };
    if (tid < RADIX) {
        // publish this tile's count, then the exclusive prefix of the segment's
        // earlier tiles (decoupled look-back) and the inclusive one
        const uint32_t tot = s_cnt[tid];
        const uint64_t AGG = (uint64_t)(2u * epoch) << 32, INC = (uint64_t)(2u * epoch + 1u) << 32;
        gu64 *mine = status + (uint64_t)tile * RADIX + tid;
        uint32_t excl = 0;
#ifdef OS_STATS
        unsigned long long nl = 0, nw = 0;
#endif
        if (tj == 0) {
            __hip_atomic_store(mine, INC | tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            __hip_atomic_store(mine, AGG | tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int64_t t = (int64_t)tile - 1;
            for (;;) {
                const uint64_t v = __hip_atomic_load(status + (uint64_t)t * RADIX + tid, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t tag = (uint32_t)(v >> 32);
#ifdef OS_STATS
                nl++;
#endif
                if (tag == 2u * epoch + 1u) {
                    excl += (uint32_t)v;
                    break;
                }
                if (tag == 2u * epoch) {
                    excl += (uint32_t)v;
                    t--;
                } else {
#ifdef OS_STATS
                    nw++;
#endif
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            __hip_atomic_store(mine, INC | (uint64_t)(excl + tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#ifdef OS_STATS
        atomicAdd(&os_stats[0], nl);
        atomicAdd(&os_stats[1], nw);
        if (tid == 0) atomicAdd(&os_stats[2], 1ull);
#endif
        // block exclusive scan of the counts over the digits
        uint32_t x = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_wsum[w] = x;
        s_start[tid] = x - tot;
        s_goff[tid] = (goff_t)T.SB[sg * RADIX + tid] + excl;
    }
    rank();
    __syncthreads();
    if (tid < RADIX) {
        uint32_t add = 0;
        for (int v = 0; v < w; v++) add += s_wsum[v];
        const uint32_t st = s_start[tid] + add;
        s_start[tid] = st;
        s_goff[tid] -= st;
        // wave offsets: exclusive over the waves
        uint32_t acc = 0;
#pragma unroll
        for (int v = 0; v < OS_WAVES; v++) {
            const uint32_t c = s_hist[v * RADIX + tid];
            s_hist[v * RADIX + tid] = (hist_t)acc;
            acc += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < OS_ITEMS; j++) {
        if (wbase + (uint64_t)j * 64 < n) {
            const uint32_t d = (uint32_t)(k[j] >> shift) & dmask;
            s_keys[s_start[d] + hw[d] + ((r[j >> 1] >> (16 * (j & 1))) & 0xFFFFu)] = k[j];
        }
    }
    __syncthreads();
    const uint32_t cnt = (uint32_t)(n - t0);
#pragma unroll 4
    for (uint32_t s = tid; s < cnt; s += OS_BLOCK) {
        const uint64_t key = s_keys[s];
        const goff_t gi = s_goff[(uint32_t)(key >> shift) & dmask] + s;
        if (gi < n_all) out[gi] = key;   // always, unless the counts were inconsistent
    }
}

// The index fill with the segment histograms of the passes B (RB-bit tables)
template <int RB>
static void fill_hist(const TxInfo *tx, uint32_t n_tx, const uint64_t *F, const uint64_t *koff, uint64_t *ent,
                      uint64_t n, const PassBits &B, uint32_t *scratch, hipStream_t st)
{
    (void)hipMemsetAsync(scratch, 0, Rx<RB>::FIXED_WORDS * sizeof(uint32_t), st);
    if (!n_tx || !n) return;
    const uint64_t segsize = (n + OS_SEG - 1) / OS_SEG;
    // 16-wave blocks, two per CU (r05: 4.84-4.97 ms at C3 against 5.71 for
    // 2048 four-wave blocks, whose 32 KB tables made a second, partial round
    // of blocks and twice the closing atomics)
    const dim3 g(std::min<uint32_t>((n_tx + 15) / 16, 512));
    hipLaunchKernelGGL(kmer_fill_hist_kernel<RB>, g, dim3(1024), (size_t)B.np * OS_SEG * Rx<RB>::R * sizeof(uint32_t),
                       st, tx, n_tx, F, koff, ent, B, segsize, scratch);
}

// The passes B over keys[0, n), ping-pong between keys and alt; true when the
// result is in alt. gen: the first pass computes the keys (8-bit passes only).
template <int RB>
static bool sort_passes(uint64_t *keys, uint64_t *alt, uint64_t n, const PassBits &B, uint32_t *scratch,
                        uint64_t *status, uint32_t &epoch, hipStream_t st, const std::function<void()> &after_prep,
                        bool counted, const KeyGen *gen)
{
    constexpr int R = Rx<RB>::R;
    const int np = B.np;
    if (n == 0 || np == 0) return false;
    uint32_t *ctr = scratch + HIST_MAXP * Rx<RB>::PASS_WORDS, *order = ctr + HIST_MAXP;
    const uint64_t segsize = (n + OS_SEG - 1) / OS_SEG;
    if (!counted) {
        (void)hipMemsetAsync(scratch, 0, Rx<RB>::FIXED_WORDS * sizeof(uint32_t), st);
        const uint64_t hb = std::min<uint64_t>((n + HIST_BLOCK * 8 - 1) / (HIST_BLOCK * 8), 1024);
        hipLaunchKernelGGL(seg_hist_kernel<RB>, dim3((unsigned)hb), dim3(HIST_BLOCK),
                           (size_t)np * OS_SEG * R * sizeof(uint32_t), st, keys, n, B, segsize, scratch);
    }
    hipLaunchKernelGGL(seg_scan_kernel<RB>, dim3(1), dim3(R), 0, st, scratch, np, n, segsize);
    const uint32_t tmax = (uint32_t)((n + OS_TILE - 1) / OS_TILE + OS_SEG);
    const unsigned grid = tmax;   // tiles beyond a pass's count exit at once
    uint64_t *src = keys, *dst = alt;
    const KeyGen G = gen ? *gen : KeyGen{};
    for (int p = 0; p < np; p++) {
        hipLaunchKernelGGL(tile_order_kernel<RB>, dim3((tmax + 255) / 256), dim3(256), 0, st, scratch, p, order, tmax);
        if constexpr (RB == 8)
            if (p == 0 && gen)
                hipLaunchKernelGGL(gen_tile_tx_kernel, dim3((tmax + 255) / 256), dim3(256), 0, st, scratch, G, tmax);
        if (p == 0 && after_prep) after_prep();
        ++epoch;
        bool done = false;
        if constexpr (RB == 8)
            if (p == 0 && gen) {
                hipLaunchKernelGGL((onesweep_kernel<true, 8>), dim3(grid), dim3(OS_BLOCK), 0, st, src, dst, B.shift[p],
                                   B.mask[p], scratch, p, order, (gu64 *)status, epoch, ctr + p, n, G);
                done = true;
            }
        if (!done)
            hipLaunchKernelGGL((onesweep_kernel<false, RB>), dim3(grid), dim3(OS_BLOCK), 0, st, src, dst, B.shift[p],
                               B.mask[p], scratch, p, order, (gu64 *)status, epoch, ctr + p, n, G);
        std::swap(src, dst);
    }
    return src == alt;
}

// Sort keys[0, n) stably on bits [bb, 64) by ping-pong passes between keys
// and alt; returns true when the result is in alt (odd pass count), false
// when it is back in keys. Scratch (caller-owned, device): os_scratch_words(n)
// u32, status os_status_words(n) u64 (zeroed once when allocated), epoch a
// counter the caller keeps across calls. n < 2^32.
uint64_t os_status_words(uint64_t n) { return ((n + OS_TILE - 1) / OS_TILE + OS_SEG) * (uint64_t)RADIX; }
uint64_t os_scratch_words(uint64_t n) { return Rx<8>::FIXED_WORDS + (n + OS_TILE - 1) / OS_TILE + OS_SEG; }

// after_prep (optional) runs once the tables and the first pass's claim order
// are queued, before the first pass: work for another stream that should not
// starve those one-block kernels (the engine starts DUST there).
// The index fill and the segment histograms of a 32-bit-key sort (bb = 32)
// in one kernel (transcripts without ambiguity codes; koff: first entry of
// each transcript); os_sort_keys(..., counted = true) then skips its count.
// ent == nullptr: counts only (the sort's first pass then generates the keys: os_sort_keys with gen).
void os_fill_hist(const TxInfo *tx, uint32_t n_tx, const uint64_t *F, const uint64_t *koff, uint64_t *ent,
                  uint64_t n, uint32_t *scratch, hipStream_t st)
{
    fill_hist<8>(tx, n_tx, F, koff, ent, n, byte_passes(32, 64), scratch, st);
}

// gen (bb = 32, counted): the first pass computes the keys from the packed
// sequence F of the transcripts tx[0, n_tx) with first entries koff[0, n_tx]
// (keys need not hold them); gen_tile: scratch of os_gen_tile_words(n) u32.
uint64_t os_gen_tile_words(uint64_t n) { return (n + OS_TILE - 1) / OS_TILE + OS_SEG; }

bool os_sort_keys(uint64_t *keys, uint64_t *alt, uint64_t n, int bb, uint32_t *scratch, uint64_t *status,
                  uint32_t &epoch, hipStream_t st, const std::function<void()> &after_prep, bool counted,
                  const TxInfo *gen_tx, const uint64_t *gen_koff, const uint64_t *gen_F, uint32_t gen_ntx,
                  uint32_t *gen_tile)
{
    const bool gen = counted && gen_koff && bb == 32;
    const KeyGen G{gen_tx, gen_koff, gen_F, gen_ntx, gen_tile};
    return sort_passes<8>(keys, alt, n, byte_passes(bb, 64), scratch, status, epoch, st, after_prep, counted,
                          gen ? &G : nullptr);
}

// ---------------------------------------------------------------------------
// The main index: global passes on the top G k-mer bits, then one workgroup
// per range.

namespace {
constexpr int IX_RB = 9;                        // digit bits of a global pass, at most
constexpr int IX_GMAX = 2 * IX_RB;              // at most two global passes
constexpr int LS_BLOCK = 512;                   // 8 waves
constexpr int LS_WAVES = LS_BLOCK / 64;
constexpr int LS_ITEMS = 24;                    // keys per thread, at most
constexpr int LS_CAP = LS_BLOCK * LS_ITEMS;     // 12288 keys: 72 KB of LDS with 16 k-mer bits a key, 96 KB with 32
constexpr int LS_RADIX = 256;                   // local digits: 8 bits at most
constexpr int LS_LIST = 64;                     // oversized ranges listed for the host
constexpr int LS_GRID = 2048;                   // workgroups, each striding over the ranges

// G bits in one pass, or in two of about half each (9 + 9 for G = 18)
inline PassBits index_passes(int G)
{
    PassBits B{};
    B.np = (G + IX_RB - 1) / IX_RB;
    int sh = 64 - G, left = G;
    for (int p = 0; p < B.np; p++) {
        const int w = left / (B.np - p);
        B.shift[p] = sh;
        B.mask[p] = (1u << w) - 1u;
        sh += w;
        left -= w;
    }
    return B;
}
}   // namespace

// off[r] = first entry of keys[0, n) (partitioned on the top G bits) whose top
// G bits are >= r, for r in [0, 2^G]: binary search, one thread per offset
__global__ void range_offsets_kernel(const uint64_t *__restrict__ keys, uint64_t n, int G, uint32_t *__restrict__ off)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x, nr = 1u << G;
    if (r > nr) return;
    uint64_t lo = 0, hi = r == 0 ? 0 : n;
    if (r == nr) lo = n;
    while (lo < hi) {   // r >= 1, so G >= 1
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint32_t)(keys[mid] >> (64 - G)) < r) lo = mid + 1; else hi = mid;
    }
    off[r] = (uint32_t)lo;
}

// bucket[x0 + x] for x in [0, nx): the first entry of the sorted keys[lo, hi)
// whose top `bits` bits are >= x0 + x (the bucket entries of one range)
__global__ void bucket_range_kernel(const uint64_t *__restrict__ keys, uint32_t lo, uint32_t hi, int bits, uint32_t x0,
                                    uint32_t nx, uint32_t *__restrict__ bucket)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nx) return;
    uint32_t a = lo, b = hi;
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if ((uint32_t)(keys[mid] >> (64 - bits)) < x0 + x) a = mid + 1; else b = mid;
    }
    bucket[x0 + x] = a;
}

// One range (the entries with one value r of the top G bits, keys[off[r],
// off[r + 1])) per workgroup at a time, in place: the range into registers, a
// wave's slice of it contiguous; stable passes of up to 8 bits over the bits
// [32, 64 - G), ranked per wave by ballots as the onesweep ranks, scattered to
// LDS in digit order and taken back in slices; the sorted range written back;
// its 2^(bits - G) bucket entries by binary search in LDS. LDS holds a key as
// its position (32 bits) and its k-mer bits below the top G (KL: 16 bits when
// they fit, which keeps two workgroups on a CU -- one loads or stores while
// the other ranks). An empty range writes its bucket entries too, the last
// range bucket[2^bits] = n. A range of more than cap keys is left as it is
// and listed: list[0] counts them, list[1 + 3 i ..] = {r, off[r], off[r + 1]}
// for the first LS_LIST.
template <typename KL>
__global__ __launch_bounds__(LS_BLOCK, sizeof(KL) == 2 ? 4 : 2) void range_local_kernel(
    uint64_t *keys, const uint32_t *__restrict__ off, int G, int bits, uint32_t cap, uint64_t n, uint32_t *list,
    uint32_t *__restrict__ bucket)
{
    static_assert(LS_CAP <= 65536 && LS_ITEMS % 2 == 0, "16-bit ranks and wave offsets");
    __shared__ uint32_t s_pos[LS_CAP];
    __shared__ KL s_kl[LS_CAP];
    __shared__ uint16_t s_hist[LS_WAVES * LS_RADIX];
    __shared__ uint32_t s_start[LS_RADIX];
    __shared__ uint32_t s_wsum[LS_RADIX / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t nr = 1u << G;
    const int sb = bits - G, LB = 32 - G, npl = (LB + 7) / 8;
    const uint32_t nx = 1u << sb, lmask = LB == 32 ? ~0u : (1u << LB) - 1u;
    const uint64_t gt_mask = lane == 63 ? 0ull : ~0ull << (lane + 1);
    uint16_t *hw = s_hist + w * LS_RADIX;
    for (uint32_t r = blockIdx.x; r < nr; r += gridDim.x) {
        const uint32_t lo = off[r], m = off[r + 1] - lo;
        const uint32_t x0 = r << sb, hi = G ? r << LB : 0u;   // the range's k-mers: hi | (KL bits)
        if (r + 1 == nr && tid == 0) bucket[1ull << bits] = (uint32_t)n;
        if (m > cap) {
            if (tid == 0) {
                const uint32_t i = atomicAdd(&list[0], 1u);
                if (i < (uint32_t)LS_LIST) {
                    list[1 + 3 * i] = r;
                    list[2 + 3 * i] = lo;
                    list[3 + 3 * i] = lo + m;
                }
            }
            continue;
        }
        if (m == 0) {
            for (uint32_t x = tid; x < nx; x += LS_BLOCK) bucket[x0 + x] = lo;
            continue;
        }
        // a wave's slice: whole rows of 64 keys, S * LS_WAVES >= m, S <= 64 LS_ITEMS
        const uint32_t S = ((m + LS_WAVES - 1) / LS_WAVES + 63u) & ~63u;
        const int nit = (int)(S >> 6);
        const uint32_t wb = (uint32_t)w * S + (uint32_t)lane;
        uint32_t kp[LS_ITEMS], kl[LS_ITEMS];
#pragma unroll
        for (int j = 0; j < LS_ITEMS; j++) {
            const uint32_t i = wb + (uint32_t)j * 64;
            const uint64_t key = (j < nit && i < m) ? keys[(uint64_t)lo + i] : 0ull;
            kp[j] = (uint32_t)key;
            kl[j] = (uint32_t)(key >> 32) & lmask;
        }
        uint32_t rk[LS_ITEMS / 2];   // two 16-bit ranks per register
        int sh = 0;
        for (int p = 0; p < npl; p++) {
            const int wd = LB / npl + (p < LB % npl ? 1 : 0);
            const uint32_t dm = (1u << wd) - 1u;
            for (int i = tid; i < LS_WAVES * LS_RADIX; i += LS_BLOCK) s_hist[i] = 0;
            __syncthreads();
            // stable rank of each key among the wave's keys of its digit
#pragma unroll
            for (int j = 0; j < LS_ITEMS; j++) {
                if (j < nit) {
                    const bool valid = wb + (uint32_t)j * 64 < m;
                    const uint32_t d = (kl[j] >> sh) & dm;
                    uint64_t peers = __ballot(valid);
#pragma unroll
                    for (int b = 0; b < 8; b++) {
                        if (b < wd) {
                            const bool bit = (d >> b) & 1u;
                            const uint64_t mm = __ballot(bit);
                            peers &= bit ? mm : ~mm;
                        }
                    }
                    const uint32_t old = hw[d];
                    const uint32_t q = old + lanes_below(peers);
                    if (j & 1) rk[j >> 1] |= q << 16;
                    else rk[j >> 1] = q;
                    if (valid && (peers & gt_mask) == 0) hw[d] = (uint16_t)(old + (uint32_t)__popcll(peers));
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("" ::: "memory");
                }
            }
            __syncthreads();
            if (tid < LS_RADIX) {
                // wave offsets (exclusive over the waves), then the digits' starts
                uint32_t acc = 0;
#pragma unroll
                for (int v = 0; v < LS_WAVES; v++) {
                    const uint32_t c = s_hist[v * LS_RADIX + tid];
                    s_hist[v * LS_RADIX + tid] = (uint16_t)acc;
                    acc += c;
                }
                uint32_t x = acc;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t y = __shfl_up(x, o, 64);
                    if (lane >= o) x += y;
                }
                if (lane == 63) s_wsum[w] = x;
                s_start[tid] = x - acc;
            }
            __syncthreads();
            if (tid < LS_RADIX) {
                uint32_t add = 0;
                for (int v = 0; v < w; v++) add += s_wsum[v];
                s_start[tid] += add;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < LS_ITEMS; j++) {
                if (j < nit && wb + (uint32_t)j * 64 < m) {
                    const uint32_t d = (kl[j] >> sh) & dm;
                    const uint32_t at = s_start[d] + hw[d] + ((rk[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
                    s_pos[at] = kp[j];
                    s_kl[at] = (KL)kl[j];
                }
            }
            __syncthreads();
            if (p + 1 < npl) {
#pragma unroll
                for (int j = 0; j < LS_ITEMS; j++) {
                    const uint32_t i = wb + (uint32_t)j * 64;
                    if (j < nit && i < m) {
                        kp[j] = s_pos[i];
                        kl[j] = s_kl[i];
                    }
                }
            }
            sh += wd;
        }
        for (uint32_t s = tid; s < m; s += LS_BLOCK)
            keys[(uint64_t)lo + s] = ((uint64_t)(hi | s_kl[s]) << 32) | s_pos[s];
        for (uint32_t x = tid; x < nx; x += LS_BLOCK) {
            uint32_t a = 0, b = m;
            while (a < b) {
                const uint32_t mid = (a + b) >> 1;
                if (((hi | s_kl[mid]) >> (32 - bits)) < x0 + x) a = mid + 1; else b = mid;
            }
            bucket[x0 + x] = lo + a;
        }
        __syncthreads();   // the next range reuses the LDS
    }
}

// The geometry of the main index of n entries with a table of 2^bits
// buckets: G, the top k-mer bits the global passes partition on, chosen so
// that a range averages at most half of cap keys (cap: the most keys a range
// may hold before it counts as oversized; at most, and by default, the
// local workgroup's capacity). G = 0: one range, no global pass. -1: even
// two global passes leave ranges averaging more than half the local capacity
// (n above 1.6 G entries, a C4 tile): such an index keeps the four 8-bit
// passes and the bucket fill (os_fill_hist, os_sort_keys).
uint32_t os_index_cap(uint32_t cap) { return cap ? std::min<uint32_t>(cap, LS_CAP) : (uint32_t)LS_CAP; }
int os_index_gbits(uint64_t n, int bits, uint32_t cap)
{
    int G = 0;
    while (G < IX_GMAX && G < bits && (n >> G) > os_index_cap(cap) / 2) G++;
    return (n >> G) > (uint64_t)LS_CAP / 2 && G == IX_GMAX ? -1 : G;
}
// buffers (caller-owned, device): the passes' scratch and status (status
// zeroed once when allocated; both also serve os_sort_keys), the range
// offsets and the list of oversized ranges (u32 words)
uint64_t os_index_status_words(uint64_t n) { return ((n + OS_TILE - 1) / OS_TILE + OS_SEG) * (uint64_t)Rx<IX_RB>::R; }
uint64_t os_index_scratch_words(uint64_t n) { return Rx<IX_RB>::FIXED_WORDS + (n + OS_TILE - 1) / OS_TILE + OS_SEG; }
uint64_t os_index_offset_words(int G) { return (1ull << G) + 1; }
uint64_t os_index_list_words() { return 1 + 3 * LS_LIST; }

// The index fill (as os_fill_hist) with the segment histograms of the G-bit
// global passes; os_index_sort(..., counted = true) then skips its count.
void os_index_fill_hist(const TxInfo *tx, uint32_t n_tx, const uint64_t *F, const uint64_t *koff, uint64_t *ent,
                        uint64_t n, int G, uint32_t *scratch, hipStream_t st)
{
    fill_hist<IX_RB>(tx, n_tx, F, koff, ent, n, index_passes(G), scratch, st);
}

// The main index of keys[0, n) (n < 2^32): the entries stably sorted on bits
// [32, 64) and bucket[0, 2^bits] over their top `bits` bits (bits >= G, 16 <=
// bits <= 32). Returns 1 when the sorted entries are in alt, 0 when in keys,
// -1 when wait failed. wait: blocks until the stream is idle (the host reads
// the list of oversized ranges; false = it failed). Each listed range is
// sorted by 8-bit passes and gets its bucket entries from a search of its
// own; more ranges than the list holds (*whole): the whole array is sorted by
// the 8-bit passes and the CALLER fills the bucket table. fb_ranges, fb_keys:
// the ranges and keys that took either fallback.
int os_index_sort(uint64_t *keys, uint64_t *alt, uint64_t n, int G, int bits, uint32_t cap, uint32_t *scratch,
                  uint64_t *status, uint32_t &epoch, uint32_t *offsets, uint32_t *list, uint32_t *bucket,
                  hipStream_t st, bool counted, const std::function<bool()> &wait, uint32_t *fb_ranges,
                  uint64_t *fb_keys, bool *whole)
{
    *fb_ranges = 0;
    *fb_keys = 0;
    *whole = false;
    const bool in_alt = sort_passes<IX_RB>(keys, alt, n, index_passes(G), scratch, status, epoch, st, nullptr, counted,
                                           nullptr);
    uint64_t *cur = in_alt ? alt : keys, *oth = in_alt ? keys : alt;
    const uint32_t nr = 1u << G;
    hipLaunchKernelGGL(range_offsets_kernel, dim3(nr / 256 + 1), dim3(256), 0, st, cur, n, G, offsets);
    (void)hipMemsetAsync(list, 0, sizeof(uint32_t), st);
    if (32 - G <= 16)
        hipLaunchKernelGGL(range_local_kernel<uint16_t>, dim3(std::min<uint32_t>(nr, LS_GRID)), dim3(LS_BLOCK), 0, st,
                           cur, offsets, G, bits, os_index_cap(cap), n, list, bucket);
    else
        hipLaunchKernelGGL(range_local_kernel<uint32_t>, dim3(std::min<uint32_t>(nr, LS_GRID)), dim3(LS_BLOCK), 0, st,
                           cur, offsets, G, bits, os_index_cap(cap), n, list, bucket);
    uint32_t h[1 + 3 * LS_LIST] = {0};
    if (hipMemcpyAsync(h, list, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess || !wait()) return -1;
    if (h[0] > (uint32_t)LS_LIST) {
        *whole = true;
        *fb_ranges = h[0];
        *fb_keys = n;
        const bool swapped = sort_passes<8>(cur, oth, n, byte_passes(32, 64), scratch, status, epoch, st, nullptr,
                                            false, nullptr);
        return (swapped ? oth : cur) == alt;
    }
    for (uint32_t i = 0; i < h[0]; i++) {
        const uint32_t r = h[1 + 3 * i], lo = h[2 + 3 * i], hi = h[3 + 3 * i], m = hi - lo;
        if (sort_passes<8>(cur + lo, oth + lo, m, byte_passes(32, 64 - G), scratch, status, epoch, st, nullptr, false,
                           nullptr))
            (void)hipMemcpyAsync(cur + lo, oth + lo, (uint64_t)m * sizeof(uint64_t), hipMemcpyDeviceToDevice, st);
        const uint32_t nx = 1u << (bits - G);
        hipLaunchKernelGGL(bucket_range_kernel, dim3((nx + 255) / 256), dim3(256), 0, st, cur, lo, hi, bits,
                           r << (bits - G), nx, bucket);
        *fb_ranges += 1;
        *fb_keys += m;
    }
    return in_alt;
}

}  // namespace rcg
