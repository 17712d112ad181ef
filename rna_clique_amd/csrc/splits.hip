// The census of the splits of a batch of replicate trees and their
// Robinson-Foulds distances (rc_split_census, rc_tree_rf). The kernels only
// read what nj_kernel left: splits (R x ns x W words, ns = N - 3) and valid.
//
// An instance is (replicate r, join t), flat index r * ns + t; only those of
// valid replicates count. Two instances are of one class when their W words
// are equal. A class is represented by its lowest flat index, and the classes
// are numbered 0..K-1 in ascending order of that index: the id of a class is
// the exclusive prefix sum of "this instance represents its class". Which
// slot of the hash table a class lands in depends on the order of the
// atomics; its representative (a minimum) and its count (an integer sum) do
// not, so the census is the same bytes on every run.
//
// The table: open addressing, linear probing, uint32 slots, a power of two
// >= 2 x instances (never more than half full, so every probe sequence ends).
// A slot holds a flat index of its class, in the end the lowest. A probe
// compares all W words: the hash only picks the first slot.
#include "device.h"
#include "launch.h"

#include <algorithm>

namespace rcg {

constexpr uint32_t SP_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t RF_INVALID = 0xFFFFFFFFu;

static inline unsigned split_grid(uint64_t n, unsigned block, unsigned cap = 65536)
{
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + block - 1) / block, cap));
}

__device__ inline uint64_t split_hash(const uint64_t *__restrict__ s, int W)
{
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int w = 0; w < W; w++) {
        h = (h ^ s[w]) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 33;
    }
    h *= 0xC4CEB9FE1A85EC53ull;
    return h ^ (h >> 29);
}

__device__ inline bool split_equal(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, int W)
{
    bool eq = true;
    for (int w = 0; w < W; w++) eq = eq && a[w] == b[w];
    return eq;
}

// Every instance of a valid replicate enters the table: it claims the first
// empty slot of its probe sequence, or lowers the flat index in the slot of
// its class.
__global__ __launch_bounds__(256) void split_insert_kernel(const uint64_t *__restrict__ splits,
                                                           const uint8_t *__restrict__ valid, uint32_t n_inst,
                                                           uint32_t ns, int W, uint32_t *table, uint32_t mask)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_inst;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t idx = (uint32_t)i;
        if (!valid[idx / ns]) continue;
        const uint64_t *mine = splits + (uint64_t)idx * W;
        uint32_t slot = (uint32_t)split_hash(mine, W) & mask;
        for (;;) {
            const uint32_t cur = atomicCAS(&table[slot], SP_EMPTY, idx);
            if (cur == SP_EMPTY) break;   // claimed
            if (split_equal(splits + (uint64_t)cur * W, mine, W)) {
                if (idx < cur) atomicMin(&table[slot], idx);
                break;
            }
            slot = (slot + 1) & mask;
        }
    }
}

// The slot of the class of `s` in a finished table: its representative, or
// SP_EMPTY when no instance has these words.
__device__ inline uint32_t split_find(const uint64_t *__restrict__ s, const uint64_t *__restrict__ splits, int W,
                                      const uint32_t *__restrict__ table, uint32_t mask)
{
    uint32_t slot = (uint32_t)split_hash(s, W) & mask;
    for (;;) {
        const uint32_t cur = table[slot];
        if (cur == SP_EMPTY || split_equal(splits + (uint64_t)cur * W, s, W)) return cur;
        slot = (slot + 1) & mask;
    }
}

// rep[i] = the representative of instance i's class (SP_EMPTY in an invalid
// replicate), flag[i] = 1 where i represents its class.
__global__ __launch_bounds__(256) void split_lookup_kernel(const uint64_t *__restrict__ splits,
                                                           const uint8_t *__restrict__ valid, uint32_t n_inst,
                                                           uint32_t ns, int W, const uint32_t *__restrict__ table,
                                                           uint32_t mask, uint32_t *__restrict__ rep,
                                                           uint32_t *__restrict__ flag)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_inst;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t idx = (uint32_t)i;
        uint32_t r = SP_EMPTY;
        if (valid[idx / ns]) r = split_find(splits + (uint64_t)idx * W, splits, W, table, mask);
        rep[idx] = r;
        flag[idx] = r == idx ? 1u : 0u;
    }
}

// ids[i] = rank[rep[i]] (-1 in an invalid replicate); count[id] += 1 (zeroed
// by the caller); the representative writes first[id].
__global__ __launch_bounds__(256) void split_id_kernel(const uint32_t *__restrict__ rep,
                                                       const uint32_t *__restrict__ rank, uint32_t n_inst,
                                                       int32_t *__restrict__ ids, uint32_t *count,
                                                       uint32_t *__restrict__ first)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_inst;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = rep[i];
        if (r == SP_EMPTY) {
            ids[i] = -1;
            continue;
        }
        const uint32_t id = rank[r];
        ids[i] = (int32_t)id;
        atomicAdd(&count[id], 1u);
        if (r == (uint32_t)i) first[id] = r;
    }
}

// out[k] = the W words of class k
__global__ __launch_bounds__(256) void split_gather_kernel(const uint64_t *__restrict__ splits,
                                                           const uint32_t *__restrict__ first, uint64_t K, int W,
                                                           uint64_t *__restrict__ out)
{
    const uint64_t n = K * (uint64_t)W;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = i / (uint64_t)W, w = i - k * (uint64_t)W;
        out[i] = splits[(uint64_t)first[k] * W + w];
    }
}

// isref[id] = 1 for every reference split that is a class of the census
// (isref zeroed by the caller; equal reference splits store the same byte)
__global__ __launch_bounds__(256) void split_ref_kernel(const uint64_t *__restrict__ ref, int n_ref,
                                                        const uint64_t *__restrict__ splits, int W,
                                                        const uint32_t *__restrict__ table, uint32_t mask,
                                                        const uint32_t *__restrict__ rank, uint8_t *isref)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_ref) return;
    const uint32_t r = split_find(ref + (uint64_t)k * W, splits, W, table, mask);
    if (r != SP_EMPTY) isref[rank[r]] = 1;
}

// to_ref[r] = n_ref + ns - 2 * |{t : isref[ids[r][t]]}|, one workgroup per
// replicate (RF_INVALID for an invalid one). A tree's ids are distinct.
__global__ __launch_bounds__(256) void rf_ref_kernel(const int32_t *__restrict__ ids,
                                                     const uint8_t *__restrict__ valid,
                                                     const uint8_t *__restrict__ isref, uint32_t ns, uint32_t n_ref,
                                                     uint32_t *__restrict__ to_ref)
{
    __shared__ uint32_t part[4];
    const uint32_t r = blockIdx.x;
    if (!valid[r]) {
        if (threadIdx.x == 0) to_ref[r] = RF_INVALID;
        return;
    }
    uint32_t hit = 0;
    for (uint32_t t = threadIdx.x; t < ns; t += blockDim.x) hit += isref[ids[(uint64_t)r * ns + t]];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) hit += __shfl_xor(hit, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = hit;
    __syncthreads();
    if (threadIdx.x == 0) to_ref[r] = n_ref + ns - 2 * (part[0] + part[1] + part[2] + part[3]);
}

constexpr int RF_WAVES = 4;

__device__ inline uint32_t rf_slot(uint32_t id, uint32_t hmask) { return (id * 2654435761u) >> 7 & hmask; }

// pairwise[a][b] = pairwise[b][a] = 2 * ns - 2 * |ids(a) & ids(b)| for b > a:
// workgroup a keeps ids(a) as a hash set in LDS (hcap slots, a power of two
// >= 2 * ns, so never more than half full), each wave streams the ids of one b
// at a time past it. Rows and columns of an invalid replicate are RF_INVALID,
// the diagonal of a valid one is 0.
__global__ __launch_bounds__(64 * RF_WAVES) void rf_pair_kernel(const int32_t *__restrict__ ids,
                                                               const uint8_t *__restrict__ valid, uint32_t R,
                                                               uint32_t ns, uint32_t hcap,
                                                               uint32_t *__restrict__ out)
{
    extern __shared__ uint32_t rf_set[];
    const uint32_t a = blockIdx.x, hmask = hcap - 1;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!valid[a]) {
        for (uint32_t b = threadIdx.x; b < R; b += blockDim.x) {
            out[(uint64_t)a * R + b] = RF_INVALID;
            out[(uint64_t)b * R + a] = RF_INVALID;
        }
        return;
    }
    for (uint32_t i = threadIdx.x; i < hcap; i += blockDim.x) rf_set[i] = SP_EMPTY;
    __syncthreads();
    const int32_t *mine = ids + (uint64_t)a * ns;
    for (uint32_t t = threadIdx.x; t < ns; t += blockDim.x) {
        const uint32_t id = (uint32_t)mine[t];
        uint32_t slot = rf_slot(id, hmask);
        while (atomicCAS(&rf_set[slot], SP_EMPTY, id) != SP_EMPTY) slot = (slot + 1) & hmask;
    }
    __syncthreads();
    if (threadIdx.x == 0) out[(uint64_t)a * R + a] = 0;
    for (uint32_t b = a + 1 + wave; b < R; b += RF_WAVES) {
        if (!valid[b]) continue;   // workgroup b writes its row and column
        const int32_t *theirs = ids + (uint64_t)b * ns;
        uint32_t hit = 0;
        for (uint32_t t = lane; t < ns; t += 64) {
            const uint32_t id = (uint32_t)theirs[t];
            uint32_t slot = rf_slot(id, hmask);
            for (;;) {
                const uint32_t cur = rf_set[slot];
                if (cur == id) {
                    hit++;
                    break;
                }
                if (cur == SP_EMPTY) break;
                slot = (slot + 1) & hmask;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) hit += __shfl_xor(hit, off);
        if (lane == 0) {
            const uint32_t d = 2 * ns - 2 * hit;
            out[(uint64_t)a * R + b] = d;
            out[(uint64_t)b * R + a] = d;
        }
    }
}

// ------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------

// slots of the table for n_inst instances: a power of two >= 2 * n_inst
uint64_t split_table_slots(uint64_t n_inst)
{
    uint64_t cap = 64;
    while (cap < 2 * n_inst) cap <<= 1;
    return cap;
}

// table: slots entries, all SP_EMPTY (0xFF bytes). n_inst < 2^31, ns >= 1.
void launch_split_insert(const uint64_t *splits, const uint8_t *valid, uint32_t n_inst, uint32_t ns, int W,
                         uint32_t *table, uint64_t slots, hipStream_t st)
{
    if (!n_inst) return;
    hipLaunchKernelGGL(split_insert_kernel, dim3(split_grid(n_inst, 256)), dim3(256), 0, st, splits, valid, n_inst, ns,
                       W, table, (uint32_t)(slots - 1));
}

void launch_split_lookup(const uint64_t *splits, const uint8_t *valid, uint32_t n_inst, uint32_t ns, int W,
                         const uint32_t *table, uint64_t slots, uint32_t *rep, uint32_t *flag, hipStream_t st)
{
    if (!n_inst) return;
    hipLaunchKernelGGL(split_lookup_kernel, dim3(split_grid(n_inst, 256)), dim3(256), 0, st, splits, valid, n_inst, ns,
                       W, table, (uint32_t)(slots - 1), rep, flag);
}

void launch_split_ids(const uint32_t *rep, const uint32_t *rank, uint32_t n_inst, int32_t *ids, uint32_t *count,
                      uint32_t *first, hipStream_t st)
{
    if (!n_inst) return;
    hipLaunchKernelGGL(split_id_kernel, dim3(split_grid(n_inst, 256)), dim3(256), 0, st, rep, rank, n_inst, ids, count,
                       first);
}

void launch_split_gather(const uint64_t *splits, const uint32_t *first, uint64_t K, int W, uint64_t *out,
                         hipStream_t st)
{
    if (!K) return;
    hipLaunchKernelGGL(split_gather_kernel, dim3(split_grid(K * (uint64_t)W, 256)), dim3(256), 0, st, splits, first, K,
                       W, out);
}

// isref: K bytes, zero
void launch_split_ref(const uint64_t *ref, int n_ref, const uint64_t *splits, int W, const uint32_t *table,
                      uint64_t slots, const uint32_t *rank, uint8_t *isref, hipStream_t st)
{
    if (n_ref < 1) return;
    hipLaunchKernelGGL(split_ref_kernel, dim3((unsigned)((n_ref + 255) / 256)), dim3(256), 0, st, ref, n_ref, splits, W,
                       table, (uint32_t)(slots - 1), rank, isref);
}

void launch_rf_ref(const int32_t *ids, const uint8_t *valid, const uint8_t *isref, uint32_t R, uint32_t ns,
                   uint32_t n_ref, uint32_t *to_ref, hipStream_t st)
{
    if (!R) return;
    hipLaunchKernelGGL(rf_ref_kernel, dim3(R), dim3(256), 0, st, ids, valid, isref, ns, n_ref, to_ref);
}

// out: R x R
void launch_rf_pairs(const int32_t *ids, const uint8_t *valid, uint32_t R, uint32_t ns, uint32_t *out, hipStream_t st)
{
    if (!R) return;
    uint32_t hcap = 64;
    while (hcap < 2 * ns) hcap <<= 1;
    hipLaunchKernelGGL(rf_pair_kernel, dim3(R), dim3(64 * RF_WAVES), hcap * sizeof(uint32_t), st, ids, valid, R, ns,
                       hcap, out);
}

}  // namespace rcg
