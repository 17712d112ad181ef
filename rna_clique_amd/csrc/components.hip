// Per-component tables of a finished graph phase and the resampling product
// over them (rc_ideal_components, rc_component_sums, rc_resample), and the
// census of every component (rc_components, rc_component_members; below).
//
// Component ids: the ideal components are numbered 0..C-1 in ascending order
// of their union-find root. cc_hook_kernel always hooks the larger root under
// the smaller, so after cc_compress_kernel a component's root is its lowest
// global gene index, ideal[v] is 1 exactly at the roots of ideal components,
// and the id of a component is the exclusive prefix sum of ideal[] at its
// root (the engine runs that scan with rocprim). This is NOT the reference's
// enumeration order: get_ideal_components follows graph insertion order.
//
// Attribution: a record counts iff ideal[parent[a]] && ideal[parent[b]], the
// test of pair_sums_kernel, and goes to the component of its b endpoint (the
// higher sample, the table's qsample/qgene: export_orthologs.py:679-684). A
// graph edge's endpoints agree; for an imported graph's sums-only record
// between two ideal components this rule decides. Node-only records add
// nothing. Summed over the components the table is rc_pair_sums exactly.
#include "device.h"
#include "launch.h"

#include <algorithm>

namespace rcg {

typedef unsigned long long ull;

static inline unsigned comp_grid(uint64_t n, unsigned block, unsigned cap = 65536)
{
    uint64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// Sort key of every gene: (component id << 32 | gene) for the members of ideal
// components, all ones for the rest. Sorted ascending, the first C * S keys
// are the members, component by component, in ascending gene index (ascending
// sample). counter[0] += members.
__global__ void comp_key_kernel(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ present,
                                const uint8_t *__restrict__ ideal, const uint32_t *__restrict__ rank, uint32_t n,
                                uint64_t *__restrict__ key, ull *counter)
{
    ull mine = 0;
    for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t k = ~0ull;
        if (present[v]) {
            const uint32_t r = parent[v];
            if (ideal[r]) {
                k = (uint64_t)rank[r] << 32 | v;
                mine++;
            }
        }
        key[v] = k;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(counter, mine);
}

// members[c * S + k] = gene of sorted key c * S + k; a key of another
// component there (a component without exactly S members) sets *bad.
__global__ void comp_member_kernel(const uint64_t *__restrict__ key, uint64_t n_members, uint32_t S,
                                   uint32_t *__restrict__ members, ull *bad)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_members;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = key[i];
        members[i] = (uint32_t)k;
        if ((k >> 32) != i / S) atomicOr(bad, 1ull);
    }
}

// One pass over the records: a qualifying record adds its sums to the cell
// (component of b, pair). Records arrive pair-major, so neighbouring lanes hit
// different components: plain 64-bit atomics.
__global__ void comp_sums_kernel(const DEdge *__restrict__ edges, uint64_t n_edges, const uint32_t *__restrict__ parent,
                                 const uint8_t *__restrict__ ideal, const uint32_t *__restrict__ rank, uint64_t P,
                                 ull *num, ull *den)
{
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < n_edges;
         e += (uint64_t)gridDim.x * blockDim.x) {
        const DEdge ed = edges[e];
        if (ed.pair == NODE_REC) continue;
        const uint32_t rb = parent[ed.b];
        if (!(ideal[parent[ed.a]] && ideal[rb])) continue;
        const uint64_t cell = (uint64_t)rank[rb] * P + (ed.pair & ~EDGE_SUM_ONLY);
        atomicAdd(&num[cell], (ull)ed.nident);
        atomicAdd(&den[cell], (ull)ed.den);
    }
}

// The cells as (num, den) 32-bit pairs for resample_kernel, and the largest
// cell (atomicMax of each wave's maximum). The packed copy is only used when
// that maximum is below 2^32.
__global__ void comp_pack_kernel(const ull *__restrict__ num, const ull *__restrict__ den, uint64_t n,
                                 uint2 *__restrict__ cells, ull *maxcell)
{
    ull m = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const ull a = num[i], b = den[i];
        cells[i] = make_uint2((uint32_t)a, (uint32_t)b);
        m = max(m, max(a, b));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (ull)__shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(maxcell, m);
}

// out[r][p] = sum over c of W[r][c] * S[c][p], for num and den at once.
//
// A lane owns one pair column, so a row of S is one coalesced 8-byte load per
// lane. A wave keeps RS_REPS replicates x (num, den) in registers; the block's
// RS_WAVES waves take RS_WAVES * RS_REPS consecutive replicates of the same
// 64 pairs. The block's weights of RS_CT components are staged in LDS
// transposed ([component][replicate]), so a wave reads its 8 weights of a
// component as one broadcast 16-byte read; they are made scalar, and a zero
// weight (about 37 % of bootstrap weights) skips its two multiply-adds.
// Cells are 32-bit and weights 16-bit: each multiply-add is one
// v_mad_u64_u32. The component range is cut into gridDim.z chunks whose
// partial sums meet in 64-bit atomicAdd: integers, so any split gives the
// same result.
constexpr int RS_REPS = 8, RS_WAVES = 4, RS_RT = RS_REPS * RS_WAVES, RS_CT = 128, RS_UNROLL = 4;

__global__ __launch_bounds__(64 * RS_WAVES) void resample_kernel(const uint2 *__restrict__ cells,
                                                                 const uint16_t *__restrict__ W, uint64_t C,
                                                                 uint64_t P, uint32_t R, uint32_t ptiles,
                                                                 uint64_t chunk, ull *out_num, ull *out_den)
{
    __shared__ uint4 wt[RS_CT * RS_WAVES];   // [component][wave]: 8 weights each
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t p = (uint64_t)(blockIdx.x % ptiles) * 64 + lane;
    const uint32_t r0 = (blockIdx.x / ptiles) * RS_RT;
    const uint64_t c_begin = blockIdx.z * chunk, c_end = c_begin + chunk < C ? c_begin + chunk : C;
    const bool live = p < P && r0 + wave * RS_REPS < R;
    ull num[RS_REPS], den[RS_REPS];
#pragma unroll
    for (int j = 0; j < RS_REPS; j++) num[j] = den[j] = 0;
    for (uint64_t c0 = c_begin; c0 < c_end; c0 += RS_CT) {
        __syncthreads();   // the previous tile's reads are done
        uint16_t *wl = reinterpret_cast<uint16_t *>(wt);
        for (int i = threadIdx.x; i < RS_CT * RS_RT; i += 64 * RS_WAVES) {
            const int rep = i / RS_CT, cc = i % RS_CT;
            const uint64_t r = (uint64_t)r0 + rep, c = c0 + cc;
            wl[cc * RS_RT + rep] = r < R && c < c_end ? W[r * C + c] : (uint16_t)0;
        }
        __syncthreads();
        const int nc = c_end - c0 < (uint64_t)RS_CT ? (int)(c_end - c0) : RS_CT;
        for (int cc = 0; cc < nc; cc += RS_UNROLL) {
            uint2 s[RS_UNROLL];
#pragma unroll
            for (int u = 0; u < RS_UNROLL; u++)
                s[u] = live && cc + u < nc ? cells[(c0 + cc + u) * P + p] : make_uint2(0u, 0u);
#pragma unroll
            for (int u = 0; u < RS_UNROLL; u++) {
                // rows past nc hold zero weights (RS_CT is a multiple of RS_UNROLL)
                const uint4 w4 = wt[(cc + u) * RS_WAVES + wave];
                const uint32_t wd[4] = {(uint32_t)__builtin_amdgcn_readfirstlane((int)w4.x),
                                        (uint32_t)__builtin_amdgcn_readfirstlane((int)w4.y),
                                        (uint32_t)__builtin_amdgcn_readfirstlane((int)w4.z),
                                        (uint32_t)__builtin_amdgcn_readfirstlane((int)w4.w)};
#pragma unroll
                for (int j = 0; j < RS_REPS; j++) {
                    const uint32_t w = (wd[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
                    if (w) {
                        num[j] += (ull)w * s[u].x;
                        den[j] += (ull)w * s[u].y;
                    }
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < RS_REPS; j++) {
        const uint64_t r = (uint64_t)r0 + wave * RS_REPS + j;
        if (r < R && (num[j] | den[j])) {
            atomicAdd(&out_num[r * P + p], num[j]);
            atomicAdd(&out_den[r * P + p], den[j]);
        }
    }
}

// distance_kernel's formula over R replicates: out[r][i][j] for order[M],
// 0 on the diagonal, NaN and ST_NO_IDEAL where a denominator is 0
__global__ void resample_distance_kernel(const ull *__restrict__ num, const ull *__restrict__ den,
                                         const int32_t *__restrict__ pair_index, const int32_t *__restrict__ order,
                                         int N, int M, uint64_t R, uint64_t P, double *__restrict__ out,
                                         unsigned int *status)
{
    const uint64_t mm = (uint64_t)M * M, n = R * mm;
    bool nan = false;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = t / mm;
        const uint32_t ij = (uint32_t)(t - r * mm);
        const int a = order[ij / M], b = order[ij % M];
        double d = 0.0;
        if (a != b) {
            const uint64_t cell = r * P + pair_index[a * N + b];
            const ull dn = den[cell], nm = num[cell];
            if (dn == 0) {
                d = __builtin_nan("");
                nan = true;
            } else {
                d = (double)(long long)(dn - nm) / (double)(long long)dn;
            }
        }
        out[t] = d;
    }
    if (__any(nan) && (threadIdx.x & 63) == 0) atomicOr(status, ST_NO_IDEAL);
}

// ------------------------------------------------------------------------
// component census (rc_components, rc_component_members)
//
// Every connected component over the present genes, numbered 0..K-1 in
// ascending order of its root (its lowest global gene index): the census id of
// a root is the exclusive prefix sum of census_flag_kernel's flag. These
// kernels only read what the graph phase left (parent, present, cnodes,
// cedges, gene_sample).
// ------------------------------------------------------------------------

// flag[v] = 1 at the root of a component of present genes
__global__ void census_flag_kernel(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ present,
                                   uint32_t n, uint32_t *__restrict__ flag)
{
    for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x)
        flag[v] = parent[v] == v && present[v] ? 1u : 0u;
}

// comp_key_kernel for every present gene: (census id << 32 | gene), all ones
// for the absent ones. Sorted ascending, the first n_present keys are the
// members, component by component, in ascending gene index. counter[0] +=
// present genes.
__global__ void census_key_kernel(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ present,
                                  const uint32_t *__restrict__ rank, uint32_t n, uint64_t *__restrict__ key,
                                  ull *counter)
{
    ull mine = 0;
    for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t k = ~0ull;
        if (present[v]) {
            k = (uint64_t)rank[parent[v]] << 32 | v;
            mine++;
        }
        key[v] = k;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(counter, mine);
}

// The table's gathered columns, one thread per gene: a root scatters itself,
// cnodes and cedges to its census id. samples[] is zeroed here for
// census_member_kernel.
__global__ void census_table_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank,
                                    const uint32_t *__restrict__ cnodes, const uint32_t *__restrict__ cedges,
                                    uint32_t n, uint32_t *__restrict__ root, uint32_t *__restrict__ nodes,
                                    uint32_t *__restrict__ edges, uint32_t *__restrict__ samples)
{
    for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
        if (!flag[v]) continue;
        const uint32_t c = rank[v];
        root[c] = (uint32_t)v;
        nodes[c] = cnodes[v];
        edges[c] = cedges[v];
        samples[c] = 0;
    }
}

// One pass over the sorted members: members[i] = gene of key i, and
// samples[c] += 1 for every member that is the first of its sample in its
// component -- it opens the component's slice, or its predecessor is of
// another sample (genes are numbered sample-major, so a component's members
// are in ascending sample). A component gets one atomic per sample it holds,
// whatever its size: a giant component is as cheap as a small one. Integer
// sums: the result does not depend on the order of the atomics.
__global__ void census_member_kernel(const uint64_t *__restrict__ key, uint64_t n_members,
                                     const int32_t *__restrict__ gene_sample, uint32_t *__restrict__ members,
                                     uint32_t *samples)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_members;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = key[i];
        const uint32_t v = (uint32_t)k, c = (uint32_t)(k >> 32);
        members[i] = v;
        bool first = i == 0;
        if (!first) {
            const uint64_t kp = key[i - 1];
            first = (uint32_t)(kp >> 32) != c || gene_sample[(uint32_t)kp] != gene_sample[v];
        }
        if (first) atomicAdd(&samples[c], 1u);
    }
}

// ------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------

void launch_census_flags(const uint32_t *parent, const uint32_t *present, uint32_t n, uint32_t *flag, hipStream_t st)
{
    if (!n) return;
    hipLaunchKernelGGL(census_flag_kernel, dim3(comp_grid(n, 256)), dim3(256), 0, st, parent, present, n, flag);
}

void launch_census_keys(const uint32_t *parent, const uint32_t *present, const uint32_t *rank, uint32_t n,
                        uint64_t *key, ull *counter, hipStream_t st)
{
    if (!n) return;
    hipLaunchKernelGGL(census_key_kernel, dim3(comp_grid(n, 256)), dim3(256), 0, st, parent, present, rank, n, key,
                       counter);
}

void launch_census_table(const uint32_t *flag, const uint32_t *rank, const uint32_t *cnodes, const uint32_t *cedges,
                         uint32_t n, uint32_t *root, uint32_t *nodes, uint32_t *edges, uint32_t *samples,
                         hipStream_t st)
{
    if (!n) return;
    hipLaunchKernelGGL(census_table_kernel, dim3(comp_grid(n, 256)), dim3(256), 0, st, flag, rank, cnodes, cedges, n,
                       root, nodes, edges, samples);
}

void launch_census_members(const uint64_t *key, uint64_t n_members, const int32_t *gene_sample, uint32_t *members,
                           uint32_t *samples, hipStream_t st)
{
    if (!n_members) return;
    hipLaunchKernelGGL(census_member_kernel, dim3(comp_grid(n_members, 256)), dim3(256), 0, st, key, n_members,
                       gene_sample, members, samples);
}

void launch_comp_keys(const uint32_t *parent, const uint32_t *present, const uint8_t *ideal, const uint32_t *rank,
                      uint32_t n, uint64_t *key, ull *counter, hipStream_t st)
{
    if (!n) return;
    hipLaunchKernelGGL(comp_key_kernel, dim3(comp_grid(n, 256)), dim3(256), 0, st, parent, present, ideal, rank, n,
                       key, counter);
}

void launch_comp_members(const uint64_t *key, uint64_t n_members, uint32_t S, uint32_t *members, ull *bad,
                         hipStream_t st)
{
    if (!n_members) return;
    hipLaunchKernelGGL(comp_member_kernel, dim3(comp_grid(n_members, 256)), dim3(256), 0, st, key, n_members, S,
                       members, bad);
}

void launch_comp_sums(const DEdge *edges, uint64_t n_edges, const uint32_t *parent, const uint8_t *ideal,
                      const uint32_t *rank, uint64_t P, ull *num, ull *den, hipStream_t st)
{
    if (!n_edges) return;
    hipLaunchKernelGGL(comp_sums_kernel, dim3(comp_grid(n_edges, 256)), dim3(256), 0, st, edges, n_edges, parent,
                       ideal, rank, P, num, den);
}

void launch_comp_pack(const ull *num, const ull *den, uint64_t n, uint2 *cells, ull *maxcell, hipStream_t st)
{
    if (!n) return;
    hipLaunchKernelGGL(comp_pack_kernel, dim3(comp_grid(n, 256, 8192)), dim3(256), 0, st, num, den, n, cells,
                       maxcell);
}

// out_num / out_den (R x P) must be zero. Returns false when the grid does not
// fit (R x P beyond 2^31 - 1 tiles of 64 pairs x 32 replicates).
bool launch_resample(const uint2 *cells, const uint16_t *W, uint64_t C, uint64_t P, uint32_t R, ull *out_num,
                     ull *out_den, hipStream_t st)
{
    if (!C || !P || !R) return true;
    const uint64_t ptiles = (P + 63) / 64, rtiles = ((uint64_t)R + RS_RT - 1) / RS_RT;
    if (ptiles * rtiles > 0x7FFFFFFFull) return false;
    // enough blocks to fill the device a few times over, in whole weight tiles
    const uint64_t tiles_c = (C + RS_CT - 1) / RS_CT;
    uint64_t chunks = (2048 + ptiles * rtiles - 1) / (ptiles * rtiles);
    chunks = std::min<uint64_t>(std::min<uint64_t>(chunks, tiles_c), 65535);
    const uint64_t chunk = (tiles_c + chunks - 1) / chunks * RS_CT;
    chunks = (C + chunk - 1) / chunk;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(ptiles * rtiles), 1, (unsigned)chunks), dim3(64 * RS_WAVES), 0,
                       st, cells, W, C, P, R, (uint32_t)ptiles, chunk, out_num, out_den);
    return true;
}

void launch_resample_distance(const ull *num, const ull *den, const int32_t *pair_index, const int32_t *order, int N,
                              int M, uint64_t R, uint64_t P, double *out, unsigned int *status, hipStream_t st)
{
    const uint64_t n = R * (uint64_t)M * M;
    if (!n) return;
    hipLaunchKernelGGL(resample_distance_kernel, dim3(comp_grid(n, 256)), dim3(256), 0, st, num, den, pair_index,
                       order, N, M, R, P, out, status);
}

}  // namespace rcg
