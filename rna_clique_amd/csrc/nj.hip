// Neighbour-joining trees of replicate distance matrices and the support of
// reference splits among them (rc_nj, rc_resample_trees).
//
// The algorithm and its operation order are those of tests/nj_oracle.py, which
// the kernel reproduces bit for bit (float64, -ffp-contract=off):
//   r[i]   = D[0][i] + D[1][i] + ... + D[n-1][i], left to right
//   q(i,j) = ((double)(n - 2) * D[i][j] - r[i]) - r[j], i < j; the minimum in
//            the total order (q, i, j)
//   li     = 0.5 * D[i][j] + (r[i] - r[j]) / (2.0 * (n - 2)), lj = D[i][j] - li
//   new[k] = 0.5 * ((D[i][k] + D[j][k]) - D[i][j]) into slot i; slot n - 1
//            moves into slot j
//
// nj_kernel: one workgroup per replicate, lane t owns slot (column) t. The
// symmetric matrix is walked by columns (D[k][t] for lane t: consecutive lanes,
// consecutive addresses), never by rows. Up to RC_NJ_LDS (128) samples the matrix
// and the leaf masks live in LDS; above that, the same code runs with both in
// a per-replicate global workspace (r, node ids and the reduction stay in LDS).
#include "device.h"
#include "launch.h"

#include <algorithm>

namespace rcg {

constexpr int NJ_MAX_WAVES = 16;   // 1024 samples

// dynamic LDS of nj_kernel: [matrix N x N][masks N x W] on the LDS path, then
// r[N], red_q[16], node[N], red_i[16], red_j[16]
size_t nj_lds_bytes(bool lds, int N, int W)
{
    size_t b = (size_t)N * 8 + NJ_MAX_WAVES * 8 + (size_t)N * 4 + 2 * NJ_MAX_WAVES * 4;
    if (lds) b += (size_t)N * N * 8 + (size_t)N * W * 8;
    return (b + 15) & ~(size_t)15;
}

__device__ inline bool nj_less(double qa, int ia, int ja, double qb, int ib, int jb)
{
    return qa < qb || (qa == qb && (ia < ib || (ia == ib && ja < jb)));
}

// D: the block's replicates, N x N each (only i < j is read). ws_m / ws_mask:
// the workspace of the global path (one N x N matrix and N x W mask words per
// block). Outputs are indexed by blockIdx.x like D.
template <bool LDS>
__global__ __launch_bounds__(LDS ? 128 : 1024) void nj_kernel(const double *__restrict__ D, int N, int W,
                                                              double *ws_m, uint64_t *ws_mask,
                                                              int32_t *__restrict__ joins,
                                                              double *__restrict__ lengths,
                                                              uint64_t *__restrict__ splits,
                                                              uint8_t *__restrict__ valid)
{
    extern __shared__ double nj_smem[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const uint64_t rep = blockIdx.x;
    double *M, *r;
    uint64_t *mask;
    if (LDS) {
        M = nj_smem;
        mask = reinterpret_cast<uint64_t *>(M + (size_t)N * N);
        r = reinterpret_cast<double *>(mask + (size_t)N * W);
    } else {
        M = ws_m + rep * (uint64_t)N * N;
        mask = ws_mask + rep * (uint64_t)N * W;
        r = nj_smem;
    }
    double *red_q = r + N;
    int *node = reinterpret_cast<int *>(red_q + NJ_MAX_WAVES);
    int *red_i = node + N, *red_j = red_i + NJ_MAX_WAVES;

    // load: mirror the upper triangle, zero diagonal; any non-finite entry
    // there makes the replicate invalid
    const double *Dr = D + rep * (uint64_t)N * N;
    const uint32_t nn = (uint32_t)N * (uint32_t)N;
    int bad = 0;
    for (uint32_t idx = tid; idx < nn; idx += nt) {
        const uint32_t i = idx / (uint32_t)N, j = idx - i * (uint32_t)N;
        if (i < j) {
            const double v = Dr[idx];
            bad |= !__builtin_isfinite(v);
            M[idx] = v;
            M[j * (uint32_t)N + i] = v;
        } else if (i == j) {
            M[idx] = 0.0;
        }
    }
    for (uint32_t idx = tid; idx < (uint32_t)(N * W); idx += nt) {
        const uint32_t s = idx / (uint32_t)W, w = idx - s * (uint32_t)W;
        mask[idx] = (s >> 6) == w ? 1ull << (s & 63) : 0ull;
    }
    if (tid < N) node[tid] = tid;
    bad = __syncthreads_or(bad);

    int32_t *jo = joins + rep * (uint64_t)(N - 2) * 3;
    double *le = lengths + rep * (uint64_t)(N - 2) * 3;
    uint64_t *sp = splits + rep * (uint64_t)(N - 3) * W;
    if (bad) {
        for (int idx = tid; idx < (N - 2) * 3; idx += nt) {
            jo[idx] = -1;
            le[idx] = __builtin_nan("");
        }
        for (int idx = tid; idx < (N - 3) * W; idx += nt) sp[idx] = 0ull;
        if (tid == 0) valid[rep] = 0;
        return;
    }

    const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    // bits of word `tid` that lie below N (the complement stays within N bits)
    const uint64_t tail = (tid == W - 1 && (N & 63)) ? (1ull << (N & 63)) - 1 : ~0ull;
    int n = N;
    while (n > 3) {
        // 1. column sums, ascending k
        if (tid < n) {
            double s = M[tid];
#pragma unroll 8
            for (int k = 1; k < n; k++) s += M[k * N + tid];   // the loads run ahead of the serial adds
            r[tid] = s;
        }
        __syncthreads();
        // 2. lane t scans column t above the diagonal (ascending i, so the
        // first minimum is the lowest i); then the minimum over the lanes
        double bq = __builtin_inf();
        int bi = 0x7FFFFFFF, bj = 0x7FFFFFFF;
        if (tid < n) {
            const double rt = r[tid], f = (double)(n - 2);
#pragma unroll 4
            for (int i = 0; i < tid; i++) {
                const double q = (f * M[i * N + tid] - r[i]) - rt;
                if (q < bq) {
                    bq = q;
                    bi = i;
                }
            }
            if (bi != 0x7FFFFFFF) bj = tid;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double oq = __shfl_xor(bq, off);
            const int oi = __shfl_xor(bi, off), oj = __shfl_xor(bj, off);
            if (nj_less(oq, oi, oj, bq, bi, bj)) {
                bq = oq;
                bi = oi;
                bj = oj;
            }
        }
        if (nw > 1) {
            if (lane == 0) {
                red_q[wave] = bq;
                red_i[wave] = bi;
                red_j[wave] = bj;
            }
            __syncthreads();
            bq = red_q[0];
            bi = red_i[0];
            bj = red_j[0];
            for (int w = 1; w < nw; w++) {
                const double oq = red_q[w];
                const int oi = red_i[w], oj = red_j[w];
                if (nj_less(oq, oi, oj, bq, bi, bj)) {
                    bq = oq;
                    bi = oi;
                    bj = oj;
                }
            }
        }
        // no q compared below +inf (every q NaN or +inf: sums that overflowed)
        if ((unsigned)bi >= (unsigned)n || (unsigned)bj >= (unsigned)n || bi >= bj) {
            bi = 0;
            bj = 1;
        }
        // 3, 4. the join's record
        const double dij = M[bi * N + bj];
        const int t = N - n;
        if (tid == 0) {
            const double li = 0.5 * dij + (r[bi] - r[bj]) / (2.0 * (double)(n - 2));
            jo[t * 3 + 0] = node[bi];
            jo[t * 3 + 1] = node[bj];
            jo[t * 3 + 2] = -1;
            le[t * 3 + 0] = li;
            le[t * 3 + 1] = dij - li;
            le[t * 3 + 2] = 0.0;
        }
        if (tid < W) {
            const uint64_t m = mask[bi * W + tid] | mask[bj * W + tid];
            const bool flip = (mask[bi * W] | mask[bj * W]) & 1ull;
            sp[t * W + tid] = flip ? ~m & tail : m;
        }
        // 5. the new row into slot i (lane k owns cells (i, k) and (k, i))
        if (tid < n && tid != bi && tid != bj) {
            const double v = 0.5 * ((M[bi * N + tid] + M[bj * N + tid]) - dij);
            M[bi * N + tid] = v;
            M[tid * N + bi] = v;
        }
        __syncthreads();   // the join's reads of node / mask / r are done; row i is written
        if (bj != n - 1 && tid < n - 1 && tid != bj) {
            const double v = M[(n - 1) * N + tid];
            M[bj * N + tid] = v;
            M[tid * N + bj] = v;
        }
        if (tid < W) {
            mask[bi * W + tid] |= mask[bj * W + tid];
            if (bj != n - 1) mask[bj * W + tid] = mask[(n - 1) * W + tid];
        }
        if (tid == 0) {
            node[bi] = N + t;
            if (bj != n - 1) node[bj] = node[n - 1];
        }
        __syncthreads();
        n--;
    }
    if (tid == 0) {
        const double d01 = M[1], d02 = M[2], d12 = M[N + 2];
        const int t = N - 3;
        jo[t * 3 + 0] = node[0];
        jo[t * 3 + 1] = node[1];
        jo[t * 3 + 2] = node[2];
        le[t * 3 + 0] = 0.5 * ((d01 + d02) - d12);
        le[t * 3 + 1] = 0.5 * ((d01 + d12) - d02);
        le[t * 3 + 2] = 0.5 * ((d02 + d12) - d01);
        valid[rep] = 1;
    }
}

// support[k] += 1 for every valid replicate whose ns splits include reference
// split k; *n_valid += valid replicates. One workgroup per replicate, a thread
// per reference split.
__global__ __launch_bounds__(128) void nj_support_kernel(const uint64_t *__restrict__ ref, int n_ref,
                                                         const uint64_t *__restrict__ splits,
                                                         const uint8_t *__restrict__ valid, int R, int ns, int W,
                                                         uint32_t *support, uint32_t *n_valid)
{
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        if (!valid[r]) continue;
        if (threadIdx.x == 0) atomicAdd(n_valid, 1u);
        const uint64_t *sp = splits + (uint64_t)r * ns * W;
        for (int k = threadIdx.x; k < n_ref; k += blockDim.x) {
            bool found = false;
            for (int s = 0; s < ns && !found; s++) {
                bool eq = true;
                for (int w = 0; w < W; w++) eq = eq && sp[(uint64_t)s * W + w] == ref[(uint64_t)k * W + w];
                found = eq;
            }
            if (found) atomicAdd(&support[k], 1u);
        }
    }
}

// ------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------

// R replicates of N samples. lds: the LDS path (the caller has checked that
// nj_lds_bytes(true, N, W) fits the device and N <= 128); else ws_m / ws_mask
// hold R matrices and mask sets.
hipError_t launch_nj(bool lds, const double *D, int R, int N, int W, double *ws_m, uint64_t *ws_mask, int32_t *joins,
                     double *lengths, uint64_t *splits, uint8_t *valid, hipStream_t st)
{
    if (R < 1) return hipSuccess;
    const size_t bytes = nj_lds_bytes(lds, N, W);
    const unsigned block = (unsigned)((N + 63) / 64 * 64);
    hipError_t err;
    if (lds) {
        err = hipFuncSetAttribute(reinterpret_cast<const void *>(&nj_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL(nj_kernel<true>, dim3((unsigned)R), dim3(block), bytes, st, D, N, W, ws_m, ws_mask, joins,
                           lengths, splits, valid);
    } else {
        hipLaunchKernelGGL(nj_kernel<false>, dim3((unsigned)R), dim3(block), bytes, st, D, N, W, ws_m, ws_mask, joins,
                           lengths, splits, valid);
    }
    return hipGetLastError();
}

void launch_nj_support(const uint64_t *ref, int n_ref, const uint64_t *splits, const uint8_t *valid, int R, int ns,
                       int W, uint32_t *support, uint32_t *n_valid, hipStream_t st)
{
    if (R < 1) return;
    hipLaunchKernelGGL(nj_support_kernel, dim3((unsigned)std::min(R, 65536)), dim3(128), 0, st, ref, n_ref, splits,
                       valid, R, ns, W, support, n_valid);
}

}  // namespace rcg
