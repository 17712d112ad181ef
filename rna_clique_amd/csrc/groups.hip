// Group tests on replicate distance matrices: PERMANOVA (pseudo-F) and ANOSIM
// (R) with label permutations (rc_group_test, rc_resample_group_test).
//
// The algorithm is that of tests/group_oracle.py (float64, -ffp-contract=off;
// of matrix D[n][n] only i < j is read, mirrored, zero diagonal):
//   PERMANOVA  v[i][j] = D[i][j] * D[i][j]
//   ANOSIM     v[i][j] = 2 * (average rank of D[i][j] among the M = n (n - 1) / 2
//              distances) = 2 #{d < D[i][j]} + #{d == D[i][j]} + 1, an integer
//   t[i]  = sum over j = 0, 1, ... ascending of (g[j] == g[i] ? v[j][i] : 0)
//   x[i]  = t[i] / (2.0 * n_g[i])  (PERMANOVA; n_g[i] = members of i's group)
//         = t[i]                   (ANOSIM, integers)
//   S(g)  = the sum of x padded with zeros to a power of two, halved until one
//           value is left: x[0:h] + x[h:2h] elementwise, h = 64, 32, ..., 1
// S depends on the partition that g describes and on nothing else: renumbered
// groups and members exchanged inside a group give the same bits. SS_W = S(g),
// SS_T = S(one group of everything), W2 = S(g) / 2.
//
// group_rank_kernel: the twice-ranks of one replicate by counting, 1024
// distances per workgroup against all M in LDS (integer-exact, no sort).
// group_kernel: a workgroup stages v of one replicate in LDS, element (row j,
// column i) at j * ld + i, so that lane i reads column i -- row i of the
// symmetric matrix -- at consecutive addresses. A wave evaluates GROUP_Q label
// vectors per pass over the matrix (one LDS read serves all of them); the label
// of row j comes out of lane j's register with v_readlane. Every wave
// evaluates the one-group vector and the observed labels first, with the code
// path of its permutations, so the bits it compares with are its own. Counts
// leave the workgroup as one integer atomic per wave; there is no
// floating-point atomic, and a replicate's bits do not depend on the grid.
#include "device.h"
#include "launch.h"

namespace rcg {

enum {
    GROUP_THREADS = 256,      // 4 waves
    GROUP_Q = 4,              // label vectors per pass over the matrix
    GROUP_WAVE_PERMS = 30,    // permutations per wave: with the two vectors every wave adds, 8 passes
    RANK_THREADS = 256,
    RANK_PER_THREAD = 4,      // distances ranked per thread: 1024 per workgroup
    NO_LABEL = 0xFF           // the label of a lane without a row: equal to no sample's (labels < 127)
};
static_assert(GROUP_PERM_CHUNK == (GROUP_THREADS / 64) * GROUP_WAVE_PERMS, "a workgroup's permutations");
static_assert((GROUP_WAVE_PERMS + 2) % GROUP_Q == 0, "whole passes");

static int group_ld(int n) { return n <= 64 ? 64 : 128; }

size_t group_lds_bytes(int method, int n) { return (size_t)n * group_ld(n) * (method == GROUP_ANOSIM ? 4 : 8); }

size_t group_rank_lds_bytes(int n)
{
    const size_t M = (size_t)n * (n - 1) / 2;
    return M * 8 + (M * 2 + 7) / 8 * 8;
}

// ------------------------------------------------------------------------
// ranks
// ------------------------------------------------------------------------

// rk2[rep][i][j] = twice the average rank of D[rep][i][j] among the replicate's
// M distances (symmetric, zero diagonal); valid[rep] = 0 and rk2 untouched for a
// replicate with a non-finite entry above its diagonal. Workgroup kb of a
// replicate ranks distances [1024 kb, 1024 (kb + 1)).
__global__ __launch_bounds__(RANK_THREADS) void group_rank_kernel(const double *__restrict__ D, int n, int nkb,
                                                                  uint32_t *__restrict__ rk2, uint8_t *__restrict__ valid)
{
    extern __shared__ double rank_x[];   // [M] distances in row-major order of (i < j), then [M] (i << 8 | j)
    const int tid = threadIdx.x;
    const uint32_t M = (uint32_t)n * (uint32_t)(n - 1) / 2, nn = (uint32_t)n * (uint32_t)n;
    uint16_t *ij = reinterpret_cast<uint16_t *>(rank_x + M);
    const uint64_t rep = blockIdx.x / (uint32_t)nkb;
    const uint32_t kb = blockIdx.x % (uint32_t)nkb;
    const double *Dr = D + rep * nn;
    uint32_t *out = rk2 + rep * nn;

    int bad = 0;
    for (uint32_t idx = tid; idx < nn; idx += RANK_THREADS) {
        const uint32_t i = idx / (uint32_t)n, j = idx - i * (uint32_t)n;
        if (i < j) {
            const uint32_t k = i * (2u * n - i - 1u) / 2u + (j - i - 1u);
            const double v = Dr[idx];
            bad |= !__builtin_isfinite(v);
            rank_x[k] = v;
            ij[k] = (uint16_t)(i << 8 | j);
        }
    }
    bad = __syncthreads_or(bad);
    if (kb == 0 && tid == 0) valid[rep] = bad ? 0 : 1;
    if (bad) return;
    if (kb == 0 && tid < n) out[(uint32_t)tid * n + tid] = 0;

    const uint32_t k0 = kb * (RANK_THREADS * RANK_PER_THREAD) + tid;
    double dk[RANK_PER_THREAD];
    uint32_t lt[RANK_PER_THREAD], le[RANK_PER_THREAD];
#pragma unroll
    for (int u = 0; u < RANK_PER_THREAD; u++) {
        const uint32_t k = k0 + u * RANK_THREADS;
        dk[u] = rank_x[k < M ? k : 0];
        lt[u] = le[u] = 0;
    }
    for (uint32_t m = 0; m < M; m++) {
        const double x = rank_x[m];   // the same address in every lane: a broadcast
#pragma unroll
        for (int u = 0; u < RANK_PER_THREAD; u++) {
            lt[u] += x < dk[u];
            le[u] += x <= dk[u];
        }
    }
#pragma unroll
    for (int u = 0; u < RANK_PER_THREAD; u++) {
        const uint32_t k = k0 + u * RANK_THREADS;
        if (k < M) {
            const uint32_t i = ij[k] >> 8, j = ij[k] & 255u;
            const uint32_t r2 = lt[u] + le[u] + 1u;   // le counts the distance itself
            out[i * n + j] = r2;
            out[j * n + i] = r2;
        }
    }
}

// ------------------------------------------------------------------------
// the tests
// ------------------------------------------------------------------------

__device__ inline double wave_sum(double v)
{
    // xor butterfly: x[0:h] + x[h:2h] for h = 32 .. 1; addition commutes, so every lane ends with the same bits
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ inline uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// What a test makes of S: PERMANOVA's F from SS_T and SS_W, ANOSIM's R from W2.
struct GroupShape {
    int n, a;
    uint32_t M, mW;   // pairs, within-group pairs
};

__device__ inline double group_stat(const GroupShape &s, double sst, double ssw)
{
    return ((sst - ssw) / (double)(s.a - 1)) / (ssw / (double)(s.n - s.a));
}

__device__ inline double group_stat(const GroupShape &s, uint32_t tot2, uint32_t w22)
{
    const uint32_t w2 = w22 / 2u, all = tot2 / 2u;   // all = M (M + 1)
    const double rw = (double)w2 / (double)(2u * s.mW);
    const double rb = (double)(all - w2) / (double)(2u * (s.M - s.mW));
    return (rb - rw) / ((double)s.M / 2.0);
}

// T = double: PERMANOVA on D; sets valid. T = uint32_t: ANOSIM on the
// twice-ranks in src (valid_in: group_rank_kernel's verdict; valid is left
// alone and may be the same array). ROWS: rows per lane (n <= 64 ROWS).
// Workgroup (rep, chunk) = blockIdx.x / nchunk, % nchunk; its wave w takes
// permutations [chunk * GROUP_PERM_CHUNK + w * GROUP_WAVE_PERMS, + GROUP_WAVE_PERMS).
// n_ge must be zero on entry.
template <typename T, int ROWS>
__global__ __launch_bounds__(GROUP_THREADS) void group_kernel(const T *__restrict__ src, const uint8_t *valid_in,
                                                              GroupShape shape, const uint8_t *__restrict__ labels,
                                                              const uint8_t *__restrict__ perm, int P, int nchunk,
                                                              double *__restrict__ stat, uint32_t *n_ge,
                                                              double *__restrict__ total, double *__restrict__ within,
                                                              double *__restrict__ perm_stat, uint8_t *valid)
{
    extern __shared__ double group_lds[];
    __shared__ uint32_t s_cnt[128];
    constexpr bool F64 = sizeof(T) == 8;
    constexpr int ld = 64 * ROWS;
    T *V = reinterpret_cast<T *>(group_lds);
    const int tid = threadIdx.x, n = shape.n;
    const uint32_t nn = (uint32_t)n * (uint32_t)n;
    const uint64_t rep = blockIdx.x / (uint32_t)nchunk;
    const int chunk = (int)(blockIdx.x % (uint32_t)nchunk);
    const T *Sr = src + rep * nn;

    // stage v, count the groups
    if (tid < 128) s_cnt[tid] = 0;
    int bad = 0;
    if (F64) {
        for (uint32_t idx = tid; idx < nn; idx += GROUP_THREADS) {
            const uint32_t i = idx / (uint32_t)n, j = idx - i * (uint32_t)n;
            if (i < j) {
                const double d = (double)Sr[idx];
                bad |= !__builtin_isfinite(d);
                const T v = (T)(d * d);
                V[j * ld + i] = v;
                V[i * ld + j] = v;
            } else if (i == j) {
                V[i * ld + i] = (T)0;
            }
        }
    } else {
        bad = !valid_in[rep];
        if (!bad) {
            for (uint32_t idx = tid; idx < nn; idx += GROUP_THREADS) {
                const uint32_t i = idx / (uint32_t)n, j = idx - i * (uint32_t)n;
                V[i * ld + j] = Sr[idx];
            }
        }
    }
    for (uint32_t idx = tid; idx < (uint32_t)n * (ld - n); idx += GROUP_THREADS) {   // the columns no sample owns
        const uint32_t j = idx / (uint32_t)(ld - n), i = n + (idx - j * (uint32_t)(ld - n));
        V[j * ld + i] = (T)0;
    }
    bad = __syncthreads_or(bad);
    if (tid < n) atomicAdd(&s_cnt[labels[tid]], 1u);
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    const int64_t p0 = (int64_t)chunk * GROUP_PERM_CHUNK + wave * GROUP_WAVE_PERMS;
    const int64_t pend = p0 + GROUP_WAVE_PERMS < P ? p0 + GROUP_WAVE_PERMS : P;
    double *pst = perm_stat ? perm_stat + rep * (uint64_t)P : nullptr;
    if (bad) {
        if (pst && lane < 32)
            for (int64_t p = p0 + lane; p < pend; p += 32) pst[p] = __builtin_nan("");
        if (chunk == 0 && tid == 0) {
            stat[rep] = total[rep] = within[rep] = __builtin_nan("");
            if (F64) valid[rep] = 0;
        }
        return;
    }

    uint32_t gobs[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) gobs[r] = lane + 64 * r < n ? labels[lane + 64 * r] : NO_LABEL;
    T raw_all = (T)0, raw_obs = (T)0;
    double fobs = 0.0;
    uint32_t count = 0;
    for (int b = 0; b * GROUP_Q < GROUP_WAVE_PERMS + 2; b++) {
        // slot 0: one group of everything; slot 1: the observed labels; slot s: permutation p0 + s - 2
        uint32_t g[GROUP_Q][ROWS];
        T t[GROUP_Q][ROWS];
#pragma unroll
        for (int q = 0; q < GROUP_Q; q++) {
            const int s = b * GROUP_Q + q;
            const int64_t p = p0 + s - 2;
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const int row = lane + 64 * r;
                g[q][r] = gobs[r];
                if (s == 0)
                    g[q][r] = row < n ? 0u : NO_LABEL;
                else if (s > 1 && p < pend && row < n)
                    g[q][r] = perm[p * n + row];
                t[q][r] = (T)0;
            }
        }
#pragma unroll
        for (int h = 0; h < ROWS; h++) {   // rows j = 64 h .. of the matrix: their labels sit in g[.][h]
            const int jn = n - 64 * h < 64 ? n - 64 * h : 64;
            const T *col = V + 64 * h * ld + lane;
            auto add_row = [&](int j, const T *v) {   // row 64 h + j of the matrix, ascending j
#pragma unroll
                for (int q = 0; q < GROUP_Q; q++) {
                    const uint32_t gj = (uint32_t)__builtin_amdgcn_readlane((int)g[q][h], j);
#pragma unroll
                    for (int r = 0; r < ROWS; r++) t[q][r] += g[q][r] == gj ? v[r] : (T)0;
                }
            };
            int j = 0;
            for (; j + 4 <= jn; j += 4, col += 4 * ld) {   // four rows' LDS reads in flight (unrolled by hand:
                T v[4][ROWS];                              // v_readlane is convergent, the compiler leaves the loop alone)
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int r = 0; r < ROWS; r++) v[u][r] = col[u * ld + 64 * r];
#pragma unroll
                for (int u = 0; u < 4; u++) add_row(j + u, v[u]);
            }
            for (; j < jn; j++, col += ld) {
                T v[ROWS];
#pragma unroll
                for (int r = 0; r < ROWS; r++) v[r] = col[64 * r];
                add_row(j, v);
            }
        }
#pragma unroll
        for (int q = 0; q < GROUP_Q; q++) {
            const int s = b * GROUP_Q + q;
            const int64_t p = p0 + s - 2;
            T x[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                x[r] = t[q][r];
                if (F64) {
                    const bool in = lane + 64 * r < n;
                    const uint32_t members = s == 0 ? (uint32_t)n : s_cnt[in ? g[q][r] : 0];
                    x[r] = (T)((double)t[q][r] / (in ? 2.0 * (double)members : 1.0));
                }
            }
            const T raw = wave_sum(ROWS == 2 ? (T)(x[0] + x[ROWS - 1]) : x[0]);
            if (s == 0) {
                raw_all = raw;
            } else if (s == 1) {
                raw_obs = raw;
                fobs = group_stat(shape, raw_all, raw_obs);
            } else if (p < pend) {
                const double f = group_stat(shape, raw_all, raw);
                count += F64 ? f >= fobs : raw <= raw_obs;   // NaN counts nothing; R falls as W2 grows
                if (pst && lane == 0) pst[p] = f;
            }
        }
    }
    if (lane == 0 && count) atomicAdd(&n_ge[rep], count);
    if (chunk == 0 && tid == 0) {
        stat[rep] = fobs;
        total[rep] = F64 ? (double)raw_all : (double)((uint32_t)raw_all / 2u);
        within[rep] = F64 ? (double)raw_obs : (double)((uint32_t)raw_obs / 2u);
        if (F64) valid[rep] = 1;
    }
}

// ------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------

// Twice-ranks of R replicates of 2 <= n <= 128 samples into rk2 (R x n x n) and
// their validity; group_rank_lds_bytes(n) fits the device.
hipError_t launch_group_rank(const double *D, int R, int n, uint32_t *rk2, uint8_t *valid, hipStream_t st)
{
    if (R < 1) return hipSuccess;
    const size_t bytes = group_rank_lds_bytes(n);
    const uint32_t M = (uint32_t)n * (uint32_t)(n - 1) / 2, per = RANK_THREADS * RANK_PER_THREAD;
    const uint32_t nkb = (M + per - 1) / per;
    if ((uint64_t)R * nkb >> 31) return hipErrorInvalidConfiguration;
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(&group_rank_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(group_rank_kernel, dim3((unsigned)(R * nkb)), dim3(RANK_THREADS), bytes, st, D, n, (int)nkb, rk2,
                       valid);
    return hipGetLastError();
}

template <typename T, int ROWS>
static hipError_t launch_group_t(const T *src, const uint8_t *valid_in, int R, const GroupShape &shape, int method,
                                 const uint8_t *labels, const uint8_t *perm, int P, double *stat, uint32_t *n_ge,
                                 double *total, double *within, double *perm_stat, uint8_t *valid, hipStream_t st)
{
    const size_t bytes = group_lds_bytes(method, shape.n);
    const int nchunk = P > 0 ? (P + GROUP_PERM_CHUNK - 1) / GROUP_PERM_CHUNK : 1;
    if ((uint64_t)R * (uint64_t)nchunk >> 31) return hipErrorInvalidConfiguration;
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(&group_kernel<T, ROWS>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((group_kernel<T, ROWS>), dim3((unsigned)(R * nchunk)), dim3(GROUP_THREADS), bytes, st, src,
                       valid_in, shape, labels, perm, P, nchunk, stat, n_ge, total, within, perm_stat, valid);
    return hipGetLastError();
}

// The test of R replicates of 2 <= n <= 128 samples in a groups with m_within
// within-group pairs: labels[n] and perm[P][n] hold group numbers below a;
// src is D (R x n x n doubles, GROUP_PERMANOVA) or group_rank_kernel's rk2 with
// valid_in (GROUP_ANOSIM). Every output is a device buffer, perm_stat may be
// null, n_ge is zero on entry. hipErrorInvalidConfiguration: R x permutation
// chunks beyond the grid.
hipError_t launch_group_test(int method, const void *src, const uint8_t *valid_in, int R, int n, int a,
                             uint32_t m_within, const uint8_t *labels, const uint8_t *perm, int P, double *stat,
                             uint32_t *n_ge, double *total, double *within, double *perm_stat, uint8_t *valid,
                             hipStream_t st)
{
    if (R < 1) return hipSuccess;
    const GroupShape shape{n, a, (uint32_t)n * (uint32_t)(n - 1) / 2, m_within};
    if (method == GROUP_ANOSIM) {
        const uint32_t *s = static_cast<const uint32_t *>(src);
        if (n <= 64)
            return launch_group_t<uint32_t, 1>(s, valid_in, R, shape, method, labels, perm, P, stat, n_ge, total, within,
                                               perm_stat, valid, st);
        return launch_group_t<uint32_t, 2>(s, valid_in, R, shape, method, labels, perm, P, stat, n_ge, total, within,
                                           perm_stat, valid, st);
    }
    const double *s = static_cast<const double *>(src);
    if (n <= 64)
        return launch_group_t<double, 1>(s, valid_in, R, shape, method, labels, perm, P, stat, n_ge, total, within,
                                         perm_stat, valid, st);
    return launch_group_t<double, 2>(s, valid_in, R, shape, method, labels, perm, P, stat, n_ge, total, within,
                                     perm_stat, valid, st);
}

}  // namespace rcg
