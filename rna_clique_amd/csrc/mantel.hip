// The Mantel test: the permutation correlation of replicate distance matrices X
// with one matrix Y (rc_mantel, rc_resample_mantel).
//
// The algorithm is that of tests/mantel_oracle.py (-ffp-contract=off; of a
// matrix only i < j is read, mirrored, zero diagonal; M = n (n - 1) / 2; every
// sum over j = 0, 1, ... ascending; H: the halving sum of groups.hip). A
// permutation p rearranges X's rows and columns together:
//   pearson (float64)
//     mx      = H(rs) / (n (n - 1)),  rs[i] = sum of X[j][i]
//     xc[i][j] = X[i][j] - mx off the diagonal, 0 on it;  sxx = H(q),
//     q[i] = sum of xc[j][i] * xc[j][i];  yc and syy likewise (mantel_prepare_y)
//     C(p)    = H(c),  c[i] = sum of xc[p(j)][p(i)] * yc[j][i]
//     r(p)    = C(p) / sqrt(sxx * syy)  (exactly 1 for Y = X)
//     X or Y constant above the diagonal: r is NaN and nothing is counted
//   spearman (integers, exact): a, b the twice-ranks of X and Y (group_rank_kernel)
//     Sab(p)  = the sum over i < j of a[p(i)][p(j)] * b[i][j]  (64 bits)
//     num(p)  = M Sab(p) - Sa Sb,  vx = M Saa - Sa Sa,  vy = M Sbb - Sb Sb
//     r(p)    = (double)num / sqrt((double)vx * (double)vy)
//     vx or vy zero: r is NaN and nothing is counted
// The counts compare a permutation with the identity on r (pearson) or on num
// (spearman): >=, <= and |.| >= |.|.
//
// mantel_kernel: a workgroup stages one replicate's X (centred doubles, or
// uint32 ranks) in LDS, element (row j, column i) at j * ld + i. Lane i owns row
// i (two rows above 64 samples) and for j ascending adds X[p(j) * ld + p(i)] *
// Y[j][i]: p(j) comes out of lane j's register with v_readlane, Y[j][.] is
// streamed from global memory (the same 128 KB for every workgroup) and one
// load of it serves MANTEL_Q permutations. Every wave evaluates the identity
// first, with the code path of its permutations. Counts leave the workgroup as
// integer atomics, once per wave; a replicate's bits do not depend on the grid.
#include "device.h"
#include "launch.h"

#include <type_traits>

namespace rcg {

enum {
    MANTEL_THREADS = 256,     // 4 waves
    MANTEL_Q = 4,             // permutations per pass over the matrix
    MANTEL_WAVE_PERMS = 31    // permutations per wave: with the identity every wave adds, 8 passes
};
static_assert(MANTEL_PERM_CHUNK == (MANTEL_THREADS / 64) * MANTEL_WAVE_PERMS, "a workgroup's permutations");
static_assert((MANTEL_WAVE_PERMS + 1) % MANTEL_Q == 0, "whole passes");

static int mantel_ld(int n) { return n <= 64 ? 64 : 128; }

size_t mantel_lds_bytes(int method, int n) { return (size_t)n * mantel_ld(n) * (method == MANTEL_SPEARMAN ? 4 : 8); }

// The halving sum of x[0..n) on the host.
static double host_halving_sum(const double *x, int n)
{
    double y[128] = {};
    int w = 1;
    while (w < n) w *= 2;
    for (int i = 0; i < n; i++) y[i] = x[i];
    for (w /= 2; w >= 1; w /= 2)
        for (int i = 0; i < w; i++) y[i] = y[i] + y[i + w];
    return y[0];
}

// Y for the pearson method, on the host: yc (n x n, mirrored, centred off the
// diagonal, zero on it) and syy; *constant: every entry above the diagonal is
// the same. 3 <= n <= 128; only i < j of Y is read.
void mantel_prepare_y(const double *Y, int n, double *yc, double *syy, int *constant)
{
    auto at = [&](int i, int j) { return i == j ? 0.0 : i < j ? Y[(size_t)i * n + j] : Y[(size_t)j * n + i]; };
    double s[128];
    int same = 1;
    for (int i = 0; i < n; i++) {
        double t = 0.0;
        for (int j = 0; j < n; j++) {
            t += at(j, i);
            if (j != i) same &= at(j, i) == Y[1];
        }
        s[i] = t;
    }
    const double my = host_halving_sum(s, n) / ((double)n * (double)(n - 1));
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) yc[(size_t)i * n + j] = i == j ? 0.0 : at(i, j) - my;
    for (int i = 0; i < n; i++) {
        double t = 0.0;
        for (int j = 0; j < n; j++) t += yc[(size_t)j * n + i] * yc[(size_t)j * n + i];
        s[i] = t;
    }
    *syy = host_halving_sum(s, n);
    *constant = same;
}

static __device__ inline double mantel_wave_sum(double v)
{
    // xor butterfly: x[0:h] + x[h:2h] for h = 32 .. 1; addition commutes, so every lane ends with the same bits
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

static __device__ inline unsigned long long mantel_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
    return v;
}

// The sum over j ascending of f(A[j][row]) for this lane's rows, then over the lanes: H for doubles.
template <typename T, typename A, int ROWS, typename F>
static __device__ inline A mantel_column_sum(const T *col, int stride, int n, const bool (&in)[ROWS], F f)
{
    A acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) acc[r] = (A)0;
    for (int j = 0; j < n; j++)
#pragma unroll
        for (int r = 0; r < ROWS; r++)
            if (in[r]) acc[r] += f(col[(size_t)j * stride + 64 * r]);
    return mantel_wave_sum(ROWS == 2 ? (A)(acc[0] + acc[ROWS - 1]) : acc[0]);
}

// T = double: pearson on X (sets valid); Yp is mantel_prepare_y's yc, syy its
// sum of squares, y_const its verdict. T = uint32_t: spearman on the twice-ranks
// of X in src (valid_in: group_rank_kernel's verdict; valid is left alone and
// may be the same array) and of Y in Yp. ROWS: rows per lane (n <= 64 ROWS).
// Workgroup (rep, chunk) = blockIdx.x / nchunk, % nchunk; its wave w takes
// permutations [chunk * MANTEL_PERM_CHUNK + w * MANTEL_WAVE_PERMS, + MANTEL_WAVE_PERMS).
// The three counts must be zero on entry.
template <typename T, int ROWS>
__global__ __launch_bounds__(MANTEL_THREADS) void mantel_kernel(const T *__restrict__ src, const uint8_t *valid_in, int n,
                                                                const T *__restrict__ Yp, double syy, int y_const,
                                                                const uint8_t *__restrict__ perm, int P, int nchunk,
                                                                double *__restrict__ stat, uint32_t *n_ge, uint32_t *n_le,
                                                                uint32_t *n_abs_ge, double *__restrict__ perm_stat,
                                                                uint8_t *valid)
{
    extern __shared__ double mantel_lds[];
    constexpr bool F64 = sizeof(T) == 8;
    constexpr int ld = 64 * ROWS;
    using Acc = typename std::conditional<F64, double, unsigned long long>::type;
    T *V = reinterpret_cast<T *>(mantel_lds);
    const int tid = threadIdx.x;
    const uint32_t nn = (uint32_t)n * (uint32_t)n;
    const uint64_t rep = blockIdx.x / (uint32_t)nchunk;
    const int chunk = (int)(blockIdx.x % (uint32_t)nchunk);
    const T *Sr = src + rep * nn;
    const int wave = tid >> 6, lane = tid & 63;
    bool in[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) in[r] = lane + 64 * r < n;

    // stage X: mirrored with a zero diagonal; the columns no sample owns are never read
    int bad = 0, differs = 0;
    if (F64) {
        const T first = Sr[1];
        for (uint32_t idx = tid; idx < nn; idx += MANTEL_THREADS) {
            const uint32_t i = idx / (uint32_t)n, j = idx - i * (uint32_t)n;
            if (i < j) {
                const T v = Sr[idx];
                bad |= !__builtin_isfinite((double)v);
                differs |= v != first;
                V[j * ld + i] = v;
                V[i * ld + j] = v;
            } else if (i == j) {
                V[i * ld + i] = (T)0;
            }
        }
    } else {
        bad = !valid_in[rep];
        if (!bad)
            for (uint32_t idx = tid; idx < nn; idx += MANTEL_THREADS) {
                const uint32_t i = idx / (uint32_t)n, j = idx - i * (uint32_t)n;
                V[i * ld + j] = Sr[idx];
            }
    }
    bad = __syncthreads_or(bad);
    differs = __syncthreads_or(differs);

    const int64_t p0 = (int64_t)chunk * MANTEL_PERM_CHUNK + wave * MANTEL_WAVE_PERMS;
    const int64_t pend = p0 + MANTEL_WAVE_PERMS < P ? p0 + MANTEL_WAVE_PERMS : P;
    double *pst = perm_stat ? perm_stat + rep * (uint64_t)P : nullptr;
    double scale = 0.0;                      // pearson: sqrt(sxx * syy)
    long long M = 0, SaSb = 0;               // spearman: num = M Sab - Sa Sb
    bool undefined = false;                  // r is NaN for every permutation
    if (!bad) {
        if (F64) {
            // centre X in place: every wave computes the mean (the same bits), every thread centres its share
            const double mx = (double)mantel_column_sum<T, Acc, ROWS>(V + lane, ld, n, in, [](T v) { return (Acc)v; }) /
                              ((double)n * (double)(n - 1));
            __syncthreads();
            for (uint32_t idx = tid; idx < nn; idx += MANTEL_THREADS) {
                const uint32_t i = idx / (uint32_t)n, j = idx - i * (uint32_t)n;
                if (i != j) V[i * ld + j] = (T)((double)V[i * ld + j] - mx);
            }
            __syncthreads();
            const double sxx = (double)mantel_column_sum<T, Acc, ROWS>(V + lane, ld, n, in,
                                                                       [](T v) { return (Acc)((double)v * (double)v); });
            scale = __builtin_sqrt(sxx * syy);
            undefined = !differs || y_const;
        } else {
            auto sq = [](T v) { return (Acc)v * (Acc)v; };
            auto id = [](T v) { return (Acc)v; };
            M = (long long)n * (n - 1) / 2;
            const long long Saa = (long long)mantel_column_sum<T, Acc, ROWS>(V + lane, ld, n, in, sq) / 2;
            const long long Sa = (long long)mantel_column_sum<T, Acc, ROWS>(V + lane, ld, n, in, id) / 2;
            const long long Sbb = (long long)mantel_column_sum<T, Acc, ROWS>(Yp + lane, n, n, in, sq) / 2;
            const long long Sb = (long long)mantel_column_sum<T, Acc, ROWS>(Yp + lane, n, n, in, id) / 2;
            const long long vx = M * Saa - Sa * Sa, vy = M * Sbb - Sb * Sb;
            SaSb = Sa * Sb;
            scale = __builtin_sqrt((double)vx * (double)vy);
            undefined = vx == 0 || vy == 0;
        }
    }
    if (bad || undefined) {
        if (pst && lane < 32)
            for (int64_t p = p0 + lane; p < pend; p += 32) pst[p] = __builtin_nan("");
        if (chunk == 0 && tid == 0) {
            stat[rep] = __builtin_nan("");
            if (F64) valid[rep] = bad ? 0 : 1;
        }
        return;
    }

    double robs = 0.0;
    long long nobs = 0;
    uint32_t c_ge = 0, c_le = 0, c_abs = 0;
    for (int b = 0; b * MANTEL_Q < MANTEL_WAVE_PERMS + 1; b++) {
        // slot 0: the identity; slot s: permutation p0 + s - 1
        uint32_t pi[MANTEL_Q][ROWS];
        Acc c[MANTEL_Q][ROWS];
#pragma unroll
        for (int q = 0; q < MANTEL_Q; q++) {
            const int s = b * MANTEL_Q + q;
            const int64_t p = p0 + s - 1;
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const int row = lane + 64 * r;
                pi[q][r] = in[r] ? (uint32_t)row : 0u;   // a lane without a row reads column 0 and multiplies it by zero
                if (s > 0 && p < pend && in[r]) pi[q][r] = perm[p * n + row];
                c[q][r] = (Acc)0;
            }
        }
#pragma unroll
        for (int h = 0; h < ROWS; h++) {   // rows j = 64 h .. of Y: p(j) sits in pi[.][h]
            const int jn = n - 64 * h < 64 ? n - 64 * h : 64;
            const T *yrow = Yp + (size_t)64 * h * n + lane;
            auto add_row = [&](int j, const T *y) {   // row 64 h + j of Y, ascending j
#pragma unroll
                for (int q = 0; q < MANTEL_Q; q++) {
                    const uint32_t pj = (uint32_t)__builtin_amdgcn_readlane((int)pi[q][h], j);
                    const T *xrow = V + pj * ld;
#pragma unroll
                    for (int r = 0; r < ROWS; r++) c[q][r] += (Acc)xrow[pi[q][r]] * (Acc)y[r];
                }
            };
            int j = 0;
            for (; j + 4 <= jn; j += 4, yrow += 4 * n) {   // four rows' loads of Y in flight
                T y[4][ROWS];
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int r = 0; r < ROWS; r++) y[u][r] = in[r] ? yrow[u * n + 64 * r] : (T)0;
#pragma unroll
                for (int u = 0; u < 4; u++) add_row(j + u, y[u]);
            }
            for (; j < jn; j++, yrow += n) {
                T y[ROWS];
#pragma unroll
                for (int r = 0; r < ROWS; r++) y[r] = in[r] ? yrow[64 * r] : (T)0;
                add_row(j, y);
            }
        }
#pragma unroll
        for (int q = 0; q < MANTEL_Q; q++) {
            const int s = b * MANTEL_Q + q;
            const int64_t p = p0 + s - 1;
            const Acc raw = mantel_wave_sum(ROWS == 2 ? (Acc)(c[q][0] + c[q][ROWS - 1]) : c[q][0]);
            long long num = 0;
            double r;
            if (F64) {
                r = (double)raw / scale;
            } else {
                num = M * (long long)((unsigned long long)raw / 2u) - SaSb;
                r = (double)num / scale;
            }
            if (s == 0) {
                robs = r;
                nobs = num;
            } else if (p < pend) {
                if (F64) {
                    c_ge += r >= robs;   // NaN counts nothing
                    c_le += r <= robs;
                    c_abs += __builtin_fabs(r) >= __builtin_fabs(robs);
                } else {
                    c_ge += num >= nobs;
                    c_le += num <= nobs;
                    c_abs += (num < 0 ? -num : num) >= (nobs < 0 ? -nobs : nobs);
                }
                if (pst && lane == 0) pst[p] = r;
            }
        }
    }
    if (lane == 0) {
        if (c_ge) atomicAdd(&n_ge[rep], c_ge);
        if (c_le) atomicAdd(&n_le[rep], c_le);
        if (c_abs) atomicAdd(&n_abs_ge[rep], c_abs);
    }
    if (chunk == 0 && tid == 0) {
        stat[rep] = robs;
        if (F64) valid[rep] = 1;
    }
}

template <typename T, int ROWS>
static hipError_t launch_mantel_t(const T *src, const uint8_t *valid_in, int R, int n, int method, const T *Yp, double syy,
                                  int y_const, const uint8_t *perm, int P, double *stat, uint32_t *n_ge, uint32_t *n_le,
                                  uint32_t *n_abs_ge, double *perm_stat, uint8_t *valid, hipStream_t st)
{
    const size_t bytes = mantel_lds_bytes(method, n);
    const int nchunk = P > 0 ? (P + MANTEL_PERM_CHUNK - 1) / MANTEL_PERM_CHUNK : 1;
    if ((uint64_t)R * (uint64_t)nchunk >> 31) return hipErrorInvalidConfiguration;
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(&mantel_kernel<T, ROWS>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((mantel_kernel<T, ROWS>), dim3((unsigned)(R * nchunk)), dim3(MANTEL_THREADS), bytes, st, src,
                       valid_in, n, Yp, syy, y_const, perm, P, nchunk, stat, n_ge, n_le, n_abs_ge, perm_stat, valid);
    return hipGetLastError();
}

// The Mantel test of R replicates of 3 <= n <= 128 samples against one matrix:
// src is X (R x n x n doubles) with Yp = mantel_prepare_y's yc (n x n doubles),
// syy and y_const (MANTEL_PEARSON), or group_rank_kernel's twice-ranks of X with
// valid_in and, in Yp, those of Y (n x n uint32; MANTEL_SPEARMAN). perm[P][n]
// holds permutations of 0..n-1, one byte each. Every output is a device
// buffer, perm_stat may be null, the counts are zero on entry.
// hipErrorInvalidConfiguration: R x permutation chunks beyond the grid.
hipError_t launch_mantel(int method, const void *src, const uint8_t *valid_in, int R, int n, const void *Yp, double syy,
                         int y_const, const uint8_t *perm, int P, double *stat, uint32_t *n_ge, uint32_t *n_le,
                         uint32_t *n_abs_ge, double *perm_stat, uint8_t *valid, hipStream_t st)
{
    if (R < 1) return hipSuccess;
    if (method == MANTEL_SPEARMAN) {
        const uint32_t *s = static_cast<const uint32_t *>(src), *y = static_cast<const uint32_t *>(Yp);
        if (n <= 64)
            return launch_mantel_t<uint32_t, 1>(s, valid_in, R, n, method, y, syy, y_const, perm, P, stat, n_ge, n_le,
                                                n_abs_ge, perm_stat, valid, st);
        return launch_mantel_t<uint32_t, 2>(s, valid_in, R, n, method, y, syy, y_const, perm, P, stat, n_ge, n_le,
                                            n_abs_ge, perm_stat, valid, st);
    }
    const double *s = static_cast<const double *>(src), *y = static_cast<const double *>(Yp);
    if (n <= 64)
        return launch_mantel_t<double, 1>(s, valid_in, R, n, method, y, syy, y_const, perm, P, stat, n_ge, n_le, n_abs_ge,
                                          perm_stat, valid, st);
    return launch_mantel_t<double, 2>(s, valid_in, R, n, method, y, syy, y_const, perm, P, stat, n_ge, n_le, n_abs_ge,
                                      perm_stat, valid, st);
}

}  // namespace rcg
