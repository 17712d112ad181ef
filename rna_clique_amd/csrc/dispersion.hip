// PERMDISP (Anderson 2006, centroid form) on replicate distance matrices with
// label permutations (rc_group_dispersion, rc_resample_group_dispersion): are
// the groups equally spread?
//
// The algorithm is that of tests/dispersion_oracle.py (float64,
// -ffp-contract=off; of matrix D[n][n] only i < j is read, mirrored, zero
// diagonal). For a label vector g, with n_g[i] the size of i's group and every
// sum over j = 0, 1, ... ascending:
//   v[i][j] = D[i][j] * D[i][j]
//   t[i]  = sum of (g[j] == g[i] ? v[j][i] : 0)      (groups.hip's t)
//   b[i]  = sum of (g[j] == g[i] ? t[j] : 0)
//   z[i]  = sqrt(|t[i] / n_g[i] - b[i] / (2.0 * n_g[i] * n_g[i])|)
//           the distance of sample i to its group's centroid in the full
//           principal-coordinate space; no eigensolver is involved
//   s[i]  = sum of (g[j] == g[i] ? z[j] : 0),  m[i] = s[i] / n_g[i]
//   SS_W  = H((z - m)^2),  zbar = H(z) / n,  SS_T = H((z - zbar)^2)
//   F     = ((SS_T - SS_W) / (a - 1)) / (SS_W / (n - a))
// H: the sum of x padded with zeros to a power of two, halved until one value
// is left (x[0:h] + x[h:2h], h = 64, 32, ..., 1). Everything depends on the
// partition that g describes and on nothing else.
//
// dispersion_kernel stages v as group_kernel does (element (row j, column i) at
// j * ld + i) and walks DISP_Q label vectors per pass over the matrix. After
// the pass t sits in lane registers; b and s are two more walks over j whose
// terms come out of lane j's registers with v_readlane -- no LDS. Every wave
// evaluates the observed labels first, with the code path of its
// permutations, so the F it compares with is its own. Counts leave the
// workgroup as one integer atomic per wave; there is no floating-point atomic,
// and a replicate's bits do not depend on the grid.
#include "device.h"
#include "launch.h"

namespace rcg {

enum {
    DISP_THREADS = 256,      // 4 waves
    DISP_Q = 4,              // label vectors per pass over the matrix
    DISP_WAVE_PERMS = 31,    // permutations per wave: with the observed labels every wave adds, 8 passes
    DISP_NO_LABEL = 0xFF     // the label of a lane without a row: equal to no sample's (labels < 127)
};
static_assert(DISP_PERM_CHUNK == (DISP_THREADS / 64) * DISP_WAVE_PERMS, "a workgroup's permutations");
static_assert((DISP_WAVE_PERMS + 1) % DISP_Q == 0, "whole passes");

static int disp_ld(int n) { return n <= 64 ? 64 : 128; }

size_t dispersion_lds_bytes(int n) { return (size_t)n * disp_ld(n) * 8; }

static __device__ inline double disp_wave_sum(double v)
{
    // xor butterfly: x[0:h] + x[h:2h] for h = 32 .. 1; addition commutes, so every lane ends with the same bits
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

static __device__ inline double disp_readlane(double v, int j)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

// ROWS: rows per lane (n <= 64 ROWS). Workgroup (rep, chunk) = blockIdx.x /
// nchunk, % nchunk; its wave w takes permutations [chunk * DISP_PERM_CHUNK +
// w * DISP_WAVE_PERMS, + DISP_WAVE_PERMS). n_ge must be zero on entry.
template <int ROWS>
__global__ __launch_bounds__(DISP_THREADS) void dispersion_kernel(const double *__restrict__ D, int n, int a,
                                                                  const uint8_t *__restrict__ labels,
                                                                  const uint8_t *__restrict__ perm, int P, int nchunk,
                                                                  double *__restrict__ stat, uint32_t *n_ge,
                                                                  double *__restrict__ total, double *__restrict__ within,
                                                                  double *__restrict__ perm_stat,
                                                                  double *__restrict__ dist, uint8_t *__restrict__ valid)
{
    extern __shared__ double disp_lds[];
    __shared__ uint32_t s_cnt[128];
    constexpr int ld = 64 * ROWS;
    double *V = disp_lds;
    const int tid = threadIdx.x;
    const uint32_t nn = (uint32_t)n * (uint32_t)n;
    const uint64_t rep = blockIdx.x / (uint32_t)nchunk;
    const int chunk = (int)(blockIdx.x % (uint32_t)nchunk);
    const double *Sr = D + rep * nn;

    // stage v, count the groups
    if (tid < 128) s_cnt[tid] = 0;
    int bad = 0;
    for (uint32_t idx = tid; idx < nn; idx += DISP_THREADS) {
        const uint32_t i = idx / (uint32_t)n, j = idx - i * (uint32_t)n;
        if (i < j) {
            const double d = Sr[idx];
            bad |= !__builtin_isfinite(d);
            const double v = d * d;
            V[j * ld + i] = v;
            V[i * ld + j] = v;
        } else if (i == j) {
            V[i * ld + i] = 0.0;
        }
    }
    for (uint32_t idx = tid; idx < (uint32_t)n * (ld - n); idx += DISP_THREADS) {   // the columns no sample owns
        const uint32_t j = idx / (uint32_t)(ld - n), i = n + (idx - j * (uint32_t)(ld - n));
        V[j * ld + i] = 0.0;
    }
    bad = __syncthreads_or(bad);
    if (tid < n) atomicAdd(&s_cnt[labels[tid]], 1u);
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    const int64_t p0 = (int64_t)chunk * DISP_PERM_CHUNK + wave * DISP_WAVE_PERMS;
    const int64_t pend = p0 + DISP_WAVE_PERMS < P ? p0 + DISP_WAVE_PERMS : P;
    double *pst = perm_stat ? perm_stat + rep * (uint64_t)P : nullptr;
    if (bad) {
        if (pst && lane < 32)
            for (int64_t p = p0 + lane; p < pend; p += 32) pst[p] = __builtin_nan("");
        if (chunk == 0 && tid < n) dist[rep * (uint64_t)n + tid] = __builtin_nan("");
        if (chunk == 0 && tid == 0) {
            stat[rep] = total[rep] = within[rep] = __builtin_nan("");
            valid[rep] = 0;
        }
        return;
    }

    uint32_t gobs[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) gobs[r] = lane + 64 * r < n ? labels[lane + 64 * r] : DISP_NO_LABEL;
    double fobs = 0.0, sst_obs = 0.0, ssw_obs = 0.0;
    uint32_t count = 0;
    for (int b = 0; b * DISP_Q < DISP_WAVE_PERMS + 1; b++) {
        // slot 0: the observed labels; slot s: permutation p0 + s - 1
        uint32_t g[DISP_Q][ROWS];
        double t[DISP_Q][ROWS];
#pragma unroll
        for (int q = 0; q < DISP_Q; q++) {
            const int s = b * DISP_Q + q;
            const int64_t p = p0 + s - 1;
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const int row = lane + 64 * r;
                g[q][r] = gobs[r];
                if (s > 0 && p < pend && row < n) g[q][r] = perm[p * n + row];
                t[q][r] = 0.0;
            }
        }
        // t: the pass over the matrix
#pragma unroll
        for (int h = 0; h < ROWS; h++) {   // rows j = 64 h .. of the matrix: their labels sit in g[.][h]
            const int jn = n - 64 * h < 64 ? n - 64 * h : 64;
            const double *col = V + 64 * h * ld + lane;
            auto add_row = [&](int j, const double *v) {   // row 64 h + j of the matrix, ascending j
#pragma unroll
                for (int q = 0; q < DISP_Q; q++) {
                    const uint32_t gj = (uint32_t)__builtin_amdgcn_readlane((int)g[q][h], j);
#pragma unroll
                    for (int r = 0; r < ROWS; r++) t[q][r] += g[q][r] == gj ? v[r] : 0.0;
                }
            };
            int j = 0;
            for (; j + 4 <= jn; j += 4, col += 4 * ld) {   // four rows' LDS reads in flight
                double v[4][ROWS];
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int r = 0; r < ROWS; r++) v[u][r] = col[u * ld + 64 * r];
#pragma unroll
                for (int u = 0; u < 4; u++) add_row(j + u, v[u]);
            }
            for (; j < jn; j++, col += ld) {
                double v[ROWS];
#pragma unroll
                for (int r = 0; r < ROWS; r++) v[r] = col[64 * r];
                add_row(j, v);
            }
        }
        // out[i] = the sum over j ascending of x[j] where g[j] == g[i]: x[j] comes out of lane j's registers
        auto own_sums = [&](const double (&x)[DISP_Q][ROWS], double (&out)[DISP_Q][ROWS]) {
#pragma unroll
            for (int q = 0; q < DISP_Q; q++)
#pragma unroll
                for (int r = 0; r < ROWS; r++) out[q][r] = 0.0;
#pragma unroll
            for (int h = 0; h < ROWS; h++) {
                const int jn = n - 64 * h < 64 ? n - 64 * h : 64;
                for (int j = 0; j < jn; j++) {
#pragma unroll
                    for (int q = 0; q < DISP_Q; q++) {
                        const uint32_t gj = (uint32_t)__builtin_amdgcn_readlane((int)g[q][h], j);
                        const double xj = disp_readlane(x[q][h], j);
#pragma unroll
                        for (int r = 0; r < ROWS; r++) out[q][r] += g[q][r] == gj ? xj : 0.0;
                    }
                }
            }
        };
        double ng[DISP_Q][ROWS], z[DISP_Q][ROWS], acc[DISP_Q][ROWS];
        own_sums(t, acc);   // b
#pragma unroll
        for (int q = 0; q < DISP_Q; q++)
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const bool in = lane + 64 * r < n;
                ng[q][r] = in ? (double)s_cnt[g[q][r]] : 1.0;
                const double z2 = t[q][r] / ng[q][r] - acc[q][r] / (2.0 * ng[q][r] * ng[q][r]);
                z[q][r] = in ? __builtin_sqrt(__builtin_fabs(z2)) : 0.0;
            }
        own_sums(z, acc);   // s
#pragma unroll
        for (int q = 0; q < DISP_Q; q++) {
            const int s = b * DISP_Q + q;
            const int64_t p = p0 + s - 1;
            double xw[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const double dw = z[q][r] - acc[q][r] / ng[q][r];
                xw[r] = lane + 64 * r < n ? dw * dw : 0.0;
            }
            const double ssw = disp_wave_sum(ROWS == 2 ? xw[0] + xw[ROWS - 1] : xw[0]);
            const double zbar = disp_wave_sum(ROWS == 2 ? z[q][0] + z[q][ROWS - 1] : z[q][0]) / (double)n;
            double xt[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const double dt = z[q][r] - zbar;
                xt[r] = lane + 64 * r < n ? dt * dt : 0.0;
            }
            const double sst = disp_wave_sum(ROWS == 2 ? xt[0] + xt[ROWS - 1] : xt[0]);
            const double f = ((sst - ssw) / (double)(a - 1)) / (ssw / (double)(n - a));
            if (s == 0) {
                fobs = f;
                sst_obs = sst;
                ssw_obs = ssw;
                if (chunk == 0 && wave == 0) {
#pragma unroll
                    for (int r = 0; r < ROWS; r++)
                        if (lane + 64 * r < n) dist[rep * (uint64_t)n + lane + 64 * r] = z[q][r];
                }
            } else if (p < pend) {
                count += f >= fobs;   // NaN counts nothing
                if (pst && lane == 0) pst[p] = f;
            }
        }
    }
    if (lane == 0 && count) atomicAdd(&n_ge[rep], count);
    if (chunk == 0 && tid == 0) {
        stat[rep] = fobs;
        total[rep] = sst_obs;
        within[rep] = ssw_obs;
        valid[rep] = 1;
    }
}

template <int ROWS>
static hipError_t launch_dispersion_t(const double *D, int R, int n, int a, const uint8_t *labels, const uint8_t *perm,
                                      int P, double *stat, uint32_t *n_ge, double *total, double *within,
                                      double *perm_stat, double *dist, uint8_t *valid, hipStream_t st)
{
    const size_t bytes = dispersion_lds_bytes(n);
    const int nchunk = P > 0 ? (P + DISP_PERM_CHUNK - 1) / DISP_PERM_CHUNK : 1;
    if ((uint64_t)R * (uint64_t)nchunk >> 31) return hipErrorInvalidConfiguration;
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(&dispersion_kernel<ROWS>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((dispersion_kernel<ROWS>), dim3((unsigned)(R * nchunk)), dim3(DISP_THREADS), bytes, st, D, n, a,
                       labels, perm, P, nchunk, stat, n_ge, total, within, perm_stat, dist, valid);
    return hipGetLastError();
}

// PERMDISP of R replicates (D: R x n x n doubles) of 2 <= n <= 128 samples in a
// groups: labels[n] and perm[P][n] hold group numbers below a. Every output is a
// device buffer (dist: R x n), perm_stat may be null, n_ge is zero on entry.
// hipErrorInvalidConfiguration: R x permutation chunks beyond the grid.
hipError_t launch_dispersion(const double *D, int R, int n, int a, const uint8_t *labels, const uint8_t *perm, int P,
                             double *stat, uint32_t *n_ge, double *total, double *within, double *perm_stat,
                             double *dist, uint8_t *valid, hipStream_t st)
{
    if (R < 1) return hipSuccess;
    if (n <= 64)
        return launch_dispersion_t<1>(D, R, n, a, labels, perm, P, stat, n_ge, total, within, perm_stat, dist, valid, st);
    return launch_dispersion_t<2>(D, R, n, a, labels, perm, P, stat, n_ge, total, within, perm_stat, dist, valid, st);
}

}  // namespace rcg
