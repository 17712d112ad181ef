// Principal coordinates (classical scaling) of replicate distance matrices
// (rc_pcoa, rc_resample_pcoa).
//
// The algorithm is that of tests/pcoa_oracle.py (float64, -ffp-contract=off):
//   E[i][j] = -0.5 * (D[i][j] * D[i][j]) for i < j, mirrored, zero diagonal
//   rowmean[i] = (E[0][i] + E[1][i] + ... ascending) / n
//   grand      = (rowmean[0] + rowmean[1] + ... ascending) / n
//   B[i][j] = ((E[i][j] - rowmean[i]) - rowmean[j]) + grand for i <= j, mirrored
//   sigma   = ||B||_F (column sums of squares ascending, then over the columns)
//   A = B + sigma I is positive semidefinite (sigma >= |lambda|): one-sided
//   (Hestenes) Jacobi orthogonalises its columns, and at convergence column c
//   is (lambda_c + sigma) v_c -- no eigenvector accumulator, no sign recovery.
//
// pcoa_kernel: one workgroup per replicate, A column-major in LDS with leading
// dimension ld. A sweep is the round-robin tournament of m = n rounded up to
// even players: m - 1 steps of m / 2 disjoint pairs, one barrier per step. 16
// lanes (one DPP row) own a pair: lane l holds rows l, l + 16, ... of both
// columns in registers from the dot products to the update, so a rotation
// reads and writes each column once. The mapping is a function of n alone: a
// matrix gives the same bits in any batch position.
#include "device.h"
#include "launch.h"

namespace rcg {

// ld = 16 (mod 32) doubles: columns of opposite parity start half a bank row
// (128 B) apart, so the two 16-lane groups of a ds_read_b64's 32-lane half,
// which hold the tournament's neighbouring pairs (columns s + g, s - g and
// s + g + 1, s - g - 1: opposite parity unless one of them wrapped), read
// disjoint banks. A multiple of 32 would put every column on the same banks.
int pcoa_ld(int n) { return (n + 15) / 32 * 32 + 16; }

size_t pcoa_lds_bytes(int n) { return (size_t)n * pcoa_ld(n) * 8; }

__device__ inline double row16_sum(double v)
{
    // xor butterfly inside a 16-lane row: every lane ends with the same bits
    v += __shfl_xor(v, 8, 16);
    v += __shfl_xor(v, 4, 16);
    v += __shfl_xor(v, 2, 16);
    v += __shfl_xor(v, 1, 16);
    return v;
}

// status[0] += invalid replicates, status[1] += replicates that still rotated
// in sweep max_sweeps. NT: rows per lane (n <= 16 NT).
template <int NT>
__global__ __launch_bounds__(1024) void pcoa_kernel(const double *__restrict__ D, int n, int ld, int k, int max_sweeps,
                                                    double *__restrict__ values, double *__restrict__ vectors,
                                                    int32_t *__restrict__ sweeps, uint8_t *__restrict__ valid,
                                                    unsigned int *status)
{
    extern __shared__ double pcoa_A[];   // [n][ld]: element (row i, column c) at c * ld + i
    __shared__ double s_mean[128], s_norm[128];
    __shared__ int s_pos[128];
    __shared__ uint8_t s_neg[128];
    double *A = pcoa_A;
    const int tid = threadIdx.x, nt = blockDim.x;
    const uint64_t rep = blockIdx.x;
    const double *Dr = D + rep * (uint64_t)n * n;
    const uint32_t nn = (uint32_t)n * (uint32_t)n;
    double *val = values + rep * (uint64_t)n;
    double *vec = vectors + rep * (uint64_t)n * k;

    // E, mirrored from the part above the diagonal
    int bad = 0;
    for (uint32_t idx = tid; idx < nn; idx += nt) {
        const uint32_t i = idx / (uint32_t)n, j = idx - i * (uint32_t)n;
        if (i < j) {
            const double v = Dr[idx];
            bad |= !__builtin_isfinite(v);
            const double e = -0.5 * (v * v);
            A[j * ld + i] = e;
            A[i * ld + j] = e;
        } else if (i == j) {
            A[i * ld + i] = 0.0;
        }
    }
    bad = __syncthreads_or(bad);
    double sigma = 0.0;
    if (!bad) {
        if (tid < n) {
            double s = A[tid];
            for (int r = 1; r < n; r++) s += A[r * ld + tid];   // row tid of the symmetric E, walked by columns
            s_mean[tid] = s / (double)n;
        }
        __syncthreads();
        double grand = s_mean[0];
        for (int r = 1; r < n; r++) grand += s_mean[r];
        grand /= (double)n;
        // B: the thread that reads cell (i, j) of E is the one that writes it and its mirror
        for (uint32_t idx = tid; idx < nn; idx += nt) {
            const uint32_t i = idx / (uint32_t)n, j = idx - i * (uint32_t)n;
            if (i <= j) {
                const double b = ((A[j * ld + i] - s_mean[i]) - s_mean[j]) + grand;
                A[j * ld + i] = b;
                A[i * ld + j] = b;
            }
        }
        __syncthreads();
        if (tid < n) {
            double s = A[tid] * A[tid];
            for (int r = 1; r < n; r++) s += A[r * ld + tid] * A[r * ld + tid];   // B is symmetric: by columns
            s_norm[tid] = s;
        }
        __syncthreads();
        double ss = s_norm[0];
        for (int r = 1; r < n; r++) ss += s_norm[r];
        sigma = __builtin_sqrt(ss);
        bad = !__builtin_isfinite(sigma);   // the same value in every thread
    }
    if (bad) {
        for (int idx = tid; idx < n; idx += nt) val[idx] = __builtin_nan("");
        for (int idx = tid; idx < n * k; idx += nt) vec[idx] = __builtin_nan("");
        if (tid == 0) {
            sweeps[rep] = 0;
            valid[rep] = 0;
            atomicAdd(&status[0], 1u);
        }
        return;
    }
    if (tid < n) A[tid * ld + tid] += sigma;
    __syncthreads();

    // the sweeps
    const int m = (n + 1) & ~1, g = tid >> 4, l = tid & 15;
    int done = 0, rotated = 1;
    while (done < max_sweeps && rotated) {
        int rot = 0;
        for (int s = 0; s < m - 1; s++) {
            int p = m - 1, q = s;
            if (g > 0) {
                p = s + g;
                q = s + m - 1 - g;
                if (p >= m - 1) p -= m - 1;
                if (q >= m - 1) q -= m - 1;
            }
            if (p > q) {
                const int t = p;
                p = q;
                q = t;
            }
            if (g < m / 2 && q < n) {   // q == n: the dummy player of an odd n
                double *ap = A + p * ld + l, *aq = A + q * ld + l;
                double x[NT], y[NT];
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const bool in = l + 16 * t < n;
                    x[t] = in ? ap[16 * t] : 0.0;
                    y[t] = in ? aq[16 * t] : 0.0;
                }
                double al = x[0] * x[0], be = y[0] * y[0], ga = x[0] * y[0];
#pragma unroll
                for (int t = 1; t < NT; t++) {
                    al += x[t] * x[t];
                    be += y[t] * y[t];
                    ga += x[t] * y[t];
                }
                al = row16_sum(al);
                be = row16_sum(be);
                ga = row16_sum(ga);
                if (al != 0.0 && be != 0.0 &&
                    __builtin_fabs(ga) > (0x1p-52 * __builtin_sqrt(al)) * __builtin_sqrt(be)) {
                    const double zeta = (be - al) / (2.0 * ga);
                    const double az = __builtin_fabs(zeta);
                    double t = 1.0 / (az + __builtin_sqrt(1.0 + zeta * zeta));
                    if (zeta < 0.0) t = -t;
                    const double c = 1.0 / __builtin_sqrt(1.0 + t * t), sn = c * t;
#pragma unroll
                    for (int u = 0; u < NT; u++) {
                        if (l + 16 * u < n) {
                            ap[16 * u] = c * x[u] - sn * y[u];
                            aq[16 * u] = sn * x[u] + c * y[u];
                        }
                    }
                    rot = 1;
                }
            }
            if (s < m - 2) __syncthreads();
        }
        rotated = __syncthreads_or(rot);
        done++;
    }

    // eigenvalues, order, signs
    if (tid < n) {
        const double *a = A + tid * ld;
        double s = a[0] * a[0], big = __builtin_fabs(a[0]);
        int neg = a[0] < 0.0;
        for (int r = 1; r < n; r++) {
            s += a[r] * a[r];
            if (__builtin_fabs(a[r]) > big) {
                big = __builtin_fabs(a[r]);
                neg = a[r] < 0.0;
            }
        }
        s_norm[tid] = __builtin_sqrt(s);
        s_neg[tid] = (uint8_t)neg;
    }
    __syncthreads();
    if (tid < n) {
        // lambda = norm - sigma is monotone in norm, but two norms may round to one lambda
        const double lam = s_norm[tid] - sigma;
        int rank = 0;
        for (int c = 0; c < n; c++) {
            const double o = s_norm[c] - sigma;
            rank += o > lam || (o == lam && c < tid);
        }
        s_pos[rank] = tid;
        val[rank] = lam;
    }
    __syncthreads();
    for (int idx = tid; idx < n * k; idx += nt) {
        const int i = idx / k, r = idx - i * k, c = s_pos[r];
        const double nrm = s_norm[c];
        double v = 0.0;
        if (nrm != 0.0) {
            v = A[c * ld + i] / nrm;
            if (s_neg[c]) v = -v;
        }
        vec[idx] = v;
    }
    if (tid == 0) {
        sweeps[rep] = done;
        valid[rep] = 1;
        if (rotated) atomicAdd(&status[1], 1u);
    }
}

// ------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------

template <int NT>
static hipError_t launch_pcoa_nt(const double *D, int R, int n, int k, int max_sweeps, double *values, double *vectors,
                                 int32_t *sweeps, uint8_t *valid, unsigned int *status, hipStream_t st)
{
    const size_t bytes = pcoa_lds_bytes(n);
    const unsigned block = (unsigned)((16 * ((n + 1) / 2) + 63) / 64 * 64);
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(&pcoa_kernel<NT>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(pcoa_kernel<NT>, dim3((unsigned)R), dim3(block), bytes, st, D, n, pcoa_ld(n), k, max_sweeps,
                       values, vectors, sweeps, valid, status);
    return hipGetLastError();
}

// R replicates of 2 <= n <= 128 samples (the caller has checked that
// pcoa_lds_bytes(n) fits the device); every output is a device buffer.
hipError_t launch_pcoa(const double *D, int R, int n, int k, int max_sweeps, double *values, double *vectors,
                       int32_t *sweeps, uint8_t *valid, unsigned int *status, hipStream_t st)
{
    if (R < 1) return hipSuccess;
    if (n <= 16) return launch_pcoa_nt<1>(D, R, n, k, max_sweeps, values, vectors, sweeps, valid, status, st);
    if (n <= 32) return launch_pcoa_nt<2>(D, R, n, k, max_sweeps, values, vectors, sweeps, valid, status, st);
    if (n <= 64) return launch_pcoa_nt<4>(D, R, n, k, max_sweeps, values, vectors, sweeps, valid, status, st);
    return launch_pcoa_nt<8>(D, R, n, k, max_sweeps, values, vectors, sweeps, valid, status, st);
}

}  // namespace rcg
