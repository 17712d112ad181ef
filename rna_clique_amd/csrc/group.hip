// The HSPs of the extension, grouped for what reads them:
//
//   group_* / mirror_*   per (query gene, subject sample): HSPs made
//                        contiguous in candidate order (the oracle's order).
//
// Host entry point: launch_group (its passes: enum GroupPass in launch.h).
#include "device.h"
#include "launch.h"

namespace rcg {

// ------------------------------------------------------------------------
// (gene, sample) groups
// ------------------------------------------------------------------------

__global__ void group_count_kernel(GroupParams P)
{
    const uint64_t sg = (uint64_t)(P.gene_end - P.gene_begin), n = sg * (uint64_t)P.N;
    // gi: the seed kernel's gene-major (query gene, subject sample) index, read
    // in order; si: sample-major, the order direct groups are placed in
    for (uint64_t gi = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; gi < n;
         gi += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t si = (gi % (uint64_t)P.N) * sg + gi / (uint64_t)P.N;
        const uint32_t o = P.gc_off[gi], c = P.gc_cnt[gi];
        uint32_t s = 0;
        for (uint32_t i = 0; i < c; i++) {
            const uint32_t nh = P.cand_nh[o + i];
            if (!nh) continue;
            s += (P.cand_hsp[o + i].strand & HSP_FWD) ? 1u : 0u;
            const uint32_t ov = P.cand_ovf[o + i];
            for (uint32_t k = 1; k < nh; k++) s += (P.ovf[ov + k - 1].strand & HSP_FWD) ? 1u : 0u;
        }
        P.cnt[si] = s;
    }
}

__global__ void group_write_kernel(GroupParams P)
{
    const uint64_t sg = (uint64_t)(P.gene_end - P.gene_begin), n = sg * (uint64_t)P.N;
    for (uint64_t gi = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; gi < n;
         gi += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t si = (gi % (uint64_t)P.N) * sg + gi / (uint64_t)P.N;
        const uint32_t o = P.gc_off[gi], c = P.gc_cnt[gi];
        uint64_t w = P.base + P.scan[si];
        const uint64_t gg = grp_index(P.gene_begin + (uint32_t)(si % sg), (int)(si / sg), P.n_genes);
        if (P.cnt[si]) {
            P.grp_off[gg] = (uint32_t)w;
            P.grp_cnt[gg] = P.cnt[si];
        }
        for (uint32_t i = 0; i < c; i++) {
            const uint32_t nh = P.cand_nh[o + i];
            if (!nh) continue;
            const DHsp &h0 = P.cand_hsp[o + i];
            if (h0.strand & HSP_FWD) P.out[w++] = h0;
            const uint32_t ov = P.cand_ovf[o + i];
            for (uint32_t k = 1; k < nh; k++)
                if (P.ovf[ov + k - 1].strand & HSP_FWD) P.out[w++] = P.ovf[ov + k - 1];
        }
    }
}

// the mirror image of a query->subject HSP, as the subject->query search reports it
__device__ __forceinline__ DHsp mirror_hsp(const DHsp &h)
{
    DHsp m = h;
    m.q_tx = h.s_tx;
    m.s_tx = h.q_tx;
    if (!(h.strand & 1)) {
        m.qstart = h.sstart; m.qend = h.send; m.sstart = h.qstart; m.send = h.qend;
    } else {
        m.qstart = h.send; m.qend = h.sstart; m.sstart = h.qend; m.send = h.qstart;
    }
    return m;
}

// candidate slot of linear candidate index li
__device__ __forceinline__ uint64_t cand_slot(const GroupParams &P, uint64_t li)
{
    int lo = 0, hi = NSHARD;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P.shard_prefix[mid] <= li) lo = mid; else hi = mid;
    }
    return (uint64_t)lo * P.cand_cap + (li - P.shard_prefix[lo]);
}

// pass 0: count mirrored HSPs per (gene of the subject tx, query sample),
// one atomic per candidate (its HSPs share the group), whose return -- the
// candidate's first slot in the group -- is kept per candidate; pass 1:
// scatter them from there, no atomics (the order inside a group is fixed
// later by mirror_sort_kernel)
__global__ void mirror_scatter_kernel(GroupParams P, int pass)
{
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < P.n_cand;
         li += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t ci = cand_slot(P, li);
        const uint32_t nh = P.cand_nh[ci];
        if (!nh) continue;
        const uint32_t ov = P.cand_ovf[ci];
        uint64_t gi = 0, slot = 0;
        uint32_t c = 0;
        for (uint32_t k = 0; k < nh; k++) {
            const DHsp &h = k ? P.ovf[ov + k - 1] : P.cand_hsp[ci];
            if (!(h.strand & HSP_REV)) continue;
            // the reverse search's query tx (its gene and isoform position) and subject tx
            const uint32_t rq = h.s_tx, rs = h.q_tx;
            if (c == 0) {
                gi = (uint64_t)(P.tx[rs].sample - P.ms0) * P.mgw + (P.tx_gene[rq] - P.mg0);   // (the tile's window)
                if (pass == 1) slot = P.mbase + P.mscan[gi] + P.mcur[li];
            }
            c++;
            if (pass == 0) continue;
            P.out[slot] = mirror_hsp(h);
            // order: (isoform position, strand) then (subject tx, index)
            P.mkey[2 * (slot - P.mbase)] = ((uint64_t)P.tx_pos[rq] << 1) | (uint64_t)(h.strand & 1);
            P.mkey[2 * (slot - P.mbase) + 1] = ((uint64_t)rs << 8) | (uint64_t)((h.strand >> HSP_IDX_SHIFT) & 7);
            slot++;
        }
        if (pass == 0 && c) P.mcur[li] = atomicAdd(&P.mcnt[gi], c);
    }
}

// sort each mirrored group by its order keys and fill the group table:
// groups of up to MSORT_SMALL entries (nearly all) by one thread's insertion
// sort; larger ones -- an isoform-rich gene against an isoform-rich ortholog
// holds tens of thousands -- go on a list for mirror_sort_big_kernel
constexpr uint32_t MSORT_SMALL = 32;
__global__ void mirror_sort_kernel(GroupParams P)
{
    const uint64_t n = (uint64_t)P.mgw * (uint64_t)P.msn;
    for (uint64_t gi = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; gi < n;
         gi += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = P.mcnt[gi];
        if (!c) continue;
        const uint64_t b = P.mscan[gi];
        // the window's (sample, gene) in the whole group table
        const uint64_t gg = grp_index(P.mg0 + (uint32_t)(gi % P.mgw), P.ms0 + (int)(gi / P.mgw), P.n_genes);
        P.grp_off[gg] = (uint32_t)(P.mbase + b);
        P.grp_cnt[gg] = c;
        if (c > MSORT_SMALL) {
            const unsigned long long k = atomicAdd(P.mbig_n, 1ull);
            P.mbig[k] = gi;   // capacity: nm / (MSORT_SMALL + 1) + 1 entries
            continue;
        }
        for (uint32_t i = 1; i < c; i++) {
            const uint64_t k1 = P.mkey[2 * (b + i)], k2 = P.mkey[2 * (b + i) + 1];
            const DHsp h = P.out[P.mbase + b + i];
            uint32_t j = i;
            while (j > 0) {
                const uint64_t p1 = P.mkey[2 * (b + j - 1)], p2 = P.mkey[2 * (b + j - 1) + 1];
                if (p1 < k1 || (p1 == k1 && p2 < k2)) break;
                P.mkey[2 * (b + j)] = p1;
                P.mkey[2 * (b + j) + 1] = p2;
                P.out[P.mbase + b + j] = P.out[P.mbase + b + j - 1];
                j--;
            }
            P.mkey[2 * (b + j)] = k1;
            P.mkey[2 * (b + j) + 1] = k2;
            P.out[P.mbase + b + j] = h;
        }
    }
}

// One workgroup per large mirrored group (persistent over the list): an
// in-place bitonic network over the group's c entries, ascending in every
// merge (the first stage of each merge compares mirrored positions), so the
// virtual +inf padding past c never moves and its comparators are skipped.
// Keys are unique per group: (isoform position, strand, subject tx, index).
__global__ __launch_bounds__(256) void mirror_sort_big_kernel(GroupParams P)
{
    const uint64_t nb = *P.mbig_n;
    for (uint64_t q = blockIdx.x; q < nb; q += gridDim.x) {
        const uint64_t gi = P.mbig[q];
        const uint32_t c = P.mcnt[gi];
        const uint64_t b = P.mscan[gi];
        uint64_t *K = P.mkey + 2 * b;
        DHsp *H = P.out + P.mbase + b;
        uint32_t np2 = 1;
        while (np2 < c) np2 <<= 1;
        auto cmpx = [&](uint32_t i, uint32_t j) {   // i < j: the smaller key to i
            if (j >= c) return;
            const uint64_t a1 = K[2 * i], a2 = K[2 * i + 1], b1 = K[2 * j], b2 = K[2 * j + 1];
            if (a1 > b1 || (a1 == b1 && a2 > b2)) {
                K[2 * i] = b1; K[2 * i + 1] = b2; K[2 * j] = a1; K[2 * j + 1] = a2;
                const DHsp t = H[i];
                H[i] = H[j];
                H[j] = t;
            }
        };
        for (uint32_t kk = 2; kk <= np2; kk <<= 1) {
            // flip stage: i in the lower half of a kk-block against its mirror
            for (uint32_t t = threadIdx.x; t < np2 / 2; t += blockDim.x) {
                const uint32_t blk = t / (kk / 2), off = t % (kk / 2);
                const uint32_t i = blk * kk + off, j = blk * kk + kk - 1 - off;
                cmpx(i, j);
            }
            __syncthreads();
            for (uint32_t j2 = kk / 4; j2 > 0; j2 >>= 1) {   // half-cleaners
                for (uint32_t t = threadIdx.x; t < np2 / 2; t += blockDim.x) {
                    const uint32_t blk = t / j2, off = t % j2;
                    const uint32_t i = blk * 2 * j2 + off;
                    cmpx(i, i + j2);
                }
                __syncthreads();
            }
        }
    }
}

void launch_group(const GroupParams &P, GroupPass pass, hipStream_t st)
{
    const bool mirror_cand = pass == GROUP_MIRROR_COUNT || pass == GROUP_MIRROR_SCATTER;
    uint64_t n = (uint64_t)(P.gene_end - P.gene_begin) * (uint64_t)P.N;
    if (mirror_cand) n = P.n_cand;
    if (pass == GROUP_MIRROR_SORT) n = (uint64_t)P.mgw * (uint64_t)P.msn;
    if (!n) return;
    uint64_t g = (n + 255) / 256;
    if (g > 65536) g = 65536;
    if (pass == GROUP_DIRECT_COUNT)
        hipLaunchKernelGGL(group_count_kernel, dim3((unsigned)g), dim3(256), 0, st, P);
    else if (pass == GROUP_DIRECT_WRITE)
        hipLaunchKernelGGL(group_write_kernel, dim3((unsigned)g), dim3(256), 0, st, P);
    else if (mirror_cand)   // the kernel's pass: 0 count, 1 scatter
        hipLaunchKernelGGL(mirror_scatter_kernel, dim3((unsigned)g), dim3(256), 0, st, P,
                           pass == GROUP_MIRROR_SCATTER ? 1 : 0);
    else {
        hipLaunchKernelGGL(mirror_sort_kernel, dim3((unsigned)g), dim3(256), 0, st, P);
        hipLaunchKernelGGL(mirror_sort_big_kernel, dim3(1024), dim3(256), 0, st, P);
    }
}

}  // namespace rcg
