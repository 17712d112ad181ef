// Analyses of a finished engine's graph: per-component tables, bootstrap
// resampling, neighbour-joining trees, the census of their splits, principal
// coordinates, group tests, PERMDISP and the Mantel test (kernels:
// components.hip, nj.hip, splits.hip, pcoa.hip, groups.hip, dispersion.hip,
// mantel.hip).
#include "engine.h"

// ------------------------------------------------------------------------
// per-component tables and resampling (kernels: components.hip)
// ------------------------------------------------------------------------

enum { CS_MEMBERS = 0, CS_MAXCELL = 1, CS_BAD = 2, CS_N = 4 };   // slots of d_cstat

// The tables of the finished graph phase, built once per graph: ranks (the
// exclusive scan of d_ideal), members, sums, their packed copy and the largest
// cell. They stay on the device until the next do_graph.
static int build_components(rc_engine *e)
{
    if (!e->finished) return fail(RC_E_STATE, "no results yet");
    if (e->an.comp_valid) return RC_OK;
    CHK(set_device(e));
    const uint32_t ng = (uint32_t)e->gene_sample.size();
    const uint64_t P = e->pair_a.size();
    const uint64_t S = e->h_stats[4];
    uint64_t C = 0;
    CHK(e->an.d_crank.ensure(ng));
    CHK(e->an.d_cstat.ensure(CS_N));
    HIPCHK(hipMemsetAsync(e->an.d_cstat.p, 0, CS_N * sizeof(unsigned long long), e->st));
    if (ng) {
        size_t tmp = 0;
        HIPCHK(rocprim::exclusive_scan(nullptr, tmp, e->d_ideal.p, e->an.d_crank.p, 0u, (size_t)ng,
                                       rocprim::plus<uint32_t>(), e->st));
        CHK(e->work.d_tmp.ensure(tmp));
        HIPCHK(rocprim::exclusive_scan(e->work.d_tmp.p, tmp, e->d_ideal.p, e->an.d_crank.p, 0u, (size_t)ng,
                                       rocprim::plus<uint32_t>(), e->st));
        uint32_t last_rank = 0;
        uint8_t last_ideal = 0;
        HIPCHK(hipMemcpyAsync(&last_rank, e->an.d_crank.p + ng - 1, 4, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(&last_ideal, e->d_ideal.p + ng - 1, 1, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipStreamSynchronize(e->st));
        C = (uint64_t)last_rank + last_ideal;
    }
    if (C != e->h_stats[1]) return fail(RC_E_STATE, "the ideal[] scan disagrees with the ideal component count");
    if (C && !S) return fail(RC_E_STATE, "ideal components without a sample count");
    // members: sort (component id, gene) keys, the members come first
    const uint64_t nm = C * S;
    CHK(e->an.d_cmember.ensure(nm));
    if (nm) {
        DBuf<uint64_t> k0, k1;
        CHK(k0.ensure(ng));
        CHK(k1.ensure(ng));
        launch_comp_keys(e->d_parent.p, e->d_present.p, e->d_ideal.p, e->an.d_crank.p, ng, k0.p,
                         e->an.d_cstat.p + CS_MEMBERS, e->st);
        HIPCHK(hipGetLastError());
        size_t tmp = 0;
        HIPCHK(rocprim::radix_sort_keys(nullptr, tmp, k0.p, k1.p, (size_t)ng, 0u, 64u, e->st));
        CHK(e->work.d_tmp.ensure(tmp));
        HIPCHK(rocprim::radix_sort_keys(e->work.d_tmp.p, tmp, k0.p, k1.p, (size_t)ng, 0u, 64u, e->st));
        unsigned long long members = 0;
        HIPCHK(hipMemcpyAsync(&members, e->an.d_cstat.p + CS_MEMBERS, 8, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipStreamSynchronize(e->st));
        if (members != nm) return fail(RC_E_STATE, "ideal components do not hold sample_count members each");
        launch_comp_members(k1.p, nm, (uint32_t)S, e->an.d_cmember.p, e->an.d_cstat.p + CS_BAD, e->st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(e->st));   // k0, k1 go out of scope
    }
    // sums, packed cells, largest cell
    const uint64_t cells = C * P;
    CHK(e->an.d_cnum.ensure(cells));
    CHK(e->an.d_cden.ensure(cells));
    CHK(e->an.d_ccell.ensure(cells));
    if (cells) {
        HIPCHK(hipMemsetAsync(e->an.d_cnum.p, 0, cells * 8, e->st));
        HIPCHK(hipMemsetAsync(e->an.d_cden.p, 0, cells * 8, e->st));
        launch_comp_sums(e->d_edges.p, e->n_edges, e->d_parent.p, e->d_ideal.p, e->an.d_crank.p, P, e->an.d_cnum.p,
                         e->an.d_cden.p, e->st);
        launch_comp_pack(e->an.d_cnum.p, e->an.d_cden.p, cells, e->an.d_ccell.p, e->an.d_cstat.p + CS_MAXCELL, e->st);
        HIPCHK(hipGetLastError());
    }
    unsigned long long st[CS_N] = {};
    HIPCHK(hipMemcpyAsync(st, e->an.d_cstat.p, sizeof st, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    if (st[CS_BAD]) return fail(RC_E_STATE, "ideal components do not hold sample_count members each");
    e->an.comp_n = C;
    e->an.comp_S = (uint32_t)S;
    e->an.comp_max_cell = st[CS_MAXCELL];
    e->an.comp_valid = true;
    return RC_OK;
}

// The census of the finished graph phase, built once per graph: the census id
// of every root (the exclusive scan of the root flag), the members (sorted
// (census id, gene) keys of the present genes) and the rows root, nodes,
// edges, samples. They stay on the device until the next do_graph.
static int build_census(rc_engine *e)
{
    if (!e->finished) return fail(RC_E_STATE, "no results yet");
    CHK(set_device(e));
    if (e->an.census_valid) return RC_OK;
    const uint32_t ng = (uint32_t)e->gene_sample.size();
    uint64_t K = 0;
    unsigned long long present = 0;
    DBuf<uint32_t> flag, rank;
    DBuf<uint64_t> k0, k1;
    CHK(e->an.d_cstat.ensure(CS_N));
    if (ng) {
        CHK(flag.ensure(ng));
        CHK(rank.ensure(ng));
        CHK(k0.ensure(ng));
        CHK(k1.ensure(ng));
        HIPCHK(hipMemsetAsync(e->an.d_cstat.p + CS_MEMBERS, 0, sizeof(unsigned long long), e->st));
        launch_census_flags(e->d_parent.p, e->d_present.p, ng, flag.p, e->st);
        HIPCHK(hipGetLastError());
        size_t tmp = 0;
        HIPCHK(rocprim::exclusive_scan(nullptr, tmp, flag.p, rank.p, 0u, (size_t)ng, rocprim::plus<uint32_t>(), e->st));
        CHK(e->work.d_tmp.ensure(tmp));
        HIPCHK(rocprim::exclusive_scan(e->work.d_tmp.p, tmp, flag.p, rank.p, 0u, (size_t)ng,
                                       rocprim::plus<uint32_t>(), e->st));
        launch_census_keys(e->d_parent.p, e->d_present.p, rank.p, ng, k0.p, e->an.d_cstat.p + CS_MEMBERS, e->st);
        HIPCHK(hipGetLastError());
        HIPCHK(rocprim::radix_sort_keys(nullptr, tmp, k0.p, k1.p, (size_t)ng, 0u, 64u, e->st));
        CHK(e->work.d_tmp.ensure(tmp));
        HIPCHK(rocprim::radix_sort_keys(e->work.d_tmp.p, tmp, k0.p, k1.p, (size_t)ng, 0u, 64u, e->st));
        uint32_t last_rank = 0, last_flag = 0;
        HIPCHK(hipMemcpyAsync(&last_rank, rank.p + ng - 1, 4, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(&last_flag, flag.p + ng - 1, 4, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(&present, e->an.d_cstat.p + CS_MEMBERS, 8, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipStreamSynchronize(e->st));
        K = (uint64_t)last_rank + last_flag;
    }
    if (K != e->h_stats[0]) return fail(RC_E_STATE, "the root scan disagrees with the component count");
    if (present != e->h_stats[3]) return fail(RC_E_STATE, "the member keys disagree with the node count");
    CHK(e->an.d_zroot.ensure(K));
    CHK(e->an.d_znodes.ensure(K));
    CHK(e->an.d_zedges.ensure(K));
    CHK(e->an.d_zsamples.ensure(K));
    CHK(e->an.d_zmember.ensure(present));
    if (K) {
        launch_census_table(flag.p, rank.p, e->d_cnodes.p, e->d_cedges.p, ng, e->an.d_zroot.p, e->an.d_znodes.p,
                            e->an.d_zedges.p, e->an.d_zsamples.p, e->st);
        launch_census_members(k1.p, present, e->d_gene_sample.p, e->an.d_zmember.p, e->an.d_zsamples.p, e->st);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(e->st));   // flag, rank, k0, k1 go out of scope
    e->an.census_n = K;
    e->an.census_members = present;
    e->an.census_valid = true;
    return RC_OK;
}

extern "C" {

int rc_components(rc_engine *e, int32_t *root_sample, int32_t *root_gene, int64_t *nodes, int64_t *edges,
                  int32_t *samples, uint64_t cap, uint64_t *n_comp)
{
    if (!e || !n_comp) return fail(RC_E_ARG, "null argument");
    CHK(build_census(e));
    const uint64_t K = e->an.census_n;
    *n_comp = K;
    const int given = !!root_sample + !!root_gene + !!nodes + !!edges + !!samples;
    if (!given) return RC_OK;
    if (given != 5) return fail(RC_E_ARG, "null argument");
    if (cap < K) return fail(RC_E_CAPACITY, "buffer too small");
    if (!K) return RC_OK;
    std::vector<uint32_t> h[4];
    const uint32_t *src[4] = {e->an.d_zroot.p, e->an.d_znodes.p, e->an.d_zedges.p, e->an.d_zsamples.p};
    for (int i = 0; i < 4; i++) {
        h[i].resize(K);
        HIPCHK(hipMemcpyAsync(h[i].data(), src[i], K * 4, hipMemcpyDeviceToHost, e->st));
    }
    HIPCHK(hipStreamSynchronize(e->st));
    for (uint64_t c = 0; c < K; c++) {
        root_sample[c] = e->gene_sample[h[0][c]];
        root_gene[c] = e->gene_id[h[0][c]];
        nodes[c] = h[1][c];
        edges[c] = h[2][c];
        samples[c] = (int32_t)h[3][c];
    }
    return RC_OK;
}

int rc_component_members(rc_engine *e, int32_t *sample, int32_t *gene, uint64_t cap, uint64_t *n_nodes)
{
    if (!e || !n_nodes) return fail(RC_E_ARG, "null argument");
    CHK(build_census(e));
    const uint64_t nm = e->an.census_members;
    *n_nodes = nm;
    if (!sample && !gene) return RC_OK;
    if (!sample || !gene) return fail(RC_E_ARG, "null argument");
    if (cap < nm) return fail(RC_E_CAPACITY, "buffer too small");
    if (!nm) return RC_OK;
    std::vector<uint32_t> m(nm);
    HIPCHK(hipMemcpyAsync(m.data(), e->an.d_zmember.p, nm * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    for (uint64_t i = 0; i < nm; i++) {
        sample[i] = e->gene_sample[m[i]];
        gene[i] = e->gene_id[m[i]];
    }
    return RC_OK;
}

int rc_ideal_components(rc_engine *e, int32_t *sample, int32_t *gene, uint64_t cap_nodes, uint64_t *n_comp,
                        int32_t *sample_count)
{
    if (!e || !n_comp || !sample_count) return fail(RC_E_ARG, "null argument");
    CHK(build_components(e));
    *n_comp = e->an.comp_n;
    *sample_count = (int32_t)e->an.comp_S;
    if (!sample && !gene) return RC_OK;
    if (!sample || !gene) return fail(RC_E_ARG, "null argument");
    const uint64_t nm = e->an.comp_n * e->an.comp_S;
    if (cap_nodes < nm) return fail(RC_E_CAPACITY, "buffer too small");
    if (!nm) return RC_OK;
    std::vector<uint32_t> m(nm);
    HIPCHK(hipMemcpy(m.data(), e->an.d_cmember.p, nm * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < nm; i++) {
        sample[i] = e->gene_sample[m[i]];
        gene[i] = e->gene_id[m[i]];
    }
    return RC_OK;
}

int rc_component_sums(rc_engine *e, int64_t *num, int64_t *den, uint64_t cap_cells, uint64_t *n_comp,
                      uint64_t *n_pairs)
{
    if (!e || !n_comp || !n_pairs) return fail(RC_E_ARG, "null argument");
    CHK(build_components(e));
    *n_comp = e->an.comp_n;
    *n_pairs = e->pair_a.size();
    if (!num && !den) return RC_OK;
    if (!num || !den) return fail(RC_E_ARG, "null argument");
    const uint64_t cells = e->an.comp_n * e->pair_a.size();
    if (cap_cells < cells) return fail(RC_E_CAPACITY, "buffer too small");
    if (!cells) return RC_OK;
    HIPCHK(hipMemcpy(num, e->an.d_cnum.p, cells * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(den, e->an.d_cden.p, cells * 8, hipMemcpyDeviceToHost));
    return RC_OK;
}

}  // extern "C"

// rc_resample up to the filled device buffers: the replicate sums in d_rnum /
// d_rden and, with `dist`, the n_rep x n x n distances in d_dist with their
// status word in d_status (queued on the stream, not waited for). Events
// EV_RESAMPLE0, EV_RESAMPLE1.
static int resample_fill(rc_engine *e, const uint16_t *weights, int32_t n_rep, uint64_t n_comp, const int32_t *order,
                         int32_t n, bool dist, bool sums_paired)
{
    CHK(build_components(e));
    const uint64_t C = e->an.comp_n, P = e->pair_a.size();
    const int N = (int)e->samples.size();
    if (n_comp != C) return fail(RC_E_ARG, "n_comp is not the number of ideal components");
    if (n_rep < 1) return fail(RC_E_ARG, "n_rep must be >= 1");
    if (C && !weights) return fail(RC_E_ARG, "null argument");
    if (!sums_paired) return fail(RC_E_ARG, "num and den go together");
    if (n < 0 || n > N || (dist && n && !order)) return fail(RC_E_ARG, "bad sample count");
    if (dist) {
        std::vector<int> seen(N, 0);
        for (int i = 0; i < n; i++) {
            if (order[i] < 0 || order[i] >= N || seen[order[i]])
                return fail(RC_E_ARG, "order must hold distinct sample ids");
            seen[order[i]] = 1;
        }
    }
    if (e->an.comp_max_cell >> 32) return fail(RC_E_LIMIT, "a component sum of 2^32 or more (stacked sums-only records)");
    const uint64_t R = (uint64_t)n_rep;
    uint16_t maxw = 0;
    for (uint64_t i = 0, nw = R * C; i < nw; i++) maxw = std::max(maxw, weights[i]);
    unsigned long long maxden = 0;
    for (unsigned long long d : e->h_den) maxden = std::max(maxden, d);
    // max weight x largest pair denominator bounds every replicate sum
    if (maxw && maxden >= ((1ull << 63) + maxw - 1) / maxw)
        return fail(RC_E_LIMIT, "weights this large could overflow the 64-bit replicate sums");
    CHK(set_device(e));
    const uint64_t cells = R * P;
    CHK(e->an.d_rweight.ensure(R * C));
    CHK(e->an.d_rnum.ensure(cells));
    CHK(e->an.d_rden.ensure(cells));
    if (R * C) HIPCHK(hipMemcpyAsync(e->an.d_rweight.p, weights, R * C * 2, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipEventRecord(e->ev[EV_RESAMPLE0], e->st));
    if (cells) {
        HIPCHK(hipMemsetAsync(e->an.d_rnum.p, 0, cells * 8, e->st));
        HIPCHK(hipMemsetAsync(e->an.d_rden.p, 0, cells * 8, e->st));
        if (!launch_resample(e->an.d_ccell.p, e->an.d_rweight.p, C, P, (uint32_t)n_rep, e->an.d_rnum.p, e->an.d_rden.p, e->st))
            return fail(RC_E_LIMIT, "n_rep x pairs beyond the resample grid");
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(e->ev[EV_RESAMPLE1], e->st));
    const uint64_t nd = dist ? R * (uint64_t)n * (uint64_t)n : 0;
    if (nd) {
        CHK(e->d_order.ensure(n));
        CHK(e->d_dist.ensure(nd));
        HIPCHK(hipMemcpyAsync(e->d_order.p, order, (size_t)n * 4, hipMemcpyHostToDevice, e->st));
        HIPCHK(hipMemsetAsync(e->d_status.p, 0, sizeof(unsigned int), e->st));
        launch_resample_distance(e->an.d_rnum.p, e->an.d_rden.p, e->d_pair_index.p, e->d_order.p, N, n, R, P, e->d_dist.p,
                                 e->d_status.p, e->st);
        HIPCHK(hipGetLastError());
    }
    return RC_OK;
}

extern "C" {

int rc_resample(rc_engine *e, const uint16_t *weights, int32_t n_rep, uint64_t n_comp, const int32_t *order,
                int32_t n, double *out, int64_t *num, int64_t *den)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    CHK(resample_fill(e, weights, n_rep, n_comp, order, n, out != nullptr, (num == nullptr) == (den == nullptr)));
    const uint64_t cells = (uint64_t)n_rep * e->pair_a.size();
    const uint64_t nd = out ? (uint64_t)n_rep * (uint64_t)n * (uint64_t)n : 0;
    unsigned int status = 0;
    if (nd) {
        HIPCHK(hipMemcpyAsync(out, e->d_dist.p, nd * 8, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(&status, e->d_status.p, 4, hipMemcpyDeviceToHost, e->st));
    }
    if (num && cells) {
        HIPCHK(hipMemcpyAsync(num, e->an.d_rnum.p, cells * 8, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(den, e->an.d_rden.p, cells * 8, hipMemcpyDeviceToHost, e->st));
    }
    HIPCHK(hipStreamSynchronize(e->st));
    e->tm.resample_ms = ev_ms(e, EV_RESAMPLE0, EV_RESAMPLE1);
    if (status & ST_NO_IDEAL) return fail(RC_E_NO_IDEAL, "No ideal components found. Cannot report distances!");
    return RC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------
// neighbour joining (nj.hip)
// ------------------------------------------------------------------------

static const int NJ_MAX_SAMPLES = 1024;
static const uint64_t NJ_WS_BYTES = 1ull << 30;   // workspace of the trees too large for LDS

// the argument checks of rc_nj / rc_resample_trees (no device work)
static int nj_check(int32_t n_rep, int32_t n, const uint64_t *ref, int32_t n_ref, const uint32_t *support)
{
    if (n < 3) return fail(RC_E_ARG, "a tree needs at least 3 samples");
    if (n_rep < 1) return fail(RC_E_ARG, "n_rep must be >= 1");
    if (n > NJ_MAX_SAMPLES) return fail(RC_E_LIMIT, "more than 1024 samples in a neighbour-joining tree");
    if (n_ref < 0 || (n_ref > 0 && !ref)) return fail(RC_E_ARG, "bad reference splits");
    if (support && !ref) return fail(RC_E_ARG, "support needs ref_splits");
    const int W = (n + 63) / 64;
    for (int64_t k = 0; k < n_ref; k++) {
        if (ref[k * W] & 1ull) return fail(RC_E_ARG, "a reference split holds position 0 (pass the other side)");
        if ((n & 63) && ref[k * W + W - 1] >> (n & 63))
            return fail(RC_E_ARG, "a reference split has bits at or above the sample count");
    }
    return RC_OK;
}

// Trees of the n_rep matrices at dD (device, n x n each) and the support of
// the reference splits; the arguments have passed nj_check. Events EV_NJ0,
// EV_NJ1. *invalid: the number of matrices with a non-finite entry.
static int nj_device(rc_engine *e, const double *dD, int32_t n_rep, int32_t n, int32_t *joins, double *lengths,
                     uint64_t *splits, uint8_t *valid, const uint64_t *ref, int32_t n_ref, uint32_t *support,
                     uint32_t *n_valid, uint32_t *invalid)
{
    const int W = (n + 63) / 64;
    const size_t R = (size_t)n_rep, nj = R * (size_t)(n - 2) * 3, ns = R * (size_t)(n - 3) * W;
    e->an.nj_n = 0;   // the trees on the device go, and the census of their splits with them
    e->an.split_valid = false;
    CHK(e->an.d_nj_joins.ensure(nj));
    CHK(e->an.d_nj_len.ensure(nj));
    CHK(e->an.d_nj_splits.ensure(ns));
    CHK(e->an.d_nj_valid.ensure(R));
    CHK(e->an.d_nj_ref.ensure((size_t)n_ref * W));
    CHK(e->an.d_nj_sup.ensure((size_t)n_ref + 1));
    int lds_max = 0;
    HIPCHK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, e->o.device));
    const bool lds = n <= e->knobs.nj_lds && nj_lds_bytes(true, n, W) <= (size_t)lds_max;
    const size_t per = (size_t)n * n * 8 + (size_t)n * W * 8;
    const size_t chunk = lds ? R : std::max<size_t>(1, std::min<size_t>(R, NJ_WS_BYTES / per));
    if (!lds) {
        CHK(e->an.d_nj_wsm.ensure(chunk * n * n));
        CHK(e->an.d_nj_wsmask.ensure(chunk * n * W));
    }
    if (n_ref) HIPCHK(hipMemcpyAsync(e->an.d_nj_ref.p, ref, (size_t)n_ref * W * 8, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemsetAsync(e->an.d_nj_sup.p, 0, ((size_t)n_ref + 1) * 4, e->st));
    HIPCHK(hipEventRecord(e->ev[EV_NJ0], e->st));
    for (size_t r0 = 0; r0 < R; r0 += chunk) {
        const size_t rc = std::min(chunk, R - r0);
        const hipError_t err = launch_nj(lds, dD + r0 * n * n, (int)rc, n, W, e->an.d_nj_wsm.p, e->an.d_nj_wsmask.p,
                                         e->an.d_nj_joins.p + r0 * (n - 2) * 3, e->an.d_nj_len.p + r0 * (n - 2) * 3,
                                         e->an.d_nj_splits.p + r0 * (n - 3) * W, e->an.d_nj_valid.p + r0, e->st);
        if (err != hipSuccess)
            return fail(RC_E_HIP, std::string("nj_kernel (") + std::to_string(nj_lds_bytes(lds, n, W)) +
                                      " bytes of LDS): " + hipGetErrorString(err));
    }
    launch_nj_support(e->an.d_nj_ref.p, n_ref, e->an.d_nj_splits.p, e->an.d_nj_valid.p, n_rep, n - 3, W, e->an.d_nj_sup.p,
                      e->an.d_nj_sup.p + n_ref, e->st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[EV_NJ1], e->st));
    uint32_t nv = 0;
    if (joins) HIPCHK(hipMemcpyAsync(joins, e->an.d_nj_joins.p, nj * 4, hipMemcpyDeviceToHost, e->st));
    if (lengths) HIPCHK(hipMemcpyAsync(lengths, e->an.d_nj_len.p, nj * 8, hipMemcpyDeviceToHost, e->st));
    if (splits && ns) HIPCHK(hipMemcpyAsync(splits, e->an.d_nj_splits.p, ns * 8, hipMemcpyDeviceToHost, e->st));
    if (valid) HIPCHK(hipMemcpyAsync(valid, e->an.d_nj_valid.p, R, hipMemcpyDeviceToHost, e->st));
    if (support && n_ref)
        HIPCHK(hipMemcpyAsync(support, e->an.d_nj_sup.p, (size_t)n_ref * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(&nv, e->an.d_nj_sup.p + n_ref, 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    e->tm.nj_ms = ev_ms(e, EV_NJ0, EV_NJ1);
    e->an.nj_rep = n_rep;
    e->an.nj_n = n;
    e->an.nj_nvalid = nv;
    if (n_valid) *n_valid = nv;
    *invalid = (uint32_t)n_rep - nv;
    return RC_OK;
}

extern "C" {

int rc_nj(rc_engine *e, const double *D, int32_t n_rep, int32_t n, int32_t *joins, double *lengths, uint64_t *splits,
          uint8_t *valid, const uint64_t *ref_splits, int32_t n_ref, uint32_t *support, uint32_t *n_valid)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    CHK(nj_check(n_rep, n, ref_splits, n_ref, support));
    if (!D) return fail(RC_E_ARG, "null argument");
    CHK(set_device(e));
    const size_t nd = (size_t)n_rep * n * n;
    CHK(e->an.d_nj_in.ensure(nd));
    HIPCHK(hipMemcpyAsync(e->an.d_nj_in.p, D, nd * 8, hipMemcpyHostToDevice, e->st));
    uint32_t invalid = 0;
    CHK(nj_device(e, e->an.d_nj_in.p, n_rep, n, joins, lengths, splits, valid, ref_splits, n_ref, support, n_valid,
                  &invalid));
    if (invalid) return fail(RC_E_NO_IDEAL, "a distance matrix has a non-finite entry: no tree for it");
    return RC_OK;
}

int rc_resample_trees(rc_engine *e, const uint16_t *weights, int32_t n_rep, uint64_t n_comp, const int32_t *order,
                      int32_t n, int32_t *joins, double *lengths, uint64_t *splits, uint8_t *valid,
                      const uint64_t *ref_splits, int32_t n_ref, uint32_t *support, uint32_t *n_valid)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    CHK(nj_check(n_rep, n, ref_splits, n_ref, support));
    CHK(resample_fill(e, weights, n_rep, n_comp, order, n, true, true));
    uint32_t invalid = 0;
    CHK(nj_device(e, e->d_dist.p, n_rep, n, joins, lengths, splits, valid, ref_splits, n_ref, support, n_valid,
                  &invalid));
    e->tm.resample_ms = ev_ms(e, EV_RESAMPLE0, EV_RESAMPLE1);
    if (invalid) return fail(RC_E_NO_IDEAL, "No ideal components found. Cannot report distances!");
    return RC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------
// split census and Robinson-Foulds distances (splits.hip)
// ------------------------------------------------------------------------

static const int32_t RF_MAX_PAIRWISE = 8192;   // replicates of a pairwise matrix (256 MB)

// The census of the splits that the last nj_device left in d_nj_splits /
// d_nj_valid, built once per batch of trees: the hash table, the rank and the
// class id of every instance, count and first instance of every class. It
// stays on the device until the next nj_device.
static int build_splits(rc_engine *e)
{
    rc_engine::Analysis &a = e->an;
    if (!a.nj_n) return fail(RC_E_STATE, "no trees on this engine yet (rc_nj, rc_resample_trees)");
    CHK(set_device(e));
    if (a.split_valid) return RC_OK;
    const uint64_t ns = (uint64_t)(a.nj_n - 3), ni = (uint64_t)a.nj_rep * ns;
    if (ni >> 31) return fail(RC_E_LIMIT, "2^31 or more splits in the replicate trees");
    const int W = (a.nj_n + 63) / 64;
    uint64_t K = 0, slots = 0;
    DBuf<uint32_t> rep, flag;
    CHK(a.d_sp_ids.ensure(ni));
    CHK(a.d_sp_rank.ensure(ni));
    if (ni) {
        slots = split_table_slots(ni);
        CHK(a.d_sp_table.ensure(slots));
        CHK(rep.ensure(ni));
        CHK(flag.ensure(ni));
        HIPCHK(hipMemsetAsync(a.d_sp_table.p, 0xFF, slots * 4, e->st));
        launch_split_insert(a.d_nj_splits.p, a.d_nj_valid.p, (uint32_t)ni, (uint32_t)ns, W, a.d_sp_table.p, slots, e->st);
        launch_split_lookup(a.d_nj_splits.p, a.d_nj_valid.p, (uint32_t)ni, (uint32_t)ns, W, a.d_sp_table.p, slots, rep.p,
                            flag.p, e->st);
        HIPCHK(hipGetLastError());
        size_t tmp = 0;
        HIPCHK(rocprim::exclusive_scan(nullptr, tmp, flag.p, a.d_sp_rank.p, 0u, (size_t)ni, rocprim::plus<uint32_t>(),
                                       e->st));
        CHK(e->work.d_tmp.ensure(tmp));
        HIPCHK(rocprim::exclusive_scan(e->work.d_tmp.p, tmp, flag.p, a.d_sp_rank.p, 0u, (size_t)ni,
                                       rocprim::plus<uint32_t>(), e->st));
        uint32_t last_rank = 0, last_flag = 0;
        HIPCHK(hipMemcpyAsync(&last_rank, a.d_sp_rank.p + ni - 1, 4, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(&last_flag, flag.p + ni - 1, 4, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipStreamSynchronize(e->st));
        K = (uint64_t)last_rank + last_flag;
    }
    CHK(a.d_sp_count.ensure(K));
    CHK(a.d_sp_first.ensure(K));
    if (K) {
        HIPCHK(hipMemsetAsync(a.d_sp_count.p, 0, K * 4, e->st));
        launch_split_ids(rep.p, a.d_sp_rank.p, (uint32_t)ni, a.d_sp_ids.p, a.d_sp_count.p, a.d_sp_first.p, e->st);
        HIPCHK(hipGetLastError());
    } else if (ni) {
        HIPCHK(hipMemsetAsync(a.d_sp_ids.p, 0xFF, ni * 4, e->st));   // no valid replicate: every id -1
    }
    HIPCHK(hipStreamSynchronize(e->st));   // rep, flag go out of scope
    a.split_K = K;
    a.split_slots = slots;
    a.split_valid = true;
    return RC_OK;
}

extern "C" {

int rc_split_census(rc_engine *e, uint64_t *splits, uint32_t *count, int32_t *ids, uint64_t cap, uint64_t *n_distinct,
                    uint32_t *n_valid)
{
    if (!e || !n_distinct) return fail(RC_E_ARG, "null argument");
    rc_engine::Analysis &a = e->an;
    if (!a.nj_n) return fail(RC_E_STATE, "no trees on this engine yet (rc_nj, rc_resample_trees)");
    CHK(set_device(e));
    HIPCHK(hipEventRecord(e->ev[EV_SPLIT0], e->st));
    CHK(build_splits(e));
    const uint64_t K = a.split_K, ni = (uint64_t)a.nj_rep * (uint64_t)(a.nj_n - 3);
    const int W = (a.nj_n + 63) / 64;
    *n_distinct = K;
    if (n_valid) *n_valid = a.nj_nvalid;
    if ((splits == nullptr) != (count == nullptr)) return fail(RC_E_ARG, "splits and count go together");
    if (splits && cap < K) return fail(RC_E_CAPACITY, "buffer too small");
    if (splits && K) {
        CHK(a.d_sp_out.ensure(K * W));
        launch_split_gather(a.d_nj_splits.p, a.d_sp_first.p, K, W, a.d_sp_out.p, e->st);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(e->ev[EV_SPLIT1], e->st));
    if (splits && K) {
        HIPCHK(hipMemcpyAsync(splits, a.d_sp_out.p, K * W * 8, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(count, a.d_sp_count.p, K * 4, hipMemcpyDeviceToHost, e->st));
    }
    if (ids && ni) HIPCHK(hipMemcpyAsync(ids, a.d_sp_ids.p, ni * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    e->tm.split_ms = ev_ms(e, EV_SPLIT0, EV_SPLIT1);
    return RC_OK;
}

int rc_tree_rf(rc_engine *e, const uint64_t *ref_splits, int32_t n_ref, uint32_t *to_ref, uint32_t *pairwise)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    rc_engine::Analysis &a = e->an;
    if (!a.nj_n) return fail(RC_E_STATE, "no trees on this engine yet (rc_nj, rc_resample_trees)");
    if (to_ref && !ref_splits) return fail(RC_E_ARG, "to_ref needs ref_splits");
    CHK(nj_check(a.nj_rep, a.nj_n, ref_splits, n_ref, nullptr));
    if (pairwise && a.nj_rep > RF_MAX_PAIRWISE)
        return fail(RC_E_LIMIT, "a pairwise distance matrix of more than 8192 replicates");
    CHK(set_device(e));
    HIPCHK(hipEventRecord(e->ev[EV_SPLIT0], e->st));
    CHK(build_splits(e));
    const uint32_t R = (uint32_t)a.nj_rep, ns = (uint32_t)(a.nj_n - 3);
    const int W = (a.nj_n + 63) / 64;
    if (to_ref) {
        CHK(a.d_nj_ref.ensure((size_t)n_ref * W));
        CHK(a.d_sp_isref.ensure(a.split_K));
        CHK(a.d_rf_ref.ensure(R));
        if (a.split_K) HIPCHK(hipMemsetAsync(a.d_sp_isref.p, 0, a.split_K, e->st));
        if (n_ref && a.split_K) {
            HIPCHK(hipMemcpyAsync(a.d_nj_ref.p, ref_splits, (size_t)n_ref * W * 8, hipMemcpyHostToDevice, e->st));
            launch_split_ref(a.d_nj_ref.p, n_ref, a.d_nj_splits.p, W, a.d_sp_table.p, a.split_slots, a.d_sp_rank.p,
                             a.d_sp_isref.p, e->st);
        }
        launch_rf_ref(a.d_sp_ids.p, a.d_nj_valid.p, a.d_sp_isref.p, R, ns, (uint32_t)n_ref, a.d_rf_ref.p, e->st);
        HIPCHK(hipGetLastError());
    }
    if (pairwise) {
        CHK(a.d_rf_pair.ensure((size_t)R * R));
        launch_rf_pairs(a.d_sp_ids.p, a.d_nj_valid.p, R, ns, a.d_rf_pair.p, e->st);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(e->ev[EV_SPLIT1], e->st));
    if (to_ref) HIPCHK(hipMemcpyAsync(to_ref, a.d_rf_ref.p, (size_t)R * 4, hipMemcpyDeviceToHost, e->st));
    if (pairwise) HIPCHK(hipMemcpyAsync(pairwise, a.d_rf_pair.p, (size_t)R * R * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    e->tm.split_ms = ev_ms(e, EV_SPLIT0, EV_SPLIT1);
    return RC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------
// principal coordinates (pcoa.hip)
// ------------------------------------------------------------------------

static const int PCOA_MAX_SAMPLES = 128;
static const int PCOA_SWEEPS = 30;   // max_sweeps == 0

// the argument checks of rc_pcoa / rc_resample_pcoa (no device work)
static int pcoa_check(int32_t n_rep, int32_t n, int32_t k, int32_t max_sweeps)
{
    if (n > PCOA_MAX_SAMPLES) return fail(RC_E_LIMIT, "more than 128 samples in a principal coordinates analysis");
    if (n < 2) return fail(RC_E_ARG, "principal coordinates need at least 2 samples");
    if (n_rep < 1) return fail(RC_E_ARG, "n_rep must be >= 1");
    if (k < 1 || k > n) return fail(RC_E_ARG, "k must lie in 1..n");
    if (max_sweeps < 0) return fail(RC_E_ARG, "max_sweeps must be >= 0");
    return RC_OK;
}

// Eigenvalues and the first k eigenvectors of the n_rep matrices at dD
// (device, n x n each); the arguments have passed pcoa_check. Events EV_PCOA0,
// EV_PCOA1. stat[0]: matrices with a non-finite entry or norm, stat[1]: matrices
// that still rotated in their last allowed sweep.
static int pcoa_device(rc_engine *e, const double *dD, int32_t n_rep, int32_t n, int32_t k, int32_t max_sweeps,
                       double *values, double *vectors, int32_t *sweeps, uint8_t *valid, unsigned int stat[2])
{
    const size_t R = (size_t)n_rep, nv = R * (size_t)n, nx = nv * (size_t)k;
    if (!max_sweeps) max_sweeps = PCOA_SWEEPS;
    int lds_max = 0;
    HIPCHK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, e->o.device));
    if (pcoa_lds_bytes(n) + 4096 > (size_t)lds_max)
        return fail(RC_E_LIMIT, "this device's LDS does not hold a matrix of " + std::to_string(n) + " samples");
    CHK(e->an.d_pcoa_val.ensure(nv));
    CHK(e->an.d_pcoa_vec.ensure(nx));
    CHK(e->an.d_pcoa_sweeps.ensure(R));
    CHK(e->an.d_pcoa_valid.ensure(R));
    CHK(e->an.d_pcoa_stat.ensure(2));
    HIPCHK(hipMemsetAsync(e->an.d_pcoa_stat.p, 0, 2 * sizeof(unsigned int), e->st));
    HIPCHK(hipEventRecord(e->ev[EV_PCOA0], e->st));
    const hipError_t err = launch_pcoa(dD, n_rep, n, k, max_sweeps, e->an.d_pcoa_val.p, e->an.d_pcoa_vec.p,
                                       e->an.d_pcoa_sweeps.p, e->an.d_pcoa_valid.p, e->an.d_pcoa_stat.p, e->st);
    if (err != hipSuccess)
        return fail(RC_E_HIP, std::string("pcoa_kernel (") + std::to_string(pcoa_lds_bytes(n)) +
                                  " bytes of LDS): " + hipGetErrorString(err));
    HIPCHK(hipEventRecord(e->ev[EV_PCOA1], e->st));
    if (values) HIPCHK(hipMemcpyAsync(values, e->an.d_pcoa_val.p, nv * 8, hipMemcpyDeviceToHost, e->st));
    if (vectors) HIPCHK(hipMemcpyAsync(vectors, e->an.d_pcoa_vec.p, nx * 8, hipMemcpyDeviceToHost, e->st));
    if (sweeps) HIPCHK(hipMemcpyAsync(sweeps, e->an.d_pcoa_sweeps.p, R * 4, hipMemcpyDeviceToHost, e->st));
    if (valid) HIPCHK(hipMemcpyAsync(valid, e->an.d_pcoa_valid.p, R, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(stat, e->an.d_pcoa_stat.p, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    e->tm.pcoa_ms = ev_ms(e, EV_PCOA0, EV_PCOA1);
    return RC_OK;
}

static int pcoa_unconverged() { return fail(RC_E_LIMIT, "a matrix still rotated in its last allowed Jacobi sweep"); }

extern "C" {

int rc_pcoa(rc_engine *e, const double *D, int32_t n_rep, int32_t n, int32_t k, int32_t max_sweeps, double *values,
            double *vectors, int32_t *sweeps, uint8_t *valid)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    CHK(pcoa_check(n_rep, n, k, max_sweeps));
    if (!D) return fail(RC_E_ARG, "null argument");
    CHK(set_device(e));
    const size_t nd = (size_t)n_rep * n * n;
    CHK(e->an.d_pcoa_in.ensure(nd));
    HIPCHK(hipMemcpyAsync(e->an.d_pcoa_in.p, D, nd * 8, hipMemcpyHostToDevice, e->st));
    unsigned int stat[2] = {};
    CHK(pcoa_device(e, e->an.d_pcoa_in.p, n_rep, n, k, max_sweeps, values, vectors, sweeps, valid, stat));
    if (stat[0]) return fail(RC_E_NO_IDEAL, "a distance matrix has a non-finite entry: no ordination for it");
    if (stat[1]) return pcoa_unconverged();
    return RC_OK;
}

int rc_resample_pcoa(rc_engine *e, const uint16_t *weights, int32_t n_rep, uint64_t n_comp, const int32_t *order,
                     int32_t n, int32_t k, int32_t max_sweeps, double *values, double *vectors, int32_t *sweeps,
                     uint8_t *valid)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    CHK(pcoa_check(n_rep, n, k, max_sweeps));
    CHK(resample_fill(e, weights, n_rep, n_comp, order, n, true, true));
    unsigned int stat[2] = {};
    CHK(pcoa_device(e, e->d_dist.p, n_rep, n, k, max_sweeps, values, vectors, sweeps, valid, stat));
    e->tm.resample_ms = ev_ms(e, EV_RESAMPLE0, EV_RESAMPLE1);
    if (stat[0]) return fail(RC_E_NO_IDEAL, "No ideal components found. Cannot report distances!");
    if (stat[1]) return pcoa_unconverged();
    return RC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------
// group tests (groups.hip)
// ------------------------------------------------------------------------

static const int GROUP_MAX_SAMPLES = 128;

// The argument checks of rc_group_test / rc_resample_group_test and of
// rc_group_dispersion / rc_resample_group_dispersion (no device work; chunk:
// the permutations one workgroup of the test's kernel walks). lab8: the observed labels, then the n_perm permuted rows, one byte
// each; *m_within: the within-group pairs.
static int group_check(int32_t n_rep, int32_t n, const int32_t *labels, int32_t a, const int32_t *perm, int32_t n_perm,
                       int32_t method, std::vector<uint8_t> &lab8, uint32_t *m_within,
                       uint64_t chunk = GROUP_PERM_CHUNK)
{
    if (n > GROUP_MAX_SAMPLES) return fail(RC_E_LIMIT, "more than 128 samples in a group test");
    if (!labels || (n_perm > 0 && !perm)) return fail(RC_E_ARG, "null argument");
    if (n_rep < 1) return fail(RC_E_ARG, "n_rep must be >= 1");
    if (n_perm < 0) return fail(RC_E_ARG, "n_perm must be >= 0");
    if (method != RC_GROUP_PERMANOVA && method != RC_GROUP_ANOSIM) return fail(RC_E_ARG, "unknown group test");
    if (a < 2 || a >= n) return fail(RC_E_ARG, "a group test needs 2 <= n_groups < n");
    if (((uint64_t)n_perm + chunk - 1) / chunk * (uint64_t)n_rep >> 31)
        return fail(RC_E_LIMIT, "n_rep x permutations beyond the group test's grid");
    std::vector<int32_t> size(a, 0), seen(a);
    lab8.resize(((size_t)n_perm + 1) * n);
    for (int i = 0; i < n; i++) {
        if (labels[i] < 0 || labels[i] >= a) return fail(RC_E_ARG, "a label outside 0..n_groups-1");
        size[labels[i]]++;
        lab8[i] = (uint8_t)labels[i];
    }
    uint32_t mw = 0;
    for (int g = 0; g < a; g++) {
        if (!size[g]) return fail(RC_E_ARG, "an empty group");
        mw += (uint32_t)size[g] * (uint32_t)(size[g] - 1) / 2;
    }
    for (int64_t p = 0; p < n_perm; p++) {
        const int32_t *row = perm + p * n;
        uint8_t *out = lab8.data() + (size_t)(p + 1) * n;
        std::fill(seen.begin(), seen.end(), 0);
        for (int i = 0; i < n; i++) {
            if (row[i] < 0 || row[i] >= a || ++seen[row[i]] > size[row[i]])
                return fail(RC_E_ARG, "a row of perm_labels is not a rearrangement of labels");
            out[i] = (uint8_t)row[i];
        }
    }
    *m_within = mw;
    return RC_OK;
}

// The test of the n_rep matrices at dD (device, n x n each); the arguments have
// passed group_check. Events EV_GROUP0, EV_GROUP1. *invalid: the number of
// matrices with a non-finite entry.
static int group_device(rc_engine *e, const double *dD, int32_t n_rep, int32_t n, int32_t a, uint32_t m_within,
                        const std::vector<uint8_t> &lab8, int32_t n_perm, int32_t method, double *stat, uint32_t *n_ge,
                        double *total, double *within, double *perm_stat, uint8_t *valid, uint32_t *invalid)
{
    rc_engine::Analysis &an = e->an;
    const size_t R = (size_t)n_rep, np = perm_stat ? R * (size_t)n_perm : 0;
    const bool anosim = method == RC_GROUP_ANOSIM;
    int lds_max = 0;
    HIPCHK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, e->o.device));
    if (std::max(group_lds_bytes(method, n), anosim ? group_rank_lds_bytes(n) : 0) + 4096 > (size_t)lds_max)
        return fail(RC_E_LIMIT, "this device's LDS does not hold a matrix of " + std::to_string(n) + " samples");
    CHK(an.d_gt_labels.ensure(lab8.size()));
    CHK(an.d_gt_stat.ensure(R));
    CHK(an.d_gt_total.ensure(R));
    CHK(an.d_gt_within.ensure(R));
    CHK(an.d_gt_nge.ensure(R));
    CHK(an.d_gt_valid.ensure(R));
    if (np) CHK(an.d_gt_perm.ensure(np));
    if (anosim) CHK(an.d_gt_rank.ensure(R * (size_t)n * n));
    HIPCHK(hipMemcpyAsync(an.d_gt_labels.p, lab8.data(), lab8.size(), hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemsetAsync(an.d_gt_nge.p, 0, R * 4, e->st));
    HIPCHK(hipEventRecord(e->ev[EV_GROUP0], e->st));
    if (anosim) {
        const hipError_t err = launch_group_rank(dD, n_rep, n, an.d_gt_rank.p, an.d_gt_valid.p, e->st);
        if (err != hipSuccess)
            return fail(RC_E_HIP, std::string("group_rank_kernel (") + std::to_string(group_rank_lds_bytes(n)) +
                                      " bytes of LDS): " + hipGetErrorString(err));
    }
    const hipError_t err =
        launch_group_test(method, anosim ? (const void *)an.d_gt_rank.p : (const void *)dD, an.d_gt_valid.p, n_rep, n, a,
                          m_within, an.d_gt_labels.p, an.d_gt_labels.p + n, n_perm, an.d_gt_stat.p, an.d_gt_nge.p,
                          an.d_gt_total.p, an.d_gt_within.p, np ? an.d_gt_perm.p : nullptr, an.d_gt_valid.p, e->st);
    if (err != hipSuccess)
        return fail(RC_E_HIP, std::string("group_kernel (") + std::to_string(group_lds_bytes(method, n)) +
                                  " bytes of LDS): " + hipGetErrorString(err));
    HIPCHK(hipEventRecord(e->ev[EV_GROUP1], e->st));
    std::vector<uint8_t> hv(R);
    if (stat) HIPCHK(hipMemcpyAsync(stat, an.d_gt_stat.p, R * 8, hipMemcpyDeviceToHost, e->st));
    if (n_ge) HIPCHK(hipMemcpyAsync(n_ge, an.d_gt_nge.p, R * 4, hipMemcpyDeviceToHost, e->st));
    if (total) HIPCHK(hipMemcpyAsync(total, an.d_gt_total.p, R * 8, hipMemcpyDeviceToHost, e->st));
    if (within) HIPCHK(hipMemcpyAsync(within, an.d_gt_within.p, R * 8, hipMemcpyDeviceToHost, e->st));
    if (np) HIPCHK(hipMemcpyAsync(perm_stat, an.d_gt_perm.p, np * 8, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(hv.data(), an.d_gt_valid.p, R, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    e->tm.group_ms = ev_ms(e, EV_GROUP0, EV_GROUP1);
    uint32_t bad = 0;
    for (size_t r = 0; r < R; r++) bad += !hv[r];
    if (valid) std::copy(hv.begin(), hv.end(), valid);
    *invalid = bad;
    return RC_OK;
}

extern "C" {

int rc_group_test(rc_engine *e, const double *D, int32_t n_rep, int32_t n, const int32_t *labels, int32_t n_groups,
                  const int32_t *perm_labels, int32_t n_perm, int32_t method, double *stat, uint32_t *n_ge,
                  double *total, double *within, double *perm_stat, uint8_t *valid)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    std::vector<uint8_t> lab8;
    uint32_t mw = 0, invalid = 0;
    CHK(group_check(n_rep, n, labels, n_groups, perm_labels, n_perm, method, lab8, &mw));
    if (!D) return fail(RC_E_ARG, "null argument");
    CHK(set_device(e));
    const size_t nd = (size_t)n_rep * n * n;
    CHK(e->an.d_gt_in.ensure(nd));
    HIPCHK(hipMemcpyAsync(e->an.d_gt_in.p, D, nd * 8, hipMemcpyHostToDevice, e->st));
    CHK(group_device(e, e->an.d_gt_in.p, n_rep, n, n_groups, mw, lab8, n_perm, method, stat, n_ge, total, within,
                     perm_stat, valid, &invalid));
    if (invalid) return fail(RC_E_NO_IDEAL, "a distance matrix has a non-finite entry: no group test for it");
    return RC_OK;
}

int rc_resample_group_test(rc_engine *e, const uint16_t *weights, int32_t n_rep, uint64_t n_comp, const int32_t *order,
                           int32_t n, const int32_t *labels, int32_t n_groups, const int32_t *perm_labels,
                           int32_t n_perm, int32_t method, double *stat, uint32_t *n_ge, double *total, double *within,
                           double *perm_stat, uint8_t *valid)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    std::vector<uint8_t> lab8;
    uint32_t mw = 0, invalid = 0;
    CHK(group_check(n_rep, n, labels, n_groups, perm_labels, n_perm, method, lab8, &mw));
    CHK(resample_fill(e, weights, n_rep, n_comp, order, n, true, true));
    CHK(group_device(e, e->d_dist.p, n_rep, n, n_groups, mw, lab8, n_perm, method, stat, n_ge, total, within, perm_stat,
                     valid, &invalid));
    e->tm.resample_ms = ev_ms(e, EV_RESAMPLE0, EV_RESAMPLE1);
    if (invalid) return fail(RC_E_NO_IDEAL, "No ideal components found. Cannot report distances!");
    return RC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------
// PERMDISP (dispersion.hip)
// ------------------------------------------------------------------------

// PERMDISP of the n_rep matrices at dD (device, n x n each); the arguments have
// passed group_check. Events EV_DISP0, EV_DISP1. *invalid: the number of
// matrices with a non-finite entry.
static int dispersion_device(rc_engine *e, const double *dD, int32_t n_rep, int32_t n, int32_t a,
                             const std::vector<uint8_t> &lab8, int32_t n_perm, double *stat, uint32_t *n_ge,
                             double *total, double *within, double *perm_stat, double *dist, uint8_t *valid,
                             uint32_t *invalid)
{
    rc_engine::Analysis &an = e->an;
    const size_t R = (size_t)n_rep, np = perm_stat ? R * (size_t)n_perm : 0, nz = R * (size_t)n;
    int lds_max = 0;
    HIPCHK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, e->o.device));
    if (dispersion_lds_bytes(n) + 4096 > (size_t)lds_max)
        return fail(RC_E_LIMIT, "this device's LDS does not hold a matrix of " + std::to_string(n) + " samples");
    CHK(an.d_gt_labels.ensure(lab8.size()));
    CHK(an.d_gt_stat.ensure(R));
    CHK(an.d_gt_total.ensure(R));
    CHK(an.d_gt_within.ensure(R));
    CHK(an.d_gt_nge.ensure(R));
    CHK(an.d_gt_valid.ensure(R));
    CHK(an.d_gt_dist.ensure(nz));
    if (np) CHK(an.d_gt_perm.ensure(np));
    HIPCHK(hipMemcpyAsync(an.d_gt_labels.p, lab8.data(), lab8.size(), hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemsetAsync(an.d_gt_nge.p, 0, R * 4, e->st));
    HIPCHK(hipEventRecord(e->ev[EV_DISP0], e->st));
    const hipError_t err =
        launch_dispersion(dD, n_rep, n, a, an.d_gt_labels.p, an.d_gt_labels.p + n, n_perm, an.d_gt_stat.p, an.d_gt_nge.p,
                          an.d_gt_total.p, an.d_gt_within.p, np ? an.d_gt_perm.p : nullptr, an.d_gt_dist.p,
                          an.d_gt_valid.p, e->st);
    if (err != hipSuccess)
        return fail(RC_E_HIP, std::string("dispersion_kernel (") + std::to_string(dispersion_lds_bytes(n)) +
                                  " bytes of LDS): " + hipGetErrorString(err));
    HIPCHK(hipEventRecord(e->ev[EV_DISP1], e->st));
    std::vector<uint8_t> hv(R);
    if (stat) HIPCHK(hipMemcpyAsync(stat, an.d_gt_stat.p, R * 8, hipMemcpyDeviceToHost, e->st));
    if (n_ge) HIPCHK(hipMemcpyAsync(n_ge, an.d_gt_nge.p, R * 4, hipMemcpyDeviceToHost, e->st));
    if (total) HIPCHK(hipMemcpyAsync(total, an.d_gt_total.p, R * 8, hipMemcpyDeviceToHost, e->st));
    if (within) HIPCHK(hipMemcpyAsync(within, an.d_gt_within.p, R * 8, hipMemcpyDeviceToHost, e->st));
    if (np) HIPCHK(hipMemcpyAsync(perm_stat, an.d_gt_perm.p, np * 8, hipMemcpyDeviceToHost, e->st));
    if (dist) HIPCHK(hipMemcpyAsync(dist, an.d_gt_dist.p, nz * 8, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(hv.data(), an.d_gt_valid.p, R, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    e->tm.disp_ms = ev_ms(e, EV_DISP0, EV_DISP1);
    uint32_t bad = 0;
    for (size_t r = 0; r < R; r++) bad += !hv[r];
    if (valid) std::copy(hv.begin(), hv.end(), valid);
    *invalid = bad;
    return RC_OK;
}

extern "C" {

int rc_group_dispersion(rc_engine *e, const double *D, int32_t n_rep, int32_t n, const int32_t *labels,
                        int32_t n_groups, const int32_t *perm_labels, int32_t n_perm, double *stat, uint32_t *n_ge,
                        double *total, double *within, double *perm_stat, double *dist, uint8_t *valid)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    std::vector<uint8_t> lab8;
    uint32_t mw = 0, invalid = 0;
    CHK(group_check(n_rep, n, labels, n_groups, perm_labels, n_perm, RC_GROUP_PERMANOVA, lab8, &mw, DISP_PERM_CHUNK));
    if (!D) return fail(RC_E_ARG, "null argument");
    CHK(set_device(e));
    const size_t nd = (size_t)n_rep * n * n;
    CHK(e->an.d_gt_in.ensure(nd));
    HIPCHK(hipMemcpyAsync(e->an.d_gt_in.p, D, nd * 8, hipMemcpyHostToDevice, e->st));
    CHK(dispersion_device(e, e->an.d_gt_in.p, n_rep, n, n_groups, lab8, n_perm, stat, n_ge, total, within, perm_stat,
                          dist, valid, &invalid));
    if (invalid) return fail(RC_E_NO_IDEAL, "a distance matrix has a non-finite entry: no dispersion test for it");
    return RC_OK;
}

int rc_resample_group_dispersion(rc_engine *e, const uint16_t *weights, int32_t n_rep, uint64_t n_comp,
                                 const int32_t *order, int32_t n, const int32_t *labels, int32_t n_groups,
                                 const int32_t *perm_labels, int32_t n_perm, double *stat, uint32_t *n_ge,
                                 double *total, double *within, double *perm_stat, double *dist, uint8_t *valid)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    std::vector<uint8_t> lab8;
    uint32_t mw = 0, invalid = 0;
    CHK(group_check(n_rep, n, labels, n_groups, perm_labels, n_perm, RC_GROUP_PERMANOVA, lab8, &mw, DISP_PERM_CHUNK));
    CHK(resample_fill(e, weights, n_rep, n_comp, order, n, true, true));
    CHK(dispersion_device(e, e->d_dist.p, n_rep, n, n_groups, lab8, n_perm, stat, n_ge, total, within, perm_stat, dist,
                          valid, &invalid));
    e->tm.resample_ms = ev_ms(e, EV_RESAMPLE0, EV_RESAMPLE1);
    if (invalid) return fail(RC_E_NO_IDEAL, "No ideal components found. Cannot report distances!");
    return RC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------
// the Mantel test (mantel.hip)
// ------------------------------------------------------------------------

static const int MANTEL_MAX_SAMPLES = 128;

// The argument checks of rc_mantel / rc_resample_mantel (no device work).
// perm8: the permutations, one byte per position.
static int mantel_check(int32_t n_rep, int32_t n, const double *Y, const int32_t *perms, int32_t n_perm, int32_t method,
                        std::vector<uint8_t> &perm8)
{
    if (n > MANTEL_MAX_SAMPLES) return fail(RC_E_LIMIT, "more than 128 samples in a Mantel test");
    if (!Y || (n_perm > 0 && !perms)) return fail(RC_E_ARG, "null argument");
    if (n < 3) return fail(RC_E_ARG, "a Mantel test needs at least 3 samples");
    if (n_rep < 1) return fail(RC_E_ARG, "n_rep must be >= 1");
    if (n_perm < 0) return fail(RC_E_ARG, "n_perm must be >= 0");
    if (method != RC_MANTEL_PEARSON && method != RC_MANTEL_SPEARMAN) return fail(RC_E_ARG, "unknown Mantel method");
    if (((uint64_t)n_perm + MANTEL_PERM_CHUNK - 1) / MANTEL_PERM_CHUNK * (uint64_t)n_rep >> 31)
        return fail(RC_E_LIMIT, "n_rep x permutations beyond the Mantel test's grid");
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++)
            if (!std::isfinite(Y[(size_t)i * n + j])) return fail(RC_E_ARG, "a non-finite entry above Y's diagonal");
    perm8.resize((size_t)n_perm * n);
    std::vector<uint8_t> seen(n);
    for (int64_t p = 0; p < n_perm; p++) {
        const int32_t *row = perms + p * n;
        std::fill(seen.begin(), seen.end(), 0);
        for (int i = 0; i < n; i++) {
            if (row[i] < 0 || row[i] >= n || seen[row[i]]++)
                return fail(RC_E_ARG, "a row of perms is not a rearrangement of 0..n-1");
            perm8[(size_t)p * n + i] = (uint8_t)row[i];
        }
    }
    return RC_OK;
}

// The Mantel test of the n_rep matrices at dD (device, n x n each) against Y
// (host, n x n); the arguments have passed mantel_check. Events EV_MANTEL0,
// EV_MANTEL1. *invalid: the number of matrices with a non-finite entry.
static int mantel_device(rc_engine *e, const double *dD, int32_t n_rep, int32_t n, const double *Y,
                         const std::vector<uint8_t> &perm8, int32_t n_perm, int32_t method, double *stat, uint32_t *n_ge,
                         uint32_t *n_le, uint32_t *n_abs_ge, double *perm_stat, uint8_t *valid, uint32_t *invalid)
{
    rc_engine::Analysis &an = e->an;
    const size_t R = (size_t)n_rep, np = perm_stat ? R * (size_t)n_perm : 0, nn = (size_t)n * n;
    const bool spearman = method == RC_MANTEL_SPEARMAN;
    int lds_max = 0;
    HIPCHK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, e->o.device));
    if (std::max(mantel_lds_bytes(method, n), spearman ? group_rank_lds_bytes(n) : 0) + 4096 > (size_t)lds_max)
        return fail(RC_E_LIMIT, "this device's LDS does not hold a matrix of " + std::to_string(n) + " samples");
    CHK(an.d_mt_perms.ensure(perm8.size() + 1));
    CHK(an.d_mt_y.ensure(nn));
    CHK(an.d_mt_stat.ensure(R));
    CHK(an.d_mt_counts.ensure(3 * R));
    CHK(an.d_mt_valid.ensure(R));
    if (np) CHK(an.d_mt_perm.ensure(np));
    if (spearman) {
        CHK(an.d_mt_rank.ensure(R * nn));
        CHK(an.d_mt_yrank.ensure(nn));
        CHK(an.d_mt_yvalid.ensure(1));
    }
    std::vector<double> yc(nn);
    double syy = 0.0;
    int y_const = 0;
    if (spearman)
        std::copy(Y, Y + nn, yc.begin());
    else
        mantel_prepare_y(Y, n, yc.data(), &syy, &y_const);
    HIPCHK(hipMemcpyAsync(an.d_mt_y.p, yc.data(), nn * 8, hipMemcpyHostToDevice, e->st));
    if (!perm8.empty())
        HIPCHK(hipMemcpyAsync(an.d_mt_perms.p, perm8.data(), perm8.size(), hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemsetAsync(an.d_mt_counts.p, 0, 3 * R * 4, e->st));
    HIPCHK(hipEventRecord(e->ev[EV_MANTEL0], e->st));
    if (spearman) {
        hipError_t err = launch_group_rank(dD, n_rep, n, an.d_mt_rank.p, an.d_mt_valid.p, e->st);
        if (err == hipSuccess) err = launch_group_rank(an.d_mt_y.p, 1, n, an.d_mt_yrank.p, an.d_mt_yvalid.p, e->st);
        if (err != hipSuccess)
            return fail(RC_E_HIP, std::string("group_rank_kernel (") + std::to_string(group_rank_lds_bytes(n)) +
                                      " bytes of LDS): " + hipGetErrorString(err));
    }
    const hipError_t err = launch_mantel(
        method, spearman ? (const void *)an.d_mt_rank.p : (const void *)dD, an.d_mt_valid.p, n_rep, n,
        spearman ? (const void *)an.d_mt_yrank.p : (const void *)an.d_mt_y.p, syy, y_const, an.d_mt_perms.p, n_perm,
        an.d_mt_stat.p, an.d_mt_counts.p, an.d_mt_counts.p + R, an.d_mt_counts.p + 2 * R,
        np ? an.d_mt_perm.p : nullptr, an.d_mt_valid.p, e->st);
    if (err != hipSuccess)
        return fail(RC_E_HIP, std::string("mantel_kernel (") + std::to_string(mantel_lds_bytes(method, n)) +
                                  " bytes of LDS): " + hipGetErrorString(err));
    HIPCHK(hipEventRecord(e->ev[EV_MANTEL1], e->st));
    std::vector<uint8_t> hv(R);
    if (stat) HIPCHK(hipMemcpyAsync(stat, an.d_mt_stat.p, R * 8, hipMemcpyDeviceToHost, e->st));
    if (n_ge) HIPCHK(hipMemcpyAsync(n_ge, an.d_mt_counts.p, R * 4, hipMemcpyDeviceToHost, e->st));
    if (n_le) HIPCHK(hipMemcpyAsync(n_le, an.d_mt_counts.p + R, R * 4, hipMemcpyDeviceToHost, e->st));
    if (n_abs_ge) HIPCHK(hipMemcpyAsync(n_abs_ge, an.d_mt_counts.p + 2 * R, R * 4, hipMemcpyDeviceToHost, e->st));
    if (np) HIPCHK(hipMemcpyAsync(perm_stat, an.d_mt_perm.p, np * 8, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(hv.data(), an.d_mt_valid.p, R, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    e->tm.mantel_ms = ev_ms(e, EV_MANTEL0, EV_MANTEL1);
    uint32_t bad = 0;
    for (size_t r = 0; r < R; r++) bad += !hv[r];
    if (valid) std::copy(hv.begin(), hv.end(), valid);
    *invalid = bad;
    return RC_OK;
}

extern "C" {

int rc_mantel(rc_engine *e, const double *X, int32_t n_rep, int32_t n, const double *Y, const int32_t *perms,
              int32_t n_perm, int32_t method, double *stat, uint32_t *n_ge, uint32_t *n_le, uint32_t *n_abs_ge,
              double *perm_stat, uint8_t *valid)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    std::vector<uint8_t> perm8;
    uint32_t invalid = 0;
    CHK(mantel_check(n_rep, n, Y, perms, n_perm, method, perm8));
    if (!X) return fail(RC_E_ARG, "null argument");
    CHK(set_device(e));
    const size_t nd = (size_t)n_rep * n * n;
    CHK(e->an.d_mt_in.ensure(nd));
    HIPCHK(hipMemcpyAsync(e->an.d_mt_in.p, X, nd * 8, hipMemcpyHostToDevice, e->st));
    CHK(mantel_device(e, e->an.d_mt_in.p, n_rep, n, Y, perm8, n_perm, method, stat, n_ge, n_le, n_abs_ge, perm_stat,
                      valid, &invalid));
    if (invalid) return fail(RC_E_NO_IDEAL, "a distance matrix has a non-finite entry: no Mantel test for it");
    return RC_OK;
}

int rc_resample_mantel(rc_engine *e, const uint16_t *weights, int32_t n_rep, uint64_t n_comp, const int32_t *order,
                       int32_t n, const double *Y, const int32_t *perms, int32_t n_perm, int32_t method, double *stat,
                       uint32_t *n_ge, uint32_t *n_le, uint32_t *n_abs_ge, double *perm_stat, uint8_t *valid)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    std::vector<uint8_t> perm8;
    uint32_t invalid = 0;
    CHK(mantel_check(n_rep, n, Y, perms, n_perm, method, perm8));
    CHK(resample_fill(e, weights, n_rep, n_comp, order, n, true, true));
    CHK(mantel_device(e, e->d_dist.p, n_rep, n, Y, perm8, n_perm, method, stat, n_ge, n_le, n_abs_ge, perm_stat, valid,
                      &invalid));
    e->tm.resample_ms = ev_ms(e, EV_RESAMPLE0, EV_RESAMPLE1);
    if (invalid) return fail(RC_E_NO_IDEAL, "No ideal components found. Cannot report distances!");
    return RC_OK;
}

}  // extern "C"
