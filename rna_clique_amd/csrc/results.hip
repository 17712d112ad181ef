// What a caller reads out of a finished engine: HSPs, gene matches table rows,
// graph statistics and edges, pair sums and distances, graph.pkl and the
// table files. Nothing here calls back into the pipeline (engine.hip).
#include "engine.h"

// od2_tables.cpp: one pair's gene matches table file
int od2_write_table(const rc_row *rows, uint64_t n, const std::string &ssample, const std::string &qsample,
                    const std::string &path);
// graph_pickle.cpp: a table of the pickle whose gene arrays the caller fills
extern "C" int graph_pickle_table(rc_gpickle *g, int32_t ssample, int32_t qsample, uint64_t n, int64_t **sgene,
                                  int64_t **qgene);

static rc_hsp to_rc_hsp(const rc_engine *e, const DHsp &d, int qs_, int ss_)
{
    rc_hsp h;
    h.q_tx = d.q_tx - e->samples[qs_].tx_begin;
    h.s_tx = d.s_tx - e->samples[ss_].tx_begin;
    h.qstart = d.qstart; h.qend = d.qend; h.sstart = d.sstart; h.send = d.send;
    h.length = d.length; h.nident = d.nident; h.mismatch = d.mismatch; h.gaps = d.gaps;
    h.gapopen = d.gapopen; h.score_half = d.score_half; h.bits10 = d.bits10; h.strand = d.strand & 1;
    const int64_t qlen = (int64_t)(e->tx_start[d.q_tx + 1] - e->tx_start[d.q_tx]);
    const double ss = qlen <= e->max_len ? e->h_ss[(size_t)ss_ * (e->max_len + 1) + (size_t)qlen]
                                         : stats::search_space(qlen, e->db_len[ss_], e->db_n[ss_]);
    // stats::evalue, its exp() taken from the table (the same product, in
    // the same order: bit-identical)
    h.evalue = d.score_half >= 0 && (size_t)d.score_half < e->h_exp.size() ? ss * stats::K * e->h_exp[d.score_half]
                                                                            : stats::evalue(ss, d.score_half);
    return h;
}

static int copy_groups(rc_engine *e, std::vector<uint32_t> &off, std::vector<uint32_t> &cnt)
{
    const size_t n = (size_t)e->gene_sample.size() * e->samples.size();
    off.resize(n);
    cnt.resize(n);
    if (!n) return RC_OK;
    HIPCHK(hipMemcpy(off.data(), e->d_grp_off.p, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cnt.data(), e->d_grp_cnt.p, n * 4, hipMemcpyDeviceToHost));
    return RC_OK;
}

extern "C" {

int rc_hsps(rc_engine *e, int32_t q, int32_t s, rc_hsp *buf, uint64_t cap, uint64_t *n)
{
    if (!e || !n) return fail(RC_E_ARG, "null argument");
    if (!e->aligned) return fail(RC_E_STATE, "no alignment yet");
    const int N = (int)e->samples.size();
    if (q < 0 || q >= N || s < 0 || s >= N) return fail(RC_E_ARG, "bad sample");
    CHK(set_device(e));
    std::vector<uint32_t> off, cnt;
    CHK(copy_groups(e, off, cnt));
    const SampleRec &Q = e->samples[q];
    const uint32_t ng = (uint32_t)e->gene_sample.size();
    uint64_t tot = 0;
    for (uint32_t g = Q.gene_begin; g < Q.gene_begin + Q.n_genes; g++) tot += cnt[grp_index(g, s, ng)];
    *n = tot;
    if (!buf) return RC_OK;
    if (cap < tot) return fail(RC_E_CAPACITY, "buffer too small");
    uint64_t w = 0;
    std::vector<DHsp> tmp;
    for (uint32_t g = Q.gene_begin; g < Q.gene_begin + Q.n_genes; g++) {
        const uint32_t c = cnt[grp_index(g, s, ng)];
        if (!c) continue;
        tmp.resize(c);
        HIPCHK(hipMemcpy(tmp.data(), e->d_hsp.p + off[grp_index(g, s, ng)], c * sizeof(DHsp), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < c; i++) buf[w++] = to_rc_hsp(e, tmp[i], q, s);
    }
    return RC_OK;
}

// A pair's rows on the host: its table rows (DRow) and their HSPs, fetched
// from the device (the engine's stream; one caller at a time).
struct PairRaw {
    int32_t s1 = 0, s2 = 0;
    uint64_t n = 0;
    const DRow *rows = nullptr;   // n rows and their HSPs: in the vectors, or in a pinned slab
    const DHsp *hs = nullptr;
    std::vector<DRow> vrows;
    std::vector<DHsp> vhs;
    std::shared_ptr<char> slab;   // (returned to its pool when the last holder lets go)
};

// Pinned host slabs the rows of many pairs come to by DMA (rc_write_outputs):
// at most `cap` of them, allocated as needed, each holding `bytes`; a slab
// goes back to the pool when its pair's last consumer drops it. Pageable
// copies faulted fresh pages for every pair (3.6 GB at C3).
struct SlabPool {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char *> all, free;
    size_t bytes = 0, cap = 0;
    ~SlabPool()
    {
        for (char *p : all) (void)hipHostFree(p);
    }
    // a slab (blocks while all `cap` are in use); nullptr if pinning fails
    std::shared_ptr<char> get()
    {
        std::unique_lock<std::mutex> lk(mu);
        if (free.empty() && all.size() < cap) {
            char *p = nullptr;
            if (hipHostMalloc((void **)&p, bytes, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                return nullptr;
            }
            all.push_back(p);
            free.push_back(p);
        }
        cv.wait(lk, [&] { return !free.empty(); });
        char *p = free.back();
        free.pop_back();
        return std::shared_ptr<char>(p, [this](char *q) {
            {
                std::lock_guard<std::mutex> g(mu);
                free.push_back(q);
            }
            cv.notify_all();
        });
    }
};

static int pair_row_range(rc_engine *e, int32_t s1, int32_t s2, uint64_t &r0, uint64_t &r1)
{
    if (!e->rbh_done || e->graph_only) return fail(RC_E_STATE, "no gene matches tables on this engine");
    const int N = (int)e->samples.size();
    if (s1 < 0 || s1 >= N || s2 < 0 || s2 >= N || s1 >= s2) return fail(RC_E_ARG, "need s1 < s2 (input order)");
    CHK(set_device(e));
    const uint64_t p = (uint64_t)e->pair_index[s1 * N + s2];
    if (p < e->pair0 || p >= e->pair1) return fail(RC_E_ARG, "pair belongs to another shard");
    const uint64_t ib = e->pair_item_begin[p] - e->item0, ie = e->pair_item_begin[p + 1] - e->item0;
    HIPCHK(hipMemcpy(&r0, e->d_off4.p + ib, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&r1, e->d_off4.p + ie, 8, hipMemcpyDeviceToHost));
    return RC_OK;
}

// a pair's rows and their HSPs to the host: into `pool`'s pinned slabs when
// given and big enough, else into the PairRaw's own vectors
static int fetch_pair(rc_engine *e, int32_t s1, int32_t s2, PairRaw &out, SlabPool *pool = nullptr,
                      const uint64_t *range = nullptr)
{
    uint64_t r0 = 0, r1 = 0;
    if (range) {
        r0 = range[0];
        r1 = range[1];
    } else {
        CHK(pair_row_range(e, s1, s2, r0, r1));
    }
    const uint64_t nr = r1 - r0;
    out.s1 = s1;
    out.s2 = s2;
    out.n = nr;
    if (!nr) return RC_OK;
    CHK(e->d_gather.ensure(nr));
    launch_gather_rows(e->d_hsp.p, e->d_rows.p + r0, nr, e->d_gather.p, e->st);
    HIPCHK(hipGetLastError());
    DRow *rows = nullptr;
    DHsp *hs = nullptr;
    if (pool && nr * (sizeof(DRow) + sizeof(DHsp)) <= pool->bytes) out.slab = pool->get();
    if (out.slab) {
        hs = reinterpret_cast<DHsp *>(out.slab.get());
        rows = reinterpret_cast<DRow *>(out.slab.get() + nr * sizeof(DHsp));
    } else {
        out.vrows.resize(nr);
        out.vhs.resize(nr);
        rows = out.vrows.data();
        hs = out.vhs.data();
    }
    HIPCHK(hipMemcpyAsync(rows, e->d_rows.p + r0, nr * sizeof(DRow), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(hs, e->d_gather.p, nr * sizeof(DHsp), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    out.rows = rows;
    out.hs = hs;
    return RC_OK;
}

// rc_row records of fetched rows (host only: thread-safe, the engine's host
// tables are read only)
static void convert_rows(const rc_engine *e, const PairRaw &raw, rc_row *buf)
{
    const int32_t s1 = raw.s1, s2 = raw.s2;
    const uint64_t nr = raw.n;
    const DRow *rows = raw.rows;
    const DHsp *hs = raw.hs;
    for (uint64_t i = 0; i < nr; i++) {
        const DHsp &d = hs[i];
        rc_row &r = buf[i];
        const bool rev = rows[i].reverse != 0;
        // forward rows: query in s2, subject in s1; reverse rows the other way round
        const int qs_ = rev ? s1 : s2, ss_ = rev ? s2 : s1;
        r.hsp = to_rc_hsp(e, d, qs_, ss_);
        const uint32_t tq = rev ? d.s_tx : d.q_tx;   // transcript of s2 (qgene side)
        const uint32_t ts = rev ? d.q_tx : d.s_tx;   // transcript of s1 (sgene side)
        r.qgene = e->tx_gene_id[tq];
        r.qiso = e->tx_iso[tq];
        r.sgene = e->tx_gene_id[ts];
        r.siso = e->tx_iso[ts];
        r.q_tx = tq - e->samples[s2].tx_begin;
        r.s_tx = ts - e->samples[s1].tx_begin;
        r.reverse = rev ? 1 : 0;
        r.label = rows[i].label;
    }
}

int rc_pair_rows(rc_engine *e, int32_t s1, int32_t s2, rc_row *buf, uint64_t cap, uint64_t *n)
{
    if (!e || !n) return fail(RC_E_ARG, "null argument");
    uint64_t r0 = 0, r1 = 0;
    CHK(pair_row_range(e, s1, s2, r0, r1));
    *n = r1 - r0;
    if (!buf) return RC_OK;
    if (cap < r1 - r0) return fail(RC_E_CAPACITY, "buffer too small");
    if (r1 == r0) return RC_OK;
    PairRaw raw;
    CHK(fetch_pair(e, s1, s2, raw));
    convert_rows(e, raw, buf);
    return RC_OK;
}

int rc_graph_stats(rc_engine *e, rc_stats *s)
{
    if (!e || !s) return fail(RC_E_ARG, "null argument");
    if (!e->finished) return fail(RC_E_STATE, "no results yet");
    s->components = (int64_t)e->h_stats[0];
    s->ideal_components = (int64_t)e->h_stats[1];
    s->ideal_nodes = (int64_t)e->h_stats[2];
    s->nodes = (int64_t)e->h_stats[3];
    s->sample_count = (int32_t)e->h_stats[4];
    s->pad = 0;
    s->edges = (int64_t)e->n_edges;
    s->hsps = (int64_t)e->n_hsps;
    s->seeds = (int64_t)e->n_seeds;
    s->candidates = (int64_t)e->n_cands;
    s->table_rows = (int64_t)e->n_rows;
    return RC_OK;
}

int rc_edges(rc_engine *e, rc_edge *buf, uint64_t cap, uint64_t *n)
{
    if (!e || !n) return fail(RC_E_ARG, "null argument");
    if (!e->finished) return fail(RC_E_STATE, "no results yet");
    *n = e->n_edges;
    if (!buf) return RC_OK;
    if (cap < e->n_edges) return fail(RC_E_CAPACITY, "buffer too small");
    CHK(set_device(e));
    std::vector<DEdge> ed(e->n_edges);
    if (!ed.empty()) HIPCHK(hipMemcpy(ed.data(), e->d_edges.p, ed.size() * sizeof(DEdge), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ed.size(); i++) {
        buf[i].sample_a = e->gene_sample[ed[i].a];
        buf[i].gene_a = e->gene_id[ed[i].a];
        buf[i].sample_b = e->gene_sample[ed[i].b];
        buf[i].gene_b = e->gene_id[ed[i].b];
    }
    return RC_OK;
}

int rc_ideal_nodes(rc_engine *e, int32_t *sample, int32_t *gene, uint64_t cap, uint64_t *n)
{
    if (!e || !n) return fail(RC_E_ARG, "null argument");
    if (!e->finished) return fail(RC_E_STATE, "no results yet");
    CHK(set_device(e));
    const uint32_t ng = (uint32_t)e->gene_sample.size();
    std::vector<uint32_t> parent(ng), present(ng);
    std::vector<uint8_t> ideal(ng);
    if (ng) {
        HIPCHK(hipMemcpy(parent.data(), e->d_parent.p, ng * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(present.data(), e->d_present.p, ng * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ideal.data(), e->d_ideal.p, ng, hipMemcpyDeviceToHost));
    }
    uint64_t c = 0;
    for (uint32_t v = 0; v < ng; v++)
        if (present[v] && ideal[parent[v]]) {
            if (sample && gene) {
                if (c >= cap) return fail(RC_E_CAPACITY, "buffer too small");
                sample[c] = e->gene_sample[v];
                gene[c] = e->gene_id[v];
            }
            c++;
        }
    *n = c;
    return RC_OK;
}

int rc_pair_sums(rc_engine *e, int64_t *num, int64_t *den)
{
    if (!e || !num || !den) return fail(RC_E_ARG, "null argument");
    if (!e->finished) return fail(RC_E_STATE, "no results yet");
    const int N = (int)e->samples.size();
    for (int a = 0; a < N; a++)
        for (int b = 0; b < N; b++) {
            if (a == b) {
                num[a * N + b] = den[a * N + b] = 0;
                continue;
            }
            const int p = e->pair_index[a * N + b];
            num[a * N + b] = (int64_t)e->h_num[p];
            den[a * N + b] = (int64_t)e->h_den[p];
        }
    return RC_OK;
}

// Unfiltered sums: every gene matches table row of the pair
// (UnfilteredSimilarity, unfiltered_distance.py:9-16 over similarities_from_dfs,
// similarity_computer.py:21-42).
int rc_pair_sums_unfiltered(rc_engine *e, int64_t *num, int64_t *den)
{
    if (!e || !num || !den) return fail(RC_E_ARG, "null argument");
    if (!e->finished) return fail(RC_E_STATE, "no results yet");
    const int N = (int)e->samples.size();
    for (int a = 0; a < N; a++)
        for (int b = 0; b < N; b++) {
            if (a == b) {
                num[a * N + b] = den[a * N + b] = 0;
                continue;
            }
            const int p = e->pair_index[a * N + b];
            num[a * N + b] = (int64_t)e->h_num_all[p];
            den[a * N + b] = (int64_t)e->h_den_all[p];
        }
    return RC_OK;
}

int rc_distance_subset(rc_engine *e, const int32_t *order, int32_t n, double *out)
{
    if (!e || (n && (!order || !out))) return fail(RC_E_ARG, "null argument");
    if (!e->finished) return fail(RC_E_STATE, "no results yet");
    const int N = (int)e->samples.size();
    if (n < 0 || n > N) return fail(RC_E_ARG, "bad sample count");
    std::vector<int> seen(N, 0);
    for (int i = 0; i < n; i++) {
        if (order[i] < 0 || order[i] >= N || seen[order[i]]) return fail(RC_E_ARG, "order must hold distinct sample ids");
        seen[order[i]] = 1;
    }
    if (!n) return RC_OK;
    CHK(set_device(e));
    CHK(e->d_order.ensure(n));
    CHK(e->d_dist.ensure((size_t)n * n));
    HIPCHK(hipMemcpyAsync(e->d_order.p, order, n * 4, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemsetAsync(e->d_status.p, 0, 4 * sizeof(unsigned int), e->st));
    launch_distance(e->d_num.p, e->d_den.p, e->d_pair_index.p, e->d_order.p, N, n, e->d_dist.p, e->d_status.p,
                    e->st);
    HIPCHK(hipGetLastError());
    unsigned int status = 0;
    HIPCHK(hipMemcpyAsync(out, e->d_dist.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(&status, e->d_status.p, 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    if (status & ST_NO_IDEAL) return fail(RC_E_NO_IDEAL, "No ideal components found. Cannot report distances!");
    return RC_OK;
}

int rc_distance(rc_engine *e, const int32_t *order, double *out)
{
    if (!e) return fail(RC_E_ARG, "null argument");
    return rc_distance_subset(e, order, (int32_t)e->samples.size(), out);
}

// graph.pkl from the engine's graph edges: build_graph over every pair's
// table in combinations order (find_all_pairs.py:224-228 as the one-process
// order; build_graph.py:40-68) needs, per pair, its distinct (s-gene, q-gene)
// edges in the order of their first table rows -- the order of the edge
// records of that pair. The records (all pairs: a single-shard run's own, a
// sharded run's after rc_import_edges) are stably sorted on the device by
// their pair's combinations rank and copied to the host; tbeg[k] is the first
// record of the k-th non-empty pair.
// graph.pkl's tables from the edge records: sorted on the device into every
// pair's table in combinations order (stable: record order inside a pair),
// then handed to the writer as node-slot pairs -- a record's genes are global
// gene indices, sample-major, so sample s's nodes are the slots
// [gene_base[s], gene_base[s + 1]) -- with the tables' row ranges. One
// record per edge (the RBH kernel aggregates an edge's rows into it), so the
// writer skips its edge deduplication.
static int edge_slots(rc_engine *e, GraphSlots &G)
{
    if (!e->finished) return fail(RC_E_STATE, "no results yet");
    CHK(set_device(e));
    const uint64_t n = e->n_edges;
    const int N = (int)e->samples.size();
    if (n > 0xFFFFFFFFull) return fail(RC_E_LIMIT, "more than 2^32 graph edges");
    const size_t ncomb = e->pair_a.size();
    std::vector<uint32_t> comb(ncomb);
    for (size_t p = 0; p < ncomb; p++) {
        const uint64_t a = (uint64_t)e->pair_a[p], b = (uint64_t)e->pair_b[p];
        comb[p] = (uint32_t)(a * (2 * (uint64_t)N - a - 1) / 2 + (b - a - 1));
    }
    G = GraphSlots();
    G.ns = N;
    G.base.assign((size_t)N + 1, 0);
    for (int32_t s : e->gene_sample) G.base[(size_t)s + 1]++;
    for (int s = 0; s < N; s++) G.base[s + 1] += G.base[s];
    G.slot_gene = e->gene_id.data();
    G.unique = true;
    G.rows = n;
    std::vector<uint64_t> first(ncomb, ~0ull);
    if (n) {
        DBuf<uint32_t> dcomb, k0, k1, v0, v1;
        DBuf<uint64_t> dfirst;
        CHK(dcomb.ensure(ncomb));
        CHK(dfirst.ensure(std::max<size_t>(ncomb, 1)));
        CHK(k0.ensure(n));
        CHK(k1.ensure(n));
        CHK(v0.ensure(n));
        CHK(v1.ensure(n));
        HIPCHK(hipMemcpyAsync(dcomb.p, comb.data(), ncomb * 4, hipMemcpyHostToDevice, e->st));
        HIPCHK(hipMemsetAsync(dfirst.p, 0xFF, ncomb * 8, e->st));
        launch_edge_key(e->d_edges.p, n, dcomb.p, k0.p, v0.p, e->st);
        HIPCHK(hipGetLastError());
        size_t tmp = 0;
        HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp, k0.p, k1.p, v0.p, v1.p, (size_t)n, 0u, 32u, e->st));
        CHK(e->work.d_tmp.ensure(tmp));
        HIPCHK(rocprim::radix_sort_pairs(e->work.d_tmp.p, tmp, k0.p, k1.p, v0.p, v1.p, (size_t)n, 0u, 32u, e->st));
        uint32_t last = 0;
        HIPCHK(hipMemcpyAsync(&last, k1.p + n - 1, 4, hipMemcpyDeviceToHost, e->st));
        // the (a, b) arrays reuse the sort's input buffers
        launch_edge_uv(e->d_edges.p, v1.p, k1.p, n, k0.p, v0.p, dfirst.p, e->st);
        HIPCHK(hipGetLastError());
        G.U = Raw<uint32_t>(n);
        G.V = Raw<uint32_t>(n);
        HIPCHK(hipMemcpyAsync(G.U.data(), k0.p, n * 4, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(G.V.data(), v0.p, n * 4, hipMemcpyDeviceToHost, e->st));
        if (ncomb) HIPCHK(hipMemcpyAsync(first.data(), dfirst.p, ncomb * 8, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipStreamSynchronize(e->st));
        if (last == ~0u)
            return fail(RC_E_STATE, "an imported graph with isolated nodes or rows outside it: no graph.pkl from edges");
    }
    // the tables: combinations with records, in order (a table ends where the
    // next one starts)
    uint64_t end = n;
    std::vector<GraphSlots::Tab> rev;
    for (size_t c = ncomb; c-- > 0;) {
        if (first[c] == ~0ull) continue;
        const uint64_t o = first[c];
        rev.push_back(GraphSlots::Tab{e->gene_sample[G.U[o]], e->gene_sample[G.V[o]], o, end - o});
        end = o;
    }
    G.tabs.assign(rev.rbegin(), rev.rend());
    return RC_OK;
}

static int write_graph_slots(const rc_engine *e, GraphSlots &G, const char *path)
{
    std::vector<const char *> names;
    for (const SampleRec &s : e->samples) names.push_back(s.label.c_str());
    return graph_pickle_write_slots(G, path, (int32_t)names.size(), names.data());
}

extern "C" int rc_write_graph(rc_engine *e, const char *path, int32_t threads)
{
    if (!e || !path) return fail(RC_E_ARG, "null argument");
    const char *otv = getenv("RC_OUT_TIMING");
    const bool otime = otv && atoi(otv);
    const auto t0 = std::chrono::steady_clock::now();
    (void)threads;   // (the writer sizes its own pool)
    GraphSlots G;
    CHK(edge_slots(e, G));
    if (otime)
        fprintf(stderr, "rc_write_graph: edge records sorted and fetched %.3f s\n",
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return write_graph_slots(e, G, path);
}

// The outputs a run writes next to matrix.h5: the od2 gene matches tables of
// the given pairs (paths[i] for pair (s1[i], s2[i]), table_paths may be NULL)
// and graph.pkl (graph_path, may be NULL; build_graph's graph over the pairs
// in the given order -- every pair of a single-shard engine, in combinations
// order). Each pair's rows leave the device once; the calling thread fetches
// them in order, `threads` workers convert and write the tables (od2_tables.
// cpp), one more thread builds and writes the pickle (graph_pickle.cpp) --
// all outside the Python interpreter.
int rc_write_outputs(rc_engine *e, int32_t n_pairs, const int32_t *s1, const int32_t *s2,
                     const char *const *table_paths, const char *graph_path, int32_t threads)
{
    if (!e || n_pairs < 0 || (n_pairs && (!s1 || !s2))) return fail(RC_E_ARG, "null argument");
    if (!table_paths && !graph_path) return RC_OK;
    if (graph_path && e->o.shard_count != 1)
        return fail(RC_E_STATE, "a sharded engine holds only its own pairs' rows: graph.pkl comes from the edges");
    const int nt = std::max(1, std::min(64, (int)threads));
    // RC_OUT_TIMING=1: where the time goes (stderr)
    const char *otv = getenv("RC_OUT_TIMING");
    const bool otime = otv && atoi(otv);
    std::atomic<long long> t_fetch{0}, t_conv{0}, t_write{0}, t_gadd{0}, t_gwrite{0};
    auto now_ns = []() {
        return (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(
                   std::chrono::steady_clock::now().time_since_epoch()).count();
    };
    const long long t_start = now_ns();
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::pair<int, std::shared_ptr<PairRaw>>> tq, gq;
    bool closed = false;
    int in_flight = 0, err = RC_OK;
    std::string err_msg;
    auto set_err = [&](int code) {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (err == RC_OK) {
                err = code;
                err_msg = rc_last_error();
            }
        }
        cv.notify_all();   // the fetch loop may be waiting for room
    };
    // graph.pkl over every pair in combinations order comes from the edge
    // records (sorted on the device first), written on its own thread beside
    // the tables; other pair lists (and imported graphs) take the rows
    GraphSlots gslots;
    bool edge_graph = false;
    if (graph_path) {
        const int N = (int)e->samples.size();
        bool all = (int64_t)n_pairs == (int64_t)N * (N - 1) / 2;
        for (int a = 0, k = 0; all && a < N; a++)
            for (int b = a + 1; all && b < N; b++, k++) all = s1[k] == a && s2[k] == b;
        edge_graph = all && edge_slots(e, gslots) == RC_OK;
    }
    auto worker = [&]() {
        std::vector<rc_row> buf;
        for (;;) {
            std::pair<int, std::shared_ptr<PairRaw>> job;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !tq.empty() || closed; });
                if (tq.empty()) return;
                job = std::move(tq.front());
                tq.pop_front();
            }
            const PairRaw &raw = *job.second;
            const int32_t js1 = raw.s1, js2 = raw.s2;
            const long long c0 = now_ns();
            buf.resize(raw.n);
            convert_rows(e, raw, buf.data());
            job.second.reset();   // (its slab goes back once the grapher is done too)
            const long long c1 = now_ns();
            const int rc = od2_write_table(buf.data(), buf.size(), e->samples[js1].label, e->samples[js2].label,
                                           table_paths[job.first]);
            t_conv += c1 - c0;
            t_write += now_ns() - c1;
            if (rc != RC_OK) set_err(rc);
            {
                std::lock_guard<std::mutex> lk(mu);
                in_flight--;
            }
            cv.notify_all();
        }
    };
    auto grapher = [&]() {
        rc_gpickle *g = nullptr;
        bool ok = true;
        if (rc_graph_pickle_begin(&g) != RC_OK) {
            // keep draining the queue (in_flight must still go down)
            set_err(RC_E_NOMEM);
            g = nullptr;
            ok = false;
        }
        for (;;) {
            std::pair<int, std::shared_ptr<PairRaw>> job;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !gq.empty() || closed; });
                if (gq.empty()) break;
                job = std::move(gq.front());
                gq.pop_front();
            }
            const PairRaw &raw = *job.second;
            const long long a0 = now_ns();
            const size_t n = raw.n;
            // the table's gene arrays, written in place (node numbering and
            // edges happen in parallel when the pickle is written)
            int64_t *sg = nullptr, *qg = nullptr;
            if (ok && graph_pickle_table(g, raw.s1, raw.s2, n, &sg, &qg) != RC_OK) {
                set_err(RC_E_LIMIT);
                ok = false;
            }
            if (ok)
                for (size_t i = 0; i < n; i++) {
                    const DHsp &d = raw.hs[i];
                    const bool rev = raw.rows[i].reverse != 0;
                    qg[i] = e->tx_gene_id[rev ? d.s_tx : d.q_tx];   // qgene: the transcript of s2
                    sg[i] = e->tx_gene_id[rev ? d.q_tx : d.s_tx];
                }
            t_gadd += now_ns() - a0;
            {
                std::lock_guard<std::mutex> lk(mu);
                in_flight--;
            }
            cv.notify_all();
        }
        if (ok) {
            const long long w0 = now_ns();
            std::vector<const char *> names;
            for (const SampleRec &s : e->samples) names.push_back(s.label.c_str());
            if (rc_graph_pickle_write(g, graph_path, (int32_t)names.size(), names.data()) != RC_OK) set_err(RC_E_IO);
            t_gwrite += now_ns() - w0;
        }
        rc_graph_pickle_free(g);
    };
    // every pair's row range first: the pinned slabs are sized to the largest
    std::vector<uint64_t> ranges(2 * (size_t)n_pairs);
    uint64_t max_rows = 0;
    for (int i = 0; i < n_pairs && (table_paths || !edge_graph); i++) {
        CHK(pair_row_range(e, s1[i], s2[i], ranges[2 * i], ranges[2 * i + 1]));
        max_rows = std::max<uint64_t>(max_rows, ranges[2 * i + 1] - ranges[2 * i]);
    }
    SlabPool slabs;
    slabs.bytes = std::max<uint64_t>(max_rows, 1) * (sizeof(DRow) + sizeof(DHsp));
    slabs.cap = (size_t)(2 * nt + 8);
    auto edge_grapher = [&]() {
        const long long w0 = now_ns();
        const int rc = write_graph_slots(e, gslots, graph_path);
        if (rc != RC_OK) set_err(rc);
        t_gwrite += now_ns() - w0;
    };
    std::vector<std::thread> pool;
    if (table_paths)
        for (int i = 0; i < nt; i++) pool.emplace_back(worker);
    if (graph_path) pool.emplace_back(edge_graph ? std::function<void()>(edge_grapher) : std::function<void()>(grapher));
    const bool row_graph = graph_path && !edge_graph;
    const int per_job = (table_paths ? 1 : 0) + (row_graph ? 1 : 0);
    const int max_flight = 4 * nt + 4;
    int rc = RC_OK;
    for (int i = 0; i < n_pairs && rc == RC_OK && per_job; i++) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return in_flight < max_flight * per_job || err != RC_OK; });
            if (err != RC_OK) break;
        }
        auto raw = std::make_shared<PairRaw>();
        const long long f0 = now_ns();
        rc = fetch_pair(e, s1[i], s2[i], *raw, &slabs, &ranges[2 * (size_t)i]);
        t_fetch += now_ns() - f0;
        if (rc != RC_OK) break;
        {
            std::lock_guard<std::mutex> lk(mu);
            if (table_paths) tq.push_back({i, raw});
            if (row_graph) gq.push_back({i, raw});
            in_flight += per_job;
        }
        cv.notify_all();
    }
    {
        std::lock_guard<std::mutex> lk(mu);
        closed = true;
    }
    cv.notify_all();
    for (std::thread &t : pool) t.join();
    if (otime)
        fprintf(stderr, "rc_write_outputs: %.3f s wall; fetch %.3f s, convert %.3f, table write %.3f (thread-s, %d threads), "
                        "graph add %.3f, graph write %.3f\n", (now_ns() - t_start) * 1e-9, t_fetch * 1e-9, t_conv * 1e-9,
                t_write * 1e-9, nt, t_gadd * 1e-9, t_gwrite * 1e-9);
    if (rc != RC_OK) return rc;
    if (err != RC_OK) return fail(err, err_msg);
    return RC_OK;
}

}  // extern "C"
