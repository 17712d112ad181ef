// Host side of the MI355X RNA-clique engine: the C ABI of include/rcgpu.h.
//
// Owns the device buffers and drives the kernels of kernels.hip on one HIP
// stream, from rc_create to the finished graph phase. What a caller reads out
// of a finished engine is in results.hip (converted back to reference
// semantics: 1-based BLAST coordinates, pandas index labels, sorted-label
// matrix order) and analysis.hip.
#include "engine.h"

static thread_local std::string g_err;

int rcg_fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

// Device bytes the engines of this process hold (now and at most), for the
// HBM footprint checks (rc_timing.dev_bytes / dev_peak_bytes)
static std::atomic<long long> g_dev_bytes{0}, g_dev_peak{0};
void dev_account(long long b)
{
    const long long v = g_dev_bytes.fetch_add(b) + b;
    long long pk = g_dev_peak.load();
    while (v > pk && !g_dev_peak.compare_exchange_weak(pk, v)) {
    }
}

// every byte is A/C/G/T in either case (a branch-free inner loop the compiler
// vectorises; the scan stops at the first 64 KiB block holding another byte)
static bool all_acgt(const char *s, uint64_t n)
{
    for (uint64_t i0 = 0; i0 < n; i0 += 65536) {
        const uint64_t i1 = std::min<uint64_t>(n, i0 + 65536);
        unsigned bad = 0;
        for (uint64_t i = i0; i < i1; i++) {
            const unsigned char c = (unsigned char)s[i] | 0x20;
            bad |= (unsigned)((c != 'a') & (c != 'c') & (c != 'g') & (c != 't'));
        }
        if (bad) return false;
    }
    return true;
}

// ------------------------------------------------------------------------
// Karlin-Altschul statistics (BLAST restated; same spec as the oracle)
// ------------------------------------------------------------------------
namespace stats {

// BLAST_ComputeLengthAdjustment
int32_t length_adjustment(double m, double n, double N)
{
    const double logK = std::log(K), adl = ALPHA / LAMBDA;
    double ell = 0, ss, ell_min = 0, ell_max, ell_next = 0;
    bool converged = false;
    {
        const double a = N, mb = m * N + n, c = n * m - std::max(m, n) / K;
        if (c < 0) return 0;
        ell_max = 2 * c / (mb + std::sqrt(mb * mb - 4 * a * c));
    }
    for (int i = 1; i <= 20; i++) {
        ell = ell_next;
        ss = (m - ell) * (n - N * ell);
        const double ell_bar = adl * (logK + std::log(ss)) + BETA;
        if (ell_bar >= ell) {
            ell_min = ell;
            if (ell_bar - ell_min <= 1.0) {
                converged = true;
                break;
            }
            if (ell_min == ell_max) break;
        } else {
            ell_max = ell;
        }
        if (ell_min <= ell_bar && ell_bar <= ell_max)
            ell_next = ell_bar;
        else
            ell_next = (i == 1) ? ell_max : (ell_min + ell_max) / 2;
    }
    if (!converged) return (int32_t)ell_min;
    int32_t adj = (int32_t)ell_min;
    ell = std::ceil(ell_min);
    if (ell <= ell_max) {
        ss = (m - ell) * (n - N * ell);
        if (adl * (logK + std::log(ss)) + BETA >= ell) adj = (int32_t)ell;
    }
    return adj;
}

double search_space(int64_t qlen, int64_t dblen, int64_t dbn)
{
    const int32_t ell = length_adjustment((double)qlen, (double)dblen, (double)dbn);
    double mq = (double)(qlen - ell), nd = (double)(dblen - dbn * (int64_t)ell);
    if (mq < 1) mq = 1;
    if (nd < 1) nd = 1;
    return mq * nd;
}

double evalue(double ss, int32_t score_half) { return ss * K * std::exp(-LAMBDA * (score_half / 2.0)); }

int32_t threshold(double ss, double cutoff)
{
    int32_t lo = 0, hi = 1 << 26;
    if (evalue(ss, hi) > cutoff) return hi;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (evalue(ss, mid) <= cutoff) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// CAlignFormatUtil::GetScoreString formatting of the bit score, in tenths
int32_t bits10(int32_t score_half)
{
    const double bits = (LAMBDA * (score_half / 2.0) - std::log(K)) / std::log(2.0);
    char buf[64];
    if (bits > 99999) {
        std::snprintf(buf, sizeof buf, "%5.3le", bits);
        return (int32_t)std::llround(std::strtod(buf, nullptr) * 10.0);
    }
    if (bits > 99.9) return (int32_t)((long)bits) * 10;
    std::snprintf(buf, sizeof buf, "%4.1lf", bits);
    return (int32_t)std::llround(std::strtod(buf, nullptr) * 10.0);
}
}  // namespace stats

// ------------------------------------------------------------------------
// engine
// ------------------------------------------------------------------------

static Knobs read_knobs()
{
    const auto env = [](const char *name) -> const char * { return getenv(name); };
    const auto num = [&](const char *name, int unset) { return env(name) ? atoi(env(name)) : unset; };
    Knobs k{};
    k.share = num("RC_SHARE", 1) != 0;
    k.tile_bases = env("RC_TILE_BASES") ? std::max<uint64_t>(strtoull(env("RC_TILE_BASES"), nullptr, 10), TILE_ALIGN)
                                        : (1ull << 32) - (1ull << 24);
    k.tile_split = num("RC_TILE_SPLIT", 1) != 0;
    k.ovf_cap0 = env("RC_OVF_CAP0") ? std::max(1, num("RC_OVF_CAP0", 1)) : 0;
    k.win_words = env("RC_WIN_WORDS") ? std::max(4, num("RC_WIN_WORDS", 4)) : 0;
    k.later = num("RC_LATER", 1) != 0;
    k.later_rows = num("RC_LATER_ROWS", 64);
    k.later_cap = env("RC_LATER_CAP") ? (uint64_t)std::max(atoll(env("RC_LATER_CAP")), 1ll) : (24ull << 20);
    k.rbh_two_pass = env("RC_RBH_TWO_PASS") != nullptr;
    k.resume = num("RC_RESUME", -1);
    k.index_cap = env("RC_INDEX_CAP") ? (uint32_t)std::max(2, num("RC_INDEX_CAP", 2)) : 0u;
    k.nj_lds = std::min(128, std::max(0, num("RC_NJ_LDS", 128)));
    return k;
}

extern "C" {

void rc_default_opts(rc_opts *o)
{
    o->top_matches = 1;
    o->keep_all = 1;
    o->evalue = 1e-99;
    o->word_size = 28;
    o->xdrop_half = 108;
    o->device = 0;
    o->shard_rank = 0;
    o->shard_count = 1;
    o->symmetric = 0;
    o->dust_level = 20;
    o->dust_window = 64;
    o->dust_linker = 1;
}

const char *rc_last_error(void) { return g_err.c_str(); }

void rc_dev_peak_reset(void) { g_dev_peak.store(g_dev_bytes.load()); }

uint64_t rc_edge_record_size(void) { return sizeof(DEdge); }

int rc_create(const rc_opts *opts, rc_engine **out)
{
    if (!opts || !out) return fail(RC_E_ARG, "null argument");
    if (opts->top_matches < 1) return fail(RC_E_ARG, "top_matches must be >= 1");
    if (opts->word_size < W16 || opts->word_size > 64) return fail(RC_E_ARG, "word_size must be in [16, 64]");
    if (opts->xdrop_half < 0) return fail(RC_E_ARG, "xdrop_half must be >= 0");
    if (opts->dust_level < 0 || (opts->dust_level > 0 && (opts->dust_window < 8 || opts->dust_window > 64 ||
                                                          opts->dust_linker < 0)))
        return fail(RC_E_ARG, "bad DUST parameters");
    if (opts->dust_level > 0 && opts->symmetric)
        return fail(RC_E_ARG, "DUST masks each direction's query: it needs symmetric = 0");
    if (opts->shard_count < 1 || opts->shard_rank < 0 || opts->shard_rank >= opts->shard_count)
        return fail(RC_E_ARG, "bad shard");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return fail(RC_E_HIP, "no HIP device available");
    }
    if (opts->device < 0 || opts->device >= ndev) return fail(RC_E_ARG, "bad device ordinal");
    rc_engine *e = new rc_engine();
    e->o = *opts;
    e->knobs = read_knobs();
    e->share = !e->o.symmetric && e->knobs.share;
    if (hipSetDevice(e->o.device) != hipSuccess || hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&e->st2, hipStreamNonBlocking) != hipSuccess) {
        delete e;
        return fail(RC_E_HIP, "stream creation failed");
    }
    for (auto &ev : e->evd)
        if (hipEventCreate(&ev) != hipSuccess) {
            delete e;
            return fail(RC_E_HIP, "event creation failed");
        }
    for (auto &ev : e->ev)
        if (hipEventCreate(&ev) != hipSuccess) {
            delete e;
            return fail(RC_E_HIP, "event creation failed");
        }
    *out = e;
    return RC_OK;
}

int rc_destroy(rc_engine *e)
{
    if (!e) return RC_OK;
    (void)hipSetDevice(e->o.device);
    delete e;  // DBuf destructors free the device buffers
    return RC_OK;
}

int rc_add_sample(rc_engine *e, const char *label, const char *seq, const uint64_t *tx_offsets,
                  const int32_t *gene, const int32_t *iso, uint32_t n_tx, int32_t *sample_id)
{
    if (!e || !label || !tx_offsets || (n_tx && (!gene || !iso))) return fail(RC_E_ARG, "null argument");
    if (e->uploaded) return fail(RC_E_STATE, "samples must be added before rc_run");
    if (e->samples.size() >= MAX_SAMPLES) return fail(RC_E_LIMIT, "at most 65535 samples per engine");
    if (tx_offsets[0] != 0) return fail(RC_E_ARG, "tx_offsets[0] must be 0");
    for (uint32_t t = 0; t < n_tx; t++) {
        if (tx_offsets[t + 1] < tx_offsets[t]) return fail(RC_E_ARG, "tx_offsets must be non-decreasing");
        if (tx_offsets[t + 1] - tx_offsets[t] > (1u << 24) - 64)
            return fail(RC_E_LIMIT, "transcripts longer than 16 Mbp are not supported");
    }
    const uint64_t nb = tx_offsets[n_tx];
    SampleRec s;
    s.label = label;
    s.base = e->total_bases;
    s.nbases = nb;
    s.tx_begin = (uint32_t)e->tx_sample.size();
    s.n_tx = n_tx;
    // seq == NULL with bases: a sample another GPU aligns (sharded runs hold
    // only the samples of their own pairs); its transcripts and genes still
    // count (graph nodes, e-value statistics)
    s.resident = nb == 0 || seq != nullptr;
    // the bases go straight to HBM (the ASCII array the pack kernels read), at
    // a TILE_ALIGN boundary (the gap filled with 'A'); the device array grows
    // geometrically, old contents moved device-side
    if (nb && seq) {
        CHK(set_device(e));
        s.abase = align_up(e->ascii_used);
        const uint64_t need = align_up(s.abase + nb) + 64;
        if (need > e->d_ascii.cap) {
            const size_t cap = std::max<size_t>({(size_t)need, e->d_ascii.cap + e->d_ascii.cap / 4, (size_t)1 << 28});
            uint8_t *np = nullptr;
            if (hipMalloc((void **)&np, cap) != hipSuccess) {
                (void)hipGetLastError();
                return fail(RC_E_NOMEM, "hipMalloc of " + std::to_string(cap) + " bytes failed");
            }
            if (e->ascii_used)
                HIPCHK(hipMemcpyAsync(np, e->d_ascii.p, e->ascii_used, hipMemcpyDeviceToDevice, e->st));
            HIPCHK(hipStreamSynchronize(e->st));
            e->d_ascii.adopt(np, cap);
        }
        HIPCHK(hipMemsetAsync(e->d_ascii.p + e->ascii_used, 'A', need - e->ascii_used, e->st));
        HIPCHK(hipMemcpyAsync(e->d_ascii.p + s.abase, seq, nb, hipMemcpyHostToDevice, e->st));
        if (!e->has_amb) e->has_amb = !all_acgt(seq, nb);
        HIPCHK(hipStreamSynchronize(e->st));   // the caller's buffer is not retained
        e->ascii_used = s.abase + nb;
    }
    e->total_bases += nb;
    const int32_t sid = (int32_t)e->samples.size();
    for (uint32_t t = 0; t < n_tx; t++) {
        e->tx_start.push_back(s.base + tx_offsets[t + 1]);
        e->tx_sample.push_back(sid);
        e->tx_gene_id.push_back(gene[t]);
        e->tx_iso.push_back(iso[t]);
    }
    e->samples.push_back(s);
    if (sample_id) *sample_id = sid;
    return RC_OK;
}

int rc_add_hsps(rc_engine *e, int32_t q, int32_t s, const rc_hsp *h, uint64_t n)
{
    if (!e || (n && !h)) return fail(RC_E_ARG, "null argument");
    if (e->uploaded) return fail(RC_E_STATE, "HSPs must be added before rc_run");
    const int N = (int)e->samples.size();
    if (q < 0 || q >= N || s < 0 || s >= N || q == s) return fail(RC_E_ARG, "bad sample pair");
    for (uint64_t i = 0; i < n; i++)
        if (h[i].q_tx >= e->samples[q].n_tx || h[i].s_tx >= e->samples[s].n_tx)
            return fail(RC_E_ARG, "HSP transcript index out of range");
    e->external = true;
    auto &v = e->ext[{q, s}];
    v.insert(v.end(), h, h + n);
    return RC_OK;
}

}  // extern "C"

// Build gene numbering, tables and upload everything that does not change
// between runs. Inputs are then resident in HBM; rc_run repacks from them.
static void shard_pairs(rc_engine *e);

// Shard plan. The C(N,2) sample pairs (a < b) are the cells
// of the (a, b) triangle; shard_count shards each take one rectangle
// [a0, a1) x [b0, b1) of it, found by recursive bisection that minimises the
// largest shard's modelled time. Both directed searches of a pair run on its
// shard, so the shard's samples -- the ones it holds, indexes and scans --
// are [a0, a1) u [b0, b1):
//   pair work    2 x (L_a + L_b) per pair (seed hits, extension, RBH)
//   queries      9 x L_s per query sample (the seed kernel's per-gene work)
//   subjects    15 x L_s per subject sample (16-mer index + reverse pass)
// (r04: least squares over the eight C3 rank shards with shared DUST masks,
// scripts/shard_time.py, profiles/r04_n: 0.94 ms per query sample, 1.5 per
// subject sample, 0.41 per pair). Pairs are
// numbered shard by shard, subject-major inside a shard; one shard gives the
// plain subject-major order (0,1), (0,2), (1,2), (0,3), ...
namespace plan {
struct Rect {
    int a0, a1, b0, b1;
};
struct Planner {
    int N;
    std::vector<double> SL;   // prefix sums of sample bases
    std::map<std::array<int, 5>, std::pair<double, std::vector<Rect>>> memo;
    double S(int i, int j) const { return j > i ? SL[j] - SL[i] : 0.0; }
    static Rect norm(Rect r)
    {
        r.a1 = std::min(r.a1, r.b1 - 1);
        r.b0 = std::max(r.b0, r.a0 + 1);
        if (r.a1 <= r.a0 || r.b1 <= r.b0) r = Rect{0, 0, 0, 0};
        return r;
    }
    static bool empty(const Rect &r) { return r.a1 <= r.a0 || r.b1 <= r.b0; }
    double leaf(const Rect &r) const
    {
        if (empty(r)) return 0.0;
        double pw = 0.0;
        for (int b = r.b0; b < r.b1; b++) {
            const int ae = std::min(r.a1, b);
            if (ae > r.a0) pw += S(r.a0, ae) + (double)(ae - r.a0) * (SL[b + 1] - SL[b]);
        }
        // a sample that is both a query and a subject of the rank pays both
        return 2.0 * pw + 9.0 * S(r.a0, r.a1) + 15.0 * S(r.b0, r.b1);
    }
    std::pair<double, std::vector<Rect>> best(Rect r, int k)
    {
        r = norm(r);
        const std::array<int, 5> key{r.a0, r.a1, r.b0, r.b1, k};
        auto it = memo.find(key);
        if (it != memo.end()) return it->second;
        std::pair<double, std::vector<Rect>> res{leaf(r), std::vector<Rect>(k, Rect{0, 0, 0, 0})};
        res.second[0] = r;
        if (k > 1 && !empty(r)) {
            const int k1 = k / 2;
            auto consider = [&](Rect x, Rect y) {
                for (int sw = 0; sw < (k1 == k - k1 ? 1 : 2); sw++) {
                    const int kx = sw ? k - k1 : k1;
                    const auto X = best(x, kx);
                    if (X.first >= res.first) continue;
                    const auto Y = best(y, k - kx);
                    const double c = std::max(X.first, Y.first);
                    if (c < res.first) {
                        res.first = c;
                        res.second = X.second;
                        res.second.insert(res.second.end(), Y.second.begin(), Y.second.end());
                    }
                }
            };
            const int nc = N > 128 ? 12 : 32;   // cut candidates per axis
            const int sa = std::max(1, (r.a1 - r.a0) / nc), sb = std::max(1, (r.b1 - r.b0) / nc);
            for (int c = r.a0 + sa; c < r.a1; c += sa) consider({r.a0, c, r.b0, r.b1}, {c, r.a1, r.b0, r.b1});
            for (int c = r.b0 + sb; c < r.b1; c += sb) consider({r.a0, r.a1, r.b0, c}, {r.a0, r.a1, c, r.b1});
        }
        memo.emplace(key, res);
        return res;
    }
};

// pair order (pair_a, pair_b) and shard cuts pair_first[shard_count + 1]
static void plan_pairs(const int64_t *bases, int N, int shards, std::vector<int32_t> &pa, std::vector<int32_t> &pb,
                       std::vector<int64_t> &first)
{
    pa.clear();
    pb.clear();
    first.assign((size_t)shards + 1, 0);
    std::vector<Rect> rects;
    if (shards == 1) {
        rects.push_back(Planner::norm({0, N, 0, N}));
    } else {
        Planner P;
        P.N = N;
        P.SL.assign((size_t)N + 1, 0.0);
        for (int i = 0; i < N; i++) P.SL[i + 1] = P.SL[i] + (double)std::max<int64_t>(bases[i], 1);
        rects = P.best({0, N, 0, N}, shards).second;
    }
    for (int r = 0; r < shards; r++) {
        first[r] = (int64_t)pa.size();
        const Rect q = rects[r];
        for (int b = q.b0; b < q.b1; b++)
            for (int a = q.a0; a < std::min(q.a1, b); a++) {
                pa.push_back(a);
                pb.push_back(b);
            }
    }
    first[shards] = (int64_t)pa.size();
}
}  // namespace plan

static int upload(rc_engine *e)
{
    if (e->uploaded) return RC_OK;
    CHK(set_device(e));
    const int N = (int)e->samples.size();
    if (N < 2) return fail(RC_E_ARG, "need at least two samples");
    if (N > MAX_SAMPLES) return fail(RC_E_LIMIT, "more than 65535 samples per engine");
    if (e->tx_sample.size() >= MAX_TX) return fail(RC_E_LIMIT, "more than 2^27 transcripts per engine");
    const uint32_t n_tx = (uint32_t)e->tx_sample.size();
    // genes: per sample distinct gene ids ascending; a gene's transcripts in input order
    e->tx_gene.assign(n_tx, 0);
    e->gene_tx_off.assign(1, 0);
    e->gene_tx.clear();
    e->gene_sample.clear();
    e->gene_id.clear();
    e->sample_gene_begin.assign(N + 1, 0);
    e->sample_tx_begin.assign(N + 1, 0);
    e->db_len.assign(N, 0);
    e->db_n.assign(N, 0);
    e->max_len = 0;
    for (int si = 0; si < N; si++) {
        SampleRec &s = e->samples[si];
        e->sample_tx_begin[si] = s.tx_begin;
        s.gene_begin = (uint32_t)e->gene_sample.size();
        e->sample_gene_begin[si] = s.gene_begin;
        std::vector<std::pair<int32_t, uint32_t>> byg;
        for (uint32_t t = 0; t < s.n_tx; t++) byg.push_back({e->tx_gene_id[s.tx_begin + t], s.tx_begin + t});
        std::stable_sort(byg.begin(), byg.end(),
                         [](const std::pair<int32_t, uint32_t> &a, const std::pair<int32_t, uint32_t> &b) {
                             return a.first < b.first;
                         });
        for (size_t i = 0; i < byg.size(); i++) {
            if (i == 0 || byg[i].first != byg[i - 1].first) {
                if (i) e->gene_tx_off.push_back((uint32_t)e->gene_tx.size());
                e->gene_sample.push_back(si);
                e->gene_id.push_back(byg[i].first);
            }
            e->tx_gene[byg[i].second] = (uint32_t)(e->gene_sample.size() - 1);
            e->gene_tx.push_back(byg[i].second);
        }
        if (!byg.empty()) e->gene_tx_off.push_back((uint32_t)e->gene_tx.size());
        s.n_genes = (uint32_t)e->gene_sample.size() - s.gene_begin;
        for (uint32_t t = 0; t < s.n_tx; t++) {
            const uint64_t L = e->tx_start[s.tx_begin + t + 1] - e->tx_start[s.tx_begin + t];
            e->db_len[si] += (int64_t)L;
            e->max_len = std::max<int32_t>(e->max_len, (int32_t)L);
        }
        e->db_n[si] = s.n_tx;
    }
    e->sample_tx_begin[N] = n_tx;
    e->sample_gene_begin[N] = (uint32_t)e->gene_sample.size();
    const uint32_t n_genes = (uint32_t)e->gene_sample.size();
    // the seed key's position field holds the longest transcript; its
    // isoform field the rest (max_iso: 65535 unless transcripts reach 2^21)
    e->xbits = pos_bits(e->max_len);
    for (uint32_t g = 0; g < n_genes; g++)
        if (e->gene_tx_off[g + 1] - e->gene_tx_off[g] > max_iso(e->xbits))
            return fail(RC_E_LIMIT, "gene " + std::to_string(e->gene_id[g]) + " has more than " +
                                        std::to_string(max_iso(e->xbits)) + " transcripts");
    // pairs (a < b) in the shard plan's order (plan::plan_pairs): every
    // shard a rectangle [a0, a1) x [b0, b1) of the pair triangle; items =
    // (pair, gene of b). (Outputs are per pair and do not depend on this.)
    {
        std::vector<int64_t> bases(N);
        for (int i = 0; i < N; i++) bases[i] = e->db_len[i];
        plan::plan_pairs(bases.data(), N, e->o.shard_count, e->pair_a, e->pair_b, e->shard_first);
    }
    e->pair_item_begin.assign(1, 0);
    e->pair_index.assign((size_t)N * N, -1);
    uint64_t items = 0;
    for (size_t p = 0; p < e->pair_a.size(); p++) {
        const int a = e->pair_a[p], b = e->pair_b[p];
        e->pair_index[a * N + b] = e->pair_index[b * N + a] = (int32_t)p;
        items += e->samples[b].n_genes;
        if (items > 0xFFFFFFFFull) return fail(RC_E_LIMIT, "too many (pair, gene) items");
        e->pair_item_begin.push_back((uint32_t)items);
    }
    e->n_items = items;
    shard_pairs(e);

    // device copies of what does not change between runs
    auto up = [&](auto &buf, const auto &vec) -> int {
        using T = typename std::remove_reference<decltype(vec)>::type::value_type;
        CHK(buf.ensure(vec.size()));
        if (!vec.empty())
            HIPCHK(hipMemcpyAsync(buf.p, vec.data(), vec.size() * sizeof(T), hipMemcpyHostToDevice, e->st));
        return RC_OK;
    };
    e->h_tx.assign(n_tx, TxInfo{});
    for (uint32_t t = 0; t < n_tx; t++) {
        e->h_tx[t].start = 0;   // a position in the current tile (load_tile)
        e->h_tx[t].len = (uint32_t)(e->tx_start[t + 1] - e->tx_start[t]);
        e->h_tx[t].sample = e->tx_sample[t];
    }
    CHK(up(e->d_tx, e->h_tx));
    {
        // per transcript: its start within its sample and the 16-mer slots of
        // the sample's transcripts before it (the tile tables' inputs)
        std::vector<uint64_t> rel(n_tx), kpre(n_tx);
        e->sample_kmers.assign(N, 0);
        for (int si = 0; si < N; si++) {
            const SampleRec &S = e->samples[si];
            uint64_t k = 0;
            for (uint32_t t = S.tx_begin; t < S.tx_begin + S.n_tx; t++) {
                rel[t] = e->tx_start[t] - S.base;
                kpre[t] = k;
                const int64_t L = (int64_t)e->h_tx[t].len;
                k += (uint64_t)(L >= W16 ? L - W16 + 1 : 0);
            }
            e->sample_kmers[si] = k;
        }
        CHK(up(e->d_tx_rel, rel));
        CHK(up(e->d_kpre, kpre));
        HIPCHK(hipStreamSynchronize(e->st));   // (rel, kpre are about to go)
    }
    {
        std::vector<IsoRec> giso(e->gene_tx.size());
        for (size_t k = 0; k < giso.size(); k++) {
            const TxInfo &x = e->h_tx[e->gene_tx[k]];
            giso[k] = IsoRec{(uint32_t)x.start, x.len, e->gene_tx[k], 0u};
        }
        CHK(up(e->d_giso, giso));
    }
    CHK(up(e->d_tx_gene, e->tx_gene));
    std::vector<uint32_t> tx_pos(n_tx, 0);
    for (uint32_t g = 0; g < n_genes; g++)
        for (uint32_t i = e->gene_tx_off[g]; i < e->gene_tx_off[g + 1]; i++) tx_pos[e->gene_tx[i]] = i - e->gene_tx_off[g];
    CHK(up(e->d_tx_pos, tx_pos));
    {
        // word-item prefix of every gene's isoforms (the seed kernel reads it
        // for genes with more than ISO_LDS isoforms): gene g's entries at
        // gene_tx_off[g] + g + i, i = 0..niso
        const int stride = e->o.word_size - W16 + 1;
        std::vector<uint32_t> ipre((size_t)n_tx + n_genes + 1, 0);
        for (uint32_t g = 0; g < n_genes; g++) {
            uint32_t pre = 0;
            const uint32_t b = e->gene_tx_off[g], n = e->gene_tx_off[g + 1] - b;
            for (uint32_t i = 0; i <= n; i++) {
                ipre[(size_t)b + g + i] = pre;
                if (i < n) {
                    const int64_t L = (int64_t)e->h_tx[e->gene_tx[b + i]].len;
                    pre += L >= W16 ? 2u * (uint32_t)((L - W16) / stride + 1) : 0u;
                }
            }
        }
        CHK(up(e->d_iso_pre, ipre));
    }
    CHK(up(e->d_gene_tx_off, e->gene_tx_off));
    CHK(up(e->d_gene_tx, e->gene_tx));
    CHK(up(e->d_gene_sample, e->gene_sample));
    CHK(up(e->d_sample_gene_begin, e->sample_gene_begin));
    CHK(up(e->d_sample_tx_begin, e->sample_tx_begin));
    CHK(up(e->d_pair_item_begin, e->pair_item_begin));
    CHK(up(e->d_pair_a, e->pair_a));
    CHK(up(e->d_pair_b, e->pair_b));
    CHK(up(e->d_pair_index, e->pair_index));
    // statistics tables
    std::vector<int32_t> thr((size_t)N * (e->max_len + 1));
    e->h_ss.assign((size_t)N * (e->max_len + 1), 0.0);
    for (int T = 0; T < N; T++)
        for (int32_t L = 0; L <= e->max_len; L++) {
            const size_t k = (size_t)T * (e->max_len + 1) + L;
            e->h_ss[k] = stats::search_space(L, e->db_len[T], e->db_n[T]);
            thr[k] = L ? stats::threshold(e->h_ss[k], e->o.evalue) : (1 << 26);
        }
    e->h_exp.resize((size_t)2 * e->max_len + 2);
    for (size_t sc = 0; sc < e->h_exp.size(); sc++) e->h_exp[sc] = std::exp(-stats::LAMBDA * ((int32_t)sc / 2.0));
    std::vector<int32_t> b10((size_t)2 * e->max_len + 2);
    for (size_t sc = 0; sc < b10.size(); sc++) b10[sc] = stats::bits10((int32_t)sc);
    CHK(up(e->d_thr, thr));
    CHK(up(e->d_bits10, b10));
    CHK(e->d_status.ensure(4));
    CHK(e->d_count.ensure(DC_N));
    HIPCHK(hipStreamSynchronize(e->st));
    e->work.tile_loaded = -1;
    e->uploaded = true;
    return RC_OK;
}

// ------------------------------------------------------------------------
// tiles
// ------------------------------------------------------------------------
//
// A tile is the unit of one alignment pass: a set of samples packed into one
// working copy (positions relative to the tile, < 2^32) and indexed together,
// and the directed searches between them. A shard's pairs form a rectangle
// [a0, a1) x [b0, b1) of the pair triangle; when its samples fit one tile
// (rc_opts-independent cap Knobs::tile_bases, default 2^32 - 2^24 bases) the
// shard is one tile, else the a- and b-ranges are cut into chunks of at most
// half the cap and every (a chunk, b chunk) with pairs is a tile. Each pass
// appends its HSPs to the shard's store; reciprocal best hits then run over
// all the shard's pairs.

static void plan_tiles(rc_engine *e)
{
    e->tiles.clear();
    std::vector<std::pair<int, int>> pairs;
    for (uint64_t p = e->pair0; p < e->pair1; p++) pairs.push_back({e->pair_a[p], e->pair_b[p]});
    if (pairs.empty()) return;
    auto bases = [&](int s) { return align_up(e->samples[s].nbases); };
    const uint64_t cap = e->knobs.tile_bases;
    std::vector<int> A, B, U;
    for (auto &pr : pairs) {
        A.push_back(pr.first);
        B.push_back(pr.second);
        U.push_back(pr.first);
        U.push_back(pr.second);
    }
    for (auto *v : {&A, &B, &U}) {
        std::sort(v->begin(), v->end());
        v->erase(std::unique(v->begin(), v->end()), v->end());
    }
    uint64_t ub = 0;
    for (int s : U) ub += bases(s);
    auto chunks = [&](const std::vector<int> &R, uint64_t lim) {
        std::vector<std::vector<int>> out(1);
        uint64_t acc = 0;
        for (int s : R) {
            if (!out.back().empty() && acc + bases(s) > lim) {
                out.push_back({});
                acc = 0;
            }
            out.back().push_back(s);
            acc += bases(s);
        }
        return out;
    };
    const bool multi = ub > cap;
    const auto CA = !multi ? std::vector<std::vector<int>>{U} : chunks(A, cap / 2);
    const auto CB = !multi ? std::vector<std::vector<int>>{U} : chunks(B, cap / 2);
    const bool no_split = !e->knobs.tile_split;
    uint64_t amax = 0;
    for (size_t j = 0; j < CB.size(); j++)
        for (size_t i = 0; i < CA.size(); i++) {
            rc_engine::Tile t;
            std::vector<char> ina(e->samples.size(), 0), inb(e->samples.size(), 0);
            for (int s : CA[i]) ina[s] = 1;
            for (int s : CB[j]) inb[s] = 1;
            int amax_s = -1, bmin_s = INT32_MAX;
            for (auto &pr : pairs)
                if (ina[pr.first] && inb[pr.second]) {
                    t.pairs.push_back(pr);
                    amax_s = std::max(amax_s, pr.first);
                    bmin_s = std::min(bmin_s, pr.second);
                }
            if (t.pairs.empty()) continue;
            for (auto &pr : t.pairs) {
                t.samples.push_back(pr.first);
                t.samples.push_back(pr.second);
            }
            std::sort(t.samples.begin(), t.samples.end());
            t.samples.erase(std::unique(t.samples.begin(), t.samples.end()), t.samples.end());
            if (multi && !no_split && amax_s < bmin_s) {
                // every a below every b: the b part (all of CB[j]: each of its
                // samples pairs with the a's) after a part padded to the
                // largest a part of any split tile
                t.bchunk = (int)j;
                uint64_t ab = 0;
                for (int s : t.samples)
                    if (s <= amax_s) ab += bases(s);
                amax = std::max(amax, ab);
            }
            e->tiles.push_back(t);
        }
    for (auto &t : e->tiles)
        if (t.bchunk >= 0) t.bstart = amax;
}

// Device tables of tile ti: packed working copy (gathered from d_ascii unless
// the tile is d_ascii's layout), transcript starts, sample ranges, the
// position -> transcript blocks and transcript-start bits, and the tile's
// transcripts for the index. Kept while the same tile is loaded.
static int load_tile(rc_engine *e, int ti)
{
    const rc_engine::Tile &T = e->tiles[ti];
    const int N = (int)e->samples.size();
    e->tile_pos.assign(N + 1, 0);
    std::vector<char> in(N, 0);
    for (int s : T.samples) in[s] = 1;
    // layout: tile samples in ascending order, each at a TILE_ALIGN boundary;
    // d_ascii holds exactly that layout when the tile is every resident sample.
    // A split tile's b part starts at T.bstart (after the a part's padding)
    uint64_t pos = 0;
    bool direct = T.bchunk < 0;
    int amax_s = -1;
    if (T.bchunk >= 0)
        for (auto &pr : T.pairs) amax_s = std::max(amax_s, pr.first);
    for (int s = 0; s < N; s++) {
        if (!in[s]) continue;
        if (T.bchunk >= 0 && s > amax_s && pos < T.bstart) pos = T.bstart;
        e->tile_pos[s] = pos;
        direct = direct && e->samples[s].abase == pos;
        pos += align_up(e->samples[s].nbases);
    }
    for (int s = 0; s < N; s++)
        if (e->samples[s].resident && e->samples[s].nbases && !in[s]) direct = false;
    const uint64_t total = pos;
    if (total >= (1ull << 32)) return fail(RC_E_LIMIT, "a tile of more than 2^32 bases");
    e->tile_total = total;
    e->tile_direct = direct;
    // the 16-mer index holds the tile's subject samples only: the b of each
    // pair (shared searches and spec 5b: query = the lower sample), or both
    const bool share = e->share;
    if (e->work.tile_loaded == ti) return RC_OK;
    std::vector<char> subj(N, 0);
    for (auto &pr : T.pairs) {
        subj[pr.second] = 1;
        if (!share && !e->o.symmetric) subj[pr.first] = 1;
    }
    // Per tile sample one TileSeg; the device builds every per-transcript and
    // per-base table from them (launch_tile_tables): transcript starts in the
    // tile, the tile's transcripts and the index's with their closed-form
    // k-mer slots, the transcript-start bits and the position -> transcript
    // blocks. The host keeps O(samples) bookkeeping only.
    auto &segs = e->h_segs;
    auto &spos = e->h_spos;   // sample ranges, monotone over all N + 1 (a sample outside the tile is empty)
    auto &send = e->h_send;   // one past each tile sample's padded range (0: not in the tile)
    segs.clear();
    spos.assign(N + 1, total);
    send.assign(N, 0);
    {
        uint64_t next = total;
        for (int s = N; s >= 0; s--) {
            if (s < N && in[s]) next = e->tile_pos[s];
            spos[s] = next;
        }
    }
    uint32_t n_ttx = 0, n_itx = 0;
    uint64_t npos = 0;
    e->tile_tx_first.assign(N + 1, 0);
    for (int s = 0; s < N; s++) {
        e->tile_tx_first[s] = n_ttx;
        if (!in[s]) continue;
        const SampleRec &S = e->samples[s];
        send[s] = e->tile_pos[s] + align_up(S.nbases);
        if (!S.n_tx) continue;
        TileSeg g;
        g.pos = e->tile_pos[s];
        g.kbase = npos;
        g.pad_bit = S.nbases < align_up(S.nbases) ? e->tile_pos[s] + S.nbases : ~0ull;
        g.tx0 = S.tx_begin;
        g.ntx = S.n_tx;
        g.ttx0 = n_ttx;
        g.itx0 = subj[s] ? n_itx : ~0u;
        segs.push_back(g);
        n_ttx += S.n_tx;
        if (subj[s]) {
            n_itx += S.n_tx;
            npos += e->sample_kmers[s];
        }
    }
    e->tile_tx_first[N] = n_ttx;
    if (npos > 0xFFFFFFFFull) return fail(RC_E_LIMIT, "more than 2^32 seed positions in a tile");
    const uint64_t nblocks = (total >> POS_TX_SHIFT) + 2, nwb = (total >> 6) + 4;
    CHK(e->work.d_tile_segs.ensure(std::max<size_t>(segs.size(), 1)));
    CHK(e->work.d_tile_tx.ensure(std::max<uint32_t>(n_ttx, 1)));
    CHK(e->work.d_tile_gid.ensure(std::max<uint32_t>(n_ttx, 1)));
    CHK(e->work.d_tile_itx.ensure(std::max<uint32_t>(n_itx, 1)));
    CHK(e->work.d_kpos_off.ensure((size_t)n_itx + 1));
    CHK(e->work.d_pos_tx.ensure(nblocks));
    CHK(e->work.d_sample_pos.ensure(spos.size()));
    CHK(e->work.d_tile_send.ensure(send.size()));
    CHK(e->work.d_txstart.ensure(nwb));
    if (!segs.empty())
        HIPCHK(hipMemcpyAsync(e->work.d_tile_segs.p, segs.data(), segs.size() * sizeof(TileSeg), hipMemcpyHostToDevice,
                              e->st));
    HIPCHK(hipMemcpyAsync(e->work.d_sample_pos.p, spos.data(), spos.size() * 8, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemcpyAsync(e->work.d_tile_send.p, send.data(), send.size() * 8, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemsetAsync(e->work.d_txstart.p, 0, nwb * 8, e->st));
    launch_tile_tables(e->work.d_tile_segs.p, (uint32_t)segs.size(), n_ttx, e->d_tx_rel.p, e->d_kpre.p, e->d_tx.p,
                       e->work.d_tile_tx.p, e->work.d_tile_gid.p, e->work.d_tile_itx.p, e->work.d_kpos_off.p, n_itx, npos,
                       e->work.d_txstart.p, e->d_giso.p, e->gene_tx.size(), e->work.d_tile_send.p, e->work.d_pos_tx.p, nblocks,
                       e->st);
    HIPCHK(hipGetLastError());
    e->tile_npos = npos;
    e->tile_ntx = n_ttx;
    e->tile_nitx = n_itx;
    // the packed working copy's source: d_ascii itself or a gathered copy
    if (!direct) {
        CHK(e->work.d_tile_ascii.ensure(total + 64));
        HIPCHK(hipMemsetAsync(e->work.d_tile_ascii.p, 'A', total + 64, e->st));
        for (int s = 0; s < N; s++)
            if (in[s] && e->samples[s].nbases)
                HIPCHK(hipMemcpyAsync(e->work.d_tile_ascii.p + e->tile_pos[s], e->d_ascii.p + e->samples[s].abase,
                                      e->samples[s].nbases, hipMemcpyDeviceToDevice, e->st));
    }
    // (no wait: the host tables above are engine members, kept until the
    // next load, which comes after this tile's last wait)
    e->work.tile_loaded = ti;
    return RC_OK;
}

// Sort index entries ent[0, npos) on key bits [bb, 64) into ent2 and build the
// bucket table over the top k-mer bits: about one bucket per entry (times
// 2^extra), at most 2^INDEX_BITS_MAX (28 measured best at C3 -- a 1 GiB table
// instead of 4 GiB, same seed-kernel time). counted: the fill left the
// sort's segment histograms in d_sort_scratch.
// G < 0 (the near-mask index; a main index of more entries than two global
// passes cut into LDS-sized ranges): 8-bit passes over the bits [bb, 64), then
// the bucket fill's pass over the sorted entries. G >= 0 (the main index, bb
// = 32): sort.hip's os_index_sort -- global passes on the top G k-mer bits, the
// rest and the bucket table per range in LDS.
constexpr int INDEX_BITS_MAX = 28;
static int index_bits(uint64_t npos, int extra)
{
    int bits = 16;
    while (bits < INDEX_BITS_MAX && (1ull << bits) < (npos << extra)) bits++;
    return bits;
}
static int sort_index(rc_engine *e, DBuf<uint64_t> &ent, DBuf<uint64_t> &ent2, uint64_t npos, unsigned bb, int extra,
                      DBuf<uint32_t> &bucket, int &bits_out, bool counted = false, int G = -1)
{
    const int bits = index_bits(npos, extra);
    bits_out = bits;
    CHK(bucket.ensure((1ull << bits) + 1));
    bool table_done = false;
    if (npos) {
        // the result must end in ent2
        if (npos > 0xFFFFFFFFull) return fail(RC_E_LIMIT, "more than 2^32 index entries");
        CHK(e->work.d_sort_scratch.ensure(G >= 0 ? os_index_scratch_words(npos) : os_scratch_words(npos)));
        const uint64_t words = G >= 0 ? os_index_status_words(npos) : os_status_words(npos);
        if (e->work.d_sort_status.cap < words) {
            CHK(e->work.d_sort_status.ensure(words));
            HIPCHK(hipMemsetAsync(e->work.d_sort_status.p, 0, words * sizeof(uint64_t), e->st));
        }
        bool in_alt;
        if (G >= 0) {
            CHK(e->work.d_range_off.ensure(os_index_offset_words(G)));
            CHK(e->work.d_range_list.ensure(os_index_list_words()));
            uint32_t fb_ranges = 0;
            uint64_t fb_keys = 0;
            bool whole = false;
            const int where = os_index_sort(ent.p, ent2.p, npos, G, bits, e->knobs.index_cap, e->work.d_sort_scratch.p,
                                            e->work.d_sort_status.p, e->sort_epoch, e->work.d_range_off.p,
                                            e->work.d_range_list.p, bucket.p, e->st, counted,
                                            [e] { return wait_st(e) == RC_OK; }, &fb_ranges, &fb_keys, &whole);
            if (where < 0) return fail(RC_E_HIP, "the index sort's read of its oversized ranges failed");
            in_alt = where == 1;
            table_done = !whole;
            e->tm.index_fb_ranges += (double)fb_ranges;
            e->tm.index_fb_keys += (double)fb_keys;
        } else {
            // (no callback after the table kernels, no key generator: keys come from the entry array)
            in_alt = os_sort_keys(ent.p, ent2.p, npos, (int)bb, e->work.d_sort_scratch.p, e->work.d_sort_status.p,
                                  e->sort_epoch, e->st, nullptr, counted, nullptr, nullptr, nullptr, 0u, nullptr);
        }
        HIPCHK(hipGetLastError());
        if (!in_alt) ent.swap(ent2);
    }
    if (!table_done) launch_bucket_fill(ent2.p, npos, bits, bucket.p, e->st);
    return RC_OK;
}

// A seed index: every 16-mer position of the transcripts txl[0, n_tx), whose
// slots koff / kpos (closed form when no base is ambiguous) give the order.
static int build_index_of(rc_engine *e, const TxInfo *txl, uint32_t n_tx, uint64_t npos, const uint64_t *kpos,
                          DBuf<uint64_t> &ent, DBuf<uint64_t> &ent2, DBuf<uint32_t> &bucket, int &bits_out,
                          uint64_t &n_out)
{
    const bool amb = e->has_amb;
    const uint64_t *offs = kpos;
    if (amb) {
        CHK(e->work.d_kcnt.ensure(n_tx + 1));
        HIPCHK(hipMemsetAsync(e->work.d_kcnt.p, 0, (n_tx + 1) * sizeof(uint64_t), e->st));
        if (n_tx) launch_kmer_count(txl, n_tx, e->work.d_AF.p + FRONT_PAD, e->work.d_kcnt.p, e->st);
        size_t tmp = 0;
        CHK(e->work.d_kpos_rel.ensure(n_tx + 1));
        HIPCHK(rocprim::exclusive_scan(nullptr, tmp, e->work.d_kcnt.p, e->work.d_kpos_rel.p, (uint64_t)0, (size_t)n_tx + 1,
                                       rocprim::plus<uint64_t>(), e->st));
        CHK(e->work.d_tmp.ensure(tmp));
        HIPCHK(rocprim::exclusive_scan(e->work.d_tmp.p, tmp, e->work.d_kcnt.p, e->work.d_kpos_rel.p, (uint64_t)0,
                                       (size_t)n_tx + 1, rocprim::plus<uint64_t>(), e->st));
        HIPCHK(hipMemcpyAsync(&npos, e->work.d_kpos_rel.p + n_tx, sizeof(uint64_t), hipMemcpyDeviceToHost, e->st));
        CHK(wait_st(e));
        offs = e->work.d_kpos_rel.p;
    }
    CHK(ent.ensure(std::max<uint64_t>(npos, 1)));
    CHK(ent2.ensure(std::max<uint64_t>(npos, 1)));
    // without ambiguity codes the fill also counts the segment histograms of
    // the sort's global passes (sort.hip), so the sort does not read the keys
    // to count them
    const bool counted = !amb && npos > 0 && npos <= 0xFFFFFFFFull;
    // (G < 0: too many entries for ranges that fit the local sort; the 8-bit passes)
    const int G = os_index_gbits(npos, index_bits(npos, 0), e->knobs.index_cap);
    if (counted && G >= 0) {
        CHK(e->work.d_sort_scratch.ensure(os_index_scratch_words(npos)));
        os_index_fill_hist(txl, n_tx, e->work.d_F.p + FRONT_PAD, offs, ent.p, npos, G, e->work.d_sort_scratch.p, e->st);
    } else if (counted) {
        CHK(e->work.d_sort_scratch.ensure(os_scratch_words(npos)));
        os_fill_hist(txl, n_tx, e->work.d_F.p + FRONT_PAD, offs, ent.p, npos, e->work.d_sort_scratch.p, e->st);
    } else if (n_tx) {
        launch_kmer_fill(amb, txl, n_tx, e->work.d_F.p + FRONT_PAD, amb ? e->work.d_AF.p + FRONT_PAD : nullptr, offs, ent.p,
                         e->st);
    }
    // sort on the k-mer (bits 32..63); the fill order is position order and the
    // radix sort is stable, so positions stay ascending per k-mer
    CHK(sort_index(e, ent, ent2, npos, 32u, 0, bucket, bits_out, counted, G));
    n_out = npos;
    return RC_OK;
}

// The seed index of the loaded tile: every 16-mer position of its subject samples' transcripts.
static int build_index(rc_engine *e)
{
    return build_index_of(e, e->work.d_tile_itx.p, e->tile_nitx, e->tile_npos, e->work.d_kpos_off.p, e->work.d_ent,
                          e->work.d_ent2, e->work.d_bucket, e->index_bits, e->n_index);
}

// Shared searches with DUST: the reverse pass's index. A reverse search whose
// SUBJECT a holds a masked base may have seeds the forward pass does not find
// (runs none of whose aligned words of a is usable); every 16-mer of such a
// run has a masked base of a nearby, so the index holds only the positions of
// masked transcripts with a masked base in [pos - (W - 16), pos + W), W = the
// word size (near_fill_kernel), sorted on all 64 key bits, with 4 buckets per
// entry.
static int build_masked_index(rc_engine *e)
{
    const uint32_t n = e->tile_ntx;
    CHK(e->work.d_tile_masked.ensure(std::max<uint32_t>(n, 1)));
    launch_tx_masked(e->work.d_tile_tx.p, n, e->work.d_dmask.p + 1, e->work.d_tile_masked.p, e->st);
    HIPCHK(hipGetLastError());
    CHK(e->work.d_rctr.ensure(4));
    if (!e->work.mnear_cap) e->work.mnear_cap = e->tile_total / 32 + (1u << 20);
    unsigned long long cnt = 0;
    for (;;) {
        CHK(e->work.d_ment.ensure(e->work.mnear_cap));
        CHK(e->work.d_ment2.ensure(e->work.mnear_cap));
        HIPCHK(hipMemsetAsync(e->work.d_rctr.p, 0, sizeof(unsigned long long), e->st));
        launch_near_fill(e->has_amb, e->work.d_tile_tx.p, n, e->work.d_tile_masked.p, e->work.d_F.p + FRONT_PAD,
                         e->has_amb ? e->work.d_AF.p + FRONT_PAD : nullptr, e->work.d_dmask.p + 1, e->work.d_ment.p,
                         e->work.mnear_cap, e->work.d_rctr.p, e->o.word_size, e->st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&cnt, e->work.d_rctr.p, sizeof cnt, hipMemcpyDeviceToHost, e->st));
        CHK(wait_st(e));
        if (cnt <= e->work.mnear_cap) break;
        e->work.mnear_cap = cnt + cnt / 4 + (1u << 20);
    }
    CHK(sort_index(e, e->work.d_ment, e->work.d_ment2, cnt, 0u, 2, e->work.d_mbucket, e->mindex_bits));
    e->n_mindex = cnt;
    e->tm.near_index += (double)cnt;
    return RC_OK;
}

// Genes of [g0, g1) with more than ISO_LDS isoforms (the seed kernel's ISOG
// launch), appended to `list`; returns their count
static uint32_t iso_genes(const rc_engine *e, uint32_t g0, uint32_t g1, std::vector<uint32_t> &list)
{
    uint32_t n = 0;
    for (uint32_t g = g0; g < g1; g++)
        if (e->gene_tx_off[g + 1] - e->gene_tx_off[g] > (uint32_t)ISO_LDS) {
            list.push_back(g);
            n++;
        }
    return n;
}

static Db make_db(rc_engine *e)
{
    Db db;
    db.F = e->work.d_F.p + FRONT_PAD;
    db.RC = e->work.d_RC.p + FRONT_PAD;
    db.AF = e->has_amb ? e->work.d_AF.p + FRONT_PAD : nullptr;
    db.ARC = e->has_amb ? e->work.d_ARC.p + FRONT_PAD : nullptr;
    db.total = e->tile_total;
    db.tx = e->d_tx.p;
    db.tx_gene = e->d_tx_gene.p;
    db.gene_tx_off = e->d_gene_tx_off.p;
    db.gene_tx = e->d_gene_tx.p;
    db.giso = e->d_giso.p;
    db.gene_sample = e->d_gene_sample.p;
    db.sample_gene_begin = e->d_sample_gene_begin.p;
    db.sample_tx_begin = e->d_sample_tx_begin.p;
    db.sample_pos_begin = e->work.d_sample_pos.p;
    db.txstart = e->work.d_txstart.p + 1;
    db.dmask = e->o.dust_level > 0 ? e->work.d_dmask.p + 1 : nullptr;
    db.n_samples = (int32_t)e->samples.size();
    return db;
}

static void shard_pairs(rc_engine *e)
{
    e->pair0 = (uint64_t)e->shard_first[e->o.shard_rank];
    e->pair1 = (uint64_t)e->shard_first[e->o.shard_rank + 1];
    e->item0 = e->pair_item_begin[e->pair0];
    e->item1 = e->pair_item_begin[e->pair1];
}

// The directed searches of tile ti: per query sample the bit set of its
// subject samples (spec 5b: only a -> b of a pair), and the runs of
// consecutive query samples (one seed launch each: their genes are contiguous).
// Subject-sample bit rows (tmw words per query sample) and the range of
// each row's set bits ([first, one past last), empty N, 0).
static int mask_words(int N) { return (N + 63) / 64; }
static void mask_ranges(const std::vector<uint64_t> &mask, int N, std::vector<int32_t> &range)
{
    const int tw = mask_words(N);
    range.assign((size_t)2 * N, 0);
    for (int q = 0; q < N; q++) {
        int lo = N, hi = 0;
        for (int w = 0; w < tw; w++) {
            const uint64_t m = mask[(size_t)q * tw + w];
            if (!m) continue;
            lo = std::min(lo, 64 * w + __builtin_ctzll(m));
            hi = std::max(hi, 64 * w + 64 - __builtin_clzll(m));
        }
        range[2 * q] = lo;
        range[2 * q + 1] = hi;
    }
}

static void tile_plan(rc_engine *e, int ti, std::vector<uint64_t> &tmask, std::vector<std::pair<int, int>> &runs)
{
    const int N = (int)e->samples.size(), tw = mask_words(N);
    tmask.assign((size_t)tw * N, 0);
    std::vector<char> q(N, 0);
    for (auto &pr : e->tiles[ti].pairs) {
        const int a = pr.first, b = pr.second;
        tmask[(size_t)tw * a + (b >> 6)] |= 1ull << (b & 63);
        q[a] = 1;
        if (!e->o.symmetric && !e->share) {   // the pair's second directed search: query b, subject a
            tmask[(size_t)tw * b + (a >> 6)] |= 1ull << (a & 63);
            q[b] = 1;
        }
    }
    runs.clear();
    for (int s = 0; s < N;) {
        if (!q[s]) {
            s++;
            continue;
        }
        int t = s;
        while (t < N && q[t]) t++;
        runs.push_back({s, t});
        s = t;
    }
}

// The reverse pass of shared searches with DUST: queries = the
// higher sample of each pair of tile ti, subjects = the near-mask index ixm.
// It keeps only the reverse-search runs the forward pass cannot see, as SEED_R
// seeds in forward-candidate coordinates; they are sorted by the forward
// query's gene (rs_key, rs_idx) for the forward pass to merge. n_rs = count.
static int reverse_pass(rc_engine *e, int ti, const Db &db, const Index &ixm, uint32_t &n_rs)
{
    const int N = (int)e->samples.size(), tw = mask_words(N);
    std::vector<uint64_t> rmask((size_t)tw * N, 0);
    std::vector<char> q(N, 0);
    for (auto &pr : e->tiles[ti].pairs) {
        rmask[(size_t)tw * pr.second + (pr.first >> 6)] |= 1ull << (pr.first & 63);
        q[pr.second] = 1;
    }
    std::vector<std::pair<int, int>> runs;
    for (int s0 = 0; s0 < N;) {
        if (!q[s0]) {
            s0++;
            continue;
        }
        int t = s0;
        while (t < N && q[t]) t++;
        runs.push_back({s0, t});
        s0 = t;
    }
    std::vector<int32_t> rrange;
    mask_ranges(rmask, N, rrange);
    CHK(e->work.d_rtmask.ensure(rmask.size()));
    CHK(e->work.d_rtrange.ensure(rrange.size()));
    HIPCHK(hipMemcpyAsync(e->work.d_rtmask.p, rmask.data(), rmask.size() * 8, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemcpyAsync(e->work.d_rtrange.p, rrange.data(), rrange.size() * 4, hipMemcpyHostToDevice, e->st));
    std::vector<uint32_t> ilist, ioff(1, 0);
    for (auto &r : runs) ioff.push_back(ioff.back() + iso_genes(e, e->sample_gene_begin[r.first],
                                                                 e->sample_gene_begin[r.second], ilist));
    CHK(e->d_iso_list_r.ensure(std::max<size_t>(ilist.size(), 1)));
    if (!ilist.empty())
        HIPCHK(hipMemcpyAsync(e->d_iso_list_r.p, ilist.data(), ilist.size() * 4, hipMemcpyHostToDevice, e->st));
    CHK(e->work.d_rctr.ensure(4));
    CHK(e->work.d_big_out.ensure(std::max<uint64_t>(e->big_list_cap, 1)));
    if (!e->rseed_cap) e->rseed_cap = 1u << 20;
    unsigned long long cnt = 0;
    for (;;) {
        CHK(e->work.d_rseeds.ensure(e->rseed_cap));
        CHK(e->work.d_rseed_gene.ensure(e->rseed_cap));
        HIPCHK(hipMemsetAsync(e->work.d_rctr.p + 1, 0, 2 * sizeof(unsigned long long), e->st));
        HIPCHK(hipMemsetAsync(e->d_status.p, 0, 4 * sizeof(unsigned int), e->st));
        for (size_t ri = 0; ri < runs.size(); ri++) {
            const auto &r = runs[ri];
            SeedParams S{};
            S.iso_list = e->d_iso_list_r.p + ioff[ri];
            S.iso_n = ioff[ri + 1] - ioff[ri];
            S.word = e->o.word_size;
            S.stride = e->o.word_size - W16 + 1;
            S.rev = 1;
            S.tx_pos = e->d_tx_pos.p;
            S.iso_pre_g = e->d_iso_pre.p;
            S.rseeds = e->work.d_rseeds.p;
            S.rseed_gene = e->work.d_rseed_gene.p;
            S.rseed_cap = e->rseed_cap;
            S.rseed_n = e->work.d_rctr.p + 1;
            S.gene_begin = e->sample_gene_begin[r.first];
            S.gene_end = e->sample_gene_begin[r.second];
            S.tmask = e->work.d_rtmask.p;
            S.tmw = tw;
            S.trange = e->work.d_rtrange.p;
            S.xbits = e->xbits;
            S.max_iso = max_iso(e->xbits);
            S.status = e->d_status.p;
            S.big_out = e->work.d_big_out.p;   // (never used: the pass keeps no seeds of its own)
            S.big_n = e->work.d_rctr.p + 2;
            S.big_list_cap = 0;
            launch_seed(e->has_amb, db, ixm, S, e->st);
            HIPCHK(hipGetLastError());
        }
        unsigned int status = 0;
        HIPCHK(hipMemcpyAsync(&cnt, e->work.d_rctr.p + 1, sizeof cnt, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(&status, e->d_status.p, sizeof status, hipMemcpyDeviceToHost, e->st));
        CHK(wait_st(e));
        if (status & ST_GENE_LIMIT)
            return fail(RC_E_LIMIT, "a query gene has more than " + std::to_string(max_iso(e->xbits)) + " isoforms");
        if (cnt <= e->rseed_cap) break;
        e->rseed_cap = cnt + cnt / 4 + 1024;
    }
    if (cnt > 0xFFFFFFFFull) return fail(RC_E_LIMIT, "more than 2^32 reverse-only seeds in a tile");
    n_rs = (uint32_t)cnt;
    e->n_rseeds += cnt;
    e->tm.reverse_seeds += (double)cnt;
    if (cnt) {
        CHK(e->work.d_rs_key.ensure(cnt));
        CHK(e->work.d_rs_idx.ensure(cnt));
        size_t tmp = 0;
        rocprim::counting_iterator<uint32_t> iota(0u);
        HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp, e->work.d_rseed_gene.p, e->work.d_rs_key.p, iota, e->work.d_rs_idx.p,
                                         (size_t)cnt, 0u, 32u, e->st));
        CHK(e->work.d_tmp.ensure(tmp));
        HIPCHK(rocprim::radix_sort_pairs(e->work.d_tmp.p, tmp, e->work.d_rseed_gene.p, e->work.d_rs_key.p, iota,
                                         e->work.d_rs_idx.p, (size_t)cnt, 0u, 32u, e->st));
    }
    return RC_OK;
}

static int load_external(rc_engine *e)
{
    const int N = (int)e->samples.size();
    const uint32_t n_genes = (uint32_t)e->gene_sample.size();
    std::vector<std::vector<DHsp>> grp((size_t)n_genes * N);
    for (auto &kv : e->ext) {
        const int q = kv.first.first, s = kv.first.second;
        for (const rc_hsp &h : kv.second) {
            DHsp d;
            d.q_tx = e->samples[q].tx_begin + h.q_tx;
            d.s_tx = e->samples[s].tx_begin + h.s_tx;
            d.qstart = h.qstart; d.qend = h.qend; d.sstart = h.sstart; d.send = h.send;
            d.length = h.length; d.nident = h.nident; d.mismatch = h.mismatch; d.gaps = h.gaps;
            d.gapopen = h.gapopen; d.score_half = h.score_half; d.bits10 = h.bits10; d.strand = h.strand;
            grp[grp_index(e->tx_gene[d.q_tx], s, n_genes)].push_back(d);
        }
    }
    std::vector<DHsp> all;
    std::vector<uint32_t> off(grp.size()), cnt(grp.size());
    for (size_t i = 0; i < grp.size(); i++) {
        off[i] = (uint32_t)all.size();
        cnt[i] = (uint32_t)grp[i].size();
        all.insert(all.end(), grp[i].begin(), grp[i].end());
    }
    CHK(e->d_hsp.ensure(all.size()));
    CHK(e->d_grp_off.ensure(off.size()));
    CHK(e->d_grp_cnt.ensure(cnt.size()));
    if (!all.empty()) HIPCHK(hipMemcpyAsync(e->d_hsp.p, all.data(), all.size() * sizeof(DHsp), hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemcpyAsync(e->d_grp_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemcpyAsync(e->d_grp_cnt.p, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    e->n_hsps = all.size();
    return RC_OK;
}

// d_hsp grows across tiles with its contents kept
static int grow_hsp(rc_engine *e, uint64_t n)
{
    if (n <= e->d_hsp.cap && e->d_hsp.p) return RC_OK;
    const size_t cap = std::max<size_t>(n, e->d_hsp.cap + e->d_hsp.cap / 2);
    DHsp *np = nullptr;
    if (hipMalloc((void **)&np, cap * sizeof(DHsp)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(RC_E_NOMEM, "hipMalloc of " + std::to_string(cap * sizeof(DHsp)) + " bytes failed");
    }
    if (e->hsp_used) HIPCHK(hipMemcpyAsync(np, e->d_hsp.p, e->hsp_used * sizeof(DHsp), hipMemcpyDeviceToDevice, e->st));
    CHK(wait_st(e));
    e->d_hsp.adopt(np, cap);
    return RC_OK;
}

// The loaded tile's packed working copy (FRONT_PAD zero words in front, zero
// words behind); EV_PACK0 marks the start of the packing.
static int pack_tile(rc_engine *e)
{
    const uint64_t total = e->tile_total;
    const uint64_t nwords = (total + 31) / 32 + 2;
    CHK(e->work.d_F.ensure(nwords + 4 + FRONT_PAD));
    CHK(e->work.d_RC.ensure(nwords + 4 + FRONT_PAD));
    HIPCHK(hipMemsetAsync(e->work.d_F.p, 0, FRONT_PAD * 8, e->st));
    HIPCHK(hipMemsetAsync(e->work.d_RC.p, 0, FRONT_PAD * 8, e->st));
    HIPCHK(hipMemsetAsync(e->work.d_F.p + FRONT_PAD + nwords, 0, 4 * 8, e->st));
    HIPCHK(hipMemsetAsync(e->work.d_RC.p + FRONT_PAD + nwords, 0, 4 * 8, e->st));
    if (e->has_amb) {
        CHK(e->work.d_AF.ensure(nwords + 4 + FRONT_PAD));
        CHK(e->work.d_ARC.ensure(nwords + 4 + FRONT_PAD));
        HIPCHK(hipMemsetAsync(e->work.d_AF.p, 0, (nwords + 4 + FRONT_PAD) * 8, e->st));
        HIPCHK(hipMemsetAsync(e->work.d_ARC.p, 0, (nwords + 4 + FRONT_PAD) * 8, e->st));
    }
    HIPCHK(hipEventRecord(e->ev[EV_PACK0], e->st));
    launch_pack(e->tile_direct ? e->d_ascii.p : e->work.d_tile_ascii.p, total, nwords, e->work.d_F.p + FRONT_PAD,
                e->work.d_RC.p + FRONT_PAD, e->has_amb ? e->work.d_AF.p + FRONT_PAD : nullptr,
                e->has_amb ? e->work.d_ARC.p + FRONT_PAD : nullptr, e->st);
    HIPCHK(hipGetLastError());
    return RC_OK;
}

// DUST masks of the given tile samples (ascending) into d_dmask, on stream st:
// one launch per run of consecutive samples (the transcripts' ranges only,
// not the padding between a split tile's parts)
static int dust_samples(rc_engine *e, const std::vector<int> &ss, hipStream_t st)
{
    const uint32_t dblocks = 256 * 28;   // at least the resident waves of the chunk kernel (<= 7 per SIMD): their scratch
    CHK(e->work.d_dust_scratch.ensure(dust_scratch_words(dblocks)));
    CHK(e->work.d_dust_events.ensure(dust_event_words(dblocks)));
    int f = -1, l = -1;
    auto flush = [&]() {
        if (f >= 0) {
            const uint32_t tx0 = e->tile_tx_first[f];
            launch_dust(e->has_amb, e->tile_pos[f], e->tile_pos[l] + align_up(e->samples[l].nbases),
                        e->work.d_F.p + FRONT_PAD, e->has_amb ? e->work.d_AF.p + FRONT_PAD : nullptr, e->work.d_txstart.p + 1,
                        e->work.d_tile_tx.p + tx0, e->tile_tx_first[l + 1] - tx0, e->o.dust_level, e->o.dust_window,
                        e->o.dust_linker, e->work.d_dust_scratch.p, e->work.d_dust_events.p, dblocks, e->work.d_dmask.p + 1,
                        st);
        }
        f = l = -1;
    };
    for (int s : ss) {
        if (f >= 0 && e->tile_pos[s] != e->tile_pos[l] + align_up(e->samples[l].nbases)) flush();
        if (f < 0) f = s;
        l = s;
    }
    flush();
    HIPCHK(hipGetLastError());
    return RC_OK;
}

// ------------------------------------------------------------------------
// one alignment pass over a tile (align_tile): its stages, in order
// ------------------------------------------------------------------------

// What the stages share
struct TileCtx {
    int ti = 0;
    std::vector<std::pair<int, int>> runs;   // runs of consecutive query samples: one seed launch each
    std::vector<uint32_t> rg0, rg1;          // per run: its genes [rg0, rg1)
    std::vector<uint32_t> ioff;              // ... its slice of d_iso_list
    std::vector<size_t> gcb, cnb;            // ... its slice of the (gene, sample) arrays, of the group counts
    int tw = 0;                              // mask words per query sample
    Db db{};
    Index ix{}, ixm{};                       // the tile's seed index; the reverse pass's (masked transcripts only)
    uint32_t n_rs = 0;                       // reverse-only seeds (reverse_pass)
    uint64_t n_cand = 0;
    bool later_on = false;                   // the later-seed rounds ran: lat holds their parameters
    LaterParams lat{};
};

// Stage 1: the tile's tables and packed copy, DUST masks (on the second
// stream), the seed index (built, or the previous tile's) and, for shared
// searches with DUST, the near-mask index. Events EV_PACK0, EV_INDEX0, EV_ALIGN0.
static int index_stage(rc_engine *e, int ti)
{
    {
        const double t0 = wall_ms();
        CHK(load_tile(e, ti));
        e->tm.load_ms += wall_ms() - t0;
    }
    const uint64_t total = e->tile_total;
    CHK(pack_tile(e));
    const bool dust = e->o.dust_level > 0;
    // a split tile of the b chunk the previous tile had: its 16-mer index
    // (the b part's) and the b part's DUST masks are on the device already
    const rc_engine::Tile &TT = e->tiles[ti];
    // (only while the index holds the b part alone: with one directed search
    // at a time -- RC_SHARE=0, not spec 5b -- it holds the a part's samples
    // too, and they differ from tile to tile)
    const bool b_only_index = e->share || e->o.symmetric;
    const bool reuse = b_only_index && TT.bchunk >= 0 && TT.bchunk == e->work.idx_bchunk && TT.bstart == e->work.idx_bstart &&
                       e->work.d_dmask.cap >= (total >> 6) + 4;
    const uint64_t dtot = reuse ? TT.bstart : total;   // masks cleared: the a part only when reusing
    // the samples whose masks DUST computes here, in tile order: a split
    // tile's a part and (unless its masks are kept) its b part, all samples
    // of any other tile -- except those given by rc_set_dust_masks, whose
    // masks are copied in (samples start at 256-base boundaries: whole words)
    std::vector<int> dust_here;
    e->dmask_only.clear();   // every sample of this tile gets its mask
    if (dust) {
        const size_t mw = (total >> 6) + 4;
        CHK(e->work.d_dmask.ensure(mw));
        HIPCHK(hipMemsetAsync(e->work.d_dmask.p, 0, (reuse ? 1 + (dtot >> 6) : mw) * 8, e->st));
        for (int s : TT.samples) {
            if (reuse && e->tile_pos[s] >= TT.bstart) continue;
            const uint64_t io = s < (int)e->dust_imp_off.size() ? e->dust_imp_off[s] : ~0ull;
            if (io == ~0ull) {
                dust_here.push_back(s);
            } else if (e->samples[s].nbases) {
                HIPCHK(hipMemcpyAsync(e->work.d_dmask.p + 1 + (e->tile_pos[s] >> 6), e->d_dust_imp.p + io,
                                      ((e->samples[s].nbases + 63) >> 6) * 8, hipMemcpyDeviceToDevice, e->st));
            }
        }
    }
    HIPCHK(hipEventRecord(e->ev[EV_INDEX0], e->st));
    // DUST masks of the tile's transcripts (the query side), bit per base, on
    // the second stream: a compute-bound scan beside the HBM-bound index
    // build, started with the fill (r03, hand-written sort and DUST: index
    // phase 55.7 vs 58.1 ms at C3 when started after the sort's table kernels)
    if (dust) {
        HIPCHK(hipEventRecord(e->evd[EVD_READY], e->st));
        HIPCHK(hipStreamWaitEvent(e->st2, e->evd[EVD_READY], 0));
        HIPCHK(hipEventRecord(e->evd[EVD_DUST0], e->st2));
        CHK(dust_samples(e, dust_here, e->st2));
        HIPCHK(hipEventRecord(e->evd[EVD_DUST1], e->st2));
    }
    if (reuse)
        e->tm.index_reused += 1.0;
    else
        CHK(build_index(e));
    e->work.idx_bchunk = TT.bchunk;
    e->work.idx_bstart = TT.bstart;
    HIPCHK(hipGetLastError());
    if (dust) HIPCHK(hipStreamWaitEvent(e->st, e->evd[EVD_DUST1], 0));
    // shared searches with DUST: reverse-search runs with no usable word of
    // the forward query inside come from a reverse pass over a near-mask index
    if (e->share && dust) CHK(build_masked_index(e));
    HIPCHK(hipEventRecord(e->ev[EV_ALIGN0], e->st));
    return RC_OK;
}

// Stage 2: the tile's directed searches as runs of query samples, their
// tables on the device, first guesses of the seed / candidate / HSP-overflow
// capacities, and the kernels' views of the tile (db, ix, ixm)
static int plan_stage(rc_engine *e, TileCtx &C)
{
    const int N = (int)e->samples.size();
    std::vector<uint64_t> tmask;
    auto &runs = C.runs;
    tile_plan(e, C.ti, tmask, runs);
    const size_t R = runs.size();
    const int tw = C.tw = mask_words(N);
    std::vector<int32_t> trange;
    mask_ranges(tmask, N, trange);
    CHK(e->work.d_tmask.ensure(tmask.size()));
    CHK(e->work.d_trange.ensure(trange.size()));
    HIPCHK(hipMemcpyAsync(e->work.d_tmask.p, tmask.data(), tmask.size() * 8, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemcpyAsync(e->work.d_trange.p, trange.data(), trange.size() * 4, hipMemcpyHostToDevice, e->st));
    std::vector<uint32_t> ilist;
    C.rg0.assign(R, 0);
    C.rg1.assign(R, 0);
    C.ioff.assign(1, 0);
    C.gcb.assign(R + 1, 0);
    C.cnb.assign(R + 1, 0);
    for (size_t r = 0; r < R; r++) {
        C.rg0[r] = e->sample_gene_begin[runs[r].first];
        C.rg1[r] = e->sample_gene_begin[runs[r].second];
        C.gcb[r + 1] = C.gcb[r] + (size_t)(C.rg1[r] - C.rg0[r]) * N;
        C.cnb[r + 1] = C.cnb[r] + (size_t)(C.rg1[r] - C.rg0[r]) * N + 1;
        C.ioff.push_back(C.ioff.back() + iso_genes(e, C.rg0[r], C.rg1[r], ilist));
    }
    CHK(e->d_iso_list.ensure(std::max<size_t>(ilist.size(), 1)));
    if (!ilist.empty())
        HIPCHK(hipMemcpyAsync(e->d_iso_list.p, ilist.data(), ilist.size() * 4, hipMemcpyHostToDevice, e->st));
    CHK(e->work.d_gc_off.ensure(std::max<size_t>(C.gcb[R], 1)));
    CHK(e->work.d_gc_cnt.ensure(std::max<size_t>(C.gcb[R], 1)));
    CHK(e->work.d_gcount.ensure(std::max<size_t>(C.cnb[R], 1)));
    CHK(e->work.d_gscan.ensure(std::max<size_t>(C.cnb[R], 1)));
    CHK(e->d_shard_cnt.ensure(2 * NSHARD));
    CHK(e->d_shard_prefix.ensure(NSHARD + 1));
    {
        // (query gene, subject sample) searches of the tile
        uint64_t nb = 1;
        for (size_t r = 0; r < R; r++)
            for (int q = runs[r].first; q < runs[r].second; q++) {
                uint64_t ns = 0;
                for (int w = 0; w < tw; w++) ns += (uint64_t)__builtin_popcountll(tmask[(size_t)tw * q + w]);
                nb += (uint64_t)(e->sample_gene_begin[q + 1] - e->sample_gene_begin[q]) * ns;
            }
        e->seed_cap = std::max<uint64_t>(e->seed_cap, nb * 16 / NSHARD + 4096);
        e->cand_cap = std::max<uint64_t>(e->cand_cap, nb * 2 / NSHARD + 1024);
        // (RC_OVF_CAP0: a smaller first guess, for tests of the overflow retry)
        const int oc = e->knobs.ovf_cap0;
        e->ovf_cap = std::max<uint64_t>(e->ovf_cap, oc ? (uint64_t)oc : nb / 4 + 1024);
    }
    C.db = make_db(e);
    C.ix.ent = e->work.d_ent2.p;
    C.ix.bucket = e->work.d_bucket.p;
    C.ix.pos_tx = e->work.d_pos_tx.p;
    C.ix.bits = e->index_bits;
    C.ixm = C.ix;
    C.ixm.ent = e->work.d_ment2.p;
    C.ixm.bucket = e->work.d_mbucket.p;
    C.ixm.bits = e->mindex_bits;
    CHK(e->d_count.ensure(DC_N));
    return RC_OK;
}

// The nb (gene, sample) passes of run S (listed in d_big_out) whose seeds
// overflow LDS: global-memory passes, at most BIG_CHUNK workgroups per
// launch; entries that overflow big_cap too are rerun with twice the scratch.
// again: the seed or candidate buffers overflowed.
static int seed_big_passes(rc_engine *e, const TileCtx &C, const SeedParams &S, unsigned long long nb, bool &again)
{
    const uint64_t BIG_CHUNK = 2048;
    unsigned long long *const big_retry_n = e->d_count.p + DC_BIG_RETRY;
    uint64_t *list = e->work.d_big_out.p;
    while (!again && nb) {
        if ((uint64_t)e->big_cap > (1ull << 22))
            return fail(RC_E_LIMIT, "a (query gene, subject sample) pass has more than 2^22 seeds");
        const uint64_t chunk = std::min<uint64_t>(nb, BIG_CHUNK);
        CHK(e->work.d_big_list.ensure(nb));
        CHK(e->work.d_big_retry.ensure(nb));
        CHK(e->work.d_big_seeds.ensure(chunk * e->big_cap));
        CHK(e->work.d_big_seg.ensure(chunk * (e->big_cap + 1)));
        CHK(e->work.d_big_segT.ensure(chunk * e->big_cap));
        if (list != e->work.d_big_list.p)
            HIPCHK(hipMemcpyAsync(e->work.d_big_list.p, list, nb * 8, hipMemcpyDeviceToDevice, e->st));
        HIPCHK(hipMemsetAsync(big_retry_n, 0, sizeof(unsigned long long), e->st));
        SeedParams B = S;
        B.big_retry = e->work.d_big_retry.p;
        B.big_list_cap = nb;
        B.big_cap = e->big_cap;
        B.big_seeds = e->work.d_big_seeds.p;
        B.big_seg = e->work.d_big_seg.p;
        B.big_segT = e->work.d_big_segT.p;
        for (uint64_t c0 = 0; c0 < nb; c0 += chunk) {
            B.big_list = e->work.d_big_list.p + c0;
            launch_seed_big(e->has_amb, C.db, C.ix, B, (uint32_t)std::min<uint64_t>(chunk, nb - c0), e->st);
            HIPCHK(hipGetLastError());
        }
        unsigned int status = 0;
        unsigned long long nr = 0;
        HIPCHK(hipMemcpyAsync(&status, e->d_status.p, sizeof status, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(&nr, big_retry_n, sizeof nr, hipMemcpyDeviceToHost, e->st));
        CHK(wait_st(e));
        if (status & ST_SEED_INDEX)
            return fail(RC_E_LIMIT, "a candidate's first seed of a directed search is past seed 65534");
        again = (status & ST_OVERFLOW) != 0;
        nb = nr;
        // the retry entries become the next list (buffers swapped, not copied)
        e->work.d_big_list.swap(e->work.d_big_retry);
        list = e->work.d_big_list.p;
        if (nb) e->big_cap *= 2;
    }
    return RC_OK;
}

// Stage 3: seeds and candidates of every run (the reverse pass first, for
// shared searches with DUST), again with larger buffers while one overflows;
// then the candidates' shard prefix. Events EV_SEED0, EV_SEED1.
static int seed_stage(rc_engine *e, TileCtx &C)
{
    const size_t R = C.runs.size();
    std::vector<unsigned long long> shard_cnt(2 * NSHARD);
    unsigned long long *const big_n = e->d_count.p + DC_BIG;
    uint64_t n_big = 0;
    HIPCHK(hipEventRecord(e->ev[EV_SEED0], e->st));
    if (e->share && e->o.dust_level > 0 && e->n_mindex) CHK(reverse_pass(e, C.ti, C.db, C.ixm, C.n_rs));
    for (int attempt = 0;; attempt++) {
        if (attempt == 6) return fail(RC_E_NOMEM, "seed/candidate buffers kept overflowing");
        if (e->seed_cap * NSHARD > 0xFFFFFFFFull || e->cand_cap * NSHARD > 0xFFFFFFFFull)
            return fail(RC_E_LIMIT, "more than 2^32 seeds or candidates in a tile: use more shards or smaller tiles");
        CHK(e->work.d_seeds.ensure(e->seed_cap * NSHARD));
        CHK(e->work.d_cands.ensure(e->cand_cap * NSHARD));
        if (e->share) CHK(e->work.d_list2.ensure(e->cand_cap * NSHARD));
        HIPCHK(hipMemsetAsync(e->d_count.p + DC_LIST2, 0, sizeof(unsigned long long), e->st));
        CHK(e->work.d_big_out.ensure(e->big_list_cap));
        HIPCHK(hipMemsetAsync(e->d_shard_cnt.p, 0, 2 * NSHARD * sizeof(unsigned long long), e->st));
        HIPCHK(hipMemsetAsync(e->d_status.p, 0, 4 * sizeof(unsigned int), e->st));
        if (C.gcb[R]) HIPCHK(hipMemsetAsync(e->work.d_gc_cnt.p, 0, C.gcb[R] * 4, e->st));
        CHK(e->work.d_prof.ensure(10));
        HIPCHK(hipMemsetAsync(e->work.d_prof.p, 0, 10 * sizeof(unsigned long long), e->st));
        // what every run of this attempt shares
        SeedParams S0{};
        S0.word = e->o.word_size;
        S0.stride = e->o.word_size - W16 + 1;
        S0.sym = e->o.symmetric;
        S0.share = e->share ? 1 : 0;
        S0.tx_pos = e->d_tx_pos.p;
        S0.iso_pre_g = e->d_iso_pre.p;
        S0.rs_rec = e->work.d_rseeds.p;
        S0.rs_key = e->work.d_rs_key.p;
        S0.rs_idx = e->work.d_rs_idx.p;
        S0.rs_n = C.n_rs;
        S0.list2 = e->work.d_list2.p;
        S0.list2_n = e->d_count.p + DC_LIST2;
        S0.seeds = e->work.d_seeds.p;
        S0.seed_cap = e->seed_cap;
        S0.seed_count = e->d_shard_cnt.p;
        S0.cands = e->work.d_cands.p;
        S0.cand_cap = e->cand_cap;
        S0.cand_count = e->d_shard_cnt.p + NSHARD;
        S0.tmask = e->work.d_tmask.p;
        S0.tmw = C.tw;
        S0.trange = e->work.d_trange.p;
        S0.xbits = e->xbits;
        S0.max_iso = max_iso(e->xbits);
        S0.status = e->d_status.p;
        S0.big_out = e->work.d_big_out.p;
        S0.big_n = big_n;
        S0.big_retry_n = e->d_count.p + DC_BIG_RETRY;
        S0.big_list_cap = e->big_list_cap;
        S0.prof = e->work.d_prof.p;
        bool again = false;
        n_big = 0;
        for (size_t r = 0; r < R && !again; r++) {
            // (DC_BIG and DC_BIG_RETRY)
            HIPCHK(hipMemsetAsync(big_n, 0, (DC_LIST2 - DC_BIG) * sizeof(unsigned long long), e->st));
            SeedParams S = S0;
            S.gene_begin = C.rg0[r];
            S.gene_end = C.rg1[r];
            if (C.n_rs) {
                CHK(e->work.d_rs_range.ensure((size_t)2 * (C.rg1[r] - C.rg0[r]) + 2));
                launch_rs_range(e->work.d_rs_key.p, C.n_rs, C.rg0[r], C.rg1[r], e->work.d_rs_range.p, e->st);
                S.rs_range = e->work.d_rs_range.p;
            }
            S.iso_list = e->d_iso_list.p + C.ioff[r];
            S.iso_n = C.ioff[r + 1] - C.ioff[r];
            S.gc_off = e->work.d_gc_off.p + C.gcb[r];
            S.gc_cnt = e->work.d_gc_cnt.p + C.gcb[r];
            launch_seed(e->has_amb, C.db, C.ix, S, e->st);
            HIPCHK(hipGetLastError());
            unsigned int status = 0;
            unsigned long long nb = 0;
            HIPCHK(hipMemcpyAsync(&status, e->d_status.p, sizeof status, hipMemcpyDeviceToHost, e->st));
            HIPCHK(hipMemcpyAsync(&nb, big_n, sizeof nb, hipMemcpyDeviceToHost, e->st));
            CHK(wait_st(e));
            if (status & ST_GENE_LIMIT)
                return fail(RC_E_LIMIT, "a query gene has more than " + std::to_string(max_iso(e->xbits)) + " isoforms");
            if (status & ST_SEED_INDEX)
                return fail(RC_E_LIMIT, "a candidate's first seed of a directed search is past seed 65534");
            if (status & ST_BIG_LIST_FULL) {   // the big-pass list itself overflowed
                e->big_list_cap = std::max<uint64_t>(4 * e->big_list_cap, nb + 1024);
                again = true;
                break;
            }
            again = (status & ST_OVERFLOW) != 0;
            n_big += nb;
            CHK(seed_big_passes(e, C, S, nb, again));
        }
        HIPCHK(hipEventRecord(e->ev[EV_SEED1], e->st));
        HIPCHK(hipMemcpyAsync(shard_cnt.data(), e->d_shard_cnt.p, 2 * NSHARD * 8, hipMemcpyDeviceToHost, e->st));
        CHK(wait_st(e));
        if (!again) break;
        uint64_t ms = 0, mc = 0;
        for (int i = 0; i < NSHARD; i++) {
            ms = std::max<uint64_t>(ms, shard_cnt[i]);
            mc = std::max<uint64_t>(mc, shard_cnt[NSHARD + i]);
        }
        e->seed_cap = std::max<uint64_t>(e->seed_cap, ms * 5 / 4 + 4096);
        e->cand_cap = std::max<uint64_t>(e->cand_cap, mc * 5 / 4 + 1024);
    }
    e->tm.big_passes += (double)n_big;
    std::vector<unsigned long long> prefix(NSHARD + 1, 0);
    for (int i = 0; i < NSHARD; i++) prefix[i + 1] = prefix[i] + shard_cnt[NSHARD + i];
    C.n_cand = prefix[NSHARD];
    for (int i = 0; i < NSHARD; i++) e->n_seeds += shard_cnt[i];
    e->n_cands += C.n_cand;
    HIPCHK(hipMemcpyAsync(e->d_shard_prefix.p, prefix.data(), (NSHARD + 1) * 8, hipMemcpyHostToDevice, e->st));
    return RC_OK;
}

// The extension kernels' parameters from the engine's buffers (as sized now)
static ExtParams ext_params(const rc_engine *e, const TileCtx &C)
{
    unsigned long long *const cnt = e->d_count.p;
    ExtParams X{};
    X.xdrop = e->o.xdrop_half;
    X.sym = e->o.symmetric;
    X.max_len = e->max_len;
    X.thr = e->d_thr.p;
    X.bits10 = e->d_bits10.p;
    X.cands = e->work.d_cands.p;
    X.seeds = e->work.d_seeds.p;
    X.shard_prefix = e->d_shard_prefix.p;
    X.n_cand = C.n_cand;
    X.cand_cap = e->cand_cap;
    X.cand_hsp = e->work.d_cand_hsp.p;
    X.cand_nh = e->work.d_cand_nh.p;
    X.cand_ovf = e->work.d_cand_ovf.p;
    X.ovf = e->work.d_ovf.p;
    X.ovf_cap = e->ovf_cap;
    X.ovf_count = cnt + DC_OVF;
    X.status = e->d_status.p;
    X.counters = cnt + DC_COUNTERS;
    {
        // row staging slot (u64 words): whole transcripts when the longest
        // fits the slot the 32-lane kernel has at full occupancy, else
        // windows of that slot (the windowed instantiation). RC_WIN_WORDS
        // forces windows of that many words (tests: many refills).
        const int need = ((e->max_len + 31) >> 5) + 4;
        const int smax = row_slot_words_max(e->has_amb);
        const int forced = e->knobs.win_words;
        X.win = forced ? 1 : (need > smax ? 1 : 0);
        X.dsw = forced ? std::min(forced, smax) : std::min(need, smax);
    }
    X.defer = e->work.d_defer.p;
    X.defer_count = cnt + DC_DEFER;
    X.work = cnt + DC_WORK;
    X.cand_box = e->work.d_cand_box.p;
    X.share = e->share ? 1 : 0;
    X.which = 0;
    X.dir = 0;
    X.cand_box2 = e->work.d_cand_box2.p;
    X.cand_hsp_r = e->work.d_cand_hsp_r.p;
    X.cand_nh_r = e->work.d_cand_nh_r.p;
    X.cand_ovf_r = e->work.d_cand_ovf_r.p;
    X.defer_r = e->work.d_defer_r.p;
    X.defer_r_count = cnt + DC_DEFER_R;
    X.list2 = e->work.d_list2.p;
    X.list2_n = cnt + DC_LIST2;
    X.work3 = cnt + DC_WORK3;
    X.wide0 = e->share ? e->work.d_wide0.p : nullptr;
    X.wide1 = e->work.d_wide1.p;
    X.wide0_n = cnt + DC_WIDE0;
    X.wide1_n = cnt + DC_WIDE1;
    {
        // save overflowing extensions for the 64-lane pass when the last
        // run had many (C3v: 39 %, C3: 0.002 %): the saving kernel costs
        // the plain one 7 % (RC_RESUME=1 always, 0 never)
        const bool on = e->knobs.resume != -1 ? e->knobs.resume == 1 : e->ovf_frac > 0.02;
        X.resume = e->work.res_cap && on ? e->work.d_resume.p : nullptr;
        X.res_cap = e->work.res_cap;
    }
    X.work_w0 = cnt + DC_WORK_W0;
    X.work_w1 = cnt + DC_WORK_W1;
    X.why = cnt + DC_WHY;
    X.chunk = 8;   // candidates per work grab of the row kernels
    return X;
}

// Later-seed rounds over the nsrch = dn0 + dn1 searches first_finish_kernel
// deferred (forward, reverse): their later seeds on the row kernels; searches
// past RC_LATER_CAP (default 24 M, 12 GB of state and work) run whole
static int later_rounds(rc_engine *e, TileCtx &C, const ExtParams &X, uint64_t dn0, uint64_t dn1)
{
    const uint64_t nsrch = dn0 + dn1, n = std::min(nsrch, e->knobs.later_cap);
    CHK(e->work.d_later.ensure(n * LATER_REC));
    CHK(e->work.d_lbox0.ensure(n * BOX_REC));
    CHK(e->work.d_lbox1.ensure(n * BOX_REC));
    CHK(e->work.d_lvc0.ensure(n));
    CHK(e->work.d_lvc1.ensure(n));
    CHK(e->work.d_llist0.ensure(n));
    CHK(e->work.d_llist1.ensure(n));
    CHK(e->work.d_lact0.ensure(n));
    CHK(e->work.d_lact1.ensure(n));
    CHK(e->work.d_lfull0.ensure(std::max<uint64_t>(dn0, 1)));
    CHK(e->work.d_lfull1.ensure(std::max<uint64_t>(dn1, 1)));
    const size_t nc = (size_t)MAX_HSP * LATER_CNT + LC_N;
    CHK(e->work.d_lcnt.ensure(nc));
    HIPCHK(hipMemsetAsync(e->work.d_lcnt.p, 0, nc * sizeof(unsigned long long), e->st));
    LaterParams &lat = C.lat;
    lat = LaterParams{};
    lat.state = e->work.d_later.p;
    lat.n_search = nsrch;
    lat.n0 = dn0;
    lat.n_cap = n;
    lat.defer0 = X.defer;
    lat.defer1 = X.defer_r;
    lat.full0 = e->work.d_lfull0.p;
    lat.full1 = e->work.d_lfull1.p;
    lat.counters = e->work.d_lcnt.p + (size_t)MAX_HSP * LATER_CNT;
    lat.full_n = lat.counters + LC_FULL_N;
    Cand *const vc[2] = {e->work.d_lvc0.p, e->work.d_lvc1.p};
    uint32_t *const ls[2] = {e->work.d_llist0.p, e->work.d_llist1.p};
    int32_t *const bx[2] = {e->work.d_lbox0.p, e->work.d_lbox1.p};
    uint32_t *const ac[2] = {e->work.d_lact0.p, e->work.d_lact1.p};
    launch_later_rounds(e->has_amb, C.db, X, e->knobs.later_rows == 32, lat, vc, ls, bx, ac, e->work.d_lcnt.p, e->st);
    HIPCHK(hipGetLastError());
    C.later_on = true;
    return RC_OK;
}

// Stage 5 (RC_ROW_TIMING builds only: their kernels count cycles): the row
// and seed kernels' cycle counters to stderr; ctr = the counters view. The
// slots past the view restart.
static int print_row_timing(rc_engine *e, const unsigned long long *ctr)
{
    unsigned long long *const cnt = e->d_count.p;
    const auto c = [&](int slot) { return (double)ctr[slot - DC_COUNTERS]; };
    unsigned long long tfs[3] = {0, 0, 0};   // fetches, window slides, extension starts (parts of the transitions)
    static_assert(DC_T_START - DC_T_FETCH == 2, "the three transition parts are adjacent");
    HIPCHK(hipMemcpy(tfs, cnt + DC_T_FETCH, sizeof tfs, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(cnt + DC_T_FETCH, 0, sizeof tfs));
    fprintf(stderr, "row kernel wave-cycles: transitions %.4g (fetches %.4g, window slides %.4g, extension "
                    "starts %.4g) steps %.4g\n",
            c(DC_T_TRANS), (double)tfs[0], (double)tfs[1], (double)tfs[2], c(DC_T_STEPS));
    // 32-lane rows: steps and candidates within a 16-lane window, its slides (profiles/r06_row16)
    unsigned long long r16[3] = {0, 0, 0};
    static_assert(DC_T_SL16 == DC_T_C16 + 1, "the two 16-lane slots are cleared together");
    HIPCHK(hipMemcpy(&r16[0], cnt + DC_T_N16, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&r16[1], cnt + DC_T_C16, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&r16[2], cnt + DC_T_SL16, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(cnt + DC_T_N16, 0, 8));
    HIPCHK(hipMemset(cnt + DC_T_C16, 0, 16));
    fprintf(stderr, "row steps before a live span over 14 diagonals %.4g of %.4g; candidates never over 14: "
                    "%.4g of %.4g; 16-lane window slides %.4g\n", (double)r16[0], c(DC_STEPS),
            (double)r16[1], c(DC_CANDS), (double)r16[2]);
    unsigned long long pr[10];
    HIPCHK(hipMemcpy(pr, e->work.d_prof.p, sizeof pr, hipMemcpyDeviceToHost));
    fprintf(stderr, "seed kernel block-cycles: prologue %.4g words: usable %.4g lookup %.4g scan %.4g "
                    "hits %.4g (loads %.4g pretest %.4g full test %.4g) sort %.4g write %.4g\n",
            (double)pr[8], (double)pr[9], (double)pr[0], (double)pr[1], (double)(pr[2] + pr[5] + pr[6] + pr[7]),
            (double)pr[5], (double)pr[6], (double)pr[7], (double)pr[3], (double)pr[4]);
    return RC_OK;
}

// Stage 4: the candidates' extensions (row kernels over first seeds, the
// later-seed rounds, extend_kernel over what they leave); extend_kernel runs
// again with a larger HSP overflow buffer while that overflows. Events
// EV_EXTEND0, EV_EXTEND1.
static int extension_stage(rc_engine *e, TileCtx &C)
{
    const uint64_t n_cand = C.n_cand, slots = e->cand_cap * NSHARD;
    unsigned long long *const cnt = e->d_count.p;
    CHK(e->work.d_cand_hsp.ensure(slots));
    CHK(e->work.d_cand_nh.ensure(slots));
    CHK(e->work.d_cand_ovf.ensure(slots));
    CHK(e->work.d_cand_box.ensure(slots * BOX_REC));
    if (e->share) {
        CHK(e->work.d_cand_box2.ensure(slots * BOX_REC));
        CHK(e->work.d_cand_hsp_r.ensure(slots));
        CHK(e->work.d_cand_nh_r.ensure(slots));
        CHK(e->work.d_cand_ovf_r.ensure(slots));
        CHK(e->work.d_defer_r.ensure(std::max<uint64_t>(n_cand, 1)));
        CHK(e->work.d_wide0.ensure(std::max<uint64_t>(n_cand, 1)));
        CHK(e->work.d_wide1.ensure(std::max<uint64_t>(n_cand, 1)));
        // room to continue the first 12 M overflowing extensions of a pass
        // (3.8 GB); later ones start over in the 64-lane pass
        e->work.res_cap = e->knobs.resume == 0 ? 0u : (uint32_t)std::min<uint64_t>(n_cand, 12u << 20);
        if (e->knobs.resume != 1 && e->ovf_frac <= 0.02) e->work.res_cap = 0;   // not needed: no buffer
        if (e->work.res_cap) CHK(e->work.d_resume.ensure((size_t)e->work.res_cap * RES_REC));
    }
    CHK(e->work.d_defer.ensure(std::max<uint64_t>(n_cand, 1)));
    // later-seed rounds: their parameters (C.lat) once they ran (a retry
    // finishes the searches again from the states, and extend_kernel takes the
    // lists of the searches they left whole instead of first_finish_kernel's)
    C.later_on = false;
    for (int attempt = 0;; attempt++) {
        if (attempt == 4) return fail(RC_E_NOMEM, "HSP overflow buffer kept overflowing");
        CHK(e->work.d_ovf.ensure(e->ovf_cap));
        if (attempt == 0) {
            // every slot the extension counts in; the seed stage's (DC_BIG,
            // DC_BIG_RETRY, DC_LIST2) and the groups' (DC_MBIG) stand
            HIPCHK(hipMemsetAsync(cnt + DC_OVF, 0, (DC_COUNTERS_END - DC_OVF) * sizeof(unsigned long long), e->st));
            HIPCHK(hipMemsetAsync(cnt + DC_DEFER_R, 0, (DC_MBIG - DC_DEFER_R) * sizeof(unsigned long long), e->st));
            HIPCHK(hipMemsetAsync(cnt + DC_WIDE0, 0, (DC_WHY_END - DC_WIDE0) * sizeof(unsigned long long), e->st));
        } else {
            // a retry redoes extend_kernel only: its overflow count restarts,
            // every other counter and list stands
            HIPCHK(hipMemsetAsync(cnt + DC_OVF, 0, sizeof(unsigned long long), e->st));
        }
        HIPCHK(hipMemsetAsync(e->d_status.p, 0, 4 * sizeof(unsigned int), e->st));
        ExtParams X = ext_params(e, C);
        if (attempt == 0) {
            HIPCHK(hipEventRecord(e->ev[EV_EXTEND0], e->st));
            launch_extend_rows(e->has_amb, C.db, X, e->st);
            HIPCHK(hipGetLastError());
            // only the searches the row kernels left (defer lists) can have
            // more than one HSP, at most MAX_HSP - 1 more each: the overflow
            // buffer at twice their count (about 1.1 more each at C3v), so a
            // first run rarely redoes extend_kernel
            unsigned long long dn[2] = {0, 0};
            HIPCHK(hipMemcpyAsync(&dn[0], X.defer_count, sizeof dn[0], hipMemcpyDeviceToHost, e->st));
            HIPCHK(hipMemcpyAsync(&dn[1], X.defer_r_count, sizeof dn[1], hipMemcpyDeviceToHost, e->st));
            CHK(wait_st(e));
            const uint64_t nd = dn[0] + dn[1];
            const uint64_t want = std::min<uint64_t>(2 * nd, (uint64_t)(MAX_HSP - 1) * nd) + 1024;
            if (want > e->ovf_cap && !e->knobs.ovf_cap0) {
                e->ovf_cap = want;
                CHK(e->work.d_ovf.ensure(e->ovf_cap));
                X.ovf = e->work.d_ovf.p;
                X.ovf_cap = e->ovf_cap;
            }
            // (RC_LATER=0: extend_kernel runs the deferred searches whole)
            if (e->share && e->knobs.later && dn[0] + dn[1]) CHK(later_rounds(e, C, X, dn[0], dn[1]));
        }
        if (C.later_on) {
            // (on a retry this counts the MAX_HSP-bound searches again, an
            // over-count of maxhsp_bound: X.counters is cleared only below)
            launch_later_finish(X, C.lat, e->st);
            X.defer = C.lat.full0;
            X.defer_count = C.lat.full_n;
            X.defer_r = C.lat.full1;
            X.defer_r_count = C.lat.full_n + 1;
        }
        if (attempt) {
            X.counters = nullptr;   // (the first attempt counted this work)
            e->tm.ext_retries += 1.0;
        }
        launch_extend_retry(e->has_amb, C.db, X, e->st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->ev[EV_EXTEND1], e->st));
        unsigned long long ovn = 0, ctr[DC_COUNTERS_END - DC_COUNTERS] = {};
        const auto c = [&](int slot) { return (double)ctr[slot - DC_COUNTERS]; };
        unsigned long long nwide[2] = {0, 0};   // shared searches: candidates the 64-lane passes took
        static_assert(DC_WIDE1 == DC_WIDE0 + 1, "read together");
        HIPCHK(hipMemcpyAsync(nwide, cnt + DC_WIDE0, sizeof nwide, hipMemcpyDeviceToHost, e->st));
        unsigned long long why[DC_WHY_END - DC_WHY] = {0, 0, 0};
        HIPCHK(hipMemcpyAsync(why, cnt + DC_WHY, sizeof why, hipMemcpyDeviceToHost, e->st));
        unsigned long long ndr = 0, nl2 = 0;   // shared searches: reverse searches redone whole, second first seeds
        HIPCHK(hipMemcpyAsync(&ndr, cnt + DC_DEFER_R, sizeof ndr, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(&nl2, cnt + DC_LIST2, sizeof nl2, hipMemcpyDeviceToHost, e->st));
        unsigned int status = 0;
        HIPCHK(hipMemcpyAsync(&ovn, cnt + DC_OVF, sizeof ovn, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(ctr, cnt + DC_COUNTERS, sizeof ctr, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(&status, e->d_status.p, sizeof status, hipMemcpyDeviceToHost, e->st));
        CHK(wait_st(e));
        if (c(DC_T_TRANS) || c(DC_T_STEPS)) CHK(print_row_timing(e, ctr));   // built with RC_ROW_TIMING
        if (!(status & ST_OVERFLOW)) {
            e->tm.ext_steps += c(DC_STEPS);
            e->tm.ext_calls += c(DC_EXTS);
            e->tm.ext_fullband += c(DC_FULLBAND);
            e->ovf_frac = n_cand ? c(DC_FULLBAND) / (double)n_cand : 0.0;
            e->tm.ext_deferred += c(DC_DEFER) + (double)ndr;
            e->tm.ext_second += e->share ? (double)nl2 : 0.0;
            e->tm.band_bound += c(DC_BAND_BOUND);
            e->tm.ext_slides += c(DC_SLIDES);
            e->tm.ext_wide += (double)(nwide[0] + nwide[1]);
            e->tm.maxhsp_bound += c(DC_MAXHSP);
            e->tm.defer_length += (double)why[0];
            e->tm.defer_gaveup += (double)why[1];
            e->tm.defer_outside += (double)why[2];
            if (C.later_on) {   // later-seed rounds: seeds extended on the row kernels, searches run whole
                std::vector<unsigned long long> lc((size_t)MAX_HSP * LATER_CNT + LC_N);
                HIPCHK(hipMemcpy(lc.data(), e->work.d_lcnt.p, lc.size() * sizeof(unsigned long long),
                                 hipMemcpyDeviceToHost));
                for (int r = 0; r < MAX_HSP; r++) e->tm.later_seeds += (double)lc[(size_t)r * LATER_CNT];
                e->tm.later_whole += (double)lc[(size_t)MAX_HSP * LATER_CNT + LC_WHOLE];
            }
            break;
        }
        e->ovf_cap = std::max<uint64_t>(e->ovf_cap, ovn * 5 / 4 + 1024);
    }
    return RC_OK;
}

// Stage 6: (query gene, subject sample) -> contiguous HSPs, appended to the
// shard's store. Direct groups of every run first, in candidate order;
// mirrored groups (spec 5b: the subject->query direction of the same
// alignments) follow, each sorted into the order that search emits. Event EV_GROUPS1.
static int group_stage(rc_engine *e, const TileCtx &C)
{
    const int N = (int)e->samples.size();
    const size_t R = C.runs.size();
    const auto &cnb = C.cnb;
    GroupParams G{};
    G.N = N;
    G.cand_nh = e->work.d_cand_nh.p;
    G.cand_hsp = e->work.d_cand_hsp.p;
    G.cand_ovf = e->work.d_cand_ovf.p;
    G.ovf = e->work.d_ovf.p;
    G.shard_prefix = e->d_shard_prefix.p;
    G.n_cand = C.n_cand;
    G.cand_cap = e->cand_cap;
    G.tx_gene = e->d_tx_gene.p;
    G.tx_pos = e->d_tx_pos.p;
    G.tx = e->d_tx.p;
    G.n_genes = (uint32_t)e->gene_sample.size();
    G.grp_off = e->d_grp_off.p;
    G.grp_cnt = e->d_grp_cnt.p;
    auto exscan = [&](const uint32_t *in, uint64_t *out, size_t n) -> int {
        size_t tmp = 0;
        HIPCHK(rocprim::exclusive_scan(nullptr, tmp, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), e->st));
        CHK(e->work.d_tmp.ensure(tmp));
        HIPCHK(rocprim::exclusive_scan(e->work.d_tmp.p, tmp, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), e->st));
        return RC_OK;
    };
    auto run_group = [&](size_t r) {
        GroupParams g = G;
        g.gene_begin = C.rg0[r];
        g.gene_end = C.rg1[r];
        g.gc_off = e->work.d_gc_off.p + C.gcb[r];
        g.gc_cnt = e->work.d_gc_cnt.p + C.gcb[r];
        g.cnt = e->work.d_gcount.p + cnb[r];
        g.scan = e->work.d_gscan.p + cnb[r];
        return g;
    };
    std::vector<uint64_t> nd(R, 0);
    for (size_t r = 0; r < R; r++) {
        const size_t nsgrp = cnb[r + 1] - cnb[r] - 1;
        HIPCHK(hipMemsetAsync(e->work.d_gcount.p + cnb[r] + nsgrp, 0, 4, e->st));
        launch_group(run_group(r), GROUP_DIRECT_COUNT, e->st);
        CHK(exscan(e->work.d_gcount.p + cnb[r], e->work.d_gscan.p + cnb[r], nsgrp + 1));
        HIPCHK(hipMemcpyAsync(&nd[r], e->work.d_gscan.p + cnb[r] + nsgrp, 8, hipMemcpyDeviceToHost, e->st));
    }
    uint64_t nm = 0;
    // the other direction's groups: mirror images (spec 5b), or the reverse
    // searches of the shared candidate set (their own HSPs, in their order)
    const bool mirror = e->o.symmetric || e->share;
    if (e->share) {
        G.cand_nh = e->work.d_cand_nh_r.p;
        G.cand_hsp = e->work.d_cand_hsp_r.p;
        G.cand_ovf = e->work.d_cand_ovf_r.p;
    }
    if (mirror) {
        // the window of the tile's mirrored groups: every HSP is between a
        // query transcript of a pair's a (lower sample) and a subject
        // transcript of its b, so its mirrored group is (gene of b, sample a)
        int a_lo = N, a_hi = 0, b_lo = N, b_hi = 0;
        for (const auto &pr : e->tiles[C.ti].pairs) {
            a_lo = std::min(a_lo, pr.first);
            a_hi = std::max(a_hi, pr.first + 1);
            b_lo = std::min(b_lo, pr.second);
            b_hi = std::max(b_hi, pr.second + 1);
        }
        if (a_hi <= a_lo || b_hi <= b_lo) a_lo = a_hi = b_lo = b_hi = 0;
        G.ms0 = a_lo;
        G.msn = a_hi - a_lo;
        G.mg0 = e->sample_gene_begin[b_lo];
        G.mgw = e->sample_gene_begin[b_hi] - e->sample_gene_begin[b_lo];
        const size_t nwin = (size_t)G.mgw * (size_t)G.msn;
        CHK(e->work.d_mcnt.ensure(nwin + 1));
        CHK(e->work.d_mcur.ensure(std::max<uint64_t>(C.n_cand, 1)));   // per candidate: its slots' start in its group
        CHK(e->work.d_mscan.ensure(nwin + 1));
        G.mcnt = e->work.d_mcnt.p;
        G.mcur = e->work.d_mcur.p;
        HIPCHK(hipMemsetAsync(e->work.d_mcnt.p, 0, (nwin + 1) * 4, e->st));
        launch_group(G, GROUP_MIRROR_COUNT, e->st);   // mirrored groups (spec 5b)
        CHK(exscan(e->work.d_mcnt.p, e->work.d_mscan.p, nwin + 1));
        HIPCHK(hipMemcpyAsync(&nm, e->work.d_mscan.p + nwin, 8, hipMemcpyDeviceToHost, e->st));
    }
    CHK(wait_st(e));
    uint64_t ndt = 0;
    for (uint64_t v : nd) ndt += v;
    const uint64_t nh = e->hsp_used + ndt + nm;
    if (nh > 0xFFFFFFFFull) return fail(RC_E_LIMIT, "more than 2^32 HSPs on one GPU: use more shards");
    CHK(grow_hsp(e, nh));
    uint64_t base = e->hsp_used;
    for (size_t r = 0; r < R; r++) {
        GroupParams g = run_group(r);
        g.cand_nh = e->work.d_cand_nh.p;
        g.cand_hsp = e->work.d_cand_hsp.p;
        g.cand_ovf = e->work.d_cand_ovf.p;
        g.out = e->d_hsp.p;
        g.base = base;
        launch_group(g, GROUP_DIRECT_WRITE, e->st);
        base += nd[r];
    }
    if (mirror) {
        CHK(e->work.d_mkey.ensure(2 * nm + 2));
        CHK(e->work.d_mbig.ensure(nm / 33 + 2));
        HIPCHK(hipMemsetAsync(e->d_count.p + DC_MBIG, 0, sizeof(unsigned long long), e->st));
        G.mscan = e->work.d_mscan.p;
        G.out = e->d_hsp.p;
        G.mbase = base;
        G.mkey = e->work.d_mkey.p;
        G.mbig = e->work.d_mbig.p;
        G.mbig_n = e->d_count.p + DC_MBIG;
        launch_group(G, GROUP_MIRROR_SCATTER, e->st);
        launch_group(G, GROUP_MIRROR_SORT, e->st);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[EV_GROUPS1], e->st));
    CHK(wait_st(e));
    e->hsp_used = nh;
    return RC_OK;
}

// One alignment pass over tile ti: pack, DUST, index, seeds (one launch per
// run of query samples), extension, and the (query gene, subject sample) HSP
// groups appended to the shard's store.
static int align_tile(rc_engine *e, int ti)
{
    TileCtx C;
    C.ti = ti;
    CHK(index_stage(e, ti));
    CHK(plan_stage(e, C));
    CHK(seed_stage(e, C));
    CHK(extension_stage(e, C));
    CHK(group_stage(e, C));
    e->tm.pack_ms += ev_ms(e, EV_PACK0, EV_INDEX0);
    e->tm.index_ms += ev_ms(e, EV_INDEX0, EV_ALIGN0);
    if (e->o.dust_level > 0 && !e->external) {
        float dms = 0;
        if (hipEventElapsedTime(&dms, e->evd[EVD_DUST0], e->evd[EVD_DUST1]) == hipSuccess) e->tm.dust_ms += dms;
    }
    e->tm.align_ms += ev_ms(e, EV_ALIGN0, EV_GROUPS1);
    e->tm.seed_kernel_ms += ev_ms(e, EV_SEED0, EV_SEED1);
    e->tm.align_kernel_ms += ev_ms(e, EV_EXTEND0, EV_EXTEND1);
    return RC_OK;
}

static int do_align_tiles(rc_engine *e);

static int do_align(rc_engine *e)
{
    CHK(upload(e));
    CHK(set_device(e));
    e->aligned = e->finished = e->rbh_done = false;
    e->tm = rc_timing{};
    const double t0 = wall_ms();
    const int rc = do_align_tiles(e);
    e->tm.align_wall_ms = wall_ms() - t0;
    return rc;
}

static int do_align_tiles(rc_engine *e)
{
    if (e->external) {
        HIPCHK(hipEventRecord(e->ev[EV_PACK0], e->st));
        CHK(load_external(e));
        HIPCHK(hipEventRecord(e->ev[EV_INDEX0], e->st));
        HIPCHK(hipEventSynchronize(e->ev[EV_INDEX0]));
        e->tm.align_ms = ev_ms(e, EV_PACK0, EV_INDEX0);
        e->aligned = true;
        return RC_OK;
    }
    const int N = (int)e->samples.size();
    // the samples of this shard's pairs must be on this GPU (a graph-only
    // engine, rc_import_edges on a fresh engine, aligns nothing and needs none)
    for (uint64_t p = e->pair0; p < e->pair1; p++)
        for (int s : {(int)e->pair_a[p], (int)e->pair_b[p]})
            if (!e->samples[s].resident)
                return fail(RC_E_STATE, "sample " + e->samples[s].label +
                                            " is aligned by this shard but was added without its sequence");
    const size_t ngrp = (size_t)e->gene_sample.size() * N;
    CHK(e->d_grp_off.ensure(ngrp));
    CHK(e->d_grp_cnt.ensure(ngrp));
    HIPCHK(hipMemsetAsync(e->d_grp_cnt.p, 0, ngrp * 4, e->st));
    HIPCHK(hipMemsetAsync(e->d_grp_off.p, 0, ngrp * 4, e->st));
    if (e->tiles_for != (int64_t)e->pair0 || e->tiles.empty()) {
        plan_tiles(e);
        e->tiles_for = (int64_t)e->pair0;
        e->work.tile_loaded = -1;
    }
    e->hsp_used = 0;
    e->n_seeds = e->n_cands = 0;
    e->work.idx_bchunk = -1;   // every run builds its indexes and masks anew
    // the tile loaded last goes first (its tables stay on the device)
    const int nt = (int)e->tiles.size();
    const int first = (e->work.tile_loaded >= 0 && e->work.tile_loaded < nt) ? e->work.tile_loaded : 0;
    for (int k = 0; k < nt; k++) CHK(align_tile(e, (first + k) % nt));
    e->tm.tiles = (double)nt;
    e->n_hsps = e->hsp_used;
    e->aligned = true;
    return RC_OK;
}

// Top-N + reciprocal best hits for this shard's items -> table rows, edges.
static int do_rbh(rc_engine *e)
{
    if (!e->aligned) return fail(RC_E_STATE, "rc_finish before rc_align");
    CHK(set_device(e));
    const int N = (int)e->samples.size();
    const uint64_t ni = e->item1 - e->item0;
    const size_t np = e->pair_a.size();
    e->finished = false;
    HIPCHK(hipEventRecord(e->ev[EV_RBH0], e->st));
    CHK(e->work.d_cnt4.ensure(4 * (ni + 1)));
    CHK(e->d_off4.ensure(4 * (ni + 1)));
    HIPCHK(hipMemsetAsync(e->work.d_cnt4.p, 0, 4 * (ni + 1) * 4, e->st));
    // the RBH selection loops' 8-byte view of the group table (bit score,
    // subject gene): r05, rbh_kernel 6.5 -> see DESIGN §4
    CHK(e->work.d_hkey.ensure(std::max<uint64_t>(e->n_hsps, 1)));   // (n_hsps: aligned or imported)
    launch_hkey(e->d_hsp.p, e->n_hsps, e->d_tx_gene.p, e->work.d_hkey.p, e->st);
    RbhParams R{};
    R.hsp = e->d_hsp.p;
    R.hk = e->work.d_hkey.p;
    R.grp_off = e->d_grp_off.p;
    R.grp_cnt = e->d_grp_cnt.p;
    R.n_genes = (uint32_t)e->gene_sample.size();
    R.tx_gene = e->d_tx_gene.p;
    R.tx = e->d_tx.p;
    R.sample_gene_begin = e->d_sample_gene_begin.p;
    R.pair_item_begin = e->d_pair_item_begin.p;
    R.pair_a = e->d_pair_a.p;
    R.pair_b = e->d_pair_b.p;
    R.n_pairs = (int32_t)np;
    R.N = N;
    R.top_n = e->o.top_matches;
    R.keep_all = e->o.keep_all;
    R.item0 = e->item0;
    R.n_items = ni;
    R.n_rows = e->work.d_cnt4.p;
    R.n_fsel = e->work.d_cnt4.p + (ni + 1);
    R.n_rsel = e->work.d_cnt4.p + 2 * (ni + 1);
    R.n_edges = e->work.d_cnt4.p + 3 * (ni + 1);
    // one pass over the groups: counts, and rows/edges in per-item slots
    CHK(e->work.d_rows_tmp.ensure(std::max<uint64_t>(ni, 1) * RBH_RMAX));
    CHK(e->work.d_edges_tmp.ensure(std::max<uint64_t>(ni, 1) * RBH_EMAX));
    HIPCHK(hipMemsetAsync(e->d_status.p + 1, 0, sizeof(unsigned int), e->st));
    R.rows_tmp = e->work.d_rows_tmp.p;
    R.edges_tmp = e->work.d_edges_tmp.p;
    R.ovf = e->d_status.p + 1;
    launch_rbh(R, 2, e->st);
    HIPCHK(hipGetLastError());
    for (int k = 0; k < 4; k++) {
        size_t tmp = 0;
        const uint32_t *in = e->work.d_cnt4.p + k * (ni + 1);
        uint64_t *out = e->d_off4.p + k * (ni + 1);
        HIPCHK(rocprim::exclusive_scan(nullptr, tmp, in, out, (uint64_t)0, (size_t)ni + 1, rocprim::plus<uint64_t>(),
                                       e->st));
        CHK(e->work.d_tmp.ensure(tmp));
        HIPCHK(rocprim::exclusive_scan(e->work.d_tmp.p, tmp, in, out, (uint64_t)0, (size_t)ni + 1,
                                       rocprim::plus<uint64_t>(), e->st));
    }
    uint64_t tot[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; k++)
        HIPCHK(hipMemcpyAsync(&tot[k], e->d_off4.p + k * (ni + 1) + ni, 8, hipMemcpyDeviceToHost, e->st));
    unsigned int slot_ovf = 0;
    HIPCHK(hipMemcpyAsync(&slot_ovf, e->d_status.p + 1, sizeof slot_ovf, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    e->n_rows = tot[0];
    e->n_edges = tot[3];
    e->n_local_edges = tot[3];
    CHK(e->d_rows.ensure(e->n_rows));
    CHK(e->d_edges.ensure(e->n_edges));
    R.row_off = e->d_off4.p;
    R.fsel_off = e->d_off4.p + (ni + 1);
    R.rsel_off = e->d_off4.p + 2 * (ni + 1);
    R.edge_off = e->d_off4.p + 3 * (ni + 1);
    R.rows = e->d_rows.p;
    R.edges = e->d_edges.p;
    if (slot_ovf || e->knobs.rbh_two_pass)
        launch_rbh(R, 1, e->st);   // an item had more rows or edges than its slots: full second pass
    else
        launch_rbh_place(R, e->st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[EV_GRAPH0], e->st));
    HIPCHK(hipEventSynchronize(e->ev[EV_GRAPH0]));
    e->tm.rbh_ms = ev_ms(e, EV_RBH0, EV_GRAPH0);
    e->rbh_done = true;
    return RC_OK;
}

// Gene matches graph over d_edges[0, n_edges): connected components, ideal
// filter, restricted pair sums.
static int do_graph(rc_engine *e)
{
    if (!e->rbh_done) return fail(RC_E_STATE, "graph phase before rc_finish");
    CHK(set_device(e));
    e->an.comp_valid = false;   // the per-component tables follow the graph
    e->an.census_valid = false;
    const int N = (int)e->samples.size();
    const uint32_t n_genes = (uint32_t)e->gene_sample.size();
    const size_t np = e->pair_a.size();
    HIPCHK(hipEventRecord(e->ev[EV_GRAPH0], e->st));
    CHK(e->d_parent.ensure(n_genes));
    CHK(e->d_present.ensure(n_genes));
    CHK(e->d_cnodes.ensure(n_genes));
    CHK(e->d_cedges.ensure(n_genes));
    CHK(e->d_ideal.ensure(n_genes));
    CHK(e->d_sample_present.ensure(N));
    CHK(e->d_stats.ensure(8));
    HIPCHK(hipMemsetAsync(e->d_sample_present.p, 0, N * 4, e->st));
    HIPCHK(hipMemsetAsync(e->d_stats.p, 0, 8 * 8, e->st));
    launch_cc(e->d_edges.p, e->n_edges, n_genes, e->d_gene_sample.p, N, e->sample_count_given, e->d_parent.p,
              e->d_present.p, e->d_cnodes.p,
              e->d_cedges.p, e->d_sample_present.p, e->d_ideal.p, e->d_stats.p, e->st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[EV_REDUCE0], e->st));
    CHK(e->d_num.ensure(np));
    CHK(e->d_den.ensure(np));
    CHK(e->d_num_all.ensure(np));
    CHK(e->d_den_all.ensure(np));
    HIPCHK(hipMemsetAsync(e->d_num.p, 0, np * 8, e->st));
    HIPCHK(hipMemsetAsync(e->d_den.p, 0, np * 8, e->st));
    HIPCHK(hipMemsetAsync(e->d_num_all.p, 0, np * 8, e->st));
    HIPCHK(hipMemsetAsync(e->d_den_all.p, 0, np * 8, e->st));
    launch_pair_sums(e->d_edges.p, e->n_edges, e->d_parent.p, e->d_ideal.p, e->d_num.p, e->d_den.p,
                     e->d_num_all.p, e->d_den_all.p, e->st);
    HIPCHK(hipGetLastError());
    e->h_num.assign(np, 0);
    e->h_den.assign(np, 0);
    e->h_num_all.assign(np, 0);
    e->h_den_all.assign(np, 0);
    e->h_stats.assign(8, 0);
    if (np) {
        HIPCHK(hipMemcpyAsync(e->h_num.data(), e->d_num.p, np * 8, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(e->h_den.data(), e->d_den.p, np * 8, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(e->h_num_all.data(), e->d_num_all.p, np * 8, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(e->h_den_all.data(), e->d_den_all.p, np * 8, hipMemcpyDeviceToHost, e->st));
    }
    HIPCHK(hipMemcpyAsync(e->h_stats.data(), e->d_stats.p, 8 * 8, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipEventRecord(e->ev[EV_REDUCE1], e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    e->tm.graph_ms = ev_ms(e, EV_GRAPH0, EV_REDUCE0);
    e->tm.reduce_ms = ev_ms(e, EV_REDUCE0, EV_REDUCE1);
    e->tm.total_ms = e->tm.pack_ms + e->tm.index_ms + e->tm.align_ms + e->tm.rbh_ms + e->tm.graph_ms + e->tm.reduce_ms;
    e->finished = true;
    return RC_OK;
}

static int do_finish(rc_engine *e)
{
    CHK(do_rbh(e));
    if (e->o.shard_count == 1) return do_graph(e);
    return RC_OK;
}

extern "C" {

int rc_upload(rc_engine *e)
{
    if (!e) return fail(RC_E_ARG, "null engine");
    return upload(e);
}

int rc_align(rc_engine *e)
{
    if (!e) return fail(RC_E_ARG, "null engine");
    return do_align(e);
}

int rc_finish(rc_engine *e)
{
    if (!e) return fail(RC_E_ARG, "null engine");
    return do_finish(e);
}

int rc_run(rc_engine *e)
{
    if (!e) return fail(RC_E_ARG, "null engine");
    if (e->o.shard_count != 1) return fail(RC_E_STATE, "sharded engines use rc_align / rc_finish / rc_import_edges");
    CHK(do_align(e));
    return do_finish(e);
}

int rc_set_sample_count(rc_engine *e, int32_t sample_count)
{
    if (!e) return fail(RC_E_ARG, "null engine");
    if (sample_count < 0) return fail(RC_E_ARG, "sample_count must be >= 0");
    e->sample_count_given = sample_count;
    return RC_OK;
}

int rc_dust_mask(rc_engine *e, int32_t s, uint8_t *buf, uint64_t cap, uint64_t *n)
{
    if (!e || !n) return fail(RC_E_ARG, "null argument");
    if (!e->aligned) return fail(RC_E_STATE, "no alignment yet");
    if (s < 0 || s >= (int)e->samples.size()) return fail(RC_E_ARG, "bad sample");
    const SampleRec &S = e->samples[s];
    *n = S.nbases;
    if (!buf) return RC_OK;
    if (cap < S.nbases) return fail(RC_E_CAPACITY, "buffer too small");
    if (!S.nbases) return RC_OK;
    if (e->o.dust_level <= 0 || e->external) {
        std::memset(buf, 0, S.nbases);
        return RC_OK;
    }
    // the mask of the loaded tile, where the sample sits at tile_pos[s]
    if (e->work.tile_loaded < 0) return fail(RC_E_STATE, "no tile loaded");
    const auto &ts = e->tiles[e->work.tile_loaded].samples;
    if (std::find(ts.begin(), ts.end(), s) == ts.end())
        return fail(RC_E_STATE, "the sample is not in the last alignment pass (tile)");
    if (!e->dmask_only.empty() && !e->dmask_only[s])
        return fail(RC_E_STATE, "the last rc_dust_masks pass did not mask this sample");
    CHK(set_device(e));
    const uint64_t b0 = e->tile_pos[s];
    const uint64_t w0 = b0 >> 6, w1 = (b0 + S.nbases + 63) >> 6;
    std::vector<uint64_t> words(w1 - w0);
    HIPCHK(hipMemcpy(words.data(), e->work.d_dmask.p + 1 + w0, words.size() * 8, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < S.nbases; i++) {
        const uint64_t p = b0 + i;
        buf[i] = (uint8_t)((words[(p >> 6) - w0] >> (p & 63)) & 1);
    }
    return RC_OK;
}

// DUST masks computed once per sample across shards: each
// sample's mask is made on one rank that holds it (rc_dust_masks), the masks
// are exchanged, and every rank hands them to its engine (rc_set_dust_masks),
// whose alignment then copies them into its tiles instead of running DUST.
// Layout: the listed samples in order, ceil(bases / 64) words each, bit b of
// word w = base 64 w + b of the sample (1: masked); bits past the last base 0.
static uint64_t mask_words(const rc_engine *e, const int32_t *samples, int32_t n)
{
    uint64_t w = 0;
    for (int32_t i = 0; i < n; i++) w += (e->samples[samples[i]].nbases + 63) >> 6;
    return w;
}

int rc_dust_masks(rc_engine *e, const int32_t *samples, int32_t n, uint64_t *out, uint64_t cap_words,
                  uint64_t *n_words, int on_device)
{
    if (!e || !n_words || n < 0 || (n && !samples)) return fail(RC_E_ARG, "null argument");
    CHK(upload(e));
    const int N = (int)e->samples.size();
    for (int32_t i = 0; i < n; i++) {
        if (samples[i] < 0 || samples[i] >= N) return fail(RC_E_ARG, "bad sample");
        if (!e->samples[samples[i]].resident)
            return fail(RC_E_STATE, "sample " + e->samples[samples[i]].label + " was added without its sequence");
    }
    const uint64_t words = mask_words(e, samples, n);
    *n_words = words;
    if (!out) return RC_OK;
    if (cap_words < words) return fail(RC_E_CAPACITY, "buffer too small");
    CHK(set_device(e));
    // passes of their own: the tile tables of a previous run are replaced. Its
    // results stay valid: HSP groups, RBH rows and edges read only the
    // transcripts' lengths and samples, never a tile's positions or masks
    std::vector<int> ss(samples, samples + n);
    std::sort(ss.begin(), ss.end());
    ss.erase(std::unique(ss.begin(), ss.end()), ss.end());
    std::vector<std::vector<uint64_t>> oof(N);   // word offsets of each listed sample in `out` (any repeats)
    {
        uint64_t o = 0;
        for (int32_t i = 0; i < n; i++) {
            oof[samples[i]].push_back(o);
            o += (e->samples[samples[i]].nbases + 63) >> 6;
        }
    }
    if (e->tiles_for != (int64_t)e->pair0 || e->tiles.empty()) {
        plan_tiles(e);
        e->tiles_for = (int64_t)e->pair0;
        e->work.tile_loaded = -1;
    }
    // the shard's own alignment tile when it is a single tile holding these
    // samples (its tables stay loaded for rc_align), else tiles of these
    // samples alone, as many as the 2^32-base tile limit takes (a C5 rank
    // masks ~4 Gbp); each packed, its DUST masks copied out
    bool own = e->tiles.size() == 1;
    for (int s : ss)
        own = own && std::binary_search(e->tiles[0].samples.begin(), e->tiles[0].samples.end(), s);
    std::vector<std::vector<int>> chunks;
    if (own) {
        chunks.push_back(ss);
    } else {
        const uint64_t cap = e->knobs.tile_bases;
        uint64_t acc = 0;
        for (int s : ss) {
            const uint64_t b = align_up(e->samples[s].nbases);
            if (chunks.empty() || (acc + b > cap && !chunks.back().empty())) {
                chunks.push_back({});
                acc = 0;
            }
            chunks.back().push_back(s);
            acc += b;
        }
    }
    const bool dust = e->o.dust_level > 0 && !e->external;
    int rc = RC_OK;
    for (size_t c = 0; c < chunks.size() && rc == RC_OK; c++) {
        int ti = 0;
        if (!own) {
            rc_engine::Tile T;
            T.samples = chunks[c];
            e->tiles.push_back(T);
            e->work.tile_loaded = -1;
            ti = (int)e->tiles.size() - 1;
        }
        rc = load_tile(e, ti);
        if (rc == RC_OK) rc = pack_tile(e);
        if (rc == RC_OK && dust) {
            const size_t mw = (e->tile_total >> 6) + 4;
            rc = e->work.d_dmask.ensure(mw);
            if (rc == RC_OK && hipMemsetAsync(e->work.d_dmask.p, 0, mw * 8, e->st) != hipSuccess)
                rc = fail(RC_E_HIP, "hipMemsetAsync");
            if (rc == RC_OK) rc = dust_samples(e, chunks[c], e->st);
        }
        for (size_t k = 0; rc == RC_OK && k < chunks[c].size(); k++) {
            const int s = chunks[c][k];
            const uint64_t nb = e->samples[s].nbases, nw = (nb + 63) >> 6;
            if (!nw) continue;
            for (uint64_t w0 : oof[s]) {
                hipError_t h = hipSuccess;
                if (dust) {
                    h = hipMemcpyAsync(out + w0, e->work.d_dmask.p + 1 + (e->tile_pos[s] >> 6), nw * 8,
                                       on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->st);
                } else if (on_device) {
                    h = hipMemsetAsync(out + w0, 0, nw * 8, e->st);
                } else {
                    std::memset(out + w0, 0, nw * 8);
                }
                if (h != hipSuccess) rc = fail(RC_E_HIP, "mask copy");
            }
        }
        if (rc == RC_OK && hipStreamSynchronize(e->st) != hipSuccess) rc = fail(RC_E_HIP, "hipStreamSynchronize");
        if (!own) {
            e->tiles.pop_back();
            e->work.tile_loaded = -1;
        }
    }
    if (own) {   // the loaded tile's masks now hold the listed samples only
        e->dmask_only.assign(N, 0);
        for (int s : ss) e->dmask_only[s] = 1;
    }
    // bits past each sample's last base cleared (its last word)
    uint64_t o = 0;
    for (int32_t i = 0; rc == RC_OK && dust && i < n; i++) {
        const uint64_t nb = e->samples[samples[i]].nbases, nw = (nb + 63) >> 6;
        o += nw;
        if (!nw || !(nb & 63)) continue;
        const uint64_t keep = (1ull << (nb & 63)) - 1ull;
        if (on_device) {
            uint64_t w = 0;
            if (hipMemcpy(&w, out + o - 1, 8, hipMemcpyDeviceToHost) != hipSuccess ||
                (w &= keep, hipMemcpy(out + o - 1, &w, 8, hipMemcpyHostToDevice)) != hipSuccess)
                rc = fail(RC_E_HIP, "mask tail");
        } else {
            out[o - 1] &= keep;
        }
    }
    e->work.idx_bchunk = -1;
    return rc;
}

int rc_set_dust_masks(rc_engine *e, const int32_t *samples, int32_t n, const uint64_t *bits, uint64_t n_words,
                      int on_device)
{
    if (!e || n < 0 || (n && !samples)) return fail(RC_E_ARG, "null argument");
    CHK(upload(e));
    const int N = (int)e->samples.size();
    for (int32_t i = 0; i < n; i++)
        if (samples[i] < 0 || samples[i] >= N) return fail(RC_E_ARG, "bad sample");
    const uint64_t words = mask_words(e, samples, n);
    if (n_words != words) return fail(RC_E_ARG, "mask words do not match the samples' lengths");
    if (words && !bits) return fail(RC_E_ARG, "null argument");
    CHK(set_device(e));
    e->dust_imp_off.assign(N, ~0ull);
    CHK(e->d_dust_imp.ensure(std::max<uint64_t>(words, 1)));
    if (words)
        HIPCHK(hipMemcpy(e->d_dust_imp.p, bits, words * 8, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    uint64_t o = 0;
    for (int32_t i = 0; i < n; i++) {
        e->dust_imp_off[samples[i]] = o;
        o += (e->samples[samples[i]].nbases + 63) >> 6;
    }
    return RC_OK;
}

int rc_timings(rc_engine *e, rc_timing *t)
{
    if (!e || !t) return fail(RC_E_ARG, "null argument");
    *t = e->tm;
    t->dev_bytes = (double)g_dev_bytes.load();
    t->dev_peak_bytes = (double)g_dev_peak.load();
    return RC_OK;
}

int rc_export_edges(rc_engine *e, void *buf, uint64_t cap, uint64_t *n, int on_device)
{
    if (!e || !n) return fail(RC_E_ARG, "null argument");
    if (!e->rbh_done) return fail(RC_E_STATE, "rc_export_edges before rc_finish");
    CHK(set_device(e));
    const uint64_t tot = e->n_local_edges;
    *n = tot;
    if (!buf) return RC_OK;
    if (cap < tot) return fail(RC_E_CAPACITY, "buffer too small");
    if (e->n_edges != e->n_local_edges || e->graph_only)
        return fail(RC_E_STATE, "edges already replaced by rc_import_edges");
    if (tot)
        HIPCHK(hipMemcpy(buf, e->d_edges.p, tot * sizeof(DEdge), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return RC_OK;
}

int rc_import_edges(rc_engine *e, const void *buf, uint64_t n, int on_device)
{
    return rc_import_edge_parts(e, buf, &n, 1, n, on_device);
}

// parts blocks of records, block r at record r * stride of buf with counts[r]
// valid records: the concatenation is imported (an all-gather's padded
// receive buffer goes in as it is, no compacted copy outside the engine)
int rc_import_edge_parts(rc_engine *e, const void *buf, const uint64_t *counts, int32_t parts, uint64_t stride,
                         int on_device)
{
    if (!e || parts < 0 || (parts && !counts)) return fail(RC_E_ARG, "null argument");
    uint64_t n = 0;
    for (int32_t r = 0; r < parts; r++) {
        if (counts[r] > stride) return fail(RC_E_ARG, "a part holds more records than the stride");
        n += counts[r];
    }
    if (n && !buf) return fail(RC_E_ARG, "null argument");
    if (!e->rbh_done) {
        // a fresh engine (samples added, nothing aligned): graph-only mode,
        // the records describe an imported graph and its tables
        if (e->aligned || e->external) return fail(RC_E_STATE, "rc_import_edges before rc_finish");
        CHK(upload(e));
        e->graph_only = e->rbh_done = true;
    }
    CHK(set_device(e));
    const uint32_t ng = (uint32_t)e->gene_sample.size();
    const uint64_t np = e->pair_a.size();
    const DEdge *src = static_cast<const DEdge *>(buf);
    if (!on_device) {
        for (int32_t r = 0; r < parts; r++) {
            const DEdge *ed = src + (uint64_t)r * stride;
            for (uint64_t i = 0; i < counts[r]; i++) {
                const bool node = ed[i].pair == NODE_REC;
                if (ed[i].a >= ng || ed[i].b >= ng || (!node && (ed[i].pair & ~EDGE_SUM_ONLY) >= np) ||
                    (node && ed[i].a != ed[i].b))
                    return fail(RC_E_ARG, "edge record out of range");
            }
        }
    }
    if (on_device) {
        // the same range check on the device, over the caller's blocks before
        // anything of the engine's is replaced: a malformed all-gather must
        // not reach the union-find kernels, and a refused import leaves the
        // engine's own edges in place
        unsigned int bad = 0;
        HIPCHK(hipMemsetAsync(e->d_status.p + 2, 0, sizeof(unsigned int), e->st));
        for (int32_t r = 0; r < parts; r++)
            if (counts[r]) launch_edge_check(src + (uint64_t)r * stride, counts[r], ng, np, e->d_status.p + 2, e->st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&bad, e->d_status.p + 2, sizeof bad, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipStreamSynchronize(e->st));
        if (bad) return fail(RC_E_ARG, "edge record out of range");
    }
    // the local edges are replaced: their buffer goes before the new one is
    // allocated (a sharded rank's peak holds the gathered records once)
    if (e->d_edges.cap < n) e->d_edges.release();
    CHK(e->d_edges.ensure(n));
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    uint64_t o = 0;
    for (int32_t r = 0; r < parts; r++) {
        if (counts[r])
            HIPCHK(hipMemcpyAsync(e->d_edges.p + o, src + (uint64_t)r * stride, counts[r] * sizeof(DEdge), kind, e->st));
        o += counts[r];
    }
    e->n_edges = n;
    e->n_local_edges = 0;   // the local edges are gone
    HIPCHK(hipStreamSynchronize(e->st));   // (the caller's host buffer is not retained)
    return do_graph(e);
}

// Free the alignment working set of a finished run (struct Work: tile copies,
// indexes, seeds, candidates, extension and grouping scratch). What the
// results need stays (inputs, HSP store and groups, table rows, edges, graph
// arrays); the next rc_align allocates the rest again.
int rc_trim(rc_engine *e)
{
    if (!e) return fail(RC_E_ARG, "null engine");
    CHK(set_device(e));
    HIPCHK(hipStreamSynchronize(e->st));
    HIPCHK(hipStreamSynchronize(e->st2));
    e->work = rc_engine::Work{};
    return RC_OK;
}

// The sample pairs in the engine's subject-major order ((0,1), (0,2), (1,2),
// (0,3), ...), cut into shard_count contiguous ranges of about equal sequence
// length (L_a + L_b per pair, the byte model of SURVEY.md §8d): pair p goes to
// the shard whose share of the total holds the midpoint of p's cost interval.
// A shard's second samples are then a contiguous sample range, and its seed
// index covers only those samples.
int rc_plan_shards(const int64_t *sample_bases, int32_t n_samples, int32_t shard_count, int64_t *pair_first)
{
    return rc_plan_pairs(sample_bases, n_samples, shard_count, nullptr, nullptr, pair_first);
}

int rc_plan_pairs(const int64_t *sample_bases, int32_t n_samples, int32_t shard_count, int32_t *pair_a,
                  int32_t *pair_b, int64_t *pair_first)
{
    if (!pair_first || shard_count < 1 || n_samples < 0 || (n_samples && !sample_bases))
        return fail(RC_E_ARG, "bad argument");
    if (n_samples > MAX_SAMPLES) return fail(RC_E_LIMIT, "more than 65535 samples");
    std::vector<int32_t> pa, pb;
    std::vector<int64_t> first;
    plan::plan_pairs(sample_bases, n_samples, shard_count, pa, pb, first);
    std::copy(first.begin(), first.end(), pair_first);
    if (pair_a) std::copy(pa.begin(), pa.end(), pair_a);
    if (pair_b) std::copy(pb.begin(), pb.end(), pair_b);
    return RC_OK;
}

int rc_pair_order(rc_engine *e, int32_t *pair_a, int32_t *pair_b)
{
    if (!e || !pair_a || !pair_b) return fail(RC_E_ARG, "null argument");
    CHK(upload(e));
    std::copy(e->pair_a.begin(), e->pair_a.end(), pair_a);
    std::copy(e->pair_b.begin(), e->pair_b.end(), pair_b);
    return RC_OK;
}

int rc_shard_pairs(rc_engine *e, int64_t *first, int64_t *last)
{
    if (!e || !first || !last) return fail(RC_E_ARG, "null argument");
    CHK(upload(e));
    *first = (int64_t)e->pair0;
    *last = (int64_t)e->pair1;
    return RC_OK;
}

}  // extern "C"
