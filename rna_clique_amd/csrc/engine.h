// Internal header of the engine's own translation units (engine.hip,
// results.hip, analysis.hip): error plumbing, the device buffer type, the
// knobs and the engine struct. Not installed; the C ABI is include/rcgpu.h.
#pragma once
#include "../../include/rcgpu.h"
#include "device.h"
#include "graph_pickle.h"
#include "fail.h"
#include "launch.h"

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

using namespace rcg;

static const size_t FRONT_PAD = 2;   // zero words in front of every packed array

// (the message is kept by engine.hip, for rc_last_error)
static inline int fail(int code, const std::string &msg) { return rcg_fail(code, msg); }

#define HIPCHK(x)                                                                                    \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) return fail(RC_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define CHK(x)                  \
    do {                        \
        int r_ = (x);           \
        if (r_ != RC_OK) return r_; \
    } while (0)

// engine.hip: the device bytes the engines of this process hold
void dev_account(long long b);

// Device buffer that only grows (no allocation once sized: reruns are alloc-free).
// It owns its allocation: moved and swapped, never copied. A move or a swap
// accounts for nothing (dev_account); a moved-from buffer is empty.
template <class T>
struct DBuf {
    T *p = nullptr;
    size_t cap = 0;
    DBuf() = default;
    DBuf(const DBuf &) = delete;
    DBuf &operator=(const DBuf &) = delete;
    DBuf(DBuf &&o) noexcept : p(o.p), cap(o.cap)
    {
        o.p = nullptr;
        o.cap = 0;
    }
    DBuf &operator=(DBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            swap(o);
        }
        return *this;
    }
    void swap(DBuf &o) noexcept
    {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
    int ensure(size_t n)
    {
        if (n <= cap && p) return RC_OK;
        release();
        size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        if (hipMalloc((void **)&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return fail(RC_E_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
        }
        cap = std::max<size_t>(n, 1);
        dev_account((long long)(cap * sizeof(T)));
        return RC_OK;
    }
    // a buffer allocated elsewhere (the growth paths that keep contents)
    void adopt(T *np, size_t ncap)
    {
        dev_account((long long)(ncap * sizeof(T)));   // both are held until the old one goes
        T *op = p;
        const size_t oc = cap;
        p = np;
        cap = ncap;
        if (op) {
            (void)hipFree(op);
            dev_account(-(long long)(oc * sizeof(T)));
        }
    }
    ~DBuf() { release(); }
    void release()
    {
        if (p) {
            (void)hipFree(p);
            dev_account(-(long long)(cap * sizeof(T)));
        }
        p = nullptr;
        cap = 0;
    }
};
static_assert(!std::is_copy_constructible<DBuf<int>>::value && !std::is_copy_assignable<DBuf<int>>::value,
              "a copy would free and account for the allocation twice");
static_assert(std::is_nothrow_move_constructible<DBuf<int>>::value, "moves only take the pointer over");

// engine.hip: Karlin-Altschul statistics
namespace stats {
const double LAMBDA = 1.28, K = 0.46, ALPHA = 1.5, BETA = -2.0;
double search_space(int64_t qlen, int64_t dblen, int64_t dbn);
double evalue(double ss, int32_t score_half);
}  // namespace stats

struct SampleRec {
    std::string label;
    uint64_t base = 0, nbases = 0;   // base: position in the concatenation of all samples (host bookkeeping)
    uint32_t tx_begin = 0, n_tx = 0;
    uint32_t gene_begin = 0, n_genes = 0;
    bool resident = true;            // bases on this GPU (rc_add_sample with a sequence)
    uint64_t abase = 0;              // resident: offset in d_ascii (a multiple of TILE_ALIGN)
};

// Samples start at multiples of TILE_ALIGN bases in d_ascii and in a tile's
// packed arrays: a 2^POS_TX_SHIFT-base block of the position -> transcript
// table never spans two samples, whatever samples a tile holds.
static const uint64_t TILE_ALIGN = 1ull << POS_TX_SHIFT;
static uint64_t align_up(uint64_t x) { return (x + TILE_ALIGN - 1) & ~(TILE_ALIGN - 1); }

// Test hooks: every one is set by a GPU test to reach a path that the default
// takes only at full size. The environment is read once, when the engine is
// created (rc_create); a variable changed later does not reach an engine that
// exists. One line per variable: name (default) and meaning.
struct Knobs {
    bool share;           // RC_SHARE (1): 0 = a pair's two directed searches one after the other
    uint64_t tile_bases;  // RC_TILE_BASES (2^32 - 2^24; at least TILE_ALIGN): a tile's most bases (tests: small tiles)
    bool tile_split;      // RC_TILE_SPLIT (1): 0 = no split tiles, so no index reuse from tile to tile
    int ovf_cap0;         // RC_OVF_CAP0 (unset = 0; else at least 1): first HSP overflow buffer size (tests: its retry)
    int win_words;        // RC_WIN_WORDS (unset = 0; else at least 4): row staging windows of that many words (tests)
    bool later;           // RC_LATER (1): 0 = extend_kernel runs the deferred searches' later seeds whole
    int later_rows;       // RC_LATER_ROWS (64): 32 = the later-seed rounds run the 32-lane pass first
    uint64_t later_cap;   // RC_LATER_CAP (24 M, at least 1): searches the later-seed rounds hold states for
    bool rbh_two_pass;    // RC_RBH_TWO_PASS (unset; any value sets it): always the full second RBH pass
    int resume;           // RC_RESUME (unset = -1: by the last run's overflows): 1 = always save 32-lane states, 0 = never
    uint32_t index_cap;   // RC_INDEX_CAP (unset = 0: the local sort's capacity; else at least 2): main-index ranges of more keys count as oversized (tests: the fallbacks)
    int nj_lds;           // RC_NJ_LDS (128; at most 128): the most samples whose neighbour-joining matrix lives in LDS; 0 = every tree through the global workspace (tests: that path)
};

// The engine's timing events (rc_engine::ev, on stream st), each named by what
// its record marks; a pair brackets one rc_timing field (ev_ms). The values
// are the order in which the events were added. External HSPs run no tile, so
// no stage records EV_PACK0 and EV_INDEX0 then: do_align_tiles reuses the two
// to bracket load_external (align_ms).
enum Ev {
    EV_PACK0 = 0,     // pack_tile: the packing starts (pack_ms to EV_INDEX0)
    EV_INDEX0 = 1,    // index_stage: packed, masks cleared; DUST and the index build start (index_ms to EV_ALIGN0)
    EV_ALIGN0 = 2,    // index_stage: indexes done (align_ms to EV_GROUPS1)
    EV_SEED0 = 3,     // seed_stage: before the reverse pass and the seed launches (seed_kernel_ms to EV_SEED1)
    EV_GROUPS1 = 4,   // group_stage: the tile's HSP groups are written
    EV_RBH0 = 5,      // do_rbh (rbh_ms to EV_GRAPH0)
    EV_GRAPH0 = 6,    // do_rbh: rows and edges placed; recorded again when do_graph starts (graph_ms to EV_REDUCE0)
    EV_REDUCE0 = 7,   // do_graph: components and ideal filter done (reduce_ms to EV_REDUCE1)
    EV_REDUCE1 = 8,   // do_graph: pair sums copied back
    EV_SEED1 = 9,     // seed_stage: an attempt's last seed launch
    EV_EXTEND0 = 10,  // extension_stage: before the row kernels (align_kernel_ms to EV_EXTEND1)
    EV_EXTEND1 = 11,  // extension_stage: after extend_kernel
    EV_RESAMPLE0 = 12, EV_RESAMPLE1 = 13,   // resample_fill: the replicate sums (resample_ms)
    EV_NJ0 = 14, EV_NJ1 = 15,               // nj_device: the trees and the split support (nj_ms)
    EV_PCOA0 = 16, EV_PCOA1 = 17,           // pcoa_device: the ordinations (pcoa_ms)
    EV_SPLIT0 = 18, EV_SPLIT1 = 19,         // rc_split_census, rc_tree_rf: the census and RF kernels (split_ms)
    EV_GROUP0 = 20, EV_GROUP1 = 21,         // group_device: the ranking and test kernels (group_ms)
    EV_DISP0 = 22, EV_DISP1 = 23,           // dispersion_device: the PERMDISP kernel (disp_ms)
    EV_MANTEL0 = 24, EV_MANTEL1 = 25,       // mantel_device: the ranking and Mantel kernels (mantel_ms)
    EV_N
};
// rc_engine::evd: DUST on the second stream
enum Evd {
    EVD_DUST0 = 0,   // on st2: DUST starts
    EVD_DUST1 = 1,   // on st2: DUST ends (st waits for it; dust_ms from EVD_DUST0)
    EVD_READY = 2,   // on st: DUST's start condition (the packed copy, the cleared masks)
    EVD_N
};

struct rc_engine {
    rc_opts o{};
    Knobs knobs{};
    hipStream_t st = nullptr;
    hipStream_t st2 = nullptr;   // DUST beside the index build
    std::vector<SampleRec> samples;
    uint64_t total_bases = 0;   // input bases added so far (all samples)
    uint64_t ascii_used = 0;    // bytes of d_ascii in use (resident samples, TILE_ALIGN-aligned)
    std::vector<uint64_t> tx_start{0};
    std::vector<int32_t> tx_sample, tx_gene_id, tx_iso;
    bool has_amb = false;

    // derived on upload
    std::vector<uint32_t> tx_gene, gene_tx_off, gene_tx, sample_gene_begin, sample_tx_begin;
    std::vector<int32_t> gene_sample, gene_id;
    std::vector<int64_t> db_len, db_n;
    std::vector<int32_t> pair_a, pair_b, pair_index;
    std::vector<int64_t> shard_first;   // shard r owns pairs [shard_first[r], shard_first[r + 1])
    std::vector<uint32_t> pair_item_begin;
    int32_t max_len = 0;
    int xbits = 24;                     // seed-key position bits (pos_bits(max_len))
    uint64_t n_items = 0;
    int index_bits = 16;
    uint64_t n_index = 0;               // entries of the loaded tile's index
    uint64_t tile_npos = 0;             // 16-mer positions of the loaded tile's indexed transcripts
    std::vector<TxInfo> h_tx;           // every transcript (start 0: the device table holds tile starts)
    std::vector<uint64_t> sample_kmers; // 16-mer positions of each sample's transcripts
    std::vector<TileSeg> h_segs;        // the loaded tile's samples (load_tile)
    std::vector<uint64_t> h_spos, h_send;

    // tiles of this shard (plan_tiles) and the one whose tables are loaded
    struct Tile {
        std::vector<int> samples;                 // ascending
        std::vector<std::pair<int, int>> pairs;   // (a, b), a < b
        // split tiles (a shard cut into several, every a below every b):
        // the b chunk's samples sit at bstart, the same in every tile of that
        // chunk, so consecutive tiles of one b chunk share its 16-mer index
        // and its DUST masks (only the a part is redone)
        int bchunk = -1;
        uint64_t bstart = 0;
    };
    std::vector<Tile> tiles;
    int64_t tiles_for = -1;
    std::vector<uint64_t> tile_pos;     // first base of each sample in the loaded tile
    uint64_t tile_total = 0;
    bool tile_direct = false;           // the loaded tile is d_ascii's layout (no gathered copy)
    uint32_t tile_ntx = 0;              // the tile's transcripts (DUST, near-mask index)
    uint32_t tile_nitx = 0;             // ... of its subject samples (the 16-mer index)
    std::vector<uint32_t> tile_tx_first;   // first transcript (in d_tile_tx) of each sample of the tile
    // DUST masks given by rc_set_dust_masks (computed once per sample across
    // shards): word offset of each sample's mask in d_dust_imp, ~0 = not given
    std::vector<uint64_t> dust_imp_off;
    // after an rc_dust_masks pass over the loaded tile itself: which samples'
    // masks it recomputed (the others were cleared); empty = every tile sample
    std::vector<char> dmask_only;
    uint64_t hsp_used = 0;              // HSPs appended to d_hsp by the tiles of this run

    // external HSPs
    bool external = false;
    std::map<std::pair<int, int>, std::vector<rc_hsp>> ext;

    // state
    bool uploaded = false, aligned = false, finished = false;
    // this shard's sample pairs [pair0, pair1) and their items [item0, item1)
    uint64_t pair0 = 0, pair1 = 0, item0 = 0, item1 = 0;
    uint64_t n_local_edges = 0;
    bool rbh_done = false;
    bool graph_only = false;        // an imported graph + tables, no alignment (rc_import_edges on a fresh engine)
    int32_t sample_count_given = 0; // > 0: the ideal test's sample count (rc_set_sample_count)

    // both directed searches of a pair from one candidate set (query = the
    // lower sample), unless spec 5b or RC_SHARE=0 (one after
    // the other); fixed when the engine is created
    bool share = false;
    // capacities and cursors that outlive a run (rc_trim keeps them: they
    // select the next run's first guesses and retry paths)
    int mindex_bits = 16;
    uint64_t n_mindex = 0;
    uint64_t rseed_cap = 0, n_rseeds = 0;
    // fraction of the last run's candidates whose first-seed extension
    // outgrew the 32-lane window (selects the saving row kernel, RC_RESUME)
    double ovf_frac = 0.0;
    uint32_t sort_epoch = 0;   // the index sort's pass counter (tags d_sort_status)
    uint64_t seed_cap = 0, cand_cap = 0, ovf_cap = 0;   // per-shard / total capacities
    uint64_t big_list_cap = 1 << 16;
    uint32_t big_cap = 1 << 13;
    // what the last run produced
    uint64_t n_rows = 0, n_edges = 0, n_hsps = 0, n_seeds = 0, n_cands = 0;

    // The alignment working set: what only rc_align (and rc_finish's RBH pass)
    // fills and reads, with the scalars that describe what these buffers hold.
    // rc_trim frees it whole (work = Work{}); the next rc_align allocates it
    // again. A finished run's results need none of it. (hidden, like Analysis:
    // the library exports none of the members the compiler generates for it)
    struct __attribute__((visibility("hidden"))) Work {
        int tile_loaded = -1;   // the tile whose tables are on the device (rc_dust_masks reads a loaded tile)
        // the b chunk (split tiles) whose index and DUST masks the device holds
        // from this run's previous tile (-1: none)
        int idx_bchunk = -1;
        uint64_t idx_bstart = 0;
        DBuf<uint8_t> d_tile_ascii;
        DBuf<TxInfo> d_tile_tx, d_tile_itx;
        DBuf<uint32_t> d_tile_gid;          // global id of each tile transcript
        DBuf<TileSeg> d_tile_segs;
        DBuf<uint64_t> d_tile_send;         // tile sample ends
        DBuf<uint64_t> d_F, d_RC, d_AF, d_ARC;
        DBuf<uint64_t> d_kpos_off, d_kcnt;
        // shared searches with DUST: masked tile transcripts, the near-mask index
        // of the reverse pass, its reverse-only seeds (sorted by forward gene)
        DBuf<uint8_t> d_tile_masked;
        DBuf<uint64_t> d_ment, d_ment2;
        DBuf<uint32_t> d_mbucket;
        uint64_t mnear_cap = 0;
        DBuf<LSeed> d_rseeds;
        DBuf<uint32_t> d_rseed_gene, d_rs_key, d_rs_idx, d_rs_range;
        DBuf<unsigned long long> d_rctr;   // [0] near-index entries, [1] reverse-only seeds
        DBuf<uint64_t> d_rtmask;
        DBuf<int32_t> d_trange, d_rtrange;   // [N][2] subject-sample range of each query sample (tmask / rtmask)
        uint32_t res_cap = 0;              // extensions d_resume has room for
        DBuf<uint64_t> d_ent, d_ent2;   // (k-mer << 32 | position), unsorted / sorted
        // the index sort's scratch (sort.hip): digit histograms + tile counters,
        // the look-back table (zeroed when allocated; tagged by pass epoch)
        DBuf<uint32_t> d_sort_scratch;
        DBuf<uint64_t> d_sort_status;
        // the main index's range offsets (2^G + 1) and its list of oversized ranges
        DBuf<uint32_t> d_range_off, d_range_list;
        DBuf<uint32_t> d_bucket;
        DBuf<PosTx> d_pos_tx;
        DBuf<uint64_t> d_sample_pos, d_txstart, d_kpos_rel, d_dmask;
        DBuf<uint32_t> d_dust_scratch;
        DBuf<uint64_t> d_dust_events;
        DBuf<unsigned long long> d_prof;
        // rocPRIM's temporary storage: the result and analysis calls size it
        // again when they need it
        DBuf<uint8_t> d_tmp;
        DBuf<HKey> d_hkey;   // RBH: (bit score, subject gene) per d_hsp entry
        DBuf<GSeed> d_seeds;
        DBuf<Cand> d_cands;
        DBuf<DHsp> d_cand_hsp, d_ovf;
        DBuf<uint8_t> d_cand_nh;
        DBuf<int32_t> d_cand_box, d_cand_box2;
        // shared searches (RC_SHARE, default): the reverse search's HSPs per candidate
        DBuf<DHsp> d_cand_hsp_r;
        DBuf<uint8_t> d_cand_nh_r;
        DBuf<uint32_t> d_cand_ovf_r, d_defer_r, d_list2, d_wide0, d_wide1;
        DBuf<int32_t> d_resume;   // saved 32-lane extension states for the 64-lane pass (RES_REC ints each)
        // later-seed rounds (shared searches): search states, the rounds' work
        // (alternating), active lists, counters
        DBuf<int32_t> d_later, d_lbox0, d_lbox1;
        DBuf<Cand> d_lvc0, d_lvc1;
        DBuf<uint32_t> d_llist0, d_llist1, d_lact0, d_lact1, d_lfull0, d_lfull1;
        DBuf<unsigned long long> d_lcnt;
        DBuf<DRow> d_rows_tmp;
        DBuf<DEdge> d_edges_tmp;
        DBuf<uint32_t> d_cand_ovf, d_gc_off, d_gc_cnt, d_gcount, d_defer;
        DBuf<uint64_t> d_gscan, d_mscan, d_mkey, d_tmask, d_mbig;
        DBuf<uint32_t> d_mcnt, d_mcur;
        // (gene, sample) seed passes too big for LDS, and their global scratch
        DBuf<uint64_t> d_big_out, d_big_list, d_big_retry;
        DBuf<LSeed> d_big_seeds;
        DBuf<uint32_t> d_big_seg;
        DBuf<uint8_t> d_big_segT;
        DBuf<uint32_t> d_cnt4;   // 4 * (n_items + 1)
    };
    Work work;

    // What analysis.hip alone owns. The per-component tables (components.hip)
    // are built by the first call that needs them after a graph phase and
    // dropped by the next one (do_graph clears comp_valid): rank of each gene's
    // ideal[] prefix, members [C][S], sums [C][P] and their 32-bit copy.
    // rc_trim keeps all of it.
    struct __attribute__((visibility("hidden"))) Analysis {
        bool comp_valid = false;
        uint64_t comp_n = 0, comp_max_cell = 0;
        uint32_t comp_S = 0;
        DBuf<uint32_t> d_crank, d_cmember;
        DBuf<unsigned long long> d_cnum, d_cden, d_cstat, d_rnum, d_rden;
        DBuf<uint2> d_ccell;
        DBuf<uint16_t> d_rweight;
        // The census of every component (build_census, with a validity flag of
        // its own: whatever clears comp_valid clears census_valid too): the
        // rows [K] root, nodes, edges, samples and the members [present genes]
        bool census_valid = false;
        uint64_t census_n = 0, census_members = 0;
        DBuf<uint32_t> d_zroot, d_znodes, d_zedges, d_zsamples, d_zmember;
        // neighbour joining (nj.hip): input matrices of rc_nj, the trees, the
        // reference splits with their support (n_ref counters, then n_valid) and
        // the workspace of the trees too large for LDS
        DBuf<double> d_nj_in, d_nj_len, d_nj_wsm;
        DBuf<int32_t> d_nj_joins;
        DBuf<uint64_t> d_nj_splits, d_nj_ref, d_nj_wsmask;
        DBuf<uint8_t> d_nj_valid;
        DBuf<uint32_t> d_nj_sup;
        // The trees that d_nj_splits / d_nj_valid hold (nj_device; nj_n == 0:
        // none yet) and the census of their splits (splits.hip), built by the
        // first rc_split_census / rc_tree_rf after them and dropped by the next
        // nj_device: the hash table, per instance the rank of its flat index
        // among the class representatives and its class id, per class the
        // count and the first instance.
        int32_t nj_rep = 0, nj_n = 0;
        uint32_t nj_nvalid = 0;
        bool split_valid = false;
        uint64_t split_K = 0, split_slots = 0;
        DBuf<uint32_t> d_sp_table, d_sp_rank, d_sp_count, d_sp_first, d_rf_ref, d_rf_pair;
        DBuf<int32_t> d_sp_ids;
        DBuf<uint64_t> d_sp_out;
        DBuf<uint8_t> d_sp_isref;
        // principal coordinates (pcoa.hip): input matrices of rc_pcoa, the results
        // and the status words (invalid, unconverged replicates)
        DBuf<double> d_pcoa_in, d_pcoa_val, d_pcoa_vec;
        DBuf<int32_t> d_pcoa_sweeps;
        DBuf<uint8_t> d_pcoa_valid;
        DBuf<unsigned int> d_pcoa_stat;
        // group tests (groups.hip): input matrices of rc_group_test, the observed
        // and permuted labels (one byte each), ANOSIM's twice-ranks and the results
        DBuf<double> d_gt_in, d_gt_stat, d_gt_total, d_gt_within, d_gt_perm;
        DBuf<uint8_t> d_gt_labels, d_gt_valid;
        DBuf<uint32_t> d_gt_rank, d_gt_nge;
        // PERMDISP (dispersion.hip) shares the group tests' buffers; the observed distances to the centroids
        DBuf<double> d_gt_dist;
        // the Mantel test (mantel.hip): input matrices of rc_mantel, Y as the kernel reads it (centred doubles
        // or twice-ranks) with its raw upload and validity, the permutations (one byte each), X's twice-ranks
        // and the results (counts: >=, <=, |.| >= |.|, n_rep each)
        DBuf<double> d_mt_in, d_mt_y, d_mt_stat, d_mt_perm;
        DBuf<uint8_t> d_mt_perms, d_mt_valid, d_mt_yvalid;
        DBuf<uint32_t> d_mt_rank, d_mt_yrank, d_mt_counts;
    };
    Analysis an;

    // device buffers, resident from upload (rc_add_sample, upload,
    // rc_set_dust_masks): they live as long as the samples
    DBuf<uint8_t> d_ascii;
    DBuf<uint64_t> d_tx_rel, d_kpre;   // per transcript: start in its sample,
                                       // 16-mer slots of its sample's transcripts before it
    DBuf<TxInfo> d_tx;
    DBuf<IsoRec> d_giso;
    DBuf<uint32_t> d_tx_gene, d_gene_tx_off, d_gene_tx, d_sample_gene_begin, d_sample_tx_begin;
    DBuf<int32_t> d_gene_sample;
    DBuf<uint64_t> d_dust_imp;
    DBuf<int32_t> d_thr, d_bits10;
    DBuf<uint32_t> d_tx_pos, d_iso_pre;
    DBuf<uint32_t> d_pair_item_begin;
    DBuf<int32_t> d_pair_a, d_pair_b, d_pair_index;

    // device buffers, results of a finished run (rc_trim keeps them)
    DBuf<DHsp> d_hsp;
    DBuf<uint32_t> d_grp_off, d_grp_cnt;
    DBuf<uint64_t> d_off4;   // 4 * (n_items + 1)
    DBuf<DRow> d_rows;
    DBuf<DEdge> d_edges;
    DBuf<uint32_t> d_parent, d_present, d_cnodes, d_cedges, d_sample_present;
    DBuf<uint8_t> d_ideal;
    DBuf<unsigned long long> d_stats, d_num, d_den, d_num_all, d_den_all;

    // device buffers, shared scratch: small, or reused by the result and
    // analysis calls (d_iso_list, d_iso_list_r, d_shard_cnt, d_shard_prefix and
    // d_count are rc_align's alone, yet rc_trim keeps them)
    DBuf<uint32_t> d_iso_list, d_iso_list_r;
    DBuf<unsigned long long> d_shard_cnt, d_shard_prefix;
    DBuf<unsigned long long> d_count;
    DBuf<unsigned int> d_status;
    DBuf<DHsp> d_gather;
    DBuf<int32_t> d_order;
    DBuf<double> d_dist;

    // host results
    std::vector<unsigned long long> h_num, h_den, h_num_all, h_den_all, h_stats;
    std::vector<double> h_ss;   // search space of a query of length L against sample T: [T][L]
    std::vector<double> h_exp;  // exp(-lambda * S / 2) per raw score in half units S (stats::evalue's factor)
    rc_timing tm{};
    hipEvent_t ev[EV_N] = {};
    hipEvent_t evd[EVD_N] = {};

    ~rc_engine()
    {
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t x : evd)
            if (x) (void)hipEventDestroy(x);
        if (st2) (void)hipStreamDestroy(st2);
        if (st) (void)hipStreamDestroy(st);
    }
};

static int set_device(rc_engine *e) { HIPCHK(hipSetDevice(e->o.device)); return RC_OK; }

static double wall_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the alignment's blocking waits on the engine's stream (rc_timing.host_wait_ms)
static int wait_st(rc_engine *e)
{
    const double t0 = wall_ms();
    HIPCHK(hipStreamSynchronize(e->st));
    e->tm.host_wait_ms += wall_ms() - t0;
    return RC_OK;
}

static double ev_ms(rc_engine *e, int a, int b)
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, e->ev[a], e->ev[b]) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return ms;
}
