// The host entry points of the kernel files: every non-static host function
// that kernels.hip, components.hip, nj.hip, splits.hip, pcoa.hip, groups.hip, dispersion.hip, mantel.hip, sort.hip,
// seed.hip, align.hip, rows.hip, finish.hip, extend.hip, group.hip and dust.hip define,
// one section per unit, declared here and nowhere else. The defining files
// include this header too, so a definition whose return type drifts from its
// declaration does not compile.
#pragma once
#include "device.h"

#include <functional>

namespace rcg {
// kernels.hip
void launch_pack(const uint8_t *, uint64_t, uint64_t, uint64_t *, uint64_t *, uint64_t *, uint64_t *, hipStream_t);
void launch_kmer_count(const TxInfo *, uint32_t, const uint64_t *, uint64_t *, hipStream_t);
void launch_kmer_fill(bool, const TxInfo *, uint32_t, const uint64_t *, const uint64_t *, const uint64_t *,
                      uint64_t *, hipStream_t);
void launch_bucket_fill(const uint64_t *, uint64_t, int, uint32_t *, hipStream_t);
void launch_tx_masked(const TxInfo *, uint32_t, const uint64_t *, uint8_t *, hipStream_t);
void launch_edge_check(const DEdge *, uint64_t, uint32_t, uint64_t, unsigned int *, hipStream_t);
void launch_edge_key(const DEdge *, uint64_t, const uint32_t *, uint32_t *, uint32_t *, hipStream_t);
void launch_edge_gather(const DEdge *, const uint32_t *, uint64_t, DEdge *, hipStream_t);
void launch_edge_uv(const DEdge *, const uint32_t *, const uint32_t *, uint64_t, uint32_t *, uint32_t *, uint64_t *,
                    hipStream_t);
void launch_tile_tables(const TileSeg *, uint32_t, uint32_t, const uint64_t *, const uint64_t *, TxInfo *, TxInfo *,
                        uint32_t *, TxInfo *, uint64_t *, uint32_t, uint64_t, uint64_t *, IsoRec *, uint64_t,
                        const uint64_t *, PosTx *, uint64_t, hipStream_t);
void launch_near_fill(bool, const TxInfo *, uint32_t, const uint8_t *, const uint64_t *, const uint64_t *,
                      const uint64_t *, uint64_t *, uint64_t, unsigned long long *, int, hipStream_t);
void launch_rbh(const RbhParams &, int, hipStream_t);
void launch_hkey(const DHsp *h, uint64_t n, const uint32_t *tx_gene, HKey *out, hipStream_t st);
void launch_rbh_place(const RbhParams &, hipStream_t);
void launch_gather_rows(const DHsp *, const DRow *, uint64_t, DHsp *, hipStream_t);
void launch_cc(const DEdge *, uint64_t, uint32_t, const int32_t *, int, int, uint32_t *, uint32_t *, uint32_t *,
               uint32_t *, uint32_t *, uint8_t *, unsigned long long *, hipStream_t);
void launch_pair_sums(const DEdge *, uint64_t, const uint32_t *, const uint8_t *, unsigned long long *,
                      unsigned long long *, unsigned long long *, unsigned long long *, hipStream_t);
void launch_distance(const unsigned long long *, const unsigned long long *, const int32_t *, const int32_t *,
                     int, int, double *, unsigned int *, hipStream_t);
// components.hip
void launch_comp_keys(const uint32_t *, const uint32_t *, const uint8_t *, const uint32_t *, uint32_t, uint64_t *,
                      unsigned long long *, hipStream_t);
void launch_comp_members(const uint64_t *, uint64_t, uint32_t, uint32_t *, unsigned long long *, hipStream_t);
void launch_comp_sums(const DEdge *, uint64_t, const uint32_t *, const uint8_t *, const uint32_t *, uint64_t,
                      unsigned long long *, unsigned long long *, hipStream_t);
void launch_comp_pack(const unsigned long long *, const unsigned long long *, uint64_t, uint2 *, unsigned long long *,
                      hipStream_t);
bool launch_resample(const uint2 *, const uint16_t *, uint64_t, uint64_t, uint32_t, unsigned long long *,
                     unsigned long long *, hipStream_t);
void launch_resample_distance(const unsigned long long *, const unsigned long long *, const int32_t *, const int32_t *,
                              int, int, uint64_t, uint64_t, double *, unsigned int *, hipStream_t);
void launch_census_flags(const uint32_t *, const uint32_t *, uint32_t, uint32_t *, hipStream_t);
void launch_census_keys(const uint32_t *, const uint32_t *, const uint32_t *, uint32_t, uint64_t *,
                        unsigned long long *, hipStream_t);
void launch_census_table(const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint32_t, uint32_t *,
                         uint32_t *, uint32_t *, uint32_t *, hipStream_t);
void launch_census_members(const uint64_t *, uint64_t, const int32_t *, uint32_t *, uint32_t *, hipStream_t);
// nj.hip
size_t nj_lds_bytes(bool, int, int);
hipError_t launch_nj(bool, const double *, int, int, int, double *, uint64_t *, int32_t *, double *, uint64_t *,
                     uint8_t *, hipStream_t);
void launch_nj_support(const uint64_t *, int, const uint64_t *, const uint8_t *, int, int, int, uint32_t *, uint32_t *,
                       hipStream_t);
// splits.hip
uint64_t split_table_slots(uint64_t);
void launch_split_insert(const uint64_t *, const uint8_t *, uint32_t, uint32_t, int, uint32_t *, uint64_t, hipStream_t);
void launch_split_lookup(const uint64_t *, const uint8_t *, uint32_t, uint32_t, int, const uint32_t *, uint64_t,
                         uint32_t *, uint32_t *, hipStream_t);
void launch_split_ids(const uint32_t *, const uint32_t *, uint32_t, int32_t *, uint32_t *, uint32_t *, hipStream_t);
void launch_split_gather(const uint64_t *, const uint32_t *, uint64_t, int, uint64_t *, hipStream_t);
void launch_split_ref(const uint64_t *, int, const uint64_t *, int, const uint32_t *, uint64_t, const uint32_t *,
                      uint8_t *, hipStream_t);
void launch_rf_ref(const int32_t *, const uint8_t *, const uint8_t *, uint32_t, uint32_t, uint32_t, uint32_t *,
                   hipStream_t);
void launch_rf_pairs(const int32_t *, const uint8_t *, uint32_t, uint32_t, uint32_t *, hipStream_t);
// pcoa.hip
int pcoa_ld(int);
size_t pcoa_lds_bytes(int);
hipError_t launch_pcoa(const double *, int, int, int, int, double *, double *, int32_t *, uint8_t *, unsigned int *,
                       hipStream_t);
// groups.hip
enum { GROUP_PERMANOVA = 0, GROUP_ANOSIM = 1 };   // rcgpu.h: RC_GROUP_PERMANOVA, RC_GROUP_ANOSIM
enum { GROUP_PERM_CHUNK = 120 };                  // permutations per workgroup
size_t group_lds_bytes(int, int);
size_t group_rank_lds_bytes(int);
hipError_t launch_group_rank(const double *, int, int, uint32_t *, uint8_t *, hipStream_t);
hipError_t launch_group_test(int, const void *, const uint8_t *, int, int, int, uint32_t, const uint8_t *,
                             const uint8_t *, int, double *, uint32_t *, double *, double *, double *, uint8_t *,
                             hipStream_t);
// dispersion.hip
enum { DISP_PERM_CHUNK = 124 };                   // permutations per workgroup
size_t dispersion_lds_bytes(int);
hipError_t launch_dispersion(const double *, int, int, int, const uint8_t *, const uint8_t *, int, double *, uint32_t *,
                             double *, double *, double *, double *, uint8_t *, hipStream_t);
// mantel.hip
enum { MANTEL_PEARSON = 0, MANTEL_SPEARMAN = 1 };   // rcgpu.h: RC_MANTEL_PEARSON, RC_MANTEL_SPEARMAN
enum { MANTEL_PERM_CHUNK = 124 };                   // permutations per workgroup
size_t mantel_lds_bytes(int, int);
void mantel_prepare_y(const double *, int, double *, double *, int *);
hipError_t launch_mantel(int, const void *, const uint8_t *, int, int, const void *, double, int, const uint8_t *, int,
                         double *, uint32_t *, uint32_t *, uint32_t *, double *, uint8_t *, hipStream_t);
// sort.hip
uint64_t os_status_words(uint64_t n);
uint64_t os_scratch_words(uint64_t n);
uint64_t os_gen_tile_words(uint64_t n);
bool os_sort_keys(uint64_t *keys, uint64_t *alt, uint64_t n, int bb, uint32_t *scratch, uint64_t *status,
                  uint32_t &epoch, hipStream_t st, const std::function<void()> &after_prep, bool counted,
                  const TxInfo *gen_tx, const uint64_t *gen_koff, const uint64_t *gen_F, uint32_t gen_ntx,
                  uint32_t *gen_tile);
void os_fill_hist(const TxInfo *tx, uint32_t n_tx, const uint64_t *F, const uint64_t *koff, uint64_t *ent,
                  uint64_t n, uint32_t *scratch, hipStream_t st);
uint32_t os_index_cap(uint32_t cap);
int os_index_gbits(uint64_t n, int bits, uint32_t cap);
uint64_t os_index_status_words(uint64_t n);
uint64_t os_index_scratch_words(uint64_t n);
uint64_t os_index_offset_words(int G);
uint64_t os_index_list_words();
void os_index_fill_hist(const TxInfo *tx, uint32_t n_tx, const uint64_t *F, const uint64_t *koff, uint64_t *ent,
                        uint64_t n, int G, uint32_t *scratch, hipStream_t st);
int os_index_sort(uint64_t *keys, uint64_t *alt, uint64_t n, int G, int bits, uint32_t cap, uint32_t *scratch,
                  uint64_t *status, uint32_t &epoch, uint32_t *offsets, uint32_t *list, uint32_t *bucket,
                  hipStream_t st, bool counted, const std::function<bool()> &wait, uint32_t *fb_ranges,
                  uint64_t *fb_keys, bool *whole);
// seed.hip
void launch_seed(bool, const Db &, const Index &, const SeedParams &, hipStream_t);
void launch_seed_big(bool, const Db &, const Index &, const SeedParams &, uint32_t, hipStream_t);
void launch_rs_range(const uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t *, hipStream_t);
// align.hip (the pass order of the extension, over the four units below)
void launch_extend_rows(bool, const Db &, const ExtParams &, hipStream_t);
void launch_later_rounds(bool, const Db &, const ExtParams &, bool, const LaterParams &, Cand *const[2],
                         uint32_t *const[2], int32_t *const[2], uint32_t *const[2], unsigned long long *, hipStream_t);
// rows.hip
void launch_rows(int rw, bool save, bool amb, const Db &, const ExtParams &, hipStream_t);
int row_slot_words_max(bool amb);
// finish.hip
void launch_first_finish(const ExtParams &, hipStream_t);
void launch_later_round(const ExtParams &, const LaterParams &, hipStream_t);
void launch_later_finish(const ExtParams &, const LaterParams &, hipStream_t);
// extend.hip
void launch_extend_retry(bool, const Db &, const ExtParams &, hipStream_t);
// group.hip
enum GroupPass { GROUP_DIRECT_COUNT, GROUP_DIRECT_WRITE, GROUP_MIRROR_COUNT, GROUP_MIRROR_SCATTER, GROUP_MIRROR_SORT };
void launch_group(const GroupParams &, GroupPass, hipStream_t);
// dust.hip
void launch_dust(bool, uint64_t, uint64_t, const uint64_t *, const uint64_t *, const uint64_t *, const TxInfo *, uint32_t, int,
                 int, int, uint32_t *, uint64_t *, uint32_t, uint64_t *, hipStream_t);
uint32_t dust_scratch_words(uint32_t);
uint64_t dust_event_words(uint32_t);
}  // namespace rcg
