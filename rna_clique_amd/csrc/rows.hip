// The row kernels of the extension (the pass order: align.hip):
//
//   extend_rows_kernel   each candidate's first seed on a sliding 32-lane
//                        sub-band row (two rows per wave), greedy X-drop; the
//                        64-lane instantiation continues what outgrew it.
//
// Host entry points: launch_rows, row_slot_words_max.
//
// Semantics: oracle/align_oracle.c ("RC-megablast v1"), bit for bit.
#include "align_common.h"
#include "launch.h"

#include <climits>
#include <cstdio>
#include <cstdlib>

namespace rcg {

// ------------------------------------------------------------------------
// extension, two candidates per wave: one 32-lane row per candidate (and the
// 64-lane rows, one candidate per wave, for what outgrows them)
// ------------------------------------------------------------------------
//
// The greedy frontier of a near-identical transcript pair stays within a few
// diagonals of the seed's, so most of the 64-diagonal band of extend_kernel is
// dead lanes. Here each row of RW lanes (32: half a wave, 64: the whole wave;
// the RW == 16 branches of the helpers, one DPP row, are not instantiated)
// runs its own candidate over the sub-band of diagonals [-RW/2, RW/2 - 1]
// (row lane rl <-> diagonal rl - RW/2). The sub-band computes exactly what the
// full band computes as long as no live diagonal reaches its edge lanes (a
// diagonal outside can only be entered from a live neighbour); the first time
// an edge lane is live while the extension continues, the candidate is handed
// to extend_kernel (list mode) whole. Rows advance independently (their own
// seeds, extensions, candidates): a row that finishes an extension does its
// bookkeeping while the other rows wait one transition, then all rows step
// together. Every extension walks forward: a left extension runs on reversed
// copies of both transcripts staged next to the forward ones.

#ifndef ROW_MIN_WAVES
#define ROW_MIN_WAVES 8   // r05_zn/zo: 8 beats 7 (C3 rows 84.1 -> 82.7 ms, C4 459 -> 450) and 6 (87.5); r02/r04: 7 was best then
#endif

// max over the 16 lanes of each DPP row, in every lane of the row
__device__ __forceinline__ int row_max(int v)
{
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, false));  // row_mirror
    return v;
}

// lane rl <- rl - 1 inside the row (rl 0 gets `edge`). Rows wider than a DPP
// row shift the whole wave: lane 0 keeps `edge` (FIX) or reads 0, and the
// first lane of the upper half-wave reads the last lane of the lower one.
// The frontier (FIX) relies on that lane being dead (-1 = edge) whenever a
// step starts: a live sub-band edge lane ends its row's extension (abort or
// done), every extension starts with only the seed diagonal live, and a row
// without work sets its lanes dead. Values other than the frontier are only
// read where the frontier neighbour is live.
template <int RW, bool FIX>
__device__ __forceinline__ int rw_from_lower(int v, int edge, int rl)
{
    if constexpr (RW == 16) {
        return __builtin_amdgcn_update_dpp(edge, v, 0x111, 0xF, 0xF, false);   // row_shr:1
    } else if constexpr (FIX) {
        return __builtin_amdgcn_update_dpp(edge, v, 0x138, 0xF, 0xF, false);   // wave_shr:1
    } else {
        return __builtin_amdgcn_mov_dpp(v, 0x138, 0xF, 0xF, true);             // edge is 0
    }
}
// lane rl <- rl + 1 inside the row (rl RW - 1 gets `edge`; as above)
template <int RW, bool FIX>
__device__ __forceinline__ int rw_from_upper(int v, int edge, int rl)
{
    if constexpr (RW == 16) {
        return __builtin_amdgcn_update_dpp(edge, v, 0x101, 0xF, 0xF, false);   // row_shl:1
    } else if constexpr (FIX) {
        return __builtin_amdgcn_update_dpp(edge, v, 0x130, 0xF, 0xF, false);   // wave_shl:1
    } else {
        return __builtin_amdgcn_mov_dpp(v, 0x130, 0xF, 0xF, true);             // edge is 0
    }
}
// max over the row, in every lane of the row
template <int RW>
__device__ __forceinline__ int rw_max(int v)
{
    v = row_max(v);
    if constexpr (RW >= 32) {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);   // DPP rows 0<->1, 2<->3
        v = max((int)r[0], (int)r[1]);
    }
    if constexpr (RW == 64) {
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);   // the two halves
        v = max((int)r[0], (int)r[1]);
    }
    return v;
}
// the RW bits of this lane's row in a wave mask
template <int RW>
__device__ __forceinline__ uint32_t rw_mask(uint64_t m, int row)
{
    if constexpr (RW == 64) return (uint32_t)m;   // (callers take the low half only)
    return (uint32_t)(m >> (RW * row)) & (RW == 32 ? 0xFFFFFFFFu : 0xFFFFu);
}

// x != 0 ? ~0 : 0 on a wave-uniform value, kept in scalar registers
__device__ __forceinline__ uint32_t s_nonzero(uint32_t x)
{
    uint32_t r;
    asm volatile("s_cmp_lg_u32 %1, 0\n\ts_cselect_b32 %0, -1, 0" : "=s"(r) : "s"(x) : "scc");
    return r;
}
// lowest set bit of a wave-uniform value (-1 for 0), one scalar instruction
__device__ __forceinline__ int s_ff1(uint32_t x)
{
    int r;
    asm volatile("s_ff1_i32_b32 %0, %1" : "=s"(r) : "s"(x));
    return r;
}
// lane masks of single compares (one v_cmp each, combined in scalar registers)
__device__ __forceinline__ uint64_t m_gt(int a, int b) { return __builtin_amdgcn_ballot_w64(a > b); }
__device__ __forceinline__ uint64_t m_ge(int a, int b) { return __builtin_amdgcn_ballot_w64(a >= b); }
__device__ __forceinline__ uint64_t m_lt(int a, int b) { return __builtin_amdgcn_ballot_w64(a < b); }
__device__ __forceinline__ uint64_t m_eq(int a, int b) { return __builtin_amdgcn_ballot_w64(a == b); }
// lane mask of a condition (the HIP __ballot goes through an int and two extra vector ops)
__device__ __forceinline__ uint64_t ballot(bool b) { return __builtin_amdgcn_ballot_w64(b); }

// spread a wave mask to whole rows: every lane of a row with a set lane (scalar work)
template <int RW>
__device__ __forceinline__ uint64_t rw_spread(uint64_t m)
{
    if constexpr (RW == 32) {   // per 32-bit half, scalar ops (the compiler turns a test of the high half into a vector compare)
        const uint32_t lo = s_nonzero((uint32_t)m), hi = s_nonzero((uint32_t)(m >> 32));
        return (uint64_t)lo | ((uint64_t)hi << 32);
    } else if constexpr (RW == 64) {
        const uint32_t a = s_nonzero((uint32_t)m | (uint32_t)(m >> 32));
        return (uint64_t)a | ((uint64_t)a << 32);
    } else {
        uint64_t r = 0;
        for (int i = 0; i < 4; i++)
            if ((m >> (16 * i)) & 0xFFFFull) r |= 0xFFFFull << (16 * i);
        return r;
    }
}
// lane in mask ? a : b, one v_cndmask with the mask as the SGPR-pair condition
__device__ __forceinline__ int lane_sel(uint64_t m, int a, int b)
{
    int r;
    asm("v_cndmask_b32_e64 %0, %2, %1, %3" : "=v"(r) : "v"(a), "v"(b), "s"(m));
    return r;
}

// 32-base windows of the row kernel's staging at absolute LDS base positions
// (4 bases per byte of LDS address): three dword reads and two v_alignbit
// each. The reads are one asm block so that the address is the position's
// dword and nothing else (through a pointer the compiler adds the staging's
// LDS symbol to every address); the block waits for its own reads.
__device__ __forceinline__ uint64_t lds_join(uint64_t w01, uint32_t w2, uint32_t p)
{
    const uint32_t w0 = (uint32_t)w01, w1 = (uint32_t)(w01 >> 32);
    const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, p * 2u), hi = __builtin_amdgcn_alignbit(w2, w1, p * 2u);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ void lds_win2(uint32_t pa, uint32_t pb, uint64_t &wa, uint64_t &wb)
{
    const uint32_t aa = (pa >> 2) & ~3u, ab = (pb >> 2) & ~3u;
    uint64_t a01, b01;
    uint32_t a2, b2;
    asm volatile("ds_read2_b32 %0, %4 offset1:1\n\t"
                 "ds_read_b32 %1, %4 offset:8\n\t"
                 "ds_read2_b32 %2, %5 offset1:1\n\t"
                 "ds_read_b32 %3, %5 offset:8\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(a01), "=&v"(a2), "=&v"(b01), "=&v"(b2)
                 : "v"(aa), "v"(ab));
    wa = lds_join(a01, a2, pa);
    wb = lds_join(b01, b2, pb);
}
__device__ __forceinline__ uint64_t lds_diff(uint32_t pa, uint32_t pb)
{
    uint64_t a, b;
    lds_win2(pa, pb, a, b);
    return a ^ b;
}

// lane in mask ? K : b, K an inline constant (no register for it)
template <int K>
__device__ __forceinline__ int lane_sel_k(uint64_t m, int b)
{
    int r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "i"(K), "s"(m));
    return r;
}

// 32 bases of each side from the dwords at byte addresses a, b holding the
// bases at LDS base positions pa, pb (+ a multiple of 16): three dword reads
// and two funnel shifts per side
__device__ __forceinline__ void lds_pair_at(uint32_t a, uint32_t b, uint32_t pa, uint32_t pb, uint64_t &wa,
                                            uint64_t &wb)
{
    uint64_t a01, b01;
    uint32_t a2, b2;
    asm volatile("ds_read2_b32 %0, %4 offset1:1\n\t"
                 "ds_read_b32 %1, %4 offset:8\n\t"
                 "ds_read2_b32 %2, %5 offset1:1\n\t"
                 "ds_read_b32 %3, %5 offset:8\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(a01), "=&v"(a2), "=&v"(b01), "=&v"(b2)
                 : "v"(a), "v"(b));
    wa = lds_join(a01, a2, pa);
    wb = lds_join(b01, b2, pb);
}

// Matching bases from (pa, pb) forward, at most maxn (>= 0); positions are
// absolute LDS base positions (lds_win2); masks (AMB) sit `moff` bases
// further on. Reads bases up to pa + max(maxn, 1) + 47 (WIN_MARGIN).
template <bool AMB>
__device__ __forceinline__ int slide_fwd(uint32_t pa, uint32_t pb, int maxn, uint32_t moff)
{
    // the first window outside any loop (a mismatch within 32 bases is the
    // common case); lanes on a run of 32+ matches go on in the loop, whose
    // dword addresses advance by 8 bytes per 32 bases (the shifts stay)
    uint64_t x = lds_diff(pa, pb);
    if (AMB) {
        uint64_t ma, mb;
        lds_win2(pa + moff, pb + moff, ma, mb);
        x |= ma | mb;
    }
    int n = x ? (int)(__builtin_ctzll(x) >> 1) : 32;
    // the loop is wave-uniform (a ballot per round): lanes whose run ended
    // keep their count and stop advancing; no exec-mask bookkeeping per round
    // (the dword addresses follow n: a stopped lane re-reads its last window)
    bool go = n == 32 && maxn > 32;
    if (__builtin_amdgcn_ballot_w64(go)) {
        const uint32_t a0 = ((pa + 32u) >> 2) & ~3u, b0 = ((pb + 32u) >> 2) & ~3u;
        do {
            const uint32_t o = ((uint32_t)(n - 32) >> 2) & ~7u;
            uint64_t wa, wb;
            lds_pair_at(a0 + o, b0 + o, pa, pb, wa, wb);
            x = wa ^ wb;
            if (AMB) {
                lds_pair_at(a0 + o + moff / 4u, b0 + o + moff / 4u, pa, pb, wa, wb);
                x |= wa | wb;
            }
            const int k = x ? (int)(__builtin_ctzll(x) >> 1) : 32;
            n = go ? n + k : n;
            go = go && k == 32 && n < maxn;
        } while (__builtin_amdgcn_ballot_w64(go));
    }
    return min(n, maxn);
}

// per-row bookkeeping in LDS: the candidate record (CAND_DWORDS dwords) and state
enum { RM_REC = 0, RM_CLO = CAND_DWORDS, RM_CHI, RM_QB, RM_TB, RM_X, RM_Y, RM_LEN,
       RM_RSC, RM_RI, RM_RJ, RM_RD, RM_RGO,
       RM_PHASE,                                  // the running extension's done action (A_RDONE / A_LDONE)
       RM_KOF,                                    // the window's diagonal offset (sliding sub-band)
       RM_PWI, RM_PWG, RM_PWD, RM_PK,             // the row's best record parked by a window slide, its diagonal
       RM_N };   // (its size is part of the row kernel's tuning: 3 more fields cost 4 VGPR spills)
// the step count and best score of an extension that outgrew the window, kept
// (SAVE kernel) in record fields the row kernel does not read (the seed
// count's high half, the padding)
enum { RM_AD6 = RM_REC + 9, RM_ABEST = RM_REC + 11 };
// a saved extension (ExtParams::resume, RES_REC ints): the bookkeeping
// RM_RSC .. RM_PK, the step count, the best score, then the window's frontier
// R and gap states
enum { RES_RSC = 0, RES_PHASE = RM_PHASE - RM_RSC, RES_KOF = RM_KOF - RM_RSC, RES_PWI = RM_PWI - RM_RSC,
       RES_PWG = RM_PWG - RM_RSC, RES_PWD = RM_PWD - RM_RSC, RES_PK = RM_PK - RM_RSC, RES_D6 = RES_PK + 1,
       RES_BEST = RES_PK + 2, RES_R = 16, RES_G = 48 };
static_assert(RES_BEST < RES_R && RES_G + 32 <= RES_REC, "resume record layout");
// fields of the record (dword offsets, layout of Cand)
enum { RC_SOFF = 0, RC_QTX = 1, RC_STX = 2, RC_CNT_STRAND = 3, RC_Q0 = 4, RC_S0 = 5, RC_LQ = 6, RC_LT = 7,
       RC_SAMS = 8, RC_SEEDHI = 9, RC_E01 = 10, RC_PAD1 = 11 };
// work cursors of a row
enum { RS_LEND, RS_SHARD, RS_SHN, RS_N };
// row actions (transition actions < A_DONE; extending: A_STEP_R / A_STEP_L = their done action + 4)
enum { A_FETCH, A_SLIDE, A_RDONE, A_LDONE, A_ABORT, A_DONE, A_STEP_R, A_STEP_L };
// bl of a row whose best record is parked in its LDS bookkeeping (a window slide)
constexpr int BL_PARKED = -64;
// The row kernel's arguments, one struct so that the kernarg segment is laid
// out as it.
struct RowArgs {
    Db db;
    ExtParams P;
};
using RowArgsK = const __attribute__((address_space(4))) RowArgs *;
// The kernarg pointer behind an opaque copy: the fields read through it are
// loaded (s_load, scalar cache) where the transitions use them instead of
// being held in SGPRs across the step loop, where ~30 SGPRs of pointers
// spilled into VGPR lanes and cost readlane/writelane pairs every step.
__device__ __forceinline__ RowArgsK row_args()
{
    RowArgsK p = (RowArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// per-row state that only transitions touch (row kernel LDS)
struct RowLds {
    int meta[RM_N];
    int st[RS_N];
};
// Windowed staging (WIN): a row's four staging slots (0: query forward, 1:
// subject forward, 2: query reverse complement, 3: subject reverse
// complement) hold windows of sw words of the packed tile arrays; the running
// extension walks slot a against slot b. Per row: the global base of the
// extension's start on each side (a: offset ni = 0, b: j = ni - diagonal =
// 0), the side's array (bit 0: 0 = F, 1 = RC) and slot (bits 1-2), the
// window's [lo, lim] in extension offsets, and the first word of each slot.
enum { WM_GA0, WM_GB0, WM_AARR, WM_BARR, WM_ALO, WM_ALIM, WM_BLO, WM_BLIM, WM_W0, WM_N = WM_W0 + 4 };
struct RowWin {
    int w[WM_N];
};
// LDS of a row-kernel block: staging (2 guard words + rows x arrays x sw
// words), shard prefix, rows' bookkeeping (+ window bookkeeping), 8 block counters
__host__ __device__ constexpr size_t row_lds_bytes(int rw, int na, int sw, bool win = false)
{
    return ((size_t)(EBLOCK / rw) * na * sw + 2) * 8 + (NSHARD + 1) * 8 + (size_t)(EBLOCK / rw) * sizeof(RowLds) + 32 +
           (win ? (size_t)(EBLOCK / rw) * sizeof(RowWin) : 0);
}
// windowed slot limits: a slide from offset ni with at most mw bases reads
// bases up to ni + max(mw, 1) + 47 (slide_fwd: three dwords from the dword
// holding the last window's start)
constexpr int WIN_MARGIN = 48;

// Extension of every candidate's FIRST seed (its smallest (x, y): always
// extended, RC-megablast spec 3) to the right and to the left. Anything
// further -- the other seeds' containment, more HSPs, purge, e-values -- is
// first_finish_kernel's; a candidate that needs more than its first seed goes
// to extend_kernel whole.
// Sliding sub-band: a row's RW lanes are the diagonals [kof - RW/2, kof +
// RW/2 - 1] of the spec's 64-diagonal band, kof = 0 when an extension starts.
// When a live lane reaches the window's edge, the window slides so that the
// live diagonals are centred (|kof| <= 31 - RW/2: its edges never meet the
// band's, so the edge lanes stay dead at every step start, as the half-wave
// seam of the frontier shifts needs); the lanes entering it are diagonals no
// live lane has reached (an outside diagonal can only come alive from a live
// edge lane, which slides first), so the extension stays exact. Only a live
// span wider than the window, or one reaching past the band's +-31, goes to
// the one-wave full-band kernel (indels: C3v).
// SAVE (32-lane rows): an extension that outgrows the window is saved for the
// 64-lane pass to continue (a separate instantiation: the save code's
// registers cost the plain kernel 7 % at C3, where nearly nothing overflows).
// WIN: transcripts longer than the staging slot -- each slot holds a window
// of the sequence from the extension's start, refilled from HBM when a
// slide would read past it (or a lane's position lies before it); the
// refill places the window at the lowest position still to be read, so the
// extension is the same as with the whole transcripts staged.
template <bool AMB, int RW, int MINW, bool SAVE = false, bool WIN = false>
__global__ __launch_bounds__(EBLOCK, MINW) void extend_rows_kernel(RowArgs)
{
    constexpr int RROWS = EBLOCK / RW;   // rows per block
    constexpr int RC0 = RW / 2;          // row lane of diagonal 0
    constexpr int NA = AMB ? 8 : 4;      // staged arrays per row: Q, T (raw words), Qrev, Trev (+ masks)
    constexpr int EBIT = 26, OBIT = 13;
    // All of the block's LDS is the dynamic allocation, staging first, so
    // that the staging starts at LDS address 0 and the step loop's window
    // addresses carry no base: [2 guard words][RROWS][NA][sw] staging, then
    // the shard prefix, the rows' bookkeeping and the block counters.
    extern __shared__ uint64_t rstg[];
    const int sw = row_args()->P.dsw;                     // u64 words per staged array
    unsigned long long *const sprefix = reinterpret_cast<unsigned long long *>(rstg + 2 + (size_t)RROWS * NA * sw);
    RowLds *const rows_lds = reinterpret_cast<RowLds *>(sprefix + NSHARD + 1);
    uint32_t *const rcnt = reinterpret_cast<uint32_t *>(rows_lds + RROWS);   // extensions, candidates, overflows
    uint32_t &s_ncand = rcnt[4];
    RowWin *const rows_win = reinterpret_cast<RowWin *>(rcnt + 8);   // (WIN only)
    {
        const RowArgsK K = row_args();
        if (threadIdx.x < 4 || threadIdx.x == 5) rcnt[threadIdx.x] = 0;   // [5]: 6 x row steps
        for (int i = threadIdx.x; i <= NSHARD; i += EBLOCK) sprefix[i] = K->P.shard_prefix[i];
        // list mode: the candidates are P.list[0, *P.list_n) (a previous row
        // kernel's deferrals), else the linear index space over the shards
        if (threadIdx.x == 0) s_ncand = K->P.list ? (uint32_t)*K->P.list_n : (uint32_t)K->P.n_cand;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, rl = lane & (RW - 1), row = lane / RW;
    const int rs = threadIdx.x / RW;                      // row slot in the block
    const int k = rl - RC0;                               // this lane's diagonal
    // two guard words in front (windows read from a word boundary before a position)
    uint64_t *stg = rstg + 2 + (size_t)rs * NA * sw;      // Q, T, Qr, Tr, [QM, TM, QMr, TMr]
    // absolute LDS base position of the row's Q array (the staging's LDS
    // offset: the low half of its generic address)
    const uint32_t base0 = 4u * (uint32_t)reinterpret_cast<uintptr_t>(rstg) + (uint32_t)(2 + rs * NA * sw) * 32u;
    const uint32_t bqr = base0 + 64u * (uint32_t)sw, btr = bqr + 32u * (uint32_t)sw;
    const uint32_t moff = 128u * (uint32_t)sw;
    RowLds &RL = rows_lds[rs];
    int *meta = RL.meta;
    int *const wm = rows_win[rs].w;   // (WIN only)
    const int X = row_args()->P.xdrop;
    // candidates come in chunks from a global counter (P.chunk >= 1); the
    // record of the next one is prefetched (one dword per lane) while the
    // current one is extended
    auto chunk = []() { return (uint32_t)max(row_args()->P.chunk, 1); };
    uint32_t lnx = 0;
    auto grab = [&]() {
        const uint32_t ncand = s_ncand, ch = chunk();
        unsigned long long b = 0;
        if (rl == 0) b = atomicAdd(row_args()->P.work, (unsigned long long)ch);
        b = (unsigned long long)__shfl((long long)b, RW * row);
        lnx = b < ncand ? (uint32_t)b : ncand;
        if (rl == 0) RL.st[RS_LEND] = (int)(lnx + ch);
    };
    // candidate slot of linear index l; the shard cursor (in LDS) only advances
    auto slot = [&](uint32_t l, int which) -> uint64_t {
        int sh = RL.st[which];
        while (sh + 1 < NSHARD && sprefix[sh + 1] <= l) sh++;
        if (rl == 0) RL.st[which] = sh;
        return (uint64_t)sh * row_args()->P.cand_cap + (l - sprefix[sh]);
    };
    auto cslot = [&](uint32_t l, int which) -> uint64_t {
        const uint32_t *list = row_args()->P.list;
        return list ? (uint64_t)list[l] : slot(l, which);
    };
    auto load_rec = [&](uint32_t l) -> int {
        if (l >= s_ncand || rl >= CAND_DWORDS) return 0;
        return reinterpret_cast<const int *>(row_args()->P.cands + cslot(l, RS_SHN))[rl];
    };
    // this pass's first-seed results (shared searches: pass 1 -> cand_box,
    // pass 2 over list2 -> cand_box2)
    auto box_out = []() {
        const RowArgsK K = row_args();
        return K->P.which ? K->P.cand_box2 : K->P.cand_box;
    };
    // row-uniform; extend_kernel takes the candidate whole -- or, shared
    // searches, a sub-band overflow (wide) the 64-lane pass over P.wide next
    // (returns the wide-list entry, row-uniform; ~0 when not listed)
    auto defer = [&](uint64_t ci, bool wide) -> unsigned long long {
        unsigned long long wi2 = ~0ull;
        if (rl == 0) {
            const RowArgsK K = row_args();
            if (!K->P.share) {   // shared searches: first_finish_kernel lists each search on its own
                const unsigned long long di = atomicAdd(K->P.defer_count, 1ull);
                K->P.defer[di] = (uint32_t)ci;
            } else if (wide && K->P.wide) {
                wi2 = atomicAdd(K->P.wide_n, 1ull);
                K->P.wide[wi2] = (uint32_t)ci;
            }
            box_out()[ci * BOX_REC + FX_STATUS] = -1;
        }
        if constexpr (SAVE) return (unsigned long long)__shfl((long long)wi2, RW * row);
        return wi2;
    };
    if (rl == 0) {
        RL.st[RS_SHARD] = 0;
        RL.st[RS_SHN] = 0;
    }
    grab();
    int recv = load_rec(lnx);

    int act = A_FETCH;
    // extension state: frontier (R, gap state), winner record, row-uniform best
    int R = -1, goe = 0, wi = 0, wg = 0, wd = 0, best = 0, bl = RC0, d6 = 0;   // d6 = 6 x greedy step
    uint32_t pa = 0, pb = 0;
    int alen = 0, blen = 0;
    // per-lane forms the step uses (k folded in once per extension):
    // pb - k (b position of diagonal k at a offset 0), blen + k, -(k + d6)
    uint32_t pbk = 0;
    int blk = 0, nkd = 0;
    int mnk = 0;   // min(alen, blk): a step's room along its diagonal is mnk - ni
    bool swap = false;                                    // spec 4b: query = the higher-numbered sample
    int wlo = 0, wlim = 0;                                // WIN: the lane's window [wlo, wlim] in extension offsets

    // ---- windowed staging (WIN) ----
    using GW = const __attribute__((address_space(1))) uint64_t *;
    // a packed tile array: 0 = F, 1 = RC (mask: their ambiguity masks)
    auto warr = [](int arr, bool mask) -> GW {
        const RowArgsK K = row_args();
        GW f = (GW)(mask ? K->db.AF : K->db.F), r = (GW)(mask ? K->db.ARC : K->db.RC);
        asm volatile("" : "+s"(f), "+s"(r));
        return arr ? r : f;
    };
    // LDS base position of a slot's word 0
    auto slot_base = [&](int slot) -> uint32_t { return base0 + 32u * (uint32_t)sw * (uint32_t)slot; };
    // the window of `slot`: words W .. of array arr, at most through word ew
    // (the last one a read of the side's sequence can reach)
    auto win_load = [&](int slot, int arr, uint32_t W, uint32_t ew) {
        const int n = ew >= W ? (int)min((uint32_t)sw, ew - W + 1u) : 0;
        GW src = warr(arr, false) + W;
        uint64_t *dst = stg + (size_t)slot * sw;
        for (int w = rl; w < n; w += RW) dst[w] = src[w];
        if (AMB) {
            GW msrc = warr(arr, true) + W;
            uint64_t *mdst = stg + (size_t)(4 + slot) * sw;
            for (int w = rl; w < n; w += RW) mdst[w] = msrc[w];
        }
    };
    // global start base of each slot's extension: right (slots 0, 1: the
    // forward arrays from the seed's end), left (2, 3: the reverse
    // complements from the seed's start, walked forward); and its sequence end
    auto slot_g = [&](int slot, uint32_t &g, uint32_t &e) {
        const uint32_t total = (uint32_t)row_args()->db.total;
        const uint32_t q0 = (uint32_t)meta[RM_REC + RC_Q0], s0 = (uint32_t)meta[RM_REC + RC_S0];
        const uint32_t Lq = (uint32_t)meta[RM_REC + RC_LQ], Lt = (uint32_t)meta[RM_REC + RC_LT];
        const uint32_t x = (uint32_t)meta[RM_X], y = (uint32_t)meta[RM_Y], len = (uint32_t)meta[RM_LEN];
        if (slot == 0) { g = q0 + x + len; e = q0 + Lq; }
        else if (slot == 1) { g = s0 + y + len; e = s0 + Lt; }
        else if (slot == 2) { g = total - q0 - x; e = total - q0; }
        else { g = total - s0 - y; e = total - s0; }
    };
    auto slot_arr = [&](int slot) -> int {
        const int strand = (meta[RM_REC + RC_CNT_STRAND] >> 16) & 1;
        return slot == 0 ? strand : (slot == 1 ? 0 : (slot == 2 ? 1 - strand : 1));
    };
    // the lane's window from the row's bookkeeping (diagonal kk = k + kof)
    auto win_lane = [&](int kk) {
        wlo = max(wm[WM_ALO], wm[WM_BLO] + kk);
        wlim = min(wm[WM_ALIM], wm[WM_BLIM] + kk);
    };
    // an extension starts (dir 0 right, 1 left): its sides' slots, start
    // bases and windows (as staged); pa, pbk, wlo, wlim of diagonal k
    auto win_begin = [&](int dir) {
        const int qsl = dir ? 2 : 0, tsl = dir ? 3 : 1;
        const int asl = swap ? tsl : qsl, bsl = swap ? qsl : tsl;
        uint32_t ga, gb, ea, eb;
        slot_g(asl, ga, ea);
        slot_g(bsl, gb, eb);
        const uint32_t Wa = (uint32_t)wm[WM_W0 + asl], Wb = (uint32_t)wm[WM_W0 + bsl];
        const int alo = (int)(32u * Wa - ga), blo = (int)(32u * Wb - gb);
        __builtin_amdgcn_wave_barrier();
        if (rl == 0) {
            wm[WM_GA0] = (int)ga;
            wm[WM_GB0] = (int)gb;
            wm[WM_AARR] = slot_arr(asl) | (asl << 1);
            wm[WM_BARR] = slot_arr(bsl) | (bsl << 1);
            wm[WM_ALO] = alo;
            wm[WM_ALIM] = alo + 32 * sw - WIN_MARGIN;
            wm[WM_BLO] = blo;
            wm[WM_BLIM] = blo + 32 * sw - WIN_MARGIN;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        pa = slot_base(asl) + (ga - 32u * Wa);
        pb = slot_base(bsl) + (gb - 32u * Wb);
        pbk = pb - (uint32_t)k;
        win_lane(k);
    };
    // refill the row's two windows at the lowest positions still to be read
    // (row-uniform amin on side a, bmin on side b)
    auto win_fill = [&](int amin, int bmin) {
        const uint32_t ga = (uint32_t)wm[WM_GA0], gb = (uint32_t)wm[WM_GB0];
        const int aa = wm[WM_AARR], ba = wm[WM_BARR];
        const uint32_t Wa = (ga + (uint32_t)amin) >> 5, Wb = (gb + (uint32_t)bmin) >> 5;
        win_load(aa >> 1, aa & 1, Wa, (ga + (uint32_t)alen + 47u) >> 5);
        win_load(ba >> 1, ba & 1, Wb, (gb + (uint32_t)blen + 47u) >> 5);
        const int alo = (int)(32u * Wa - ga), blo = (int)(32u * Wb - gb);
        __builtin_amdgcn_wave_barrier();
        if (rl == 0) {
            wm[WM_W0 + (aa >> 1)] = (int)Wa;
            wm[WM_W0 + (ba >> 1)] = (int)Wb;
            wm[WM_ALO] = alo;
            wm[WM_ALIM] = alo + 32 * sw - WIN_MARGIN;
            wm[WM_BLO] = blo;
            wm[WM_BLIM] = blo + 32 * sw - WIN_MARGIN;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int kk = k + meta[RM_KOF];
        pa = slot_base(aa >> 1) + (ga - 32u * Wa);
        pbk = slot_base(ba >> 1) + (gb - 32u * Wb) - (uint32_t)kk;
        win_lane(kk);
    };
    // finish the slides whose reads left the window (pend): refill the
    // windows of the rows concerned at their lowest pending position, go on
    // sliding; the lowest pending lane always advances (it is inside both
    // new windows), so this ends. Wave-uniform call.
    auto win_resolve = [&](int ni, int &s, int m, bool pend) {
        do {
            const int kk = k + meta[RM_KOF];
            const int c = ni + s;
            const int amin = -rw_max<RW>(pend ? -c : -INT_MAX), bmin = -rw_max<RW>(pend ? -(c - kk) : -INT_MAX);
            if (amin != INT_MAX) win_fill(amin, bmin);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (pend) {
                const int c2 = ni + s, mr = m - s;
                const int mw = c2 < wlo ? -1 : min(mr, wlim - c2);
                const int s2 = slide_fwd<AMB>(pa + (uint32_t)c2, pbk + (uint32_t)c2, max(mw, 0), moff);
                pend = mw < mr && s2 >= mw;
                s += s2;
            }
        } while (ballot(pend));
    };

#ifdef RC_ROW_TIMING
    unsigned long long t_ei = 0;   // extension starts (part of the transitions)
#endif
    auto ext_init = [&](int done_act) {
#ifdef RC_ROW_TIMING
        const unsigned long long e0t = __builtin_readcyclecounter();
#endif
        int r0 = 0;
        if constexpr (WIN) {
            win_begin(done_act == A_LDONE ? 1 : 0);
            const int m0 = min(alen, blen);
            bool pend = false;
            if (rl == RC0) {
                const int mw = min(m0, wlim);
                r0 = slide_fwd<AMB>(pa, pb, max(mw, 0), moff);
                pend = mw < m0 && r0 >= mw;
            }
            if (ballot(pend)) win_resolve(0, r0, m0, pend);
        } else {
            if (rl == RC0) r0 = slide_fwd<AMB>(pa, pb, min(alen, blen), moff);
        }
        r0 = __shfl(r0, RW * row + RC0);
        best = 2 * r0;
        bl = RC0;
        if (rl == RC0) {
            wi = r0;
            wg = 0;
            wd = 0;
        }
        R = rl == RC0 ? r0 : -1;
        goe = 0;
        if (rl == 0 && d6) atomicAdd(&rcnt[5], (uint32_t)d6);   // the previous extension's steps
        d6 = 0;
        if constexpr (!WIN) pbk = pb - (uint32_t)k;   // (WIN: win_begin / win_fill set it)
        blk = blen + k;
        mnk = max(min(alen, blk), 0);
        nkd = -k;
        if (rl == 0) {
            atomicAdd(&rcnt[0], 1u);
            meta[RM_PHASE] = done_act;
            meta[RM_KOF] = 0;
        }
        act = (min(alen, blen) - r0 <= 0) ? done_act : done_act + (A_STEP_R - A_RDONE);
#ifdef RC_ROW_TIMING
        t_ei += __builtin_readcyclecounter() - e0t;
#endif
    };

#ifdef RC_ROW_TIMING
    unsigned long long t_tr = 0, t_st = 0, t_fe = 0, t_sl = 0;   // transitions, steps; fetches and window slides (parts of the transitions)
    // what 16-lane rows could take (r06, profiles/r06_row16): a row's steps
    // until its candidate's live span first outgrows a 16-lane window (14
    // diagonals, simulated with its own centring), the candidates that never
    // do, and that window's slides
    unsigned long long n16 = 0, c16 = 0, sl16 = 0;
    bool ov16 = false, had = false;
    int w16 = 0;
#endif
    for (;;) {
#ifdef RC_ROW_TIMING
        const unsigned long long c0t = __builtin_readcyclecounter();
#endif
        // ---------------- transitions ----------------
        while (act < A_DONE) {
            if (act == A_FETCH) {
#ifdef RC_ROW_TIMING
                const unsigned long long f0t = __builtin_readcyclecounter();
#endif
                if (lnx >= s_ncand) {
                    // no work left: the row's lanes go dead for good (the
                    // other row's steps shift this row's edge lanes in)
                    R = -1;
                    act = A_DONE;
                    continue;
                }
                const uint64_t ci = cslot(lnx, RS_SHARD);
#ifdef RC_ROW_TIMING
                if (rl == 0 && had && !ov16) c16++;   // the previous candidate stayed within 14 diagonals
                ov16 = false;
                had = true;
#endif
                if (rl < CAND_DWORDS) meta[RM_REC + rl] = recv;
                if (rl == 0) {
                    meta[RM_CLO] = (int)(uint32_t)ci;
                    meta[RM_CHI] = (int)(uint32_t)(ci >> 32);
                }
                const uint32_t lidx = lnx;   // list index (the 64-lane pass's resume record)
                // prefetch the next record
                if (++lnx >= (uint32_t)RL.st[RS_LEND]) grab();
                recv = load_rec(lnx);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int Lq = meta[RM_REC + RC_LQ], Lt = meta[RM_REC + RC_LT];
                const uint64_t q0 = (uint64_t)(uint32_t)meta[RM_REC + RC_Q0];
                const uint64_t s0 = (uint64_t)(uint32_t)meta[RM_REC + RC_S0];
                const int strand = (meta[RM_REC + RC_CNT_STRAND] >> 16) & 1;
                const int nwq = (int)(((q0 & 31) + (uint64_t)Lq) >> 5) + 3;
                const int nwt = (int)(((s0 & 31) + (uint64_t)Lt) >> 5) + 3;
                const RowArgsK K = row_args();
                uint32_t qb = 0, tb = 0;
                if constexpr (WIN) {
                    // the first seed, then each slot's window from its
                    // extension's start (right: the seed's end; left: its start)
                    const uint32_t e01 = (uint32_t)meta[RM_REC + RC_E01];
                    const GSeed g0 =
                        K->P.seeds[(uint32_t)meta[RM_REC + RC_SOFF] + (K->P.which ? e01 >> 16 : e01 & 0xFFFFu)];
                    if (rl == 0) {
                        meta[RM_X] = (int)g0.x;
                        meta[RM_Y] = (int)g0.y;
                        meta[RM_LEN] = (int)(g0.len & SEED_LEN);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    for (int sl = 0; sl < 4; sl++) {
                        uint32_t g, e;
                        slot_g(sl, g, e);
                        win_load(sl, slot_arr(sl), g >> 5, (e + 47u) >> 5);
                        if (rl == 0) wm[WM_W0 + sl] = (int)(g >> 5);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                } else {
                // the left extensions walk reversed copies: the other
                // orientation's array from the mirrored start (complements on
                // both sides: the same matches), staged like the forward ones
                const uint64_t total = K->db.total;
                const uint64_t rq0 = total - q0 - (uint64_t)Lq, rs0 = total - s0 - (uint64_t)Lt;
                const int nwqr = (int)(((rq0 & 31) + (uint64_t)Lq) >> 5) + 3;
                const int nwtr = (int)(((rs0 & 31) + (uint64_t)Lt) >> 5) + 3;
                if (nwq > sw || nwt > sw || nwqr > sw || nwtr > sw) {
                    if (rl == 0 && row_args()->P.why) atomicAdd(&row_args()->P.why[0], 1ull);
                    defer(ci, false);
                    continue;
                }
                // raw words of query and subject, and the first seed: one round trip
                // both strands' pointers as scalars, selected per lane (an
                // indexed read of the kernarg segment would be a vector load,
                // one more round trip in front of the staging loads)
                GW dF = (GW)K->db.F, dRC = (GW)K->db.RC;
                asm volatile("" : "+s"(dF), "+s"(dRC));
                const GW QA = strand ? dRC : dF, QR = strand ? dF : dRC;
                const GW qw = QA + (q0 >> 5), tw = dF + (s0 >> 5);
                const GW qrw = QR + (rq0 >> 5), trw = dRC + (rs0 >> 5);
                {
                    // the first two words per lane of the four arrays in two
                    // batches (forward with the first seed, then reverse), each
                    // in flight together: the empty asm takes a batch whole, so
                    // the scheduler cannot sink its loads behind the LDS writes
                    // (r05_z: 2 round trips instead of 6, extension -0.5 ms at
                    // C3; one batch of all eight spills 16 VGPRs: +0.5 ms)
                    const uint32_t e01 = (uint32_t)meta[RM_REC + RC_E01];
                    const GSeed g0 =
                        K->P.seeds[(uint32_t)meta[RM_REC + RC_SOFF] + (K->P.which ? e01 >> 16 : e01 & 0xFFFFu)];
                    const uint64_t a0 = rl < nwq ? qw[rl] : 0ull, a1 = rl + RW < nwq ? qw[rl + RW] : 0ull;
                    const uint64_t b0 = rl < nwt ? tw[rl] : 0ull, b1 = rl + RW < nwt ? tw[rl + RW] : 0ull;
                    asm volatile("" ::"v"(a0), "v"(a1), "v"(b0), "v"(b1));
                    if (rl < nwq) stg[rl] = a0;
                    if (rl + RW < nwq) stg[rl + RW] = a1;
                    if (rl < nwt) stg[sw + rl] = b0;
                    if (rl + RW < nwt) stg[sw + rl + RW] = b1;
                    const uint64_t c0 = rl < nwqr ? qrw[rl] : 0ull, c1 = rl + RW < nwqr ? qrw[rl + RW] : 0ull;
                    const uint64_t d0 = rl < nwtr ? trw[rl] : 0ull, d1 = rl + RW < nwtr ? trw[rl + RW] : 0ull;
                    asm volatile("" ::"v"(c0), "v"(c1), "v"(d0), "v"(d1));
                    if (rl < nwqr) stg[2 * sw + rl] = c0;
                    if (rl + RW < nwqr) stg[2 * sw + rl + RW] = c1;
                    if (rl < nwtr) stg[3 * sw + rl] = d0;
                    if (rl + RW < nwtr) stg[3 * sw + rl + RW] = d1;
                    if (rl == 0) {
                        meta[RM_X] = (int)g0.x;
                        meta[RM_Y] = (int)g0.y;
                        meta[RM_LEN] = (int)(g0.len & SEED_LEN);
                    }
                }
                // (transcripts of more than 2 RW words: the rest)
                for (int w = rl + 2 * RW; w < nwq; w += RW) stg[w] = qw[w];
                for (int w = rl + 2 * RW; w < nwt; w += RW) stg[sw + w] = tw[w];
                for (int w = rl + 2 * RW; w < nwqr; w += RW) stg[2 * sw + w] = qrw[w];
                for (int w = rl + 2 * RW; w < nwtr; w += RW) stg[3 * sw + w] = trw[w];
                if (AMB) {
                    GW dAF = (GW)K->db.AF, dARC = (GW)K->db.ARC;
                    asm volatile("" : "+s"(dAF), "+s"(dARC));
                    const GW qm = (strand ? dARC : dAF) + (q0 >> 5), tm = dAF + (s0 >> 5);
                    const GW qrm = (strand ? dAF : dARC) + (rq0 >> 5), trm = dARC + (rs0 >> 5);
                    for (int w = rl; w < nwq; w += RW) stg[4 * sw + w] = qm[w];
                    for (int w = rl; w < nwt; w += RW) stg[5 * sw + w] = tm[w];
                    for (int w = rl; w < nwqr; w += RW) stg[6 * sw + w] = qrm[w];
                    for (int w = rl; w < nwtr; w += RW) stg[7 * sw + w] = trm[w];
                }
                qb = base0 + (uint32_t)(q0 & 31);
                tb = base0 + 32u * (uint32_t)sw + (uint32_t)(s0 & 31);
                if (rl == 0) {
                    meta[RM_QB] = (int)(bqr + (uint32_t)(rq0 & 31));
                    meta[RM_TB] = (int)(btr + (uint32_t)(rs0 & 31));
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                }
                if (rl == 0) atomicAdd(&rcnt[1], 1u);
                // right extension from the seed's end
                const int x = meta[RM_X], y = meta[RM_Y], len = meta[RM_LEN];
                const uint32_t sams = (uint32_t)meta[RM_REC + RC_SAMS];
                swap = (sams & 0xFFFFu) > (sams >> 16);
                pa = qb + (uint32_t)(x + len);
                alen = Lq - (x + len);
                pb = tb + (uint32_t)(y + len);
                blen = Lt - (y + len);
                if (swap) {
                    const uint32_t t = pa; pa = pb; pb = t;
                    const int u = alen; alen = blen; blen = u;
                }
                if constexpr (RW == 64) {
                    // a 32-lane extension that outgrew its window: continue it
                    // from the saved state (the diagonals outside the window
                    // were never reached, so the full band's state is it)
                    if (K->P.resume && K->P.list && lidx < K->P.res_cap) {
                        const int *rec = K->P.resume + (size_t)lidx * RES_REC;
                        const int phase = rec[RES_PHASE], kof = rec[RES_KOF];
                        if (phase == A_LDONE) {
                            if (rl < 5) meta[RM_RSC + rl] = rec[RES_RSC + rl];
                            // left extension: forward from reversed position L - x
                            pa = (uint32_t)meta[RM_QB] + (uint32_t)(Lq - x);
                            alen = x;
                            pb = (uint32_t)meta[RM_TB] + (uint32_t)(Lt - y);
                            blen = y;
                            if (swap) {
                                const uint32_t t = pa; pa = pb; pb = t;
                                const int u = alen; alen = blen; blen = u;
                            }
                        }
                        // the previous extension's steps; the resumed one's steps
                        // before the resume were counted by its first pass
                        if (rl == 0) atomicAdd(&rcnt[5], (uint32_t)(d6 - rec[RES_D6]));
                        d6 = rec[RES_D6];
                        best = rec[RES_BEST];
                        const int kb = rec[RES_PK];
                        bl = kb + RC0;
                        const int w = rl - RC0 - kof + 16;   // this diagonal's lane in the saved window
                        const bool inw = w >= 0 && w < 32;
                        R = inw ? rec[RES_R + (inw ? w : 0)] : -1;
                        goe = inw ? rec[RES_G + (inw ? w : 0)] : 0;
                        if (rl == bl) {
                            wi = rec[RES_PWI];
                            wg = rec[RES_PWG];
                            wd = rec[RES_PWD];
                        }
                        if constexpr (WIN) win_begin(phase == A_LDONE ? 1 : 0); else pbk = pb - (uint32_t)k;
                        blk = blen + k;
                        mnk = max(min(alen, blk), 0);
                        nkd = -(k + d6);
                        if (rl == 0) {
                            atomicAdd(&rcnt[0], 1u);
                            meta[RM_PHASE] = phase;
                            meta[RM_KOF] = 0;
                        }
                        act = phase + (A_STEP_R - A_RDONE);
                        continue;
                    }
                }
                ext_init(A_RDONE);
#ifdef RC_ROW_TIMING
                t_fe += __builtin_readcyclecounter() - f0t;
#endif
            } else if (act == A_SLIDE) {
#ifdef RC_ROW_TIMING
                const unsigned long long s0t = __builtin_readcyclecounter();
#endif
                // a live lane at the window's edge: centre the live diagonals
                const uint32_t livem = rw_mask<RW>(ballot(R >= 0), row);
                const int kof = meta[RM_KOF];
                const int lmin = __builtin_ctz(livem), lmax = 31 - __builtin_clz(livem);
                constexpr int KMAX = 31 - RW / 2;
                const int kn = max(-KMAX, min(KMAX, kof + ((lmin + lmax + 1) >> 1) - RC0));
                const int s = kn - kof;
                if (s == 0 || lmin - s < 1 || lmax - s > RW - 2) {
                    act = A_ABORT;   // wider than the window, or at the band's edge
                    if constexpr (SAVE && RW == 32) {
                        // what the 64-lane pass needs to continue it (A_ABORT
                        // saves it with the frontier): the best record parked
                        // as a slide parks it, the step count, the best score
                        if (bl != BL_PARKED) {
                            const int bsrc = RW * row + bl;
                            const int pwi = __shfl(wi, bsrc), pwg = __shfl(wg, bsrc), pwd = __shfl(wd, bsrc);
                            if (rl == 0) {
                                meta[RM_PWI] = pwi;
                                meta[RM_PWG] = pwg;
                                meta[RM_PWD] = pwd;
                                meta[RM_PK] = bl - RC0 + kof;
                            }
                        }
                        if (rl == 0) {
                            meta[RM_AD6] = d6;
                            meta[RM_ABEST] = best;
                        }
                    }
                    continue;
                }
                if (bl != BL_PARKED) {
                    // the row's best record leaves its lane's hands (that lane may leave the window)
                    const int bsrc = RW * row + bl;
                    const int pwi = __shfl(wi, bsrc), pwg = __shfl(wg, bsrc), pwd = __shfl(wd, bsrc);
                    if (rl == 0) {
                        meta[RM_PWI] = pwi;
                        meta[RM_PWG] = pwg;
                        meta[RM_PWD] = pwd;
                        meta[RM_PK] = bl - RC0 + kof;
                    }
                    bl = BL_PARKED;
                }
                const int from = rl + s;
                const bool in = from >= 0 && from < RW;
                const int nR = __shfl(R, RW * row + (in ? from : rl)), ng = __shfl(goe, RW * row + (in ? from : rl));
                R = in ? nR : -1;
                goe = in ? ng : 0;
                // this lane's diagonal was k + kof and is k + kn: refold it
                // into the per-lane constants (pb and blen are not kept)
                pbk -= (uint32_t)s;
                blk += s;
                mnk = max(min(alen, blk), 0);
                nkd -= s;
                if constexpr (WIN) win_lane(k + kn);
                if (rl == 0) {
                    meta[RM_KOF] = kn;
                    atomicAdd(&rcnt[3], 1u);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                act = meta[RM_PHASE] + (A_STEP_R - A_RDONE);
#ifdef RC_ROW_TIMING
                t_sl += __builtin_readcyclecounter() - s0t;
#endif
            } else if (act == A_RDONE || act == A_LDONE) {
                int ei, ed, ego, kb;   // the best record and its diagonal
                if (bl == BL_PARKED) {
                    ei = meta[RM_PWI];
                    ed = meta[RM_PWD] / 6;
                    ego = meta[RM_PWG];
                    kb = meta[RM_PK];
                } else {
                    const int src = RW * row + bl;
                    ei = __shfl(wi, src);
                    ed = __shfl(wd, src) / 6;
                    ego = __shfl(wg, src);
                    kb = bl - RC0 + meta[RM_KOF];
                }
                int ej = ei - kb;
                if (swap) {
                    const int t = ei; ei = ej; ej = t;
                }
                if (act == A_RDONE) {
                    if (rl == 0) {
                        meta[RM_RSC] = best;
                        meta[RM_RI] = ei;
                        meta[RM_RJ] = ej;
                        meta[RM_RD] = ed;
                        meta[RM_RGO] = ego;
                    }
                    // left extension: forward from reversed position L - x
                    // (= base x - 1) of the reversed copies
                    const int x = meta[RM_X], y = meta[RM_Y];
                    const int Lq = meta[RM_REC + RC_LQ], Lt = meta[RM_REC + RC_LT];
                    pa = (uint32_t)meta[RM_QB] + (uint32_t)(Lq - x);
                    alen = x;
                    pb = (uint32_t)meta[RM_TB] + (uint32_t)(Lt - y);
                    blen = y;
                    if (swap) {
                        const uint32_t t = pa; pa = pb; pb = t;
                        const int u = alen; alen = blen; blen = u;
                    }
                    ext_init(A_LDONE);
                } else {
                    // both results of the first seed: first_finish_kernel builds the box
                    const uint64_t ci = (uint64_t)(uint32_t)meta[RM_CLO] | ((uint64_t)(uint32_t)meta[RM_CHI] << 32);
                    int v = 0;
                    if (rl >= FX_R && rl < FX_R + 5) v = meta[RM_RSC + (rl - FX_R)];
                    if (rl == FX_L) v = best;
                    if (rl == FX_L + 1) v = ei;
                    if (rl == FX_L + 2) v = ej;
                    if (rl == FX_L + 3) v = ed;
                    if (rl == FX_L + 4) v = ego;
                    if (rl < BOX_REC) box_out()[ci * BOX_REC + rl] = v;
                    act = A_FETCH;
                }
            } else {   // A_ABORT: the sub-band overflowed
                const uint64_t ci = (uint64_t)(uint32_t)meta[RM_CLO] | ((uint64_t)(uint32_t)meta[RM_CHI] << 32);
                const unsigned long long wi2 = defer(ci, true);
                if constexpr (SAVE && RW == 32) {
                    // the wide pass continues from here: the window's frontier
                    // and the header A_SLIDE left in the bookkeeping
                    if (wi2 != ~0ull) {
                        const RowArgsK K = row_args();
                        if (K->P.resume && wi2 < K->P.res_cap) {
                            int *rec = K->P.resume + (size_t)wi2 * RES_REC;
                            rec[RES_R + rl] = R;
                            rec[RES_G + rl] = goe;
                            // the bookkeeping from the right results to the best
                            // record, the step count, the best score
                            if (rl <= RES_PK) rec[rl] = meta[RM_RSC + rl];
                            if (rl == RES_D6) rec[rl] = meta[RM_AD6];
                            if (rl == RES_BEST) rec[rl] = meta[RM_ABEST];
                        }
                    }
                }
                if (rl == 0) atomicAdd(&rcnt[2], 1u);
                act = A_FETCH;
            }
        }
#ifdef RC_ROW_TIMING
        const unsigned long long c1t = __builtin_readcyclecounter();
        t_tr += c1t - c0t;
#endif
        const bool ext = act >= A_STEP_R;
        const uint64_t mext = m_ge(act, A_STEP_R);
        if (!mext) break;
        // ---------------- one greedy step of every extending row ----------------
        if (ext) {
            d6 += 6;
            nkd -= 6;
            const int Rl = rw_from_lower<RW, true>(R, -1, rl), Rr = rw_from_upper<RW, true>(R, -1, rl);
            const int gl = rw_from_lower<RW, false>(goe, 0, rl), gr = rw_from_upper<RW, false>(goe, 0, rl);
            // candidates; ties prefer mismatch, then insertion, then deletion (a
            // frontier value R >= 0 has j = R - k >= 0, so unsigned compares
            // carry the lower bounds)
            // (j = R - k < blen  <=>  R < blk;  j + 1 = Rr - k < blen + 1  <=>  Rr <= blk)
            const int cm = ((uint32_t)R < (uint32_t)mnk) ? R + 1 : -1;
            const int cil = ((uint32_t)Rl < (uint32_t)alen) ? Rl + 1 : -1;
            const int cd = (Rr >= 0 && Rr <= blk) ? Rr : -1;
            int ni = max(max(cm, cil), cd);
            const bool fm = ni >= 0 && cm == ni, fi = !fm && cil == ni;
            // gap state of the chosen move: G | O << 13 | E << 26 (E: 1 insertion, 2 deletion)
            const int src = fm ? goe : (fi ? gl : gr);
            const int e = fm ? 0 : (fi ? 1 : 2);
            const int pe = (src >> EBIT) & 3;
            // (E goes in after the slide: matches after the move clear it)
            const int ngb = (src & ~(3 << EBIT)) + (fm ? 0 : 1 + (pe == e ? 0 : (1 << OBIT)));
            int ee = e;
            // the score of a lane live after the step; its bound (the score
            // if every remaining base matched): 2 (ni + s) - k - d6 + 2 (m - s)
            // = 2 min(alen, blk) + nkd, on every lane (only live lanes' are read)
            int score = 0;
            const int bound = 2 * mnk + nkd;
            if constexpr (WIN) {
                // slides stop at the window; the ones that reached it (or
                // start outside it) are finished after a refill
                int m = 0, s = 0;
                bool pend = false;
                if (ni >= 0) {
                    m = mnk - ni;
                    const int mw = ni < wlo ? -1 : min(m, wlim - ni);
                    s = slide_fwd<AMB>(pa + (uint32_t)ni, pbk + (uint32_t)ni, max(mw, 0), moff);
                    pend = mw < m && s >= mw;
                }
                if (ballot(pend)) win_resolve(ni, s, m, pend);
                if (ni >= 0) {
                    ni += s;
                    if (s > 0) ee = 0;
                    score = 2 * ni + nkd;   // 2 ni - k - d6
                    if (score < best - X) ni = -1;
                }
            } else if (ni >= 0) {
                const int m = mnk - ni;
                const int s = slide_fwd<AMB>(pa + (uint32_t)ni, pbk + (uint32_t)ni, m, moff);
                ni += s;
                if (s > 0) ee = 0;
                score = 2 * ni + nkd;   // 2 ni - k - d6
                if (score < best - X) ni = -1;
            }
            const int ng = ngb + (ee << EBIT);
            R = ni;
            goe = ng;
            const bool live = ni >= 0;
            // row-wide decisions as lane masks (scalar), applied with v_cndmask.
            // A lane X-dropped this step has score < best.
            const uint64_t mlive = m_ge(ni, 0);
#ifdef RC_ROW_TIMING
            if constexpr (RW == 32) {
                const uint32_t lv = rw_mask<RW>(mlive, row);
                if (d6 == 6) w16 = 0;   // an extension's first step: the window starts centred
                if (lv) {
                    const int kofr = meta[RM_KOF];
                    const int dmin = __builtin_ctz(lv) - RC0 + kofr, dmax = (31 - __builtin_clz(lv)) - RC0 + kofr;
                    if (dmax - dmin + 1 > 14 || dmin < w16 - 8 || dmax > w16 + 7) {
                        ov16 = true;
                    } else if (!ov16 && (dmin == w16 - 8 || dmax == w16 + 7)) {
                        const int c = (dmin + dmax + 1) >> 1;
                        if (c < -23 || c > 23) ov16 = true;
                        else {
                            w16 = c;
                            if (rl == 0) sl16++;
                        }
                    }
                }
                if (!ov16 && rl == 0) n16++;
            }
#endif
            const uint64_t mi = m_gt(score, best) & mlive;
            const uint64_t mimp = rw_spread<RW>(mi);
            if (mimp) {
                uint64_t mwin;
                const uint32_t lo = (uint32_t)mi, hi = (uint32_t)(mi >> 32);
                if (RW == 32 && !(lo & (lo - 1)) && !(hi & (hi - 1))) {
                    // at most one improving lane per row (the usual case): it is
                    // the row's new best, read out directly, no row reduction
                    // (a row without an improving lane reads an unused lane)
                    const int a = s_ff1(lo) & 31, b = s_ff1(hi) & 31;
                    const int s0 = __builtin_amdgcn_readlane(score, a), s1 = __builtin_amdgcn_readlane(score, 32 + b);
                    constexpr uint64_t ROW0 = 0xFFFFFFFFull;
                    best = lane_sel(mimp & ROW0, s0, lane_sel(mimp & ~ROW0, s1, best));
                    bl = lane_sel(mimp & ROW0, a, lane_sel(mimp & ~ROW0, b, bl));
                    mwin = mi;
                } else {
                    const int mk = rw_max<RW>(live ? score * RW + (RW - 1 - rl) : INT_MIN);
                    best = lane_sel(mimp, mk >> (RW == 64 ? 6 : (RW == 32 ? 5 : 4)), best);
                    bl = lane_sel(mimp, RW - 1 - (mk & (RW - 1)), bl);
                    mwin = mimp & m_eq(rl, bl);
                }
                wi = lane_sel(mwin, R, wi);
                wg = lane_sel(mwin, goe, wg);
                wd = lane_sel(mwin, d6, wd);
            }
            // bound >= score, so a lane that can still beat best is live
            // a live lane at a sub-band edge: the candidate goes to a wider
            // pass; 64-lane rows are the spec's band itself (no edge abort)
            constexpr uint64_t EDGES = RW == 64 ? 0ull : (RW == 32 ? 0x8000000180000001ull : 0x8001800180018001ull);
            const uint64_t mcont = rw_spread<RW>(mlive & m_gt(bound, best)) & m_lt(d6, 6 * DMAX);
            const uint64_t medge = RW == 64 ? 0ull : rw_spread<RW>(mlive & EDGES);
            act = lane_sel(mcont, lane_sel_k<A_SLIDE>(medge, act), act - (A_STEP_R - A_RDONE));
        }
#ifdef RC_ROW_TIMING
        t_st += __builtin_readcyclecounter() - c1t;
#endif
    }
#ifdef RC_ROW_TIMING
    unsigned long long *const counters = row_args()->P.counters;
    if (lane == 0 && counters) {
        atomicAdd(&counters[DC_T_TRANS - DC_COUNTERS], t_tr);
        atomicAdd(&counters[DC_T_STEPS - DC_COUNTERS], t_st);
        atomicAdd(&counters[DC_T_FETCH - DC_COUNTERS], t_fe);   // (the DC_T_* slots past the view: nothing else uses them)
        atomicAdd(&counters[DC_T_SLIDE - DC_COUNTERS], t_sl);
        atomicAdd(&counters[DC_T_START - DC_COUNTERS], t_ei);
    }
    if (rl == 0 && had && !ov16) c16++;
    if (rl == 0 && counters) {
        atomicAdd(&counters[DC_T_N16 - DC_COUNTERS], n16);
        atomicAdd(&counters[DC_T_C16 - DC_COUNTERS], c16);
        atomicAdd(&counters[DC_T_SL16 - DC_COUNTERS], sl16);
    }
#endif
    unsigned long long *const ctr = row_args()->P.counters;
    if (rl == 0 && d6) atomicAdd(&rcnt[5], (uint32_t)d6);   // the last extension's steps
    __syncthreads();
    if (threadIdx.x < 4 && ctr) atomicAdd(&ctr[DC_EXTS - DC_COUNTERS + threadIdx.x], (unsigned long long)rcnt[threadIdx.x]);   // ... DC_SLIDES
    if (threadIdx.x == 5 && ctr) atomicAdd(&ctr[DC_STEPS - DC_COUNTERS], (unsigned long long)(rcnt[5] / 6u));
}

// A row-kernel launch: the windowed instantiation when the staging slot is
// shorter than the longest transcript (P.win), one resident round of blocks.
template <bool A, int RWV, bool SV, bool WV>
static void launch_rows_t(const Db &db, const ExtParams &P, hipStream_t st)
{
    auto kern = extend_rows_kernel<A, RWV, ROW_MIN_WAVES, SV, WV>;
    const size_t lds = row_lds_bytes(RWV, A ? 8 : 4, P.dsw, WV);
    hipLaunchKernelGGL(kern, dim3(resident_blocks(kern, lds)), dim3(EBLOCK), lds, st, RowArgs{db, P});
}
template <int RWV, bool SV>
static void launch_rows_aw(bool amb, const Db &db, const ExtParams &P, hipStream_t st)
{
    if (amb) {
        if (P.win) launch_rows_t<true, RWV, SV, true>(db, P, st); else launch_rows_t<true, RWV, SV, false>(db, P, st);
    } else {
        if (P.win) launch_rows_t<false, RWV, SV, true>(db, P, st); else launch_rows_t<false, RWV, SV, false>(db, P, st);
    }
}
// The row kernels there are: 32-lane rows, plain or saving (save: an extension
// that outgrows the window is kept in P.resume for the 64-lane pass), and
// 64-lane rows; each with and without ambiguity masks and windowed staging.
// Any other (rw, save) is a mistake in the pass order: there is no kernel to
// fall back to.
void launch_rows(int rw, bool save, bool amb, const Db &db, const ExtParams &P, hipStream_t st)
{
    if (rw == 32 && !save) return launch_rows_aw<32, false>(amb, db, P, st);
    if (rw == 32 && save) return launch_rows_aw<32, true>(amb, db, P, st);
    if (rw == 64 && !save) return launch_rows_aw<64, false>(amb, db, P, st);
    fprintf(stderr, "launch_rows: no row kernel for rw %d, save %d\n", rw, (int)save);
    std::abort();
}

// Staging slot (u64 words per staged array) the 32-lane row kernel can have
// at ROW_MIN_WAVES waves per SIMD (as many 4-wave blocks per CU in 160 KB of LDS); a longer
// transcript runs on the windowed instantiation.
int row_slot_words_max(bool amb)
{
    const int na = amb ? 8 : 4, rows = EBLOCK / 32;
    const size_t per_block = (size_t)(160 * 1024) / (size_t)ROW_MIN_WAVES;
    const size_t fixed = row_lds_bytes(32, na, 0, true);
    return (int)((per_block - fixed) / ((size_t)rows * na * 8));
}

}  // namespace rcg
