// Test-only probe of the main index's sort (tests/index_sort_probe.py builds
// it with the product's own sort.hip and kernels.hip into
// tests/_build/libindexsortprobe.so). Never linked into librcgpu.so.
//
// A plain C ABI: host pointers in and out, every device buffer owned by the
// handle, every HIP call checked, the stream synchronised before a result is
// copied back. Calls return 0 or a negative code; isp_error() has the message.
//
// One handle = one stream plus the sort's scratch, look-back status table and
// epoch, kept across calls the way the engine's sort_index keeps them: the
// status table is zeroed only when it grows, the epoch starts at 0 and is
// advanced by the sort alone.
#include "launch.h"

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

namespace rcg {
int isp_tile_keys();
int isp_local_cap();
int isp_list_len();
int isp_gbits_max();
}  // namespace rcg

using rcg::TxInfo;

namespace {

constexpr size_t FRONT_PAD = 2;   // engine.h: zero words in front of every packed array
constexpr size_t BACK_PAD = 4;    // and behind
constexpr int ISP_E_ARG = -1, ISP_E_HIP = -2, ISP_E_CAP = -3;

std::string g_err;   // errors without a handle (isp_create)

template <typename T>
struct Buf {
    T *p = nullptr;
    uint64_t cap = 0;   // elements
    hipError_t ensure(uint64_t n)
    {
        if (n <= cap) return hipSuccess;
        release();
        const hipError_t r = hipMalloc((void **)&p, n * sizeof(T));
        if (r == hipSuccess) cap = n;
        else p = nullptr;
        return r;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace

struct isp_handle {
    hipStream_t st = nullptr;
    uint32_t epoch = 0;
    Buf<uint32_t> scratch, offsets, list, bucket;
    Buf<uint64_t> status;
    Buf<uint64_t> a, b;                 // entries, ping-pong
    Buf<uint8_t> ascii;
    Buf<uint64_t> F, AF, RC, ARC;       // FRONT_PAD + nwords + BACK_PAD words each
    Buf<TxInfo> tx;
    Buf<uint64_t> koff, kcnt;
    std::string err;
};

namespace {

int fail(isp_handle *h, int code, const std::string &msg)
{
    (h ? h->err : g_err) = msg;
    return code;
}

#define ISPHIP(h, x)                                                                                   \
    do {                                                                                               \
        const hipError_t r_ = (x);                                                                     \
        if (r_ != hipSuccess)                                                                          \
            return fail(h, ISP_E_HIP, std::string(#x) + ": " + hipGetErrorString(r_));                 \
    } while (0)

#define ISPCHK(x)                   \
    do {                            \
        const int c_ = (x);         \
        if (c_ != 0) return c_;     \
    } while (0)

uint64_t pack_words(uint64_t total) { return (total + 31) / 32 + 2; }   // engine.hip pack_tile

// engine.hip index_bits: about one bucket per entry, 2^16 to 2^28
int index_bits(uint64_t n)
{
    int bits = 16;
    while (bits < 28 && (1ull << bits) < n) bits++;
    return bits;
}

// the buffers of an index of n entries with 2^bits buckets, as sort_index sizes them
int sort_state(isp_handle *h, uint64_t n, int G, int bits)
{
    ISPHIP(h, h->scratch.ensure(rcg::os_index_scratch_words(n)));
    const uint64_t words = rcg::os_index_status_words(n);
    if (h->status.cap < words) {
        ISPHIP(h, h->status.ensure(words));
        ISPHIP(h, hipMemsetAsync(h->status.p, 0, words * sizeof(uint64_t), h->st));
    }
    ISPHIP(h, h->offsets.ensure(rcg::os_index_offset_words(G)));
    ISPHIP(h, h->list.ensure(rcg::os_index_list_words()));
    ISPHIP(h, h->bucket.ensure((1ull << bits) + 1));
    return 0;
}

// a[0, n) sorted and its bucket table, as the engine's sort_index does it;
// both copied out. info[0..2] = fallback ranges, fallback keys, whole.
int run_index_sort(isp_handle *h, uint64_t n, int G, int bits, uint32_t cap, bool counted, uint64_t *ent,
                   uint32_t *bucket, uint64_t *info)
{
    const uint64_t nb = (1ull << bits) + 1;
    ISPCHK(sort_state(h, n, G, bits));
    // every slot left unwritten shows in the comparison
    ISPHIP(h, hipMemsetAsync(h->bucket.p, 0xFF, nb * sizeof(uint32_t), h->st));
    uint64_t *res = h->a.p;
    uint32_t fb_ranges = 0;
    uint64_t fb_keys = 0;
    bool whole = false, table_done = false;
    if (n) {
        hipStream_t st = h->st;
        const int where = rcg::os_index_sort(h->a.p, h->b.p, n, G, bits, cap, h->scratch.p, h->status.p, h->epoch,
                                             h->offsets.p, h->list.p, h->bucket.p, st, counted,
                                             [st] { return hipStreamSynchronize(st) == hipSuccess; }, &fb_ranges,
                                             &fb_keys, &whole);
        if (where < 0) return fail(h, ISP_E_HIP, "os_index_sort: the read of the oversized ranges failed");
        ISPHIP(h, hipGetLastError());
        res = where == 1 ? h->b.p : h->a.p;
        table_done = !whole;
    }
    if (!table_done) rcg::launch_bucket_fill(res, n, bits, h->bucket.p, h->st);
    ISPHIP(h, hipGetLastError());
    if (n) ISPHIP(h, hipMemcpyAsync(ent, res, n * 8, hipMemcpyDeviceToHost, h->st));
    ISPHIP(h, hipMemcpyAsync(bucket, h->bucket.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
    ISPHIP(h, hipStreamSynchronize(h->st));
    if (info) {
        info[0] = fb_ranges;
        info[1] = fb_keys;
        info[2] = whole;
    }
    return 0;
}

// ascii[0, total) packed into the handle's F / AF / RC / ARC with the engine's padding
int run_pack(isp_handle *h, const uint8_t *ascii, uint64_t total)
{
    const uint64_t nwords = pack_words(total), all = nwords + BACK_PAD + FRONT_PAD;
    ISPHIP(h, h->ascii.ensure(std::max<uint64_t>(total, 1)));
    ISPHIP(h, h->F.ensure(all));
    ISPHIP(h, h->RC.ensure(all));
    ISPHIP(h, h->AF.ensure(all));
    ISPHIP(h, h->ARC.ensure(all));
    if (total) ISPHIP(h, hipMemcpyAsync(h->ascii.p, ascii, total, hipMemcpyHostToDevice, h->st));
    ISPHIP(h, hipMemsetAsync(h->F.p, 0, all * 8, h->st));
    ISPHIP(h, hipMemsetAsync(h->RC.p, 0, all * 8, h->st));
    ISPHIP(h, hipMemsetAsync(h->AF.p, 0, all * 8, h->st));
    ISPHIP(h, hipMemsetAsync(h->ARC.p, 0, all * 8, h->st));
    rcg::launch_pack(h->ascii.p, total, nwords, h->F.p + FRONT_PAD, h->RC.p + FRONT_PAD, h->AF.p + FRONT_PAD,
                     h->ARC.p + FRONT_PAD, h->st);
    ISPHIP(h, hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char *isp_error(isp_handle *h) { return (h ? h->err : g_err).c_str(); }

isp_handle *isp_create(void)
{
    isp_handle *h = new isp_handle();
    const hipError_t r = hipStreamCreate(&h->st);
    if (r != hipSuccess) {
        g_err = std::string("hipStreamCreate: ") + hipGetErrorString(r);
        delete h;
        return nullptr;
    }
    return h;
}

void isp_destroy(isp_handle *h)
{
    if (!h) return;
    if (h->st) (void)hipStreamSynchronize(h->st);
    h->scratch.release();
    h->offsets.release();
    h->list.release();
    h->bucket.release();
    h->status.release();
    h->a.release();
    h->b.release();
    h->ascii.release();
    h->F.release();
    h->AF.release();
    h->RC.release();
    h->ARC.release();
    h->tx.release();
    h->koff.release();
    h->kcnt.release();
    if (h->st) (void)hipStreamDestroy(h->st);
    delete h;
}

// keys per tile of a global pass, keys a range-local workgroup holds, ranges
// the oversized list holds, most bits of the global passes (host only)
void isp_geometry(int *tile, int *local_cap, int *list_len, int *gmax)
{
    if (tile) *tile = rcg::isp_tile_keys();
    if (local_cap) *local_cap = rcg::isp_local_cap();
    if (list_len) *list_len = rcg::isp_list_len();
    if (gmax) *gmax = rcg::isp_gbits_max();
}

// the engine's choice for an index of n entries: bucket bits and G (host only)
void isp_choice(uint64_t n, uint32_t cap, int *bits, int *G)
{
    *bits = index_bits(n);
    *G = rcg::os_index_gbits(n, *bits, cap);
}

uint32_t isp_epoch(isp_handle *h) { return h ? h->epoch : 0u; }

// ent[0, n) = keys[0, n) sorted stably on bits [32, 64), bucket[0, 2^bits] its
// table: os_index_sort, uncounted, with G global bits and ranges of more
// than cap keys (0: the local capacity) counted as oversized
int isp_sort(isp_handle *h, const uint64_t *keys, uint64_t n, int G, int bits, uint32_t cap, uint64_t *ent,
             uint32_t *bucket, uint64_t *info)
{
    if (!h) return fail(nullptr, ISP_E_ARG, "null handle");
    if (bits < 1 || bits > 28 || G < 0 || G > bits || G > rcg::isp_gbits_max())
        return fail(h, ISP_E_ARG, "bits must be in [1, 28], G in [0, min(bits, G max)]");
    if (n > 0xFFFFFFFFull) return fail(h, ISP_E_ARG, "more than 2^32 keys");
    if (!bucket || (n && (!keys || !ent))) return fail(h, ISP_E_ARG, "null array");
    ISPHIP(h, h->a.ensure(std::max<uint64_t>(n, 1)));
    ISPHIP(h, h->b.ensure(std::max<uint64_t>(n, 1)));
    if (n) ISPHIP(h, hipMemcpyAsync(h->a.p, keys, n * 8, hipMemcpyHostToDevice, h->st));
    return run_index_sort(h, n, G, bits, cap, false, ent, bucket, info);
}

// The main index of the transcripts (tx_start[t], tx_len[t]) of ascii[0,
// total) as build_index_of builds it: pack, fill, os_index_sort with the
// engine's choice of bits and G (isp_choice).
//   amb 0: os_index_fill_hist + counted sort (the engine's default)
//   amb 1: launch_kmer_count, host scan, launch_kmer_fill(true) + uncounted sort
// ent[0, ent_cap) receives *n entries, bucket[0, 2^bits] the table of
// *bits_out bits (room for 2^bits_cap + 1).
int isp_index(isp_handle *h, const uint8_t *ascii, uint64_t total, const uint64_t *tx_start, const uint32_t *tx_len,
              uint32_t n_tx, int amb, uint32_t cap, uint64_t *ent, uint64_t ent_cap, uint64_t *n_out,
              uint32_t *bucket, int bits_cap, int *bits_out, int *G_out, uint64_t *info)
{
    if (!h) return fail(nullptr, ISP_E_ARG, "null handle");
    if ((total && !ascii) || (n_tx && (!tx_start || !tx_len)) || !n_out || (ent_cap && !ent) || !bucket || !bits_out ||
        !G_out)
        return fail(h, ISP_E_ARG, "null array");
    if (total > 0xFFFFFFFFull) return fail(h, ISP_E_ARG, "positions are 32-bit");
    std::vector<TxInfo> tx(n_tx);
    std::vector<uint64_t> off((size_t)n_tx + 1, 0);
    for (uint32_t t = 0; t < n_tx; t++) {
        if (tx_start[t] > total || tx_len[t] > total - tx_start[t])
            return fail(h, ISP_E_ARG, "transcript " + std::to_string(t) + " leaves the sequence");
        tx[t] = TxInfo{tx_start[t], tx_len[t], 0};
        off[t + 1] = off[t] + (tx_len[t] >= (uint32_t)rcg::W16 ? tx_len[t] - rcg::W16 + 1 : 0u);
    }
    ISPCHK(run_pack(h, ascii, total));
    ISPHIP(h, h->tx.ensure((uint64_t)n_tx + 1));
    ISPHIP(h, h->koff.ensure((uint64_t)n_tx + 1));
    if (n_tx) ISPHIP(h, hipMemcpyAsync(h->tx.p, tx.data(), (size_t)n_tx * sizeof(TxInfo), hipMemcpyHostToDevice, h->st));
    uint64_t n = off[n_tx];
    const uint64_t n_all = n;   // every window: what the fill can write at most
    if (amb) {
        // the valid windows per transcript, scanned on the host
        ISPHIP(h, h->kcnt.ensure((uint64_t)n_tx + 1));
        ISPHIP(h, hipMemsetAsync(h->kcnt.p, 0, ((size_t)n_tx + 1) * 8, h->st));
        if (n_tx) rcg::launch_kmer_count(h->tx.p, n_tx, h->AF.p + FRONT_PAD, h->kcnt.p, h->st);
        ISPHIP(h, hipGetLastError());
        std::vector<uint64_t> cnt((size_t)n_tx + 1, 0);
        ISPHIP(h, hipMemcpyAsync(cnt.data(), h->kcnt.p, ((size_t)n_tx + 1) * 8, hipMemcpyDeviceToHost, h->st));
        ISPHIP(h, hipStreamSynchronize(h->st));
        uint64_t acc = 0;
        for (uint32_t t = 0; t <= n_tx; t++) {
            // a count above the closed form would let the fill write past the entry array
            if (t < n_tx && cnt[t] > off[t + 1] - off[t])
                return fail(h, ISP_E_CAP, "kmer_count gave transcript " + std::to_string(t) + " more windows than it has");
            const uint64_t c = t < n_tx ? cnt[t] : 0;
            off[t] = acc;
            acc += c;
        }
        n = off[n_tx];
    }
    *n_out = n;
    if (n > ent_cap) return fail(h, ISP_E_CAP, "index has " + std::to_string(n) + " entries, room for " + std::to_string(ent_cap));
    const int bits = index_bits(n), G = rcg::os_index_gbits(n, bits, cap);
    *bits_out = bits;
    *G_out = G;
    if (G < 0) return fail(h, ISP_E_ARG, "an index of this size keeps the 8-bit passes: not this probe's");
    if (bits > bits_cap) return fail(h, ISP_E_CAP, "the bucket table needs " + std::to_string(bits) + " bits");
    ISPHIP(h, hipMemcpyAsync(h->koff.p, off.data(), ((size_t)n_tx + 1) * 8, hipMemcpyHostToDevice, h->st));
    // room for every window: a fill that disagrees with the counts stays inside the array
    ISPHIP(h, h->a.ensure(std::max<uint64_t>(n_all, 1)));
    ISPHIP(h, h->b.ensure(std::max<uint64_t>(n_all, 1)));
    // entries the fill leaves unwritten show in the comparison
    ISPHIP(h, hipMemsetAsync(h->a.p, 0xFF, std::max<uint64_t>(n_all, 1) * 8, h->st));
    const bool counted = !amb && n > 0;   // as build_index_of: an empty index is not counted
    if (counted) {
        ISPHIP(h, h->scratch.ensure(rcg::os_index_scratch_words(n)));
        rcg::os_index_fill_hist(h->tx.p, n_tx, h->F.p + FRONT_PAD, h->koff.p, h->a.p, n, G, h->scratch.p, h->st);
    } else if (n_tx) {
        rcg::launch_kmer_fill(amb != 0, h->tx.p, n_tx, h->F.p + FRONT_PAD, amb ? h->AF.p + FRONT_PAD : nullptr,
                              h->koff.p, h->a.p, h->st);
    }
    ISPHIP(h, hipGetLastError());
    return run_index_sort(h, n, G, bits, cap, counted, ent, bucket, info);
}

}  // extern "C"
