// Test-only probe of the seed index kernels (oracle/index_probe.py builds it
// with the product's own sort.hip and kernels.hip into
// oracle/_build/libindexprobe.so). Never linked into librcgpu.so.
//
// A plain C ABI: host pointers in and out, every device buffer owned by the
// handle, every HIP call checked, the stream synchronised before a result is
// copied back. Calls return 0 or a negative code; ip_error() has the message.
//
// One handle = one stream plus the sort's scratch, look-back status table and
// epoch, kept across calls the way the engine's sort_index keeps them: the
// status table is zeroed only when it grows, the epoch starts at 0 and is
// advanced by os_sort_keys alone.
#include "launch.h"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

namespace rcg {
int os_tile_keys();
int os_segments();
int bucket_fill_per_thread();
}  // namespace rcg

using rcg::TxInfo;

namespace {

constexpr size_t FRONT_PAD = 2;   // engine.h: zero words in front of every packed array
constexpr size_t BACK_PAD = 4;    // and behind
constexpr int IP_E_ARG = -1, IP_E_HIP = -2, IP_E_CAP = -3;

std::string g_err;   // errors without a handle (ip_create)

template <typename T>
struct Buf {
    T *p = nullptr;
    uint64_t cap = 0;   // elements
    hipError_t ensure(uint64_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) {
            const hipError_t r = hipFree(p);
            p = nullptr;
            cap = 0;
            if (r != hipSuccess) return r;
        }
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

struct ip_handle {
    hipStream_t st = nullptr;
    uint32_t epoch = 0;
    Buf<uint32_t> scratch;
    Buf<uint64_t> status;
    Buf<uint64_t> a, b;                 // keys / entries, ping-pong
    Buf<uint8_t> ascii;
    Buf<uint64_t> F, AF, RC, ARC;       // FRONT_PAD + nwords + BACK_PAD words each
    Buf<TxInfo> tx;
    Buf<uint64_t> koff, kcnt;
    Buf<uint32_t> bucket;
    std::string err;
};

namespace {

int fail(ip_handle *h, int code, const std::string &msg)
{
    (h ? h->err : g_err) = msg;
    return code;
}

#define IPHIP(h, x)                                                                                    \
    do {                                                                                               \
        const hipError_t r_ = (x);                                                                     \
        if (r_ != hipSuccess)                                                                          \
            return fail(h, IP_E_HIP, std::string(#x) + ": " + hipGetErrorString(r_));                  \
    } while (0)

#define IPCHK(x)                    \
    do {                            \
        const int c_ = (x);         \
        if (c_ != 0) return c_;     \
    } while (0)

uint64_t pack_words(uint64_t total) { return (total + 31) / 32 + 2; }   // engine.hip pack_tile

// the sort's scratch and status table for n keys, as sort_index sizes them
int sort_state(ip_handle *h, uint64_t n)
{
    IPHIP(h, h->scratch.ensure(rcg::os_scratch_words(n)));
    const uint64_t words = rcg::os_status_words(n);
    if (h->status.cap < words) {
        IPHIP(h, h->status.ensure(words));
        IPHIP(h, hipMemsetAsync(h->status.p, 0, words * sizeof(uint64_t), h->st));
    }
    return 0;
}

// uncounted or counted sort of a[0, n); *res = the buffer that holds the result
int run_sort(ip_handle *h, uint64_t n, int bb, bool counted, uint64_t **res)
{
    *res = h->a.p;
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull) return fail(h, IP_E_ARG, "more than 2^32 keys");
    IPCHK(sort_state(h, n));
    const bool in_alt = rcg::os_sort_keys(h->a.p, h->b.p, n, bb, h->scratch.p, h->status.p, h->epoch, h->st, nullptr,
                                          counted, nullptr, nullptr, nullptr, 0u, nullptr);
    IPHIP(h, hipGetLastError());
    *res = in_alt ? h->b.p : h->a.p;
    return 0;
}

// ascii[0, total) packed into the handle's F / AF / RC / ARC with the engine's padding
int run_pack(ip_handle *h, const uint8_t *ascii, uint64_t total)
{
    const uint64_t nwords = pack_words(total), all = nwords + BACK_PAD + FRONT_PAD;
    IPHIP(h, h->ascii.ensure(std::max<uint64_t>(total, 1)));
    IPHIP(h, h->F.ensure(all));
    IPHIP(h, h->RC.ensure(all));
    IPHIP(h, h->AF.ensure(all));
    IPHIP(h, h->ARC.ensure(all));
    if (total) IPHIP(h, hipMemcpyAsync(h->ascii.p, ascii, total, hipMemcpyHostToDevice, h->st));
    IPHIP(h, hipMemsetAsync(h->F.p, 0, FRONT_PAD * 8, h->st));
    IPHIP(h, hipMemsetAsync(h->RC.p, 0, FRONT_PAD * 8, h->st));
    IPHIP(h, hipMemsetAsync(h->F.p + FRONT_PAD + nwords, 0, BACK_PAD * 8, h->st));
    IPHIP(h, hipMemsetAsync(h->RC.p + FRONT_PAD + nwords, 0, BACK_PAD * 8, h->st));
    IPHIP(h, hipMemsetAsync(h->AF.p, 0, all * 8, h->st));
    IPHIP(h, hipMemsetAsync(h->ARC.p, 0, all * 8, h->st));
    rcg::launch_pack(h->ascii.p, total, nwords, h->F.p + FRONT_PAD, h->RC.p + FRONT_PAD, h->AF.p + FRONT_PAD,
                     h->ARC.p + FRONT_PAD, h->st);
    IPHIP(h, hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char *ip_error(ip_handle *h) { return (h ? h->err : g_err).c_str(); }

ip_handle *ip_create(void)
{
    ip_handle *h = new ip_handle();
    const hipError_t r = hipStreamCreate(&h->st);
    if (r != hipSuccess) {
        g_err = std::string("hipStreamCreate: ") + hipGetErrorString(r);
        delete h;
        return nullptr;
    }
    return h;
}

void ip_destroy(ip_handle *h)
{
    if (!h) return;
    if (h->st) (void)hipStreamSynchronize(h->st);
    h->scratch.release();
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
    h->bucket.release();
    if (h->st) (void)hipStreamDestroy(h->st);
    delete h;
}

// the sort's tile and segment count and the bucket fill's entries per thread (host only)
void ip_geometry(int *os_tile, int *os_seg, int *bf_per)
{
    if (os_tile) *os_tile = rcg::os_tile_keys();
    if (os_seg) *os_seg = rcg::os_segments();
    if (bf_per) *bf_per = rcg::bucket_fill_per_thread();
}

// words per packed array that ip_pack returns for `total` bases
uint64_t ip_pack_words(uint64_t total) { return pack_words(total); }

// the handle's sort epoch (read only: os_sort_keys alone advances it)
uint32_t ip_epoch(ip_handle *h) { return h ? h->epoch : 0u; }

// out[0, n) = keys[0, n) sorted stably on bits [bb, 64): os_sort_keys, uncounted
int ip_sort(ip_handle *h, const uint64_t *keys, uint64_t n, int bb, uint64_t *out)
{
    if (!h) return fail(nullptr, IP_E_ARG, "null handle");
    if (bb < 0 || bb > 56 || bb % 8) return fail(h, IP_E_ARG, "bb must be a multiple of 8 in [0, 56]");
    if (n && (!keys || !out)) return fail(h, IP_E_ARG, "null array");
    IPHIP(h, h->a.ensure(std::max<uint64_t>(n, 1)));
    IPHIP(h, h->b.ensure(std::max<uint64_t>(n, 1)));
    if (n) IPHIP(h, hipMemcpyAsync(h->a.p, keys, n * 8, hipMemcpyHostToDevice, h->st));
    uint64_t *res = nullptr;
    IPCHK(run_sort(h, n, bb, false, &res));
    if (n) IPHIP(h, hipMemcpyAsync(out, res, n * 8, hipMemcpyDeviceToHost, h->st));
    IPHIP(h, hipStreamSynchronize(h->st));
    return 0;
}

// bucket[0, 2^bits] of sorted[0, n): launch_bucket_fill
int ip_bucket(ip_handle *h, const uint64_t *sorted, uint64_t n, int bits, uint32_t *bucket)
{
    if (!h) return fail(nullptr, IP_E_ARG, "null handle");
    if (bits < 1 || bits > 28) return fail(h, IP_E_ARG, "bits must be in [1, 28]");
    if (n > 0xFFFFFFFFull) return fail(h, IP_E_ARG, "more than 2^32 entries");
    if (!bucket || (n && !sorted)) return fail(h, IP_E_ARG, "null array");
    const uint64_t nb = (1ull << bits) + 1;
    IPHIP(h, h->a.ensure(std::max<uint64_t>(n, 1)));
    IPHIP(h, h->bucket.ensure(nb));
    if (n) IPHIP(h, hipMemcpyAsync(h->a.p, sorted, n * 8, hipMemcpyHostToDevice, h->st));
    // every slot the kernel leaves unwritten shows in the comparison
    IPHIP(h, hipMemsetAsync(h->bucket.p, 0xFF, nb * sizeof(uint32_t), h->st));
    rcg::launch_bucket_fill(h->a.p, n, bits, h->bucket.p, h->st);
    IPHIP(h, hipGetLastError());
    IPHIP(h, hipMemcpyAsync(bucket, h->bucket.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
    IPHIP(h, hipStreamSynchronize(h->st));
    return 0;
}

// F / AF / RC / ARC [0, ip_pack_words(total)) of ascii[0, total): launch_pack
int ip_pack(ip_handle *h, const uint8_t *ascii, uint64_t total, uint64_t *F, uint64_t *AF, uint64_t *RC,
            uint64_t *ARC)
{
    if (!h) return fail(nullptr, IP_E_ARG, "null handle");
    if ((total && !ascii) || !F || !AF || !RC || !ARC) return fail(h, IP_E_ARG, "null array");
    IPCHK(run_pack(h, ascii, total));
    const uint64_t nwords = pack_words(total);
    IPHIP(h, hipMemcpyAsync(F, h->F.p + FRONT_PAD, nwords * 8, hipMemcpyDeviceToHost, h->st));
    IPHIP(h, hipMemcpyAsync(AF, h->AF.p + FRONT_PAD, nwords * 8, hipMemcpyDeviceToHost, h->st));
    IPHIP(h, hipMemcpyAsync(RC, h->RC.p + FRONT_PAD, nwords * 8, hipMemcpyDeviceToHost, h->st));
    IPHIP(h, hipMemcpyAsync(ARC, h->ARC.p + FRONT_PAD, nwords * 8, hipMemcpyDeviceToHost, h->st));
    IPHIP(h, hipStreamSynchronize(h->st));
    return 0;
}

// The sorted index entries of the transcripts (tx_start[t], tx_len[t]) of
// ascii[0, total): pack, fill, sort on the k-mer (bb = 32).
//   path 0: os_fill_hist + counted sort (the engine's default)
//   path 1: launch_kmer_fill(false) + uncounted sort
//   path 2: launch_kmer_count, host scan, launch_kmer_fill(true) + uncounted sort
// ent[0, cap) receives *n entries.
int ip_index(ip_handle *h, const uint8_t *ascii, uint64_t total, const uint64_t *tx_start, const uint32_t *tx_len,
             uint32_t n_tx, int path, uint64_t *ent, uint64_t cap, uint64_t *n_out)
{
    if (!h) return fail(nullptr, IP_E_ARG, "null handle");
    if (path < 0 || path > 2) return fail(h, IP_E_ARG, "path must be 0, 1 or 2");
    if ((total && !ascii) || (n_tx && (!tx_start || !tx_len)) || !n_out || (cap && !ent))
        return fail(h, IP_E_ARG, "null array");
    if (total > 0xFFFFFFFFull) return fail(h, IP_E_ARG, "positions are 32-bit");
    std::vector<TxInfo> tx(n_tx);
    std::vector<uint64_t> off((size_t)n_tx + 1, 0);
    for (uint32_t t = 0; t < n_tx; t++) {
        if (tx_start[t] > total || tx_len[t] > total - tx_start[t])
            return fail(h, IP_E_ARG, "transcript " + std::to_string(t) + " leaves the sequence");
        tx[t] = TxInfo{tx_start[t], tx_len[t], 0};
        off[t + 1] = off[t] + (tx_len[t] >= (uint32_t)rcg::W16 ? tx_len[t] - rcg::W16 + 1 : 0u);
    }
    IPCHK(run_pack(h, ascii, total));
    IPHIP(h, h->tx.ensure((uint64_t)n_tx + 1));
    IPHIP(h, h->koff.ensure((uint64_t)n_tx + 1));
    if (n_tx) IPHIP(h, hipMemcpyAsync(h->tx.p, tx.data(), (size_t)n_tx * sizeof(TxInfo), hipMemcpyHostToDevice, h->st));
    uint64_t n = off[n_tx];
    const uint64_t n_all = n;   // every window: what the fill can write at most
    if (path == 2) {
        // the valid windows per transcript, scanned on the host
        IPHIP(h, h->kcnt.ensure((uint64_t)n_tx + 1));
        IPHIP(h, hipMemsetAsync(h->kcnt.p, 0, ((size_t)n_tx + 1) * 8, h->st));
        if (n_tx) rcg::launch_kmer_count(h->tx.p, n_tx, h->AF.p + FRONT_PAD, h->kcnt.p, h->st);
        IPHIP(h, hipGetLastError());
        std::vector<uint64_t> cnt((size_t)n_tx + 1, 0);
        IPHIP(h, hipMemcpyAsync(cnt.data(), h->kcnt.p, ((size_t)n_tx + 1) * 8, hipMemcpyDeviceToHost, h->st));
        IPHIP(h, hipStreamSynchronize(h->st));
        for (uint32_t t = 0; t < n_tx; t++) {
            // a count above the closed form would let the fill write past the entry array
            if (cnt[t] > off[t + 1] - off[t])
                return fail(h, IP_E_CAP, "kmer_count gave transcript " + std::to_string(t) + " more windows than it has");
        }
        uint64_t acc = 0;
        for (uint32_t t = 0; t <= n_tx; t++) {
            off[t] = acc;
            acc += cnt[t];
        }
        n = off[n_tx];
    }
    if (n > 0xFFFFFFFFull) return fail(h, IP_E_ARG, "more than 2^32 index entries");
    *n_out = n;
    if (n > cap) return fail(h, IP_E_CAP, "index has " + std::to_string(n) + " entries, room for " + std::to_string(cap));
    IPHIP(h, hipMemcpyAsync(h->koff.p, off.data(), ((size_t)n_tx + 1) * 8, hipMemcpyHostToDevice, h->st));
    // room for every window: a fill that disagrees with the counts stays inside the array
    IPHIP(h, h->a.ensure(std::max<uint64_t>(n_all, 1)));
    IPHIP(h, h->b.ensure(std::max<uint64_t>(n_all, 1)));
    // entries the fill leaves unwritten show in the comparison
    IPHIP(h, hipMemsetAsync(h->a.p, 0xFF, std::max<uint64_t>(n_all, 1) * 8, h->st));
    const bool counted = path == 0 && n > 0;   // as build_index_of: an empty index is not counted
    if (counted) {
        IPHIP(h, h->scratch.ensure(rcg::os_scratch_words(n)));
        rcg::os_fill_hist(h->tx.p, n_tx, h->F.p + FRONT_PAD, h->koff.p, h->a.p, n, h->scratch.p, h->st);
    } else if (n_tx) {
        rcg::launch_kmer_fill(path == 2, h->tx.p, n_tx, h->F.p + FRONT_PAD, path == 2 ? h->AF.p + FRONT_PAD : nullptr,
                              h->koff.p, h->a.p, h->st);
    }
    IPHIP(h, hipGetLastError());
    uint64_t *res = nullptr;
    IPCHK(run_sort(h, n, 32, counted, &res));
    if (n) IPHIP(h, hipMemcpyAsync(ent, res, n * 8, hipMemcpyDeviceToHost, h->st));
    IPHIP(h, hipStreamSynchronize(h->st));
    return 0;
}

}  // extern "C"
