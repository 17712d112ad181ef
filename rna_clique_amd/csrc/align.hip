// The extension of seed-and-extend (the BLAST+ replacement; the seeds:
// seed.hip): the order of its passes. Host code only: every kernel lives in
// the unit named with it and is launched from there, through launch.h.
//
//   extend_rows_kernel   each candidate's first seed on a sliding 32-lane
//     (rows.hip)         sub-band row (two rows per wave), greedy X-drop; the
//                        64-lane instantiation continues what outgrew it.
//   first_finish_kernel  one thread per candidate: a search whose seeds all
//     (finish.hip)       lie in the first seed's box is done (cuts, record).
//   later_round_kernel   the other searches, one seed per round: the next
//   later_finish_kernel  seed outside every box goes to the 64-lane rows;
//     (finish.hip)       then purge and cuts, one thread per search.
//   extend_kernel        one wave per search (the full band, seeds by
//     (extend.hip)       selection, purge, cuts): what the rounds cannot take.
//   group_* / mirror_*   per (query gene, subject sample): HSPs made
//     (group.hip)        contiguous in candidate order (the oracle's order).
//
// Semantics: oracle/align_oracle.c ("RC-megablast v1"), bit for bit.
#include "device.h"
#include "launch.h"

namespace rcg {

// Later-seed rounds over the searches first_finish_kernel deferred (shared
// searches; after launch_extend_rows): MAX_HSP rounds of
// later_round_kernel, with the row kernels (32-lane, then the 64-lane pass
// over what outgrew the sliding sub-band) over each round's seeds between
// them. Every count stays on the device: an empty round is a few idle
// launches. cnt: LATER_CNT zeroed counters per round; the work buffers
// (vc, list, box) and the active lists alternate between rounds.
void launch_later_rounds(bool amb, const Db &db, const ExtParams &P, bool rows32_first, const LaterParams &L0,
                         Cand *const vc[2], uint32_t *const list[2], int32_t *const box[2], uint32_t *const act[2],
                         unsigned long long *cnt, hipStream_t st)
{
    if (!L0.n_search) return;
    const bool widep = P.wide0 != nullptr;
    // later seeds nearly all outgrow the 32-lane window (C3v: 15.3 M of 15.3 M,
    // profiles/r06_later): straight to 64-lane rows unless rows32_first
    // (RC_LATER_ROWS=32: the 32-lane pass first)
    for (int r = 0; r < MAX_HSP; r++) {
        unsigned long long *c = cnt + (size_t)r * LATER_CNT;
        LaterParams L = L0;
        L.round = r;
        L.vc = vc[r & 1];
        L.list = list[r & 1];
        L.vc_in = vc[(r + 1) & 1];
        L.box_in = box[(r + 1) & 1];
        L.act_out = act[r & 1];
        L.act_out_n = c + 1;
        L.act_in = act[(r + 1) & 1];
        L.act_in_n = r ? cnt + (size_t)(r - 1) * LATER_CNT + 1 : nullptr;
        L.work_n = c;
        launch_later_round(P, L, st);
        if (r == MAX_HSP - 1) break;   // (every search has MAX_HSP boxes or none to add)
        ExtParams B = P;
        B.which = 0;
        B.cands = vc[r & 1];
        B.cand_box = box[r & 1];
        B.list = list[r & 1];
        B.list_n = c;
        B.work = c + 2;
        if (!rows32_first) {   // RC_LATER_ROWS=64: straight to the spec's whole band
            B.wide = nullptr;
            B.wide_n = nullptr;
            B.resume = nullptr;
            launch_rows(64, false, amb, db, B, st);
            continue;
        }
        B.wide = widep ? P.wide0 : nullptr;
        B.wide_n = c + 3;
        B.resume = widep ? P.resume : nullptr;
        launch_rows(32, B.resume != nullptr, amb, db, B, st);
        if (widep) {
            ExtParams V = B;
            V.list = P.wide0;
            V.list_n = c + 3;
            V.work = c + 4;
            V.wide = nullptr;
            V.wide_n = nullptr;
            launch_rows(64, false, amb, db, V, st);
        }
    }
}

// Row kernels (first seeds) over all candidates, then first_finish_kernel
// (the caller sizes the HSP overflow buffer from the defer counts, then
// launch_extend_retry)
void launch_extend_rows(bool amb, const Db &db, const ExtParams &P, hipStream_t st)
{
    if (P.n_cand == 0) return;
    ExtParams W = P;
    W.list = nullptr;
    W.list_n = nullptr;
    // saved extension states: only the shared-search 32-lane passes write
    // them and only their 64-lane passes read them
    W.resume = nullptr;
    if (P.share) {
        // shared searches: first seeds e0 over every candidate, then e1 over
        // list2 (reverse searches whose first seed is another seed), then each
        // directed search checked (or listed for extend_kernel) on its own
        // each 32-lane pass is followed by a 64-lane pass (the spec's whole
        // band) over the candidates whose live diagonals outgrew the sliding
        // sub-band. Most of them also have seeds outside the first box;
        // extend_kernel starts those searches from the first seed's HSP, so
        // the 64-lane pass is not redone: C3v 806 vs 875 ms per step.
        const bool widep = P.wide0 != nullptr;
        auto wide_pass = [&](const ExtParams &B, uint32_t *lst, unsigned long long *lst_n, unsigned long long *wk) {
            ExtParams V = B;
            V.list = lst;
            V.list_n = lst_n;
            V.work = wk;
            V.wide = nullptr;
            V.wide_n = nullptr;
            launch_rows(64, false, amb, db, V, st);
        };
        W.which = 0;
        W.wide = widep ? P.wide0 : nullptr;
        W.wide_n = P.wide0_n;
        W.resume = widep ? P.resume : nullptr;
        auto rows_pass = [&](const ExtParams &B) { launch_rows(32, B.resume != nullptr, amb, db, B, st); };
        rows_pass(W);
        if (widep) wide_pass(W, P.wide0, P.wide0_n, P.work_w0);
        ExtParams W2 = W;
        W2.which = 1;
        W2.list = P.list2;
        W2.list_n = P.list2_n;
        W2.work = P.work3;
        W2.wide = widep ? P.wide1 : nullptr;
        W2.wide_n = P.wide1_n;
        rows_pass(W2);
        if (widep) wide_pass(W2, P.wide1, P.wide1_n, P.work_w1);
        W.list = nullptr;
        W.list_n = nullptr;
        launch_first_finish(W, st);
        return;
    }
    // independent searches / spec 5b: 32-lane rows over every candidate
    launch_rows(32, false, amb, db, W, st);
    launch_first_finish(W, st);
}

}  // namespace rcg
