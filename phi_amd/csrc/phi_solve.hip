// phi_solve.hip -- stages 2b-3 of ILP_function (src/ILP_index.cpp:670-1525) behind phi_solve().
//
// Host orchestration of GPU kernels:
//   1. match + shared-anchor filter                      (anchors.hip)    <- :643-743
//   2. exact solve replacing model.optimize() (:1418):   (dp.hip)
//        The reference objective counts each minimiser at most once (z_i, :830/:876):
//            true(P) = #{i : some anchor of i traversed by P} - 2*(R/2) * #recombinations(P).
//        The DP maximises an ADDITIVE score sum_a w_a [a traversed] - cost.  Used three ways:
//          upper bound   for any set S of minimisers:  true(P) <= |S| + DP(w = 1 outside S, 0 on S)
//          lower bound   true(P) of any path the DP returns
//          branching     OPT = max over "minimiser i is counted only at cluster c of its anchors"
//                        (clusters = groups of pairwise mutually exclusive anchors), each child
//                        again solved by the DP with the other clusters' weights set to 0.
//        The root closes with one DP run when the optimal path traverses no minimiser twice and
//        typically with two or three otherwise (S := the doubly-counted minimisers).
//   3. decode (:1431-1525): path vertices / haplotype labels, recombination count.
//
// The file, top to bottom:
//   * the walk entries as the host reads them, phi_host_anchors;
//   * dp_prepare_blocks: the cuts of the chain of compact steps, once per solve (and again on a fallback);
//   * run_dp: one DP run = per-run event records, then one of blocks on class lanes / blocks on walk lanes / the whole
//     event chain / the dense kernel, then end pick and backtrack; a strategy that cannot finish names a DpRetry, and the
//     loop at the top of run_dp acts on it;
//   * struct Solve and the stages of phi_solve_impl, in the order it calls them: read_spectrum, match_and_compact,
//     filter_shared_anchors, expand_kept_records, check_anchors_choose_mode, anchors_to_host, anchor_entry_csr,
//     check_score_range, dp_inputs, anchors_of_minimisers, repeat_set, search (search_node: weights, run_dp, path cover,
//     bound, tighten, branch, children; to_host ends device mode), decode.
// The rules among these that need no GPU -- block placement, the max-plus chain, the host anchor arrays, the score bound, the
// minimiser -> anchors map, repeats, clusters, tighten and branch -- are plain host code in solve_host.h, checked stand-alone
// by host/solve_host_selftest.cpp.
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <set>
#include <unordered_map>
#include "phi_ctx.h"
#include "phi_dev.h"

// The walk entries as the solve's host code reads them: from the context's host copy, or -- a chromosome-scale graph keeps none
// (phi_set_graph) -- from the device copy: single entries for the backtrack, whole stretches for the decoded path.
static bool have_host_walks(const phi_ctx *c) { return (int64_t)c->h_walk_vtx.size() == c->n_entries; }
static int walk_vtx_at(phi_ctx *c, int64_t e, int32_t *v)
{
    if (have_host_walks(c)) { *v = c->h_walk_vtx[(size_t)e]; return PHI_OK; }
    return phi_hip_check(c, phi_copy_sync(c, v, c->d_walk_vtx.as<int32_t>() + e, 4, hipMemcpyDeviceToHost), "walk entry D2H");
}
static int walk_vtx_range(phi_ctx *c, int64_t es, int64_t n, int32_t *dst)
{
    if (have_host_walks(c)) { memcpy(dst, c->h_walk_vtx.data() + es, (size_t)n * 4); return PHI_OK; }
    return phi_hip_check(c, phi_copy_sync(c, dst, c->d_walk_vtx.as<int32_t>() + es, (size_t)n * 4, hipMemcpyDeviceToHost), "walk entries D2H");
}
// (the branch and bound proper and the host-side score bound index the array freely: fetched whole, once)
static int ensure_host_walks(phi_ctx *c)
{
    if (have_host_walks(c)) return PHI_OK;
    if (!c->h_walk_vtx.resize((size_t)c->n_entries)) return phi_fail(c, PHI_ERR_NOMEM, "host allocation failed");
    return phi_hip_check(c, phi_copy_sync(c, c->h_walk_vtx.data(), c->d_walk_vtx.p, (size_t)c->n_entries * 4, hipMemcpyDeviceToHost), "walk entries D2H");
}

struct Seg { int32_t h; int64_t es, ee; };     // path segment: walk h, entries es..ee (inclusive)

// the host copy of the kept anchors (a large model is solved on the device copy: solve_dev.hip)
int phi_host_anchors(phi_ctx *c)
{
    if (c->anchors_host) return PHI_OK;
    const int64_t n = c->n_kept;
    PHICHK(phi_pin_ensure(c, (size_t)std::max<int64_t>(n, 1) * sizeof(PhiAnchorHost)));
    c->h_kept = PhiAnchorSpan{static_cast<PhiAnchorHost *>(c->h_pin), n};
    if (n) HIPCHK(hipMemcpyAsync(c->h_kept.p, c->d_anchors.p, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->h_dp_own.clear();
    c->h_dp = c->h_kept;                                       // (device mode only runs when every kept anchor spans an edge)
    c->anchors_host = true;
    return PHI_OK;
}

// ------------------------------------------------------------------------------------------ blocks of steps
// Up to 64 walks: cut the chain of compact steps into blocks that the DP kernel solves in parallel (dp_events.hip
// DP_ROW / DP_PATH).  A cut may sit before step k when the graph allows it (phi_set_graph: no recombination edge from
// before the cut, not inside a pair of allele steps) and, on every walk, some entry between the walk's events around the
// cut is split by no dp anchor -- found here, once per solve, from all dp anchors whatever their weights.  Where the cuts
// go is phi_place_blocks of solve_host.h; the kernels, the tables and the switches are here.
static int dp_prepare_blocks(phi_ctx *c, int64_t n_dp)
{
    c->dp_blocks = false;
    c->n_blk = 0;
    c->dp_cls = false;
    if (!c->dp_events || c->n_walks > PHI_DP_EVENT_MAX_WALKS || getenv("PHI_DP_NOBLOCKS") || c->n_k < 4) return PHI_OK;
    // more than 64 walks: short blocks, whose rows run on class lanes (dp_events.hip); few sites per block keep the
    // walks of a block in at most 64 classes
    const bool cls = c->n_walks > 64;
    c->blk_ls = cls ? 256 : 64;
    const int64_t ne = c->n_entries;
    const int32_t nk = c->n_k;
    // (scratch of ne + 3 ints twice: the per-run prefix-sum buffers, which no run is using yet -- at chromosome scale
    //  every buffer of this size is 5 GB that the driver clears on allocation)
    PHICHK(phi_dev_ensure(c, c->d_off_end, (size_t)(ne + 3) * 4));
    PHICHK(phi_dev_ensure(c, c->d_off_start, (size_t)(ne + 3) * 4));
    PHICHK(phi_dev_ensure(c, c->d_stepdiff, (size_t)(nk + 2) * 4));
    int32_t *d_a = c->d_off_end.as<int32_t>(), *d_b = c->d_off_start.as<int32_t>();
    HIPCHK(hipMemsetAsync(c->d_stepdiff.p, 0, (size_t)(nk + 2) * 4, c->stream));
    if (getenv("PHI_CUT_COUNTED")) {                                   // (tests: the flags from counted coverage, as until round 4)
        HIPCHK(hipMemsetAsync(d_a, 0, (size_t)(ne + 3) * 4, c->stream));
        phi_launch_cut_cov(c->stream, c->d_a_e1.as<phi_ent_t>(), c->d_g_span.as<uint8_t>(), n_dp, d_a);
        PHICHK(phi_scan(c, d_a, ne + 1, d_b));                                                                               // d_b[e + 1] = anchors a cut before e splits
        phi_launch_cut_clean(c->stream, d_b, ne, d_a);                                                                       // d_a[e] = clean
    } else {
        phi_launch_cut_clean_direct(c->stream, c->d_g_off.as<int64_t>(), c->d_g_span.as<uint8_t>(), ne, d_a);               // d_a[e] = clean
    }
    PHICHK(phi_scan(c, d_a, ne + 1, d_b));                                                                                   // d_b[e] = clean entries before e
    phi_launch_cut_events(c->stream, c->d_ev_e.as<phi_ent_t>(), c->n_ev, c->d_ev_off.as<int64_t>(), c->d_walk_off.as<int64_t>(), c->n_walks,
                          c->d_walk_vtx.as<int32_t>(), c->d_cvtx.as<int32_t>(), d_b, c->d_stepdiff.as<int32_t>());
    std::vector<int32_t> closed((size_t)nk + 2);
    HIPCHK(hipMemcpyAsync(closed.data(), c->d_stepdiff.p, (size_t)(nk + 2) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int32_t k = 1; k <= nk + 1; k++) closed[(size_t)k] += closed[(size_t)k - 1];          // > 0: some walk forbids a cut before step k
    const PhiCutFlags cut_ok{c->h_k_cut_ok.data(), closed.data(), nk};
    if (getenv("PHI_TIMING")) {
        int64_t n_struct = 0, n_both = 0, longest = 0, run = 0, longest_s = 0, run_s = 0;
        for (int32_t k = 1; k < nk; k++) {
            n_struct += c->h_k_cut_ok[(size_t)k] != 0;
            if (cut_ok(k)) { n_both++; run = 0; } else longest = std::max(longest, ++run);
            if (c->h_k_cut_ok[(size_t)k]) run_s = 0; else longest_s = std::max(longest_s, ++run_s);
        }
        fprintf(stderr, "[phi timing] solve: cuts: %lld of %d steps allowed by the graph (longest closed stretch %lld), %lld also clean of anchors (longest closed stretch %lld)\n",
                (long long)n_struct, nk, (long long)longest_s, (long long)n_both, (long long)longest);
    }
    // block length: enough blocks to fill the machine with (walks + 1) tasks each, few enough to keep the chain short;
    // a block is at most as long as its ring of tops: 1024 steps, or 2048 where the longest stretch without a cut needs it
    // (256-step blocks first: their tasks take 51 instead of 69 KB of LDS, three per CU; their queues hold 8 live runs
    //  per lane, and a solve that meets more comes back here with blk_no_small set)
    const int32_t rings_walk[] = {256, 1024, 2048}, rings_cls[] = {256, 512};
    static_assert(PHI_DP_BLOCK_MAX == 2048, "the largest ring of tops");
    const int32_t ring = phi_place_blocks(cut_ok, cls ? rings_cls : rings_walk, cls ? 2 : 3, c->blk_no_small, [&](int32_t ring_) {
        int64_t target = (int64_t)nk * (c->n_walks + 1) / 4096;
        target = std::max<int64_t>(64, std::min<int64_t>(ring_ / 2, target));
        if (cls) target = c->blk_cls_target;
        if (const char *e = getenv("PHI_DP_BLOCK_STEPS")) target = std::max(1, std::min(ring_, atoi(e)));   // tests: many small blocks
        return target;
    }, c->h_blk_lo);
    if (!ring) return PHI_OK;                                  // the chain stays whole
    c->blk_ring = ring;
    c->n_blk = (int32_t)c->h_blk_lo.size() - 1;
    if (c->n_blk < 2) { c->n_blk = 0; return PHI_OK; }
    c->blk_max_len = 0;
    for (int32_t b = 0; b < c->n_blk; b++) c->blk_max_len = std::max(c->blk_max_len, c->h_blk_lo[(size_t)b + 1] - c->h_blk_lo[(size_t)b]);
    const size_t nbk = (size_t)c->n_blk, ls = (size_t)c->blk_ls, nrow = cls ? 65 : (size_t)(c->n_walks + 1);
    PHICHK(phi_dev_ensure(c, c->d_blk_lo, (nbk + 1) * 4));
    PHICHK(phi_dev_ensure(c, c->d_blk_ev, nbk * ls * 4));
    PHICHK(phi_dev_ensure(c, c->d_blk_S, nbk * ls * 4));
    PHICHK(phi_dev_ensure(c, c->d_blk_keys, nbk * ls * 4));
    PHICHK(phi_dev_ensure(c, c->d_blk_carry, nbk * ls * 4));
    {
        // The chain over class-lane blocks adds "no value" (NEGK) to whatever lies in the rows of class lanes a block does not
        // use, without looking: that must be a value NEGK can be added to -- not what an earlier owner of the memory left there
        // (found when a freed buffer of segment rows, holding sums of two NEGK, came back as this table: NEGK + INT32_MIN wraps
        // into a valid key).  A table allocated anew is filled with 0xC0C0C0C0 (below NEGK / 2, and NEGK plus it stays inside
        // int32); afterwards only keys and NEGK are written into it.  "Anew" is the buffer's generation, not its address: a
        // table below the pool's threshold goes back to the driver, and the larger one may come back at the same address.
        const uint32_t before = c->d_row_out.gen;
        PHICHK(phi_dev_ensure(c, c->d_row_out, nbk * nrow * 64 * 4));
        if (c->d_row_out.gen != before) HIPCHK(hipMemsetAsync(c->d_row_out.p, 0xC0, c->d_row_out.cap, c->stream));
    }
    PHICHK(phi_dev_ensure(c, c->d_rowend, nbk * nrow * 4));
    if (cls) {
        PHICHK(phi_dev_ensure(c, c->d_lane_walk, nbk * 64 * 4));
        PHICHK(phi_dev_ensure(c, c->d_walk_lane, nbk * ls * 4));
        PHICHK(phi_dev_ensure(c, c->d_coff, nbk * ls * 4));
        PHICHK(phi_dev_ensure(c, c->d_blk_ncls, nbk * 4));
        PHICHK(phi_dev_ensure(c, c->d_rownew, nbk * nrow * 4));
        PHICHK(phi_dev_ensure(c, c->d_rowdiag, nbk * 64 * 4));
        PHICHK(phi_dev_ensure(c, c->d_blk_bad, 64));
    }
    HIPCHK(hipMemcpyAsync(c->d_blk_lo.p, c->h_blk_lo.data(), (nbk + 1) * 4, hipMemcpyHostToDevice, c->stream));
    phi_launch_blk_ev(c->stream, c->d_blk_lo.as<int32_t>(), c->n_blk, c->d_ev_e.as<phi_ent_t>(), c->d_ev_off.as<int64_t>(), c->n_walks,
                      c->d_walk_vtx.as<int32_t>(), c->d_cvtx.as<int32_t>(), c->d_blk_ev.as<int32_t>());
    HIPCHK(hipStreamSynchronize(c->stream));                   // h_blk_lo is a member, but the launch above must have its copy
    c->dp_blocks = true;
    c->dp_cls = cls;
    if (getenv("PHI_TIMING")) fprintf(stderr, "[phi timing] solve: %d compact steps in %d blocks (rings of %d steps)%s\n", nk, c->n_blk, c->blk_ring, cls ? ", rows on class lanes" : "");
    return PHI_OK;
}

// ------------------------------------------------------------------------------------------ DP
struct DpHost {
    std::vector<int32_t> ends, bstart, ent_u, ent_h;
    std::vector<int32_t> rows, rowend, S, keys, carry;          // blocks in parallel: transfer rows, entry vectors, what the blocks report
};

// what every kernel of a DP run writes and the backtrack reads
struct DpOut {
    int32_t n_ent;                                             // length of the per-step outputs
    int32_t *dmax, *bstart, *ent_src, *ent_h;
};
static DpOut dp_out(const phi_ctx *c)
{
    const int32_t n_ent = c->dp_events ? c->n_k : c->n_vtx;
    return DpOut{n_ent, c->d_dmax.as<int32_t>(), c->d_bstart.as<int32_t>(), c->d_ent.as<int32_t>(), c->d_ent.as<int32_t>() + n_ent};
}

// What a DP run that could not finish asks of run_dp before the next attempt.  The first three come from the block
// strategies (dp_blocks_fallback), the last from the end fetch (dp_fetch_ends).
enum DpRetry {
    DP_DONE = 0,
    DP_HALVE_CLASS_TARGET,      // halve the class target and place blocks again
    DP_NO_SMALL_BLOCKS,         // no 256-step blocks: place blocks again
    DP_GIVE_UP_BLOCKS,          // the whole chain from now on
    DP_DENSE                    // event queue overflow: the every-vertex kernel from now on
};

// per run: prefix sums of the anchor weights -> one record per event (phi_dp_event_fill_kernel); A: what every event kernel takes
static int dp_event_records(phi_ctx *c, const DpOut &O, PhiDpEventArgs &A, PhiStageTimer &tr)
{
    const int64_t n_dp = c->n_dp;
    PHICHK(phi_dev_ensure(c, c->d_wpre, (size_t)(n_dp + 1) * 4));
    PHICHK(phi_scan(c, c->d_a_weight.as<uint8_t>(), n_dp, c->d_wpre.as<int32_t>()));
    A.n_k = c->n_k; A.n_walks = c->n_walks; A.n_ev = c->n_ev;
    A.k_rec = c->d_k_rec.as<int32_t>(); A.k_in_packed = c->d_k_in.as<int32_t>();
    A.walk_off = c->d_walk_off.as<int64_t>();
    A.ev_e = c->d_ev_e.as<phi_ent_t>(); A.ev_off = c->d_ev_off.as<int64_t>();
    A.ev = c->d_ev.p;
    A.g_off = c->d_g_off.as<int64_t>(); A.g_span = c->d_g_span.as<uint8_t>(); A.a_weight = c->d_a_weight.as<uint8_t>();
    A.cost = 2 * (c->recombination / 2);                   // (c_1/2) twice, ILP_index.cpp:1276,1299
    A.dmax = O.dmax; A.bstart = O.bstart;
    A.tops = c->d_top.as<int32_t>();
    A.ent_src = O.ent_src; A.ent_h = O.ent_h;
    A.err = (uint32_t *)(c->d_scalars.as<uint64_t>() + S_ERR);
    A.q_limit = getenv("PHI_DP_QLIMIT") ? atoi(getenv("PHI_DP_QLIMIT")) : 0;      // tests: provoke the fallback
    phi_launch_dp_event_fill(c->stream, A, c->d_e_out.as<uint8_t>(), c->d_walk_vtx.as<int32_t>(), c->d_cvtx.as<int32_t>(),
                             c->d_a_e1.as<phi_ent_t>(), c->d_wpre.as<int32_t>(), c->n_entries);
    if (tr.on) { (void)hipStreamSynchronize(c->stream); tr.lap("weights + per-run records"); }
    A.lane_stride = c->blk_ls;
    return PHI_OK;
}

// the tables of the blocks that both block strategies pass to their kernels
static void dp_block_args(const phi_ctx *c, PhiDpEventArgs &A)
{
    A.n_blk = c->n_blk; A.blk_ring = c->blk_ring; A.blk_max_len = c->blk_max_len; A.blk_lo = c->d_blk_lo.as<int32_t>(); A.blk_ev = c->d_blk_ev.as<int32_t>(); A.blk_S = c->d_blk_S.as<int32_t>();
    A.row_out = c->d_row_out.as<int32_t>(); A.rowend_out = c->d_rowend.as<int32_t>();
    A.blk_keys_out = c->d_blk_keys.as<int32_t>(); A.blk_carry = c->d_blk_carry.as<int32_t>();
}

// The kernels of a block strategy raised `bit`: the error word is cleared, and *want says how run_dp goes on.
static int dp_blocks_fallback(phi_ctx *c, uint32_t kerr, uint32_t bit, DpRetry *want)
{
    // (both flags: block tasks that ran on clamped classes may have overflowed their queues as well)
    kerr &= ~(bit | PHI_KERR_DP_QUEUE | PHI_KERR_DP_CLASSES);
    HIPCHK(phi_copy_sync(c, c->d_scalars.as<uint64_t>() + S_ERR, &kerr, 4, hipMemcpyHostToDevice));
    // a block with more than 64 classes of walks (denser variation than the block length was chosen for):
    // shorter blocks hold fewer sites; only below two steps per block does the whole chain take over
    if (bit == PHI_KERR_DP_CLASSES && c->blk_cls_target > 2 && !getenv("PHI_DP_BLOCK_STEPS")) { *want = DP_HALVE_CLASS_TARGET; return PHI_OK; }
    // more than 8 live runs on a lane of a 256-step block task: the longer blocks have queues of 16
    if (bit == PHI_KERR_DP_QUEUE && c->blk_ring <= 256 && !c->blk_no_small) { *want = DP_NO_SMALL_BLOCKS; return PHI_OK; }
    if (getenv("PHI_DP_STRICT")) return phi_fail(c, PHI_ERR_DEVICE, "DP blocks given up (kernel flag %u) under PHI_DP_STRICT", bit);   // tests
    *want = DP_GIVE_UP_BLOCKS;
    return PHI_OK;
}

// the chain over the class-lane blocks: one workgroup, 1.1 us per block -- or, from a few thousand blocks on, cut into segments
// whose matrices are made in parallel, chained, and replayed in parallel (dp_blocks.hip; PHI_DP_CHAIN_SEGMENTS: tests)
static int dp_chain_class_rows(phi_ctx *c, const PhiBlkClassArgs &G, const PhiDpEventArgs &A)
{
    const int32_t nb = c->n_blk;
    int32_t n_seg = nb >= 4096 ? std::min<int32_t>(64, nb / 1024) : 0;
    if (const char *e = getenv("PHI_DP_CHAIN_SEGMENTS")) n_seg = std::max(0, std::min(atoi(e), nb));
    if (n_seg >= 2) {
        std::vector<int32_t> seg_lo((size_t)n_seg + 1);
        for (int32_t g_ = 0; g_ <= n_seg; g_++) seg_lo[(size_t)g_] = (int32_t)((int64_t)nb * g_ / n_seg);
        PHICHK(phi_dev_ensure(c, c->d_seg_lo, ((size_t)n_seg + 1) * 4));
        PHICHK(phi_dev_ensure(c, c->d_seg_row, (size_t)n_seg * (size_t)(c->n_walks + 1) * (size_t)c->blk_ls * 4));
        PHICHK(phi_dev_ensure(c, c->d_seg_S, (size_t)n_seg * (size_t)c->blk_ls * 4));
        HIPCHK(phi_copy_sync(c, c->d_seg_lo.p, seg_lo.data(), seg_lo.size() * 4, hipMemcpyHostToDevice));
        phi_launch_blk_chain_segments(c->stream, G, A.row_out, A.rownew_out, A.rowdiag_out, c->d_blk_S.as<int32_t>(), n_seg,
                                      c->d_seg_lo.as<int32_t>(), c->d_seg_row.as<int32_t>(), c->d_seg_S.as<int32_t>());
    } else {
        phi_launch_blk_chain(c->stream, G, A.row_out, A.rownew_out, A.rowdiag_out, c->d_blk_S.as<int32_t>());
    }
    HIPCHK(hipGetLastError());
    return PHI_OK;
}

// More than 64 walks.  1. the walks of every block in classes (this run's weights); 2. every block from every class
// lane: rows of its transfer matrix; 3. the chain over the blocks, on the device; 4. the blocks again, on walk lanes,
// from their true entry vectors; 5. the two passes must agree
static int dp_blocks_on_class_lanes(phi_ctx *c, PhiDpEventArgs &A, PhiStageTimer &tr, DpRetry *want)
{
    const int32_t nb = c->n_blk;
    dp_block_args(c, A);
    A.rownew_out = c->d_rownew.as<int32_t>();
    A.rowdiag_out = c->d_rowdiag.as<int32_t>();
    A.lane_walk = c->d_lane_walk.as<int32_t>();
    PhiBlkClassArgs G{};
    G.n_blk = nb; G.n_walks = c->n_walks; G.lane_stride = c->blk_ls;
    G.blk_lo = A.blk_lo; G.blk_ev = A.blk_ev; G.ev_off = A.ev_off; G.walk_off = A.walk_off; G.ev = A.ev;
    G.lane_walk = c->d_lane_walk.as<int32_t>(); G.walk_lane = c->d_walk_lane.as<int32_t>(); G.coff = c->d_coff.as<int32_t>();
    G.blk_ncls = c->d_blk_ncls.as<int32_t>(); G.err = A.err;
    phi_launch_blk_classes(c->stream, G);
    uint32_t kerr = 0;
    if (tr.on) {
        HIPCHK(hipMemcpyAsync(&kerr, c->d_scalars.as<uint64_t>() + S_ERR, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        tr.lap("block classes");
        if (kerr & PHI_KERR_DP_CLASSES) return dp_blocks_fallback(c, kerr, PHI_KERR_DP_CLASSES, want);
    }
    phi_launch_dp_block_rows(c->stream, A);
    if (tr.on) { (void)hipStreamSynchronize(c->stream); tr.lap("block rows"); }
    PHICHK(dp_chain_class_rows(c, G, A));
    if (tr.on) { (void)hipStreamSynchronize(c->stream); tr.lap("block chain"); }
    A.lane_walk = nullptr;
    phi_launch_dp_block_paths_wide(c->stream, A);
    int32_t bad[2] = {0, INT32_MAX};
    HIPCHK(hipMemcpyAsync(c->d_blk_bad.p, bad, 8, hipMemcpyHostToDevice, c->stream));
    phi_launch_blk_check(c->stream, A.blk_keys_out, A.blk_S, nb, c->blk_ls, c->n_walks, c->d_blk_bad.as<int32_t>());
    HIPCHK(hipMemcpyAsync(bad, c->d_blk_bad.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&kerr, c->d_scalars.as<uint64_t>() + S_ERR, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (tr.on) tr.lap("block paths + check");
    if (kerr & PHI_KERR_DP_CLASSES) return dp_blocks_fallback(c, kerr, PHI_KERR_DP_CLASSES, want);   // (rows and chain ran on clamped classes: void)
    if (kerr & PHI_KERR_DP_QUEUE) return dp_blocks_fallback(c, kerr, PHI_KERR_DP_QUEUE, want);
    if (bad[0])
        return phi_fail(c, PHI_ERR_DEVICE, "DP blocks: %d keys leaving blocks (first in block %d) differ from the chained class rows (internal error)", bad[0], bad[1]);
    return PHI_OK;
}

// Up to 64 walks.  1. every block from every entry walk (and from the walk starts inside it): rows of its transfer
// matrix; 2. the max-plus chain over them, on the host (phi_chain_blocks); 3. the blocks again, in parallel, each from
// its true entry vector: everything the backtrack reads; 4. the two passes must agree on what leaves every block (and
// so on the chain as a whole)
static int dp_blocks_on_walk_lanes(phi_ctx *c, PhiDpEventArgs &A, DpHost &H, PhiStageTimer &tr, DpRetry *want)
{
    const int32_t nb = c->n_blk, nwk = c->n_walks, nrow = nwk + 1;
    dp_block_args(c, A);
    phi_launch_dp_block_rows(c->stream, A);
    H.rows.resize((size_t)nb * nrow * 64); H.rowend.resize((size_t)nb * nrow);
    HIPCHK(hipMemcpyAsync(H.rows.data(), A.row_out, H.rows.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(H.rowend.data(), A.rowend_out, H.rowend.size() * 4, hipMemcpyDeviceToHost, c->stream));
    uint32_t kerr = 0;
    HIPCHK(hipMemcpyAsync(&kerr, c->d_scalars.as<uint64_t>() + S_ERR, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (tr.on) tr.lap("block rows");
    if (kerr & PHI_KERR_DP_QUEUE) return dp_blocks_fallback(c, kerr, PHI_KERR_DP_QUEUE, want);   // (more live runs than a block task's queue holds)
    (void)phi_chain_blocks(H.rows.data(), H.rowend.data(), nb, nwk, H.S);      // (the value of the best path is read off the second pass)
    HIPCHK(hipMemcpyAsync(c->d_blk_S.p, H.S.data(), H.S.size() * 4, hipMemcpyHostToDevice, c->stream));
    phi_launch_dp_block_paths(c->stream, A);
    H.keys.resize((size_t)nb * 64); H.carry.resize((size_t)nb * 64);
    HIPCHK(hipMemcpyAsync(H.keys.data(), A.blk_keys_out, H.keys.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(H.carry.data(), A.blk_carry, H.carry.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&kerr, c->d_scalars.as<uint64_t>() + S_ERR, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (kerr & PHI_KERR_DP_QUEUE) return dp_blocks_fallback(c, kerr, PHI_KERR_DP_QUEUE, want);
    int32_t b = 0, h = 0, got = 0, wanted = 0;
    if (!phi_chain_agrees(H.S.data(), H.keys.data(), nb, nwk, &b, &h, &got, &wanted))
        return phi_fail(c, PHI_ERR_DEVICE, "DP blocks: block %d leaves key %d on walk %d, the chained matrices say %d (internal error)", b, got, h, wanted);
    return PHI_OK;
}

// the every-vertex kernel of dp.hip
static int dp_dense(phi_ctx *c, const DpOut &O)
{
    PHICHK(phi_dev_ensure(c, c->d_word, (size_t)c->n_entries * 8));          // (only the every-vertex kernel needs it)
    phi_launch_dp_words(c->stream, c->d_e_out.as<uint8_t>(), c->d_g_off.as<int64_t>(), c->d_g_span.as<uint8_t>(),
                        c->d_a_weight.as<uint8_t>(), c->n_entries, c->d_word.as<uint64_t>());
    PhiDpArgs A{};
    A.n_vtx = c->n_vtx; A.n_walks = c->n_walks;
    A.st_rec = c->d_st_rec.as<int32_t>(); A.st_mask = c->d_st_mask.as<unsigned long long>();
    A.in_packed = c->d_in_packed.as<int32_t>();
    A.walk_off = c->d_walk_off.as<int64_t>();
    A.word = c->d_word.as<uint64_t>();
    A.g_off = c->d_g_off.as<int64_t>(); A.g_span = c->d_g_span.as<uint8_t>(); A.a_weight = c->d_a_weight.as<uint8_t>();
    A.cost = 2 * (c->recombination / 2);
    A.dmax = O.dmax; A.bstart = O.bstart;
    A.tops = c->d_top.as<int32_t>();
    A.ent_src = O.ent_src; A.ent_h = O.ent_h;
    phi_launch_dp(c->stream, A);
    return PHI_OK;
}

// the DP's value at the last entry of every walk, and the event kernels' error word
static int dp_fetch_ends(phi_ctx *c, const DpOut &O, bool events, DpHost &H, PhiStageTimer &tr, DpRetry *want)
{
    H.ends.resize(c->n_walks);
    phi_launch_gather_i32(c->stream, O.dmax, c->d_walk_last.as<phi_ent_t>(), c->n_walks, c->d_list3.as<int32_t>());
    HIPCHK(hipMemcpyAsync(H.ends.data(), c->d_list3.p, (size_t)c->n_walks * 4, hipMemcpyDeviceToHost, c->stream));
    uint32_t kerr = 0;
    if (events) HIPCHK(hipMemcpyAsync(&kerr, c->d_scalars.as<uint64_t>() + S_ERR, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    tr.lap("kernel");
    if (kerr & PHI_KERR_DP_QUEUE) {
        // a lane of the four-wave event kernel had more live runs than its queue holds: this graph takes
        // the every-vertex kernel from now on
        kerr &= ~PHI_KERR_DP_QUEUE;
        HIPCHK(phi_copy_sync(c, c->d_scalars.as<uint64_t>() + S_ERR, &kerr, 4, hipMemcpyHostToDevice));
        if (!c->dp_dense_ready) return phi_fail(c, PHI_ERR_DEVICE, "event DP queue overflow without a dense fallback (internal error)");
        *want = DP_DENSE;
    }
    return PHI_OK;
}

// end at (last(h), h) for the best h; ties go to the lowest walk id
static int dp_pick_end(phi_ctx *c, const DpHost &H, int32_t *bh_, int64_t *value)
{
    int32_t bh = -1;
    int64_t best = INT64_MIN;
    for (int32_t h = 0; h < c->n_walks; h++) {
        const int32_t d = H.ends[h];
        if (d > -(1 << 28) && d > best) { best = d; bh = h; }
    }
    if (bh < 0) return phi_fail(c, PHI_ERR_DEVICE, "DP found no s->e path (internal error)");
    *bh_ = bh;
    *value = best;
    return PHI_OK;
}

// entry of walk h on vertex u, whose topological rank is `rank` (ranks increase along a walk); -1: the walk is not on u
static int entry_on_vertex(phi_ctx *c, int32_t h, int32_t rank, int32_t u, int64_t *e_)
{
    int64_t lo = c->h_walk_off[h], hi = c->h_walk_off[h + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        int32_t vm = 0;
        PHICHK(walk_vtx_at(c, mid, &vm));
        if (c->h_topo_rank[vm] < rank) lo = mid + 1; else hi = mid;
    }
    *e_ = -1;
    if (lo < c->h_walk_off[h + 1]) {
        int32_t vl = 0;
        PHICHK(walk_vtx_at(c, lo, &vl));
        if (vl == u) *e_ = lo;
    }
    return PHI_OK;
}

// The argmax path back from the last entry of walk h.  Backtracking touches a handful of entries (two per haplotype
// switch): read them one by one instead of downloading them per walk entry; a path with very many switches (tiny R)
// falls back to one bulk download.
static int dp_backtrack(phi_ctx *c, const DpOut &O, bool events, DpHost &H, int32_t h, std::vector<Seg> *segs)
{
    bool bulk = false;
    auto fetch_bulk = [&]() -> int {
        H.bstart.resize(c->n_entries); H.ent_u.resize(O.n_ent); H.ent_h.resize(O.n_ent);
        HIPCHK(hipMemcpyAsync(H.bstart.data(), O.bstart, (size_t)c->n_entries * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(H.ent_u.data(), O.ent_src, (size_t)O.n_ent * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(H.ent_h.data(), O.ent_h, (size_t)O.n_ent * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        bulk = true;
        return PHI_OK;
    };
    segs->clear();
    int64_t e = c->h_walk_off[h + 1] - 1;
    for (int64_t guard = 0; guard <= (int64_t)c->n_vtx; guard++) {
        if (!bulk && guard == 64) PHICHK(fetch_bulk());
        int32_t bs = 0;
        if (bulk) bs = H.bstart[e];
        else HIPCHK(phi_copy_sync(c, &bs, O.bstart + e, 4, hipMemcpyDeviceToHost));
        if (bs < 0 && c->dp_blocks && events) {
            // the run crossed into its block: follow it back through the blocks it was carried over
            int32_t vq = 0;
            PHICHK(walk_vtx_at(c, e, &vq));
            const int32_t kq = c->h_cstep[c->h_topo_rank[vq]];
            int32_t b = (int32_t)(std::upper_bound(c->h_blk_lo.begin(), c->h_blk_lo.end(), kq) - c->h_blk_lo.begin()) - 1;
            if (c->dp_cls) {
                int32_t out[2] = {-1, -1};
                phi_launch_carry_resolve(c->stream, c->d_blk_carry.as<int32_t>(), c->blk_ls, b, h, c->d_blk_bad.as<int32_t>() + 2);
                HIPCHK(hipMemcpyAsync(out, c->d_blk_bad.as<int32_t>() + 2, 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipStreamSynchronize(c->stream));
                bs = out[1];
            } else {
                while (bs < 0 && --b >= 0) bs = H.carry[(size_t)b * 64 + h];
            }
            if (bs < 0) return phi_fail(c, PHI_ERR_DEVICE, "DP backtrack: a carried run has no beginning (internal error)");
        }
        const int64_t es = c->h_walk_off[h] + bs;
        if (es < c->h_walk_off[h] || es > e) return phi_fail(c, PHI_ERR_DEVICE, "DP backtrack left the walk (internal error)");
        segs->push_back(Seg{h, es, e});
        if (es == c->h_walk_off[h]) break;                     // reached s_{first(h),h}
        int32_t v = 0;
        PHICHK(walk_vtx_at(c, es, &v));
        const int32_t step = events ? c->h_cstep[c->h_topo_rank[v]] : c->h_topo_rank[v];
        if (step < 0) return phi_fail(c, PHI_ERR_DEVICE, "DP backtrack: run begins on a vertex without events (internal error)");
        int32_t src, h2;
        if (bulk) { src = H.ent_u[step]; h2 = H.ent_h[step]; }
        else {
            HIPCHK(phi_copy_sync(c, &src, O.ent_src + step, 4, hipMemcpyDeviceToHost));
            HIPCHK(phi_copy_sync(c, &h2, O.ent_h + step, 4, hipMemcpyDeviceToHost));
        }
        if (events && src >= 0) src = c->h_kstep[src];          // compact step -> topological step
        const int32_t u = src >= 0 ? c->h_topo[src] : -1;
        if (u < 0 || h2 < 0) return phi_fail(c, PHI_ERR_DEVICE, "DP backtrack hit a vertex without an entry (internal error)");
        int64_t e2 = -1;
        PHICHK(entry_on_vertex(c, h2, src, u, &e2));
        if (e2 < 0) return phi_fail(c, PHI_ERR_DEVICE, "DP backtrack: walk %d is not on vertex %d (internal error)", h2, u);
        h = h2; e = e2;
    }
    std::reverse(segs->begin(), segs->end());
    return PHI_OK;
}

// what a caller that looks into a run (phi_dp_probe) learns besides its value and path
struct DpTrace {
    uint32_t retries = 0;                                      // bit (r - 1): DpRetry r was taken on the way
    int32_t end_walk = -1;                                     // dp_pick_end's walk
};
static_assert((1u << (DP_HALVE_CLASS_TARGET - 1)) == PHI_DP_RETRY_HALVE_CLASS_TARGET && (1u << (DP_NO_SMALL_BLOCKS - 1)) == PHI_DP_RETRY_NO_SMALL_BLOCKS &&
              (1u << (DP_GIVE_UP_BLOCKS - 1)) == PHI_DP_RETRY_GIVE_UP_BLOCKS && (1u << (DP_DENSE - 1)) == PHI_DP_RETRY_DENSE, "phi_dp_probe_info.retries (phi_amd.h)");

// One DP run with the given anchor weights (wgt == nullptr: the weights are on the device already): its value and the
// argmax path.  An attempt that names a DpRetry has left the error word clean; the next one starts over, weights included.
static int run_dp(phi_ctx *c, const std::vector<uint8_t> *wgt, DpHost &H, int64_t *value, std::vector<Seg> *segs, DpTrace *trace = nullptr)
{
    for (DpRetry want = DP_DONE;;) {
        if (want != DP_DONE) {
            c->dp_retries |= 1u << (want - 1);
            if (trace) trace->retries |= 1u << (want - 1);
        }
        switch (want) {
        case DP_DONE: break;
        case DP_HALVE_CLASS_TARGET: c->blk_cls_target /= 2; PHICHK(dp_prepare_blocks(c, c->n_dp)); break;
        case DP_NO_SMALL_BLOCKS: c->blk_no_small = true; PHICHK(dp_prepare_blocks(c, c->n_dp)); break;
        case DP_GIVE_UP_BLOCKS: c->dp_blocks = false; c->dp_cls = false; break;
        case DP_DENSE: c->dp_events = false; break;
        }
        want = DP_DONE;
        const bool events = c->dp_events;
        const DpOut O = dp_out(c);
        PhiStageTimer tr("dp run");
        if (c->n_dp && wgt) HIPCHK(hipMemcpyAsync(c->d_a_weight.p, wgt->data(), (size_t)c->n_dp, hipMemcpyHostToDevice, c->stream));
        if (events) {
            PhiDpEventArgs A{};
            PHICHK(dp_event_records(c, O, A, tr));
            if (c->dp_blocks && c->dp_cls) PHICHK(dp_blocks_on_class_lanes(c, A, tr, &want));
            else if (c->dp_blocks) PHICHK(dp_blocks_on_walk_lanes(c, A, H, tr, &want));
            else phi_launch_dp_events(c->stream, A);
            if (want != DP_DONE) continue;
        } else {
            PHICHK(dp_dense(c, O));
        }
        HIPCHK(hipGetLastError());
        PHICHK(dp_fetch_ends(c, O, events, H, tr, &want));
        if (want != DP_DONE) continue;
        int32_t bh = -1;
        PHICHK(dp_pick_end(c, H, &bh, value));
        if (trace) trace->end_walk = bh;
        PHICHK(dp_backtrack(c, O, events, H, bh, segs));
        tr.lap("backtrack");
        return PHI_OK;
    }
}

// phi_dp_probe: run_dp itself, once, on the state the last solve left, with the caller's weights -- what a relaxation of
// the search does between its weights and its path cover.  The ends are dp_fetch_ends' (a walk without a state: INT32_MIN),
// value and end walk dp_pick_end's, the segments run_dp's with positions inside their walk.  Test introspection.
int phi_dp_probe_impl(phi_ctx *c, const uint8_t *weights, int32_t *out_ends, int64_t *out_value, int32_t *out_end_walk,
                      int32_t *out_seg_walk, int64_t *out_seg_first, int64_t *out_seg_last, int64_t seg_cap, int64_t *n_seg, uint32_t *retries)
{
    std::vector<uint8_t> wgt((size_t)c->n_dp, 1);
    if (weights) wgt.assign(weights, weights + c->n_dp);
    DpHost H;
    DpTrace T;
    std::vector<Seg> segs;
    int64_t value = 0;
    PHICHK(run_dp(c, &wgt, H, &value, &segs, &T));
    for (int32_t h = 0; h < c->n_walks; h++) out_ends[h] = H.ends[(size_t)h] > -(1 << 28) ? H.ends[(size_t)h] : INT32_MIN;
    *out_value = value;
    *out_end_walk = T.end_walk;
    *retries = T.retries;
    *n_seg = (int64_t)segs.size();
    if ((int64_t)segs.size() > seg_cap) return PHI_OK;
    for (size_t i = 0; i < segs.size(); i++) {
        const int64_t w0 = c->h_walk_off[(size_t)segs[i].h];
        out_seg_walk[i] = segs[i].h; out_seg_first[i] = segs[i].es - w0; out_seg_last[i] = segs[i].ee - w0;
    }
    return PHI_OK;
}

// dp anchors traversed by a path: calls f(anchor index)
template <class F> static void for_covered(const phi_ctx *c, const std::vector<Seg> &segs, F f)
{
    const PhiAnchorSpan &A = c->h_dp;                         // sorted by e1
    for (const Seg &s : segs) {
        auto lo = std::lower_bound(A.begin(), A.end(), s.es, [](const PhiAnchorHost &a, int64_t e) { return (int64_t)a.e1 < e; });
        for (auto it = lo; it != A.end() && (int64_t)it->e1 <= s.ee; ++it)
            if ((int64_t)it->e0 >= s.es) f((int64_t)(it - A.begin()));
    }
}

// ------------------------------------------------------------------------------------------ solve
struct Node {
    std::vector<std::pair<uint32_t, int32_t>> assign;          // minimiser slot -> chosen cluster
    int64_t ub = INT64_MAX;                                    // bound proven for the parent (holds for the child)
};

// The exact search, across its nodes.  Branch and bound is finite and exact.  The reference's model.optimize()
// (ILP_index.cpp:1412-1418) has no limit; this search has a budget counted in DP runs (phi_set_solve_budget, default 4096;
// <= 0 = none), never in wall-clock time: the same input gives the same `optimal` flag on every run and every machine.
struct Search {
    std::vector<Node> stack;
    std::vector<int64_t> open_ub;                              // bounds of nodes given up on
    int64_t incumbent = INT64_MIN, global_ub = INT64_MIN, best_cov = 0;
    int n_runs = 0;
    bool exhausted = false;                                    // out of DP runs
};

// One phi_solve: what its stages hand on to each other.  A stage is a function over this object; phi_solve_impl is their
// schedule.  `dev`: the anchors stay on the device (a large model whose anchors all span an edge) until to_host ends that.
struct Solve {
    phi_ctx *const c;
    PhiStageTimer tm{"solve"};
    int64_t n_matched = 0, n_kept_rec = 0, n_kept = 0, n_dp = 0;
    int64_t filtered = 0, in_model = 0, spectrum = 0;
    bool anchors_prepped = false;                              // the expansion filled the DP's per-anchor arrays and the checks' counters on its way
    bool dev = false;
    PhiAnchorArrays arr;                                       // host mode: dp_walk, a_e1, a_span of the dp anchors
    std::vector<int32_t> sa_off, sa_idx;                       // minimiser -> dp anchors (device mode: on the device only, until the host needs them)
    std::vector<uint8_t> wgt;                                  // host weights (host mode)
    std::vector<int32_t> cov_all, cov_w;                       // per minimiser: dp anchors traversed (all / weighted)
    std::vector<uint32_t> touched;                             // minimisers with cov_all > 0
    std::set<uint32_t> S0;                                     // minimisers that repeat along a walk
    DpHost H;
    Search bb;
    std::vector<Seg> best_segs;
    explicit Solve(phi_ctx *c_) : c(c_) {}
};

// The pending allocations and launches are waited for, then the read spectrum: its size enters the result.
static int read_spectrum(Solve &S)
{
    phi_ctx *c = S.c;
    if (c->dp_alloc_future.valid()) PHICHK(c->dp_alloc_future.get());     // (a phi_set_graph that failed midway left it behind)
    PHICHK(phi_sync_check(c));
    S.tm = PhiStageTimer("solve");                             // (the solve's time starts behind what was pending)
    uint64_t sc[S_N];
    HIPCHK(phi_copy_sync(c, sc, c->d_scalars.p, sizeof sc, hipMemcpyDeviceToHost));
    uint64_t n_distinct = 0;
    PHICHK(phi_spectrum_count(c, &n_distinct));                   // (enters the logged novel read hashes into the set: the read set's one de-duplication)
    S.tm.lap("read spectrum (set from the log)");
    S.spectrum = c->spectrum_override >= 0 ? c->spectrum_override : (int64_t)n_distinct;
    return PHI_OK;
}

// ---- 1. anchors = walk minimisers whose hash is in the read spectrum (:495-526)
static int match_and_compact(Solve &S)
{
    phi_ctx *c = S.c;
    const int64_t n_rec = c->n_rec;
    PHICHK(phi_dev_ensure(c, c->d_flags, (size_t)std::max<int64_t>(n_rec, 1)));
    phi_launch_match_flags(c->stream, c->d_rec_slot.as<uint32_t>(), n_rec, c->d_u_uid.as<uint32_t>(),
                           c->d_hit.as<uint8_t>(), c->d_flags.as<uint8_t>());
    PHICHK(phi_compact(c, c->d_flags.as<uint8_t>(), n_rec, c->d_m_rec, &S.n_matched));
    S.tm.lap("match + compact");
    return PHI_OK;
}

// ---- 2. shared-anchor filter (:670-743): the kept class records, as a list in d_list and as flags in d_flags
static int filter_shared_anchors(Solve &S)
{
    phi_ctx *c = S.c;
    const int64_t n_rec = c->n_rec, n_matched = S.n_matched;
    PhiFilterArgs F{};
    // (over the CLASS records of contexts.hip: a record stands for cls_mult walk entries; its vertex list is read
    //  at the class representative's entries)
    F.rec_slot = c->d_rec_slot.as<uint32_t>(); F.rec_e0 = c->d_rec_e0.as<phi_ent_t>(); F.rec_e1 = c->d_rec_e1.as<phi_ent_t>();
    F.walk_vtx = c->d_walk_vtx.as<int32_t>();
    F.rec_cls = c->d_rec_cls.as<int32_t>(); F.cls_mult = c->d_cls_mult.as<int32_t>();
    F.m_rec = c->d_m_rec.as<int32_t>();
    const uint64_t g_cap = pow2_at_least(std::max<uint64_t>(1024, 2 * (uint64_t)n_matched));
    PHICHK(phi_dev_ensure(c, c->d_g_keys, g_cap * 8));
    PHICHK(phi_dev_ensure(c, c->d_g_rep, g_cap * 4));
    PHICHK(phi_dev_ensure(c, c->d_g_cnt, g_cap * 4));
    PHICHK(phi_dev_ensure(c, c->d_m_group, (size_t)std::max<int64_t>(n_matched, 1) * 4));
    const size_t n_slot_ids = (size_t)std::max<int64_t>(c->n_unique, 1);
    PHICHK(phi_dev_ensure(c, c->d_slot_maxcnt, n_slot_ids * 4));
    PHICHK(phi_dev_ensure(c, c->d_slot_multi, n_slot_ids));
    F.g_keys = c->d_g_keys.as<uint64_t>(); F.g_rep = c->d_g_rep.as<int32_t>(); F.g_cnt = c->d_g_cnt.as<uint32_t>();
    F.g_mask = g_cap - 1;
    F.m_group = c->d_m_group.as<int32_t>();
    F.u_uid = c->d_u_uid.as<uint32_t>();
    F.slot_maxcnt = c->d_slot_maxcnt.as<uint32_t>(); F.slot_multi = c->d_slot_multi.as<uint8_t>();
    F.limit = c->threshold * (float)(uint32_t)c->n_walks;      // threshold * num_walks, float (:698)
    F.counters = (unsigned long long *)scalar(c, S_FILTERED);
    F.err = (uint32_t *)scalar(c, S_ERR);
    for (int attempt = 0;; attempt++) {
        F.seed = 0x243F6A8885A308D3ull + 0x9E3779B97F4A7C15ull * (uint64_t)attempt;
        phi_launch_fill_u64(c->stream, F.g_keys, (int64_t)g_cap, PHI_EMPTY_KEY);
        phi_launch_fill_u32(c->stream, (uint32_t *)F.g_rep, (int64_t)g_cap, 0xFFFFFFFFu);
        HIPCHK(hipMemsetAsync(F.g_cnt, 0, g_cap * 4, c->stream));
        phi_launch_group_insert(c->stream, F, n_matched);
        phi_launch_group_count(c->stream, F, n_matched);
        HIPCHK(hipStreamSynchronize(c->stream));
        uint32_t err = 0;
        HIPCHK(phi_copy_sync(c, &err, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost));
        if (err & PHI_KERR_TABLE_FULL) return phi_fail(c, PHI_ERR_OVERFLOW, "anchor group table overflow");
        if (!(err & PHI_KERR_FP_COLLISION)) break;
        if (attempt == 7) return phi_fail(c, PHI_ERR_DEVICE, "anchor fingerprints collide under 8 seeds (internal error)");
        HIPCHK(phi_memset_sync(c, scalar(c, S_ERR), 0, 4));
    }
    HIPCHK(hipMemsetAsync(F.slot_maxcnt, 0, n_slot_ids * 4, c->stream));
    HIPCHK(hipMemsetAsync(F.slot_multi, 0, n_slot_ids, c->stream));
    HIPCHK(hipMemsetAsync(scalar(c, S_FILTERED), 0, 16, c->stream));
    phi_launch_group_max(c->stream, F, n_matched);
    phi_launch_slot_count(c->stream, F, c->n_unique);
    PHICHK(phi_dev_ensure(c, c->d_flags, (size_t)std::max<int64_t>(std::max(n_matched, n_rec), 1)));
    PHICHK(phi_dev_ensure(c, c->d_flags2, (size_t)std::max<int64_t>(n_matched, 1)));
    phi_launch_kept_flags(c->stream, F, n_matched, c->d_flags.as<uint8_t>(), c->d_flags2.as<uint8_t>());
    PHICHK(phi_compact(c, c->d_flags.as<uint8_t>(), n_matched, c->d_list, &S.n_kept_rec));
    S.tm.lap("filter kernels");
    return PHI_OK;
}

// The kept class records are expanded into the anchors of the model: every walk entry of a record's class
// carries one, (minimiser id, first entry, last entry), in entry order = position order along the walks.
// They go to the host as triples; their hashes stay behind (phi_kept_anchors derives them from the ids).
static int expand_kept_records(Solve &S)
{
    phi_ctx *c = S.c;
    const int64_t n_rec = c->n_rec, n_matched = S.n_matched, n_kept_rec = S.n_kept_rec;
    const int32_t nw = c->n_walks;
    const int64_t nr = std::max<int64_t>(n_rec, 1);
    PHICHK(phi_dev_ensure(c, c->d_flags2, (size_t)std::max<int64_t>(nr, n_matched)));
    HIPCHK(hipMemsetAsync(c->d_flags2.p, 0, (size_t)nr, c->stream));
    phi_launch_mark_list(c->stream, c->d_list.as<int32_t>(), c->d_m_rec.as<int32_t>(), n_kept_rec, c->d_flags2.as<uint8_t>());
    PHICHK(phi_dev_ensure(c, c->d_list3, (size_t)std::max<int64_t>(c->n_cls, (int64_t)nw) * 4));
    phi_launch_class_sel_count(c->stream, c->d_flags2.as<uint8_t>(), c->d_cls_rec_off.as<int32_t>(), c->n_cls, c->d_list3.as<int32_t>());
    PhiExpandArgs X{};
    X.ent_cls = c->d_ent_cls.as<int32_t>(); X.e_lo = 0; X.e_hi = c->n_entries;
    X.cls_rec_off = c->d_cls_rec_off.as<int32_t>(); X.cls_rep = c->d_cls_rep.as<phi_ent_t>();
    X.sel = c->d_flags2.as<uint8_t>(); X.sel_cnt = c->d_list3.as<int32_t>();
    X.rec_slot = c->d_rec_slot.as<uint32_t>(); X.u_uid = c->d_u_uid.as<uint32_t>();
    X.rec_e0 = c->d_rec_e0.as<phi_ent_t>(); X.rec_e1 = c->d_rec_e1.as<phi_ent_t>();
    const int64_t nb = phi_expand_num_blocks(c->n_entries);
    PHICHK(phi_dev_ensure(c, c->d_blk_cnt, (size_t)nb * 4));
    PHICHK(phi_dev_ensure(c, c->d_blk_off, (size_t)(nb + 1) * 8));
    X.block_cnt = c->d_blk_cnt.as<int32_t>(); X.block_off = c->d_blk_off.as<int64_t>();
    phi_launch_expand_count(c->stream, X);
    PHICHK(phi_scan(c, c->d_blk_cnt.as<int32_t>(), nb, c->d_blk_off.as<int64_t>()));
    int64_t n_kept = 0;
    HIPCHK(hipMemcpyAsync(&n_kept, c->d_blk_off.as<int64_t>() + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n_kept >= (int64_t)1 << 31) return phi_fail(c, PHI_ERR_UNSUPPORTED, "more than 2^31 anchors in the model");
    S.n_kept = n_kept;
    c->h_kept = PhiAnchorSpan{}; c->h_dp = PhiAnchorSpan{}; c->anchors_host = false;
    c->n_kept = n_kept; c->n_dp = 0;
    c->h_kept_hash.clear();
    PHICHK(phi_dev_ensure(c, c->d_anchors, (size_t)std::max<int64_t>(n_kept, 1) * 12));
    static_assert(sizeof(PhiAnchorHost) == 12, "PhiAnchorHost is the device triple");
    // (the DP's per-anchor arrays and the counters of the anchor checks: the packed expansion fills them on its way)
    PHICHK(phi_dev_ensure(c, c->d_a_e1, (size_t)std::max<int64_t>(n_kept, 1) * 4));
    PHICHK(phi_dev_ensure(c, c->d_g_span, (size_t)std::max<int64_t>(n_kept, 1)));
    PHICHK(phi_dev_ensure(c, c->d_ctr, (size_t)(nw + 8) * 8));
    HIPCHK(hipMemsetAsync(c->d_ctr.p, 0, (size_t)(nw + 8) * 8, c->stream));
    if (n_kept && getenv("PHI_EXPAND_GENERIC")) {               // (tests: the generic expansion, record by record)
        X.out_tri = c->d_anchors.as<uint32_t>();
        phi_launch_expand_write(c->stream, X, 1);
    } else if (n_kept) {
        // the selected records packed per class, then the anchors from those alone (contexts.hip)
        PHICHK(phi_dev_ensure(c, c->d_sel_off, (size_t)(c->n_cls + 1) * 4));
        PHICHK(phi_dev_ensure(c, c->d_sel_tri, (size_t)std::max<int64_t>(n_kept_rec, 1) * 12));
        PHICHK(phi_scan(c, c->d_list3.as<int32_t>(), c->n_cls, c->d_sel_off.as<int32_t>()));
        phi_launch_class_sel_tri(c->stream, c->d_flags2.as<uint8_t>(), c->d_cls_rec_off.as<int32_t>(), c->n_cls, c->d_sel_off.as<int32_t>(), c->d_cls_rep.as<phi_ent_t>(),
                                 c->d_rec_slot.as<uint32_t>(), c->d_u_uid.as<uint32_t>(), c->d_rec_e0.as<phi_ent_t>(), c->d_rec_e1.as<phi_ent_t>(), c->d_sel_tri.as<int32_t>());
        unsigned long long *d_ctr = c->d_ctr.as<unsigned long long>();
        phi_launch_expand_tri(c->stream, c->d_ent_cls.as<int32_t>(), 0, c->n_entries, c->d_sel_off.as<int32_t>(), c->d_sel_tri.as<int32_t>(),
                              c->d_blk_off.as<int64_t>(), c->d_anchors.as<uint32_t>(), c->d_a_e1.as<phi_ent_t>(), c->d_g_span.as<uint8_t>(),
                              c->d_walk_off.as<int64_t>(), nw, d_ctr + 8, d_ctr, n_kept);
        S.anchors_prepped = true;
    }
    return PHI_OK;
}

// The DP's per-anchor arrays (last entry, span), the anchors per walk and the checks on them, on the device.
// A large model whose anchors all span an edge (vertices shorter than k: every graph chopped to 30 bp) stays
// there: the host copy (6 GB at 5 * 10^8 anchors) is fetched only if the branch and bound proper needs it.
static int check_anchors_choose_mode(Solve &S)
{
    phi_ctx *c = S.c;
    const int32_t nw = c->n_walks;
    const int64_t n_kept = S.n_kept;
    unsigned long long *d_ctr = c->d_ctr.as<unsigned long long>();
    if (!S.anchors_prepped)
        phi_launch_anchor_prep(c->stream, c->d_anchors.as<uint32_t>(), n_kept, c->d_walk_off.as<int64_t>(), nw, c->d_a_e1.as<phi_ent_t>(), c->d_g_span.as<uint8_t>(), d_ctr + 8, d_ctr);
    std::vector<unsigned long long> hc((size_t)nw + 8);
    HIPCHK(hipMemcpyAsync(hc.data(), d_ctr, hc.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (hc[1] & 1) return phi_fail(c, PHI_ERR_DEVICE, "dp anchors not sorted by last entry (internal error)");
    if (hc[1] & 2)
        return phi_fail(c, c->k > PHI_RCAP ? PHI_ERR_UNSUPPORTED : PHI_ERR_DEVICE, "an anchor spans %d edges or more%s", PHI_RCAP,
                        c->k > PHI_RCAP ? ": with k > 32 the graph's vertices must be long enough for a k-mer to cover at most 32 of them" : " (internal error)");
    c->h_n_anchors.assign(nw, 0);
    for (int32_t h = 0; h < nw; h++) c->h_n_anchors[h] = (int64_t)hc[(size_t)h + 8];
    int64_t dev_min = (int64_t)1 << 16;                    // below this the host loops are as fast as the extra launches
    if (const char *e = getenv("PHI_SOLVE_DEVICE")) dev_min = atoi(e) ? 0 : INT64_MAX;     // tests: force either way
    S.dev = hc[0] == 0 && n_kept >= dev_min && n_kept > 0;
    uint64_t sc[S_N];
    HIPCHK(phi_copy_sync(c, sc, c->d_scalars.p, sizeof sc, hipMemcpyDeviceToHost));
    S.filtered = (int64_t)sc[S_FILTERED]; S.in_model = (int64_t)sc[S_INMODEL];
    return PHI_OK;
}

// Host mode: the kept anchors to the host, then the dp anchors, the anchors per walk and the DP's per-anchor arrays
// (phi_anchor_arrays).  Device mode: every kept anchor is a dp anchor, and nothing moves.
static int anchors_to_host(Solve &S)
{
    phi_ctx *c = S.c;
    const int64_t n_kept = S.n_kept;
    if (S.dev) {
        S.tm.lap("anchor arrays (device)");
        c->n_dp = n_kept;
    } else {
        PHICHK(phi_pin_ensure(c, (size_t)std::max<int64_t>(n_kept, 1) * sizeof(PhiAnchorHost)));
        c->h_kept = PhiAnchorSpan{static_cast<PhiAnchorHost *>(c->h_pin), n_kept};
        if (n_kept) HIPCHK(hipMemcpyAsync(c->h_kept.p, c->d_anchors.p, (size_t)n_kept * 12, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->anchors_host = true;
        S.tm.lap("anchors D2H");
        PhiHostError herr;
        if (phi_anchor_arrays(c->h_kept, c->h_walk_off.data(), c->n_walks, c->k, c->h_dp_own, S.arr, c->h_n_anchors, herr))
            return phi_fail(c, herr.code, "%s", herr.msg.c_str());
        c->h_dp = S.arr.dp;
        c->n_dp = (int64_t)c->h_dp.size();
    }
    S.n_dp = c->n_dp;
    if (S.tm.on) fprintf(stderr, "[phi timing] solve: class records %lld, matched %lld, kept %lld -> anchors kept %lld, dp %lld\n", (long long)c->n_rec, (long long)S.n_matched, (long long)S.n_kept_rec, (long long)n_kept, (long long)S.n_dp);
    S.tm.lap("filter (GPU) + anchors D2H");
    return PHI_OK;
}

// ---- 3. DP inputs, first the CSR of the dp anchors by last entry
static int anchor_entry_csr(Solve &S)
{
    phi_ctx *c = S.c;
    const int64_t n_dp = S.n_dp;
    PHICHK(phi_dev_ensure(c, c->d_a_weight, (size_t)std::max<int64_t>(n_dp, 1)));
    PHICHK(phi_dev_ensure(c, c->d_g_off, (size_t)(c->n_entries + 1) * 8));
    if (n_dp && !S.dev) {
        // (the dp list may be shorter than the kept list the device arrays were made from)
        HIPCHK(hipMemcpyAsync(c->d_a_e1.p, S.arr.a_e1.data(), (size_t)n_dp * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_g_span.p, S.arr.a_span.data(), (size_t)n_dp, hipMemcpyHostToDevice, c->stream));
    }
    phi_launch_entry_csr(c->stream, c->d_a_e1.as<phi_ent_t>(), n_dp, c->n_entries, c->d_g_off.as<int64_t>());
    return PHI_OK;
}

// DP scores are int32 with -2^28 as "no state", and a path scores at most one per anchor: from 2^27 dp anchors on, the most a
// path could score (the sum over vertices of the most anchors that end there on one walk, phi_score_bound) has to stay
// below 2^27.  Host mode counts on the host arrays, device mode on the CSR by last entry.
static int score_bound_host(Solve &S, int64_t *bound)
{
    phi_ctx *c = S.c;
    PHICHK(ensure_host_walks(c));
    *bound = phi_score_bound(S.arr.a_e1.data(), S.n_dp, c->h_walk_vtx.data(), c->n_vtx);
    return PHI_OK;
}
static int score_bound_dev(Solve &S, int64_t *bound)
{
    phi_ctx *c = S.c;
    PHICHK(phi_dev_ensure(c, c->d_vmax, (size_t)c->n_vtx * 4));
    HIPCHK(hipMemsetAsync(c->d_vmax.p, 0, (size_t)c->n_vtx * 4, c->stream));
    HIPCHK(hipMemsetAsync(c->d_ctr.p, 0, 8, c->stream));
    phi_launch_vertex_most(c->stream, c->d_g_off.as<int64_t>(), c->n_entries, c->d_walk_vtx.as<int32_t>(), c->d_vmax.as<int32_t>());
    phi_launch_sum_i32(c->stream, c->d_vmax.as<int32_t>(), c->n_vtx, c->d_ctr.as<unsigned long long>());
    unsigned long long sum = 0;
    HIPCHK(hipMemcpyAsync(&sum, c->d_ctr.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *bound = (int64_t)sum;
    return PHI_OK;
}
static int check_score_range(Solve &S)
{
    phi_ctx *c = S.c;
    if (S.n_dp < ((int64_t)1 << 27)) return PHI_OK;
    int64_t bound = 0;
    PHICHK(S.dev ? score_bound_dev(S, &bound) : score_bound_host(S, &bound));
    if (bound >= ((int64_t)1 << 27)) return phi_fail(c, PHI_ERR_UNSUPPORTED, "a path could score %lld >= 2^27 anchors", (long long)bound);
    return PHI_OK;
}

// the rest of the DP inputs: the walks' last entries, the DP's buffers, and the blocks of this solve
static int dp_inputs(Solve &S)
{
    phi_ctx *c = S.c;
    const int32_t nw = c->n_walks;
    HIPCHK(hipStreamSynchronize(c->stream));
    {
        std::vector<phi_ent_t> last(nw);
        for (int32_t h = 0; h < nw; h++) last[h] = (phi_ent_t)(c->h_walk_off[h + 1] - 1);
        PHICHK(phi_dev_ensure(c, c->d_walk_last, (size_t)nw * 4));
        PHICHK(phi_dev_ensure(c, c->d_list3, (size_t)nw * 4));
        HIPCHK(phi_copy_sync(c, c->d_walk_last.p, last.data(), (size_t)nw * 4, hipMemcpyHostToDevice));
    }
    PHICHK(phi_dev_ensure(c, c->d_dmax, (size_t)c->n_entries * 4));
    PHICHK(phi_dev_ensure(c, c->d_bstart, (size_t)c->n_entries * 4));
    if (c->dp_events) {
        const int64_t ne1 = c->n_entries + 1;
        PHICHK(phi_dev_ensure(c, c->d_off_end, (size_t)(ne1 + 2) * 4));      // (+2: also the scratch of dp_prepare_blocks)
        PHICHK(phi_dev_ensure(c, c->d_off_start, (size_t)(ne1 + 2) * 4));
        PHICHK(phi_dev_ensure(c, c->d_ev, (size_t)std::max<int64_t>(c->n_ev, 1) * 48));
    }
    PHICHK(phi_dev_ensure(c, c->d_top, (size_t)c->n_vtx * 5 * 4));
    PHICHK(phi_dev_ensure(c, c->d_ent, (size_t)c->n_vtx * 2 * 4));
    c->blk_no_small = false;
    c->blk_cls_target = 16;
    c->dp_retries = 0;
    PHICHK(dp_prepare_blocks(c, S.n_dp));
    S.tm.lap("DP inputs");
    return PHI_OK;
}

// ---- 4. exact solve
// dp anchors of every minimiser (CSR over the dense minimiser ids), ascending anchor index, where the dp list is the kept
// list, whose triples are on the device: count / scan / scatter / sort there (1-2 ms for 10^7 anchors; the host loop,
// phi_anchor_csr, takes 4 ms per million).  fetch: the map also goes to the host (sa_off, sa_idx).
static int anchor_csr_dev(Solve &S, bool fetch)
{
    phi_ctx *c = S.c;
    const int64_t n_ids = c->n_unique, n_dp = S.n_dp;
    const uint32_t *tri = c->d_anchors.as<uint32_t>();
    PHICHK(phi_dev_ensure(c, c->d_sa_cnt, (size_t)(n_ids + 1) * 4));
    PHICHK(phi_dev_ensure(c, c->d_sa_cur, (size_t)(n_ids + 1) * 4));
    PHICHK(phi_dev_ensure(c, c->d_sa_off, (size_t)(n_ids + 2) * 4));
    PHICHK(phi_dev_ensure(c, c->d_sa_idx, (size_t)n_dp * 4));
    HIPCHK(hipMemsetAsync(c->d_sa_cnt.p, 0, (size_t)(n_ids + 1) * 4, c->stream));
    HIPCHK(hipMemsetAsync(c->d_sa_cur.p, 0, (size_t)(n_ids + 1) * 4, c->stream));
    phi_launch_csr_count(c->stream, tri, n_dp, n_ids, c->d_sa_cnt.as<int32_t>(), (uint32_t *)scalar(c, S_ERR));
    PHICHK(phi_scan(c, c->d_sa_cnt.as<int32_t>(), n_ids, c->d_sa_off.as<int32_t>()));
    phi_launch_csr_scatter(c->stream, tri, n_dp, n_ids, c->d_sa_off.as<int32_t>(), c->d_sa_cur.as<int32_t>(), c->d_sa_idx.as<int32_t>());
    phi_launch_csr_sort(c->stream, c->d_sa_off.as<int32_t>(), n_ids, c->d_sa_idx.as<int32_t>());
    int32_t total = 0;
    if (fetch) {
        S.sa_off.resize((size_t)n_ids + 1); S.sa_idx.resize((size_t)std::max<int64_t>(n_dp, 1));
        HIPCHK(hipMemcpyAsync(S.sa_off.data(), c->d_sa_off.p, (size_t)(n_ids + 1) * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(S.sa_idx.data(), c->d_sa_idx.p, (size_t)n_dp * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipMemcpyAsync(&total, c->d_sa_off.as<int32_t>() + n_ids, 4, hipMemcpyDeviceToHost, c->stream));
    uint32_t kerr = 0;
    HIPCHK(hipMemcpyAsync(&kerr, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((kerr & PHI_KERR_CSR_ID) || total != (int32_t)n_dp)
        return phi_fail(c, PHI_ERR_DEVICE, "minimiser id out of range (internal error)");
    return PHI_OK;
}

// (device mode does without the map -- repeats walk by walk, weights from a flag per minimiser -- until the branch and
//  bound proper asks for the host copies: at chromosome scale building it is 0.16 of the solve's 0.95 s)
static int anchors_of_minimisers(Solve &S)
{
    phi_ctx *c = S.c;
    const int64_t n_ids = c->n_unique, n_dp = S.n_dp;
    if (!S.dev) {
        const bool dp_is_kept = c->h_dp.p == c->h_kept.p && c->h_dp.size() == c->h_kept.size();
        if (dp_is_kept && n_dp > 0) PHICHK(anchor_csr_dev(S, true));
        else if (!phi_anchor_csr(c->h_dp, n_ids, S.sa_off, S.sa_idx)) return phi_fail(c, PHI_ERR_DEVICE, "minimiser id out of range (internal error)");
    }
    S.tm.lap("minimiser -> anchors map");
    return PHI_OK;
}

// Minimisers with two anchors on ONE walk (repeats along a haplotype) are what an additive DP counts
// twice on sight: start the relaxation with them in S instead of discovering them by a first run.
static int repeat_set_dev(Solve &S)
{
    phi_ctx *c = S.c;
    const int64_t n_ids = c->n_unique;
    PHICHK(phi_dev_ensure(c, c->d_flags, (size_t)std::max<int64_t>(n_ids, 1)));
    PHICHK(phi_dev_ensure(c, c->d_last_walk, (size_t)std::max<int64_t>(n_ids, 1) * 4));
    HIPCHK(hipMemsetAsync(c->d_flags.p, 0, (size_t)std::max<int64_t>(n_ids, 1), c->stream));
    HIPCHK(hipMemsetAsync(c->d_last_walk.p, 0xFF, (size_t)std::max<int64_t>(n_ids, 1) * 4, c->stream));
    int64_t lo = 0;                                            // the kept anchors come in walk order: walk h has h_n_anchors[h] of them
    for (int32_t h = 0; h < c->n_walks; h++) {
        phi_launch_repeat_walk(c->stream, c->d_anchors.as<uint32_t>(), lo, lo + c->h_n_anchors[h], h, c->d_last_walk.as<int32_t>(), c->d_flags.as<uint8_t>());
        lo += c->h_n_anchors[h];
    }
    if (lo != S.n_dp) return phi_fail(c, PHI_ERR_DEVICE, "anchors per walk do not add up (internal error)");
    int64_t n_rep = 0;
    PHICHK(phi_compact(c, c->d_flags.as<uint8_t>(), n_ids, c->d_list, &n_rep));
    std::vector<uint32_t> rep((size_t)n_rep);
    if (n_rep) HIPCHK(phi_copy_sync(c, rep.data(), c->d_list.p, (size_t)n_rep * 4, hipMemcpyDeviceToHost));
    S.S0.insert(rep.begin(), rep.end());                       // (ascending: linear-time insertion)
    return PHI_OK;
}
static int repeat_set(Solve &S)
{
    if (!getenv("PHI_NO_S0")) {
        if (S.dev) PHICHK(repeat_set_dev(S));
        else phi_repeat_set(S.sa_off, S.sa_idx, S.arr.dp_walk, S.c->n_unique, S.S0);
        if (S.tm.on) fprintf(stderr, "[phi timing] solve: %zu minimisers repeat along a walk\n", S.S0.size());
    }
    S.tm.lap("repeat set");
    return PHI_OK;
}

struct Span {
    const int32_t *p; int32_t n;
    const int32_t *begin() const { return p; }
    const int32_t *end() const { return p + n; }
    int32_t operator[](int32_t i) const { return p[i]; }
};
static Span anchors_of(const Solve &S, uint32_t s) { return Span{S.sa_idx.data() + S.sa_off[s], S.sa_off[s + 1] - S.sa_off[s]}; }

// the clusters of a minimiser's anchors (phi_clusters), from the ranks of their end vertices and their walks
static std::vector<std::vector<int32_t>> clusters_of(const Solve &S, uint32_t slot)
{
    const phi_ctx *c = S.c;
    std::vector<PhiAnchorIv> iv;
    for (int32_t a : anchors_of(S, slot)) {
        const PhiAnchorHost &A = c->h_dp[a];
        iv.push_back(PhiAnchorIv{c->h_topo_rank[c->h_walk_vtx[A.e0]], c->h_topo_rank[c->h_walk_vtx[A.e1]], phi_entry_walk(c, A.e0), a});
    }
    return phi_clusters(std::move(iv));
}

// device mode ends where the branch and bound proper begins: the host copies arrive, the search goes on unchanged
static int to_host(Solve &S)
{
    phi_ctx *c = S.c;
    const int64_t n_ids = c->n_unique, n_dp = S.n_dp;
    PHICHK(ensure_host_walks(c));                               // (clusters_of indexes the walk entries freely)
    if (!S.dev) return PHI_OK;
    PhiStageTimer th("solve");
    PHICHK(phi_host_anchors(c));
    if (n_dp) PHICHK(anchor_csr_dev(S, true));                  // (the minimiser -> anchors map, made now that it is needed)
    else { S.sa_off.assign((size_t)n_ids + 1, 0); S.sa_idx.assign(1, 0); }
    S.wgt.assign((size_t)n_dp, 1);
    S.cov_all.assign((size_t)n_ids, 0); S.cov_w.assign((size_t)n_ids, 0);
    S.touched.clear();
    S.dev = false;
    th.lap("  anchors and their map to the host (branch and bound)");
    return PHI_OK;
}

// what a node of the search keeps across its relaxations
struct NodeState {
    std::map<uint32_t, int32_t> assign;                        // the node's assignments
    std::map<uint32_t, std::vector<std::vector<int32_t>>> assign_clusters;
    std::set<uint32_t> S;                                      // minimisers bounded by the constant 1
    std::set<std::set<uint32_t>> seenS;
    std::set<uint32_t> lastD, lastZ;                           // what a branching candidate is chosen from
    bool have_sets = false;
    int64_t ub = INT64_MAX;
};
// one relaxation of a node: its DP run, and what the run's path says about S
struct Relaxation {
    std::vector<uint32_t> Sv;                                  // S as a list (device mode)
    int64_t val = 0;                                           // the DP's value
    std::vector<Seg> segs;                                     // its path
    int64_t add_w = 0, n_touched = 0;                          // the path's anchors of weight 1; the minimisers it covers
    std::set<uint32_t> D, Z;                                   // minimisers counted twice by the path; minimisers of S it does not cover
};

// the weights of a relaxation: 0 on the anchors of S and on the clusters the node has ruled out, 1 elsewhere
static int weights_dev(Solve &S, const NodeState &N, Relaxation &R)
{
    phi_ctx *c = S.c;
    const int64_t n_ids = c->n_unique;
    // (no assignments in device mode: to_host() runs before the first node that has one)
    R.Sv.assign(N.S.begin(), N.S.end());
    PHICHK(phi_dev_ensure(c, c->d_slots, std::max<size_t>(R.Sv.size(), 1) * 4));
    PHICHK(phi_dev_ensure(c, c->d_slots2, std::max<size_t>(R.Sv.size(), 1) * 4));
    PHICHK(phi_dev_ensure(c, c->d_in_s, (size_t)std::max<int64_t>(n_ids, 1)));
    if (!R.Sv.empty()) HIPCHK(hipMemcpyAsync(c->d_slots.p, R.Sv.data(), R.Sv.size() * 4, hipMemcpyHostToDevice, c->stream));
    // a flag per minimiser of S, then one pass over the anchors (no minimiser -> anchors map in device mode)
    HIPCHK(hipMemsetAsync(c->d_in_s.p, 0, (size_t)std::max<int64_t>(n_ids, 1), c->stream));
    phi_launch_mark_list(c->stream, c->d_slots.as<int32_t>(), nullptr, (int64_t)R.Sv.size(), c->d_in_s.as<uint8_t>());
    phi_launch_weights(c->stream, c->d_anchors.as<uint32_t>(), S.n_dp, c->d_in_s.as<uint8_t>(), c->d_a_weight.as<uint8_t>());
    HIPCHK(hipStreamSynchronize(c->stream));       // Sv is read by the copy
    return PHI_OK;
}
static int weights_host(Solve &S, const NodeState &N, Relaxation &)
{
    std::fill(S.wgt.begin(), S.wgt.end(), 1);
    for (uint32_t s : N.S) for (int32_t a : anchors_of(S, s)) S.wgt[a] = 0;
    for (auto &kv : N.assign) {
        if (N.S.count(kv.first)) continue;
        const auto &cl = N.assign_clusters.at(kv.first);
        for (size_t ci = 0; ci < cl.size(); ci++)
            if ((int32_t)ci != kv.second) for (int32_t a : cl[ci]) S.wgt[a] = 0;
    }
    return PHI_OK;
}

// The path's additive value under the weights and the minimisers it covers.  Device mode: cover counts per minimiser on
// the device; back come the two sums and the two short lists D and Z.
static int path_cover_dev(Solve &S, Relaxation &R)
{
    phi_ctx *c = S.c;
    const std::vector<Seg> &segs = R.segs;
    const uint32_t *d_tri = c->d_anchors.as<uint32_t>();
    std::vector<phi_ent_t> sg(segs.size() * 2);
    for (size_t i = 0; i < segs.size(); i++) { sg[2 * i] = (phi_ent_t)segs[i].es; sg[2 * i + 1] = (phi_ent_t)segs[i].ee; }
    const int64_t twice_cap = (int64_t)1 << 22;
    PHICHK(phi_dev_ensure(c, c->d_segs, std::max<size_t>(sg.size(), 2) * 4));
    PHICHK(phi_dev_ensure(c, c->d_list, (size_t)twice_cap * 4));
    unsigned long long *d_ctr = c->d_ctr.as<unsigned long long>();
    HIPCHK(hipMemcpyAsync(c->d_segs.p, sg.data(), sg.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_ctr, 0, 32, c->stream));
    phi_launch_path_cover(c->stream, false, c->d_segs.as<phi_ent_t>(), (int32_t)segs.size(), c->d_g_off.as<int64_t>(), d_tri, c->d_a_weight.as<uint8_t>(),
                          c->d_cov_all.as<int32_t>(), c->d_cov_w.as<int32_t>(), d_ctr, c->d_list.as<uint32_t>(), twice_cap);
    phi_launch_uncovered_slots(c->stream, c->d_slots.as<uint32_t>(), (int64_t)R.Sv.size(), c->d_cov_all.as<int32_t>(), d_ctr, c->d_slots2.as<uint32_t>());
    phi_launch_path_cover(c->stream, true, c->d_segs.as<phi_ent_t>(), (int32_t)segs.size(), c->d_g_off.as<int64_t>(), d_tri, c->d_a_weight.as<uint8_t>(),
                          c->d_cov_all.as<int32_t>(), c->d_cov_w.as<int32_t>(), d_ctr, c->d_list.as<uint32_t>(), twice_cap);
    unsigned long long hc[4];
    HIPCHK(hipMemcpyAsync(hc, d_ctr, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((int64_t)hc[2] > twice_cap) return phi_fail(c, PHI_ERR_OVERFLOW, "more than 2^22 minimisers counted twice by one path");
    R.add_w = (int64_t)hc[0]; R.n_touched = (int64_t)hc[1];
    std::vector<uint32_t> dl((size_t)hc[2]), zl((size_t)hc[3]);
    if (hc[2]) HIPCHK(phi_copy_sync(c, dl.data(), c->d_list.p, dl.size() * 4, hipMemcpyDeviceToHost));
    if (hc[3]) HIPCHK(phi_copy_sync(c, zl.data(), c->d_slots2.p, zl.size() * 4, hipMemcpyDeviceToHost));
    R.D.insert(dl.begin(), dl.end());
    R.Z.insert(zl.begin(), zl.end());
    return PHI_OK;
}
// Host mode: the cover counts per minimiser stay in cov_all / cov_w for tighten_sets_host.
static int path_cover_host(Solve &S, Relaxation &R)
{
    const phi_ctx *c = S.c;
    for (uint32_t s : S.touched) { S.cov_all[s] = 0; S.cov_w[s] = 0; }
    S.touched.clear();
    for_covered(c, R.segs, [&](int64_t a) {
        const uint32_t s = c->h_dp[a].slot;
        if (!S.cov_all[s]++) S.touched.push_back(s);
        if (S.wgt[a]) { S.cov_w[s]++; R.add_w++; }
    });
    R.n_touched = (int64_t)S.touched.size();
    return PHI_OK;
}

// The run's path against its own value, the incumbent and the bounds; the progress line.  *closed: the node's bound does not
// exceed the incumbent.
static int note_bounds(Solve &S, NodeState &N, Relaxation &R, int64_t *ub_, int64_t *true_val_, bool *closed)
{
    phi_ctx *c = S.c;
    Search &B = S.bb;
    const int64_t cost = 2 * (int64_t)(c->recombination / 2);
    const int64_t n_sw = (int64_t)R.segs.size() - 1;
    R.add_w -= cost * n_sw;
    if (R.add_w != R.val) return phi_fail(c, PHI_ERR_DEVICE, "DP value %lld != value %lld of its own path (internal error)", (long long)R.val, (long long)R.add_w);
    const int64_t true_val = R.n_touched - cost * n_sw;
    if (true_val > B.incumbent) { B.incumbent = true_val; S.best_segs = R.segs; B.best_cov = R.n_touched; }
    const int64_t ub = R.val + (int64_t)N.S.size();
    N.ub = std::min(N.ub, ub);
    if (B.n_runs == 1) B.global_ub = ub;
    // a search that goes on says so (the reference's model.optimize() prints Gurobi's log; the command line runs without a
    // budget unless --dp-budget gives one): every 64 DP runs, and the 16th (PHI_PROGRESS=0: never; =n: every n runs)
    static const int every = getenv("PHI_PROGRESS") ? atoi(getenv("PHI_PROGRESS")) : 64;
    if (every > 0 && (B.n_runs % every == 0 || (every == 64 && B.n_runs == 16)))
        fprintf(stderr, "[M::solve] exact search: %d DP runs, best path %lld, proven bound %lld, %zu open node(s)%s\n", B.n_runs,
                (long long)B.incumbent, (long long)B.global_ub, B.stack.size() + 1, c->solve_budget > 0 ? "" : " (no budget: --dp-budget N limits it)");
    *ub_ = ub; *true_val_ = true_val;
    *closed = N.ub <= B.incumbent;
    return PHI_OK;
}

// Host mode: D = the minimisers the path counts twice under the weights, Z = the minimisers of S none of whose anchors the
// node still allows is traversed (device mode: both came back with the cover counts)
static void tighten_sets_host(Solve &S, const NodeState &N, Relaxation &R)
{
    const phi_ctx *c = S.c;
    for (uint32_t s : S.touched) if (S.cov_w[s] >= 2) R.D.insert(s);
    for (uint32_t s : N.S) {
        // is any anchor this node still allows for s traversed?
        bool covered = false;
        if (S.cov_all[s]) {
            auto it = N.assign.find(s);
            if (it == N.assign.end()) covered = true;
            else {
                const auto &cl = N.assign_clusters.at(s)[it->second];
                for_covered(c, R.segs, [&](int64_t a) {
                    if (c->h_dp[a].slot == s && std::find(cl.begin(), cl.end(), (int32_t)a) != cl.end()) covered = true;
                });
            }
        }
        if (!covered) R.Z.insert(s);
    }
}

// One node: up to 8 relaxations, each a DP run, until its bound closes, S stops moving or the budget is out; then the
// node's children, one per cluster of the minimiser branched on.
static int search_node(Solve &S, const Node &node)
{
    phi_ctx *c = S.c;
    Search &B = S.bb;
    const int64_t max_runs = c->solve_budget;
    NodeState N;
    N.assign.insert(node.assign.begin(), node.assign.end());
    N.ub = node.ub;
    if (!N.assign.empty()) PHICHK(to_host(S));
    for (auto &kv : N.assign) N.assign_clusters[kv.first] = clusters_of(S, kv.first);
    if (node.assign.empty()) N.S = S.S0;
    for (int iter = 0; iter < 8; iter++) {
        if (max_runs > 0 && B.n_runs >= max_runs) { B.exhausted = true; break; }
        Relaxation R;
        PHICHK((S.dev ? weights_dev : weights_host)(S, N, R));
        S.tm.lap("  weights of the relaxation");
        PHICHK(run_dp(c, S.dev ? nullptr : &S.wgt, S.H, &R.val, &R.segs));
        B.n_runs++;
        S.tm.lap("  DP run + backtrack");
        PHICHK((S.dev ? path_cover_dev : path_cover_host)(S, R));
        int64_t ub = 0, true_val = 0;
        bool closed = false;
        PHICHK(note_bounds(S, N, R, &ub, &true_val, &closed));
        if (closed) return PHI_OK;
        if (!S.dev) tighten_sets_host(S, N, R);
        if (S.tm.on) fprintf(stderr, "[phi timing] solve:   run %d: DP value %lld + |S| %zu = bound %lld; path: exact %lld, %lld switches; doubly counted %zu, unused constants %zu\n",
                             B.n_runs, (long long)R.val, N.S.size(), (long long)ub, (long long)true_val, (long long)R.segs.size() - 1, R.D.size(), R.Z.size());
        S.tm.lap("  path value, tighten sets");
        if (R.D.empty() && R.Z.empty()) return PHI_OK;          // bound attained by this path
        N.lastD = R.D; N.lastZ = R.Z; N.have_sets = true;
        if (!phi_tighten(N.S, R.D, R.Z, N.seenS)) break;
    }
    uint32_t branch_slot = 0;
    bool have_branch = false;
    if (N.have_sets && !B.exhausted) {
        PHICHK(to_host(S));                                    // (the minimiser -> anchors map)
        have_branch = phi_choose_branch(N.lastD, N.lastZ, N.assign, S.sa_off, S.sa_idx, &branch_slot);
    }
    if (B.exhausted || !have_branch) { B.open_ub.push_back(std::min(N.ub, B.global_ub)); return PHI_OK; }
    const auto cl = clusters_of(S, branch_slot);
    for (int32_t ci = (int32_t)cl.size() - 1; ci >= 0; ci--) {
        Node ch = node;
        ch.ub = N.ub;
        ch.assign.emplace_back(branch_slot, ci);
        B.stack.push_back(ch);
    }
    return PHI_OK;
}

// the search: depth first from the root, until no node is open or the budget is out; upper_bound = the incumbent or the
// highest bound of a node left open
static int search(Solve &S, int64_t *upper_bound)
{
    phi_ctx *c = S.c;
    Search &B = S.bb;
    const int64_t n_ids = c->n_unique;
    if (S.dev) {
        PHICHK(phi_dev_ensure(c, c->d_cov_all, (size_t)std::max<int64_t>(n_ids, 1) * 4));
        PHICHK(phi_dev_ensure(c, c->d_cov_w, (size_t)std::max<int64_t>(n_ids, 1) * 4));
        HIPCHK(hipMemsetAsync(c->d_cov_all.p, 0, (size_t)std::max<int64_t>(n_ids, 1) * 4, c->stream));
        HIPCHK(hipMemsetAsync(c->d_cov_w.p, 0, (size_t)std::max<int64_t>(n_ids, 1) * 4, c->stream));
    } else {
        S.wgt.assign((size_t)S.n_dp, 1);
        S.cov_all.assign((size_t)n_ids, 0); S.cov_w.assign((size_t)n_ids, 0);
    }
    B.stack.push_back(Node{});
    while (!B.stack.empty() && !B.exhausted) {
        const Node node = B.stack.back();
        B.stack.pop_back();
        PHICHK(search_node(S, node));
    }
    for (const Node &n : B.stack) B.open_ub.push_back(std::min(n.ub, B.global_ub));
    *upper_bound = B.incumbent;
    for (int64_t u : B.open_ub) *upper_bound = std::max(*upper_bound, u);
    S.tm.lap("DP runs + certificate");
    return PHI_OK;
}

// ---- 5. decode (:1431-1525)
static int decode(Solve &S, int64_t upper_bound)
{
    phi_ctx *c = S.c;
    const std::vector<Seg> &best_segs = S.best_segs;
    int64_t n_path_vtx = 0;
    for (const Seg &s : best_segs) n_path_vtx += s.ee - s.es + 1;
    c->h_path_vtx.resize((size_t)n_path_vtx);
    c->h_path_hap.resize((size_t)n_path_vtx);
    int64_t hap_len = 0;
    {
        int64_t o = 0;
        for (const Seg &s : best_segs) {
            PHICHK(walk_vtx_range(c, s.es, s.ee - s.es + 1, c->h_path_vtx.data() + o));
            std::fill(c->h_path_hap.begin() + o, c->h_path_hap.begin() + o + (s.ee - s.es + 1), s.h);
            for (int64_t i = 0; i <= s.ee - s.es; i++) { const int32_t v = c->h_path_vtx[(size_t)(o + i)]; hap_len += c->h_seq_off[v + 1] - c->h_seq_off[v]; }
            o += s.ee - s.es + 1;
        }
    }
    // adjacent label changes (:1517-1519): the labels change exactly between the path's stretches
    int32_t recomb = 0;
    for (size_t i = 1; i < best_segs.size(); i++) recomb += best_segs[i].h != best_segs[i - 1].h;

    phi_result &R = c->result;
    R.objective = S.bb.incumbent;
    R.upper_bound = upper_bound;
    R.optimal = upper_bound == S.bb.incumbent;
    R.n_dp_runs = S.bb.n_runs;
    R.n_covered = S.bb.best_cov;                               // minimisers covered by the best path (counted when it was found)
    R.n_path = (int64_t)c->h_path_vtx.size();
    R.path_vtx = c->h_path_vtx.data();
    R.path_hap = c->h_path_hap.data();
    R.recombination_count = recomb;
    R.n_switches = (int32_t)best_segs.size() - 1;
    R.hap_len = hap_len;
    R.n_walks = c->n_walks;
    R.n_minimizers = c->h_n_minimizers.data();
    R.n_anchors = c->h_n_anchors.data();
    R.spectrum_size = S.spectrum;
    R.filtered = S.filtered;
    R.retained = S.spectrum - S.filtered;
    R.n_in_model = S.in_model;
    S.tm.lap("decode");
    c->path_segs.clear();                                      // (phi_calls_path expands them on the device)
    for (const Seg &s : best_segs) c->path_segs.push_back({s.h, s.es, s.ee});
    c->calls.have = false;
    c->solved = true;
    return PHI_OK;
}

// the body of phi_solve: the schedule of the stages above
int phi_solve_impl(phi_ctx *c)
{
    c->solved = false;
    Solve S(c);
    PHICHK(read_spectrum(S));
    PHICHK(match_and_compact(S));
    PHICHK(filter_shared_anchors(S));
    PHICHK(expand_kept_records(S));
    PHICHK(check_anchors_choose_mode(S));
    PHICHK(anchors_to_host(S));
    PHICHK(anchor_entry_csr(S));
    PHICHK(check_score_range(S));
    PHICHK(dp_inputs(S));
    PHICHK(anchors_of_minimisers(S));
    PHICHK(repeat_set(S));
    int64_t upper_bound = 0;
    PHICHK(search(S, &upper_bound));
    return decode(S, upper_bound);
}
