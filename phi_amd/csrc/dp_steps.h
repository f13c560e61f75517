// dp_steps.h -- what phi_set_graph computes on the host threads from plain arrays: the validation of the topology and the
// DP step stream that dp.hip and dp_events.hip consume (record layout: PhiDpArgs / PhiDpEventArgs of phi_kernels.h).
// No HIP include and nothing of the context: set_graph.hip calls it between its uploads, and host/dp_steps_selftest.cpp
// runs it stand-alone under the sanitizers.  Every result is independent of thread timing.  A function that fails has set
// `err` (code and text of the phi_fail its caller makes of it) and returns err.code.
#pragma once
#include <limits.h>
#include <memory>
#include "../../include/phi_amd.h"
#include "phi_dp_flags.h"
#include "phi_host_par.h"

// topo[r] = the vertex of rank r, if topo_rank is a permutation of [0, n_vtx)
static inline int phi_topo_from_ranks(int32_t n_vtx, const int32_t *topo_rank, std::vector<int32_t> &topo, PhiHostError &err)
{
    topo.assign((size_t)n_vtx, -1);
    phi_parallel_chunks(n_vtx, 1 << 16, [&](int64_t lo, int64_t hi, int) {
        for (int64_t v = lo; v < hi && !err.failed(); v++) {
            const int32_t r = topo_rank[v];
            int32_t none = -1;
            if (r < 0 || r >= n_vtx || !__atomic_compare_exchange_n(&topo[(size_t)r], &none, (int32_t)v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
                err.set(PHI_ERR_INVALID, "topo_rank is not a permutation (vertex %d): is the graph cyclic?", (int)v);
                return;
            }
        }
    });
    return err.failed() ? err.code : PHI_OK;
}

// Every edge target in range.  With indeg (n_vtx zeros): every edge must also go forward in topo_rank (acyclic GFA,
// README.md:70-75), and indeg[v] becomes the in-edges of v.  Without: the range alone, which is all phi_set_graph_chopped
// indexes with before the chopped graph gets the whole check.
static inline int phi_check_edges(int32_t n_vtx, const int64_t *adj_off, const int32_t *adj, const int32_t *topo_rank, int64_t *indeg,
                                  PhiHostError &err)
{
    phi_parallel_chunks(n_vtx, 1 << 16, [&](int64_t lo, int64_t hi, int) {
        for (int64_t u = lo; u < hi && !err.failed(); u++)
            for (int64_t x = adj_off[u]; x < adj_off[u + 1]; x++) {
                const int32_t v = adj[x];
                if (v < 0 || v >= n_vtx) { err.set(PHI_ERR_INVALID, "edge target %d out of range", v); return; }
                if (!indeg) continue;
                if (topo_rank[u] >= topo_rank[v]) { err.set(PHI_ERR_INVALID, "edge %d->%d goes backwards in topo_rank: graph must be acyclic", (int)u, v); return; }
                __atomic_fetch_add(&indeg[(size_t)v], 1, __ATOMIC_RELAXED);
            }
    });
    return err.failed() ? err.code : PHI_OK;
}

// A validated graph as the step stream sees it.  topo: the inverse of topo_rank (phi_topo_from_ranks); cnt_edge: walks per
// edge (phi_launch_walk_edges); walk_ends: [2 * n_walks] first and last vertex of every walk.
struct PhiDpGraph {
    int32_t n_vtx, n_walks;
    const int64_t *adj_off;
    const int32_t *adj, *topo_rank, *topo, *cnt_edge, *walk_ends;
};

struct PhiDpSteps {
    // the every-vertex stream of dp.hip (phi_dp_steps_dense)
    std::unique_ptr<int32_t[]> st_rec;               // [n_vtx][8]; not value-initialised: first touched by whoever writes it
    std::vector<int32_t> in_packed;
    // the compact stream of dp_events.hip (phi_dp_steps_compact, then phi_dp_steps_cuts)
    std::vector<int32_t> k_rec, k_in, cvtx;          // [n_k][8], the in-edges beyond the third of a step, vertex -> compact step
    std::vector<int32_t> cstep, kstep;               // topological step -> compact step (-1) and back
    std::vector<int32_t> cut_ok;                     // [n_k + 1]: 1 = structurally a cut may sit before step k
    int32_t n_k = 0;
    int64_t n_pairs = 0;
};

// ---- DP step stream (dp.hip): per step the live in-edges as (steps back, out-edge index).  All host threads: the records
//      are 32 bytes per vertex (268 MB at chromosome scale, first touched by whoever writes them), the in-edges of a vertex
//      are gathered with an atomic cursor and then sorted, so that the stream does not depend on who came first.
static inline int phi_dp_steps_dense(const PhiDpGraph &g, PhiDpSteps &out, PhiHostError &err)
{
    const int32_t n_vtx = g.n_vtx;
    const int64_t *adj_off = g.adj_off;
    const int32_t *adj = g.adj, *topo_rank = g.topo_rank, *cnt_edge = g.cnt_edge;
    std::vector<int32_t> cont_total((size_t)n_vtx, 0);
    for (int32_t u = 0; u < n_vtx; u++)
        for (int64_t x = adj_off[u]; x < adj_off[u + 1]; x++) cont_total[(size_t)u] += cnt_edge[x];
    out.st_rec.reset(new int32_t[(size_t)n_vtx * 8]);
    int32_t *const st_rec = out.st_rec.get();
    std::vector<int32_t> &in_packed = out.in_packed;
    // live in-edges of v: (u, x) with some walk on u continuing along another edge than x
    std::vector<int32_t> live_cnt((size_t)n_vtx + 1, 0);
    std::vector<uint8_t> tops((size_t)n_vtx, 0);
    const int64_t VCH = 1 << 16;
    phi_parallel_chunks(n_vtx, VCH, [&](int64_t lo, int64_t hi, int) {
        for (int64_t u = lo; u < hi; u++)
            for (int64_t x = adj_off[u]; x < adj_off[u + 1]; x++)
                if (cont_total[(size_t)u] - cnt_edge[x] > 0) {
                    const int64_t back = (int64_t)topo_rank[adj[x]] - topo_rank[u];
                    if (back >= (1 << 23)) { err.set(PHI_ERR_UNSUPPORTED, "edge spans more than 2^23 topological steps"); return; }
                    __atomic_fetch_add(&live_cnt[(size_t)adj[x] + 1], 1, __ATOMIC_RELAXED);
                    tops[(size_t)u] = 1;
                }
    });
    if (err.failed()) return err.code;
    for (int32_t v = 0; v < n_vtx; v++) live_cnt[(size_t)v + 1] += live_cnt[(size_t)v];
    std::vector<int32_t> live((size_t)std::max<int32_t>(live_cnt[(size_t)n_vtx], 1)), cur(live_cnt.begin(), live_cnt.end() - 1);
    phi_parallel_chunks(n_vtx, VCH, [&](int64_t lo, int64_t hi, int) {
        for (int64_t u = lo; u < hi; u++)
            for (int64_t x = adj_off[u]; x < adj_off[u + 1]; x++)
                if (cont_total[(size_t)u] - cnt_edge[x] > 0) {
                    const int64_t back = (int64_t)topo_rank[adj[x]] - topo_rank[u];
                    live[(size_t)__atomic_fetch_add(&cur[(size_t)adj[x]], 1, __ATOMIC_RELAXED)] = (int32_t)(back << 8) | (int32_t)(x - adj_off[u]);
                }
    });
    // the in-edges beyond the third of a step go to in_packed: where, from the counts
    std::vector<int64_t> extra_off((size_t)n_vtx + 1, 0);
    for (int32_t s = 0; s < n_vtx; s++) {
        const int32_t v = g.topo[s];
        const int n_in = live_cnt[(size_t)v + 1] - live_cnt[(size_t)v];
        if (n_in > 255) { err.set(PHI_ERR_UNSUPPORTED, "vertex %d has more than 255 in-edges", v); return err.code; }
        extra_off[(size_t)s + 1] = extra_off[(size_t)s] + std::max(0, n_in - 3);
    }
    if (extra_off[(size_t)n_vtx] > INT32_MAX) { err.set(PHI_ERR_UNSUPPORTED, "more than 2^31 recombination in-edges"); return err.code; }
    in_packed.assign((size_t)extra_off[(size_t)n_vtx], 0);
    phi_parallel_chunks(n_vtx, VCH, [&](int64_t lo, int64_t hi, int) {
        for (int64_t s = lo; s < hi; s++) {
            const int32_t v = g.topo[(size_t)s];
            int32_t *r = &st_rec[(size_t)s * 8];
            const int n_in = live_cnt[(size_t)v + 1] - live_cnt[(size_t)v];
            int32_t *in = live.data() + live_cnt[(size_t)v];
            if (n_in > 1) std::sort(in, in + n_in);
            r[0] = (n_in ? PHI_DP_NEED_ENTRY : 0) | (tops[(size_t)v] ? PHI_DP_NEED_TOPS : 0) | (n_in << 8);
            r[1] = (int32_t)extra_off[(size_t)s];
            r[2] = r[3] = r[4] = 0;
            for (int j = 0; j < n_in; j++) {
                if (j < 3) r[2 + j] = in[j];
                else in_packed[(size_t)extra_off[(size_t)s] + (size_t)(j - 3)] = in[j];
            }
            r[5] = v; r[6] = 0; r[7] = 0;
        }
    });
    return PHI_OK;
}

// ---- compact step stream of the event-driven DP (dp_events.hip): only the vertices where a recombination can enter or
//      leave, or a walk starts or ends; in-edges count compact steps back.  After phi_dp_steps_dense.
static inline int phi_dp_steps_compact(const PhiDpGraph &g, PhiDpSteps &out, PhiHostError &err)
{
    const int32_t n_vtx = g.n_vtx;
    const int32_t *const st_rec = out.st_rec.get();
    std::vector<int32_t> &k_rec = out.k_rec, &k_in = out.k_in, &cvtx = out.cvtx, &cstep = out.cstep, &kstep = out.kstep;
    std::vector<uint8_t> lane_only((size_t)n_vtx, 0);
    for (int64_t i = 0; i < 2 * (int64_t)g.n_walks; i++) lane_only[(size_t)g.walk_ends[i]] = 1;
    {
        // the compact steps, numbered in step order: counted per chunk of steps, then written, by all threads
        const int64_t SCH = 1 << 16, n_sch = ((int64_t)n_vtx + SCH - 1) / SCH;
        std::vector<int32_t> ch_cnt((size_t)n_sch + 1, 0);
        cstep.resize((size_t)n_vtx);
        auto keeps = [&](int64_t s_) { return (st_rec[(size_t)s_ * 8] & 3) || lane_only[(size_t)g.topo[(size_t)s_]]; };
        phi_parallel_chunks(n_vtx, SCH, [&](int64_t lo, int64_t hi, int) {
            int32_t n = 0;
            for (int64_t s_ = lo; s_ < hi; s_++) n += keeps(s_);
            ch_cnt[(size_t)(lo / SCH) + 1] = n;
        });
        for (int64_t i = 0; i < n_sch; i++) ch_cnt[(size_t)i + 1] += ch_cnt[(size_t)i];
        kstep.resize((size_t)ch_cnt[(size_t)n_sch]);
        phi_parallel_chunks(n_vtx, SCH, [&](int64_t lo, int64_t hi, int) {
            int32_t k_ = ch_cnt[(size_t)(lo / SCH)];
            for (int64_t s_ = lo; s_ < hi; s_++) {
                if (keeps(s_)) { cstep[(size_t)s_] = k_; kstep[(size_t)k_++] = (int32_t)s_; }
                else cstep[(size_t)s_] = -1;
            }
        });
    }
    const int32_t n_k = out.n_k = (int32_t)kstep.size();
    k_rec.assign((size_t)n_k * 8, 0); k_in.clear(); cvtx.assign((size_t)n_vtx, 0);
    for (int32_t k = 0; k < n_k; k++) {
        const int32_t s = kstep[(size_t)k];
        const int32_t *ro = &st_rec[(size_t)s * 8];
        int32_t *r = &k_rec[(size_t)k * 8];
        const int n_in = (ro[0] >> 8) & 0xFF;
        r[0] = ro[0] | (lane_only[(size_t)g.topo[s]] ? PHI_DP_LANE_ONLY : 0);
        r[1] = (int32_t)k_in.size();
        for (int j = 0; j < n_in; j++) {
            const int32_t p = j < 3 ? ro[2 + j] : out.in_packed[(size_t)(ro[1] + j - 3)];
            const int32_t kc = cstep[(size_t)(s - (int32_t)((uint32_t)p >> 8))];
            if (kc < 0) { err.set(PHI_ERR_DEVICE, "live in-edge from a vertex without leaving states (internal error)"); return err.code; }
            const int32_t pc = ((k - kc) << 8) | (p & 0xFF);
            if (j < 3) r[2 + j] = pc; else k_in.push_back(pc);
        }
        r[5] = ro[5];
    }
    // two alleles of one site: consecutive in topological order, no edge between them (so no walk
    // visits both), neither leaves recombination states -> the consumer takes them in one iteration
    out.n_pairs = 0;
    for (int32_t k = 0; k + 1 < n_k; k++) {
        int32_t *r0 = &k_rec[(size_t)k * 8], *r1 = r0 + 8;
        if ((r0[0] | r1[0]) & PHI_DP_NEED_TOPS) continue;
        const int32_t s0 = kstep[(size_t)k], s1 = kstep[(size_t)k + 1];
        if (s1 != s0 + 1) continue;
        const int32_t v0 = g.topo[s0], v1 = g.topo[s1];
        bool edge = false;
        for (int64_t a = g.adj_off[v0]; a < g.adj_off[v0 + 1] && !edge; a++) edge = g.adj[a] == v1;
        if (edge) continue;
        r0[0] |= PHI_DP_PAIR;
        out.n_pairs++;
        k++;                                           // pairs do not overlap
    }
    phi_parallel_chunks(n_vtx, 1 << 16, [&](int64_t lo, int64_t hi, int) { for (int64_t v = lo; v < hi; v++) cvtx[(size_t)v] = cstep[(size_t)g.topo_rank[v]]; });
    return PHI_OK;
}

// where the chain of compact steps may be cut (dp_blocks.hip, blocks in parallel): not between the two steps of a pair,
// and only where no recombination edge of this or a later step comes from before the cut.  After phi_dp_steps_compact.
static inline void phi_dp_steps_cuts(PhiDpSteps &out)
{
    const int32_t n_k = out.n_k;
    const std::vector<int32_t> &k_rec = out.k_rec, &k_in = out.k_in;
    out.cut_ok.assign((size_t)n_k + 1, 1);
    int32_t min_src = INT32_MAX;                       // smallest source step of an in-edge of any step >= k
    for (int32_t k = n_k - 1; k >= 0; k--) {
        const int32_t *r = &k_rec[(size_t)k * 8];
        const int n_in = (r[0] >> 8) & 0xFF;
        for (int j = 0; j < n_in; j++) {
            const int32_t pk = j < 3 ? r[2 + j] : k_in[(size_t)r[1] + j - 3];
            min_src = std::min(min_src, k - (int32_t)((uint32_t)pk >> 8));
        }
        if (min_src < k) out.cut_ok[(size_t)k] = 0;
        if (k > 0 && (k_rec[(size_t)(k - 1) * 8] & PHI_DP_PAIR)) out.cut_ok[(size_t)k] = 0;
    }
    out.cut_ok[0] = 0; out.cut_ok[(size_t)n_k] = 0;
}
