// solve_host.h -- the rules of phi_solve that need no GPU, over plain arrays and vectors: where the chain of compact steps
// is cut into blocks, the max-plus chain over the blocks' transfer rows, the host arrays of the dp anchors and their score
// bound, the minimiser -> anchors map and the repeat set, the clusters of mutually exclusive anchors, and the set
// tightening and branch choice of the exact search.
// No HIP include and nothing of the context: phi_solve.hip calls it between its launches, and host/solve_host_selftest.cpp
// runs it stand-alone under the sanitizers.  Every result is independent of thread timing.  A function that refuses its
// input has set `err` (code and text of the phi_fail its caller makes of it) and returns err.code.
#pragma once
#include <limits.h>
#include <map>
#include <set>
#include "../../include/phi_amd.h"
#include "phi_dp_flags.h"
#include "phi_host_par.h"

struct PhiAnchorHost {       // one dp anchor on the host (certificate / branch-and-bound)
    uint32_t slot;           // minimiser identity: dense id (rank of first occurrence among the walk minimisers)
    uint32_t e0, e1;         // first / last walk entry (phi_ent_t of phi_kernels.h: unsigned, below PHI_MAX_ENTRIES)
};

// view of host anchors: the pinned download buffer, or an owned vector
struct PhiAnchorSpan {
    PhiAnchorHost *p = nullptr;
    int64_t n = 0;
    size_t size() const { return (size_t)n; }
    PhiAnchorHost &operator[](int64_t i) const { return p[i]; }
    PhiAnchorHost *begin() const { return p; }
    PhiAnchorHost *end() const { return p + n; }
};

// walk of a walk entry; walk_off: [n_walks + 1]
static inline int32_t phi_walk_of_entry(const int64_t *walk_off, int32_t n_walks, int64_t e)
{
    return (int32_t)(std::upper_bound(walk_off, walk_off + n_walks + 1, e) - walk_off) - 1;
}

// ------------------------------------------------------------------------------------------ block placement
// A cut may sit before step k when the graph allows it (graph_ok, [n_k + 1]) and no walk forbids it (closed, [n_k + 2],
// prefix-summed: > 0 = some walk has no entry clean of anchors around the cut).
struct PhiCutFlags {
    const int32_t *graph_ok, *closed;
    int32_t nk;
    bool operator()(int32_t k) const { return k > 0 && k < nk && graph_ok[(size_t)k] && closed[(size_t)k] == 0; }
};

// Cuts the nk compact steps into blocks of about target_of(ring) steps, none longer than the ring of tops it is placed at:
// the first ring of `rings` (ascending) at which every stretch without an allowed cut fits.  A ring of 256 is passed over
// when no_small is set.  Returns that ring with blk_lo = the first step of every block and nk at the end, or 0: the chain
// stays whole (blk_lo is then what the last ring tried left behind).
template <class T> static int32_t phi_place_blocks(const PhiCutFlags &cut_ok, const int32_t *rings, int n_rings, bool no_small, T target_of,
                                                   std::vector<int32_t> &blk_lo)
{
    const int32_t nk = cut_ok.nk;
    for (int ri = 0; ri < n_rings; ri++) {
        const int32_t ring = rings[ri];
        if (ring == 256 && no_small) continue;
        const int64_t target = target_of(ring);
        blk_lo.assign(1, 0);
        bool ok = true;
        for (int32_t start = 0; nk - start > target && ok;) {
            int32_t cut = -1;
            const int32_t hi = (int32_t)std::min<int64_t>((int64_t)start + ring, nk - 1);
            for (int32_t k = (int32_t)(start + target); k <= hi && cut < 0; k++) if (cut_ok(k)) cut = k;
            for (int32_t k = (int32_t)(start + target) - 1; k > start && cut < 0; k--) if (cut_ok(k)) cut = k;
            if (cut < 0) {
                if (nk - start > ring) ok = false;             // no usable cut within a ring's length
                break;                                         // (else: the rest is one block)
            }
            blk_lo.push_back(cut);
            start = cut;
        }
        if (ok && nk - blk_lo.back() <= ring) { blk_lo.push_back(nk); return ring; }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ max-plus chain
// Blocks on walk lanes: rows[(b * (nwk + 1) + j) * 64 + h] is the key on walk h at the end of block b of a run that entered
// the block on walk j (j == nwk: that began inside it), rowend[b * (nwk + 1) + j] the best value of a path that ends inside.
// The chain  S_{b+1}[h'] = max(rows of walk starts, max_j S_b[j] + row_j[h'])  (max-plus, PHI_DP_NEGK = no run) gives
// S[b * 64 + h] = the key entering block b on walk h.  Returns the best value of a path that ends inside a block
// (INT64_MIN: none).
static inline int64_t phi_chain_blocks(const int32_t *rows, const int32_t *rowend, int32_t nb, int32_t nwk, std::vector<int32_t> &S)
{
    const int32_t nrow = nwk + 1;
    S.assign((size_t)nb * 64, PHI_DP_NEGK);
    std::vector<int64_t> cur(64, PHI_DP_NEGK), nxt(64);
    int64_t end_best = INT64_MIN;
    for (int32_t b = 0; b < nb; b++) {
        for (int h = 0; h < 64; h++) S[(size_t)b * 64 + h] = cur[h] > PHI_DP_NEGK / 2 ? (int32_t)cur[h] : PHI_DP_NEGK;
        std::fill(nxt.begin(), nxt.end(), (int64_t)PHI_DP_NEGK);
        for (int32_t j = 0; j <= nwk; j++) {
            const int64_t base = j == nwk ? 0 : cur[j];
            if (j < nwk && base <= PHI_DP_NEGK / 2) continue;
            const int32_t *row = &rows[((size_t)b * nrow + j) * 64];
            for (int32_t h2 = 0; h2 < nwk; h2++)
                if (row[h2] > PHI_DP_NEGK / 2) nxt[h2] = std::max(nxt[h2], base + row[h2]);
            const int32_t re = rowend[(size_t)b * nrow + j];
            if (re > -(1 << 27)) end_best = std::max(end_best, base + re);
        }
        cur.swap(nxt);
    }
    return end_best;
}

// The second pass (every block from its true entry vector) must agree with the chain on what leaves every block:
// keys[b * 64 + h] against S[(b + 1) * 64 + h]; two "no run" values agree whatever they are (a walk that begins inside
// block b + 1 or ended before it carries nothing that is ever read).  False: the first disagreement in (b, h, got, want).
static inline bool phi_chain_agrees(const int32_t *S, const int32_t *keys, int32_t nb, int32_t nwk, int32_t *b_, int32_t *h_, int32_t *got_, int32_t *want_)
{
    for (int32_t b = 0; b + 1 < nb; b++)
        for (int32_t h = 0; h < nwk; h++) {
            const int32_t want = S[(size_t)(b + 1) * 64 + h], got = keys[(size_t)b * 64 + h];
            if (want != got && !(want <= PHI_DP_NEGK / 2 && got <= PHI_DP_NEGK / 2)) { *b_ = b; *h_ = h; *got_ = got; *want_ = want; return false; }
        }
    return true;
}

// ------------------------------------------------------------------------------------------ host anchor arrays
// From the kept triples (in walk order, and within a walk by position): the dp anchors (span >= 1 edge; single-vertex
// anchors are ignored, ILP_index.cpp:795/:846) and the DP's per-anchor arrays, on host threads over chunks of the kept
// list, order preserved.
struct PhiAnchorArrays {
    PhiAnchorSpan dp;                                          // the kept list itself (usually: vertices shorter than k), or dp_own
    std::vector<int16_t> dp_walk;                              // walk of every dp anchor
    std::vector<uint32_t> a_e1;                                // its last entry
    std::vector<uint8_t> a_span;                               // the edges it spans
};
// dp_own: storage of the dp list where it is shorter than the kept list (cleared otherwise); n_anchors: [n_walks] kept
// anchors per walk.  Refused: an anchor that spans PHI_RCAP edges or more (k: the code depends on it), dp anchors not
// sorted by last entry.
static inline int phi_anchor_arrays(PhiAnchorSpan kept, const int64_t *walk_off, int32_t nw, int32_t k, std::vector<PhiAnchorHost> &dp_own,
                                    PhiAnchorArrays &A, std::vector<int64_t> &n_anchors, PhiHostError &herr)
{
    const int64_t n_kept = kept.n;
    n_anchors.assign(nw, 0);
    const int64_t chunk = (int64_t)1 << 16;
    const int64_t n_chunks = (n_kept + chunk - 1) / chunk;
    std::vector<int64_t> dp_cnt(n_chunks + 1, 0);
    std::vector<std::vector<int32_t>> walk_cnt(phi_host_threads(), std::vector<int32_t>(nw, 0));
    phi_parallel_chunks(n_kept, chunk, [&](int64_t lo, int64_t hi, int worker) {
        int64_t n = 0;
        int32_t hw = phi_walk_of_entry(walk_off, nw, kept[lo].e0);
        for (int64_t i = lo; i < hi; i++) {
            const PhiAnchorHost &a = kept[i];
            n += a.e1 > a.e0;
            while (a.e0 >= walk_off[hw + 1]) hw++;               // kept anchors come in walk order
            walk_cnt[worker][hw]++;
        }
        dp_cnt[lo / chunk + 1] = n;
    });
    for (int64_t i = 0; i < n_chunks; i++) dp_cnt[i + 1] += dp_cnt[i];
    for (const auto &wc : walk_cnt) for (int32_t h = 0; h < nw; h++) n_anchors[h] += wc[h];
    const int64_t n_dp0 = dp_cnt[n_chunks];
    // usually every kept anchor spans an edge (vertices shorter than k): the dp list is the kept list
    const bool same = n_dp0 == n_kept;
    if (same) { dp_own.clear(); A.dp = kept; }
    else { dp_own.resize(n_dp0); A.dp = PhiAnchorSpan{dp_own.data(), n_dp0}; }
    A.dp_walk.resize(n_dp0);
    A.a_e1.resize(n_dp0);
    A.a_span.resize(n_dp0);
    phi_parallel_chunks(n_kept, chunk, [&](int64_t lo, int64_t hi, int) {
        int64_t o = dp_cnt[lo / chunk];
        int32_t hw = phi_walk_of_entry(walk_off, nw, kept[lo].e0);
        for (int64_t i = lo; i < hi; i++) {
            const PhiAnchorHost &a = kept[i];
            while (a.e0 >= walk_off[hw + 1]) hw++;
            if (a.e1 <= a.e0) continue;
            A.dp_walk[o] = (int16_t)hw;
            if (a.e1 - a.e0 >= (uint32_t)PHI_RCAP) { herr.set(k > PHI_RCAP ? PHI_ERR_UNSUPPORTED : PHI_ERR_DEVICE, "an anchor spans %u edges (at most %d are supported)", a.e1 - a.e0, PHI_RCAP - 1); return; }
            if (!same) A.dp[o] = a;
            A.a_e1[o] = a.e1;
            A.a_span[o] = (uint8_t)(a.e1 - a.e0);
            o++;
        }
    });
    if (herr.failed()) return herr.code;
    phi_parallel_chunks(n_dp0, chunk, [&](int64_t lo, int64_t hi, int) {
        for (int64_t i = std::max<int64_t>(lo, 1); i < hi; i++)
            if (A.a_e1[i] < A.a_e1[i - 1]) { herr.set(PHI_ERR_DEVICE, "dp anchors not sorted by last entry (internal error)"); return; }
    });
    return herr.failed() ? herr.code : PHI_OK;
}

// A path is on one walk at every vertex, so it scores at most the sum over vertices of the most anchors that end there on
// one walk: that sum, not the number of anchors, has to stay inside the DP's score range.  a_e1: ascending.
static inline int64_t phi_score_bound(const uint32_t *a_e1, int64_t n_dp, const int32_t *walk_vtx, int32_t n_vtx)
{
    std::vector<int32_t> vmax((size_t)n_vtx, 0);
    for (int64_t i = 0; i < n_dp;) {
        int64_t j = i;
        while (j < n_dp && a_e1[j] == a_e1[i]) j++;
        int32_t &m = vmax[walk_vtx[a_e1[i]]];
        m = std::max<int32_t>(m, (int32_t)std::min<int64_t>(j - i, INT32_MAX));
        i = j;
    }
    int64_t bound = 0;
    for (int32_t m : vmax) bound += m;
    return bound;
}

// ------------------------------------------------------------------------------------------ minimiser -> anchors map, repeats
// dp anchors of every minimiser (CSR over the dense minimiser ids), ascending anchor index.  False: an id of n_ids or more.
// (tried on host threads with atomic counters and per-list sorts: 7.5 ms against 4.3 ms for this loop)
static inline bool phi_anchor_csr(PhiAnchorSpan dp, int64_t n_ids, std::vector<int32_t> &sa_off, std::vector<int32_t> &sa_idx)
{
    const int64_t n_dp = dp.n;
    sa_off.assign((size_t)n_ids + 1, 0);
    sa_idx.resize((size_t)std::max<int64_t>(n_dp, 1));
    for (const PhiAnchorHost &a : dp) {
        if ((int64_t)a.slot >= n_ids) return false;
        sa_off[a.slot + 1]++;
    }
    for (int64_t i = 0; i < n_ids; i++) sa_off[i + 1] += sa_off[i];
    std::vector<int32_t> cur(sa_off.begin(), sa_off.end() - 1);
    for (int64_t i = 0; i < n_dp; i++) sa_idx[cur[dp[i].slot]++] = (int32_t)i;
    return true;
}

// Minimisers with two anchors on ONE walk (repeats along a haplotype): the anchors of a minimiser ascend, and with them
// their walks, so two on one walk are neighbours in its list.
static inline void phi_repeat_set(const std::vector<int32_t> &sa_off, const std::vector<int32_t> &sa_idx, const std::vector<int16_t> &dp_walk, int64_t n_ids,
                                  std::set<uint32_t> &S0)
{
    std::vector<std::vector<uint32_t>> found(phi_host_threads());
    phi_parallel_chunks(n_ids, (int64_t)1 << 14, [&](int64_t lo, int64_t hi, int worker) {
        for (int64_t u = lo; u < hi; u++)
            for (int32_t j = sa_off[u] + 1; j < sa_off[u + 1]; j++)
                if (dp_walk[sa_idx[j]] == dp_walk[sa_idx[j - 1]]) { found[worker].push_back((uint32_t)u); break; }
    });
    for (const auto &f : found) S0.insert(f.begin(), f.end());
}

// ------------------------------------------------------------------------------------------ clusters
// Clusters of pairwise mutually exclusive anchors of one minimiser: anchors on different walks whose topological-rank
// intervals overlap cannot both be traversed (a path holds one haplotype label per vertex).  Anything else becomes a
// singleton cluster.
struct PhiAnchorIv { int32_t lo, hi, h, a; };                  // rank of first vertex, rank of last vertex, walk, anchor index
static inline std::vector<std::vector<int32_t>> phi_clusters(std::vector<PhiAnchorIv> iv)
{
    typedef PhiAnchorIv Iv;
    std::sort(iv.begin(), iv.end(), [](const Iv &x, const Iv &y) { return x.lo != y.lo ? x.lo < y.lo : x.a < y.a; });
    std::vector<std::vector<int32_t>> out;
    std::vector<Iv> cur;
    auto flush = [&]() {
        if (cur.empty()) return;
        bool ok = true;
        for (size_t i = 0; i < cur.size() && ok; i++)
            for (size_t j = i + 1; j < cur.size() && ok; j++)
                ok = cur[i].h != cur[j].h && cur[i].lo <= cur[j].hi && cur[j].lo <= cur[i].hi;
        if (ok) { out.emplace_back(); for (const Iv &x : cur) out.back().push_back(x.a); }
        else for (const Iv &x : cur) out.push_back({x.a});
        cur.clear();
    };
    int32_t reach = -1;
    for (const Iv &x : iv) {
        if (!cur.empty() && x.lo > reach) flush();
        cur.push_back(x);
        reach = std::max(reach, x.hi);
    }
    flush();
    return out;
}

// ------------------------------------------------------------------------------------------ tighten and branch
// Tighten: bound the doubly-counted minimisers D by the constant 1, release the unused constants Z.  S becomes
// S + D - Z and S as it was is remembered in `seen`; false (S and seen untouched): that set is S itself or was seen before.
static inline bool phi_tighten(std::set<uint32_t> &S, const std::set<uint32_t> &D, const std::set<uint32_t> &Z, std::set<std::set<uint32_t>> &seen)
{
    std::set<uint32_t> S2 = S;
    for (uint32_t s : D) S2.insert(s);
    for (uint32_t s : Z) S2.erase(s);
    if (S2 == S || seen.count(S2)) return false;
    seen.insert(S);
    S.swap(S2);
    return true;
}

// The minimiser to branch on, in canonical = first anchor order: the lowest first anchor among lastD, else (lastD empty)
// among the minimisers of lastZ the node has not assigned yet.  False: none.
static inline bool phi_choose_branch(const std::set<uint32_t> &lastD, const std::set<uint32_t> &lastZ, const std::map<uint32_t, int32_t> &assign,
                                     const std::vector<int32_t> &sa_off, const std::vector<int32_t> &sa_idx, uint32_t *slot)
{
    auto first_anchor = [&](uint32_t s) { return sa_idx[(size_t)sa_off[s]]; };
    int32_t best_a = INT32_MAX;
    for (uint32_t s : lastD) if (first_anchor(s) < best_a) { best_a = first_anchor(s); *slot = s; }
    if (lastD.empty()) for (uint32_t s : lastZ) if (!assign.count(s) && first_anchor(s) < best_a) { best_a = first_anchor(s); *slot = s; }
    return best_a != INT32_MAX;
}
