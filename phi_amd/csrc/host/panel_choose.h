// panel_choose.h -- the rule that picks a panel of walks from the read support per block and walk (phi_scout_scores).
// Plain host code on the host threads (../phi_host_par.h), no HIP include: libphi_host.so exports it as phi_panel_choose,
// libphi_amd.so calls it from phi_scout_choose, panel_choose_selftest.cpp runs it under the sanitizers.
//
// It stands in for the step the reference leaves to other tools: `vg haplotypes` samples a personalised panel from the
// reads' k-mers (data/vg_haplotypes.py:21-29), the reference's own panels are lists of names (data/chop_graph.sh:46-66).
// THE RULE IS THIS PROJECT'S OWN; it is not `vg haplotypes`' and has not been compared with it.
//
//   1. the `always` walks are in; more of them than n_want: refused.  1 <= n_want <= min(n_walks, 1022)
//   2. in block b the walks are ordered by (-S[b][h], h)
//   3. round r = 0, 1, ...: votes[h] = the number of blocks whose r-th walk is h with S[b][h] > 0; the walks with votes that
//      are not yet in enter in the order (votes descending, total = sum over b of S[b][h] descending, id ascending) until
//      the panel holds n_want walks
//   4. a round that brings no votes ends the rounds: the rest is filled by (total descending, id ascending)
// round_of[h]: -1 an `always` walk, r entered in round r, n_walks entered in the fill, -2 not chosen.
//
// The r-th walk of a block is found lazily.  While the panel is not full, a round r has r < n_want: once every block's
// first r + 1 walks are in, the panel holds r + 1 walks at least.  So a block keeps only its n_want best cells above zero
// (a selection, not a sort) and sorts a prefix of them that doubles when a round asks beyond it.  Host memory beside the
// matrix: 8 bytes x n_blocks x min(n_want, walks above zero in the block) -- 0.5 GB at 65 536 blocks and n_want = 1022.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "../phi_host_par.h"

#define PHI_PANEL_CHOOSE_MAX 1022     // the DP's walks (PHI_DP_MAX_WALKS of ../phi_kernels.h)

// returns 0, or -1 for arguments the rule refuses; *n_rounds (may be NULL): the rounds that were run
static inline int phi_panel_choose_rule(const int32_t *S, int32_t n_blocks, int32_t n_walks, const uint8_t *always, int32_t n_want,
                                        uint8_t *keep, int32_t *round_of, int32_t *n_rounds)
{
    if (n_rounds) *n_rounds = 0;
    if (!S || !keep || n_blocks < 1 || n_walks < 1) return -1;
    if (n_want < 1 || n_want > n_walks || n_want > PHI_PANEL_CHOOSE_MAX) return -1;
    int32_t n_in = 0;
    for (int32_t h = 0; h < n_walks; h++) n_in += always && always[h];
    if (n_in > n_want) return -1;
    for (int32_t h = 0; h < n_walks; h++) {
        keep[h] = always && always[h];
        if (round_of) round_of[h] = keep[h] ? -1 : -2;
    }
    // totals: every thread sums the columns of its blocks, the partial sums are added in thread order
    const int nt = phi_host_threads();
    std::vector<std::vector<int64_t>> part((size_t)nt);
    phi_parallel_chunks(n_blocks, 64, [&](int64_t lo, int64_t hi, int worker) {
        std::vector<int64_t> &p = part[(size_t)worker];
        if (p.empty()) p.assign((size_t)n_walks, 0);
        for (int64_t b = lo; b < hi; b++) {
            const int32_t *row = S + b * n_walks;
            for (int32_t h = 0; h < n_walks; h++) p[(size_t)h] += row[h];
        }
    });
    std::vector<int64_t> total((size_t)n_walks, 0);
    for (const auto &p : part)
        if (!p.empty()) for (int32_t h = 0; h < n_walks; h++) total[(size_t)h] += p[(size_t)h];

    typedef std::pair<int32_t, int32_t> Cell;                // (score, walk)
    const auto before = [](const Cell &a, const Cell &b) { return a.first != b.first ? a.first > b.first : a.second < b.second; };
    std::vector<std::vector<Cell>> cells((size_t)n_blocks);
    std::vector<size_t> sorted((size_t)n_blocks, 0);
    std::vector<int32_t> pick((size_t)n_blocks), votes((size_t)n_walks), cand;
    bool collected = false;
    for (int32_t r = 0; n_in < n_want && r < n_walks; r++) {
        phi_parallel_chunks(n_blocks, 16, [&](int64_t lo, int64_t hi, int) {
            for (int64_t b = lo; b < hi; b++) {
                std::vector<Cell> &c = cells[(size_t)b];
                if (!collected) {
                    const int32_t *row = S + b * n_walks;
                    for (int32_t h = 0; h < n_walks; h++) if (row[h] > 0) c.emplace_back(row[h], h);
                    if (c.size() > (size_t)n_want) {
                        std::nth_element(c.begin(), c.begin() + n_want, c.end(), before);
                        c.resize((size_t)n_want);
                        c.shrink_to_fit();
                    }
                }
                pick[(size_t)b] = -1;
                if ((size_t)r >= c.size()) continue;
                size_t &done = sorted[(size_t)b];
                if ((size_t)r >= done) {
                    const size_t upto = std::min(c.size(), std::max<size_t>(2 * done, 8));
                    std::partial_sort(c.begin() + (ptrdiff_t)done, c.begin() + (ptrdiff_t)upto, c.end(), before);
                    done = upto;
                }
                pick[(size_t)b] = c[(size_t)r].second;
            }
        });
        collected = true;
        std::fill(votes.begin(), votes.end(), 0);
        bool any = false;
        for (int32_t b = 0; b < n_blocks; b++) if (pick[(size_t)b] >= 0) { votes[(size_t)pick[(size_t)b]]++; any = true; }
        if (!any) break;
        if (n_rounds) *n_rounds = r + 1;
        cand.clear();
        for (int32_t h = 0; h < n_walks; h++) if (votes[(size_t)h] > 0 && !keep[h]) cand.push_back(h);
        std::sort(cand.begin(), cand.end(), [&](int32_t a, int32_t b) {
            if (votes[(size_t)a] != votes[(size_t)b]) return votes[(size_t)a] > votes[(size_t)b];
            if (total[(size_t)a] != total[(size_t)b]) return total[(size_t)a] > total[(size_t)b];
            return a < b;
        });
        for (int32_t h : cand) {
            if (n_in >= n_want) break;
            keep[h] = 1; n_in++;
            if (round_of) round_of[h] = r;
        }
    }
    if (n_in < n_want) {
        cand.clear();
        for (int32_t h = 0; h < n_walks; h++) if (!keep[h]) cand.push_back(h);
        std::sort(cand.begin(), cand.end(), [&](int32_t a, int32_t b) {
            if (total[(size_t)a] != total[(size_t)b]) return total[(size_t)a] > total[(size_t)b];
            return a < b;
        });
        for (int32_t h : cand) {
            if (n_in >= n_want) break;
            keep[h] = 1; n_in++;
            if (round_of) round_of[h] = n_walks;
        }
    }
    return 0;
}
