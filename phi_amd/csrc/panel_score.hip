// panel_score.hip -- read support per block of the graph and per walk, for the panel chosen from the reads (phi_scout_scores)
// and the choice on top of it (phi_scout_choose).
//
// It stands in for the k-mer counting of `vg haplotypes` (data/vg_haplotypes.py:21-29), which answers "which haplotypes does
// this read set look like" before anything is inferred, and feeds the step that data/chop_graph.sh:46-66 does by name.
//
// S[b][h] = the number of minimiser occurrences (hash, pos) of walk h -- the list phi_walk_minimizers(h) returns -- whose
// hash has its hit flag set and whose base pos lies in a vertex of block b; block of vertex v = topo_rank[v] * n_blocks /
// n_vtx.  The occurrences of a walk are never stored: they are the class records of its entries (contexts.hip), and the
// entry that owns a record's first base, rec_e0 relative to the class representative, names the same vertex for every
// entry of the class.  So:
//     record   per class record, once: its block from walk_vtx[rec_e0[r]] and its hit bit from hits[u_uid[rec_slot[r]]],
//              packed into one word (block << 1 | hit)
//     class    per class, once: (block of its first record, hit records in that block) as 8 bytes, and a flag when a record
//              of the class lies in another block (a k-mer that starts in a later vertex, across a block border)
//     entry    one pass over the walk entries in the manner of phi_walk_sum_kernel (contexts.hip): every wave takes a
//              contiguous slice, a row of 64 entries reads 4 bytes each plus the 8-byte gather from the class table, and
//              the (walk, block) cell of every lane is its key.  A row that lies in one cell -- nearly every row of a long
//              walk -- is added lane by lane into the run carried along, without a shuffle, as phi_walk_sum_kernel adds;
//              in any other row equal keys of neighbouring lanes form runs that a segmented scan over the lanes sums
//              (phi_wave.h's shuffles), the run that reaches the row's last lane is carried on, and every other run costs
//              ONE atomic, by its last lane.  Ranks ascend along a walk,
//              so a walk's blocks are contiguous runs and a wave meets few of them -- that is for speed only: any order of
//              keys gives the same sums.  A flagged class adds its records outside the first block one by one; an entry
//              whose class has no record borrows its neighbour's key, so that it does not break a row.
// 4 bytes and one gather per entry, as phi_walk_sum_kernel<true>: bound by HBM and by the gather's hit rate in the cache.
// Thousands of atomics onto a few addresses would serialise at ~12 ns each (the note in contexts.hip); here an address is
// added to once per run and wave.
#include <string.h>
#include <algorithm>
#include "phi_ctx.h"
#include "phi_wave.h"
#include "host/panel_choose.h"

#define SCORE_MAX_BLOCKS 65536

namespace {

unsigned grid_for(int64_t n, int tpb, int64_t cap)
{
    const int64_t nb = (n + tpb - 1) / tpb;
    return (unsigned)std::max<int64_t>(1, std::min(nb, cap));
}

__global__ void __launch_bounds__(256) score_record_kernel(const phi_ent_t *__restrict__ rec_e0, const uint32_t *__restrict__ rec_slot, int64_t n_rec,
                                                           const int32_t *__restrict__ walk_vtx, const int32_t *__restrict__ topo_rank,
                                                           const uint32_t *__restrict__ u_uid, const uint8_t *__restrict__ hits, int32_t n_vtx,
                                                           int32_t n_blocks, int32_t *__restrict__ rec_bh)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t v = walk_vtx[rec_e0[r]];                // (in range: the walk-entry pass has checked every entry)
        const int32_t b = (int32_t)((int64_t)topo_rank[v] * n_blocks / n_vtx);
        rec_bh[r] = b << 1 | (hits[u_uid[rec_slot[r]]] != 0);
    }
}

// cls_tab[c] = (block of the first record, hit records in that block << 1 | a record lies in another block); a class without
// records (an entry in which no k-mer starts: common where vertices are a few bases long) has block -1
__global__ void __launch_bounds__(256) score_class_kernel(const int32_t *__restrict__ cls_rec_off, int64_t n_cls, const int32_t *__restrict__ rec_bh,
                                                          int2 *__restrict__ cls_tab, unsigned long long *__restrict__ n_flagged)
{
    int mine = 0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_cls; c += (int64_t)gridDim.x * blockDim.x) {
        const int32_t lo = cls_rec_off[c], hi = cls_rec_off[c + 1];
        int32_t b0 = -1, sum = 0, other = 0;
        if (hi > lo) {
            b0 = rec_bh[lo] >> 1;
            for (int32_t r = lo; r < hi; r++) {
                const int32_t x = rec_bh[r];
                if ((x >> 1) == b0) sum += x & 1; else other = 1;
            }
        }
        cls_tab[c] = make_int2(b0, sum << 1 | other);
        mine += other;
    }
    mine = phi_wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_flagged, (unsigned long long)mine);
}

// walk of entry e: walk_off[h] <= e < walk_off[h + 1]
__device__ __forceinline__ int32_t score_walk_of(const int64_t *__restrict__ walk_off, int32_t n_walks, int64_t e)
{
    int32_t lo = 0, hi = n_walks;
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (walk_off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) score_entry_kernel(const int32_t *__restrict__ ent_cls, const int2 *__restrict__ cls_tab,
                                                          const int32_t *__restrict__ cls_rec_off, const int32_t *__restrict__ rec_bh,
                                                          const int64_t *__restrict__ walk_off, int32_t n_walks, int64_t n_entries,
                                                          int32_t *__restrict__ S)
{
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x / 64);
    const int64_t gw = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t per = ((n_entries + n_waves - 1) / n_waves + 63) & ~(int64_t)63;
    const int64_t lo = gw * per, hi = lo + per < n_entries ? lo + per : n_entries;
    if (lo >= hi) return;
    // wave-uniform: the walk of the row's first entry and where it ends; the run carried over from the row before
    int32_t h = score_walk_of(walk_off, n_walks, lo);
    int64_t h_end = walk_off[h + 1];
    int32_t carry_key = -1, acc = 0;                          // the run carried along: its cell, and every lane's part of its sum
    for (int64_t e0 = lo; e0 < hi; e0 += 64) {
        const int64_t e = e0 + lane;
        int32_t key = -1, v = 0, hh = h;                      // key = the cell's index in S; -1: no entry
        if (e < hi) {
            if (e >= h_end) hh = score_walk_of(walk_off, n_walks, e);   // (the row crosses into later walks)
            const int32_t c = ent_cls[e];
            const int2 t = cls_tab[c];
            key = t.x < 0 ? -1 : t.x * n_walks + hh;
            v = t.y >> 1;
            if (t.y & 1) {
                // records outside the first block: one by one
                for (int32_t r = cls_rec_off[c], re = cls_rec_off[c + 1]; r < re; r++) {
                    const int32_t x = rec_bh[r];
                    if ((x & 1) && (x >> 1) != t.x) atomicAdd(&S[(int64_t)(x >> 1) * n_walks + hh], 1);
                }
            }
        }
        // A lane without a key of its own -- an entry whose class has no record, or no entry at all -- adds nothing: it takes
        // the key of the nearest lane before it that has one, else the carried run's, else the first one's behind it, so that
        // it does not break a row that is otherwise one cell
        const unsigned long long has = __ballot(key >= 0);
        if (has != ~0ull) {
            const unsigned long long before = has & ((1ull << lane) - 1);
            const int src = before ? 63 - __clzll((long long)before) : has ? __ffsll((long long)has) - 1 : 0;
            int32_t k = __shfl(key, src, 64);
            if (!before && carry_key >= 0) k = carry_key;
            if (key < 0) key = k;
        }
        const int32_t k0 = __shfl(key, 0, 64);
        if (__all(key == k0)) {
            // the whole row lies in one cell, as nearly every row of a long walk does: no shuffle, the lanes add up their own
            if (k0 != carry_key) {
                const int32_t tot = phi_wave_sum(acc);
                if (lane == 0 && tot) atomicAdd(&S[carry_key], tot);     // (tot != 0 only with a carried key >= 0)
                acc = 0; carry_key = k0;
            }
            acc += v;
        } else {
            const int32_t tot = phi_wave_sum(acc);
            if (lane == 0) {
                if (key == carry_key) v += tot;
                else if (tot) atomicAdd(&S[carry_key], tot);
            }
            // segmented inclusive scan: a lane whose left neighbour holds another key starts a run
            const int32_t left = __shfl_up(key, 1, 64);
            int head = lane == 0 || key != left;
            int32_t x = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int32_t y = __shfl_up(x, d, 64);
                const int f = __shfl_up(head, d, 64);
                if (lane >= d) {
                    if (!head) x += y;
                    head |= f;
                }
            }
            const int32_t right = __shfl_down(key, 1, 64);
            if (lane != 63 && key != right && x && key >= 0) atomicAdd(&S[key], x);
            carry_key = __shfl(key, 63, 64);
            const int32_t last = __shfl(x, 63, 64);
            acc = lane == 0 && carry_key >= 0 ? last : 0;
        }
        // the next row's first walk, when this row reached the end of its own: the last lane's, or the one behind it when that
        // walk ends with this row.  (Only then: a load of walk_off behind every row would put its latency between the rows)
        if (e0 + 64 >= h_end && e0 + 64 < hi) {
            h = __shfl(hh, 63, 64);
            h_end = walk_off[h + 1];
            if (h_end <= e0 + 64 && h + 1 < n_walks) { h++; h_end = walk_off[h + 1]; }
        }
    }
    const int32_t tot = phi_wave_sum(acc);
    if (lane == 0 && tot) atomicAdd(&S[carry_key], tot);
}

__global__ void __launch_bounds__(256) score_nonzero_kernel(const int32_t *__restrict__ S, int64_t n, unsigned long long *__restrict__ out)
{
    int mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) mine += S[i] != 0;
    mine = phi_wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(out, (unsigned long long)mine);
}

struct ScoreEvents {
    hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~ScoreEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

}  // namespace

extern "C" {

int phi_scout_scores(phi_ctx *c, int32_t n_blocks, int32_t *scores, phi_scout_info *info)
{
    if (!c) return PHI_ERR_INVALID;
    if (!c->have_graph || !c->scout.on) return phi_fail(c, PHI_ERR_STATE, "phi_scout_scores: the context holds no scout graph (phi_scout_graph)");
    const int32_t n_walks = c->n_walks, n_vtx = c->n_vtx;
    const int32_t nb = n_blocks > 0 ? n_blocks : (int32_t)std::min<int64_t>(SCORE_MAX_BLOCKS, std::max<int64_t>(1, ((int64_t)n_vtx + 1023) / 1024));
    if (nb > SCORE_MAX_BLOCKS) return phi_fail(c, PHI_ERR_INVALID, "phi_scout_scores: more than %d blocks", SCORE_MAX_BLOCKS);
    const int64_t n_cells = (int64_t)nb * n_walks;
    if (n_cells >= (int64_t)1 << 31) return phi_fail(c, PHI_ERR_INVALID, "phi_scout_scores: %d blocks x %d walks is 2^31 cells or more", nb, n_walks);
    HIPCHK(hipSetDevice(c->device));
    PHICHK(phi_sync_check(c));                                 // (the read batches so far have landed, their errors are reported as theirs)
    auto &X = c->scout;
    X.n_blocks = 0;
    const int64_t n_rec = c->n_rec, n_cls = c->n_cls, n_entries = c->n_entries;
    DevBuf d_rec_bh, d_cls_tab, d_cnt;
    PhiDevGuard guard{{&d_rec_bh, &d_cls_tab, &d_cnt}};
    PHICHK(phi_dev_ensure(c, d_rec_bh, (size_t)std::max<int64_t>(n_rec, 1) * 4));
    PHICHK(phi_dev_ensure(c, d_cls_tab, (size_t)std::max<int64_t>(n_cls, 1) * 8));
    PHICHK(phi_dev_ensure(c, d_cnt, 16));
    PHICHK(phi_dev_ensure(c, X.d_scores, (size_t)n_cells * 4));
    ScoreEvents ev;
    for (hipEvent_t &x : ev.e) HIPCHK(hipEventCreate(&x));
    HIPCHK(hipMemsetAsync(X.d_scores.p, 0, (size_t)n_cells * 4, c->stream));
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, 16, c->stream));
    unsigned long long *cnt = d_cnt.as<unsigned long long>();
    HIPCHK(hipEventRecord(ev.e[0], c->stream));
    if (n_rec > 0)
        hipLaunchKernelGGL(score_record_kernel, dim3(grid_for(n_rec, 256, 8192)), dim3(256), 0, c->stream, c->d_rec_e0.as<phi_ent_t>(), c->d_rec_slot.as<uint32_t>(),
                           n_rec, c->d_walk_vtx.as<int32_t>(), c->d_topo_rank.as<int32_t>(), c->d_u_uid.as<uint32_t>(), c->d_hit.as<uint8_t>(), n_vtx, nb,
                           d_rec_bh.as<int32_t>());
    HIPCHK(hipEventRecord(ev.e[1], c->stream));
    if (n_cls > 0)
        hipLaunchKernelGGL(score_class_kernel, dim3(grid_for(n_cls, 256, 8192)), dim3(256), 0, c->stream, c->d_cls_rec_off.as<int32_t>(), n_cls,
                           d_rec_bh.as<int32_t>(), d_cls_tab.as<int2>(), cnt);
    HIPCHK(hipEventRecord(ev.e[2], c->stream));
    // (at least 64 rows a wave, as phi_walk_sum_kernel, so that a wave's few atomics are spread over many rows; up to 4 096
    //  workgroups: a row is two dependent loads, and it is the number of resident waves that hides them)
    const unsigned entry_grid = grid_for(n_entries, 256 * 64, 4096);
    if (n_entries > 0)
        hipLaunchKernelGGL(score_entry_kernel, dim3(entry_grid), dim3(256), 0, c->stream, c->d_ent_cls.as<int32_t>(), d_cls_tab.as<int2>(),
                           c->d_cls_rec_off.as<int32_t>(), d_rec_bh.as<int32_t>(), c->d_walk_off.as<int64_t>(), n_walks, n_entries, X.d_scores.as<int32_t>());
    HIPCHK(hipEventRecord(ev.e[3], c->stream));
    hipLaunchKernelGGL(score_nonzero_kernel, dim3(grid_for(n_cells, 256, 1024)), dim3(256), 0, c->stream, X.d_scores.as<int32_t>(), n_cells, cnt + 1);
    // PHI_SCOUT_REF (profiles): phi_walk_sum_kernel<true> over the same entries in the same call, for scale
    const bool ref = getenv("PHI_SCOUT_REF") != nullptr;
    if (ref) {
        PHICHK(phi_dev_ensure(c, c->d_list2, (size_t)(n_walks + 1) * 8));
        HIPCHK(hipMemsetAsync(c->d_list2.p, 0, (size_t)(n_walks + 1) * 8, c->stream));
        HIPCHK(hipEventRecord(ev.e[4], c->stream));
        phi_launch_walk_rec_counts(c->stream, c->d_ent_cls.as<int32_t>(), c->d_cls_rec_off.as<int32_t>(), c->d_walk_off.as<int64_t>(), n_walks, n_entries,
                                   c->d_list2.as<unsigned long long>());
        HIPCHK(hipEventRecord(ev.e[5], c->stream));
    }
    HIPCHK(hipGetLastError());
    unsigned long long h_cnt[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h_cnt, cnt, 16, hipMemcpyDeviceToHost, c->stream));
    if (scores) HIPCHK(hipMemcpyAsync(scores, X.d_scores.p, (size_t)n_cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    X.n_blocks = nb;
    if (info) {
        memset(info, 0, sizeof *info);
        info->n_blocks = nb; info->n_walks = n_walks;
        info->n_classes_flagged = (int64_t)h_cnt[0]; info->n_nonzero = (int64_t)h_cnt[1];
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1])); info->record_gpu_ms = ms;
        HIPCHK(hipEventElapsedTime(&ms, ev.e[1], ev.e[2])); info->class_gpu_ms = ms;
        HIPCHK(hipEventElapsedTime(&ms, ev.e[2], ev.e[3])); info->entry_gpu_ms = ms;
        if (ref) { HIPCHK(hipEventElapsedTime(&ms, ev.e[4], ev.e[5])); info->walk_sum_gpu_ms = ms; }
    }
    return PHI_OK;
}

int phi_scout_choose(phi_ctx *c, const uint8_t *always, int32_t n_want, uint8_t *keep, int32_t *round_of)
{
    if (!c || !keep) return PHI_ERR_INVALID;
    if (!c->have_graph || !c->scout.on) return phi_fail(c, PHI_ERR_STATE, "phi_scout_choose: the context holds no scout graph (phi_scout_graph)");
    auto &X = c->scout;
    if (X.n_blocks <= 0) return phi_fail(c, PHI_ERR_STATE, "phi_scout_choose before phi_scout_scores on this scout graph");
    HIPCHK(hipSetDevice(c->device));
    const int32_t n_walks = c->n_walks;
    std::vector<int32_t> S((size_t)X.n_blocks * (size_t)n_walks);
    HIPCHK(phi_copy_sync(c, S.data(), X.d_scores.p, S.size() * 4, hipMemcpyDeviceToHost));
    if (phi_panel_choose_rule(S.data(), X.n_blocks, n_walks, always, n_want, keep, round_of, nullptr))
        return phi_fail(c, PHI_ERR_INVALID, "phi_scout_choose: n_want = %d must lie in 1 .. min(%d walks, %d) and hold the always-kept walks", n_want, n_walks,
                        PHI_PANEL_CHOOSE_MAX);
    return PHI_OK;
}

}  // extern "C"
