// dp_blocks.hip -- the event-driven DP over BLOCKS of steps: everything around the step kernels of dp_events.hip.
//   * where the chain over the compact steps may be cut (per solve): phi_cut_*, and phi_blk_ev, each walk's first event in a block
//   * more than 64 walks: the classes of walks per block, the max-plus chain over the blocks on class lanes (whole, or cut
//     into segments), the check that the two passes agree, the backtrack across blocks
// The blocks' rows and paths themselves (DP_ROW / DP_PATH) are step kernels: dp_events.hip.  DESIGN.md 5.2, 5.3.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <type_traits>
#include "phi_kernels.h"
#include "dp_dev.h"

// ------------------------------------------------------------------ where the chain may be cut (per solve)
// diff[e0 + 1] += 1, diff[e1 + 1] -= 1 for every dp anchor (first / last entry e0 < e1): the prefix sum at entry e
// is the number of anchors with e0 < e <= e1, i.e. that a cut right before e would split
__global__ void __launch_bounds__(256) phi_cut_cov_kernel(const phi_ent_t *__restrict__ a_e1, const uint8_t *__restrict__ a_span, int64_t n_a,
                                                          int32_t *__restrict__ diff)
{
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_a; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e1 = a_e1[g];
        const int32_t sp = a_span[g];
        if (sp <= 0) continue;
        atomicAdd(&diff[e1 - sp + 1], 1);
        atomicAdd(&diff[e1 + 1], -1);
    }
}
// clean[e] = 1 iff no anchor is split by a cut before entry e (cov_excl = exclusive prefix sums of diff)
__global__ void __launch_bounds__(256) phi_cut_clean_kernel(const int32_t *__restrict__ cov_excl, int64_t n_entries, int32_t *__restrict__ clean)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= n_entries; e += (int64_t)gridDim.x * blockDim.x)
        clean[e] = e < n_entries && cov_excl[e + 1] == 0;
}
// The same flags without counting: a cut before e is split by an anchor iff some anchor ending at x >= e has span > x - e,
// and spans are below PHI_RCAP, so x <= e + 30.  A block takes a tile of entries, looks through the anchors ending on the
// tile and the 30 entries behind it (the dp anchors are sorted by last entry: g_off is their CSR) and marks in LDS the
// entries each one covers; what is left unmarked is clean.  (The counting version -- two atomics per anchor into a difference
// array, a prefix sum over all entries, a pass for the flags -- took 36 ms at config 5; nothing else read the counts.)
#define CUT_TILE 4096
__global__ void __launch_bounds__(256) phi_cut_clean_direct_kernel(const int64_t *__restrict__ g_off, const uint8_t *__restrict__ g_span, int64_t n_entries,
                                                                   int32_t *__restrict__ clean)
{
    __shared__ uint8_t s_dirty[CUT_TILE];
    const int64_t n_tiles = (n_entries + 1 + CUT_TILE - 1) / CUT_TILE;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t e0 = t * CUT_TILE;
        for (int i = threadIdx.x; i < CUT_TILE / 4; i += 256) reinterpret_cast<uint32_t *>(s_dirty)[i] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < CUT_TILE + PHI_RCAP - 1; i += 256) {
            const int64_t x = e0 + i;
            if (x >= n_entries) break;
            const int64_t lo = g_off[x], hi = g_off[x + 1];
            int m = 0;
            for (int64_t g = lo; g < hi; g++) m = max(m, (int)g_span[g]);
            // the entries e with x - m < e <= x, inside the tile
            for (int64_t e = max(e0, x - m + 1); e <= x && e < e0 + CUT_TILE; e++) s_dirty[e - e0] = 1;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < CUT_TILE; i += 256) {
            const int64_t e = e0 + i;
            if (e <= n_entries) clean[e] = e < n_entries && !s_dirty[i];
        }
        __syncthreads();
    }
}
void phi_launch_cut_clean_direct(hipStream_t st, const int64_t *g_off, const uint8_t *g_span, int64_t n_entries, int32_t *clean)
{
    int64_t nb = (n_entries + 1 + CUT_TILE - 1) / CUT_TILE;
    if (nb > 16384) nb = 16384;
    hipLaunchKernelGGL(phi_cut_clean_direct_kernel, dim3((unsigned)nb), dim3(256), 0, st, g_off, g_span, n_entries, clean);
}

// Between two consecutive events of a walk (entries l < p on compact steps a < b) the walk only runs along chain
// vertices: a cut before any step in (a, b] is fine for this walk iff some entry in (l, p] is clean.  Where none is,
// the steps a+1 .. b are closed: stepdiff[a + 1] += 1, stepdiff[b + 1] -= 1.
__global__ void __launch_bounds__(256) phi_cut_events_kernel(const phi_ent_t *__restrict__ ev_e, int64_t n_ev, const int64_t *__restrict__ ev_off,
                                                             const int64_t *__restrict__ walk_off, int32_t n_walks,
                                                             const int32_t *__restrict__ walk_vtx, const int32_t *__restrict__ cvtx,
                                                             const int32_t *__restrict__ ncl_excl, int32_t *__restrict__ stepdiff)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ev; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = ev_e[i];
        const int lo = phi_walk_of_entry(walk_off, n_walks, p);
        if (i == ev_off[lo]) continue;                        // the walk's first event: nothing before it
        const int64_t l = ev_e[i - 1];
        if (ncl_excl[p + 1] - ncl_excl[l + 1] > 0) continue;   // a clean entry in (l, p]
        const int32_t a = cvtx[walk_vtx[l]], b = cvtx[walk_vtx[p]];
        atomicAdd(&stepdiff[a + 1], 1);
        atomicAdd(&stepdiff[b + 1], -1);
    }
}
// blk_ev[b][h] = first event of walk h on a compact step >= blk_lo[b]
__global__ void __launch_bounds__(256) phi_blk_ev_kernel(const int32_t *__restrict__ blk_lo, int32_t n_blk, const phi_ent_t *__restrict__ ev_e,
                                                         const int64_t *__restrict__ ev_off, int32_t n_walks, const int32_t *__restrict__ walk_vtx,
                                                         const int32_t *__restrict__ cvtx, int32_t *__restrict__ blk_ev)
{
    const int b = blockIdx.x, h = threadIdx.x;             // blockDim.x = the lane stride: 64 or 256
    if (b >= n_blk) return;
    int32_t out = 0;
    if (h < n_walks) {
        const int32_t k0 = blk_lo[b];
        int64_t lo = ev_off[h], hi = ev_off[h + 1];
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (cvtx[walk_vtx[ev_e[mid]]] < k0) lo = mid + 1; else hi = mid;
        }
        out = (int32_t)lo;
    }
    blk_ev[(int64_t)b * blockDim.x + h] = out;
}
void phi_launch_cut_cov(hipStream_t st, const phi_ent_t *a_e1, const uint8_t *a_span, int64_t n_a, int32_t *diff)
{
    if (n_a <= 0) return;
    int64_t nb = (n_a + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(phi_cut_cov_kernel, dim3((unsigned)nb), dim3(256), 0, st, a_e1, a_span, n_a, diff);
}
void phi_launch_cut_clean(hipStream_t st, const int32_t *cov_excl, int64_t n_entries, int32_t *clean)
{
    int64_t nb = (n_entries + 1 + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(phi_cut_clean_kernel, dim3((unsigned)nb), dim3(256), 0, st, cov_excl, n_entries, clean);
}
void phi_launch_cut_events(hipStream_t st, const phi_ent_t *ev_e, int64_t n_ev, const int64_t *ev_off, const int64_t *walk_off, int32_t n_walks,
                           const int32_t *walk_vtx, const int32_t *cvtx, const int32_t *ncl_excl, int32_t *stepdiff)
{
    if (n_ev <= 0) return;
    int64_t nb = (n_ev + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(phi_cut_events_kernel, dim3((unsigned)nb), dim3(256), 0, st, ev_e, n_ev, ev_off, walk_off, n_walks, walk_vtx, cvtx,
                       ncl_excl, stepdiff);
}
void phi_launch_blk_ev(hipStream_t st, const int32_t *blk_lo, int32_t n_blk, const phi_ent_t *ev_e, const int64_t *ev_off, int32_t n_walks,
                       const int32_t *walk_vtx, const int32_t *cvtx, int32_t *blk_ev)
{
    if (n_blk > 0)
        hipLaunchKernelGGL(phi_blk_ev_kernel, dim3((unsigned)n_blk), dim3(n_walks <= 64 ? 64 : 256), 0, st, blk_lo, n_blk, ev_e, ev_off, n_walks,
                           walk_vtx, cvtx, blk_ev);
}


// ------------------------------------------------------------------ more than 64 walks: blocks on CLASS LANES
// Inside a short block of steps most walks do the same thing: they run through the same vertices over the same
// anchors (haplotypes that share the alleles of the block's few sites).  What a block does to a walk is a function of
// the walk's event records inside it -- steps, entry distances, anchor counts relative to the walk's count at the
// block's first event, out-edges -- so walks whose records agree form a CLASS, and the block's transfer matrix is
// needed per class, not per walk: <= 64 class lanes run on the one-wave consumer kernel (DP_ROW), whatever the number
// of walks.  A block with more than 64 classes raises PHI_KERR_DP_CLASSES (the caller keeps the whole chain).
//
// Per run and block: sig(walk) = 128-bit hash of (begun before the block, events left, and per event inside the
// block: step - k0, entry - first entry, walk start / walk end, End - c, SB - c, the window counts G[a] for
// a <= entry - first entry (older windows reach before the cut and are never read for a run that began inside),
// the out-edge).  With c = SB at a walk's first event of the block, walks j, r of one class have
// End_j - End_r = SB_j - SB_r = c_j - c_r throughout the block; d_j = c_j - c_r(class of j) is the walk's OFFSET
// from the walk r that plays its class lane.
__device__ __forceinline__ unsigned long long cls_mix(unsigned long long h, unsigned long long x, unsigned long long m)
{
    h = (h ^ x) * m;
    return h ^ (h >> 29);
}
__global__ void __launch_bounds__(256) phi_blk_classes_kernel(PhiBlkClassArgs G)
{
    __shared__ unsigned long long s_a[256], s_b[256];
    __shared__ int32_t s_idx[256], s_c0[256];
    __shared__ int32_t s_wcnt[4];
    const int b = blockIdx.x, h = threadIdx.x, lane = h & 63, wid = h >> 6;
    const int32_t LS = G.lane_stride;
    const bool has_walk = h < G.n_walks;
    unsigned long long ha = 0x243F6A8885A308D3ull, hb = 0x13198A2E03707344ull;
    int32_t c0 = 0;
    if (has_walk) {
        const uint4 *evg = reinterpret_cast<const uint4 *>(G.ev);
        const int32_t k0 = G.blk_lo[b];
        const int64_t v0 = G.ev_off[h], ve = G.ev_off[h + 1];
        const int64_t vb = G.blk_ev[(int64_t)b * LS + h];
        const int64_t vend = b + 1 < G.n_blk ? (int64_t)G.blk_ev[(int64_t)(b + 1) * LS + h] : ve;
        const int64_t eb = G.walk_off[h], ee = G.walk_off[h + 1];
        const unsigned long long head = (vb > v0 ? 1u : 0u) | (vb < ve ? 2u : 0u);
        ha = cls_mix(ha, head, 0x9E3779B97F4A7C15ull); hb = cls_mix(hb, head, 0xC2B2AE3D27D4EB4Full);
        int64_t e_first = 0;
        for (int64_t i = vb; i < vend; i++) {
            const uint4 A = evg[i * 3 + 0], B = evg[i * 3 + 1], C = evg[i * 3 + 2];
            const int64_t e = (int64_t)A.y;
            if (i == vb) { e_first = e; c0 = (int32_t)A.w; }
            const int64_t rel = e - e_first;
            unsigned long long w[4] = {(unsigned long long)B.x | ((unsigned long long)B.y << 32), (unsigned long long)B.z | ((unsigned long long)B.w << 32),
                                       (unsigned long long)C.x | ((unsigned long long)C.y << 32), (unsigned long long)C.z | ((unsigned long long)C.w << 32)};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int64_t keep = rel + 1 - 8 * q;              // bytes 8q .. 8q+7 hold the counts of ages 8q .. 8q+7
                unsigned long long m = keep >= 8 ? ~0ull : keep <= 0 ? 0ull : ((1ull << (8 * keep)) - 1);
                if (q == 3) m |= 0xFF00000000000000ull;            // byte 31: the out-edge
                w[q] &= m;
            }
            const unsigned long long f0 = ((unsigned long long)(uint32_t)((int32_t)(A.x & 0x7FFFFFFFu) - k0) << 32) | (unsigned long long)(uint32_t)rel;
            const unsigned long long f1 = ((unsigned long long)(uint32_t)((int32_t)A.z - c0) << 32) | (unsigned long long)(uint32_t)((int32_t)A.w - c0);
            unsigned long long f2 = (e == eb ? 1u : 0u) | (e == ee - 1 ? 2u : 0u);
            if (A.x >> 31) f2 |= 4u | ((unsigned long long)(h + 1) << 8);   // counted from the walk's own anchors: a class of its own
            const unsigned long long f[7] = {f0, f1, f2, w[0], w[1], w[2], w[3]};
#pragma unroll
            for (int q = 0; q < 7; q++) { ha = cls_mix(ha, f[q], 0x9E3779B97F4A7C15ull); hb = cls_mix(hb, f[q], 0xC2B2AE3D27D4EB4Full); }
        }
    }
    s_a[h] = ha; s_b[h] = hb; s_c0[h] = c0;
    if (h < 64) G.lane_walk[(int64_t)b * 64 + h] = -1;
    __syncthreads();
    // the class of a walk is led by the first walk with its signature
    int32_t leader = h;
    if (has_walk)
        for (int j = 0; j < h; j++)
            if (s_a[j] == ha && s_b[j] == hb) { leader = j; break; }
    const bool is_leader = has_walk && leader == h;
    const unsigned long long bal = __ballot(is_leader);
    if (lane == 0) s_wcnt[wid] = __popcll(bal);
    __syncthreads();
    int32_t before = __popcll(bal & ((1ull << lane) - 1));
    for (int x = 0; x < wid; x++) before += s_wcnt[x];
    const int32_t total = s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
    s_idx[h] = before;
    __syncthreads();
    if (h == 0) {
        G.blk_ncls[b] = total < 64 ? total : 64;
        if (total > 64) atomicOr(G.err, PHI_KERR_DP_CLASSES);
    }
    if (has_walk) {
        const int32_t idx = s_idx[leader];
        if (is_leader && idx < 64) G.lane_walk[(int64_t)b * 64 + idx] = h;
        G.walk_lane[(int64_t)b * LS + h] = idx < 64 ? idx : 0;
        G.coff[(int64_t)b * LS + h] = c0 - s_c0[leader];       // relative to the walk that plays the class lane

    }
}

// The chain over the blocks, on class lanes: S_{b+1}[x] for every walk x from S_b and the block's class rows.
// With l(x) the class lane of walk x in block b and d the offsets (keys of walk x are keys of its lane minus d[x]):
//   own run, and runs begun on x's lane by it       S[x] + row[l(x)][l(x)]
//   another walk j of x's class                     S[j] + d[j] + rownew[l(x)] - d[x]
//   a walk j of another class C                     S[j] + d[j] + row[C][l(x)] - d[x]
//   a walk that starts inside the block             row[64][l(x)] - d[x]
// Only the best S[j] + d[j] of a class matters (and, for the walks that reach it, whether another walk does too or
// else the second best).  One workgroup, one block per iteration, two barriers; thread (wave w, lane l) holds, in
// registers, column l of the rows of classes C = w, w + 4, ..: the "another class" term is a function of the class
// lane alone, so the four waves split the classes and leave four partial maxima per lane in LDS.  Rows and tables
// of block b + DEPTH are on their way while block b is chained.  All sums stay far inside int32: keys and offsets are
// bounded by the anchors of one walk (< 2^27, phi_solve.hip).
//
// The chain is a sequence of max-plus AFFINE maps of the walks' keys (S' = M_b (x) S (+) T_b: every term above is a maximum of
// sums, T_b the walk starts inside the block), so it can be cut: MODE 1 runs the blocks of one SEGMENT from a unit vector
// ("key 0 on walk u", walk starts switched off: column u of the segment's matrix) or from no key at all with the starts on
// (its constant term) -- segments x (walks + 1) independent workgroups --, phi_seg_chain_kernel chains the segments'
// matrices (one workgroup, segments x walks rows), and MODE 2 replays every segment from its true entry keys, in
// parallel, writing what MODE 0 (the whole chain by one workgroup) writes.  C5: 94 671 blocks in 64 segments.
// U: unit vectors one workgroup of MODE 1 carries through its segment AT ONCE.  The blocks' rows are the same for every unit
// vector of a segment (24 MB per segment at C5, read by 201 workgroups: 316 GB through the L2s per DP run), and what a
// workgroup spends per block is latency -- two barriers, LDS atomics, dependent reads --, not arithmetic: with U chains
// interleaved in one instruction stream a block's rows are loaded once for U of them and the barriers are shared.
template <int MODE, int U = 1>
__global__ void __launch_bounds__(256) phi_blk_chain_kernel(PhiBlkClassArgs G, const int32_t *__restrict__ rows, const int32_t *__restrict__ rownew,
                                                            const int32_t *__restrict__ rowdiag, int32_t *__restrict__ blk_S,
                                                            const int32_t *__restrict__ seg_lo, int32_t *__restrict__ seg_row,
                                                            const int32_t *__restrict__ seg_S)
{
    static_assert(MODE == 1 || U == 1, "several unit vectors at once: the segments' matrices only");
    constexpr int NR = 65 * 64;
    constexpr int DEPTH = 4;
    // "no value" is NEGK everywhere: NEGK + a key (|key| < 2^27) and NEGK + NEGK stay below NEGK / 2 and inside int32, so a
    // maximum of sums needs no test of its operands (the loop is the longest dependent chain of an iteration: one
    // workgroup walks 10^5 blocks, 1.1 us each, and what it costs is its instruction count -- C5: 112 ms per DP run)
    constexpr int32_t NONE = NEGK;
    __shared__ int32_t s_b1[2][U][64], s_b2[2][U][64], s_n1[2][U][64];  // per class: best S + d, second best, walks that reach the best
    __shared__ int32_t s_diag[2][64], s_start[2][64], s_new[2][64];
    __shared__ int32_t s_part[2][U][4][64];
    const int x = threadIdx.x, lane = x & 63, wid = __builtin_amdgcn_readfirstlane(x >> 6);
    const int32_t LS = G.lane_stride;
    const bool has_walk = x < G.n_walks;
    // the blocks this workgroup chains, the keys it starts from, whether walks may start inside
    const int32_t groups = MODE == 1 ? (G.n_walks + 1 + U - 1) / U : 1;
    const int32_t seg = MODE == 0 ? 0 : MODE == 1 ? (int32_t)blockIdx.x / groups : (int32_t)blockIdx.x;
    const int32_t unit0 = MODE == 1 ? ((int32_t)blockIdx.x % groups) * U : -1;
    const int32_t b_lo = MODE == 0 ? 0 : seg_lo[seg], nb = MODE == 0 ? G.n_blk : seg_lo[seg + 1];
    int32_t S[U];
    bool with_starts[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        with_starts[u] = MODE != 1 || unit0 + u == G.n_walks;           // (units past the last one carry nothing: all keys stay NEGK)
        S[u] = NEGK;
        if (MODE == 1 && x == unit0 + u) S[u] = 0;
        if (MODE == 2 && has_walk) S[u] = seg_S[(int64_t)seg * LS + x];
    }
    int32_t st_row[DEPTH][16], st_x[DEPTH], st_lx[DEPTH], st_dx[DEPTH];
    const int32_t *p_row = rows + wid * 64 + lane;   // + b * NR + 256 * i
    const int32_t *p_x = wid == 0 ? rows + 64 * 64 + lane : wid == 1 ? rownew + lane : rowdiag + lane;   // + b * (NR | 65 | 64): walk starts (wave 0), new-run keys (wave 1), the rows' own columns (wave 2)
    const int32_t x_stride = wid == 0 ? NR : wid == 1 ? 65 : 64;
    const int32_t xs = has_walk ? x : 0;
    auto issue = [&](auto J, int32_t b) {
        constexpr int j = decltype(J)::value;
        const int32_t *src = p_row + (int64_t)b * NR;
#pragma unroll
        for (int i = 0; i < 16; i++) st_row[j][i] = src[256 * i];
        st_x[j] = wid < 3 ? p_x[(int64_t)b * x_stride] : NEGK;
        st_lx[j] = G.walk_lane[(int64_t)b * LS + xs];
        st_dx[j] = G.coff[(int64_t)b * LS + xs];
    };
    auto step = [&](auto J, int32_t b) {
        constexpr int j = decltype(J)::value;
        const int p = b & 1;
        const int32_t lx = st_lx[j], dx = st_dx[j];
        if (wid == 0) s_start[p][lane] = st_x[j];                         // (lanes past the block's classes are never read)
        if (wid == 1) s_new[p][lane] = st_x[j];
        if (wid == 2) s_diag[p][lane] = st_x[j];
        if (MODE != 1 && has_walk) blk_S[(int64_t)b * LS + x] = S[0];
        bool live[U];
        int32_t v[U], b1[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            live[u] = has_walk && S[u] > NEGK / 2;
            v[u] = S[u] + dx;
            if (live[u]) atomicMax(&s_b1[p][u][lx], v[u]);               // (reset in the previous iteration, a barrier ago)
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < U; u++) {
            b1[u] = s_b1[p][u][lx];
            if (live[u]) { if (v[u] == b1[u]) atomicAdd(&s_n1[p][u][lx], 1); else atomicMax(&s_b2[p][u][lx], v[u]); }
        }
        if (x < 64) {
#pragma unroll
            for (int u = 0; u < U; u++) { s_b1[p ^ 1][u][x] = NONE; s_b2[p ^ 1][u][x] = NONE; s_n1[p ^ 1][u][x] = 0; }   // for the next iteration (last read before this iteration's first barrier)
        }
        // partial maxima over this wave's classes, for class lane `lane`
        // (branch-free: the sixteen LDS reads go out together.  Classes past the block's count have no live walk: their
        //  maximum is NONE, and NONE plus whatever lies in their rows -- keys of an earlier solve at most -- stays "no
        //  value"; the row's own column holds NEGK, see the row pass)
#pragma unroll
        for (int u = 0; u < U; u++) {
            int32_t part = NONE;
            int32_t o16[16];
#pragma unroll
            for (int i = 0; i < 16; i++) o16[i] = s_b1[p][u][wid + 4 * i];
#pragma unroll
            for (int i = 0; i < 16; i++) part = max(part, o16[i] + st_row[j][i]);
            s_part[p][u][wid][lane] = part;
        }
        issue(J, min(b + DEPTH, nb - 1));                      // (always: the compiler can then count the loads in flight instead of draining them)
        __syncthreads();
#pragma unroll
        for (int u = 0; u < U; u++) {
            int32_t best = NEGK;
            if (has_walk) {
                if (live[u]) { const int32_t r = s_diag[p][lx]; if (r > NEGK / 2) best = S[u] + r; }
                {
                    // the best of the other walks of the class
                    const int32_t o = (live[u] && v[u] == b1[u] && s_n1[p][u][lx] == 1) ? s_b2[p][u][lx] : b1[u];
                    const int32_t kn = s_new[p][lx];
                    if (o > NEGK / 2 && kn > NEGK / 2 && o + kn - dx > best) best = o + kn - dx;
                }
                const int32_t d = max(max(s_part[p][u][0][lx], s_part[p][u][1][lx]), max(s_part[p][u][2][lx], s_part[p][u][3][lx]));
                if (d > NEGK / 2 && d - dx > best) best = d - dx;
                if (with_starts[u]) { const int32_t r = s_start[p][lx]; if (r > NEGK / 2 && r - dx > best) best = r - dx; }
            }
            S[u] = best > NEGK / 2 ? best : NEGK;
        }
        // (no barrier here: the next iteration writes the other parity only, and what it reads of it was settled
        //  before this iteration's second barrier)
    };
    if (x < 64) {
#pragma unroll
        for (int u = 0; u < U; u++) { s_b1[b_lo & 1][u][x] = NONE; s_b2[b_lo & 1][u][x] = NONE; s_n1[b_lo & 1][u][x] = 0; }
    }
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
    issue(I0{}, min(b_lo, nb - 1));
    issue(I1{}, min(b_lo + 1, nb - 1));
    issue(I2{}, min(b_lo + 2, nb - 1));
    issue(I3{}, min(b_lo + 3, nb - 1));
    __syncthreads();
    int32_t b = b_lo;
    for (; b + DEPTH <= nb; b += DEPTH) {
        step(I0{}, b);
        step(I1{}, b + 1);
        step(I2{}, b + 2);
        step(I3{}, b + 3);
    }
    if (b < nb) step(I0{}, b);
    if (b + 1 < nb) step(I1{}, b + 1);
    if (b + 2 < nb) step(I2{}, b + 2);
    if (MODE == 1 && has_walk) {
#pragma unroll
        for (int u = 0; u < U; u++)
            if (unit0 + u <= G.n_walks) seg_row[((int64_t)seg * (G.n_walks + 1) + unit0 + u) * LS + x] = S[u];      // what leaves the segment
    }
}

// The segments' matrices chained: seg_S[g] = the keys entering segment g.  seg_row[(g * (walks + 1) + u) * LS + x] = the key
// leaving segment g on walk x when key 0 entered on walk u (u = walks: when nothing entered -- the walk starts inside).
__global__ void __launch_bounds__(256) phi_seg_chain_kernel(int32_t n_seg, int32_t n_walks, int32_t LS, const int32_t *__restrict__ seg_row,
                                                            int32_t *__restrict__ seg_S)
{
    __shared__ int32_t s_S[256];
    const int x = threadIdx.x;
    int32_t S = NEGK;
    for (int32_t g = 0; g < n_seg; g++) {
        seg_S[(int64_t)g * LS + x] = S;
        s_S[x] = S;
        __syncthreads();
        const int32_t *R = seg_row + (int64_t)g * (n_walks + 1) * LS + x;
        int32_t best = R[(int64_t)n_walks * LS];
#pragma unroll 8
        for (int32_t u = 0; u < n_walks; u++) best = max(best, s_S[u] + R[(int64_t)u * LS]);   // (NEGK + anything stays "no value")
        S = best > NEGK / 2 ? best : NEGK;
        __syncthreads();
    }
}

// the two passes must agree on what leaves every block: keys_out[b] (DP_PATH) against S[b + 1] (the chain)
__global__ void __launch_bounds__(256) phi_blk_check_kernel(const int32_t *__restrict__ keys, const int32_t *__restrict__ S, int32_t n_blk,
                                                            int32_t LS, int32_t n_walks, int32_t *__restrict__ bad)
{
    const int64_t n = (int64_t)(n_blk - 1) * LS;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t h = (int32_t)(i % LS);
        if (h >= n_walks) continue;
        const int32_t got = keys[i], want = S[i + LS];
        // (a walk that begins inside the next block or ended before it carries nothing that is ever read)
        if (got != want && !(got <= NEGK / 2 && want <= NEGK / 2)) { atomicAdd(&bad[0], 1); atomicMin(&bad[1], (int32_t)(i / LS)); }
    }
}

// backtrack across blocks: the last block before b_from in which the run carried on walk h began -> out = {block, start}
__global__ void __launch_bounds__(256) phi_carry_resolve_kernel(const int32_t *__restrict__ carry, int32_t LS, int32_t b_from, int32_t h,
                                                                int32_t *__restrict__ out)
{
    __shared__ int32_t s_best;
    for (int32_t hi = b_from - 1; hi >= 0; hi -= 256) {
        if (threadIdx.x == 0) s_best = -1;
        __syncthreads();
        const int32_t b = hi - (int32_t)threadIdx.x;
        const int32_t v = b >= 0 ? carry[(int64_t)b * LS + h] : -1;
        if (v >= 0) atomicMax(&s_best, b);
        __syncthreads();
        const int32_t bb = s_best;
        if (bb >= 0) {
            if (b == bb) { out[0] = bb; out[1] = v; }
            return;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = -1; out[1] = -1; }
}

void phi_launch_blk_classes(hipStream_t st, const PhiBlkClassArgs &G)
{
    if (G.n_blk > 0) hipLaunchKernelGGL(phi_blk_classes_kernel, dim3((unsigned)G.n_blk), dim3(256), 0, st, G);
}
void phi_launch_blk_chain(hipStream_t st, const PhiBlkClassArgs &G, const int32_t *rows, const int32_t *rownew, const int32_t *rowdiag, int32_t *blk_S)
{
    hipLaunchKernelGGL(phi_blk_chain_kernel<0>, dim3(1), dim3(256), 0, st, G, rows, rownew, rowdiag, blk_S, nullptr, nullptr, nullptr);
}
// the same chain cut into n_seg segments (d_seg_lo[n_seg + 1]: first block of each): unit rows, segment chain, replay
void phi_launch_blk_chain_segments(hipStream_t st, const PhiBlkClassArgs &G, const int32_t *rows, const int32_t *rownew, const int32_t *rowdiag, int32_t *blk_S,
                                   int32_t n_seg, const int32_t *d_seg_lo, int32_t *seg_row, int32_t *seg_S)
{
    const int units = getenv("PHI_DP_CHAIN_UNITS") ? atoi(getenv("PHI_DP_CHAIN_UNITS")) : 3;      // unit vectors per workgroup (tests: 1, 2)
    const unsigned nu = (unsigned)(G.n_walks + 1);
    if (units >= 4) hipLaunchKernelGGL((phi_blk_chain_kernel<1, 4>), dim3((unsigned)n_seg * ((nu + 3) / 4)), dim3(256), 0, st, G, rows, rownew, rowdiag, blk_S, d_seg_lo, seg_row, seg_S);
    else if (units == 3) hipLaunchKernelGGL((phi_blk_chain_kernel<1, 3>), dim3((unsigned)n_seg * ((nu + 2) / 3)), dim3(256), 0, st, G, rows, rownew, rowdiag, blk_S, d_seg_lo, seg_row, seg_S);
    else if (units == 2) hipLaunchKernelGGL((phi_blk_chain_kernel<1, 2>), dim3((unsigned)n_seg * ((nu + 1) / 2)), dim3(256), 0, st, G, rows, rownew, rowdiag, blk_S, d_seg_lo, seg_row, seg_S);
    else hipLaunchKernelGGL((phi_blk_chain_kernel<1, 1>), dim3((unsigned)n_seg * nu), dim3(256), 0, st, G, rows, rownew, rowdiag, blk_S, d_seg_lo, seg_row, seg_S);
    hipLaunchKernelGGL(phi_seg_chain_kernel, dim3(1), dim3(256), 0, st, n_seg, G.n_walks, G.lane_stride, seg_row, seg_S);
    hipLaunchKernelGGL(phi_blk_chain_kernel<2>, dim3((unsigned)n_seg), dim3(256), 0, st, G, rows, rownew, rowdiag, blk_S, d_seg_lo, seg_row, seg_S);
}
void phi_launch_blk_check(hipStream_t st, const int32_t *keys, const int32_t *S, int32_t n_blk, int32_t LS, int32_t n_walks, int32_t *bad)
{
    int64_t nb = ((int64_t)(n_blk - 1) * LS + 255) / 256;
    if (nb < 1) nb = 1;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(phi_blk_check_kernel, dim3((unsigned)nb), dim3(256), 0, st, keys, S, n_blk, LS, n_walks, bad);
}
void phi_launch_carry_resolve(hipStream_t st, const int32_t *carry, int32_t LS, int32_t b_from, int32_t h, int32_t *out)
{
    hipLaunchKernelGGL(phi_carry_resolve_kernel, dim3(1), dim3(256), 0, st, carry, LS, b_from, h, out);
}

// loads this translation unit's code object (see phi_warm_dp of dp.hip)
__global__ void phi_warm_dp_blocks_kernel() {}
void phi_warm_dp_blocks(hipStream_t st) { hipLaunchKernelGGL(phi_warm_dp_blocks_kernel, dim3(1), dim3(64), 0, st); }
