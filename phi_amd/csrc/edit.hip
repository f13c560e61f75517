// edit.hip -- unit-cost global (NW) edit distance of byte strings: what the reference's evaluation computes with edlib
// (data/edlib_edits.py:24-27, data/postprocessing_2_MIQP.py:21-42, data/get_edit_stats.sh) between an inferred haplotype
// and a ground truth, both a whole MHC (~5 Mbp).
//
// Algorithm: Myers' bit-vector in Hyyro's block form with Ukkonen's band, doubled until the distance is proven (edlib's).
//   - The shorter sequence Q gives the rows, the longer T the columns (the distance is symmetric).  Rows go in 64-row
//     blocks; a block's column is the vertical deltas of its 64 cells as two bit vectors (Pv, Mv) and the value of its
//     bottom cell.
//   - Threshold k: a path of cost <= k stays on diagonals j - i in [-e, delta + e], delta = n - m, e = (k - delta) / 2.
//     Block b works on the columns where one of its rows meets that band, [lo(b), hi(b)]; a block entering the band starts
//     from vertical deltas +1 below the cell above it, the row above a block that left the band grows by +1 per column.
//     Every value computed that way is an upper bound of the true one and exact on any path that stays in the band, so a
//     result <= k is the distance and a result > k proves distance > k: the host doubles k and runs the pair again.
//   - One workgroup per pair.  A STRIPE is up to `lanes` consecutive blocks, one block per lane; lanes run as a diagonal
//     wavefront (lane g works on column t - g at step t), the horizontal delta and the bottom value of a block go one
//     lane down through a DPP shift inside a wave and through LDS between waves, one barrier per step.  Waves with no lane
//     in the band skip the update.  The stripe's bottom row leaves its horizontal deltas in HBM (2 bits per column) and
//     the next stripe's first lane reads them back as its top input.
//   - After each stripe the bottom row bounds the distance from below: every path crosses it, at some column c, at a cost
//     of at least D(row, c) + |(n - c) - (m - row)|.  When every such bound exceeds k the pass stops there.
//   - Peq (which rows of a block hold a given byte) is built per stripe from Q in HBM into LDS, [code][lane]; bytes are
//     mapped to dense codes (the bytes of Q, one more code for every byte Q lacks), so the comparison is exact on bytes.
//   - No workgroup waits on another; inside the workgroup every wait is a barrier.
#include <algorithm>
#include <string.h>
#include <vector>
#include "phi_ctx.h"

#define HIPCHK(call) do { int rc_ = phi_hip_check(c, (call), #call); if (rc_) return rc_; } while (0)
#define PHICHK(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

#define ED_MAX_LANES 1024               // lanes (= blocks of a stripe) of the largest workgroup
#define ED_PEQ_WORDS (16 * 1024)        // 128 KB of Peq: codes x lanes <= 16 K (DNA: 5-6 codes x 1 024 lanes)
#define ED_RING 2048                    // columns of T staged in LDS (a stripe spans at most 1 024 + 1)
#define ED_CHUNK 256                    // columns staged per refill, two chunks ahead
#define ED_EXCEEDED (-2)                // the pass proved distance > k

namespace {

struct EdPair {
    int64_t q_off, t_off;   // Q (rows, the shorter) and T (columns) in the device copy of the input
    int64_t m, n;           // |Q| >= 1, |T| >= m
    int64_t k;              // threshold of this pass
    int64_t words_off;      // this pair's 2-bit row of deltas (n / 16 + 2 words)
};

__device__ __forceinline__ uint32_t shift_down_one_lane(uint32_t v)
{
    // lane l gets lane l - 1's value (wave_shr:1); lane 0 keeps its own, replaced by the caller
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false);
}

__global__ void __launch_bounds__(ED_MAX_LANES) phi_edit_band_kernel(const uint8_t *__restrict__ seq, const EdPair *__restrict__ pairs,
                                                                     uint32_t *__restrict__ words_all, int64_t *__restrict__ out)
{
    __shared__ uint64_t peq[ED_PEQ_WORDS];
    __shared__ uint8_t ring[ED_RING];               // code of T[c - 1] at ring[c % ED_RING]
    __shared__ uint32_t dring[ED_RING / 16];        // 2-bit deltas of the row above the stripe, same columns
    __shared__ uint8_t code_of[256];
    __shared__ uint32_t present[256];
    __shared__ uint32_t carry[2][ED_MAX_LANES / 64][2];  // (hout + 1, bottom value) of each wave's last lane, by step parity
    __shared__ int64_t s_prev[3];                   // row above the stripe: first and last column written, value before the first
    __shared__ int64_t s_res[2];                    // lower bound of the stripe's bottom row; the distance (last stripe)
    __shared__ int32_t s_alpha, s_absent;

    const EdPair P = pairs[blockIdx.x];
    const uint8_t *Q = seq + P.q_off, *T = seq + P.t_off;
    uint32_t *words = words_all + P.words_off;
    const int64_t m = P.m, n = P.n, k = P.k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x;

    // ---- alphabet: the bytes of Q get codes 0.., every other byte the code after them (its Peq rows are all zero)
    for (int i = tid; i < 256; i += nthr) present[i] = 0;
    __syncthreads();
    for (int64_t i = tid; i < m; i += nthr) present[Q[i]] = 1;
    __syncthreads();
    if (tid == 0) {
        int a = 0;
        for (int x = 0; x < 256; x++) if (present[x]) code_of[x] = (uint8_t)a++;
        const int absent = a < 256 ? a : 0;
        for (int x = 0; x < 256; x++) if (!present[x]) code_of[x] = (uint8_t)absent;
        s_alpha = a < 256 ? a + 1 : 256;
        s_absent = absent;
        s_prev[0] = 1; s_prev[1] = 0; s_prev[2] = 0;     // row 0: D(0, c) = c, every delta +1
        s_res[1] = -1;
    }
    __syncthreads();
    const int alpha = s_alpha;
    const int lanes = min(nthr, (ED_PEQ_WORDS / alpha) & ~63);     // >= 64: alpha <= 256
    const uint8_t absent_code = (uint8_t)s_absent;

    const int64_t delta = n - m;
    const int64_t e = max((int64_t)1, (k - delta) / 2);
    const int64_t dmin = -e, dmax = delta + e;
    const int64_t nb = (m + 63) / 64;
    int64_t dist = -1;

    for (int64_t b0 = 0; b0 < nb; b0 += lanes) {
        const int h = (int)min((int64_t)lanes, nb - b0);
        const bool has_block = tid < h;
        const int64_t b = b0 + tid;
        const int64_t lo = max((int64_t)1, 64 * b + 1 + dmin);
        const int64_t hi = min(n, 64 * b + 64 + dmax);
        const int64_t key = lo + tid;                  // lane works on column t - tid: in the band while 0 <= t - key <= hi - lo
        const uint64_t span = has_block ? (uint64_t)(hi - lo) : 0;
        const bool bottom = tid == h - 1;
        const bool last_stripe = b0 + h == nb;

        // Peq of this lane's block, rows beyond m never match
        if (has_block) {
            for (int a = 0; a < alpha; a++) peq[a * lanes + tid] = 0;
            for (int i = 0; i < 64; i++) {
                const int64_t row = 64 * b + i;
                if (row < m) peq[code_of[Q[row]] * lanes + tid] |= 1ull << i;
            }
        }
        const int64_t prev_first = s_prev[0], prev_last = s_prev[1];
        // value of the row above at column lo(b0) - 1, from the value before prev_first and the deltas up to there
        uint32_t above_run = 0;
        if (tid == 0) {
            int64_t v = s_prev[2];
            for (int64_t col = prev_first; col < lo; col++)
                v += col <= prev_last ? (int64_t)((words[col >> 4] >> (2 * (col & 15))) & 3) - 1 : 1;
            above_run = (uint32_t)v;
        }
        const int64_t t_begin = min(n, max((int64_t)1, 64 * b0 + 1 + dmin));
        const int64_t t_end = min(n, 64 * (b0 + h - 1) + 64 + dmax) + h - 1;
        const int64_t chunk0 = t_begin & ~(int64_t)(ED_CHUNK - 1);

        auto stage = [&](int64_t first) {            // columns [first, first + ED_CHUNK) into the rings (wave 0)
            for (int j = lane; j < ED_CHUNK; j += 64) {
                const int64_t col = first + j;
                ring[col & (ED_RING - 1)] = col >= 1 && col <= n ? code_of[T[col - 1]] : absent_code;
            }
            if (lane < ED_CHUNK / 16) {
                const int64_t w = (first >> 4) + lane;
                dring[w & (ED_RING / 16 - 1)] = w <= (prev_last >> 4) ? words[w] : 0u;
            }
        };
        if (wave == 0) { stage(chunk0); stage(chunk0 + ED_CHUNK); }
        __syncthreads();

        uint64_t Pv = ~0ull, Mv = 0;
        uint32_t score = 0, hout_u = 2, acc = 0;         // hout_u = hout + 1
        int64_t lb = INT64_MAX, base = 0;
        if (bottom && lo == 1) lb = 64 * b + 64 + llabs(delta + 64 * b + 64);   // the path may cross the bottom row at column 0

        for (int64_t t = t_begin; t <= t_end; t++) {
            if (wave == 0 && (t & (ED_CHUNK - 1)) == 0 && t > chunk0) stage(t + ED_CHUNK);
            uint32_t hin_u = shift_down_one_lane(hout_u), above = shift_down_one_lane(score);
            if (lane == 0) {
                if (wave == 0) {
                    hin_u = t <= prev_last ? (dring[(t >> 4) & (ED_RING / 16 - 1)] >> (2 * (t & 15))) & 3 : 2;
                    above_run += hin_u - 1;
                    above = above_run;
                } else {
                    hin_u = carry[(t - 1) & 1][wave - 1][0];
                    above = carry[(t - 1) & 1][wave - 1][1];
                }
            }
            const int64_t col = t - tid;
            const bool active = (uint64_t)(t - key) <= span && has_block;
            hout_u = 2;
            if (__ballot(active)) {
                if (active) {
                    if (col == lo) {                       // entering the band: deltas +1 below the cell above
                        Pv = ~0ull; Mv = 0;
                        score = lo == 1 ? (uint32_t)(64 * b + 64) : above - (hin_u - 1) + 64;
                        base = score;
                    }
                    uint64_t Eq = peq[ring[col & (ED_RING - 1)] * lanes + tid];
                    const uint64_t hneg = hin_u == 0, hpos = hin_u == 2;
                    const uint64_t Xv = Eq | Mv;
                    Eq |= hneg;
                    const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
                    uint64_t Ph = Mv | ~(Xh | Pv);
                    uint64_t Mh = Pv & Xh;
                    hout_u = 1 + (uint32_t)(Ph >> 63) - (uint32_t)(Mh >> 63);
                    Ph = (Ph << 1) | hpos;
                    Mh = (Mh << 1) | hneg;
                    Pv = Mh | ~(Xv | Ph);
                    Mv = Ph & Xv;
                    score += hout_u - 1;
                    if (bottom) {
                        acc |= hout_u << (2 * (col & 15));
                        if ((col & 15) == 15 || col == hi) { words[col >> 4] = acc; acc = 0; }
                        if (last_stripe) {
                            if (col == n) {                // the distance: the bottom value less the padding rows' deltas
                                const int r = (int)(m - 64 * b);
                                const uint64_t pad = r >= 64 ? 0 : ~0ull << r;
                                s_res[1] = (int64_t)score - __popcll(Pv & pad) + __popcll(Mv & pad);
                            }
                        } else {
                            lb = min(lb, (int64_t)score + llabs((n - col) - (m - 64 * b - 64)));
                        }
                    }
                }
            }
            if (lane == 63) { carry[t & 1][wave][0] = hout_u; carry[t & 1][wave][1] = score; }
            __syncthreads();
        }
        if (bottom) { s_res[0] = lb; s_prev[0] = lo; s_prev[1] = hi; s_prev[2] = base; }   // base: the value at lo - 1
        __syncthreads();
        if (last_stripe) { dist = s_res[1]; break; }
        if (s_res[0] > k) break;             // no path of cost <= k crosses this row
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = dist >= 0 && dist <= k ? dist : ED_EXCEEDED;
}

}  // namespace

extern "C" {

int phi_edit_distances(phi_ctx *c, const char *a, const int64_t *a_off, const char *b, const int64_t *b_off,
                       int64_t n_pairs, int64_t max_distance, int64_t *out)
{
    if (!c) return PHI_ERR_INVALID;
    if (n_pairs < 0 || (n_pairs > 0 && (!a_off || !b_off || !out)))
        return phi_fail(c, PHI_ERR_INVALID, "phi_edit_distances: null pointer or negative pair count");
    if (n_pairs == 0) return PHI_OK;
    if (a_off[0] < 0 || b_off[0] < 0) return phi_fail(c, PHI_ERR_INVALID, "phi_edit_distances: negative offset");
    for (int64_t i = 0; i < n_pairs; i++) {
        if (a_off[i + 1] < a_off[i] || b_off[i + 1] < b_off[i])
            return phi_fail(c, PHI_ERR_INVALID, "phi_edit_distances: offsets not monotone at pair %lld", (long long)i);
        if (a_off[i + 1] - a_off[i] >= ((int64_t)1 << 31) || b_off[i + 1] - b_off[i] >= ((int64_t)1 << 31))
            return phi_fail(c, PHI_ERR_UNSUPPORTED, "phi_edit_distances: pair %lld has a sequence of 2^31 bytes or more", (long long)i);
    }
    const int64_t a_bytes = a_off[n_pairs] - a_off[0], b_bytes = b_off[n_pairs] - b_off[0];
    if ((a_bytes > 0 && !a) || (b_bytes > 0 && !b)) return phi_fail(c, PHI_ERR_INVALID, "phi_edit_distances: null sequence");

    // pairs decided without the device: an empty side, or |n - m| above the cap
    std::vector<int64_t> k(n_pairs, 0);
    std::vector<int> pending;
    for (int64_t i = 0; i < n_pairs; i++) {
        const int64_t la = a_off[i + 1] - a_off[i], lb = b_off[i + 1] - b_off[i];
        const int64_t d0 = std::max(la, lb) - std::min(la, lb);
        out[i] = -1;
        if (max_distance >= 0 && d0 > max_distance) continue;
        if (std::min(la, lb) == 0) { out[i] = d0; continue; }
        k[i] = std::max<int64_t>(64, d0 + 64);
        if (max_distance >= 0) k[i] = std::min(k[i], max_distance);
        pending.push_back((int)i);
    }
    if (pending.empty()) return PHI_OK;

    HIPCHK(hipSetDevice(c->device));
    DevBuf d_seq, d_pairs, d_words, d_out;
    struct Guard { DevBuf *b[4]; ~Guard() { for (DevBuf *x : b) if (x->p) (void)hipFree(x->p); } } guard{{&d_seq, &d_pairs, &d_words, &d_out}};
    const size_t a_bytes_pad = ((size_t)a_bytes + 15) & ~(size_t)15;
    PHICHK(phi_dev_ensure(c, d_seq, std::max<size_t>(a_bytes_pad + (size_t)b_bytes, 16)));
    if (a_bytes) HIPCHK(hipMemcpyAsync(d_seq.p, a + a_off[0], (size_t)a_bytes, hipMemcpyHostToDevice, c->stream));
    if (b_bytes) HIPCHK(hipMemcpyAsync(d_seq.as<uint8_t>() + a_bytes_pad, b + b_off[0], (size_t)b_bytes, hipMemcpyHostToDevice, c->stream));

    std::vector<EdPair> pairs;
    std::vector<int64_t> res;
    while (!pending.empty()) {
        pairs.clear();
        int64_t words = 0, need_lanes = 64;
        for (int i : pending) {
            const int64_t la = a_off[i + 1] - a_off[i], lb = b_off[i + 1] - b_off[i];
            const int64_t pa = a_off[i] - a_off[0], pb = (int64_t)a_bytes_pad + b_off[i] - b_off[0];
            EdPair p;
            if (la <= lb) { p.q_off = pa; p.m = la; p.t_off = pb; p.n = lb; }
            else          { p.q_off = pb; p.m = lb; p.t_off = pa; p.n = la; }
            p.k = k[i];
            p.words_off = words;
            words += p.n / 16 + 2;
            const int64_t e = std::max<int64_t>(1, (p.k - (p.n - p.m)) / 2);
            const int64_t band_blocks = (p.n - p.m + 2 * e + 63) / 64 + 2;
            need_lanes = std::max(need_lanes, std::min(band_blocks, (p.m + 63) / 64));
            pairs.push_back(p);
        }
        const int threads = (int)std::min<int64_t>(ED_MAX_LANES, (need_lanes + 63) & ~(int64_t)63);
        PHICHK(phi_dev_ensure(c, d_pairs, pairs.size() * sizeof(EdPair)));
        PHICHK(phi_dev_ensure(c, d_words, (size_t)words * 4));
        PHICHK(phi_dev_ensure(c, d_out, pairs.size() * 8));
        HIPCHK(hipMemcpyAsync(d_pairs.p, pairs.data(), pairs.size() * sizeof(EdPair), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(phi_edit_band_kernel, dim3((unsigned)pairs.size()), dim3(threads), 0, c->stream,
                           d_seq.as<const uint8_t>(), d_pairs.as<const EdPair>(), d_words.as<uint32_t>(), d_out.as<int64_t>());
        HIPCHK(hipGetLastError());
        res.resize(pairs.size());
        HIPCHK(hipMemcpyAsync(res.data(), d_out.p, pairs.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        std::vector<int> again;
        for (size_t j = 0; j < pairs.size(); j++) {
            const int i = pending[j];
            if (res[j] >= 0) { out[i] = res[j]; continue; }
            if (max_distance >= 0 && k[i] >= max_distance) continue;            // out[i] stays -1
            if (k[i] > pairs[j].n + pairs[j].m)                                   // a band of k >= n always proves the distance
                return phi_fail(c, PHI_ERR_DEVICE, "phi_edit_distances: pair %d not proven at k = %lld (internal error)", i, (long long)k[i]);
            k[i] = 2 * k[i];
            if (max_distance >= 0) k[i] = std::min(k[i], max_distance);
            again.push_back(i);
        }
        pending.swap(again);
    }
    return PHI_OK;
}

}  // extern "C"
