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
// The pass and its per-column block update are in edit_band.inc, shared with the alignment path (edit_path.hip).
#include <algorithm>
#include <string.h>
#include <vector>
#include "phi_ctx.h"

namespace {

#include "edit_band.inc"

__global__ void __launch_bounds__(ED_MAX_LANES) phi_edit_band_kernel(const uint8_t *__restrict__ seq, const EdPair *__restrict__ pairs,
                                                                     uint32_t *__restrict__ words_all, int64_t *__restrict__ out)
{
    ed_band_pass<false>(seq, pairs, words_all, out, nullptr);
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
