// edit_path.hip -- one optimal global alignment (unit costs) of byte strings whose edit distance is known: the CIGAR and
// the counts behind the alignment identity the reference's evaluation prints next to the distance (data/edlib_edits.py:
// 8-43, data/postprocessing_2_MIQP.py:21-39), at whole-MHC length.  DESIGN.md section 4.7.
//
// Given d = the distance (phi_edit_distances), every optimal path lies in Ukkonen's band for k = d and the band's values
// are exact on it (edit.hip).  Three kernels, the first two built from edit_band.inc so that their values are the band
// pass's, bit for bit:
//   - phi_edit_ckpt_kernel: the band pass at k = d (one workgroup per pair), where every lane also stores its 64-row
//     block's bottom-row horizontal deltas over the block's band columns (2 bits each) and the value of the row above
//     the block at the column before its band: the checkpoints, ~|Q| (d + 64) / 256 bytes per pair.
//   - phi_edit_rows_kernel: given the checkpoint of block b - 1, block row b is independent of every other; one lane per
//     block row sweeps its band columns and writes each column's vertical deltas (Pv, Mv) and the value of the row above
//     it (top) to HBM.  The host runs block rows in batches from the last one up, as far as device memory allows.
//   - phi_edit_walk_kernel: one wave per pair walks from (|Q|, |T|) back to (0, 0) over the batch's block rows, taking at
//     each cell the first predecessor that keeps the value (diagonal, then the step that consumes the caller's a, then
//     the one that consumes b) and emitting run-length operations.  The walk state is wave-uniform: a window of 64
//     columns of the current block row sits one column per lane, read with readlane, reloaded when the walk leaves it.
//     It stops at the batch's first block row and resumes there after the next batch.
// The walk checks that every cell's value is the one the previous step expected; any inconsistency, a cell outside its
// block's band, or a path longer than |Q| + |T| steps sets an error flag the host reports as PHI_ERR_DEVICE.
#include <algorithm>
#include <string.h>
#include <vector>
#include "phi_ctx.h"

namespace {

#include "edit_band.inc"

#define EP_AREA_MAX ((int64_t)16 << 30)  // bytes of block rows per batch at most: beyond, fewer batches save little

enum { EP_EQ = 0, EP_X = 1, EP_I = 2, EP_D = 3 };       // CIGAR operations in the caller's orientation
enum { EP_ERR_NONE = 0, EP_ERR_STEP = 1, EP_ERR_VALUE = 2, EP_ERR_BAND = 3, EP_ERR_RUNS = 4, EP_ERR_LONG = 5 };

struct EpPair {
    int64_t q_off, t_off;       // Q (rows, the shorter) and T (columns) in the device copy of the input
    int64_t m, n;
    int64_t dmin, dmax;         // the band's diagonals at k = d
    int64_t d;
    uint32_t *ck_words;         // checkpoints (EdCkpt)
    uint32_t *ck_top;
    int64_t ck_stride;
    int64_t rec_stride;         // records per block row in the batch area: the widest block's columns + 1
    int64_t code_off;           // this pair's 256-byte code table (bytes of Q -> dense codes)
    int64_t run_off, run_cap;   // this pair's run buffer
    int32_t swap;               // Q is the caller's b
    int32_t pad;
};

struct EpTask {                 // one workgroup of the recompute: up to 64 consecutive block rows of one pair
    int32_t pair, count;
    int64_t b_first;
    int64_t rec_first;          // batch-area record of block row b_first's first column
};

struct EpBatch {                // one pair's block rows in the current batch: from b_lo on, block row b_lo at record rec_lo
    int64_t b_lo, rec_lo;
    int32_t pair, pad;
};

struct EpWalk {                 // walk state of one pair, kept between batches
    int64_t i, j;               // current cell
    int64_t expect;             // its value, as the previous step found it
    int64_t steps;
    int64_t n_runs;
    int64_t run_len;
    int64_t cnt[4];
    int32_t run_op, done, err, pad;
};

struct EpRec {                  // the batch area, structure of arrays
    uint64_t *pv, *mv;
    uint32_t *top;
};

__device__ __forceinline__ int64_t ep_lo(int64_t b, int64_t dmin) { return max((int64_t)1, 64 * b + 1 + dmin); }
__device__ __forceinline__ int64_t ep_hi(int64_t b, int64_t dmax, int64_t n) { return min(n, 64 * b + 64 + dmax); }

__global__ void __launch_bounds__(ED_MAX_LANES) phi_edit_ckpt_kernel(const uint8_t *__restrict__ seq, const EdPair *__restrict__ pairs,
                                                                     uint32_t *__restrict__ words_all, int64_t *__restrict__ out,
                                                                     const EdCkpt *__restrict__ ckpts)
{
    ed_band_pass<true>(seq, pairs, words_all, out, ckpts);
}

// block row b of pair task.pair: record 0 is column lo(b) - 1 (the band entry: deltas +1), record c - lo(b) + 1 column c
__global__ void __launch_bounds__(64) phi_edit_rows_kernel(const uint8_t *__restrict__ seq, const uint8_t *__restrict__ codes,
                                                           const EpPair *__restrict__ pairs, const EpTask *__restrict__ tasks, EpRec rec)
{
    extern __shared__ uint64_t peq[];               // [code][lane]
    __shared__ uint8_t code_of[256];
    const EpTask task = tasks[blockIdx.x];
    const EpPair P = pairs[task.pair];
    const int lane = threadIdx.x;
    const uint8_t *Q = seq + P.q_off, *T = seq + P.t_off;
    for (int x = lane; x < 256; x += 64) code_of[x] = codes[P.code_off + x];
    __syncthreads();
    if (lane >= task.count) return;
    const int64_t b = task.b_first + lane, m = P.m, n = P.n;
    int alpha = 0;
    for (int x = 0; x < 256; x++) alpha = max(alpha, (int)code_of[x] + 1);
    for (int a = 0; a < alpha; a++) peq[a * 64 + lane] = 0;
    for (int i = 0; i < 64; i++) {
        const int64_t row = 64 * b + i;
        if (row < m) peq[code_of[Q[row]] * 64 + lane] |= 1ull << i;
    }
    const int64_t lo = ep_lo(b, P.dmin), hi = ep_hi(b, P.dmax, n);
    const int64_t plo = ep_lo(b - 1, P.dmin), phi = b > 0 ? ep_hi(b - 1, P.dmax, n) : 0;   // the row above: block b - 1's band
    const uint32_t *above = P.ck_words + (b > 0 ? b - 1 : 0) * P.ck_stride;
    const int64_t rbase = task.rec_first + lane * P.rec_stride;
    uint64_t Pv = ~0ull, Mv = 0;                    // the band entry, from the value the checkpoint pass entered with
    uint32_t top = P.ck_top[b];
    rec.pv[rbase] = Pv; rec.mv[rbase] = Mv; rec.top[rbase] = top;
    for (int64_t c0 = lo; c0 <= hi; c0 += 16) {
        uint8_t tb[16];
#pragma unroll
        for (int u = 0; u < 16; u++) tb[u] = c0 + u <= hi ? T[c0 + u - 1] : 0;
        // 2-bit deltas of the row above for columns c0 .. c0 + 15 (block b - 1's checkpoint from column plo)
        uint32_t hw = 0;
        if (b > 0 && c0 <= phi) {
            const int64_t p = c0 - plo, w = p >> 4;
            const uint64_t lo_w = above[w], hi_w = w + 1 < P.ck_stride ? above[w + 1] : 0;
            hw = (uint32_t)((lo_w | (hi_w << 32)) >> (2 * (p & 15)));
        }
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int64_t col = c0 + u;
            if (col <= hi) {
                const uint32_t hin_u = b > 0 && col <= phi ? (hw >> (2 * u)) & 3 : 2;
                top += hin_u - 1;
                (void)ed_block_step(peq[code_of[tb[u]] * 64 + lane], hin_u, Pv, Mv);
                const int64_t r = rbase + (col - lo) + 1;
                rec.pv[r] = Pv; rec.mv[r] = Mv; rec.top[r] = top;
            }
        }
    }
}

__device__ __forceinline__ uint64_t ep_readlane64(uint64_t v, int l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// value of row 64 b + r + 1 at a column whose record is (pv, mv, top): top plus the deltas of rows 0..r of the block
__device__ __forceinline__ int64_t ep_value(uint64_t pv, uint64_t mv, uint32_t top, int r)
{
    const uint64_t mask = ~0ull >> (63 - r);
    return (int64_t)top + __popcll(pv & mask) - __popcll(mv & mask);
}

__global__ void __launch_bounds__(64) phi_edit_walk_kernel(const uint8_t *__restrict__ seq, const EpPair *__restrict__ pairs,
                                                           const EpBatch *__restrict__ batch, EpRec rec, EpWalk *__restrict__ walks,
                                                           int64_t *__restrict__ runs)
{
    const EpBatch B = batch[blockIdx.x];
    const EpPair P = pairs[B.pair];
    EpWalk *W = walks + B.pair;
    const int lane = threadIdx.x;
    if (W->done || W->err) return;
    const uint8_t *Q = seq + P.q_off, *T = seq + P.t_off;
    int64_t i = W->i, j = W->j, expect = W->expect, steps = W->steps, n_runs = W->n_runs, run_len = W->run_len;
    int64_t cnt0 = W->cnt[0], cnt1 = W->cnt[1], cnt2 = W->cnt[2], cnt3 = W->cnt[3];
    int run_op = W->run_op, err = EP_ERR_NONE, done = 0;
    const int vert_op = P.swap ? EP_D : EP_I, horz_op = P.swap ? EP_I : EP_D;
    const int64_t max_steps = P.m + P.n + 1;

    auto emit = [&](int op, int64_t len) {
        if (op == run_op) { run_len += len; return; }
        if (run_len > 0) {
            if (n_runs >= P.run_cap) { err = EP_ERR_RUNS; return; }
            if (lane == 0) runs[P.run_off + n_runs] = run_len << 2 | run_op;
            n_runs++;
        }
        run_op = op; run_len = len;
    };

    int64_t cur_b = -1, wb = 0, rec_first = 0;
    uint64_t pv = 0, mv = 0;
    uint32_t top = 0;
    uint8_t tb = 0, qb = 0;
    while (!err) {
        if (i == 0 || j == 0) {                        // the first row or column: one straight run to (0, 0)
            if (expect != (i == 0 ? j : i)) { err = EP_ERR_VALUE; break; }
            if (i > 0) { emit(vert_op, i); if (vert_op == EP_I) cnt2 += i; else cnt3 += i; }
            if (j > 0) { emit(horz_op, j); if (horz_op == EP_I) cnt2 += j; else cnt3 += j; }
            steps += i + j;
            i = 0; j = 0;
            emit(-1, 0);                               // flush the last run
            done = 1;
            break;
        }
        const int64_t b = (i - 1) >> 6;
        if (b < B.b_lo) break;                         // the next batch has this block row
        if (b != cur_b || j - 1 < wb) {
            const int64_t lo = ep_lo(b, P.dmin), hi = ep_hi(b, P.dmax, P.n);
            if (j < lo || j > hi) { err = EP_ERR_BAND; break; }
            rec_first = lo - 1;
            wb = max(rec_first, j - 63);
            const int64_t c = wb + lane;
            if (c <= hi) {
                const int64_t r = B.rec_lo + (b - B.b_lo) * P.rec_stride + (c - rec_first);
                pv = rec.pv[r]; mv = rec.mv[r]; top = rec.top[r];
                tb = c >= 1 ? T[c - 1] : 0;
            }
            if (b != cur_b) { qb = 64 * b + lane < P.m ? Q[64 * b + lane] : 0; cur_b = b; }
        }
        if (++steps > max_steps) { err = EP_ERR_LONG; break; }
        const int r = (int)((i - 1) & 63), lj = (int)(j - wb);
        const uint64_t pvj = ep_readlane64(pv, lj), mvj = ep_readlane64(mv, lj);
        const uint64_t pvl = ep_readlane64(pv, lj - 1), mvl = ep_readlane64(mv, lj - 1);
        const uint32_t topj = (uint32_t)__builtin_amdgcn_readlane((int)top, lj);
        const uint32_t topl = (uint32_t)__builtin_amdgcn_readlane((int)top, lj - 1);
        const int64_t v = ep_value(pvj, mvj, topj, r);
        if (v != expect) { err = EP_ERR_VALUE; break; }
        const int64_t vup = v - (int64_t)((pvj >> r) & 1) + (int64_t)((mvj >> r) & 1);
        const int64_t vleft = ep_value(pvl, mvl, topl, r);
        const int64_t vdiag = r == 0 ? (int64_t)topl : ep_value(pvl, mvl, topl, r - 1);
        const int neq = __builtin_amdgcn_readlane((int)qb, r) != __builtin_amdgcn_readlane((int)tb, lj);
        const bool up_ok = vup + 1 == v, left_ok = vleft + 1 == v;
        if (vdiag + neq == v) {
            emit(neq ? EP_X : EP_EQ, 1);
            if (neq) cnt1++; else cnt0++;
            i--; j--; expect = vdiag;
        } else if (P.swap ? left_ok : up_ok) {         // the step that consumes the caller's a: I
            emit(EP_I, 1); cnt2++;
            if (P.swap) { j--; expect = vleft; } else { i--; expect = vup; }
        } else if (P.swap ? up_ok : left_ok) {         // then the one that consumes b: D
            emit(EP_D, 1); cnt3++;
            if (P.swap) { i--; expect = vup; } else { j--; expect = vleft; }
        } else {
            err = EP_ERR_STEP;
        }
    }
    if (lane == 0) {
        W->i = i; W->j = j; W->expect = expect; W->steps = steps; W->n_runs = n_runs; W->run_len = run_len;
        W->cnt[0] = cnt0; W->cnt[1] = cnt1; W->cnt[2] = cnt2; W->cnt[3] = cnt3;
        W->run_op = run_op; W->done = done; W->err = err;
    }
}

const char *ep_err_text(int e)
{
    switch (e) {
    case EP_ERR_STEP: return "a cell with no predecessor that keeps its value";
    case EP_ERR_VALUE: return "a cell whose value differs from the one its successor expected";
    case EP_ERR_BAND: return "a cell outside its block's band";
    case EP_ERR_RUNS: return "more CIGAR runs than 2d + 1";
    case EP_ERR_LONG: return "a path longer than |a| + |b| steps";
    default: return "unknown";
    }
}

}  // namespace

extern "C" {

int phi_edit_alignments(phi_ctx *c, const char *a, const int64_t *a_off, const char *b, const int64_t *b_off,
                        int64_t n_pairs, const int64_t *dist, int64_t *counts, char *cigar, const int64_t *cigar_off)
{
    if (!c) return PHI_ERR_INVALID;
    if (n_pairs < 0 || (n_pairs > 0 && (!a_off || !b_off || !dist || !counts || (cigar && !cigar_off))))
        return phi_fail(c, PHI_ERR_INVALID, "phi_edit_alignments: null pointer or negative pair count");
    if (n_pairs == 0) return PHI_OK;
    if (a_off[0] < 0 || b_off[0] < 0 || (cigar && cigar_off[0] < 0))
        return phi_fail(c, PHI_ERR_INVALID, "phi_edit_alignments: negative offset");
    for (int64_t i = 0; i < n_pairs; i++) {
        if (a_off[i + 1] < a_off[i] || b_off[i + 1] < b_off[i] || (cigar && cigar_off[i + 1] < cigar_off[i]))
            return phi_fail(c, PHI_ERR_INVALID, "phi_edit_alignments: offsets not monotone at pair %lld", (long long)i);
        if (a_off[i + 1] - a_off[i] >= ((int64_t)1 << 31) || b_off[i + 1] - b_off[i] >= ((int64_t)1 << 31))
            return phi_fail(c, PHI_ERR_UNSUPPORTED, "phi_edit_alignments: pair %lld has a sequence of 2^31 bytes or more", (long long)i);
    }
    const int64_t a_bytes = a_off[n_pairs] - a_off[0], b_bytes = b_off[n_pairs] - b_off[0];
    if ((a_bytes > 0 && !a) || (b_bytes > 0 && !b)) return phi_fail(c, PHI_ERR_INVALID, "phi_edit_alignments: null sequence");
    for (int64_t i = 0; i < n_pairs; i++) {
        const int64_t la = a_off[i + 1] - a_off[i], lb = b_off[i + 1] - b_off[i], d = dist[i];
        if (d < -1) return phi_fail(c, PHI_ERR_INVALID, "phi_edit_alignments: pair %lld: distance %lld", (long long)i, (long long)d);
        if (d >= 0 && (d < std::max(la, lb) - std::min(la, lb) || d > std::max(la, lb)))
            return phi_fail(c, PHI_ERR_INVALID, "phi_edit_alignments: pair %lld: no alignment of lengths %lld and %lld costs %lld",
                            (long long)i, (long long)la, (long long)lb, (long long)d);
        if (d >= 0 && cigar && cigar_off[i + 1] - cigar_off[i] < 11 * (2 * d + 1))
            return phi_fail(c, PHI_ERR_INVALID, "phi_edit_alignments: pair %lld: CIGAR capacity %lld below 11 (2d + 1) = %lld",
                            (long long)i, (long long)(cigar_off[i + 1] - cigar_off[i]), (long long)(11 * (2 * d + 1)));
    }

    // the host's share: skipped pairs and an empty side
    auto put_cigar = [&](int64_t i, const std::vector<int64_t> &runs_fwd) {   // runs as len << 2 | op, in order
        if (!cigar) { int64_t len = 0; char tmp[24]; for (int64_t r : runs_fwd) len += snprintf(tmp, sizeof tmp, "%lld", (long long)(r >> 2)) + 1; counts[5 * i + 4] = len; return; }
        char *o = cigar + cigar_off[i];
        int64_t len = 0;
        for (int64_t r : runs_fwd) {
            len += snprintf(o + len, 12, "%lld", (long long)(r >> 2));
            o[len++] = "=XID"[r & 3];
        }
        counts[5 * i + 4] = len;
    };
    std::vector<int> pending;
    for (int64_t i = 0; i < n_pairs; i++) {
        const int64_t la = a_off[i + 1] - a_off[i], lb = b_off[i + 1] - b_off[i];
        int64_t *ct = counts + 5 * i;
        if (dist[i] < 0) { for (int q = 0; q < 5; q++) ct[q] = -1; continue; }
        if (std::min(la, lb) > 0) { pending.push_back((int)i); continue; }
        ct[0] = 0; ct[1] = 0; ct[2] = la; ct[3] = lb;
        std::vector<int64_t> r;
        if (la) r.push_back(la << 2 | EP_I);
        if (lb) r.push_back(lb << 2 | EP_D);
        put_cigar(i, r);
    }
    if (pending.empty()) return PHI_OK;

    HIPCHK(hipSetDevice(c->device));
    DevBuf d_seq, d_pairs, d_words, d_out, d_ck, d_ckp, d_ep, d_codes, d_runs, d_walk, d_tasks, d_batch, d_rec;
    struct Guard {
        DevBuf *b[13];
        ~Guard() { for (DevBuf *x : b) if (x->p) (void)hipFree(x->p); }
    } guard{{&d_seq, &d_pairs, &d_words, &d_out, &d_ck, &d_ckp, &d_ep, &d_codes, &d_runs, &d_walk, &d_tasks, &d_batch, &d_rec}};
    const size_t a_bytes_pad = ((size_t)a_bytes + 15) & ~(size_t)15;
    PHICHK(phi_dev_ensure(c, d_seq, std::max<size_t>(a_bytes_pad + (size_t)b_bytes, 16)));
    if (a_bytes) HIPCHK(hipMemcpyAsync(d_seq.p, a + a_off[0], (size_t)a_bytes, hipMemcpyHostToDevice, c->stream));
    if (b_bytes) HIPCHK(hipMemcpyAsync(d_seq.as<uint8_t>() + a_bytes_pad, b + b_off[0], (size_t)b_bytes, hipMemcpyHostToDevice, c->stream));

    // every pair's layout at k = d, and what its checkpoints take
    struct Plan { EdPair ed; EpPair ep; int64_t nb, ck_words, ck_bytes, row_bytes; uint8_t code_of[256]; int alpha; };
    std::vector<Plan> plan(pending.size());
    for (size_t j = 0; j < pending.size(); j++) {
        const int i = pending[j];
        Plan &p = plan[j];
        const int64_t la = a_off[i + 1] - a_off[i], lb = b_off[i + 1] - b_off[i];
        const int64_t pa = a_off[i] - a_off[0], pb = (int64_t)a_bytes_pad + b_off[i] - b_off[0];
        const bool swap = la > lb;
        p.ed.q_off = swap ? pb : pa; p.ed.m = swap ? lb : la;
        p.ed.t_off = swap ? pa : pb; p.ed.n = swap ? la : lb;
        p.ed.k = dist[i];
        const int64_t m = p.ed.m, n = p.ed.n, delta = n - m;
        const int64_t e = std::max<int64_t>(1, (dist[i] - delta) / 2);    // as the band pass computes it
        p.nb = (m + 63) / 64;
        const int64_t width = std::min(n, 64 + delta + 2 * e);             // columns of the widest block
        p.ep = EpPair{};
        p.ep.q_off = p.ed.q_off; p.ep.t_off = p.ed.t_off; p.ep.m = m; p.ep.n = n;
        p.ep.dmin = -e; p.ep.dmax = delta + e; p.ep.d = dist[i];
        p.ep.ck_stride = (width + 15) / 16 + 1;
        p.ep.rec_stride = width + 1;
        p.ep.swap = swap;
        p.ck_words = p.nb * p.ep.ck_stride + p.nb + n / 16 + 2;           // checkpoints, tops, the stripes' row
        p.ck_bytes = 4 * p.ck_words;
        p.row_bytes = 20 * p.ep.rec_stride;
        const char *q = swap ? b + b_off[i] : a + a_off[i];
        bool present[256] = {};
        for (int64_t x = 0; x < m; x++) present[(uint8_t)q[x]] = true;
        int na = 0;
        for (int x = 0; x < 256; x++) if (present[x]) p.code_of[x] = (uint8_t)na++;
        for (int x = 0; x < 256; x++) if (!present[x]) p.code_of[x] = (uint8_t)(na < 256 ? na : 0);
        p.alpha = na < 256 ? na + 1 : 256;
    }

    // launches: groups of pairs whose checkpoints take at most half of the free device memory, the rest for block rows
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const int64_t reserve = (int64_t)1 << 29;
    const int64_t avail = std::max<int64_t>(0, ((int64_t)free_b - reserve) / 10 * 9);
    for (size_t j = 0; j < plan.size(); j++)
        if (plan[j].ck_bytes + 64 * plan[j].row_bytes > avail)
            return phi_fail(c, PHI_ERR_NOMEM, "phi_edit_alignments: pair %d needs %lld bytes of checkpoints and block rows, %lld are free",
                            pending[j], (long long)(plan[j].ck_bytes + 64 * plan[j].row_bytes), (long long)avail);

    std::vector<int64_t> runs_h;
    for (size_t g0 = 0; g0 < plan.size();) {
        size_t g1 = g0;
        int64_t ck_total = 0, rows_total = 0;
        while (g1 < plan.size() && (g1 == g0 || (ck_total + plan[g1].ck_bytes <= avail / 2 &&
                                                 ck_total + plan[g1].ck_bytes + 64 * (rows_total + plan[g1].row_bytes) <= avail))) {
            ck_total += plan[g1].ck_bytes; rows_total += plan[g1].row_bytes; g1++;
        }
        const int ng = (int)(g1 - g0);

        // ---- checkpoint pass (the band pass at k = d)
        std::vector<EdPair> ed(ng);
        std::vector<EdCkpt> ck(ng);
        std::vector<EpPair> ep(ng);
        int64_t words = 0, ck_off = 0, run_total = 0, need_lanes = 64;
        std::vector<uint8_t> codes(256 * (size_t)ng);
        int alpha_max = 1;
        int64_t nb_max = 0;
        for (int q = 0; q < ng; q++) {
            const Plan &p = plan[g0 + q];
            ed[q] = p.ed; ed[q].words_off = words; words += p.ed.n / 16 + 2;
            ep[q] = p.ep;
            ep[q].code_off = 256 * (int64_t)q;
            ep[q].run_off = run_total; ep[q].run_cap = 2 * p.ep.d + 1; run_total += ep[q].run_cap;
            memcpy(codes.data() + 256 * (size_t)q, p.code_of, 256);
            alpha_max = std::max(alpha_max, p.alpha);
            nb_max = std::max(nb_max, p.nb);
            const int64_t band_blocks = (p.ep.dmax - p.ep.dmin + 63) / 64 + 2;
            need_lanes = std::max(need_lanes, std::min(band_blocks, p.nb));
        }
        PHICHK(phi_dev_ensure(c, d_ck, (size_t)std::max<int64_t>(ck_total - 4 * words, 4)));
        PHICHK(phi_dev_ensure(c, d_words, (size_t)words * 4));
        for (int q = 0; q < ng; q++) {
            const Plan &p = plan[g0 + q];
            ck[q].words = d_ck.as<uint32_t>() + ck_off; ck_off += p.nb * p.ep.ck_stride;
            ck[q].top = d_ck.as<uint32_t>() + ck_off; ck_off += p.nb;
            ck[q].stride = p.ep.ck_stride;
            ep[q].ck_words = ck[q].words; ep[q].ck_top = ck[q].top; ep[q].ck_stride = ck[q].stride;
        }
        PHICHK(phi_dev_ensure(c, d_pairs, ng * sizeof(EdPair)));
        PHICHK(phi_dev_ensure(c, d_ckp, ng * sizeof(EdCkpt)));
        PHICHK(phi_dev_ensure(c, d_out, ng * 8));
        HIPCHK(hipMemcpyAsync(d_pairs.p, ed.data(), ng * sizeof(EdPair), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_ckp.p, ck.data(), ng * sizeof(EdCkpt), hipMemcpyHostToDevice, c->stream));
        const int threads = (int)std::min<int64_t>(ED_MAX_LANES, (need_lanes + 63) & ~(int64_t)63);
        hipLaunchKernelGGL(phi_edit_ckpt_kernel, dim3((unsigned)ng), dim3(threads), 0, c->stream, d_seq.as<const uint8_t>(),
                           d_pairs.as<const EdPair>(), d_words.as<uint32_t>(), d_out.as<int64_t>(), d_ckp.as<const EdCkpt>());
        HIPCHK(hipGetLastError());
        std::vector<int64_t> res(ng);
        HIPCHK(hipMemcpyAsync(res.data(), d_out.p, ng * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int q = 0; q < ng; q++)
            if (res[q] != plan[g0 + q].ep.d)
                return phi_fail(c, PHI_ERR_INVALID, "phi_edit_alignments: pair %d: no alignment costs the given distance %lld (%s)",
                                pending[g0 + q], (long long)plan[g0 + q].ep.d,
                                res[q] < 0 ? "the distance is larger" : "the distance is smaller");

        // ---- block rows in batches from the last one up, each followed by the walk over it
        PHICHK(phi_dev_ensure(c, d_ep, ng * sizeof(EpPair)));
        PHICHK(phi_dev_ensure(c, d_codes, codes.size()));
        PHICHK(phi_dev_ensure(c, d_runs, (size_t)run_total * 8));
        PHICHK(phi_dev_ensure(c, d_walk, ng * sizeof(EpWalk)));
        HIPCHK(hipMemcpyAsync(d_ep.p, ep.data(), ng * sizeof(EpPair), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice, c->stream));
        std::vector<EpWalk> walk(ng);
        for (int q = 0; q < ng; q++) {
            walk[q] = EpWalk{};
            walk[q].i = ep[q].m; walk[q].j = ep[q].n; walk[q].expect = ep[q].d; walk[q].run_op = -1;
        }
        HIPCHK(hipMemcpyAsync(d_walk.p, walk.data(), ng * sizeof(EpWalk), hipMemcpyHostToDevice, c->stream));
        const int64_t area = std::min(avail - ck_total, EP_AREA_MAX);
        const int64_t rows = std::min(nb_max, std::max<int64_t>(1, area / rows_total));
        int64_t recs = 0;
        for (int q = 0; q < ng; q++) recs += std::min(rows, plan[g0 + q].nb) * ep[q].rec_stride;
        PHICHK(phi_dev_ensure(c, d_rec, (size_t)recs * 20));
        EpRec rec{d_rec.as<uint64_t>(), d_rec.as<uint64_t>() + recs, reinterpret_cast<uint32_t *>(d_rec.as<uint64_t>() + 2 * recs)};
        std::vector<int64_t> b_hi(ng);
        for (int q = 0; q < ng; q++) b_hi[q] = plan[g0 + q].nb - 1;
        std::vector<EpTask> tasks;
        std::vector<EpBatch> batch;
        for (int64_t round = 0; round * rows < nb_max; round++) {
            tasks.clear(); batch.clear();
            int64_t at = 0;
            for (int q = 0; q < ng; q++) {
                if (b_hi[q] < 0) continue;
                const int64_t lo_b = std::max<int64_t>(0, b_hi[q] - rows + 1);
                for (int64_t bb = lo_b; bb <= b_hi[q]; bb += 64)
                    tasks.push_back(EpTask{q, (int32_t)std::min<int64_t>(64, b_hi[q] - bb + 1), bb, at + (bb - lo_b) * ep[q].rec_stride});
                batch.push_back(EpBatch{lo_b, at, q, 0});
                at += (b_hi[q] - lo_b + 1) * ep[q].rec_stride;
                b_hi[q] = lo_b - 1;
            }
            if (at > recs) return phi_fail(c, PHI_ERR_DEVICE, "phi_edit_alignments: batch area overrun (internal error)");
            PHICHK(phi_dev_ensure(c, d_tasks, tasks.size() * sizeof(EpTask)));
            PHICHK(phi_dev_ensure(c, d_batch, batch.size() * sizeof(EpBatch)));
            HIPCHK(hipMemcpyAsync(d_tasks.p, tasks.data(), tasks.size() * sizeof(EpTask), hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d_batch.p, batch.data(), batch.size() * sizeof(EpBatch), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(phi_edit_rows_kernel, dim3((unsigned)tasks.size()), dim3(64), (size_t)alpha_max * 64 * 8, c->stream,
                               d_seq.as<const uint8_t>(), d_codes.as<const uint8_t>(), d_ep.as<const EpPair>(), d_tasks.as<const EpTask>(), rec);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(phi_edit_walk_kernel, dim3((unsigned)batch.size()), dim3(64), 0, c->stream, d_seq.as<const uint8_t>(),
                               d_ep.as<const EpPair>(), d_batch.as<const EpBatch>(), rec, d_walk.as<EpWalk>(), d_runs.as<int64_t>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(c->stream));     // the host rewrites the task and batch lists
        }
        HIPCHK(hipMemcpyAsync(walk.data(), d_walk.p, ng * sizeof(EpWalk), hipMemcpyDeviceToHost, c->stream));
        runs_h.resize((size_t)run_total);
        HIPCHK(hipMemcpyAsync(runs_h.data(), d_runs.p, (size_t)run_total * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int q = 0; q < ng; q++) {
            const EpWalk &w = walk[q];
            const int i = pending[g0 + q];
            if (w.err || !w.done)
                return phi_fail(c, PHI_ERR_DEVICE, "phi_edit_alignments: pair %d: the walk met %s at (%lld, %lld) (internal error)",
                                i, w.err ? ep_err_text(w.err) : "the end of the last batch", (long long)w.i, (long long)w.j);
            if (w.cnt[1] + w.cnt[2] + w.cnt[3] != ep[q].d)
                return phi_fail(c, PHI_ERR_DEVICE, "phi_edit_alignments: pair %d: the walk's path costs %lld, not %lld (internal error)",
                                i, (long long)(w.cnt[1] + w.cnt[2] + w.cnt[3]), (long long)ep[q].d);
            int64_t *ct = counts + 5 * (int64_t)i;
            for (int o = 0; o < 4; o++) ct[o] = w.cnt[o];
            std::vector<int64_t> fwd(runs_h.begin() + ep[q].run_off, runs_h.begin() + ep[q].run_off + w.n_runs);
            std::reverse(fwd.begin(), fwd.end());
            put_cigar(i, fwd);
        }
        (void)hipFree(d_rec.p);                          // the next group's checkpoints may need its room
        d_rec = DevBuf{};
        g0 = g1;
    }
    return PHI_OK;
}

}  // extern "C"
