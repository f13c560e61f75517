// edit_band.inc -- the banded pass of the edit distance (edit.hip, phi_edit_band_kernel) and the per-column block update
// it is made of, shared with the alignment path (edit_path.hip: the checkpoint pass and the recompute of block rows), so
// that every value the path recomputes is bit-identical to the one the pass computed.  Included inside an anonymous
// namespace after phi_ctx.h; edit.hip's header comment describes the algorithm.

#define ED_MAX_LANES 1024               // lanes (= blocks of a stripe) of the largest workgroup
#define ED_PEQ_WORDS (16 * 1024)        // 128 KB of Peq: codes x lanes <= 16 K (DNA: 5-6 codes x 1 024 lanes)
#define ED_RING 2048                    // columns of T staged in LDS (a stripe spans at most 1 024 + 1)
#define ED_CHUNK 256                    // columns staged per refill, two chunks ahead
#define ED_EXCEEDED (-2)                // the pass proved distance > k

struct EdPair {
    int64_t q_off, t_off;   // Q (rows, the shorter) and T (columns) in the device copy of the input
    int64_t m, n;           // |Q| >= 1, |T| >= m
    int64_t k;              // threshold of this pass
    int64_t words_off;      // this pair's 2-bit row of deltas (n / 16 + 2 words)
};

// Checkpoints of one pair (edit_path.hip): for every 64-row block b, the horizontal deltas of its bottom row over its
// band columns [lo(b), hi(b)] (column lo(b) + p at 2 bits in words[b * stride + p / 16]) and the value of the row above
// it at column lo(b) - 1 (top[b]).
struct EdCkpt {
    uint32_t *words;
    uint32_t *top;
    int64_t stride;         // words per block
};

__device__ __forceinline__ uint32_t shift_down_one_lane(uint32_t v)
{
    // lane l gets lane l - 1's value (wave_shr:1); lane 0 keeps its own, replaced by the caller
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false);
}

// Band entry of block b at column lo: vertical deltas +1 below the cell above.  `above` is the value of the row above at
// column lo and hin_u its horizontal delta there (+1); `score` becomes the block's bottom value at column lo - 1.  (A
// macro, not a function: inlined as a function it compiles the pass to a different, longer sequence.)
#define ED_BLOCK_ENTER(score, lo, b, above, hin_u, Pv, Mv)                                     \
    do {                                                                                        \
        Pv = ~0ull; Mv = 0;                                                                     \
        score = (lo) == 1 ? (uint32_t)(64 * (b) + 64) : (above) - ((hin_u) - 1) + 64;           \
    } while (0)

// One column of a 64-row block (Myers / Hyyro): Eq = rows equal to the column's byte, hin_u = horizontal delta + 1 of
// the row above; updates the vertical deltas (Pv, Mv) and returns the bottom row's horizontal delta + 1.
__device__ __forceinline__ uint32_t ed_block_step(uint64_t Eq, uint32_t hin_u, uint64_t &Pv, uint64_t &Mv)
{
    const uint64_t hneg = hin_u == 0, hpos = hin_u == 2;
    const uint64_t Xv = Eq | Mv;
    Eq |= hneg;
    const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    uint64_t Ph = Mv | ~(Xh | Pv);
    uint64_t Mh = Pv & Xh;
    const uint32_t hout_u = 1 + (uint32_t)(Ph >> 63) - (uint32_t)(Mh >> 63);
    Ph = (Ph << 1) | hpos;
    Mh = (Mh << 1) | hneg;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
    return hout_u;
}

// One pass at threshold k of pair blockIdx.x; CKPT: every lane also leaves its block's checkpoint (EdCkpt).
template <bool CKPT>
__device__ __forceinline__ void ed_band_pass(const uint8_t *__restrict__ seq, const EdPair *__restrict__ pairs,
                                             uint32_t *__restrict__ words_all, int64_t *__restrict__ out, const EdCkpt *__restrict__ ckpts)
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
        [[maybe_unused]] uint32_t cacc = 0;              // CKPT: this lane's deltas since its last full word
        [[maybe_unused]] uint32_t *cwords = nullptr;
        if constexpr (CKPT) cwords = ckpts[blockIdx.x].words + b * ckpts[blockIdx.x].stride;

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
                        ED_BLOCK_ENTER(score, lo, b, above, hin_u, Pv, Mv);
                        base = score;
                        if constexpr (CKPT) ckpts[blockIdx.x].top[b] = score - 64;
                    }
                    const uint64_t Eq = peq[ring[col & (ED_RING - 1)] * lanes + tid];
                    hout_u = ed_block_step(Eq, hin_u, Pv, Mv);
                    score += hout_u - 1;
                    if constexpr (CKPT) {
                        const int64_t p = col - lo;
                        cacc |= hout_u << (2 * (p & 15));
                        if ((p & 15) == 15 || col == hi) { cwords[p >> 4] = cacc; cacc = 0; }
                    }
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
