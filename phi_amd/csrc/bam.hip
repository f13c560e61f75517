// bam.hip -- the reads of a BAM file found and decoded ON THE DEVICE (include/phi_amd.h phi_reads_bam_*).
//
// The reference reads FASTA / FASTQ with kseq (src/ILP_index.cpp:313-328); long-read instruments hand out unaligned BAM, and a
// user runs `samtools fastq` into a second file first.  Here the INFLATED bytes of the BAM go to HBM as they are, piece by
// piece, and these kernels turn them into the (bases, read offsets) that phi_add_reads_device takes.
//
// A BAM record chain (next = pos + 4 + block_size) is serial by definition.  It is walked in parallel the way the inflater
// finds its block starts: speculate, then confirm.
//   tile      one wave per tile of tile_bytes: the tile and a halo are staged in LDS; the lanes test candidate positions for a
//             plausible record (bam_plausible), the lowest accepted one is the tile's speculative start; from it the wave lists
//             the tile's record starts and its exit, the first start at or beyond the tile's end -- a chain of LDS reads.
//             Tile 0 starts at the piece's first byte, which IS on the true chain (the header's end, or the carry).
//   link      one lane per tile: does the tile's exit equal the speculative start of the next tile that has one?  If every link
//             holds, every list is the true chain's (next is a function of the position alone: two chains that share a position
//             are one from there on) -- a parallel comparison, no walk.
//   fix       one wave, from the first link that does not hold: the true incoming position is looked up in the entered tile's
//             list (used from there on) or the tile is walked again from it; tiles the chain passes over are emptied.  Serial
//             over TILES behind the first false link, never one dependent global load per record of the piece.
//   records   one lane per record: kept (flag & 0x900 == 0, l_seq > 0)?  Counters.
//   (phi_compact, phi_scan of scan.hip: kept records in order, their lengths summed into read offsets)
//   kept      one lane per kept record: length, where its sequence starts, reverse; are all lengths one?
//   decode    every wave fills 2 KB of bases: finds its first record by a search in the offsets, turns nibbles into ASCII --
//             mirrored and complemented for a reverse record -- with coalesced byte stores.
// Nothing the finder accepts wrongly can change the output: a wrong list is never entered by the true chain, or entered at a
// position it holds -- then it is right from there on.  It costs a re-walk, and those are counted.
//
// UNTRUSTED INPUT.  Every position is compared with the piece's end before anything is loaded from it; a record is listed only
// when its fixed part and its whole block lie inside the piece; block_size is used as a 64-bit sum, so no value of it wraps;
// a record that is not well-formed ends the chain there (every well-formed step advances by 37 bytes at least), and every
// chain loop is bounded by tile_bytes / 37 + 2 turns besides.  All positions are offsets into one buffer [carry | piece],
// below 2^32.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "phi_ctx.h"
#include "phi_kernels.h"
#include "phi_wave.h"
#include "bam_header.h"

#define BAM_FIXED 36u            // block_size + the 32 fixed bytes: what a record's plausibility is read from
#define BAM_MIN_STEP 37u         // 4 + 32 + l_read_name >= 1
#define BAM_HALO 304u            // staged behind a tile: the fixed part and the longest name of a record that starts on its last byte
#define BAM_NONE 0xFFFFFFFFu
#define BAM_TILE_DEFAULT 32768
#define BAM_TILE_MAX 49152       // tile + halo within the 64 KB of LDS a workgroup gets without asking
#define BAM_DECODE_WAVE 2048u
#define BAM_ST_OK 0u             // the walk left the tile: exit = the first start at or beyond its end
#define BAM_ST_REST 1u           // exit = a record whose fixed part or block passes the piece's end: the unfinished rest
#define BAM_ST_BAD 2u            // exit = a record that is not well-formed

struct PhiBamSummary {
    uint32_t status, rest_pos;                 // of the true chain: BAM_ST_OK / _REST (the carry starts at rest_pos) / _BAD (at rest_pos)
    uint32_t first_bad_tile, last_tile;        // link kernel: the first tile whose link does not hold (BAM_NONE: all hold); the last tile with a start
    uint32_t tiles_used, tiles_rewalked;
    uint32_t n_secsup, n_empty, n_rev, not_uniform;
    uint32_t pad_[2];
};

struct PhiBamArgs {
    const uint8_t *buf;                        // [carry | piece]; readable up to end + 63
    uint32_t start, end;                       // the bytes are buf[start, end)
    uint32_t tile, n_tiles, list_cap;
    int32_t n_ref;
    uint32_t *t_first, *t_exit, *t_status, *t_list;      // per tile; t_list[tile * list_cap + i]
    int32_t *t_cnt, *t_skip, *t_has, *t_has_pre, *t_use, *t_base;
    uint32_t *rec_pos; uint8_t *rec_keep;
    PhiBamSummary *sum;
};

namespace {

extern __shared__ uint4 s_stage[];

__device__ __forceinline__ uint32_t s_u8(const uint8_t *s, uint32_t i) { return s[i]; }
__device__ __forceinline__ uint32_t s_u16(const uint8_t *s, uint32_t i) { return s_u8(s, i) | s_u8(s, i + 1) << 8; }
__device__ __forceinline__ uint32_t s_u32(const uint8_t *s, uint32_t i) { return s_u16(s, i) | s_u16(s, i + 2) << 16; }

// buf[a0, stage_end) -> LDS, a0 a multiple of 16 (the loads run up to 15 bytes past stage_end: inside the buffer's padding)
__device__ __forceinline__ void bam_stage(const uint8_t *buf, uint32_t a0, uint32_t stage_end)
{
    const uint4 *g = reinterpret_cast<const uint4 *>(buf + a0);
    const uint32_t n16 = (stage_end - a0 + 15u) >> 4;
    for (uint32_t i = threadIdx.x; i < n16; i += 64) s_stage[i] = g[i];
    __syncthreads();
}

// The record whose first byte is LDS byte i (its 36 fixed bytes are staged and inside the piece): well-formed?  *step = 4 + block_size.
__device__ __forceinline__ bool bam_wellformed(const uint8_t *s, uint32_t i, uint64_t *step)
{
    const int32_t bs = (int32_t)s_u32(s, i);
    const uint32_t lrn = s_u8(s, i + 12), nc = s_u16(s, i + 16);
    const int32_t ls = (int32_t)s_u32(s, i + 20);
    *step = 4ull + (uint64_t)(uint32_t)bs;
    if (bs < 0 || lrn < 1 || ls < 0) return false;
    const uint64_t need = 32ull + lrn + 4ull * nc + (((uint64_t)(uint32_t)ls + 1) >> 1) + (uint64_t)(uint32_t)ls;
    return (uint64_t)(uint32_t)bs >= need;
}

// The finder's test of position p (p + 36 <= end, staged): well-formed, refID and next_refID in [-1, n_ref), a name of printable
// bytes that ends in NUL -- as far as the name is staged and inside the piece.
__device__ __forceinline__ bool bam_plausible(const uint8_t *s, uint32_t a0, uint32_t p, uint32_t lim, int32_t n_ref, uint64_t *step)
{
    const uint32_t i = p - a0;
    if (!bam_wellformed(s, i, step)) return false;
    const int32_t ref = (int32_t)s_u32(s, i + 4), nref = (int32_t)s_u32(s, i + 24);
    if (ref < -1 || ref >= n_ref || nref < -1 || nref >= n_ref) return false;
    const uint32_t lrn = s_u8(s, i + 12);
    for (uint32_t j = 0; j < lrn; j++) {
        const uint32_t q = p + BAM_FIXED + j;
        if (q >= lim) break;                              // (not staged, or past the piece: not looked at)
        const uint32_t ch = s_u8(s, q - a0);
        if (j + 1 == lrn ? ch != 0 : (ch < 33 || ch > 126)) return false;
    }
    return true;
}

// The chain from `first` (inside the tile, or at or beyond its end: then nothing starts here) over the staged tile, by the whole
// wave in step (every LDS read is a broadcast).  Lane 0 lists the starts of the records that lie whole inside the piece.
__device__ __forceinline__ void bam_walk(const uint8_t *s, uint32_t a0, uint32_t first, uint32_t tile_end, uint32_t end, uint32_t list_cap,
                                         uint32_t *list, uint32_t *cnt_out, uint32_t *exit_out, uint32_t *status_out)
{
    uint32_t p = first, cnt = 0, status = BAM_ST_OK;
    for (uint32_t it = 0; it < list_cap; it++) {
        if (p >= tile_end) break;
        if ((uint64_t)p + BAM_FIXED > end) { status = BAM_ST_REST; break; }
        uint64_t step;
        if (!bam_wellformed(s, p - a0, &step)) { status = BAM_ST_BAD; break; }
        const uint64_t next = (uint64_t)p + step;
        if (next > end) { status = BAM_ST_REST; break; }
        if (threadIdx.x == 0) list[cnt] = p;
        cnt++;
        p = (uint32_t)next;
    }
    *cnt_out = cnt; *exit_out = p; *status_out = status;
}

__global__ void __launch_bounds__(64) phi_bam_tile_kernel(PhiBamArgs A)
{
    const uint32_t t = blockIdx.x;
    const uint32_t tile_begin = A.start + t * A.tile;                     // < end: the grid is ceil((end - start) / tile)
    const uint32_t tile_end = (uint32_t)min((uint64_t)tile_begin + A.tile, (uint64_t)A.end);
    const uint32_t stage_end = (uint32_t)min((uint64_t)tile_end + BAM_HALO, (uint64_t)A.end);
    const uint32_t a0 = tile_begin & ~15u;
    bam_stage(A.buf, a0, stage_end);
    const uint8_t *s = reinterpret_cast<const uint8_t *>(s_stage);
    uint32_t first = BAM_NONE;
    if (t == 0) first = A.start;                                           // the true chain's own position
    else {
        // candidates: positions of the tile whose fixed part lies inside the piece
        const uint32_t scan_end = (uint32_t)min((uint64_t)tile_end, (uint64_t)A.end - (BAM_FIXED - 1));    // (end - start >= 36: the host's business)
        for (uint32_t base = tile_begin; base < scan_end && first == BAM_NONE; base += 64) {
            const uint32_t p = base + threadIdx.x;
            bool ok = false;
            if (p < scan_end) {
                uint64_t step;
                ok = bam_plausible(s, a0, p, stage_end, A.n_ref, &step);
                // ... and the chain from it stays plausible for three more records, or up to the tile's end or the piece's
                uint64_t q = (uint64_t)p + step;
                for (int more = 0; ok && more < 3; more++) {
                    if (q >= tile_end || q + BAM_FIXED > A.end) break;
                    ok = bam_plausible(s, a0, (uint32_t)q, stage_end, A.n_ref, &step);
                    q += step;
                }
            }
            const unsigned long long m = __ballot(ok);
            if (m) first = base + (uint32_t)__ffsll((long long)m) - 1u;
        }
    }
    uint32_t cnt = 0, ex = 0, status = BAM_ST_OK;
    if (first != BAM_NONE) bam_walk(s, a0, first, tile_end, A.end, A.list_cap, A.t_list + (size_t)t * A.list_cap, &cnt, &ex, &status);
    if (threadIdx.x == 0) {
        A.t_first[t] = first; A.t_exit[t] = ex; A.t_status[t] = status; A.t_cnt[t] = (int32_t)cnt; A.t_skip[t] = 0;
        A.t_has[t] = first != BAM_NONE;
    }
}

// does tile t's chain go on exactly where the next tile that has a start begins?  (t_has_pre: exclusive prefix sums of t_has)
__global__ void __launch_bounds__(256) phi_bam_link_kernel(PhiBamArgs A)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= A.n_tiles || !A.t_has[t]) return;
    const int32_t after = A.t_has_pre[A.n_tiles] - A.t_has_pre[t + 1];    // tiles with a start behind t
    const uint32_t e = A.t_exit[t];
    bool ok;
    if (A.t_status[t] != BAM_ST_OK || (uint64_t)e + BAM_FIXED > A.end) ok = after == 0;      // the chain ends in t
    else {
        const uint32_t u = (e - A.start) / A.tile;                        // e < end: a tile of the grid, behind t
        ok = A.t_first[u] == e && A.t_has_pre[u] - A.t_has_pre[t + 1] == 0;
    }
    if (!ok) atomicMin(&A.sum->first_bad_tile, t);
    if (after == 0) A.sum->last_tile = t;                                 // (one tile only)
}

// From the first link that does not hold: the true chain tile by tile (one wave).
__global__ void __launch_bounds__(64) phi_bam_fix_kernel(PhiBamArgs A)
{
    const uint8_t *s = reinterpret_cast<const uint8_t *>(s_stage);
    uint32_t t = A.sum->first_bad_tile;
    uint32_t rewalked = 0;
    if (t == BAM_NONE) t = A.sum->last_tile;                              // every link holds: the chain ends in the last tile with a start
    else {
        uint32_t in = A.t_exit[t], st = A.t_status[t];
        for (uint32_t turn = 0; turn < A.n_tiles; turn++) {
            const bool ends = st != BAM_ST_OK || (uint64_t)in + BAM_FIXED > A.end;
            const uint32_t u = ends ? A.n_tiles : (in - A.start) / A.tile;      // the tile the chain enters (behind t: in >= t's end)
            for (uint32_t x = t + 1 + threadIdx.x; x < u; x += 64) A.t_has[x] = 0;      // passed over, or behind the chain's end
            if (ends) break;
            // `in` among u's starts?  (the first one, nearly always)
            uint32_t j = BAM_NONE;
            if (A.t_has[u]) {
                if (A.t_first[u] == in) j = 0;
                else {
                    const uint32_t n = (uint32_t)A.t_cnt[u];
                    const uint32_t *list = A.t_list + (size_t)u * A.list_cap;
                    for (uint32_t base = 0; base < n && j == BAM_NONE; base += 64) {
                        const uint32_t x = base + threadIdx.x;
                        const unsigned long long m = __ballot(x < n && list[x] == in);
                        if (m) j = base + (uint32_t)__ffsll((long long)m) - 1u;
                    }
                }
            }
            if (j != BAM_NONE) {
                if (threadIdx.x == 0) A.t_skip[u] = (int32_t)j;
                in = A.t_exit[u]; st = A.t_status[u];
            } else {
                const uint32_t tile_begin = A.start + u * A.tile;
                const uint32_t tile_end = (uint32_t)min((uint64_t)tile_begin + A.tile, (uint64_t)A.end);
                const uint32_t stage_end = (uint32_t)min((uint64_t)tile_end + BAM_HALO, (uint64_t)A.end);
                const uint32_t a0 = tile_begin & ~15u;
                __syncthreads();                                          // (the walk before has read the LDS)
                bam_stage(A.buf, a0, stage_end);
                uint32_t cnt, ex, status;
                bam_walk(s, a0, in, tile_end, A.end, A.list_cap, A.t_list + (size_t)u * A.list_cap, &cnt, &ex, &status);
                if (threadIdx.x == 0) {
                    A.t_first[u] = in; A.t_exit[u] = ex; A.t_status[u] = status; A.t_cnt[u] = (int32_t)cnt; A.t_skip[u] = 0; A.t_has[u] = 1;
                }
                rewalked++;
                in = ex; st = status;
            }
            t = u;
        }
    }
    if (threadIdx.x == 0) {
        // (t's entries were written before this kernel, or by this lane)
        const uint32_t e = A.t_exit[t], st = A.t_status[t];
        A.sum->rest_pos = e;
        A.sum->status = st == BAM_ST_BAD ? BAM_ST_BAD : e < A.end ? BAM_ST_REST : BAM_ST_OK;
        A.sum->tiles_rewalked = rewalked;
    }
}

// records a tile gives to the true chain
__global__ void __launch_bounds__(256) phi_bam_use_kernel(PhiBamArgs A)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= A.n_tiles) return;
    const bool has = A.t_has[t] != 0;
    A.t_use[t] = has ? A.t_cnt[t] - A.t_skip[t] : 0;
    if (has) atomicAdd(&A.sum->tiles_used, 1u);
}

// one wave per tile, a lane per record: its place, kept or not, the counters
__global__ void __launch_bounds__(64) phi_bam_records_kernel(PhiBamArgs A)
{
    const uint32_t t = blockIdx.x;
    const uint32_t n = (uint32_t)A.t_use[t], skip = (uint32_t)A.t_skip[t];
    const uint32_t r0 = (uint32_t)A.t_base[t];
    const uint32_t *list = A.t_list + (size_t)t * A.list_cap + skip;
    uint32_t n_secsup = 0, n_empty = 0, n_rev = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 64) {
        const uint32_t p = list[i];                                       // p + 36 <= end: listed by the walk
        const uint8_t *q = A.buf + p;
        const uint32_t flag = q[18] | (uint32_t)q[19] << 8;
        const uint32_t ls = q[20] | (uint32_t)q[21] << 8 | (uint32_t)q[22] << 16 | (uint32_t)q[23] << 24;
        const bool secsup = (flag & 0x900u) != 0, empty = ls == 0, keep = !secsup && !empty;
        n_secsup += secsup; n_empty += !secsup && empty; n_rev += keep && (flag & 0x10u);
        A.rec_pos[r0 + i] = p;
        A.rec_keep[r0 + i] = keep;
    }
    n_secsup = phi_wave_sum(n_secsup); n_empty = phi_wave_sum(n_empty); n_rev = phi_wave_sum(n_rev);
    if (threadIdx.x == 0) {
        if (n_secsup) atomicAdd(&A.sum->n_secsup, n_secsup);
        if (n_empty) atomicAdd(&A.sum->n_empty, n_empty);
        if (n_rev) atomicAdd(&A.sum->n_rev, n_rev);
    }
}

// per kept record: length, where the sequence starts, reverse; one length? (as phi_text_uniform_kernel)
__global__ void __launch_bounds__(256) phi_bam_kept_kernel(const uint8_t *__restrict__ buf, const uint32_t *__restrict__ rec_pos,
                                                           const int32_t *__restrict__ kidx, int64_t n_kept, int32_t *__restrict__ klen,
                                                           uint32_t *__restrict__ kseq, uint8_t *__restrict__ krev, PhiBamSummary *sum)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_kept) return;
    const uint8_t *q0 = buf + rec_pos[kidx[0]];
    const uint32_t len0 = q0[20] | (uint32_t)q0[21] << 8 | (uint32_t)q0[22] << 16 | (uint32_t)q0[23] << 24;
    const uint32_t p = rec_pos[kidx[j]];
    const uint8_t *q = buf + p;
    const uint32_t lrn = q[12], nc = q[16] | (uint32_t)q[17] << 8, flag = q[18] | (uint32_t)q[19] << 8;
    const uint32_t ls = q[20] | (uint32_t)q[21] << 8 | (uint32_t)q[22] << 16 | (uint32_t)q[23] << 24;
    klen[j] = (int32_t)ls;
    kseq[j] = p + BAM_FIXED + lrn + 4u * nc;                              // inside the record, which is inside the piece
    krev[j] = (flag & 0x10u) != 0;
    if (ls != len0) sum->not_uniform = 1;
}

// nibble -> ASCII: "=ACMGRSV" "TWYHKDBN", little-endian; the complement of a code is its four bits reversed
__device__ __forceinline__ uint32_t bam_base(uint32_t nib)
{
    const uint64_t lo = 0x565352474D43413Dull, hi = 0x4E42444B48595754ull;
    return (uint32_t)(((nib & 8u) ? hi : lo) >> (8u * (nib & 7u))) & 0xFFu;
}

__global__ void __launch_bounds__(256) phi_bam_decode_kernel(const uint8_t *__restrict__ buf, const int64_t *__restrict__ roff, int64_t n_kept,
                                                             const uint32_t *__restrict__ kseq, const uint8_t *__restrict__ krev,
                                                             uint8_t *__restrict__ bases)
{
    const int64_t n_out = roff[n_kept];
    const int lane = threadIdx.x & 63;
    int64_t o = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * BAM_DECODE_WAVE;
    if (o >= n_out) return;
    const int64_t o_end = min(n_out, o + (int64_t)BAM_DECODE_WAVE);
    int64_t lo = 0, hi = n_kept;                                          // the last record j with roff[j] <= o  (roff[n_kept] = n_out > o)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (roff[mid] <= o) lo = mid; else hi = mid;
    }
    int64_t j = lo;
    while (o < o_end && j < n_kept) {
        const int64_t b = roff[j], e = roff[j + 1];
        if (e <= o) { j++; continue; }
        const int64_t d = o - b, len = e - b, take = min(e - o, o_end - o);
        const uint8_t *src = buf + kseq[j];
        const bool rev = krev[j] != 0;
        for (int64_t x = lane; x < take; x += 64) {
            const int64_t at = rev ? len - 1 - (d + x) : d + x;          // the stored base this output base comes from
            const uint32_t byte = src[at >> 1];
            uint32_t nib = (at & 1) ? byte & 15u : byte >> 4;
            if (rev) nib = __brev(nib) >> 28;
            bases[o + x] = (uint8_t)bam_base(nib);
        }
        o += take;
        j++;
    }
}

}  // namespace

// ------------------------------------------------------------------ the stream
static int bam_fail(phi_ctx *c, int code, const char *fmt, long long off)
{
    c->bam.failed = true;
    return phi_fail(c, code, fmt, off);
}

// one piece of the record stream: m bytes at p (host memory) or at d_src (device memory)
static int bam_piece(phi_ctx *c, const void *p, const void *d_src, uint32_t m)
{
    auto &T = c->bam;
    T.dbg_reads = 0; T.dbg_bases = 0;
    const int slot = T.slot ^ 1;
    const uint32_t C = T.carry_cap, start = C - T.carry_len, end = C + m;
    uint8_t *buf = T.text[slot].as<uint8_t>();
    // the piece crosses the link on aux_stream, as the text stream's chunks do (reads_text: text_piece); everything else on `stream`
    HIPCHK(hipMemcpyAsync(buf + C, p ? p : d_src, m, p ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->aux_stream));
    HIPCHK(hipEventRecord(T.ev_copy, c->aux_stream));
    if (T.carry_len)
        HIPCHK(hipMemcpyAsync(buf + start, T.text[T.slot].as<uint8_t>() + T.carry_at, T.carry_len, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamWaitEvent(c->stream, T.ev_copy, 0));
    const int64_t off0 = T.fed - (int64_t)T.carry_len;                   // stream offset of buf[start]
    auto take_rest = [&](uint32_t rest_pos) -> int {
        const uint32_t tail = end - rest_pos;
        if (tail > C) return bam_fail(c, PHI_ERR_UNSUPPORTED, "BAM record at byte offset %lld of the inflated stream is longer than the stream's buffers (phi_reads_bam_begin: max_chunk_bytes)", (long long)(off0 + (rest_pos - start)));
        T.carry_len = tail; T.carry_at = rest_pos; T.slot = slot; T.fed += m;
        return PHI_OK;
    };
    if (end - start < BAM_FIXED) { HIPCHK(hipStreamSynchronize(c->stream)); return take_rest(start); }      // (p is borrowed for the call)

    PhiBamArgs A{};
    A.buf = buf; A.start = start; A.end = end; A.tile = T.tile; A.list_cap = T.list_cap; A.n_ref = T.n_ref;
    A.n_tiles = (uint32_t)(((uint64_t)(end - start) + T.tile - 1) / T.tile);
    A.t_first = T.t_first.as<uint32_t>(); A.t_exit = T.t_exit.as<uint32_t>(); A.t_status = T.t_status.as<uint32_t>(); A.t_list = T.t_list.as<uint32_t>();
    A.t_cnt = T.t_cnt.as<int32_t>(); A.t_skip = T.t_skip.as<int32_t>(); A.t_has = T.t_has.as<int32_t>(); A.t_has_pre = T.t_has_pre.as<int32_t>();
    A.t_use = T.t_use.as<int32_t>(); A.t_base = T.t_base.as<int32_t>();
    A.rec_pos = T.rec_pos.as<uint32_t>(); A.rec_keep = T.rec_keep.as<uint8_t>(); A.sum = T.sum.as<PhiBamSummary>();
    if (A.n_tiles > T.max_tiles) return phi_fail(c, PHI_ERR_INVALID, "phi_add_reads_bam: internal: %u tiles, tables of %u", A.n_tiles, T.max_tiles);
    const uint32_t lds = T.tile + BAM_HALO + 32;
    const uint32_t tb = (A.n_tiles + 255) / 256;
    HIPCHK(hipMemsetAsync(T.sum.p, 0, sizeof(PhiBamSummary), c->stream));
    HIPCHK(hipMemsetAsync(&T.sum.as<PhiBamSummary>()->first_bad_tile, 0xFF, 4, c->stream));
    hipLaunchKernelGGL(phi_bam_tile_kernel, dim3(A.n_tiles), dim3(64), lds, c->stream, A);
    PHICHK(phi_scan(c, A.t_has, (int64_t)A.n_tiles, A.t_has_pre));
    hipLaunchKernelGGL(phi_bam_link_kernel, dim3(tb), dim3(256), 0, c->stream, A);
    hipLaunchKernelGGL(phi_bam_fix_kernel, dim3(1), dim3(64), lds, c->stream, A);
    hipLaunchKernelGGL(phi_bam_use_kernel, dim3(tb), dim3(256), 0, c->stream, A);
    PHICHK(phi_scan(c, A.t_use, (int64_t)A.n_tiles, A.t_base));
    HIPCHK(hipGetLastError());
    PhiBamSummary *S = (PhiBamSummary *)T.h_sum;
    int32_t *h_nrec = (int32_t *)((char *)T.h_sum + sizeof(PhiBamSummary));
    int64_t *h_nbases = (int64_t *)((char *)T.h_sum + sizeof(PhiBamSummary) + 8);
    HIPCHK(hipMemcpyAsync(S, T.sum.p, sizeof(PhiBamSummary), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h_nrec, A.t_base + A.n_tiles, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (S->rest_pos < start || S->rest_pos > end || *h_nrec < 0 || (uint32_t)*h_nrec > T.max_rec)
        return bam_fail(c, PHI_ERR_DEVICE, "phi_add_reads_bam: internal: the chain's summary is out of range (piece at byte offset %lld)", (long long)off0);
    if (S->status == BAM_ST_BAD)
        return bam_fail(c, PHI_ERR_INVALID, "BAM record at byte offset %lld of the inflated stream is not well-formed (l_read_name >= 1, l_seq >= 0, block_size >= 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq)", (long long)(off0 + (S->rest_pos - start)));
    if (end - S->rest_pos > C) return take_rest(S->rest_pos);           // (refused: nothing of the piece is taken)
    const int64_t n_rec = *h_nrec;
    int64_t n_kept = 0, n_bases = 0;
    if (n_rec) {
        hipLaunchKernelGGL(phi_bam_records_kernel, dim3(A.n_tiles), dim3(64), 0, c->stream, A);
        PHICHK(phi_compact(c, A.rec_keep, n_rec, T.kidx, &n_kept));       // (waits)
    }
    if (n_kept) {
        hipLaunchKernelGGL(phi_bam_kept_kernel, dim3((unsigned)((n_kept + 255) / 256)), dim3(256), 0, c->stream, buf, A.rec_pos, T.kidx.as<int32_t>(),
                           n_kept, T.klen.as<int32_t>(), T.kseq.as<uint32_t>(), T.krev.as<uint8_t>(), A.sum);
        PHICHK(phi_scan(c, T.klen.as<int32_t>(), n_kept, T.roff.as<int64_t>()));
        // (a base takes half a byte of the piece at least: the grid covers whatever the offsets sum to)
        const uint64_t max_bases = 2ull * (end - start);
        const unsigned blocks = (unsigned)((max_bases + 4 * BAM_DECODE_WAVE - 1) / (4 * BAM_DECODE_WAVE));
        hipLaunchKernelGGL(phi_bam_decode_kernel, dim3(blocks), dim3(256), 0, c->stream, buf, T.roff.as<int64_t>(), n_kept, T.kseq.as<uint32_t>(),
                           T.krev.as<uint8_t>(), T.bases.as<uint8_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_nbases, T.roff.as<int64_t>() + n_kept, 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipMemcpyAsync(S, T.sum.p, sizeof(PhiBamSummary), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n_kept) n_bases = *h_nbases;
    if (n_bases < 0 || (uint64_t)n_bases > 2ull * (end - start))
        return bam_fail(c, PHI_ERR_DEVICE, "phi_add_reads_bam: internal: the decoded bases are out of range (piece at byte offset %lld)", (long long)off0);
    const uint32_t rest_pos = S->rest_pos;
    if (n_kept) {
        const int64_t len = n_bases / n_kept;
        const bool one = !S->not_uniform && n_bases % n_kept == 0;
        const bool uni = one && len >= 32;                                 // the sketch kernel computes the read starts, no offsets
        PHICHK(phi_score_resident_batch(c, T.bases.p, uni ? nullptr : T.roff.p, n_kept, n_bases));
        T.info.batches++; T.info.batches_without_offsets += uni;
        if (!one || (T.one_len >= 0 && T.one_len != len)) T.one_len = -2;
        else if (T.one_len == -1) T.one_len = len;
        T.dbg_reads = n_kept; T.dbg_bases = n_bases;
    }
    T.info.n_records += n_rec; T.info.n_kept += n_kept; T.info.n_bases += n_bases;
    T.info.n_secondary_supplementary += S->n_secsup; T.info.n_empty += S->n_empty; T.info.n_reverse += S->n_rev;
    T.info.tiles += A.n_tiles; T.info.tiles_rewalked += S->tiles_rewalked; T.info.tiles_confirmed += (int64_t)S->tiles_used - S->tiles_rewalked;
    return take_rest(rest_pos);
}

// the bytes of the record stream (the header is behind us), cut into pieces the buffers hold
static int bam_feed(phi_ctx *c, const unsigned char *p, const unsigned char *d_src, int64_t n)
{
    auto &T = c->bam;
    for (int64_t at = 0; at < n; ) {
        const uint32_t m = (uint32_t)std::min<int64_t>(n - at, T.chunk_cap);
        PHICHK(bam_piece(c, p ? p + at : nullptr, d_src ? d_src + at : nullptr, m));
        at += m;
    }
    return PHI_OK;
}

// the header from the bytes gathered so far: PHI_OK with header_done set or not (more bytes needed)
static int bam_try_header(phi_ctx *c, const unsigned char *b, int64_t n, int64_t *records_start)
{
    auto &T = c->bam;
    char err[160];
    int32_t n_ref = 0;
    const int r = phi_bam_header_parse(b, n, records_start, &n_ref, err, (int)sizeof err);
    if (r == PHI_BAM_HDR_BAD) { T.failed = true; return phi_fail(c, PHI_ERR_INVALID, "%s (inflated stream)", err); }
    if (r == PHI_BAM_HDR_MORE) {
        if (*records_start > ((int64_t)1 << 30)) { T.failed = true; return phi_fail(c, PHI_ERR_UNSUPPORTED, "BAM header of more than 1 GB (%lld bytes at least)", (long long)*records_start); }
        return PHI_OK;
    }
    T.header_done = true; T.n_ref = n_ref; T.fed = *records_start;
    T.info.n_ref = n_ref; T.info.header_bytes = *records_start;
    return PHI_OK;
}

static int bam_check_open(phi_ctx *c, const char *who)
{
    auto &T = c->bam;
    if (!T.active) return phi_fail(c, PHI_ERR_STATE, "%s before phi_reads_bam_begin", who);
    if (T.failed) return phi_fail(c, PHI_ERR_STATE, "%s on a BAM stream that has failed: end it and begin a new one", who);
    return PHI_OK;
}

static int bam_add_host(phi_ctx *c, const unsigned char *b, int64_t n)
{
    auto &T = c->bam;
    if (T.header_done) return bam_feed(c, b, nullptr, n);
    int64_t rs = 0;
    if (T.h_hdr.empty()) {
        // the usual case, the header inside the stream's first piece: parsed where the bytes lie, the records fed from there --
        // no byte of the piece is copied on the host
        PHICHK(bam_try_header(c, b, n, &rs));
        if (T.header_done) return rs < n ? bam_feed(c, b + rs, nullptr, n - rs) : PHI_OK;
    }
    // a header longer than the piece(s) so far: gathered on the host until it is whole (pieces inside the header only)
    const int64_t had = (int64_t)T.h_hdr.size();
    T.h_hdr.insert(T.h_hdr.end(), b, b + n);
    PHICHK(bam_try_header(c, T.h_hdr.data(), (int64_t)T.h_hdr.size(), &rs));
    if (!T.header_done) return PHI_OK;
    std::vector<unsigned char>().swap(T.h_hdr);
    const int64_t at = rs - had;                               // where the records start in this piece (the header ended in it)
    return at < n ? bam_feed(c, b + at, nullptr, n - at) : PHI_OK;
}

void phi_bam_drop(phi_ctx *c)
{
    auto &T = c->bam;
    DevBuf *all[] = {&T.text[0], &T.text[1], &T.bases, &T.roff, &T.sum, &T.t_first, &T.t_exit, &T.t_status, &T.t_cnt, &T.t_skip, &T.t_list, &T.t_has,
                     &T.t_has_pre, &T.t_use, &T.t_base, &T.rec_pos, &T.rec_keep, &T.kidx, &T.klen, &T.kseq, &T.krev};
    for (DevBuf *b : all) phi_dev_free(*b);
    if (T.h_sum) { (void)hipHostFree(T.h_sum); T.h_sum = nullptr; }
    if (T.ev_copy) { (void)hipEventDestroy(T.ev_copy); T.ev_copy = nullptr; }
    T.active = false;
}

extern "C" {

int phi_reads_bam_begin(phi_ctx *c, int64_t max_chunk_bytes, int64_t tile_bytes)
{
    if (!c) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_reads_bam_begin before phi_set_graph");
    if (max_chunk_bytes <= 0) return phi_fail(c, PHI_ERR_INVALID, "phi_reads_bam_begin: bad chunk size");
    if (tile_bytes <= 0) tile_bytes = BAM_TILE_DEFAULT;
    if (tile_bytes < 64 || tile_bytes > BAM_TILE_MAX) return phi_fail(c, PHI_ERR_INVALID, "phi_reads_bam_begin: tile_bytes %lld outside [64, %d]", (long long)tile_bytes, BAM_TILE_MAX);
    HIPCHK(hipSetDevice(c->device));
    PHICHK(phi_sync_check(c));                                // (batches handed over without a wait: their overflow shows here)
    c->rlog.async_batches = false;
    auto &T = c->bam;
    const uint32_t chunk = (uint32_t)std::min<int64_t>(std::max<int64_t>(max_chunk_bytes, 64), (int64_t)1 << 28);
    // the carry holds what a piece leaves unfinished: a record at most
    // (PHI_BAM_CARRY=bytes, INTEGRATION.md: tests of the refusal; 64 .. 2^30, so that carry + chunk stays below 2^32)
    const uint32_t carry = getenv("PHI_BAM_CARRY") ? (uint32_t)std::min<long long>(std::max<long long>(64, atoll(getenv("PHI_BAM_CARRY"))), 1ll << 30) & ~15u
                                                    : std::max<uint32_t>((chunk / 2) & ~15u, 1u << 24);
    const uint64_t bytes = (uint64_t)carry + chunk;
    T.tile = (uint32_t)tile_bytes;
    T.list_cap = T.tile / BAM_MIN_STEP + 2;
    T.max_tiles = (uint32_t)((bytes + T.tile - 1) / T.tile) + 1;
    T.max_rec = (uint32_t)(bytes / BAM_MIN_STEP) + 1;
    for (int i = 0; i < 2; i++) PHICHK(phi_dev_ensure(c, T.text[i], (size_t)bytes + 64));
    PHICHK(phi_dev_ensure(c, T.bases, 2 * (size_t)bytes + 64));
    PHICHK(phi_dev_ensure(c, T.roff, ((size_t)T.max_rec + 2) * 8));
    PHICHK(phi_dev_ensure(c, T.sum, sizeof(PhiBamSummary)));
    DevBuf *per_tile[] = {&T.t_first, &T.t_exit, &T.t_status, &T.t_cnt, &T.t_skip, &T.t_has, &T.t_has_pre, &T.t_use, &T.t_base};
    for (DevBuf *b : per_tile) PHICHK(phi_dev_ensure(c, *b, ((size_t)T.max_tiles + 2) * 4));
    PHICHK(phi_dev_ensure(c, T.t_list, (size_t)T.max_tiles * T.list_cap * 4));
    PHICHK(phi_dev_ensure(c, T.rec_pos, ((size_t)T.max_rec + 2) * 4));
    PHICHK(phi_dev_ensure(c, T.rec_keep, (size_t)T.max_rec + 2));
    PHICHK(phi_dev_ensure(c, T.klen, ((size_t)T.max_rec + 2) * 4));
    PHICHK(phi_dev_ensure(c, T.kseq, ((size_t)T.max_rec + 2) * 4));
    PHICHK(phi_dev_ensure(c, T.krev, (size_t)T.max_rec + 2));
    if (!T.h_sum) HIPCHK(hipHostMalloc(&T.h_sum, sizeof(PhiBamSummary) + 64, hipHostMallocDefault));
    if (!T.ev_copy) HIPCHK(hipEventCreateWithFlags(&T.ev_copy, hipEventDisableTiming));
    T.carry_cap = carry; T.chunk_cap = chunk;
    T.active = true; T.failed = false; T.header_done = false; T.n_ref = 0;
    T.h_hdr.clear(); T.fed = 0; T.slot = 0; T.carry_len = 0; T.carry_at = carry; T.one_len = -1; T.dbg_reads = T.dbg_bases = 0;
    memset(&T.info, 0, sizeof T.info);
    return PHI_OK;
}

int phi_add_reads_bam(phi_ctx *c, const void *bytes, int64_t n)
{
    if (!c) return PHI_ERR_INVALID;
    if (n < 0 || (n > 0 && !bytes)) return phi_fail(c, PHI_ERR_INVALID, "phi_add_reads_bam: bad arguments");
    PHICHK(bam_check_open(c, "phi_add_reads_bam"));
    c->bam.dbg_reads = c->bam.dbg_bases = 0;
    if (n == 0) return PHI_OK;
    HIPCHK(hipSetDevice(c->device));
    return bam_add_host(c, (const unsigned char *)bytes, n);
}

int phi_add_reads_bam_parked(phi_ctx *c, phi_text_park *park, int32_t index)
{
    if (!c) return PHI_ERR_INVALID;
    PHICHK(bam_check_open(c, "phi_add_reads_bam_parked"));
    const void *d = nullptr;
    int64_t n = 0;
    if (phi_text_park_piece_dev(park, index, c->device, &d, &n) != PHI_OK) return phi_fail(c, PHI_ERR_INVALID, "phi_add_reads_bam_parked: no such piece on this context's device");
    HIPCHK(hipSetDevice(c->device));
    auto &T = c->bam;
    T.dbg_reads = T.dbg_bases = 0;
    const unsigned char *dp = (const unsigned char *)d;
    if (T.header_done) return bam_feed(c, nullptr, dp, n);
    std::vector<unsigned char> h;
    if (T.h_hdr.empty()) {
        // the stream's first piece: the header from a prefix fetched to the host, the records from where they lie
        for (int64_t k = std::min<int64_t>(n, 1 << 16);;) {
            h.resize((size_t)k);
            HIPCHK(phi_copy_sync(c, h.data(), dp, (size_t)k, hipMemcpyDeviceToHost));
            int64_t rs = 0;
            PHICHK(bam_try_header(c, h.data(), k, &rs));
            if (T.header_done) return rs < n ? bam_feed(c, nullptr, dp + rs, n - rs) : PHI_OK;
            if (k == n) break;
            k = std::min<int64_t>(n, std::max<int64_t>(2 * k, rs));
        }
    } else {
        h.resize((size_t)n);
        HIPCHK(phi_copy_sync(c, h.data(), dp, (size_t)n, hipMemcpyDeviceToHost));
    }
    return bam_add_host(c, h.data(), n);                                   // (a header longer than the piece: gathered on the host)
}

int phi_reads_bam_end(phi_ctx *c, phi_bam_info *info)
{
    if (!c) return PHI_ERR_INVALID;
    auto &T = c->bam;
    if (info) memset(info, 0, sizeof *info);
    if (!T.active) return phi_fail(c, PHI_ERR_STATE, "phi_reads_bam_end before phi_reads_bam_begin");
    T.active = false;
    T.info.one_length = T.one_len > 0 && T.one_len <= 0x7FFFFFFF ? (int32_t)T.one_len : 0;
    if (info) *info = T.info;
    if (T.failed) return PHI_ERR_STATE;                        // (phi_last_error still says why it failed)
    if (!T.header_done)
        return phi_fail(c, PHI_ERR_INVALID, "BAM stream ends inside its header at byte offset %lld of the inflated stream", (long long)T.h_hdr.size());
    if (T.carry_len)
        return phi_fail(c, PHI_ERR_INVALID, "BAM stream ends inside the record that begins at byte offset %lld of the inflated stream (%lld bytes of it are there)",
                        (long long)(T.fed - (int64_t)T.carry_len), (long long)T.carry_len);
    return PHI_OK;
}

int phi_reads_bam_last_batch(phi_ctx *c, char *bases, int64_t cap_bases, int64_t *off, int64_t cap_reads, int64_t *n_reads, int64_t *n_bases)
{
    if (!c || !n_reads || !n_bases) return PHI_ERR_INVALID;
    auto &T = c->bam;
    *n_reads = T.dbg_reads; *n_bases = T.dbg_bases;
    if (T.dbg_reads == 0 || cap_reads < T.dbg_reads || cap_bases < T.dbg_bases || !off) return PHI_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (T.dbg_bases && bases) HIPCHK(phi_copy_sync(c, bases, T.bases.p, (size_t)T.dbg_bases, hipMemcpyDeviceToHost));
    HIPCHK(phi_copy_sync(c, off, T.roff.p, (size_t)(T.dbg_reads + 1) * 8, hipMemcpyDeviceToHost));
    return PHI_OK;
}

}  // extern "C"
