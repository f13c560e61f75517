// deflate.hip -- BGZF written on the GPU: every run of PHI_BGZF_BLOCK input bytes becomes one gzip member, compressed by one
// workgroup with nothing shared between blocks.
//
// One workgroup of 256 threads per block; the block's bytes stay in LDS from the first phase to the last:
//   1. MATCH    a table of 2^14 entries keyed by a hash of four bytes holds the latest position of every key.  Positions are
//               taken in tiles of 256, one per thread: every thread reads its key's entry, then (after a barrier) all of them
//               enter their position with atomicMax.  An entry read is therefore the latest position of that key IN AN EARLIER
//               TILE -- a function of the input, whatever order the threads ran in.  Nearer copies, inside the tile, are
//               looked for directly at distances 1..4 (runs, short periods).  Every candidate is verified against the bytes,
//               four at a time, and the longest copy (at least 4, at most 255 bytes, distance at most 32768) of each position
//               goes to a scratch word per position in device memory.
//   2. PARSE    thread i owns the segment [255 i, 255 i + 255): a greedy walk, a copy where the position has one (cut at the
//               segment's end: that is what removes the serial walk over the block) and the copy is cheaper than its bytes as
//               literals, priced by the code the block would have with every byte a literal; a literal otherwise.  The token of every
//               visited position goes to a byte per position in LDS (where the table was), the symbols into histograms in LDS.
//   3. CODES    two lanes build the literal/length and the distance code from the histograms, one then builds the code-length
//               code over their run-length coded lengths (deflate_codes.h: the same functions the CPU selftest calls).
//   4. SIZES    every thread adds up the bits of its segment's tokens; the workgroup scan (phi_wave.h) gives every segment
//               its bit offset and the block its size.  A block whose dynamic form is not smaller than 5 + n bytes is stored.
//   5. BITS     the member's deflate area in device memory is zeroed, then every thread ORs its segment's bits into it, whole
//               32-bit words at a time (the words at a segment's ends are shared with its neighbours: atomicOr).
//   6. FRAME    CRC32 per segment from the bytes in LDS, shifted to the block's end (a multiplication modulo the CRC's
//               polynomial) and XORed together; BGZF header and trailer.
// A second, tiny pass scans the members' sizes into file offsets and gathers the members to their places.
// No workgroup waits on another; every loop is bounded by the block size (tiles, segment length, copy length, alphabet sizes).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "../../include/phi_amd.h"
#include "phi_ctx.h"
#include "phi_wave.h"
#include "dev_run.h"
#include "deflate_codes.h"

#define DFL_T 256                       // threads per workgroup = positions per tile = segments per block
#define DFL_SEG 255                     // bytes per segment: no copy is longer
#define DFL_HASH_BITS 14
#define DFL_MIN_COPY 4                  // the key is four bytes
#define DFL_NEAR 4                      // distances looked for directly
#define DFL_HDR 18                      // BGZF member header
#define DFL_MEMBER_AT 2                 // a member starts here in its slot: its deflate data is then 4-byte aligned
#define DFL_SLOT 65344                  // bytes of staging per block: 2 + 18 + 5 + 65280 + 8 and the last word's slack, rounded to 64
#define DFL_BATCH_MAX 4096
static_assert(DFL_T * DFL_SEG == PHI_BGZF_BLOCK, "one segment per thread covers the block");
static_assert(DFL_MEMBER_AT + DFL_HDR + 5 + PHI_BGZF_BLOCK + 8 + 4 <= DFL_SLOT && DFL_SLOT % 64 == 0, "slot");
static_assert(DFL_HDR + 5 + PHI_BGZF_BLOCK + 8 <= 65536, "BSIZE fits 16 bits");

namespace {

struct DflBlockStat { int32_t size, stored, matches, match_bytes; };

struct DflLds {
    uint32_t in[PHI_BGZF_BLOCK / 4 + 8];            // the block's bytes, zeros behind them
    union {
        uint32_t tab[1 << DFL_HASH_BITS];           // phase 1: position + 1 of the latest entry, 0 = none
        uint8_t tok[PHI_BGZF_BLOCK];                // from phase 2: 1 = a literal, 4..255 = a copy of that length (at visited positions)
    };
    uint32_t hist_lit[DFL_MAX_SYMS], hist_dist[32], hist_cl[20];
    uint32_t hist_pre[256];                         // every byte of the block as a literal: the price list of the parse
    uint8_t len_pre[256];
    uint16_t code_lit[DFL_MAX_SYMS], code_dist[32], code_cl[20];
    uint8_t len_lit[DFL_MAX_SYMS], len_dist[32], len_cl[20];
    uint8_t seq[DFL_NLIT + DFL_NDIST + 4];          // the code lengths sent: literal/length, then distance
    uint8_t cl_sym[DFL_NLIT + DFL_NDIST + 4], cl_extra[DFL_NLIT + DFL_NDIST + 4];
    DflWork work[2];
    uint32_t crc_tab[256];
    int32_t s_w[DFL_T / 64];
    int32_t hlit, hdist, hclen, ncl, hdr_bits;
    int32_t matches, match_bytes;
    uint32_t crc;
};

__constant__ uint8_t c_dfl_clord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t dfl_load4(const uint32_t *in, int p)
{
    const uint64_t w = ((uint64_t)in[(p >> 2) + 1] << 32) | in[p >> 2];
    return (uint32_t)(w >> (8 * (p & 3)));
}
__device__ __forceinline__ uint32_t dfl_byte(const uint32_t *in, int p) { return (in[p >> 2] >> (8 * (p & 3))) & 0xffu; }
__device__ __forceinline__ uint32_t dfl_hash(uint32_t v) { return (v * 2654435761u) >> (32 - DFL_HASH_BITS); }

// the bytes at p and q agree in their first four: how many agree, at most maxlen (at most 63 turns)
__device__ __forceinline__ int dfl_extend(const uint32_t *in, int p, int q, int maxlen)
{
    int l = 4;
    for (; l < maxlen; l += 4) {
        const uint32_t x = dfl_load4(in, p + l) ^ dfl_load4(in, q + l);
        if (x) { l += (__ffs((int)x) - 1) >> 3; break; }
    }
    return l < maxlen ? l : maxlen;
}

// Whether a copy is cheaper than its bytes as literals.  The literals are priced by the code of the block with every byte a
// literal (len_pre), the first DFL_PRICED of them exactly and one bit -- the least a literal can cost -- for each one beyond; the
// copy by the fixed code's lengths (7 bits for the length symbol, 5 for the distance symbol) and its extra bits.  Without
// this, text of high entropy per byte (DNA: 2 bits a base) pays 20 bits for copies of four bases worth 8.
#define DFL_PRICED 32
__device__ __forceinline__ bool dfl_copy_pays(const uint32_t *in, const uint8_t *len_pre, int p, int len, int dist)
{
    int ne, ex, cost = 7 + 5;
    (void)dfl_length_symbol(len, &ne, &ex);
    cost += ne;
    (void)dfl_dist_symbol(dist, &ne, &ex);
    cost += ne;
    const int priced = len < DFL_PRICED ? len : DFL_PRICED;
    int lit = len - priced;
    for (int k = 0; k < priced; k++) lit += len_pre[dfl_byte(in, p + k)];
    return lit > cost;
}

// bits ORed into a zeroed image of 32-bit words, least significant first; at most 32 bits a call
struct DflBits {
    uint32_t *img;
    uint32_t word;
    int fill;
    uint64_t acc;
    __device__ void start(uint32_t *image, uint32_t bitpos) { img = image; word = bitpos >> 5; fill = (int)(bitpos & 31); acc = 0; }
    __device__ void put(uint32_t v, int n)
    {
        acc |= (uint64_t)v << fill;
        fill += n;
        if (fill >= 32) {
            atomicOr(&img[word++], (uint32_t)acc);
            acc >>= 32;
            fill -= 32;
        }
    }
    __device__ void finish() { if (fill > 0 && (uint32_t)acc) atomicOr(&img[word], (uint32_t)acc); }
};

// in: the batch's bytes (4-byte aligned, readable up to the next multiple of 4); res: PHI_BGZF_BLOCK words of scratch per block
// (unused with no_match); stage: DFL_SLOT bytes per block, where the finished member is left at DFL_MEMBER_AT
__global__ void __launch_bounds__(DFL_T) phi_deflate_block_kernel(const uint8_t *__restrict__ in, int64_t n_bytes, uint32_t *__restrict__ res_all,
                                                                  uint8_t *__restrict__ stage, DflBlockStat *__restrict__ stat, int no_match)
{
    __shared__ DflLds L;
    const int tid = (int)threadIdx.x;
    const int64_t blk = blockIdx.x;
    const int64_t at = blk * PHI_BGZF_BLOCK;
    const int N = (int)(n_bytes - at < PHI_BGZF_BLOCK ? n_bytes - at : PHI_BGZF_BLOCK);      // 1 .. PHI_BGZF_BLOCK
    uint32_t *res = res_all + (no_match ? 0 : at);
    uint8_t *slot = stage + blk * DFL_SLOT;

    // ---- 0. the block into LDS, zeros behind its last byte whatever the memory holds there
    {
        const uint32_t *g = (const uint32_t *)(in + at);
        for (int w = tid; w < PHI_BGZF_BLOCK / 4 + 8; w += DFL_T) {
            const int nv = N - 4 * w;
            uint32_t v = 0;
            if (nv > 0) {
                v = g[w];
                if (nv < 4) v &= (1u << (8 * nv)) - 1u;
            }
            L.in[w] = v;
        }
        for (int i = tid; i < DFL_MAX_SYMS; i += DFL_T) L.hist_lit[i] = 0;
        L.hist_pre[tid] = 0;
        if (tid < 32) L.hist_dist[tid] = 0;
        {
            uint32_t c = (uint32_t)tid;                         // dfl_crc_byte, written out: the call compiles to other code
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ (DFL_CRC_POLY & (0u - (c & 1u)));
            L.crc_tab[tid] = c;
        }
        if (tid == 0) { L.matches = 0; L.match_bytes = 0; L.crc = 0; }
        if (!no_match)
            for (int i = tid; i < (1 << DFL_HASH_BITS); i += DFL_T) L.tab[i] = 0;
    }
    __syncthreads();

    // ---- 1. the longest verified copy of every position
    if (!no_match) {
        const int ntiles = (N + DFL_T - 1) / DFL_T;
        for (int t = 0; t < ntiles; t++) {
            const int p = t * DFL_T + tid;
            const bool can = p + DFL_MIN_COPY <= N;
            uint32_t v = 0, h = 0;
            int best = 0, best_d = 0;
            if (can) {
                v = dfl_load4(L.in, p);
                h = dfl_hash(v);
                const int maxlen = N - p < DFL_SEG ? N - p : DFL_SEG;
#pragma unroll
                for (int d = 1; d <= DFL_NEAR; d++)
                    if (p >= d && dfl_load4(L.in, p - d) == v) {
                        const int l = dfl_extend(L.in, p, p - d, maxlen);
                        if (l > best) { best = l; best_d = d; }
                    }
                const uint32_t c = L.tab[h];
                if (c) {
                    const int q = (int)c - 1, d = p - q;
                    if (d <= DFL_WINDOW && dfl_load4(L.in, q) == v) {
                        const int l = dfl_extend(L.in, p, q, maxlen);
                        if (l > best) { best = l; best_d = d; }
                    }
                }
            }
            if (p < N) res[p] = best >= DFL_MIN_COPY ? (uint32_t)best | ((uint32_t)(best_d - 1) << 16) : 0u;
            __syncthreads();                                    // every read of this tile before any entry of this tile
            if (can) atomicMax(&L.tab[h], (uint32_t)p + 1u);
            __syncthreads();
        }
        __threadfence();                                        // res is read by other threads of the workgroup below
        __syncthreads();
    }

    // ---- 2. the parse of this thread's segment
    const int s0 = tid * DFL_SEG, s1 = s0 + DFL_SEG < N ? s0 + DFL_SEG : N;
    if (!no_match) {                                            // what a byte costs as a literal when every byte is one
        for (int p = s0; p < s1; p++) atomicAdd(&L.hist_pre[dfl_byte(L.in, p)], 1u);
        __syncthreads();
        if (tid == 0) dfl_build_lengths(L.hist_pre, 256, 15, L.len_pre, &L.work[0]);
        __syncthreads();
    }
    {
        int nm = 0, mb = 0;
        for (int p = s0; p < s1;) {
            const uint32_t r = no_match ? 0u : res[p];
            int len = (int)(r & 0xffffu);
            if (len > s1 - p) len = s1 - p;
            if (len >= DFL_MIN_COPY && dfl_copy_pays(L.in, L.len_pre, p, len, (int)(r >> 16) + 1)) {
                int ne, ex;
                L.tok[p] = (uint8_t)len;
                atomicAdd(&L.hist_lit[dfl_length_symbol(len, &ne, &ex)], 1u);
                atomicAdd(&L.hist_dist[dfl_dist_symbol((int)(r >> 16) + 1, &ne, &ex)], 1u);
                nm++;
                mb += len;
                p += len;
            } else {
                L.tok[p] = 1;
                atomicAdd(&L.hist_lit[dfl_byte(L.in, p)], 1u);
                p++;
            }
        }
        if (nm) { atomicAdd(&L.matches, nm); atomicAdd(&L.match_bytes, mb); }
        if (tid == 0) L.hist_lit[256] = 1;                      // (nobody else counts end-of-block)
    }
    __syncthreads();

    // ---- 3. the three codes
    if (tid == 0) dfl_build_lengths(L.hist_lit, DFL_NLIT, 15, L.len_lit, &L.work[0]);
    if (tid == 64) dfl_build_lengths(L.hist_dist, DFL_NDIST, 15, L.len_dist, &L.work[1]);
    __syncthreads();
    if (tid == 0) {
        int hlit = DFL_NLIT, hdist = DFL_NDIST;
        while (hlit > 257 && !L.len_lit[hlit - 1]) hlit--;
        while (hdist > 1 && !L.len_dist[hdist - 1]) hdist--;    // (no copy at all: one distance code of length 0)
        for (int s = 0; s < hlit; s++) L.seq[s] = L.len_lit[s];
        for (int s = 0; s < hdist; s++) L.seq[hlit + s] = L.len_dist[s];
        const int ncl = dfl_rle_lengths(L.seq, hlit + hdist, L.cl_sym, L.cl_extra);
        for (int s = 0; s < 20; s++) L.hist_cl[s] = 0;
        for (int k = 0; k < ncl; k++) L.hist_cl[L.cl_sym[k]]++;
        int used = 0;
        for (int s = 0; s < DFL_NCL; s++) used += L.hist_cl[s] != 0;
        if (used < 2) L.hist_cl[L.hist_cl[0] ? 1 : 0] = 1;      // a complete code-length code needs two codes
        dfl_build_lengths(L.hist_cl, DFL_NCL, 7, L.len_cl, &L.work[0]);
        int hclen = DFL_NCL;
        while (hclen > 4 && !L.len_cl[c_dfl_clord[hclen - 1]]) hclen--;
        int bits = 3 + 5 + 5 + 4 + 3 * hclen;
        for (int k = 0; k < ncl; k++) bits += L.len_cl[L.cl_sym[k]] + dfl_cl_extra_bits(L.cl_sym[k]);
        dfl_canonical_codes(L.len_lit, DFL_NLIT, L.code_lit);
        dfl_canonical_codes(L.len_cl, DFL_NCL, L.code_cl);
        L.hlit = hlit; L.hdist = hdist; L.hclen = hclen; L.ncl = ncl; L.hdr_bits = bits;
    }
    if (tid == 64) dfl_canonical_codes(L.len_dist, DFL_NDIST, L.code_dist);
    __syncthreads();

    // ---- 4. sizes
    int my_bits = 0;
    for (int p = s0; p < s1;) {
        const int t = L.tok[p];
        if (t == 1) { my_bits += L.len_lit[dfl_byte(L.in, p)]; p++; }
        else {
            int ne, ex;
            my_bits += L.len_lit[dfl_length_symbol(t, &ne, &ex)] + ne;
            my_bits += L.len_dist[dfl_dist_symbol((int)(res[p] >> 16) + 1, &ne, &ex)] + ne;
            p += t;
        }
    }
    int tok_bits = 0;
    const int my_off = phi_block_excl_scan<DFL_T / 64>(my_bits, L.s_w, &tok_bits);
    const int total_bits = L.hdr_bits + tok_bits + L.len_lit[256];
    const int dyn_bytes = (total_bits + 7) >> 3;
    const bool stored = dyn_bytes >= N + 5;
    const int body = stored ? N + 5 : dyn_bytes;
    uint8_t *mem = slot + DFL_MEMBER_AT, *dfl = mem + DFL_HDR;

    // ---- 5. the deflate data
    if (stored) {
        if (tid == 0) {
            dfl[0] = 1;                                          // BFINAL, BTYPE 00, padding
            dfl[1] = (uint8_t)(N & 255); dfl[2] = (uint8_t)(N >> 8);
            dfl[3] = (uint8_t)(~N & 255); dfl[4] = (uint8_t)((~N >> 8) & 255);
        }
        for (int p = tid; p < N; p += DFL_T) dfl[5 + p] = (uint8_t)dfl_byte(L.in, p);
    } else {
        uint32_t *img = (uint32_t *)dfl;
        const int nwords = (dyn_bytes + 3) >> 2;
        for (int w = tid; w < nwords; w += DFL_T) img[w] = 0;
        __threadfence();
        __syncthreads();
        DflBits b;
        if (tid == 0) {
            b.start(img, 0);
            b.put(1, 1);                                         // BFINAL
            b.put(2, 2);                                         // dynamic
            b.put((uint32_t)(L.hlit - 257), 5);
            b.put((uint32_t)(L.hdist - 1), 5);
            b.put((uint32_t)(L.hclen - 4), 4);
            for (int k = 0; k < L.hclen; k++) b.put(L.len_cl[c_dfl_clord[k]], 3);
            for (int k = 0; k < L.ncl; k++) {
                const int s = L.cl_sym[k];
                b.put(L.code_cl[s], L.len_cl[s]);
                if (s >= 16) b.put(L.cl_extra[k], dfl_cl_extra_bits(s));
            }
            b.finish();
            b.start(img, (uint32_t)(L.hdr_bits + tok_bits));
            b.put(L.code_lit[256], L.len_lit[256]);
            b.finish();
        }
        b.start(img, (uint32_t)(L.hdr_bits + my_off));
        for (int p = s0; p < s1;) {
            const int t = L.tok[p];
            if (t == 1) {
                const uint32_t c = dfl_byte(L.in, p);
                b.put(L.code_lit[c], L.len_lit[c]);
                p++;
            } else {
                int ne, ex;
                const int ls = dfl_length_symbol(t, &ne, &ex);
                b.put(L.code_lit[ls], L.len_lit[ls]);
                b.put((uint32_t)ex, ne);
                const int ds = dfl_dist_symbol((int)(res[p] >> 16) + 1, &ne, &ex);
                b.put(L.code_dist[ds], L.len_dist[ds]);
                b.put((uint32_t)ex, ne);
                p += t;
            }
        }
        b.finish();
    }

    // ---- 6. CRC32 of the block, header, trailer
    if (s0 < s1) {
        uint32_t c = 0;
        for (int p = s0; p < s1; p++) c = L.crc_tab[(c ^ dfl_byte(L.in, p)) & 0xffu] ^ (c >> 8);
        atomicXor(&L.crc, dfl_crc_shift(c, (uint32_t)(N - s1)));
    }
    __threadfence();                                            // the trailer's bytes share a word with the last bits
    __syncthreads();
    if (tid == 0) {
        const uint32_t crc = L.crc ^ dfl_crc_shift(0xffffffffu, (uint32_t)N) ^ 0xffffffffu;
        const int size = DFL_HDR + body + 8, bsize = size - 1;
        const uint8_t hdr[DFL_HDR] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 255), (uint8_t)(bsize >> 8)};
        for (int k = 0; k < DFL_HDR; k++) mem[k] = hdr[k];
        uint8_t *tr = dfl + body;
        for (int k = 0; k < 4; k++) { tr[k] = (uint8_t)(crc >> (8 * k)); tr[4 + k] = (uint8_t)((uint32_t)N >> (8 * k)); }
        stat[blk] = DflBlockStat{size, stored ? 1 : 0, stored ? 0 : L.matches, stored ? 0 : L.match_bytes};
    }
}

// off[0..nb] = the exclusive prefix sums of the members' sizes: one workgroup, tiles of 1024
__global__ void __launch_bounds__(1024) phi_deflate_offsets_kernel(const DflBlockStat *__restrict__ stat, int nb, int64_t *__restrict__ off)
{
    __shared__ int64_t s_w[16];
    int64_t carry = 0;
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const int64_t v = i < nb ? stat[i].size : 0;
        int64_t tile;
        const int64_t e = phi_block_excl_scan<16>(v, s_w, &tile);
        if (i < nb) off[i] = carry + e;
        carry += tile;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[nb] = carry;
}

__global__ void __launch_bounds__(256) phi_deflate_gather_kernel(const uint8_t *__restrict__ stage, const DflBlockStat *__restrict__ stat,
                                                                 const int64_t *__restrict__ off, uint8_t *__restrict__ out)
{
    const uint8_t *src = stage + (int64_t)blockIdx.x * DFL_SLOT + DFL_MEMBER_AT;
    uint8_t *dst = out + off[blockIdx.x];
    const int size = stat[blockIdx.x].size;
    for (int i = (int)threadIdx.x; i < size; i += 256) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------ host

const uint8_t BGZF_EOF[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

int64_t batch_blocks()
{
    const char *e = getenv("PHI_DEFLATE_BATCH");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? std::min<long long>(v, DFL_BATCH_MAX) : PHI_DEFLATE_BATCH_DEFAULT;
}

int64_t n_blocks(int64_t n) { return (n + PHI_BGZF_BLOCK - 1) / PHI_BGZF_BLOCK; }

int check_args(const void *in, int64_t n, int32_t flags, int64_t *out_size, phi_deflate_info *info)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!out_size || n < 0 || (n > 0 && !in)) return fail(info, PHI_ERR_INVALID, "phi_deflate_bgzf: null pointer or negative size");
    if (flags & ~(PHI_DEFLATE_NO_MATCH | PHI_DEFLATE_NO_EOF)) return fail(info, PHI_ERR_INVALID, "phi_deflate_bgzf: unknown flags 0x%x", (unsigned)flags);
    *out_size = 0;
    return PHI_OK;
}

// the whole file into dst[0, phi_deflate_bgzf_bound(n)) on the host; *out_size = its bytes (arguments checked by the caller).
// d_src (may be null): the same n bytes already on the device, 64 readable bytes behind them -- the batches then read their
// blocks there and nothing is uploaded.  member_off (may be null) receives off[0..blocks]: where every member begins in the
// file, and where the EOF block does (bgzf_index.hip; phi_deflate_run below)
int deflate_run(int32_t device, const uint8_t *src, int64_t n, int32_t flags, uint8_t *dst, int64_t *out_size, phi_deflate_info *info,
                const uint8_t *d_src = nullptr, std::vector<int64_t> *member_off = nullptr)
{
    const int64_t nb_all = n_blocks(n);
    int64_t total = 0;
    if (info) { info->in_bytes = n; info->blocks = nb_all; }
    if (nb_all > 0) {
        Dev dev;
        if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return fail(info, PHI_ERR_DEVICE, "phi_deflate_bgzf: no device %d", device); }
        DCHK(hipStreamCreateWithFlags(&dev.st, hipStreamNonBlocking));
        DCHK(hipEventCreate(&dev.ev[0]));
        DCHK(hipEventCreate(&dev.ev[1]));
        hipStream_t st = dev.st;
        const int64_t B = std::min(batch_blocks(), nb_all);
        const bool no_match = (flags & PHI_DEFLATE_NO_MATCH) != 0;
        DALLOC(d_in, uint8_t, d_src ? 16 : (size_t)B * PHI_BGZF_BLOCK + 64);
        DALLOC(d_res, uint32_t, no_match ? 16 : (size_t)B * PHI_BGZF_BLOCK * 4);
        DALLOC(d_stage, uint8_t, (size_t)B * DFL_SLOT);
        DALLOC(d_stat, DflBlockStat, (size_t)B * sizeof(DflBlockStat));
        DALLOC(d_off, int64_t, (size_t)(B + 1) * 8);
        DALLOC(d_out, uint8_t, (size_t)B * (PHI_BGZF_BLOCK + 31));
        std::vector<DflBlockStat> stat((size_t)B);
        for (int64_t b0 = 0; b0 < nb_all; b0 += B) {
            const int nb = (int)std::min(B, nb_all - b0);
            const int64_t at = b0 * PHI_BGZF_BLOCK, bytes = std::min<int64_t>(n - at, (int64_t)nb * PHI_BGZF_BLOCK);
            if (!d_src) DCHK(hipMemcpyAsync(d_in, src + at, (size_t)bytes, hipMemcpyHostToDevice, st));
            DCHK(hipEventRecord(dev.ev[0], st));
            hipLaunchKernelGGL(phi_deflate_block_kernel, dim3((unsigned)nb), dim3(DFL_T), 0, st, d_src ? d_src + at : d_in, bytes, d_res, d_stage, d_stat, no_match ? 1 : 0);
            DCHK(hipGetLastError());
            hipLaunchKernelGGL(phi_deflate_offsets_kernel, dim3(1), dim3(1024), 0, st, d_stat, nb, d_off);
            DCHK(hipGetLastError());
            hipLaunchKernelGGL(phi_deflate_gather_kernel, dim3((unsigned)nb), dim3(256), 0, st, d_stage, d_stat, d_off, d_out);
            DCHK(hipGetLastError());
            DCHK(hipEventRecord(dev.ev[1], st));
            int64_t got = 0;
            DCHK(hipMemcpyAsync(&got, d_off + nb, 8, hipMemcpyDeviceToHost, st));
            DCHK(hipMemcpyAsync(stat.data(), d_stat, (size_t)nb * sizeof(DflBlockStat), hipMemcpyDeviceToHost, st));
            DCHK(hipStreamSynchronize(st));
            if (got < (int64_t)nb * (DFL_HDR + 8) || got > (int64_t)nb * (PHI_BGZF_BLOCK + 31))
                return fail(info, PHI_ERR_DEVICE, "phi_deflate_bgzf: %d blocks came back as %lld bytes (internal error)", nb, (long long)got);
            DCHK(hipMemcpyAsync(dst + total, d_out, (size_t)got, hipMemcpyDeviceToHost, st));
            DCHK(hipStreamSynchronize(st));
            if (member_off) {
                int64_t o = total;
                for (int b = 0; b < nb; b++) { member_off->push_back(o); o += stat[(size_t)b].size; }
            }
            total += got;
            if (info) {
                float ms = 0;
                (void)hipEventElapsedTime(&ms, dev.ev[0], dev.ev[1]);
                info->device_ms += ms;
                for (int b = 0; b < nb; b++) {
                    info->stored_blocks += stat[(size_t)b].stored;
                    info->matches += stat[(size_t)b].matches;
                    info->match_bytes += stat[(size_t)b].match_bytes;
                }
            }
        }
    }
    if (member_off) member_off->push_back(total);
    if (!(flags & PHI_DEFLATE_NO_EOF)) { memcpy(dst + total, BGZF_EOF, sizeof BGZF_EOF); total += (int64_t)sizeof BGZF_EOF; }
    if (info) info->out_bytes = total;
    *out_size = total;
    return PHI_OK;
}

}  // namespace

int phi_deflate_run(int32_t device, const uint8_t *src, const uint8_t *d_src, int64_t n, int32_t flags, uint8_t *dst, int64_t *out_size,
                    phi_deflate_info *info, std::vector<int64_t> *member_off)
{
    if (info) memset(info, 0, sizeof(*info));
    if (member_off) member_off->clear();
    *out_size = 0;
    return deflate_run(device, src, n, flags, dst, out_size, info, d_src, member_off);
}

extern "C" {

int64_t phi_deflate_bgzf_bound(int64_t n)
{
    if (n < 0) n = 0;
    return n + n_blocks(n) * (DFL_HDR + 5 + 8) + (int64_t)sizeof BGZF_EOF;
}

int phi_deflate_bgzf(int32_t device, const void *in, int64_t n, void *out, int64_t cap, int32_t flags, int64_t *out_size, phi_deflate_info *info)
{
    int rc = check_args(in, n, flags, out_size, info);
    if (rc) return rc;
    if (cap < 0 || (cap > 0 && !out)) return fail(info, PHI_ERR_INVALID, "phi_deflate_bgzf: null output or negative capacity");
    const int64_t bound = phi_deflate_bgzf_bound(n);
    if (cap >= bound) return deflate_run(device, (const uint8_t *)in, n, flags, (uint8_t *)out, out_size, info);
    uint8_t *tmp = (uint8_t *)malloc((size_t)bound);             // the size is known only at the end: nothing reaches out[] unless all of it fits
    if (!tmp) return fail(info, PHI_ERR_NOMEM, "phi_deflate_bgzf: %lld bytes of host memory", (long long)bound);
    rc = deflate_run(device, (const uint8_t *)in, n, flags, tmp, out_size, info);
    if (!rc && cap >= *out_size && *out_size > 0) memcpy(out, tmp, (size_t)*out_size);
    free(tmp);
    return rc;
}

int phi_deflate_bgzf_alloc(int32_t device, const void *in, int64_t n, int32_t flags, void **out, int64_t *out_size, phi_deflate_info *info)
{
    if (out) *out = nullptr;
    int rc = check_args(in, n, flags, out_size, info);
    if (rc) return rc;
    if (!out) return fail(info, PHI_ERR_INVALID, "phi_deflate_bgzf_alloc: null output");
    const int64_t bound = phi_deflate_bgzf_bound(n);
    uint8_t *h = (uint8_t *)malloc((size_t)bound);
    if (!h) return fail(info, PHI_ERR_NOMEM, "phi_deflate_bgzf_alloc: %lld bytes of host memory", (long long)bound);
    rc = deflate_run(device, (const uint8_t *)in, n, flags, h, out_size, info);
    if (rc) { free(h); return rc; }
    *out = h;
    return PHI_OK;
}

void phi_deflate_free(void *p) { free(p); }

}  // extern "C"
