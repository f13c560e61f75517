// inflate.hip -- gzip (RFC 1952) / DEFLATE (RFC 1951) inflated on the GPU, one stream cut into chunks decoded in parallel.
//
// Scheme:
//   - The compressed bytes are cut into chunks of C bytes.  Chunk 0 starts at the first member's deflate data; for every
//     other chunk the FINDER searches the chunk's bit offsets for the start of a non-final block: a dynamic-Huffman header
//     (HLIT <= 286, HDIST <= 30, complete code-length code, complete literal/length code with a coded end-of-block,
//     complete or single-code distance code) or a stored block (zero padding, LEN == ~NLEN).  64 lanes test 64 offsets
//     side by side; the lowest offset that then decodes a whole block without error, followed by a plausible block
//     header (final and fixed-Huffman allowed), is the chunk's start.
//   - The DECODER of a chunk inflates from its start without the 32 KB window before it: it writes 16-bit symbols, a
//     byte (< 256) or a MARKER 256 + j meaning "byte j of the 32 KB before this piece's first output byte".  It keeps
//     decoding past its chunk until, at a block boundary, it stands exactly on the start another chunk's decoder began
//     at (or the stream ends).  Starting from chunk 0, that relation gives the CHAIN of decoders that began at true block
//     boundaries: every other decoder's output is dropped, and a chunk whose start was missing or false has its range
//     decoded by its predecessor.  Nothing depends on the finder being right: with no starts at all, decoder 0 inflates
//     the whole stream.
//   - Resolution: the last 32 KB of each piece, in chain order (one workgroup, one step per piece), then every marker of
//     every piece in parallel; the bytes land in one contiguous output.
//   - Members: after a final block the decoder reads the trailer (CRC32, ISIZE) and the next member's header, and goes
//     on.  A distance reaching before the member's first byte is an error, inside a piece on the device and across
//     pieces at resolution.  CRC32 per 4 KB segment on the device, combined per member on the host by the GF(2) shift.
//
// This file: the kernels, and the host side as stages over one InfRun (upload, find, decode, redecode, layout and resolve,
// CRC and check, info) that hold launches and copies only.  What both sides share -- records, status values, the gzip
// header parser -- and every host rule between the launches is plain code in inflate_host.h, checked on the CPU by
// host/inflate_host_selftest.cpp; the stream, events and buffers of a run are dev_run.h's.
//
// Mapping: one decoder per wave (64-thread workgroup), its state wave-uniform; the Huffman tables of the block in LDS
// (10-bit first level, canonical decoding beyond); literals written by lane 0, match copies and stored blocks by all lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "../../include/phi_amd.h"
#include "phi_ctx.h"
#include "dev_run.h"
#include "inflate_host.h"

#define INF_TB 10               // first-level table bits of the literal/length and distance codes

namespace {

// ------------------------------------------------------------------------------------------------ device

__constant__ uint16_t c_lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
                                     131, 163, 195, 227, 258};
__constant__ uint8_t c_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t c_dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
                                     2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t c_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t c_clord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};


struct InfTables {
    uint16_t lit[1 << INF_TB], dst[1 << INF_TB];    // (symbol << 4) | length; 0: longer than INF_TB bits, or no code
    uint16_t lsort[320], dsort[32];                 // symbols by (length, symbol)
    uint16_t lcount[16], dcount[16];
    uint16_t offs[16], first[16];
    uint8_t lens[320];
    uint8_t clen[20];
    int32_t fixed;                                   // the tables hold the fixed code
};

// wave-uniform LSB-first bit reader over 32-bit words (the input is padded so reads a few words past the end are safe)
struct Br {
    const uint32_t *w;
    uint64_t bb;
    int64_t wp;
    int nb;
    __device__ void fill()
    {
        if (nb <= 32) { bb |= (uint64_t)w[wp] << nb; wp++; nb += 32; }
    }
    __device__ void at(int64_t p)
    {
        wp = p >> 5;
        const int s = (int)(p & 31);
        bb = w[wp] >> s;
        nb = 32 - s;
        wp++;
        fill();
    }
    __device__ int64_t pos() const { return wp * 32 - nb; }
    __device__ uint32_t peek(int n) const { return (uint32_t)bb & ((1u << n) - 1u); }
    __device__ void drop(int n) { bb >>= n; nb -= n; }
    __device__ uint32_t get(int n) { const uint32_t v = peek(n); drop(n); return v; }
};

// decoder output: symbols written while they fit, counted always
struct Out {
    uint16_t *sym;
    int64_t o, cap, ms;         // ms: first output position of the current member in this piece (negative: before it)
    bool wr;
};

// canonical code of len[0, n) into a first-level table of tb bits; returns the Kraft remainder (< 0: oversubscribed),
// *mx the longest length.  Every lane of the (one-wave) workgroup calls it.
__device__ int inf_build(const uint8_t *len, int n, uint16_t *tab, int tb, uint16_t *count, uint16_t *sorted,
                         uint16_t *offs, uint16_t *first, int *mx)
{
    const int lane = threadIdx.x;
    for (int e = lane; e < (1 << tb); e += 64) tab[e] = 0;
    if (lane < 16) {
        int c = 0;
        if (lane > 0)
            for (int s = 0; s < n; s++) c += (len[s] == lane);
        count[lane] = (uint16_t)c;
    }
    __syncthreads();
    int left = 1, m = 0, total = 0;
    for (int l = 1; l < 16; l++) {
        left = (left << 1) - count[l];
        if (count[l]) m = l;
        total += count[l];
        if (left < 0) break;
    }
    *mx = m;
    if (left < 0) return left;
    if (lane < 16) {
        int off = 0, code = 0;
        for (int l = 1; l <= lane; l++) {
            code = (code + count[l - 1]) << 1;
            if (l < lane) off += count[l];
        }
        offs[lane] = (uint16_t)off;
        first[lane] = (uint16_t)code;
    }
    __syncthreads();
    if (lane >= 1 && lane < 16) {
        int idx = offs[lane];
        for (int s = 0; s < n; s++)
            if (len[s] == lane) sorted[idx++] = (uint16_t)s;
    }
    __syncthreads();
    for (int k = lane; k < total; k += 64) {
        const int sym = sorted[k], l = len[sym];
        if (l > tb) continue;
        const uint32_t code = first[l] + (k - offs[l]);
        const uint32_t rev = __brev(code) >> (32 - l);
        for (uint32_t r = rev; r < (1u << tb); r += 1u << l) tab[r] = (uint16_t)((sym << 4) | l);
    }
    __syncthreads();
    return left;
}

// one symbol; -1 when the bits are no code
__device__ inline int inf_sym(Br &r, const uint16_t *tab, int tb, const uint16_t *count, const uint16_t *sorted)
{
    r.fill();
    const uint32_t e = tab[r.peek(tb)];
    if (e) { r.drop(e & 15); return (int)(e >> 4); }
    const uint32_t bits = r.peek(15);
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; l++) {
        code |= (bits >> (l - 1)) & 1;
        const int cnt = count[l];
        if (code < first + cnt) { r.drop(l); return sorted[index + code - first]; }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

__device__ bool inf_code_ok(int left, int mx) { return left == 0 || (left > 0 && mx <= 1); }

// the block at the reader's position.  0: a non-final block ended, 1: the final block ended, < 0: error.
__device__ int inf_block(Br &r, int64_t nbits, InfTables &t, Out &out)
{
    const int lane = threadIdx.x;
    r.fill();
    const uint32_t h = r.get(3);
    const int bfinal = h & 1, type = h >> 1;
    if (type == 0) {
        const int64_t p = (r.pos() + 7) & ~(int64_t)7;
        if (p + 32 > nbits) return INF_E_TRUNC;
        r.at(p);
        const uint32_t len = r.get(16), nlen = r.get(16);
        if (len != (~nlen & 0xffffu)) return INF_E_BLOCK;
        const int64_t bp = p / 8 + 4;
        if ((bp + len) * 8 > nbits) return INF_E_TRUNC;
        if (out.o + len > out.cap) out.wr = false;
        if (out.wr) {
            const uint8_t *in8 = (const uint8_t *)r.w;
            for (int64_t k = lane; k < len; k += 64) out.sym[out.o + k] = in8[bp + k];
        }
        out.o += len;
        r.at((bp + len) * 8);
        return bfinal;
    }
    if (type == 3) return INF_E_BLOCK;
    int mx;
    if (type == 1) {
        if (!t.fixed) {
            for (int s = lane; s < 320; s += 64) t.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
            __syncthreads();
            inf_build(t.lens, 288, t.lit, INF_TB, t.lcount, t.lsort, t.offs, t.first, &mx);
            inf_build(t.lens + 288, 32, t.dst, INF_TB, t.dcount, t.dsort, t.offs, t.first, &mx);
            t.fixed = 1;
        }
    } else {
        t.fixed = 0;
        r.fill();
        const int hlit = r.get(5) + 257, hdist = r.get(5) + 1, hclen = r.get(4) + 4;
        if (hlit > 286 || hdist > 30) return INF_E_BLOCK;
        if (lane < 20) t.clen[lane] = 0;
        __syncthreads();
        for (int k = 0; k < hclen; k++) {
            r.fill();
            const uint8_t v = (uint8_t)r.get(3);
            if (lane == 0) t.clen[c_clord[k]] = v;
        }
        __syncthreads();
        if (inf_build(t.clen, 19, t.lit, 7, t.lcount, t.lsort, t.offs, t.first, &mx) != 0) return INF_E_BLOCK;
        const int n = hlit + hdist;
        for (int i = 0; i < n;) {
            const int sym = inf_sym(r, t.lit, 7, t.lcount, t.lsort);
            if (sym < 0) return INF_E_BLOCK;
            if (sym < 16) {
                if (lane == 0) t.lens[i] = (uint8_t)sym;
                i++;
            } else {
                r.fill();
                int l = 0, rep;
                if (sym == 16) {
                    if (i == 0) return INF_E_BLOCK;
                    l = t.lens[i - 1];
                    rep = 3 + r.get(2);
                } else if (sym == 17) {
                    rep = 3 + r.get(3);
                } else {
                    rep = 11 + r.get(7);
                }
                if (i + rep > n) return INF_E_BLOCK;
                for (int k = lane; k < rep; k += 64) t.lens[i + k] = (uint8_t)l;
                i += rep;
            }
            __syncthreads();
            if (r.pos() > nbits) return INF_E_TRUNC;
        }
        if (t.lens[256] == 0) return INF_E_BLOCK;
        if (!inf_code_ok(inf_build(t.lens, hlit, t.lit, INF_TB, t.lcount, t.lsort, t.offs, t.first, &mx), mx)) return INF_E_BLOCK;
        if (!inf_code_ok(inf_build(t.lens + hlit, hdist, t.dst, INF_TB, t.dcount, t.dsort, t.offs, t.first, &mx), mx)) return INF_E_BLOCK;
    }
    for (;;) {
        if (r.pos() > nbits) return INF_E_TRUNC;
        int sym = inf_sym(r, t.lit, INF_TB, t.lcount, t.lsort);
        if (sym < 0) return INF_E_CODE;
        if (sym < 256) {
            if (out.o >= out.cap) out.wr = false;
            if (out.wr && lane == 0) out.sym[out.o] = (uint16_t)sym;
            out.o++;
            continue;
        }
        if (sym == 256) break;
        sym -= 257;
        if (sym >= 29) return INF_E_CODE;
        r.fill();
        const int len = c_lbase[sym] + (int)r.get(c_lext[sym]);
        const int ds = inf_sym(r, t.dst, INF_TB, t.dcount, t.dsort);
        if (ds < 0 || ds >= 30) return INF_E_CODE;
        r.fill();
        const int dist = c_dbase[ds] + (int)r.get(c_dext[ds]);
        if (out.o - dist < out.ms) return INF_E_DIST;
        if (out.o + len > out.cap) out.wr = false;
        if (out.wr) {
            // The source symbols were stored by this wave: literals by lane 0 alone, copies by any lane.  One wave's vector
            // memory operations reach memory in program order (gfx9: one in-order queue per wave, a write-through L1), so the
            // loads below see those stores; the wavefront-scope fence keeps the compiler from moving a load above them.
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const int64_t o = out.o;
            for (int k = lane; k < len; k += 64) {
                const int64_t s = o - dist + (dist >= len ? k : k % dist);
                out.sym[o + k] = s >= 0 ? out.sym[s] : (uint16_t)(256 + INF_WIN + s);
            }
        }
        out.o += len;
    }
    if (r.pos() > nbits) return INF_E_TRUNC;
    return bfinal;
}

// a lane's cheap test of one bit offset (no LDS tables: the per-lane scratch `sc` holds 19 + 8 + 19 + 16 + 16 entries)
__device__ inline uint32_t inf_bits(const uint32_t *w, int64_t p, int n)
{
    const uint64_t v = ((uint64_t)w[(p >> 5) + 1] << 32) | w[p >> 5];
    return (uint32_t)(v >> (p & 31)) & ((1u << n) - 1u);
}

// the header after a candidate's block (final and fixed-Huffman allowed): a stored block's LEN == ~NLEN, a dynamic
// block's HLIT, HDIST and complete code-length code
__device__ bool inf_next_ok(const uint32_t *w, int64_t nbits, int64_t p)
{
    if (p + 3 > nbits) return false;
    const uint32_t t = inf_bits(w, p, 3) >> 1;
    if (t == 1) return true;
    if (t == 0) {
        const int64_t q = (p + 3 + 7) & ~(int64_t)7;
        return q + 32 <= nbits && inf_bits(w, q, 16) == (~inf_bits(w, q + 16, 16) & 0xffffu);
    }
    if (t == 3 || p + 17 > nbits) return false;
    const int hclen = inf_bits(w, p + 13, 4) + 4;
    if (inf_bits(w, p + 3, 5) + 257 > 286 || inf_bits(w, p + 8, 5) + 1 > 30 || p + 17 + 3 * hclen > nbits) return false;
    uint32_t kraft = 0;
    for (int k = 0; k < hclen; k++) {
        const uint32_t l = inf_bits(w, p + 17 + 3 * k, 3);
        if (l) kraft += 128u >> l;
    }
    return kraft == 128;
}

__device__ bool inf_plausible(const uint32_t *w, int64_t nbits, int64_t p, uint16_t *sc)
{
    if (p + 17 > nbits) return false;
    const uint32_t h = inf_bits(w, p, 3);
    if (h & 1) return false;
    if ((h >> 1) == 0) {
        const int64_t q = (p + 3 + 7) & ~(int64_t)7;
        if (q + 32 > nbits) return false;
        if (q > p + 3 && inf_bits(w, p + 3, (int)(q - p - 3)) != 0) return false;
        const uint32_t len = inf_bits(w, q, 16), nlen = inf_bits(w, q + 16, 16);
        return len == (~nlen & 0xffffu) && q + 32 + 8 * (int64_t)len <= nbits;
    }
    if ((h >> 1) != 2) return false;
    const int hlit = inf_bits(w, p + 3, 5) + 257, hdist = inf_bits(w, p + 8, 5) + 1, hclen = inf_bits(w, p + 13, 4) + 4;
    if (hlit > 286 || hdist > 30) return false;
    int64_t q = p + 17 + 3 * hclen;
    if (q > nbits) return false;
    uint16_t *cl = sc, *cc = sc + 19, *cs = sc + 27, *lc = sc + 46, *dc = sc + 62;
    for (int k = 0; k < 19; k++) cl[k] = 0;
    for (int k = 0; k < 8; k++) cc[k] = 0;
    for (int k = 0; k < 16; k++) { lc[k] = 0; dc[k] = 0; }
    for (int k = 0; k < hclen; k++) cl[c_clord[k]] = inf_bits(w, p + 17 + 3 * k, 3);
    for (int k = 0; k < 19; k++) cc[cl[k]]++;
    int left = 1;
    for (int l = 1; l < 8; l++) {
        left = (left << 1) - cc[l];
        if (left < 0) return false;
    }
    if (left != 0) return false;
    {
        int idx = 0;
        for (int l = 1; l < 8; l++)
            for (int k = 0; k < 19; k++)
                if (cl[k] == l) cs[idx++] = k;
    }
    const int n = hlit + hdist;
    int prev = -1, eob = 0;
    for (int i = 0; i < n;) {
        if (q + 14 > nbits) return false;
        const uint32_t bits = inf_bits(w, q, 7);
        int code = 0, first = 0, index = 0, sym = -1;
        for (int l = 1; l < 8; l++) {
            code |= (bits >> (l - 1)) & 1;
            if (code < first + cc[l]) { sym = cs[index + code - first]; q += l; break; }
            index += cc[l];
            first = (first + cc[l]) << 1;
            code <<= 1;
        }
        if (sym < 0) return false;
        int l, rep;
        if (sym < 16) { l = sym; rep = 1; }
        else if (sym == 16) { if (prev < 0) return false; l = prev; rep = 3 + inf_bits(w, q, 2); q += 2; }
        else if (sym == 17) { l = 0; rep = 3 + inf_bits(w, q, 3); q += 3; }
        else { l = 0; rep = 11 + inf_bits(w, q, 7); q += 7; }
        if (i + rep > n) return false;
        prev = l;
        for (int k = 0; k < rep; k++, i++) {
            if (i < hlit) { lc[l]++; if (i == 256) eob = l; }
            else dc[l]++;
        }
    }
    if (!eob) return false;
    int ll = 1, dl = 1, dn = 0, dm = 0;
    for (int l = 1; l < 16; l++) {
        ll = (ll << 1) - lc[l];
        dl = (dl << 1) - dc[l];
        if (ll < 0 || dl < 0) return false;
        dn += dc[l];
        if (dc[l]) dm = l;
    }
    return ll == 0 && (dl == 0 || (dn == 1 && dm == 1));
}

__global__ void __launch_bounds__(64) phi_inflate_find_kernel(const uint32_t *__restrict__ in, int64_t nbits, int64_t chunk_bits,
                                                              int64_t *__restrict__ starts)
{
    __shared__ InfTables t;
    __shared__ uint16_t scratch[64][80];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x + 1;
    const int64_t lo = i * chunk_bits, hi = min(lo + chunk_bits, nbits);
    if (lane == 0) t.fixed = 0;
    __syncthreads();
    int64_t found = -1;
    for (int64_t base = lo; base < hi && found < 0; base += 64) {
        const int64_t c = base + lane;
        const bool ok = c < hi && inf_plausible(in, nbits, c, scratch[lane]);
        uint64_t m = __ballot(ok);
        while (m) {
            const int l = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            Br r;
            r.w = in;
            r.at(base + l);
            Out out{nullptr, 0, 0, -INF_WIN, false};
            if (inf_block(r, nbits, t, out) == 0 && inf_next_ok(in, nbits, r.pos())) { found = base + l; break; }
        }
    }
    if (lane == 0) starts[i] = found;
}

__global__ void __launch_bounds__(64) phi_inflate_decode_kernel(const uint32_t *__restrict__ in, int64_t nbytes,
                                                                const int64_t *__restrict__ starts, int32_t nch,
                                                                const InfJob *__restrict__ jobs, InfResult *__restrict__ res,
                                                                InfMember *__restrict__ mem, int32_t *__restrict__ n_mem,
                                                                int32_t mem_cap)
{
    __shared__ InfTables t;
    const int lane = threadIdx.x;
    const InfJob job = jobs[blockIdx.x];
    const int64_t nbits = nbytes * 8;
    const uint8_t *in8 = (const uint8_t *)in;
    if (lane == 0) t.fixed = 0;
    __syncthreads();
    Br r;
    r.w = in;
    r.at(job.start);
    Out out{job.sym, 0, job.cap, job.chunk == 0 ? 0 : -INF_WIN, true};
    int j = job.chunk + 1, status, end_chunk = nch;
    for (;;) {
        const int64_t p = r.pos();
        while (j < nch && starts[j] < p) j++;
        if (j < nch && starts[j] == p) { end_chunk = j; status = INF_STOP; break; }
        const int rc = inf_block(r, nbits, t, out);
        if (rc < 0) { status = rc; break; }
        if (rc == 1) {
            int64_t bp = (r.pos() + 7) >> 3;
            if (bp + 8 > nbytes) { status = INF_E_TRUNC; break; }
            const uint32_t crc = in8[bp] | (in8[bp + 1] << 8) | (in8[bp + 2] << 16) | ((uint32_t)in8[bp + 3] << 24);
            const uint32_t isz = in8[bp + 4] | (in8[bp + 5] << 8) | (in8[bp + 6] << 16) | ((uint32_t)in8[bp + 7] << 24);
            if (mem && lane == 0) {
                const int idx = atomicAdd(n_mem, 1);
                if (idx < mem_cap) mem[idx] = InfMember{(int32_t)blockIdx.x, 0, out.o, crc, isz};
            }
            bp += 8;
            if (bp == nbytes) { status = INF_END; break; }
            const int64_t q = inf_gz_header(in8, nbytes, bp);
            if (q < 0) { status = q == -2 ? INF_E_TRUNC : INF_E_HEADER; break; }
            r.at(q * 8);
            out.ms = out.o;
        }
    }
    if (lane == 0) res[blockIdx.x] = InfResult{out.o, r.pos(), end_chunk, status, out.wr ? 0 : 1, 0};
}

__device__ inline bool inf_resolve(const InfPiece &pc, int64_t k, uint8_t *out, int *markers)
{
    const uint16_t v = pc.sym[k];
    if (v < 256) { out[pc.abs + k] = (uint8_t)v; return true; }
    const int64_t a = pc.abs - INF_WIN + (v - 256);
    if (a < pc.lo) return false;
    out[pc.abs + k] = out[a];
    (*markers)++;
    return true;
}

// the last 32 KB of every piece, in stream order: one workgroup, one step per piece
__global__ void __launch_bounds__(1024) phi_inflate_tail_kernel(const InfPiece *__restrict__ pieces, int32_t np, uint8_t *out,
                                                                unsigned long long *markers, int32_t *err)
{
    int mk = 0;
    bool ok = true;
    for (int p = 0; p < np; p++) {
        const InfPiece pc = pieces[p];
        for (int64_t k = max((int64_t)0, pc.len - INF_WIN) + threadIdx.x; k < pc.len; k += blockDim.x) ok &= inf_resolve(pc, k, out, &mk);
        __syncthreads();
    }
    if (!ok) atomicExch(err, 1);
    if (mk) atomicAdd(markers, (unsigned long long)mk);
}

// everything before each piece's last 32 KB, in parallel
__global__ void __launch_bounds__(256) phi_inflate_resolve_kernel(const InfPiece *__restrict__ pieces, const InfSlab *__restrict__ slabs,
                                                                  uint8_t *out, unsigned long long *markers, int32_t *err)
{
    const InfSlab sl = slabs[blockIdx.x];
    const InfPiece pc = pieces[sl.piece];
    int mk = 0;
    bool ok = true;
    for (int64_t k = sl.k0 + threadIdx.x; k < sl.k1; k += blockDim.x) ok &= inf_resolve(pc, k, out, &mk);
    if (!ok) atomicExch(err, 1);
    if (mk) atomicAdd(markers, (unsigned long long)mk);
}

// CRC32 of each segment, zero initial value and no final inversion (so that segments combine linearly)
__global__ void __launch_bounds__(256) phi_inflate_crc_kernel(const uint8_t *__restrict__ out, const InfSeg *__restrict__ segs,
                                                              int64_t nseg, uint32_t *__restrict__ crc)
{
    __shared__ uint32_t tab[256];
    {
        uint32_t c = threadIdx.x;                               // dfl_crc_byte, written out: the call compiles to other code
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (DFL_CRC_POLY & (0u - (c & 1u)));
        tab[threadIdx.x] = c;
    }
    __syncthreads();
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    const InfSeg sg = segs[s];
    uint32_t c = 0;
    for (int64_t k = 0; k < sg.len; k++) c = tab[(c ^ out[sg.off + k]) & 0xffu] ^ (c >> 8);
    crc[s] = c;
}

// ------------------------------------------------------------------------------------------------ host

// One inflate, from the compressed bytes on the host to the checked text in one of dev's buffers, as stages: each is
// launches and copies, and between them the rules of inflate_host.h.  Every host vector a copy reads or fills lives here,
// for the whole run.
struct InfRun {
    Dev &dev;
    phi_inflate_info *info;
    const uint8_t *src;
    int64_t n;
    int32_t flags;
    int64_t hdr = 0;                                            // byte offset of the first member's deflate data
    const int64_t *known = nullptr;                             // (may be null) byte offsets where deflate data begins, ascending: members whose
    int64_t n_known = 0;                                        // bounds the caller knows (BGZF); they stand in for the finder
    int64_t cap_hint = 0;                                       // with them: symbols a decoder may write on its first run, at the least
    InfChunks ck{};
    hipStream_t st = nullptr;
    uint32_t *d_in = nullptr;
    int64_t *d_starts = nullptr;
    InfMember *d_mem = nullptr;
    uint8_t *d_out = nullptr;
    unsigned long long *d_stat = nullptr, stat[2] = {0, 0};     // [0] marker bytes, [1] a distance reached before its member
    std::vector<int64_t> starts;
    std::vector<int> job_of, chunk_of, chain;
    std::vector<InfJob> jobs, jobs2;                            // (2: the second run)
    std::vector<InfResult> res, res2;
    int32_t nmem = 0;
    std::vector<InfMember> mem;
    std::vector<InfPiece> pieces;
    std::vector<InfEnd> ends;
    int64_t total = 0;
    std::vector<InfSlab> slabs;
    std::vector<InfSeg> segs;
    std::vector<uint32_t> crcs;
    InfErr err;

    int refused() { return fail(info, err.code, "%s", err.text); }
    int upload(int32_t device);
    int find();
    int run_decoders(const std::vector<InfJob> &js, InfMember *d_m, int32_t *d_nm, int32_t mem_cap, std::vector<InfResult> &out);
    int decode();
    int redecode();
    int layout_resolve();
    int crc_check();
    void fill_info();
};

int InfRun::upload(int32_t device)
{
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return fail(info, PHI_ERR_DEVICE, "phi_inflate: no device %d", device); }
    DCHK(hipStreamCreateWithFlags(&dev.st, hipStreamNonBlocking));
    DCHK(hipEventCreate(&dev.ev[0]));
    DCHK(hipEventCreate(&dev.ev[1]));
    st = dev.st;
    const size_t in_pad = (((size_t)n + 3) & ~(size_t)3) + 256;
    DALLOC(p, uint32_t, in_pad);
    d_in = p;
    DCHK(hipMemsetAsync(d_in, 0, in_pad, st));
    DCHK(hipMemcpyAsync(d_in, src, (size_t)n, hipMemcpyHostToDevice, st));
    DCHK(hipEventRecord(dev.ev[0], st));
    return PHI_OK;
}

// 1. the finder: a start for every chunk but the first, -1 where it found none
int InfRun::find()
{
    const int nch = ck.nch;
    DALLOC(p, int64_t, (size_t)nch * 8);
    d_starts = p;
    starts.assign((size_t)nch, -1);
    starts[0] = hdr * 8;
    if (known) {
        // A member of one final block has no start the finder takes (it looks for a block that is not the last, followed by a
        // plausible one), so a BGZF file of such members would be decoded by one decoder.  A chunk's start is then the first
        // known one that lies in it; the decoders and the chain treat it as a found one
        for (int64_t k = 0; k < n_known; k++) {
            const int64_t c = known[k] / ck.C;
            if (known[k] > hdr && known[k] < n && c >= 1 && c < nch && starts[(size_t)c] < 0) starts[(size_t)c] = known[k] * 8;
        }
    }
    DCHK(hipMemcpyAsync(d_starts, starts.data(), (size_t)nch * 8, hipMemcpyHostToDevice, st));
    if (nch > 1 && !known && !(flags & PHI_INFLATE_NO_FINDER)) {
        hipLaunchKernelGGL(phi_inflate_find_kernel, dim3(nch - 1), dim3(64), 0, st, d_in, n * 8, ck.C * 8, d_starts);
        DCHK(hipGetLastError());
        DCHK(hipMemcpyAsync(starts.data(), d_starts, (size_t)nch * 8, hipMemcpyDeviceToHost, st));
        DCHK(hipStreamSynchronize(st));
        starts[0] = hdr * 8;
    }
    return PHI_OK;
}

// the jobs js through the decode kernel; their results are in `out` once the stream is synchronised
int InfRun::run_decoders(const std::vector<InfJob> &js, InfMember *d_m, int32_t *d_nm, int32_t mem_cap, std::vector<InfResult> &out)
{
    const size_t nj = js.size();
    DALLOC(d_jobs, InfJob, nj * sizeof(InfJob));
    DALLOC(d_res, InfResult, nj * sizeof(InfResult));
    DCHK(hipMemcpyAsync(d_jobs, js.data(), nj * sizeof(InfJob), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(phi_inflate_decode_kernel, dim3((unsigned)nj), dim3(64), 0, st, d_in, n, d_starts, ck.nch, d_jobs, d_res, d_m, d_nm, mem_cap);
    DCHK(hipGetLastError());
    out.resize(nj);
    DCHK(hipMemcpyAsync(out.data(), d_res, nj * sizeof(InfResult), hipMemcpyDeviceToHost, st));
    return PHI_OK;
}

// 2. one decoder per found start, and 3. the chain of those that began at true block boundaries
int InfRun::decode()
{
    inf_job_index(starts, job_of, chunk_of);
    const size_t nj = chunk_of.size();
    const int64_t cap = std::max(inf_sym_capacity(src, n, ck.C), cap_hint);
    const int32_t mem_cap = inf_member_capacity(n, (int64_t)nj);
    DALLOC(d_sym, uint16_t, nj * (size_t)cap * 2);
    inf_job_list(starts, chunk_of, cap, d_sym, jobs);
    DALLOC(m, InfMember, (size_t)mem_cap * sizeof(InfMember));
    d_mem = m;
    DALLOC(d_nmem, int32_t, 64);
    DCHK(hipMemsetAsync(d_nmem, 0, 64, st));
    if (const int rc = run_decoders(jobs, d_mem, d_nmem, mem_cap, res)) return rc;
    DCHK(hipMemcpyAsync(&nmem, d_nmem, 4, hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    if (nmem > mem_cap) return fail(info, PHI_ERR_OVERFLOW, "phi_inflate: %d member records, capacity %d", nmem, mem_cap);
    return inf_chain(job_of, res, chain, err) ? refused() : PHI_OK;
}

// the chain's decoders whose output outgrew the guess: again, at its size (no member records: the first run's stand)
int InfRun::redecode()
{
    InfAgain A;
    inf_again_plan(chain, res, A);
    if (A.again.empty()) return PHI_OK;
    DALLOC(d_sym2, uint16_t, (size_t)A.total * 2);
    inf_again_jobs(A, res, d_sym2, jobs, jobs2);
    if (const int rc = run_decoders(jobs2, nullptr, nullptr, 0, res2)) return rc;
    DCHK(hipStreamSynchronize(st));
    return inf_again_check(A, jobs, res, res2, err) ? refused() : PHI_OK;
}

// 4. pieces and members, and 5. the markers resolved: the tails in order, then everything else in parallel
int InfRun::layout_resolve()
{
    mem.resize((size_t)nmem);
    if (nmem) {
        DCHK(hipMemcpyAsync(mem.data(), d_mem, (size_t)nmem * sizeof(InfMember), hipMemcpyDeviceToHost, st));
        DCHK(hipStreamSynchronize(st));
    }
    if (inf_layout(chain, res, jobs, mem, pieces, ends, total, err)) return refused();
    DALLOC(o, uint8_t, (size_t)total + 16);
    d_out = o;
    DALLOC(d_pieces, InfPiece, pieces.size() * sizeof(InfPiece));
    DALLOC(s, unsigned long long, 64);
    d_stat = s;
    DCHK(hipMemsetAsync(d_stat, 0, 64, st));
    DCHK(hipMemcpyAsync(d_pieces, pieces.data(), pieces.size() * sizeof(InfPiece), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(phi_inflate_tail_kernel, dim3(1), dim3(1024), 0, st, d_pieces, (int32_t)pieces.size(), d_out, d_stat, (int32_t *)(d_stat + 1));
    DCHK(hipGetLastError());
    inf_slabs(pieces, slabs);
    if (!slabs.empty()) {
        DALLOC(d_slabs, InfSlab, slabs.size() * sizeof(InfSlab));
        DCHK(hipMemcpyAsync(d_slabs, slabs.data(), slabs.size() * sizeof(InfSlab), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(phi_inflate_resolve_kernel, dim3((unsigned)slabs.size()), dim3(256), 0, st, d_pieces, d_slabs, d_out, d_stat, (int32_t *)(d_stat + 1));
        DCHK(hipGetLastError());
    }
    return PHI_OK;
}

// 6. CRC32 and ISIZE of every member
int InfRun::crc_check()
{
    inf_segments(ends, segs);
    crcs.assign(segs.size(), 0);
    if (!segs.empty()) {
        DALLOC(d_segs, InfSeg, segs.size() * sizeof(InfSeg));
        DALLOC(d_crc, uint32_t, segs.size() * 4);
        DCHK(hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(InfSeg), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(phi_inflate_crc_kernel, dim3((unsigned)((segs.size() + 255) / 256)), dim3(256), 0, st, d_out, d_segs, (int64_t)segs.size(), d_crc);
        DCHK(hipGetLastError());
        DCHK(hipMemcpyAsync(crcs.data(), d_crc, segs.size() * 4, hipMemcpyDeviceToHost, st));
    }
    DCHK(hipMemcpyAsync(stat, d_stat, 16, hipMemcpyDeviceToHost, st));
    DCHK(hipEventRecord(dev.ev[1], st));
    DCHK(hipStreamSynchronize(st));
    if ((int32_t)(stat[1] & 0xffffffffu))
        return fail(info, PHI_ERR_INVALID, "gzip stream corrupt: a distance reaches before the start of its member");
    return inf_member_check(ends, segs, crcs, err) ? refused() : PHI_OK;
}

void InfRun::fill_info()
{
    float ms = 0;
    (void)hipEventElapsedTime(&ms, dev.ev[0], dev.ev[1]);
    info->out_bytes = total;
    info->members = (int64_t)ends.size();
    info->confirmed = (int64_t)chain.size() - 1;
    info->redecoded = ck.nch - (int64_t)chain.size();
    info->marker_bytes = (int64_t)stat[0];
    info->device_ms = ms;
}

// the whole inflate; the checked output stays in *d_out_ret (one of dev's buffers), *out_size bytes
int inflate_run(Dev &dev, int32_t device, const void *in, int64_t n, int64_t chunk_bytes, int32_t flags, int64_t *out_size,
                uint8_t **d_out_ret, phi_inflate_info *info, const int64_t *known = nullptr, int64_t n_known = 0, int64_t cap_hint = 0)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!out_size || n < 0 || (n > 0 && !in)) return fail(info, PHI_ERR_INVALID, "phi_inflate: null pointer or negative size");
    *out_size = 0;
    InfRun R{dev, info, (const uint8_t *)in, n, flags};
    R.known = n_known > 0 ? known : nullptr;
    R.n_known = n_known;
    R.cap_hint = R.known ? cap_hint : 0;
    R.hdr = inf_gz_header(R.src, n, 0);
    if (R.hdr < 0) return fail(info, PHI_ERR_INVALID, "phi_inflate: %s gzip header", R.hdr == -2 ? "truncated" : "not a");
    if (inf_chunk_plan(n, chunk_bytes, getenv("PHI_INFLATE_CHUNK"), R.ck, R.err)) return R.refused();
    if (info) { info->in_bytes = n; info->chunks = R.ck.nch; }
    int rc;
    if ((rc = R.upload(device)) || (rc = R.find()) || (rc = R.decode()) || (rc = R.redecode()) || (rc = R.layout_resolve()) || (rc = R.crc_check())) return rc;
    if (info) R.fill_info();
    *out_size = R.total;
    *d_out_ret = R.d_out;
    return PHI_OK;
}

}  // namespace

extern "C" {

int phi_gzip_header(const void *data, int64_t n, int64_t pos, int64_t *deflate_start)
{
    if (!data || n < 0 || pos < 0 || !deflate_start) return PHI_ERR_INVALID;
    const int64_t q = inf_gz_header((const uint8_t *)data, n, pos);
    if (q < 0) return PHI_ERR_INVALID;
    *deflate_start = q;
    return PHI_OK;
}

uint32_t phi_crc32_combine(uint32_t crc_a, uint32_t crc_b, int64_t len_b) { return inf_crc_combine(crc_a, crc_b, (uint64_t)(len_b < 0 ? 0 : len_b)); }

int phi_inflate(int32_t device, const void *in, int64_t n, void *out, int64_t cap, int64_t chunk_bytes, int32_t flags,
                int64_t *out_size, phi_inflate_info *info)
{
    if (cap < 0 || (cap > 0 && !out)) return fail(info, PHI_ERR_INVALID, "phi_inflate: null output or negative capacity");
    Dev dev;
    uint8_t *d_out = nullptr;
    const int rc = inflate_run(dev, device, in, n, chunk_bytes, flags, out_size, &d_out, info);
    if (rc) return rc;
    if (cap >= *out_size && *out_size > 0) DCHK(hipMemcpy(out, d_out, (size_t)*out_size, hipMemcpyDeviceToHost));
    return PHI_OK;
}

int phi_inflate_alloc(int32_t device, const void *in, int64_t n, int64_t chunk_bytes, int32_t flags, void **out, int64_t *out_size,
                      phi_inflate_info *info)
{
    if (!out) return fail(info, PHI_ERR_INVALID, "phi_inflate_alloc: null output");
    *out = nullptr;
    Dev dev;
    uint8_t *d_out = nullptr;
    const int rc = inflate_run(dev, device, in, n, chunk_bytes, flags, out_size, &d_out, info);
    if (rc) return rc;
    void *h = malloc((size_t)std::max<int64_t>(*out_size, 1));
    if (!h) return fail(info, PHI_ERR_NOMEM, "phi_inflate_alloc: %lld bytes of host memory", (long long)*out_size);
    if (*out_size > 0) {
        const hipError_t e = hipMemcpy(h, d_out, (size_t)*out_size, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { free(h); return fail(info, PHI_ERR_DEVICE, "phi_inflate_alloc: %s", hipGetErrorString(e)); }
    }
    *out = h;
    return PHI_OK;
}

void phi_inflate_free(void *p) { free(p); }

// the library's own callers (phi_text_park_gzip_end): the output stays on the device, in a buffer the caller frees (hipFree)
int phi_inflate_to_device(int32_t device, const void *in, int64_t n, int64_t chunk_bytes, int32_t flags, void **d_out,
                          int64_t *out_size, phi_inflate_info *info)
{
    Dev dev;
    uint8_t *d = nullptr;
    const int rc = inflate_run(dev, device, in, n, chunk_bytes, flags, out_size, &d, info);
    if (rc) return rc;
    dev.bufs.erase(std::find(dev.bufs.begin(), dev.bufs.end(), (void *)d));   // (kept: the caller owns it now)
    *d_out = d;
    return PHI_OK;
}

// phi_inflate_to_device for members whose bounds the caller knows (vcf_region.hip: BGZF members followed by BSIZE): starts[0,
// n_starts) are the byte offsets in `in` where a member's deflate data begins, ascending; they stand in for the finder, which
// finds no start in members of one final block.  A wrong offset costs what a false start of the finder costs: its decoder's
// output is not used.  sym_cap: symbols a decoder may write on its first run, at the least (0: the usual guess)
int phi_inflate_to_device_starts(int32_t device, const void *in, int64_t n, int64_t chunk_bytes, const int64_t *starts, int64_t n_starts, int64_t sym_cap,
                                 void **d_out, int64_t *out_size, phi_inflate_info *info)
{
    Dev dev;
    uint8_t *d = nullptr;
    const int rc = inflate_run(dev, device, in, n, chunk_bytes, 0, out_size, &d, info, starts, n_starts, sym_cap);
    if (rc) return rc;
    dev.bufs.erase(std::find(dev.bufs.begin(), dev.bufs.end(), (void *)d));   // (kept: the caller owns it now)
    *d_out = d;
    return PHI_OK;
}

}  // extern "C"
