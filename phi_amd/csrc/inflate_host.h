// inflate_host.h -- what inflate.hip's host side and its kernels share (records, status values, constants, the gzip member
// header) and the rules of an inflate that need no GPU, over plain vectors: the chunk plan, the symbol capacity of a decoder,
// the job list, the chain of decoders that began at true block boundaries, the second run of decoders that outgrew their
// capacity, the layout of pieces and members, the slabs and CRC segments, and the members' CRC32 / ISIZE check.
// No HIP include and nothing of the context: inflate.hip calls these between its launches, and
// host/inflate_host_selftest.cpp runs them stand-alone under the sanitizers.  A function that refuses its input has set
// `err` (code and text of the fail() its caller makes of it) and returns err.code.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "../../include/phi_amd.h"
#include "crc32_shift.h"

#define INF_SEG 4096            // CRC segment
#define INF_WIN 32768
#define INF_SLAB 65536          // symbols one workgroup of the resolve kernel takes

namespace {                     // internal to the file that includes this, like the kernels whose parameters these are

enum : int {
    INF_STOP = 0,               // stood on another decoder's start
    INF_END = 1,                // the stream's last trailer
    INF_E_CODE = -1,            // invalid Huffman code / symbol
    INF_E_TRUNC = -2,           // ran past the input
    INF_E_DIST = -3,            // distance before the member's first byte
    INF_E_HEADER = -4,          // bad gzip member header
    INF_E_BLOCK = -5,           // bad block type, bad dynamic header, LEN != ~NLEN
};

struct InfJob { int64_t start; int64_t cap; uint16_t *sym; int32_t chunk; int32_t pad; };
struct InfResult { int64_t out_len; int64_t end_bit; int32_t end_chunk; int32_t status; int32_t ovf; int32_t pad; };
struct InfMember { int32_t job; int32_t pad; int64_t pos; uint32_t crc; uint32_t isize; };
struct InfPiece { int64_t abs; int64_t len; int64_t lo; const uint16_t *sym; };
struct InfSlab { int32_t piece; int32_t pad; int64_t k0; int64_t k1; };
struct InfSeg { int64_t off; int64_t len; };

struct InfErr {
    int code = 0;
    char text[192] = "";
    int set(int code_, const char *fmt, ...) __attribute__((format(printf, 3, 4)))
    {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof text, fmt, ap);
        va_end(ap);
        return code = code_;
    }
};

// ------------------------------------------------------------------------------------------------ shared host/device

DFL_HD uint32_t inf_crc_bitwise(uint32_t c, const uint8_t *p, int64_t n)
{
    c = ~c;
    for (int64_t i = 0; i < n; i++) c = dfl_crc_byte(c ^ p[i]);
    return ~c;
}

// a gzip member header at byte p of b[0, n): the byte offset of its deflate data, -1 when invalid, -2 when truncated
DFL_HD int64_t inf_gz_header(const uint8_t *b, int64_t n, int64_t p)
{
    if (p + 10 > n) return -2;
    if (b[p] != 0x1f || b[p + 1] != 0x8b || b[p + 2] != 8) return -1;
    const uint32_t flg = b[p + 3];
    if (flg & 0xe0) return -1;
    int64_t q = p + 10;
    if (flg & 4) {                                              // FEXTRA
        if (q + 2 > n) return -2;
        q += 2 + (b[q] | (b[q + 1] << 8));
        if (q > n) return -2;
    }
    for (uint32_t f = 8; f <= 16; f <<= 1)                      // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            while (q < n && b[q]) q++;
            if (q >= n) return -2;
            q++;
        }
    if (flg & 2) {                                              // FHCRC: low 16 bits of the header's CRC32
        if (q + 2 > n) return -2;
        if ((inf_crc_bitwise(0, b + p, q - p) & 0xffffu) != (uint32_t)(b[q] | (b[q + 1] << 8))) return -1;
        q += 2;
    }
    return q;
}

// ------------------------------------------------------------------------------------------------ CRC32 shift, 64-bit
// pw[k] = x^(8 * 2^k) mod P: a register times pw[k] is the register after 2^k more zero bytes
struct InfCrcPow {
    uint32_t pw[64];
    InfCrcPow()
    {
        pw[0] = 0x00800000u;                                    // x^8
        for (int k = 1; k < 64; k++) pw[k] = dfl_crc_mul(pw[k - 1], pw[k - 1]);
    }
};
static inline const InfCrcPow &inf_crc_pow()
{
    static const InfCrcPow P;
    return P;
}
// the register c (zero initial value, no final inversion) after nbytes more zero bytes
static inline uint32_t inf_crc_shift(uint32_t c, uint64_t nbytes)
{
    const InfCrcPow &P = inf_crc_pow();
    for (int k = 0; nbytes && c; k++, nbytes >>= 1)
        if (nbytes & 1) c = dfl_crc_mul(c, P.pw[k]);
    return c;
}
// crc(A B) from crc(A), crc(B) and |B|: the initial and final inversions of crc(A) and crc(B) cancel
static inline uint32_t inf_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return inf_crc_shift(crc_a, len_b) ^ crc_b; }

// ------------------------------------------------------------------------------------------------ chunks, capacity, jobs

static inline const char *inf_status_text(int s)
{
    switch (s) {
    case INF_E_CODE: return "invalid Huffman code";
    case INF_E_TRUNC: return "truncated stream";
    case INF_E_DIST: return "distance before the start of the member";
    case INF_E_HEADER: return "bad gzip member header";
    case INF_E_BLOCK: return "invalid block header";
    default: return "error";
    }
}

// The n compressed bytes in chunks of C: the caller's chunk_bytes, 64 at least; without one (<= 0) the value of
// PHI_INFLATE_CHUNK (`env`, may be null) where that is a positive number, else PHI_INFLATE_CHUNK_DEFAULT.  2^30 chunks
// or more are refused.
struct InfChunks { int64_t C; int32_t nch; };
static inline int inf_chunk_plan(int64_t n, int64_t chunk_bytes, const char *env, InfChunks &P, InfErr &err)
{
    const long long v = env ? atoll(env) : 0;
    P.C = chunk_bytes > 0 ? std::max<int64_t>(chunk_bytes, 64) : v > 0 ? v : PHI_INFLATE_CHUNK_DEFAULT;
    const int64_t nch = n / P.C + (n % P.C != 0);
    P.nch = 0;
    if (nch >= (1 << 30)) return err.set(PHI_ERR_UNSUPPORTED, "phi_inflate: %lld chunks", (long long)nch);
    P.nch = (int32_t)nch;
    return PHI_OK;
}

// Symbols a decoder may write on its first run: its chunk times the stream's ratio, a quarter more, and 4096.  The ratio
// is a guess from the last four bytes (the last member's ISIZE) over n, kept within [4, 1100]; 4 for a stream shorter than
// an empty member.  A decoder that outgrows it runs again.
static inline int64_t inf_sym_capacity(const uint8_t *src, int64_t n, int64_t C)
{
    double ratio = 4.0;
    if (n >= 18) {
        const uint32_t isz = src[n - 4] | (src[n - 3] << 8) | (src[n - 2] << 16) | ((uint32_t)src[n - 1] << 24);
        ratio = std::max(ratio, std::min(1100.0, (double)isz / (double)n));
    }
    return (int64_t)((double)C * ratio * 1.25) + 4096;
}

// One job per chunk with a start (starts[i] >= 0), in chunk order: job_of[chunk] (-1: none) and chunk_of[job]
static inline void inf_job_index(const std::vector<int64_t> &starts, std::vector<int> &job_of, std::vector<int> &chunk_of)
{
    job_of.assign(starts.size(), -1);
    chunk_of.clear();
    for (size_t i = 0; i < starts.size(); i++)
        if (starts[i] >= 0) { job_of[i] = (int)chunk_of.size(); chunk_of.push_back((int)i); }
}

// The jobs of that index: job k decodes from its chunk's start into cap symbols at sym + k * cap (sym: device memory, never
// read through here)
static inline void inf_job_list(const std::vector<int64_t> &starts, const std::vector<int> &chunk_of, int64_t cap, uint16_t *sym,
                                std::vector<InfJob> &jobs)
{
    jobs.resize(chunk_of.size());
    for (size_t k = 0; k < chunk_of.size(); k++) jobs[k] = InfJob{starts[(size_t)chunk_of[k]], cap, sym + k * (size_t)cap, chunk_of[k], 0};
}

// Member records the decoders of nj jobs may write: a member is 18 bytes at least, and a job may see a few that others see too
static inline int32_t inf_member_capacity(int64_t n, int64_t nj) { return (int32_t)std::min<int64_t>(n / 18 + 4 * nj + 64, 1 << 30); }

// ------------------------------------------------------------------------------------------------ the chain
// From chunk 0's job: a job that stopped on another decoder's start (INF_STOP) is followed by that chunk's job, the job
// that read the stream's last trailer (INF_END) ends the chain; jobs not reached are dropped.  A negative status on the way
// is the stream's error.  The decode kernel promises that a STOP names a later chunk that has a job; a result that breaks
// the promise is refused, not followed.
static inline int inf_chain(const std::vector<int> &job_of, const std::vector<InfResult> &res, std::vector<int> &chain, InfErr &err)
{
    const int nch = (int)job_of.size();
    chain.clear();
    if (nch < 1 || job_of[0] < 0) return err.set(PHI_ERR_DEVICE, "phi_inflate: chunk 0 has no decoder (internal error)");
    for (int ch = 0;;) {
        const int k = job_of[(size_t)ch];
        const InfResult &r = res[(size_t)k];
        chain.push_back(k);
        if (r.status < 0)
            return err.set(PHI_ERR_INVALID, "gzip stream corrupt: %s (near compressed byte %lld)", inf_status_text(r.status), (long long)(r.end_bit / 8));
        if (r.status == INF_END) break;
        if (r.end_chunk <= ch || r.end_chunk >= nch || job_of[(size_t)r.end_chunk] < 0)
            return err.set(PHI_ERR_DEVICE, "phi_inflate: decoder of chunk %d stopped on chunk %d of %d, which has no decoder after it (internal error)",
                           ch, r.end_chunk, nch);
        ch = r.end_chunk;
    }
    return PHI_OK;
}

// ------------------------------------------------------------------------------------------------ the second run
// The chain's jobs whose output outgrew their capacity decode again, each into out_len + 1 symbols of one buffer:
// again[q] the job, off[q] its symbols' offset, total the buffer's symbols
struct InfAgain { std::vector<int> again; std::vector<int64_t> off; int64_t total = 0; };
static inline void inf_again_plan(const std::vector<int> &chain, const std::vector<InfResult> &res, InfAgain &A)
{
    A = InfAgain{};
    for (int k : chain)
        if (res[(size_t)k].ovf) {
            A.again.push_back(k);
            A.off.push_back(A.total);
            A.total += res[(size_t)k].out_len + 1;
        }
}
// their jobs (j2), and jobs[] pointed at the new symbols
static inline void inf_again_jobs(const InfAgain &A, const std::vector<InfResult> &res, uint16_t *sym2, std::vector<InfJob> &jobs, std::vector<InfJob> &j2)
{
    j2.clear();
    for (size_t q = 0; q < A.again.size(); q++) {
        InfJob &j = jobs[(size_t)A.again[q]];
        j.sym = sym2 + A.off[q];
        j2.push_back(InfJob{j.start, res[(size_t)A.again[q]].out_len + 1, j.sym, j.chunk, 0});
    }
}
// a second run repeats the first one's length and status, and fits
static inline int inf_again_check(const InfAgain &A, const std::vector<InfJob> &jobs, const std::vector<InfResult> &res, const std::vector<InfResult> &r2,
                                  InfErr &err)
{
    for (size_t q = 0; q < A.again.size(); q++) {
        const InfResult &a = res[(size_t)A.again[q]];
        if (r2[q].ovf || r2[q].out_len != a.out_len || r2[q].status != a.status)
            return err.set(PHI_ERR_DEVICE, "phi_inflate: decoder of chunk %d differs on its second run (internal error)", jobs[(size_t)A.again[q]].chunk);
    }
    return PHI_OK;
}

// ------------------------------------------------------------------------------------------------ pieces and members
// One piece per chain job, in chain order, at abs = the output bytes before it.  A member ends where a chain job's member
// record says (records of dropped jobs count for nothing); ends by (abs, record index), so that an empty member follows
// the one before it.  The last end is the output's end.  lo of a piece: the first byte of the member its first byte lies
// in -- the last end at or before its abs -- which no distance of the piece's markers may reach before.
struct InfEnd { int64_t abs; int idx; uint32_t crc, isize; };
static inline int inf_layout(const std::vector<int> &chain, const std::vector<InfResult> &res, const std::vector<InfJob> &jobs,
                             const std::vector<InfMember> &mem, std::vector<InfPiece> &pieces, std::vector<InfEnd> &ends, int64_t &total, InfErr &err)
{
    std::vector<int> piece_of(res.size(), -1);
    pieces.clear();
    ends.clear();
    total = 0;
    for (int k : chain) {
        piece_of[(size_t)k] = (int)pieces.size();
        pieces.push_back(InfPiece{total, res[(size_t)k].out_len, 0, jobs[(size_t)k].sym});
        total += res[(size_t)k].out_len;
    }
    for (size_t q = 0; q < mem.size(); q++) {
        if (mem[q].job < 0 || (size_t)mem[q].job >= res.size())
            return err.set(PHI_ERR_DEVICE, "phi_inflate: member record %zu of decoder %d (internal error)", q, mem[q].job);
        const int pc = piece_of[(size_t)mem[q].job];
        if (pc >= 0) ends.push_back(InfEnd{pieces[(size_t)pc].abs + mem[q].pos, (int)q, mem[q].crc, mem[q].isize});
    }
    std::sort(ends.begin(), ends.end(), [](const InfEnd &a, const InfEnd &b) { return a.abs != b.abs ? a.abs < b.abs : a.idx < b.idx; });
    if (ends.empty() || ends.back().abs != total) return err.set(PHI_ERR_DEVICE, "phi_inflate: member ends do not cover the output (internal error)");
    size_t e = 0;
    int64_t lo = 0;
    for (InfPiece &pc : pieces) {
        while (e < ends.size() && ends[e].abs <= pc.abs) lo = ends[e++].abs;
        pc.lo = lo;
    }
    return PHI_OK;
}

// Everything before a piece's last INF_WIN symbols, in slabs of INF_SLAB
static inline void inf_slabs(const std::vector<InfPiece> &pieces, std::vector<InfSlab> &slabs)
{
    slabs.clear();
    for (size_t p = 0; p < pieces.size(); p++) {
        const int64_t body = std::max<int64_t>(0, pieces[p].len - INF_WIN);
        for (int64_t k = 0; k < body; k += INF_SLAB) slabs.push_back(InfSlab{(int32_t)p, 0, k, std::min<int64_t>(body, k + INF_SLAB)});
    }
}

// Every member's bytes in segments of INF_SEG from its first byte, the last one shorter; an empty member has none
static inline void inf_segments(const std::vector<InfEnd> &ends, std::vector<InfSeg> &segs)
{
    segs.clear();
    int64_t s = 0;
    for (const InfEnd &e : ends) {
        for (int64_t k = s; k < e.abs; k += INF_SEG) segs.push_back(InfSeg{k, std::min<int64_t>(INF_SEG, e.abs - k)});
        s = e.abs;
    }
}

// CRC32 and ISIZE of every member against its trailer.  crcs[s]: the register of segment s run from zero without the final
// inversion, so a member's register is the segments' combined by the shift, a full segment by the one constant x^(8 INF_SEG).
static inline int inf_member_check(const std::vector<InfEnd> &ends, const std::vector<InfSeg> &segs, const std::vector<uint32_t> &crcs, InfErr &err)
{
    const uint32_t full = inf_crc_pow().pw[12];
    static_assert(INF_SEG == 1 << 12, "pw[12] shifts by one full segment");
    size_t sg = 0;
    int64_t start = 0;
    for (size_t m = 0; m < ends.size(); m++) {
        const int64_t len = ends[m].abs - start;
        uint32_t raw = 0;
        for (; sg < segs.size() && segs[sg].off < ends[m].abs; sg++)
            raw = (segs[sg].len == INF_SEG ? dfl_crc_mul(raw, full) : inf_crc_shift(raw, (uint64_t)segs[sg].len)) ^ crcs[sg];
        const uint32_t crc = inf_crc_shift(0xffffffffu, (uint64_t)len) ^ raw ^ 0xffffffffu;
        if (crc != ends[m].crc)
            return err.set(PHI_ERR_INVALID, "gzip stream corrupt: CRC32 mismatch in member %zu (%08x, trailer %08x)", m, crc, ends[m].crc);
        if ((uint32_t)len != ends[m].isize)
            return err.set(PHI_ERR_INVALID, "gzip stream corrupt: ISIZE mismatch in member %zu (%u, trailer %u)", m, (uint32_t)len, ends[m].isize);
        start = ends[m].abs;
    }
    return PHI_OK;
}

}  // namespace
