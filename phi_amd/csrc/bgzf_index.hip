// bgzf_index.hip -- the indexes of a BGZF file, built while the file is written: phi_deflate_bgzf_indexed.
//
// .gzi needs the members' offsets and nothing else: host code (bgzf_index_host.h).  For .tbi (VCF preset) the text is uploaded
// once, the writer's batches compress it from there (deflate.hip, phi_deflate_run), and the index is found over the BYTES of the
// text, never by a lane walking a line: a structural variant's REF is tens of kilobases and a line straddles blocks and batches.
//   1. MARKS    every lane takes 16 bytes in one load and forms three 16-bit masks: newlines, tabs, and the rare places where
//               "END=" follows a tab or ';'.  Counts per workgroup, one scan of them (scan.hip), and the same lanes write three
//               ascending lists of 64-bit positions; every newline also keeps how many tabs and END places lie before it, so a
//               line finds its own tabs by index.  The masks are formed twice, from the text, and not stored between.
//   2. LINES    one lane per line: meta ('#'), record, or empty (refused).  The records are compacted (scan.hip).
//   3. RECORDS  one lane per record, from the lists: the ends of its first eight fields are tab positions, len(REF) a difference
//               of two of them; at most 10 digits of POS; the first END place inside INFO by bisection, at most 10 digits of it;
//               CHROM against the previous record's, at most 1024 bytes; beg, end, bin, both virtual offsets; the refusals.
//   4. CHUNKS   run heads -- contig or bin differs from the record before -- and contig heads, both compacted (scan.hip); a lane
//               per chunk gathers bin and virtual offsets, a lane per contig where its name stands.
//   5. WINDOWS  a lane per record: the contig by bisection of the contig heads, atomicMax for the contig's last end; then, the
//               window arrays sized, a 64-bit atomicMin per (record, window it overlaps).  Integer min and max: the result does
//               not depend on the order.
// Every loop is bounded: 16 bytes, 10 digits, 1024 name bytes, a bisection, and 2^29 >> 14 windows of a record.  A refusal is
// the smallest (line, reason) raised by any lane, so the message does not depend on the order either.
// The host then groups the chunks by bin, fills the empty windows and lays the bytes out (bgzf_index_host.h), and the index
// goes through the same writer.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/phi_amd.h"
#include "phi_ctx.h"
#include "phi_wave.h"
#include "dev_run.h"
#include "vcf_lines_dev.h"
#include "text_bytes.h"
#include "bgzf_index_host.h"

#define BIX_MAX_LINES 2147483646ll      // lines are numbered in 32 bits (the compaction's indices)
static_assert(PHI_BGZF_BLOCK == bgzfx::BLOCK, "one block size");

namespace {

enum { BIX_EMPTY = 1, BIX_FIELDS, BIX_POS, BIX_END, BIX_ORDER, BIX_RANGE, BIX_NAME };

// the three masks of the 16 bytes at 16 g (text is readable to the next multiple of BIX_WG and 64 bytes beyond)
__device__ __forceinline__ void bix_masks(const uint8_t *__restrict__ text, int64_t n, int64_t g, uint32_t *nl, uint32_t *tab, uint32_t *end)
{
    const int64_t p0 = g * BIX_LANE;
    *nl = *tab = *end = 0;
    if (p0 >= n) return;
    const PhiText16 v = phi_load16(text, p0);
    const uint32_t valid = phi_valid16(p0, 0, n);
    uint32_t m_e = phi_eq16(v, 'E') & valid;
    uint32_t m_end = 0;
    while (m_e) {                                       // at most 16 turns, and 'E' is rare
        const int j = __ffs((int)m_e) - 1;
        m_e &= m_e - 1;
        const int64_t p = p0 + j;
        if (p < 1 || p + 3 >= n) continue;
        const uint8_t b = text[p - 1];
        if ((b == '\t' || b == ';') && text[p + 1] == 'N' && text[p + 2] == 'D' && text[p + 3] == '=') m_end |= 1u << j;
    }
    *nl = phi_eq16(v, '\n') & valid;
    *tab = phi_eq16(v, '\t') & valid;
    *end = m_end;
}

// cnt[k * nblk + workgroup]: its newlines (k = 0), tabs (1), END places (2)
__global__ void __launch_bounds__(BIX_T) phi_bix_mark_count_kernel(const uint8_t *__restrict__ text, int64_t n, int64_t nblk, int32_t *__restrict__ cnt)
{
    __shared__ int s_w[3][BIX_T / 64];
    uint32_t nl, tab, end;
    bix_masks(text, n, (int64_t)blockIdx.x * BIX_T + threadIdx.x, &nl, &tab, &end);
    const int c[3] = {phi_wave_sum((int)__popc(nl)), phi_wave_sum((int)__popc(tab)), phi_wave_sum((int)__popc(end))};
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; k++) s_w[k][threadIdx.x >> 6] = c[k];
    __syncthreads();
    if (threadIdx.x < 3) {
        int t = 0;
        for (int i = 0; i < BIX_T / 64; i++) t += s_w[threadIdx.x][i];
        cnt[(int64_t)threadIdx.x * nblk + blockIdx.x] = t;
    }
}

// off[k * (nblk + 1) + workgroup]: the scans of cnt.  The lists, ascending; list sizes are off[k * (nblk + 1) + nblk]
__global__ void __launch_bounds__(BIX_T) phi_bix_mark_write_kernel(const uint8_t *__restrict__ text, int64_t n, int64_t nblk, const int64_t *__restrict__ off,
                                                                   int64_t *__restrict__ nl_pos, int64_t *__restrict__ nl_tab, int64_t *__restrict__ nl_end,
                                                                   int64_t *__restrict__ tab_pos, int64_t *__restrict__ end_pos)
{
    __shared__ int s_w[3][BIX_T / 64];
    uint32_t nl, tab, end;
    const int64_t g = (int64_t)blockIdx.x * BIX_T + threadIdx.x;
    bix_masks(text, n, g, &nl, &tab, &end);
    int64_t o_nl = off[blockIdx.x] + phi_block_excl_scan<BIX_T / 64>((int)__popc(nl), s_w[0]);
    int64_t o_tab = off[(nblk + 1) + blockIdx.x] + phi_block_excl_scan<BIX_T / 64>((int)__popc(tab), s_w[1]);
    int64_t o_end = off[2 * (nblk + 1) + blockIdx.x] + phi_block_excl_scan<BIX_T / 64>((int)__popc(end), s_w[2]);
    uint32_t any = nl | tab | end;
    while (any) {                                       // in the order of the text: a newline sees the tabs before it
        const int j = __ffs((int)any) - 1;
        const uint32_t bit = 1u << j;
        any &= any - 1;
        const int64_t p = g * BIX_LANE + j;
        if (tab & bit) tab_pos[o_tab++] = p;
        if (end & bit) end_pos[o_end++] = p;
        if (nl & bit) { nl_pos[o_nl] = p; nl_tab[o_nl] = o_tab; nl_end[o_nl] = o_end; o_nl++; }
    }
}

__device__ __forceinline__ void bix_raise(unsigned long long *err, int64_t line, int why)
{
    atomicMin(err, ((unsigned long long)line << 8) | (unsigned long long)why);
}

__global__ void __launch_bounds__(256) phi_bix_lines_kernel(BixLists L, int64_t n_lines, uint8_t *__restrict__ is_rec, unsigned long long *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_lines) return;
    const BixLine l = bix_line(L, i);
    if (l.e == l.s) { is_rec[i] = 0; bix_raise(err, i, BIX_EMPTY); return; }
    is_rec[i] = L.text[l.s] != '#';
}

__device__ __forceinline__ uint64_t bix_voff(const int64_t *__restrict__ off, int64_t p)
{
    return ((uint64_t)off[p / PHI_BGZF_BLOCK] << 16) | (uint64_t)(p % PHI_BGZF_BLOCK);
}

struct BixRecords {                                     // per record (device pointers)
    int32_t *beg, *end, *bin, *ctg;
    uint64_t *vbeg, *vend;
    uint8_t *new_ctg, *head;
};

__global__ void __launch_bounds__(256) phi_bix_records_kernel(BixLists L, const int32_t *__restrict__ rec_line, int64_t n_rec, const int64_t *__restrict__ off,
                                                              BixRecords R, unsigned long long *__restrict__ err)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rec) return;
    const uint8_t *__restrict__ text = L.text;
    const int64_t li = rec_line[r];
    const BixLine l = bix_line(L, li);
    int64_t beg = 0, end = 1;
    bool is_new = r == 0;
    const int64_t next = l.e < L.n ? l.e + 1 : L.n;     // the byte after the line
    R.vbeg[r] = bix_voff(off, l.s);
    R.vend[r] = bix_voff(off, next);
    const int64_t ntab = l.tab_hi - l.tab_lo;
    if (ntab < 7) bix_raise(err, li, BIX_FIELDS);
    else {
        int64_t pos = -1;
        const int bad = bix_interval(L, l, &beg, &end, &pos);
        bool ok = !bad;
        if (bad) bix_raise(err, li, bad == 1 ? BIX_POS : BIX_END);
        else if (end > bgzfx::MAX_END) { bix_raise(err, li, BIX_RANGE); ok = false; }
        const int64_t t0 = L.tab_pos[l.tab_lo];
        const int64_t len = t0 - l.s;
        if (len > bgzfx::MAX_NAME) { bix_raise(err, li, BIX_NAME); ok = false; }
        else if (r > 0) {
            const int64_t pi = rec_line[r - 1];
            const BixLine p = bix_line(L, pi);
            if (p.tab_hi - p.tab_lo < 2) is_new = true;                  // (that record is refused by its own lane)
            else {
                const int64_t p0 = L.tab_pos[p.tab_lo], p1 = L.tab_pos[p.tab_lo + 1];
                bool same = p0 - p.s == len;
                for (int64_t k = 0; same && k < len; k++) same = text[p.s + k] == text[l.s + k];
                is_new = !same;
                if (same && pos >= 0) {
                    const int64_t ppos = bix_number(text, p0 + 1, p1);
                    if (ppos > pos) bix_raise(err, li, BIX_ORDER);
                }
            }
        }
        if (!ok) { beg = 0; end = 1; }
    }
    // reg2bin (bgzf_index_host.h has the host's copy)
    const int64_t e1 = end - 1;
    int32_t bin = 0;
    if (beg >> 14 == e1 >> 14) bin = (int32_t)(4681 + (beg >> 14));
    else if (beg >> 17 == e1 >> 17) bin = (int32_t)(585 + (beg >> 17));
    else if (beg >> 20 == e1 >> 20) bin = (int32_t)(73 + (beg >> 20));
    else if (beg >> 23 == e1 >> 23) bin = (int32_t)(9 + (beg >> 23));
    else if (beg >> 26 == e1 >> 26) bin = (int32_t)(1 + (beg >> 26));
    R.beg[r] = (int32_t)beg;
    R.end[r] = (int32_t)end;
    R.bin[r] = bin;
    R.new_ctg[r] = is_new;
}

__global__ void __launch_bounds__(256) phi_bix_heads_kernel(BixRecords R, int64_t n_rec)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rec) return;
    R.head[r] = r == 0 || R.new_ctg[r] || R.bin[r] != R.bin[r - 1];
}

struct BixChunk { uint64_t beg, end; int32_t bin, new_ctg; };
struct BixName { int64_t at, len; };

__global__ void __launch_bounds__(256) phi_bix_chunks_kernel(BixRecords R, int64_t n_rec, const int32_t *__restrict__ head_rec, int64_t n_chunks,
                                                             BixChunk *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_chunks) return;
    const int64_t r0 = head_rec[k], r1 = k + 1 < n_chunks ? (int64_t)head_rec[k + 1] : n_rec;
    out[k] = BixChunk{R.vbeg[r0], R.vend[r1 - 1], R.bin[r0], R.new_ctg[r0]};
}

__global__ void __launch_bounds__(256) phi_bix_names_kernel(BixLists L, const int32_t *__restrict__ rec_line, const int32_t *__restrict__ ctg_rec, int64_t n_ctg,
                                                            BixName *__restrict__ out)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_ctg) return;
    const BixLine l = bix_line(L, rec_line[ctg_rec[c]]);
    out[c] = BixName{l.s, L.tab_pos[l.tab_lo] - l.s};   // (every record has its tabs: the refusals were looked at before)
}

// ctg[r] = the contig of record r, max_end[c] = the last end of contig c (zeroed before)
__global__ void __launch_bounds__(256) phi_bix_contigs_kernel(BixRecords R, int64_t n_rec, const int32_t *__restrict__ ctg_rec, int64_t n_ctg,
                                                              int32_t *__restrict__ max_end)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rec) return;
    const int64_t lo = phi_last_le(ctg_rec, n_ctg, r);  // the last contig head at or before r (ctg_rec[0] == 0)
    R.ctg[r] = (int32_t)lo;
    atomicMax(&max_end[lo], R.end[r]);
}

// lin[w_base[c] + w] (all ones before) = the smallest record start among the records of contig c that overlap window w
__global__ void __launch_bounds__(256) phi_bix_windows_kernel(BixRecords R, int64_t n_rec, const int64_t *__restrict__ w_base, unsigned long long *__restrict__ lin)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rec) return;
    unsigned long long *mine = lin + w_base[R.ctg[r]];
    const int w1 = (R.end[r] - 1) >> bgzfx::LIN_SHIFT;  // at most 2^29 >> 14 turns
    for (int w = R.beg[r] >> bgzfx::LIN_SHIFT; w <= w1; w++) atomicMin(&mine[w], (unsigned long long)R.vbeg[r]);
}

inline unsigned grid(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

const char *why_text(int why)
{
    switch (why) {
    case BIX_EMPTY: return "an empty line";
    case BIX_FIELDS: return "a record with fewer than 8 fields";
    case BIX_POS: return "POS is empty, not all digits or longer than 10 digits";
    case BIX_END: return "the END of INFO is empty, not all digits or longer than 10 digits";
    case BIX_ORDER: return "POS is smaller than the previous record's on the same contig";
    case BIX_RANGE: return "the record ends beyond 2^29, where a CSI index would be needed (not written)";
    case BIX_NAME: return "a contig name longer than 1024 bytes";
    }
    return "internal error";
}

// events around a run of launches, the stream waited for, the time added to info->device_ms
#define BIX_BEGIN() DCHK(hipEventRecord(dev.ev[0], st))
#define BIX_END_WAIT() do { DCHK(hipGetLastError()); DCHK(hipEventRecord(dev.ev[1], st)); DCHK(hipStreamSynchronize(st)); float ms_ = 0; \
                            (void)hipEventElapsedTime(&ms_, dev.ev[0], dev.ev[1]); info->device_ms += ms_; } while (0)

// flags[0, n) -> *list (allocated here), *count
#define BIX_COMPACT(flags, n, list, count) \
    int32_t *list = nullptr; int64_t count = 0; \
    { BIX_BEGIN(); phi_compact_count(st, flags, n, d_blk_cnt, d_blk_off); BIX_END_WAIT(); \
      DCHK(hipMemcpy(&count, d_blk_off + phi_compact_blocks(n), 8, hipMemcpyDeviceToHost)); \
      list = dev.alloc<int32_t>((size_t)count * 4); if (!list) return fail(info, PHI_ERR_NOMEM, "device allocation of %lld indices failed", (long long)count); \
      BIX_BEGIN(); phi_compact_write(st, flags, n, d_blk_off, list); BIX_END_WAIT(); }

// the uncompressed bytes of the .tbi of text[0, n) (d_text: the same on the device, readable to the next multiple of BIX_WG and
// 64 bytes beyond); off[0..blocks]: where the members begin
int tbi_run(Dev &dev, const uint8_t *text, const uint8_t *d_text, int64_t n, const std::vector<int64_t> &off, phi_bgzf_index_info *info,
            std::vector<uint8_t> *bytes)
{
    hipStream_t st = dev.st;
    std::vector<bgzfx::TbiContig> contigs;
    bgzfx::TbiCounts counts;
    if (n == 0) { *bytes = bgzfx::tbi_bytes(contigs, &counts); return PHI_OK; }

    // ---- 1. marks
    BixLists L{};
    if (const int mrc = bix_mark_run(dev, d_text, n, &L, info, &info->device_ms, "phi_deflate_bgzf_indexed")) return mrc;
    const int64_t n_nl = L.n_nl;
    const int64_t n_lines = n_nl + (text[n - 1] != '\n');
    if (n_lines > BIX_MAX_LINES) return fail(info, PHI_ERR_UNSUPPORTED, "phi_deflate_bgzf_indexed: %lld lines, more than 2^31 - 2", (long long)n_lines);
    DALLOC(d_is_rec, uint8_t, (size_t)n_lines);
    DALLOC(d_err, unsigned long long, 8);
    const int64_t nscr = phi_compact_blocks(n_lines);
    DALLOC(d_blk_cnt, int32_t, (size_t)nscr * 4);
    DALLOC(d_blk_off, int64_t, (size_t)(nscr + 1) * 8);
    DALLOC(d_off, int64_t, off.size() * 8);
    DCHK(hipMemcpyAsync(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, st));
    DCHK(hipMemsetAsync(d_err, 0xff, 8, st));

    // ---- 2. lines
    BIX_BEGIN();
    hipLaunchKernelGGL(phi_bix_lines_kernel, dim3(grid(n_lines)), dim3(256), 0, st, L, n_lines, d_is_rec, d_err);
    BIX_END_WAIT();
    BIX_COMPACT(d_is_rec, n_lines, d_rec_line, n_rec);
    if (n_rec < 0 || n_rec > n_lines) return fail(info, PHI_ERR_DEVICE, "phi_deflate_bgzf_indexed: %lld records in %lld lines (internal error)", (long long)n_rec, (long long)n_lines);

    // ---- 3. records
    BixRecords R{};
    if (n_rec > 0) {
        DALLOC(d_beg, int32_t, (size_t)n_rec * 4);
        DALLOC(d_end, int32_t, (size_t)n_rec * 4);
        DALLOC(d_bin, int32_t, (size_t)n_rec * 4);
        DALLOC(d_ctg, int32_t, (size_t)n_rec * 4);
        DALLOC(d_vbeg, uint64_t, (size_t)n_rec * 8);
        DALLOC(d_vend, uint64_t, (size_t)n_rec * 8);
        DALLOC(d_new, uint8_t, (size_t)n_rec);
        DALLOC(d_head, uint8_t, (size_t)n_rec);
        R = BixRecords{d_beg, d_end, d_bin, d_ctg, d_vbeg, d_vend, d_new, d_head};
        BIX_BEGIN();
        hipLaunchKernelGGL(phi_bix_records_kernel, dim3(grid(n_rec)), dim3(256), 0, st, L, d_rec_line, n_rec, d_off, R, d_err);
        hipLaunchKernelGGL(phi_bix_heads_kernel, dim3(grid(n_rec)), dim3(256), 0, st, R, n_rec);
        BIX_END_WAIT();
    }
    unsigned long long err = 0;
    DCHK(hipMemcpy(&err, d_err, 8, hipMemcpyDeviceToHost));
    if (err != ~0ull) {
        const int why = (int)(err & 0xff);
        return fail(info, why == BIX_RANGE || why == BIX_NAME ? PHI_ERR_UNSUPPORTED : PHI_ERR_INVALID, "phi_deflate_bgzf_indexed: line %lld: %s",
                    (long long)(err >> 8) + 1, why_text(why));
    }
    info->records = n_rec;
    info->meta_lines = n_lines - n_rec;

    if (n_rec > 0) {
        // ---- 4. chunks and contigs
        BIX_COMPACT(R.head, n_rec, d_head_rec, n_chunks);
        BIX_COMPACT(R.new_ctg, n_rec, d_ctg_rec, n_ctg);
        if (n_chunks < 1 || n_chunks > n_rec || n_ctg < 1 || n_ctg > n_chunks)
            return fail(info, PHI_ERR_DEVICE, "phi_deflate_bgzf_indexed: %lld chunks, %lld contigs of %lld records (internal error)", (long long)n_chunks, (long long)n_ctg, (long long)n_rec);
        DALLOC(d_chunks, BixChunk, (size_t)n_chunks * sizeof(BixChunk));
        DALLOC(d_names, BixName, (size_t)n_ctg * sizeof(BixName));
        DALLOC(d_max_end, int32_t, (size_t)n_ctg * 4);
        DALLOC(d_w_base, int64_t, (size_t)n_ctg * 8);
        DCHK(hipMemsetAsync(d_max_end, 0, (size_t)n_ctg * 4, st));
        BIX_BEGIN();
        hipLaunchKernelGGL(phi_bix_chunks_kernel, dim3(grid(n_chunks)), dim3(256), 0, st, R, n_rec, d_head_rec, n_chunks, d_chunks);
        hipLaunchKernelGGL(phi_bix_names_kernel, dim3(grid(n_ctg)), dim3(256), 0, st, L, d_rec_line, d_ctg_rec, n_ctg, d_names);
        hipLaunchKernelGGL(phi_bix_contigs_kernel, dim3(grid(n_rec)), dim3(256), 0, st, R, n_rec, d_ctg_rec, n_ctg, d_max_end);
        BIX_END_WAIT();
        std::vector<BixChunk> chunks((size_t)n_chunks);
        std::vector<BixName> names((size_t)n_ctg);
        std::vector<int32_t> max_end((size_t)n_ctg);
        DCHK(hipMemcpy(chunks.data(), d_chunks, (size_t)n_chunks * sizeof(BixChunk), hipMemcpyDeviceToHost));
        DCHK(hipMemcpy(names.data(), d_names, (size_t)n_ctg * sizeof(BixName), hipMemcpyDeviceToHost));
        DCHK(hipMemcpy(max_end.data(), d_max_end, (size_t)n_ctg * 4, hipMemcpyDeviceToHost));
        std::vector<std::string> name_list;
        for (const BixName &nm : names) {
            if (nm.at < 0 || nm.len < 0 || nm.len > bgzfx::MAX_NAME || nm.at + nm.len > n) return fail(info, PHI_ERR_DEVICE, "phi_deflate_bgzf_indexed: a contig name outside the text (internal error)");
            name_list.emplace_back((const char *)text + nm.at, (size_t)nm.len);
        }
        const int64_t again = bgzfx::repeated_name(name_list);
        if (again >= 0) return fail(info, PHI_ERR_INVALID, "phi_deflate_bgzf_indexed: contig %.100s comes back after another contig", name_list[(size_t)again].c_str());

        // ---- 5. windows
        std::vector<int64_t> w_base((size_t)n_ctg + 1, 0);
        for (int64_t c = 0; c < n_ctg; c++) {
            if (max_end[(size_t)c] < 1 || max_end[(size_t)c] > bgzfx::MAX_END) return fail(info, PHI_ERR_DEVICE, "phi_deflate_bgzf_indexed: contig %lld ends at %d (internal error)", (long long)c, max_end[(size_t)c]);
            w_base[(size_t)c + 1] = w_base[(size_t)c] + bgzfx::n_windows(max_end[(size_t)c]);
        }
        const int64_t n_win = w_base[(size_t)n_ctg];
        DALLOC(d_lin, unsigned long long, (size_t)n_win * 8);
        DCHK(hipMemcpyAsync(d_w_base, w_base.data(), (size_t)n_ctg * 8, hipMemcpyHostToDevice, st));
        DCHK(hipMemsetAsync(d_lin, 0xff, (size_t)n_win * 8, st));
        BIX_BEGIN();
        hipLaunchKernelGGL(phi_bix_windows_kernel, dim3(grid(n_rec)), dim3(256), 0, st, R, n_rec, d_w_base, d_lin);
        BIX_END_WAIT();
        std::vector<uint64_t> lin((size_t)n_win);
        DCHK(hipMemcpy(lin.data(), d_lin, (size_t)n_win * 8, hipMemcpyDeviceToHost));

        // ---- the host's share: chunks to their contigs, then bgzf_index_host.h
        contigs.resize((size_t)n_ctg);
        int64_t c = -1;
        for (const BixChunk &k : chunks) {
            if (k.new_ctg) c++;
            if (c < 0 || c >= n_ctg) return fail(info, PHI_ERR_DEVICE, "phi_deflate_bgzf_indexed: chunks and contigs disagree (internal error)");
            contigs[(size_t)c].chunks.push_back(bgzfx::Chunk{k.bin, k.beg, k.end});
        }
        for (c = 0; c < n_ctg; c++) {
            contigs[(size_t)c].name = name_list[(size_t)c];
            contigs[(size_t)c].lin.assign(lin.begin() + w_base[(size_t)c], lin.begin() + w_base[(size_t)c + 1]);
        }
    }
    *bytes = bgzfx::tbi_bytes(contigs, &counts);
    info->contigs = (int64_t)contigs.size();
    info->bins = counts.bins;
    info->chunks = counts.chunks;
    info->windows = counts.windows;
    return PHI_OK;
}

struct HostBuf {                                        // freed unless handed out
    uint8_t *p = nullptr;
    ~HostBuf() { free(p); }
    uint8_t *release() { uint8_t *q = p; p = nullptr; return q; }
};

int indexed_run(int32_t device, const uint8_t *in, int64_t n, int32_t flags, int32_t kind, void **out, int64_t *out_size, void **index, int64_t *index_size,
                phi_deflate_info *dinfo, phi_bgzf_index_info *info)
{
    Dev dev;
    const uint8_t *d_text = nullptr;
    if (kind == PHI_BGZF_INDEX_TBI_VCF && n > 0) {      // the text crosses the link once: the writer's batches read it here
        if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return fail(info, PHI_ERR_DEVICE, "phi_deflate_bgzf_indexed: no device %d", device); }
        DCHK(hipStreamCreateWithFlags(&dev.st, hipStreamNonBlocking));
        DCHK(hipEventCreate(&dev.ev[0]));
        DCHK(hipEventCreate(&dev.ev[1]));
        const size_t padded = (size_t)((n + BIX_WG - 1) / BIX_WG) * BIX_WG + 64;
        uint8_t *d = dev.alloc<uint8_t>(padded);
        if (!d) return fail(info, PHI_ERR_NOMEM, "phi_deflate_bgzf_indexed: the text (%lld bytes) does not fit the device", (long long)n);
        DCHK(hipMemcpyAsync(d, in, (size_t)n, hipMemcpyHostToDevice, dev.st));
        DCHK(hipStreamSynchronize(dev.st));
        d_text = d;
    }
    const int64_t bound = phi_deflate_bgzf_bound(n);
    HostBuf file, idx;
    if (!(file.p = (uint8_t *)malloc((size_t)bound))) return fail(info, PHI_ERR_NOMEM, "phi_deflate_bgzf_indexed: %lld bytes of host memory", (long long)bound);
    std::vector<int64_t> off;
    int64_t file_size = 0, idx_size = 0;
    int rc = phi_deflate_run(device, in, d_text, n, flags, file.p, &file_size, dinfo, &off);
    if (rc) return fail(info, rc, "%s", dinfo->detail);
    const int64_t nb = (int64_t)off.size() - 1;
    if (kind == PHI_BGZF_INDEX_GZI) {
        const std::vector<uint8_t> b = bgzfx::gzi_bytes(off.data(), nb);
        if (!(idx.p = (uint8_t *)malloc(b.size()))) return fail(info, PHI_ERR_NOMEM, "phi_deflate_bgzf_indexed: %zu bytes of host memory", b.size());
        memcpy(idx.p, b.data(), b.size());
        idx_size = (int64_t)b.size();
        info->chunks = nb > 1 ? nb - 1 : 0;
    } else {
        std::vector<uint8_t> b;
        if ((rc = tbi_run(dev, in, d_text, n, off, info, &b))) return rc;
        const int64_t ib = phi_deflate_bgzf_bound((int64_t)b.size());
        if (!(idx.p = (uint8_t *)malloc((size_t)ib))) return fail(info, PHI_ERR_NOMEM, "phi_deflate_bgzf_indexed: %lld bytes of host memory", (long long)ib);
        phi_deflate_info xi;
        if ((rc = phi_deflate_run(device, b.data(), nullptr, (int64_t)b.size(), 0, idx.p, &idx_size, &xi, nullptr))) return fail(info, rc, "%s", xi.detail);
    }
    info->index_bytes = idx_size;
    *out = file.release();
    *out_size = file_size;
    *index = idx.release();
    *index_size = idx_size;
    return PHI_OK;
}

}  // namespace

// the marks for the units that read VCF text on the device (vcf_lines_dev.h: bix_mark_run)
void phi_bix_mark_count(hipStream_t st, const uint8_t *d_text, int64_t n, int32_t *cnt, int64_t *off)
{
    const int64_t nblk = (n + BIX_WG - 1) / BIX_WG;
    hipLaunchKernelGGL(phi_bix_mark_count_kernel, dim3((unsigned)nblk), dim3(BIX_T), 0, st, d_text, n, nblk, cnt);
    for (int k = 0; k < 3; k++) phi_scan_tiles(st, cnt + k * nblk, nblk, off + k * (nblk + 1));
}

void phi_bix_mark_write(hipStream_t st, const uint8_t *d_text, int64_t n, const int64_t *off, int64_t *nl_pos, int64_t *nl_tab, int64_t *nl_end,
                        int64_t *tab_pos, int64_t *end_pos)
{
    const int64_t nblk = (n + BIX_WG - 1) / BIX_WG;
    hipLaunchKernelGGL(phi_bix_mark_write_kernel, dim3((unsigned)nblk), dim3(BIX_T), 0, st, d_text, n, nblk, off, nl_pos, nl_tab, nl_end, tab_pos, end_pos);
}

extern "C" int phi_deflate_bgzf_indexed(int32_t device, const void *in, int64_t n, int32_t flags, int32_t index_kind, void **out, int64_t *out_size,
                                        void **index, int64_t *index_size, phi_deflate_info *dinfo, phi_bgzf_index_info *info)
{
    phi_deflate_info d_local;
    phi_bgzf_index_info i_local;
    if (!dinfo) dinfo = &d_local;
    if (!info) info = &i_local;
    memset(dinfo, 0, sizeof(*dinfo));
    memset(info, 0, sizeof(*info));
    if (out) *out = nullptr;
    if (index) *index = nullptr;
    if (out_size) *out_size = 0;
    if (index_size) *index_size = 0;
    if (!out || !out_size || !index || !index_size || n < 0 || (n > 0 && !in)) return fail(info, PHI_ERR_INVALID, "phi_deflate_bgzf_indexed: null pointer or negative size");
    if (flags & ~(PHI_DEFLATE_NO_MATCH | PHI_DEFLATE_NO_EOF)) return fail(info, PHI_ERR_INVALID, "phi_deflate_bgzf_indexed: unknown flags 0x%x", (unsigned)flags);
    if (index_kind != PHI_BGZF_INDEX_GZI && index_kind != PHI_BGZF_INDEX_TBI_VCF)
        return fail(info, PHI_ERR_INVALID, "phi_deflate_bgzf_indexed: index_kind %d is neither PHI_BGZF_INDEX_GZI nor PHI_BGZF_INDEX_TBI_VCF", index_kind);
    if (flags & PHI_DEFLATE_NO_EOF) return fail(info, PHI_ERR_INVALID, "phi_deflate_bgzf_indexed: PHI_DEFLATE_NO_EOF with an index (its offsets are those of a whole file)");
    return indexed_run(device, (const uint8_t *)in, n, flags, index_kind, out, out_size, index, index_size, dinfo, info);
}
