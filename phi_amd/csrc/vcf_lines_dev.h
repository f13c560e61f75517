// vcf_lines_dev.h -- VCF text on the device as lists of positions, shared by the unit that indexes the text it writes
// (bgzf_index.hip) and the unit that filters the text it reads (vcf_region.hip).  The marks --
// every lane takes 16 bytes in one load and flags newlines, tabs and the places where "END=" follows a tab or ';' -- are counted,
// scanned and written as ascending lists by kernels that stay in bgzf_index.hip, which exports their launches; here are the
// lists' structure, a line's bounds and its tabs by index, a number of at most 10 digits, the interval of a record as
// include/phi_amd.h states it for the .tbi (device code in an unnamed namespace), and the host code that runs the marks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/phi_amd.h"
#include "phi_ctx.h"
#include "phi_wave.h"
#include "dev_run.h"
#include "text_bytes.h"

#define BIX_T 256                       // threads per workgroup
#define BIX_LANE 16                     // bytes per lane: one 16-byte load
#define BIX_WG (BIX_T * BIX_LANE)       // bytes per workgroup

// bgzf_index.hip, where the mark kernels live: their launches on a stream over scratch of the caller, nothing waited for.
// cnt[3 * nblk] and off[3 * (nblk + 1)] with nblk = ceil(n / BIX_WG): per workgroup the newlines, tabs and END places, and their
// scans (the list sizes are off[k * (nblk + 1) + nblk]); then the lists themselves, ascending
void phi_bix_mark_count(hipStream_t st, const uint8_t *d_text, int64_t n, int32_t *cnt, int64_t *off);
void phi_bix_mark_write(hipStream_t st, const uint8_t *d_text, int64_t n, const int64_t *off, int64_t *nl_pos, int64_t *nl_tab, int64_t *nl_end,
                        int64_t *tab_pos, int64_t *end_pos);

namespace {

// the position lists of phase 1 (device pointers) and their sizes
struct BixLists {
    const uint8_t *text;
    int64_t n;
    const int64_t *nl_pos, *nl_tab, *nl_end;            // per newline: where, and the tabs / END places before it
    const int64_t *tab_pos, *end_pos;
    int64_t n_nl, n_tab, n_end;
};
struct BixLine { int64_t s, e, tab_lo, tab_hi, end_lo, end_hi; };       // text[s, e) without its newline; its tabs, its END places

__device__ __forceinline__ BixLine bix_line(const BixLists &L, int64_t i)
{
    BixLine l;
    l.s = i ? L.nl_pos[i - 1] + 1 : 0;
    l.tab_lo = i ? L.nl_tab[i - 1] : 0;
    l.end_lo = i ? L.nl_end[i - 1] : 0;
    const bool closed = i < L.n_nl;                     // (the last line may have no newline)
    l.e = closed ? L.nl_pos[i] : L.n;
    l.tab_hi = closed ? L.nl_tab[i] : L.n_tab;
    l.end_hi = closed ? L.nl_end[i] : L.n_end;
    return l;
}

// text[a, b) as a number: 1 to 10 digits and nothing else, or -1
__device__ __forceinline__ int64_t bix_number(const uint8_t *__restrict__ text, int64_t a, int64_t b)
{
    const int64_t len = b - a;
    if (len < 1 || len > 10) return -1;
    int64_t v = 0;
    for (int64_t k = 0; k < len; k++) {
        const int c = text[a + k];
        if (c < '0' || c > '9') return -1;
        v = v * 10 + (c - '0');
    }
    return v;
}

// The interval of the record on line l (at least 8 fields: l.tab_hi - l.tab_lo >= 7): beg = max(POS - 1, 0), end = beg + len(REF)
// or the first END of INFO, an end <= beg becomes beg + 1.  0, or 1 for a malformed POS, 2 for a malformed END (*pos_out: POS, -1
// when malformed).
__device__ __forceinline__ int bix_interval(const BixLists &L, const BixLine &l, int64_t *beg_out, int64_t *end_out, int64_t *pos_out)
{
    const uint8_t *__restrict__ text = L.text;
    int64_t t[7];
#pragma unroll
    for (int k = 0; k < 7; k++) t[k] = L.tab_pos[l.tab_lo + k];
    const int64_t info_end = l.tab_hi - l.tab_lo > 7 ? L.tab_pos[l.tab_lo + 7] : l.e;
    const int64_t pos = bix_number(text, t[0] + 1, t[1]);
    *pos_out = pos;
    if (pos < 0) return 1;
    const int64_t beg = pos > 0 ? pos - 1 : 0;
    int64_t end = beg + (t[3] - t[2] - 1);
    int bad = 0;
    const int64_t lo = phi_first_ge(L.end_pos, l.end_lo, l.end_hi, t[6] + 1);     // the first END place at or behind INFO's first byte
    if (lo < l.end_hi && L.end_pos[lo] < info_end) {
        const int64_t a = L.end_pos[lo] + 4;
        int64_t b = a;
        while (b < info_end && b - a <= 10 && text[b] != ';') b++;
        const int64_t v = bix_number(text, a, b);
        if (v < 0) bad = 2;
        else end = v;
    }
    if (end <= beg) end = beg + 1;
    *beg_out = beg;
    *end_out = end;
    return bad;
}

// The marks of d_text[0, n), n > 0 (readable to the next multiple of BIX_WG and 64 bytes beyond): the lists allocated from dev and
// filled on its stream, *L set; *ms gains the GPU time by dev's events.  `what` stands in the messages.
template <class Info>
int bix_mark_run(Dev &dev, const uint8_t *d_text, int64_t n, BixLists *L, Info *info, double *ms, const char *what)
{
    hipStream_t st = dev.st;
    const int64_t nblk = (n + BIX_WG - 1) / BIX_WG;
    DALLOC(d_cnt, int32_t, (size_t)nblk * 3 * 4);
    DALLOC(d_cnt_off, int64_t, (size_t)(nblk + 1) * 3 * 8);
    float t = 0;
    DCHK(hipEventRecord(dev.ev[0], st));
    phi_bix_mark_count(st, d_text, n, d_cnt, d_cnt_off);
    DCHK(hipGetLastError());
    DCHK(hipEventRecord(dev.ev[1], st));
    DCHK(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&t, dev.ev[0], dev.ev[1]);
    *ms += t;
    int64_t total[3];
    for (int k = 0; k < 3; k++) DCHK(hipMemcpy(&total[k], d_cnt_off + k * (nblk + 1) + nblk, 8, hipMemcpyDeviceToHost));
    const int64_t n_nl = total[0], n_tab = total[1], n_end = total[2];
    if (n_nl < 0 || n_nl > n || n_tab < 0 || n_tab > n || n_end < 0 || n_end > n)
        return fail(info, PHI_ERR_DEVICE, "%s: %lld newlines, %lld tabs in %lld bytes (internal error)", what, (long long)n_nl, (long long)n_tab, (long long)n);
    DALLOC(d_nl_pos, int64_t, (size_t)n_nl * 8);
    DALLOC(d_nl_tab, int64_t, (size_t)n_nl * 8);
    DALLOC(d_nl_end, int64_t, (size_t)n_nl * 8);
    DALLOC(d_tab_pos, int64_t, (size_t)n_tab * 8);
    DALLOC(d_end_pos, int64_t, (size_t)n_end * 8);
    DCHK(hipEventRecord(dev.ev[0], st));
    phi_bix_mark_write(st, d_text, n, d_cnt_off, d_nl_pos, d_nl_tab, d_nl_end, d_tab_pos, d_end_pos);
    DCHK(hipGetLastError());
    DCHK(hipEventRecord(dev.ev[1], st));
    DCHK(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&t, dev.ev[0], dev.ev[1]);
    *ms += t;
    *L = BixLists{d_text, n, d_nl_pos, d_nl_tab, d_nl_end, d_tab_pos, d_end_pos, n_nl, n_tab, n_end};
    return PHI_OK;
}

}  // namespace
