// vcf_region.hip -- the records of one region out of the BGZF members an index points at: phi_vcf_region_filter.
//
// The host has planned which members to read (region_host.h); here they are inflated on the device (inflate.hip, told where every member
// begins: BGZF members are independent gzip members, decoded in parallel) and the exact filter runs over the BYTES of the inflated text:
//   1. MARKS    vcf_lines_dev.h, shared with the .tbi writer (bgzf_index.hip): newlines, tabs, END places as ascending lists.
//   2. LINES    one lane per line: does it start inside one of the ranges, is it a record, is its CHROM the name, does its
//               interval -- the .tbi writer's: bix_interval -- overlap [beg, end).  A range's first byte is a line's first byte
//               even where no newline stands before it (members that are not neighbours in the file are neighbours here).
//   3. OFFSETS  the kept lines compacted (scan.hip), their lengths scanned: where every line goes in the output.
//   4. COPY     divided over the OUTPUT bytes, 16 a lane, not over the lines: a line is 40 bytes or hundreds of kilobytes.  A
//               lane whose 16 bytes lie inside one line takes two aligned 16-byte loads and shifts; the others go byte by byte.
// The members go through in batches (PHI_VCF_REGION_BATCH), so device memory stays bounded; a batch that ends inside a line starts
// the next one at the member that holds that line's first byte, and a line is looked at in the one batch that holds its newline.
// Every loop is bounded: 16 bytes, 10 digits, the name's bytes, a bisection.  A refusal is the smallest (offset, reason) raised by
// any lane, so the message does not depend on the order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/phi_amd.h"
#include "phi_ctx.h"
#include "phi_wave.h"
#include "dev_run.h"
#include "vcf_lines_dev.h"
#include "region_host.h"

extern "C" int phi_inflate_to_device_starts(int32_t device, const void *in, int64_t n, int64_t chunk_bytes, const int64_t *starts, int64_t n_starts, int64_t sym_cap,
                                            void **d_out, int64_t *out_size, phi_inflate_info *info);      // inflate.hip

#define RGN_MIN_CHUNK 1024              // the smallest inflate chunk
#define RGN_SYM_CAP (3 * 65536 + 4096)  // a decoder's room on its first run: three BGZF members of text (one that crosses more runs again)
#define RGN_MAX_LINES 2147483646ll      // lines of a batch are numbered in 32 bits (the compaction's indices)
#define RGN_MAX_LINE 2147483646ll       // a kept line's bytes are counted in 32 bits (the scan's items)

namespace {

enum { RGN_FIELDS = 1, RGN_POS, RGN_END, RGN_LONG };

struct RgnQuery {                                       // device pointers and the region
    const int64_t *range;                               // [2 * n_ranges], coordinates of the whole planned text
    int32_t n_ranges;
    const uint8_t *name;
    int32_t name_len;
    int64_t beg, end;
    int64_t g0;                                         // where this batch's text begins in the planned text
    int64_t done;                                       // lines that begin before it were looked at by an earlier batch
};

// keep[i], and for a kept line where it begins in the batch's text and its bytes with the line feed; seen: lines inside a range
__global__ void __launch_bounds__(256) phi_rgn_lines_kernel(BixLists L, int64_t n_lines, RgnQuery Q, uint8_t *__restrict__ keep, int64_t *__restrict__ src,
                                                            int32_t *__restrict__ len, unsigned long long *__restrict__ err, unsigned long long *__restrict__ seen)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int mine = 0;
    if (i < n_lines) {
        BixLine l = bix_line(L, i);
        bool kept = false;
        const int64_t s_g = Q.g0 + l.s, e_g = Q.g0 + l.e;
        if (s_g >= Q.done && Q.n_ranges > 0) {
            // the last range that begins before the line's end (an empty line: at or before its only position)
            const int64_t bound = e_g > s_g ? e_g : s_g + 1;
            const int64_t lo = phi_first_ge_key((int64_t)0, (int64_t)Q.n_ranges, bound, [&Q](int64_t r) { return Q.range[2 * r]; });
            if (lo > 0) {
                const int64_t p0 = Q.range[2 * (lo - 1)], p1 = Q.range[2 * (lo - 1) + 1];
                const int64_t start = p0 > s_g ? p0 : s_g;
                if (start < p1) {
                    mine = 1;
                    if (p0 > s_g) {                     // the range begins inside what the newlines call one line: its line begins there
                        l.s = p0 - Q.g0;
                        l.tab_lo = phi_first_ge(L.tab_pos, l.tab_lo, l.tab_hi, l.s);
                        l.end_lo = phi_first_ge(L.end_pos, l.end_lo, l.end_hi, l.s);
                    }
                    const unsigned long long at = (unsigned long long)(Q.g0 + l.s) << 8;
                    if (l.e > l.s && L.text[l.s] == '#') {}
                    else if (l.tab_hi - l.tab_lo < 7) atomicMin(err, at | RGN_FIELDS);
                    else {
                        int64_t b = 0, e = 1, pos = -1;
                        const int bad = bix_interval(L, l, &b, &e, &pos);
                        if (bad) atomicMin(err, at | (bad == 1 ? RGN_POS : RGN_END));
                        else {
                            const int64_t nlen = L.tab_pos[l.tab_lo] - l.s;
                            bool same = nlen == Q.name_len;
                            for (int64_t k = 0; same && k < nlen; k++) same = L.text[l.s + k] == Q.name[k];
                            if (same && b < Q.end && e > Q.beg) {
                                if (l.e - l.s + 1 > RGN_MAX_LINE) atomicMin(err, at | RGN_LONG);
                                else { kept = true; src[i] = l.s; len[i] = (int32_t)(l.e - l.s + 1); }
                            }
                        }
                    }
                }
            }
        }
        keep[i] = kept;
    }
    const int total = phi_wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && total) atomicAdd(seen, (unsigned long long)total);
}

__global__ void __launch_bounds__(256) phi_rgn_gather_kernel(const int32_t *__restrict__ list, int64_t n_keep, const int64_t *__restrict__ src, const int32_t *__restrict__ len,
                                                             int64_t *__restrict__ ksrc, int32_t *__restrict__ klen)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_keep) return;
    ksrc[k] = src[list[k]];
    klen[k] = len[list[k]];
}

// out[16 g, 16 g + 16): kept line k goes to out[koff[k], koff[k + 1]), its last byte a line feed.  text[0, n) is readable to the
// next multiple of BIX_WG and 64 bytes beyond; out holds a multiple of 16 bytes
__global__ void __launch_bounds__(256) phi_rgn_copy_kernel(const uint8_t *__restrict__ text, int64_t n, const int64_t *__restrict__ ksrc, const int64_t *__restrict__ koff,
                                                           int64_t n_keep, int64_t total, uint8_t *__restrict__ out)
{
    const int64_t o = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (o >= total) return;
    int64_t k = phi_last_le(koff, n_keep, o);           // the last line that begins at or before o (koff[0] == 0)
    const int64_t a = ksrc[k] + (o - koff[k]);
    if (o + 16 <= koff[k + 1] && ksrc[k] + (koff[k + 1] - koff[k]) <= n) {      // inside one line whose line feed stands in the text
        const PhiText16 v = phi_load16_unaligned(text, a);
        *(uint4 *)(out + o) = uint4{v.x, v.y, v.z, v.w};
        return;
    }
    uint32_t w[4] = {0, 0, 0, 0};
    for (int j = 0; j < 16 && o + j < total; j++) {
        while (o + j >= koff[k + 1]) k++;               // (lines hold at least their line feed: at most 16 turns in all)
        const int64_t rel = o + j - koff[k];
        const uint8_t c = o + j + 1 == koff[k + 1] ? (uint8_t)'\n' : text[ksrc[k] + rel];
        w[j >> 2] |= (uint32_t)c << (8 * (j & 3));
    }
    *(uint4 *)(out + o) = uint4{w[0], w[1], w[2], w[3]};
}

inline unsigned grid(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

const char *why_text(int why)
{
    switch (why) {
    case RGN_FIELDS: return "a line with fewer than 8 fields";
    case RGN_POS: return "POS is empty, not all digits or longer than 10 digits";
    case RGN_END: return "the END of INFO is empty, not all digits or longer than 10 digits";
    case RGN_LONG: return "a record of 2^31 bytes or more";
    }
    return "internal error";
}

struct HostText {                                       // freed unless handed out
    char *p = nullptr;
    int64_t n = 0, cap = 0;
    ~HostText() { free(p); }
    bool room(int64_t more)
    {
        if (n + more + 1 <= cap) return true;
        const int64_t want = std::max<int64_t>(n + more + 1, cap * 2);
        char *q = (char *)realloc(p, (size_t)want);
        if (!q) return false;
        p = q;
        cap = want;
        return true;
    }
};

struct Batch { int64_t m0, m1; bool final; };

#define RGN_BEGIN() DCHK(hipEventRecord(dev.ev[0], st))
#define RGN_END_WAIT() do { DCHK(hipGetLastError()); DCHK(hipEventRecord(dev.ev[1], st)); DCHK(hipStreamSynchronize(st)); float ms_ = 0; \
                            (void)hipEventElapsedTime(&ms_, dev.ev[0], dev.ev[1]); info->filter_ms += ms_; } while (0)

// One batch: members [m0, m1) of the plan inflated and filtered, the kept lines appended to out.  *open_at: where the line
// begins that the batch ends inside (planned-text coordinates), or -1 when its text ends with a line feed or is the last
int batch_run(Dev &dev, int32_t device, const uint8_t *gz, const std::vector<regionx::Member> &mem, const std::vector<int64_t> &text_off, const Batch &b,
              RgnQuery Q, HostText &out, int64_t *open_at, phi_vcf_region_info *info)
{
    hipStream_t st = dev.st;
    *open_at = -1;
    const int64_t want = text_off[(size_t)b.m1] - text_off[(size_t)b.m0];
    const int64_t gz0 = mem[(size_t)b.m0].at, gz1 = mem[(size_t)b.m1 - 1].at + mem[(size_t)b.m1 - 1].size;
    phi_inflate_info inf;
    memset(&inf, 0, sizeof inf);
    void *d_raw = nullptr;
    int64_t n = 0;
    // phi_inflate cuts the COMPRESSED bytes into chunks, gives every chunk in which a block start is found one decoder, and its
    // finder takes no start in a member of one final block -- what a BGZF writer makes of 64 KiB of VCF text -- so such a file went
    // through ONE decoder (measured: 9.4 MB/s of text, whatever the chunk size).  The members' bounds are known here: chunks of
    // about a member's size, every chunk's start the first member that begins in it, and room for the members a decoder then
    // crosses on its first run (PHI_INFLATE_CHUNK from the environment still sets the chunk size)
    const int64_t nm = b.m1 - b.m0;
    const int64_t chunk = getenv("PHI_INFLATE_CHUNK") ? 0 : std::max<int64_t>(RGN_MIN_CHUNK, (gz1 - gz0) / nm);
    std::vector<int64_t> known((size_t)nm);
    for (int64_t k = 0; k < nm; k++) known[(size_t)k] = mem[(size_t)(b.m0 + k)].data_at - gz0;
    const int irc = phi_inflate_to_device_starts(device, gz + gz0, gz1 - gz0, chunk, known.data(), nm, RGN_SYM_CAP, &d_raw, &n, &inf);
    if (irc) return fail(info, irc, "%s", inf.detail);
    dev.bufs.push_back(d_raw);
    info->inflate_ms += inf.device_ms;
    if (n != want) return fail(info, PHI_ERR_INVALID, "phi_vcf_region_filter: members %lld..%lld inflate to %lld bytes, their ISIZE fields say %lld", (long long)b.m0,
                               (long long)b.m1 - 1, (long long)n, (long long)want);
    if (n == 0) return PHI_OK;
    DCHK(hipSetDevice(device));
    const size_t padded = (size_t)((n + BIX_WG - 1) / BIX_WG) * BIX_WG + 64;
    DALLOC(d_text, uint8_t, padded);
    DCHK(hipMemcpyAsync(d_text, d_raw, (size_t)n, hipMemcpyDeviceToDevice, st));
    uint8_t last = 0;
    DCHK(hipMemcpyAsync(&last, (const uint8_t *)d_raw + n - 1, 1, hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    dev.bufs.erase(std::find(dev.bufs.begin(), dev.bufs.end(), d_raw));      // (the unpadded copy: done with)
    (void)hipFree(d_raw);

    // ---- 1. marks
    BixLists L{};
    if (const int mrc = bix_mark_run(dev, d_text, n, &L, info, &info->filter_ms, "phi_vcf_region_filter")) return mrc;
    const bool open = last != '\n';
    const int64_t n_lines = L.n_nl + (open && b.final);
    if (open && !b.final) {
        int64_t nl = -1;
        if (L.n_nl) DCHK(hipMemcpy(&nl, L.nl_pos + L.n_nl - 1, 8, hipMemcpyDeviceToHost));
        *open_at = Q.g0 + nl + 1;
    }
    if (n_lines > RGN_MAX_LINES) return fail(info, PHI_ERR_UNSUPPORTED, "phi_vcf_region_filter: %lld lines in one batch, more than 2^31 - 2", (long long)n_lines);
    if (n_lines == 0) return PHI_OK;

    // ---- 2. lines
    DALLOC(d_keep, uint8_t, (size_t)n_lines);
    DALLOC(d_src, int64_t, (size_t)n_lines * 8);
    DALLOC(d_len, int32_t, (size_t)n_lines * 4);
    DALLOC(d_stat, unsigned long long, 16);              // [0] the smallest refusal, [1] lines inside a range
    const int64_t nscr = phi_compact_blocks(n_lines);
    DALLOC(d_blk_cnt, int32_t, (size_t)nscr * 4);
    DALLOC(d_blk_off, int64_t, (size_t)(nscr + 1) * 8);
    DCHK(hipMemsetAsync(d_stat, 0xff, 8, st));
    DCHK(hipMemsetAsync(d_stat + 1, 0, 8, st));
    RGN_BEGIN();
    hipLaunchKernelGGL(phi_rgn_lines_kernel, dim3(grid(n_lines)), dim3(256), 0, st, L, n_lines, Q, d_keep, d_src, d_len, d_stat, d_stat + 1);
    phi_compact_count(st, d_keep, n_lines, d_blk_cnt, d_blk_off);
    RGN_END_WAIT();
    unsigned long long stat[2] = {0, 0};
    int64_t n_keep = 0;
    DCHK(hipMemcpy(stat, d_stat, 16, hipMemcpyDeviceToHost));
    DCHK(hipMemcpy(&n_keep, d_blk_off + nscr, 8, hipMemcpyDeviceToHost));
    if (stat[0] != ~0ull) {
        const int why = (int)(stat[0] & 0xff);
        const int64_t at = (int64_t)(stat[0] >> 8);
        const int64_t m = (int64_t)(std::upper_bound(text_off.begin(), text_off.end(), at) - text_off.begin()) - 1;
        return fail(info, why == RGN_LONG ? PHI_ERR_UNSUPPORTED : PHI_ERR_INVALID, "phi_vcf_region_filter: the line at offset %lld of the inflated members (member %lld, byte %lld): %s",
                    (long long)at, (long long)m, (long long)(at - text_off[(size_t)std::max<int64_t>(m, 0)]), why_text(why));
    }
    if (n_keep < 0 || n_keep > n_lines) return fail(info, PHI_ERR_DEVICE, "phi_vcf_region_filter: %lld lines kept of %lld (internal error)", (long long)n_keep, (long long)n_lines);
    info->lines_seen += (int64_t)stat[1];
    info->lines_kept += n_keep;
    if (n_keep == 0) return PHI_OK;

    // ---- 3. offsets
    DALLOC(d_list, int32_t, (size_t)n_keep * 4);
    DALLOC(d_ksrc, int64_t, (size_t)n_keep * 8);
    DALLOC(d_klen, int32_t, (size_t)n_keep * 4);
    DALLOC(d_koff, int64_t, (size_t)(n_keep + 1) * 8);
    RGN_BEGIN();
    phi_compact_write(st, d_keep, n_lines, d_blk_off, d_list);
    hipLaunchKernelGGL(phi_rgn_gather_kernel, dim3(grid(n_keep)), dim3(256), 0, st, d_list, n_keep, d_src, d_len, d_ksrc, d_klen);
    phi_scan_tiles(st, d_klen, n_keep, d_koff);
    RGN_END_WAIT();
    int64_t total = 0;
    DCHK(hipMemcpy(&total, d_koff + n_keep, 8, hipMemcpyDeviceToHost));
    if (total < n_keep || total > n + 1) return fail(info, PHI_ERR_DEVICE, "phi_vcf_region_filter: %lld bytes kept of %lld (internal error)", (long long)total, (long long)n);

    // ---- 4. copy
    const int64_t n16 = (total + 15) / 16;
    DALLOC(d_out, uint8_t, (size_t)n16 * 16);
    RGN_BEGIN();
    hipLaunchKernelGGL(phi_rgn_copy_kernel, dim3(grid(n16)), dim3(256), 0, st, d_text, n, d_ksrc, d_koff, n_keep, total, d_out);
    RGN_END_WAIT();
    if (!out.room(total)) return fail(info, PHI_ERR_NOMEM, "phi_vcf_region_filter: %lld bytes of host memory", (long long)(out.n + total));
    DCHK(hipMemcpy(out.p + out.n, d_out, (size_t)total, hipMemcpyDeviceToHost));
    out.n += total;
    return PHI_OK;
}

int region_run(int32_t device, const uint8_t *gz, int64_t n_gz, const int64_t *range, int32_t n_ranges, const char *name, int64_t beg, int64_t end,
               char **text, int64_t *n_text, phi_vcf_region_info *info)
{
    // the members and where their text begins, from the bytes alone (region_host.h: nothing is inflated for this)
    std::vector<regionx::Member> mem;
    std::vector<int64_t> text_off(1, 0);
    const regionx::Bytes src{gz, n_gz};
    for (int64_t at = 0; at < n_gz;) {
        regionx::Member m;
        if (!regionx::member_at(src, at, &m)) return fail(info, PHI_ERR_INVALID, "phi_vcf_region_filter: no BGZF member at byte %lld of the compressed input", (long long)at);
        mem.push_back(m);
        text_off.push_back(text_off.back() + m.isize);
        at += m.size;
    }
    const int64_t M = (int64_t)mem.size(), total_text = text_off.back();
    for (int32_t r = 0; r < n_ranges; r++)
        if (range[2 * r] < (r ? range[2 * r - 1] : 0) || range[2 * r + 1] <= range[2 * r] || range[2 * r + 1] > total_text)
            return fail(info, PHI_ERR_INVALID, "phi_vcf_region_filter: range %d [%lld, %lld) is empty, out of order or beyond the members' %lld bytes", r, (long long)range[2 * r],
                        (long long)range[2 * r + 1], (long long)total_text);
    info->members = M;
    info->gz_bytes = n_gz;
    info->text_bytes = total_text;
    HostText out;
    if (!out.room(0)) return fail(info, PHI_ERR_NOMEM, "phi_vcf_region_filter: host memory");
    if (M > 0 && n_ranges > 0 && total_text > 0) {
        int64_t per = PHI_VCF_REGION_BATCH_DEFAULT;
        if (const char *e = getenv("PHI_VCF_REGION_BATCH")) per = atoll(e);
        per = std::max<int64_t>(1, std::min<int64_t>(per, 1 << 20));
        Dev dev;
        if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return fail(info, PHI_ERR_DEVICE, "phi_vcf_region_filter: no device %d", device); }
        DCHK(hipStreamCreateWithFlags(&dev.st, hipStreamNonBlocking));
        DCHK(hipEventCreate(&dev.ev[0]));
        DCHK(hipEventCreate(&dev.ev[1]));
        const size_t name_len = strlen(name);
        DALLOC(d_range, int64_t, (size_t)n_ranges * 16);
        DALLOC(d_name, uint8_t, name_len);
        DCHK(hipMemcpy(d_range, range, (size_t)n_ranges * 16, hipMemcpyHostToDevice));
        if (name_len) DCHK(hipMemcpy(d_name, name, name_len, hipMemcpyHostToDevice));
        const size_t kept_bufs = dev.bufs.size();
        RgnQuery Q{d_range, n_ranges, d_name, (int32_t)name_len, beg, end, 0, 0};
        int64_t m0 = 0, cur = per;
        while (m0 < M) {
            const Batch b{m0, std::min(M, m0 + cur), m0 + cur >= M};
            Q.g0 = text_off[(size_t)b.m0];
            int64_t open_at = -1;
            const int rc = batch_run(dev, device, gz, mem, text_off, b, Q, out, &open_at, info);
            if (rc) return rc;
            info->batches++;
            while (dev.bufs.size() > kept_bufs) { (void)hipFree(dev.bufs.back()); dev.bufs.pop_back(); }
            if (open_at < 0) { Q.done = text_off[(size_t)b.m1]; m0 = b.m1; cur = per; continue; }
            // the batch ends inside a line: the next begins at the member that holds that line's first byte
            Q.done = open_at;
            int64_t r = (int64_t)(std::upper_bound(text_off.begin() + b.m0, text_off.begin() + b.m1, open_at) - text_off.begin()) - 1;
            r = std::max(r, b.m0);
            cur = r == b.m0 ? cur * 2 : per;            // a line longer than the batch: a larger one from the same member
            info->reinflated_members += b.m1 - r;
            m0 = r;
        }
    }
    out.p[out.n] = 0;
    *text = out.p;
    *n_text = out.n;
    out.p = nullptr;
    return PHI_OK;
}

}  // namespace

extern "C" int phi_vcf_region_filter(int32_t device, const void *gz, int64_t n_gz, const int64_t *range, int32_t n_ranges, const char *name, int64_t beg, int64_t end,
                                     char **text, int64_t *n_text, phi_vcf_region_info *info)
{
    phi_vcf_region_info local;
    if (!info) info = &local;
    memset(info, 0, sizeof(*info));
    if (text) *text = nullptr;
    if (n_text) *n_text = 0;
    if (!text || !n_text || !name || n_gz < 0 || n_ranges < 0 || (n_gz > 0 && !gz) || (n_ranges > 0 && !range))
        return fail(info, PHI_ERR_INVALID, "phi_vcf_region_filter: null pointer or negative size");
    return region_run(device, (const uint8_t *)gz, n_gz, range, n_ranges, name, beg, end, text, n_text, info);
}

extern "C" void phi_vcf_region_free(char *text) { free(text); }
