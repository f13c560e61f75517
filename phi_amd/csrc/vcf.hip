// vcf.hip -- the two device stages of "set graph" from a phased VCF (the reference's vcf2gfa.py:27-64 route, phi_amd/vcf2gfa.py's
// rule; host side: csrc/host/vcf_reader.cpp).
//
// GENOTYPES.  The sample columns of a VCF are the bulk of its bytes.  The host lays the slices of the kept records back to back,
// one line feed behind each, so record and field of every byte follow from the text alone: record = line feeds before it,
// field = tabs since the last line feed.  Three launches over tiles of VCF_TILE bytes (VCF_TPB lanes x 16 bytes, one 16-byte
// load per lane, the tab / line-feed masks of a lane in two 16-bit words):
//     summary   per tile: line feeds, and tabs behind the last one (all of them when the tile holds none)
//     carry     one workgroup joins the tile summaries (a run of tiles per lane, one scan): record and field at every tile's first byte
//     parse     the same masks again, a segmented scan over the workgroup's lanes (the operator of the summaries), then every lane
//               takes the fields that BEGIN behind a delimiter of its 16 bytes: field s < n_samples of record r is read from
//               there -- gi ':' skipped, the GT part split at '|' / '/', two decimal values -- and gt[r][s] and ploidy[s] are
//               written.  A field is a few bytes; a slice may be four bytes or tens of kilobytes and never has to fit anything.
// What the kernel does not decide it flags per record, and the host's scalar parser (phi_vcf_parse_gt) fills that row: a value
// of more than four digits (the matrix holds 16 bits), fewer fields than samples or fewer ':' parts than GT's index (errors
// there), a GT part not closed within VCF_MAX_WALK bytes.  Algorithmic bytes: the text once + 4 bytes per record and sample.
//
// WALKS.  Every kept haplotype's walk over UNITS (backbone, its allele, backbone, ...: 2 * sites + 1 entries) from the choice
// matrix; chop.hip's count / scan / expand then turns units into segment ids with unit_first in the place of first.
#include <string.h>
#include <algorithm>
#include "phi_ctx.h"
#include "text_bytes.h"

#define VCF_TPB 256
#define VCF_TILE (VCF_TPB * 16)
#define VCF_MAX_WALK 4096

namespace {

struct VcfSeg { uint32_t nl, tabs; };                  // line feeds; tabs behind the last of them (all tabs when nl == 0)
__device__ __forceinline__ VcfSeg vcf_join(VcfSeg a, VcfSeg b) { return VcfSeg{a.nl + b.nl, b.nl ? b.tabs : a.tabs + b.tabs}; }

// the 16 bytes of a lane (the tail-safe load: the buffer ends with the text, and bytes behind it read as zero) -> masks of its line
// feeds and tabs, formed byte by byte: for two characters at once this measured faster than phi_eq16 (profiles/text_bytes_ab.json)
__device__ __forceinline__ void vcf_masks(const uint8_t *__restrict__ text, int64_t n, int64_t at, uint32_t *nl_mask, uint32_t *tab_mask)
{
    const PhiText16 v = phi_load16_tail(text, at, n);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t nl = 0, tab = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        nl |= (uint32_t)(b == '\n') << i;
        tab |= (uint32_t)(b == '\t') << i;
    }
    *nl_mask = nl; *tab_mask = tab;
}

__device__ __forceinline__ VcfSeg vcf_lane_seg(uint32_t nl_mask, uint32_t tab_mask)
{
    if (!nl_mask) return VcfSeg{0u, (uint32_t)__popc(tab_mask)};
    const int last = 31 - __clz(nl_mask);
    return VcfSeg{(uint32_t)__popc(nl_mask), (uint32_t)__popc(tab_mask >> (last + 1))};
}

// inclusive segmented scan over the workgroup's lanes (Hillis-Steele through LDS); returns the EXCLUSIVE value of the lane
__device__ VcfSeg vcf_block_scan(VcfSeg mine, VcfSeg *s_a, VcfSeg *s_b, VcfSeg *total)
{
    const int tid = threadIdx.x;
    VcfSeg *src = s_a, *dst = s_b;
    src[tid] = mine;
    __syncthreads();
    for (int d = 1; d < VCF_TPB; d <<= 1) {
        VcfSeg v = src[tid];
        if (tid >= d) v = vcf_join(src[tid - d], v);
        dst[tid] = v;
        __syncthreads();
        VcfSeg *t = src; src = dst; dst = t;
    }
    *total = src[VCF_TPB - 1];
    const VcfSeg ex = tid ? src[tid - 1] : VcfSeg{0u, 0u};
    __syncthreads();
    return ex;
}

__global__ void __launch_bounds__(VCF_TPB) vcf_summary_kernel(const uint8_t *__restrict__ text, int64_t n, VcfSeg *__restrict__ tile_seg)
{
    __shared__ VcfSeg s_a[VCF_TPB], s_b[VCF_TPB];
    const int64_t at = (int64_t)blockIdx.x * VCF_TILE + (int64_t)threadIdx.x * 16;
    uint32_t nl, tab;
    vcf_masks(text, n, at, &nl, &tab);
    VcfSeg total;
    (void)vcf_block_scan(vcf_lane_seg(nl, tab), s_a, s_b, &total);
    if (threadIdx.x == 0) tile_seg[blockIdx.x] = total;
}

// one workgroup: tile_seg[t] <- (record, field) at the first byte of tile t; the last carry to tile_seg[n_tiles].  Every lane
// joins a run of consecutive tiles, one scan over the 256 run totals, then every lane walks its run again with its prefix:
// one pass whatever the text's length (two 8-byte loads and a store per tile, no barrier per 256 tiles)
__global__ void __launch_bounds__(VCF_TPB) vcf_carry_kernel(VcfSeg *__restrict__ tile_seg, int64_t n_tiles)
{
    __shared__ VcfSeg s_a[VCF_TPB], s_b[VCF_TPB];
    const int64_t per = (n_tiles + VCF_TPB - 1) / VCF_TPB;
    const int64_t lo = min(n_tiles, (int64_t)threadIdx.x * per), hi = min(n_tiles, lo + per);
    VcfSeg mine{0u, 0u};
    for (int64_t t = lo; t < hi; t++) mine = vcf_join(mine, tile_seg[t]);
    VcfSeg total;
    VcfSeg run = vcf_block_scan(mine, s_a, s_b, &total);
    for (int64_t t = lo; t < hi; t++) {
        const VcfSeg here = tile_seg[t];
        tile_seg[t] = run;
        run = vcf_join(run, here);
    }
    if (threadIdx.x == 0) tile_seg[n_tiles] = total;
}

struct VcfParseArgs {
    const uint8_t *text; int64_t n;
    const VcfSeg *tile_pre;
    const int32_t *gi;                                 // per record: index of GT in FORMAT
    int64_t n_rec; int32_t n_samples;
    uint16_t *gt; int32_t *ploidy; uint8_t *flag;      // flag[r] != 0: the row of record r is the host's to fill
    uint32_t *err;                                     // more line feeds than records (the layout is not the reader's)
};

// the field that begins at text[p]: sample s of record r
__device__ void vcf_field(const VcfParseArgs &A, int64_t p, uint32_t r, uint32_t s)
{
    const uint8_t *__restrict__ text = A.text;
    int32_t skip = A.gi[r];
    int budget = VCF_MAX_WALK;
    // (every walk ends at a line feed at the latest, and the text's last byte is one)
    while (skip > 0) {
        const uint32_t ch = text[p];
        if (ch == '\t' || ch == '\n' || --budget < 0) { A.flag[r] = 1; return; }      // fewer ':' parts than GT's index: the host says so
        if (ch == ':') skip--;
        p++;
    }
    uint32_t val[2] = {0, 0};
    int part = 0, n_called = 0;
    bool odd = false;
    for (;;) {
        uint32_t v = 0;
        int len = 0;
        bool digits = true, dot = false;
        uint32_t ch;
        for (;;) {
            ch = text[p];
            if (ch == '|' || ch == '/' || ch == ':' || ch == '\t' || ch == '\n') break;
            if (--budget < 0) { A.flag[r] = 1; return; }
            dot = len == 0 && ch == '.';
            if (ch >= '0' && ch <= '9') v = v * 10 + (ch - '0'); else digits = false;
            if (len < 8) len++; else digits = false, odd = odd || part < 2;          // (no wrap of v: nine digits and more are the host's)
            p++;
        }
        if (!(len == 1 && dot)) n_called++;
        if (part < 2) {
            if (digits && len > 4) odd = true;                                      // may not fit 16 bits
            val[part] = (digits && len > 0) ? v : 0;
        }
        part++;
        if (ch != '|' && ch != '/') break;
        p++;
    }
    if (odd) { A.flag[r] = 1; return; }
    uint16_t *o = A.gt + ((size_t)r * (size_t)A.n_samples + s) * 2;
    *reinterpret_cast<uint32_t *>(o) = val[0] | (val[1] << 16);
    const int32_t pl = n_called < 2 ? n_called : 2;
    if (A.ploidy[s] < pl) atomicMax(A.ploidy + s, pl);
}

__global__ void __launch_bounds__(VCF_TPB) vcf_parse_kernel(const VcfParseArgs A)
{
    __shared__ VcfSeg s_a[VCF_TPB], s_b[VCF_TPB];
    const int64_t at = (int64_t)blockIdx.x * VCF_TILE + (int64_t)threadIdx.x * 16;
    uint32_t nl, tab;
    vcf_masks(A.text, A.n, at, &nl, &tab);
    VcfSeg total;
    const VcfSeg ex = vcf_block_scan(vcf_lane_seg(nl, tab), s_a, s_b, &total);
    const VcfSeg here = vcf_join(A.tile_pre[blockIdx.x], ex);
    uint32_t r = here.nl, s = here.tabs;
    if (at == 0 && A.n > 0 && A.n_samples > 0) vcf_field(A, 0, 0, 0);               // the text's first field stands behind no delimiter
    uint32_t m = nl | tab;
    while (m) {
        const int i = __ffs(m) - 1;
        m &= m - 1;
        if ((nl >> i) & 1u) {
            if (r >= A.n_rec) { *A.err = 1u; return; }
            if (s + 1 < (uint32_t)A.n_samples) A.flag[r] = 1;                       // fewer fields than samples: the host says so
            r++; s = 0;
        } else s++;
        const int64_t p = at + i + 1;
        if (p < A.n && s < (uint32_t)A.n_samples) {
            if (r >= A.n_rec) { *A.err = 1u; return; }
            vcf_field(A, p, r, s);
        }
    }
}

// entry j of kept haplotype h's walk over units: site backbone, its allele, ..., the last backbone
__global__ void __launch_bounds__(256) vcf_unit_walks_kernel(const int32_t *__restrict__ site_backbone, const int32_t *__restrict__ site_allele0,
                                                             const int32_t *__restrict__ choice, int64_t n_sites, int32_t n_haps, int32_t last_unit,
                                                             int32_t *__restrict__ out)
{
    const int64_t per = 2 * n_sites + 1, n = per * n_haps;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int64_t h = e / per, j = e - h * per, site = j >> 1;
        int32_t u;
        if (j == per - 1) u = last_unit;
        else if (j & 1) u = site_allele0[site] + choice[site * n_haps + h];
        else u = site_backbone[site];
        out[e] = u;
    }
}

}  // namespace

int64_t phi_vcf_num_tiles(int64_t n_bytes) { return (n_bytes + VCF_TILE - 1) / VCF_TILE; }

// text: 16-byte aligned, n bytes, the last one a line feed; tile_seg: [tiles + 1] pairs of uint32; gt [n_rec][n_samples][2],
// ploidy [n_samples] and flag [n_rec] zeroed by the caller
void phi_launch_vcf_genotypes(hipStream_t st, const uint8_t *text, int64_t n, void *tile_seg, const int32_t *gt_index, int64_t n_rec, int32_t n_samples,
                              uint16_t *gt, int32_t *ploidy, uint8_t *flag, uint32_t *err)
{
    const int64_t n_tiles = phi_vcf_num_tiles(n);
    if (n_tiles <= 0) return;
    VcfSeg *seg = static_cast<VcfSeg *>(tile_seg);
    hipLaunchKernelGGL(vcf_summary_kernel, dim3((unsigned)n_tiles), dim3(VCF_TPB), 0, st, text, n, seg);
    hipLaunchKernelGGL(vcf_carry_kernel, dim3(1), dim3(VCF_TPB), 0, st, seg, n_tiles);
    const VcfParseArgs A{text, n, seg, gt_index, n_rec, n_samples, gt, ploidy, flag, err};
    hipLaunchKernelGGL(vcf_parse_kernel, dim3((unsigned)n_tiles), dim3(VCF_TPB), 0, st, A);
}

void phi_launch_vcf_unit_walks(hipStream_t st, const int32_t *site_backbone, const int32_t *site_allele0, const int32_t *choice, int64_t n_sites,
                               int32_t n_haps, int32_t last_unit, int32_t *out)
{
    const int64_t n = (2 * n_sites + 1) * n_haps;
    if (n <= 0) return;
    const unsigned nb = (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(vcf_unit_walks_kernel, dim3(nb), dim3(256), 0, st, site_backbone, site_allele0, choice, n_sites, n_haps, last_unit, out);
}

// ---- host side (C ABI of include/phi_amd.h)

extern "C" {

// vcf2gfa.py:27-64, the sample columns: the text of the kept records' slices to the device, the genotype kernel (vcf.hip) over it,
// matrix, ploidy and the per-record flags back.
int phi_vcf_genotypes(phi_ctx *c, const char *text, int64_t n_text, const int64_t *text_off, const int32_t *gt_index, int64_t n_records,
                      int32_t n_samples, uint16_t *gt, int32_t *ploidy, uint8_t *flagged)
{
    if (!c) return PHI_ERR_INVALID;
    if (n_text < 0 || n_records < 0 || n_samples < 0 || !text_off || (n_records > 0 && (!text || !gt_index || !flagged)) ||
        (n_samples > 0 && !ploidy) || (n_records > 0 && n_samples > 0 && !gt))
        return phi_fail(c, PHI_ERR_INVALID, "phi_vcf_genotypes: null pointer or negative size");
    // the layout the kernel relies on: slices back to back, one line feed behind each and nowhere else
    if (text_off[0] != 0 || text_off[n_records] != n_text) return phi_fail(c, PHI_ERR_INVALID, "phi_vcf_genotypes: the offsets do not cover the text");
    for (int64_t r = 0; r < n_records; r++)
        if (text_off[r + 1] <= text_off[r] || text[text_off[r + 1] - 1] != '\n')
            return phi_fail(c, PHI_ERR_INVALID, "phi_vcf_genotypes: the slice of record %lld is not followed by a line feed", (long long)r);
    // (the text, the matrix and the flags have to fit device memory side by side: phi_dev_ensure says so where they do not;
    //  this only keeps the record index in 32 bits and the grid within what a launch takes)
    if (n_records >= ((int64_t)1 << 31) || phi_vcf_num_tiles(n_text) >= ((int64_t)1 << 31))
        return phi_fail(c, PHI_ERR_UNSUPPORTED, "phi_vcf_genotypes: 2^31 kept records and more");
    HIPCHK(hipSetDevice(c->device));
    PhiStageTimer tm("vcf genotypes");
    c->vcf.have = false;
    phi_vcf_info info{};
    info.text_bytes = n_text; info.n_records = n_records; info.n_samples = n_samples;
    for (int32_t s = 0; s < n_samples; s++) ploidy[s] = 0;
    if (n_records > 0) memset(flagged, 0, (size_t)n_records);
    if (n_records == 0 || n_samples == 0) { c->vcf.info = info; c->vcf.have = true; return PHI_OK; }
    const size_t n_cells = (size_t)n_records * (size_t)n_samples;
    const int64_t n_tiles = phi_vcf_num_tiles(n_text);
    DevBuf d_text, d_seg, d_gi, d_gt, d_ploidy, d_flag, d_err;
    PhiDevGuard guard{{&d_text, &d_seg, &d_gi, &d_gt, &d_ploidy, &d_flag, &d_err}};
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int i = 0; i < 2; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
    for (int i = 0; i < 2; i++) HIPCHK(hipEventCreate(&ev[i]));
    PHICHK(upload(c, d_text, text, (size_t)n_text));
    PHICHK(upload(c, d_gi, gt_index, (size_t)n_records));
    PHICHK(phi_dev_ensure(c, d_seg, ((size_t)n_tiles + 1) * 8));
    PHICHK(phi_dev_ensure(c, d_gt, n_cells * 4));
    PHICHK(phi_dev_ensure(c, d_ploidy, (size_t)n_samples * 4));
    PHICHK(phi_dev_ensure(c, d_flag, (size_t)n_records));
    PHICHK(phi_dev_ensure(c, d_err, 4));
    HIPCHK(hipMemsetAsync(d_gt.p, 0, n_cells * 4, c->stream));
    HIPCHK(hipMemsetAsync(d_ploidy.p, 0, (size_t)n_samples * 4, c->stream));
    HIPCHK(hipMemsetAsync(d_flag.p, 0, (size_t)n_records, c->stream));
    HIPCHK(hipMemsetAsync(d_err.p, 0, 4, c->stream));
    tm.lap("text to the device");
    HIPCHK(hipEventRecord(ev[0], c->stream));
    phi_launch_vcf_genotypes(c->stream, d_text.as<uint8_t>(), n_text, d_seg.p, d_gi.as<int32_t>(), n_records, n_samples, d_gt.as<uint16_t>(),
                             d_ploidy.as<int32_t>(), d_flag.as<uint8_t>(), d_err.as<uint32_t>());
    HIPCHK(hipEventRecord(ev[1], c->stream));
    uint32_t kerr = 0;
    HIPCHK(hipMemcpyAsync(gt, d_gt.p, n_cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ploidy, d_ploidy.p, (size_t)n_samples * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(flagged, d_flag.p, (size_t)n_records, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&kerr, d_err.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    if (kerr) return phi_fail(c, PHI_ERR_INVALID, "phi_vcf_genotypes: a line feed inside a slice (the text is not laid out as phi_vcf_read lays it out)");
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    info.genotype_gpu_ms = ms;
    for (int64_t r = 0; r < n_records; r++) info.n_flagged += flagged[r] != 0;
    tm.lap("genotype kernel, matrix back");
    c->vcf.info = info; c->vcf.have = true;
    return PHI_OK;
}

// vcf2gfa.py:27-64, the W-lines that are never written: every kept haplotype's walk over units from the choice matrix
// (vcf.hip), then chop.hip's count / scan / expand with unit_first in the place of first; the entries and their offsets
// are left where phi_walk_text_resolve leaves them.
static int vcf_walks(phi_ctx *c, const int32_t *unit_first, int64_t n_units, const int32_t *site_backbone, const int32_t *site_allele0,
                     int64_t n_sites, const int32_t *choice, int32_t n_haps, int64_t *walk_off_out, int32_t max_haps)
{
    if (!c) return PHI_ERR_INVALID;
    if (!unit_first || !walk_off_out || n_units < 1 || n_sites < 0 || n_haps < 1 || (n_sites > 0 && (!site_backbone || !site_allele0 || !choice)))
        return phi_fail(c, PHI_ERR_INVALID, "phi_vcf_walks: null pointer or empty table");
    if (n_units > INT32_MAX - 1 || n_units < 2 * n_sites + 1) return phi_fail(c, PHI_ERR_INVALID, "phi_vcf_walks: %lld units for %lld sites", (long long)n_units, (long long)n_sites);
    if (n_haps > max_haps) return phi_fail(c, PHI_ERR_UNSUPPORTED, "more than %d walks", max_haps);
    if (unit_first[0] != 0) return phi_fail(c, PHI_ERR_INVALID, "phi_vcf_walks: unit_first must start at 0");
    for (int64_t u = 0; u < n_units; u++)
        if (unit_first[u + 1] <= unit_first[u]) return phi_fail(c, PHI_ERR_INVALID, "phi_vcf_walks: unit %lld holds no segment", (long long)u);
    const int64_t per = 2 * n_sites + 1, n_in = per * n_haps;
    if (n_in > PHI_MAX_ENTRIES) return phi_fail(c, PHI_ERR_UNSUPPORTED, "more than 2^32 - 64 walk entries");
    HIPCHK(hipSetDevice(c->device));
    PhiStageTimer tm("vcf walks");
    DevBuf d_sb, d_sa, d_choice, d_units, d_out;
    PhiDevGuard guard{{&d_sb, &d_sa, &d_choice, &d_units, &d_out}};
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int i = 0; i < 2; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
    for (int i = 0; i < 2; i++) HIPCHK(hipEventCreate(&ev[i]));
    PHICHK(upload(c, d_sb, site_backbone, (size_t)n_sites));
    PHICHK(upload(c, d_sa, site_allele0, (size_t)n_sites));
    PHICHK(upload(c, d_choice, choice, (size_t)n_sites * (size_t)n_haps));
    PHICHK(phi_dev_ensure(c, d_units, (size_t)n_in * 4));
    HIPCHK(hipEventRecord(ev[0], c->stream));
    phi_launch_vcf_unit_walks(c->stream, d_sb.as<int32_t>(), d_sa.as<int32_t>(), d_choice.as<int32_t>(), n_sites, n_haps, (int32_t)n_units - 1,
                              d_units.as<int32_t>());
    HIPCHK(hipEventRecord(ev[1], c->stream));
    std::vector<int64_t> woff_in((size_t)n_haps + 1), walk_off2;
    for (int32_t h = 0; h <= n_haps; h++) woff_in[(size_t)h] = per * h;
    std::vector<int32_t> ends;
    int64_t n_out = 0;
    double expand_ms = 0.0;
    // (a choice beyond its site's alleles names a unit of the next site or none at all: the count reports the latter as a vertex out of range)
    PHICHK(chop_expand_entries(c, d_units.as<int32_t>(), n_in, unit_first, (int32_t)n_units, woff_in.data(), n_haps, 0, d_out, walk_off2, ends, &n_out, &expand_ms));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    // (only now: after a refusal above, walks an earlier phi_walk_text_resolve / phi_vcf_walks left on the device are as they were)
    std::swap(c->d_walk_vtx, d_out);                           // (the guard lets the entries the context held go)
    c->wtext.ends.swap(ends);
    c->walks_on_device = true;
    c->walks_on_device_n = n_out;
    memcpy(walk_off_out, walk_off2.data(), walk_off2.size() * 8);
    c->vcf.info.n_units = n_units;
    c->vcf.info.n_entries = n_out;
    c->vcf.info.walks_gpu_ms = (double)ms + expand_ms;
    c->vcf.have = true;
    tm.lap("unit walks, count, scan, expand");
    return PHI_OK;
}

int phi_vcf_walks(phi_ctx *c, const int32_t *unit_first, int64_t n_units, const int32_t *site_backbone, const int32_t *site_allele0,
                  int64_t n_sites, const int32_t *choice, int32_t n_haps, int64_t *walk_off_out)
{
    return vcf_walks(c, unit_first, n_units, site_backbone, site_allele0, n_sites, choice, n_haps, walk_off_out, PHI_DP_MAX_WALKS);
}

// every haplotype of a population VCF, for phi_scout_graph (set_graph.hip): the same body, the scout's limit
int phi_vcf_walks_wide(phi_ctx *c, const int32_t *unit_first, int64_t n_units, const int32_t *site_backbone, const int32_t *site_allele0,
                       int64_t n_sites, const int32_t *choice, int32_t n_haps, int64_t *walk_off_out)
{
    return vcf_walks(c, unit_first, n_units, site_backbone, site_allele0, n_sites, choice, n_haps, walk_off_out, PHI_SCOUT_MAX_WALKS);
}

int phi_vcf_stats(phi_ctx *c, phi_vcf_info *out)
{
    if (!c || !out) return PHI_ERR_INVALID;
    if (!c->vcf.have) return phi_fail(c, PHI_ERR_STATE, "phi_vcf_stats: no phi_vcf_genotypes / phi_vcf_walks on this context");
    *out = c->vcf.info;
    return PHI_OK;
}

}  // extern "C"
