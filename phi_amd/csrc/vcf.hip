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
#include <algorithm>
#include "phi_kernels.h"

#define VCF_TPB 256
#define VCF_TILE (VCF_TPB * 16)
#define VCF_MAX_WALK 4096

namespace {

struct VcfSeg { uint32_t nl, tabs; };                  // line feeds; tabs behind the last of them (all tabs when nl == 0)
__device__ __forceinline__ VcfSeg vcf_join(VcfSeg a, VcfSeg b) { return VcfSeg{a.nl + b.nl, b.nl ? b.tabs : a.tabs + b.tabs}; }

// the 16 bytes of a lane (zero behind the text's end) -> masks of its line feeds and tabs
__device__ __forceinline__ void vcf_masks(const uint8_t *__restrict__ text, int64_t n, int64_t at, uint32_t *nl_mask, uint32_t *tab_mask)
{
    uint32_t w[4] = {0, 0, 0, 0};
    if (at + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + at);      // (the buffer is 16-byte aligned, `at` a multiple of 16)
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        for (int i = 0; i < 16; i++)
            if (at + i < n) w[i >> 2] |= (uint32_t)text[at + i] << (8 * (i & 3));
    }
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
