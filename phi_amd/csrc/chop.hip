// chop.hip -- the walk entries of a graph whose vertices are chopped into pieces of at most N bases, made ON THE DEVICE.
//
// The reference's pipeline never hands PHI a graph as the graph builder wrote it: an external tool chops every segment to
// at most 30 bases first (data/chop_graph.sh:3 `hal2vg --chop 30`, :62-66 `gfa2gbwt -m 30`), because the model lets the path
// switch haplotypes at vertex borders only and ignores every anchor inside one vertex (ILP_index.cpp:795/:846).
// phi_set_graph_chopped (phi_abi.hip) does that step inside "set graph".  The per-vertex arrays are small and are chopped on
// the host; the walk entries multiply (a 1-kbp segment is 34 pieces at N = 30) and at chromosome scale exist only in HBM,
// so they are expanded where they lie:
//     count    pieces of every entry's vertex (first[v + 1] - first[v]); an entry outside [0, n_vtx) is reported
//     scan     64-bit exclusive scan of the counts (phi_launch_scan_i64 of dp_events.hip) = where every entry's pieces go
//     expand   a workgroup owns a tile of CHOP_TILE consecutive OUTPUT entries -- one input entry may become a million
//              outputs and the next one a single one --, finds the input entries that cover the tile (one search of the
//              scanned offsets per tile, all lanes probing), stages their starts and first pieces in LDS, and every lane
//              writes four consecutive entries with one 16-byte store
//     walks    the new walk offsets and the first / last piece of every walk (what the host pass of set_graph looks at)
// The expansion is bound by HBM: 4 bytes written per output entry; per INPUT entry 8 bytes of offsets, 4 of the entry and
// one gather into first[].
#include <algorithm>
#include "phi_kernels.h"

#define CHOP_TILE 4096
#define CHOP_TPB 256

namespace {

__global__ void __launch_bounds__(256) chop_count_kernel(const int32_t *__restrict__ walk_vtx, int64_t n, const int32_t *__restrict__ first,
                                                         int32_t n_vtx, int32_t *__restrict__ cnt, unsigned long long *__restrict__ bad)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int32_t v = walk_vtx[e];
        int32_t k = 1;
        if ((uint32_t)v >= (uint32_t)n_vtx) atomicMin(bad, (unsigned long long)e);      // (the smallest such entry: the one the host names)
        else k = first[v + 1] - first[v];
        cnt[e] = k;
    }
}

__global__ void __launch_bounds__(CHOP_TPB) chop_expand_kernel(const int32_t *__restrict__ walk_vtx, const int64_t *__restrict__ off, int64_t n_in,
                                                               const int32_t *__restrict__ first, int32_t *__restrict__ out, int64_t n_out)
{
    // per covering input entry: where its pieces start relative to the tile (negative for an entry that began before it)
    // and first piece - start, so that output q of the tile is s_base + q (unsigned: the true value fits, the parts wrap)
    __shared__ int32_t s_start[CHOP_TILE];
    __shared__ uint32_t s_base[CHOP_TILE];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * CHOP_TILE;
    const int64_t t1 = min(n_out, t0 + CHOP_TILE);
    if (t0 >= n_out) return;
    // the last input entry whose pieces start at or before t0: 256 probes a round over [lo, hi), off[lo] <= t0 throughout
    int64_t lo = 0, hi = n_in;
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + CHOP_TPB - 1) / CHOP_TPB;
        const int64_t idx = lo + tid * step;
        const int n_le = __syncthreads_count(idx < hi && off[idx] <= t0);      // (off ascends: the lanes that say yes are the first n_le)
        lo += (n_le - 1) * step;
        hi = min(hi, lo + step);
    }
    // stage the entries that start before the tile's end (each holds at least one piece: at most CHOP_TILE of them)
    int n_cov = 0;
    for (int b = 0; b < CHOP_TILE; b += CHOP_TPB) {
        const int64_t e = lo + b + tid;
        bool ok = false;
        if (e < n_in) {
            const int64_t o = off[e];
            if (o < t1) {
                ok = true;
                const int32_t st = (int32_t)(o - t0);
                s_start[b + tid] = st;
                s_base[b + tid] = (uint32_t)first[walk_vtx[e]] - (uint32_t)st;
            }
        }
        const int n_ok = __syncthreads_count(ok);
        n_cov += n_ok;
        if (n_ok < CHOP_TPB) break;
    }
    const int p2 = n_cov > 1 ? 1 << (31 - __clz(n_cov - 1)) : 0;
    const int n_here = (int)(t1 - t0);
    for (int q0 = tid * 4; q0 < n_here; q0 += CHOP_TPB * 4) {
        int i = 0;
        for (int s = p2; s; s >>= 1) {
            const int m = i + s;
            if (m < n_cov && s_start[m] <= q0) i = m;
        }
        uint32_t val[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int q = q0 + j;
            if (j && i + 1 < n_cov && s_start[i + 1] <= q) i++;                 // (starts ascend strictly: one step at most)
            val[j] = s_base[i] + (uint32_t)q;
        }
        int32_t *dst = out + t0 + q0;
        if (q0 + 4 <= n_here) {
            *reinterpret_cast<int4 *>(dst) = make_int4((int)val[0], (int)val[1], (int)val[2], (int)val[3]);
        } else {
            for (int j = 0; q0 + j < n_here; j++) dst[j] = (int32_t)val[j];
        }
    }
}

__global__ void __launch_bounds__(256) chop_walks_kernel(const int32_t *__restrict__ walk_vtx, const int64_t *__restrict__ off,
                                                         const int64_t *__restrict__ walk_off, int32_t n_walks, const int32_t *__restrict__ first,
                                                         int64_t *__restrict__ walk_off_out, int32_t *__restrict__ ends)
{
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h > n_walks) return;
    walk_off_out[h] = off[walk_off[h]];
    if (h < n_walks) {
        ends[2 * h] = first[walk_vtx[walk_off[h]]];
        ends[2 * h + 1] = first[walk_vtx[walk_off[h + 1] - 1] + 1] - 1;
    }
}

}  // namespace

void phi_launch_chop_count(hipStream_t st, const int32_t *walk_vtx, int64_t n_entries, const int32_t *first, int32_t n_vtx, int32_t *cnt,
                           unsigned long long *bad_entry)
{
    if (n_entries <= 0) return;
    const unsigned nb = (unsigned)std::min<int64_t>((n_entries + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(chop_count_kernel, dim3(nb), dim3(256), 0, st, walk_vtx, n_entries, first, n_vtx, cnt, bad_entry);
}

// ent_off[0 .. n_entries]: the scanned counts; n_out = ent_off[n_entries]; out is 16-byte aligned
void phi_launch_chop_expand(hipStream_t st, const int32_t *walk_vtx, const int64_t *ent_off, int64_t n_entries, const int32_t *first,
                            int32_t *out, int64_t n_out)
{
    if (n_out <= 0) return;
    const unsigned nb = (unsigned)((n_out + CHOP_TILE - 1) / CHOP_TILE);
    hipLaunchKernelGGL(chop_expand_kernel, dim3(nb), dim3(CHOP_TPB), 0, st, walk_vtx, ent_off, n_entries, first, out, n_out);
}

void phi_launch_chop_walks(hipStream_t st, const int32_t *walk_vtx, const int64_t *ent_off, const int64_t *walk_off, int32_t n_walks,
                           const int32_t *first, int64_t *walk_off_out, int32_t *ends)
{
    hipLaunchKernelGGL(chop_walks_kernel, dim3((unsigned)(n_walks / 256 + 1)), dim3(256), 0, st, walk_vtx, ent_off, walk_off, n_walks, first,
                       walk_off_out, ends);
}
