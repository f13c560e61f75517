// chop.hip -- the walk entries of a graph whose vertices are chopped into pieces of at most N bases, made ON THE DEVICE.
//
// The reference's pipeline never hands PHI a graph as the graph builder wrote it: an external tool chops every segment to
// at most 30 bases first (data/chop_graph.sh:3 `hal2vg --chop 30`, :62-66 `gfa2gbwt -m 30`), because the model lets the path
// switch haplotypes at vertex borders only and ignores every anchor inside one vertex (ILP_index.cpp:795/:846).
// phi_set_graph_chopped (below, behind the kernels) does that step inside "set graph".  The per-vertex arrays are small and are chopped on
// the host; the walk entries multiply (a 1-kbp segment is 34 pieces at N = 30) and at chromosome scale exist only in HBM,
// so they are expanded where they lie:
//     count    pieces of every entry's vertex (first[v + 1] - first[v]); an entry outside [0, n_vtx) is reported
//     scan     64-bit exclusive scan of the counts (phi_scan of scan.hip) = where every entry's pieces go
//     expand   a workgroup owns a tile of CHOP_TILE consecutive OUTPUT entries -- one input entry may become a million
//              outputs and the next one a single one --, finds the input entries that cover the tile (one search of the
//              scanned offsets per tile, all lanes probing), stages their starts and first pieces in LDS, and every lane
//              writes four consecutive entries with one 16-byte store
//     walks    the new walk offsets and the first / last piece of every walk (what the host pass of set_graph looks at)
// The expansion is bound by HBM: 4 bytes written per output entry; per INPUT entry 8 bytes of offsets, 4 of the entry and
// one gather into first[].
#include <string.h>
#include <algorithm>
#include "phi_ctx.h"
#include "dp_steps.h"

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

// ---- host side (C ABI of include/phi_amd.h)

// chop.hip's count / 64-bit scan / tiled expand, the one entry point of everything that multiplies walk entries on the device:
// entry e of d_in (a vertex of [0, n_vtx): phi_set_graph_chopped; a unit: phi_vcf_walks) becomes the consecutive ids
// first[v] .. first[v + 1] - 1 in d_out (allocated here once the counts say how large), with the new walk offsets, the first
// and last id of every walk (what set_graph_impl's host pass looks at) and the GPU time of count + scan + expand by events
// on the context's stream.  Refusals are decided from the counts, before d_out exists.
int chop_expand_entries(phi_ctx *c, const int32_t *d_in, int64_t n_in, const int32_t *first, int32_t n_vtx, const int64_t *walk_off,
                        int32_t n_walks, int32_t max_len, DevBuf &d_out, std::vector<int64_t> &walk_off2, std::vector<int32_t> &ends,
                        int64_t *n_out_p, double *gpu_ms)
{
    DevBuf d_first, d_cnt, d_off, d_woff_in, d_woff_out, d_ends, d_bad;
    PhiDevGuard guard{{&d_first, &d_cnt, &d_off, &d_woff_in, &d_woff_out, &d_ends, &d_bad}};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int i = 0; i < 4; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
    for (int i = 0; i < 4; i++) HIPCHK(hipEventCreate(&ev[i]));
    PHICHK(upload(c, d_first, first, (size_t)n_vtx + 1));
    PHICHK(upload(c, d_woff_in, walk_off, (size_t)n_walks + 1));
    PHICHK(phi_dev_ensure(c, d_cnt, (size_t)n_in * 4));
    PHICHK(phi_dev_ensure(c, d_off, ((size_t)n_in + 1) * 8));
    PHICHK(phi_dev_ensure(c, d_bad, 8));
    PHICHK(phi_dev_ensure(c, d_woff_out, ((size_t)n_walks + 1) * 8));
    PHICHK(phi_dev_ensure(c, d_ends, (size_t)n_walks * 8));
    HIPCHK(hipMemsetAsync(d_bad.p, 0xFF, 8, c->stream));
    HIPCHK(hipEventRecord(ev[0], c->stream));
    phi_launch_chop_count(c->stream, d_in, n_in, d_first.as<int32_t>(), n_vtx, d_cnt.as<int32_t>(), d_bad.as<unsigned long long>());
    PHICHK(phi_scan(c, d_cnt.as<int32_t>(), n_in, d_off.as<int64_t>()));
    HIPCHK(hipEventRecord(ev[1], c->stream));
    unsigned long long bad = 0;
    int64_t n_out = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&n_out, d_off.as<int64_t>() + n_in, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    if (bad != ~0ull) {
        int32_t v = 0;
        HIPCHK(phi_copy_sync(c, &v, d_in + bad, 4, hipMemcpyDeviceToHost));
        const int32_t h = (int32_t)(std::upper_bound(walk_off, walk_off + n_walks + 1, (int64_t)bad) - walk_off) - 1;
        return phi_fail(c, PHI_ERR_WALK, "walk %d holds vertex %d out of range", h, v);
    }
    // (decided from the counts: nothing has been allocated for the chopped entries yet, and walks resolved on the device are as they were)
    if (n_out > PHI_MAX_ENTRIES && max_len > 0)
        return phi_fail(c, PHI_ERR_UNSUPPORTED, "chopped to %d bases the walks have %lld entries: more than 2^32 - 64", max_len, (long long)n_out);
    if (n_out > PHI_MAX_ENTRIES) return phi_fail(c, PHI_ERR_UNSUPPORTED, "the walks have %lld entries: more than 2^32 - 64", (long long)n_out);
    PHICHK(phi_dev_ensure(c, d_out, (size_t)n_out * 4));
    HIPCHK(hipEventRecord(ev[2], c->stream));
    phi_launch_chop_expand(c->stream, d_in, d_off.as<int64_t>(), n_in, d_first.as<int32_t>(), d_out.as<int32_t>(), n_out);
    phi_launch_chop_walks(c->stream, d_in, d_off.as<int64_t>(), d_woff_in.as<int64_t>(), n_walks, d_first.as<int32_t>(), d_woff_out.as<int64_t>(),
                          d_ends.as<int32_t>());
    HIPCHK(hipEventRecord(ev[3], c->stream));
    walk_off2.resize((size_t)n_walks + 1);
    ends.resize((size_t)n_walks * 2);
    HIPCHK(hipMemcpyAsync(walk_off2.data(), d_woff_out.p, walk_off2.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ends.data(), d_ends.p, ends.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    float ms_a = 0.f, ms_b = 0.f;
    HIPCHK(hipEventElapsedTime(&ms_a, ev[0], ev[1]));
    HIPCHK(hipEventElapsedTime(&ms_b, ev[2], ev[3]));
    *n_out_p = n_out;
    *gpu_ms = (double)ms_a + (double)ms_b;
    return PHI_OK;
}

extern "C" {

// data/chop_graph.sh:3,62 inside "set graph": the per-vertex arrays chopped here on the host threads, the walk entries on the
// device (the kernels above), then set_graph_impl (set_graph.hip) on the chopped graph with its walks where the expansion left them.
int phi_set_graph_chopped(phi_ctx *c, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off, const int64_t *adj_off,
                          const int32_t *adj, int32_t n_walks, const int64_t *walk_off, const int32_t *walk_vtx,
                          const int32_t *topo_rank, int32_t max_len, int64_t *walk_off_out)
{
    if (!c) return PHI_ERR_INVALID;
    const bool dev_walks = walk_vtx == nullptr;
    // (the offsets the chop itself indexes with are checked there; what else it indexes with -- topo_rank, the edge targets --
    //  below; the rest by set_graph_impl on the chopped graph)
    PHICHK(set_graph_check_args(c, n_vtx, seq_concat, seq_off, adj_off, adj, n_walks, walk_off, walk_vtx, topo_rank));
    if (max_len < 1) return phi_fail(c, PHI_ERR_INVALID, "phi_set_graph_chopped: max_len %d (a piece holds at least one base)", max_len);
    PhiStageTimer tm("set_graph_chopped");
    PHICHK(set_graph_check_offsets(c, n_vtx, seq_off, adj_off, n_walks, walk_off));
    const int64_t n_edges = adj_off[n_vtx], n_in = walk_off[n_walks];
    // ---- pieces of every vertex, first piece of every vertex
    const int64_t N = max_len;
    std::vector<int64_t> first64((size_t)n_vtx + 1, 0);
    for (int32_t v = 0; v < n_vtx; v++) {
        const int64_t L = seq_off[v + 1] - seq_off[v];
        first64[(size_t)v + 1] = first64[(size_t)v] + std::max<int64_t>(1, (L + N - 1) / N);
    }
    const int64_t nv2 = first64[(size_t)n_vtx];
    if (nv2 > INT32_MAX)
        return phi_fail(c, PHI_ERR_UNSUPPORTED, "chopped to %d bases the graph has %lld vertices: more than 2^31 - 1", max_len, (long long)nv2);
    auto &first = c->chop.first;
    first.resize((size_t)n_vtx + 1);
    for (int32_t v = 0; v <= n_vtx; v++) first[(size_t)v] = (int32_t)first64[(size_t)v];
    std::vector<int64_t>().swap(first64);
    phi_chop_info info{};
    info.n_vtx_in = n_vtx; info.n_vtx_out = nv2; info.n_entries_in = n_in; info.n_entries_out = n_in; info.max_len = max_len;
    if (nv2 == n_vtx) {
        // nothing to chop: the graph as passed in
        PHICHK(set_graph_impl(c, n_vtx, seq_concat, seq_off, adj_off, adj, n_walks, walk_off, walk_vtx, topo_rank));
        if (walk_off_out) memcpy(walk_off_out, walk_off, ((size_t)n_walks + 1) * 8);
        c->chop.info = info; c->chop.on = true;
        return PHI_OK;
    }
    // ---- the per-vertex arrays (all host threads; everything is a closed form of first[])
    std::vector<int32_t> topo_inv;
    {
        PhiHostError verr;
        if (phi_topo_from_ranks(n_vtx, topo_rank, topo_inv, verr) || phi_check_edges(n_vtx, adj_off, adj, topo_rank, nullptr, verr))
            return phi_fail(c, verr.code, "%s", verr.msg.c_str());
    }
    const int64_t n_edges2 = n_edges + (nv2 - n_vtx);
    std::vector<int64_t> seq_off2((size_t)nv2 + 1), adj_off2((size_t)nv2 + 1), rank0((size_t)n_vtx);
    std::vector<int32_t> adj2((size_t)std::max<int64_t>(n_edges2, 1)), topo2((size_t)nv2);
    {
        int64_t run = 0;                                       // first rank of every vertex: the counts summed in topological order
        for (int32_t r = 0; r < n_vtx; r++) {
            const int32_t v = topo_inv[(size_t)r];
            rank0[(size_t)v] = run;
            run += first[(size_t)v + 1] - first[(size_t)v];
        }
    }
    phi_parallel_chunks(n_vtx, 1 << 14, [&](int64_t lo, int64_t hi, int) {
        for (int64_t v = lo; v < hi; v++) {
            const int64_t p0 = first[(size_t)v], np = first[(size_t)v + 1] - p0;
            const int64_t a0 = adj_off[v] + (p0 - v);          // (every piece but a vertex's last has one edge more than the graph had)
            for (int64_t j = 0; j < np; j++) {
                seq_off2[(size_t)(p0 + j)] = seq_off[v] + j * N;
                adj_off2[(size_t)(p0 + j)] = a0 + j;
                topo2[(size_t)(p0 + j)] = (int32_t)(rank0[(size_t)v] + j);
                if (j + 1 < np) adj2[(size_t)(a0 + j)] = (int32_t)(p0 + j + 1);
            }
            int64_t a = a0 + np - 1;
            for (int64_t x = adj_off[v]; x < adj_off[v + 1]; x++) adj2[(size_t)a++] = first[(size_t)adj[x]];
        }
    });
    seq_off2[(size_t)nv2] = seq_off[n_vtx];
    adj_off2[(size_t)nv2] = n_edges2;
    std::vector<int32_t>().swap(topo_inv);
    std::vector<int64_t>().swap(rank0);
    tm.lap("chop: per-vertex arrays");
    // ---- the walk entries, on the device
    DevBuf d_in_own, d_out;
    PhiDevGuard guard{{&d_in_own, &d_out}};
    if (!dev_walks) PHICHK(upload(c, d_in_own, walk_vtx, (size_t)n_in));
    const int32_t *d_in = dev_walks ? c->d_walk_vtx.as<int32_t>() : d_in_own.as<int32_t>();
    std::vector<int64_t> walk_off2;
    std::vector<int32_t> ends;
    int64_t n_out = 0;
    PHICHK(chop_expand_entries(c, d_in, n_in, first.data(), n_vtx, walk_off, n_walks, max_len, d_out, walk_off2, ends, &n_out, &info.expand_gpu_ms));
    info.n_entries_out = n_out;
    tm.lap("chop: walk entries on the device");
    // the chopped entries become the context's walks, as if phi_walk_text_resolve had left them
    std::swap(c->d_walk_vtx, d_out);                           // (the guard lets the unchopped ones go)
    c->wtext.ends.swap(ends);
    c->walks_on_device = true;
    c->walks_on_device_n = n_out;
    for (DevBuf *x : guard.b) phi_dev_free(*x);
    const int rc = set_graph_impl(c, (int32_t)nv2, seq_concat, seq_off2.data(), adj_off2.data(), adj2.data(), n_walks, walk_off2.data(), nullptr, topo2.data());
    c->walks_on_device = false;
    if (rc) return rc;
    if (walk_off_out) memcpy(walk_off_out, walk_off2.data(), walk_off2.size() * 8);
    c->chop.info = info; c->chop.on = true;
    return PHI_OK;
}

int phi_chop_origin(phi_ctx *c, const int32_t *vtx, int64_t n, int32_t *orig_vtx, int32_t *orig_off)
{
    if (!c || n < 0 || (n > 0 && !vtx)) return PHI_ERR_INVALID;
    PHICHK(phi_refuse_scout(c, "phi_chop_origin"));
    if (!c->have_graph || !c->chop.on) return phi_fail(c, PHI_ERR_STATE, "phi_chop_origin: the graph was not set with phi_set_graph_chopped");
    const auto &first = c->chop.first;
    for (int64_t i = 0; i < n; i++) {
        const int32_t id = vtx[i];                            // (read first: the outputs may be the input array)
        if (id < 0 || id >= first.back()) return phi_fail(c, PHI_ERR_INVALID, "phi_chop_origin: vertex %d is not in the chopped graph", id);
        const int32_t v = (int32_t)(std::upper_bound(first.begin(), first.end(), id) - first.begin()) - 1;
        if (orig_vtx) orig_vtx[i] = v;
        if (orig_off) orig_off[i] = (id - first[(size_t)v]) * c->chop.info.max_len;
    }
    return PHI_OK;
}

int phi_chop_stats(phi_ctx *c, phi_chop_info *out)
{
    if (!c || !out) return PHI_ERR_INVALID;
    PHICHK(phi_refuse_scout(c, "phi_chop_stats"));
    if (!c->have_graph || !c->chop.on) return phi_fail(c, PHI_ERR_STATE, "phi_chop_stats: the graph was not set with phi_set_graph_chopped");
    *out = c->chop.info;
    return PHI_OK;
}

}  // extern "C"
