// panel.hip -- "set graph" against a PANEL of the graph's haplotypes: the subgraph induced by the kept walks, its walk entries
// made ON THE DEVICE.
//
// The reference's progressive-imputation experiment builds one graph from the full VCF (data/chop_graph.sh:46-50), removes
// samples from the haplotype index (:51-61 `vg gbwt ... -R SAMPLE`, the lists drawn nested by data/get_ids.py and
// data/get_ids_2.py), writes one GFA per panel (:62-66) and runs PHI once per panel (data/run_batch_9.py to run_batch_13.py).
// phi_set_graph_panel (below, behind the kernels) does the reduction inside "set graph".  The per-vertex arrays are small and
// are reduced on the host; the walk entries are the bulk and at chromosome scale exist only in HBM, so they are renamed where
// they lie:
//     mark     a workgroup owns a tile of PANEL_TILE consecutive KEPT entries (output positions), finds the kept walks that
//              cover the tile (one search of the output offsets per tile, all lanes probing, as chop_expand_kernel does),
//              stages their starts in LDS, and for every entry checks the vertex' range, flags the vertex and flags the
//              graph edge(s) to the next entry of the same walk (a short scan of the vertex' edge list).  The flags are
//              bytes in buffers zeroed for the call; lanes that meet on a byte store the same value: no atomics
//     scan     the vertex flags compacted (phi_compact of scan.hip: flag count, 64-bit scan, ordered write) into the list of kept
//              vertices, which a scatter turns into new_id[]
//     remap    the same tiling; every lane writes four consecutive entries new_id[in[src]] with one 16-byte store
//     ends     the first and the last vertex of every kept walk (what the host pass of set_graph looks at)
// No workgroup waits for another and nothing spins on memory.  Both passes are bound by HBM: 4 bytes read per kept entry and
// a gather (mark: the edge list of the vertex, remap: new_id[]); mark adds a scattered byte per vertex and edge, remap 4 bytes
// written per entry.
#include <string.h>
#include <algorithm>
#include <chrono>
#include "phi_ctx.h"

#define PANEL_TILE 4096
#define PANEL_TPB 256

namespace {

// The kept walks that cover output entries [t0, t1): walk lo + i (in kept order) for i < n_cov, its first output entry
// relative to the tile in s_start[i] (negative for a walk that began before the tile) and, in s_delta[i], how far its
// input entries lie behind its output entries (input index = output index + delta; both below 2^32, delta >= 0).
// Every kept walk holds at least one entry: at most PANEL_TILE of them start inside a tile.  Returns n_cov; *end_last =
// the output entry behind the last covering walk.
__device__ __forceinline__ int panel_cover(const int64_t *__restrict__ kout, const int64_t *__restrict__ kin, int32_t n_kept, int64_t t0,
                                           int64_t t1, int32_t *s_start, uint32_t *s_delta, int64_t *end_last)
{
    const int tid = threadIdx.x;
    // the last kept walk that starts at or before t0: 256 probes a round over [lo, hi), kout[lo] <= t0 throughout
    int64_t lo = 0, hi = n_kept;
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + PANEL_TPB - 1) / PANEL_TPB;
        const int64_t idx = lo + tid * step;
        const int n_le = __syncthreads_count(idx < hi && kout[idx] <= t0);     // (kout ascends: the lanes that say yes are the first n_le)
        lo += (n_le - 1) * step;
        hi = min(hi, lo + step);
    }
    int n_cov = 0;
    for (int b = 0; b < PANEL_TILE; b += PANEL_TPB) {
        const int64_t k = lo + b + tid;
        bool ok = false;
        if (k < n_kept) {
            const int64_t o = kout[k];
            if (o < t1) {
                ok = true;
                s_start[b + tid] = (int32_t)(o - t0);
                s_delta[b + tid] = (uint32_t)(kin[k] - o);
            }
        }
        const int n_ok = __syncthreads_count(ok);
        n_cov += n_ok;
        if (n_ok < PANEL_TPB) break;
    }
    *end_last = kout[lo + n_cov];
    return n_cov;
}

// the covering walk of output q0 of the tile (the last start at or before it)
__device__ __forceinline__ int panel_find(const int32_t *s_start, int n_cov, int q0)
{
    const int p2 = n_cov > 1 ? 1 << (31 - __clz(n_cov - 1)) : 0;
    int i = 0;
    for (int s = p2; s; s >>= 1) {
        const int m = i + s;
        if (m < n_cov && s_start[m] <= q0) i = m;
    }
    return i;
}

__global__ void __launch_bounds__(PANEL_TPB) panel_mark_kernel(const int32_t *__restrict__ in, const int64_t *__restrict__ kout,
                                                               const int64_t *__restrict__ kin, int32_t n_kept, int64_t n_out,
                                                               const int64_t *__restrict__ adj_off, const int32_t *__restrict__ adj, int32_t n_vtx,
                                                               uint8_t *__restrict__ used_vtx, uint8_t *__restrict__ used_edge,
                                                               unsigned long long *__restrict__ bad)
{
    __shared__ int32_t s_start[PANEL_TILE];
    __shared__ uint32_t s_delta[PANEL_TILE];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * PANEL_TILE;
    const int64_t t1 = min(n_out, t0 + PANEL_TILE);
    if (t0 >= n_out) return;
    int64_t end_last;
    const int n_cov = panel_cover(kout, kin, n_kept, t0, t1, s_start, s_delta, &end_last);
    const int n_here = (int)(t1 - t0);
    for (int q0 = tid * 4; q0 < n_here; q0 += PANEL_TPB * 4) {
        int i = panel_find(s_start, n_cov, q0);
        for (int j = 0; j < 4 && q0 + j < n_here; j++) {
            const int q = q0 + j;
            if (j && i + 1 < n_cov && s_start[i + 1] <= q) i++;                 // (starts ascend strictly: one step at most)
            const int64_t src = t0 + q + (int64_t)s_delta[i];
            const int64_t walk_end = i + 1 < n_cov ? t0 + s_start[i + 1] : end_last;
            const int32_t u = in[src];
            // the range check comes before anything is indexed with the vertex; the smallest such entry is the one the host names
            if ((uint32_t)u >= (uint32_t)n_vtx) { atomicMin(bad, (unsigned long long)src); continue; }
            used_vtx[u] = 1;
            if (t0 + q + 1 < walk_end) {
                const int32_t v = in[src + 1];
                // (a step without a graph edge flags nothing: set_graph reports it on the panel graph)
                for (int64_t x = adj_off[u], xe = adj_off[u + 1]; x < xe; x++)
                    if (adj[x] == v) used_edge[x] = 1;
            }
        }
    }
}

__global__ void __launch_bounds__(256) panel_new_id_kernel(const int32_t *__restrict__ origin, int32_t n_kept_vtx, int32_t *__restrict__ new_id)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_kept_vtx) new_id[origin[j]] = j;
}

__global__ void __launch_bounds__(PANEL_TPB) panel_remap_kernel(const int32_t *__restrict__ in, const int64_t *__restrict__ kout,
                                                                const int64_t *__restrict__ kin, int32_t n_kept, int64_t n_out,
                                                                const int32_t *__restrict__ new_id, int32_t *__restrict__ out)
{
    __shared__ int32_t s_start[PANEL_TILE];
    __shared__ uint32_t s_delta[PANEL_TILE];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * PANEL_TILE;
    const int64_t t1 = min(n_out, t0 + PANEL_TILE);
    if (t0 >= n_out) return;
    int64_t end_last;
    const int n_cov = panel_cover(kout, kin, n_kept, t0, t1, s_start, s_delta, &end_last);
    const int n_here = (int)(t1 - t0);
    for (int q0 = tid * 4; q0 < n_here; q0 += PANEL_TPB * 4) {
        int i = panel_find(s_start, n_cov, q0);
        int32_t val[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int q = q0 + j;
            if (q < n_here) {
                if (j && i + 1 < n_cov && s_start[i + 1] <= q) i++;
                val[j] = new_id[in[t0 + q + (int64_t)s_delta[i]]];              // (in range: the mark pass has checked every kept entry)
            }
        }
        int32_t *dst = out + t0 + q0;
        if (q0 + 4 <= n_here) {
            *reinterpret_cast<int4 *>(dst) = make_int4(val[0], val[1], val[2], val[3]);
        } else {
            for (int j = 0; q0 + j < n_here; j++) dst[j] = val[j];
        }
    }
}

__global__ void __launch_bounds__(256) panel_ends_kernel(const int32_t *__restrict__ in, const int64_t *__restrict__ kout,
                                                         const int64_t *__restrict__ kin, int32_t n_kept, const int32_t *__restrict__ new_id,
                                                         int32_t *__restrict__ ends)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_kept) return;
    const int64_t len = kout[k + 1] - kout[k];
    ends[2 * k] = new_id[in[kin[k]]];
    ends[2 * k + 1] = new_id[in[kin[k] + len - 1]];
}

struct PanelEvents {
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~PanelEvents() { for (int i = 0; i < 5; i++) if (e[i]) (void)hipEventDestroy(e[i]); }
};

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" {

// data/chop_graph.sh:46-66 inside "set graph": the kept walks' entries marked and renamed on the device (the kernels above),
// the per-vertex arrays reduced here on the host threads, the ranks by Kahn with a FIFO queue as the host reader sorts
// (ILP_index.cpp:115-154), then set_graph_impl or phi_set_graph_chopped on the panel graph with its walks where remap left them.
int phi_set_graph_panel(phi_ctx *c, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off, const int64_t *adj_off,
                        const int32_t *adj, int32_t n_walks, const int64_t *walk_off, const int32_t *walk_vtx, const uint8_t *keep,
                        int32_t max_len, uint32_t flags, int64_t *walk_off_out)
{
    if (!c) return PHI_ERR_INVALID;
    if (n_vtx <= 0 || n_walks <= 0 || !seq_concat || !seq_off || !adj_off || !walk_off || !keep)
        return phi_fail(c, PHI_ERR_INVALID, "phi_set_graph_panel: null pointer or empty graph");
    if (adj_off[n_vtx] > 0 && !adj) return phi_fail(c, PHI_ERR_INVALID, "phi_set_graph_panel: adj is null");
    if (flags & ~(uint32_t)(PHI_PANEL_RETAIN | PHI_PANEL_KEEP_READS)) return phi_fail(c, PHI_ERR_INVALID, "phi_set_graph_panel: unknown flags %u", flags);
    HIPCHK(hipSetDevice(c->device));
    if (c->ipc) return phi_fail(c, PHI_ERR_STATE, "phi_set_graph on a context in a group of processes: phi_ipc_destroy first (the peers have this context's hit vectors mapped)");
    PhiStageTimer tm("set_graph_panel");
    PHICHK(set_graph_check_offsets(c, n_vtx, seq_off, adj_off, n_walks, walk_off));
    const int64_t n_edges = adj_off[n_vtx], n_in = walk_off[n_walks];
    auto &P = c->panel;
    // ---- where the full entries are: the caller's, freshly resolved on this context, or retained by an earlier call
    enum { FROM_HOST, FROM_RESOLVED, FROM_RETAINED, FROM_SCOUT } from = FROM_HOST;
    if (!walk_vtx) {
        const bool same_off = P.full_off.size() == (size_t)n_walks + 1 && std::equal(P.full_off.begin(), P.full_off.end(), walk_off);
        if (c->scout.on && same_off) from = FROM_SCOUT;           // (phi_scout_graph: the full entries are the scout's walks)
        else if (c->walks_on_device && c->walks_on_device_n == n_in && (int32_t)(c->wtext.ends.size() / 2) == n_walks) from = FROM_RESOLVED;
        else if (P.d_full.p && P.full_off.size() == (size_t)n_walks + 1 && std::equal(P.full_off.begin(), P.full_off.end(), walk_off)) from = FROM_RETAINED;
        else return phi_fail(c, PHI_ERR_STATE, "phi_set_graph_panel without walk_vtx: these walks are neither freshly resolved on this context nor retained by an earlier panel");
    }
    // ---- refusals that the counts decide: before anything is allocated, the context as it was
    std::vector<int32_t> kept;
    for (int32_t h = 0; h < n_walks; h++) if (keep[h]) kept.push_back(h);
    const int32_t n_kept = (int32_t)kept.size();
    if (n_kept == 0) return phi_fail(c, PHI_ERR_INVALID, "phi_set_graph_panel: no walk is kept");
    if (n_kept > PHI_DP_MAX_WALKS) return phi_fail(c, PHI_ERR_UNSUPPORTED, "more than %d walks", PHI_DP_MAX_WALKS);
    c->have_graph = false;
    c->chop.on = false;
    P.on = false;
    phi_scout_end(c);                                          // (the choice has been made: the score matrix goes before the panel's index is built)
    c->solved = false;
    c->calls.have = false;
    // PHI_PANEL_KEEP_READS: a finished store steps aside while the graph is set anew (every stage below drops what it finds) and
    // comes back when the panel stands; on failure it goes, as the graph it was collected under has
    struct KeptReads {
        phi_ctx *c;
        phi_ctx::PhiLadder store;
        ~KeptReads() { for (DevBuf *b : {&store.d_bases, &store.d_off}) phi_dev_free(*b); }
    } kept_reads{c, {}};
    if (flags & PHI_PANEL_KEEP_READS) phi_ladder_detach(c, kept_reads.store);
    phi_ladder_drop(c);
    if (from == FROM_SCOUT) {                                  // the scout's entries count as retained, and stay so
        phi_dev_free(P.d_full);
        std::swap(P.d_full, c->d_walk_vtx);
        from = FROM_RETAINED;
        flags |= PHI_PANEL_RETAIN;
    }
    std::vector<int64_t> kin((size_t)n_kept), kout((size_t)n_kept + 1, 0);
    for (int32_t k = 0; k < n_kept; k++) {
        kin[(size_t)k] = walk_off[kept[(size_t)k]];
        kout[(size_t)k + 1] = kout[(size_t)k] + (walk_off[kept[(size_t)k] + 1] - walk_off[kept[(size_t)k]]);
    }
    const int64_t n_out = kout[(size_t)n_kept];
    phi_panel_info info{};
    info.n_walks_in = n_walks; info.n_walks_out = n_kept; info.n_vtx_in = n_vtx; info.n_edges_in = n_edges;
    info.n_entries_in = n_in; info.n_entries_out = n_out;

    // ---- mark, on the device
    DevBuf d_in_own, d_out, d_kin, d_kout, d_adj_off, d_adj, d_used_vtx, d_used_edge, d_bad, d_origin, d_new_id, d_ends;
    PhiDevGuard guard{{&d_in_own, &d_out, &d_kin, &d_kout, &d_adj_off, &d_adj, &d_used_vtx, &d_used_edge, &d_bad, &d_origin, &d_new_id, &d_ends}};
    PanelEvents ev;
    for (int i = 0; i < 5; i++) HIPCHK(hipEventCreate(&ev.e[i]));
    if (from == FROM_HOST) PHICHK(upload(c, d_in_own, walk_vtx, (size_t)n_in));
    const int32_t *d_in = from == FROM_HOST ? d_in_own.as<int32_t>() : from == FROM_RESOLVED ? c->d_walk_vtx.as<int32_t>() : P.d_full.as<int32_t>();
    PHICHK(upload(c, d_kin, kin.data(), kin.size()));
    PHICHK(upload(c, d_kout, kout.data(), kout.size()));
    PHICHK(upload(c, d_adj_off, adj_off, (size_t)n_vtx + 1));
    if (n_edges) PHICHK(upload(c, d_adj, adj, (size_t)n_edges));
    else PHICHK(phi_dev_ensure(c, d_adj, 4));
    const size_t ne1 = (size_t)std::max<int64_t>(n_edges, 1);
    PHICHK(phi_dev_ensure(c, d_used_vtx, (size_t)n_vtx));
    PHICHK(phi_dev_ensure(c, d_used_edge, ne1));
    PHICHK(phi_dev_ensure(c, d_bad, 8));
    PHICHK(phi_dev_ensure(c, d_new_id, (size_t)n_vtx * 4));
    PHICHK(phi_dev_ensure(c, d_ends, (size_t)n_kept * 8));
    HIPCHK(hipMemsetAsync(d_used_vtx.p, 0, (size_t)n_vtx, c->stream));
    HIPCHK(hipMemsetAsync(d_used_edge.p, 0, ne1, c->stream));
    HIPCHK(hipMemsetAsync(d_bad.p, 0xFF, 8, c->stream));
    const unsigned n_tiles = (unsigned)((n_out + PANEL_TILE - 1) / PANEL_TILE);
    HIPCHK(hipEventRecord(ev.e[0], c->stream));
    hipLaunchKernelGGL(panel_mark_kernel, dim3(n_tiles), dim3(PANEL_TPB), 0, c->stream, d_in, d_kout.as<int64_t>(), d_kin.as<int64_t>(), n_kept, n_out,
                       d_adj_off.as<int64_t>(), d_adj.as<int32_t>(), n_vtx, d_used_vtx.as<uint8_t>(), d_used_edge.as<uint8_t>(),
                       d_bad.as<unsigned long long>());
    HIPCHK(hipEventRecord(ev.e[1], c->stream));
    std::vector<uint8_t> used_vtx((size_t)n_vtx), used_edge(ne1, 0);
    unsigned long long bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(used_vtx.data(), d_used_vtx.p, (size_t)n_vtx, hipMemcpyDeviceToHost, c->stream));
    if (n_edges) HIPCHK(hipMemcpyAsync(used_edge.data(), d_used_edge.p, (size_t)n_edges, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    if (bad != ~0ull) {
        int32_t v = 0;
        HIPCHK(phi_copy_sync(c, &v, d_in + bad, 4, hipMemcpyDeviceToHost));
        const int32_t h = (int32_t)(std::upper_bound(walk_off, walk_off + n_walks + 1, (int64_t)bad) - walk_off) - 1;
        return phi_fail(c, PHI_ERR_WALK, "walk %d holds vertex %d out of range", h, v);
    }
    // ---- scan: the kept vertices in their old order, new_id = the number of kept vertices before
    HIPCHK(hipEventRecord(ev.e[2], c->stream));
    int64_t nv2_64 = 0;
    PHICHK(phi_compact(c, d_used_vtx.as<uint8_t>(), n_vtx, d_origin, &nv2_64));
    const int32_t nv2 = (int32_t)nv2_64;
    hipLaunchKernelGGL(panel_new_id_kernel, dim3((unsigned)(nv2 / 256 + 1)), dim3(256), 0, c->stream, d_origin.as<int32_t>(), nv2, d_new_id.as<int32_t>());
    HIPCHK(hipEventRecord(ev.e[3], c->stream));
    // ---- remap (runs while the host reduces the per-vertex arrays below)
    PHICHK(phi_dev_ensure(c, d_out, (size_t)std::max<int64_t>(n_out, 4) * 4));
    hipLaunchKernelGGL(panel_remap_kernel, dim3(n_tiles), dim3(PANEL_TPB), 0, c->stream, d_in, d_kout.as<int64_t>(), d_kin.as<int64_t>(), n_kept, n_out,
                       d_new_id.as<int32_t>(), d_out.as<int32_t>());
    hipLaunchKernelGGL(panel_ends_kernel, dim3((unsigned)(n_kept / 256 + 1)), dim3(256), 0, c->stream, d_in, d_kout.as<int64_t>(), d_kin.as<int64_t>(), n_kept,
                       d_new_id.as<int32_t>(), d_ends.as<int32_t>());
    HIPCHK(hipEventRecord(ev.e[4], c->stream));
    std::vector<int32_t> ends((size_t)n_kept * 2);
    HIPCHK(hipMemcpyAsync(ends.data(), d_ends.p, ends.size() * 4, hipMemcpyDeviceToHost, c->stream));
    tm.lap("panel: mark + scan, remap queued");

    // ---- the per-vertex arrays of the panel graph (all host threads)
    const auto t_red = std::chrono::steady_clock::now();
    std::vector<int32_t> origin, new_id((size_t)n_vtx, -1);
    origin.reserve((size_t)nv2);
    for (int32_t v = 0; v < n_vtx; v++)
        if (used_vtx[(size_t)v]) { new_id[(size_t)v] = (int32_t)origin.size(); origin.push_back(v); }
    if ((int32_t)origin.size() != nv2) {
        (void)hipStreamSynchronize(c->stream);
        return phi_fail(c, PHI_ERR_DEVICE, "panel: the device counts %d kept vertices, the host %lld (internal error)", nv2, (long long)origin.size());
    }
    std::vector<int64_t> seq_off2((size_t)nv2 + 1, 0), adj_off2((size_t)nv2 + 1, 0);
    phi_parallel_chunks(nv2, 1 << 14, [&](int64_t lo, int64_t hi, int) {
        for (int64_t j = lo; j < hi; j++) {
            const int32_t v = origin[(size_t)j];
            int64_t d = 0;
            for (int64_t x = adj_off[v]; x < adj_off[v + 1]; x++) d += used_edge[(size_t)x];
            adj_off2[(size_t)j + 1] = d;
            seq_off2[(size_t)j + 1] = seq_off[v + 1] - seq_off[v];
        }
    });
    for (int32_t j = 0; j < nv2; j++) {
        adj_off2[(size_t)j + 1] += adj_off2[(size_t)j];
        seq_off2[(size_t)j + 1] += seq_off2[(size_t)j];
    }
    const int64_t n_edges2 = adj_off2[(size_t)nv2];
    std::vector<char> seq2((size_t)std::max<int64_t>(seq_off2[(size_t)nv2], 1));
    std::vector<int32_t> adj2((size_t)std::max<int64_t>(n_edges2, 1));
    phi_parallel_chunks(nv2, 1 << 14, [&](int64_t lo, int64_t hi, int) {
        for (int64_t j = lo; j < hi; j++) {
            const int32_t v = origin[(size_t)j];
            if (seq_off[v + 1] > seq_off[v]) memcpy(seq2.data() + seq_off2[(size_t)j], seq_concat + seq_off[v], (size_t)(seq_off[v + 1] - seq_off[v]));
            int64_t a = adj_off2[(size_t)j];
            for (int64_t x = adj_off[v]; x < adj_off[v + 1]; x++)
                if (used_edge[(size_t)x]) adj2[(size_t)a++] = new_id[(size_t)adj[x]];   // (a flagged edge ends at an entry the mark pass flagged)
        }
    });
    info.n_vtx_out = nv2; info.n_edges_out = n_edges2;
    info.reduce_host_s = seconds_since(t_red);
    // ---- the ranks the host reader gives the panel graph: Kahn's algorithm, FIFO, sources in id order (ILP_index.cpp:115-154)
    const auto t_kahn = std::chrono::steady_clock::now();
    std::vector<int32_t> topo2((size_t)nv2, 0);
    {
        std::vector<int32_t> indeg((size_t)nv2, 0), q((size_t)nv2);
        for (int64_t x = 0; x < n_edges2; x++) indeg[(size_t)adj2[(size_t)x]]++;
        int32_t head = 0, tail = 0;
        for (int32_t i = 0; i < nv2; i++) if (indeg[(size_t)i] == 0) q[(size_t)tail++] = i;
        while (head < tail) {
            const int32_t u = q[(size_t)head];
            topo2[(size_t)u] = head++;
            for (int64_t x = adj_off2[(size_t)u]; x < adj_off2[(size_t)u + 1]; x++)
                if (--indeg[(size_t)adj2[(size_t)x]] == 0) q[(size_t)tail++] = adj2[(size_t)x];
        }
        if (head != nv2) {
            (void)hipStreamSynchronize(c->stream);
            return phi_fail(c, PHI_ERR_INVALID, "graph is not acyclic: %d of %d vertices sorted", head, nv2);
        }
    }
    info.kahn_host_s = seconds_since(t_kahn);
    tm.lap("panel: per-vertex arrays + Kahn");
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1])); info.mark_gpu_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[2], ev.e[3])); info.scan_gpu_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[3], ev.e[4])); info.remap_gpu_ms = ms;
    tm.lap("panel: wait for remap");

    // ---- the panel's entries become the context's walks, as if phi_walk_text_resolve had left them; the full ones are
    //      retained, or go
    if (flags & PHI_PANEL_RETAIN) {
        if (from == FROM_HOST) { phi_dev_free(P.d_full); std::swap(P.d_full, d_in_own); }
        else if (from == FROM_RESOLVED) { phi_dev_free(P.d_full); std::swap(P.d_full, c->d_walk_vtx); }
        P.full_off.assign(walk_off, walk_off + n_walks + 1);
    } else if (from == FROM_RETAINED) {
        phi_dev_free(P.d_full);
        P.full_off.clear();
    }
    std::swap(c->d_walk_vtx, d_out);                           // (the guard lets what the context held go)
    c->wtext.ends.swap(ends);
    c->walks_on_device = true;
    c->walks_on_device_n = n_out;
    for (DevBuf *x : guard.b) phi_dev_free(*x);
    std::vector<int64_t> woff2((size_t)n_kept + 1);
    int rc;
    if (max_len > 0) {
        rc = phi_set_graph_chopped(c, nv2, seq2.data(), seq_off2.data(), adj_off2.data(), adj2.data(), n_kept, kout.data(), nullptr, topo2.data(),
                                   max_len, woff2.data());
    } else {
        rc = set_graph_impl(c, nv2, seq2.data(), seq_off2.data(), adj_off2.data(), adj2.data(), n_kept, kout.data(), nullptr, topo2.data());
        woff2 = kout;
    }
    c->walks_on_device = false;
    if (rc) return rc;
    if (walk_off_out) memcpy(walk_off_out, woff2.data(), woff2.size() * 8);
    P.origin.swap(origin);
    P.kept.swap(kept);
    P.info = info;
    P.on = true;
    phi_ladder_attach(c, kept_reads.store);
    return PHI_OK;
}

int phi_panel_origin(phi_ctx *c, const int32_t *vtx, int64_t n, int32_t *orig_vtx)
{
    if (!c || n < 0 || (n > 0 && (!vtx || !orig_vtx))) return PHI_ERR_INVALID;
    PHICHK(phi_refuse_scout(c, "phi_panel_origin"));
    if (!c->have_graph || !c->panel.on) return phi_fail(c, PHI_ERR_STATE, "phi_panel_origin: the graph was not set with phi_set_graph_panel");
    const auto &origin = c->panel.origin;
    for (int64_t i = 0; i < n; i++) {
        const int32_t id = vtx[i];                            // (read first: the output may be the input array)
        if (id < 0 || (size_t)id >= origin.size()) return phi_fail(c, PHI_ERR_INVALID, "phi_panel_origin: vertex %d is not in the panel graph", id);
        orig_vtx[i] = origin[(size_t)id];
    }
    return PHI_OK;
}

int phi_panel_walks(phi_ctx *c, int32_t *orig_walk, int32_t cap, int32_t *n_kept)
{
    if (!c || !n_kept) return PHI_ERR_INVALID;
    PHICHK(phi_refuse_scout(c, "phi_panel_walks"));
    if (!c->have_graph || !c->panel.on) return phi_fail(c, PHI_ERR_STATE, "phi_panel_walks: the graph was not set with phi_set_graph_panel");
    const auto &kept = c->panel.kept;
    *n_kept = (int32_t)kept.size();
    if (orig_walk && cap >= *n_kept) memcpy(orig_walk, kept.data(), kept.size() * 4);
    return PHI_OK;
}

int phi_panel_stats(phi_ctx *c, phi_panel_info *out)
{
    if (!c || !out) return PHI_ERR_INVALID;
    PHICHK(phi_refuse_scout(c, "phi_panel_stats"));
    if (!c->have_graph || !c->panel.on) return phi_fail(c, PHI_ERR_STATE, "phi_panel_stats: the graph was not set with phi_set_graph_panel");
    *out = c->panel.info;
    return PHI_OK;
}

int phi_panel_release(phi_ctx *c)
{
    if (!c) return PHI_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    phi_dev_free(c->panel.d_full);
    c->panel.full_off.clear();
    return PHI_OK;
}

}  // extern "C"
