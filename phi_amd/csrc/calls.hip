// calls.hip -- the inferred path (or any walk) written as VARIANT CALLS against a reference walk of the set graph, ON THE DEVICE.
//
// The reference has no counterpart: its one product is a FASTA (ILP_index.cpp:1577-1581), and its own comparison with a
// genotyper goes the other way, PanGenie's VCF turned into a FASTA with `bcftools consensus` (data/run_PG.py:54-60).  The
// calls below make the result comparable with a genotyper's or a truth VCF without an alignment.  THE RULE IS THIS PROJECT'S
// OWN (include/phi_amd.h states it): it is not `vg deconstruct`'s and has not been compared with it or with `bcftools`.
//
// Everything the calls are made from lies in HBM already -- the walk entries (d_walk_vtx: at panel scale they exist nowhere
// else), the vertex lengths (d_vlen), the sequences (d_seq, d_seq_off), and the path as a handful of stretches of those
// entries (phi_solve.hip keeps them) -- so the query is compared with the reference walk where both lie:
//     table    pos_of[v] = index of vertex v on the reference walk, -1 elsewhere: a fill, then a scatter from the walk's
//              entries, which also gathers the entries' lengths
//     query    a walk: its entries where they lie.  The path: its stretches expanded from d_walk_vtx
//     mark     per query entry its length and shared = pos_of[vertex] >= 0
//     scans    64-bit exclusive scans of both length arrays (phi_scan): base offsets along the reference walk and the query
//     shared   phi_compact of the flags: the shared query indices, ascending by construction
//     pairs    per consecutive shared pair the order check of the rule and call / no call
//     calls    phi_compact of those flags; per call POS, the anchor, the padded lengths of REF and ALT, and where on its
//              walk each allele's bytes start (first base, first and last vertex index); two scans of the lengths
//     fill     REF from the reference walk, ALT from the query: one launch each.  The work is divided over the OUTPUT BYTES
//              (an allele of 52 kb stands beside thousands of one-base ones at MHC scale): every lane owns four consecutive
//              bytes and stores them as one word, a wave 256 consecutive bytes; a lane finds its call by a search of the
//              allele offsets and its source vertex by a search of the base offsets between the call's two vertex indices
// The base offsets of both walks, the anchors and the allele sources of the calls stay on the device behind the call, and the
// query as stretches of walk entries on the host: phi_calls_support (calls_support.hip) counts every call's read support from them.
// Every output has a fixed place: no atomics but the error words, the same bytes from run to run, nothing read before it
// is written.  Bound (from the code): the 4-byte gathers into pos_of[] and d_vlen[] per entry and
// the per-vertex gathers into d_seq -- latency, not HBM bandwidth.
#include <string.h>
#include <algorithm>
#include "phi_ctx.h"

#define CALLS_TPB 256
#define CALLS_LANE_BYTES 4                              // output bytes per lane of the fill: one 32-bit store
#define CALLS_FILL_TILE (CALLS_TPB * CALLS_LANE_BYTES)  // output bytes per workgroup

namespace {

// pos_of[] is filled with -1 before; the reference walk's entries scatter their index and gather their length
__global__ void __launch_bounds__(CALLS_TPB) calls_table_kernel(const int32_t *__restrict__ ref, int32_t n_ref, const int32_t *__restrict__ vlen,
                                                                int32_t n_vtx, int32_t *__restrict__ pos_of, int32_t *__restrict__ ref_len)
{
    const int64_t p = (int64_t)blockIdx.x * CALLS_TPB + threadIdx.x;
    if (p >= n_ref) return;
    const int32_t v = ref[p];
    int32_t len = 0;
    if ((uint32_t)v < (uint32_t)n_vtx) {                   // (set_graph has checked every entry: nothing is indexed out of range even so)
        pos_of[v] = (int32_t)p;
        len = vlen[v];
    }
    ref_len[p] = len;
}

// the path's stretches (walk entries src[s] .. of out[s + 1] - out[s] entries each) expanded to the query's vertices
__global__ void __launch_bounds__(CALLS_TPB) calls_expand_kernel(const int32_t *__restrict__ walk_vtx, const int64_t *__restrict__ seg_out,
                                                                 const int64_t *__restrict__ seg_src, int32_t n_seg, int32_t n_query,
                                                                 int32_t *__restrict__ query)
{
    const int64_t i = (int64_t)blockIdx.x * CALLS_TPB + threadIdx.x;
    if (i >= n_query) return;
    int lo = 0, hi = n_seg;                                // the last stretch that starts at or before i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_out[mid] <= i) lo = mid; else hi = mid;
    }
    query[i] = walk_vtx[seg_src[lo] + (i - seg_out[lo])];
}

__global__ void __launch_bounds__(CALLS_TPB) calls_mark_kernel(const int32_t *__restrict__ query, int32_t n_query, const int32_t *__restrict__ vlen,
                                                               const int32_t *__restrict__ pos_of, int32_t n_vtx, int32_t *__restrict__ q_len,
                                                               uint8_t *__restrict__ shared)
{
    const int64_t i = (int64_t)blockIdx.x * CALLS_TPB + threadIdx.x;
    if (i >= n_query) return;
    const int32_t v = query[i];
    const bool ok = (uint32_t)v < (uint32_t)n_vtx;
    q_len[i] = ok ? vlen[v] : 0;
    shared[i] = ok && pos_of[v] >= 0;
}

// consecutive shared vertices a = query[sh[j]], b = query[sh[j + 1]]: the reference indices must ascend (err[0] = the first
// pair where they do not); a call unless b follows a directly on both
__global__ void __launch_bounds__(CALLS_TPB) calls_pair_kernel(const int32_t *__restrict__ query, const int32_t *__restrict__ sh, int32_t n_pairs,
                                                               const int32_t *__restrict__ pos_of, uint8_t *__restrict__ is_call,
                                                               unsigned long long *__restrict__ err)
{
    const int64_t j = (int64_t)blockIdx.x * CALLS_TPB + threadIdx.x;
    if (j >= n_pairs) return;
    const int32_t i = sh[j], i2 = sh[j + 1];
    const int32_t p = pos_of[query[i]], p2 = pos_of[query[i2]];
    if (p2 <= p) atomicMin(err, (unsigned long long)j);
    is_call[j] = !(i2 == i + 1 && p2 == p + 1);
}

// the called span in bases of the reference walk and of the query: first shared vertex's first base .. behind the last one's
__global__ void calls_span_kernel(const int32_t *__restrict__ query, const int32_t *__restrict__ sh, int32_t n_shared, const int32_t *__restrict__ pos_of,
                                  const int64_t *__restrict__ r_base, const int64_t *__restrict__ q_base, int32_t n_ref, int32_t n_query,
                                  int64_t *__restrict__ span)
{
    if (threadIdx.x || blockIdx.x) return;
    const int32_t i0 = sh[0], i1 = sh[n_shared - 1];
    span[0] = r_base[pos_of[query[i0]]];
    span[1] = r_base[pos_of[query[i1]] + 1];
    span[2] = q_base[i0];
    span[3] = q_base[i1 + 1];
    span[4] = r_base[n_ref];                               // the whole walks' bases
    span[5] = q_base[n_query];
}

using CallSrc = phi_ctx::PhiCallSrc;       // where an allele's bytes lie on its walk

// call k = shared pair pairs[k].  REF = the reference walk's vertices p + 1 .. p2 - 1, ALT = the query's i + 1 .. i2 - 1; when
// one is empty both get the last base of a in front, which on either walk is the base right before the allele's own.
// err[1] = the first call with an allele of 2^31 bytes or more
__global__ void __launch_bounds__(CALLS_TPB) calls_record_kernel(const int32_t *__restrict__ query, const int32_t *__restrict__ sh,
                                                                 const int32_t *__restrict__ pairs, int32_t n_calls, const int32_t *__restrict__ pos_of,
                                                                 const int64_t *__restrict__ r_base, const int64_t *__restrict__ q_base,
                                                                 int64_t *__restrict__ pos, int32_t *__restrict__ anchor, int32_t *__restrict__ ref_n,
                                                                 int32_t *__restrict__ alt_n, CallSrc *__restrict__ ref_src, CallSrc *__restrict__ alt_src,
                                                                 unsigned long long *__restrict__ err)
{
    const int64_t k = (int64_t)blockIdx.x * CALLS_TPB + threadIdx.x;
    if (k >= n_calls) return;
    const int32_t j = pairs[k];
    const int32_t i = sh[j], i2 = sh[j + 1];
    const int32_t p = pos_of[query[i]], p2 = pos_of[query[i2]];
    const int64_t r0 = r_base[p + 1], a0 = q_base[i + 1];
    int64_t rl = r_base[p2] - r0, al = q_base[i2] - a0;
    const int pad = rl == 0 || al == 0;
    rl += pad; al += pad;
    if (rl > 0x7fffffffLL || al > 0x7fffffffLL) { atomicMin(err + 1, (unsigned long long)k); rl = al = 1; }
    pos[k] = r0 - pad;
    anchor[k] = i;
    ref_n[k] = (int32_t)rl;
    alt_n[k] = (int32_t)al;
    ref_src[k] = CallSrc{r0 - pad, pad ? p : p + 1, p2};
    alt_src[k] = CallSrc{a0 - pad, pad ? i : i + 1, i2};
}

// out[off[k] .. off[k + 1]) = the bytes of walk[] (vertex lengths summed in w_base[]) from src[k].base on.  A lane owns
// CALLS_LANE_BYTES consecutive output bytes and walks forward through calls and vertices from where its searches put it;
// every allele holds at least one byte, so off[] ascends strictly.
__global__ void __launch_bounds__(CALLS_TPB) calls_fill_kernel(const int64_t *__restrict__ off, int32_t n_calls, const CallSrc *__restrict__ src,
                                                               const int32_t *__restrict__ walk, const int64_t *__restrict__ w_base,
                                                               const uint8_t *__restrict__ seq, const int64_t *__restrict__ seq_off,
                                                               uint8_t *__restrict__ out, int64_t total)
{
    const int64_t g = ((int64_t)blockIdx.x * CALLS_TPB + threadIdx.x) * CALLS_LANE_BYTES;
    if (g >= total) return;
    int32_t k = 0;
    {
        int32_t hi = n_calls;                              // the last call that starts at or before g
        while (hi - k > 1) {
            const int32_t mid = (int32_t)(((int64_t)k + hi) >> 1);
            if (off[mid] <= g) k = mid; else hi = mid;
        }
    }
    int64_t call_end = 0, vtx_end = 0, x = 0;
    int32_t vi = 0;
    const uint8_t *sp = nullptr;
    bool fresh = true;
    uint32_t word = 0;
    int n_here = 0;
#pragma unroll
    for (int b = 0; b < CALLS_LANE_BYTES; b++) {
        const int64_t o = g + b;
        if (o >= total) break;
        if (!fresh && o >= call_end) { k++; fresh = true; }
        if (fresh) {
            const CallSrc s = src[k];
            const int64_t o0 = off[k];
            call_end = off[k + 1];
            x = s.base + (o - o0);
            int32_t lo = s.v0, hi = s.v1;                  // the last vertex index in [v0, v1) whose first base is at or before x
            while (hi - lo > 1) {
                const int32_t mid = (int32_t)(((int64_t)lo + hi) >> 1);
                if (w_base[mid] <= x) lo = mid; else hi = mid;
            }
            vi = lo;
            vtx_end = w_base[vi + 1];
            sp = seq + seq_off[walk[vi]] + (x - w_base[vi]);
            fresh = false;
        } else if (x >= vtx_end) {                         // (no vertex is empty: one step)
            vi++;
            vtx_end = w_base[vi + 1];
            sp = seq + seq_off[walk[vi]];
        }
        word |= (uint32_t)(*sp++) << (8 * b);
        x++;
        n_here++;
    }
    if (n_here == CALLS_LANE_BYTES) *reinterpret_cast<uint32_t *>(out + g) = word;     // (out is 256-byte aligned, g a multiple of 4)
    else for (int b = 0; b < n_here; b++) out[g + b] = (uint8_t)(word >> (8 * b));
}

struct CallsEvents {
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~CallsEvents() { for (int i = 0; i < 5; i++) if (e[i]) (void)hipEventDestroy(e[i]); }
};

inline unsigned blocks_of(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + CALLS_TPB - 1) / CALLS_TPB); }

// The calls of a query of n_query vertices -- d_query, or when that is null the path's stretches expanded here -- against
// reference walk r.  On any refusal the context's graph, reads and result are as they were and the last calls are gone.
int calls_impl(phi_ctx *c, const char *what, const int32_t *d_query, int64_t q_ent0, int64_t n_query64, int32_t r, phi_calls *out)
{
    auto &K = c->calls;
    K.have = false;
    K.support.have = false;
    const int32_t n_vtx = c->n_vtx;
    const int64_t n_ref64 = c->h_walk_off[(size_t)r + 1] - c->h_walk_off[(size_t)r];
    if (n_query64 >= 0x7fffffffLL || n_ref64 >= 0x7fffffffLL)
        return phi_fail(c, PHI_ERR_UNSUPPORTED, "%s: a query or a reference walk of 2^31 - 1 entries or more", what);
    if (n_query64 <= 0 || n_ref64 <= 0) return phi_fail(c, PHI_ERR_UNSUPPORTED, "%s: the query and reference walk %d share no vertex", what, r);
    const int32_t n_query = (int32_t)n_query64, n_ref = (int32_t)n_ref64;
    const int32_t *d_ref = c->d_walk_vtx.as<int32_t>() + c->h_walk_off[(size_t)r];
    const int32_t *vlen = c->d_vlen.as<int32_t>();
    phi_calls_info info{};
    info.n_query = n_query; info.n_ref = n_ref;

    DevBuf d_pos_of, d_ref_len, d_q_own, d_seg, d_q_len, d_shared, d_sh, d_is_call, d_pairs, d_err, d_span;
    DevBuf d_pos, d_ref_n, d_alt_n, d_ref_off, d_alt_off, d_ref_out, d_alt_out;
    PhiDevGuard guard{{&d_pos_of, &d_ref_len, &d_q_own, &d_seg, &d_q_len, &d_shared, &d_sh, &d_is_call, &d_pairs, &d_err, &d_span,
                       &d_pos, &d_ref_n, &d_alt_n, &d_ref_off, &d_alt_off, &d_ref_out, &d_alt_out}};
    // (these five stay behind the call, for phi_calls_support)
    DevBuf &d_r_base = K.d_r_base, &d_q_base = K.d_q_base, &d_anchor = K.d_anchor, &d_ref_src = K.d_ref_src, &d_alt_src = K.d_alt_src;
    CallsEvents ev;
    for (int i = 0; i < 5; i++) HIPCHK(hipEventCreate(&ev.e[i]));
    PHICHK(phi_dev_ensure(c, d_pos_of, (size_t)n_vtx * 4));
    PHICHK(phi_dev_ensure(c, d_ref_len, (size_t)n_ref * 4));
    PHICHK(phi_dev_ensure(c, d_r_base, ((size_t)n_ref + 1) * 8));
    PHICHK(phi_dev_ensure(c, d_q_len, (size_t)n_query * 4));
    PHICHK(phi_dev_ensure(c, d_q_base, ((size_t)n_query + 1) * 8));
    PHICHK(phi_dev_ensure(c, d_shared, (size_t)n_query));
    PHICHK(phi_dev_ensure(c, d_err, 16));
    PHICHK(phi_dev_ensure(c, d_span, 48));

    // ---- table: the position of every vertex on the reference walk
    HIPCHK(hipEventRecord(ev.e[0], c->stream));
    HIPCHK(hipMemsetAsync(d_pos_of.p, 0xFF, (size_t)n_vtx * 4, c->stream));
    HIPCHK(hipMemsetAsync(d_err.p, 0xFF, 16, c->stream));
    hipLaunchKernelGGL(calls_table_kernel, dim3(blocks_of(n_ref)), dim3(CALLS_TPB), 0, c->stream, d_ref, n_ref, vlen, n_vtx, d_pos_of.as<int32_t>(),
                       d_ref_len.as<int32_t>());
    PHICHK(phi_scan(c, d_ref_len.as<int32_t>(), n_ref, d_r_base.as<int64_t>()));
    HIPCHK(hipEventRecord(ev.e[1], c->stream));

    // ---- the query's vertices, their lengths and shared flags, the shared list
    if (!d_query) {
        const size_t ns = c->path_segs.size();
        std::vector<int64_t> seg((size_t)2 * ns + 1, 0);    // [0, ns]: where every stretch starts in the query; behind: its first walk entry
        for (size_t s = 0; s < ns; s++) {
            seg[s + 1] = seg[s] + (c->path_segs[s].ee - c->path_segs[s].es + 1);
            seg[ns + 1 + s] = c->path_segs[s].es;
        }
        PHICHK(upload(c, d_seg, seg.data(), seg.size()));
        PHICHK(phi_dev_ensure(c, d_q_own, (size_t)n_query * 4));
        hipLaunchKernelGGL(calls_expand_kernel, dim3(blocks_of(n_query)), dim3(CALLS_TPB), 0, c->stream, c->d_walk_vtx.as<int32_t>(), d_seg.as<int64_t>(),
                           d_seg.as<int64_t>() + ns + 1, (int32_t)ns, n_query, d_q_own.as<int32_t>());
        HIPCHK(hipStreamSynchronize(c->stream));            // (seg is the host's: the copy has to be done before it goes)
        d_query = d_q_own.as<int32_t>();
    }
    hipLaunchKernelGGL(calls_mark_kernel, dim3(blocks_of(n_query)), dim3(CALLS_TPB), 0, c->stream, d_query, n_query, vlen, d_pos_of.as<int32_t>(), n_vtx,
                       d_q_len.as<int32_t>(), d_shared.as<uint8_t>());
    PHICHK(phi_scan(c, d_q_len.as<int32_t>(), n_query, d_q_base.as<int64_t>()));
    int64_t n_shared = 0;
    PHICHK(phi_compact(c, d_shared.as<uint8_t>(), n_query, d_sh, &n_shared));
    HIPCHK(hipEventRecord(ev.e[2], c->stream));
    info.n_shared = n_shared;
    if (n_shared == 0) {
        HIPCHK(hipStreamSynchronize(c->stream));
        return phi_fail(c, PHI_ERR_UNSUPPORTED, "%s: the query and reference walk %d share no vertex", what, r);
    }

    // ---- pairs of consecutive shared vertices: the order check, call or no call; the calls' records
    const int32_t n_pairs = (int32_t)n_shared - 1;
    info.n_pairs = n_pairs;
    int64_t n_calls = 0;
    hipLaunchKernelGGL(calls_span_kernel, dim3(1), dim3(64), 0, c->stream, d_query, d_sh.as<int32_t>(), (int32_t)n_shared, d_pos_of.as<int32_t>(),
                       d_r_base.as<int64_t>(), d_q_base.as<int64_t>(), n_ref, n_query, d_span.as<int64_t>());
    if (n_pairs > 0) {
        PHICHK(phi_dev_ensure(c, d_is_call, (size_t)n_pairs));
        hipLaunchKernelGGL(calls_pair_kernel, dim3(blocks_of(n_pairs)), dim3(CALLS_TPB), 0, c->stream, d_query, d_sh.as<int32_t>(), n_pairs,
                           d_pos_of.as<int32_t>(), d_is_call.as<uint8_t>(), d_err.as<unsigned long long>());
        PHICHK(phi_compact(c, d_is_call.as<uint8_t>(), n_pairs, d_pairs, &n_calls));
    }
    unsigned long long err[2] = {~0ull, ~0ull};
    int64_t span[6] = {0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(err, d_err.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(span, d_span.p, 48, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    if (err[0] != ~0ull)
        return phi_fail(c, PHI_ERR_WALK, "%s: shared vertices %llu and %llu of the query lie on reference walk %d in the opposite order (the graph is not acyclic along these walks)",
                        what, err[0], err[0] + 1, r);
    info.n_calls = n_calls;
    info.ref_bases = span[4]; info.query_bases = span[5];
    const size_t nc = (size_t)n_calls;
    K.pos.assign(nc, 0);
    K.anchor.assign(nc, 0);
    K.ref_off.assign(nc + 1, 0);
    K.alt_off.assign(nc + 1, 0);
    K.ref_bytes.clear();
    K.alt_bytes.clear();
    if (n_calls > 0) {
        PHICHK(phi_dev_ensure(c, d_pos, nc * 8));
        PHICHK(phi_dev_ensure(c, d_anchor, nc * 4));
        PHICHK(phi_dev_ensure(c, d_ref_n, nc * 4));
        PHICHK(phi_dev_ensure(c, d_alt_n, nc * 4));
        PHICHK(phi_dev_ensure(c, d_ref_src, nc * sizeof(CallSrc)));
        PHICHK(phi_dev_ensure(c, d_alt_src, nc * sizeof(CallSrc)));
        PHICHK(phi_dev_ensure(c, d_ref_off, (nc + 1) * 8));
        PHICHK(phi_dev_ensure(c, d_alt_off, (nc + 1) * 8));
        hipLaunchKernelGGL(calls_record_kernel, dim3(blocks_of(n_calls)), dim3(CALLS_TPB), 0, c->stream, d_query, d_sh.as<int32_t>(), d_pairs.as<int32_t>(),
                           (int32_t)n_calls, d_pos_of.as<int32_t>(), d_r_base.as<int64_t>(), d_q_base.as<int64_t>(), d_pos.as<int64_t>(),
                           d_anchor.as<int32_t>(), d_ref_n.as<int32_t>(), d_alt_n.as<int32_t>(), d_ref_src.as<CallSrc>(), d_alt_src.as<CallSrc>(),
                           d_err.as<unsigned long long>());
        PHICHK(phi_scan(c, d_ref_n.as<int32_t>(), n_calls, d_ref_off.as<int64_t>()));
        PHICHK(phi_scan(c, d_alt_n.as<int32_t>(), n_calls, d_alt_off.as<int64_t>()));
        HIPCHK(hipMemcpyAsync(err, d_err.p, 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(K.pos.data(), d_pos.p, nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(K.anchor.data(), d_anchor.p, nc * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(K.ref_off.data(), d_ref_off.p, (nc + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(K.alt_off.data(), d_alt_off.p, (nc + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipEventRecord(ev.e[3], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    if (err[1] != ~0ull) return phi_fail(c, PHI_ERR_UNSUPPORTED, "%s: call %llu has an allele of 2^31 bytes or more", what, err[1]);

    // ---- fill: the allele bytes gathered from the sequences, the work divided over the output bytes
    const int64_t ref_total = K.ref_off[nc], alt_total = K.alt_off[nc];
    info.ref_bytes = ref_total; info.alt_bytes = alt_total;
    if (std::max(ref_total, alt_total) / CALLS_FILL_TILE >= 0x7fffffffLL) return phi_fail(c, PHI_ERR_UNSUPPORTED, "%s: 2^41 allele bytes or more", what);
    K.ref_bytes.resize((size_t)ref_total);
    K.alt_bytes.resize((size_t)alt_total);
    if (n_calls > 0) {
        PHICHK(phi_dev_ensure(c, d_ref_out, (size_t)ref_total + CALLS_LANE_BYTES));
        PHICHK(phi_dev_ensure(c, d_alt_out, (size_t)alt_total + CALLS_LANE_BYTES));
        hipLaunchKernelGGL(calls_fill_kernel, dim3((unsigned)((ref_total + CALLS_FILL_TILE - 1) / CALLS_FILL_TILE)), dim3(CALLS_TPB), 0, c->stream,
                           d_ref_off.as<int64_t>(), (int32_t)n_calls, d_ref_src.as<CallSrc>(), d_ref, d_r_base.as<int64_t>(), c->d_seq.as<uint8_t>(),
                           c->d_seq_off.as<int64_t>(), d_ref_out.as<uint8_t>(), ref_total);
        hipLaunchKernelGGL(calls_fill_kernel, dim3((unsigned)((alt_total + CALLS_FILL_TILE - 1) / CALLS_FILL_TILE)), dim3(CALLS_TPB), 0, c->stream,
                           d_alt_off.as<int64_t>(), (int32_t)n_calls, d_alt_src.as<CallSrc>(), d_query, d_q_base.as<int64_t>(), c->d_seq.as<uint8_t>(),
                           c->d_seq_off.as<int64_t>(), d_alt_out.as<uint8_t>(), alt_total);
    }
    HIPCHK(hipEventRecord(ev.e[4], c->stream));
    if (n_calls > 0) {
        HIPCHK(hipMemcpyAsync(K.ref_bytes.data(), d_ref_out.p, (size_t)ref_total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(K.alt_bytes.data(), d_alt_out.p, (size_t)alt_total, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1])); info.table_gpu_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[1], ev.e[2])); info.shared_gpu_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[2], ev.e[3])); info.pairs_gpu_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[3], ev.e[4])); info.fill_gpu_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[4])); info.gpu_ms = ms;
    // the algorithmic bytes, kernel by kernel as DESIGN.md 4.16 counts them
    const int64_t nq = n_query, nr = n_ref, nsh = n_shared, np = n_pairs, ncl = n_calls;
    info.bytes_moved = 4 * (int64_t)n_vtx + 16 * nr             // table: the fill; per reference entry the entry, pos_of[], vlen[], its length
                       + (d_q_own.p ? 8 * nq : 0)               // expand: an entry read, an entry written
                       + 17 * nq                                // mark: the entry, vlen[], pos_of[], the length, the flag
                       + 16 * (nr + nq)                         // scans int32 -> int64: 4 read (twice beyond 8192 items), 8 written
                       + 2 * nq + 4 * nsh                       // shared: the flags read twice, the list written
                       + 25 * np + 2 * np + 4 * ncl             // pairs: two list items, two entries, two pos_of[], the flag; their compaction
                       + 144 * ncl                              // records: 28 of indices, 32 of base offsets, 52 written; two scans (32)
                       + 2 * (ref_total + alt_total)            // fill: a sequence byte read, a byte written
                       + 60 * ((ref_total + alt_total + 3) / 4);// fill, per lane: its call's record and offsets (32), two base offsets, the entry, seq_off[] (28); the searches' probes, shared between neighbouring lanes, are not counted
    K.info = info;
    K.ref_walk = r;
    {
        // the query as stretches of walk entries, for phi_calls_support: a walk is one stretch
        const size_t ns = q_ent0 >= 0 ? 1 : c->path_segs.size();
        K.stretches.assign(3 * ns + 1, 0);
        for (size_t s = 0; s < ns; s++) {
            const int64_t es = q_ent0 >= 0 ? q_ent0 : c->path_segs[s].es;
            K.stretches[s + 1] = K.stretches[s] + (q_ent0 >= 0 ? (int64_t)n_query : c->path_segs[s].ee - es + 1);
            K.stretches[ns + 1 + s] = es;
            K.stretches[2 * ns + 1 + s] = q_ent0 >= 0 ? q_ent0 : c->h_walk_off[(size_t)c->path_segs[s].h];
        }
    }
    K.span[0] = span[0]; K.span[1] = span[1]; K.span[2] = span[2]; K.span[3] = span[3];
    K.have = true;
    if (out) {
        out->n_calls = n_calls;
        out->pos = K.pos.data();
        out->ref_off = K.ref_off.data();
        out->alt_off = K.alt_off.data();
        out->ref_bytes = K.ref_bytes.data();
        out->alt_bytes = K.alt_bytes.data();
        out->anchor = K.anchor.data();
        out->n_shared = n_shared; out->n_query = n_query; out->n_ref = n_ref;
        out->ref_span[0] = span[0]; out->ref_span[1] = span[1];
        out->query_span[0] = span[2]; out->query_span[1] = span[3];
        out->gpu_ms = info.gpu_ms;
    }
    return PHI_OK;
}

int calls_check(phi_ctx *c, const char *what, int32_t ref_walk, phi_calls *out)
{
    if (!out) return phi_fail(c, PHI_ERR_INVALID, "%s: out is null", what);
    memset(out, 0, sizeof *out);
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "%s before phi_set_graph", what);
    PHICHK(phi_refuse_scout(c, what));
    if (ref_walk < 0 || ref_walk >= c->n_walks)
        return phi_fail(c, PHI_ERR_INVALID, "%s: reference walk %d is not among the set graph's %d walks", what, ref_walk, c->n_walks);
    return PHI_OK;
}

}  // namespace

extern "C" {

int phi_calls_path(phi_ctx *c, int32_t ref_walk, phi_calls *out)
{
    if (!c) return PHI_ERR_INVALID;
    PHICHK(calls_check(c, "phi_calls_path", ref_walk, out));
    if (!c->solved) return phi_fail(c, PHI_ERR_STATE, "phi_calls_path before phi_solve");
    HIPCHK(hipSetDevice(c->device));
    int64_t n = 0;
    for (const auto &s : c->path_segs) n += s.ee - s.es + 1;
    return calls_impl(c, "phi_calls_path", nullptr, -1, n, ref_walk, out);
}

int phi_calls_walk(phi_ctx *c, int32_t walk, int32_t ref_walk, phi_calls *out)
{
    if (!c) return PHI_ERR_INVALID;
    PHICHK(calls_check(c, "phi_calls_walk", ref_walk, out));
    if (walk < 0 || walk >= c->n_walks)
        return phi_fail(c, PHI_ERR_INVALID, "phi_calls_walk: walk %d is not among the set graph's %d walks", walk, c->n_walks);
    HIPCHK(hipSetDevice(c->device));
    return calls_impl(c, "phi_calls_walk", c->d_walk_vtx.as<int32_t>() + c->h_walk_off[(size_t)walk], c->h_walk_off[(size_t)walk],
                      c->h_walk_off[(size_t)walk + 1] - c->h_walk_off[(size_t)walk], ref_walk, out);
}

int phi_calls_stats(phi_ctx *c, phi_calls_info *out)
{
    if (!c || !out) return PHI_ERR_INVALID;
    if (!c->calls.have) return phi_fail(c, PHI_ERR_STATE, "phi_calls_stats before a phi_calls_path / phi_calls_walk that succeeded");
    *out = c->calls.info;
    return PHI_OK;
}

}  // extern "C"
