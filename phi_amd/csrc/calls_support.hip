// calls_support.hip -- the READ SUPPORT of every variant call (phi_calls_support): how many minimiser occurrences witness the
// call's ALT and REF, and how many of those the reads have seen, counted ON THE DEVICE behind the calls of calls.hip.
//
// The reference has no counterpart (it writes no calls).  THE RULE IS THIS PROJECT'S OWN (include/phi_amd.h states it in full):
// it is no genotyper's evidence field and has not been compared with any other tool.
//
// Everything the counts are made from lies in HBM after a solve and a call: the walk entries, the class of every entry
// (d_ent_cls), the class records with their position relative to the entry (rec_rel) and their table slot (rec_slot, through
// u_uid the dense id), the hit vector the reads wrote, and what calls.hip leaves behind (base offsets of both walks' entries,
// the anchors of every call).  The minimisers of a walk are never materialised (contexts.hip); here neither:
//     count    per (call, side) the TARGET ENTRIES -- those whose bases meet (A0 - k, A1): from the entry that holds base
//              max(A0 - k + 1, 0) through the one before the right anchor -- by a search of the base offsets
//     scan     phi_scan of the counts: the offsets of the (call, side, target entry) ITEMS
//     items    one lane per item, never per call (MHC_4 has alleles of thousands of entries beside one-entry ones).  The lane
//              finds its (call, side) by a search of the offsets, as calls_fill_kernel finds its call.  An occurrence that
//              lies in entry e belongs to the class of the entry its WINDOW starts in: e itself or one of the walk's own
//              entries before it, as long as fewer than w - 1 bases lie between that entry's last base and e's first (a window
//              is w k-mer starts long; phi_class_rec_kernel: rec_rel is the K-MER's first base relative to the first base of
//              the entry the window starts in, and the record of the left base's own window is not among the class records).
//              So the lane walks back from e, never below the walk's first entry, sums the lengths D of what it passed, keeps
//              the records with 0 <= rec_rel - D < bases of e and applies rule 3 in query coordinates.  At most w - 1
//              entries back.
//     sums     counts are integers: no order.  Consecutive items mostly share a (call, side): the lanes of a wave add up per
//              run of equal keys with a segmented scan (the pattern of panel_score.hip) and every run costs ONE atomicAdd
//              per counter, by its last lane.
// The counters are zeroed by a fill first; nothing is read before it is written.  Bound (from the code):
// launches and the host's waits, then the 4-byte gathers into the class records -- latency, not HBM bandwidth.
#include <string.h>
#include <algorithm>
#include "phi_ctx.h"
#include "phi_wave.h"

#define SUP_TPB 256

namespace {

using CallSrc = phi_ctx::PhiCallSrc;

struct SupArgs {
    const int32_t *anchor;                 // [n_calls] query index of the left anchor
    const CallSrc *alt_src, *ref_src;      // [n_calls]
    const int64_t *q_base, *r_base;        // base offsets of the query's and the reference walk's entries
    int32_t n_calls, k, w;
};

// side 0: ALT on the query, side 1: REF on the reference walk.  The anchors' indices lo < hi on that walk, from what the calls
// kept: a padded call's allele source starts at the left anchor itself, an unpadded one's right behind it.
struct SupSpan { int32_t lo, hi; int64_t a0, a1; const int64_t *base; };
__device__ __forceinline__ SupSpan sup_span(const SupArgs &A, int32_t call, int side)
{
    const int32_t i = A.anchor[call];
    const CallSrc as = A.alt_src[call], rs = A.ref_src[call];
    const bool pad = as.v0 == i;
    SupSpan s;
    s.lo = side ? (pad ? rs.v0 : rs.v0 - 1) : i;
    s.hi = side ? rs.v1 : as.v1;
    s.base = side ? A.r_base : A.q_base;
    s.a0 = s.base[s.lo + 1];
    s.a1 = s.base[s.hi];
    return s;
}

__global__ void __launch_bounds__(SUP_TPB) support_count_kernel(SupArgs A, int32_t *__restrict__ first, int32_t *__restrict__ cnt)
{
    const int64_t s = (int64_t)blockIdx.x * SUP_TPB + threadIdx.x;
    if (s >= 2 * (int64_t)A.n_calls) return;
    const SupSpan sp = sup_span(A, (int32_t)(s >> 1), (int)(s & 1));
    const int64_t b = sp.a0 - A.k + 1 > 0 ? sp.a0 - A.k + 1 : 0;
    int32_t lo = 0, hi = sp.lo + 2;                        // the last entry in [0, lo + 1] whose first base is at or before b
    while (hi - lo > 1) {
        const int32_t mid = (int32_t)(((int64_t)lo + hi) >> 1);
        if (sp.base[mid] <= b) lo = mid; else hi = mid;
    }
    first[s] = lo;
    cnt[s] = sp.hi > lo ? sp.hi - lo : 0;                  // (k = 1 and an empty allele: no k-mer holds both junction bases)
}

struct SupWalks {
    const int64_t *seg_out, *seg_src, *seg_first;          // the query's stretches: start in the query, first walk entry, first entry of the walk
    int32_t n_seg;
    int64_t ref_ent0;                                      // the reference walk's first entry
    const int32_t *walk_vtx, *vlen, *ent_cls, *cls_rec_off, *rec_rel;
    const uint32_t *rec_slot, *u_uid;
    const uint8_t *hit;
};

// out[0 .. 4 * n_calls): alt_hit, alt_n, ref_hit, ref_n.  tot[0] += walk entries whose class was read, tot[1] += class
// records looked at.  Every lane of a wave reaches the shuffles.
__global__ void __launch_bounds__(SUP_TPB) support_item_kernel(SupArgs A, SupWalks W, const int64_t *__restrict__ off, const int32_t *__restrict__ first,
                                                               int64_t n_items, int32_t *__restrict__ out, unsigned long long *__restrict__ tot)
{
    const int64_t g = (int64_t)blockIdx.x * SUP_TPB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t key = -1, n_wit = 0, n_hit = 0, n_vis = 0, n_rec = 0;
    if (g < n_items) {
        int32_t s = 0;
        {
            int32_t hi = 2 * A.n_calls;                    // the last (call, side) that starts at or before g: its range holds g
            while (hi - s > 1) {
                const int32_t mid = (int32_t)(((int64_t)s + hi) >> 1);
                if (off[mid] <= g) s = mid; else hi = mid;
            }
        }
        key = s;
        const int side = s & 1;
        const SupSpan sp = sup_span(A, s >> 1, side);
        const int32_t t = first[s] + (int32_t)(g - off[s]);
        int64_t e, e_first;
        if (side) { e = W.ref_ent0 + t; e_first = W.ref_ent0; }
        else {
            int lo = 0, hi = W.n_seg;                      // the last stretch that starts at or before t
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (W.seg_out[mid] <= t) lo = mid; else hi = mid;
            }
            e = W.seg_src[lo] + (t - W.seg_out[lo]);
            e_first = W.seg_first[lo];
        }
        const int64_t e_base = sp.base[t], e_len = sp.base[t + 1] - e_base;
        int64_t dist = 0;                                  // bases from the visited entry's first base to e's first base
        for (;;) {
            const int32_t c = W.ent_cls[e];
            n_vis++;
            for (int32_t r = W.cls_rec_off[c], re = W.cls_rec_off[c + 1]; r < re; r++) {
                n_rec++;
                const int64_t rel = (int64_t)W.rec_rel[r] - dist;
                if (rel < 0 || rel >= e_len) continue;     // the k-mer starts in another entry
                const int64_t x = e_base + rel;
                if (x < sp.a1 && x + A.k > sp.a0) {
                    n_wit++;
                    n_hit += W.hit[W.u_uid[W.rec_slot[r]]] != 0;
                }
            }
            // the entry before starts windows that reach e only while fewer than w - 1 bases lie between its last base and e
            if (e == e_first || dist > (int64_t)A.w - 2) break;
            e--;
            dist += W.vlen[W.walk_vtx[e]];
        }
    }
    // segmented inclusive scan over the lanes: a lane whose left neighbour holds another key starts a run
    long long x = (long long)n_hit << 32 | (unsigned)n_wit;
    const int32_t left = __shfl_up(key, 1, 64);
    int head = lane == 0 || key != left;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long y = __shfl_up(x, d, 64);
        const int f = __shfl_up(head, d, 64);
        if (lane >= d) {
            if (!head) x += y;
            head |= f;
        }
    }
    const int32_t right = __shfl_down(key, 1, 64);
    if ((lane == 63 || key != right) && key >= 0 && x) {
        int32_t *o = out + (int64_t)(key & 1) * 2 * A.n_calls + (key >> 1);
        if (x >> 32) atomicAdd(o, (int32_t)(x >> 32));
        atomicAdd(o + A.n_calls, (int32_t)(x & 0xffffffffLL));
    }
    const long long vis = phi_wave_sum((long long)n_vis), rec = phi_wave_sum((long long)n_rec);
    if (lane == 0 && vis) {
        atomicAdd(tot, (unsigned long long)vis);
        atomicAdd(tot + 1, (unsigned long long)rec);
    }
}

struct SupEvents {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~SupEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

inline unsigned blocks_of(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + SUP_TPB - 1) / SUP_TPB); }

int support_impl(phi_ctx *c, phi_call_support *out)
{
    auto &K = c->calls;
    auto &S = K.support;
    S.have = false;
    const int64_t nc = K.info.n_calls;
    phi_calls_support_info info{};
    info.n_calls = nc;
    S.cnt.assign((size_t)(4 * nc), 0);
    float ms = 0.f;
    int64_t n_items = 0;
    unsigned long long tot[2] = {0, 0};
    if (nc > 0) {
        const size_t ns = (K.stretches.size() - 1) / 3;
        DevBuf d_seg, d_first, d_cnt, d_off, d_out, d_tot;
        PhiDevGuard guard{{&d_seg, &d_first, &d_cnt, &d_off, &d_out, &d_tot}};
        SupEvents ev;
        for (hipEvent_t &x : ev.e) HIPCHK(hipEventCreate(&x));
        PHICHK(phi_dev_ensure(c, d_first, (size_t)nc * 8));
        PHICHK(phi_dev_ensure(c, d_cnt, (size_t)nc * 8));
        PHICHK(phi_dev_ensure(c, d_off, ((size_t)2 * nc + 1) * 8));
        PHICHK(phi_dev_ensure(c, d_out, (size_t)nc * 16));
        PHICHK(phi_dev_ensure(c, d_tot, 16));
        PHICHK(upload(c, d_seg, K.stretches.data(), K.stretches.size()));   // (K.stretches lives as long as the calls: the copy may land later)
        SupArgs A{K.d_anchor.as<int32_t>(), K.d_alt_src.as<CallSrc>(), K.d_ref_src.as<CallSrc>(), K.d_q_base.as<int64_t>(), K.d_r_base.as<int64_t>(),
                  (int32_t)nc, c->k, c->w};
        SupWalks W{d_seg.as<int64_t>(), d_seg.as<int64_t>() + ns + 1, d_seg.as<int64_t>() + 2 * ns + 1, (int32_t)ns, c->h_walk_off[(size_t)K.ref_walk],
                   c->d_walk_vtx.as<int32_t>(), c->d_vlen.as<int32_t>(), c->d_ent_cls.as<int32_t>(), c->d_cls_rec_off.as<int32_t>(), c->d_rec_rel.as<int32_t>(),
                   c->d_rec_slot.as<uint32_t>(), c->d_u_uid.as<uint32_t>(), c->d_hit.as<uint8_t>()};
        HIPCHK(hipEventRecord(ev.e[0], c->stream));
        HIPCHK(hipMemsetAsync(d_out.p, 0, (size_t)nc * 16, c->stream));
        HIPCHK(hipMemsetAsync(d_tot.p, 0, 16, c->stream));
        hipLaunchKernelGGL(support_count_kernel, dim3(blocks_of(2 * nc)), dim3(SUP_TPB), 0, c->stream, A, d_first.as<int32_t>(), d_cnt.as<int32_t>());
        PHICHK(phi_scan(c, d_cnt.as<int32_t>(), 2 * nc, d_off.as<int64_t>()));
        HIPCHK(hipMemcpyAsync(&n_items, d_off.as<int64_t>() + 2 * nc, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipGetLastError());
        if (n_items / SUP_TPB >= 0x7fffffffLL) return phi_fail(c, PHI_ERR_UNSUPPORTED, "phi_calls_support: 2^39 items or more");
        if (n_items > 0)
            hipLaunchKernelGGL(support_item_kernel, dim3(blocks_of(n_items)), dim3(SUP_TPB), 0, c->stream, A, W, d_off.as<int64_t>(), d_first.as<int32_t>(),
                               n_items, d_out.as<int32_t>(), d_tot.as<unsigned long long>());
        HIPCHK(hipEventRecord(ev.e[1], c->stream));
        HIPCHK(hipMemcpyAsync(S.cnt.data(), d_out.p, (size_t)nc * 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(tot, d_tot.p, 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    }
    phi_call_support &R = S.out;
    R = phi_call_support{};
    R.n_calls = nc;
    const int32_t *p = S.cnt.data();
    R.alt_hit = p; R.alt_n = p + nc; R.ref_hit = p + 2 * nc; R.ref_n = p + 3 * nc;
    for (int64_t k = 0; k < nc; k++) {
        R.alt_hit_total += R.alt_hit[k]; R.alt_n_total += R.alt_n[k];
        R.ref_hit_total += R.ref_hit[k]; R.ref_n_total += R.ref_n[k];
    }
    R.n_items = n_items;
    R.gpu_ms = ms;
    info.n_items = n_items;
    info.n_visited = (int64_t)tot[0];
    info.n_records = (int64_t)tot[1];
    info.n_witnesses = R.alt_n_total + R.ref_n_total;
    info.gpu_ms = ms;
    // the algorithmic bytes, kernel by kernel as DESIGN.md 4.16 counts them
    info.bytes_moved = 16 * nc + 16                                      // the fill of the counters
                       + 2 * nc * (4 + 32 + 16 + 8)                      // count, per (call, side): the anchor, two allele sources, two base offsets; first and count written
                       + 2 * nc * 16                                     // scan int32 -> int64 (as the calls count theirs)
                       + n_items * (12 + 4 + 32 + 16 + 16)               // items, per item: offset and first entry, the anchor, two allele sources, the interval's and the entry's base offsets
                       + info.n_visited * 12 + (info.n_visited - n_items) * 8   // per visited entry its class and the class's two record offsets; per step back the entry and its length
                       + info.n_records * 4                              // rec_rel
                       + info.n_witnesses * 9                            // rec_slot, u_uid[], the flag
                       + 8 * (2 * nc);                                   // the atomics, at least one run per (call, side): two counters (runs cut by a wave's end are not counted)
    S.info = info;
    S.have = true;
    *out = R;
    return PHI_OK;
}

}  // namespace

extern "C" {

int phi_calls_support(phi_ctx *c, phi_call_support *out)
{
    if (!c) return PHI_ERR_INVALID;
    if (!out) return phi_fail(c, PHI_ERR_INVALID, "phi_calls_support: out is null");
    memset(out, 0, sizeof *out);
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_calls_support before phi_set_graph");
    PHICHK(phi_refuse_scout(c, "phi_calls_support"));
    if (!c->calls.have) return phi_fail(c, PHI_ERR_STATE, "phi_calls_support without a current result of phi_calls_path / phi_calls_walk");
    HIPCHK(hipSetDevice(c->device));
    PHICHK(phi_sync_check(c));                                 // (the read batches so far have landed: the hit vector is the current one)
    return support_impl(c, out);
}

int phi_calls_support_stats(phi_ctx *c, phi_calls_support_info *out)
{
    if (!c || !out) return PHI_ERR_INVALID;
    if (!c->have_graph || !c->calls.have || !c->calls.support.have)
        return phi_fail(c, PHI_ERR_STATE, "phi_calls_support_stats before a phi_calls_support that succeeded");
    *out = c->calls.support.info;
    return PHI_OK;
}

}  // extern "C"
