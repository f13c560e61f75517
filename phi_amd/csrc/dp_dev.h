// dp_dev.h -- the step rules of the max-plus DP, stated once for its three serial kernels: phi_dp_kernel (dp.hip, one step
// per vertex), phi_dp_events_kernel and phi_dp_events_pc_kernel (dp_events.hip, event driven).  The solve falls back from
// one kernel to another (PHI_KERR_DP_QUEUE, PHI_KERR_DP_CLASSES, PHI_DP_DENSE) and expects the same transitions, the same
// tie-breaks and the same outputs: they are the same because they are these functions.  Device code only.
//   * the packed tops of a step: layout, what an in-edge gets from them
//   * the recombination entry into a step: which in-edge wins (larger value, lower walk, lower source step)
//   * the best states leaving a step: top1 overall, top2 on another out-edge, the lowest walk id on ties
// How a kernel keeps its runs, refills its rings and carries results out is its own business and stays in its file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "phi_dp_flags.h"

#define NEG (-(1 << 28))        // "no state" in score space
#define NEGK PHI_DP_NEGK        // "no run" in key space

// the walk of a walk entry: the last h in [lo, n_walks) with walk_off[h] <= e (lo: a walk known to begin at or before e)
__device__ __forceinline__ int phi_walk_of_entry(const int64_t *walk_off, int32_t n_walks, int64_t e, int lo = 0)
{
    int hi = n_walks;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (walk_off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// (value, walk) as one key: the larger value wins, then the smaller walk id.  0 is below every key.
__device__ __forceinline__ unsigned long long pack_vh(int32_t val, int32_t h)
{
    return ((unsigned long long)(uint32_t)(val - NEG) << 32) | (uint32_t)(0x7FFFFFFF - h);
}
__device__ __forceinline__ int32_t vh_value(unsigned long long k) { return (int32_t)(uint32_t)(k >> 32) + NEG; }
__device__ __forceinline__ int32_t vh_walk(unsigned long long k) { return 0x7FFFFFFF - (int32_t)(uint32_t)k; }

// max over the 64 lanes on the VALU: DPP rotations inside each row of 16 lanes, then the four row
// results through v_readlane.  (__shfl_xor is ds_bpermute: six LDS round trips per reduction.)
__device__ __forceinline__ int32_t wave_max_i32(int32_t v)
{
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x121, 0xF, 0xF, false));     // row_ror:1
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x122, 0xF, 0xF, false));     // row_ror:2
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xF, 0xF, false));     // row_ror:4
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xF, 0xF, false));     // row_ror:8
    const int32_t a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const int32_t c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return max(max(a, b), max(c, d));
}

// ------------------------------------------------------------------ the packed tops of a step
// 16 bytes: x = top1 value, y = top2 value, z = (top1 walk + 1) | (top1 out-edge + 1) << 10 | (top2 walk + 1) << 20
// (a walk id + 1 has 10 bits: PHI_DP_MAX_WALKS).  top1 is the best state leaving the step, top2 the best on another out-edge.
struct DpTops { int32_t t1v = NEG, t1h = -1, t1n = -1, t2v = NEG, t2h = -1; };   // value, walk, out-edge; -1: none
__device__ __forceinline__ int4 pack_tops(const DpTops t)
{
    return make_int4(t.t1v, t.t2v, (t.t1h + 1) | ((t.t1n + 1) << 10) | ((t.t2h + 1) << 20), 0);
}
// what a recombination gets that arrives from these tops over out-edge oj of their step: top1, unless top1 itself
// continues along oj (that is no recombination) -- then top2.  hh < 0: nothing leaves that way.
__device__ __forceinline__ void tops_for_edge(const int4 q, int32_t oj, int32_t &val, int32_t &hh)
{
    const int32_t t1h = (q.z & 0x3FF) - 1, t1n = ((q.z >> 10) & 0x3FF) - 1, t2h = ((q.z >> 20) & 0x3FF) - 1;
    const bool cont = t1n == oj;
    val = cont ? q.y : q.x;
    hh = cont ? t2h : t1h;
}

// ------------------------------------------------------------------ recombination entry into a step
// The best entry into the vertex of step record (ra, rb) at step `step`, uniform over the workgroup: value E (the cost
// paid), walk Eh (-1: none) and source step Esrc, written once at the end.  Larger value first, then the lower walk, then the lower source step.
// In-edges are (steps back << 8 | out-edge index at the source): three inline in the record, the rest in in_packed.
// s_top is the LDS ring of the tops of the last RG steps; older sources are read from the HBM copy `tops`, unless
// OLD_FROM_HBM is off (a kernel whose steps never reach behind its ring and that writes no HBM copy).
template <int RG, bool OLD_FROM_HBM>
__device__ __forceinline__ void dp_eval_entry(const int4 ra, const int4 rb, int32_t step, const int4 *s_top, const int32_t *in_packed,
                                              const int4 *tops, int32_t cost, int32_t &E_out, int32_t &Eh_out, int32_t &Esrc_out)
{
    int32_t E = NEG, Eh = -1, Esrc = -1;
    const int n_in = (ra.x >> 8) & 0xFF;
    auto consider = [&](const int4 q, int32_t oj, int32_t src) {
        int32_t val, hh;
        tops_for_edge(q, oj, val, hh);
        if (hh < 0) return;
        if (val > E || (val == E && (hh < Eh || (hh == Eh && src < Esrc)))) { E = val; Eh = hh; Esrc = src; }
    };
    const uint32_t b0 = (uint32_t)ra.z >> 8, b1 = (uint32_t)ra.w >> 8, b2 = (uint32_t)rb.x >> 8;
    if (n_in <= 3 && (b0 | b1 | b2) < RG) {
        // usual case: all sources in the LDS ring, the three look-ups in flight together
        const int4 q0 = s_top[(step - b0) & (RG - 1)];
        const int4 q1 = s_top[(step - b1) & (RG - 1)];
        const int4 q2 = s_top[(step - b2) & (RG - 1)];
        consider(q0, ra.z & 0xFF, step - (int32_t)b0);
        if (n_in > 1) consider(q1, ra.w & 0xFF, step - (int32_t)b1);
        if (n_in > 2) consider(q2, rb.x & 0xFF, step - (int32_t)b2);
    } else {
        for (int j = 0; j < n_in; j++) {
            const int32_t p = j == 0 ? ra.z : j == 1 ? ra.w : j == 2 ? rb.x : in_packed[ra.y + j - 3];
            const int32_t back = (int32_t)((uint32_t)p >> 8);
            const int32_t src = step - back;
            const int4 q = (back < RG || !OLD_FROM_HBM) ? s_top[src & (RG - 1)] : tops[src];
            consider(q, p & 0xFF, src);
        }
    }
    if (Eh >= 0) E -= cost;
    E_out = E; Eh_out = Eh; Esrc_out = Esrc;
}

// ------------------------------------------------------------------ best states leaving a step
// `leaving`: this lane's walk leaves the vertex with score dmax over out-edge oidx.  Returns the tops, uniform.
// One wave (lane = walk id):
__device__ __forceinline__ DpTops dp_tops_wave(bool leaving, int32_t dmax, int32_t oidx)
{
    DpTops t;
    const int32_t m1 = wave_max_i32(leaving ? dmax : NEG);
    if (m1 > NEG / 2) {
        const int l1 = __ffsll((long long)__ballot(leaving && dmax == m1)) - 1;   // lowest walk id
        t.t1v = m1; t.t1h = l1;
        t.t1n = __builtin_amdgcn_readlane(oidx, l1);
        const bool other = leaving && oidx != t.t1n;
        const int32_t m2 = wave_max_i32(other ? dmax : NEG);
        if (m2 > NEG / 2) { t.t2v = m2; t.t2h = __ffsll((long long)__ballot(other && dmax == m2)) - 1; }
    }
    return t;
}
// NW waves (thread = walk id), every thread of the workgroup calls it: two reductions through s_red[NW] and s_oidx[NW * 64]
// of the caller, three barriers; the caller puts one more before it comes back (s_oidx and s_red are rewritten).
template <int NW>
__device__ __forceinline__ DpTops dp_tops_waves(bool leaving, int32_t dmax, int32_t oidx, unsigned long long *s_red, int32_t *s_oidx)
{
    const int h = threadIdx.x, lane = h & 63, wid = h >> 6;
    DpTops t;
    s_oidx[h] = oidx;
    const int32_t m1 = wave_max_i32(leaving ? dmax : NEG);
    unsigned long long k1 = 0;
    if (m1 > NEG / 2) k1 = pack_vh(m1, wid * 64 + __ffsll((long long)__ballot(leaving && dmax == m1)) - 1);
    if (lane == 0) s_red[wid] = k1;
    __syncthreads();
    k1 = s_red[0];
#pragma unroll
    for (int x = 1; x < NW; x++) k1 = s_red[x] > k1 ? s_red[x] : k1;
    if (k1) {
        t.t1v = vh_value(k1);
        t.t1h = vh_walk(k1);
        t.t1n = s_oidx[t.t1h];
    }
    __syncthreads();
    const bool other = leaving && oidx != t.t1n;
    const int32_t m2 = wave_max_i32(other ? dmax : NEG);
    unsigned long long k2 = 0;
    if (m2 > NEG / 2) k2 = pack_vh(m2, wid * 64 + __ffsll((long long)__ballot(other && dmax == m2)) - 1);
    if (lane == 0) s_red[wid] = k2;
    __syncthreads();
    k2 = s_red[0];
#pragma unroll
    for (int x = 1; x < NW; x++) k2 = s_red[x] > k2 ? s_red[x] : k2;
    if (k2) {
        t.t2v = vh_value(k2);
        t.t2h = vh_walk(k2);
    }
    return t;
}
