// dp_events.hip -- the max-plus DP of dp.hip, event driven: only the vertices where something can
// happen are walked serially, everything else is prefix sums made by wide kernels.
//
// dp.hip spends one serial step on EVERY vertex because each lane shifts a 31-slot run-length
// window per walk entry.  Here a run of walk h that began at entry s (entered by a recombination
// of value E_s, or the walk start with E = 0) is kept as that pair only.  With
//     End(x) = number of weight-1 anchors of the walk with last entry  <= x
//     SB(s)  = number of weight-1 anchors of the walk with first entry <  s
// its score at entry x is  E_s + #{anchors inside [s, x]}, which is
//     E_s - SB(s) + End(x)                      once x - s >= 31  (no anchor spans more than 31 edges)
//     E_s + G_x[x - s]                          before that, G_x[a] = #{anchors inside [x - a, x]}
// End, SB and the 31 small counts G_x are functions of the anchor weights only: three wide kernels
// make them per DP run (phi_dp_event_fill_kernel packs them into a 48-byte record per EVENT).  An
// event is a walk entry on a vertex where the serial part has work: a recombination can enter
// (ENTRY), leave (TOPS), or the walk starts / ends.  On the synthetic MHC graph that is one vertex
// in four; chain vertices cost nothing.
//
// Per lane (= walk) the live runs form a deque in LDS.  A new run (s, E) is dropped when an older
// run already has E' >= E: the older run contains every anchor the younger one does, and ties go
// to the older run as in dp.hip.  When it is kept it evicts, from the back, the runs whose key
// E' - SB(s') is smaller than its own: they lead by fewer anchors than they trail in value and
// can never catch up.  Runs older than 30 entries are folded into one scalar (the best key).  A
// query (TOPS / walk end) is then max(best key + End, max over the few young runs of E_s + G[age]).
//
// Same transitions, same tie-breaks and the same outputs as dp.hip (which stays as the kernel for
// more than 256 walks and as the fallback): the entry rule, the packed tops and their selection are the
// functions of dp_dev.h in all three kernels, and tests/test_gpu_parity.py runs them on the same inputs.
//
// This file: which entries are events, the event records, the two step kernels and their launchers.
// Where the chain may be cut and the chain over blocks on class lanes: dp_blocks.hip.
#include <hip/hip_runtime.h>
#include "phi_kernels.h"
#include "dp_dev.h"

#define CHK PHI_DP_CHUNK
#define RING PHI_DP_RING
enum { DP_SEQ = 0, DP_ROW = 1, DP_PATH = 2 };   // modes of the event kernels (see phi_dp_events_pc_kernel)

// ------------------------------------------------------------------ static: which entries are events
__global__ void __launch_bounds__(256) phi_event_flags_kernel(const int32_t *__restrict__ walk_vtx, int64_t n_entries,
                                                              const int32_t *__restrict__ cvtx, uint8_t *__restrict__ flags)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_entries; e += (int64_t)gridDim.x * blockDim.x)
        flags[e] = cvtx[walk_vtx[e]] >= 0;
}

// ev_off[h] = first event of walk h (ev_e ascending, walk_off[n_walks] = n_entries)
__global__ void phi_event_off_kernel(const phi_ent_t *__restrict__ ev_e, int64_t n_ev, const int64_t *__restrict__ walk_off,
                                     int32_t n_walks, int64_t *__restrict__ ev_off)
{
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h > n_walks) return;
    const int64_t key = walk_off[h];
    int64_t lo = 0, hi = n_ev;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)ev_e[mid] < key) lo = mid + 1; else hi = mid;
    }
    ev_off[h] = lo;
}

void phi_launch_event_flags(hipStream_t st, const int32_t *walk_vtx, int64_t n_entries, const int32_t *cvtx, uint8_t *flags)
{
    if (n_entries <= 0) return;
    int64_t nb = (n_entries + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(phi_event_flags_kernel, dim3((unsigned)nb), dim3(256), 0, st, walk_vtx, n_entries, cvtx, flags);
}

void phi_launch_event_off(hipStream_t st, const phi_ent_t *ev_e, int64_t n_ev, const int64_t *walk_off, int32_t n_walks,
                          int64_t *ev_off)
{
    hipLaunchKernelGGL(phi_event_off_kernel, dim3((unsigned)((n_walks + 1 + 63) / 64)), dim3(64), 0, st, ev_e, n_ev,
                       walk_off, n_walks, ev_off);
}

// ------------------------------------------------------------------ per run: event records
// One 48-byte record per event:
//   int4  A = { compact step | overflow << 31, entry (phi_ent_t), End (inclusive), SB }
//         End / SB = weight-1 anchors of the walk that end at or before / begin before the entry.  With the anchors sorted by
//         last entry and W = prefix sums of their weights (wpre), "end before entry x" is W[g_off[x]]; an anchor that
//         begins before e and ends at or after it ends within the next 30 entries (span <= 31): a short range to look at.
//         (Until round 3 both came from per-ENTRY counters -- two arrays of 4 bytes per walk entry zeroed, filled by an
//          atomic per anchor and prefix-summed in every DP run: 35 of a run's 204 ms at chromosome scale.)
//   32 B  G : byte a (1..30) = #{weight-1 anchors of the walk inside [entry - a, entry]}, byte 0 = 0,
//             byte 31 = out-edge index of the entry (255: the walk ends here)
// overflow: more than 255 anchors end inside the window (the DP then counts from the CSR).
// The anchors an event looks at -- those ending on the 30 entries up to it (G, End) and on the 31 from it (SB) -- are ONE range
// of the list sorted by last entry, and the ranges of a block's 256 consecutive events overlap almost entirely: the block loads
// the union once, coalesced, into LDS (last entry; span | weight << 7) and every event counts from there.  (Round 3: every
// event walked its ranges in global memory, three dependent loads per anchor and 24 anchors per event at config 5: 30 ms per
// DP run.)  A block whose union is longer than the stage (events far apart along chain vertices) reads global memory as before.
// (3 072 entries = 15 KB: ten workgroups per CU; with 6 144 -- five -- the kernel took 19-21 instead of 15.6 ms at config 5, with 1 024
//  too many blocks fell back to global memory: 18.8)
#define EVF_STAGE 3072
__global__ void __launch_bounds__(256) phi_dp_event_fill_kernel(const phi_ent_t *__restrict__ ev_e, int64_t n_ev,
                                                                const int32_t *__restrict__ walk_vtx,
                                                                const int32_t *__restrict__ cvtx,
                                                                const int64_t *__restrict__ walk_off, int32_t n_walks,
                                                                const uint8_t *__restrict__ e_out,
                                                                const int64_t *__restrict__ g_off,
                                                                const uint8_t *__restrict__ g_span,
                                                                const uint8_t *__restrict__ a_weight,
                                                                const phi_ent_t *__restrict__ a_e1,
                                                                const int32_t *__restrict__ wpre, int64_t n_entries,
                                                                uint4 *__restrict__ ev)
{
    __shared__ uint32_t s_e1[EVF_STAGE];
    __shared__ uint8_t s_sw[EVF_STAGE];
    __shared__ int64_t s_rng[2];
    const int64_t n_blocks = (n_ev + 255) / 256;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t i = blk * 256 + threadIdx.x;
        const bool in = i < n_ev;
        const int64_t e = ev_e[in ? i : n_ev - 1];
        // walk of e: last h with walk_off[h] <= e.  Events are in entry order: nearly every wave lies inside one walk --
        // found once, for the wave's first event, on the scalar unit; the lanes search for themselves only when the wave
        // straddles walks (eight dependent loads per event otherwise, for 2.4 * 10^8 events per DP run at chromosome scale)
        const int64_t e1st = ((int64_t)__builtin_amdgcn_readfirstlane((int)(e >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)e);
        int lo = phi_walk_of_entry(walk_off, n_walks, e1st);
        if (__ballot(e >= walk_off[lo + 1]) != 0ull) lo = phi_walk_of_entry(walk_off, n_walks, e, lo);    // (wave-uniform; events ascend: from the first one's walk on)
        const int64_t eb = walk_off[lo];
        const int64_t x0 = e - 29 > eb ? e - 29 : eb;
        const int64_t xe = e + 31 < n_entries ? e + 31 : n_entries;
        // the dp anchors are sorted by their last entry: those ending on the entries x0 .. e are ONE range of the list (two
        // loads of the CSR instead of two per entry of the window), those ending on e .. e + 30 another
        const int64_t g_lo = g_off[x0], g_e = g_off[e], g_hi = g_off[e + 1], g_fe = g_off[xe];
        if (threadIdx.x == 0) s_rng[0] = g_lo;                 // (both bounds grow with the event)
        if (i == (n_ev < blk * 256 + 256 ? n_ev : blk * 256 + 256) - 1) s_rng[1] = g_fe;
        __syncthreads();
        const int64_t gb = s_rng[0], ge = s_rng[1];
        const bool staged = ge - gb <= EVF_STAGE;
        if (staged)
            for (int64_t j = threadIdx.x; j < ge - gb; j += 256) {
                s_e1[j] = a_e1[gb + j];
                s_sw[j] = (uint8_t)(g_span[gb + j] | (a_weight[gb + j] ? 0x80 : 0));
            }
        __syncthreads();
        if (in) {
            unsigned long long w[4] = {0, 0, 0, 0};
            int total = 0;
            int32_t sb_extra = 0;
            auto count = [&](int a) {                          // age a run needs to contain this anchor
                if (a > 30) return;
                total++;
                const unsigned long long one = 1ull << (8 * (a & 7));
                if ((a >> 3) == 0) w[0] += one; else if ((a >> 3) == 1) w[1] += one; else if ((a >> 3) == 2) w[2] += one; else w[3] += one;
            };
            const uint32_t e32 = (uint32_t)e;
            if (staged) {
                for (int64_t g = g_lo - gb; g < g_hi - gb; g++) {
                    const uint32_t sw = s_sw[g];
                    if (sw & 0x80) count((int)(e32 - (s_e1[g] - (sw & 0x7F))));
                }
                for (int64_t g = g_e - gb; g < g_fe - gb; g++) {
                    const uint32_t sw = s_sw[g];
                    sb_extra += (sw & 0x80) && (int64_t)s_e1[g] - (int64_t)(sw & 0x7F) < e;
                }
            } else {
                for (int64_t g = g_lo; g < g_hi; g++)
                    if (a_weight[g]) count((int)(e - ((int64_t)a_e1[g] - g_span[g])));
                for (int64_t g = g_e; g < g_fe; g++) sb_extra += a_weight[g] && (int64_t)a_e1[g] - g_span[g] < e;
            }
            const bool ovf = total > 255;
            // byte-wise inclusive prefix sums across the four words
            unsigned long long carry = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                w[q] = w[q] * 0x0101010101010101ull + carry * 0x0101010101010101ull;
                carry = w[q] >> 56;
            }
            w[3] = (w[3] & 0x00FFFFFFFFFFFFFFull) | ((unsigned long long)e_out[e] << 56);
            // End and SB count from the walk's first entry (anchors of earlier walks have both begun and ended before it):
            // keys E - SB stay within the score range whatever the number of walks
            const int32_t base = wpre[g_off[eb]];
            uint4 A;
            A.x = (uint32_t)cvtx[walk_vtx[e]] | (ovf ? 0x80000000u : 0u);
            A.y = (uint32_t)e;
            A.z = (uint32_t)(wpre[g_hi] - base);
            A.w = (uint32_t)(wpre[g_e] - base + sb_extra);
            ev[i * 3 + 0] = A;
            ev[i * 3 + 1] = make_uint4((uint32_t)w[0], (uint32_t)(w[0] >> 32), (uint32_t)w[1], (uint32_t)(w[1] >> 32));
            ev[i * 3 + 2] = make_uint4((uint32_t)w[2], (uint32_t)(w[2] >> 32), (uint32_t)w[3], (uint32_t)(w[3] >> 32));
        }
        __syncthreads();                                       // (the stage is refilled for the next block of events)
    }
}

void phi_launch_dp_event_fill(hipStream_t st, const PhiDpEventArgs &A, const uint8_t *e_out, const int32_t *walk_vtx,
                              const int32_t *cvtx, const phi_ent_t *a_e1, const int32_t *wpre, int64_t n_entries)
{
    if (A.n_ev <= 0) return;
    int64_t nb = (A.n_ev + 255) / 256;
    if (nb > 16384) nb = 16384;
    hipLaunchKernelGGL(phi_dp_event_fill_kernel, dim3((unsigned)nb), dim3(256), 0, st, A.ev_e, A.n_ev, walk_vtx, cvtx,
                       A.walk_off, A.n_walks, e_out, A.g_off, A.g_span, A.a_weight, a_e1, wpre, n_entries,
                       reinterpret_cast<uint4 *>(A.ev));
}

// ------------------------------------------------------------------ the DP
// (the entry rule, the tops and their selection: dp_dev.h, shared with dp.hip.  What follows is the consumer
//  kernel's own path for steps with at most two out-edges in use.)
// (score, walk) of a leaving state as one key: larger score first, then the lower walk id.  Scores lie
// above NEG = -2^28, so the key is below 2^38: a positive (denormal) double bit pattern, whose IEEE order
// is the integer order -- v_max_f64 reduces it, and the winner's walk comes out of the key (no ballot,
// no find-first, no branches).  0 = no leaving state.
__device__ __forceinline__ unsigned long long ev_key(int32_t val, int lane)
{
    return ((unsigned long long)(uint32_t)(val - NEG) << 8) | (unsigned long long)(255 - lane);
}
__device__ __forceinline__ unsigned long long ev_max_u53(unsigned long long a, unsigned long long b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(__longlong_as_double((long long)a)), "v"(__longlong_as_double((long long)b)));
    return (unsigned long long)__double_as_longlong(r);
}
#define EV_DPP64(x, ctrl, rm, bc)                                                                                             \
    (((unsigned long long)(uint32_t)__builtin_amdgcn_update_dpp((int)((x) >> 32), (int)((x) >> 32), ctrl, rm, 0xF, bc) << 32) | \
     (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(x), (int)(uint32_t)(x), ctrl, rm, 0xF, bc))
// wave maxima of two keys, the two DPP chains interleaved; the result is uniform (read from lane 63)
__device__ __forceinline__ void ev_wave_max2_key(unsigned long long a, unsigned long long b, unsigned long long &ma, unsigned long long &mb)
{
    a = ev_max_u53(a, EV_DPP64(a, 0x121, 0xF, false)); b = ev_max_u53(b, EV_DPP64(b, 0x121, 0xF, false));   // row_ror:1
    a = ev_max_u53(a, EV_DPP64(a, 0x122, 0xF, false)); b = ev_max_u53(b, EV_DPP64(b, 0x122, 0xF, false));   // row_ror:2
    a = ev_max_u53(a, EV_DPP64(a, 0x124, 0xF, false)); b = ev_max_u53(b, EV_DPP64(b, 0x124, 0xF, false));   // row_ror:4
    a = ev_max_u53(a, EV_DPP64(a, 0x128, 0xF, false)); b = ev_max_u53(b, EV_DPP64(b, 0x128, 0xF, false));   // row_ror:8
    a = ev_max_u53(a, EV_DPP64(a, 0x142, 0xA, false)); b = ev_max_u53(b, EV_DPP64(b, 0x142, 0xA, false));   // row_bcast:15 into rows 1, 3
    a = ev_max_u53(a, EV_DPP64(a, 0x143, 0xC, false)); b = ev_max_u53(b, EV_DPP64(b, 0x143, 0xC, false));   // row_bcast:31 into rows 2, 3
    ma = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(a >> 32), 63) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)a, 63);
    mb = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(b >> 32), 63) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, 63);
}

// exact count for an event whose window overflowed the byte counters: weight-1 anchors inside [es, e]
__device__ int32_t ev_count_inside(const PhiDpEventArgs &A, int64_t es, int64_t e)
{
    int32_t n = 0;
    for (int64_t x = es; x <= e; x++)
        for (int64_t g = A.g_off[x]; g < A.g_off[x + 1]; g++)
            if (A.a_weight[g] && x - A.g_span[g] >= es) n++;
    return n;
}

// MODE: DP_SEQ (one workgroup, all steps) or DP_PATH (one workgroup per block of steps, from the block's entry
// vector A.blk_S; see the modes of phi_dp_events_pc_kernel below)
template <int NW, int MODE>   // waves in the workgroup: 2 or 4 (one wave of walks takes phi_dp_events_pc_kernel)
__global__ void __launch_bounds__(NW * 64) phi_dp_events_kernel(PhiDpEventArgs A)
{
    static_assert(NW == 2 || NW == 4, "65..128 or 129..256 walks");
    constexpr int NT = NW * 64;
    constexpr int D = NW == 2 ? 8 : 4;               // per-lane ring of event records
    constexpr int P = D / 2;                         // refill period in steps
    // four waves: 160 KB of LDS hold queues of 16 runs (31 can be alive in theory, 2-3 are in practice: a
    // deeper one raises PHI_KERR_DP_QUEUE and the caller reruns with dp.hip) and the tops of 512 steps
    constexpr int QD = NW == 2 ? 32 : 16;
    constexpr int RNG = NW == 2 ? RING : 512;
    __shared__ int4 s_rec[2][CHK][2];
    __shared__ int4 s_top[RNG];                     // packed tops of recent steps
    __shared__ uint4 s_ev[D][3][NT];
    __shared__ int32_t s_qs[QD][NT], s_qE[QD][NT], s_qK[QD][NT];   // live young runs: start, value, key
    const int32_t q_limit = A.q_limit > 0 && A.q_limit < QD ? A.q_limit : (QD == 32 ? 32 : QD);
    __shared__ unsigned long long s_red[NW];
    __shared__ int32_t s_oidx[NT];

    const int h = threadIdx.x;
    const bool has_walk = h < A.n_walks;
    const int64_t eb = has_walk ? A.walk_off[h] : 0;
    const int64_t ee = has_walk ? A.walk_off[h + 1] : 0;
    const int32_t sb = MODE == DP_PATH ? (int32_t)blockIdx.x : 0;
    const int32_t kbeg = MODE == DP_PATH ? A.blk_lo[sb] : 0, kend = MODE == DP_PATH ? A.blk_lo[sb + 1] : A.n_k;
    // events of this lane: [vb, ve) (DP_PATH: from the first one inside the block)
    const int64_t vb = !has_walk ? 0 : MODE == DP_PATH ? (int64_t)A.blk_ev[(int64_t)sb * A.lane_stride + h] : A.ev_off[h];
    const int64_t ve = has_walk ? A.ev_off[h + 1] : 0;
    int64_t vi = vb;                                 // next event
    int64_t wl = vb;                                 // first event not yet in the ring
    const uint4 *evg = reinterpret_cast<const uint4 *>(A.ev);

    // ring refill in two halves (see dp.hip): loads issued at step 0 mod P land P/2 steps later
    uint4 wtmp[P][3];
    int64_t whi = vb;
    auto issue = [&]() {
        whi = min(ve, vi + D);
#pragma unroll
        for (int j = 0; j < P; j++) {
            const int64_t x = (ve > vb) ? min(wl + j, ve - 1) : 0;
            wtmp[j][0] = evg[x * 3 + 0]; wtmp[j][1] = evg[x * 3 + 1]; wtmp[j][2] = evg[x * 3 + 2];
        }
    };
    auto land = [&]() {
#pragma unroll
        for (int j = 0; j < P; j++) {
            const int64_t x = wl + j;
            if (x < whi) {
                const int sl = (int)(x & (D - 1));
                s_ev[sl][0][h] = wtmp[j][0]; s_ev[sl][1][h] = wtmp[j][1]; s_ev[sl][2][h] = wtmp[j][2];
            }
        }
        wl = max(wl, min(whi, wl + P));
    };
    if (A.n_ev > 0) { issue(); land(); issue(); land(); }
    // the next event of this lane, in registers
    uint4 cA = make_uint4(0xFFFFFFFFu, 0, 0, 0);
    if (vi < ve) cA = s_ev[vi & (D - 1)][0][h];

    int32_t qh = 0, qt = 0;                          // deque [qh, qt) of young runs
    int32_t M = NEGK, sL = 0, Emax = NEG;            // best key of the old runs, its start; best value ever entered
    if (MODE == DP_PATH) { sL = -1; if (has_walk) M = A.blk_S[(int64_t)sb * A.lane_stride + h]; }   // (-1: began before this block)

    const int32_t n_steps = kend - kbeg;
    const int n_chunks = (n_steps + CHK - 1) / CHK;
    auto stage = [&](int c) {
        const int b = c & 1;
        const int32_t s0 = kbeg + c * CHK;
        const int32_t ns = min(CHK, kend - s0);
        const int4 *src = reinterpret_cast<const int4 *>(A.k_rec + (int64_t)s0 * 8);
        int4 *dst = &s_rec[b][0][0];
        for (int i = h; i < ns * 2; i += NT) dst[i] = src[i];
    };
    stage(0);
    __syncthreads();

    for (int c = 0; c < n_chunks; c++) {
        const int b = c & 1;
        if (c + 1 < n_chunks) stage(c + 1);
        const int32_t s0 = kbeg + c * CHK;
        const int32_t ns = min(CHK, kend - s0);
        int4 ra = s_rec[b][0][0], rb = s_rec[b][0][1];
        for (int i = 0; i < ns; i++) {
            const int inx = min(i + 1, CHK - 1);
            const int4 na = s_rec[b][inx][0], nb = s_rec[b][inx][1];
            if ((c | i) && (i & (P - 1)) == 0) issue();
            if ((c | i) && (i & (P - 1)) == P / 2) {
                land();
                if (vi < ve) cA = s_ev[vi & (D - 1)][0][h];     // (a peek made before its record landed saw a stale slot)
            }
            const int32_t k = s0 + i;
            const int32_t flags = ra.x;
            const bool active = (int32_t)(cA.x & 0x7FFFFFFFu) == k;      // (no event: 0xFFFFFFFF, a step no block reaches)

            // ---- recombination entry into this vertex (uniform over the workgroup)
            int32_t E = NEG, Eh = -1, Esrc = -1;
            if (flags & PHI_DP_NEED_ENTRY) {
                dp_eval_entry<RNG, true>(ra, rb, k, s_top, A.k_in_packed, reinterpret_cast<const int4 *>(A.tops), A.cost, E, Eh, Esrc);
                if (h == 0) { A.ent_src[k] = Esrc; A.ent_h[k] = Eh; }
            }

            int32_t dmax = NEG;
            int32_t oidx = 255;
            if (active) {
                const int64_t e = (int64_t)cA.y;
                const bool ovf = (cA.x >> 31) != 0;
                const int32_t t = (int32_t)(e - eb);
                const int32_t End = (int32_t)cA.z, SB = (int32_t)cA.w;
                const int sl = (int)(vi & (D - 1));
                const uint8_t *gb = reinterpret_cast<const uint8_t *>(&s_ev[sl][1][h]);
                oidx = reinterpret_cast<const uint8_t *>(&s_ev[sl][2][h])[15];
                // runs older than 30 entries: one scalar
                while (qh != qt && t - s_qs[qh & (QD - 1)][h] >= 31) {
                    const int32_t key = s_qK[qh & (QD - 1)][h];
                    if (key > M) { M = key; sL = s_qs[qh & (QD - 1)][h]; }
                    qh++;
                }
                // a run begins here: the walk start, or a recombination entry worth keeping
                int32_t newE = NEG;
                if (t == 0) { newE = 0; qh = qt = 0; M = NEGK; Emax = NEG; }
                else if ((flags & PHI_DP_NEED_ENTRY) && Eh >= 0) newE = E;
                if (newE > Emax) {
                    Emax = newE;
                    const int32_t key = newE - SB;
                    while (qh != qt && s_qK[(qt - 1) & (QD - 1)][h] < key) qt--;
                    if (qt - qh >= q_limit) { atomicOr(A.err, PHI_KERR_DP_QUEUE); qt--; }   // result void: the caller falls back
                    s_qs[qt & (QD - 1)][h] = t; s_qE[qt & (QD - 1)][h] = newE; s_qK[qt & (QD - 1)][h] = key;
                    qt++;
                }
                if ((flags & PHI_DP_NEED_TOPS) || e == ee - 1) {
                    // oldest first, strict improvement: ties keep the older run
                    int32_t best = M > NEGK / 2 ? M + End : NEG, bs = sL;
                    for (int32_t j = qh; j != qt; j++) {
                        const int32_t s = s_qs[j & (QD - 1)][h];
                        const int a = t - s;
                        int32_t inside;
                        if (!ovf) inside = a < 16 ? gb[a] : reinterpret_cast<const uint8_t *>(&s_ev[sl][2][h])[a - 16];
                        else inside = ev_count_inside(A, eb + s, e);
                        const int32_t val = s_qE[j & (QD - 1)][h] + inside;
                        if (val > best) { best = val; bs = s; }
                    }
                    if (best > NEG / 2) { dmax = best; A.dmax[e] = best; A.bstart[e] = bs; }
                    else { A.dmax[e] = NEG; A.bstart[e] = 0; }
                }
                vi++;
                cA = make_uint4(0xFFFFFFFFu, 0, 0, 0);
                if (vi < ve) cA = s_ev[vi & (D - 1)][0][h];
            }

            // ---- best states leaving this vertex (dp_dev.h)
            if (flags & PHI_DP_NEED_TOPS) {
                const bool leaving = active && oidx != 255 && dmax > NEG / 2;
                const DpTops t = dp_tops_waves<NW>(leaving, dmax, oidx, s_red, s_oidx);
                if (h == 0) {
                    const int4 q = pack_tops(t);
                    s_top[k & (RNG - 1)] = q;
                    reinterpret_cast<int4 *>(A.tops)[k] = q;
                }
                __syncthreads();                             // ring entry visible to the other waves
            }
            ra = na; rb = nb;
        }
        __threadfence_block();
        __syncthreads();
    }
    if (MODE == DP_PATH) {
        // what crosses the cut at the block's end: the best key of this walk's live runs (oldest first, ties keep the
        // older run) and where that run began
        int32_t best = M > NEGK / 2 ? M : NEGK, bs = sL;
        for (int32_t j = qh; j != qt; j++) {
            const int32_t key = s_qK[j & (QD - 1)][h];
            if (key > best) { best = key; bs = s_qs[j & (QD - 1)][h]; }
        }
        A.blk_keys_out[(int64_t)sb * A.lane_stride + h] = (has_walk && vb < ve) ? best : NEGK;
        A.blk_carry[(int64_t)sb * A.lane_stride + h] = bs;
    }
}

// ------------------------------------------------------------------ up to 64 walks: consumer + producers
// The serial wave (the consumer) touches LDS only.  NPW producer waves of the same workgroup keep it
// fed and carry its results out, one barrier every P steps:
//   * refill the per-lane event ring from HBM and stage the step records, a period ahead;
//   * write the (best score, run start) pairs of the events consumed in the previous period, the
//     packed tops and the entry choices of its steps back to HBM.
//
// BLOCKS OF STEPS IN PARALLEL.  The chain over the compact steps can be cut between steps k-1 and k when no
// recombination edge crosses the cut and, on every walk, no anchor spans it (phi_solve.hip picks such "clean"
// cuts): a run that crosses a clean cut scores its anchors left and right of it independently, so all that
// crosses is ONE number per walk -- the best key  E_s - SB(s)  of its live runs -- and the steps of a block are a
// max-plus linear map of that vector.  Three modes of the same kernel:
//   DP_SEQ   one workgroup walks all steps (the only mode for graphs without usable cuts)
//   DP_ROW   one workgroup per (block, entry walk j): the block's steps from the unit vector "key 0 on walk j"
//            (walk starts inside the block only in the extra row j = n_walks) -> row j of the block's transfer
//            matrix: the keys on all walks at the block's end, and the best value of a path ending inside
//   DP_PATH  one workgroup per block, from the TRUE entry vector (the host chains the matrices): writes what
//            DP_SEQ writes (best scores / run starts per event, tops, entries) plus, per walk, where the run
//            that carries the best key out of the block began -- the backtrack follows runs across blocks

// CK: steps of the step stream staged at a time (two chunks in LDS).  Blocks of at most 64 steps -- the class-lane blocks of a
// chromosome-scale graph are ~18 -- take CK = 32 and a ring of 64 tops: 26 instead of 35 KB of LDS, six workgroups per CU instead of four.
template <int NPW, int MODE, int P, int RINGT, int QD, int CK = CHK>
__global__ void __launch_bounds__(64 * (1 + NPW)) phi_dp_events_pc_kernel(PhiDpEventArgs A)
{
    constexpr int D = 2 * P;
    constexpr int PER_CHUNK = CK / P;
    static_assert(P % NPW == 0 && CK % P == 0, "ring geometry");
    __shared__ int4 s_rec[2 * CK][2];              // step records: ring of two chunks, index = (step - k0) mod 2*CHK
    __shared__ int4 s_top[RINGT];                   // packed tops of recent steps
    __shared__ int2 s_ent[2 * P];                   // (source step, walk) of the entries of the last two periods
    __shared__ uint4 s_ev[D][3][64];
    __shared__ int4 s_res[D][64];                   // (best score, run start, entry) of consumed events
    __shared__ int32_t s_qs[QD][64], s_qE[QD][64], s_qK[QD][64];
    __shared__ int32_t s_vi[2][64];              // the consumer's position at each barrier, double-buffered: written for period p + 1 while the producers still read period p's

    const int wave = threadIdx.x >> 6, h = threadIdx.x & 63;
    // the block of steps of this workgroup, and (DP_ROW) the lane the unit vector sits on.  DP_ROW may run on CLASS
    // LANES (A.lane_walk, more than 64 walks): lane l stands for all walks that do the same inside the block and is
    // played by the first of them; rows 0..63 are the class lanes, row 64 the walk starts.
    const bool cls = MODE == DP_ROW && A.lane_walk != nullptr;
    const unsigned n_rows = cls ? 65u : (unsigned)(A.n_walks + 1);
    int32_t sb = 0, row_j = -1;
    if (MODE == DP_ROW) { sb = (int32_t)(blockIdx.x / n_rows); row_j = (int32_t)(blockIdx.x % n_rows); }
    if (MODE == DP_PATH) sb = (int32_t)blockIdx.x;
    const bool start_row = MODE == DP_ROW && row_j == (int32_t)n_rows - 1;
    int32_t w = h;                                   // the walk behind this lane
    bool has_walk = h < A.n_walks;
    if (cls) { w = A.lane_walk[(int64_t)sb * 64 + h]; has_walk = w >= 0; if (!has_walk) w = 0; }
    const int32_t k0 = MODE == DP_SEQ ? 0 : A.blk_lo[sb];
    const int32_t k1 = MODE == DP_SEQ ? A.n_k : A.blk_lo[sb + 1];
    const int32_t n_steps = k1 - k0;
    const phi_ent_t eb = has_walk ? (phi_ent_t)A.walk_off[w] : 0;
    const phi_ent_t e_last = has_walk ? (phi_ent_t)(A.walk_off[w + 1] - 1) : 0xFFFFFFFFu;     // (0xFFFFFFFF: no entry, PHI_MAX_ENTRIES)
    const int32_t v0 = has_walk ? (int32_t)A.ev_off[w] : 0;     // events of this lane's walk: [v0, ve)
    const int32_t ve = has_walk ? (int32_t)A.ev_off[w + 1] : 0;
    const int32_t vb = MODE == DP_SEQ ? v0 : (has_walk ? A.blk_ev[(int64_t)sb * A.lane_stride + w] : 0);   // first event inside the block
    const int n_per = (n_steps + P - 1) / P;
    if (MODE == DP_ROW && !start_row) {
        const int32_t wj = cls ? A.lane_walk[(int64_t)sb * 64 + row_j] : row_j;
        if (wj < 0) return;                                      // no such class in this block (uniform)
        // a walk that has not begun before the block, or has no event left, carries nothing in: the row is empty
        const int32_t jb = A.blk_ev[(int64_t)sb * A.lane_stride + wj];
        if (jb <= (int32_t)A.ev_off[wj] || jb >= (int32_t)A.ev_off[wj + 1]) {            // uniform over the workgroup
            if (wave == 0) {
                A.row_out[(int64_t)blockIdx.x * 64 + h] = NEGK;
                if (h == 0) { A.rowend_out[blockIdx.x] = NEG; if (A.rownew_out) A.rownew_out[blockIdx.x] = NEGK; if (A.rowdiag_out) A.rowdiag_out[(int64_t)sb * 64 + row_j] = NEGK; }
            }
            return;
        }
    }

    if (wave > 0) {
        // ================================================================ producers
        const int pw = wave - 1;
        const uint4 *evg = reinterpret_cast<const uint4 *>(A.ev);
        auto stage = [&](int c) {
            const int32_t s0 = k0 + c * CK;
            const int32_t ns = min(CK, k1 - s0);
            const int4 *src = reinterpret_cast<const int4 *>(A.k_rec + (int64_t)s0 * 8);
            int4 *dst = &s_rec[(c & 1) * CK][0];
            for (int i = pw * 64 + h; i < ns * 2; i += 64 * NPW) dst[i] = src[i];
        };
        stage(0);
#pragma unroll
        for (int n = 0; n < D / NPW; n++) {
            const int32_t x = vb + pw + n * NPW;
            if (x < ve) {
                const uint4 a = evg[(int64_t)x * 3 + 0], g0 = evg[(int64_t)x * 3 + 1], g1 = evg[(int64_t)x * 3 + 2];
                s_ev[x & (D - 1)][0][h] = a; s_ev[x & (D - 1)][1][h] = g0; s_ev[x & (D - 1)][2][h] = g1;
            }
        }
        int32_t wl = min(ve, vb + D);                // first event not in the ring (the same in every producer wave)
        int32_t vprev = vb;                          // consumer position one barrier ago
        __syncthreads();                             // B_0
        for (int p = 0;; p++) {
            const int32_t vi = has_walk ? s_vi[p & 1][h] : 0;
            if (MODE != DP_ROW) {
                // 1. results of the events consumed during the previous period
#pragma unroll
                for (int n = 0; n < P / NPW; n++) {
                    const int32_t x = vprev + pw + n * NPW;
                    if (x < vi) {
                        const int4 r = s_res[x & (D - 1)][h];
                        A.dmax[(phi_ent_t)r.z] = r.x; A.bstart[(phi_ent_t)r.z] = r.y;
                    }
                }
                // 2. tops and entry choices of the previous period's steps (values of steps without
                //    TOPS / ENTRY are never read back)
                if (pw == 0 && p > 0 && h < P) {
                    const int32_t r = (p - 1) * P + h;
                    if (r < n_steps) {
                        const int32_t k = k0 + r;
                        reinterpret_cast<int4 *>(A.tops)[k] = s_top[k & (RINGT - 1)];
                        const int2 en = s_ent[r & (2 * P - 1)];
                        A.ent_src[k] = en.x; A.ent_h[k] = en.y;
                    }
                }
            }
            if (p == n_per) break;                   // after the last barrier: only the write-backs
            // 3. refill: events [wl, min(ve, vi + D)), at most P of them; all loads first
            const int32_t hi = min(ve, vi + D);
            uint4 t0[P / NPW], t1[P / NPW], t2[P / NPW];
#pragma unroll
            for (int n = 0; n < P / NPW; n++) {
                const int64_t xc = (ve > v0) ? min(wl + pw + n * NPW, ve - 1) : 0;
                t0[n] = evg[xc * 3 + 0]; t1[n] = evg[xc * 3 + 1]; t2[n] = evg[xc * 3 + 2];
            }
#pragma unroll
            for (int n = 0; n < P / NPW; n++) {
                const int32_t x = wl + pw + n * NPW;
                if (x < hi) { s_ev[x & (D - 1)][0][h] = t0[n]; s_ev[x & (D - 1)][1][h] = t1[n]; s_ev[x & (D - 1)][2][h] = t2[n]; }
            }
            wl = max(wl, min(hi, wl + P));
            // 4. the step records of the next chunk
            if (p % PER_CHUNK == 0 && (p / PER_CHUNK + 1) * CK < n_steps) stage(p / PER_CHUNK + 1);
            vprev = vi;
            __syncthreads();                         // B_{p+1}
        }
        return;
    }

    // ==================================================================== the consumer
    int32_t vi = vb;                                 // next event
    s_vi[0][h] = vi;
    __syncthreads();                                 // B_0
    uint4 cA = make_uint4(0xFFFFFFFFu, 0, 0, 0);     // the next event of this lane, in registers
    if (vi < ve) cA = s_ev[vi & (D - 1)][0][h];
    // live young runs: deque in LDS; the head (start, value) and the tail key also in registers
    int32_t qh = 0, qn = 0, hs = 0, hE = 0, tk = 0;
    int32_t M = NEGK, sL = MODE == DP_SEQ ? 0 : -1, Emax = NEG;   // best key of the old runs and its start (-1: began before this block); best value ever entered
    if (MODE == DP_ROW && h == row_j) M = 0;
    if (MODE == DP_PATH && has_walk) M = A.blk_S[(int64_t)sb * A.lane_stride + h];
    const bool starts_on = MODE != DP_ROW || start_row;   // walks may begin inside the block
    int32_t endbest = NEG;
    int32_t Kn = NEGK;                               // DP_ROW: best key of a run that began inside the block on this lane                           // DP_ROW: best value at a walk's last entry inside the block
    int4 ra = s_rec[0][0], rb = s_rec[0][1];
    int4 lastq = make_int4(NEG, NEG, 0, 0);          // tops of the latest TOPS step, forwarded in registers
    int32_t lastk = -1;

    // recombination entry into the vertex of one step record (uniform): value, walk and source step
    auto eval_entry = [&](const int4 xa, const int4 xb, int32_t k, int32_t &E, int32_t &Eh, int32_t &Esrc) {
        const uint32_t b0 = (uint32_t)xa.z >> 8;
        if (((xa.x >> 8) & 0xFF) == 1 && b0 < RINGT) {
            // one in-edge (the usual case of a chain of bubbles): nothing to compare, and the tops of the latest TOPS
            // step are still in registers
            const int32_t src = k - (int32_t)b0;
            int32_t val, hh;
            tops_for_edge(src == lastk ? lastq : s_top[src & (RINGT - 1)], xa.z & 0xFF, val, hh);
            E = NEG; Eh = -1; Esrc = -1;
            if (hh >= 0) { E = val - A.cost; Eh = hh; Esrc = src; }
        } else {
            // tops older than the ring come from HBM: the producers wrote them at least RINGT - 2P steps ago.  (DP_ROW
            // writes none and never needs them: a block of steps is never longer than its ring, and no edge enters it
            // from before)
            dp_eval_entry<RINGT, MODE != DP_ROW>(xa, xb, k, s_top, A.k_in_packed, reinterpret_cast<const int4 *>(A.tops), A.cost, E, Eh, Esrc);
        }
        if (h == 0) s_ent[(k - k0) & (2 * P - 1)] = make_int2(Esrc, Eh);
    };

    for (int p = 0; p < n_per; p++) {
        const int32_t r_end = min(n_steps, (p + 1) * P);
        // The ring is guaranteed to hold this lane's next P events when a period begins, not one more: a lane that
        // consumed an event on every step of the last period peeked at a record the producers were still loading
        // (a stale slot: the lane then never saw its next event).  Peek again now that the barrier has passed.
        if (vi < ve) cA = s_ev[vi & (D - 1)][0][h];
        for (int32_t r = p * P; r < r_end;) {
            const int32_t k = k0 + r;
            // records of the next two steps (past the last step: stale records, never used)
            const int4 na = s_rec[(r + 1) & (2 * CK - 1)][0], nb = s_rec[(r + 1) & (2 * CK - 1)][1];
            const int4 n2a = s_rec[(r + 2) & (2 * CK - 1)][0], n2b = s_rec[(r + 2) & (2 * CK - 1)][1];
            // two alleles of one site (PHI_DP_PAIR: neither leaves states, no walk visits both): one iteration
            const bool pair = (ra.x & PHI_DP_PAIR) && r + 1 < r_end;
            const int32_t stepk = (int32_t)(cA.x & 0x7FFFFFFFu);    // (no event: 0xFFFFFFFF, a step no block reaches)
            const bool second = pair && stepk == k + 1;
            const bool active = stepk == k || second;
            const int32_t flags = second ? na.x : ra.x;

            // ---- recombination entry into this vertex (uniform per step)
            int32_t E = NEG, Eh = -1, Esrc = -1;
            if (ra.x & PHI_DP_NEED_ENTRY) eval_entry(ra, rb, k, E, Eh, Esrc);
            if (pair && (na.x & PHI_DP_NEED_ENTRY)) {
                int32_t E1, Eh1, Esrc1;
                eval_entry(na, nb, k + 1, E1, Eh1, Esrc1);
                if (second) { E = E1; Eh = Eh1; Esrc = Esrc1; }
            } else if (second) { E = NEG; Eh = -1; }

            int32_t dmax = NEG;
            int32_t oidx = 255;
            if (active) {
                const int sl = (int)(vi & (D - 1));
                const phi_ent_t e = cA.y;
                const bool ovf = (cA.x >> 31) != 0;
                const int32_t t = (int32_t)(e - eb);
                const int32_t End = (int32_t)cA.z, SB = (int32_t)cA.w;
                const uint8_t *gb = reinterpret_cast<const uint8_t *>(&s_ev[sl][1][h]);   // byte a of G at gb[(a & 15) + (a >> 4) * 1024]
                oidx = gb[15 + 1024];
                // runs older than 30 entries: one scalar
                while (qn > 0 && t - hs >= 31) {
                    const int32_t key = qn == 1 ? tk : s_qK[qh & (QD - 1)][h];
                    if (key > M) { M = key; sL = hs; }
                    qh++; qn--;
                    if (qn > 0) { hs = s_qs[qh & (QD - 1)][h]; hE = s_qE[qh & (QD - 1)][h]; }
                }
                // a run begins here: the walk start, or a recombination entry worth keeping
                int32_t newE = NEG;
                if (t == 0) { newE = starts_on ? 0 : NEG; qn = 0; M = NEGK; Emax = NEG; }
                else if ((flags & PHI_DP_NEED_ENTRY) && Eh >= 0) newE = E;
                if (newE > Emax) {
                    Emax = newE;
                    const int32_t key = newE - SB;
                    while (qn > 0 && tk < key) {
                        qn--;
                        if (qn > 0) tk = s_qK[(qh + qn - 1) & (QD - 1)][h];
                    }
                    if (QD < 32 && qn == QD) { atomicOr(A.err, PHI_KERR_DP_QUEUE); qn--; }   // result void: the caller takes DP_SEQ
                    const int slq = (qh + qn) & (QD - 1);
                    s_qs[slq][h] = t; s_qE[slq][h] = newE; s_qK[slq][h] = key;
                    if (qn == 0) { hs = t; hE = newE; }
                    tk = key;
                    qn++;
                    if (MODE == DP_ROW && key > Kn) Kn = key;
                }
                int32_t bs = 0;
                if ((flags & PHI_DP_NEED_TOPS) || e == e_last) {
                    // oldest first, strict improvement: ties keep the older run
                    int32_t best = M > NEGK / 2 ? M + End : NEG;
                    bs = sL;
                    for (int32_t j = 0; j < qn; j++) {
                        const int32_t s = j == 0 ? hs : s_qs[(qh + j) & (QD - 1)][h];
                        const int32_t Es = j == 0 ? hE : s_qE[(qh + j) & (QD - 1)][h];
                        const int a = t - s;
                        const int32_t inside = !ovf ? (int32_t)gb[(a & 15) + (a >> 4) * 1024] : ev_count_inside(A, (int64_t)eb + s, e);
                        const int32_t val = Es + inside;
                        if (val > best) { best = val; bs = s; }
                    }
                    if (best > NEG / 2) dmax = best; else bs = 0;
                    if (MODE == DP_ROW && e == e_last) endbest = max(endbest, dmax);
                }
                s_res[sl][h] = make_int4(dmax, bs, (int32_t)e, 0);
                vi++;
                cA = make_uint4(0xFFFFFFFFu, 0, 0, 0);
                if (vi < ve) cA = s_ev[vi & (D - 1)][0][h];
            }

            // ---- best states leaving this vertex (dp_dev.h); never for a pair
            if (!pair && (ra.x & PHI_DP_NEED_TOPS)) {
                const bool leaving = active && oidx != 255 && dmax > NEG / 2;
                DpTops t;
                if (__ballot(leaving && oidx > 1) == 0ull) {
                    // at most two out-edges in use (a bubble): best walk per edge, two independent reductions
                    const bool on0 = leaving && oidx == 0, on1 = leaving && oidx == 1;
                    unsigned long long K0, K1;
                    ev_wave_max2_key(on0 ? ev_key(dmax, h) : 0ull, on1 ? ev_key(dmax, h) : 0ull, K0, K1);
                    // top1: larger value, then the lower walk id (= the larger key); top2: the best on the other edge
                    const bool first0 = K0 >= K1;
                    const unsigned long long Kf = first0 ? K0 : K1, Ks = first0 ? K1 : K0;
                    t.t1v = Kf ? (int32_t)(uint32_t)(Kf >> 8) + NEG : NEG;
                    t.t1h = Kf ? 255 - (int32_t)(Kf & 255) : -1;
                    t.t1n = Kf ? (first0 ? 0 : 1) : -1;
                    t.t2v = Ks ? (int32_t)(uint32_t)(Ks >> 8) + NEG : NEG;
                    t.t2h = Ks ? 255 - (int32_t)(Ks & 255) : -1;
                } else {
                    t = dp_tops_wave(leaving, dmax, oidx);
                }
                lastq = pack_tops(t);
                lastk = k;
                if (h == 0) s_top[k & (RINGT - 1)] = lastq;
            }
            if (pair) { ra = n2a; rb = n2b; r += 2; }
            else { ra = na; rb = nb; r += 1; }
        }
        s_vi[(p + 1) & 1][h] = vi;
        __syncthreads();                             // B_{p+1}
    }
    if (MODE != DP_SEQ) {
        // what crosses the cut at the block's end: the best key of this walk's live runs (oldest first, ties keep the
        // older run) and where that run began
        int32_t best = M > NEGK / 2 ? M : NEGK, bs = sL;
        for (int32_t j = 0; j < qn; j++) {
            const int32_t key = s_qK[(qh + j) & (QD - 1)][h];
            if (key > best) { best = key; bs = s_qs[(qh + j) & (QD - 1)][h]; }
        }
        if (MODE == DP_ROW) {
            // (class lanes: the row's own column goes to an array of its own and leaves NEGK behind -- the chain then takes the
            //  other classes' maximum over the whole row without looking for the diagonal)
            const bool on_diag = A.rowdiag_out && h == row_j;
            if (on_diag) A.rowdiag_out[(int64_t)sb * 64 + h] = has_walk ? best : NEGK;
            A.row_out[(int64_t)blockIdx.x * 64 + h] = has_walk && !on_diag ? best : NEGK;
            const int32_t eb_all = wave_max_i32(endbest);
            if (h == 0) A.rowend_out[blockIdx.x] = eb_all;
            // what a walk of the unit lane's class other than the one that carries the key gets: the new runs of that lane
            if (A.rownew_out && h == row_j) A.rownew_out[blockIdx.x] = Kn;
            if (A.rownew_out && start_row && h == 0) A.rownew_out[blockIdx.x] = NEGK;
        } else {
            // (a walk with no event left when the block began carries nothing that is ever read: reported as "no run",
            //  as the row pass does)
            A.blk_keys_out[(int64_t)sb * A.lane_stride + h] = (has_walk && vb < ve) ? best : NEGK;
            A.blk_carry[(int64_t)sb * A.lane_stride + h] = bs;
        }
    }
}

// DP_PATH on walk lanes for more than 64 walks (blocks of at most 512 steps)
void phi_launch_dp_block_paths_wide(hipStream_t st, const PhiDpEventArgs &A)
{
    if (A.n_walks <= 128) hipLaunchKernelGGL((phi_dp_events_kernel<2, DP_PATH>), dim3((unsigned)A.n_blk), dim3(128), 0, st, A);
    else hipLaunchKernelGGL((phi_dp_events_kernel<4, DP_PATH>), dim3((unsigned)A.n_blk), dim3(256), 0, st, A);
}

void phi_launch_dp_events(hipStream_t st, const PhiDpEventArgs &A)
{
    if (A.n_walks <= 64) hipLaunchKernelGGL((phi_dp_events_pc_kernel<2, DP_SEQ, 8, RING, 32>), dim3(1), dim3(64 * 3), 0, st, A);
    else if (A.n_walks <= 128) hipLaunchKernelGGL((phi_dp_events_kernel<2, DP_SEQ>), dim3(1), dim3(128), 0, st, A);
    else hipLaunchKernelGGL((phi_dp_events_kernel<4, DP_SEQ>), dim3(1), dim3(256), 0, st, A);    // n_walks <= PHI_DP_EVENT_MAX_WALKS
}

// blocks of steps in parallel (<= 64 walks): the rows of the blocks' transfer matrices, then (the host has chained
// them into the entry vector of every block) the blocks themselves.  A block is at most as long as its ring of tops
// (A.blk_ring: 1024 steps, two workgroups per CU; 2048 for graphs whose longest stretch without a cut needs it).
void phi_launch_dp_block_rows(hipStream_t st, const PhiDpEventArgs &A)
{
    const unsigned grid = (unsigned)A.n_blk * (A.lane_walk ? 65u : (unsigned)(A.n_walks + 1));
    // (blocks of at most 256 steps: a ring of 256 tops and queues of 8 runs make a task 51 KB of LDS, three per CU
    //  instead of two -- the consumer wave is latency-bound, so throughput follows the number of resident tasks;
    //  the second pass keeps this layout, the rows go one step further:)
    // (a period of two steps instead of four halves the event ring and the result ring: 35 KB, FOUR tasks per CU; the extra
    //  barriers cost the consumer less than the fourth task gains -- C2 rows 2.8 -> 2.3 ms with their copy to the host)
    if (A.blk_ring <= 256 && A.blk_max_len > 0 && A.blk_max_len <= 64 && !getenv("PHI_DP_ROWS_LARGE"))
        hipLaunchKernelGGL((phi_dp_events_pc_kernel<2, DP_ROW, 2, 64, 8, 32>), dim3(grid), dim3(64 * 3), 0, st, A);
    else if (A.blk_ring <= 256) hipLaunchKernelGGL((phi_dp_events_pc_kernel<2, DP_ROW, 2, 256, 8>), dim3(grid), dim3(64 * 3), 0, st, A);
    else if (A.blk_ring <= 1024) hipLaunchKernelGGL((phi_dp_events_pc_kernel<2, DP_ROW, 4, 1024, 16>), dim3(grid), dim3(64 * 3), 0, st, A);
    else hipLaunchKernelGGL((phi_dp_events_pc_kernel<2, DP_ROW, 4, 2048, 16>), dim3(grid), dim3(64 * 3), 0, st, A);
}
void phi_launch_dp_block_paths(hipStream_t st, const PhiDpEventArgs &A)
{
    if (A.blk_ring <= 256) hipLaunchKernelGGL((phi_dp_events_pc_kernel<2, DP_PATH, 4, 256, 8>), dim3((unsigned)A.n_blk), dim3(64 * 3), 0, st, A);
    else if (A.blk_ring <= 1024) hipLaunchKernelGGL((phi_dp_events_pc_kernel<2, DP_PATH, 4, 1024, 16>), dim3((unsigned)A.n_blk), dim3(64 * 3), 0, st, A);
    else hipLaunchKernelGGL((phi_dp_events_pc_kernel<2, DP_PATH, 4, 2048, 16>), dim3((unsigned)A.n_blk), dim3(64 * 3), 0, st, A);
}

// One empty launch loads this translation unit's code object onto the device: the HIP runtime does that lazily, at the
// first launch of any of its kernels (0.5-1.3 ms per unit, measured inside phi_set_graph / phi_solve before
// phi_ctx_create did it up front).
__global__ void phi_warm_dp_events_kernel() {}
void phi_warm_dp_events(hipStream_t st) { hipLaunchKernelGGL(phi_warm_dp_events_kernel, dim3(1), dim3(64), 0, st); }
