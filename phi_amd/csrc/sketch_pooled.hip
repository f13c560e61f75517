// sketch_pooled.hip -- the POOLED instances of the read sketch kernel and their launcher, in a translation unit of their
// own: phi_amd/build.py compiles this file, and no other, with -mllvm -disable-machine-licm (see the note at
// phi_launch_sketch_pooled below).  The helpers come from sketch_dev.h; sketch.hip describes the phases.
#include "sketch_dev.h"

// The read kernel (PHI_MODE_PROBE) for batches of 12 Mbases and more, k <= 32 (phi_launch_sketch).
// Wave g of A.wave_stride takes the chunks g, g + stride, g + 2 stride, ... and hashes their items
// in rounds of 64 FULL lanes -- the items a round leaves over (fewer than 64) wait in one register pair per lane for the
// next chunk's.  A chunk of short reads yields ~40 items: hashed chunk by chunk (phi_sketch_kernel) the rounds run at 61 %
// of their lanes, and hash + probe are 38 % of that kernel's instructions.  Phases 0 - 3b of a chunk are
// those of phi_sketch_kernel (sketch_phases.inc).
template <bool WIDE, int KT, int WT>
__global__ void __launch_bounds__(TPB, 6) phi_sketch_pool_kernel(PhiSketchArgs A)   // (six waves per SIMD, at most 80 VGPRs)
{
    constexpr int MODE = PHI_MODE_PROBE;
    constexpr bool FUSED = true, NEED_POS = false, POOL = true;      // (names of the shared phases)
    constexpr bool FMIN = KT > 0 && KT <= 31;            // values < 2^62: minima by v_min_f64
    static_assert(KT >= 0, "k <= 32");
    extern __shared__ uint64_t s_dyn[];

    const int k = KT > 0 ? KT : A.k, w = WT ? WT : A.w;
    const int64_t N = A.n_bases;
    const int64_t n_chunks_all = (N + WCH - 1) / WCH;
    const int64_t stride = (int64_t)A.wave_stride;
    int mine;                                             // chunks of this wave (wave-uniform)
    {
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        const int64_t gw = (int64_t)blockIdx.x * (TPB / 64) + wid;      // this wave's job
        if (A.ipc_mb && gw == 0 && lane == 0)             // (a group of processes: see PhiSketchArgs)
            __hip_atomic_store(A.ipc_mb + PHI_MB_SCORED, A.ipc_scored, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (gw >= n_chunks_all || gw >= stride) {         // wave-uniform
            // read batches, first launch after a reset: this wave's share of the buffers the previous generation of
            // reads filled (stores into buffers nothing in this launch reads: no ordering needed)
            if (A.q_clean) clean_finish(A, gw, (int64_t)gridDim.x * (TPB / 64), lane);
            return;
        }
        mine = __builtin_amdgcn_readfirstlane((int)((n_chunks_all - gw + stride - 1) / stride));
    }
    const uint64_t kmask = phi_kmask(k);
    const int M = WCH + w;                                // canonical values m[l], l -> k-mer c0-1+l
    const int span = w + k - 1;                           // bases under one window
    const bool have_bad = true;

    using MetaT = uint16_t;
    constexpr uint32_t ITEM_FIRST = 1u << 15;            // the first window of its sequence
    constexpr uint32_t ITEM_NOEMIT = 1u << 14;           // only its hash is needed (the window before a candidate)
    int n_emit = 0, n_log = 0, n_nov_slow = 0;
    // the items waiting for a full round -- lane j < pend holds item j: its minimum and its flags (for k <= 31 in
    // the two bits a value leaves free) -- and the hash of the last item hashed
    uint64_t pv = 0;
    uint32_t pf = 0;
    int pend = 0;
    uint64_t carry = PHI_EMPTY_KEY;

    // the 16 bases of this lane in the NEXT chunk, loaded a turn ahead
    uint4 xn = load_bases16(A.ascii, N, ((int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6)) * WCH, (int)(threadIdx.x & 63));
    // (one more turn after the wave's last chunk, for the round of the items still waiting -- so that the code of a round
    //  exists once)
    for (int ci = 0; ci <= mine; ci++) {
    // (what depends on the lane is worked out again in every turn -- the compiler would otherwise keep all of it, addresses,
    //  masks, the chunk's 64-bit position, in registers across the loop: 106 VGPRs in scratch at the 80-register bound;
    //  for the same reason this file is compiled with machine LICM off, see phi_launch_sketch_pooled)
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    // (the wave's index as a scalar: the chunk's position and the wave's LDS region are scalar arithmetic)
    const int lane = (int)(tid & 63u), wid = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int64_t gw = (int64_t)blockIdx.x * (TPB / 64) + wid;
    const int64_t chunk = gw + ci * stride;
    const int64_t c0 = chunk * WCH;                       // first window start of this chunk
    int ncand = 0;
    bool chunk_bad = false;
    int64_t out_base = 0;                                 // (a name of the shared phases: the ordered write of the walks)
    (void)out_base;
    uint64_t *s_mp = s_dyn + (size_t)wid * phi_wave_region_u64(w, k, NEED_POS);   // k-mers; later the window minima
    uint64_t *s_words = s_mp + phi_wave_mp_u64(w);
    unsigned long long *s_bits = (unsigned long long *)(s_words + SWW);
    unsigned long long *s_bad = s_bits + SBW;
    MetaT *s_meta = (MetaT *)(s_bad + SBW);               // WCH + 1 items + 8 trash slots
    uint64_t *s_q = s_mp + lane * (Q + 1);                // SM(lane * Q + x) == s_q[x + (x >> 3)]
    if (ci) wave_sync();                                  // the rounds of the chunk before have read its items
    if (ci < mine) {
#include "sketch_phases.inc"

#if PHI_ABL == 15
    { asm volatile("" :: "v"(ncand)); return; }
#endif
#if PHI_ABL == 2
    ncand = 0;
#endif
    }   // phases 0 - 3b of a chunk
    // ---- phases 4 + 5: items on dense lanes, 64 per round: murmur3 of the item's minimum, the hash-change test against
    //      the item before it (the lane below; lane 0 takes the last lane of the round before), table probes
    {
        // items of this chunk: 0 .. ncand (none when it has no candidate, none in the last turn).  Full rounds while there
        // are 64 items between the waiting ones and these; what is left joins (or becomes) the waiting ones; the last
        // turn's round takes the waiting ones as they are
        const int n_items = ncand > 0 ? ncand + 1 : 0;
        const bool flush = ci == mine;
        int taken = 0;
        while (pend + (n_items - taken) >= 64 || (flush && pend > 0)) {
            uint64_t v = pv;
            uint32_t f = pf;
            if (lane >= pend && !flush) {
                const uint32_t meta = s_meta[taken + lane - pend];
                v = SM((int)(meta & 0x3FFu));
                f = meta >> 14;                           // ITEM_FIRST, ITEM_NOEMIT: bits 15, 14 of a 16-bit item
                if (FMIN) v |= (uint64_t)f << 62;
            }
            const bool valid = !flush || lane < pend;
            taken += 64 - pend;
            pend = 0;
            // one round: hash, hash-change test against the item before, probes, slot log
            const uint64_t h = phi_kmer_hash(FMIN ? (v & 0x3FFFFFFFFFFFFFFFull) : v, k);
            const uint32_t flg = FMIN ? (uint32_t)(v >> 62) : f;              // bit 1: first window of its sequence, bit 0: only its hash is needed
            const uint64_t hp = wave_prev_u64(h, carry, lane);
            carry = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(h >> 32), 63) << 32) |
                    (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)h, 63);
            const bool emit = valid && !(flg & 1u) && ((flg & 2u) || h != hp);
            const unsigned long long bal = __ballot(emit);
            bool novel = false;
            const KArgs R = kargs_now();
#if PHI_ABL == 5
            asm volatile("" :: "v"(h));                   // (experiment: hash, no probe)
#else
            if (emit) {
                const ProbeArgs P{R->u_rt, R->u_bmask, R->hit, R->err};
                novel = probe_table(P, h);
            }
#endif
            // the round's novel hashes, appended to the wave's log in lane order (coalesced): the log entries of the wave's
            // chunks, one after the other -- entry pos of the wave is entry pos % cap of its chunk number pos / cap
            const unsigned long long ib = __ballot(novel);
            const int pos = n_log + __popcll(ib & ((1ull << lane) - 1));
            const int sh = R->nov_shift, room = mine << sh;
            if (novel && pos < room) R->nov_log[((R->log_base + gw + (int64_t)(pos >> sh) * stride) << sh) + (pos & ((1 << sh) - 1))] = h;
            n_log += __popcll(ib);
            if (n_log > room) {                           // (wave-uniform, rare) past the wave's log: the overflow list
                const OverflowArgs O{R->ov_list, R->ov_count, R->ov_cap, R->err};
                overflow_novel(O, novel && pos >= room, h, lane);
            }
            n_emit += __popcll(bal);
        }
        const int rem = flush ? 0 : n_items - taken;      // < 64 - pend
        if (lane >= pend && lane < pend + rem) {
            const uint32_t meta = s_meta[taken + lane - pend];
            pv = SM((int)(meta & 0x3FFu));
            pf = meta >> 14;
            if (FMIN) pv |= (uint64_t)pf << 62;
        }
        pend += rem;
    }

    if (chunk_bad) {
        // (rare) windows over a base outside ACGTacgt, or right after one: the exact byte-wise routine, by the wave
        // that owns the chunk (its novel hashes go to the overflow list)
        int n_emit_slow = 0;
        slow_windows<MODE>(A, c0, chunk, lane, k, w, s_bits, s_bad, false, 0, n_emit_slow, n_nov_slow);
        n_emit += n_emit_slow;
    }
    }   // chunks of this wave
    uint32_t tid_end = threadIdx.x;
    asm volatile("" : "+v"(tid_end));                     // (worked out again: not kept from the wave's start in two registers)
    const int lane = (int)(tid_end & 63u);
    const int64_t gw = (int64_t)blockIdx.x * (TPB / 64) + __builtin_amdgcn_readfirstlane((int)(tid_end >> 6));
    {
        // (the arguments of this part are loaded now, not kept in scalar registers through the loop)
        const KArgs R = kargs_now();
        if (R->q_clean) clean_finish(*R, gw, (int64_t)gridDim.x * (TPB / 64), lane);
        {
            // entries of the log: 1 << nov_shift per chunk of this wave, filled in order
            const int sh = R->nov_shift, cap = 1 << sh;
            for (int j = lane; j < mine; j += 64) {
                const int left = n_log - (j << sh);
                R->nov_cnt[R->log_base + gw + j * stride] = (uint16_t)(left < 0 ? 0 : left < cap ? left : cap);
            }
        }
        // one atomic per wave for the number of novel hashes logged (n_log counts them: wave-uniform) and emitted records
        const int n_nov_wave = n_log + n_nov_slow;
        if (lane == 0) {
            const int stripe = (int)(gw & (PHI_STRIPES - 1)) * 8;
            if (n_nov_wave && R->n_logged) atomicAdd(R->n_logged + stripe, (unsigned long long)n_nov_wave);
            if (n_emit && R->n_emitted) atomicAdd(R->n_emitted + stripe, (unsigned long long)n_emit);
        }
    }
}

// This translation unit is compiled with machine LICM off: the POOLED instances are alone in it because
// their loop over a wave's chunks runs at the 80-register bound of six waves per SIMD, and constants and addresses hoisted
// out of it stay in registers through every turn (106 VGPRs in scratch).  The one-chunk instances keep the default.
void phi_launch_sketch_pooled(hipStream_t st, unsigned nb, size_t lds, const PhiSketchArgs &A, hipEvent_t t0, hipEvent_t t1)
{
    if (A.k == 31 && A.w == 25) hipExtLaunchKernelGGL((phi_sketch_pool_kernel<true, 31, 25>), dim3(nb), dim3(TPB), lds, st, t0, t1, 0, A);
    else if (A.w > Q) hipExtLaunchKernelGGL((phi_sketch_pool_kernel<true, 0, 0>), dim3(nb), dim3(TPB), lds, st, t0, t1, 0, A);
    else hipExtLaunchKernelGGL((phi_sketch_pool_kernel<false, 0, 0>), dim3(nb), dim3(TPB), lds, st, t0, t1, 0, A);
}
