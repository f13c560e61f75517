// sketch.hip -- packing and (w,k)-minimiser sketch kernels for gfx950.
//
// Replaces the per-position std::string loops of the reference:
//   ILP_index::compute_hashes  src/ILP_index.cpp:447-493  (reads)
//   ILP_index::index_kmers     src/ILP_index.cpp:359-445  (haplotype walks, minus the vertex map)
// Semantics reproduced bit for bit: upper-casing, canonical k-mer =
// min(fwd, revcomp) in string order, window minimum with the rightmost tie, one record per
// window whose minimum hashes differently from the previous window's (prev_hash starts at
// UINT64_MAX per sequence), MurmurHash3_x64_128 seed 0 folded h1^h2.
//
// One flat base space holds all sequences of a batch back to back; a bitmap marks sequence
// starts.  A window is live iff no sequence starts inside it.  Every WAVE owns PHI_WCH consecutive
// window positions and never waits for another wave (no workgroup barrier):
//   phase 0  stage the chunk's packed words and bitmaps into LDS (the only global reads)
//   phase 1  canonical k-mers of the chunk (rolling 2-bit arithmetic)      -> LDS
//   phase 2  sliding-window minima, Q+1 consecutive windows per lane from a
//            suffix-min / core / prefix-min split (w+Q LDS reads per lane)
//   phase 3  candidate windows (minimum changed, or first window of a sequence), compacted
//            into LDS with a wave scan so that the hash runs on dense lanes only
//   phase 4  murmur3 of each candidate, hash-change test against its predecessor
//   phase 5  ballot/prefix-sum compaction of the emitted records and, by mode,
//            count | ordered write | table probe + coalesced log of the read hashes that are not walk minimisers
//
// Bases outside ACGTacgt (the reference keeps them as bytes: N sorts between G and T and is its
// own complement, ILP_index.cpp:350-353) cannot live in 2 bits.  The pack kernels set one bit per
// such base; the 2-bit path skips every window that, together with its predecessor, touches a
// marked base, and an exact byte-wise kernel (phi_sketch_bytes_kernel, launched after the 2-bit
// kernel; it leaves at once when the batch holds no such base) handles exactly those windows.
// With `allslow` the byte-wise kernel handles every window (ordered write of walks that contain
// such bases).
//
// This unit holds the pack, one-chunk, window-space and byte-wise kernels and every launcher.  Two read kernels are
// translation units of their own: the pooled one (sketch_pooled.hip, built with other flags) and the fixed-geometry
// window one (sketch_win_fixed.hip).  Constants, LDS geometry and the device routines all three share: sketch_dev.h.
#include "sketch_dev.h"

__global__ void __launch_bounds__(256) phi_pack_ascii_kernel(const uint8_t *__restrict__ bases, int64_t n,
                                                             uint64_t *__restrict__ words, int64_t n_words,
                                                             uint32_t *__restrict__ badbits,
                                                             unsigned long long *__restrict__ n_bad)
{
    pack_ascii_word((int64_t)blockIdx.x * blockDim.x + threadIdx.x, bases, n, words, n_words, badbits, n_bad);
}

// starts bitmap: bit (p & 63) of word p >> 6 set iff a sequence starts at base p.
__global__ void phi_mark_starts_kernel(const int64_t *__restrict__ seq_off, int64_t n_seq,
                                       unsigned long long *__restrict__ starts)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_seq) return;
    const int64_t p = seq_off[i];
    if (seq_off[i + 1] > p)                 // empty sequences own no base
        atomicOr(&starts[p >> 6], 1ull << (p & 63));
}

// one launch that forgets all reads: zero hit vector, zero striped counters (only when two resets follow each other with
// no read launch in between: otherwise the waves of the next read launch do it, see clean_finish)
__global__ void __launch_bounds__(256) phi_reset_reads_kernel(uint64_t *__restrict__ hit_words, int64_t n_hit_words,
                                                              uint64_t *__restrict__ stripes, int64_t n_stripe_words)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = t; i < n_hit_words; i += stride) hit_words[i] = 0;
    for (int64_t i = t; i < n_stripe_words; i += stride) stripes[i] = 0;
}

// WIDE: w > Q (windows of one lane overlap in a common core); otherwise brute force per window.
// KT/WT: compile-time k and w of the specialised instance (0 = take them from the arguments).
template <int MODE, bool WIDE, int KT, int WT>
__global__ void __launch_bounds__(TPB, MODE == PHI_MODE_PROBE ? 6 : 1) phi_sketch_kernel(PhiSketchArgs A)   // (reads: six waves per SIMD, at most 80 VGPRs)
{
    constexpr bool FUSED = MODE == PHI_MODE_PROBE;      // read batches come as ASCII + read offsets (see phase 0)
    constexpr bool NEED_POS = MODE == PHI_MODE_WRITE;   // only the ordered write stores positions (ILP_index.cpp:423)
    constexpr bool FMIN = !NEED_POS && KT > 0 && KT <= 31;   // values < 2^62: minima by v_min_f64
    extern __shared__ uint64_t s_dyn[];

    // (wid stays a vector register: as a scalar -- readfirstlane -- the values derived from it overflow the SGPR file,
    //  +9 % VALU instructions of v_writelane / v_readlane traffic; reading the output phase's arguments late, through
    //  a laundered kernarg pointer, frees the SGPRs but pushes four VGPRs into scratch at the 80-register bound: -35 %)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int k = KT > 0 ? KT : A.k, w = WT ? WT : A.w;       // (KT = -1: the instantiation for k > 32, see below)
    const int64_t N = A.n_bases;
    const int64_t chunk = (int64_t)blockIdx.x * (TPB / 64) + wid;
    const int64_t c0 = chunk * WCH;                       // first window start of this chunk
    if (FUSED && A.ipc_mb && chunk == 0 && lane == 0)      // (a group of processes: see PhiSketchArgs)
        __hip_atomic_store(A.ipc_mb + PHI_MB_SCORED, A.ipc_scored, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    if (c0 >= N) {                                        // wave-uniform
        // read batches, first launch after a reset: this wave's share of the buffers the previous generation of
        // reads filled (stores into buffers nothing in this launch reads: no ordering needed)
        if (FUSED && A.q_clean) clean_finish(A, chunk, (int64_t)gridDim.x * (TPB / 64), lane);
        return;
    }
    const uint64_t kmask = phi_kmask(k);
    const int M = WCH + w;                                // canonical values m[l], l -> k-mer c0-1+l
    const int span = w + k - 1;                           // bases under one window
    const bool have_bad = FUSED || A.badbits != nullptr;

    using MetaT = typename std::conditional<NEED_POS, uint32_t, uint16_t>::type;
    constexpr uint32_t ITEM_FIRST = NEED_POS ? 1u << 31 : 1u << 15;        // the first window of its sequence
    constexpr uint32_t ITEM_NOEMIT = NEED_POS ? 1u << 30 : 1u << 14;       // only its hash is needed (the window before a candidate)
    uint64_t *s_mp = s_dyn + (size_t)wid * phi_wave_region_u64(w, k, NEED_POS);   // k-mers; later the window minima
    uint64_t *s_words = s_mp + phi_wave_mp_u64(w);
    unsigned long long *s_bits = (unsigned long long *)(s_words + SWW);
    unsigned long long *s_bad = s_bits + SBW;
    MetaT *s_meta = (MetaT *)(s_bad + SBW);               // WCH + 1 items + 8 trash slots
    uint64_t *s_q = s_mp + lane * (Q + 1);                // SM(lane * Q + x) == s_q[x + (x >> 3)]

    // (names the shared phases use; the last four only matter in the pooled kernel)
    constexpr bool POOL = false;
    bool chunk_bad = false;
    int ncand = 0, n_emit = 0, n_log = 0, n_nov_slow = 0;
    int64_t out_base = 0;
    uint4 xn = make_uint4(0, 0, 0, 0);
    const int ci = 0, mine = 1;
    const int64_t stride = 0;
#include "sketch_phases.inc"

#if PHI_ABL == 15
    { asm volatile("" :: "v"(ncand)); return; }
#endif
    // ---- phases 4 + 5: items on dense lanes, 64 per round: murmur3 of the item's minimum, the
    //      hash-change test against the item before it (the lane below; lane 0 takes the last lane of
    //      the round before), ordered compaction, output
#if PHI_ABL == 2
    ncand = 0;
#endif
#include "sketch_rounds.inc"

    if (FUSED && chunk_bad) {
        // (rare) windows over a base outside ACGTacgt, or right after one: the exact byte-wise routine, by the wave
        // that owns the chunk (its novel hashes go to the overflow list)
        int n_emit_slow = 0;
        slow_windows<MODE>(A, c0, chunk, lane, k, w, s_bits, s_bad, false, 0, n_emit_slow, n_nov_slow);
        n_emit += n_emit_slow;
    }
    if (FUSED && A.q_clean) clean_finish(A, chunk, (int64_t)gridDim.x * (TPB / 64), lane);
    if (MODE == PHI_MODE_COUNT) {
        if (lane == 0) A.block_cnt[chunk] = n_emit;
    } else if (MODE == PHI_MODE_PROBE) {
        // one atomic per wave for the number of novel hashes logged (n_log counts them: wave-uniform; an upper bound of what
        // the set will grow by) and of emitted records
        if (lane == 0) {
            const int cap = 1 << A.nov_shift;
            A.nov_cnt[A.log_base + chunk] = (uint16_t)(n_log < cap ? n_log : cap);
            const int n_nov_wave = n_log + n_nov_slow;
            const int stripe = (int)(chunk & (PHI_STRIPES - 1)) * 8;
            if (n_nov_wave && A.n_logged) atomicAdd(A.n_logged + stripe, (unsigned long long)n_nov_wave);
            if (n_emit && A.n_emitted) atomicAdd(A.n_emitted + stripe, (unsigned long long)n_emit);
        }
    }
}

// The read kernel for batches of ONE read length, in window space: R = A.win_reads whole reads per wave.  Its geometry and
// its LDS layout are described in sketch_dev.h (phi_win_mp_u64), with the routines it shares with sketch_win_fixed.hip.
template <bool WIDE, int KT, int WT>
__global__ void __launch_bounds__(TPB, 7) phi_sketch_win_kernel(PhiSketchArgs A)   // (seven waves per SIMD, at most 72 VGPRs)
{
    constexpr int MODE = PHI_MODE_PROBE;
    constexpr bool NEED_POS = false;                     // (names of the shared phases)
    constexpr bool FMIN = KT > 0 && KT <= 31;            // values < 2^62: minima by v_min_f64
    static_assert(KT >= 0, "k <= 32");
    extern __shared__ uint64_t s_dyn[];

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int k = KT > 0 ? KT : A.k, w = WT ? WT : A.w;
    const int64_t N = A.n_bases;
    const int L = A.uniform_len, span = w + k - 1, V = L - span + 1;
    const int G = (V + Q - 1) / Q, s = G + (w + Q - 1) / Q, R = A.win_reads;
    const int64_t chunk = (int64_t)blockIdx.x * (TPB / 64) + wid;     // this wave's reads: chunk * R .. + R - 1
    const int64_t rd0 = chunk * R;
    if (A.ipc_mb && chunk == 0 && lane == 0)               // (a group of processes: see PhiSketchArgs)
        __hip_atomic_store(A.ipc_mb + PHI_MB_SCORED, A.ipc_scored, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    if (rd0 >= A.n_reads) {                                // wave-uniform
        if (A.q_clean) clean_finish(A, chunk, (int64_t)gridDim.x * (TPB / 64), lane);
        return;
    }
    const int nr = A.n_reads - rd0 < R ? (int)(A.n_reads - rd0) : R;   // reads of this wave
    const uint64_t kmask = phi_kmask(k);
    // staging origin: the 32-base word holding the wave's first base.  Local base lb <-> base c0-32+lb, local bit lp <->
    // base c0-64+lp, as in base space; R L <= 928 (phi_sketch_win_reads) keeps every word and bit a lane reads staged
    const int64_t c0 = (rd0 * (int64_t)L) & ~(int64_t)31;
    // this lane's read and lane group: rl = lane / G (exact in single precision for lane < 64), j = lane % G
    const int rl = (int)(((float)lane + 0.5f) * (1.0f / (float)G)), j = lane - rl * G;
    const bool live = rl < nr;

    using MetaT = uint16_t;
    constexpr uint32_t ITEM_FIRST = 1u << 15;            // the first window of its read
    constexpr uint32_t ITEM_NOEMIT = 1u << 14;           // only its hash is needed (the window before a candidate)
    uint64_t *s_mp = s_dyn + (size_t)wid * phi_win_region_u64(R, s, w, k);   // k-mers; later the window minima and the items
    uint64_t *s_words = s_mp;                             // staged words: until phase 1 has taken its extracts
    unsigned long long *s_bad = (unsigned long long *)s_mp;   // bitmap (chunk_bad only): staged where the region is dead
    MetaT *s_meta = (MetaT *)(s_mp + 9 * (64 + 1));      // items: behind the minima
    uint64_t *s_q = s_mp + (live ? 9 * (rl * s + j) : 0);   // k-mer 8j - 1 + x of the lane's read: s_q[x + (x >> 3)]

    // ---- phase 0: lane -> the 16 bases c0 - 32 + 16 lane .. + 15: one 32-bit half of a packed word + 16 flags of bases
    //      outside ACGTacgt (the text of sketch_phases.inc, phase 0); the flags only decide chunk_bad here (stage_bad_bits)
    bool chunk_bad;
    {
        const uint4 v = load_bases16<1>(A.ascii, N, c0, lane);
        const uint32_t x[4] = {v.x, v.y, v.z, v.w};
        uint32_t code = 0, bad = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t t = ((x[q] >> 1) ^ (x[q] >> 2)) & 0x03030303u;
            const uint32_t c8 = (t * 0x40100401u) >> 24;
            code = (code << 8) | c8;
            if (__builtin_amdgcn_perm(0x54474341u, 0x54474341u, t) != (x[q] & 0xDFDFDFDFu)) {
#pragma unroll
                for (int b = 0; b < 4; b++) bad |= (uint32_t)(!phi_is_acgt((x[q] >> (8 * b)) & 0xFFu)) << (4 * q + b);
            }
        }
        reinterpret_cast<uint32_t *>(s_words)[lane ^ 1] = code;
        chunk_bad = __ballot(lane < 62 && bad != 0) != 0ull;   // wave-uniform
    }
    wave_sync();

    // ---- phase 1: the read's L - k + 1 canonical k-mers, P consecutive per lane of its group.  Every lane takes its two
    //      extracts of the staged words first: the k-mers go over them
    {
        int n = 0, u = 0;
        uint64_t F = 0, Rc = 0, nxt = 0;
        if (live) {
            const int n_km = L - k + 1, P = (n_km + G - 1) / G;
            const int t0 = j * P;
            n = n_km - t0 < P ? n_km - t0 : P;
            if (n > 0) {
                const int lb = (int)((rd0 + rl) * (int64_t)L + t0 - c0) + 32;
                F = lds_extract64(s_words, lb) >> (64 - 2 * k);
                nxt = lds_extract64(s_words, lb + k);                 // the bases after the first k-mer
                u = 8 * s * rl + 1 + t0;                               // slot of k-mer t0
            }
        }
        wave_sync();
        if (n > 0) {
            Rc = phi_revcomp(F, k);
            for (int i = 0; i < n; i++, u++) {
                if (i) {
                    const uint64_t b = nxt >> 62;
                    nxt <<= 2;
                    F = ((F << 2) | b) & kmask;
                    Rc = (Rc >> 2) | ((3 - b) << (2 * k - 2));
                }
                s_mp[u + (u >> 3)] = FMIN ? min_u62(F, Rc) : (F < Rc ? F : Rc);
            }
        }
    }
    wave_sync();

    // ---- phase 2: minima of the lane's windows 8j - 1 .. 8j + 7 of its read (k-mers 8j - 1 .. 8j + 6 + w)
#include "sketch_minima.inc"

    // ---- phase 3: candidate windows i = 1..Q of this lane (window 8j + i - 1 of its read)
    if (chunk_bad) {                                      // (wave-uniform, rare) every lane has read its k-mers: the bitmap over them
        wave_sync();
        stage_bad_bits(A.ascii, N, c0, lane, s_bad);
        wave_sync();
    }
    uint32_t cflag = 0, fflag = 0, pflag = 0;             // candidates; first windows; candidates that carry their predecessor
    if (live) {
        const int imax = V - Q * j < Q ? V - Q * j : Q;   // windows i <= imax exist
        const uint32_t in_read = (2u << imax) - 2u;        // bits 1 .. imax
        const uint32_t first = j == 0 ? 2u : 0u;           // window 0 of the read
        uint32_t changed = 0;
#pragma unroll
        for (int i = 1; i <= Q; i++) changed |= (uint32_t)(wv[i] != wv[i - 1]) << i;
        // bit i of `dall`: a base outside ACGT under window i or its predecessor (bases a-1 .. a+span-1; for a read's first
        // window a-1 is the last base of the read before, as in base space): such windows take the byte-wise routine, and
        // the first window after a stretch of them carries its own predecessor
        uint32_t dall = 0, reseed = 0;
        if (chunk_bad) {
            const int lp0 = (int)((rd0 + rl) * (int64_t)L + Q * j - 1 - (c0 - 64));   // local bit of window 0's base
            for (int i = 0; i <= Q; i++) dall |= (uint32_t)range_has_bit(s_bad, lp0 + i - 1, lp0 + i + span - 1) << i;
            reseed = ~dall & (dall << 1);
        }
        cflag = in_read & ~dall & (first | changed | reseed);
        fflag = cflag & first;
        pflag = cflag & reseed & ~first;
    }
    // wave prefix sum of the per-lane candidate counts
    int ncand, coff;
    {
        const int cnt = __popc(cflag) + __popc(pflag);
        const int v = wave_scan_inclusive(cnt);
        ncand = __builtin_amdgcn_readlane(v, 63);
        coff = v - cnt;
    }
    wave_sync();                                          // every lane has read its k-mers
    {
        // the minimum of window i of lane goes to SM(lane * Q + i) -- the layout of base space
        uint64_t *s_w = s_mp + 9 * lane;
#define SW(x) s_w[(x) + ((x) >> 3)]
        if (lane == 0) SW(0) = wv[0];
#pragma unroll
        for (int i = 1; i <= Q; i++) SW(i) = wv[i];
#undef SW
        int c = coff + 1;
        if (!chunk_bad) {
            for (uint32_t f = cflag; f; f &= f - 1) {
                const uint32_t i = (uint32_t)__ffs((int)f) - 1;
                s_meta[c++] = (MetaT)((uint32_t)(lane * Q) + i + (((fflag >> i) & 1u) ? ITEM_FIRST : 0u));
            }
        } else {
#pragma unroll
            for (int i = 1; i <= Q; i++) {
                if ((cflag >> i) & 1u) {
                    if ((pflag >> i) & 1u) s_meta[c++] = (MetaT)((uint32_t)(lane * Q + i - 1) | ITEM_NOEMIT);
                    s_meta[c++] = (MetaT)((uint32_t)(lane * Q + i) | (((fflag >> i) & 1u) ? ITEM_FIRST : 0u));
                }
            }
        }
        if (coff == 0 && cflag) s_meta[0] = (MetaT)((uint32_t)(lane * Q + __ffs((int)cflag) - 2) | ITEM_NOEMIT);
    }
    wave_sync();
#undef SQ

    // ---- phases 4 + 5, as in base space
    int n_emit = 0, n_log = 0, n_nov_slow = 0;
    const int64_t out_base = 0;
#include "sketch_rounds.inc"

    if (chunk_bad) {
        // (the wave's region from a scalar: its vector address would be one register too many around the byte-wise routine)
        unsigned long long *s_bad_s = (unsigned long long *)(s_dyn + (size_t)__builtin_amdgcn_readfirstlane(wid) * phi_win_region_u64(R, s, w, k));
        wave_sync();                                      // the rounds have read the minima and the items: the bitmap over them
        stage_bad_bits(A.ascii, N, c0, lane, s_bad_s);
        wave_sync();
        int n_emit_slow = 0;
        slow_windows_reads(A, rd0, nr, L, V, c0, lane, k, w, s_bad_s, n_emit_slow, n_nov_slow);
        n_emit += n_emit_slow;
    }
    {
        // (the arguments of the epilogue are loaded now, not kept in scalar registers from the start: seven waves per SIMD
        //  leave 94 of them, and each one too many is a v_writelane / v_readlane pair in a lane of a vector register)
        const KArgs P = kargs_now();
        if (P->q_clean) clean_finish(*P, chunk, (int64_t)gridDim.x * (TPB / 64), lane);
        if (lane == 0) {
            const int cap = 1 << P->nov_shift;
            P->nov_cnt[P->log_base + chunk] = (uint16_t)(n_log < cap ? n_log : cap);
            const int n_nov_wave = n_log + n_nov_slow;
            const int stripe = (int)(chunk & (PHI_STRIPES - 1)) * 8;
            if (n_nov_wave && P->n_logged) atomicAdd(P->n_logged + stripe, (unsigned long long)n_nov_wave);
            if (n_emit && P->n_emitted) atomicAdd(P->n_emitted + stripe, (unsigned long long)n_emit);
        }
    }
}

void phi_launch_sketch_pooled(hipStream_t st, unsigned nb, size_t lds, const PhiSketchArgs &A, hipEvent_t t0, hipEvent_t t1);   // sketch_pooled.hip
bool phi_launch_sketch_win_fixed(hipStream_t st, unsigned nb, size_t lds, const PhiSketchArgs &A, hipEvent_t t0, hipEvent_t t1);   // sketch_win_fixed.hip

// Exact byte-wise kernel: every wave walks chunks in a grid-stride loop.
//   allslow = 0 (reads): launched after the 2-bit kernel with a small grid; leaves at once when the
//                        batch holds no base outside ACGT (*batch_bad == 0), else handles the windows
//                        the 2-bit kernel skipped;
//   allslow = 1        : every window (count / ordered write of sequences with such bases).
template <int MODE>
__global__ void __launch_bounds__(TPB) phi_sketch_bytes_kernel(PhiSketchArgs A, const unsigned long long *batch_bad)
{
    __shared__ unsigned long long s_all[(TPB / 64) * 2 * SBW];
    bytes_role<MODE>(A, batch_bad, blockIdx.x, gridDim.x, s_all);
}

// ---------------------------------------------------------------------------------- launchers

void phi_launch_pack_ascii(hipStream_t st, const uint8_t *bases, int64_t n, uint64_t *words, int64_t n_words,
                           uint32_t *badbits, unsigned long long *n_bad)
{
    if (n_words <= 0) return;
    const int64_t nb = (n_words + 4 + 255) / 256;
    hipLaunchKernelGGL(phi_pack_ascii_kernel, dim3((unsigned)nb), dim3(256), 0, st, bases, n, words, n_words, badbits,
                       n_bad);
}

void phi_launch_mark_starts(hipStream_t st, const int64_t *seq_off, int64_t n_seq, unsigned long long *starts)
{
    if (n_seq <= 0) return;
    const int64_t nb = (n_seq + 255) / 256;
    hipLaunchKernelGGL(phi_mark_starts_kernel, dim3((unsigned)nb), dim3(256), 0, st, seq_off, n_seq, starts);
}

void phi_launch_sketch_bytes(hipStream_t st, int mode, const PhiSketchArgs &A, const unsigned long long *batch_bad)
{
    const int64_t nchunks = phi_sketch_num_blocks(A.n_bases);
    if (nchunks <= 0) return;
    int64_t nb = (nchunks + TPB / 64 - 1) / (TPB / 64);
    if (!A.allslow && nb > 1024) nb = 1024;           // usually leaves at once: keep the launch small
    // (count / ordered write of sequences with bases outside ACGT; the read kernel does such windows itself)
    if (mode == PHI_MODE_COUNT)
        hipLaunchKernelGGL(phi_sketch_bytes_kernel<PHI_MODE_COUNT>, dim3((unsigned)nb), dim3(TPB), 0, st, A, batch_bad);
    else
        hipLaunchKernelGGL(phi_sketch_bytes_kernel<PHI_MODE_WRITE>, dim3((unsigned)nb), dim3(TPB), 0, st, A, batch_bad);
}

void phi_launch_reset_reads(hipStream_t st, uint64_t *hit_words, int64_t n_hit_words, uint64_t *stripes, int64_t n_stripe_words)
{
    int64_t n = n_hit_words > n_stripe_words ? n_hit_words : n_stripe_words;
    int64_t nb = (n + 255) / 256;
    if (nb > 2048) nb = 2048;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(phi_reset_reads_kernel, dim3((unsigned)nb), dim3(256), 0, st, hit_words, n_hit_words, stripes, n_stripe_words);
}

// number of per-wave chunks (= entries of block_cnt / block_off)
int64_t phi_sketch_num_blocks(int64_t n_bases) { return n_bases <= 0 ? 0 : (n_bases + WCH - 1) / WCH; }

// t0 / t1 (optional): events that take the kernel's own start / end timestamps (hipExtLaunchKernelGGL:
// no extra marker packets on the stream, unlike hipEventRecord around the launch)
template <int MODE>
static void launch_sketch_mode(hipStream_t st, unsigned nb, size_t lds, const PhiSketchArgs &A, hipEvent_t t0, hipEvent_t t1, bool pooled)
{
    // the reference's defaults (options.cpp:7-8) get a fully unrolled instance, except for the
    // ordered write whose position tracking would push it past 128 VGPRs
    if constexpr (MODE == PHI_MODE_PROBE) {
        if (pooled) { phi_launch_sketch_pooled(st, nb, lds, A, t0, t1); return; }      // (k <= 32: see phi_launch_sketch)
    }
    if constexpr (MODE != PHI_MODE_WRITE) {
        if (A.k == 31 && A.w == 25) {
            hipExtLaunchKernelGGL((phi_sketch_kernel<MODE, true, 31, 25>), dim3(nb), dim3(TPB), lds, st, t0, t1, 0, A);
            return;
        }
    }
    if constexpr (MODE == PHI_MODE_PROBE) {
        if (A.k > PHI_MAX_K_PACKED) {                      // reads with k > 32: staging, read starts and bookkeeping of the fused kernel, every window byte-wise
            hipExtLaunchKernelGGL((phi_sketch_kernel<MODE, true, -1, 0>), dim3(nb), dim3(TPB), lds, st, t0, t1, 0, A);
            return;
        }
    }
    if (A.w > Q) hipExtLaunchKernelGGL((phi_sketch_kernel<MODE, true, 0, 0>), dim3(nb), dim3(TPB), lds, st, t0, t1, 0, A);
    else hipExtLaunchKernelGGL((phi_sketch_kernel<MODE, false, 0, 0>), dim3(nb), dim3(TPB), lds, st, t0, t1, 0, A);
}

// chunks from which a read batch takes the pooled kernel
static int64_t pool_min_chunks()
{
    int64_t min_chunks = 4 * 6144;
    if (const char *e = getenv("PHI_SKETCH_POOL_MIN")) min_chunks = atoll(e);
    return min_chunks;
}

// Reads of one length: whole reads per wave of phi_sketch_win_kernel, or 0 for base space.  A wave holds R reads of
// G = ceil(V / Q) lanes each (R G <= 64), its staged bases (R L <= 928: the 1 024 bases of phase 0, less the alignment of the
// first read and the word read past a k-mer's last base), no more LDS than the base-space kernel for the same (k, w) (so
// never fewer waves per SIMD), and a lane rolls at most 32 k-mers (one staged word of bases ahead).  It pays when the
// wave's R L bases outnumber the 512 positions of a base-space chunk clearly -- R L >= 576: at most 8 waves where base
// space has 9 (long reads have few positions that are not windows: L = 300 at (31, 25) gives R = 2, 600 bases, 4 %
// fewer waves).  It also takes the batches of 12 Mbases and more that the pooled kernel took (C3: 495 -> 633 Gbases/s,
// DESIGN.md 4.1), unless PHI_SKETCH_POOL_MIN is set: then batches from that size on stay pooled (tests of that kernel).
// PHI_SKETCH_WINDOWS: "0" never, "1" whenever the geometry allows (tests run a batch both ways).
int phi_sketch_win_reads(int k, int w, int64_t uniform_len, int64_t n_reads, int64_t n_bases)
{
    if (uniform_len <= 0 || n_reads <= 0 || k > PHI_MAX_K_PACKED) return 0;
    int force = -1;
    if (const char *e = getenv("PHI_SKETCH_WINDOWS")) force = atoi(e) ? 1 : 0;
    if (force == 0) return 0;
    const int64_t L = uniform_len, V = L - (k + w - 1) + 1;
    if (V < 1 || L > 928) return 0;
    const int G = (int)((V + Q - 1) / Q), s = G + (w + Q - 1) / Q;
    if (G > 64 || (L - k + 1 + G - 1) / G > 32) return 0;
    int R = 64 / G;
    if (R > 928 / L) R = (int)(928 / L);
    // (R as when the staged words and bitmap lay behind the k-mers: the reads of a wave do not change with the smaller region)
    while (R > 0 && phi_win_region_u64(R, s, w, k) + SWW + SBW > phi_wave_region_u64(w, k, false)) R--;
    if (R < 1) return 0;
    if (force != 1 && (R * L < WCH + WCH / 8 || (getenv("PHI_SKETCH_POOL_MIN") && phi_sketch_num_blocks(n_bases) >= pool_min_chunks()))) return 0;
    return R;
}

int64_t phi_sketch_read_chunks(int k, int w, int64_t uniform_len, int64_t n_reads, int64_t n_bases)
{
    const int R = phi_sketch_win_reads(k, w, uniform_len, n_reads, n_bases);
    return R > 0 ? (n_reads + R - 1) / R : phi_sketch_num_blocks(n_bases);
}

void phi_launch_sketch(hipStream_t st, int mode, const PhiSketchArgs &A0, hipEvent_t t0, hipEvent_t t1)
{
    const int64_t nchunks = phi_sketch_num_blocks(A0.n_bases);
    if (nchunks <= 0) return;
    PhiSketchArgs A = A0;
    if (mode == PHI_MODE_PROBE) {
        const int R = phi_sketch_win_reads(A.k, A.w, A.uniform_len, A.n_reads, A.n_bases);
        if (R > 0) {
            // reads of one length in window space: R whole reads per wave (phi_sketch_win_kernel)
            A.win_reads = R;
            const int64_t waves = (A.n_reads + R - 1) / R;
            const unsigned nb = (unsigned)((waves + TPB / 64 - 1) / (TPB / 64));
            const int V = (int)(A.uniform_len - (A.k + A.w - 1) + 1);
            const int s = (V + Q - 1) / Q + (A.w + Q - 1) / Q;
            const size_t lds = (size_t)phi_win_region_u64(R, s, A.w, A.k) * 8 * (TPB / 64);
            if (phi_launch_sketch_win_fixed(st, nb, lds, A, t0, t1)) return;      // (a geometry with an instance of its own)
            if (A.k == 31 && A.w == 25) hipExtLaunchKernelGGL((phi_sketch_win_kernel<true, 31, 25>), dim3(nb), dim3(TPB), lds, st, t0, t1, 0, A);
            else if (A.w > Q) hipExtLaunchKernelGGL((phi_sketch_win_kernel<true, 0, 0>), dim3(nb), dim3(TPB), lds, st, t0, t1, 0, A);
            else hipExtLaunchKernelGGL((phi_sketch_win_kernel<false, 0, 0>), dim3(nb), dim3(TPB), lds, st, t0, t1, 0, A);
            return;
        }
    }
    // Reads (k <= 32), batches of 12 Mbases and more: wave g of `njobs` takes the chunks g, g + njobs, ... and hashes their
    // items in full rounds (POOL in the kernel).  Four times as many waves as the machine holds at once (256 CUs x 4 SIMDs
    // x 6 waves of this kernel): the SIMDs serve their oldest wave first, so waves of equal shares end far apart (the first
    // in half the time of the last) and it takes waves in waiting to fill the slots they leave -- measured at C3 / C5s:
    // 6 144 waves 417 / -, 12 288 424 / 439, 18 432 433 / 443, 24 576 447 / 451, 36 864 439 / 442 Gbases/s.  Fewer than
    // three chunks per wave are not worth a loop: smaller batches run one chunk per wave as before.
    int64_t njobs = nchunks;
    bool pooled = false;
    if (mode == PHI_MODE_PROBE && A.k <= PHI_MAX_K_PACKED) {
        int64_t slots = 4 * 256 * 4 * 6;
        const int64_t min_chunks = pool_min_chunks();
        if (const char *e = getenv("PHI_SKETCH_WAVES")) slots = atoll(e) > 0 ? atoll(e) : slots;
        if (nchunks >= min_chunks) {
            int64_t m = (nchunks + slots - 1) / slots;          // chunks per wave
            if (m < 3) m = 3;
            njobs = (nchunks + m - 1) / m;
            if (njobs > 0x7FFFFFFF) njobs = 0x7FFFFFFF;
            A.wave_stride = (int32_t)njobs;
            pooled = true;
        }
    }
    const unsigned nb = (unsigned)((njobs + TPB / 64 - 1) / (TPB / 64));
    const size_t lds = (size_t)phi_wave_region_u64(A.w, A.k, mode == PHI_MODE_WRITE) * 8 * (TPB / 64);
    if (mode == PHI_MODE_COUNT) launch_sketch_mode<PHI_MODE_COUNT>(st, nb, lds, A, t0, t1, false);
    else if (mode == PHI_MODE_WRITE) launch_sketch_mode<PHI_MODE_WRITE>(st, nb, lds, A, t0, t1, false);
    else launch_sketch_mode<PHI_MODE_PROBE>(st, nb, lds, A, t0, t1, pooled);
}

// One empty launch loads this translation unit's code object onto the device: the HIP runtime does that lazily, at the
// first launch of any of its kernels (0.5-1.3 ms per unit, measured inside phi_set_graph / phi_solve before
// phi_ctx_create did it up front).
__global__ void phi_warm_sketch_kernel() {}
void phi_warm_sketch(hipStream_t st) { hipLaunchKernelGGL(phi_warm_sketch_kernel, dim3(1), dim3(64), 0, st); }
