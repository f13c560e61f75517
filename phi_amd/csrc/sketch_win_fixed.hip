// sketch_win_fixed.hip -- the window-space read kernel with its whole geometry known at compile time: 150-bp reads at
// the reference's defaults k = 31, w = 25 (its own data and every one-length bench set).  The helpers it shares with the
// kernels of sketch.hip and sketch_pooled.hip come from sketch_dev.h; phi_launch_sketch calls the launcher below
// whenever it takes window space for such a batch.  PHI_SKETCH_WIN_FIXED=0 sends those batches to phi_sketch_win_kernel.
//
// What phi_sketch_win_kernel computes at run time is constant here:
//  - the wave's first base, its staging and its base load depend on blockIdx and the lane alone: the load is issued before
//    anything else, and the lane's read and lane group (rl, j) come after it, by a multiply-shift;
//  - phase 1 has no roll: a lane takes the 48 bases from its first k-mer's (three funnel shifts of four staged words), their
//    reverse complement in registers, and each of its P = 10 canonical k-mers is two 62-bit extracts at constant shifts and
//    one v_min_f64, stored at constant offsets from one of four addresses;
//  - every window of a lane exists (V = 96 = 8 G): phase 3 has no `imax`.
// Phases 2 - 5, the byte-wise routine for bases outside ACGTacgt, the log, clean_finish and the epilogue are those of
// phi_sketch_win_kernel, and so are its outputs -- except that a clean wave (every base ACGTacgt) of a graph with a k-mer table
// (A.k_rt) probes by k-mer and logs novel k-mers, without MurmurHash3: sketch_rounds_kmer.inc.
#include "sketch_dev.h"

// reverse complement of 16 bases in 2 bits (first base in the top bits)
__device__ __forceinline__ uint32_t revcomp16(uint32_t x)
{
    x = __builtin_bitreverse32(x);                                   // bases reversed, the two bits of each swapped
    return ~(((x >> 1) & 0x55555555u) | ((x << 1) & 0xAAAAAAAAu));  // swapped back, complemented (3 - b)
}

// bits S .. S + 61 of the 96-bit value u0:u1:u2 (u2 the lowest word): a 31-mer
template <int S>
__device__ __forceinline__ uint64_t bits62(uint32_t u0, uint32_t u1, uint32_t u2)
{
    static_assert(S >= 0 && S <= 34, "inside the 96 bits");
    uint32_t lo, hi;
    if constexpr (S >= 32) {
        lo = __builtin_amdgcn_alignbit(u0, u1, S - 32);
        hi = (u0 >> (S - 32)) & 0x3FFFFFFFu;
    } else {
        // (v_alignbit_b32 spelled out: the compiler turns the 64-bit shift of the high word into four instructions)
        lo = __builtin_amdgcn_alignbit(u1, u2, S);
        hi = __builtin_amdgcn_alignbit(u0, u1, S) & 0x3FFFFFFFu;
    }
    return ((uint64_t)hi << 32) | lo;
}

template <int KT, int WT, int LT>
__global__ void __launch_bounds__(TPB, 7) phi_sketch_winfix_kernel(PhiSketchArgs A)   // (seven waves per SIMD, at most 72 VGPRs)
{
    constexpr int MODE = PHI_MODE_PROBE;
    constexpr bool NEED_POS = false, WIDE = true, FMIN = true;   // (names of the shared phases)
    constexpr int k = KT, w = WT, L = LT, span = w + k - 1, V = L - span + 1;
    constexpr int G = (V + Q - 1) / Q, s = G + (w + Q - 1) / Q, R = 64 / G;
    constexpr int NKM = L - k + 1, P = NKM / G;              // k-mers of a read; k-mers of a lane
    static_assert(k == 31 && w > Q, "31-mers: values below 2^62, two 62-bit extracts of 48 bases");
    static_assert(V == Q * G && NKM == P * G && P == 10, "every window and k-mer of a lane exists; the store offsets below");
    static_assert(R * L <= 928 && R * G <= 64, "the staging of phase 0");
    extern __shared__ uint64_t s_dyn[];

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t chunk = (int64_t)blockIdx.x * (TPB / 64) + wid;     // this wave's reads: chunk * R .. + R - 1
    const int64_t rd0 = chunk * R;
    // staging origin: the 32-base word holding the wave's first base (local base lb <-> base c0 - 32 + lb, local bit lp <->
    // base c0 - 64 + lp, as in phi_sketch_win_kernel)
    const int64_t c0 = (rd0 * L) & ~(int64_t)31;
    const int64_t N = A.n_bases;
    // ---- phase 0, issued first: lane -> the 16 bases c0 - 32 + 16 lane .. + 15 (a wave past the batch loads nothing)
    const uint4 bv = load_bases16<1>(A.ascii, N, c0, lane);
    if (A.ipc_mb && chunk == 0 && lane == 0)               // (a group of processes: see PhiSketchArgs)
        __hip_atomic_store(A.ipc_mb + PHI_MB_SCORED, A.ipc_scored, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    if (rd0 >= A.n_reads) {                                // wave-uniform
        if (A.q_clean) clean_finish(A, chunk, (int64_t)gridDim.x * (TPB / 64), lane);
        return;
    }
    const int nr = A.n_reads - rd0 < R ? (int)(A.n_reads - rd0) : R;   // reads of this wave
    // this lane's read and lane group: rl = lane / G, j = lane % G (lane < 64: a multiply-shift)
    const int rl = (int)((unsigned)lane / (unsigned)G), j = lane - rl * G;
    const bool live = rl < nr;

    using MetaT = uint16_t;
    constexpr uint32_t ITEM_FIRST = 1u << 15;            // the first window of its read
    constexpr uint32_t ITEM_NOEMIT = 1u << 14;           // only its hash is needed (the window before a candidate)
    uint64_t *s_mp = s_dyn + (size_t)wid * phi_win_region_u64(R, s, w, k);   // k-mers; later the window minima and the items
    uint32_t *s_code = (uint32_t *)s_mp;                  // staged bases: 16 per word in base order, until phase 1 has read them
    unsigned long long *s_bad = (unsigned long long *)s_mp;   // bitmap (chunk_bad only): staged where the region is dead
    MetaT *s_meta = (MetaT *)(s_mp + 9 * (64 + 1));      // items: behind the minima
    uint64_t *s_q = s_mp + (live ? 9 * (rl * s + j) : 0);   // k-mer 8j - 1 + x of the lane's read: s_q[x + (x >> 3)]

    bool chunk_bad;
    {
        const uint32_t x[4] = {bv.x, bv.y, bv.z, bv.w};
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
        s_code[lane] = code;
        chunk_bad = __ballot(lane < 62 && bad != 0) != 0ull;   // wave-uniform
    }
    const bool kmer_keys = !chunk_bad && A.k_rt != nullptr;   // wave-uniform: the rounds of sketch_rounds_kmer.inc
    wave_sync();

    // ---- phase 1: k-mers P j .. P j + P - 1 of the lane's read (bases P j .. P j + P + k - 2), canonical, to slots
    //      8 s rl + 1 + P j + i.  The four staged words from the one before the lane's first base: u0:u1:u2 = the 48 bases
    //      from it, z0:z1:z2 their reverse complement; k-mer i is bits 34 - 2i .. of u, its reverse complement bits 2i .. of z
    {
        const int lb = (int)((rd0 * L) & 31) + rl * L + P * j + 32;    // local base of the lane's first k-mer (>= 32)
        const int d0 = (lb - 1) >> 4, rsh = 30 - 2 * ((lb - 1) & 15);  // base lb is 2 (16 - rsh / 2) bits into word d0
        const uint32_t d[4] = {s_code[d0], s_code[d0 + 1], s_code[d0 + 2], s_code[d0 + 3]};
        wave_sync();                                      // every lane has read its words: the k-mers go over them
        const uint32_t u0 = __builtin_amdgcn_alignbit(d[0], d[1], rsh);
        const uint32_t u1 = __builtin_amdgcn_alignbit(d[1], d[2], rsh);
        const uint32_t u2 = __builtin_amdgcn_alignbit(d[2], d[3], rsh);
        const uint32_t z0 = revcomp16(u2), z1 = revcomp16(u1), z2 = revcomp16(u0);
        uint64_t km[P];
#define KM(i) km[i] = min_u62(bits62<34 - 2 * (i)>(u0, u1, u2), bits62<2 * (i)>(z0, z1, z2))
        KM(0); KM(1); KM(2); KM(3); KM(4); KM(5); KM(6); KM(7); KM(8); KM(9);
#undef KM
        if (live) {
            // slot u = 8 s rl + 1 + P j + i lies at u + (u >> 3).  8 s rl is a multiple of 8 and (1 + 10 j) & 7 = 1 + 2 (j & 3),
            // so the pad words before slot i of the lane are: 0 for i = 0; for i = 1, 2: j & 3 == 3; 3, 4: j & 3 >= 2;
            // 5, 6: j & 3 >= 1; 7, 8: 1; 9: 1 + (j & 3 == 3) -- four addresses, constant offsets from each
            const int u = 8 * s * rl + 1 + P * j, m = j & 3;
            uint64_t *b0 = s_mp + u + (u >> 3);
            uint64_t *b1 = b0 + (m == 3), *b2 = b0 + (m >= 2), *b3 = b0 + (m >= 1);
            b0[0] = km[0];
            b1[1] = km[1]; b1[2] = km[2];
            b2[3] = km[3]; b2[4] = km[4];
            b3[5] = km[5]; b3[6] = km[6];
            b0[8] = km[7]; b0[9] = km[8];
            b1[10] = km[9];
        }
    }
    wave_sync();

    // ---- phase 2: minima of the lane's windows 8j - 1 .. 8j + 7 of its read (k-mers 8j - 1 .. 8j + 6 + w)
#include "sketch_minima.inc"

    // ---- phase 3: candidate windows i = 1..Q of this lane (window 8j + i - 1 of its read; all Q exist)
    if (chunk_bad) {                                      // (wave-uniform, rare) every lane has read its k-mers: the bitmap over them
        wave_sync();
        stage_bad_bits(A.ascii, N, c0, lane, s_bad);
        wave_sync();
    }
    uint32_t cflag = 0, fflag = 0, pflag = 0;             // candidates; first windows; candidates that carry their predecessor
    if (live) {
        constexpr uint32_t in_read = (2u << Q) - 2u;       // bits 1 .. Q
        const uint32_t first = j == 0 ? 2u : 0u;           // window 0 of the read
        uint32_t changed = 0;
#pragma unroll
        for (int i = 1; i <= Q; i++) changed |= (uint32_t)(wv[i] != wv[i - 1]) << i;
        // bit i of `dall`: a base outside ACGT under window i or its predecessor (see phi_sketch_win_kernel)
        uint32_t dall = 0, reseed = 0;
        if (chunk_bad) {
            const int lp0 = (int)((rd0 * L) & 31) + rl * L + Q * j - 1 + 64;   // local bit of window 0's base
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
        if (coff == 0 && cflag && !kmer_keys) s_meta[0] = (MetaT)((uint32_t)(lane * Q + __ffs((int)cflag) - 2) | ITEM_NOEMIT);
    }
    wave_sync();
#undef SQ

    // ---- phases 4 + 5, as in base space
    int n_emit = 0, n_log = 0, n_nov_slow = 0;
    const int64_t out_base = 0;
    bool hashed = !kmer_keys;                            // wave-uniform: the chunk's log holds hashes
    if (!hashed) {
#include "sketch_rounds_kmer.inc"
    }
    if (hashed) {
#include "sketch_rounds.inc"
    }

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
        // (the arguments of the epilogue are loaded now, not kept in scalar registers from the start: see phi_sketch_win_kernel)
        const KArgs PA = kargs_now();
        if (PA->q_clean) clean_finish(*PA, chunk, (int64_t)gridDim.x * (TPB / 64), lane);
        if (lane == 0) {
            const int cap = 1 << PA->nov_shift;
            PA->nov_cnt[PA->log_base + chunk] = (uint16_t)((uint32_t)(n_log < cap ? n_log : cap) | (hashed ? 0u : PHI_NOV_KMERS));
            const int n_nov_wave = n_log + n_nov_slow;
            const int stripe = (int)(chunk & (PHI_STRIPES - 1)) * 8;
            if (n_nov_wave && PA->n_logged) atomicAdd(PA->n_logged + stripe, (unsigned long long)n_nov_wave);
            if (n_emit && PA->n_emitted) atomicAdd(PA->n_emitted + stripe, (unsigned long long)n_emit);
        }
    }
}

// The fixed-geometry instance for a window-space launch that phi_launch_sketch has set up (A.win_reads, the grid, the LDS),
// when the batch has its geometry: false, launching nothing, otherwise (or with PHI_SKETCH_WIN_FIXED=0).
bool phi_launch_sketch_win_fixed(hipStream_t st, unsigned nb, size_t lds, const PhiSketchArgs &A, hipEvent_t t0, hipEvent_t t1)
{
    if (!(A.k == 31 && A.w == 25 && A.uniform_len == 150 && A.win_reads == 5)) return false;
    if (const char *e = getenv("PHI_SKETCH_WIN_FIXED"))
        if (!atoi(e)) return false;
    hipExtLaunchKernelGGL((phi_sketch_winfix_kernel<31, 25, 150>), dim3(nb), dim3(TPB), lds, st, t0, t1, 0, A);
    return true;
}
