// sketch_dev.h -- what the three translation units of the sketch kernels share (sketch.hip, sketch_pooled.hip,
// sketch_win_fixed.hip): constants, LDS geometry and the device routines of the phases.  No kernel and no launcher
// lives here; sketch.hip describes the phases.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <hip/hip_ext.h>
#include "phi_dev.h"
#include "phi_kernels.h"
#ifndef PHI_ABL
#define PHI_ABL 0      // ablation / occupancy experiments: 0 = the product
#endif

#define TPB PHI_TPB
#define Q 8                     // windows per lane

// ---------------------------------------------------------------------------------- packing

// 32 ASCII bases per lane -> one packed word (+ one 32-bit mask of the bases outside ACGTacgt).
static __device__ __forceinline__ void pack_ascii_word(int64_t wi, const uint8_t *__restrict__ bases, int64_t n,
                                                       uint64_t *__restrict__ words, int64_t n_words,
                                                       uint32_t *__restrict__ badbits,
                                                       unsigned long long *__restrict__ n_bad)
{
    if (wi >= n_words + 4) return;
    if (wi >= n_words) {                                    // zero padding: 2 words, 4 mask words
        if (wi < n_words + 2) words[wi] = 0;
        if (badbits) badbits[wi] = 0;
        return;
    }
    const int64_t b0 = wi * 32;
    uint64_t word = 0;
    uint32_t bad = 0;
    if (b0 + 32 <= n && ((uintptr_t)(bases + b0) & 15) == 0) {
        const uint4 *p = reinterpret_cast<const uint4 *>(bases + b0);
        uint4 v[2] = {p[0], p[1]};
        const uint32_t *u = reinterpret_cast<const uint32_t *>(v);
#pragma unroll
        for (int q = 0; q < 8; q++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t c = (u[q] >> (8 * j)) & 0xFFu;
                bad |= (uint32_t)(!phi_is_acgt(c)) << (4 * q + j);
                word = (word << 2) | phi_code(c);
            }
        }
    } else {
        for (int j = 0; j < 32; j++) {
            uint32_t c = 'A';
            if (b0 + j < n) { c = bases[b0 + j]; bad |= (uint32_t)(!phi_is_acgt(c)) << j; }
            word = (word << 2) | phi_code(c);
        }
    }
    words[wi] = word;
    if (badbits) badbits[wi] = bad;
    if (bad) atomicAdd(n_bad, (unsigned long long)__popc(bad));
}

// The bitmap of phi_mark_starts_kernel (sketch.hip), one whole word per lane: no memset, no atomics.  Word j covers bases [64j, 64j+64).
static __device__ __forceinline__ void start_bitmap_word(int64_t j, const int64_t *__restrict__ seq_off, int64_t n_seq,
                                                         unsigned long long *__restrict__ starts, int64_t n_sw, int64_t total = 0)
{
    if (j >= n_sw) return;
    const int64_t lo_b = j * 64, hi_b = lo_b + 64;
    // first sequence with seq_off >= lo_b (n_seq if none).  Reads are of similar lengths, so the answer
    // lies close to lo_b / mean length: gallop away from that guess, then bisect the bracket (3-4
    // dependent loads instead of log2(n_seq))
    int64_t lo = 0, hi = n_seq;
    if (total > 0 && n_seq > 64) {
        int64_t g = (int64_t)((double)lo_b / (double)total * (double)n_seq);
        g = g < 0 ? 0 : (g > n_seq - 1 ? n_seq - 1 : g);
        if (seq_off[g] >= lo_b) {                      // answer <= g
            hi = g;
            int64_t step = 1;
            while (hi - step >= 0) {
                if (seq_off[hi - step] < lo_b) { lo = hi - step + 1; break; }
                hi -= step;
                step <<= 1;
            }
        } else {                                       // answer > g
            lo = g + 1;
            int64_t step = 1;
            while (lo + step < n_seq) {
                if (seq_off[lo + step] >= lo_b) { hi = lo + step; break; }
                lo += step + 1;
                step <<= 1;
            }
        }
    }
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (seq_off[mid] < lo_b) lo = mid + 1; else hi = mid;
    }
    unsigned long long word = 0;
    for (int64_t r = lo; r < n_seq; r++) {
        const int64_t p = seq_off[r];
        if (p >= hi_b) break;
        if (seq_off[r + 1] > p) word |= 1ull << (p & 63);   // empty sequences own no base
    }
    starts[j] = word;
}

// ---------------------------------------------------------------------------------- helpers

// Lanes of one wave exchange data through LDS without a workgroup barrier: LDS instructions of a
// wave execute in issue order, so only the compiler has to be kept from reordering them.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// first set bit at local index >= from and < limit in an LDS bitmap, or INT_MAX
__device__ __forceinline__ int next_start_lds(const unsigned long long *s_bits, int from, int limit)
{
    if (from >= limit) return INT_MAX;
    int wi = from >> 6;
    const int wl = (limit - 1) >> 6;
    unsigned long long word = s_bits[wi] & (~0ull << (from & 63));
    for (;;) {
        if (word) {
            const int p = (wi << 6) + (__ffsll((long long)word) - 1);
            return p < limit ? p : INT_MAX;
        }
        if (++wi > wl) return INT_MAX;
        word = s_bits[wi];
    }
}

// 32 bases starting at local base lb of the staged words, left-aligned
__device__ __forceinline__ uint64_t lds_extract64(const uint64_t *s_words, int lb)
{
    const int wi = lb >> 5, s = (lb & 31) * 2;                 // s <= 62: no special case for s == 0
    return (s_words[wi] << s) | ((s_words[wi + 1] >> 1) >> (63 - s));
}

struct MinEnt { uint64_t v; int i; };
// b lies to the right of a: ties go right (the reference's deque pops on >=, ILP_index.cpp:397)
__device__ __forceinline__ MinEnt take_right(MinEnt a, MinEnt b) { return (b.v <= a.v) ? b : a; }

// Walk-minimiser table probe of one emitted read hash.  A hash found in the walk table is recorded by its hit flag
// alone; the others -- NOVEL hashes: sequencing errors, alleles no walk carries -- only feed |Sp_R| and the log counters
// that derive from it (ILP_index.cpp:622-641, 738-743, 883).  They are not entered into a set here (round 3: an atomicCAS
// per novel hash into a 64-MB table, a second dependent round trip behind the probe and ~100 bytes of write traffic per
// 8-byte key: 45 % of the launch on long noisy reads): the wave appends them to its LOG, coalesced, and the set is made
// from the log once, when somebody asks for |Sp_R| (read_batches.hip phi_sp_flush).
// The table is the read table of table.hip (phi_launch_read_table): aligned 32-byte buckets of two (key, id) slots, home
// bucket h & bmask.  A lookup loads its whole home bucket -- both slots, keys and ids, issued before one wait -- and is done
// unless the bucket's OVERFLOWED flag says that a key whose home it is lies in a later bucket (3e-4 of the buckets at
// C2); only then does it walk on, bucket by bucket, to a match or to a bucket with a free slot.  The old one-slot table
// took a dependent trip per displaced slot in most waves.
// returns true when h is NOT a walk minimiser
struct ProbeArgs { const uint64_t *u_rt; uint64_t u_bmask; uint8_t *hit; uint32_t *err; };
// one bucket: both keys, both ids and the flags in registers.  (Every half made live here: left alone the compiler loads
// the keys, and each id in a second, dependent load inside the branch of its match.)
__device__ __forceinline__ void rt_bucket(const uint64_t *rt, uint64_t b, ulonglong2 &s0, uint3 &s1)
{
    const uint64_t *p = rt + 4 * b;
    s0 = *reinterpret_cast<const ulonglong2 *>(p);               // key 0, id 0 | flags << 32
    s1 = *reinterpret_cast<const uint3 *>(p + 2);                // key 1 (x, y), id 1 (z): the word after it carries nothing
    asm volatile("" : "+v"(s0.x), "+v"(s0.y), "+v"(s1.x), "+v"(s1.y), "+v"(s1.z));
}
// (SENT = false: the key cannot be the sentinel -- phi_kmer_mix of a k-mer, phi_dev.h)
template <bool SENT = true>
__device__ __forceinline__ bool probe_table(const ProbeArgs &A, uint64_t h)
{
    if (SENT && h == PHI_EMPTY_KEY) { atomicOr(A.err, PHI_KERR_SENTINEL); return false; }
    uint64_t b = h & A.u_bmask;
    ulonglong2 s0;
    uint3 s1;
    rt_bucket(A.u_rt, b, s0, s1);
    // walk-minimiser table: lookup, mark the minimiser as hit
    const uint64_t k1 = ((uint64_t)s1.y << 32) | s1.x;
    if (s0.x == h) { A.hit[(uint32_t)s0.y] = 1; return false; }
    if (k1 == h) { A.hit[s1.z] = 1; return false; }
    if ((s0.y >> 32) & PHI_RT_OVERFLOWED) {
        for (int probes = 1; probes <= PHI_MAX_PROBE; probes++) {
            b = (b + 1) & A.u_bmask;
            rt_bucket(A.u_rt, b, s0, s1);
            const uint64_t n1 = ((uint64_t)s1.y << 32) | s1.x;
            if (s0.x == h) { A.hit[(uint32_t)s0.y] = 1; return false; }
            if (n1 == h) { A.hit[s1.z] = 1; return false; }
            if (n1 == PHI_EMPTY_KEY) break;                      // a bucket with room ends every chain through it
        }
    }
    return true;
}

__device__ __forceinline__ bool probe_table(const PhiSketchArgs &A, uint64_t h)
{
    const ProbeArgs P{A.u_rt, A.u_bmask, A.hit, A.err};
    return probe_table(P, h);
}

// Novel hashes a wave's log has no room for (a chunk that emits more than 1.5x what random sequence does; the byte-wise
// routine's windows): one atomic per round for all of them, then a coalesced store into the generation's overflow list.
// A full list raises PHI_KERR_TABLE_FULL: phi_add_reads grows it and replays the batch.  Wave-uniform call.
// returns how many the round sent there
struct OverflowArgs { uint64_t *list; unsigned long long *count; int64_t cap; uint32_t *err; };
__device__ __forceinline__ int overflow_novel(const OverflowArgs &O, bool ov, uint64_t h, int lane)
{
    const unsigned long long ob = __ballot(ov);
    if (!ob) return 0;
    const int first = __ffsll((long long)ob) - 1, n = __popcll(ob);
    unsigned long long base = 0;
    if (lane == first) base = atomicAdd(O.count, (unsigned long long)n);
    base = __shfl(base, first, 64);
    if (ov) {
        const unsigned long long idx = base + (unsigned long long)__popcll(ob & ((1ull << lane) - 1));
        if ((int64_t)idx < O.cap) O.list[idx] = h;
        else atomicOr(O.err, PHI_KERR_TABLE_FULL);
    }
    return n;
}
// The kernel's arguments where the launch put them (the kernarg segment; the one struct parameter sits at its start), through
// a pointer the compiler cannot see through: what is read this way is loaded (scalar loads) where it is used instead of
// living in scalar registers from the start of the kernel -- the read kernel's loop over a wave's chunks runs with every
// scalar register taken, and each value too many costs v_writelane / v_readlane pairs in every turn.
typedef const __attribute__((address_space(4))) PhiSketchArgs *KArgs;
__device__ __forceinline__ KArgs kargs_now()
{
    KArgs p = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// ---------------------------------------------------------------------------------- byte-wise routine
// Exact restatement on ASCII for windows the 2-bit path cannot take (ILP_index.cpp:330-357, 388-414).

struct KRef { int64_t pos; int rc; };        // a k-mer: start base and strand

__device__ __forceinline__ uint32_t up_byte(uint32_t c) { return (c >= 'a' && c <= 'z') ? c - 32 : c; }
__device__ __forceinline__ uint32_t comp_byte(uint32_t c)     // c is upper case; others map to themselves
{
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}
__device__ __forceinline__ uint32_t kbyte(const uint8_t *__restrict__ s, KRef r, int x, int k)
{
    return r.rc ? comp_byte(up_byte(s[r.pos + k - 1 - x])) : up_byte(s[r.pos + x]);
}
__device__ __forceinline__ int kcmp(const uint8_t *__restrict__ s, KRef a, KRef b, int k)
{
    for (int x = 0; x < k; x++) {
        const uint32_t ca = kbyte(s, a, x, k), cb = kbyte(s, b, x, k);
        if (ca != cb) return ca < cb ? -1 : 1;
    }
    return 0;
}
__device__ __forceinline__ KRef canon_bytes(const uint8_t *__restrict__ s, int64_t i, int k)
{
    const KRef f{i, 0}, r{i, 1};
    return kcmp(s, r, f, k) < 0 ? r : f;                    // std::min(fwd, rev)
}
__device__ KRef window_best_bytes(const uint8_t *__restrict__ s, int64_t a, int k, int w)
{
    KRef best = canon_bytes(s, a, k);
    for (int j = 1; j < w; j++) {
        const KRef c = canon_bytes(s, a + j, k);
        if (kcmp(s, c, best, k) <= 0) best = c;             // ties go right
    }
    return best;
}
template <bool LONGK>   // LONGK: k may exceed 32 (eight lanes; kept out of the kernels that never see such k)
__device__ uint64_t khash_bytes(const uint8_t *__restrict__ s, KRef r, int k)
{
    if (LONGK && k > PHI_MAX_K_PACKED) {
        uint64_t e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int g = 0; g < 8; g++) {                               // (constant indices: the lanes stay in registers)
            uint64_t v = 0;
            for (int x = 8 * g; x < 8 * g + 8 && x < k; x++) v |= (uint64_t)kbyte(s, r, x, k) << (8 * (x & 7));
            e[g] = v;
        }
        return phi_murmur_lanes8(e, k);
    }
    uint64_t e0 = 0, e1 = 0, e2 = 0, e3 = 0;
    for (int x = 0; x < k; x++) {
        const uint64_t b = (uint64_t)kbyte(s, r, x, k) << (8 * (x & 7));
        if (x < 8) e0 |= b; else if (x < 16) e1 |= b; else if (x < 24) e2 |= b; else e3 |= b;
    }
    return phi_murmur_lanes(e0, e1, e2, e3, k);
}

__device__ __forceinline__ bool range_has_bit(const unsigned long long *s_bits, int lo, int hi)   // [lo, hi]
{
    return next_start_lds(s_bits, lo, hi + 1) != INT_MAX;
}

// Windows la = 1..WCH of this wave's chunk that need the byte-wise path, in position order.
template <int MODE, bool LONGK = false>
__device__ __forceinline__ void slow_windows(const PhiSketchArgs &A, int64_t c0, int64_t chunk, int lane, int k, int w,
                                          const unsigned long long *s_bits, const unsigned long long *s_bad,
                                          bool allslow, int64_t out_base, int &n_emit, int &n_nov)
{
    const int64_t N = A.n_bases;
    const int span = w + k - 1;
    for (int r = 0; r < PHI_WCH / 64; r++) {
        const int la = 1 + r * 64 + lane;
        const int64_t a = c0 - 1 + la;
        const int lp = la + 63;                                     // local bit of base a
        bool todo = (a + span <= N) && !range_has_bit(s_bits, lp + 1, lp + span - 1);
        if (todo && !allslow) todo = range_has_bit(s_bad, lp - 1, lp + span - 1);
        bool emit = false;
        uint64_t h = 0;
        int64_t pos = 0;
        if (todo) {
            const bool first = (s_bits[lp >> 6] >> (lp & 63)) & 1ull;
            const KRef best = window_best_bytes(A.ascii, a, k, w);
            h = khash_bytes<LONGK>(A.ascii, best, k);
            pos = best.pos;
            if (first) emit = h != PHI_EMPTY_KEY;                   // prev_hash = UINT64_MAX (:383, :455)
            else {
                const KRef prev = window_best_bytes(A.ascii, a - 1, k, w);
                emit = !(prev.pos == best.pos && prev.rc == best.rc) && khash_bytes<LONGK>(A.ascii, prev, k) != h;
            }
        }
        const unsigned long long bal = __ballot(emit);
        bool novel = false;
        if (emit) {
            const int rank = n_emit + __popcll(bal & ((1ull << lane) - 1));
            if (MODE == PHI_MODE_WRITE) {
                A.out_hash[out_base + rank] = h;
                A.out_pos[out_base + rank] = pos;
            } else if (MODE == PHI_MODE_PROBE) {
                novel = probe_table(A, h);
            }
        }
        if (MODE == PHI_MODE_PROBE) {
            const OverflowArgs O{A.ov_list, A.ov_count, A.ov_cap, A.err};
            n_nov += overflow_novel(O, novel, h, lane);               // (the byte-wise routine's novel hashes: straight to the overflow list)
        }
        n_emit += __popcll(bal);
    }
    (void)chunk;
}

// ---------------------------------------------------------------------------------- sketch

#define WCH PHI_WCH
#define SWW 32          // staged packed words per wave:  (WCH + w + k + 62) / 32 + 1 <= 29
#define SBW 16          // staged bitmap words per wave:  (WCH + 64 + w + k) / 64 + 2 <= 16
#define SM(l) s_mp[(l) + ((l) >> 3)]   // one pad word per 8 entries: lane t reads entries 8t+i
                                        // = u64 index 9t+i: conflict-free for ds_read_b64

// k-mer slots of one wave: every lane rolls P = ceil((WCH + w) / 64) consecutive k-mers and stores all
// of them (the lanes past WCH + w write k-mers nobody reads), so the roll needs no per-store check
// (lanes whose first k-mer lies past WCH + w store nothing: the region ends with the last storing lane's P slots)
__host__ __device__ static inline int phi_wave_mp_u64(int w)
{
    const int M = WCH + w, P = (M + 63) / 64;
    const int slots = ((M - 1) / P + 1) * P;
    return ((slots + 8) * 9) / 8 + 8;
}
// items of one chunk: the window before its first candidate, its candidates, and one more per stretch of
// windows the 2-bit path leaves to the byte-wise one (a stretch is longer than a window's span: the first
// window after it carries its own predecessor, see phase 3); + 4 trash slots
__host__ __device__ static inline int phi_wave_items(int w, int k) { return 1 + WCH + WCH / (w + k + 1) + 2; }
// An item is 32 bits when it carries the minimiser's position (ordered write of the walks), 16 bits otherwise
// (slot 0 .. 512, "first window of its sequence", "only its hash is needed"): with the k-mer region above that is
// 6.5 KB of LDS per wave for the read kernel -- six workgroups per CU instead of five, which is worth 10 % (the
// kernel waits on its probes: DESIGN.md 4.1).
__host__ __device__ static inline int phi_wave_region_u64(int w, int k, bool pos)
{
    const int item_bytes = pos ? 4 : 2;
    return phi_wave_mp_u64(w) + SWW + 2 * SBW + ((phi_wave_items(w, k) + 4) * item_bytes + 7) / 8
#if PHI_ABL == 4
           + 256          // (occupancy experiment: fewer workgroups per CU)
#endif
        ;
}

// minimum of two k-mer values below 2^62 (k <= 31) in one instruction: bit patterns with the two top
// bits clear are non-negative finite doubles (never NaN or infinity), and IEEE order of non-negative
// doubles is the unsigned order of their bit patterns; f64 denormals are kept by the kernels' mode
// register (.amdhsa_float_denorm_mode_16_64 3), so the selected operand comes back unchanged
__device__ __forceinline__ uint64_t min_u62(uint64_t a, uint64_t b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(__longlong_as_double((long long)a)), "v"(__longlong_as_double((long long)b)));
    return (uint64_t)__double_as_longlong(r);
}

// the value one lane below (lane 0 gets `first`): DPP wave_shr:1, no LDS round trip
__device__ __forceinline__ uint64_t wave_prev_u64(uint64_t v, uint64_t first, int lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x138, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x138, 0xF, 0xF, false);
    const uint64_t p = ((uint64_t)hi << 32) | lo;
    return lane == 0 ? first : p;
}

// inclusive prefix sum over the 64 lanes on the VALU (DPP row shifts + row broadcasts; __shfl_up
// would be six ds_bpermute round trips)
__device__ __forceinline__ int wave_scan_inclusive(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);      // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);      // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);      // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);      // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);     // row_bcast:15 into rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);     // row_bcast:31 into rows 2, 3
    return v;
}

// The byte-wise path of one workgroup: chunks blk, blk + n_blk, ... (see phi_sketch_bytes_kernel).
template <int MODE>
static __device__ __forceinline__ void bytes_role(const PhiSketchArgs &A, const unsigned long long *batch_bad,
                                                  int64_t blk, int64_t n_blk, unsigned long long *s_all)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (!A.allslow && batch_bad && *batch_bad == 0) return;
    const int64_t N = A.n_bases;
    const int64_t n_chunks = (N + WCH - 1) / WCH;
    const int64_t n_sw = N / 64 + 2;
    unsigned long long *s_bits = s_all + (size_t)wid * 2 * SBW, *s_bad = s_bits + SBW;
    for (int64_t chunk = blk * (TPB / 64) + wid; chunk < n_chunks; chunk += n_blk * (TPB / 64)) {
        const int64_t c0 = chunk * WCH;
        unsigned long long my_bad = 0;
        wave_sync();
        if (lane < SBW) {
            const int64_t wi = (c0 >> 6) - 1 + lane;
            s_bits[lane] = (wi >= 0 && wi < n_sw) ? A.starts[wi] : 0;
        } else if (lane < 2 * SBW) {
            const int64_t wi = (c0 >> 6) - 1 + (lane - SBW);
            if (A.badbits) my_bad = (wi >= 0 && wi < n_sw) ? A.badbits[wi] : 0;
            s_bad[lane - SBW] = my_bad;
        }
        const bool chunk_bad = __ballot(my_bad != 0) != 0ull;
        wave_sync();
        int n_emit = 0, n_nov = 0;
        if (A.allslow || chunk_bad) {
            const int64_t out_base = (MODE == PHI_MODE_WRITE) ? A.block_off[chunk] : 0;
            if (A.k > PHI_MAX_K_PACKED) slow_windows<MODE, true>(A, c0, chunk, lane, A.k, A.w, s_bits, s_bad, A.allslow != 0, out_base, n_emit, n_nov);
            else slow_windows<MODE>(A, c0, chunk, lane, A.k, A.w, s_bits, s_bad, A.allslow != 0, out_base, n_emit, n_nov);
        }
        if (MODE == PHI_MODE_COUNT) {
            if (lane == 0) A.block_cnt[chunk] = n_emit;
        }
    }
}


// ---- read batches: what used to be a preparation launch, done by the waves of the sketch launch

// This wave's share of emptying the buffers of the previous generation of reads (phi_reset_reads swaps the
// context's double buffers; the generation after this one will fill them again): its hit vector and its striped
// counters -- stores into buffers nothing in this launch reads.  (Until round 3 also the slots that generation had
// filled in a spectrum set, from a log of slots: the set is now made from the log of novel hashes when it is asked
// for, and nothing of it lives across a reset.)
template <class AT>
__device__ __forceinline__ void clean_finish(const AT &A, int64_t gw, int64_t n_waves, int lane)
{
    if (gw == 0 && lane == 0 && A.ov_zero) *A.ov_zero = 0;              // the overflow counter of the generation after this one
    if (A.ipc_mb && A.ipc_need) {
        // a group of processes: the hit vector about to be zeroed may still be read by a peer until this rank's gather
        // ipc_need has ended (phi_ipc.hip) -- it has, long ago, unless a peer lags: then wait (bounded: the gather itself gives up)
        // (relaxed polls: an acquire load would invalidate the XCD's L2 with every poll; the stores below depend on the loop's exit)
        while (__hip_atomic_load(A.ipc_mb + PHI_MB_GATHERED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < A.ipc_need) __builtin_amdgcn_s_sleep(32);
    }
    // (wave-uniform guards: most waves of a large launch have nothing to empty and skip on scalar compares)
    if (gw * 64 < A.q_n_hit_words)
        for (int64_t i = gw * 64 + lane; i < A.q_n_hit_words; i += n_waves * 64) A.q_hit_words[i] = 0;
    if (gw * 64 < A.q_n_stripe_words)
        for (int64_t i = gw * 64 + lane; i < A.q_n_stripe_words; i += n_waves * 64) A.q_stripes[i] = 0;
}

// Read starts of a chunk from the read offsets.  The chunk's bitmap covers bases [c0-64, c0-64+64*SBW); the first
// read starting at or after its first base is found by probing 64 consecutive offsets around position / mean
// read length (one load when reads are of similar lengths), then 64-ary narrowing.
struct StartProbe { int64_t base; int64_t v; int64_t nx; };
__device__ __forceinline__ StartProbe start_probe_issue(const PhiSketchArgs &A, int64_t c0, int lane)
{
    const int64_t lo_b = c0 - 64 > 0 ? c0 - 64 : 0;
    // (a guess: any value is safe, the probe is checked for bracketing the chunk.  Position x reads per base in 0.32
    //  fixed point: wave-uniform integer arithmetic instead of a double division per lane)
    int64_t g = (int64_t)(((unsigned long long)lo_b * A.reads_per_base_q32) >> 32) - 24;
    g = g < 0 ? 0 : (g > A.n_reads - 63 ? (A.n_reads - 63 > 0 ? A.n_reads - 63 : 0) : g);
    StartProbe p;
    p.base = g;
    const int64_t idx = g + lane;
    p.v = idx <= A.n_reads ? A.read_off[idx] : INT64_MAX;              // read_off[n_reads] = n_bases closes the array
    p.nx = idx + 1 <= A.n_reads ? A.read_off[idx + 1] : INT64_MAX;
    return p;
}
__device__ __forceinline__ void set_start_bit(unsigned long long *s_bits, int64_t p, int64_t lo_b)
{
    const int bit = (int)(p - lo_b);
    atomicOr(reinterpret_cast<unsigned int *>(s_bits) + (bit >> 5), 1u << (bit & 31));
}
__device__ __forceinline__ void start_bits_from_offsets(const PhiSketchArgs &A, int64_t c0, int lane, StartProbe pr,
                                                        unsigned long long *s_bits)
{
    const int64_t lo_b = c0 - 64, hi_b = lo_b + 64 * SBW;
    const unsigned long long ge = __ballot(pr.v >= lo_b), lt = __ballot(pr.v < hi_b);
    if ((pr.base == 0 || !(ge & 1ull)) && !(lt >> 63)) {
        // the 64 probed reads bracket the chunk (reads of similar lengths: nearly always): their offsets are all it takes
        if (pr.base + lane < A.n_reads && pr.v >= lo_b && pr.v < hi_b && pr.nx > pr.v) set_start_bit(s_bits, pr.v, lo_b);
        return;
    }
    {
        // reads of uneven lengths (long reads): the guess by mean length was off; correct it by what the probe saw --
        // the distance in bases from its middle offset, over the mean length -- and probe 64 reads there
        int64_t vm = __shfl(pr.v, 32, 64);
        if (vm == INT64_MAX) vm = A.n_bases;
        int64_t nb_all = A.n_bases, nr_all = A.n_reads;
        asm volatile("" : "+s"(nb_all), "+s"(nr_all));    // (not hoisted out of the loop over a wave's chunks: a division kept in registers through every turn)
        const double mean = (double)nb_all / (double)nr_all;
        int64_t g = pr.base + 32 + (int64_t)((double)(lo_b - vm) / mean) - 24;
        g = g < 0 ? 0 : (g > A.n_reads - 63 ? (A.n_reads - 63 > 0 ? A.n_reads - 63 : 0) : g);
        const int64_t idx = g + lane;
        const int64_t v2 = idx <= A.n_reads ? A.read_off[idx] : INT64_MAX;
        const int64_t nx2 = idx + 1 <= A.n_reads ? A.read_off[idx + 1] : INT64_MAX;
        const unsigned long long ge2 = __ballot(v2 >= lo_b), lt2 = __ballot(v2 < hi_b);
        if ((g == 0 || !(ge2 & 1ull)) && !(lt2 >> 63)) {
            if (idx < A.n_reads && v2 >= lo_b && v2 < hi_b && nx2 > v2) set_start_bit(s_bits, v2, lo_b);
            return;
        }
    }
    // first index r0 in [0, n_reads] with read_off[r0] >= lo_b  (read_off[n_reads] = n_bases > lo_b): 64-ary narrowing
    int64_t lo = 0, hi = A.n_reads;
    int64_t base = pr.base, stride = 1, v = pr.v;
    for (int round = 0; round < 64 && lo < hi; round++) {
        if (round) {
            stride = (hi - lo + 63) / 64;
            base = lo;
            const int64_t idx = base + lane * stride;
            v = idx <= A.n_reads ? A.read_off[idx] : INT64_MAX;
        }
        const unsigned long long g2 = __ballot(v >= lo_b);
        const int f = g2 ? __ffsll((long long)g2) - 1 : 64;              // the true lanes are a suffix
        if (f == 0) { hi = base < hi ? base : hi; }
        else {
            const int64_t below = base + (int64_t)(f - 1) * stride;      // read_off[below] < lo_b
            lo = below + 1 > lo ? below + 1 : lo;
            if (f < 64) { const int64_t at = base + (int64_t)f * stride; hi = at < hi ? at : hi; }
        }
    }
    // every read from r0 = lo on that starts below hi_b and owns a base sets its bit
    for (int64_t r = lo + lane;; r += 64) {
        int64_t p = INT64_MAX, nx = INT64_MAX;
        if (r < A.n_reads) { p = A.read_off[r]; nx = A.read_off[r + 1]; }
        if (p >= lo_b && p < hi_b && nx > p) set_start_bit(s_bits, p, lo_b);
        if (__shfl(p, 63, 64) >= hi_b) break;                             // offsets are monotone: nothing further starts here
    }
}

// Reads of ONE length (short-read sets as sequencers write them): no offsets array at all -- read r starts at r * len.  The
// starts inside a chunk's bitmap are the multiples of len in its base range: one division per lane (in double precision,
// corrected), lane j sets the j-th of them.  ~25 instructions and no memory access instead of a probe of 64 offsets.
__device__ __forceinline__ void start_bits_uniform(const PhiSketchArgs &A, int64_t c0, int lane, unsigned long long *s_bits)
{
    const int64_t org = c0 - 64, hi_b = org + 64 * SBW;
    const int64_t from = org > 0 ? org : 0;
    const uint32_t L = (uint32_t)A.uniform_len;
    if (A.n_bases <= 0xFFFFFFFFll) {
        // batches below 4 Gbases (all but whole-genome sets in one batch): the chunk's first base is the same for the whole
        // wave, so the division runs on the SCALAR unit -- a multiply by floor(2^32 / L), one correction -- and a lane adds its
        // multiple of L: no vector instruction but the last few
        const uint32_t x = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)from);
        uint32_t q = __umulhi(x, A.inv_len_q32);               // floor(x / L) or one less
        uint32_t r = x - q * L;
        if (r >= L) { q++; r -= L; }
        const uint32_t first = x + (r ? L - r : 0u);             // the first multiple of L at or after x (may wrap past 2^32: then it is past the batch)
        const uint64_t p = (uint64_t)first + (uint64_t)(uint32_t)lane * (uint64_t)L;
        if (first >= x && (int64_t)p < hi_b && (int64_t)p < A.n_bases) set_start_bit(s_bits, (int64_t)p, org);
        return;
    }
    int64_t q = (int64_t)((double)from * A.inv_len);
    int64_t r = from - q * (int64_t)L;
    if (r < 0) { q--; r += L; }
    if (r >= (int64_t)L) { q++; r -= L; }
    const int64_t p = (q + (r != 0) + lane) * (int64_t)L;       // the (lane)-th multiple of L at or after `from`
    if (p < hi_b && p < A.n_bases) set_start_bit(s_bits, p, org);  // (64 lanes cover the range: L >= 32 > 1024 / 63)
}

// phase 0 of a read chunk: lane -> the 16 bases c0 - 32 + 16 lane .. + 15 as four words ('A' beyond the batch).
// (ONE: phi_sketch_win_kernel's own instance -- the compiler otherwise derives the function's properties from the calls of
// both kernels, and the base-space kernels' code changes with it)
template <int ONE = 0>
__device__ __forceinline__ uint4 load_bases16(const uint8_t *__restrict__ ascii, int64_t N, int64_t c0, int lane)
{
    const int64_t b = c0 - 32 + 16 * (int64_t)lane;
    if (b >= 0 && b + 16 <= N && (((uintptr_t)ascii + (uintptr_t)b) & 15) == 0) return *reinterpret_cast<const uint4 *>(ascii + b);
    uint32_t x[4] = {0x41414141u, 0x41414141u, 0x41414141u, 0x41414141u};
    if (b + 16 > 0 && b < N) {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (b + j >= 0 && b + j < N) x[j >> 2] = (x[j >> 2] & ~(0xFFu << (8 * (j & 3)))) | ((uint32_t)ascii[b + j] << (8 * (j & 3)));
    }
    return make_uint4(x[0], x[1], x[2], x[3]);
}

// ---- read batches of ONE length in WINDOW space (phi_launch_sketch: uniform_len > 0, k <= 32, phi_sketch_win_reads > 0)
// A read of length L has V = L - (k + w - 1) + 1 windows; the base-space kernel (phi_sketch_kernel) spends its lanes on all
// L positions of it (150-bp reads at (31, 25): 96 windows, 150 positions -- a third of phases 2 - 3b on positions that cannot
// be windows).  In window space (phi_sketch_win_kernel, phi_sketch_winfix_kernel) a wave takes R = A.win_reads WHOLE reads: read rl of the wave gets G = ceil(V / Q) lanes, lane j of it the
// read's windows 8j .. 8j + 7 (those past V are masked), and the lanes past R * G idle.  No read starts inside a window,
// so the read-start search and the `blocked` mask go; phase 1 rolls only the read's own L - k + 1 k-mers.
//
// LDS of a wave (phi_win_mp_u64): read rl's k-mers lie in s = G + ceil(w / Q) rows of 9 u64 (8 slots + the pad word SM
// keeps), k-mer t in slot 8 s rl + 1 + t, so that lane j reads its Q + w k-mers at constant offsets from one address, as in
// base space; once they are read, the lanes' minima go to slots 8 lane + i (rows 0 .. 64, the layout phases 4 - 5 and the
// items expect) and the 16-bit items behind them.  The SWW staged words and the SBW bitmap words of bases outside ACGTacgt
// take no room of their own: the staged words lie at the start of the region until every lane has taken its two extracts
// (phase 1), and the bitmap is only needed on the rare path of a wave whose bases are not all ACGTacgt (chunk_bad): there
// it is staged again, from global memory, into a part of the region that is dead at that point (before phase 3 and after
// the rounds).  At L = 150, (31, 25): G = 12, s = 16, R = 5 (480 windows a wave instead of ~330), 5 760 B a wave (768 u64
// with the staging behind the k-mers; base space: 6 560 B) -- seven workgroups of four waves per CU instead of six, so
// that the 6 880 waves of C2 are resident at once.
__host__ __device__ static inline int phi_win_items_u64(int w, int k) { return ((phi_wave_items(w, k) + 4) * 2 + 7) / 8; }
__host__ __device__ static inline int phi_win_mp_u64(int R, int s, int w, int k)
{
    const int kmers = 9 * R * s;                                  // R reads of s rows
    const int minima = 9 * (64 + 1) + phi_win_items_u64(w, k);    // minima of 64 lanes (rows 0 .. 64), then the items
    return kmers > minima ? kmers : minima;
}
__host__ __device__ static inline int phi_win_region_u64(int R, int s, int w, int k) { return phi_win_mp_u64(R, s, w, k); }

// The bitmap of bases outside ACGTacgt for local bits 0 .. 64 SBW (bases c0 - 64 ..), as phase 0 of the base-space kernel
// lays it out: lane < 62 -> bits 64 + 16 lane .. + 15 (its 16 staged bases); the first 32 bits are 0.  Staged again from
// global memory on the rare path that needs it (see phi_win_mp_u64); the caller syncs the wave around it.
__device__ __forceinline__ void stage_bad_bits(const uint8_t *__restrict__ ascii, int64_t N, int64_t c0, int lane,
                                               unsigned long long *s_bad)
{
    uint32_t bad = 0;
    if (lane < 62) {
        const uint4 v = load_bases16<1>(ascii, N, c0, lane);
        const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int b = 0; b < 16; b++) bad |= (uint32_t)(!phi_is_acgt((x[b >> 2] >> (8 * (b & 3))) & 0xFFu)) << b;
    }
    reinterpret_cast<uint16_t *>(s_bad)[lane < 62 ? lane + 2 : lane - 62] = (uint16_t)bad;
}

// The byte-wise routine for the windows of this wave's reads that touch a base outside ACGTacgt (window, or its predecessor:
// the same partition as in base space).  Window q of the wave = window v of read rl: base (r0 + rl) L + v.
__device__ __forceinline__ void slow_windows_reads(const PhiSketchArgs &A, int64_t r0, int nr, int L, int V, int64_t c0, int lane,
                                                   int k, int w, const unsigned long long *s_bad, int &n_emit, int &n_nov)
{
    const int span = w + k - 1, n_win = nr * V;
    for (int q0 = 0; q0 < n_win; q0 += 64) {
        const int q = q0 + lane;
        const int rl = q / V, v = q - rl * V;
        const int64_t a = (r0 + rl) * (int64_t)L + v;
        const int lp = (int)(a - (c0 - 64));                       // local bit of base a
        const bool todo = q < n_win && range_has_bit(s_bad, lp - 1, lp + span - 1);
        bool emit = false;
        uint64_t h = 0;
        if (todo) {
            const KRef best = window_best_bytes(A.ascii, a, k, w);
            h = khash_bytes<false>(A.ascii, best, k);
            if (v == 0) emit = h != PHI_EMPTY_KEY;                   // prev_hash = UINT64_MAX (:383, :455)
            else {
                const KRef prev = window_best_bytes(A.ascii, a - 1, k, w);
                emit = !(prev.pos == best.pos && prev.rc == best.rc) && khash_bytes<false>(A.ascii, prev, k) != h;
            }
        }
        const unsigned long long bal = __ballot(emit);
        const bool novel = emit && probe_table(A, h);
        const OverflowArgs O{A.ov_list, A.ov_count, A.ov_cap, A.err};
        n_nov += overflow_novel(O, novel, h, lane);                   // (straight to the overflow list, as in base space)
        n_emit += __popcll(bal);
    }
}
