// table.hip -- open-addressed hash tables in HBM (linear probing, 64-bit keys, atomicCAS).
//
// Replaces the reference's std::map<uint64_t,int32_t> Sp_R (src/ILP_index.cpp:616-635) and the
// per-minimiser std::map::find of compute_anchors (:495-526).  Roles are swapped with respect to
// the reference so that reads can stream and shard across GPUs: the table is built once from
// the walk minimisers (the "index"), reads probe it; a second set holds the distinct read
// hashes only to report |Sp_R| (:641).
#include <hip/hip_runtime.h>
#include "phi_dev.h"
#include "phi_kernels.h"
#include "phi_wave.h"

__global__ void phi_fill_u64_kernel(uint64_t *p, int64_t n, uint64_t v)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = v;
}
__global__ void phi_fill_u32_kernel(uint32_t *p, int64_t n, uint32_t v)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = v;
}

static inline unsigned grid_for(int64_t n, int tpb)
{
    int64_t nb = (n + tpb - 1) / tpb;
    if (nb > 256 * 16) nb = 256 * 16;        // grid-stride beyond 16 workgroups per CU
    if (nb < 1) nb = 1;
    return (unsigned)nb;
}

// The read table (phi_kernels.h phi_launch_read_table): every slot empty, every id and flag word 0
__global__ void __launch_bounds__(256) phi_read_table_clear_kernel(ulonglong2 *__restrict__ rt, int64_t n_slots)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * blockDim.x)
        rt[i] = make_ulonglong2(PHI_EMPTY_KEY, 0ull);
}
// One lane per slot of the walk-minimiser table that holds a key: the first free slot from its home bucket on (slot 0 of a
// bucket before slot 1, so a bucket with a free slot has its slot 1 free), then its id; a key that lands past its home
// flags the home bucket.  Ids and flags share a word and are both OR-ed in: no order between the lanes matters.
__global__ void __launch_bounds__(256) phi_read_table_insert_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ uid,
                                                                    int64_t cap, unsigned long long *__restrict__ rt, uint64_t bmask,
                                                                    uint32_t *__restrict__ err)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i];
        if (key == PHI_EMPTY_KEY) continue;
        const uint64_t home = key & bmask;
        uint64_t b = home;
        int probes = 0;
        for (;;) {
            unsigned long long *s = rt + 4 * b;
            if (atomicCAS(&s[0], PHI_EMPTY_KEY, key) == PHI_EMPTY_KEY) { atomicOr(&s[1], (unsigned long long)uid[i]); break; }
            if (atomicCAS(&s[2], PHI_EMPTY_KEY, key) == PHI_EMPTY_KEY) { atomicOr(&s[3], (unsigned long long)uid[i]); break; }
            b = (b + 1) & bmask;
            if (++probes > PHI_MAX_PROBE) { atomicOr(err, PHI_KERR_TABLE_FULL); break; }
        }
        if (b != home) atomicOr(&rt[4 * home + 1], (unsigned long long)PHI_RT_OVERFLOWED << 32);
    }
}

void phi_launch_read_table(hipStream_t st, const uint64_t *keys, const uint32_t *uid, int64_t cap, uint64_t *rt,
                           int64_t n_buckets, uint32_t *err)
{
    if (n_buckets > 0)
        hipLaunchKernelGGL(phi_read_table_clear_kernel, dim3(grid_for(2 * n_buckets, 256)), dim3(256), 0, st, (ulonglong2 *)rt,
                           2 * n_buckets);
    if (cap > 0 && n_buckets > 0)
        hipLaunchKernelGGL(phi_read_table_insert_kernel, dim3(grid_for(cap, 256)), dim3(256), 0, st, keys, uid, cap,
                           (unsigned long long *)rt, (uint64_t)n_buckets - 1, err);
}

void phi_launch_fill_u64(hipStream_t st, uint64_t *p, int64_t n, uint64_t v)
{
    if (n > 0) hipLaunchKernelGGL(phi_fill_u64_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, p, n, v);
}
__global__ void phi_iota_i64_kernel(int64_t *p, int64_t n, int64_t step)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = i * step;
}
void phi_launch_iota_i64(hipStream_t st, int64_t *p, int64_t n, int64_t step)
{
    if (n > 0) hipLaunchKernelGGL(phi_iota_i64_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, p, n, step);
}

void phi_launch_fill_u32(hipStream_t st, uint32_t *p, int64_t n, uint32_t v)
{
    if (n > 0) hipLaunchKernelGGL(phi_fill_u32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, p, n, v);
}

__global__ void __launch_bounds__(256) phi_table_build_kernel(const uint64_t *__restrict__ rec_hash, int64_t n_rec,
                                                              uint64_t *__restrict__ u_keys,
                                                              uint32_t *__restrict__ u_rep, uint64_t u_mask,
                                                              uint32_t *__restrict__ rec_slot,
                                                              uint32_t *__restrict__ err)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rec;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t h = rec_hash[i];
        if (h == PHI_EMPTY_KEY) { atomicOr(err, PHI_KERR_SENTINEL); rec_slot[i] = 0; continue; }
        uint64_t slot = h & u_mask;
        int probes = 0;
        for (;;) {
            // the walks of a pangenome share most minimisers: look before the atomic (a key, once
            // written, never changes)
            unsigned long long prev = __builtin_nontemporal_load((const unsigned long long *)&u_keys[slot]);
            if (prev == PHI_EMPTY_KEY) prev = atomicCAS((unsigned long long *)&u_keys[slot], PHI_EMPTY_KEY, h);
            if (prev == PHI_EMPTY_KEY || prev == h) break;
            slot = (slot + 1) & u_mask;
            if (++probes > PHI_MAX_PROBE) { atomicOr(err, PHI_KERR_TABLE_FULL); break; }
        }
        // smallest record index: same on every rank.  The stored value only falls, so a record that
        // sees a smaller one already there has nothing to add
        if (__builtin_nontemporal_load(&u_rep[slot]) > (uint32_t)i) atomicMin(&u_rep[slot], (uint32_t)i);
        rec_slot[i] = (uint32_t)slot;
    }
}

void phi_launch_table_build(hipStream_t st, const uint64_t *rec_hash, int64_t n_rec, uint64_t *u_keys,
                            uint32_t *u_rep, uint64_t u_mask, uint32_t *rec_slot, uint32_t *err)
{
    if (n_rec > 0)
        hipLaunchKernelGGL(phi_table_build_kernel, dim3(grid_for(n_rec, 256)), dim3(256), 0, st, rec_hash, n_rec,
                           u_keys, u_rep, u_mask, rec_slot, err);
}

// flags[i] = record i is the representative (first record) of its hash
__global__ void __launch_bounds__(256) phi_rep_flags_kernel(const uint32_t *__restrict__ rec_slot, int64_t n_rec,
                                                            const uint32_t *__restrict__ u_rep,
                                                            uint8_t *__restrict__ flags)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += (int64_t)gridDim.x * blockDim.x)
        flags[i] = u_rep[rec_slot[i]] == (uint32_t)i;
}
// dense minimiser ids: uid = rank of the representative record in position order, identical on
// every rank because the records are
__global__ void __launch_bounds__(256) phi_slot_uid_kernel(const int32_t *__restrict__ rep_list, int64_t n_unique,
                                                           const uint32_t *__restrict__ rec_slot,
                                                           uint32_t *__restrict__ u_uid)
{
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_unique; j += (int64_t)gridDim.x * blockDim.x)
        u_uid[rec_slot[rep_list[j]]] = (uint32_t)j;
}
void phi_launch_rep_flags(hipStream_t st, const uint32_t *rec_slot, int64_t n_rec, const uint32_t *u_rep,
                          uint8_t *flags)
{
    if (n_rec > 0)
        hipLaunchKernelGGL(phi_rep_flags_kernel, dim3(grid_for(n_rec, 256)), dim3(256), 0, st, rec_slot, n_rec, u_rep,
                           flags);
}
void phi_launch_slot_uid(hipStream_t st, const int32_t *rep_list, int64_t n_unique, const uint32_t *rec_slot,
                         uint32_t *u_uid)
{
    if (n_unique > 0)
        hipLaunchKernelGGL(phi_slot_uid_kernel, dim3(grid_for(n_unique, 256)), dim3(256), 0, st, rep_list, n_unique,
                           rec_slot, u_uid);
}

// The table phi_table_build makes is sized by the RECORDS (every walk repeats most minimisers):
// 2^26 slots for ~10^6 distinct keys at C2, 768 MB that every read probe walks into at random.
// Once the distinct keys are known they are re-inserted into a table sized by THEM (load <= 0.25,
// 32 MB at C2: cache resident) and every record looks its new slot up.
__global__ void __launch_bounds__(256) phi_table_compact_insert_kernel(const int32_t *__restrict__ rep_list, int64_t n_unique,
                                                                       const uint64_t *__restrict__ rec_hash,
                                                                       uint64_t *__restrict__ keys, uint32_t *__restrict__ uid,
                                                                       uint64_t mask, uint32_t *__restrict__ err)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_unique; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t h = rec_hash[rep_list[i]];
        uint64_t slot = h & mask;
        int probes = 0;
        for (;;) {
            const unsigned long long prev = atomicCAS((unsigned long long *)&keys[slot], PHI_EMPTY_KEY, h);
            if (prev == PHI_EMPTY_KEY) break;                  // the keys are distinct
            slot = (slot + 1) & mask;
            if (++probes > PHI_MAX_PROBE) { atomicOr(err, PHI_KERR_TABLE_FULL); break; }
        }
        uid[slot] = (uint32_t)i;
    }
}

__global__ void __launch_bounds__(256) phi_table_lookup_kernel(const uint64_t *__restrict__ rec_hash, int64_t n_rec,
                                                               const uint64_t *__restrict__ keys, uint64_t mask,
                                                               uint32_t *__restrict__ rec_slot, uint32_t *__restrict__ err)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t h = rec_hash[i];
        uint64_t slot = h & mask;
        int probes = 0;
        while (keys[slot] != h) {
            slot = (slot + 1) & mask;
            if (++probes > PHI_MAX_PROBE) { atomicOr(err, PHI_KERR_TABLE_FULL); break; }
        }
        rec_slot[i] = (uint32_t)slot;
    }
}

void phi_launch_table_compact(hipStream_t st, const int32_t *rep_list, int64_t n_unique, const uint64_t *rec_hash, int64_t n_rec,
                              uint64_t *keys, uint32_t *uid, uint64_t mask, uint32_t *rec_slot, uint32_t *err)
{
    if (n_unique > 0)
        hipLaunchKernelGGL(phi_table_compact_insert_kernel, dim3(grid_for(n_unique, 256)), dim3(256), 0, st, rep_list, n_unique,
                           rec_hash, keys, uid, mask, err);
    if (n_rec > 0)
        hipLaunchKernelGGL(phi_table_lookup_kernel, dim3(grid_for(n_rec, 256)), dim3(256), 0, st, rec_hash, n_rec, keys, mask,
                           rec_slot, err);
}

// hist[c] += 1 for every slot of the table that holds a key and occurs in c walks
__global__ void __launch_bounds__(256) phi_share_hist_kernel(const uint64_t *__restrict__ keys, int64_t cap,
                                                             const int32_t *__restrict__ n_walks_of,
                                                             unsigned long long *__restrict__ hist)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (int64_t)gridDim.x * blockDim.x)
        if (keys[s] != PHI_EMPTY_KEY) atomicAdd(&hist[n_walks_of[s]], 1ull);
}

void phi_launch_share_hist(hipStream_t st, const uint64_t *keys, int64_t cap, const int32_t *n_walks_of, unsigned long long *hist)
{
    if (cap > 0)
        hipLaunchKernelGGL(phi_share_hist_kernel, dim3(grid_for(cap, 256)), dim3(256), 0, st, keys, cap, n_walks_of, hist);
}

// u_keys != nullptr: a hash found in the walk-minimiser table sets its hit flag instead (the set holds
// only hashes absent from the table, see probe_tables in sketch.hip)
__global__ void __launch_bounds__(256) phi_spectrum_insert_kernel(const uint64_t *__restrict__ hashes, int64_t n,
                                                                  uint64_t *__restrict__ sp_keys, uint64_t sp_mask,
                                                                  unsigned long long *__restrict__ sp_count,
                                                                  const uint64_t *__restrict__ u_keys, uint64_t u_mask,
                                                                  const uint32_t *__restrict__ u_uid, uint8_t *__restrict__ hit,
                                                                  uint32_t *__restrict__ err)
{
    int n_new = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t h = hashes[i];
        if (h == PHI_EMPTY_KEY) continue;
        if (u_keys) {
            bool found = false;
            uint64_t su = h & u_mask;
            for (int probes = 0; probes <= PHI_MAX_PROBE; probes++) {
                const uint64_t key = u_keys[su];
                if (key == h) { hit[u_uid[su]] = 1; found = true; break; }
                if (key == PHI_EMPTY_KEY) break;
                su = (su + 1) & u_mask;
            }
            if (found) continue;
        }
        uint64_t slot = h & sp_mask;
        int probes = 0;
        for (;;) {
            const unsigned long long prev = atomicCAS((unsigned long long *)&sp_keys[slot], PHI_EMPTY_KEY, h);
            if (prev == PHI_EMPTY_KEY) { n_new++; break; }
            if (prev == h) break;
            slot = (slot + 1) & sp_mask;
            if (++probes > PHI_MAX_PROBE) { atomicOr(err, PHI_KERR_TABLE_FULL); break; }
        }
    }
    n_new = phi_wave_sum(n_new);
    if ((threadIdx.x & 63) == 0 && n_new)
        atomicAdd(sp_count + (size_t)((blockIdx.x * 4 + (threadIdx.x >> 6)) & (PHI_STRIPES - 1)) * 8, (unsigned long long)n_new);
}

void phi_launch_spectrum_insert(hipStream_t st, const uint64_t *hashes, int64_t n, uint64_t *sp_keys,
                                uint64_t sp_mask, unsigned long long *sp_count, const uint64_t *u_keys, uint64_t u_mask,
                                const uint32_t *u_uid, uint8_t *hit, uint32_t *err)
{
    if (n > 0)
        hipLaunchKernelGGL(phi_spectrum_insert_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, hashes, n, sp_keys,
                           sp_mask, sp_count, u_keys, u_mask, u_uid, hit, err);
}

// The read-spectrum set from the log of novel hashes (sketch.hip): thread -> entry (chunk, i); every lane of a wave
// that holds a logged hash inserts it, the wave adds its new entries to a striped counter.  All lanes of the launch are
// inserts (in the sketch kernel an insert was a lane's second dependent round trip behind its table probe).
// A chunk tagged PHI_NOV_KMERS (a clean wave of phi_sketch_winfix_kernel, sketch_rounds_kmer.inc) holds the novel K-MERS:
// their MurmurHash3 is taken here, once per read set, and phi_kmer_flush_rule (phi_dev.h) decides: the hash enters the set
// unless it is the sentinel, a walk minimiser's hash (u_keys: the walk-minimiser table) or the hash of another k-mer in
// the entry before (the lane below: entry i - 1 of the chunk, i > 0; lane 0 loads and hashes it).
__global__ void __launch_bounds__(256) phi_spectrum_flush_kernel(const uint64_t *__restrict__ nov_log, const uint16_t *__restrict__ nov_cnt,
                                                                 int64_t c_lo, int64_t n_ent, int32_t shift,
                                                                 uint64_t *__restrict__ sp_keys, uint64_t sp_mask,
                                                                 unsigned long long *__restrict__ sp_count, int32_t k,
                                                                 const uint64_t *__restrict__ u_keys, uint64_t u_mask, uint32_t *__restrict__ err)
{
    int n_new = 0;
    const int lane = threadIdx.x & 63;
    // (whole waves take every turn: the lanes past n_ent hold nothing, the shuffle below needs them there)
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); t0 < n_ent; t0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = t0 + lane;
        bool have = false, kmers = false;
        int i = 0;
        int64_t c = 0;
        uint64_t h = 0, v = 0;
        if (t < n_ent) {
            c = c_lo + (t >> shift);
            i = (int)(t & ((1 << shift) - 1));
            const uint32_t cnt = nov_cnt[c];
            kmers = (cnt & PHI_NOV_KMERS) != 0;
            have = i < (int)(cnt & (PHI_NOV_KMERS - 1));
            if (have) {
                h = __builtin_nontemporal_load(&nov_log[(c << shift) + i]);
                if (kmers) { v = h; h = phi_kmer_hash(v, k); }
            }
        }
        // entry i - 1 of the same chunk is the lane below (a chunk's entries are consecutive threads; i > 0 and lane > 0)
        uint64_t hp = __shfl_up(h, 1, 64), vp = __shfl_up(v, 1, 64);
        if (have && kmers) {
            if (lane == 0 && i > 0) { vp = nov_log[(c << shift) + i - 1]; hp = phi_kmer_hash(vp, k); }
            bool in_walks = false;
            if (h != PHI_EMPTY_KEY) {
                uint64_t su = h & u_mask;
                for (int probes = 0; probes <= PHI_MAX_PROBE; probes++) {
                    const uint64_t key = u_keys[su];
                    if (key == h) { in_walks = true; break; }
                    if (key == PHI_EMPTY_KEY) break;
                    su = (su + 1) & u_mask;
                }
            }
            const uint32_t e = phi_kmer_flush_rule(h, v, i > 0, hp, vp, in_walks);
            if (e) { atomicOr(err, e); have = false; }
        }
        if (!have) continue;
        uint64_t slot = h & sp_mask;
        int probes = 0;
        for (;;) {
            const unsigned long long prev = atomicCAS((unsigned long long *)&sp_keys[slot], PHI_EMPTY_KEY, h);
            if (prev == PHI_EMPTY_KEY) { n_new++; break; }
            if (prev == h) break;
            slot = (slot + 1) & sp_mask;
            if (++probes > PHI_MAX_PROBE) { atomicOr(err, PHI_KERR_TABLE_FULL); break; }
        }
    }
    n_new = phi_wave_sum(n_new);
    if ((threadIdx.x & 63) == 0 && n_new)
        atomicAdd(sp_count + (size_t)((blockIdx.x * 4 + (threadIdx.x >> 6)) & (PHI_STRIPES - 1)) * 8, (unsigned long long)n_new);
}

void phi_launch_spectrum_flush(hipStream_t st, const uint64_t *nov_log, const uint16_t *nov_cnt, int64_t c_lo, int64_t c_hi, int32_t shift,
                               uint64_t *sp_keys, uint64_t sp_mask, unsigned long long *sp_count, int32_t k, const uint64_t *u_keys,
                               uint64_t u_mask, uint32_t *err)
{
    const int64_t n_ent = (c_hi - c_lo) << shift;
    if (n_ent > 0)
        hipLaunchKernelGGL(phi_spectrum_flush_kernel, dim3(grid_for(n_ent, 256)), dim3(256), 0, st, nov_log, nov_cnt, c_lo, n_ent, shift,
                           sp_keys, sp_mask, sp_count, k, u_keys, u_mask, err);
}

// The k-mer keys of the walk minimisers (phi_kernels.h phi_launch_kmer_keys): one lane per class record.  The record's
// k-mer from the class-space text -- 32 bases from its first one, the k-mer's strand by value as the sketch takes it --,
// checked against the hash the sketch gave the record, then entered under the record's table slot: every record of a slot
// must bring the same k-mer.
__global__ void __launch_bounds__(256) phi_kmer_keys_kernel(const int32_t *__restrict__ rec_cls, const int32_t *__restrict__ rec_rel,
                                                            const uint64_t *__restrict__ rec_hash, const uint32_t *__restrict__ rec_slot,
                                                            int64_t n_rec, const int64_t *__restrict__ cls_base, const uint8_t *__restrict__ cls_left,
                                                            const uint64_t *__restrict__ words, const uint32_t *__restrict__ badbits, int32_t k,
                                                            uint64_t *__restrict__ kkeys, unsigned long long *__restrict__ ctr)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = rec_cls[i];
        const int64_t p = cls_base[c] + cls_left[c] + rec_rel[i];
        const int64_t wi = p >> 5;
        const int s = (int)(p & 31);
        const uint64_t bad = (((uint64_t)badbits[wi + 1] << 32) | badbits[wi]) >> s;      // bit j: base p + j (s + k <= 62)
        if (bad & ((1ull << k) - 1)) { atomicAdd(&ctr[0], 1ull); continue; }
        const uint64_t f = phi_extract64(words, p) >> (64 - 2 * k), r = phi_revcomp(f, k);
        const uint64_t v = f < r ? f : r;
        if (phi_kmer_hash(v, k) != rec_hash[i]) { atomicAdd(&ctr[1], 1ull); continue; }
        const uint64_t key = phi_kmer_mix(v);
        unsigned long long *slot = (unsigned long long *)&kkeys[rec_slot[i]];
        unsigned long long prev = __builtin_nontemporal_load(slot);
        if (prev == PHI_EMPTY_KEY) prev = atomicCAS(slot, PHI_EMPTY_KEY, key);
        if (prev != PHI_EMPTY_KEY && prev != key) atomicAdd(&ctr[2], 1ull);
    }
}
void phi_launch_kmer_keys(hipStream_t st, const int32_t *rec_cls, const int32_t *rec_rel, const uint64_t *rec_hash, const uint32_t *rec_slot,
                          int64_t n_rec, const int64_t *cls_base, const uint8_t *cls_left, const uint64_t *words, const uint32_t *badbits,
                          int32_t k, uint64_t *kkeys, unsigned long long *ctr)
{
    if (n_rec > 0)
        hipLaunchKernelGGL(phi_kmer_keys_kernel, dim3(grid_for(n_rec, 256)), dim3(256), 0, st, rec_cls, rec_rel, rec_hash, rec_slot, n_rec,
                           cls_base, cls_left, words, badbits, k, kkeys, ctr);
}

__global__ void __launch_bounds__(256) phi_rt_overflowed_kernel(const uint64_t *__restrict__ rt, int64_t n_buckets,
                                                                unsigned long long *__restrict__ n_out)
{
    int cnt = 0;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_buckets; b += (int64_t)gridDim.x * blockDim.x)
        cnt += (int)((rt[4 * b + 1] >> 32) & PHI_RT_OVERFLOWED);
    cnt = phi_wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_out, (unsigned long long)cnt);
}
void phi_launch_rt_overflowed(hipStream_t st, const uint64_t *rt, int64_t n_buckets, unsigned long long *n_out)
{
    if (n_buckets > 0)
        hipLaunchKernelGGL(phi_rt_overflowed_kernel, dim3(grid_for(n_buckets, 256)), dim3(256), 0, st, rt, n_buckets, n_out);
}

// number of set hit flags (bytes != 0), added to *n_out
__global__ void __launch_bounds__(256) phi_count_flags_kernel(const uint8_t *__restrict__ flags, int64_t n,
                                                              unsigned long long *__restrict__ n_out)
{
    int cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        cnt += flags[i] != 0;
    cnt = phi_wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_out, (unsigned long long)cnt);
}

void phi_launch_count_flags(hipStream_t st, const uint8_t *flags, int64_t n, unsigned long long *n_out)
{
    if (n > 0) hipLaunchKernelGGL(phi_count_flags_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, flags, n, n_out);
}

__global__ void __launch_bounds__(256) phi_spectrum_export_kernel(const uint64_t *__restrict__ sp_keys, int64_t cap,
                                                                  uint64_t *__restrict__ out,
                                                                  unsigned long long *__restrict__ n_out)
{
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < cap; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        const uint64_t key = i < cap ? sp_keys[i] : PHI_EMPTY_KEY;
        const bool occ = key != PHI_EMPTY_KEY;
        const unsigned long long bal = __ballot(occ);
        const int lane = threadIdx.x & 63;
        unsigned long long base = 0;
        if (lane == 0 && bal) base = atomicAdd(n_out, (unsigned long long)__popcll(bal));
        base = __shfl(base, 0, 64);
        if (occ) out[base + __popcll(bal & ((1ull << lane) - 1))] = key;
    }
}

void phi_launch_spectrum_export(hipStream_t st, const uint64_t *sp_keys, int64_t cap, uint64_t *out,
                                unsigned long long *n_out)
{
    if (cap > 0)
        hipLaunchKernelGGL(phi_spectrum_export_kernel, dim3(grid_for(cap, 256)), dim3(256), 0, st, sp_keys, cap, out,
                           n_out);
}

// One empty launch loads this translation unit's code object onto the device: the HIP runtime does that lazily, at the
// first launch of any of its kernels (0.5-1.3 ms per unit, measured inside phi_set_graph / phi_solve before
// phi_ctx_create did it up front).
__global__ void phi_warm_table_kernel() {}
void phi_warm_table(hipStream_t st) { hipLaunchKernelGGL(phi_warm_table_kernel, dim3(1), dim3(64), 0, st); }
