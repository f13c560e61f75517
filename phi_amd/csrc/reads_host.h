// reads_host.h -- the rules of the read path that need no GPU, from numbers to small plan structs: how the log of novel read
// hashes, its overflow list and the read-spectrum set are sized, the check of a batch's offsets and the one-length decisions,
// the fixed-point fields of a read launch, the pool's best-fit choice, and the sizes and the host carry of the text stream.
// No HIP include and nothing of the context: dev_mem.hip, read_batches.hip and text_stream.hip act on the plans with HIP
// calls and keep no arithmetic of their own, and host/reads_host_selftest.cpp runs the rules stand-alone under the sanitizers.
// Every result is independent of thread timing.
#pragma once
#include <stddef.h>
#include <string.h>
#include "phi_host_par.h"

static inline uint64_t pow2_at_least(uint64_t x) { uint64_t p = 1; while (p < x) p <<= 1; return p; }

// ------------------------------------------------------------------------------------------ the log of novel hashes
// A batch's part of the log: 1 << nov_shift entries of 8 bytes per chunk, behind the chunks logged so far, and 2 bytes per chunk
// in the count buffer.  A log (or a count buffer) that has no room grows -- keeping what it holds -- to twice its size, up to
// the budget; a log that holds something and would pass the budget is entered into the set first and starts over.  (A batch
// larger than the log has it made as large as the batch.)  A replay writes the entries of the last batch again: the log is
// rewound by that batch's chunks first, so that a replay's plan is that of its first pass.
struct PhiLogPlan {
    int64_t base;              // chunks in the log in front of this batch, the replay's rewind applied (before a flush)
    bool flush_first;          // enter what the log holds into the set and start it over: the batch then begins at chunk 0
    size_t log_bytes, cnt_bytes;   // what the two buffers must hold at least (0, 0: both have room)
    size_t keep_log, keep_cnt;     // of what they hold, the bytes to keep when they grow
};
static inline PhiLogPlan phi_log_plan(int64_t log_chunks, int64_t last_log_chunks, bool replay, int64_t batch_chunks, int32_t nov_shift,
                                      size_t log_cap, size_t cnt_cap, size_t budget)
{
    PhiLogPlan P{};
    P.base = replay ? log_chunks - last_log_chunks : log_chunks;
    const size_t ent = (size_t)8 << nov_shift;
    size_t chunks = (size_t)P.base, need = (chunks + (size_t)batch_chunks) * ent;
    const auto full = [&]() { return need > log_cap || (chunks + (size_t)batch_chunks) * 2 > cnt_cap; };
    if (!full()) return P;
    if (chunks > 0 && need > budget) {
        P.flush_first = true;
        chunks = 0;
        need = (size_t)batch_chunks * ent;
    }
    if (full()) {
        const size_t want = std::max(need, std::min(2 * log_cap, budget));
        P.log_bytes = want; P.cnt_bytes = want / ent * 2 + 64;
        P.keep_log = chunks * ent; P.keep_cnt = chunks * 2;
    }
    return P;
}

// ------------------------------------------------------------------------------------------ the overflow list
// What a batch may send to the list at most: everything it can emit at 1.5x the density of random sequence (2 / (w + 1) per
// base) -- reads full of N, or k > 32, send ALL their novel hashes there.
static inline int64_t phi_ov_batch_bound(int64_t n_bases, int32_t w)
{
    return (int64_t)((double)n_bases * std::min(1.0, 3.0 / (w + 1))) + 16;
}
// the capacity (entries) the list must have under that bound: its own, or -- the bound has passed it -- a larger one
static inline int64_t phi_ov_capacity(int64_t bound, int64_t cap)
{
    return bound > cap ? std::max<int64_t>(std::max<int64_t>(bound, 2 * cap), 1 << 16) : cap;
}
// a list that ran full under a batch that wanted `wanted` entries: everything below the old capacity is valid
struct PhiOvReplay { unsigned long long valid; int64_t cap; };
static inline PhiOvReplay phi_ov_replay(unsigned long long wanted, int64_t cap)
{
    PhiOvReplay R;
    R.valid = std::min<unsigned long long>(wanted, (unsigned long long)cap);
    R.cap = (int64_t)std::max<unsigned long long>(4ull * (unsigned long long)cap, 2 * wanted);
    return R;
}

// ------------------------------------------------------------------------------------------ the read-spectrum set
// capacity of the set for in_set + more keys: a power of two, load factor <= 0.5
static inline uint64_t phi_set_capacity(uint64_t in_set, uint64_t more)
{
    return pow2_at_least(std::max<uint64_t>(1u << 16, 2 * (in_set + more)));
}
// the set of another generation of reads is emptied and used as it is when it is large enough and not much too large
static inline bool phi_set_reusable(uint64_t cap, uint64_t need) { return cap >= need && cap <= 4 * need; }

// ------------------------------------------------------------------------------------------ a batch's offsets
// The first read r of [0, n) whose length off[r + 1] - off[r] is negative (one_length = false) or differs from len
// (one_length = true), -1 when there is none.  Branch-free spans, so that the compiler vectorises them: 33 000 offsets in a
// few microseconds; all host threads from 2^20 offsets up.
template <bool ONE> static inline int phi_offsets_span_bad(const int64_t *off, int64_t lo, int64_t hi, int64_t len)
{
    int bad = 0;
    for (int64_t r = lo; r < hi; r++) bad |= ONE ? (uint64_t)off[r + 1] - (uint64_t)off[r] != (uint64_t)len : off[r + 1] < off[r];
    return bad;
}
static inline int64_t phi_offsets_first_bad(const int64_t *off, int64_t n, bool one_length, int64_t len)
{
    const auto span = [=](int64_t lo, int64_t hi) { return one_length ? phi_offsets_span_bad<true>(off, lo, hi, len) : phi_offsets_span_bad<false>(off, lo, hi, len); };
    int64_t from = 0, to = n;
    if (n < (1 << 20)) {
        if (!span(0, n)) return -1;
    } else {
        std::atomic<int64_t> first{INT64_MAX};               // the lowest piece with an offender
        phi_parallel_chunks(n, (int64_t)1 << 20, [&](int64_t lo, int64_t hi, int) {
            if (!span(lo, hi)) return;
            int64_t seen = first.load();
            while (lo < seen && !first.compare_exchange_weak(seen, lo)) {}
        });
        if (first.load() == INT64_MAX) return -1;
        from = first.load(); to = std::min(n, from + ((int64_t)1 << 20));
    }
    for (int64_t r = from; r < to; r++)
        if (span(r, r + 1)) return r;
    return -1;
}
// phi_add_reads: reads of one length (>= 32) need no offsets on the device.  off[0] = 0 and monotone offsets are checked before.
static inline bool phi_reads_one_length(const int64_t *off, int64_t n_reads)
{
    const int64_t n_bases = off[n_reads], len0 = off[1];
    int64_t all = 0;
    return n_bases > 0 && len0 >= 32 && !__builtin_mul_overflow(len0, n_reads, &all) && all == n_bases &&
           phi_offsets_first_bad(off, n_reads, true, len0) < 0;
}
// phi_add_reads_device without offsets, n_bases a multiple of n_reads: the one length the kernel computes the read starts
// from, or -- shorter than the kernel's arithmetic covers, or absurdly long -- offsets to be made, `step` apart
struct PhiOneLength { int64_t uniform_len; bool make_offsets; int64_t step; };
static inline PhiOneLength phi_device_one_length(int64_t n_reads, int64_t n_bases)
{
    PhiOneLength L;
    L.step = n_bases / n_reads;
    L.make_offsets = L.step < 32 || L.step > 0x7FFFFFFF;
    L.uniform_len = L.make_offsets ? 0 : L.step;
    return L;
}

// ------------------------------------------------------------------------------------------ fixed-point fields of a read launch
static inline uint32_t phi_inv_len_q32(int64_t uniform_len)
{
    return uniform_len ? (uint32_t)(((uint64_t)1 << 32) / (uint64_t)uniform_len) : 0u;
}
// (a guess: clamped, never wrong to round)
static inline uint32_t phi_reads_per_base_q32(int64_t n_reads, int64_t n_bases)
{
    const double q = (double)n_reads / (double)n_bases * 4294967296.0;
    return q >= 2147483648.0 ? 0x80000000u : (uint32_t)q;
}

// ------------------------------------------------------------------------------------------ the pool of large device buffers
// best fit: the smallest of the n capacities in [want, want + want / 8], -1 when there is none
static inline int phi_pool_best_fit(const size_t *cap, int n, size_t want)
{
    int best = -1;
    for (int i = 0; i < n; i++)
        if (cap[i] >= want && cap[i] <= want + want / 8 && (best < 0 || cap[i] < cap[best])) best = i;
    return best;
}

// ------------------------------------------------------------------------------------------ the text stream
// The carry holds what a chunk leaves unfinished: a record at most (the longest reads are a few Mbases, twice that as FASTQ).
// carry_env: the value of PHI_TEXT_CARRY (tests), or null.  A line of a read file is 75 bytes on average, never 16 (then: irregular).
struct PhiTextSizes { uint32_t chunk, carry, line_cap; };
static inline PhiTextSizes phi_text_sizes(int64_t max_chunk_bytes, const char *carry_env)
{
    PhiTextSizes Z;
    Z.chunk = (uint32_t)std::min<int64_t>(std::max<int64_t>(max_chunk_bytes, 64), (int64_t)1 << 28);
    Z.carry = carry_env ? (uint32_t)std::max<long long>(64, atoll(carry_env)) & ~15u : std::max<uint32_t>(Z.chunk / 2, 1u << 24);
    Z.line_cap = (Z.carry + Z.chunk) / 16 + 1024;
    return Z;
}
// the bytes a piece (m bytes at p) leaves untaken, on the host: the last `tail` bytes of (carry before + this piece)
static inline void phi_text_carry_update(std::vector<char> &carry, const char *p, uint32_t m, uint32_t tail)
{
    if (tail == 0) carry.clear();
    else if (tail <= m) carry.assign(p + m - tail, p + m);
    else {
        const size_t keep = tail - m;                        // of the carry before
        carry.erase(carry.begin(), carry.end() - (ptrdiff_t)keep);
        carry.insert(carry.end(), p, p + m);
    }
}
