// deflate_codes.h -- the parts of a DEFLATE writer (RFC 1951) that are plain code: length-limited prefix codes from a histogram,
// the run-length coding of code lengths (symbols 16 / 17 / 18), canonical codes, the length and distance symbols; the CRC32
// shift comes with them, from crc32_shift.h.  __host__ __device__: the compressor's kernel (deflate.hip) calls them from single
// lanes, host/deflate_codes_selftest.cpp calls them on the CPU.  Every loop is bounded by the alphabet size (at most DFL_MAX_SYMS) or by a constant.
#pragma once
#include <stdint.h>
#include "crc32_shift.h"        // DFL_HD, dfl_crc_mul, dfl_crc_shift

#define DFL_NLIT 286            // literal/length symbols that may be coded
#define DFL_NDIST 30
#define DFL_NCL 19
#define DFL_MAX_SYMS 288
#define DFL_MIN_MATCH 3
#define DFL_MAX_MATCH 258
#define DFL_WINDOW 32768

// ------------------------------------------------------------------------------------------------ symbols of copies

DFL_HD int dfl_log2(uint32_t v)   // floor(log2 v), v >= 1
{
    int r = 0;
    for (int s = 16; s >= 1; s >>= 1)
        if (v >> s) { v >>= s; r += s; }
    return r;
}

// length 3..258 -> literal/length symbol 257..285, the number of its extra bits and their value (RFC 1951 3.2.5: eight
// lengths without extra bits, then four symbols for each count of extra bits 1..5, then 258 alone)
DFL_HD int dfl_length_symbol(int len, int *nextra, int *extra)
{
    const int l = len - 3;
    if (l < 8) { *nextra = 0; *extra = 0; return 257 + l; }
    if (len == 258) { *nextra = 0; *extra = 0; return 285; }
    const int e = dfl_log2((uint32_t)l) - 2;
    *nextra = e;
    *extra = l & ((1 << e) - 1);
    return 257 + 4 * e + 4 + ((l >> e) & 3);
}

// distance 1..32768 -> distance symbol 0..29 (four without extra bits, then two for each count 1..13)
DFL_HD int dfl_dist_symbol(int dist, int *nextra, int *extra)
{
    const int d = dist - 1;
    if (d < 4) { *nextra = 0; *extra = 0; return d; }
    const int e = dfl_log2((uint32_t)d) - 1;
    *nextra = e;
    *extra = d & ((1 << e) - 1);
    return 2 * e + 2 + ((d >> e) & 1);
}

// ------------------------------------------------------------------------------------------------ code lengths

// Workspace of dfl_build_lengths (the caller's: LDS in the kernel)
struct DflWork {
    uint32_t key[DFL_MAX_SYMS];     // (count << 9) | symbol of the used symbols, sorted ascending
    uint32_t a[DFL_MAX_SYMS];       // in-place code-length computation over the sorted counts
};

// Code lengths len[0..n) of a prefix code for the counts freq[0..n), no length above `limit` (n <= DFL_MAX_SYMS, counts below
// 2^22, 2^limit >= the number of used symbols).  No used symbol: all zero.  One: that symbol gets length 1 (the caller decides
// whether a second code must stand beside it).  Two or more: a complete code, Kraft sum exactly 1.
// The lengths are Huffman's (Moffat and Katajainen's in-place computation over the sorted counts); where the deepest leaf
// exceeds the limit, the leaves beyond it move up to the limit and the count of codes per length is repaired from the longest
// lengths down until the Kraft sum is 1 again; lengths then go to the symbols by descending count, so a rarer symbol never gets
// a shorter code.  Ties in the counts break by symbol: the result is a function of the histogram alone.
// Returns the depth of the unlimited code (what the limit had to cut).
DFL_HD int dfl_build_lengths(const uint32_t *freq, int n, int limit, uint8_t *len, DflWork *w)
{
    int m = 0;
    for (int s = 0; s < n; s++) {
        len[s] = 0;
        if (freq[s]) w->key[m++] = (freq[s] << 9) | (uint32_t)s;
    }
    if (m == 0) return 0;
    if (m == 1) { len[w->key[0] & 511] = 1; return 1; }
    // shell sort (gaps 3h + 1), ascending
    int gap = 1;
    while (gap < m / 3) gap = 3 * gap + 1;
    for (; gap >= 1; gap /= 3)
        for (int i = gap; i < m; i++) {
            const uint32_t k = w->key[i];
            int j = i;
            for (; j >= gap && w->key[j - gap] > k; j -= gap) w->key[j] = w->key[j - gap];
            w->key[j] = k;
        }
    uint32_t *A = w->a;
    for (int i = 0; i < m; i++) A[i] = w->key[i] >> 9;
    // phase 1: internal nodes' weights, then parent indices, in place
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < m - 1; next++) {
        if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; }
        else A[next] = A[leaf++];
        if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; }
        else A[next] += A[leaf++];
    }
    // phase 2: depths of the internal nodes
    A[m - 2] = 0;
    for (int next = m - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
    // phase 3: depths of the leaves, A[i] for the i-th smallest count (non-increasing in i)
    {
        int avbl = 1, used = 0, dpth = 0, rt = m - 2, next = m - 1;
        while (avbl > 0) {
            while (rt >= 0 && (int)A[rt] == dpth) { used++; rt--; }
            while (avbl > used) { A[next--] = (uint32_t)dpth; avbl--; }
            avbl = 2 * used;
            dpth++;
            used = 0;
        }
    }
    const int depth = (int)A[0];
    // codes per length, the overlong ones at the limit
    int cnt[33];
    for (int l = 0; l <= 32; l++) cnt[l] = 0;
    for (int i = 0; i < m; i++) cnt[(int)A[i] > limit ? limit : (int)A[i]]++;
    if (depth > limit) {
        uint32_t total = 0;                                            // Kraft sum in units of 2^-limit
        for (int l = 1; l <= limit; l++) total += (uint32_t)cnt[l] << (limit - l);
        for (int guard = 0; total > (1u << limit) && guard < DFL_MAX_SYMS; guard++) {
            // one code leaves the limit; the deepest shorter leaf takes a sibling there: the sum falls by exactly one unit
            cnt[limit]--;
            for (int l = limit - 1; l >= 1; l--)
                if (cnt[l]) { cnt[l]--; cnt[l + 1] += 2; break; }
            total--;
        }
    }
    // the rarest symbols take the longest codes
    int i = 0;
    for (int l = limit; l >= 1; l--)
        for (int c = 0; c < cnt[l]; c++) len[w->key[i++] & 511] = (uint8_t)l;
    return depth;
}

// Canonical codes of RFC 1951 3.2.2, each reversed so that it goes out least significant bit first like every other field
DFL_HD void dfl_canonical_codes(const uint8_t *len, int n, uint16_t *code)
{
    int cnt[16], next[16];
    for (int l = 0; l < 16; l++) cnt[l] = 0;
    for (int s = 0; s < n; s++) cnt[len[s]]++;
    cnt[0] = 0;
    int c = 0;
    next[0] = 0;
    for (int l = 1; l < 16; l++) { c = (c + cnt[l - 1]) << 1; next[l] = c; }
    for (int s = 0; s < n; s++) {
        const int l = len[s];
        uint32_t v = l ? (uint32_t)next[l]++ : 0, r = 0;
        for (int k = 0; k < l; k++) { r = (r << 1) | (v & 1); v >>= 1; }
        code[s] = (uint16_t)r;
    }
}

// The code lengths seq[0..n) as code-length symbols: sym[k] in 0..18, extra[k] the value of its extra bits (16: 2 bits,
// repeat the last length 3..6 times; 17: 3 bits, 3..10 zeros; 18: 7 bits, 11..138 zeros).  Greedy: the longest repeat first.
// Returns the number of symbols (at most n).
DFL_HD int dfl_rle_lengths(const uint8_t *seq, int n, uint8_t *sym, uint8_t *extra)
{
    int k = 0;
    for (int i = 0; i < n;) {
        const int v = seq[i];
        int run = 1;
        while (i + run < n && seq[i + run] == v) run++;
        if (v == 0 && run >= 3) {
            const int r = run > 138 ? 138 : run;
            if (r <= 10) { sym[k] = 17; extra[k] = (uint8_t)(r - 3); }
            else { sym[k] = 18; extra[k] = (uint8_t)(r - 11); }
            k++;
            i += r;
        } else if (i > 0 && seq[i - 1] == v && run >= 3) {
            const int r = run > 6 ? 6 : run;
            sym[k] = 16; extra[k] = (uint8_t)(r - 3);
            k++;
            i += r;
        } else {
            sym[k] = (uint8_t)v; extra[k] = 0;
            k++;
            i++;
        }
    }
    return k;
}

DFL_HD int dfl_cl_extra_bits(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }
