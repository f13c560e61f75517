// text_bytes.h -- the byte-level idioms of the kernels that read text sixteen bytes per lane (reads_text.hip, walk_text.hip,
// gfa_text.hip, vcf.hip, bgzf_index.hip with vcf_lines_dev.h, vcf_region.hip): which bytes equal a character, which of a
// lane's bytes lie inside a window, the 16-byte loads, sixteen bytes from an unaligned address, and the bisection of an ascending
// list.  One copy, so that a lane border, a tile border and the end of the text are looked at once.
//
// Everything that is integer arithmetic is plain code (host and device): csrc/host/text_bytes_selftest.cpp checks it against
// byte-at-a-time code.  The loads are device code.  Masks have bit k for byte k, byte k being the one at the lower address
// (little endian: byte 0 of a word is its low byte).
#pragma once
#include <stdint.h>
#include "phi_dev.h"                                    // PHI_HD: host and device, or plain inline without HIP

struct PhiText16 { uint32_t x, y, z, w; };              // sixteen consecutive bytes, as a 16-byte load returns them

// ------------------------------------------------------------------ byte equality
// the bytes of x that equal the character ch (0..255), as 4 bits.  Exact: the sum below never carries out of a byte (0x7f + 0x7f),
// so a byte's flag depends on that byte alone
PHI_HD uint32_t phi_eq4(uint32_t x, uint32_t ch)
{
    const uint32_t y = x ^ (ch * 0x01010101u);
    const uint32_t z = ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y) & 0x80808080u;        // 0x80 in every zero byte of y
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

PHI_HD uint32_t phi_eq16(PhiText16 v, uint32_t ch)
{
    return phi_eq4(v.x, ch) | (phi_eq4(v.y, ch) << 4) | (phi_eq4(v.z, ch) << 8) | (phi_eq4(v.w, ch) << 12);
}

// ------------------------------------------------------------------ the valid mask
// which of the positions at .. at + 15 lie in the window [lo, hi): 16 bits, 0 when none does (lo >= hi included)
PHI_HD uint32_t phi_valid16(int64_t at, int64_t lo, int64_t hi)
{
    const int64_t a = lo - at, b = hi - at;             // the window in the lane's own coordinates
    if (b <= 0 || a >= 16 || a >= b) return 0u;
    const uint32_t below_b = b >= 16 ? 0xffffu : (1u << (int)b) - 1u;
    const uint32_t below_a = a <= 0 ? 0u : (1u << (int)a) - 1u;
    return below_b & ~below_a;
}

// ------------------------------------------------------------------ sixteen bytes from an unaligned address
// bytes sh .. sh + 15 (sh in 0..15) of the 32 bytes a, b; with sh == 0 b is not looked at.  Whole words first, by the bits of
// sh >> 2, then every word from its neighbour by the last 0..3 bytes (a funnel shift: one instruction on the device)
PHI_HD PhiText16 phi_shift16(PhiText16 a, PhiText16 b, uint32_t sh)
{
    uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    if (sh & 8u)
        for (int j = 0; j < 6; j++) x[j] = x[j + 2];
    if (sh & 4u)
        for (int j = 0; j < 5; j++) x[j] = x[j + 1];
    const uint32_t r = 8u * (sh & 3u);
    uint32_t o[4];
    for (int j = 0; j < 4; j++) o[j] = (uint32_t)((((uint64_t)x[j + 1] << 32) | x[j]) >> r);
    return PhiText16{o[0], o[1], o[2], o[3]};
}

// ------------------------------------------------------------------ bisection
// Over an ascending key(i) (equal neighbours allowed), i of the index type I; key and x are compared as they are, so they are of
// one type or of types that compare without loss.  The list forms below read a[i]; a caller whose key is part of an element, or
// lies at a stride, passes the key itself (reads_text.hip: the low half of a 64-bit pair; vcf_region.hip: the first of two).
// the last index i in [0, n) with key(i) <= x, for n >= 1 and key(0) <= x; 0 where key(0) > x
template <class I, class T, class K>
PHI_HD I phi_last_le_key(I n, T x, K key)
{
    I lo = 0, hi = n;                                   // key(lo) <= x < key(hi), key(n) standing for infinity
    while (hi - lo > 1) {
        const I mid = lo + ((hi - lo) >> 1);
        if (key(mid) <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// the first index i in [lo, hi) with key(i) >= x; hi where there is none
template <class I, class T, class K>
PHI_HD I phi_first_ge_key(I lo, I hi, T x, K key)
{
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (key(mid) < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <class I, class E, class T>
PHI_HD I phi_last_le(const E *a, I n, T x)
{
    static_assert(sizeof(E) <= sizeof(T), "x is as wide as the elements: nothing is cut off in the comparison");
    return phi_last_le_key(n, x, [a](I i) { return (T)a[i]; });
}

template <class I, class E, class T>
PHI_HD I phi_first_ge(const E *a, I lo, I hi, T x)
{
    static_assert(sizeof(E) <= sizeof(T), "x is as wide as the elements: nothing is cut off in the comparison");
    return phi_first_ge_key(lo, hi, x, [a](I i) { return (T)a[i]; });
}

// ------------------------------------------------------------------ the loads (device code)
// Every text buffer these kernels read, and how many bytes behind its n bytes of text an aligned 16-byte load may touch.  A lane
// loads the 16 bytes at `at` only when at < n, so 15 bytes of slack are what phi_load16 needs; a buffer with none goes through
// phi_load16_tail.
//   buffer                                      allocated in                                  bytes                       behind n
//   reads text [carry | chunk], both slots      text_stream.hip  phi_reads_text_begin         carry + chunk + 64          64
//   walk text in 4-KB tiles                     walk_text.hip    phi_walk_text_upload,        tiles * WT_TILE + 256       the tile's rest
//                                               gfa_text.hip     phi_gfa_gzip_split                                       and 256
//   inflated text (GFA split, region batches)   inflate.hip      InfRun::layout_resolve       total + 16                  16
//   VCF text of the .tbi writer                 bgzf_index.hip   indexed_run                  ceil(n / BIX_WG) BIX_WG + 64  64 and more
//   VCF text of a region batch                  vcf_region.hip   batch_run                    ceil(n / BIX_WG) BIX_WG + 64  64 and more
//   kept slices of the genotype kernels         vcf.hip          phi_vcf_genotypes (upload)   n                           0: phi_load16_tail
// (the GFA split's scan also reads the 4 bytes at at + 16 where at + 16 < n, its copy the aligned word behind a walk's last byte:
//  both inside the 16)
#if defined(__HIPCC__)
// the 16 bytes at text + at, a multiple of 16 from a 16-byte aligned text
__device__ __forceinline__ PhiText16 phi_load16(const uint8_t *__restrict__ text, int64_t at)
{
    const uint4 v = *reinterpret_cast<const uint4 *>(text + at);
    return PhiText16{v.x, v.y, v.z, v.w};
}

// the same from a buffer that ends with its text: no byte at or behind n is touched, and those read as zero
__device__ __forceinline__ PhiText16 phi_load16_tail(const uint8_t *__restrict__ text, int64_t at, int64_t n)
{
    if (at + 16 <= n) return phi_load16(text, at);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int i = 0; i < 16; i++)
        if (at + i < n) w[i >> 2] |= (uint32_t)text[at + i] << (8 * (i & 3));
    return PhiText16{w[0], w[1], w[2], w[3]};
}

// text[a, a + 16) for any a: the aligned word that holds text[a] and, unless a is aligned, the one behind it, which is read whole
__device__ __forceinline__ PhiText16 phi_load16_unaligned(const uint8_t *__restrict__ text, int64_t a)
{
    const uint32_t sh = (uint32_t)(a & 15);
    const PhiText16 v0 = phi_load16(text, a - sh);
    return phi_shift16(v0, sh ? phi_load16(text, a - sh + 16) : v0, sh);
}
#endif
