// kmer_keys_selftest.cpp -- the host side of the k-mer keys (../phi_dev.h, no HIP): phi_kmer_mix is a bijection whose inverse
// is phi_kmer_unmix, no k-mer of up to 31 bases maps to the table sentinel, and phi_kmer_flush_rule -- what the flush makes
// of a logged novel k-mer -- reports every way in which a MurmurHash3 collision could make the k-mer route differ from the
// hash route.  Prints one line per check ("name ok ..." or "name FAILED ..."); exit status 1 if any failed.
#include <stdint.h>
#include <stdio.h>
#include "../phi_dev.h"

static int n_failed = 0;
static void line(const char *name, bool ok, const char *what)
{
    printf("%s %s %s\n", name, ok ? "ok" : "FAILED", what);
    if (!ok) n_failed++;
}

// splitmix64: the random inputs are the same in every build
static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main()
{
    char buf[256];
    {
        long bad = 0;
        for (int i = 0; i < 1000000; i++) {
            const uint64_t x = rnd();
            bad += phi_kmer_unmix(phi_kmer_mix(x)) != x;
            bad += phi_kmer_mix(phi_kmer_unmix(x)) != x;
        }
        snprintf(buf, sizeof buf, "random=1000000 bad=%ld", bad);
        line("inverse_random", bad == 0, buf);
    }
    {
        const uint64_t edge[3] = {0ull, (1ull << 62) - 1, ~0ull};
        bool ok = true;
        for (uint64_t x : edge) ok = ok && phi_kmer_unmix(phi_kmer_mix(x)) == x;
        line("inverse_edges", ok, "0, 2^62 - 1, ~0");
    }
    {
        const uint64_t pre = phi_kmer_unmix(PHI_EMPTY_KEY);
        snprintf(buf, sizeof buf, "preimage=0x%016llx", (unsigned long long)pre);
        line("sentinel_preimage", pre >= (1ull << 62) && phi_kmer_mix(pre) == PHI_EMPTY_KEY, buf);
        line("multiplier_inverse", (uint64_t)(PHI_KMER_MIX_MUL * PHI_KMER_MIX_INV) == 1ull, "mul * inv == 1 mod 2^64");
    }
    {
        // the home bucket is key & bmask: 2^16 k-mers that differ in their FIRST bases only (the top bits of the value) and 2^16
        // that differ in their last bases only must both spread over 2^16 buckets as random keys do (1 - 1/e = 63 % of them taken;
        // 55 % asked for: a multiply that left the low bits to the low bits alone would take 2^-k of them)
        int taken_hi = 0, taken_lo = 0;
        static uint8_t hi[1 << 16], lo[1 << 16];
        for (uint64_t i = 0; i < (1u << 16); i++) {
            uint8_t &a = hi[phi_kmer_mix((i << 46) | 0x2AAAAAAAAAAull) & 0xFFFF], &b = lo[phi_kmer_mix((0x1555ull << 46) | i) & 0xFFFF];
            taken_hi += !a; a = 1;
            taken_lo += !b; b = 1;
        }
        snprintf(buf, sizeof buf, "taken_hi=%d taken_lo=%d of 65536", taken_hi, taken_lo);
        line("low_bits_mixed", taken_hi > 36000 && taken_lo > 36000, buf);
    }
    // ---- the flush rule on hand-made (h, v) pairs
    const uint64_t H = 0x0123456789ABCDEFull, V = 0x1B1B1B1B1B1B1Bull, V2 = 0x2C2C2C2C2C2C2Cull;
    line("rule_plain_first", phi_kmer_flush_rule(H, V, false, 0, 0, false) == 0, "first entry of a chunk, not a walk hash: inserted");
    line("rule_plain_prev_differs", phi_kmer_flush_rule(H, V, true, H + 1, V2, false) == 0, "another k-mer with another hash before it: inserted");
    line("rule_same_kmer_twice", phi_kmer_flush_rule(H, V, true, H, V, false) == 0, "the same k-mer before it (the next read's first window): inserted");
    line("rule_novel_novel", phi_kmer_flush_rule(H, V, true, H, V2, false) == PHI_KERR_HASH_COLLISION, "equal hash, different k-mer before it: collision");
    line("rule_novel_novel_no_prev", phi_kmer_flush_rule(H, V, false, H, V2, false) == 0, "the same pair without a predecessor (entry 0): hp, vp ignored");
    line("rule_novel_walk", phi_kmer_flush_rule(H, V, false, 0, 0, true) == PHI_KERR_HASH_COLLISION, "the hash of a novel k-mer is a walk minimiser's: collision");
    line("rule_both", phi_kmer_flush_rule(H, V, true, H, V2, true) == PHI_KERR_HASH_COLLISION, "both at once: one bit");
    line("rule_sentinel", phi_kmer_flush_rule(PHI_EMPTY_KEY, V, false, 0, 0, false) == PHI_KERR_SENTINEL, "h == PHI_EMPTY_KEY: sentinel");
    line("rule_sentinel_first", phi_kmer_flush_rule(PHI_EMPTY_KEY, V, true, PHI_EMPTY_KEY, V2, true) == PHI_KERR_SENTINEL, "the sentinel goes before everything else");
    line("error_bits", PHI_KERR_HASH_COLLISION == 128u && PHI_KERR_SENTINEL == 1u, "128, 1");
    {
        // the hash of a k-mer value is MurmurHash3 of its ASCII spelling: a known vector (ACGT repeated, 31 bases), both ways
        uint64_t v = 0;
        for (int i = 0; i < 31; i++) v = (v << 2) | (uint64_t)(i & 3);
        const uint64_t e0 = 0x5447434154474341ull, e3 = 0x0047434154474341ull;   // "ACGTACGT" little-endian; 7 bytes in the last lane
        line("hash_of_value", phi_kmer_hash(v, 31) == phi_murmur_lanes(e0, e0, e0, e3, 31), "phi_kmer_hash(v) == murmur of the spelled bytes");
    }
    return n_failed ? 1 : 0;
}
