// text_bytes_selftest.cpp -- the plain code of ../text_bytes.h (no HIP) against byte-at-a-time code: the equality masks, the valid
// mask of a lane against a window, sixteen bytes at an unaligned offset, and the two bisections.  Prints one line per check
// ("name ok ..." or "name FAILED ..."); exit status 1 if any failed.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../text_bytes.h"

static int n_failed = 0;
static void line(const char *name, long bad, long cases)
{
    printf("%s %s cases=%ld bad=%ld\n", name, bad ? "FAILED" : "ok", cases, bad);
    if (bad) n_failed++;
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

static PhiText16 words_of(const uint8_t *b)             // as a little-endian 16-byte load
{
    uint32_t w[4];
    memcpy(w, b, 16);
    return PhiText16{w[0], w[1], w[2], w[3]};
}

static uint32_t eq_bytes(const uint8_t *b, int n, uint32_t ch)
{
    uint32_t m = 0;
    for (int k = 0; k < n; k++) m |= (uint32_t)(b[k] == ch) << k;
    return m;
}

int main()
{
    {   // every character; words whose bytes are drawn from the borrow and high-bit neighbours of it, in every combination
        long bad = 0, cases = 0;
        for (uint32_t c = 0; c < 256; c++) {
            const uint8_t pool[8] = {(uint8_t)c, (uint8_t)(c - 1), (uint8_t)(c + 1), (uint8_t)(c ^ 0x80), 0x00, 0x7f, 0x80, 0xff};
            for (int i = 0; i < 8 * 8 * 8 * 8; i++) {
                const uint8_t b[4] = {pool[i & 7], pool[(i >> 3) & 7], pool[(i >> 6) & 7], pool[(i >> 9) & 7]};
                uint32_t x;
                memcpy(&x, b, 4);
                bad += phi_eq4(x, c) != eq_bytes(b, 4, c);
                cases++;
            }
        }
        line("eq4_neighbours", bad, cases);
    }
    {   // 16 bytes: the same pool at random, and random bytes
        long bad = 0, cases = 0;
        for (uint32_t c = 0; c < 256; c++) {
            const uint8_t pool[8] = {(uint8_t)c, (uint8_t)(c - 1), (uint8_t)(c + 1), (uint8_t)(c ^ 0x80), 0x00, 0x7f, 0x80, 0xff};
            for (int i = 0; i < 256; i++) {
                uint8_t b[16];
                for (int k = 0; k < 16; k++) { const uint64_t r = rnd(); b[k] = (i & 1) ? (uint8_t)(r >> 8) : pool[r & 7]; }
                bad += phi_eq16(words_of(b), c) != eq_bytes(b, 16, c);
                cases++;
            }
        }
        line("eq16", bad, cases);
    }
    {   // the valid mask: every lane of three, every window lo <= hi of [0, 48]
        long bad = 0, cases = 0;
        for (int64_t at = 0; at <= 32; at += 16)
            for (int64_t lo = 0; lo <= 48; lo++)
                for (int64_t hi = lo; hi <= 48; hi++) {
                    uint32_t want = 0;
                    for (int k = 0; k < 16; k++) want |= (uint32_t)(at + k >= lo && at + k < hi) << k;
                    bad += phi_valid16(at, lo, hi) != want;
                    cases++;
                }
        // (a window given the wrong way round is empty; a text far longer than 32 bits)
        bad += phi_valid16(16, 20, 18) != 0u;
        bad += phi_valid16(((int64_t)1 << 33) + 16, 0, ((int64_t)1 << 33) + 19) != 0x7u;
        cases += 2;
        line("valid16", bad, cases);
    }
    {   // sixteen bytes at every shift: all-distinct bytes, and random ones
        long bad = 0, cases = 0;
        for (int round = 0; round < 64; round++) {
            uint8_t b[32];
            for (int k = 0; k < 32; k++) b[k] = round == 0 ? (uint8_t)(k + 1) : round == 1 ? (uint8_t)(0xff - 7 * k) : (uint8_t)rnd();
            for (uint32_t sh = 0; sh < 16; sh++) {
                const PhiText16 got = phi_shift16(words_of(b), words_of(b + 16), sh), want = words_of(b + sh);
                bad += memcmp(&got, &want, 16) != 0;
                cases++;
            }
            // with sh == 0 the second word is not looked at: whatever it holds
            const PhiText16 got = phi_shift16(words_of(b), PhiText16{~0u, 0x5a5a5a5au, 0u, ~0u}, 0), want = words_of(b);
            bad += memcmp(&got, &want, 16) != 0;
            cases++;
        }
        line("shift16", bad, cases);
    }
    {   // the bisections: n = 1..70, strictly and non-strictly ascending, every x from a[0] to a[n - 1] + 1; int and int64_t indices
        long bad = 0, cases = 0;
        for (int strict = 0; strict < 2; strict++)
            for (int n = 1; n <= 70; n++) {
                std::vector<int64_t> a((size_t)n);
                std::vector<int32_t> a32((size_t)n);
                int64_t v = (int64_t)(rnd() % 5);
                for (int i = 0; i < n; i++) {
                    v += strict ? 1 + (int64_t)(rnd() % 3) : (int64_t)(rnd() % 3);
                    a[(size_t)i] = v;
                    a32[(size_t)i] = (int32_t)v;
                }
                for (int64_t x = a[0]; x <= a[(size_t)n - 1] + 1; x++) {
                    int want = 0;
                    for (int i = 0; i < n; i++) if (a[(size_t)i] <= x) want = i;
                    bad += phi_last_le(a.data(), n, x) != want;
                    bad += phi_last_le(a.data(), (int64_t)n, x) != (int64_t)want;
                    bad += phi_last_le(a32.data(), (int64_t)n, x) != (int64_t)want;
                    int first = n;
                    for (int i = n - 1; i >= 0; i--) if (a[(size_t)i] >= x) first = i;
                    bad += phi_first_ge(a.data(), (int64_t)0, (int64_t)n, x) != (int64_t)first;
                    cases += 4;
                }
                // below a[0]: index 0 from the one, 0 from the other; an inner range [lo, hi)
                bad += phi_last_le(a.data(), n, a[0] - 1) != 0;
                bad += phi_first_ge(a.data(), (int64_t)0, (int64_t)n, a[0] - 1) != 0;
                const int64_t lo = n / 3, hi = n - n / 4;
                for (int64_t x = a[0] - 1; x <= a[(size_t)n - 1] + 1; x++) {
                    int64_t first = hi;
                    for (int64_t i = hi - 1; i >= lo; i--) if (a[(size_t)i] >= x) first = i;
                    bad += phi_first_ge(a.data(), lo, hi, x) != first;
                    cases++;
                }
                cases += 2;
            }
        line("bisection", bad, cases);
    }
    {   // the key form: 64-bit pairs whose low halves ascend, against a 32-bit x; the first of two at a stride
        long bad = 0, cases = 0;
        for (uint32_t n = 1; n <= 70; n++) {
            std::vector<uint64_t> a(n);
            uint32_t v = 0;
            for (uint32_t i = 0; i < n; i++) { v += (uint32_t)(rnd() % 4); a[i] = ((uint64_t)(i / 3) << 32) | v; }
            for (uint32_t x = (uint32_t)a[0]; x <= v + 1; x++) {
                uint32_t want = 0;
                for (uint32_t i = 0; i < n; i++) if ((uint32_t)a[i] <= x) want = i;
                bad += phi_last_le_key(n, x, [&a](uint32_t i) { return (uint32_t)a[i]; }) != want;
                cases++;
            }
            std::vector<int64_t> pair(2 * (size_t)n);           // (first ascending, second anything)
            for (uint32_t i = 0; i < n; i++) { pair[2 * i] = (int64_t)(uint32_t)a[i]; pair[2 * i + 1] = -(int64_t)i; }
            for (int64_t x = pair[0] - 1; x <= (int64_t)v + 1; x++) {
                int64_t first = n;
                for (int64_t i = (int64_t)n - 1; i >= 0; i--) if (pair[2 * (size_t)i] >= x) first = i;
                bad += phi_first_ge_key((int64_t)0, (int64_t)n, x, [&pair](int64_t i) { return pair[2 * (size_t)i]; }) != first;
                cases++;
            }
        }
        line("bisection_key", bad, cases);
    }
    return n_failed ? 1 : 0;
}
