// deflate_codes_selftest.cpp -- ../deflate_codes.h on the CPU: the length-limited code construction, the run-length coding of
// code lengths, the canonical codes, the symbols of copies and the CRC32 shift, as the compressor's kernel (../deflate.hip)
// calls them.  Prints one line per check ("name ok ..." or "name FAILED ..."); exit status 1 if any failed.
//
// For every histogram: no length above the limit; the Kraft sum is exactly 1 (no used symbol: no code; one: a single code of
// length 1); a rarer symbol never has the shorter code; the cost is not above that of the fixed code of RFC 1951 3.2.6 where
// one is defined (286 and 30 symbols); the run-length coding of the lengths, expanded again, gives the lengths back; the
// canonical codes are prefix-free.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../deflate_codes.h"

static int n_failed = 0;
static void line(const char *name, bool ok, const char *what)
{
    printf("%s %s %s\n", name, ok ? "ok" : "FAILED", what);
    if (!ok) n_failed++;
}

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int fixed_len(int n, int s) { return n == DFL_NDIST ? 5 : s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

struct Tally { long checked = 0, bad_limit = 0, bad_kraft = 0, bad_order = 0, bad_cost = 0, bad_rle = 0, bad_prefix = 0; int depth = 0, longest = 0; };

static void expand(const uint8_t *sym, const uint8_t *extra, int k, std::vector<uint8_t> &out, bool *ok)
{
    out.clear();
    for (int i = 0; i < k; i++) {
        if (sym[i] < 16) out.push_back(sym[i]);
        else if (sym[i] == 16) {
            if (out.empty() || extra[i] > 3) { *ok = false; return; }
            out.insert(out.end(), 3 + extra[i], out.back());
        } else if (sym[i] == 17) { if (extra[i] > 7) { *ok = false; return; } out.insert(out.end(), 3 + extra[i], 0); }
        else if (sym[i] == 18) { if (extra[i] > 127) { *ok = false; return; } out.insert(out.end(), 11 + extra[i], 0); }
        else { *ok = false; return; }
    }
}

static void check(const uint32_t *freq, int n, int limit, Tally &t)
{
    static DflWork w;
    uint8_t len[DFL_MAX_SYMS];
    uint16_t code[DFL_MAX_SYMS];
    const int depth = dfl_build_lengths(freq, n, limit, len, &w);
    t.checked++;
    if (depth > t.depth) t.depth = depth;
    int used = 0;
    uint64_t kraft = 0, cost = 0, fixed = 0;
    bool in_limit = true, coded = true;
    for (int s = 0; s < n; s++) {
        if (len[s] > t.longest) t.longest = len[s];
        in_limit = in_limit && len[s] <= limit;
        coded = coded && ((freq[s] != 0) == (len[s] != 0));
        if (!freq[s]) continue;
        used++;
        if (len[s]) kraft += 1ull << (32 - len[s]);
        cost += (uint64_t)freq[s] * len[s];
        fixed += (uint64_t)freq[s] * (uint64_t)fixed_len(n, s);
    }
    t.bad_limit += !in_limit || !coded;
    t.bad_kraft += used >= 2 ? kraft != (1ull << 32) : used == 1 ? kraft != (1ull << 31) : kraft != 0;
    bool order = true;
    for (int a = 0; a < n && order; a++)
        for (int b = 0; b < n; b++)
            if (freq[a] && freq[b] && freq[a] < freq[b] && len[a] < len[b]) { order = false; break; }
    t.bad_order += !order;
    if (n == DFL_NLIT || n == DFL_NDIST) t.bad_cost += cost > fixed;
    // the run-length coding, and back
    uint8_t sym[DFL_MAX_SYMS], extra[DFL_MAX_SYMS];
    const int k = dfl_rle_lengths(len, n, sym, extra);
    std::vector<uint8_t> back;
    bool rle_ok = k <= n;
    expand(sym, extra, k, back, &rle_ok);
    t.bad_rle += !rle_ok || (int)back.size() != n || memcmp(back.data(), len, (size_t)n) != 0;
    // canonical codes: distinct, and none a prefix of another (codes are reversed: compare the low bits)
    dfl_canonical_codes(len, n, code);
    bool prefix_free = true;
    if (used <= 64)
        for (int a = 0; a < n && prefix_free; a++)
            for (int b = 0; b < n; b++)
                if (a != b && len[a] && len[b] && len[a] <= len[b] && (code[b] & ((1u << len[a]) - 1)) == code[a]) { prefix_free = false; break; }
    t.bad_prefix += !prefix_free;
}

static bool clean(const Tally &t) { return !(t.bad_limit || t.bad_kraft || t.bad_order || t.bad_cost || t.bad_rle || t.bad_prefix); }
static void report(const char *name, const Tally &t, bool more = true)
{
    char buf[256];
    snprintf(buf, sizeof buf, "histograms=%ld depth=%d longest=%d limit=%ld kraft=%ld order=%ld cost=%ld rle=%ld prefix=%ld", t.checked, t.depth, t.longest,
             t.bad_limit, t.bad_kraft, t.bad_order, t.bad_cost, t.bad_rle, t.bad_prefix);
    line(name, clean(t) && more, buf);
}

int main()
{
    const int alphabets[3][2] = {{DFL_NLIT, 15}, {DFL_NDIST, 15}, {DFL_NCL, 7}};
    uint32_t f[DFL_MAX_SYMS];
    {   // every histogram with 0, 1 and 2 used symbols (the counts equal, and far apart either way)
        Tally t;
        for (const auto &ab : alphabets) {
            const int n = ab[0];
            memset(f, 0, sizeof f);
            check(f, n, ab[1], t);
            for (int a = 0; a < n; a++) {
                for (uint32_t ca : {1u, 65280u}) { f[a] = ca; check(f, n, ab[1], t); }
                for (int b = a + 1; b < n; b++) {
                    f[a] = 1; f[b] = 1; check(f, n, ab[1], t);
                    f[a] = 1; f[b] = 65279; check(f, n, ab[1], t);
                    f[a] = 65279; f[b] = 1; check(f, n, ab[1], t);
                    f[b] = 0;
                }
                f[a] = 0;
            }
        }
        report("few_symbols", t, t.longest == 1);
    }
    {
        Tally t;
        for (int s = 0; s < DFL_NLIT; s++) f[s] = 100;
        check(f, DFL_NLIT, 15, t);
        report("flat_286", t, t.longest == 9 && t.depth == 9);
    }
    {
        Tally t;
        for (int s = 0; s < DFL_NDIST; s++) f[s] = 7;
        check(f, DFL_NDIST, 15, t);
        report("flat_30", t, t.longest == 5 && t.depth == 5);
    }
    {   // Fibonacci counts 1, 1, 2, 3, ... over 22 symbols (sum 46367): Huffman's code is 21 deep
        Tally t;
        memset(f, 0, sizeof f);
        uint32_t a = 1, b = 1, sum = 0;
        for (int s = 0; s < 22; s++) { f[40 + 3 * s] = a; sum += a; const uint32_t c = a + b; a = b; b = c; }
        check(f, DFL_NLIT, 15, t);
        report("fibonacci_22_limit_15", t, sum == 46367 && t.depth == 21 && t.longest == 15);
    }
    {   // the same shape over 11 of the 19 code-length symbols, limit 7: 10 deep unlimited
        Tally t;
        memset(f, 0, sizeof f);
        uint32_t a = 1, b = 1;
        for (int s = 0; s < 11; s++) { f[18 - s] = a; const uint32_t c = a + b; a = b; b = c; }
        check(f, DFL_NCL, 7, t);
        report("fibonacci_11_limit_7", t, t.depth == 10 && t.longest == 7);
    }
    {   // 2000 seeded random histograms: the three alphabets, sparse and dense, flat and steep counts
        Tally t;
        for (int i = 0; i < 2000; i++) {
            const auto &ab = alphabets[i % 3];
            const int n = ab[0], shape = (int)(rnd() % 4);
            const uint64_t density = rnd() % 100;
            uint64_t total = 0;
            for (int s = 0; s < n; s++) {
                uint32_t c = 0;
                if (rnd() % 100 <= density) {
                    if (shape == 0) c = 1 + (uint32_t)(rnd() % 1000);
                    else if (shape == 1) c = 1u << (rnd() % 16);                          // powers of two: deep trees
                    else if (shape == 2) c = 1 + (uint32_t)((rnd() % 65000) >> (rnd() % 16));
                    else c = (uint32_t)(1.0 + 1.6 * (double)(total ? total : 1) * (double)(rnd() % 3 != 0));   // each about the sum so far
                }
                if (total + c > 4000000) c = 1;
                f[s] = c;
                total += c;
            }
            check(f, n, ab[1], t);
        }
        report("random_2000", t, t.checked == 2000 && t.depth > 15);
    }
    {   // the symbols of copies against RFC 1951 3.2.5, built from its rule
        int lbase[29], lext[29], dbase[30], dext[30];
        for (int k = 0; k < 8; k++) { lbase[k] = 3 + k; lext[k] = 0; }
        for (int k = 8; k < 28; k++) { lext[k] = (k - 4) / 4; lbase[k] = lbase[k - 1] + (1 << lext[k - 1]); }
        lbase[28] = 258; lext[28] = 0;
        for (int k = 0; k < 30; k++) { dext[k] = k < 4 ? 0 : (k - 2) / 2; dbase[k] = k ? dbase[k - 1] + (1 << dext[k - 1]) : 1; }
        long bad = 0;
        for (int len = 3; len <= 258; len++) {
            int ne, ex;
            const int s = dfl_length_symbol(len, &ne, &ex) - 257;
            bad += s < 0 || s > 28 || ne != lext[s] || lbase[s] + ex != len || ex >= (1 << ne);
        }
        for (int d = 1; d <= 32768; d++) {
            int ne, ex;
            const int s = dfl_dist_symbol(d, &ne, &ex);
            bad += s < 0 || s > 29 || ne != dext[s] || dbase[s] + ex != d || ex >= (1 << ne);
        }
        char buf[96];
        snprintf(buf, sizeof buf, "lengths=256 distances=32768 bad=%ld", bad);
        line("copy_symbols", bad == 0 && lbase[27] == 227 && dbase[29] == 24577, buf);
    }
    {   // the CRC32 shift against the bitwise register run over zero bytes, and a two-part CRC put together with it
        long bad = 0;
        for (int i = 0; i < 200; i++) {
            const uint32_t c = (uint32_t)rnd(), nz = i < 8 ? (uint32_t)i : (uint32_t)(rnd() % 70000);
            uint32_t r = c;
            for (uint32_t k = 0; k < nz * 8; k++) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u)));
            bad += dfl_crc_shift(c, nz) != r;
        }
        line("crc_shift", bad == 0 && dfl_crc_mul(0x80000000u, 0x12345678u) == 0x12345678u, "200 registers over 0..70000 zero bytes");
    }
    return n_failed ? 1 : 0;
}
