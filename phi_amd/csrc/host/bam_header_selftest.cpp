// bam_header_selftest.cpp -- the BAM header parser (../bam_header.h) on untrusted bytes, as a program of its own: built under
// AddressSanitizer + UndefinedBehaviorSanitizer by `make bam_sanitize` and run by tests/test_cpu_bam_host.py.
// Every input lies in a heap block of exactly its size, so that a read past the bytes given is a report, not luck.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../bam_header.h"

static void put32(std::string &s, int32_t v) { for (int i = 0; i < 4; i++) s.push_back((char)((uint32_t)v >> (8 * i))); }

static std::string header(const std::string &text, int n_ref, int name_len)
{
    std::string s("BAM\1", 4);
    put32(s, (int32_t)text.size());
    s += text;
    put32(s, n_ref);
    for (int r = 0; r < n_ref; r++) {
        std::string name = "chr" + std::to_string(r);
        name.resize((size_t)name_len - 1, 'x');
        put32(s, name_len);
        s += name;
        s.push_back(0);
        put32(s, 1000 + r);
    }
    return s;
}

// the parser on an exact-size heap copy of s[0, n)
static int run(const std::string &s, size_t n, int64_t *start, int32_t *n_ref)
{
    unsigned char *p = (unsigned char *)malloc(n ? n : 1);
    if (n) memcpy(p, s.data(), n);
    char err[128];
    const int r = phi_bam_header_parse(n ? p : nullptr, (int64_t)n, start, n_ref, err, (int)sizeof err);
    if (r == PHI_BAM_HDR_BAD && !err[0]) { fprintf(stderr, "BAD without a message\n"); exit(2); }
    free(p);
    return r;
}

int main()
{
    long n_ok = 0, n_more = 0, n_bad = 0;
    const int refs[] = {0, 1, 3, 300};
    for (int nr : refs) {
        const std::string h = header(nr ? "@HD\tVN:1.6\n" : "", nr, 12) + std::string(40, '\7');     // (bytes of a first record behind it)
        const size_t hl = h.size() - 40;
        // every truncation point: MORE with a bound beyond n up to the header's end, OK from there on
        for (size_t n = 0; n <= h.size(); n++) {
            int64_t st = -1; int32_t k = -1;
            const int r = run(h, n, &st, &k);
            if (n < hl) {
                if (r != PHI_BAM_HDR_MORE || st <= (int64_t)n || st > (int64_t)hl) { fprintf(stderr, "n_ref %d cut at %zu: status %d, bound %lld\n", nr, n, r, (long long)st); return 1; }
                n_more++;
            } else {
                if (r != PHI_BAM_HDR_OK || st != (int64_t)hl || k != nr) { fprintf(stderr, "n_ref %d, %zu bytes: status %d, start %lld\n", nr, n, r, (long long)st); return 1; }
                n_ok++;
            }
        }
    }
    {
        // wrong magic at each of its bytes, and what other formats begin with
        for (int i = 0; i < 4; i++) {
            std::string h = header("", 0, 2);
            h[(size_t)i] ^= 0x20;
            for (size_t n = (size_t)i + 1; n <= h.size(); n++) { int64_t st; int32_t k; if (run(h, n, &st, &k) != PHI_BAM_HDR_BAD) { fprintf(stderr, "magic byte %d accepted\n", i); return 1; } n_bad++; }
        }
        const char *others[] = {"CRAM\3\0", "@HD\tVN:1.6\n", "@read1\nACGT\n+\nIIII\n", ">r\nACGT\n"};
        for (const char *o : others) { int64_t st; int32_t k; if (run(std::string(o), strlen(o), &st, &k) != PHI_BAM_HDR_BAD) { fprintf(stderr, "%s accepted\n", o); return 1; } n_bad++; }
    }
    {
        // negative and huge lengths: BAD, or MORE with a bound -- never a read past the bytes
        const int32_t vals[] = {-1, -4, INT32_MIN, INT32_MAX, 0x7ffffff0};
        const std::string h = header("@CO\tx\n", 2, 5);
        const size_t at_text = 4, at_nref = 8 + 6, at_name = at_nref + 4;
        for (int32_t v : vals)
            for (size_t at : {at_text, at_nref, at_name}) {
                std::string m = h;
                for (int i = 0; i < 4; i++) m[at + (size_t)i] = (char)((uint32_t)v >> (8 * i));
                int64_t st; int32_t k;
                const int r = run(m, m.size(), &st, &k);
                if (v < 0 && r != PHI_BAM_HDR_BAD) { fprintf(stderr, "%d at %zu: status %d\n", (int)v, at, r); return 1; }
                if (v > 0 && (r != PHI_BAM_HDR_MORE || st <= (int64_t)m.size())) { fprintf(stderr, "%d at %zu: status %d, bound %lld\n", (int)v, at, r, (long long)st); return 1; }
                (v < 0 ? n_bad : n_more)++;
            }
        std::string z = h;                                   // an l_name of 0: a name holds its NUL at least
        memset(&z[at_name], 0, 4);
        int64_t st; int32_t k;
        if (run(z, z.size(), &st, &k) != PHI_BAM_HDR_BAD) { fprintf(stderr, "l_name 0 accepted\n"); return 1; }
        n_bad++;
    }
    {
        // random bytes behind the magic, every length up to 64: any status, no report from the sanitizers
        uint64_t x = 0x9E3779B97F4A7C15ull;
        for (int it = 0; it < 20000; it++) {
            std::string s("BAM\1", 4);
            const size_t n = 4 + (size_t)(it % 61);
            while (s.size() < n) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; s.push_back((x & 3) ? (char)(x >> 8 & 3) : (char)(x >> 8)); }
            int64_t st; int32_t k;
            const int r = run(s, s.size(), &st, &k);
            if (r == PHI_BAM_HDR_OK && (st > (int64_t)s.size() || st < 12)) { fprintf(stderr, "random: start %lld of %zu\n", (long long)st, s.size()); return 1; }
            (r == PHI_BAM_HDR_OK ? n_ok : r == PHI_BAM_HDR_MORE ? n_more : n_bad)++;
        }
    }
    printf("bam_header_selftest: ok %ld, need more %ld, refused %ld\n", n_ok, n_more, n_bad);
    return 0;
}
