// panel_choose_selftest.cpp -- stand-alone check of panel_choose.h (the rule that picks a panel from the read support per
// block and walk) on the CPU: no GPU, no ROCm.  Built plain, with AddressSanitizer + UndefinedBehaviorSanitizer and with
// ThreadSanitizer by the Makefile's panel_choose_sanitize; tests/test_cpu_panel_choose.py runs the three at 1 and 8 host
// threads (argv[1]) and compares their output with each other and with phi_amd.panel.choose_panel on the same matrices.
//
// The cases come from SplitMix64 (value j of seed s: phi_amd.ladder.splitmix64(s, j)), case c with seed 0x5EED0000 + c:
//   n_blocks = 1 + v(0) % 12, n_walks = 1 + v(1) % 40, n_want = 1 + v(2) % n_walks, S[i] from v(8 + i) by the kind c % 5:
//     0  v % 6 (ties and zeros everywhere)            1  all zero
//     2  v % 50, block b all zero when value b of seed + 0xB10C is even
//     3  v % 4, n_want = n_walks                      4  n_walks >= 2, n_want = 1, every walk always kept: refused
//   always[h] = value h of seed + 0xA1 is a multiple of 8 (kinds 0-3; n_want raised to their number)
// and two large cases (200, 201): 300 x 1500 and 40 x 5000, S = v % 1000 where v % 16 == 0, else 0; n_want 200 and 1022.
// Every case is also computed by a serial restatement below (full sort of every block) that shares no code with the
// header.  One line per case: sizes, status and a hash of keep and round_of.  Exit status 0 = every case agreed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "panel_choose.h"

namespace {

uint64_t value(uint64_t seed, uint64_t j)
{
    uint64_t z = seed + (j + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Case {
    int32_t n_blocks = 0, n_walks = 0, n_want = 0;
    std::vector<int32_t> S;
    std::vector<uint8_t> always;
};

Case make_case(int c)
{
    Case k;
    const uint64_t seed = 0x5EED0000ull + (uint64_t)c;
    if (c >= 200) {
        k.n_blocks = c == 200 ? 300 : 40; k.n_walks = c == 200 ? 1500 : 5000; k.n_want = c == 200 ? 200 : 1022;
        k.S.resize((size_t)k.n_blocks * k.n_walks);
        for (size_t i = 0; i < k.S.size(); i++) { const uint64_t v = value(seed, 8 + i); k.S[i] = v % 16 == 0 ? (int32_t)(v % 1000) : 0; }
        k.always.assign((size_t)k.n_walks, 0);
        return k;
    }
    const int kind = c % 5;
    k.n_blocks = 1 + (int32_t)(value(seed, 0) % 12);
    k.n_walks = 1 + (int32_t)(value(seed, 1) % 40);
    if (kind == 4 && k.n_walks < 2) k.n_walks = 2;
    k.n_want = 1 + (int32_t)(value(seed, 2) % (uint64_t)k.n_walks);
    k.S.resize((size_t)k.n_blocks * k.n_walks);
    for (size_t i = 0; i < k.S.size(); i++) {
        const uint64_t v = value(seed, 8 + i);
        const int32_t b = (int32_t)(i / (size_t)k.n_walks);
        k.S[i] = kind == 0 ? (int32_t)(v % 6) : kind == 1 ? 0 : kind == 2 ? (value(seed + 0xB10C, (uint64_t)b) % 2 == 0 ? 0 : (int32_t)(v % 50)) : (int32_t)(v % 4);
    }
    k.always.assign((size_t)k.n_walks, 0);
    if (kind == 4) { k.n_want = 1; std::fill(k.always.begin(), k.always.end(), 1); return k; }
    int32_t n_always = 0;
    for (int32_t h = 0; h < k.n_walks; h++) { k.always[(size_t)h] = value(seed + 0xA1, (uint64_t)h) % 8 == 0; n_always += k.always[(size_t)h]; }
    if (kind == 3) k.n_want = k.n_walks;
    k.n_want = std::max(k.n_want, n_always);
    return k;
}

// the rule from its definition: every block sorted in full, one thread
int serial_choose(const Case &k, std::vector<uint8_t> &keep, std::vector<int32_t> &round_of)
{
    const int32_t W = k.n_walks, B = k.n_blocks;
    keep.assign((size_t)W, 0); round_of.assign((size_t)W, -2);
    int32_t n_in = 0;
    for (int32_t h = 0; h < W; h++) if (k.always[(size_t)h]) { keep[(size_t)h] = 1; round_of[(size_t)h] = -1; n_in++; }
    if (k.n_want < 1 || k.n_want > W || k.n_want > 1022 || n_in > k.n_want) return -1;
    std::vector<long long> total((size_t)W, 0);
    std::vector<std::vector<int32_t>> order((size_t)B, std::vector<int32_t>((size_t)W));
    for (int32_t b = 0; b < B; b++) {
        const int32_t *row = k.S.data() + (size_t)b * W;
        for (int32_t h = 0; h < W; h++) total[(size_t)h] += row[h];
        std::iota(order[(size_t)b].begin(), order[(size_t)b].end(), 0);
        std::stable_sort(order[(size_t)b].begin(), order[(size_t)b].end(), [&](int32_t x, int32_t y) { return row[x] > row[y]; });
    }
    for (int32_t r = 0; r < W && n_in < k.n_want; r++) {
        std::vector<int32_t> votes((size_t)W, 0);
        bool any = false;
        for (int32_t b = 0; b < B; b++) {
            const int32_t h = order[(size_t)b][(size_t)r];
            if (k.S[(size_t)b * W + h] > 0) { votes[(size_t)h]++; any = true; }
        }
        if (!any) break;
        std::vector<int32_t> cand;
        for (int32_t h = 0; h < W; h++) if (votes[(size_t)h] && !keep[(size_t)h]) cand.push_back(h);
        std::stable_sort(cand.begin(), cand.end(), [&](int32_t x, int32_t y) {
            return votes[(size_t)x] != votes[(size_t)y] ? votes[(size_t)x] > votes[(size_t)y] : total[(size_t)x] > total[(size_t)y];
        });
        for (int32_t h : cand) if (n_in < k.n_want) { keep[(size_t)h] = 1; round_of[(size_t)h] = r; n_in++; }
    }
    std::vector<int32_t> rest;
    for (int32_t h = 0; h < W; h++) if (!keep[(size_t)h]) rest.push_back(h);
    std::stable_sort(rest.begin(), rest.end(), [&](int32_t x, int32_t y) { return total[(size_t)x] > total[(size_t)y]; });
    for (int32_t h : rest) if (n_in < k.n_want) { keep[(size_t)h] = 1; round_of[(size_t)h] = W; n_in++; }
    return 0;
}

uint64_t hash_result(const std::vector<uint8_t> &keep, const std::vector<int32_t> &round_of)
{
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < keep.size(); i++) {
        h = (h ^ (uint64_t)keep[i]) * 0x100000001B3ull;
        h = (h ^ (uint64_t)(uint32_t)round_of[i]) * 0x100000001B3ull;
    }
    return h;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1) setenv("PHI_HOST_THREADS", argv[1], 1);
    int failed = 0;
    for (int c = 0; c < 202; c++) {
        const Case k = make_case(c);
        std::vector<uint8_t> keep((size_t)k.n_walks, 7), keep_ref;
        std::vector<int32_t> round_of((size_t)k.n_walks, 7), round_ref;
        int32_t rounds = -1;
        const int rc = phi_panel_choose_rule(k.S.data(), k.n_blocks, k.n_walks, k.always.data(), k.n_want, keep.data(), round_of.data(), &rounds);
        const int rc_ref = serial_choose(k, keep_ref, round_ref);
        bool ok = rc == rc_ref;
        if (ok && rc == 0) {
            ok = keep == keep_ref && round_of == round_ref;
            int32_t n = 0;
            for (uint8_t x : keep) n += x;
            ok = ok && n == k.n_want;
        }
        if (!ok) failed++;
        if (rc) printf("case %d blocks=%d walks=%d want=%d refused%s\n", c, k.n_blocks, k.n_walks, k.n_want, ok ? "" : " FAILED");
        else printf("case %d blocks=%d walks=%d want=%d rounds=%d hash=%016llx%s\n", c, k.n_blocks, k.n_walks, k.n_want, rounds,
                    (unsigned long long)hash_result(keep, round_of), ok ? "" : " FAILED");
    }
    return failed ? 1 : 0;
}
