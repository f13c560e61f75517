// solve_host_selftest.cpp -- stand-alone check of ../solve_host.h (the rules of phi_solve that need no GPU) on the CPU: no
// GPU, no ROCm.  Built plain, with AddressSanitizer + UndefinedBehaviorSanitizer and with ThreadSanitizer by the Makefile's
// solve_host_sanitize; tests/test_cpu_solve_host.py runs the three and compares their output.
//
// Every case runs at PHI_HOST_THREADS=1 and =8 and must give the same line both times.  The header's results are compared
// with restatements below (namespace ref) that are serial, written from the definitions and share no code with it, or with
// brute force:
//   * clusters: the components of the interval overlap graph (closed intervals of topological ranks; union-find over all
//     pairs); a component is one cluster exactly when every pair in it lies on different walks and overlaps, else each of
//     its anchors is a cluster of its own;
//   * chain: S[b][h] = the best sum over every sequence of walks through the blocks before b that begins inside a block
//     (row n_walks) and leaves block b - 1 on walk h; "no run" entries break a sequence;
//   * anchor arrays: one loop over the kept list;
//   * block placement: from `start`, the cut is the first allowed step in [start + target, min(start + ring, nk - 1)], else
//     the last allowed step in (start, start + target); without one the rest is one block if it fits the ring, else this ring
//     fails; the first ring that places everything wins;
//   * CSR and repeats: O(n^2) recounts;
//   * tighten and branch: the cases by hand.
// One line per case on stdout: name, ok or FAILED, sizes and a hash of the results.  Exit status 0 = every case agreed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <map>
#include <numeric>
#include <set>
#include <string>
#include <vector>
#include "../solve_host.h"

namespace {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    bool chance(int percent) { return below(100) < percent; }
};

struct Hash {
    uint64_t h = 0xCBF29CE484222325ull;
    void add(int64_t v) { for (int i = 0; i < 8; i++) { h ^= (uint64_t)(v >> (8 * i)) & 0xFF; h *= 0x100000001B3ull; } }
    template <class T> void add_all(const std::vector<T> &v) { add((int64_t)v.size()); for (const T &x : v) add((int64_t)x); }
};

int n_failed = 0;
std::string fmt(const char *f, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}
// body(detail) -> agreed; run at 1 and at 8 host threads, the two details must be equal
void run_case(const char *name, const std::function<bool(std::string &)> &body)
{
    std::string d[2];
    bool ok = true;
    for (int t = 0; t < 2; t++) {
        setenv("PHI_HOST_THREADS", t ? "8" : "1", 1);
        ok = body(d[t]) && ok;
    }
    ok = ok && d[0] == d[1];
    if (!ok) n_failed++;
    printf("%s %s %s\n", name, ok ? "ok" : "FAILED", d[0].c_str());
}
// a case the header must refuse: the line is the refusal itself
void run_refusal(const char *name, const std::function<std::string()> &body)
{
    std::string d[2];
    for (int t = 0; t < 2; t++) {
        setenv("PHI_HOST_THREADS", t ? "8" : "1", 1);
        d[t] = body();
    }
    if (d[0] != d[1] || d[0].compare(0, 8, "refused ") != 0) { n_failed++; printf("%s FAILED %s | %s\n", name, d[0].c_str(), d[1].c_str()); }
    else printf("%s %s\n", name, d[0].c_str());
}

// ------------------------------------------------------------------------------------------ clusters
namespace ref {
std::vector<std::vector<int32_t>> clusters(const std::vector<PhiAnchorIv> &iv)
{
    const size_t n = iv.size();
    std::vector<size_t> root(n);
    std::iota(root.begin(), root.end(), (size_t)0);
    std::function<size_t(size_t)> find = [&](size_t x) { return root[x] == x ? x : root[x] = find(root[x]); };
    auto overlap = [&](size_t i, size_t j) { return iv[i].lo <= iv[j].hi && iv[j].lo <= iv[i].hi; };
    for (size_t i = 0; i < n; i++) for (size_t j = i + 1; j < n; j++) if (overlap(i, j)) root[find(i)] = find(j);
    std::vector<std::vector<int32_t>> out;
    for (size_t r = 0; r < n; r++) {
        if (find(r) != r) continue;
        std::vector<size_t> comp;
        for (size_t i = 0; i < n; i++) if (find(i) == r) comp.push_back(i);
        bool exclusive = true;
        for (size_t i : comp) for (size_t j : comp) if (i < j && (iv[i].h == iv[j].h || !overlap(i, j))) exclusive = false;
        if (exclusive) { out.emplace_back(); for (size_t i : comp) out.back().push_back(iv[i].a); }
        else for (size_t i : comp) out.push_back({iv[i].a});
    }
    return out;
}
}   // namespace ref

std::vector<std::vector<int32_t>> normal(std::vector<std::vector<int32_t>> cl)
{
    for (auto &x : cl) std::sort(x.begin(), x.end());
    std::sort(cl.begin(), cl.end());
    return cl;
}
bool clusters_case(const std::vector<PhiAnchorIv> &iv, const std::vector<std::vector<int32_t>> *want, std::string &d)
{
    const auto got = normal(phi_clusters(iv));
    bool ok = got == normal(ref::clusters(iv));
    if (want) ok = ok && got == normal(*want);
    Hash h;
    for (const auto &x : got) h.add_all(x);
    d = fmt("anchors=%zu clusters=%zu hash=%016llx", iv.size(), got.size(), (unsigned long long)h.h);
    return ok;
}
void test_clusters()
{
    typedef std::vector<std::vector<int32_t>> CL;
    const struct { const char *name; std::vector<PhiAnchorIv> iv; CL want; } fixed[] = {
        {"clusters_one", {{3, 5, 0, 0}}, {{0}}},
        {"clusters_same_walk", {{3, 5, 1, 0}, {4, 6, 1, 1}}, {{0}, {1}}},
        {"clusters_disjoint", {{3, 5, 0, 0}, {6, 8, 1, 1}}, {{0}, {1}}},
        {"clusters_three_overlap", {{3, 6, 0, 0}, {4, 7, 1, 1}, {5, 8, 2, 2}}, {{0, 1, 2}}},
        // a - b - c, a and c apart: one component, not pairwise exclusive
        {"clusters_chain", {{1, 3, 0, 0}, {3, 6, 1, 1}, {5, 8, 2, 2}}, {{0}, {1}, {2}}},
    };
    for (const auto &f : fixed) run_case(f.name, [&](std::string &d) { return clusters_case(f.iv, &f.want, d); });
    run_case("clusters_random", [&](std::string &d) {
        Rng rng(11);
        Hash all;
        bool ok = true;
        for (int it = 0; it < 200; it++) {
            const int n = 1 + rng.below(8), nw = 1 + rng.below(4);
            std::vector<PhiAnchorIv> iv;
            for (int a = 0; a < n; a++) { const int lo = rng.below(12); iv.push_back(PhiAnchorIv{lo, lo + rng.below(4), rng.below(nw), a}); }
            std::string one;
            ok = clusters_case(iv, nullptr, one) && ok;
            for (char ch : one) all.add(ch);
        }
        d = fmt("sets=200 hash=%016llx", (unsigned long long)all.h);
        return ok;
    });
}

// ------------------------------------------------------------------------------------------ chain
struct Blocks {
    int32_t nb, nwk;
    std::vector<int32_t> rows, rowend;                         // [nb][nwk + 1][64], [nb][nwk + 1]
    int32_t row(int b, int j, int h) const { return rows[((size_t)b * (nwk + 1) + j) * 64 + h]; }
};
namespace ref {
// best sum of a sequence that is on walk h at the end of block b (INT64_MIN: none): it began inside block b, or came in on a walk j
int64_t leaving(const Blocks &B, int b, int h)
{
    int64_t best = INT64_MIN;
    if (B.row(b, B.nwk, h) > PHI_DP_NEGK / 2) best = B.row(b, B.nwk, h);
    if (b > 0)
        for (int j = 0; j < B.nwk; j++) {
            const int64_t in = leaving(B, b - 1, j);
            if (in != INT64_MIN && B.row(b, j, h) > PHI_DP_NEGK / 2) best = std::max(best, in + B.row(b, j, h));
        }
    return best;
}
int64_t ending(const Blocks &B)
{
    int64_t best = INT64_MIN;
    for (int b = 0; b < B.nb; b++)
        for (int j = 0; j <= B.nwk; j++) {
            const int32_t re = B.rowend[(size_t)b * (B.nwk + 1) + j];
            if (re <= -(1 << 27)) continue;
            if (j == B.nwk) best = std::max<int64_t>(best, re);
            else if (b > 0 && leaving(B, b - 1, j) != INT64_MIN) best = std::max(best, leaving(B, b - 1, j) + re);
        }
    return best;
}
}   // namespace ref

void test_chain()
{
    run_case("chain_random", [&](std::string &d) {
        Rng rng(23);
        Hash all;
        bool ok = true;
        for (int it = 0; it < 300; it++) {
            Blocks B;
            B.nb = 1 + rng.below(4); B.nwk = 1 + rng.below(3);
            B.rows.assign((size_t)B.nb * (B.nwk + 1) * 64, PHI_DP_NEGK);
            B.rowend.assign((size_t)B.nb * (B.nwk + 1), -(1 << 28));
            for (int b = 0; b < B.nb; b++)
                for (int j = 0; j <= B.nwk; j++) {
                    for (int h = 0; h < B.nwk; h++) if (rng.chance(65)) B.rows[((size_t)b * (B.nwk + 1) + j) * 64 + h] = rng.below(200) - 100;
                    if (rng.chance(50)) B.rowend[(size_t)b * (B.nwk + 1) + j] = rng.below(200) - 100;
                }
            std::vector<int32_t> S;
            const int64_t end_best = phi_chain_blocks(B.rows.data(), B.rowend.data(), B.nb, B.nwk, S);
            ok = ok && S.size() == (size_t)B.nb * 64 && end_best == ref::ending(B);
            for (int b = 0; b < B.nb && ok; b++)
                for (int h = 0; h < 64; h++) {
                    const int64_t want = b > 0 && h < B.nwk ? ref::leaving(B, b - 1, h) : INT64_MIN;
                    ok = ok && S[(size_t)b * 64 + h] == (want == INT64_MIN ? PHI_DP_NEGK : (int32_t)want);
                }
            all.add_all(S);
            all.add(end_best);
        }
        d = fmt("chains=300 hash=%016llx", (unsigned long long)all.h);
        return ok;
    });
    // the second pass against the chain: two blocks of two walks
    auto agree = [](int32_t want0, int32_t got0, std::string &d) {
        std::vector<int32_t> S(2 * 64, PHI_DP_NEGK), keys(2 * 64, PHI_DP_NEGK);
        S[64 + 0] = 7; keys[0] = 7;
        S[64 + 1] = want0; keys[1] = got0;
        int32_t b = -1, h = -1, got = 0, want = 0;
        const bool same = phi_chain_agrees(S.data(), keys.data(), 2, 2, &b, &h, &got, &want);
        d = same ? "agree" : fmt("block %d walk %d got %d want %d", b, h, got, want);
        return same;
    };
    run_case("chain_key_differs", [&](std::string &d) { return !agree(5, 4, d) && d == "block 0 walk 1 got 4 want 5"; });
    run_case("chain_key_against_no_run", [&](std::string &d) { return !agree(PHI_DP_NEGK, 4, d); });
    // (two "no run" values of different bits: NEGK itself and NEGK plus a cost that was subtracted on the way)
    run_case("chain_both_no_run", [&](std::string &d) { return agree(PHI_DP_NEGK, PHI_DP_NEGK - 200, d) && d == "agree"; });
}

// ------------------------------------------------------------------------------------------ anchor arrays
struct Kept {
    std::vector<PhiAnchorHost> a;
    std::vector<int64_t> walk_off;
};
// n anchors three entries apart, spans from span_of(i), over nw walks of equal length
Kept make_kept(int64_t n, int32_t nw, const std::function<uint32_t(int64_t)> &span_of)
{
    Kept K;
    for (int64_t i = 0; i < n; i++) K.a.push_back(PhiAnchorHost{(uint32_t)(i % 97), (uint32_t)(3 * i), (uint32_t)(3 * i) + span_of(i)});
    const int64_t n_entries = 3 * n + 40;
    for (int32_t h = 0; h <= nw; h++) K.walk_off.push_back(n_entries * h / nw);
    return K;
}
std::string anchor_arrays_line(Kept &K, int32_t k, bool *agreed)
{
    const int32_t nw = (int32_t)K.walk_off.size() - 1;
    const PhiAnchorSpan kept{K.a.data(), (int64_t)K.a.size()};
    std::vector<PhiAnchorHost> own;
    PhiAnchorArrays A;
    std::vector<int64_t> n_anchors;
    PhiHostError err;
    if (phi_anchor_arrays(kept, K.walk_off.data(), nw, k, own, A, n_anchors, err)) return fmt("refused %d %s", err.code, err.msg.c_str());
    // the restatement: one loop
    std::vector<int64_t> r_n(nw, 0);
    std::vector<PhiAnchorHost> r_dp;
    std::vector<int16_t> r_walk;
    for (const PhiAnchorHost &a : K.a) {
        int32_t h = 0;
        while (!(K.walk_off[h] <= (int64_t)a.e0 && (int64_t)a.e0 < K.walk_off[h + 1])) h++;
        r_n[h]++;
        if (a.e1 > a.e0) { r_dp.push_back(a); r_walk.push_back((int16_t)h); }
    }
    const bool same = r_dp.size() == K.a.size();
    bool ok = n_anchors == r_n && A.dp.size() == r_dp.size() && A.dp_walk == r_walk && A.a_e1.size() == r_dp.size() && A.a_span.size() == r_dp.size();
    ok = ok && (same ? A.dp.p == kept.p && own.empty() : A.dp.p == own.data() && own.size() == r_dp.size());
    Hash h;
    for (size_t i = 0; i < r_dp.size() && ok; i++) {
        ok = A.dp[(int64_t)i].slot == r_dp[i].slot && A.dp[(int64_t)i].e0 == r_dp[i].e0 && A.dp[(int64_t)i].e1 == r_dp[i].e1 && A.a_e1[i] == r_dp[i].e1 &&
             A.a_span[i] == r_dp[i].e1 - r_dp[i].e0;
        h.add(r_dp[i].e1); h.add(A.a_span[i]); h.add(A.dp_walk[i]);
    }
    h.add_all(n_anchors);
    *agreed = ok;
    return fmt("kept=%zu dp=%zu %s hash=%016llx", K.a.size(), r_dp.size(), same ? "same_as_kept" : "own_list", (unsigned long long)h.h);
}
void test_anchor_arrays()
{
    const int64_t big = 3 * 65536 + 17;
    auto mixed = [](int64_t i) { return (uint32_t)((i * 2654435761u >> 7) % 4); };       // spans 0..3: single-vertex anchors mixed in
    auto edge = [](int64_t i) { return (uint32_t)(1 + i % 3); };
    const struct { const char *name; int64_t n; int32_t nw; std::function<uint32_t(int64_t)> span; } cases[] = {
        {"anchors_none", 0, 2, edge}, {"anchors_one", 1, 2, edge}, {"anchors_all_span", 50, 3, edge}, {"anchors_mixed", 50, 3, mixed},
        {"anchors_three_chunks", big, 5, mixed},
    };
    for (const auto &cs : cases)
        run_case(cs.name, [&](std::string &d) {
            Kept K = make_kept(cs.n, cs.nw, cs.span);
            bool ok = false;
            d = anchor_arrays_line(K, 31, &ok);
            return ok;
        });
    bool unused = false;
    run_refusal("anchors_span_rcap", [&]() {
        Kept K = make_kept(50, 3, [](int64_t i) { return i == 20 ? (uint32_t)PHI_RCAP : 1u; });
        return anchor_arrays_line(K, 31, &unused);
    });
    run_refusal("anchors_span_rcap_long_k", [&]() {
        Kept K = make_kept(50, 3, [](int64_t i) { return i == 20 ? (uint32_t)PHI_RCAP : 1u; });
        return anchor_arrays_line(K, 33, &unused);
    });
    run_refusal("anchors_unsorted_across_chunks", [&]() {
        // every anchor spans an edge, so dp index = kept index: anchor 65535 ends one entry behind anchor 65536
        Kept K = make_kept(big, 5, [](int64_t i) { return i == 65535 ? 5u : 1u; });
        return anchor_arrays_line(K, 31, &unused);
    });
    run_case("score_bound_random", [&](std::string &d) {
        Rng rng(5);
        Hash all;
        bool ok = true;
        for (int it = 0; it < 100; it++) {
            const int n_vtx = 1 + rng.below(6), ne = 1 + rng.below(20), n = rng.below(40);
            std::vector<int32_t> walk_vtx(ne);
            for (int32_t &v : walk_vtx) v = rng.below(n_vtx);
            std::vector<uint32_t> e1(n);
            for (uint32_t &e : e1) e = (uint32_t)rng.below(ne);
            std::sort(e1.begin(), e1.end());
            int64_t want = 0;
            for (int v = 0; v < n_vtx; v++) {
                int64_t most = 0;
                for (int e = 0; e < ne; e++) if (walk_vtx[e] == v) most = std::max<int64_t>(most, std::count(e1.begin(), e1.end(), (uint32_t)e));
                want += most;
            }
            const int64_t got = phi_score_bound(e1.data(), n, walk_vtx.data(), n_vtx);
            ok = ok && got == want;
            all.add(got);
        }
        d = fmt("models=100 hash=%016llx", (unsigned long long)all.h);
        return ok;
    });
}

// ------------------------------------------------------------------------------------------ block placement
namespace ref {
// 0: the chain stays whole
int32_t place(const std::vector<int32_t> &graph_ok, const std::vector<int32_t> &closed, int32_t nk, const std::vector<int32_t> &rings, bool no_small,
              const std::function<int64_t(int32_t)> &target_of, std::vector<int32_t> &lo)
{
    auto allowed = [&](int64_t k) { return k > 0 && k < nk && graph_ok[(size_t)k] != 0 && closed[(size_t)k] == 0; };
    for (int32_t ring : rings) {
        if (no_small && ring == 256) continue;
        const int64_t target = target_of(ring);
        lo = {0};
        bool failed = false;
        while (nk - lo.back() > target) {
            const int64_t start = lo.back(), last = std::min<int64_t>(start + ring, nk - 1);
            int64_t cut = -1;
            for (int64_t k = start + target; k <= last; k++) if (allowed(k)) { cut = k; break; }
            if (cut < 0) for (int64_t k = start + target - 1; k > start; k--) if (allowed(k)) { cut = k; break; }
            if (cut < 0) { failed = nk - start > ring; break; }
            lo.push_back((int32_t)cut);
        }
        if (!failed && nk - lo.back() <= ring) { lo.push_back(nk); return ring; }
    }
    return 0;
}
}   // namespace ref

bool blocks_case(const std::vector<int32_t> &graph_ok, const std::vector<int32_t> &closed, int32_t nk, bool no_small, int64_t target, int32_t want_ring,
                 std::string &d)
{
    const std::vector<int32_t> rings = {256, 1024, 2048};
    auto target_of = [&](int32_t ring) { return std::min<int64_t>(ring, target); };
    std::vector<int32_t> lo, r_lo;
    const PhiCutFlags flags{graph_ok.data(), closed.data(), nk};
    const int32_t ring = phi_place_blocks(flags, rings.data(), (int)rings.size(), no_small, target_of, lo);
    const int32_t r_ring = ref::place(graph_ok, closed, nk, rings, no_small, target_of, r_lo);
    bool ok = ring == r_ring && (want_ring < 0 || ring == want_ring);
    if (ring) {
        ok = ok && lo == r_lo && lo.front() == 0 && lo.back() == nk;
        for (size_t b = 0; b + 1 < lo.size() && ok; b++) {
            ok = lo[b + 1] > lo[b] && lo[b + 1] - lo[b] <= ring;                                  // every block at most one ring long
            if (b > 0) ok = ok && graph_ok[(size_t)lo[b]] && closed[(size_t)lo[b]] == 0;              // every cut is allowed
        }
    }
    Hash h;
    if (ring) h.add_all(lo);
    d = fmt("steps=%d ring=%d blocks=%zu hash=%016llx", nk, ring, ring ? lo.size() - 1 : (size_t)0, (unsigned long long)h.h);
    return ok;
}
void test_blocks()
{
    run_case("blocks_below_target", [&](std::string &d) {
        const int32_t nk = 50;
        return blocks_case(std::vector<int32_t>(nk + 1, 1), std::vector<int32_t>(nk + 2, 0), nk, false, 64, 256, d) && d.find("blocks=1 ") != std::string::npos;
    });
    // steps 100 .. 499 closed: 400 steps without a cut, more than a ring of 256 holds
    const int32_t nk = 1500;
    std::vector<int32_t> graph_ok(nk + 1, 1), closed(nk + 2, 0);
    for (int32_t k = 100; k < 500; k++) closed[(size_t)k] = 1;
    run_case("blocks_long_stretch", [&](std::string &d) { return blocks_case(graph_ok, closed, nk, false, 64, 1024, d); });
    run_case("blocks_long_stretch_no_small", [&](std::string &d) { return blocks_case(graph_ok, closed, nk, true, 64, 1024, d); });
    // (every cut allowed: placed at 256 -- unless the small blocks are ruled out)
    run_case("blocks_open", [&](std::string &d) { return blocks_case(graph_ok, std::vector<int32_t>(nk + 2, 0), nk, false, 64, 256, d); });
    run_case("blocks_open_no_small", [&](std::string &d) { return blocks_case(graph_ok, std::vector<int32_t>(nk + 2, 0), nk, true, 64, 1024, d); });
    run_case("blocks_random", [&](std::string &d) {
        Rng rng(37);
        Hash all;
        bool ok = true;
        int placed = 0, whole = 0;
        for (int it = 0; it < 300; it++) {
            const int32_t n = 4 + rng.below(6000);
            const int dens = 1 + rng.below(60);
            std::vector<int32_t> g(n + 1), cl(n + 2);
            for (int32_t &x : g) x = rng.chance(dens);
            if (it % 3 == 0) { std::fill(g.begin(), g.end(), 0); for (int i = rng.below(4); i > 0; i--) g[(size_t)rng.below(n + 1)] = 1; }   // (so sparse that rings fail)
            for (int32_t &x : cl) x = rng.chance(30) ? 1 + rng.below(3) : 0;
            std::string one;
            ok = blocks_case(g, cl, n, rng.chance(30), 1 + rng.below(700), -1, one) && ok;
            (one.find("ring=0 ") != std::string::npos ? whole : placed)++;
            for (char ch : one) all.add(ch);
        }
        d = fmt("chains=300 placed=%d whole=%d hash=%016llx", placed, whole, (unsigned long long)all.h);
        return ok && placed > 0 && whole > 0;
    });
}

// ------------------------------------------------------------------------------------------ CSR and repeats
void test_csr()
{
    run_case("csr_repeats_random", [&](std::string &d) {
        Rng rng(41);
        Hash all;
        bool ok = true;
        for (int it = 0; it < 200; it++) {
            const int n = rng.below(65), n_ids = 1 + rng.below(16), nw = 1 + rng.below(4);
            std::vector<PhiAnchorHost> a(n);
            std::vector<int16_t> walk(n);
            for (int i = 0; i < n; i++) { a[i] = PhiAnchorHost{(uint32_t)rng.below(n_ids), (uint32_t)i, (uint32_t)i + 1}; walk[i] = (int16_t)rng.below(nw); }
            std::sort(walk.begin(), walk.end());                 // anchors come in walk order
            std::vector<int32_t> off, idx;
            ok = phi_anchor_csr(PhiAnchorSpan{a.data(), n}, n_ids, off, idx) && ok;
            std::set<uint32_t> S0, want0;
            phi_repeat_set(off, idx, walk, n_ids, S0);
            ok = ok && off.size() == (size_t)n_ids + 1 && off[0] == 0 && off[n_ids] == n && idx.size() == (size_t)std::max(n, 1);
            for (int u = 0; u < n_ids && ok; u++) {
                std::vector<int32_t> mine;
                for (int i = 0; i < n; i++) if (a[i].slot == (uint32_t)u) mine.push_back(i);
                ok = std::vector<int32_t>(idx.begin() + off[u], idx.begin() + off[u + 1]) == mine;
                for (int32_t i : mine) for (int32_t j : mine) if (i < j && walk[i] == walk[j]) want0.insert((uint32_t)u);
            }
            ok = ok && S0 == want0;
            all.add_all(off); all.add_all(idx);
            for (uint32_t s : S0) all.add(s);
        }
        d = fmt("models=200 hash=%016llx", (unsigned long long)all.h);
        return ok;
    });
    run_refusal("csr_id_out_of_range", [&]() {
        std::vector<PhiAnchorHost> a = {{0, 0, 1}, {3, 1, 2}, {1, 2, 3}};
        std::vector<int32_t> off, idx;
        return std::string(phi_anchor_csr(PhiAnchorSpan{a.data(), 3}, 3, off, idx) ? "accepted" : "refused id 3 of 3");
    });
}

// ------------------------------------------------------------------------------------------ tighten and branch
typedef std::set<uint32_t> U;
std::string show(const U &s)
{
    std::string o = "{";
    for (uint32_t x : s) o += fmt(o.size() > 1 ? ",%u" : "%u", x);
    return o + "}";
}
void test_tighten()
{
    // S, D, Z, seen -> moved?, the S and the seen afterwards
    auto tighten = [](U S, const U &D, const U &Z, std::set<U> seen, bool moved, const U &S_after, size_t seen_after, std::string &d) {
        const bool got = phi_tighten(S, D, Z, seen);
        d = fmt("%s S=%s seen=%zu", got ? "moved" : "stopped", show(S).c_str(), seen.size());
        return got == moved && S == S_after && seen.size() == seen_after;
    };
    run_case("tighten_nothing", [&](std::string &d) { return tighten({1, 2}, {}, {}, {}, false, {1, 2}, 0, d); });
    run_case("tighten_d_only", [&](std::string &d) { return tighten({1, 2}, {5}, {}, {}, true, {1, 2, 5}, 1, d); });
    run_case("tighten_z_only", [&](std::string &d) { return tighten({1, 2}, {}, {2}, {}, true, {1}, 1, d); });
    run_case("tighten_both", [&](std::string &d) { return tighten({1, 2}, {5, 6}, {1}, {}, true, {2, 5, 6}, 1, d); });
    run_case("tighten_revisit", [&](std::string &d) { return tighten({1, 2}, {5}, {2}, {{1, 5}}, false, {1, 2}, 1, d); });
    // anchors of minimisers 0 .. 3: {4, 9}, {2, 7}, {2}, {0}   (1 and 2 made to tie on purpose: the lower id wins)
    const std::vector<int32_t> sa_off = {0, 2, 4, 5, 6}, sa_idx = {4, 9, 2, 7, 2, 0};
    auto branch = [&](const U &D, const U &Z, const std::map<uint32_t, int32_t> &assign, int want, std::string &d) {
        uint32_t slot = 99;
        const bool got = phi_choose_branch(D, Z, assign, sa_off, sa_idx, &slot);
        d = got ? fmt("branch on %u", slot) : std::string("no branch");
        return want < 0 ? !got : got && slot == (uint32_t)want;
    };
    run_case("branch_lowest_first_anchor", [&](std::string &d) { return branch({0, 1}, {3}, {}, 1, d); });
    run_case("branch_tie", [&](std::string &d) { return branch({2, 1, 0}, {}, {}, 1, d); });
    run_case("branch_from_z", [&](std::string &d) { return branch({}, {0, 3}, {{3, 0}}, 0, d); });
    run_case("branch_none", [&](std::string &d) { return branch({}, {0, 3}, {{0, 1}, {3, 0}}, -1, d); });
}

}   // namespace

int main()
{
    test_clusters();
    test_chain();
    test_anchor_arrays();
    test_blocks();
    test_csr();
    test_tighten();
    if (n_failed) printf("FAILED %d case(s)\n", n_failed);
    return n_failed ? 1 : 0;
}
