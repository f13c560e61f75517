// dp_steps_selftest.cpp -- stand-alone check of ../dp_steps.h (the topology validation and the DP step stream of
// phi_set_graph) on the CPU: no GPU, no ROCm.  Built plain, with AddressSanitizer + UndefinedBehaviorSanitizer and with
// ThreadSanitizer by the Makefile's dp_steps_sanitize; tests/test_cpu_dp_steps.py runs the three and compares their output.
//
// Every case is a DAG with walks; the walks per edge (cnt_edge) are counted serially here, or fed directly.  The header's
// result at PHI_HOST_THREADS=1 and =8 must equal, array by array, a second implementation below (namespace ref) that is
// serial, written from the definitions and shares no code with the header:
//   * an edge x of u is LIVE when some walk on u continues along another out-edge: sum of cnt_edge over u's out-edges
//     minus cnt_edge[x] > 0;
//   * dense record of step s, v = topo[s]: word 0 = ENTRY (v has a live in-edge) | TOPS (v has a live out-edge) | n_in << 8;
//     the live in-edges as (rank[v] - rank[u]) << 8 | index of x among u's out-edges, ascending, the first three in words
//     2-4, the rest in in_packed from word 1; word 5 = v; words 6-7 = 0;
//   * compact steps: the steps with ENTRY or TOPS or whose vertex is the first or last of a walk (LANE_ONLY); cstep / kstep
//     mutually inverse, cstep -1 elsewhere; in-edges re-based to compact steps back; cvtx[v] = cstep[rank[v]];
//   * PAIR, greedily from the left and without overlap: two consecutive compact steps on adjacent topological steps, neither
//     with TOPS, no edge from the first vertex to the second;
//   * cut_ok[k] = 1 exactly when 0 < k < n_k, no in-edge of a step >= k comes from a step < k, and step k - 1 is no PAIR.
// One line per case on stdout: name, sizes and a hash of every output array.  Exit status 0 = every case agreed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <set>
#include <string>
#include <utility>
#include <vector>
#include "../dp_steps.h"

namespace {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    bool chance(int percent) { return below(100) < percent; }
};

struct Graph {
    int32_t n_vtx = 0;
    std::vector<int64_t> adj_off;
    std::vector<int32_t> adj, rank, cnt_edge;
    std::vector<std::vector<int32_t>> walks;
    std::vector<int32_t> ends() const
    {
        std::vector<int32_t> e;
        for (const auto &w : walks) { e.push_back(w.front()); e.push_back(w.back()); }
        return e;
    }
};

// edges (u, v) in any order -> adjacency by vertex, in the order given
void set_edges(Graph &g, const std::vector<std::pair<int32_t, int32_t>> &edges)
{
    g.adj_off.assign((size_t)g.n_vtx + 1, 0);
    for (const auto &e : edges) g.adj_off[(size_t)e.first + 1]++;
    for (int32_t v = 0; v < g.n_vtx; v++) g.adj_off[(size_t)v + 1] += g.adj_off[(size_t)v];
    g.adj.assign(edges.size(), 0);
    std::vector<int64_t> cur(g.adj_off.begin(), g.adj_off.end() - 1);
    for (const auto &e : edges) g.adj[(size_t)cur[(size_t)e.first]++] = e.second;
}

// walks per edge, serially; a walk that steps where no edge is: a mistake of the generator
bool count_edges(Graph &g)
{
    g.cnt_edge.assign(std::max<size_t>(g.adj.size(), 1), 0);
    for (const auto &w : g.walks)
        for (size_t i = 0; i + 1 < w.size(); i++) {
            int64_t x = g.adj_off[(size_t)w[i]];
            while (x < g.adj_off[(size_t)w[i] + 1] && g.adj[(size_t)x] != w[i + 1]) x++;
            if (x == g.adj_off[(size_t)w[i] + 1]) return false;
            g.cnt_edge[(size_t)x]++;
        }
    return true;
}

namespace ref {

struct Steps {
    std::vector<int32_t> topo, st_rec, in_packed, k_rec, k_in, cvtx, cstep, kstep, cut_ok;
    std::vector<int64_t> indeg;
    int32_t n_k = 0;
    int64_t n_pairs = 0;
};

Steps build(const Graph &g, bool compact)
{
    Steps R;
    const int32_t n = g.n_vtx;
    R.topo.assign((size_t)n, -1);
    for (int32_t v = 0; v < n; v++) R.topo[(size_t)g.rank[(size_t)v]] = v;
    R.indeg.assign((size_t)n, 0);
    // live edges, gathered at their targets
    std::vector<std::vector<std::pair<int32_t, int32_t>>> in((size_t)n);     // per vertex: (source vertex, index among its out-edges)
    std::vector<char> has_live_out((size_t)n, 0), is_end((size_t)n, 0);
    for (int32_t u = 0; u < n; u++) {
        int64_t total = 0;
        for (int64_t x = g.adj_off[(size_t)u]; x < g.adj_off[(size_t)u + 1]; x++) total += g.cnt_edge[(size_t)x];
        for (int64_t x = g.adj_off[(size_t)u]; x < g.adj_off[(size_t)u + 1]; x++) {
            R.indeg[(size_t)g.adj[(size_t)x]]++;
            if (total - g.cnt_edge[(size_t)x] > 0) {
                in[(size_t)g.adj[(size_t)x]].push_back({u, (int32_t)(x - g.adj_off[(size_t)u])});
                has_live_out[(size_t)u] = 1;
            }
        }
    }
    for (const auto &w : g.walks) { is_end[(size_t)w.front()] = 1; is_end[(size_t)w.back()] = 1; }
    R.st_rec.assign((size_t)n * 8, 0);
    for (int32_t s = 0; s < n; s++) {
        const int32_t v = R.topo[(size_t)s];
        std::vector<int32_t> codes;
        for (const auto &e : in[(size_t)v]) codes.push_back(((g.rank[(size_t)v] - g.rank[(size_t)e.first]) << 8) | e.second);
        std::sort(codes.begin(), codes.end());
        int32_t *r = &R.st_rec[(size_t)s * 8];
        r[0] = (codes.empty() ? 0 : PHI_DP_NEED_ENTRY) | (has_live_out[(size_t)v] ? PHI_DP_NEED_TOPS : 0) | ((int32_t)codes.size() << 8);
        r[1] = (int32_t)R.in_packed.size();
        for (size_t j = 0; j < codes.size(); j++) {
            if (j < 3) r[2 + j] = codes[j];
            else R.in_packed.push_back(codes[j]);
        }
        r[5] = v;
    }
    if (!compact) return R;
    R.cstep.assign((size_t)n, -1);
    for (int32_t s = 0; s < n; s++) {
        const int32_t v = R.topo[(size_t)s];
        if (!in[(size_t)v].empty() || has_live_out[(size_t)v] || is_end[(size_t)v]) { R.cstep[(size_t)s] = (int32_t)R.kstep.size(); R.kstep.push_back(s); }
    }
    R.n_k = (int32_t)R.kstep.size();
    R.k_rec.assign((size_t)R.n_k * 8, 0);
    R.cvtx.assign((size_t)n, 0);
    for (int32_t v = 0; v < n; v++) R.cvtx[(size_t)v] = R.cstep[(size_t)g.rank[(size_t)v]];
    std::vector<int32_t> cut_diff((size_t)R.n_k + 2, 0);                    // +1 over the cuts an in-edge crosses
    for (int32_t k = 0; k < R.n_k; k++) {
        const int32_t v = R.topo[(size_t)R.kstep[(size_t)k]];
        std::vector<int32_t> codes;
        for (const auto &e : in[(size_t)v]) {
            const int32_t k_src = R.cvtx[(size_t)e.first];                  // (a vertex with a live out-edge is a compact step)
            codes.push_back(((k - k_src) << 8) | e.second);
            cut_diff[(size_t)k_src + 1]++; cut_diff[(size_t)k + 1]--;        // cuts before steps k_src + 1 .. k
        }
        std::sort(codes.begin(), codes.end());
        int32_t *r = &R.k_rec[(size_t)k * 8];
        r[0] = (codes.empty() ? 0 : PHI_DP_NEED_ENTRY) | (has_live_out[(size_t)v] ? PHI_DP_NEED_TOPS : 0) | (is_end[(size_t)v] ? PHI_DP_LANE_ONLY : 0) |
               ((int32_t)codes.size() << 8);
        r[1] = (int32_t)R.k_in.size();
        for (size_t j = 0; j < codes.size(); j++) {
            if (j < 3) r[2 + j] = codes[j];
            else R.k_in.push_back(codes[j]);
        }
        r[5] = v;
    }
    for (int32_t k = 0; k + 1 < R.n_k;) {
        const int32_t v0 = R.topo[(size_t)R.kstep[(size_t)k]], v1 = R.topo[(size_t)R.kstep[(size_t)k + 1]];
        bool ok = R.kstep[(size_t)k + 1] == R.kstep[(size_t)k] + 1 && !has_live_out[(size_t)v0] && !has_live_out[(size_t)v1];
        for (int64_t x = g.adj_off[(size_t)v0]; ok && x < g.adj_off[(size_t)v0 + 1]; x++) ok = g.adj[(size_t)x] != v1;
        if (ok) { R.k_rec[(size_t)k * 8] |= PHI_DP_PAIR; R.n_pairs++; k += 2; }
        else k++;
    }
    R.cut_ok.assign((size_t)R.n_k + 1, 0);
    int32_t crossing = 0;
    for (int32_t k = 0; k <= R.n_k; k++) {
        crossing += cut_diff[(size_t)k];
        const bool inside = k > 0 && k < R.n_k;
        R.cut_ok[(size_t)k] = inside && crossing == 0 && !(R.k_rec[(size_t)(k - 1) * 8] & PHI_DP_PAIR);
    }
    return R;
}

}  // namespace ref

uint64_t fnv(uint64_t h, const void *p, size_t bytes)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < bytes; i++) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}
template <class T> uint64_t fnv_vec(uint64_t h, const std::vector<T> &v)
{
    const uint64_t n = v.size();
    h = fnv(h, &n, 8);
    return v.empty() ? h : fnv(h, v.data(), v.size() * sizeof(T));
}

int n_failed = 0;
void fail(const std::string &name, const char *what)
{
    printf("%s FAILED: %s\n", name.c_str(), what);
    n_failed++;
}

struct Outcome { int code = 0; std::string msg; };

// the header at `threads` host threads, against the reference; *hash = of every output array
Outcome run_header(const Graph &g, bool compact, int threads, const ref::Steps *want, const std::string &name, uint64_t *hash)
{
    char buf[16];
    snprintf(buf, sizeof buf, "%d", threads);
    setenv("PHI_HOST_THREADS", buf, 1);
    Outcome o;
    PhiHostError err;
    std::vector<int32_t> topo;
    std::vector<int64_t> indeg((size_t)g.n_vtx, 0);
    if (phi_topo_from_ranks(g.n_vtx, g.rank.data(), topo, err) || phi_check_edges(g.n_vtx, g.adj_off.data(), g.adj.data(), g.rank.data(), indeg.data(), err)) {
        o.code = err.code; o.msg = err.msg;
        return o;
    }
    const std::vector<int32_t> ends = g.ends();
    const PhiDpGraph dg{g.n_vtx, (int32_t)g.walks.size(), g.adj_off.data(), g.adj.data(), g.rank.data(), topo.data(), g.cnt_edge.data(), ends.data()};
    PhiDpSteps st;
    if (phi_dp_steps_dense(dg, st, err) || (compact && phi_dp_steps_compact(dg, st, err))) {
        o.code = err.code; o.msg = err.msg;
        return o;
    }
    if (compact) phi_dp_steps_cuts(st);
    const std::vector<int32_t> st_rec(st.st_rec.get(), st.st_rec.get() + (size_t)g.n_vtx * 8);
    uint64_t h = 0xCBF29CE484222325ull;
    h = fnv_vec(h, topo); h = fnv_vec(h, indeg); h = fnv_vec(h, st_rec); h = fnv_vec(h, st.in_packed);
    h = fnv_vec(h, st.k_rec); h = fnv_vec(h, st.k_in); h = fnv_vec(h, st.cvtx); h = fnv_vec(h, st.cstep); h = fnv_vec(h, st.kstep); h = fnv_vec(h, st.cut_ok);
    h = fnv(h, &st.n_k, 4); h = fnv(h, &st.n_pairs, 8);
    *hash = h;
    if (want) {
        if (topo != want->topo) fail(name, "topo");
        if (indeg != want->indeg) fail(name, "indeg");
        if (st_rec != want->st_rec) fail(name, "st_rec");
        if (st.in_packed != want->in_packed) fail(name, "in_packed");
        if (compact) {
            if (st.n_k != want->n_k || st.n_pairs != want->n_pairs) fail(name, "n_k / n_pairs");
            if (st.k_rec != want->k_rec) fail(name, "k_rec");
            if (st.k_in != want->k_in) fail(name, "k_in");
            if (st.cvtx != want->cvtx) fail(name, "cvtx");
            if (st.cstep != want->cstep) fail(name, "cstep");
            if (st.kstep != want->kstep) fail(name, "kstep");
            if (st.cut_ok != want->cut_ok) fail(name, "cut_ok");
            // cstep and kstep are mutually inverse
            for (int32_t k = 0; k < st.n_k; k++) if (st.cstep[(size_t)st.kstep[(size_t)k]] != k) { fail(name, "cstep[kstep[k]] != k"); break; }
        }
    }
    return o;
}

// a case the header must accept: the reference once, the header at 1 and at 8 threads, with and without the compact stream
ref::Steps accepted(const std::string &name, const Graph &g)
{
    const ref::Steps want = ref::build(g, true);
    uint64_t h1 = 0, h8 = 0, hd = 0;
    const Outcome a = run_header(g, true, 1, &want, name, &h1), b = run_header(g, true, 8, &want, name, &h8), d = run_header(g, false, 8, &want, name, &hd);
    if (a.code || b.code || d.code) fail(name, (a.code ? a.msg : b.code ? b.msg : d.msg).c_str());
    else if (h1 != h8) fail(name, "1 and 8 threads differ");
    printf("%s ok vertices=%d edges=%zu walks=%zu compact=%d pairs=%lld spilled=%zu hash=%016llx\n", name.c_str(), g.n_vtx, g.adj.size(), g.walks.size(),
           want.n_k, (long long)want.n_pairs, want.in_packed.size(), (unsigned long long)h1);
    return want;
}

// a case the header must refuse, with this code and a text that starts like this
void refused(const std::string &name, const Graph &g, int code, const char *text)
{
    for (int threads : {1, 8}) {
        uint64_t h = 0;
        const Outcome o = run_header(g, true, threads, nullptr, name, &h);
        if (o.code != code || o.msg.compare(0, strlen(text), text) != 0) fail(name, ("got: " + std::to_string(o.code) + " " + o.msg).c_str());
    }
    printf("%s refused %d %s\n", name.c_str(), code, text);
}

// n sources 0 .. n-1, each with an edge to the hub n and one to the sink n + 1; one walk goes 0 -> sink, the rest of
// cnt_edge is fed directly: a walk on every source towards the sink makes each of the hub's n in-edges live
Graph star(int32_t n)
{
    Graph g;
    g.n_vtx = n + 2;
    std::vector<std::pair<int32_t, int32_t>> edges;
    for (int32_t i = 0; i < n; i++) { edges.push_back({i, n}); edges.push_back({i, n + 1}); }
    set_edges(g, edges);
    for (int32_t v = 0; v < g.n_vtx; v++) g.rank.push_back(v);
    g.walks = {{0, n + 1}};
    g.cnt_edge.assign(g.adj.size(), 0);
    for (int32_t i = 0; i < n; i++) g.cnt_edge[(size_t)g.adj_off[(size_t)i] + 1] = 1;
    return g;
}

// A chain of sites: backbone, one to three alleles, backbone, ...; extra forward edges (deletions among them); vertex ids
// shuffled against the topological order; walks follow edges from a random start until a sink or a random stop.
Graph bubble_chain(Rng &rng, int32_t n_target, int n_walks, int extra_percent)
{
    Graph g;
    std::vector<int32_t> order;                                             // by topological position: a label of the layout
    std::vector<std::pair<int32_t, int32_t>> pos_edges;                     // between positions
    int32_t pos = 0, backbone = pos++;
    while (pos + 2 <= n_target) {
        const int n_alleles = std::min<int>(1 + rng.below(3), n_target - pos - 1);
        const int32_t next = pos + n_alleles;
        for (int a = 0; a < n_alleles; a++) { pos_edges.push_back({backbone, pos + a}); pos_edges.push_back({pos + a, next}); }
        backbone = next;
        pos = next + 1;
    }
    if (pos < n_target) { pos_edges.push_back({backbone, pos}); pos++; }    // (exactly n_target vertices)
    const int32_t n = g.n_vtx = pos;
    std::set<std::pair<int32_t, int32_t>> have(pos_edges.begin(), pos_edges.end());
    const int64_t n_extra = (int64_t)n * extra_percent / 100;
    for (int64_t i = 0; i < n_extra && n > 1; i++) {
        const int32_t a = rng.below(n - 1), b = a + 1 + rng.below(std::min(n - 1 - a, 6));
        if (have.insert({a, b}).second) pos_edges.push_back({a, b});
    }
    std::vector<int32_t> id_of((size_t)n);                                  // position -> vertex id
    for (int32_t i = 0; i < n; i++) id_of[(size_t)i] = i;
    for (int32_t i = n - 1; i > 0; i--) std::swap(id_of[(size_t)i], id_of[(size_t)rng.below(i + 1)]);
    g.rank.assign((size_t)n, 0);
    for (int32_t i = 0; i < n; i++) g.rank[(size_t)id_of[(size_t)i]] = i;
    for (int64_t i = (int64_t)pos_edges.size() - 1; i > 0; i--) std::swap(pos_edges[(size_t)i], pos_edges[(size_t)rng.below((int)(i + 1))]);
    std::vector<std::pair<int32_t, int32_t>> edges;
    for (const auto &e : pos_edges) edges.push_back({id_of[(size_t)e.first], id_of[(size_t)e.second]});
    set_edges(g, edges);
    for (int h = 0; h < n_walks; h++) {
        int32_t v = id_of[(size_t)(rng.chance(70) ? 0 : rng.below(n))];
        std::vector<int32_t> w{v};
        const int stop_per_mille = rng.chance(60) ? 0 : 1 + rng.below(100);
        while (g.adj_off[(size_t)v + 1] > g.adj_off[(size_t)v] && rng.below(1000) >= stop_per_mille) {
            v = g.adj[(size_t)g.adj_off[(size_t)v] + (size_t)rng.below((int)(g.adj_off[(size_t)v + 1] - g.adj_off[(size_t)v]))];
            w.push_back(v);
        }
        g.walks.push_back(w);
    }
    return g;
}

Graph from_lists(int32_t n, const std::vector<std::pair<int32_t, int32_t>> &edges, const std::vector<int32_t> &rank, const std::vector<std::vector<int32_t>> &walks)
{
    Graph g;
    g.n_vtx = n;
    set_edges(g, edges);
    g.rank = rank;
    g.walks = walks;
    return g;
}

}  // namespace

int main()
{
    // ---- the smallest shapes
    {
        Graph g = from_lists(1, {}, {0}, {{0}});
        if (!count_edges(g)) return 2;
        const ref::Steps r = accepted("one_vertex", g);
        if (r.n_k != 1 || r.cut_ok != std::vector<int32_t>{0, 0}) fail("one_vertex", "expected one compact step and no cut");
    }
    {
        Graph g = from_lists(2, {{1, 0}}, {1, 0}, {{1, 0}});
        if (!count_edges(g)) return 2;
        const ref::Steps r = accepted("two_vertices", g);
        if (r.n_k != 2 || r.n_pairs != 0 || r.cut_ok != std::vector<int32_t>{0, 1, 0}) fail("two_vertices", "expected two compact steps, no pair, one cut");
    }
    {
        // one bi-allelic site: 0 -> {1, 2} -> 3, a walk through either allele
        Graph g = from_lists(4, {{0, 1}, {0, 2}, {1, 3}, {2, 3}}, {0, 1, 2, 3}, {{0, 1, 3}, {0, 2, 3}});
        if (!count_edges(g)) return 2;
        const ref::Steps r = accepted("one_site", g);
        if (r.n_pairs != 1 || !(r.k_rec[(size_t)r.cvtx[1] * 8] & PHI_DP_PAIR) || r.cut_ok[(size_t)r.cvtx[2]] != 0) fail("one_site", "expected the two alleles as one pair, no cut inside it");
    }
    {
        // walks that start and end at interior vertices of 0 -> 1 -> {2, 3} -> 4 -> 5
        Graph g = from_lists(6, {{0, 1}, {1, 2}, {1, 3}, {2, 4}, {3, 4}, {4, 5}}, {0, 1, 2, 3, 4, 5}, {{1, 2, 4}, {0, 1, 3, 4, 5}, {3, 4}});
        if (!count_edges(g)) return 2;
        const ref::Steps r = accepted("interior_ends", g);
        // (every vertex is a compact step here; all but vertex 2 begin or end a walk)
        for (int32_t v = 0; v < 6; v++)
            if (r.cvtx[(size_t)v] < 0 || ((r.k_rec[(size_t)r.cvtx[(size_t)v] * 8] & PHI_DP_LANE_ONLY) != 0) != (v != 2)) fail("interior_ends", "LANE_ONLY");
    }
    // ---- in-edges: the first spill into in_packed, the most a record holds, one more
    {
        // through real walks: two walks on every source, one to the hub and one to the sink
        Graph g = star(4);
        g.walks.clear();
        for (int32_t i = 0; i < 4; i++) { g.walks.push_back({i, 4}); g.walks.push_back({i, 5}); }
        if (!count_edges(g)) return 2;
        const ref::Steps r = accepted("four_in_edges", g);
        if (r.in_packed.size() != 2 || ((r.st_rec[4 * 8] >> 8) & 0xFF) != 4) fail("four_in_edges", "expected one spilled in-edge at the hub and one at the sink");
    }
    {
        const ref::Steps r = accepted("255_in_edges", star(255));
        if (((r.st_rec[255 * 8] >> 8) & 0xFF) != 255 || r.in_packed.size() != 252) fail("255_in_edges", "expected 255 in-edges at the hub");
    }
    refused("256_in_edges", star(256), PHI_ERR_UNSUPPORTED, "vertex 256 has more than 255 in-edges");
    // ---- the validation
    refused("not_a_permutation", from_lists(2, {{0, 1}}, {0, 0}, {{0, 1}}), PHI_ERR_INVALID, "topo_rank is not a permutation (vertex 1): is the graph cyclic?");
    refused("rank_out_of_range", from_lists(2, {{0, 1}}, {0, 2}, {{0, 1}}), PHI_ERR_INVALID, "topo_rank is not a permutation (vertex 1)");
    {
        Graph g = from_lists(2, {{0, 1}}, {1, 0}, {{0, 1}});
        if (!count_edges(g)) return 2;
        refused("backward_edge", g, PHI_ERR_INVALID, "edge 0->1 goes backwards in topo_rank: graph must be acyclic");
        g.rank = {0, 1}; g.adj[0] = 2;
        refused("edge_target_out_of_range", g, PHI_ERR_INVALID, "edge target 2 out of range");
    }
    // ---- random bubble chains with extra forward edges
    {
        Rng rng(20240607);
        uint64_t all = 0xCBF29CE484222325ull;
        int64_t n_pairs = 0, n_spilled = 0, n_cuts = 0;
        const int n_cases = 300;
        for (int i = 0; i < n_cases; i++) {
            Graph g = bubble_chain(rng, 2 + rng.below(39), 1 + rng.below(10), rng.below(200));
            if (!count_edges(g)) return 2;
            const std::string name = "random_" + std::to_string(i);
            const ref::Steps want = ref::build(g, true);
            uint64_t h1 = 0, h8 = 0;
            const Outcome a = run_header(g, true, 1, &want, name, &h1), b = run_header(g, true, 8, &want, name, &h8);
            if (a.code || b.code) fail(name, (a.code ? a.msg : b.msg).c_str());
            else if (h1 != h8) fail(name, "1 and 8 threads differ");
            all = fnv(all, &h1, 8);
            n_pairs += want.n_pairs; n_spilled += (int64_t)want.in_packed.size();
            for (int32_t x : want.cut_ok) n_cuts += x;
        }
        printf("random ok cases=%d pairs=%lld spilled=%lld cuts=%lld hash=%016llx\n", n_cases, (long long)n_pairs, (long long)n_spilled, (long long)n_cuts, (unsigned long long)all);
        if (n_pairs == 0 || n_spilled == 0 || n_cuts == 0) fail("random", "the cases never made a pair, a spilled in-edge or a cut");
    }
    // ---- more than one chunk of 65536 vertices: the threaded paths run
    {
        Rng rng(7);
        Graph g = bubble_chain(rng, 3 * 65536 + 17, 12, 30);
        if (g.n_vtx != 3 * 65536 + 17 || !count_edges(g)) return 2;
        accepted("three_chunks", g);
    }
    if (n_failed) { printf("%d checks failed\n", n_failed); return 1; }
    return 0;
}
