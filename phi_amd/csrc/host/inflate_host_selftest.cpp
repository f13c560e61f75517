// inflate_host_selftest.cpp -- stand-alone check of ../inflate_host.h (the rules of the device inflater that need no GPU, and
// the gzip header parser its decode kernel calls) on the CPU: no GPU, no ROCm.  Built plain and with AddressSanitizer +
// UndefinedBehaviorSanitizer by the Makefile's inflate_host_sanitize; tests/test_cpu_inflate_host.py runs both and compares
// their output.
//
// The header's results are compared with restatements below (namespace ref) that are serial, written from the rules'
// sentences and share no code with it:
//   * chunks: the fewest chunks of C bytes that hold n, in 128-bit arithmetic; C = the request, 64 at least, or the
//     environment's positive number, or 65536;
//   * capacity: floor(C * r * 1.25) + 4096 with r = ISIZE / n kept within [4, 1100], on values where the product is exact;
//   * chain: one scan over the chunks in order that waits for the chunk the last chain job stopped on;
//   * second run: offsets are the running sum of out_len + 1 over the chain's overflowed jobs;
//   * layout: a piece starts where the chain's earlier pieces end; the ends are the chain jobs' records in record order,
//     stably sorted by position; lo of a piece is the largest end not beyond its start, found by a scan of all ends;
//   * slabs / segments: they tile [0, len - 32768) / every member in order, full but for the last of each;
//   * CRC32: a register stepped bit by bit with the polynomial written here; the 64-bit shift against dfl_crc_shift applied
//     in pieces that fit 32 bits.
// One line per case on stdout: name, ok or FAILED, and what was found.  Exit status 0 = every case agreed.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "../inflate_host.h"

namespace {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    uint64_t below(uint64_t n) { return next() % n; }
};

int n_failed = 0;
std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char *f, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}
void line(const char *name, bool ok, const std::string &detail)
{
    if (!ok) n_failed++;
    printf("%s %s %s\n", name, ok ? "ok" : "FAILED", detail.c_str());
}

uint16_t *const SYM = (uint16_t *)(uintptr_t)0x40000000, *const SYM2 = (uint16_t *)(uintptr_t)0x7000000000;   // never read through

namespace ref {
typedef unsigned __int128 u128;

uint32_t step_bits(uint32_t r, uint64_t nbits)
{
    for (uint64_t k = 0; k < nbits; k++) r = (r & 1u) ? (r >> 1) ^ 0xEDB88320u : r >> 1;
    return r;
}
uint32_t raw(const uint8_t *p, size_t n, uint32_t r = 0)      // no inversions
{
    for (size_t i = 0; i < n; i++) r = step_bits(r ^ p[i], 8);
    return r;
}
uint32_t crc(const uint8_t *p, size_t n) { return ~raw(p, n, 0xffffffffu); }

// 0: the chain is whole; 1: a negative status at the chain's last job; 2: a result that cannot be followed
int chain(const std::vector<int> &job_of, const std::vector<InfResult> &res, std::vector<int> &out)
{
    const int nch = (int)job_of.size();
    int expect = 0;
    out.clear();
    for (int ch = 0; ch < nch; ch++) {
        if (ch != expect) continue;
        if (job_of[(size_t)ch] < 0) return 2;
        const InfResult &r = res[(size_t)job_of[(size_t)ch]];
        out.push_back(job_of[(size_t)ch]);
        if (r.status < 0) return 1;
        if (r.status == INF_END) return 0;
        if (r.end_chunk <= ch || r.end_chunk >= nch) return 2;
        if (job_of[(size_t)r.end_chunk] < 0) return 2;
        expect = r.end_chunk;
    }
    return 2;
}

struct End { int64_t abs; int idx; uint32_t crc, isize; };
struct Layout { std::vector<int64_t> abs, len, lo; std::vector<End> ends; int64_t total = 0; bool covered = false; };
Layout layout(const std::vector<int> &chain, const std::vector<InfResult> &res, const std::vector<InfMember> &mem)
{
    Layout L;
    for (size_t i = 0; i < chain.size(); i++) {
        int64_t before = 0;
        for (size_t j = 0; j < i; j++) before += res[(size_t)chain[j]].out_len;
        L.abs.push_back(before);
        L.len.push_back(res[(size_t)chain[i]].out_len);
        L.total = before + L.len.back();
    }
    for (size_t q = 0; q < mem.size(); q++)
        for (size_t i = 0; i < chain.size(); i++)
            if (chain[i] == mem[q].job) L.ends.push_back(End{L.abs[i] + mem[q].pos, (int)q, mem[q].crc, mem[q].isize});
    std::stable_sort(L.ends.begin(), L.ends.end(), [](const End &a, const End &b) { return a.abs < b.abs; });
    L.covered = !L.ends.empty() && L.ends.back().abs == L.total;
    for (size_t i = 0; i < chain.size(); i++) {
        int64_t lo = 0;
        for (const End &e : L.ends)
            if (e.abs <= L.abs[i] && e.abs > lo) lo = e.abs;
        L.lo.push_back(lo);
    }
    return L;
}
}  // namespace ref

// ------------------------------------------------------------------------------------------------ chunks, capacity, jobs

bool chunks_are(int64_t n, int64_t chunk_bytes, const char *env, int64_t C, std::string &d)
{
    InfChunks P{};
    InfErr err;
    const int rc = inf_chunk_plan(n, chunk_bytes, env, P, err);
    const ref::u128 want = ((ref::u128)n + (ref::u128)C - 1) / (ref::u128)C;
    d += fmt("%lld:%lld,%d ", (long long)n, (long long)P.C, P.nch);
    return rc == PHI_OK && err.code == 0 && P.C == C && (ref::u128)P.nch == want && (ref::u128)P.nch * C >= (ref::u128)n && (P.nch == 0 || (ref::u128)(P.nch - 1) * C < (ref::u128)n);
}

void chunk_cases()
{
    {
        std::string d;
        bool ok = true;
        const int64_t C = 4096;
        for (int64_t n : {(int64_t)0, (int64_t)1, C - 1, C, C + 1, 10 * C, 10 * C + 1}) ok = chunks_are(n, C, nullptr, C, d) && ok;
        line("chunk_n_around_C", ok, d);
    }
    {
        std::string d;
        bool ok = chunks_are(63, 1, "4096", 64, d);
        ok = chunks_are(64, 1, nullptr, 64, d) && ok;
        ok = chunks_are(65, 63, nullptr, 64, d) && ok;
        ok = chunks_are(129, 65, nullptr, 65, d) && ok;
        line("chunk_floor_64", ok, d);
    }
    {
        std::string d;
        bool ok = chunks_are(65536 * 3 + 1, 0, nullptr, PHI_INFLATE_CHUNK_DEFAULT, d);
        ok = chunks_are(65536, -5, nullptr, 65536, d) && ok;
        ok = chunks_are(65537, 0, "", 65536, d) && ok;
        ok = chunks_are(65537, 0, "0", 65536, d) && ok;
        ok = chunks_are(65537, 0, "-3", 65536, d) && ok;
        ok = chunks_are(65537, 0, "zlib", 65536, d) && ok;
        line("chunk_default_no_env", ok, d);
    }
    {
        std::string d;
        bool ok = chunks_are(100000, 0, "32768", 32768, d);
        ok = chunks_are(100, 0, "1", 1, d) && ok;                // (the environment's number is taken as it is)
        ok = chunks_are(100000, 8192, "32768", 8192, d) && ok;   // (a request goes before it)
        line("chunk_default_env", ok, d);
    }
    {
        const int64_t C = 64, edge = ((int64_t)1 << 30) * C;
        std::string d;
        bool ok = chunks_are(edge - C, C, nullptr, C, d);         // 2^30 - 1 chunks: the most
        for (int64_t n : {edge - C + 1, edge, INT64_MAX}) {
            InfChunks P{};
            InfErr err;
            const int rc = inf_chunk_plan(n, C, nullptr, P, err);
            const ref::u128 want = ((ref::u128)n + C - 1) / C;
            ok = ok && rc == PHI_ERR_UNSUPPORTED && err.code == rc && err.text == fmt("phi_inflate: %lld chunks", (long long)want);
            d += fmt("%lld:refused ", (long long)n);
        }
        line("chunk_2pow30_refused", ok, d);
    }
}

std::vector<uint8_t> stream_with_isize(size_t n, uint32_t isize)
{
    std::vector<uint8_t> v(n, 0xa5);
    for (int k = 0; k < 4 && n >= 4; k++) v[n - 4 + k] = (uint8_t)(isize >> (8 * k));
    return v;
}

void capacity_cases()
{
    const int64_t C = 4096;
    auto one = [&](const char *name, size_t n, uint32_t isize, int64_t want) {
        const std::vector<uint8_t> v = stream_with_isize(n, isize);
        const int64_t got = inf_sym_capacity(v.data(), (int64_t)n, C);
        line(name, got == want, fmt("n=%zu isize=%u cap=%lld", n, isize, (long long)got));
    };
    one("cap_short_stream", 17, 0xffffffffu, C * 5 + 4096);                  // n < 18: the last bytes are not looked at
    {
        const int64_t got = inf_sym_capacity(nullptr, 0, C);
        line("cap_empty_stream", got == C * 5 + 4096, fmt("cap=%lld", (long long)got));
    }
    one("cap_ratio_below_4", 1000, 1000, C * 5 + 4096);
    one("cap_ratio_between", 1000, 10000, C * 10 * 5 / 4 + 4096);
    one("cap_ratio_above_1100", 1000, 4000000000u, C * 1375 + 4096);
    one("cap_18_bytes_top_isize", 18, 0xffffffffu, C * 1375 + 4096);
    one("cap_ratio_exactly_1100", 1000, 1100000, C * 1375 + 4096);
}

void job_cases()
{
    {
        const std::vector<int64_t> starts = {80, -1, 5000, -1, -1, 9000, -1};
        std::vector<int> job_of, chunk_of;
        std::vector<InfJob> jobs;
        inf_job_index(starts, job_of, chunk_of);
        inf_job_list(starts, chunk_of, 1000, SYM, jobs);
        bool ok = job_of == std::vector<int>({0, -1, 1, -1, -1, 2, -1}) && chunk_of == std::vector<int>({0, 2, 5}) && jobs.size() == 3;
        std::string d;
        for (size_t k = 0; ok && k < jobs.size(); k++) {
            ok = jobs[k].start == starts[(size_t)chunk_of[k]] && jobs[k].cap == 1000 && jobs[k].sym == SYM + 1000 * k && jobs[k].chunk == chunk_of[k];
            d += fmt("%d@%lld+%lld ", jobs[k].chunk, (long long)jobs[k].start, (long long)(jobs[k].sym - SYM));
        }
        line("jobs_from_starts", ok, d);
    }
    {
        const int32_t a = inf_member_capacity(0, 1), b = inf_member_capacity(18 * 1000, 10), c = inf_member_capacity((int64_t)1 << 40, 5), e = inf_member_capacity(17, 0);
        line("member_capacity", a == 68 && b == 1000 + 40 + 64 && c == 1 << 30 && e == 64, fmt("%d %d %d %d", a, b, c, e));
    }
}

// ------------------------------------------------------------------------------------------------ the chain

struct ChainCase {
    std::vector<int64_t> starts;
    std::vector<int> job_of, chunk_of;
    std::vector<InfResult> res;
    explicit ChainCase(const std::vector<int> &has)
    {
        for (size_t i = 0; i < has.size(); i++) starts.push_back(has[i] ? (int64_t)(80 + 32768 * i) : -1);
        inf_job_index(starts, job_of, chunk_of);
        res.assign(chunk_of.size(), InfResult{0, 0, (int32_t)has.size(), INF_END, 0, 0});
    }
    InfResult &of_chunk(int ch) { return res[(size_t)job_of[(size_t)ch]]; }
    void stop(int ch, int on) { of_chunk(ch) = InfResult{1000 + ch, starts[(size_t)std::min<int>(std::max(on, 0), (int)starts.size() - 1)], on, INF_STOP, 0, 0}; }
    void end(int ch) { of_chunk(ch) = InfResult{1000 + ch, 8 * 4096 * (int64_t)starts.size(), (int32_t)starts.size(), INF_END, 0, 0}; }
    void bad(int ch, int status, int64_t bit) { of_chunk(ch) = InfResult{7, bit, (int32_t)starts.size(), status, 0, 0}; }
};

std::string ints(const std::vector<int> &v)
{
    std::string s;
    for (int x : v) s += fmt("%d,", x);
    return s.empty() ? "-" : s;
}

void chain_case(const char *name, ChainCase &c, int want_rc, const std::vector<int> &want_chain, const char *want_text)
{
    std::vector<int> chain, rchain;
    InfErr err;
    const int rc = inf_chain(c.job_of, c.res, chain, err);
    const int rr = ref::chain(c.job_of, c.res, rchain);
    bool ok = rc == want_rc && err.code == rc && rr == (rc == PHI_OK ? 0 : rc == PHI_ERR_INVALID ? 1 : 2);
    if (rc != PHI_ERR_DEVICE) ok = ok && chain == want_chain && chain == rchain;
    if (rc == PHI_ERR_DEVICE) ok = ok && strstr(err.text, "(internal error)") != nullptr;
    if (want_text) ok = ok && !strcmp(err.text, want_text);
    line(name, ok, fmt("rc=%d chain=%s %s", rc, ints(chain).c_str(), rc == PHI_ERR_INVALID ? err.text : ""));
}

void chain_cases()
{
    { ChainCase c({1}); c.end(0); chain_case("chain_single_job_end", c, PHI_OK, {0}, nullptr); }
    {
        ChainCase c({1, 1, 1, 1, 1, 1});
        for (int ch = 0; ch < 5; ch++) c.stop(ch, ch + 1);
        c.end(5);
        chain_case("chain_every_chunk_confirmed", c, PHI_OK, {0, 1, 2, 3, 4, 5}, nullptr);
    }
    { ChainCase c({1, 0, 0, 0, 0, 0}); c.end(0); chain_case("chain_no_start_but_chunk_0", c, PHI_OK, {0}, nullptr); }
    {
        ChainCase c({1, 0, 1, 1, 0, 1});                      // jobs 0..3 at chunks 0, 2, 3, 5; chunk 2's start is false
        c.stop(0, 3); c.stop(2, 3); c.stop(3, 5); c.end(5);
        chain_case("chain_false_start_dropped", c, PHI_OK, {0, 2, 3}, nullptr);
        c.bad(2, INF_E_CODE, 12345);                           // (what a decoder from a false start usually meets: no matter)
        chain_case("chain_false_start_in_error_dropped", c, PHI_OK, {0, 2, 3}, nullptr);
    }
    {
        ChainCase c({1, 1, 1, 1});
        for (int ch = 0; ch < 3; ch++) c.stop(ch, ch + 1);
        c.end(3);
        ChainCase first = c, middle = c, last = c;
        first.bad(0, INF_E_BLOCK, 8 * 99 + 7);
        chain_case("chain_error_at_first", first, PHI_ERR_INVALID, {0}, "gzip stream corrupt: invalid block header (near compressed byte 99)");
        middle.bad(2, INF_E_DIST, 8 * 70000);
        chain_case("chain_error_in_middle", middle, PHI_ERR_INVALID, {0, 1, 2}, "gzip stream corrupt: distance before the start of the member (near compressed byte 70000)");
        last.bad(3, INF_E_TRUNC, 8 * (((int64_t)1 << 33) + 5) + 1);
        chain_case("chain_error_at_last", last, PHI_ERR_INVALID, {0, 1, 2, 3}, "gzip stream corrupt: truncated stream (near compressed byte 8589934597)");
        ChainCase code = c, header = c, other = c;
        code.bad(1, INF_E_CODE, 80);
        chain_case("chain_error_code", code, PHI_ERR_INVALID, {0, 1}, "gzip stream corrupt: invalid Huffman code (near compressed byte 10)");
        header.bad(1, INF_E_HEADER, 80);
        chain_case("chain_error_header", header, PHI_ERR_INVALID, {0, 1}, "gzip stream corrupt: bad gzip member header (near compressed byte 10)");
        other.bad(1, -77, 80);
        chain_case("chain_error_unknown", other, PHI_ERR_INVALID, {0, 1}, "gzip stream corrupt: error (near compressed byte 10)");
    }
    {
        ChainCase base({1, 1, 0, 1});
        base.stop(0, 1); base.stop(1, 3); base.end(3);
        ChainCase self = base, back = base, beyond = base, far = base, negative = base, hole = base;
        self.stop(1, 1);
        chain_case("chain_malformed_stop_on_itself", self, PHI_ERR_DEVICE, {}, nullptr);
        back.stop(1, 0);
        chain_case("chain_malformed_stop_before_itself", back, PHI_ERR_DEVICE, {}, nullptr);
        beyond.stop(1, 4);
        chain_case("chain_malformed_stop_on_nch", beyond, PHI_ERR_DEVICE, {}, nullptr);
        far.stop(1, INT32_MAX);
        chain_case("chain_malformed_stop_far_beyond", far, PHI_ERR_DEVICE, {}, nullptr);
        negative.stop(1, INT32_MIN);
        chain_case("chain_malformed_stop_negative", negative, PHI_ERR_DEVICE, {}, nullptr);
        hole.stop(1, 2);
        chain_case("chain_malformed_stop_on_chunk_without_job", hole, PHI_ERR_DEVICE, {}, nullptr);
    }
    {
        Rng rng(1951);
        int differ = 0, errors = 0, dropped = 0;
        size_t longest = 0;
        for (int it = 0; it < 2000; it++) {
            const int nch = 1 + (int)rng.below(40);
            std::vector<int> has((size_t)nch);
            for (int i = 0; i < nch; i++) has[(size_t)i] = i == 0 || rng.below(3) != 0;
            ChainCase c(has);
            std::vector<int> later, truth;
            auto later_of = [&](int ch) { later.clear(); for (int i = ch + 1; i < nch; i++) if (has[(size_t)i]) later.push_back(i); };
            std::vector<char> on_chain((size_t)nch, 0);
            const bool with_error = rng.below(8) == 0;
            int want = 0;
            for (int ch = 0;;) {
                on_chain[(size_t)ch] = 1;
                truth.push_back(c.job_of[(size_t)ch]);
                later_of(ch);
                if (with_error && rng.below(4) == 0) { c.bad(ch, -1 - (int)rng.below(5), (int64_t)rng.below(1 << 20)); want = 1; break; }
                if (later.empty() || rng.below(6) == 0) { c.end(ch); break; }
                const int nx = later[(size_t)rng.below(std::min<uint64_t>(later.size(), 3))];
                c.stop(ch, nx);
                ch = nx;
            }
            for (int ch = 0; ch < nch; ch++) {
                if (!has[(size_t)ch] || on_chain[(size_t)ch]) continue;
                dropped++;
                later_of(ch);
                const uint64_t what = rng.below(3);
                if (what == 0 && !later.empty()) c.stop(ch, later[(size_t)rng.below(later.size())]);
                else if (what == 1) c.end(ch);
                else c.bad(ch, -1 - (int)rng.below(5), (int64_t)rng.below(1 << 20));
            }
            std::vector<int> chain, rchain;
            InfErr err;
            const int rc = inf_chain(c.job_of, c.res, chain, err);
            const int rr = ref::chain(c.job_of, c.res, rchain);
            if (rr != want || rc != (want ? PHI_ERR_INVALID : PHI_OK) || chain != truth || rchain != truth) differ++;
            errors += want;
            longest = std::max(longest, chain.size());
        }
        line("chain_random", differ == 0 && errors > 50 && dropped > 2000 && longest > 8,
             fmt("instances=2000 differ=%d with_error=%d dropped_jobs=%d longest=%zu", differ, errors, dropped, longest));
    }
}

// ------------------------------------------------------------------------------------------------ the second run

struct Run {            // nj jobs at chunks 0, 2, 4, ..., the chain, their results
    std::vector<InfJob> jobs;
    std::vector<InfResult> res;
    std::vector<int> chain;
    Run(int nj, const std::vector<int> &chain_, const std::vector<int64_t> &out_len, const std::vector<int> &ovf) : chain(chain_)
    {
        for (int k = 0; k < nj; k++) {
            jobs.push_back(InfJob{80 + 1000 * (int64_t)k, 500, SYM + 500 * k, 2 * k, 0});
            res.push_back(InfResult{out_len[(size_t)k], 0, 0, k + 1 < nj ? INF_STOP : INF_END, ovf[(size_t)k], 0});
        }
    }
};

bool again_agrees(Run &r, InfAgain &A, std::vector<InfJob> &j2, std::string &d)
{
    const std::vector<InfJob> before = r.jobs;
    inf_again_plan(r.chain, r.res, A);
    inf_again_jobs(A, r.res, SYM2, r.jobs, j2);
    bool ok = A.again.size() == A.off.size() && j2.size() == A.again.size();
    int64_t sum = 0;
    size_t q = 0;
    for (int k : r.chain) {
        if (!r.res[(size_t)k].ovf) continue;
        ok = ok && q < A.again.size() && A.again[q] == k && A.off[q] == sum;
        if (!ok) break;
        const InfJob &j = j2[q];
        ok = j.start == before[(size_t)k].start && j.chunk == before[(size_t)k].chunk && j.cap == r.res[(size_t)k].out_len + 1 && j.sym == SYM2 + sum && r.jobs[(size_t)k].sym == SYM2 + sum;
        d += fmt("%d@%lld ", k, (long long)sum);
        sum += r.res[(size_t)k].out_len + 1;
        q++;
    }
    ok = ok && q == A.again.size() && A.total == sum;
    for (size_t k = 0; k < before.size(); k++) {
        const bool moved = std::find(A.again.begin(), A.again.end(), (int)k) != A.again.end();
        ok = ok && r.jobs[k].start == before[k].start && r.jobs[k].cap == before[k].cap && r.jobs[k].chunk == before[k].chunk && (moved || r.jobs[k].sym == before[k].sym);
    }
    d += fmt("total=%lld", (long long)A.total);
    return ok;
}

void again_cases()
{
    InfAgain A;
    std::vector<InfJob> j2;
    {
        Run r(3, {0, 1, 2}, {100, 200, 300}, {0, 0, 0});
        std::string d;
        const bool ok = again_agrees(r, A, j2, d);
        line("again_none", ok && A.again.empty() && A.total == 0, d);
    }
    {
        Run r(3, {0, 1, 2}, {100, 700, 300}, {0, 1, 0});
        std::string d;
        const bool ok = again_agrees(r, A, j2, d);
        line("again_one", ok && A.again == std::vector<int>({1}) && A.total == 701, d);
    }
    {
        Run r(3, {0, 1, 2}, {600, 700, 0}, {1, 1, 1});
        std::string d;
        const bool ok = again_agrees(r, A, j2, d);
        line("again_all", ok && A.again == std::vector<int>({0, 1, 2}) && A.off == std::vector<int64_t>({0, 601, 1302}) && A.total == 1303, d);
    }
    {
        Run r(4, {0, 2, 3}, {600, 9000, 100, 800}, {1, 1, 0, 1});            // job 1 is no chain job
        std::string d;
        const bool ok = again_agrees(r, A, j2, d);
        line("again_dropped_job_ignored", ok && A.again == std::vector<int>({0, 3}) && A.total == 601 + 801 && r.jobs[1].sym == SYM + 500, d);
    }
    {
        Run r(5, {0, 1, 3, 4}, {((int64_t)1 << 32) + 5, 1, 77, ((int64_t)1 << 31), 9}, {1, 0, 1, 1, 1});
        std::string d;
        const bool ok = again_agrees(r, A, j2, d);
        line("again_offsets_and_total", ok && A.off == std::vector<int64_t>({0, ((int64_t)1 << 32) + 6, ((int64_t)1 << 32) + 6 + ((int64_t)1 << 31) + 1}) &&
                                            A.total == ((int64_t)1 << 32) + 6 + ((int64_t)1 << 31) + 1 + 10, d);
    }
    {
        Run r(4, {0, 2, 3}, {600, 9000, 100, 800}, {1, 1, 0, 1});
        r.res[0].status = INF_STOP; r.res[3].status = INF_END;
        std::string d;
        bool ok = again_agrees(r, A, j2, d);
        std::vector<InfResult> same = {r.res[0], r.res[3]};
        for (InfResult &x : same) { x.ovf = 0; x.end_bit += 1; x.end_chunk += 1; }     // (neither is compared)
        InfErr e0;
        ok = ok && inf_again_check(A, r.jobs, r.res, same, e0) == PHI_OK && e0.code == 0;
        line("again_second_run_agrees", ok, d);
        const char *names[3] = {"again_second_differs_in_length", "again_second_differs_in_status", "again_second_overflows_again"};
        for (int what = 0; what < 3; what++)
            for (int which = 0; which < 2; which++) {
                std::vector<InfResult> r2 = same;
                if (what == 0) r2[(size_t)which].out_len -= 1;
                if (what == 1) r2[(size_t)which].status = which ? INF_STOP : INF_END;
                if (what == 2) r2[(size_t)which].ovf = 1;
                InfErr err;
                const int rc = inf_again_check(A, r.jobs, r.res, r2, err);
                const std::string want = fmt("phi_inflate: decoder of chunk %d differs on its second run (internal error)", which ? 6 : 0);
                if (which == 0) { ok = rc == PHI_ERR_DEVICE && err.text == want; d = err.text; }
                else line(names[what], ok && rc == PHI_ERR_DEVICE && err.code == rc && err.text == want, d + " | " + err.text);
            }
    }
}

// ------------------------------------------------------------------------------------------------ pieces and members

struct LayoutOut { std::vector<InfPiece> pieces; std::vector<InfEnd> ends; int64_t total = -1; InfErr err; int rc = 0; };
// the header's layout of a run with these member records, against the restatement
bool layout_agrees(const Run &r, const std::vector<InfMember> &mem, LayoutOut &L, std::string &d)
{
    L = LayoutOut{};
    L.rc = inf_layout(r.chain, r.res, r.jobs, mem, L.pieces, L.ends, L.total, L.err);
    const ref::Layout R = ref::layout(r.chain, r.res, mem);
    if (!R.covered) {
        d += "refused";
        return L.rc == PHI_ERR_DEVICE && L.err.code == L.rc && !strcmp(L.err.text, "phi_inflate: member ends do not cover the output (internal error)");
    }
    bool ok = L.rc == PHI_OK && L.err.code == 0 && L.total == R.total && L.pieces.size() == r.chain.size() && L.ends.size() == R.ends.size();
    for (size_t i = 0; ok && i < L.pieces.size(); i++)
        ok = L.pieces[i].abs == R.abs[i] && L.pieces[i].len == R.len[i] && L.pieces[i].lo == R.lo[i] && L.pieces[i].sym == r.jobs[(size_t)r.chain[i]].sym;
    for (size_t i = 0; ok && i < L.ends.size(); i++)
        ok = L.ends[i].abs == R.ends[i].abs && L.ends[i].idx == R.ends[i].idx && L.ends[i].crc == R.ends[i].crc && L.ends[i].isize == R.ends[i].isize;
    d += "lo=";
    for (const InfPiece &p : L.pieces) d += fmt("%lld,", (long long)p.lo);
    d += " ends=";
    for (const InfEnd &e : L.ends) d += fmt("%lld#%d,", (long long)e.abs, e.idx);
    d += fmt(" total=%lld", (long long)L.total);
    return ok;
}

std::vector<int64_t> los(const LayoutOut &L)
{
    std::vector<int64_t> v;
    for (const InfPiece &p : L.pieces) v.push_back(p.lo);
    return v;
}
std::vector<int> end_order(const LayoutOut &L)
{
    std::vector<int> v;
    for (const InfEnd &e : L.ends) v.push_back(e.idx);
    return v;
}

void layout_cases()
{
    LayoutOut L;
    auto M = [](int job, int64_t pos, uint32_t id) { return InfMember{job, 0, pos, 0xC0000000u + id, 0x50000000u + id}; };
    {
        Run r(1, {0}, {100}, {0});
        std::string d;
        const bool ok = layout_agrees(r, {M(0, 100, 0)}, L, d);
        line("layout_one_member_one_piece", ok && L.total == 100 && los(L) == std::vector<int64_t>({0}) && L.ends.size() == 1 && L.ends[0].crc == 0xC0000000u && L.ends[0].isize == 0x50000000u, d);
    }
    {
        Run r(2, {0, 1}, {100, 100}, {0, 0});
        std::string d;
        const bool ok = layout_agrees(r, {M(0, 100, 0), M(1, 100, 1)}, L, d);
        line("layout_end_on_piece_boundary", ok && los(L) == std::vector<int64_t>({0, 100}) && L.total == 200, d);
    }
    {
        Run r(2, {0, 1}, {300, 50}, {0, 0});
        std::string d;
        const bool ok = layout_agrees(r, {M(0, 200, 0), M(1, 50, 1), M(0, 100, 2), M(0, 299, 3)}, L, d);
        line("layout_members_inside_one_piece", ok && los(L) == std::vector<int64_t>({0, 299}) && end_order(L) == std::vector<int>({2, 0, 3, 1}), d);
    }
    {
        Run r(3, {0, 1, 2}, {100, 100, 100}, {0, 0, 0});
        std::string d;
        const bool ok = layout_agrees(r, {M(2, 100, 0), M(0, 50, 1)}, L, d);
        line("layout_member_spans_three_pieces", ok && los(L) == std::vector<int64_t>({0, 50, 50}) && L.total == 300, d);
    }
    {
        Run r(2, {0, 1}, {100, 40}, {0, 0});
        std::string d;
        // the records come in any order: three at byte 100 (a member's end, then two empty members), by record index
        const bool ok = layout_agrees(r, {M(1, 40, 0), M(1, 0, 1), M(0, 100, 2), M(0, 60, 3), M(1, 0, 4)}, L, d);
        line("layout_empty_members_by_index", ok && end_order(L) == std::vector<int>({3, 1, 2, 4, 0}) && los(L) == std::vector<int64_t>({0, 100}), d);
    }
    {
        Run r(4, {0, 2, 3}, {100, 5000, 100, 100}, {0, 0, 0, 0});             // job 1 was dropped
        std::string d;
        const bool ok = layout_agrees(r, {M(1, 30, 0), M(3, 100, 1), M(1, 5000, 2), M(0, 70, 3)}, L, d);
        line("layout_dropped_jobs_records_ignored", ok && end_order(L) == std::vector<int>({3, 1}) && los(L) == std::vector<int64_t>({0, 70, 70}) && L.total == 300, d);
    }
    {
        Run r(2, {0, 1}, {100, 100}, {0, 0});
        std::string d;
        const bool ok = layout_agrees(r, {M(0, 100, 0), M(1, 99, 1)}, L, d);
        line("layout_last_end_short_refused", ok && L.rc == PHI_ERR_DEVICE, d);
    }
    {
        Run r(2, {0, 1}, {100, 100}, {0, 0});
        std::string d;
        const bool ok = layout_agrees(r, {M(0, 100, 0), M(1, 101, 1)}, L, d);
        line("layout_last_end_beyond_refused", ok && L.rc == PHI_ERR_DEVICE, d);
    }
    {
        Run r(3, {0, 2}, {100, 100, 100}, {0, 0, 0});
        std::string d, d2;
        bool ok = layout_agrees(r, {}, L, d) && L.rc == PHI_ERR_DEVICE;
        ok = ok && layout_agrees(r, {M(1, 100, 0)}, L, d2) && L.rc == PHI_ERR_DEVICE;      // (none of a chain job)
        line("layout_no_ends_refused", ok, d);
    }
    {
        Run r(2, {0, 1}, {100, 100}, {0, 0});
        bool ok = true;
        std::string d;
        for (int job : {-1, 2, INT32_MAX, INT32_MIN}) {
            InfErr err;
            std::vector<InfPiece> pieces;
            std::vector<InfEnd> ends;
            int64_t total;
            const int rc = inf_layout(r.chain, r.res, r.jobs, {M(0, 100, 0), M(job, 5, 1), M(1, 100, 2)}, pieces, ends, total, err);
            ok = ok && rc == PHI_ERR_DEVICE && strstr(err.text, "(internal error)");
            d += fmt("%d:%d ", job, rc);
        }
        line("layout_record_of_no_job_refused", ok, d);
    }
    {
        Rng rng(1952);
        int differ = 0, refused = 0, empties = 0, multi = 0;
        for (int it = 0; it < 2000; it++) {
            const int nj = 1 + (int)rng.below(10);
            std::vector<int> chain = {0};
            for (int k = 1; k < nj; k++) if (rng.below(3)) chain.push_back(k);
            std::vector<int64_t> len((size_t)nj);
            for (int64_t &l : len) l = rng.below(4) ? (int64_t)rng.below(500) : 0;
            Run r(nj, chain, len, std::vector<int>((size_t)nj, 0));
            std::vector<int64_t> abs;
            int64_t total = 0;
            for (int k : chain) { abs.push_back(total); total += len[(size_t)k]; }
            // member ends at rising positions (some twice: empty members), the last at the output's end; each recorded by a piece that holds it
            std::vector<InfMember> mem;
            const bool spoil = rng.below(10) == 0;
            int64_t at = 0;
            for (uint32_t id = 0;; id++) {
                if (rng.below(4)) at = std::min(total, at + 1 + (int64_t)rng.below(400)); else empties++;
                if (rng.below(5) == 0) at = total;
                std::vector<size_t> holds;
                for (size_t i = 0; i < chain.size(); i++) if (abs[i] <= at && at <= abs[i] + len[(size_t)chain[i]]) holds.push_back(i);
                const size_t i = holds[(size_t)rng.below(holds.size())];
                mem.push_back(M(chain[i], at - abs[i], id));
                if (at == total && rng.below(3)) break;
            }
            if (spoil) mem.pop_back();
            for (int k = 0; k < nj; k++)
                if (std::find(chain.begin(), chain.end(), k) == chain.end() && rng.below(2)) mem.push_back(M(k, (int64_t)rng.below(1000), 900 + (uint32_t)k));
            for (size_t i = mem.size(); i > 1; i--) std::swap(mem[i - 1], mem[(size_t)rng.below(i)]);
            std::string d;
            if (!layout_agrees(r, mem, L, d)) differ++;
            refused += L.rc != PHI_OK;
            multi += chain.size() > 2;
        }
        line("layout_random", differ == 0 && refused > 20 && refused < 1000 && empties > 500 && multi > 1000,
             fmt("layouts=2000 differ=%d refused=%d empty_members=%d three_pieces_or_more=%d", differ, refused, empties, multi));
    }
}

void slab_cases()
{
    const int64_t lens[] = {0, 1, INF_WIN, INF_WIN + 1, INF_WIN + 65536, INF_WIN + 65537, INF_WIN - 1, INF_WIN + 3 * 65536 + 17};
    std::vector<InfPiece> pieces;
    for (int64_t l : lens) pieces.push_back(InfPiece{0, l, 0, SYM});
    std::vector<InfSlab> slabs = {InfSlab{9, 9, 9, 9}};
    inf_slabs(pieces, slabs);
    bool ok = true;
    std::string d;
    size_t s = 0;
    for (size_t p = 0; p < pieces.size(); p++) {
        const int64_t body = lens[p] > 32768 ? lens[p] - 32768 : 0;
        int64_t at = 0;
        int count = 0;
        for (; s < slabs.size() && slabs[s].piece == (int32_t)p; s++, count++) {
            const int64_t n = slabs[s].k1 - slabs[s].k0;
            ok = ok && slabs[s].k0 == at && n >= 1 && n <= 65536 && (n == 65536 || slabs[s].k1 == body) && slabs[s].pad == 0;
            at = slabs[s].k1;
        }
        ok = ok && at == body;
        d += fmt("%lld:%d ", (long long)lens[p], count);
    }
    line("slabs_by_piece_length", ok && s == slabs.size(), d);
    inf_slabs({}, slabs);
    line("slabs_no_pieces", slabs.empty(), "0");
}

bool segments_tile(const std::vector<int64_t> &member_len, std::string &d)
{
    std::vector<InfEnd> ends;
    int64_t at = 0;
    for (size_t m = 0; m < member_len.size(); m++) { at += member_len[m]; ends.push_back(InfEnd{at, (int)m, 0, 0}); }
    std::vector<InfSeg> segs = {InfSeg{9, 9}};
    inf_segments(ends, segs);
    bool ok = true;
    size_t s = 0;
    int64_t start = 0;
    for (size_t m = 0; m < ends.size(); m++) {
        int64_t k = start;
        int count = 0;
        for (; s < segs.size() && segs[s].off < ends[m].abs; s++, count++) {
            ok = ok && segs[s].off == k && segs[s].len >= 1 && segs[s].len <= 4096 && (segs[s].len == 4096 || k + segs[s].len == ends[m].abs);
            k += segs[s].len;
        }
        ok = ok && k == ends[m].abs && count == (member_len[m] + 4095) / 4096;
        d += fmt("%lld:%d ", (long long)member_len[m], count);
        start = ends[m].abs;
    }
    return ok && s == segs.size();
}

void segment_cases()
{
    {
        std::string d;
        bool ok = true;
        for (int64_t l : {0, 1, 4095, 4096, 4097, 8192, 5 * 4096}) ok = segments_tile({l}, d) && ok;
        line("segments_by_member_length", ok, d);
    }
    {
        std::string d;
        std::vector<InfSeg> segs;
        inf_segments({InfEnd{4097, 0, 0, 0}, InfEnd{4097 + 5000, 1, 0, 0}}, segs);
        const bool exact = segs.size() == 4 && segs[0].off == 0 && segs[0].len == 4096 && segs[1].off == 4096 && segs[1].len == 1 && segs[2].off == 4097 &&
                           segs[2].len == 4096 && segs[3].off == 8193 && segs[3].len == 904;
        line("segments_two_members_back_to_back", segments_tile({4097, 5000}, d) && exact, d);
    }
    {
        std::string d;
        line("segments_empty_members_between", segments_tile({0, 4096, 0, 0, 1, 8192, 0}, d), d);
    }
}

// ------------------------------------------------------------------------------------------------ CRC32

// members of these lengths back to back, of random bytes: ends with true trailers, segments, the segments' registers
struct Members {
    std::vector<uint8_t> bytes;
    std::vector<InfEnd> ends;
    std::vector<InfSeg> segs;
    std::vector<uint32_t> crcs;
    Members(const std::vector<size_t> &lens, uint64_t seed)
    {
        Rng rng(seed);
        for (size_t m = 0; m < lens.size(); m++) {
            const size_t at = bytes.size();
            for (size_t i = 0; i < lens[m]; i++) bytes.push_back((uint8_t)rng.below(256));
            ends.push_back(InfEnd{(int64_t)bytes.size(), (int)m, ref::crc(bytes.data() + at, lens[m]), (uint32_t)lens[m]});
        }
        inf_segments(ends, segs);
        for (const InfSeg &s : segs) crcs.push_back(ref::raw(bytes.data() + s.off, (size_t)s.len));
    }
};

void member_check_cases()
{
    {
        Members M({0, 1, 5, 100, 4096, 5000, 0, 4095, 4097}, 11);
        InfErr err;
        const int rc = inf_member_check(M.ends, M.segs, M.crcs, err);
        line("mcheck_short_members", rc == PHI_OK && err.code == 0, fmt("members=%zu segments=%zu rc=%d", M.ends.size(), M.segs.size(), rc));
    }
    {
        Members M({3 * 4096 + 5}, 12);
        InfErr err;
        const int rc = inf_member_check(M.ends, M.segs, M.crcs, err);
        const uint32_t whole = ref::crc(M.bytes.data(), M.bytes.size());
        // the combined value itself, in the words of a refusal: the trailer off by one bit
        std::vector<InfEnd> off = M.ends;
        off[0].crc ^= 0x00010000u;
        InfErr e2;
        const int rc2 = inf_member_check(off, M.segs, M.crcs, e2);
        const std::string want = fmt("gzip stream corrupt: CRC32 mismatch in member 0 (%08x, trailer %08x)", whole, whole ^ 0x00010000u);
        line("mcheck_3x4096_plus_5", rc == PHI_OK && M.segs.size() == 4 && rc2 == PHI_ERR_INVALID && e2.text == want, fmt("segments=%zu crc=%08x", M.segs.size(), whole));
    }
    {
        Members M({100, 5000, 9000}, 13);
        std::vector<InfEnd> bad = M.ends;
        bad[1].crc += 1;
        InfErr err;
        const int rc = inf_member_check(bad, M.segs, M.crcs, err);
        const std::string want = fmt("gzip stream corrupt: CRC32 mismatch in member 1 (%08x, trailer %08x)", M.ends[1].crc, M.ends[1].crc + 1);
        line("mcheck_wrong_crc", rc == PHI_ERR_INVALID && err.code == rc && err.text == want, err.text);
        std::vector<uint32_t> crcs = M.crcs;
        crcs.back() ^= 0x80u;                                                     // a wrong byte in the output shows the same way
        InfErr e2;
        const int rc2 = inf_member_check(M.ends, M.segs, crcs, e2);
        line("mcheck_wrong_segment", rc2 == PHI_ERR_INVALID && strstr(e2.text, "CRC32 mismatch in member 2 (") != nullptr, e2.text);
    }
    {
        Members M({100, 5000, 9000}, 13);
        std::vector<InfEnd> bad = M.ends;
        bad[2].isize = 9001;
        InfErr err;
        const int rc = inf_member_check(bad, M.segs, M.crcs, err);
        line("mcheck_wrong_isize", rc == PHI_ERR_INVALID && err.code == rc && !strcmp(err.text, "gzip stream corrupt: ISIZE mismatch in member 2 (9000, trailer 9001)"), err.text);
    }
    {
        // 2^32 + 7 zero bytes: their segments' registers are all zero, so the member's CRC32 is the shift of the initial value alone
        const int64_t len = ((int64_t)1 << 32) + 7;
        uint32_t r = 0xffffffffu;
        r = dfl_crc_shift(r, 0x80000000u);
        r = dfl_crc_shift(r, 0x80000000u);
        r = ~ref::step_bits(r, 56);
        InfErr err, e2, e3;
        const int rc = inf_member_check({InfEnd{len, 0, r, 7}}, {}, {}, err);
        const int rc2 = inf_member_check({InfEnd{len, 0, r, 8}}, {}, {}, e2);
        const int rc3 = inf_member_check({InfEnd{len, 0, ~ref::step_bits(0xffffffffu, 56), 7}}, {}, {}, e3);       // the CRC32 of 7 zeros: a count cut to 32 bits
        line("mcheck_2pow32_plus_7_zeros", rc == PHI_OK && rc2 == PHI_ERR_INVALID && !strcmp(e2.text, "gzip stream corrupt: ISIZE mismatch in member 0 (7, trailer 8)") &&
                                               rc3 == PHI_ERR_INVALID && strstr(e3.text, "CRC32 mismatch"), fmt("crc=%08x isize=7", r));
    }
}

void crc_cases()
{
    {
        const uint64_t lens[] = {0, 1, 4096, 0xffffffffull, 0x100000000ull, (uint64_t)1 << 40, ((uint64_t)1 << 40) + 0x123456789ull};
        const uint32_t regs[] = {0xffffffffu, 0x80000000u, 1u, 0x12345678u, 0u};
        bool ok = true;
        std::string d;
        for (uint64_t n : lens) {
            for (uint32_t c : regs) {
                uint32_t want = c;
                for (uint64_t left = n; left;) {
                    const uint32_t piece = (uint32_t)std::min<uint64_t>(left, 0x80000000ull);
                    want = dfl_crc_shift(want, piece);
                    left -= piece;
                }
                ok = ok && inf_crc_shift(c, n) == want;
            }
            d += fmt("%llu:%08x ", (unsigned long long)n, inf_crc_shift(0xffffffffu, n));
        }
        ok = ok && inf_crc_shift(0x12345678u, 0) == 0x12345678u && inf_crc_shift(0x00000001u, 1) == ref::step_bits(1u, 8) && inf_crc_pow().pw[12] == dfl_crc_shift(0x80000000u, 4096);
        line("crc_shift_64", ok, d);
    }
    {
        Rng rng(14);
        int bad = 0;
        const size_t pairs[][2] = {{0, 0}, {1, 0}, {0, 1}, {3, 5}, {4096, 4096}, {10000, 1234}, {1, 70000}};
        for (auto &p : pairs) {
            std::vector<uint8_t> v(p[0] + p[1]);
            for (uint8_t &b : v) b = (uint8_t)rng.below(256);
            bad += inf_crc_combine(ref::crc(v.data(), p[0]), ref::crc(v.data() + p[0], p[1]), p[1]) != ref::crc(v.data(), v.size());
            bad += inf_crc_bitwise(0, v.data(), (int64_t)v.size()) != ref::crc(v.data(), v.size());
            bad += inf_crc_bitwise(inf_crc_bitwise(0, v.data(), (int64_t)p[0]), v.data() + p[0], (int64_t)p[1]) != ref::crc(v.data(), v.size());
        }
        for (uint32_t c = 0; c < 256; c++) bad += dfl_crc_byte(c) != ref::step_bits(c, 8);
        const uint8_t check[] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
        line("crc_combine_and_bitwise", bad == 0 && inf_crc_bitwise(0, check, 9) == 0xCBF43926u, fmt("differ=%d crc(123456789)=%08x", bad, inf_crc_bitwise(0, check, 9)));
    }
}

// ------------------------------------------------------------------------------------------------ gzip member header

std::vector<uint8_t> gz_header(int flags, const std::string &extra = "", const std::string &name = "", const std::string &comment = "", bool bad_hcrc = false)
{
    std::vector<uint8_t> h = {0x1f, 0x8b, 8, (uint8_t)flags, 0, 0, 0, 0, 0, 3};
    if (flags & 4) { h.push_back((uint8_t)(extra.size() & 255)); h.push_back((uint8_t)(extra.size() >> 8)); h.insert(h.end(), extra.begin(), extra.end()); }
    if (flags & 8) { h.insert(h.end(), name.begin(), name.end()); h.push_back(0); }
    if (flags & 16) { h.insert(h.end(), comment.begin(), comment.end()); h.push_back(0); }
    if (flags & 2) {
        const uint32_t c = ref::crc(h.data(), h.size()) ^ (bad_hcrc ? 1u : 0u);
        h.push_back((uint8_t)(c & 255)); h.push_back((uint8_t)((c >> 8) & 255));
    }
    return h;
}
// the parser over an allocation of exactly these bytes: a read one past the end is the sanitizer's
int64_t parse_exact(const std::vector<uint8_t> &v, int64_t p)
{
    std::unique_ptr<uint8_t[]> b(new uint8_t[v.size()]);
    if (!v.empty()) memcpy(b.get(), v.data(), v.size());
    return inf_gz_header(b.get(), (int64_t)v.size(), p);
}

void header_cases()
{
    struct Case { const char *name; int flags; std::string extra, name_, comment; };
    const Case good[] = {{"gzhdr_plain", 0, "", "", ""}, {"gzhdr_fname", 8, "", "reads.fq", ""}, {"gzhdr_fextra", 4, std::string("BC\x02\x00\x10\x00", 6), "", ""},
                         {"gzhdr_fcomment", 16, "", "", "hi"}, {"gzhdr_fhcrc", 2, "", "", ""}, {"gzhdr_every_field", 2 | 4 | 8 | 16, std::string(700, '\x01'), "a", "b"}};
    for (const Case &c : good) {
        const std::vector<uint8_t> h = gz_header(c.flags, c.extra, c.name_, c.comment);
        std::vector<uint8_t> data = {'p', 'a', 'd'};
        data.insert(data.end(), h.begin(), h.end());
        const int64_t bare = parse_exact(data, 3);                                 // nothing behind the header
        data.push_back(3); data.push_back(0);
        const int64_t got = parse_exact(data, 3);
        // cut anywhere, it is truncated; (a cut inside the magic is too: fewer than ten bytes)
        int not_truncated = 0;
        for (size_t cut = 0; cut < h.size(); cut++) not_truncated += parse_exact(std::vector<uint8_t>(h.begin(), h.begin() + (long)cut), 0) != -2;
        line(c.name, got == 3 + (int64_t)h.size() && bare == got && not_truncated == 0, fmt("header=%zu data_at=%lld cuts_not_truncated=%d", h.size(), (long long)got, not_truncated));
    }
    auto bad = [&](const char *name, const std::vector<uint8_t> &v, int64_t want) {
        const int64_t got = parse_exact(v, 0);
        line(name, got == want, fmt("%lld", (long long)got));
    };
    std::vector<uint8_t> h = gz_header(0);
    h[2] = 7;
    bad("gzhdr_bad_method", h, -1);
    h = gz_header(0);
    h[1] = 0x8c;
    bad("gzhdr_bad_magic", h, -1);
    h = gz_header(8, "", "x");
    h.pop_back();
    bad("gzhdr_fname_unterminated", h, -2);
    h = gz_header(4, "abcdef");
    h.resize(h.size() - 2);
    bad("gzhdr_fextra_cut", h, -2);
    bad("gzhdr_bad_fhcrc", gz_header(2, "", "", "", true), -1);
    h = gz_header(0);
    h[3] = 0x20;
    bad("gzhdr_reserved_flag", h, -1);
    bad("gzhdr_two_bytes", {0x1f, 0x8b}, -2);
    bad("gzhdr_no_bytes", {}, -2);
    h = gz_header(4, std::string(65535, 'e'));
    bad("gzhdr_fextra_65535", h, (int64_t)h.size());
    h = gz_header(2 | 8, "", "name");
    h[11] ^= 0x20;                                                                  // a byte under the header's CRC
    bad("gzhdr_fhcrc_covers_the_name", h, -1);
}

}  // namespace

int main()
{
    chunk_cases();
    capacity_cases();
    job_cases();
    chain_cases();
    again_cases();
    layout_cases();
    slab_cases();
    segment_cases();
    member_check_cases();
    crc_cases();
    header_cases();
    printf("cases_failed %d\n", n_failed);
    return n_failed ? 1 : 0;
}
