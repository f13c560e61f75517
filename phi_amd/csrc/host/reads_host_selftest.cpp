// reads_host_selftest.cpp -- stand-alone check of ../reads_host.h (the rules of the read path that need no GPU) on the CPU: no
// GPU, no ROCm.  Built plain, with AddressSanitizer + UndefinedBehaviorSanitizer and with ThreadSanitizer by the Makefile's
// reads_host_sanitize; tests/test_cpu_reads_host.py runs the three and compares their output.
//
// Every case runs at PHI_HOST_THREADS=1 and =8 and must give the same line both times.  The header's results are compared
// with restatements below (namespace ref) that are serial, written from the rules' sentences and share no code with it:
//   * log plan: a chunk takes 8 << shift bytes of the log and 2 of the counts.  The batch starts behind the chunks logged so
//     far, less the last batch's on a replay.  When log and counts hold it, nothing happens.  Else, a log that holds chunks
//     and would pass the budget is flushed and the batch starts at chunk 0; and if log or counts still do not hold the batch,
//     the log becomes max(bytes needed, min(twice its size, budget)), the counts 2 bytes per chunk of that log + 64, and the
//     chunks in front of the batch are kept.  In 128-bit arithmetic, so that a wrap of the header's size_t would show;
//   * overflow list: a batch adds n_bases * min(1, 3 / (w + 1)) + 16 to the bound (w <= 2: n_bases + 16 exactly; beyond, the
//     exact quotient 3 n / (w + 1) rounded down, give or take the one unit a double may be off by); a bound above the
//     capacity makes it max(bound, 2 cap, 65536); a replay keeps min(wanted, cap) entries and grows to max(4 cap, 2 wanted);
//   * set: the smallest power of two that is >= 65536 and >= twice the keys; another generation's set is reused in [need, 4 need];
//   * offsets: a serial scan with a branch per read;
//   * fixed point: floor(2^32 / length); floor(2^32 n_reads / n_bases) give or take one, 2^31 from one read per two bases up;
//   * pool: a scan that keeps the smallest capacity in [want, want + want / 8];
//   * text: chunk = the request within [64, 2^28]; carry = PHI_TEXT_CARRY (at least 64) rounded down to 16, or max(chunk / 2,
//     2^24); lines = (carry + chunk) / 16 + 1024; the host carry after a piece = the last `tail` bytes of carry || piece.
// One line per case on stdout: name, ok or FAILED, and what was found.  Exit status 0 = every case agreed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <functional>
#include <string>
#include <vector>
#include "../reads_host.h"

namespace {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    uint64_t below(uint64_t n) { return next() % n; }
};

struct Hash {
    uint64_t h = 0xCBF29CE484222325ull;
    void add(uint64_t v) { for (int i = 0; i < 8; i++) { h ^= (v >> (8 * i)) & 0xFF; h *= 0x100000001B3ull; } }
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

namespace ref {
typedef unsigned __int128 u128;

struct LogPlan { int64_t base; bool flush; u128 log_bytes, cnt_bytes, keep_log, keep_cnt; };
LogPlan log_plan(int64_t in_log, int64_t last, bool replay, int64_t batch, int shift, u128 log_cap, u128 cnt_cap, u128 budget)
{
    LogPlan P{};
    P.base = in_log;
    if (replay) P.base -= last;
    const u128 per_chunk = (u128)8 << shift;
    u128 front = (u128)P.base;
    bool holds = (front + (u128)batch) * per_chunk <= log_cap && (front + (u128)batch) * 2 <= cnt_cap;
    if (holds) return P;
    if (front != 0 && (front + (u128)batch) * per_chunk > budget) {
        P.flush = true;
        front = 0;
        holds = (u128)batch * per_chunk <= log_cap && (u128)batch * 2 <= cnt_cap;
        if (holds) return P;
    }
    const u128 needed = (front + (u128)batch) * per_chunk;
    u128 grown = 2 * log_cap;
    if (grown > budget) grown = budget;
    P.log_bytes = needed > grown ? needed : grown;
    P.cnt_bytes = P.log_bytes / per_chunk * 2 + 64;
    P.keep_log = front * per_chunk;
    P.keep_cnt = front * 2;
    return P;
}

int64_t first_bad(const std::vector<int64_t> &off, bool one_length, int64_t len)
{
    for (size_t r = 0; r + 1 < off.size(); r++) {
        if (one_length) { if (off[r + 1] - off[r] != len) return (int64_t)r; }
        else if (off[r + 1] < off[r]) return (int64_t)r;
    }
    return -1;
}

int best_fit(const std::vector<size_t> &cap, size_t want)
{
    int at = -1;
    for (size_t i = 0; i < cap.size(); i++) {
        if (cap[i] < want || cap[i] > want + want / 8) continue;
        if (at < 0 || cap[i] < cap[(size_t)at]) at = (int)i;
    }
    return at;
}
}  // namespace ref

bool same_plan(const PhiLogPlan &P, const ref::LogPlan &R)
{
    return P.base == R.base && P.flush_first == R.flush && (ref::u128)P.log_bytes == R.log_bytes && (ref::u128)P.cnt_bytes == R.cnt_bytes &&
           (ref::u128)P.keep_log == R.keep_log && (ref::u128)P.keep_cnt == R.keep_cnt;
}
bool same_plan(const PhiLogPlan &A, const PhiLogPlan &B)
{
    return A.base == B.base && A.flush_first == B.flush_first && A.log_bytes == B.log_bytes && A.cnt_bytes == B.cnt_bytes && A.keep_log == B.keep_log &&
           A.keep_cnt == B.keep_cnt;
}
std::string plan_text(const PhiLogPlan &P)
{
    return fmt("base=%lld flush=%d log=%zu cnt=%zu keep=%zu,%zu", (long long)P.base, (int)P.flush_first, P.log_bytes, P.cnt_bytes, P.keep_log, P.keep_cnt);
}
// one state of the log against the restatement
bool log_case(std::string &d, int64_t in_log, int64_t last, bool replay, int64_t batch, int shift, size_t log_cap, size_t cnt_cap, size_t budget)
{
    const PhiLogPlan P = phi_log_plan(in_log, last, replay, batch, shift, log_cap, cnt_cap, budget);
    d = plan_text(P);
    return same_plan(P, ref::log_plan(in_log, last, replay, batch, shift, log_cap, cnt_cap, budget));
}

void log_cases()
{
    const size_t GB = (size_t)1 << 30;
    // shift 6: 512 bytes of log per chunk
    run_case("log_empty", [&](std::string &d) {
        const bool ok = log_case(d, 0, 0, false, 10, 6, 0, 0, GB);
        const PhiLogPlan P = phi_log_plan(0, 0, false, 10, 6, 0, 0, GB);
        return ok && !P.flush_first && P.log_bytes == 5120 && P.cnt_bytes == 84 && P.keep_log == 0 && P.keep_cnt == 0 && P.base == 0;
    });
    run_case("log_fits_exactly", [&](std::string &d) {
        const bool ok = log_case(d, 30, 0, false, 10, 6, 40 * 512, 40 * 2, GB);
        const PhiLogPlan P = phi_log_plan(30, 0, false, 10, 6, 40 * 512, 40 * 2, GB);
        return ok && !P.flush_first && P.log_bytes == 0 && P.cnt_bytes == 0 && P.base == 30;
    });
    run_case("log_one_entry_over", [&](std::string &d) {
        const bool ok = log_case(d, 30, 0, false, 10, 6, 40 * 512 - 8, 1 << 20, GB);
        const PhiLogPlan P = phi_log_plan(30, 0, false, 10, 6, 40 * 512 - 8, 1 << 20, GB);
        return ok && !P.flush_first && P.log_bytes == 2 * (40 * 512 - 8) && P.keep_log == 30 * 512 && P.keep_cnt == 60;
    });
    run_case("log_counts_are_the_limit", [&](std::string &d) {
        const bool ok = log_case(d, 30, 0, false, 10, 6, 1 << 20, 40 * 2 - 1, GB);
        const PhiLogPlan P = phi_log_plan(30, 0, false, 10, 6, 1 << 20, 40 * 2 - 1, GB);
        return ok && !P.flush_first && P.log_bytes == 2 << 20 && P.cnt_bytes == (2 << 20) / 512 * 2 + 64 && P.keep_cnt == 60;
    });
    run_case("log_over_budget_nothing_logged", [&](std::string &d) {
        const bool ok = log_case(d, 0, 0, false, 100, 6, 4096, 4096, 4096);
        const PhiLogPlan P = phi_log_plan(0, 0, false, 100, 6, 4096, 4096, 4096);
        return ok && !P.flush_first && P.log_bytes == 100 * 512 && P.keep_log == 0;
    });
    run_case("log_over_budget_flushes_first", [&](std::string &d) {
        const bool ok = log_case(d, 7, 0, false, 100, 6, 4096, 4096, 4096);
        const PhiLogPlan P = phi_log_plan(7, 0, false, 100, 6, 4096, 4096, 4096);
        return ok && P.flush_first && P.base == 7 && P.log_bytes == 100 * 512 && P.keep_log == 0 && P.keep_cnt == 0;
    });
    run_case("log_flushed_batch_fits_what_is_there", [&](std::string &d) {
        const bool ok = log_case(d, 7, 0, false, 4, 6, 4096, 4096, 4096);
        const PhiLogPlan P = phi_log_plan(7, 0, false, 4, 6, 4096, 4096, 4096);
        return ok && P.flush_first && P.log_bytes == 0 && P.cnt_bytes == 0;
    });
    run_case("log_doubling_capped_by_budget", [&](std::string &d) {
        const bool ok = log_case(d, 100, 0, false, 10, 6, 100 * 512, 1 << 20, 150 * 512);
        const PhiLogPlan P = phi_log_plan(100, 0, false, 10, 6, 100 * 512, 1 << 20, 150 * 512);
        return ok && !P.flush_first && P.log_bytes == 150 * 512 && P.keep_log == 100 * 512;
    });
    run_case("log_replay_same_plan", [&](std::string &d) {
        // the first pass from 30 chunks, then its replay from the state that pass left (40 chunks, 10 of them the last batch's)
        bool ok = true;
        for (int grown = 0; grown < 2; grown++) {
            const size_t log_cap = 35 * 512, cnt_cap = 70;
            const PhiLogPlan first = phi_log_plan(30, 99, false, 10, 6, log_cap, cnt_cap, GB);
            const size_t lc = grown ? first.log_bytes : log_cap, cc = grown ? first.cnt_bytes : cnt_cap;
            const PhiLogPlan again = phi_log_plan(40, 10, true, 10, 6, lc, cc, GB);
            std::string dd;
            ok = ok && log_case(dd, 40, 10, true, 10, 6, lc, cc, GB);
            if (grown) ok = ok && again.base == first.base && !again.flush_first && again.log_bytes == 0 && again.cnt_bytes == 0;
            else ok = ok && same_plan(first, again);
            d += (grown ? " | grown: " : "as it was: ") + plan_text(again);
        }
        return ok;
    });
    run_case("log_2pow40_bases", [&](std::string &d) {
        // 2^40 bases in chunks of 512 windows: 2^31 chunks, at 4096 bytes each (shift 9), behind 2^31 chunks logged before
        const int64_t n = (int64_t)1 << 31;
        bool ok = log_case(d, 0, 0, false, n, 9, 0, 0, GB);
        std::string d2;
        ok = ok && log_case(d2, n, 0, false, n, 9, (size_t)n * 4096, (size_t)n * 2 + 64, ~(size_t)0 >> 1);
        const PhiLogPlan P = phi_log_plan(n, 0, false, n, 9, (size_t)n * 4096, (size_t)n * 2 + 64, ~(size_t)0 >> 1);
        d += " | " + d2;
        return ok && P.log_bytes == (size_t)1 << 44 && P.keep_log == (size_t)1 << 43 && P.keep_cnt == (size_t)1 << 32;
    });
    run_case("log_random", [&](std::string &d) {
        Rng rng(20240607);
        Hash H;
        int bad = 0, flushes = 0, grows = 0;
        for (int i = 0; i < 2000; i++) {
            const int shift = (int)rng.below(10);
            const size_t ent = (size_t)8 << shift;
            const int64_t batch = 1 + (int64_t)rng.below(5000), last = 1 + (int64_t)rng.below(5000);
            const bool replay = rng.below(4) == 0;
            const int64_t in_log = (replay ? last : 0) + (rng.below(3) ? (int64_t)rng.below(20000) : 0);
            const size_t budget = rng.below(3) ? (size_t)1 << 30 : 1 + (size_t)rng.below(40000) * ent;
            // capacities around what the batch needs: short of it, exactly it, beyond it
            const size_t front = (size_t)(in_log - (replay ? last : 0)) + (size_t)batch;
            const size_t log_cap = rng.below(5) == 0 ? 0 : front * ent - ent + (size_t)rng.below(3 * ent);
            const size_t cnt_cap = rng.below(5) == 0 ? 0 : front * 2 - 2 + (size_t)rng.below(200);
            const PhiLogPlan P = phi_log_plan(in_log, last, replay, batch, shift, log_cap, cnt_cap, budget);
            if (!same_plan(P, ref::log_plan(in_log, last, replay, batch, shift, log_cap, cnt_cap, budget))) bad++;
            flushes += P.flush_first; grows += P.log_bytes != 0;
            H.add((uint64_t)P.base); H.add(P.flush_first); H.add(P.log_bytes); H.add(P.cnt_bytes); H.add(P.keep_log); H.add(P.keep_cnt);
        }
        d = fmt("states=2000 differ=%d flushed=%d grown=%d hash=%016llx", bad, flushes, grows, (unsigned long long)H.h);
        return bad == 0 && flushes > 20 && grows > 200;
    });
}

void overflow_cases()
{
    run_case("ov_bound_by_w", [&](std::string &d) {
        bool ok = true;
        const int ws[] = {1, 2, 3, 25, 255};
        const int64_t ns[] = {0, 1, 150, 5200000, 26000, ((int64_t)1 << 40) + 12345};
        for (int w : ws)
            for (int64_t n : ns) {
                const int64_t got = phi_ov_batch_bound(n, w);
                if (w <= 2) ok = ok && got == n + 16;
                else {
                    const int64_t exact = (int64_t)((ref::u128)3 * (ref::u128)n / (ref::u128)(w + 1)) + 16;
                    ok = ok && got >= exact - 1 && got <= exact + 1;
                }
                if (n == 5200000) d += fmt("w=%d:%lld ", w, (long long)got);
            }
        return ok;
    });
    run_case("ov_capacity_around_the_bound", [&](std::string &d) {
        const int64_t cap = 100000;
        const int64_t below = phi_ov_capacity(cap - 1, cap), equal = phi_ov_capacity(cap, cap), above = phi_ov_capacity(cap + 1, cap);
        const int64_t far = phi_ov_capacity(3 * cap + 7, cap);
        d = fmt("below=%lld equal=%lld above=%lld far=%lld", (long long)below, (long long)equal, (long long)above, (long long)far);
        return below == cap && equal == cap && above == 2 * cap && far == 3 * cap + 7;
    });
    run_case("ov_capacity_floor", [&](std::string &d) {
        const int64_t first = phi_ov_capacity(17, 0), small = phi_ov_capacity(1001, 1000);
        d = fmt("first=%lld small=%lld", (long long)first, (long long)small);
        return first == 65536 && small == 65536;
    });
    run_case("ov_replay_one_over", [&](std::string &d) {
        const PhiOvReplay R = phi_ov_replay(50 + 1, 50);
        d = fmt("valid=%llu cap=%lld", R.valid, (long long)R.cap);
        return R.valid == 50 && R.cap == 200;
    });
    run_case("ov_replay_ten_times", [&](std::string &d) {
        const PhiOvReplay R = phi_ov_replay(10 * 50, 50);
        const PhiOvReplay U = phi_ov_replay(20, 50);           // (not full after all: everything wanted is valid)
        d = fmt("valid=%llu cap=%lld under: valid=%llu cap=%lld", R.valid, (long long)R.cap, U.valid, (long long)U.cap);
        return R.valid == 50 && R.cap == 1000 && U.valid == 20 && U.cap == 200;
    });
}

void set_cases()
{
    run_case("set_capacity", [&](std::string &d) {
        bool ok = true;
        const uint64_t keys[] = {0, 32768, 32769, 65536, 65537, 1000000, (uint64_t)1 << 33};
        for (uint64_t n : keys) {
            uint64_t want = 65536;
            while (want < 2 * n) want *= 2;
            const uint64_t got = phi_set_capacity(n / 3, n - n / 3);
            ok = ok && got == want && (got & (got - 1)) == 0 && 2 * n <= got;
            d += fmt("%llu:%llu ", (unsigned long long)n, (unsigned long long)got);
        }
        return ok && phi_set_capacity(0, 0) == 65536 && phi_set_capacity(32768, 0) == 65536 && phi_set_capacity(0, 32769) == 131072;
    });
    run_case("set_reuse", [&](std::string &d) {
        const uint64_t need = 131072;
        const bool exact = phi_set_reusable(need, need), four = phi_set_reusable(4 * need, need), over = phi_set_reusable(4 * need + 1, need),
                   half = phi_set_reusable(need / 2, need), none = phi_set_reusable(0, need);
        d = fmt("need=%d four=%d four_and_one=%d half=%d none=%d", (int)exact, (int)four, (int)over, (int)half, (int)none);
        return exact && four && !over && !half && !none;
    });
}

void offset_cases()
{
    const int64_t M = (int64_t)1 << 20;
    const int64_t sizes[] = {1, M - 1, M, M + 1, 2 * M + 5};
    run_case("offsets_monotone_sizes", [&](std::string &d) {
        bool ok = true;
        for (int64_t n : sizes) {
            std::vector<int64_t> off((size_t)n + 1);
            for (int64_t r = 0; r <= n; r++) off[(size_t)r] = r * 3 / 2;       // (lengths 1 and 2)
            ok = ok && phi_offsets_first_bad(off.data(), n, false, 0) == -1 && ref::first_bad(off, false, 0) == -1;
            d += fmt("%lld ", (long long)n);
        }
        return ok;
    });
    run_case("offsets_one_bad_read", [&](std::string &d) {
        bool ok = true;
        for (int64_t n : sizes) {
            // the offender at the first read, at the last, and on either side of every seam between two pieces of 2^20
            std::vector<int64_t> at = {0, n - 1};
            for (int64_t s = M; s < n; s += M) { at.push_back(s - 1); at.push_back(s); }
            for (int64_t r : at) {
                if (r < 0 || r >= n) continue;
                for (int one = 0; one < 2; one++) {
                    std::vector<int64_t> off((size_t)n + 1);
                    for (int64_t i = 0; i <= n; i++) off[(size_t)i] = i * 40;
                    if (one) { for (int64_t i = r + 1; i <= n; i++) off[(size_t)i] += 1; }   // read r is 41 long
                    else off[(size_t)r + 1] = off[(size_t)r] - 1;                            // read r is -1 long
                    const int64_t got = phi_offsets_first_bad(off.data(), n, one != 0, 40);
                    ok = ok && got == r && ref::first_bad(off, one != 0, 40) == r;
                }
                d += fmt("%lld@%lld ", (long long)n, (long long)r);
            }
        }
        return ok;
    });
    run_case("offsets_first_of_several", [&](std::string &d) {
        Rng rng(77);
        bool ok = true;
        Hash H;
        for (int t = 0; t < 6; t++) {
            const int64_t n = t < 3 ? 5000 : 3 * M + 11;
            std::vector<int64_t> off((size_t)n + 1);
            for (int64_t i = 0; i <= n; i++) off[(size_t)i] = i * 100;
            for (int j = 0; j < 3; j++) { const int64_t r = 1 + (int64_t)rng.below((uint64_t)n - 1); off[(size_t)r] -= 150; }
            const int64_t a = phi_offsets_first_bad(off.data(), n, false, 0), b = phi_offsets_first_bad(off.data(), n, true, 100);
            ok = ok && a == ref::first_bad(off, false, 0) && b == ref::first_bad(off, true, 100) && a >= 0 && b >= 0 && b <= a;
            H.add((uint64_t)a); H.add((uint64_t)b);
        }
        d = fmt("hash=%016llx", (unsigned long long)H.h);
        return ok;
    });
    run_case("offsets_empty_reads", [&](std::string &d) {
        std::vector<int64_t> off(1000, 0), mixed = {0, 0, 40, 40, 40, 90};
        const int64_t a = phi_offsets_first_bad(off.data(), 999, false, 0), b = phi_offsets_first_bad(mixed.data(), 5, false, 0);
        const bool one = phi_reads_one_length(off.data(), 999);
        d = fmt("all_empty=%lld mixed=%lld one_length=%d", (long long)a, (long long)b, (int)one);
        return a == -1 && b == -1 && !one;
    });
    run_case("one_length_31_and_32", [&](std::string &d) {
        bool ok = true;
        for (int64_t len : {31, 32, 33, 150}) {
            for (int64_t n : {(int64_t)1, (int64_t)7, M + 3}) {
                std::vector<int64_t> off((size_t)n + 1);
                for (int64_t i = 0; i <= n; i++) off[(size_t)i] = i * len;
                ok = ok && phi_reads_one_length(off.data(), n) == (len >= 32);
                if (n > 1 && len >= 32) { off[(size_t)n / 2] += 1; ok = ok && !phi_reads_one_length(off.data(), n); }   // two reads differ, the sum does not
            }
            d += fmt("%lld:%d ", (long long)len, (int)(len >= 32));
        }
        return ok;
    });
    run_case("one_length_product_agrees_reads_do_not", [&](std::string &d) {
        const std::vector<int64_t> off = {0, 32, 50, 96};          // 32 * 3 = 96, lengths 32, 18, 46
        const bool one = phi_reads_one_length(off.data(), 3);
        const int64_t r = phi_offsets_first_bad(off.data(), 3, true, 32);
        // a first length whose product with the read count does not fit 64 bits is no one length either
        const std::vector<int64_t> huge = {0, (int64_t)1 << 62, (int64_t)1 << 62, (int64_t)1 << 62, (int64_t)1 << 62, (int64_t)1 << 62};
        const bool one_huge = phi_reads_one_length(huge.data(), 5);
        d = fmt("one_length=%d first_other=%lld huge=%d", (int)one, (long long)r, (int)one_huge);
        return !one && r == 1 && !one_huge;
    });
    run_case("device_one_length", [&](std::string &d) {
        bool ok = true;
        const int64_t lens[] = {1, 31, 32, 150, 0x7FFFFFFF, (int64_t)0x7FFFFFFF + 1};
        for (int64_t len : lens) {
            const int64_t n = len > 1000 ? 3 : 1000;
            const PhiOneLength L = phi_device_one_length(n, n * len);
            const bool make = len < 32 || len > 2147483647ll;
            ok = ok && L.make_offsets == make && L.step == len && L.uniform_len == (make ? 0 : len);
            d += fmt("%lld:%s ", (long long)len, L.make_offsets ? "offsets" : "computed");
        }
        return ok;
    });
}

void fixed_point_cases()
{
    run_case("q32_inverse_length", [&](std::string &d) {
        bool ok = phi_inv_len_q32(0) == 0;
        const int64_t lens[] = {32, 150, 0x7FFFFFFF};
        for (int64_t len : lens) {
            const uint32_t got = phi_inv_len_q32(len);
            const ref::u128 want = ((ref::u128)1 << 32) / (ref::u128)len;
            ok = ok && (ref::u128)got == want;
            d += fmt("%lld:%u ", (long long)len, got);
        }
        return ok && phi_inv_len_q32(32) == 134217728u && phi_inv_len_q32(150) == 28633115u && phi_inv_len_q32(0x7FFFFFFF) == 2u;
    });
    run_case("q32_reads_per_base", [&](std::string &d) {
        bool ok = true;
        const int64_t pairs[][2] = {{1, 150}, {34666, 5199900}, {1, 32}, {1, 3}, {1, 2}, {1, 1}, {5, 3}, {1, (int64_t)1 << 40}, {(int64_t)1 << 33, (int64_t)1 << 40}};
        for (auto &p : pairs) {
            const uint32_t got = phi_reads_per_base_q32(p[0], p[1]);
            const ref::u128 exact = ((ref::u128)p[0] << 32) / (ref::u128)p[1];
            if (2 * p[0] >= p[1]) ok = ok && got == 0x80000000u;                      // the clamp
            else ok = ok && (ref::u128)got + 1 >= exact && (ref::u128)got <= exact + 1;
            d += fmt("%lld/%lld:%u ", (long long)p[0], (long long)p[1], got);
        }
        return ok;
    });
}

void pool_cases()
{
    const size_t want = (size_t)64 << 20, slack = want / 8;
    auto one = [&](const char *name, std::vector<size_t> caps, int expect) {
        run_case(name, [&](std::string &d) {
            const int got = phi_pool_best_fit(caps.data(), (int)caps.size(), want);
            d = fmt("index=%d", got);
            return got == expect && got == ref::best_fit(caps, want);
        });
    };
    one("pool_exact_fit", {want / 2, want, 3 * want}, 1);
    one("pool_upper_end_taken", {want + slack}, 0);
    one("pool_one_beyond_not_taken", {want + slack + 1, want - 1}, -1);
    one("pool_smaller_of_two", {want + slack, want + 4096, 2 * want, want + 8192}, 1);
    one("pool_none", {}, -1);
    run_case("pool_random", [&](std::string &d) {
        Rng rng(5);
        int bad = 0, hits = 0;
        for (int i = 0; i < 2000; i++) {
            const size_t w = 256 + (size_t)rng.below(1 << 20);
            std::vector<size_t> caps(rng.below(12));
            for (size_t &c : caps) c = w - 64 + (size_t)rng.below(w / 4 + 128);
            const int got = phi_pool_best_fit(caps.data(), (int)caps.size(), w);
            bad += got != ref::best_fit(caps, w); hits += got >= 0;
        }
        d = fmt("differ=%d taken=%d", bad, hits);
        return bad == 0 && hits > 200;
    });
}

void text_cases()
{
    run_case("text_sizes_carry_from_env", [&](std::string &d) {
        const PhiTextSizes a = phi_text_sizes(1 << 20, "64"), b = phi_text_sizes(1 << 20, "70"), c = phi_text_sizes(1 << 20, "5"), e = phi_text_sizes(1 << 20, "4096");
        d = fmt("64:%u 70:%u 5:%u 4096:%u lines=%u", a.carry, b.carry, c.carry, e.carry, b.line_cap);
        return a.carry == 64 && b.carry == 64 && c.carry == 64 && e.carry == 4096 && a.chunk == 1u << 20 && b.line_cap == (64 + (1u << 20)) / 16 + 1024;
    });
    run_case("text_sizes_default_carry", [&](std::string &d) {
        bool ok = true;
        const int64_t asks[] = {1, 64, (int64_t)1 << 24, (int64_t)1 << 26, (int64_t)1 << 28, ((int64_t)1 << 28) + 1, (int64_t)1 << 40};
        for (int64_t ask : asks) {
            const PhiTextSizes z = phi_text_sizes(ask, nullptr);
            const uint64_t chunk = ask < 64 ? 64 : ask > ((int64_t)1 << 28) ? (uint64_t)1 << 28 : (uint64_t)ask;
            const uint64_t carry = chunk / 2 > ((uint64_t)1 << 24) ? chunk / 2 : (uint64_t)1 << 24;
            ok = ok && z.chunk == chunk && z.carry == carry && z.line_cap == (carry + chunk) / 16 + 1024 && z.carry % 16 == 0;
            d += fmt("%lld:%u,%u,%u ", (long long)ask, z.chunk, z.carry, z.line_cap);
        }
        return ok;
    });
    run_case("text_carry_update", [&](std::string &d) {
        Rng rng(31);
        bool ok = true;
        const uint32_t carry_len = 37, m = 20;
        const uint32_t tails[] = {0, 1, m - 1, m, m + 1, m + carry_len - 1, m + carry_len};
        for (uint32_t tail : tails) {
            std::vector<char> carry(carry_len), piece(m);
            for (char &c : carry) c = (char)('a' + rng.below(26));
            for (char &c : piece) c = (char)('A' + rng.below(26));
            std::vector<char> all(carry);
            all.insert(all.end(), piece.begin(), piece.end());
            const std::vector<char> want(all.end() - tail, all.end());
            phi_text_carry_update(carry, piece.data(), m, tail);
            ok = ok && carry == want;
            d += fmt("%u:%zu ", tail, carry.size());
        }
        // a piece of no bytes leaves the carry's tail
        std::vector<char> carry = {'x', 'y', 'z'};
        phi_text_carry_update(carry, "", 0, 2);
        ok = ok && carry == std::vector<char>({'y', 'z'});
        return ok;
    });
}

}  // namespace

int main()
{
    log_cases();
    overflow_cases();
    set_cases();
    offset_cases();
    fixed_point_cases();
    pool_cases();
    text_cases();
    printf("cases_failed %d\n", n_failed);
    return n_failed ? 1 : 0;
}
