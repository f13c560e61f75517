// bgzf_index_selftest.cpp -- ../bgzf_index_host.h on the CPU: reg2bin, virtual offsets, the bytes of a .gzi, the grouping of
// chunks by bin, the filling of empty windows and the layout of a .tbi, as the indexed BGZF writer (../bgzf_index.hip) calls
// them, over hand-made chunk lists and window arrays.  Prints one line per check ("name ok ..." or "name FAILED ..."); exit
// status 1 if any failed.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../bgzf_index_host.h"

using namespace bgzfx;

static int n_failed = 0;
static void line(const char *name, bool ok, const std::string &what)
{
    printf("%s %s %s\n", name, ok ? "ok" : "FAILED", what.c_str());
    if (!ok) n_failed++;
}

// the bin by the definition: the smallest interval of the five levels' grid that holds [beg, end), else bin 0
static int32_t bin_by_definition(int64_t beg, int64_t end)
{
    const int shift[5] = {14, 17, 20, 23, 26};
    const int32_t first[5] = {4681, 585, 73, 9, 1};
    for (int l = 0; l < 5; l++) {
        const int64_t size = (int64_t)1 << shift[l], k = beg / size;
        if (end <= (k + 1) * size) return first[l] + (int32_t)k;
    }
    return 0;
}

static uint32_t get_u32(const std::vector<uint8_t> &b, size_t &at)
{
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) v |= (uint32_t)b.at(at + k) << (8 * k);
    at += 4;
    return v;
}
static uint64_t get_u64(const std::vector<uint8_t> &b, size_t &at)
{
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)b.at(at + k) << (8 * k);
    at += 8;
    return v;
}

int main()
{
    // ---- reg2bin at every edge of every level, intervals of length 1, 2 and up to the level's size, and the whole range
    {
        long checked = 0, bad = 0;
        const int shift[5] = {14, 17, 20, 23, 26};
        for (int l = 0; l < 5; l++) {
            const int64_t size = (int64_t)1 << shift[l];
            for (int64_t edge = 0; edge <= MAX_END; edge += size) {
                const int64_t begs[5] = {edge - size, edge - 2, edge - 1, edge, edge + 1};
                const int64_t lens[5] = {1, 2, size - 1, size, size + 1};
                for (int64_t beg : begs)
                    for (int64_t len : lens) {
                        if (beg < 0 || beg + len > MAX_END) continue;
                        checked++;
                        bad += reg2bin(beg, beg + len) != bin_by_definition(beg, beg + len);
                    }
            }
        }
        bad += reg2bin(0, MAX_END) != 0 || reg2bin(0, 1) != 4681 || reg2bin(MAX_END - 1, MAX_END) != 4681 + 32767 || reg2bin(16383, 16385) != 585;
        bad += reg2bin(((int64_t)1 << 26) - 1, ((int64_t)1 << 26) + 1) != 0 || reg2bin((int64_t)1 << 26, ((int64_t)1 << 26) + 1) != 4681 + 4096;
        line("reg2bin", bad == 0, "checked=" + std::to_string(checked) + " bad=" + std::to_string(bad));
    }
    // ---- virtual offsets and the .gzi
    {
        const int64_t off[4] = {0, 1000, 70000, 70028};          // three members, then the EOF block
        int bad = 0;
        bad += virtual_offset(off, 0) != 0;
        bad += virtual_offset(off, BLOCK - 1) != (uint64_t)(BLOCK - 1);
        bad += virtual_offset(off, BLOCK) != ((uint64_t)1000 << 16);
        bad += virtual_offset(off, 2 * BLOCK + 5) != (((uint64_t)70000 << 16) | 5);
        bad += virtual_offset(off, 3 * BLOCK) != ((uint64_t)70028 << 16);          // n a multiple of the block: the EOF block
        const std::vector<uint8_t> g = gzi_bytes(off, 3);
        size_t at = 0;
        bad += g.size() != 8 + 2 * 16 || get_u64(g, at) != 2 || get_u64(g, at) != 1000 || get_u64(g, at) != (uint64_t)BLOCK || get_u64(g, at) != 70000 ||
               get_u64(g, at) != (uint64_t)(2 * BLOCK);
        const std::vector<uint8_t> g1 = gzi_bytes(off, 1), g0 = gzi_bytes(off, 0);
        bad += g1 != std::vector<uint8_t>(8, 0) || g0 != std::vector<uint8_t>(8, 0);
        line("gzi", bad == 0, "bad=" + std::to_string(bad));
    }
    // ---- grouping: bins ascend, chunks of a bin keep file order
    const std::vector<Chunk> chunks = {{4681, 10, 20}, {585, 20, 30}, {4681, 30, 40}, {0, 40, 50}, {4682, 50, 60}, {585, 60, 70}, {4681, 70, 80}};
    {
        const std::vector<Bin> bins = group_bins(chunks.data(), (int64_t)chunks.size());
        int bad = bins.size() != 4;
        const int32_t want_bin[4] = {0, 585, 4681, 4682};
        const std::vector<std::vector<uint64_t>> want_beg = {{40}, {20, 60}, {10, 30, 70}, {50}};
        for (size_t b = 0; b < bins.size() && b < 4; b++) {
            bad += bins[b].bin != want_bin[b] || bins[b].chunks.size() != want_beg[b].size();
            for (size_t k = 0; k < bins[b].chunks.size() && k < want_beg[b].size(); k++) bad += bins[b].chunks[k].beg != want_beg[b][k] || bins[b].chunks[k].end != want_beg[b][k] + 10;
        }
        bad += !group_bins(nullptr, 0).empty();
        line("group_bins", bad == 0, "bins=" + std::to_string(bins.size()) + " bad=" + std::to_string(bad));
    }
    // ---- back-fill
    {
        std::vector<uint64_t> lin = {NO_OFFSET, NO_OFFSET, 7, NO_OFFSET, 9, 9, NO_OFFSET, NO_OFFSET, 30};
        const std::vector<uint64_t> want = {0, 0, 7, 7, 9, 9, 9, 9, 30};
        backfill(lin.data(), (int64_t)lin.size());
        std::vector<uint64_t> all_empty(3, NO_OFFSET);
        backfill(all_empty.data(), 3);
        backfill(nullptr, 0);
        const int bad = (lin != want) + (all_empty != std::vector<uint64_t>(3, 0)) + (n_windows(1) != 1) + (n_windows(16384) != 1) + (n_windows(16385) != 2) +
                        (n_windows(MAX_END) != 32768);
        line("backfill", bad == 0, "bad=" + std::to_string(bad));
    }
    // ---- names
    {
        const int bad = (repeated_name({"a", "b", "c"}) != -1) + (repeated_name({"a", "b", "a", "b"}) != 2) + (repeated_name({}) != -1) + (repeated_name({"x", "x"}) != 1);
        line("names", bad == 0, "bad=" + std::to_string(bad));
    }
    // ---- the layout, read back field by field
    {
        std::vector<TbiContig> ctg(2);
        ctg[0].name = "chr1";
        ctg[0].chunks = chunks;
        ctg[0].lin = {NO_OFFSET, 10, NO_OFFSET};
        ctg[1].name = "c2";
        ctg[1].chunks = {{4681, 80, 90}};
        ctg[1].lin = {80};
        TbiCounts cnt;
        const std::vector<uint8_t> b = tbi_bytes(ctg, &cnt);
        size_t at = 4;
        int bad = memcmp(b.data(), "TBI\1", 4) != 0;
        const uint32_t want_head[8] = {2, 2, 1, 2, 0, '#', 0, 8};
        for (uint32_t w : want_head) bad += get_u32(b, at) != w;
        bad += memcmp(b.data() + at, "chr1\0c2\0", 8) != 0;
        at += 8;
        bad += get_u32(b, at) != 4;                                     // contig 0: four bins
        const uint32_t want_bins[4][2] = {{0, 1}, {585, 2}, {4681, 3}, {4682, 1}};
        for (const auto &wb : want_bins) {
            bad += get_u32(b, at) != wb[0];
            const uint32_t nc = get_u32(b, at);
            bad += nc != wb[1];
            for (uint32_t k = 0; k < nc; k++) { const uint64_t beg = get_u64(b, at), end = get_u64(b, at); bad += end != beg + 10; }
        }
        bad += get_u32(b, at) != 3 || get_u64(b, at) != 0 || get_u64(b, at) != 10 || get_u64(b, at) != 10;
        bad += get_u32(b, at) != 1 || get_u32(b, at) != 4681 || get_u32(b, at) != 1 || get_u64(b, at) != 80 || get_u64(b, at) != 90;
        bad += get_u32(b, at) != 1 || get_u64(b, at) != 80;
        bad += get_u64(b, at) != 0 || at != b.size();                   // n_no_coor, and nothing behind it
        bad += cnt.bins != 5 || cnt.chunks != 8 || cnt.windows != 4;
        std::vector<TbiContig> none;
        const std::vector<uint8_t> e = tbi_bytes(none, &cnt);
        at = 4;
        bad += e.size() != 4 + 8 * 4 + 8 || get_u32(e, at) != 0 || cnt.bins != 0 || cnt.chunks != 0 || cnt.windows != 0;
        line("tbi_layout", bad == 0, "bytes=" + std::to_string(b.size()) + " bad=" + std::to_string(bad));
    }
    return n_failed ? 1 : 0;
}
