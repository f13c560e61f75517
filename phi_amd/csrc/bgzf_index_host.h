// bgzf_index_host.h -- the rules of the BGZF indexes that need no GPU, as plain host code: virtual offsets,
// reg2bin, the bytes of a .gzi, and from the chunk list and the window arrays that bgzf_index.hip brings back from the device
// the bytes of a .tbi -- chunks grouped by bin, empty windows filled from their predecessor, the layout.  No HIP, no host
// threads; host/bgzf_index_selftest.cpp calls the same functions over hand-made lists.
//
// The formats are written from their specifications (SAM/tabix: "The Tabix index file format"; bgzip's .gzi: a count and pairs
// of offsets) and from the rules stated in include/phi_amd.h.  They are NOT compared with the output of `tabix -p vcf` or
// `bgzip -i`: htslib merges nearby chunks and adds a pseudo-bin, this writer does neither (both are allowed by the format).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

namespace bgzfx {

constexpr int64_t BLOCK = 65280;                        // PHI_BGZF_BLOCK
constexpr int64_t MAX_END = (int64_t)1 << 29;           // what the 5-level, 14-bit binning covers
constexpr int LIN_SHIFT = 14;
constexpr uint64_t NO_OFFSET = ~(uint64_t)0;            // an empty window, as the device's atomicMin leaves it
constexpr int64_t MAX_NAME = 1024;

// off[0..nb]: the file offsets of the members, off[nb] the EOF block's.  p in [0, n]
inline uint64_t virtual_offset(const int64_t *off, int64_t p) { return ((uint64_t)off[p / BLOCK] << 16) | (uint64_t)(p % BLOCK); }

// [beg, end) zero-based, end > beg, end <= MAX_END
inline int32_t reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (int32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int32_t)(1 + (beg >> 26));
    return 0;
}

inline void put_u32(std::vector<uint8_t> &o, uint32_t v) { for (int k = 0; k < 4; k++) o.push_back((uint8_t)(v >> (8 * k))); }
inline void put_u64(std::vector<uint8_t> &o, uint64_t v) { for (int k = 0; k < 8; k++) o.push_back((uint8_t)(v >> (8 * k))); }

// .gzi: the count nb - 1, then for the members 1 .. nb-1 where they begin, compressed and uncompressed
inline std::vector<uint8_t> gzi_bytes(const int64_t *off, int64_t nb)
{
    std::vector<uint8_t> o;
    put_u64(o, (uint64_t)(nb > 1 ? nb - 1 : 0));
    for (int64_t b = 1; b < nb; b++) { put_u64(o, (uint64_t)off[b]); put_u64(o, (uint64_t)(BLOCK * b)); }
    return o;
}

// a maximal run of consecutive records of one contig and one bin: [beg, end) as virtual offsets
struct Chunk { int32_t bin; uint64_t beg, end; };
struct Bin { int32_t bin; std::vector<Chunk> chunks; };

// the chunks of one contig, in file order -> its bins in ascending number, every bin's chunks in file order
inline std::vector<Bin> group_bins(const Chunk *ch, int64_t n)
{
    std::vector<int64_t> order((size_t)n);
    for (int64_t k = 0; k < n; k++) order[(size_t)k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return ch[a].bin < ch[b].bin; });
    std::vector<Bin> bins;
    for (int64_t k : order) {
        if (bins.empty() || bins.back().bin != ch[k].bin) bins.push_back(Bin{ch[k].bin, {}});
        bins.back().chunks.push_back(ch[k]);
    }
    return bins;
}

// an empty window takes its predecessor's value; leading empty windows are 0
inline void backfill(uint64_t *lin, int64_t n)
{
    uint64_t last = 0;
    for (int64_t w = 0; w < n; w++) {
        if (lin[w] == NO_OFFSET) lin[w] = last;
        else last = lin[w];
    }
}

// the windows of a contig whose records end at max_end at the latest (max_end >= 1)
inline int64_t n_windows(int64_t max_end) { return ((max_end - 1) >> LIN_SHIFT) + 1; }

// the first contig whose name an earlier contig has: -1 when every name is new (a name that comes back after another contig)
inline int64_t repeated_name(const std::vector<std::string> &names)
{
    std::vector<std::pair<std::string, int64_t>> s;
    for (size_t c = 0; c < names.size(); c++) s.emplace_back(names[c], (int64_t)c);
    std::sort(s.begin(), s.end());
    int64_t first = -1;
    for (size_t k = 1; k < s.size(); k++)
        if (s[k].first == s[k - 1].first && (first < 0 || s[k].second < first)) first = s[k].second;
    return first;
}

struct TbiContig {
    std::string name;
    std::vector<Chunk> chunks;      // file order
    std::vector<uint64_t> lin;      // n_windows(max end) values, NO_OFFSET where no record overlaps
};
struct TbiCounts { int64_t bins = 0, chunks = 0, windows = 0; };

// the uncompressed bytes of a .tbi with the VCF preset (the file is these bytes as BGZF)
inline std::vector<uint8_t> tbi_bytes(std::vector<TbiContig> &ctg, TbiCounts *cnt)
{
    std::vector<uint8_t> o;
    const uint8_t magic[4] = {'T', 'B', 'I', 1};
    o.insert(o.end(), magic, magic + 4);
    int64_t l_nm = 0;
    for (const TbiContig &c : ctg) l_nm += (int64_t)c.name.size() + 1;
    put_u32(o, (uint32_t)ctg.size());
    put_u32(o, 2);                  // format: VCF
    put_u32(o, 1);                  // col_seq
    put_u32(o, 2);                  // col_beg
    put_u32(o, 0);                  // col_end
    put_u32(o, (uint32_t)'#');      // meta
    put_u32(o, 0);                  // skip
    put_u32(o, (uint32_t)l_nm);
    for (const TbiContig &c : ctg) { o.insert(o.end(), c.name.begin(), c.name.end()); o.push_back(0); }
    TbiCounts t;
    for (TbiContig &c : ctg) {
        const std::vector<Bin> bins = group_bins(c.chunks.data(), (int64_t)c.chunks.size());
        put_u32(o, (uint32_t)bins.size());
        for (const Bin &b : bins) {
            put_u32(o, (uint32_t)b.bin);
            put_u32(o, (uint32_t)b.chunks.size());
            for (const Chunk &k : b.chunks) { put_u64(o, k.beg); put_u64(o, k.end); }
            t.chunks += (int64_t)b.chunks.size();
        }
        t.bins += (int64_t)bins.size();
        backfill(c.lin.data(), (int64_t)c.lin.size());
        put_u32(o, (uint32_t)c.lin.size());
        for (uint64_t v : c.lin) put_u64(o, v);
        t.windows += (int64_t)c.lin.size();
    }
    put_u64(o, 0);                  // n_no_coor
    if (cnt) *cnt = t;
    return o;
}

}  // namespace bgzfx
