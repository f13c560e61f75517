// region_host.h -- the rules of a region read of an indexed VCF and FASTA that need no GPU, as plain host code:
// what `tabix FILE REGION` and `samtools faidx FILE REGION` do before any record is looked at.
//   parse_region    NAME, NAME:BEG, NAME:BEG-END (1-based, inclusive, commas allowed) and its refusals
//   parse_tbi       the uncompressed bytes of a .tbi with the VCF preset, every count checked against the bytes that are left:
//                   several chunks per bin, chunks merged, pseudo-bin 37450 (skipped), n_no_coor of any value or absent
//   select_chunks   reg2bins over the 5 levels of 14 bits, the chunks that end at or before the linear index's value for the
//                   region's first window dropped, the rest sorted and merged where they touch or overlap
//   plan_members    the BGZF members those chunks lie in, followed by their BSIZE with pread (nothing is inflated), their ISIZE
//                   from their last four bytes, and every chunk as a byte range of the members' inflated concatenation
//   header_text     the ## lines and the #CHROM line, inflated from the file's first members
//   read_fai, fasta_slice   a record's bases [b, e) through .fai (and .gzi for a BGZF FASTA: only the members that hold them)
// The formats are read from their specifications (SAM/tabix "The Tabix index file format", samtools' faidx(5), bgzip's .gzi);
// the selection has NOT been compared with `tabix` or `bcftools`.  No HIP; host/region_host_selftest.cpp calls the same
// functions over bytes made in memory, tests/test_cpu_region.py through libphi_host.
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "bgzf_index_host.h"

namespace regionx {

constexpr int32_t PSEUDO_BIN = 37450;                   // htslib's bin of per-contig counts: no records
constexpr int64_t MAX_END = bgzfx::MAX_END;

// ------------------------------------------------------------------ the region string

struct Region {
    std::string name;
    int64_t beg1 = 1, end1 = -1;                        // 1-based, inclusive; end1 < 0: to the contig's end
};

// digits with commas between them, at most 18 digits: the value, or -1
inline int64_t region_number(const char *p, size_t n)
{
    int64_t v = 0;
    int digits = 0;
    for (size_t i = 0; i < n; i++) {
        if (p[i] == ',') continue;
        if (p[i] < '0' || p[i] > '9' || ++digits > 18) return -1;
        v = v * 10 + (p[i] - '0');
    }
    return digits ? v : -1;
}

// "" when the string is a region; else what is wrong with it.  The last ':' splits name and interval when digits, commas and at
// most one '-' follow it; a name may hold colons of its own (HLA-A*01:01)
inline std::string parse_region(const std::string &s, Region *out)
{
    *out = Region{};
    if (s.empty()) return "the region is empty";
    const size_t colon = s.rfind(':');
    bool interval = colon != std::string::npos;
    if (interval) {
        if (colon + 1 == s.size()) return "the region ends with ':'";
        for (size_t i = colon + 1; i < s.size() && interval; i++) interval = (s[i] >= '0' && s[i] <= '9') || s[i] == ',' || s[i] == '-';
    }
    if (!interval) { out->name = s; return ""; }
    if (colon == 0) return "the region has no contig name";
    out->name = s.substr(0, colon);
    const std::string iv = s.substr(colon + 1);
    const size_t dash = iv.find('-');
    if (dash != std::string::npos && iv.find('-', dash + 1) != std::string::npos) return "the region's interval holds more than one '-'";
    const std::string b = dash == std::string::npos ? iv : iv.substr(0, dash);
    out->beg1 = region_number(b.data(), b.size());
    if (out->beg1 < 0) return "the region's BEG is no number of at most 18 digits";
    if (out->beg1 < 1) return "the region's BEG is 0 (coordinates are 1-based)";
    if (dash != std::string::npos && dash + 1 < iv.size()) {
        out->end1 = region_number(iv.data() + dash + 1, iv.size() - dash - 1);
        if (out->end1 < 0) return "the region's END is no number of at most 18 digits";
        if (out->end1 < out->beg1) return "the region's END lies before its BEG (an inverted interval)";
    }
    return "";
}

// the half-open 0-based interval of a region on a contig of `len` bases: "" or why it is empty
inline std::string resolve_region(const Region &r, int64_t len, int64_t *b, int64_t *e)
{
    *b = r.beg1 - 1;
    *e = (r.end1 < 0 || r.end1 > len) ? len : r.end1;
    if (*b >= *e) return "the region is empty: it begins at base " + std::to_string(r.beg1) + ", the contig has " + std::to_string(len);
    return "";
}

// ------------------------------------------------------------------ .tbi

struct Chunk { uint64_t beg, end; };
struct TbiBin { uint32_t bin; std::vector<Chunk> chunks; };
struct TbiContig { std::string name; std::vector<TbiBin> bins; std::vector<uint64_t> lin; };
struct Tbi { std::vector<TbiContig> contigs; bool has_no_coor = false; uint64_t n_no_coor = 0; };

struct Cursor {                                         // bounds-checked little-endian reads
    const uint8_t *p; size_t n, at = 0;
    bool take(void *dst, size_t k) { if (k > n - at) return false; memcpy(dst, p + at, k); at += k; return true; }
    bool i32(int32_t *v) { uint8_t b[4]; if (!take(b, 4)) return false; *v = (int32_t)((uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24); return true; }
    bool u64(uint64_t *v) { uint8_t b[8]; if (!take(b, 8)) return false; *v = 0; for (int k = 7; k >= 0; k--) *v = (*v << 8) | b[k]; return true; }
    size_t left() const { return n - at; }
};

// "" when bytes[0, n) is a .tbi of the VCF preset; else what is refused
inline std::string parse_tbi(const uint8_t *bytes, size_t n, Tbi *out)
{
    *out = Tbi{};
    Cursor c{bytes, n};
    uint8_t magic[4];
    if (!c.take(magic, 4)) return "the index is shorter than its magic";
    if (memcmp(magic, "CSI\1", 4) == 0) return "a CSI index: unsupported (only .tbi is read)";
    if (memcmp(magic, "TBI\1", 4) != 0) return "no TBI magic";
    int32_t h[8];
    for (int k = 0; k < 8; k++) if (!c.i32(&h[k])) return "the index ends inside its header";
    const int32_t n_ref = h[0], l_nm = h[7];
    if ((h[1] & 0xffff) != 2 || h[2] != 1 || h[3] != 2 || h[5] != '#')
        return "the index has another preset than VCF (format 2, col_seq 1, col_beg 2, meta '#'): unsupported";
    if (n_ref < 0 || l_nm < 0 || (size_t)l_nm > c.left()) return "the index ends inside its names";
    const char *nm = (const char *)bytes + c.at;
    c.at += (size_t)l_nm;
    for (int32_t at = 0; at < l_nm;) {
        const void *z = memchr(nm + at, 0, (size_t)(l_nm - at));
        if (!z) return "a contig name of the index is not terminated";
        out->contigs.push_back(TbiContig{std::string(nm + at, (const char *)z), {}, {}});
        at = (int32_t)((const char *)z - nm) + 1;
    }
    if ((int64_t)out->contigs.size() != n_ref) return "the index names another number of contigs than n_ref";
    for (TbiContig &ctg : out->contigs) {
        int32_t n_bin;
        if (!c.i32(&n_bin) || n_bin < 0 || (size_t)n_bin > c.left() / 8) return "the index ends inside a contig's bins";
        ctg.bins.reserve((size_t)n_bin);
        for (int32_t k = 0; k < n_bin; k++) {
            int32_t bin, n_chunk;
            if (!c.i32(&bin) || !c.i32(&n_chunk) || n_chunk < 0 || (size_t)n_chunk > c.left() / 16) return "the index ends inside a bin";
            TbiBin b{(uint32_t)bin, {}};
            b.chunks.resize((size_t)n_chunk);
            for (Chunk &ch : b.chunks) if (!c.u64(&ch.beg) || !c.u64(&ch.end)) return "the index ends inside a chunk";
            ctg.bins.push_back(std::move(b));
        }
        int32_t n_intv;
        if (!c.i32(&n_intv) || n_intv < 0 || (size_t)n_intv > c.left() / 8) return "the index ends inside a linear index";
        ctg.lin.resize((size_t)n_intv);
        for (uint64_t &v : ctg.lin) if (!c.u64(&v)) return "the index ends inside a linear index";
    }
    if (c.left() == 8) { out->has_no_coor = true; (void)c.u64(&out->n_no_coor); }
    else if (c.left() != 0) return "the index ends inside n_no_coor, or bytes follow it";
    return "";
}

// every bin that can hold a record overlapping [beg, end), 0 <= beg < end <= MAX_END
inline std::vector<uint32_t> reg2bins(int64_t beg, int64_t end)
{
    --end;
    std::vector<uint32_t> bins{0};
    static const int shift[5] = {26, 23, 20, 17, 14};
    static const int first[5] = {1, 9, 73, 585, 4681};
    for (int l = 0; l < 5; l++)
        for (int64_t k = first[l] + (beg >> shift[l]); k <= first[l] + (end >> shift[l]); k++) bins.push_back((uint32_t)k);
    return bins;
}

// the chunks of contig c that can hold a record overlapping [b, e): sorted, merged where they touch or overlap
inline std::vector<Chunk> select_chunks(const TbiContig &c, int64_t b, int64_t e)
{
    std::vector<Chunk> out;
    if (b < 0) b = 0;
    if (e > MAX_END) e = MAX_END;
    if (b >= e || (uint64_t)(b >> bgzfx::LIN_SHIFT) >= c.lin.size()) return out;     // a window beyond the list: no records
    const uint64_t least = c.lin[(size_t)(b >> bgzfx::LIN_SHIFT)];
    std::vector<uint32_t> want = reg2bins(b, e);
    std::sort(want.begin(), want.end());
    for (const TbiBin &bin : c.bins) {
        if (bin.bin == (uint32_t)PSEUDO_BIN || !std::binary_search(want.begin(), want.end(), bin.bin)) continue;
        for (const Chunk &k : bin.chunks) if (k.end > least && k.end > k.beg) out.push_back(k);
    }
    std::sort(out.begin(), out.end(), [](const Chunk &x, const Chunk &y) { return x.beg != y.beg ? x.beg < y.beg : x.end < y.end; });
    size_t w = 0;
    for (size_t k = 0; k < out.size(); k++) {
        if (w && out[k].beg <= out[w - 1].end) out[w - 1].end = std::max(out[w - 1].end, out[k].end);
        else out[w++] = out[k];
    }
    out.resize(w);
    return out;
}

// ------------------------------------------------------------------ BGZF members, read with pread

struct Fd {
    int fd = -1;
    int64_t size = 0;
    ~Fd() { if (fd >= 0) ::close(fd); }
    bool open(const char *path)
    {
        fd = ::open(path, O_RDONLY);
        struct stat st;
        if (fd < 0 || fstat(fd, &st) != 0) return false;
        size = (int64_t)st.st_size;
        return true;
    }
    bool read(void *dst, int64_t n, int64_t at) const
    {
        if (at < 0 || n < 0 || at > size || n > size - at) return false;
        for (int64_t got = 0; got < n;) {
            const ssize_t r = pread(fd, (char *)dst + got, (size_t)(n - got), (off_t)(at + got));
            if (r <= 0) return false;
            got += r;
        }
        return true;
    }
};

inline bool is_gzip(const Fd &f) { uint8_t m[2]; return f.size >= 2 && f.read(m, 2, 0) && m[0] == 0x1f && m[1] == 0x8b; }

struct Member { int64_t at, size, data_at, isize; };    // file offset, BSIZE + 1, where the deflate data begins, ISIZE

// the BGZF member at offset `at` of what f.read(dst, n, at) reads: false when there is none (no gzip header with the BC subfield,
// or it runs past the end)
template <class Reader>
inline bool member_at(const Reader &f, int64_t at, Member *m)
{
    uint8_t h[12];
    if (!f.read(h, 12, at) || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return false;
    const int64_t xlen = h[10] | ((int64_t)h[11] << 8);
    std::vector<uint8_t> x((size_t)xlen);
    if (!f.read(x.data(), xlen, at + 12)) return false;
    for (int64_t k = 0; k + 4 <= xlen;) {
        const int64_t slen = x[(size_t)k + 2] | ((int64_t)x[(size_t)k + 3] << 8);
        if (x[(size_t)k] == 'B' && x[(size_t)k + 1] == 'C' && slen == 2 && k + 6 <= xlen) {
            const int64_t size = (x[(size_t)k + 4] | ((int64_t)x[(size_t)k + 5] << 8)) + 1;
            uint8_t t[4];
            if (size < 12 + xlen + 8 || !f.read(t, 4, at + size - 4)) return false;
            *m = Member{at, size, at + 12 + xlen, (int64_t)t[0] | ((int64_t)t[1] << 8) | ((int64_t)t[2] << 16) | ((int64_t)t[3] << 24)};
            return true;
        }
        k += 4 + slen;
    }
    return false;
}

// bytes in memory read as a file is
struct Bytes {
    const uint8_t *p;
    int64_t size;
    bool read(void *dst, int64_t n, int64_t at) const
    {
        if (at < 0 || n < 0 || at > size || n > size - at) return false;
        if (n) memcpy(dst, p + at, (size_t)n);
        return true;
    }
};

// the member's text appended to out: false for a corrupt member (deflate, ISIZE or CRC32)
inline bool inflate_member(const Fd &f, const Member &m, std::vector<char> &out)
{
    std::vector<uint8_t> raw((size_t)m.size);
    if (!f.read(raw.data(), m.size, m.at)) return false;
    const size_t o = out.size();
    out.resize(o + (size_t)m.isize);
    if (m.isize == 0) return true;
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = raw.data() + (m.data_at - m.at);
    zs.avail_in = (uInt)(m.size - (m.data_at - m.at) - 8);
    zs.next_out = (unsigned char *)out.data() + o;
    zs.avail_out = (uInt)m.isize;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.avail_out == 0;
    inflateEnd(&zs);
    if (!ok) return false;
    const uint8_t *t = raw.data() + m.size - 8;
    const uint32_t want = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    return (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const unsigned char *)out.data() + o, (uInt)m.isize) == want;
}

// ------------------------------------------------------------------ the member plan

struct Plan {
    std::vector<Member> members;                        // ascending file offsets, each once
    std::vector<int64_t> text_off;                      // [members + 1]: where each begins in the inflated concatenation
    std::vector<int64_t> range;                         // [2 * n]: every chunk as [p0, p1) of that concatenation, ascending, disjoint
    std::vector<char> gz;                               // the members' compressed bytes back to back: a multi-member gzip stream
};

// "" or what is wrong with the index or the file
inline std::string plan_members(const Fd &f, const std::vector<Chunk> &chunks, Plan *out, bool load = true)
{
    *out = Plan{};
    out->text_off.push_back(0);
    auto add = [&](const Member &m) {
        out->members.push_back(m);
        out->text_off.push_back(out->text_off.back() + m.isize);
    };
    for (const Chunk &k : chunks) {
        const int64_t c0 = (int64_t)(k.beg >> 16), u0 = (int64_t)(k.beg & 0xffff), c1 = (int64_t)(k.end >> 16), u1 = (int64_t)(k.end & 0xffff);
        if (!out->members.empty() && c0 < out->members.back().at) return "the index's chunks overlap after merging (internal error)";
        int64_t at = c0, p0 = -1, p1 = -1;
        for (;;) {
            const bool last = at == c1;
            if (last && u1 == 0) break;
            Member m;
            if (!out->members.empty() && out->members.back().at == at) m = out->members.back();      // (the chunk before ended inside it)
            else {
                if (!member_at(f, at, &m)) return "no BGZF member at file offset " + std::to_string(at) + ", where the index points";
                add(m);
            }
            const int64_t base = out->text_off[out->text_off.size() - 2];
            if (at == c0) { if (u0 > m.isize) return "a chunk begins behind the end of its member (file offset " + std::to_string(at) + ")"; p0 = base + u0; }
            if (last) { if (u1 > m.isize) return "a chunk ends behind the end of its member (file offset " + std::to_string(at) + ")"; p1 = base + u1; break; }
            at += m.size;
            if (at > c1) return "a chunk's end (file offset " + std::to_string(c1) + ") is no member's first byte";
        }
        if (p0 < 0) continue;                            // (an empty chunk at a member's first byte)
        if (p1 < 0) p1 = out->text_off.back();
        if (p1 > p0) { out->range.push_back(p0); out->range.push_back(p1); }
    }
    if (load) {
        int64_t total = 0;
        for (const Member &m : out->members) total += m.size;
        out->gz.resize((size_t)total);
        int64_t o = 0;
        for (const Member &m : out->members) {
            if (!f.read(out->gz.data() + o, m.size, m.at)) return "cannot read the member at file offset " + std::to_string(m.at);
            o += m.size;
        }
    }
    return "";
}

// every ## line and the #CHROM line of a BGZF VCF, inflated from the file's first members
inline std::string header_text(const Fd &f, std::vector<char> *out)
{
    out->clear();
    size_t line = 0;                                    // where the line under inspection begins
    for (int64_t at = 0; at < f.size;) {
        Member m;
        if (!member_at(f, at, &m)) return "no BGZF member at file offset " + std::to_string(at);
        if (!inflate_member(f, m, *out)) return "the member at file offset " + std::to_string(at) + " is corrupt";
        at += m.size;
        for (;;) {
            if (line < out->size() && (*out)[line] != '#') { out->resize(line); return ""; }      // a record: the header is over
            const void *nl = line < out->size() ? memchr(out->data() + line, '\n', out->size() - line) : nullptr;
            if (!nl) break;
            const size_t next = (size_t)((const char *)nl - out->data()) + 1;
            const bool chrom = next - line >= 6 && memcmp(out->data() + line, "#CHROM", 6) == 0;
            line = next;
            if (chrom) { out->resize(line); return ""; }
        }
    }
    if (!out->empty() && out->back() != '\n') out->push_back('\n');
    return "";
}

// ------------------------------------------------------------------ .fai, .gzi, the reference slice

struct FaiRecord { std::string name; int64_t len, offset, line_bases, line_width; };

inline std::string parse_fai(const char *text, size_t n, std::vector<FaiRecord> *out)
{
    out->clear();
    for (size_t at = 0; at < n;) {
        const void *nl = memchr(text + at, '\n', n - at);
        size_t le = nl ? (size_t)((const char *)nl - text) : n;
        const size_t next = nl ? le + 1 : n;
        if (le > at && text[le - 1] == '\r') le--;
        if (le > at) {
            std::vector<std::pair<size_t, size_t>> col;
            for (size_t s = at;;) {
                const void *t = memchr(text + s, '\t', le - s);
                const size_t ce = t ? (size_t)((const char *)t - text) : le;
                col.emplace_back(s, ce);
                if (!t) break;
                s = ce + 1;
            }
            const std::string where = "line " + std::to_string(out->size() + 1) + " of the .fai";
            if (col.size() < 5) return where + " has fewer than 5 columns";
            int64_t v[4];
            for (int k = 0; k < 4; k++) {
                v[k] = 0;
                const size_t a = col[(size_t)k + 1].first, b = col[(size_t)k + 1].second;
                if (b == a || b - a > 18) return where + ": column " + std::to_string(k + 2) + " is no number";
                for (size_t i = a; i < b; i++) {
                    if (text[i] < '0' || text[i] > '9') return where + ": column " + std::to_string(k + 2) + " is no number";
                    v[k] = v[k] * 10 + (text[i] - '0');
                }
            }
            if (v[2] < 1 || v[3] < v[2]) return where + ": LINEBASES " + std::to_string(v[2]) + ", LINEWIDTH " + std::to_string(v[3]);
            out->push_back(FaiRecord{std::string(text + col[0].first, col[0].second - col[0].first), v[0], v[1], v[2], v[3]});
        }
        at = next;
    }
    return "";
}

// where base i of the record stands in the uncompressed file
inline int64_t fai_offset(const FaiRecord &r, int64_t i) { return r.offset + (i / r.line_bases) * r.line_width + i % r.line_bases; }

// the uncompressed byte range [u0, u1) that holds bases [b, e), 0 <= b < e <= len
inline void fai_range(const FaiRecord &r, int64_t b, int64_t e, int64_t *u0, int64_t *u1) { *u0 = fai_offset(r, b); *u1 = fai_offset(r, e - 1) + 1; }

// raw[0, n) without its line ends, upper-cased, appended to out
inline void fasta_bases(const char *raw, size_t n, std::vector<char> *out)
{
    for (size_t i = 0; i < n; i++) {
        const char c = raw[i];
        if (c == '\n' || c == '\r') continue;
        out->push_back((c >= 'a' && c <= 'z') ? (char)(c - 32) : c);
    }
}

// .gzi: pairs (compressed offset, uncompressed offset) of the members 1.., with (0, 0) put in front
inline std::string parse_gzi(const uint8_t *bytes, size_t n, std::vector<std::pair<int64_t, int64_t>> *out)
{
    out->assign(1, {0, 0});
    Cursor c{bytes, n};
    uint64_t count;
    if (!c.u64(&count) || count > c.left() / 16 || c.left() != count * 16) return "the .gzi's size does not fit its count";
    for (uint64_t k = 0; k < count; k++) {
        uint64_t a = 0, b = 0;
        (void)c.u64(&a); (void)c.u64(&b);
        if ((int64_t)a <= out->back().first || (int64_t)b < out->back().second) return "the .gzi's offsets do not ascend";
        out->emplace_back((int64_t)a, (int64_t)b);
    }
    return "";
}

inline bool read_whole(const std::string &path, std::vector<char> *out)
{
    Fd f;
    if (!f.open(path.c_str())) return false;
    out->resize((size_t)f.size);
    return f.read(out->data(), f.size, 0);
}

// bases [b, e) of record r of the FASTA at path (plain, or BGZF with path + ".gzi"), upper-cased: "" or what is refused
inline std::string fasta_slice(const std::string &path, const FaiRecord &r, int64_t b, int64_t e, std::vector<char> *out, int64_t *members_read = nullptr)
{
    out->clear();
    if (members_read) *members_read = 0;
    if (b < 0 || e > r.len || b > e) return "bases [" + std::to_string(b) + ", " + std::to_string(e) + ") lie outside the record";
    if (b == e) return "";
    Fd f;
    if (!f.open(path.c_str())) return "cannot open " + path;
    int64_t u0, u1;
    fai_range(r, b, e, &u0, &u1);
    std::vector<char> raw;
    if (!is_gzip(f)) {
        raw.resize((size_t)(u1 - u0));
        if (!f.read(raw.data(), u1 - u0, u0)) return path + " ends before byte " + std::to_string(u1) + ", where its .fai puts the bases";
    } else {
        Member m;
        if (!member_at(f, 0, &m)) return path + " is gzip but not BGZF: a region read needs bgzip's blocks";
        std::vector<char> gzi_raw;
        if (!read_whole(path + ".gzi", &gzi_raw)) return "cannot open " + path + ".gzi (bgzip -r writes it; a BGZF FASTA is sliced through it)";
        std::vector<std::pair<int64_t, int64_t>> pairs;
        const std::string why = parse_gzi((const uint8_t *)gzi_raw.data(), gzi_raw.size(), &pairs);
        if (!why.empty()) return path + ".gzi: " + why;
        size_t k = (size_t)(std::upper_bound(pairs.begin(), pairs.end(), u0, [](int64_t u, const std::pair<int64_t, int64_t> &p) { return u < p.second; }) - pairs.begin()) - 1;
        const int64_t first = pairs[k].second;
        for (; k < pairs.size() && pairs[k].second < u1; k++) {
            if (!member_at(f, pairs[k].first, &m)) return "no BGZF member at file offset " + std::to_string(pairs[k].first) + ", where " + path + ".gzi points";
            if (!inflate_member(f, m, raw)) return "the member of " + path + " at file offset " + std::to_string(m.at) + " is corrupt";
            if (members_read) ++*members_read;
        }
        if ((int64_t)raw.size() < u1 - first) return path + " ends before byte " + std::to_string(u1) + ", where its .fai puts the bases";
        raw.erase(raw.begin(), raw.begin() + (u0 - first));
        raw.resize((size_t)(u1 - u0));
    }
    out->reserve((size_t)(e - b));
    fasta_bases(raw.data(), raw.size(), out);
    if ((int64_t)out->size() != e - b) return path + ".fai does not describe the file: " + std::to_string(out->size()) + " bases where " + std::to_string(e - b) + " were asked for";
    return "";
}

}  // namespace regionx
