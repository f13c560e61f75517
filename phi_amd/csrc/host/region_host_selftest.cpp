// region_host_selftest.cpp -- the plain host code of ../region_host.h in a program of its own (make region_host_sanitize: plain,
// and under AddressSanitizer + UndefinedBehaviorSanitizer); tests/test_cpu_region.py runs it.  Every section prints "ok NAME".
//   region_grammar    NAME, NAME:BEG, NAME:BEG-END, commas, names with colons, every refusal, the interval on a contig
//   tbi_parse         an index built in memory by the writer's own layout (../bgzf_index_host.h) read back field for field
//   chunk_selection   for random regions the selected chunks cover every record that overlaps, none ends at or before the
//                     linear index's value, and they are sorted and disjoint; windows beyond the list select nothing
//   htslib_style      the same index with the chunks of a bin merged, pseudo-bin 37450 added and n_no_coor 7 or absent
//   tbi_truncated     the index cut at every byte: refused (the one cut that only drops n_no_coor is read), nothing read
//                     out of bounds -- the buffer is exactly as long as the cut
//   fai_arithmetic    offsets at line ends and on the last, shorter line; the slice of a file written here, plain
//   member_plan       a BGZF file written here with zlib: members, ISIZE sums, ranges, the bytes of the members back to back
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <string>
#include <vector>
#include "../region_host.h"

using namespace regionx;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

struct Rec { int64_t beg, end; uint64_t vbeg, vend; };

// records of one contig, 40 bytes of text each, members of 4000 bytes of text at file offsets 1000 apart
static std::vector<Rec> make_records(std::mt19937_64 &rng, int n)
{
    std::vector<Rec> r;
    int64_t pos = 0;
    for (int i = 0; i < n; i++) {
        pos += (int64_t)(rng() % 3000);
        int64_t len = 1 + (int64_t)(rng() % 5);
        if (i % 37 == 0) len = 20000 + (int64_t)(rng() % 300000);       // long records: higher levels of the binning
        const int64_t p = 40 * (int64_t)i, q = p + 40;
        r.push_back(Rec{pos, pos + len, (uint64_t)(p / 4000 * 1000) << 16 | (uint64_t)(p % 4000), (uint64_t)(q / 4000 * 1000) << 16 | (uint64_t)(q % 4000)});
    }
    return r;
}

static bgzfx::TbiContig contig_of(const std::string &name, const std::vector<Rec> &recs)
{
    bgzfx::TbiContig c;
    c.name = name;
    int64_t max_end = 1;
    for (const Rec &r : recs) max_end = std::max(max_end, r.end);
    c.lin.assign((size_t)bgzfx::n_windows(max_end), bgzfx::NO_OFFSET);
    for (size_t i = 0; i < recs.size(); i++) {
        const Rec &r = recs[i];
        const int32_t bin = bgzfx::reg2bin(r.beg, r.end);
        if (!c.chunks.empty() && c.chunks.back().bin == bin) c.chunks.back().end = r.vend;
        else c.chunks.push_back(bgzfx::Chunk{bin, r.vbeg, r.vend});
        for (int64_t w = r.beg >> 14; w <= (r.end - 1) >> 14; w++) c.lin[(size_t)w] = std::min(c.lin[(size_t)w], r.vbeg);
    }
    return c;
}

// the index rewritten: a bin's chunks merged where one ends in the member the next begins in, pseudo-bin 37450, n_no_coor
static std::vector<uint8_t> htslib_bytes(const Tbi &t, int no_coor /* < 0: absent */)
{
    std::vector<uint8_t> o{'T', 'B', 'I', 1};
    int64_t l_nm = 0;
    for (const TbiContig &c : t.contigs) l_nm += (int64_t)c.name.size() + 1;
    const uint32_t h[8] = {(uint32_t)t.contigs.size(), 2, 1, 2, 0, '#', 0, (uint32_t)l_nm};
    for (uint32_t v : h) bgzfx::put_u32(o, v);
    for (const TbiContig &c : t.contigs) { o.insert(o.end(), c.name.begin(), c.name.end()); o.push_back(0); }
    for (const TbiContig &c : t.contigs) {
        bgzfx::put_u32(o, (uint32_t)c.bins.size() + 1);
        for (const TbiBin &b : c.bins) {
            std::vector<Chunk> m;
            for (const Chunk &k : b.chunks) {
                if (!m.empty() && (m.back().end >> 16) >= (k.beg >> 16) && k.beg >= m.back().end) m.back().end = k.end;
                else m.push_back(k);
            }
            bgzfx::put_u32(o, b.bin);
            bgzfx::put_u32(o, (uint32_t)m.size());
            for (const Chunk &k : m) { bgzfx::put_u64(o, k.beg); bgzfx::put_u64(o, k.end); }
        }
        bgzfx::put_u32(o, (uint32_t)PSEUDO_BIN);
        bgzfx::put_u32(o, 2);
        for (uint64_t v : {(uint64_t)0, ~(uint64_t)0 >> 1, (uint64_t)12345, (uint64_t)0}) bgzfx::put_u64(o, v);      // offsets of the contig, counts
        bgzfx::put_u32(o, (uint32_t)c.lin.size());
        for (uint64_t v : c.lin) bgzfx::put_u64(o, v);
    }
    if (no_coor >= 0) bgzfx::put_u64(o, (uint64_t)no_coor);
    return o;
}

static void check_selection(const Tbi &t, const std::vector<std::vector<Rec>> &recs, std::mt19937_64 &rng)
{
    for (int trial = 0; trial < 3000; trial++) {
        const size_t ci = (size_t)(rng() % t.contigs.size());
        const TbiContig &c = t.contigs[ci];
        const std::vector<Rec> &rs = recs[ci];
        const Rec &pick = rs[(size_t)(rng() % rs.size())];
        static const int64_t widths[6] = {1, 10, 1000, 20000, 400000, 50000000};
        const int64_t w = widths[rng() % 6];
        const int64_t b = std::max<int64_t>(0, pick.beg - (int64_t)(rng() % (uint64_t)w)), e = std::min(MAX_END, std::max(b + 1, pick.end + (int64_t)(rng() % (uint64_t)w) - 2));
        const std::vector<Chunk> sel = select_chunks(c, b, e);
        const uint64_t least = (size_t)(b >> 14) < c.lin.size() ? c.lin[(size_t)(b >> 14)] : ~(uint64_t)0;
        for (size_t k = 0; k < sel.size(); k++) {
            CHECK(sel[k].end > sel[k].beg && sel[k].end > least);
            if (k) CHECK(sel[k].beg > sel[k - 1].end);
        }
        for (const Rec &r : rs) {
            if (!(r.beg < e && r.end > b)) continue;
            bool covered = false;
            for (const Chunk &k : sel) covered = covered || (k.beg <= r.vbeg && r.vend <= k.end);
            CHECK(covered);
            if (!covered) return;
        }
    }
    for (const TbiContig &c : t.contigs) {
        const int64_t beyond = (int64_t)c.lin.size() << 14;
        CHECK(select_chunks(c, beyond, beyond + 100).empty() && select_chunks(c, MAX_END, MAX_END + 5).empty());
        CHECK(select_chunks(c, 500, 500).empty() && select_chunks(c, 600, 500).empty());
        CHECK(!select_chunks(c, 0, MAX_END + 1000).empty());
    }
}

static std::vector<uint8_t> bgzf_member(const std::string &text)
{
    std::vector<uint8_t> body(compressBound((uLong)text.size()) + 16);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    deflateInit2(&zs, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
    zs.next_in = (Bytef *)text.data();
    zs.avail_in = (uInt)text.size();
    zs.next_out = body.data();
    zs.avail_out = (uInt)body.size();
    deflate(&zs, Z_FINISH);
    body.resize(zs.total_out);
    deflateEnd(&zs);
    std::vector<uint8_t> m{0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    const size_t size = 18 + body.size() + 8;
    m.push_back((uint8_t)((size - 1) & 0xff));
    m.push_back((uint8_t)((size - 1) >> 8));
    m.insert(m.end(), body.begin(), body.end());
    bgzfx::put_u32(m, (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)text.data(), (uInt)text.size()));
    bgzfx::put_u32(m, (uint32_t)text.size());
    return m;
}

int main()
{
    std::mt19937_64 rng(20261021);
    {   // ---- region_grammar
        Region r;
        CHECK(parse_region("chr6", &r).empty() && r.name == "chr6" && r.beg1 == 1 && r.end1 == -1);
        CHECK(parse_region("chr6:28,510,120-33,480,577", &r).empty() && r.name == "chr6" && r.beg1 == 28510120 && r.end1 == 33480577);
        CHECK(parse_region("chr6:100", &r).empty() && r.beg1 == 100 && r.end1 == -1);
        CHECK(parse_region("chr6:100-", &r).empty() && r.beg1 == 100 && r.end1 == -1);
        CHECK(parse_region("c:7-7", &r).empty() && r.beg1 == 7 && r.end1 == 7);
        CHECK(parse_region("HLA-A*01:01", &r).empty() && r.name == "HLA-A*01" && r.beg1 == 1);      // (phi_region_open tries the whole string as a name too)
        CHECK(parse_region("HLA-A*01:01:5-9", &r).empty() && r.name == "HLA-A*01:01" && r.beg1 == 5 && r.end1 == 9);
        CHECK(parse_region("a:b", &r).empty() && r.name == "a:b");
        for (const char *bad : {"", "chr1:", ":5-10", "chr1:10-5", "chr1:0-5", "chr1:0", "chr1:1-2-3", "chr1:-5", "chr1:1234567890123456789", "chr1:,", "chr1:5-,"})
            CHECK(!parse_region(bad, &r).empty());
        int64_t b, e;
        CHECK(parse_region("c:11-20", &r).empty() && resolve_region(r, 100, &b, &e).empty() && b == 10 && e == 20);
        CHECK(parse_region("c:11", &r).empty() && resolve_region(r, 100, &b, &e).empty() && b == 10 && e == 100);
        CHECK(parse_region("c:11-500", &r).empty() && resolve_region(r, 100, &b, &e).empty() && b == 10 && e == 100);
        CHECK(parse_region("c", &r).empty() && resolve_region(r, 100, &b, &e).empty() && b == 0 && e == 100);
        CHECK(parse_region("c:100", &r).empty() && resolve_region(r, 100, &b, &e).empty() && b == 99 && e == 100);
        CHECK(parse_region("c:101", &r).empty() && !resolve_region(r, 100, &b, &e).empty());
        CHECK(parse_region("c", &r).empty() && !resolve_region(r, 0, &b, &e).empty());
        printf("ok region_grammar\n");
    }
    std::vector<std::vector<Rec>> recs{make_records(rng, 4000), make_records(rng, 900), make_records(rng, 1)};
    std::vector<bgzfx::TbiContig> ctg{contig_of("chr1", recs[0]), contig_of("chr10", recs[1]), contig_of("x", recs[2])};
    const std::vector<bgzfx::TbiContig> ctg_in = ctg;
    const std::vector<uint8_t> bytes = bgzfx::tbi_bytes(ctg, nullptr);
    Tbi t;
    {   // ---- tbi_parse
        const std::string why = parse_tbi(bytes.data(), bytes.size(), &t);
        CHECK(why.empty() && t.contigs.size() == 3 && t.has_no_coor && t.n_no_coor == 0);
        for (size_t c = 0; c < t.contigs.size() && c < 3; c++) {
            CHECK(t.contigs[c].name == ctg[c].name && t.contigs[c].lin == ctg[c].lin);
            size_t chunks = 0;
            for (size_t k = 0; k < t.contigs[c].bins.size(); k++) {
                if (k) CHECK(t.contigs[c].bins[k].bin > t.contigs[c].bins[k - 1].bin);
                chunks += t.contigs[c].bins[k].chunks.size();
            }
            CHECK(chunks == ctg_in[c].chunks.size());
        }
        std::vector<uint8_t> other = bytes;
        memcpy(other.data(), "CSI\1", 4);
        Tbi u;
        CHECK(parse_tbi(other.data(), other.size(), &u).find("CSI") != std::string::npos);
        for (const int at : {8, 12, 16, 24}) {                  // format, col_seq, col_beg, meta
            other = bytes;
            other[(size_t)at] ^= 1;
            CHECK(parse_tbi(other.data(), other.size(), &u).find("preset") != std::string::npos);
        }
        other = bytes;
        other.push_back(0);
        CHECK(!parse_tbi(other.data(), other.size(), &u).empty());
        printf("ok tbi_parse\n");
    }
    check_selection(t, recs, rng);
    printf("ok chunk_selection\n");
    {   // ---- htslib_style
        for (const int no_coor : {7, -1}) {
            const std::vector<uint8_t> hb = htslib_bytes(t, no_coor);
            Tbi h;
            CHECK(parse_tbi(hb.data(), hb.size(), &h).empty() && h.has_no_coor == (no_coor >= 0) && h.n_no_coor == (uint64_t)std::max(no_coor, 0));
            size_t a = 0, b = 0;
            for (const TbiContig &c : t.contigs) for (const TbiBin &k : c.bins) a += k.chunks.size();
            for (const TbiContig &c : h.contigs) for (const TbiBin &k : c.bins) b += k.chunks.size();
            CHECK(b < a + 2 * h.contigs.size() && h.contigs[0].bins.back().bin == (uint32_t)PSEUDO_BIN);
            check_selection(h, recs, rng);
        }
        printf("ok htslib_style\n");
    }
    {   // ---- tbi_truncated: a heap buffer of exactly the cut's length, so that a read beyond it is seen
        const std::vector<uint8_t> small = [&] { std::vector<bgzfx::TbiContig> c{contig_of("chr1", make_records(rng, 60)), contig_of("b", make_records(rng, 3))}; return bgzfx::tbi_bytes(c, nullptr); }();
        Tbi u;
        CHECK(parse_tbi(small.data(), small.size(), &u).empty());
        for (size_t cut = 0; cut < small.size(); cut++) {
            uint8_t *p = (uint8_t *)malloc(cut ? cut : 1);
            if (cut) memcpy(p, small.data(), cut);
            const std::string why = parse_tbi(p, cut, &u);
            CHECK(why.empty() == (cut == small.size() - 8));
            free(p);
        }
        printf("ok tbi_truncated\n");
    }
    {   // ---- fai_arithmetic
        const FaiRecord r{"s", 125, 7, 60, 61};
        CHECK(fai_offset(r, 0) == 7 && fai_offset(r, 59) == 66 && fai_offset(r, 60) == 68 && fai_offset(r, 119) == 127 && fai_offset(r, 120) == 129 && fai_offset(r, 124) == 133);
        int64_t u0, u1;
        fai_range(r, 59, 61, &u0, &u1);
        CHECK(u0 == 66 && u1 == 69);
        fai_range(r, 120, 125, &u0, &u1);
        CHECK(u0 == 129 && u1 == 134);
        std::string seq, file = ">skip\nACGT\n>s d\n";
        for (int i = 0; i < 125; i++) seq.push_back("acgtN"[rng() % 5]);
        const int64_t off = (int64_t)file.size();
        for (size_t i = 0; i < seq.size(); i += 60) file += seq.substr(i, 60) + "\n";
        const std::string fai = "skip\t4\t6\t4\t5\ns\t125\t" + std::to_string(off) + "\t60\t61\n";
        std::vector<FaiRecord> fr;
        CHECK(parse_fai(fai.data(), fai.size(), &fr).empty() && fr.size() == 2 && fr[1].name == "s" && fr[1].len == 125 && fr[1].offset == off);
        CHECK(!parse_fai("s\t1\t2\t3\n", 8, &fr).empty() && !parse_fai("s\t1\t2\t0\t1\n", 10, &fr).empty() && !parse_fai("s\t1\tx\t3\t4\n", 10, &fr).empty());
        char path[] = "/tmp/region_selftest_XXXXXX";
        const int fd = mkstemp(path);
        CHECK(fd >= 0 && write(fd, file.data(), file.size()) == (ssize_t)file.size());
        ::close(fd);
        std::string up = seq;
        for (char &c : up) if (c >= 'a' && c <= 'z') c = (char)(c - 32);
        const FaiRecord s{"s", 125, off, 60, 61};
        for (int64_t b = 0; b <= 125; b++)
            for (int64_t e = b; e <= 125; e += 1 + (e - b) / 7) {
                std::vector<char> out;
                CHECK(fasta_slice(path, s, b, e, &out).empty() && std::string(out.begin(), out.end()) == up.substr((size_t)b, (size_t)(e - b)));
            }
        std::vector<char> out;
        CHECK(!fasta_slice(path, s, 0, 126, &out).empty());
        const FaiRecord lie{"s", 500, off, 60, 61};
        CHECK(!fasta_slice(path, lie, 100, 400, &out).empty());
        unlink(path);
        printf("ok fai_arithmetic\n");
    }
    {   // ---- member_plan: five members of 50 lines of 20 bytes
        std::vector<std::string> texts;
        std::vector<uint8_t> file;
        std::vector<int64_t> at;
        for (int m = 0; m < 5; m++) {
            std::string s;
            for (int i = 0; i < 50; i++) { char ln[32]; snprintf(ln, sizeof ln, "member%d line %06d\n", m, i); s += ln; }
            texts.push_back(s);
            at.push_back((int64_t)file.size());
            const std::vector<uint8_t> mb = bgzf_member(s);
            file.insert(file.end(), mb.begin(), mb.end());
        }
        at.push_back((int64_t)file.size());
        const std::vector<uint8_t> eof = bgzf_member("");
        file.insert(file.end(), eof.begin(), eof.end());
        char path[] = "/tmp/region_selftest_XXXXXX";
        const int fd = mkstemp(path);
        CHECK(fd >= 0 && write(fd, file.data(), file.size()) == (ssize_t)file.size());
        ::close(fd);
        Fd f;
        CHECK(f.open(path) && is_gzip(f));
        auto v = [&](int m, int u) { return (uint64_t)at[(size_t)m] << 16 | (uint64_t)u; };
        // inside member 0; from member 1 into member 2 and on from there; member 4 to the EOF block's first byte
        const std::vector<Chunk> chunks{{v(0, 40), v(0, 400)}, {v(1, 980), v(2, 20)}, {v(2, 600), v(2, 1000)}, {v(4, 0), v(5, 0)}};
        Plan p;
        const std::string why = plan_members(f, chunks, &p);
        if (!why.empty()) printf("plan_members: %s\n", why.c_str());
        CHECK(why.empty());
        CHECK(p.members.size() == 4 && p.members[0].at == at[0] && p.members[1].at == at[1] && p.members[2].at == at[2] && p.members[3].at == at[4]);
        CHECK((p.text_off == std::vector<int64_t>{0, 1000, 2000, 3000, 4000}));
        CHECK((p.range == std::vector<int64_t>{40, 400, 1980, 2020, 2600, 3000, 3000, 4000}));
        std::vector<char> all;
        const Bytes mem{(const uint8_t *)p.gz.data(), (int64_t)p.gz.size()};
        int64_t o = 0;
        for (size_t k = 0; k < p.members.size(); k++) {
            Member m;
            CHECK(member_at(mem, o, &m) && m.size == p.members[k].size && m.isize == 1000);
            o += p.members[k].size;
        }
        CHECK(o == (int64_t)p.gz.size());
        for (const Member &m : p.members) CHECK(inflate_member(f, m, all));
        CHECK(std::string(all.begin(), all.end()) == texts[0] + texts[1] + texts[2] + texts[4]);
        Plan q;
        CHECK(!plan_members(f, {{v(0, 0), (uint64_t)(at[1] + 3) << 16 | 5}}, &q).empty());        // an end that is no member's first byte
        CHECK(!plan_members(f, {{v(0, 2000), v(1, 0)}}, &q).empty());                             // begins behind its member's text
        CHECK(!plan_members(f, {{(uint64_t)(file.size() + 10) << 16, (uint64_t)(file.size() + 20) << 16 | 1}}, &q).empty());
        CHECK(plan_members(f, {}, &q).empty() && q.members.empty() && q.range.empty() && q.gz.empty());
        std::vector<char> hdr;
        CHECK(header_text(f, &hdr).empty() && hdr.empty());                                      // the first line is a record: no header
        unlink(path);
        printf("ok member_plan\n");
    }
    if (failures) { printf("%d check(s) failed\n", failures); return 1; }
    return 0;
}
