// vcf_reader.cpp -- a phased multi-sample VCF + a reference FASTA -> the graph of phi_amd/vcf2gfa.py, without the GFA in between
// (the reference's second input route: vcf2gfa.py:27-64 `vg construct | vg gbwt | gfa2gbwt -m 30`, README "VCF + FASTA").
//
//   phi_vcf_read       the FASTA record (upper-cased) and the VCF's FIXED columns: record selection (one contig, REF checked
//                      against the FASTA, GT in FORMAT, sequence ALTs only, inside the contig), the stable sort by (start, end),
//                      the sites (maximal runs of records that overlap or touch); the SAMPLE columns of the kept records are
//                      not parsed, they are laid out back to back -- each slice followed by one line feed, so that a slice's
//                      end is found in the text itself -- for one upload (include/phi_amd.h phi_vcf_genotypes)
//   phi_vcf_parse_gt   the exact scalar statement of the field rules (vcf2gfa.py read_vcf): what the device kernel computes,
//                      and its fallback for the records it flags
//   phi_vcf_build      genotype matrix -> per site the strings the haplotypes spell and their distinct alleles -> units
//                      (backbone, alleles, backbone, ...), segments of at most max_len bases, adjacency, Kahn order
//                      (gfa_reader.cpp's routine: ILP_index.cpp:115-154), hap names; and for the device the unit tables and
//                      choice[site][kept haplotype] from which phi_vcf_walks (phi_amd.h) writes the walk entries
// The middle stage is O(sites x haplotypes) over two small integers per cell and compares a handful of short strings per
// site exactly: it stays on the host, threaded over sites (at most 16 threads).
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include "gz_source.h"
#include <algorithm>
#include <atomic>
#include <numeric>
#include <string>
#include <thread>
#include <vector>
#include "../../../include/phi_host.h"
#include "phi_graph.h"

namespace {

int vfail(char *err, int cap, int code, const char *fmt, ...)
{
    if (err && cap > 0) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, (size_t)cap, fmt, ap);
        va_end(ap);
    }
    return code;
}

int vcf_threads()
{
    int nt = (int)std::thread::hardware_concurrency();
    if (const char *e = getenv("PHI_HOST_THREADS")) nt = atoi(e);
    return std::max(1, std::min(nt, 16));
}

// fn(lo, hi) over [0, n) in chunks handed out dynamically, on at most 16 threads
template <class F> void vcf_parallel(int64_t n, int64_t chunk, F fn)
{
    const int64_t n_chunks = (n + chunk - 1) / chunk;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(vcf_threads(), n_chunks));
    std::atomic<int64_t> next{0};
    auto work = [&]() { for (int64_t i; (i = next.fetch_add(1)) < n_chunks;) fn(i * chunk, std::min(n, (i + 1) * chunk)); };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}

// the bytes of a file, plain or gzip / BGZF (gz_source.h): 0 ok, -1 cannot open / read, -2 gzip stream corrupt
int load_file(const char *path, std::vector<char> &out)
{
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return -1;
    unsigned char magic[2] = {0, 0};
    const ssize_t got = pread(fd, magic, 2, 0);
    if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
        ::close(fd);
        GzSource gz;
        if (!gz.open(path, vcf_threads())) return -1;
        std::vector<char> blk;
        while (gz.next(blk)) {
            if (out.capacity() < out.size() + blk.size()) out.reserve(std::max(out.capacity() * 2, out.size() + blk.size()));
            out.insert(out.end(), blk.begin(), blk.end());
        }
        const bool ok = gz.ok();
        gz.close();
        return ok ? 0 : -2;
    }
    struct stat st;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) out.reserve((size_t)st.st_size);
    char tmp[1 << 16];
    ssize_t r;
    while ((r = read(fd, tmp, sizeof tmp)) > 0) out.insert(out.end(), tmp, tmp + r);
    ::close(fd);
    return r < 0 ? -1 : 0;
}

inline bool py_space(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); }      // bytes.strip() / bytes.split()
inline char up(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }

struct Sl { const char *p; size_t n; };

}  // namespace

struct phi_vcf {
    std::string contig, ref_name;
    std::vector<char> ref;                             // the FASTA record, upper-cased
    std::vector<std::string> samples;
    int64_t n_other = 0, n_mismatch = 0;
    int64_t origin = 0, n_outside = 0;                 // a region read: where ref begins on the contig; records that reach beyond ref
    // kept records, sorted by (start, end) (stable)
    std::vector<int64_t> start, end;
    std::vector<int32_t> gi;                           // index of GT in FORMAT
    std::vector<int64_t> alt_off;                      // [n_rec + 1] into alt_pos
    std::vector<int64_t> alt_pos;                      // [n_alts + 1] into alt_bytes
    std::vector<char> alt_bytes;                       // the ALT strings, upper-cased
    std::vector<char> text;                            // the sample columns, every slice followed by '\n'
    std::vector<int64_t> text_off;                     // [n_rec + 1]
    std::vector<int64_t> site_off;                     // [n_sites + 1] records of every site
    // phi_vcf_build
    bool built = false;
    std::vector<int32_t> unit_first;                   // [n_units + 1]
    std::vector<int32_t> site_backbone, site_allele0;  // per real site: its backbone unit, its first allele unit
    std::vector<int32_t> choice;                       // [n_real][n_keep]
    std::vector<int32_t> keep;                         // kept haplotypes (0 = reference, 1 + 2 * sample + column)
};

namespace {

// Python's int() on the POS column, as far as a VCF can hold one: optional blanks and sign, decimal digits
bool parse_pos(Sl s, int64_t *out)
{
    size_t i = 0, e = s.n;
    while (i < e && py_space((unsigned char)s.p[i])) i++;
    while (e > i && py_space((unsigned char)s.p[e - 1])) e--;
    bool neg = false;
    if (i < e && (s.p[i] == '+' || s.p[i] == '-')) neg = s.p[i++] == '-';
    if (i >= e) return false;
    int64_t v = 0;
    for (; i < e; i++) {
        if (s.p[i] < '0' || s.p[i] > '9') return false;
        if (v > (INT64_MAX - 9) / 10) return false;
        v = v * 10 + (s.p[i] - '0');
    }
    *out = neg ? -v : v;
    return true;
}

int read_fasta_single(const char *path, phi_vcf *v, char *err, int cap)
{
    std::vector<char> raw;
    const int rc = load_file(path, raw);
    if (rc) return vfail(err, cap, PHI_HOST_ERR_IO, rc == -2 ? "%s: corrupt gzip stream" : "cannot open or read %s", path);
    bool have = false;
    v->ref.reserve(raw.size());
    const char *p = raw.data(), *e = p + raw.size();
    while (p < e) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
        const char *le = nl ? nl : e;
        if (*p == '>') {
            if (have) return vfail(err, cap, PHI_HOST_ERR_INVALID, "the reference FASTA holds more than one record; vcf2gfa handles one contig");
            have = true;
            const char *a = p + 1;
            while (a < le && py_space((unsigned char)*a)) a++;
            const char *b = a;
            while (b < le && !py_space((unsigned char)*b)) b++;
            v->ref_name.assign(a, b);
        } else {
            const char *a = p, *b = le;
            while (a < b && py_space((unsigned char)*a)) a++;
            while (b > a && py_space((unsigned char)b[-1])) b--;
            for (; a < b; a++) v->ref.push_back(up(*a));
        }
        p = nl ? nl + 1 : e;
    }
    if (!have) return vfail(err, cap, PHI_HOST_ERR_INVALID, "no FASTA record in the reference file");
    return PHI_HOST_OK;
}

struct RawRec { int64_t start, end; int32_t gi; Sl alt; Sl cols; };

// The rule pass over VCF text in memory: v->ref is the reference (a whole record, or its bases from `origin` on), a record's
// position is POS - 1 - origin, `only` (may be null) the one contig to read -- without it the first contig seen.  vcf_path
// stands in the messages.
int vcf_rules(phi_vcf *v, const char *text, size_t n_text, int64_t origin, const char *only, const char *vcf_path, char *err, int err_cap)
{
    const int64_t ref_len = (int64_t)v->ref.size();
    v->origin = origin;
    std::vector<RawRec> recs;
    bool have_contig = only != nullptr;
    Sl contig{only, only ? strlen(only) : 0};
    const char *p = text, *e = p + n_text;
    int64_t line_no = 0;
    while (p < e) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
        const char *le = nl ? nl : e;
        const char *next = nl ? nl + 1 : e;
        line_no++;
        const size_t ln = (size_t)(le - p);
        if (ln >= 2 && p[0] == '#' && p[1] == '#') { p = next; continue; }
        while (le > p && (le[-1] == '\r' || le[-1] == '\n')) le--;                    // rstrip(b"\r\n")
        // the first nine tabs
        Sl col[9];
        int nc = 0;
        const char *a = p;
        const char *rest = nullptr;
        while (nc < 9) {
            const char *t = (const char *)memchr(a, '\t', (size_t)(le - a));
            if (!t) break;
            col[nc++] = Sl{a, (size_t)(t - a)};
            a = t + 1;
        }
        if (nc == 9) rest = a;
        if (ln >= 6 && memcmp(p, "#CHROM", 6) == 0) {
            if (!recs.empty() && rest)
                return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "%s line %lld: the #CHROM header stands behind data lines", vcf_path, (long long)line_no);
            v->samples.clear();
            for (const char *s = rest; s;) {
                const char *t = (const char *)memchr(s, '\t', (size_t)(le - s));
                v->samples.emplace_back(s, t ? t : le);
                s = t ? t + 1 : nullptr;
            }
            p = next;
            continue;
        }
        if (!rest) { p = next; continue; }                                            // fewer than 10 columns
        if (!have_contig) { have_contig = true; contig = col[0]; }
        if (col[0].n != contig.n || memcmp(col[0].p, contig.p, contig.n) != 0) { v->n_other++; p = next; continue; }
        int64_t pos1 = 0;
        if (!parse_pos(col[1], &pos1))
            return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "%s line %lld: POS is no integer", vcf_path, (long long)line_no);
        const int64_t pos = pos1 - 1 - origin;
        // GT in FORMAT
        int32_t gi = -1, fi = 0;
        for (const char *s = col[8].p, *fe = s + col[8].n;; fi++) {
            const char *t = (const char *)memchr(s, ':', (size_t)(fe - s));
            const char *pe = t ? t : fe;
            if (gi < 0 && pe - s == 2 && s[0] == 'G' && s[1] == 'T') gi = fi;
            if (!t) break;
            s = t + 1;
        }
        const int64_t rl = (int64_t)col[3].n;
        if (gi >= 0 && (pos < 0 || pos + rl > ref_len)) v->n_outside++;
        if (gi < 0 || pos < 0 || pos + rl > ref_len) { p = next; continue; }
        bool same = true;
        for (int64_t i = 0; i < rl && same; i++) same = up(col[3].p[i]) == v->ref[(size_t)(pos + i)];
        if (!same) { v->n_mismatch++; p = next; continue; }
        bool ok = true;
        for (const char *s = col[4].p, *ae = s + col[4].n; ok;) {
            const char *t = (const char *)memchr(s, ',', (size_t)(ae - s));
            const char *pe = t ? t : ae;
            if (pe == s || *s == '<' || (pe - s == 1 && *s == '*') || memchr(s, '[', (size_t)(pe - s)) || memchr(s, ']', (size_t)(pe - s))) ok = false;
            if (!t) break;
            s = t + 1;
        }
        if (!ok) { p = next; continue; }
        recs.push_back(RawRec{pos, pos + rl, gi, col[4], Sl{rest, (size_t)(le - rest)}});
        p = next;
    }
    if (have_contig) v->contig.assign(contig.p, contig.n);
    // stable sort by (start, end)
    std::vector<int64_t> order(recs.size());
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        const RawRec &a = recs[(size_t)x], &b = recs[(size_t)y];
        return a.start != b.start ? a.start < b.start : a.end < b.end;
    });
    const size_t n = recs.size();
    v->start.resize(n); v->end.resize(n); v->gi.resize(n);
    v->alt_off.assign(n + 1, 0); v->text_off.assign(n + 1, 0);
    v->alt_pos.assign(1, 0);
    size_t text_bytes = 0;
    for (const RawRec &r : recs) text_bytes += r.cols.n + 1;
    v->text.resize(text_bytes);
    for (size_t i = 0; i < n; i++) {
        const RawRec &r = recs[(size_t)order[i]];
        v->start[i] = r.start; v->end[i] = r.end; v->gi[i] = r.gi;
        for (const char *s = r.alt.p, *ae = s + r.alt.n;;) {
            const char *t = (const char *)memchr(s, ',', (size_t)(ae - s));
            const char *pe = t ? t : ae;
            for (const char *q = s; q < pe; q++) v->alt_bytes.push_back(up(*q));
            v->alt_pos.push_back((int64_t)v->alt_bytes.size());
            if (!t) break;
            s = t + 1;
        }
        v->alt_off[i + 1] = (int64_t)v->alt_pos.size() - 1;
        // (65 535 stands for "an allele index of 65 535 or more" in the genotype matrix: every real index must lie below)
        if (v->alt_off[i + 1] - v->alt_off[i] >= 65535) return vfail(err, err_cap, PHI_HOST_ERR_UNSUPPORTED, "a record with 65 535 or more ALT alleles");
        char *dst = v->text.data() + v->text_off[i];
        if (r.cols.n) memcpy(dst, r.cols.p, r.cols.n);
        dst[r.cols.n] = '\n';
        v->text_off[i + 1] = v->text_off[i] + (int64_t)r.cols.n + 1;
    }
    // sites: maximal runs of records that overlap or touch
    v->site_off.clear();
    int64_t cur_end = 0;
    for (size_t i = 0; i < n; i++) {
        if (!v->site_off.empty() && v->start[i] <= cur_end) cur_end = std::max(cur_end, v->end[i]);
        else { v->site_off.push_back((int64_t)i); cur_end = v->end[i]; }
    }
    v->site_off.push_back((int64_t)n);
    if (n == 0) v->site_off.assign(1, 0);
    return PHI_HOST_OK;
}

}  // namespace

extern "C" {

int phi_vcf_read(const char *vcf_path, const char *fasta_path, phi_vcf **out, char *err, int err_cap)
{
    if (!vcf_path || !fasta_path || !out) return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "null argument");
    *out = nullptr;
    phi_vcf *v = new phi_vcf;
    struct Guard { phi_vcf *&v; ~Guard() { delete v; } } guard{v};
    int rc = read_fasta_single(fasta_path, v, err, err_cap);
    if (rc) return rc;
    std::vector<char> raw;
    rc = load_file(vcf_path, raw);
    if (rc) return vfail(err, err_cap, PHI_HOST_ERR_IO, rc == -2 ? "%s: corrupt gzip stream" : "cannot open or read %s", vcf_path);
    if ((rc = vcf_rules(v, raw.data(), raw.size(), 0, nullptr, vcf_path, err, err_cap))) return rc;
    *out = v;
    v = nullptr;
    return PHI_HOST_OK;
}

int phi_vcf_read_text(const char *text, int64_t n_text, const char *ref, int64_t ref_len, const char *ref_name, int64_t origin, const char *contig,
                      phi_vcf **out, char *err, int err_cap)
{
    if (!out || n_text < 0 || ref_len < 0 || (n_text > 0 && !text) || (ref_len > 0 && !ref)) return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "null argument or negative size");
    *out = nullptr;
    phi_vcf *v = new phi_vcf;
    struct Guard { phi_vcf *&v; ~Guard() { delete v; } } guard{v};
    v->ref.resize((size_t)ref_len);
    for (int64_t i = 0; i < ref_len; i++) v->ref[(size_t)i] = up(ref[i]);
    if (ref_name) v->ref_name = ref_name;
    const int rc = vcf_rules(v, text, (size_t)n_text, origin, contig, "the VCF text", err, err_cap);
    if (rc) return rc;
    *out = v;
    v = nullptr;
    return PHI_HOST_OK;
}

void phi_vcf_free(phi_vcf *v) { delete v; }
int32_t phi_vcf_n_samples(const phi_vcf *v) { return (int32_t)v->samples.size(); }
const char *phi_vcf_sample_name(const phi_vcf *v, int32_t s) { return (s >= 0 && s < (int32_t)v->samples.size()) ? v->samples[(size_t)s].c_str() : ""; }
const char *phi_vcf_contig(const phi_vcf *v) { return v->contig.c_str(); }
int64_t phi_vcf_n_records(const phi_vcf *v) { return (int64_t)v->start.size(); }
int64_t phi_vcf_n_sites(const phi_vcf *v) { return (int64_t)v->site_off.size() - 1; }
int64_t phi_vcf_n_other_contig(const phi_vcf *v) { return v->n_other; }
int64_t phi_vcf_n_ref_mismatch(const phi_vcf *v) { return v->n_mismatch; }
int64_t phi_vcf_origin(const phi_vcf *v) { return v->origin; }
int64_t phi_vcf_n_outside(const phi_vcf *v) { return v->n_outside; }
int64_t phi_vcf_ref_len(const phi_vcf *v) { return (int64_t)v->ref.size(); }
const char *phi_vcf_ref_seq(const phi_vcf *v) { return v->ref.data(); }
const int64_t *phi_vcf_rec_start(const phi_vcf *v) { return v->start.data(); }
const int64_t *phi_vcf_rec_end(const phi_vcf *v) { return v->end.data(); }
const int32_t *phi_vcf_rec_gt_index(const phi_vcf *v) { return v->gi.data(); }
const int64_t *phi_vcf_rec_alt_off(const phi_vcf *v) { return v->alt_off.data(); }
const int64_t *phi_vcf_alt_pos(const phi_vcf *v) { return v->alt_pos.data(); }
const char *phi_vcf_alt_bytes(const phi_vcf *v) { return v->alt_bytes.data(); }
const int64_t *phi_vcf_site_off(const phi_vcf *v) { return v->site_off.data(); }
const char *phi_vcf_text(const phi_vcf *v) { return v->text.data(); }
const int64_t *phi_vcf_text_off(const phi_vcf *v) { return v->text_off.data(); }

/* vcf2gfa.py read_vcf, the sample columns: record r's slice is text[text_off[r], text_off[r + 1] - 1) (a line feed follows it);
 * sample s's field starts after the slice's s-th tab; its GT part is the gt_index[r]-th ':'-separated part; '/' reads as '|';
 * the first two '|'-separated parts give gt[(r * n_samples + s) * 2 + {0, 1}]: a non-empty run of ASCII digits is its value
 * (65 535 for that and more), anything else 0; ploidy[s] = max(ploidy[s], min(2, parts other than ".")).  Rows [rec_lo, rec_hi).
 * PHI_HOST_ERR_INVALID where the Python raises: fewer fields than samples, fewer ':' parts than gt_index + 1. */
int phi_vcf_parse_gt(const char *text, const int64_t *text_off, const int32_t *gt_index, int64_t rec_lo, int64_t rec_hi, int32_t n_samples,
                     uint16_t *gt, int32_t *ploidy, char *err, int err_cap)
{
    if (rec_hi > rec_lo && (!text || !text_off || !gt_index || (n_samples > 0 && (!gt || !ploidy)))) return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "null argument");
    for (int64_t r = rec_lo; r < rec_hi; r++) {
        const char *p = text + text_off[r], *e = text + text_off[r + 1] - 1;
        const int32_t gi = gt_index[r];
        for (int32_t s = 0; s < n_samples; s++) {
            if (!p) return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "kept record %lld has %d sample columns, the header names %d", (long long)r, s, n_samples);
            const char *t = (const char *)memchr(p, '\t', (size_t)(e - p));
            const char *fe = t ? t : e;
            const char *g = p;
            for (int32_t k = 0; k < gi; k++) {
                const char *c = (const char *)memchr(g, ':', (size_t)(fe - g));
                if (!c) return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "kept record %lld, sample %d: the field has %d ':' parts, GT is part %d", (long long)r, s, k + 1, gi + 1);
                g = c + 1;
            }
            const char *ge = (const char *)memchr(g, ':', (size_t)(fe - g));
            if (!ge) ge = fe;
            uint16_t a[2] = {0, 0};
            int32_t part = 0, n_called = 0;
            for (const char *q = g;; part++) {
                const char *pe = q;
                while (pe < ge && *pe != '|' && *pe != '/') pe++;
                if (!(pe - q == 1 && *q == '.')) n_called++;
                if (part < 2 && pe > q) {
                    uint32_t val = 0;
                    bool digits = true;
                    for (const char *d = q; d < pe && digits; d++) {
                        if (*d < '0' || *d > '9') digits = false;
                        else val = std::min<uint32_t>(65535u, val * 10 + (uint32_t)(*d - '0'));
                    }
                    a[part] = digits ? (uint16_t)val : 0;
                }
                if (pe >= ge) break;
                q = pe + 1;
            }
            uint16_t *o = gt + ((size_t)r * (size_t)n_samples + (size_t)s) * 2;
            o[0] = a[0]; o[1] = a[1];
            ploidy[s] = std::max(ploidy[s], std::min(2, n_called));
            p = t ? t + 1 : nullptr;
        }
    }
    return PHI_HOST_OK;
}

/* vcf2gfa.py build + write_gfa as phi_gfa_read_deferred would return the file: the graph with its walks left to the caller
 * (walk_off / walk_vtx empty: phi_vcf_walks of phi_amd.h writes the entries on the device from the tables below). */
int phi_vcf_build(phi_vcf *v, const uint16_t *gt, const int32_t *ploidy, int32_t max_len, phi_graph **out, char *err, int err_cap)
{
    if (!v || !out) return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "null argument");
    *out = nullptr;
    const int32_t n_s = (int32_t)v->samples.size();
    const int64_t n_rec = (int64_t)v->start.size(), n_sites = (int64_t)v->site_off.size() - 1;
    if (max_len < 1) return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "max_len %d (a segment holds at least one base)", max_len);
    if (n_s > 0 && n_rec > 0 && !gt) return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "null genotype matrix");
    if (n_s > 0 && !ploidy) return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "null ploidy");
    if (n_s > (INT32_MAX - 1) / 2) return vfail(err, err_cap, PHI_HOST_ERR_UNSUPPORTED, "too many samples");
    v->built = false;
    const int32_t n_hap = 1 + 2 * n_s;
    const char *ref = v->ref.data();
    const int64_t ref_len = (int64_t)v->ref.size();
    // ---- per site: the distinct strings the haplotypes spell (reference first, then ascending), and every haplotype's allele
    struct SiteOut { std::vector<std::string> alleles; std::vector<int32_t> of_hap; };      // alleles empty: nobody differs
    std::vector<SiteOut> so((size_t)n_sites);
    vcf_parallel(n_sites, 64, [&](int64_t lo, int64_t hi) {
        std::vector<std::pair<std::string, int32_t>> sp;
        std::string seq;
        for (int64_t si = lo; si < hi; si++) {
            const int64_t r0 = v->site_off[(size_t)si], r1 = v->site_off[(size_t)si + 1];
            const int64_t s = v->start[(size_t)r0];
            int64_t e = v->end[(size_t)r0];
            for (int64_t r = r0; r < r1; r++) e = std::max(e, v->end[(size_t)r]);
            sp.clear();
            for (int32_t h = 1; h < n_hap; h++) {
                const int32_t smp = (h - 1) / 2, col = (h - 1) % 2;
                int64_t at = s;
                bool any = false;
                for (int64_t r = r0; r < r1; r++) {
                    const int64_t a = gt[((size_t)r * (size_t)n_s + (size_t)smp) * 2 + (size_t)col];
                    const int64_t n_alt = v->alt_off[(size_t)r + 1] - v->alt_off[(size_t)r];
                    if (a <= 0 || a > n_alt || v->start[(size_t)r] < at) continue;      // reference allele, or in conflict with a record already applied
                    if (!any) { any = true; seq.clear(); }
                    seq.append(ref + at, (size_t)(v->start[(size_t)r] - at));
                    const int64_t ai = v->alt_off[(size_t)r] + a - 1;
                    seq.append(v->alt_bytes.data() + v->alt_pos[(size_t)ai], (size_t)(v->alt_pos[(size_t)ai + 1] - v->alt_pos[(size_t)ai]));
                    at = v->end[(size_t)r];
                }
                if (!any) continue;
                seq.append(ref + at, (size_t)(e - at));
                if (seq.size() == (size_t)(e - s) && memcmp(seq.data(), ref + s, seq.size()) == 0) continue;      // spells the reference after all
                sp.emplace_back(seq, h);
            }
            if (sp.empty()) continue;
            SiteOut &o = so[(size_t)si];
            std::sort(sp.begin(), sp.end(), [](const std::pair<std::string, int32_t> &x, const std::pair<std::string, int32_t> &y) {
                const size_t m = std::min(x.first.size(), y.first.size());
                const int c = m ? memcmp(x.first.data(), y.first.data(), m) : 0;
                if (c) return c < 0;
                if (x.first.size() != y.first.size()) return x.first.size() < y.first.size();
                return x.second < y.second;
            });
            o.of_hap.assign((size_t)n_hap, 0);
            o.alleles.emplace_back(ref + s, (size_t)(e - s));
            for (size_t i = 0; i < sp.size(); i++) {
                if (i == 0 || sp[i].first != sp[i - 1].first) o.alleles.push_back(sp[i].first);
                o.of_hap[(size_t)sp[i].second] = (int32_t)o.alleles.size() - 1;
            }
        }
    });
    // ---- kept haplotypes and their names
    v->keep.assign(1, 0);
    phi_graph *g = new phi_graph;
    struct GGuard { phi_graph *&g; ~GGuard() { delete g; } } gguard{g};
    g->hap_names.push_back("REF.0");
    for (int32_t s = 0; s < n_s; s++)
        for (int32_t col = 0; col < 2; col++)
            if (col < std::max(1, ploidy[s])) {
                v->keep.push_back(1 + 2 * s + col);
                g->hap_names.push_back(v->samples[(size_t)s] + "." + std::to_string(col + 1));
            }
    const size_t n_keep = v->keep.size();
    // ---- units: backbone, alleles, backbone, alleles, ..., backbone; segments of at most max_len bases, ids in that order
    struct Unit { const char *p; int64_t n; };
    std::vector<Unit> units;
    v->site_backbone.clear(); v->site_allele0.clear(); v->choice.clear();
    std::vector<int64_t> real;                          // the sites somebody differs at
    int64_t pos = 0;
    for (int64_t si = 0; si < n_sites; si++) {
        const SiteOut &o = so[(size_t)si];
        if (o.alleles.empty()) continue;
        const int64_t s = v->start[(size_t)v->site_off[(size_t)si]];
        if (s <= pos && pos == 0)
            return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "a variant at the first base of the contig would leave the graph without a single source vertex "
                         "(PHI's walks must start at one): trim the record or pad the reference by a base");
        if (units.size() + o.alleles.size() + 2 > (size_t)INT32_MAX) return vfail(err, err_cap, PHI_HOST_ERR_UNSUPPORTED, "more than 2^31 - 1 units");
        v->site_backbone.push_back((int32_t)units.size());
        units.push_back(Unit{ref + pos, s - pos});
        v->site_allele0.push_back((int32_t)units.size());
        for (const std::string &a : o.alleles) units.push_back(Unit{a.data(), (int64_t)a.size()});
        for (size_t k = 0; k < n_keep; k++) v->choice.push_back(o.of_hap[(size_t)v->keep[k]]);
        real.push_back(si);
        pos = pos + (s - pos) + (int64_t)o.alleles[0].size();
    }
    if (pos >= ref_len)
        return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "a variant at the last base of the contig would leave the graph without a single sink vertex: "
                     "trim the record or pad the reference by a base");
    units.push_back(Unit{ref + pos, ref_len - pos});
    const size_t n_units = units.size();
    std::vector<int64_t> first((size_t)n_units + 1, 0), base((size_t)n_units + 1, 0);
    for (size_t u = 0; u < n_units; u++) {
        if (units[u].n <= 0) return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "internal: unit %lld is empty", (long long)u);
        first[u + 1] = first[u] + (units[u].n + max_len - 1) / max_len;
        base[u + 1] = base[u] + units[u].n;
    }
    const int64_t n_seg = first[n_units];
    if (n_seg > INT32_MAX) return vfail(err, err_cap, PHI_HOST_ERR_UNSUPPORTED, "cut to %d bases the graph has %lld segments: more than 2^31 - 1", max_len, (long long)n_seg);
    v->unit_first.resize(n_units + 1);
    for (size_t u = 0; u <= n_units; u++) v->unit_first[u] = (int32_t)first[u];
    g->n_seg = (int32_t)n_seg;
    g->seq_concat = (char *)malloc((size_t)std::max<int64_t>(base[n_units], 1));
    if (!g->seq_concat) return vfail(err, err_cap, PHI_HOST_ERR_INVALID, "out of memory");
    g->seq_off.resize((size_t)n_seg + 1);
    g->adj_off.resize((size_t)n_seg + 1);
    // out-edges: inside a unit segment j -> j + 1; the last segment of a backbone -> the first segment of every allele of its
    // site (ascending); the last segment of an allele -> the first segment of the next backbone
    std::vector<int32_t> next_backbone(n_units, -1), n_alleles(n_units, 0);
    for (size_t i = 0; i < real.size(); i++) {
        const int32_t b = v->site_backbone[i], a0 = v->site_allele0[i];
        const int32_t nb = i + 1 < real.size() ? v->site_backbone[i + 1] : (int32_t)n_units - 1;
        n_alleles[(size_t)b] = nb - a0;
        for (int32_t u = a0; u < nb; u++) next_backbone[(size_t)u] = nb;
    }
    std::vector<int64_t> edge0(n_units + 1, 0);
    for (size_t u = 0; u < n_units; u++)
        edge0[u + 1] = edge0[u] + (first[u + 1] - first[u] - 1) + (n_alleles[u] ? n_alleles[u] : (next_backbone[u] >= 0 ? 1 : 0));
    g->adj.resize((size_t)edge0[n_units]);
    vcf_parallel((int64_t)n_units, 256, [&](int64_t lo, int64_t hi) {
        for (int64_t u = lo; u < hi; u++) {
            memcpy(g->seq_concat + base[(size_t)u], units[(size_t)u].p, (size_t)units[(size_t)u].n);
            const int64_t f = first[(size_t)u], np = first[(size_t)u + 1] - f;
            int64_t x = edge0[(size_t)u];
            for (int64_t j = 0; j < np; j++) {
                g->seq_off[(size_t)(f + j)] = base[(size_t)u] + j * max_len;
                g->adj_off[(size_t)(f + j)] = x;
                if (j + 1 < np) g->adj[(size_t)x++] = (int32_t)(f + j + 1);
            }
            if (n_alleles[(size_t)u]) for (int32_t a = 0; a < n_alleles[(size_t)u]; a++) g->adj[(size_t)x++] = (int32_t)first[(size_t)u + 1 + (size_t)a];
            else if (next_backbone[(size_t)u] >= 0) g->adj[(size_t)x++] = (int32_t)first[(size_t)next_backbone[(size_t)u]];
        }
    });
    g->seq_off[(size_t)n_seg] = base[n_units];
    g->adj_off[(size_t)n_seg] = edge0[n_units];
    // Kahn's algorithm, FIFO: the reader's routine (gfa_reader.cpp; ILP_index.cpp:115-154), so that the DP breaks ties alike
    {
        std::vector<int32_t> indeg((size_t)n_seg, 0), q((size_t)n_seg);
        for (int32_t t : g->adj) indeg[(size_t)t]++;
        int32_t head = 0, tail = 0;
        for (int32_t i = 0; i < n_seg; i++) if (indeg[(size_t)i] == 0) q[(size_t)tail++] = i;
        g->topo_rank.assign((size_t)n_seg, 0);
        while (head < tail) {
            const int32_t u = q[(size_t)head];
            g->topo_rank[(size_t)u] = head++;
            for (int64_t x = g->adj_off[(size_t)u]; x < g->adj_off[(size_t)u + 1]; x++)
                if (--indeg[(size_t)g->adj[(size_t)x]] == 0) q[(size_t)tail++] = g->adj[(size_t)x];
        }
        if (head != n_seg) return vfail(err, err_cap, PHI_HOST_ERR_CYCLE, "internal: the built graph is not acyclic");
    }
    // segment names 1, 2, 3, ... as write_gfa writes them
    g->name_off.resize((size_t)n_seg + 1);
    {
        char buf[16];
        for (int64_t i = 0; i < n_seg; i++) {
            g->name_off[(size_t)i] = (int64_t)g->name_arena.size();
            const int n = snprintf(buf, sizeof buf, "%lld", (long long)(i + 1));
            g->name_arena.insert(g->name_arena.end(), buf, buf + n + 1);
        }
        g->name_off[(size_t)n_seg] = (int64_t)g->name_arena.size();
    }
    v->built = true;
    *out = g;
    g = nullptr;
    return PHI_HOST_OK;
}

int64_t phi_vcf_n_units(const phi_vcf *v) { return v->built ? (int64_t)v->unit_first.size() - 1 : 0; }
const int32_t *phi_vcf_unit_first(const phi_vcf *v) { return v->unit_first.data(); }
int64_t phi_vcf_n_real_sites(const phi_vcf *v) { return v->built ? (int64_t)v->site_backbone.size() : 0; }
const int32_t *phi_vcf_site_backbone(const phi_vcf *v) { return v->site_backbone.data(); }
const int32_t *phi_vcf_site_allele0(const phi_vcf *v) { return v->site_allele0.data(); }
int32_t phi_vcf_n_kept_haps(const phi_vcf *v) { return v->built ? (int32_t)v->keep.size() : 0; }
const int32_t *phi_vcf_choice(const phi_vcf *v) { return v->choice.data(); }

}  // extern "C"
