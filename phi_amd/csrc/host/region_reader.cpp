// region_reader.cpp -- the C entry points of ../region_host.h (include/phi_host.h, phi_region_*): what `tabix FILE REGION` and
// `samtools faidx FILE REGION` do on the host before phi_vcf_region_filter (include/phi_amd.h) looks at a record.
#include <stdarg.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "gz_source.h"
#include "../region_host.h"
#include "../../../include/phi_host.h"

namespace {

int rfail(char *err, int cap, int code, const char *fmt, ...)
{
    if (err && cap > 0) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, (size_t)cap, fmt, ap);
        va_end(ap);
    }
    return code;
}

bool exists(const std::string &path) { struct stat st; return stat(path.c_str(), &st) == 0; }

// a small BGZF file (an index) inflated with gz_source.h: 0 ok, -1 cannot open / no gzip, -2 corrupt
int load_gz(const std::string &path, std::vector<char> &out)
{
    GzSource gz;
    if (!gz.open(path.c_str(), 1)) return -1;
    std::vector<char> blk;
    while (gz.next(blk)) out.insert(out.end(), blk.begin(), blk.end());
    const bool ok = gz.ok();
    gz.close();
    return ok ? 0 : -2;
}

}  // namespace

struct phi_region {
    std::string name;
    int64_t beg = 0, end = 0, contig_len = 0;
    bool in_index = false;
    regionx::Plan plan;
    std::vector<int64_t> member_at;
    std::vector<char> header, ref;
    int64_t fasta_members = 0;
};

namespace {

// the plan of [b, e) on contig `name` of the BGZF VCF at vcf_path, through vcf_path + ".tbi"
int plan_vcf(const char *vcf_path, const char *name, int64_t b, int64_t e, bool load, phi_region *r, char *err, int cap)
{
    const std::string vcf(vcf_path), tbi_path = vcf + ".tbi";
    regionx::Fd f;
    if (!f.open(vcf_path)) return rfail(err, cap, PHI_HOST_ERR_IO, "cannot open %s", vcf_path);
    regionx::Member m0;
    if (!regionx::is_gzip(f) || !regionx::member_at(f, 0, &m0))
        return rfail(err, cap, PHI_HOST_ERR_UNSUPPORTED, "%s is %s: a region read needs a BGZF file (bgzip) with its .tbi", vcf_path, regionx::is_gzip(f) ? "gzip but not BGZF" : "not compressed");
    if (!exists(tbi_path)) {
        if (exists(vcf + ".csi")) return rfail(err, cap, PHI_HOST_ERR_UNSUPPORTED, "%s.csi: a CSI index is unsupported, and there is no %s (tabix -p vcf writes it)", vcf_path, tbi_path.c_str());
        return rfail(err, cap, PHI_HOST_ERR_IO, "cannot open %s (tabix -p vcf writes it; a region read goes through it)", tbi_path.c_str());
    }
    std::vector<char> raw;
    const int lrc = load_gz(tbi_path, raw);
    if (lrc) return rfail(err, cap, lrc == -2 ? PHI_HOST_ERR_INVALID : PHI_HOST_ERR_IO, lrc == -2 ? "%s: corrupt gzip stream" : "cannot open %s, or it is not compressed", tbi_path.c_str());
    regionx::Tbi tbi;
    std::string why = regionx::parse_tbi((const uint8_t *)raw.data(), raw.size(), &tbi);
    if (!why.empty()) return rfail(err, cap, why.find("unsupported") != std::string::npos ? PHI_HOST_ERR_UNSUPPORTED : PHI_HOST_ERR_INVALID, "%s: %s", tbi_path.c_str(), why.c_str());
    r->name = name;
    r->beg = b;
    r->end = e;
    std::vector<regionx::Chunk> chunks;
    for (const regionx::TbiContig &c : tbi.contigs)
        if (c.name == r->name) { r->in_index = true; chunks = regionx::select_chunks(c, b, e); break; }
    why = regionx::plan_members(f, chunks, &r->plan, load);
    if (!why.empty()) return rfail(err, cap, PHI_HOST_ERR_INVALID, "%s: %s", vcf_path, why.c_str());
    for (const regionx::Member &m : r->plan.members) r->member_at.push_back(m.at);
    why = regionx::header_text(f, &r->header);
    if (!why.empty()) return rfail(err, cap, PHI_HOST_ERR_INVALID, "%s: %s", vcf_path, why.c_str());
    return PHI_HOST_OK;
}

// the .fai record `name` of the FASTA at path (NULL when the file holds none of that name)
int fai_find(const char *fasta_path, const std::string &name, regionx::FaiRecord *rec, bool *found, char *err, int cap)
{
    const std::string fai_path = std::string(fasta_path) + ".fai";
    std::vector<char> raw;
    if (!regionx::read_whole(fai_path, &raw)) return rfail(err, cap, PHI_HOST_ERR_IO, "cannot open %s (samtools faidx writes it; a region read goes through it)", fai_path.c_str());
    std::vector<regionx::FaiRecord> recs;
    const std::string why = regionx::parse_fai(raw.data(), raw.size(), &recs);
    if (!why.empty()) return rfail(err, cap, PHI_HOST_ERR_INVALID, "%s: %s", fai_path.c_str(), why.c_str());
    *found = false;
    for (const regionx::FaiRecord &x : recs)
        if (x.name == name) { *rec = x; *found = true; break; }
    return PHI_HOST_OK;
}

}  // namespace

extern "C" {

int phi_region_parse(const char *region, char *name, int name_cap, int64_t *beg1, int64_t *end1, char *err, int err_cap)
{
    if (!region || !name || name_cap < 1 || !beg1 || !end1) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "null argument");
    regionx::Region r;
    const std::string why = regionx::parse_region(region, &r);
    if (!why.empty()) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "--region %s: %s", region, why.c_str());
    if ((int)r.name.size() >= name_cap) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "--region: a contig name of %zu bytes", r.name.size());
    memcpy(name, r.name.c_str(), r.name.size() + 1);
    *beg1 = r.beg1;
    *end1 = r.end1;
    return PHI_HOST_OK;
}

int phi_region_plan(const char *vcf_path, const char *name, int64_t beg, int64_t end, int32_t load, phi_region **out, char *err, int err_cap)
{
    if (!vcf_path || !name || !out) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "null argument");
    *out = nullptr;
    phi_region *r = new phi_region;
    const int rc = plan_vcf(vcf_path, name, beg, end, load != 0, r, err, err_cap);
    if (rc) { delete r; return rc; }
    *out = r;
    return PHI_HOST_OK;
}

int phi_fasta_slice(const char *fasta_path, const char *name, int64_t beg, int64_t end, char **bases, int64_t *n_bases, int64_t *contig_len,
                    int64_t *members_read, char *err, int err_cap)
{
    if (!fasta_path || !name || !bases || !n_bases) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "null argument");
    *bases = nullptr;
    *n_bases = 0;
    regionx::FaiRecord rec;
    bool found = false;
    const int rc = fai_find(fasta_path, name, &rec, &found, err, err_cap);
    if (rc) return rc;
    if (!found) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "%s.fai holds no record named %s", fasta_path, name);
    if (contig_len) *contig_len = rec.len;
    if (end < 0 || end > rec.len) end = rec.len;
    std::vector<char> out;
    const std::string why = regionx::fasta_slice(fasta_path, rec, beg, end, &out, members_read);
    if (!why.empty()) {
        const bool unsup = why.find("not BGZF") != std::string::npos, io = why.find("cannot open") != std::string::npos;
        return rfail(err, err_cap, unsup ? PHI_HOST_ERR_UNSUPPORTED : io ? PHI_HOST_ERR_IO : PHI_HOST_ERR_INVALID, "%s", why.c_str());
    }
    char *p = (char *)malloc(out.size() + 1);
    if (!p) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "out of memory");
    if (!out.empty()) memcpy(p, out.data(), out.size());
    p[out.size()] = 0;
    *bases = p;
    *n_bases = (int64_t)out.size();
    return PHI_HOST_OK;
}

int phi_region_open(const char *vcf_path, const char *fasta_path, const char *region, phi_region **out, char *err, int err_cap)
{
    if (!vcf_path || !fasta_path || !region || !out) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "null argument");
    *out = nullptr;
    regionx::Region rg;
    std::string why = regionx::parse_region(region, &rg);
    if (!why.empty()) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "--region %s: %s", region, why.c_str());
    regionx::FaiRecord rec;
    bool found = false;
    int rc = fai_find(fasta_path, rg.name, &rec, &found, err, err_cap);
    if (rc) return rc;
    if (!found && rg.name != region) {                  // a name with a colon of its own that looks like an interval
        rc = fai_find(fasta_path, region, &rec, &found, err, err_cap);
        if (found) { rg = regionx::Region{}; rg.name = region; }
    }
    if (!found) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "--region %s: %s.fai holds no record named %s", region, fasta_path, rg.name.c_str());
    int64_t b, e;
    why = regionx::resolve_region(rg, rec.len, &b, &e);
    if (!why.empty()) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "--region %s: %s", region, why.c_str());
    phi_region *r = new phi_region;
    struct Guard { phi_region *&r; ~Guard() { delete r; } } guard{r};
    if ((rc = plan_vcf(vcf_path, rg.name.c_str(), b, e, true, r, err, err_cap))) return rc;
    if (!r->in_index) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "--region %s: %s.tbi holds no contig named %s", region, vcf_path, rg.name.c_str());
    r->contig_len = rec.len;
    why = regionx::fasta_slice(fasta_path, rec, b, e, &r->ref, &r->fasta_members);
    if (!why.empty()) {
        const bool unsup = why.find("not BGZF") != std::string::npos, io = why.find("cannot open") != std::string::npos;
        return rfail(err, err_cap, unsup ? PHI_HOST_ERR_UNSUPPORTED : io ? PHI_HOST_ERR_IO : PHI_HOST_ERR_INVALID, "%s", why.c_str());
    }
    *out = r;
    r = nullptr;
    return PHI_HOST_OK;
}

// the rule pass of phi_vcf_read over the header and the lines phi_vcf_region_filter kept, against the reference slice
int phi_vcf_read_region(const phi_region *rg, const char *lines, int64_t n_lines, phi_vcf **out, char *err, int err_cap)
{
    if (!rg || !out || n_lines < 0 || (n_lines > 0 && !lines)) return rfail(err, err_cap, PHI_HOST_ERR_INVALID, "null argument or negative size");
    std::string text(phi_region_header(rg), (size_t)phi_region_n_header(rg));
    if (n_lines) text.append(lines, (size_t)n_lines);
    return phi_vcf_read_text(text.data(), (int64_t)text.size(), phi_region_ref(rg), phi_region_n_ref(rg), phi_region_name(rg), phi_region_beg(rg),
                             phi_region_name(rg), out, err, err_cap);
}

void phi_region_free(phi_region *r) { delete r; }
void phi_region_free_bases(char *p) { free(p); }
const char *phi_region_name(const phi_region *r) { return r->name.c_str(); }
int64_t phi_region_beg(const phi_region *r) { return r->beg; }
int64_t phi_region_end(const phi_region *r) { return r->end; }
int64_t phi_region_contig_len(const phi_region *r) { return r->contig_len; }
int32_t phi_region_in_index(const phi_region *r) { return r->in_index; }
int64_t phi_region_n_members(const phi_region *r) { return (int64_t)r->plan.members.size(); }
const int64_t *phi_region_member_at(const phi_region *r) { return r->member_at.data(); }
const int64_t *phi_region_member_text_off(const phi_region *r) { return r->plan.text_off.data(); }
int32_t phi_region_n_ranges(const phi_region *r) { return (int32_t)(r->plan.range.size() / 2); }
const int64_t *phi_region_ranges(const phi_region *r) { return r->plan.range.data(); }
const char *phi_region_gz(const phi_region *r) { return r->plan.gz.data(); }
int64_t phi_region_n_gz(const phi_region *r) { return (int64_t)r->plan.gz.size(); }
const char *phi_region_header(const phi_region *r) { return r->header.data(); }
int64_t phi_region_n_header(const phi_region *r) { return (int64_t)r->header.size(); }
const char *phi_region_ref(const phi_region *r) { return r->ref.data(); }
int64_t phi_region_n_ref(const phi_region *r) { return (int64_t)r->ref.size(); }
int64_t phi_region_fasta_members(const phi_region *r) { return r->fasta_members; }

}  // extern "C"
