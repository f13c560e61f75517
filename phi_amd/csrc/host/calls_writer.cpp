// calls_writer.cpp -- the variant calls of phi_calls_path / phi_calls_walk (include/phi_amd.h) written as plain-text VCFv4.2.
// The reference writes no VCF (its one product is the FASTA of ILP_index.cpp:1590-1598); the file serves the comparison it
// makes the other way round with `bcftools consensus` (data/run_PG.py:54-60).  Plain host code.  The text
// is also handed out in memory (phi_format_calls_vcf, phi_format_fasta) for the device's BGZF writer (phi_deflate_bgzf, phi_amd.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "../../../include/phi_host.h"

namespace {

int fail(char *err, int err_cap, int code, const std::string &msg)
{
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", msg.c_str());
    return code;
}

// the four count arrays of phi_calls_support (phi_amd.h), or none: the plain file
struct Support { const int32_t *alt_hit, *alt_n, *ref_hit, *ref_n; };

// the file's text, with FORMAT/AK and RK where sup is given; the arguments are checked by the callers
int format_calls(std::string &out, const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos, const int64_t *ref_off,
                 const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph, const Support *sup, int64_t *n_written,
                 int64_t *n_dropped, char *err, int err_cap, const char *who)
{
    if (sup && n_calls > 0 && (!sup->alt_hit || !sup->alt_n || !sup->ref_hit || !sup->ref_n))
        return fail(err, err_cap, PHI_HOST_ERR_INVALID, std::string(who) + ": null argument");
    if (!contig || !sample || n_calls < 0 || (n_calls > 0 && (!pos || !ref_off || !alt_off || !ref_bytes || !alt_bytes)))
        return fail(err, err_cap, PHI_HOST_ERR_INVALID, std::string(who) + ": null argument");
    for (int64_t k = 0; k < n_calls; k++)
        if (ref_off[k + 1] <= ref_off[k] || alt_off[k + 1] <= alt_off[k] || pos[k] < 0)
            return fail(err, err_cap, PHI_HOST_ERR_INVALID, std::string(who) + ": call " + std::to_string(k) + " has an empty allele or a negative position");
    out += "##fileformat=VCFv4.2\n##source=phi_amd\n##contig=<ID=";
    out += contig;
    out += ",length=" + std::to_string((long long)contig_len) + ">\n";
    out += "##INFO=<ID=PH,Number=1,Type=String,Description=\"Panel haplotype the inferred path follows through the call\">\n";
    out += "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n";
    if (sup) {
        out += "##FORMAT=<ID=AK,Number=2,Type=Integer,Description=\"ALT witness minimisers: seen in the reads, all\">\n";
        out += "##FORMAT=<ID=RK,Number=2,Type=Integer,Description=\"REF witness minimisers: seen in the reads, all\">\n";
    }
    out += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t";
    out += sample;
    out += '\n';
    int64_t nw = 0, nd = 0;
    for (int64_t k = 0; k < n_calls; k++) {
        const size_t rn = (size_t)(ref_off[k + 1] - ref_off[k]), an = (size_t)(alt_off[k + 1] - alt_off[k]);
        const char *r = ref_bytes + ref_off[k], *a = alt_bytes + alt_off[k];
        if (rn == an && memcmp(r, a, rn) == 0) { nd++; continue; }      // other vertices, the same sequence: no variant
        out += contig;
        out += '\t';
        out += std::to_string((long long)pos[k] + 1);
        out += "\t.\t";
        out.append(r, rn);
        out += '\t';
        out.append(a, an);
        const char *name = ph ? ph[k] : nullptr;
        if (name && *name) { out += "\t.\tPASS\tPH="; out += name; }
        else out += "\t.\tPASS\t.";
        if (sup) {
            out += "\tGT:AK:RK\t1:" + std::to_string(sup->alt_hit[k]) + "," + std::to_string(sup->alt_n[k]) + ":" + std::to_string(sup->ref_hit[k]) + "," +
                   std::to_string(sup->ref_n[k]) + "\n";
        } else out += "\tGT\t1\n";
        nw++;
    }
    if (n_written) *n_written = nw;
    if (n_dropped) *n_dropped = nd;
    return PHI_HOST_OK;
}

int hand_over(const std::string &text, char **out, int64_t *n)
{
    char *p = (char *)malloc(text.size() ? text.size() : 1);
    if (!p) return PHI_HOST_ERR_IO;
    memcpy(p, text.data(), text.size());
    *out = p;
    *n = (int64_t)text.size();
    return PHI_HOST_OK;
}

// the text handed out in memory: the body of phi_format_calls_vcf and phi_format_calls_vcf_support
int format_to_memory(const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos, const int64_t *ref_off,
                     const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph, const Support *sup, char **out, int64_t *n,
                     int64_t *n_written, int64_t *n_dropped, char *err, int err_cap, const char *who)
{
    if (n_written) *n_written = 0;
    if (n_dropped) *n_dropped = 0;
    if (!out || !n) return fail(err, err_cap, PHI_HOST_ERR_INVALID, std::string(who) + ": null argument");
    *out = nullptr;
    *n = 0;
    std::string text;
    int64_t nw = 0, nd = 0;
    const int rc = format_calls(text, contig, contig_len, sample, n_calls, pos, ref_off, ref_bytes, alt_off, alt_bytes, ph, sup, &nw, &nd, err, err_cap, who);
    if (rc) return rc;
    if (hand_over(text, out, n)) return fail(err, err_cap, PHI_HOST_ERR_IO, std::string(who) + ": out of memory");
    if (n_written) *n_written = nw;
    if (n_dropped) *n_dropped = nd;
    return PHI_HOST_OK;
}

// the text written to a file: the body of phi_write_calls_vcf and phi_write_calls_vcf_support
int format_to_file(const char *path, const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos, const int64_t *ref_off,
                   const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph, const Support *sup, int64_t *n_written,
                   int64_t *n_dropped, char *err, int err_cap, const char *who)
{
    if (n_written) *n_written = 0;
    if (n_dropped) *n_dropped = 0;
    if (!path) return fail(err, err_cap, PHI_HOST_ERR_INVALID, std::string(who) + ": null argument");
    const size_t pn = strlen(path);
    if (pn >= 3 && strcmp(path + pn - 3, ".gz") == 0)
        return fail(err, err_cap, PHI_HOST_ERR_INVALID, std::string("cannot write ") + path + ": this writer writes plain text and has no deflate of its own; give a name that does not end in .gz, or compress the text of phi_format_calls_vcf with phi_deflate_bgzf (PHI --bgzf, write_vcf(bgzf=True))");
    std::string text;
    int64_t nw = 0, nd = 0;
    const int rc = format_calls(text, contig, contig_len, sample, n_calls, pos, ref_off, ref_bytes, alt_off, alt_bytes, ph, sup, &nw, &nd, err, err_cap, who);
    if (rc) return rc;
    FILE *fp = fopen(path, "w");
    if (!fp) return fail(err, err_cap, PHI_HOST_ERR_IO, std::string("cannot write ") + path);
    const bool ok = fwrite(text.data(), 1, text.size(), fp) == text.size();
    if (fclose(fp) != 0 || !ok) return fail(err, err_cap, PHI_HOST_ERR_IO, std::string("cannot write ") + path);
    if (n_written) *n_written = nw;
    if (n_dropped) *n_dropped = nd;
    return PHI_HOST_OK;
}

}  // namespace

extern "C" {

int phi_format_calls_vcf(const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos, const int64_t *ref_off,
                         const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph, char **out, int64_t *n,
                         int64_t *n_written, int64_t *n_dropped, char *err, int err_cap)
{
    return format_to_memory(contig, contig_len, sample, n_calls, pos, ref_off, ref_bytes, alt_off, alt_bytes, ph, nullptr, out, n, n_written, n_dropped, err,
                            err_cap, "phi_format_calls_vcf");
}

int phi_format_calls_vcf_support(const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos, const int64_t *ref_off,
                                 const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph, const int32_t *alt_hit,
                                 const int32_t *alt_n, const int32_t *ref_hit, const int32_t *ref_n, char **out, int64_t *n, int64_t *n_written,
                                 int64_t *n_dropped, char *err, int err_cap)
{
    const Support sup{alt_hit, alt_n, ref_hit, ref_n};
    return format_to_memory(contig, contig_len, sample, n_calls, pos, ref_off, ref_bytes, alt_off, alt_bytes, ph, &sup, out, n, n_written, n_dropped, err,
                            err_cap, "phi_format_calls_vcf_support");
}

int phi_write_calls_vcf(const char *path, const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos,
                        const int64_t *ref_off, const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph,
                        int64_t *n_written, int64_t *n_dropped, char *err, int err_cap)
{
    return format_to_file(path, contig, contig_len, sample, n_calls, pos, ref_off, ref_bytes, alt_off, alt_bytes, ph, nullptr, n_written, n_dropped, err,
                          err_cap, "phi_write_calls_vcf");
}

int phi_write_calls_vcf_support(const char *path, const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos,
                                const int64_t *ref_off, const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph,
                                const int32_t *alt_hit, const int32_t *alt_n, const int32_t *ref_hit, const int32_t *ref_n, int64_t *n_written,
                                int64_t *n_dropped, char *err, int err_cap)
{
    const Support sup{alt_hit, alt_n, ref_hit, ref_n};
    return format_to_file(path, contig, contig_len, sample, n_calls, pos, ref_off, ref_bytes, alt_off, alt_bytes, ph, &sup, n_written, n_dropped, err,
                          err_cap, "phi_write_calls_vcf_support");
}

// exactly the bytes phi_write_fasta (reads_reader.cpp) writes: ">" name " LN:" len, then 80-column lines
int phi_format_fasta(const char *name, const char *seq, int64_t len, char **out, int64_t *n)
{
    if (!name || !out || !n || len < 0 || (len > 0 && !seq)) return PHI_HOST_ERR_INVALID;
    const std::string head = std::string(">") + name + " LN:" + std::to_string((long long)len) + "\n";
    const int64_t lines = (len + 79) / 80, total = (int64_t)head.size() + len + lines;
    char *p = (char *)malloc((size_t)(total > 0 ? total : 1));
    if (!p) return PHI_HOST_ERR_IO;
    memcpy(p, head.data(), head.size());
    char *o = p + head.size();
    for (int64_t j = 0; j < len; j += 80) {
        const int64_t k = len - j < 80 ? len - j : 80;
        memcpy(o, seq + j, (size_t)k);
        o[k] = '\n';
        o += k + 1;
    }
    *out = p;
    *n = total;
    return PHI_HOST_OK;
}

// the .fai line of that text: NAME (the header up to its first blank), LEN, where the sequence begins, bases and bytes per line
int phi_format_fasta_fai(const char *name, int64_t len, char **out, int64_t *n)
{
    if (!name || !out || !n || len < 0) return PHI_HOST_ERR_INVALID;
    const std::string head = std::string(">") + name + " LN:" + std::to_string((long long)len) + "\n";
    size_t id = 0;
    while (name[id] && name[id] != ' ' && name[id] != '\t') id++;
    const long long bases = len < 80 ? len : 80, width = len > 0 ? bases + 1 : 0;
    const std::string line = std::string(name, id) + "\t" + std::to_string((long long)len) + "\t" + std::to_string(head.size()) + "\t" +
                             std::to_string(bases) + "\t" + std::to_string(width) + "\n";
    char *p = (char *)malloc(line.size());
    if (!p) return PHI_HOST_ERR_IO;
    memcpy(p, line.data(), line.size());
    *out = p;
    *n = (int64_t)line.size();
    return PHI_HOST_OK;
}

void phi_host_free_text(char *p) { free(p); }

}  // extern "C"
