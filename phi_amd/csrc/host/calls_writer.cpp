// calls_writer.cpp -- the variant calls of phi_calls_path / phi_calls_walk (include/phi_amd.h) written as plain-text VCFv4.2.
// The reference writes no VCF (its one product is the FASTA of ILP_index.cpp:1590-1598); the file serves the comparison it
// makes the other way round with `bcftools consensus` (data/run_PG.py:54-60).  Plain host code: no deflate writer.
#include <stdio.h>
#include <string.h>
#include <string>
#include "../../../include/phi_host.h"

namespace {

int fail(char *err, int err_cap, int code, const std::string &msg)
{
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", msg.c_str());
    return code;
}

}  // namespace

extern "C" {

int phi_write_calls_vcf(const char *path, const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos,
                        const int64_t *ref_off, const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph,
                        int64_t *n_written, int64_t *n_dropped, char *err, int err_cap)
{
    if (n_written) *n_written = 0;
    if (n_dropped) *n_dropped = 0;
    if (!path || !contig || !sample || n_calls < 0 || (n_calls > 0 && (!pos || !ref_off || !alt_off || !ref_bytes || !alt_bytes)))
        return fail(err, err_cap, PHI_HOST_ERR_INVALID, "phi_write_calls_vcf: null argument");
    const size_t pn = strlen(path);
    if (pn >= 3 && strcmp(path + pn - 3, ".gz") == 0)
        return fail(err, err_cap, PHI_HOST_ERR_INVALID, std::string("cannot write ") + path + ": the calls are written as plain text (there is no deflate writer); give a name that does not end in .gz");
    for (int64_t k = 0; k < n_calls; k++)
        if (ref_off[k + 1] <= ref_off[k] || alt_off[k + 1] <= alt_off[k] || pos[k] < 0)
            return fail(err, err_cap, PHI_HOST_ERR_INVALID, "phi_write_calls_vcf: call " + std::to_string(k) + " has an empty allele or a negative position");
    FILE *fp = fopen(path, "w");
    if (!fp) return fail(err, err_cap, PHI_HOST_ERR_IO, std::string("cannot write ") + path);
    fprintf(fp, "##fileformat=VCFv4.2\n##source=phi_amd\n##contig=<ID=%s,length=%lld>\n", contig, (long long)contig_len);
    fputs("##INFO=<ID=PH,Number=1,Type=String,Description=\"Panel haplotype the inferred path follows through the call\">\n", fp);
    fputs("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n", fp);
    fprintf(fp, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n", sample);
    int64_t nw = 0, nd = 0;
    bool ok = true;
    for (int64_t k = 0; k < n_calls && ok; k++) {
        const size_t rn = (size_t)(ref_off[k + 1] - ref_off[k]), an = (size_t)(alt_off[k + 1] - alt_off[k]);
        const char *r = ref_bytes + ref_off[k], *a = alt_bytes + alt_off[k];
        if (rn == an && memcmp(r, a, rn) == 0) { nd++; continue; }      // other vertices, the same sequence: no variant
        fprintf(fp, "%s\t%lld\t.\t", contig, (long long)pos[k] + 1);
        ok = fwrite(r, 1, rn, fp) == rn && fputc('\t', fp) != EOF && fwrite(a, 1, an, fp) == an;
        const char *name = ph ? ph[k] : nullptr;
        if (name && *name) fprintf(fp, "\t.\tPASS\tPH=%s\tGT\t1\n", name);
        else fputs("\t.\tPASS\t.\tGT\t1\n", fp);
        nw++;
    }
    if (fclose(fp) != 0 || !ok) return fail(err, err_cap, PHI_HOST_ERR_IO, std::string("cannot write ") + path);
    if (n_written) *n_written = nw;
    if (n_dropped) *n_dropped = nd;
    return PHI_HOST_OK;
}

}  // extern "C"
