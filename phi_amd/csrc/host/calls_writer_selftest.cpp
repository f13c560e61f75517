// calls_writer_selftest.cpp -- the VCF writer of the calls (calls_writer.cpp), plain and with the read support of every call, on
// hand-made records: a substitution, a padded insertion, a REF = ALT call that is dropped, a padded deletion in lower case (the
// records of tests/test_cpu_calls_host.py).  A stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C phi_amd/csrc/host calls_writer_sanitize`); tests/test_cpu_calls_support_host.py runs it as a child process.
//   calls_writer_selftest [file to write]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../../include/phi_host.h"

static int n_checks = 0;
#define CHECK(cond) do { n_checks++; if (!(cond)) { fprintf(stderr, "calls_writer_selftest: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// the support text with its two header lines and the :AK:RK columns taken out
static std::string stripped(const std::string &text)
{
    std::string out;
    size_t at = 0;
    while (at < text.size()) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        std::string ln = text.substr(at, end - at);
        at = end + 1;
        if (ln.rfind("##FORMAT=<ID=AK,", 0) == 0 || ln.rfind("##FORMAT=<ID=RK,", 0) == 0) continue;
        if (ln[0] != '#') {
            const size_t f = ln.find("\tGT:AK:RK\t1:");
            if (f != std::string::npos) ln = ln.substr(0, f) + "\tGT\t1";
        }
        out += ln + "\n";
    }
    return out;
}

int main(int argc, char **argv)
{
    const int64_t pos[4] = {2, 9, 12, 15}, ref_off[5] = {0, 2, 3, 5, 9}, alt_off[5] = {0, 3, 6, 8, 9};
    const char *ref_bytes = "GTTCCgtca", *alt_bytes = "cccTAACCg";
    const char *ph[4] = {"hapA.1", "hapA.1", "hapB.1", "hapC.2"};
    const int32_t alt_hit[4] = {3, 0, 77, 2}, alt_n[4] = {5, 0, 99, 2147483647}, ref_hit[4] = {0, 1, 88, 0}, ref_n[4] = {4, 6, 99, 12};
    char err[256] = "";
    char *plain = nullptr, *sup = nullptr;
    int64_t n_plain = 0, n_sup = 0, nw = -1, nd = -1;

    CHECK(phi_format_calls_vcf("chrT", 25, "sample_1", 4, pos, ref_off, ref_bytes, alt_off, alt_bytes, ph, &plain, &n_plain, &nw, &nd, err, 256) == PHI_HOST_OK);
    CHECK(nw == 3 && nd == 1);
    CHECK(phi_format_calls_vcf_support("chrT", 25, "sample_1", 4, pos, ref_off, ref_bytes, alt_off, alt_bytes, ph, alt_hit, alt_n, ref_hit, ref_n, &sup, &n_sup,
                                       &nw, &nd, err, 256) == PHI_HOST_OK);
    CHECK(nw == 3 && nd == 1);
    const std::string p(plain, (size_t)n_plain), s(sup, (size_t)n_sup);
    phi_host_free_text(plain);
    phi_host_free_text(sup);
    CHECK(stripped(s) == p && s != p);
    CHECK(s.find("##FORMAT=<ID=AK,Number=2,Type=Integer,Description=\"ALT witness minimisers: seen in the reads, all\">\n"
                 "##FORMAT=<ID=RK,Number=2,Type=Integer,Description=\"REF witness minimisers: seen in the reads, all\">\n#CHROM") != std::string::npos);
    CHECK(s.find("chrT\t3\t.\tGT\tccc\t.\tPASS\tPH=hapA.1\tGT:AK:RK\t1:3,5:0,4\n") != std::string::npos);
    CHECK(s.find("chrT\t10\t.\tT\tTAA\t.\tPASS\tPH=hapA.1\tGT:AK:RK\t1:0,0:1,6\n") != std::string::npos);
    CHECK(s.find("chrT\t16\t.\tgtca\tg\t.\tPASS\tPH=hapC.2\tGT:AK:RK\t1:2,2147483647:0,12\n") != std::string::npos);
    CHECK(s.find("77") == std::string::npos && s.find("88") == std::string::npos && s.find("hapB.1") == std::string::npos);   // the dropped call's counts go with it

    // without tags; no call at all; refusals
    CHECK(phi_format_calls_vcf_support("chrT", 25, "s", 4, pos, ref_off, ref_bytes, alt_off, alt_bytes, nullptr, alt_hit, alt_n, ref_hit, ref_n, &sup, &n_sup,
                                       nullptr, nullptr, err, 256) == PHI_HOST_OK);
    CHECK(std::string(sup, (size_t)n_sup).find("\tPASS\t.\tGT:AK:RK\t1:3,5:0,4\n") != std::string::npos);
    phi_host_free_text(sup);
    CHECK(phi_format_calls_vcf_support("chrT", 25, "s", 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &sup, &n_sup,
                                       &nw, &nd, err, 256) == PHI_HOST_OK);
    CHECK(nw == 0 && nd == 0 && std::string(sup, (size_t)n_sup).find("ID=RK") != std::string::npos && sup[n_sup - 1] == '\n');
    phi_host_free_text(sup);
    sup = (char *)1;
    CHECK(phi_format_calls_vcf_support("chrT", 25, "s", 4, pos, ref_off, ref_bytes, alt_off, alt_bytes, ph, alt_hit, nullptr, ref_hit, ref_n, &sup, &n_sup, &nw,
                                       &nd, err, 256) == PHI_HOST_ERR_INVALID);
    CHECK(sup == nullptr && n_sup == 0 && strstr(err, "null argument"));
    const int64_t bad_off[5] = {0, 3, 3, 8, 9};
    CHECK(phi_format_calls_vcf_support("chrT", 25, "s", 4, pos, ref_off, ref_bytes, bad_off, alt_bytes, ph, alt_hit, alt_n, ref_hit, ref_n, &sup, &n_sup, &nw, &nd,
                                       err, 256) == PHI_HOST_ERR_INVALID);
    CHECK(strstr(err, "empty allele"));
    CHECK(phi_write_calls_vcf_support("x.vcf.gz", "chrT", 25, "s", 4, pos, ref_off, ref_bytes, alt_off, alt_bytes, ph, alt_hit, alt_n, ref_hit, ref_n, &nw, &nd,
                                      err, 256) == PHI_HOST_ERR_INVALID);
    CHECK(strstr(err, ".gz"));

    if (argc > 1) {                                        // the file holds the text
        CHECK(phi_write_calls_vcf_support(argv[1], "chrT", 25, "sample_1", 4, pos, ref_off, ref_bytes, alt_off, alt_bytes, ph, alt_hit, alt_n, ref_hit, ref_n, &nw,
                                          &nd, err, 256) == PHI_HOST_OK);
        CHECK(nw == 3 && nd == 1);
        FILE *fp = fopen(argv[1], "rb");
        CHECK(fp != nullptr);
        std::vector<char> buf(s.size() + 16);
        const size_t got = fread(buf.data(), 1, buf.size(), fp);
        fclose(fp);
        CHECK(got == s.size() && memcmp(buf.data(), s.data(), got) == 0);
    }
    printf("calls_writer_selftest: ok %d checks\n", n_checks);
    return 0;
}
