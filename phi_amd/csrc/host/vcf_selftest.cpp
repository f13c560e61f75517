// vcf_selftest.cpp -- a driver of the VCF route's host side (vcf_reader.cpp) for the sanitizer build (`make vcf_sanitize`:
// AddressSanitizer + UndefinedBehaviorSanitizer; CPU only).  Test infrastructure.
//
//   vcf_selftest DIR     writes its own inputs into DIR -- a generated VCF with overlapping, multi-allelic and haploid records
//                        and GT second in FORMAT on some lines; the same with its last line truncated; one with a line of too
//                        few sample columns; a zero-length VCF -- and runs phi_vcf_read, phi_vcf_parse_gt and phi_vcf_build
//                        (at max_len 30, 7 and 1000) over each.  Prints one line per input: "name ok <checksum>" or
//                        "name error <code>"; exit status 0 unless something that must hold does not.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../../include/phi_host.h"

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

static bool write_file(const std::string &path, const std::string &data)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = data.empty() || fwrite(data.data(), 1, data.size(), f) == data.size();
    return fclose(f) == 0 && ok;
}

// -> 0 and a checksum, or the (negative) code of the step that refused
static int run(const std::string &vcf, const std::string &fa, uint64_t *sum)
{
    char err[512] = "";
    phi_vcf *v = nullptr;
    int rc = phi_vcf_read(vcf.c_str(), fa.c_str(), &v, err, sizeof err);
    if (rc) return rc;
    const int32_t ns = phi_vcf_n_samples(v);
    const int64_t nr = phi_vcf_n_records(v);
    std::vector<uint16_t> gt((size_t)nr * (size_t)ns * 2 + 1, 0);
    std::vector<int32_t> ploidy((size_t)ns + 1, 0);
    rc = phi_vcf_parse_gt(phi_vcf_text(v), phi_vcf_text_off(v), phi_vcf_rec_gt_index(v), 0, nr, ns, gt.data(), ploidy.data(), err, sizeof err);
    if (rc) { phi_vcf_free(v); return rc; }
    uint64_t h = 0xcbf29ce484222325ull;
    h = fnv(h, gt.data(), (size_t)nr * (size_t)ns * 4);
    h = fnv(h, ploidy.data(), (size_t)ns * 4);
    h = fnv(h, phi_vcf_site_off(v), (size_t)(phi_vcf_n_sites(v) + 1) * 8);
    const int lens[3] = {30, 7, 1000};
    for (int li = 0; li < 3; li++) {
        phi_graph *g = nullptr;
        rc = phi_vcf_build(v, gt.data(), ploidy.data(), lens[li], &g, err, sizeof err);
        if (rc) { phi_vcf_free(v); return rc; }
        const int32_t nv = phi_graph_n_vtx(g), nw = phi_graph_n_walks(g);
        h = fnv(h, &nv, 4); h = fnv(h, &nw, 4);
        h = fnv(h, phi_graph_seq_off(g), (size_t)(nv + 1) * 8);
        h = fnv(h, phi_graph_seq_concat(g), (size_t)phi_graph_seq_off(g)[nv]);
        h = fnv(h, phi_graph_adj_off(g), (size_t)(nv + 1) * 8);
        h = fnv(h, phi_graph_adj(g), (size_t)phi_graph_n_edges(g) * 4);
        h = fnv(h, phi_graph_topo_rank(g), (size_t)nv * 4);
        for (int32_t w = 0; w < nw; w++) { const char *s = phi_graph_hap_name(g, w); h = fnv(h, s, strlen(s) + 1); }
        h = fnv(h, phi_graph_seg_name(g, nv - 1), strlen(phi_graph_seg_name(g, nv - 1)));
        const int64_t nu = phi_vcf_n_units(v), nrs = phi_vcf_n_real_sites(v);
        if (phi_vcf_n_kept_haps(v) != nw || phi_vcf_unit_first(v)[nu] != nv || nu < 2 * nrs + 1) { phi_graph_free(g); phi_vcf_free(v); return -100; }
        h = fnv(h, phi_vcf_unit_first(v), (size_t)(nu + 1) * 4);
        h = fnv(h, phi_vcf_site_backbone(v), (size_t)nrs * 4);
        h = fnv(h, phi_vcf_site_allele0(v), (size_t)nrs * 4);
        h = fnv(h, phi_vcf_choice(v), (size_t)nrs * (size_t)nw * 4);
        phi_graph_free(g);
    }
    phi_vcf_free(v);
    *sum = h;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: vcf_selftest DIR\n"); return 2; }
    const std::string dir = argv[1];
    std::string ref;
    for (int i = 0; i < 5000; i++) ref += "ACGT"[rnd(4)];
    std::string fa = ">chr some words\n";
    for (size_t i = 0; i < ref.size(); i += 60) fa += ref.substr(i, 60) + "\r\n";
    const int n_s = 7;                                  // sample 6 is haploid
    std::string vcf = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
    for (int s = 0; s < n_s; s++) vcf += "\tS" + std::to_string(s);
    vcf += "\n";
    std::string last_line;
    for (size_t pos = 5; pos + 80 < ref.size();) {
        const size_t rl = rnd(2) ? 1 : 1 + rnd(40);
        const int n_alt = 1 + (int)rnd(3);
        std::string alts;
        for (int a = 0; a < n_alt; a++) {
            std::string s(1, ref[pos]);
            for (uint32_t k = rnd(4) ? 0 : rnd(44); k > 0; k--) s += "ACGT"[rnd(4)];
            if (s.size() == 1 && rl == 1) s[0] = s[0] == 'A' ? 'C' : 'A';
            alts += (a ? "," : "") + s;
        }
        const bool second = rnd(3) == 0;
        std::string line = "chr\t" + std::to_string(pos + 1) + "\t.\t" + ref.substr(pos, rl) + "\t" + alts + "\t60\t.\t.\t" + (second ? "DP:GT:FT" : "GT");
        for (int s = 0; s < n_s; s++) {
            std::string g = std::to_string(rnd((uint32_t)n_alt + 2));            // (one beyond the ALTs: not applied)
            if (s < 6) g += (rnd(8) ? "|" : "/") + (rnd(10) ? std::to_string(rnd((uint32_t)n_alt + 1)) : std::string("."));
            line += "\t" + (second ? "35:" + g + ":PASS" : g);
        }
        last_line = line;
        vcf += line + (rnd(5) ? "\n" : "\r\n");
        const uint32_t step = rnd(20);
        pos += step < 2 ? 0 : step < 7 ? 1 + rnd((uint32_t)rl) : rl + rnd(60);
    }
    if (!write_file(dir + "/r.fa", fa) || !write_file(dir + "/full.vcf", vcf)) { fprintf(stderr, "cannot write into %s\n", dir.c_str()); return 2; }
    // the last line cut inside its sample columns, no line feed: fewer fields than samples
    std::string cut = vcf;
    while (!cut.empty() && (cut.back() == '\n' || cut.back() == '\r')) cut.pop_back();
    cut.resize(cut.size() - 9);
    // a line with too few sample columns in the middle
    std::string few = vcf;
    {
        const size_t at = few.find("\nchr\t", few.size() / 2);
        const size_t le = few.find('\n', at + 1);
        size_t t = few.rfind('\t', le);
        t = few.rfind('\t', t - 1);
        few.erase(t, le - t);
    }
    // the last line cut inside its fixed columns: fewer than ten columns, skipped
    std::string cut_fixed = vcf.substr(0, vcf.size() - last_line.size() - 1) + last_line.substr(0, 12);
    if (!write_file(dir + "/cut.vcf", cut) || !write_file(dir + "/few.vcf", few) || !write_file(dir + "/cut_fixed.vcf", cut_fixed) ||
        !write_file(dir + "/empty.vcf", "") || !write_file(dir + "/two.fa", fa + ">second\nACGT\n"))
        return 2;
    int bad = 0;
    struct Case { const char *name, *vcf, *fa; bool must_fail; } cases[] = {
        {"full", "/full.vcf", "/r.fa", false}, {"cut", "/cut.vcf", "/r.fa", true}, {"few", "/few.vcf", "/r.fa", true},
        {"cut_fixed", "/cut_fixed.vcf", "/r.fa", false}, {"empty", "/empty.vcf", "/r.fa", false}, {"two_records", "/full.vcf", "/two.fa", true},
        {"missing", "/none.vcf", "/r.fa", true}};
    for (const Case &c : cases) {
        uint64_t sum = 0;
        const int rc = run(dir + c.vcf, dir + c.fa, &sum);
        if (rc) printf("%s error %d\n", c.name, rc);
        else printf("%s ok %016llx\n", c.name, (unsigned long long)sum);
        if ((rc != 0) != c.must_fail || rc == -100) bad = 1;
    }
    return bad;
}
