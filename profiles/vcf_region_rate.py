"""A region read of an indexed VCF and FASTA (set_graph_vcf(region=), phi_vcf_region_filter): what it costs beside
the two ways there were.  Run by hand on the MI355X; writes profiles/vcf_region_rate.json, everything taken in one run.  The
input is written here: a population-style VCF that phi_amd/vcf2gfa.py reads (phased GT, --samples samples, --contigs contigs of
--contig-bases bases, a record every ~60 bases), compressed and indexed on the device (phi_amd.deflate_bgzf_indexed), and its
reference as a BGZF FASTA with .fai and .gzi.  For ONE region of about 3 % of the file:

  (i)   the region route: wall time of Context.vcf_graph(vcf.gz, fa.gz, region=R) and its stats (phi_vcf_region_info, plan_s,
        filter_s, read_s, ...); a warm-up, then --repeats runs, the median
  (ii)  today's route on a pre-cut plain file: the header and the region's lines with POS shifted, a one-record FASTA
  (iii) phi_vcf_read over the whole file with its first contig in a one-record FASTA, as the parent commit has to do it (the
        host's read stage only: ilp_index.VcfGraph; the first contig seen is the one it keeps)

    python profiles/vcf_region_rate.py [--samples 2504] [--contigs 4] [--contig-bases 2000000] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401  (its HIP runtime initialises first, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import phi_amd                                                  # noqa: E402
from phi_amd import ilp_index as H                              # noqa: E402

LINE = 60


def make_inputs(tmp, n_samples, n_contigs, contig_bases, seed=7):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    names = [f"ctg{c + 1}" for c in range(n_contigs)]
    ref = {n: acgt[rng.integers(0, 4, contig_bases)].tobytes() for n in names}
    head = [b"##fileformat=VCFv4.2"] + [b"##contig=<ID=%s,length=%d>" % (n.encode(), contig_bases) for n in names]
    head += [b'##FORMAT=<ID=GT,Number=1,Type=String,Description="genotype">',
             ("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"S{i}" for i in range(n_samples))).encode()]
    gt = np.array([b"0|0", b"0|1", b"1|0", b"1|1"], dtype="S3")
    parts, recs = [b"\n".join(head) + b"\n"], {n: [] for n in names}
    for n in names:
        seq, pos = ref[n], 200
        while pos < contig_bases - 400:
            r = seq[pos:pos + 1]
            alt = b"C" if r != b"C" else b"G"
            af = float(rng.choice([0.01, 0.05, 0.3]))
            cols = b"\t".join(gt[(rng.random(n_samples) < af).astype(np.int8) + 2 * (rng.random(n_samples) < af).astype(np.int8)].tolist())
            line = b"%s\t%d\t.\t%s\t%s\t.\tPASS\tAF=%.2f\tGT\t%s\n" % (n.encode(), pos + 1, r, alt, af, cols)
            parts.append(line)
            recs[n].append((pos, line))
            pos += int(rng.integers(30, 90))
    text = b"".join(parts)
    data, tbi, _ = phi_amd.deflate_bgzf_indexed(text, "tbi")
    vcf = os.path.join(tmp, "pop.vcf.gz")
    open(vcf, "wb").write(data)
    open(vcf + ".tbi", "wb").write(tbi)
    fasta, fai, at = [], [], 0
    for n in names:
        hdr = b">" + n.encode() + b"\n"
        body = b"".join(ref[n][i:i + LINE] + b"\n" for i in range(0, contig_bases, LINE))
        fai.append(b"%s\t%d\t%d\t%d\t%d\n" % (n.encode(), contig_bases, at + len(hdr), LINE, LINE + 1))
        fasta += [hdr, body]
        at += len(hdr) + len(body)
    packed, gzi, _ = phi_amd.deflate_bgzf_indexed(b"".join(fasta), "gzi")
    fa = os.path.join(tmp, "pop.fa.gz")
    open(fa, "wb").write(packed)
    open(fa + ".gzi", "wb").write(gzi)
    open(fa + ".fai", "wb").write(b"".join(fai))
    return dict(vcf=vcf, fa=fa, text=text, head=parts[0], ref=ref, recs=recs, names=names, vcf_bytes=len(data))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--contigs", type=int, default=4)
    ap.add_argument("--contig-bases", type=int, default=2000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_region_rate.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        inp = make_inputs(tmp, a.samples, a.contigs, a.contig_bases)
        made_s = time.perf_counter() - t0
        name = inp["names"][len(inp["names"]) // 2]
        width = int(0.03 * a.contigs * a.contig_bases)
        b = a.contig_bases // 3
        recs = inp["recs"][name]
        while any(p - 2 <= b <= p + 2 for p, _ in recs):
            b += 1
        e = b + width
        while any(p - 2 <= e <= p + 2 for p, _ in recs):
            e += 1
        region = f"{name}:{b + 1}-{e}"
        lines = [ln for p, ln in recs if b <= p < e]
        cut_vcf, cut_fa, one_fa = os.path.join(tmp, "cut.vcf"), os.path.join(tmp, "cut.fa"), os.path.join(tmp, "one.fa")
        with open(cut_vcf, "wb") as f:
            f.write(inp["head"])
            for ln in lines:
                c = ln.split(b"\t", 2)
                f.write(b"\t".join((c[0], b"%d" % (int(c[1]) - b), c[2])))
        open(cut_fa, "wb").write(b">cut\n" + inp["ref"][name][b:e] + b"\n")
        first = inp["names"][0]                                 # phi_vcf_read keeps the first contig seen
        open(one_fa, "wb").write(b">" + first.encode() + b"\n" + inp["ref"][first] + b"\n")
        ctx = phi_amd.Context(0)
        ctx.set_params()
        out = dict(samples=a.samples, contigs=a.contigs, contig_bases=a.contig_bases, text_bytes=len(inp["text"]), vcf_gz_bytes=inp["vcf_bytes"], region=region,
                   region_lines=len(lines), inputs_made_s=made_s, repeats=a.repeats, region_route=[], cut_route=[], whole_file_read_s=[])
        for rep in range(a.repeats + 1):
            t0 = time.perf_counter()
            v = ctx.vcf_graph(inp["vcf"], inp["fa"], region=region, wide=True)
            t1 = time.perf_counter()
            w = ctx.vcf_graph(cut_vcf, cut_fa, wide=True)
            t2 = time.perf_counter()
            assert v.n_records == w.n_records == len(lines) and bytes(v.seq_concat) == bytes(w.seq_concat) and np.array_equal(v.walk_off, w.walk_off)
            if rep:
                out["region_route"].append(dict(v.stats, wall_s=t1 - t0))
                out["cut_route"].append(dict(w.stats, wall_s=t2 - t1))
        for rep in range(min(a.repeats, 2)):                   # (the parent commit's way: minutes at full size, so two runs at most)
            t0 = time.perf_counter()
            whole = H.VcfGraph(inp["vcf"], one_fa)
            out["whole_file_read_s"].append(time.perf_counter() - t0)
            assert whole.n_other_contig > 0
            whole.close()
        out["median"] = dict(region_wall_s=statistics.median(r["wall_s"] for r in out["region_route"]), cut_wall_s=statistics.median(r["wall_s"] for r in out["cut_route"]),
                             whole_file_read_s=statistics.median(out["whole_file_read_s"]))
        ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, default=float)
    print(json.dumps(out["median"]))


if __name__ == "__main__":
    main()
