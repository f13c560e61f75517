#!/usr/bin/env python3
"""The VCF route measured: a synthetic phased VCF + reference FASTA to "set graph" done,
  baseline   `python -m phi_amd.vcf2gfa` to a GFA file, then the GFA stage (host reader) and set_graph, the only route before
  new        Context.set_graph_vcf: host read, genotype kernel, host build, walk kernels, set_graph
on point 1 (5 Mbp, 20 diploid samples, 50 000 records), where the arrays of the two routes are compared; and the new route
alone on point 2 (50 Mbp, 100 samples, 500 000 records).  Writes profiles/vcf_route_rate.json.  The input is generated here
(fixed seed): SNVs, short indels, some multi-allelic records, some overlapping ones.

    python profiles/vcf_route.py [--out profiles/vcf_route_rate.json] [--skip-large]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_input(d, name, ref_len, n_samples, n_records, seed):
    rng = np.random.default_rng(seed)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=ref_len)
    fa = os.path.join(d, name + ".fa")
    with open(fa, "wb") as f:
        f.write(b">chr1\n")
        lines = ref[:ref_len // 60 * 60].reshape(-1, 60)
        f.write(b"\n".join(r.tobytes() for r in lines) + b"\n" + ref[ref_len // 60 * 60:].tobytes() + b"\n")
    raw = ref.tobytes()
    pos = np.sort(rng.choice(np.arange(10, ref_len - 100), size=n_records, replace=False))
    # some records overlap the one before: moved to within its span
    close = rng.random(n_records) < 0.03
    pos[1:][close[1:]] = pos[:-1][close[1:]] + rng.integers(0, 3, size=int(close[1:].sum()))
    pos.sort()
    kind = rng.random(n_records)
    n_alt = np.where(rng.random(n_records) < 0.08, 2, 1)
    gt = rng.random((n_records, n_samples, 2)) < 0.12
    al = rng.integers(1, 3, size=(n_records, n_samples, 2))
    vcf = os.path.join(d, name + ".vcf")
    with open(vcf, "wb") as f:
        f.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + b"\t".join(b"S%d" % i for i in range(n_samples)) + b"\n")
        out = []
        for i in range(n_records):
            p = int(pos[i])
            if kind[i] < 0.8:                                  # SNV
                r = raw[p:p + 1]
                alts = [bytes([c]) for c in b"ACGT" if c != r[0]][:int(n_alt[i])]
            elif kind[i] < 0.9:                                # deletion
                r = raw[p:p + 1 + int(rng.integers(1, 12))]
                alts = [r[:1], r[:2]][:int(n_alt[i])] if len(r) > 2 else [r[:1]]
            else:                                              # insertion
                r = raw[p:p + 1]
                alts = [r + bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(1, 12))).tolist()) for _ in range(int(n_alt[i]))]
                alts = list(dict.fromkeys(alts))
            a = np.where(gt[i], np.minimum(al[i], len(alts)), 0)
            cols = b"\t".join(b"%d|%d" % (x, y) for x, y in a.tolist())
            out.append(b"chr1\t%d\t.\t%s\t%s\t60\tPASS\t.\tGT\t%s\n" % (p + 1, r, b",".join(alts), cols))
            if len(out) >= 20000:
                f.write(b"".join(out)); out = []
        f.write(b"".join(out))
    return vcf, fa


def new_route(vcf, fa):
    import phi_amd
    ctx = phi_amd.Context(0)
    ctx.set_params()
    ctx.device_synchronize()
    t0 = time.perf_counter()
    v = ctx.set_graph_vcf(vcf, fa)
    ctx.device_synchronize()
    total = time.perf_counter() - t0
    st = v.stats
    res = dict(total_s=total, read_s=st["read_s"], genotypes_s=st["genotypes_s"], genotype_gpu_ms=st["genotype_gpu_ms"],
               genotype_text_bytes=st["text_bytes"], genotype_text_gb_per_s=st["text_bytes"] / (st["genotype_gpu_ms"] * 1e-3) / 1e9,
               genotype_algorithmic_gb_per_s=(st["text_bytes"] + 4 * st["n_records"] * st["n_samples"]) / (st["genotype_gpu_ms"] * 1e-3) / 1e9,
               build_s=st["build_s"], walks_s=st["walks_s"], walks_gpu_ms=st["walks_gpu_ms"], n_entries=st["n_entries"],
               entries_gb_per_s=4 * st["n_entries"] / (st["walks_gpu_ms"] * 1e-3) / 1e9, set_graph_s=st["set_graph_s"],
               n_records=st["n_records"], n_samples=st["n_samples"], n_flagged=st["n_flagged"], n_units=st["n_units"], n_vtx=v.n_vtx, n_walks=v.num_walks)
    return ctx, v, res


def baseline(vcf, fa, d):
    import phi_amd
    from phi_amd import ilp_index as H
    gfa = os.path.join(d, "baseline.gfa")
    t0 = time.perf_counter()
    with open(gfa, "wb") as f:
        subprocess.check_call([sys.executable, "-m", "phi_amd.vcf2gfa", "-v", vcf, "-r", fa], stdout=f, cwd=ROOT)
    t1 = time.perf_counter()
    ctx = phi_amd.Context(0)
    ctx.set_params()
    ctx.device_synchronize()
    t2 = time.perf_counter()
    g = H.Graph(gfa)
    t3 = time.perf_counter()
    ctx.set_graph(g.seq_concat, g.seq_off, g.adj_off, g.adj, g.walk_off, g.walk_vtx, g.top_order_map)
    ctx.device_synchronize()
    t4 = time.perf_counter()
    ctx.close()
    return g, dict(total_s=(t1 - t0) + (t4 - t2), vcf2gfa_s=t1 - t0, gfa_read_s=t3 - t2, set_graph_s=t4 - t3, gfa_bytes=os.path.getsize(gfa))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_route_rate.json"))
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.ensure_built()
    out = {"hbm_peak_gb_per_s": 8000.0}
    with tempfile.TemporaryDirectory() as d:
        vcf, fa = write_input(d, "p1", 5_000_000, 20, 50_000, seed=1)
        ctx, v, res = new_route(vcf, fa)                        # (first: the contexts of both routes start warm alike, each made before its clock)
        ctx.close()
        ctx, v, res = new_route(vcf, fa)
        g, base = baseline(vcf, fa, d)
        same = all(np.array_equal(getattr(v, f), getattr(g, f)) for f in ("seq_off", "seq_concat", "adj_off", "adj", "walk_off", "top_order_map"))
        same = same and v.hap_id2name == g.hap_id2name and np.array_equal(ctx.walk_entries(), g.walk_vtx)
        ctx.close()
        out["point1"] = dict(ref_bases=5_000_000, samples=20, records=50_000, vcf_bytes=os.path.getsize(vcf), gfa_bytes=base["gfa_bytes"],
                             baseline=base, new=res, arrays_equal=bool(same), speedup=base["total_s"] / res["total_s"])
        print(json.dumps(out["point1"]), flush=True)
        ok = same and res["total_s"] < base["total_s"]
        if not args.skip_large:
            vcf, fa = write_input(d, "p2", 50_000_000, 100, 500_000, seed=2)
            ctx, v, res = new_route(vcf, fa)
            ctx.close()
            out["point2"] = dict(ref_bases=50_000_000, samples=100, records=500_000, vcf_bytes=os.path.getsize(vcf), new=res)
            print(json.dumps(out["point2"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not ok:
        print("FAILED: arrays_equal=%s, new %.3f s against baseline %.3f s" % (same, out["point1"]["new"]["total_s"], out["point1"]["baseline"]["total_s"]))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
