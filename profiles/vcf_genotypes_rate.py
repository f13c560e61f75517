"""The genotype kernels of the VCF route (phi_vcf_genotypes, vcf.hip) on their own: the population-style VCF of
profiles/vcf_region_rate.py with one contig, read whole (no region), so that every record's sample columns go through the
summary / carry / parse kernels; genotype_gpu_ms of phi_vcf_stats is the three kernels between two events.  Run by hand on the
MI355X, alone or under `rocprofv3 --kernel-trace --stats -- python3 profiles/vcf_genotypes_rate.py` for the vcf_* kernels one
by one; writes profiles/vcf_genotypes_rate.json.

    python profiles/vcf_genotypes_rate.py [--samples 1000] [--contig-bases 1000000] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch  # noqa: F401  (its HIP runtime initialises first, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import phi_amd                                                  # noqa: E402
from vcf_region_rate import make_inputs                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--contig-bases", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_genotypes_rate.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        inp = make_inputs(tmp, a.samples, 1, a.contig_bases)
        name = inp["names"][0]
        fa = os.path.join(tmp, "one.fa")
        open(fa, "wb").write(b">" + name.encode() + b"\n" + inp["ref"][name] + b"\n")
        ctx = phi_amd.Context(0)
        ctx.set_params()
        runs = []
        for rep in range(a.repeats + 1):
            t0 = time.perf_counter()
            v = ctx.vcf_graph(inp["vcf"], fa, wide=True)
            dt = time.perf_counter() - t0
            st = ctx.vcf_stats()
            assert v.n_records == len(inp["recs"][name]) and st["n_samples"] == a.samples
            if rep:                                             # (the first turn is the warm-up)
                runs.append({"wall_s": dt, "genotype_gpu_ms": st["genotype_gpu_ms"], "text_bytes": st["text_bytes"], "n_flagged": st["n_flagged"]})
        ctx.close()
    ms = statistics.median(r["genotype_gpu_ms"] for r in runs)
    out = {"device": torch.cuda.get_device_name(0), "samples": a.samples, "records": len(inp["recs"][name]), "vcf_text_bytes": len(inp["text"]), "runs": runs,
           "median_genotype_gpu_ms": ms, "median_genotype_text_gb_per_s": runs[0]["text_bytes"] / ms / 1e6}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, default=float)
        f.write("\n")
    print(json.dumps(out, default=float))


if __name__ == "__main__":
    main()
