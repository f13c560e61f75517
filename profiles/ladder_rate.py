"""A 7-level coverage ladder on C3 (49 walks over 5 Mbp, 10x of 150-bp reads): one read set collected, planned and scored band
by band (phi_reads_collect_*, phi_ladder_*; ladder.hip) against the way the job was done before -- seven host-sampled read
sets, each through reset_reads + add_reads + solve.  Writes profiles/ladder_rate.json.

  (i)   collect + plan + 7 x (advance + solve), wall time ending in a device synchronise, with its parts
  (ii)  7 x (reset_reads + add_reads + solve) on read sets sampled on the host by phi_amd/ladder.py's rule BEFORE the clock
        starts (the reference's `seqkit sample` files are not timed either)
  (iii) the plan's GPU time per kernel (events), the copy kernel's GB/s (bytes read + written), and scoring the top level
        once from the planned bands (reset_reads + ladder_advance(top))
(i) and (ii) alternate, --repeats times each after one unrecorded round of both; every level's solve is compared.

    python profiles/ladder_rate.py [--repeats 3] [--config C3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phi_amd                                                  # noqa: E402
from phi_amd import ladder as rule                              # noqa: E402
from phi_amd import synth                                      # noqa: E402

COVERAGES = [0.1, 0.5, 1, 2, 5, 10, 15]            # the reference ladder (data/preprocess.py:83-107); 15x clips to all reads
GENOME = 5_000_000
SEED = 1


def subset(bases, off, keep):
    lens = np.diff(off)[keep]
    new_off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=new_off[1:])
    src = np.repeat(off[:-1][keep] - new_off[:-1], lens) + np.arange(int(new_off[-1]), dtype=np.int64)
    return np.ascontiguousarray(bases[src]), new_off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "ladder_rate.json"))
    a = ap.parse_args()
    gk, rk = synth.CONFIGS[a.config]
    g = synth.make_graph(**gk)
    bases, off, _ = synth.make_reads(g, **rk)
    bases = np.ascontiguousarray(np.frombuffer(bases, np.uint8) if not isinstance(bases, np.ndarray) else bases)
    off = np.ascontiguousarray(off, np.int64)
    n_reads, n_bases = len(off) - 1, int(off[-1])
    fr = rule.fractions_from_coverage(COVERAGES, GENOME, n_bases)
    band = rule.bands(SEED, np.arange(n_reads), fr)
    levels = [subset(bases, off, band <= j) for j in range(len(fr))]
    print(f"{a.config}: {n_reads} reads, {n_bases} bases; fractions {fr}; level reads {[len(o) - 1 for _, o in levels]}", flush=True)

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = phi_amd.Context(0)
    ctx.set_params(k=31, w=25, threshold=1.0, recombination=100)
    ctx.set_stream(stream.cuda_stream)
    A = g.arrays()
    ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])
    torch.cuda.synchronize()

    def run_ladder():
        t = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.reset_reads()
        ctx.collect_begin()
        ctx.add_reads((bases, off))
        ctx.collect_end()
        t1 = time.perf_counter()
        info = ctx.ladder_plan(SEED, fr)
        t2 = time.perf_counter()
        adv = sol = 0.0
        res = []
        for j in range(len(fr)):
            s0 = time.perf_counter()
            ctx.ladder_advance(j)
            s1 = time.perf_counter()
            res.append(ctx.solve())
            s2 = time.perf_counter()
            adv += s1 - s0
            sol += s2 - s1
        torch.cuda.synchronize()
        t["total_s"] = time.perf_counter() - t0
        t.update(collect_s=t1 - t0, plan_s=t2 - t1, advance_s=adv, solve_s=sol)
        return t, info, res

    def run_host_sampled():
        t = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        add = sol = 0.0
        res = []
        for lb, lo in levels:
            s0 = time.perf_counter()
            ctx.reset_reads()
            ctx.add_reads((lb, lo))
            s1 = time.perf_counter()
            res.append(ctx.solve())
            s2 = time.perf_counter()
            add += s1 - s0
            sol += s2 - s1
        torch.cuda.synchronize()
        t["total_s"] = time.perf_counter() - t0
        t.update(add_reads_s=add, solve_s=sol)
        return t, res

    out = {"config": a.config, "n_reads": n_reads, "n_bases": n_bases, "coverages": COVERAGES, "genome_size": GENOME, "seed": SEED,
           "fractions": fr, "level_reads": [len(o) - 1 for _, o in levels], "level_bases": [int(o[-1]) for _, o in levels],
           "bases_scored_host_sampled": int(sum(int(o[-1]) for _, o in levels)), "ladder": [], "host_sampled": [], "plan": []}
    keys = ("objective", "spectrum_size", "filtered", "n_in_model")
    for rep in range(a.repeats + 1):
        tl, info, rl = run_ladder()
        th, rh = run_host_sampled()
        for j, (x, y) in enumerate(zip(rl, rh)):
            assert all(x[k] == y[k] for k in keys) and np.array_equal(x["path_vtx"], y["path_vtx"]), (j, [(x[k], y[k]) for k in keys])
        assert info["band_reads"] == [int((band == j).sum()) for j in range(len(fr))] and info["one_length"] == 150
        if rep == 0:
            continue                                            # (warm-up: first launches, first allocations)
        out["ladder"].append(tl)
        out["host_sampled"].append(th)
        out["plan"].append({k: info[k] for k in ("count_gpu_ms", "scan_gpu_ms", "scatter_gpu_ms", "copy_gpu_ms")})
        print(rep, tl, th, out["plan"][-1], flush=True)
    # scoring the top level once, from the planned bands (no upload) and from the host (with it)
    top = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.reset_reads()
        ctx.ladder_advance(len(fr) - 1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ctx.reset_reads()
        ctx.add_reads(levels[-1])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        top.append({"advance_all_bands_ms": (t1 - t0) * 1e3, "add_reads_with_upload_ms": (t2 - t1) * 1e3})
    out["top_level_score"] = top
    med = lambda rows, k: float(np.median([r[k] for r in rows]))   # noqa: E731
    out["ladder_median_s"] = med(out["ladder"], "total_s")
    out["host_sampled_median_s"] = med(out["host_sampled"], "total_s")
    out["speedup"] = out["host_sampled_median_s"] / out["ladder_median_s"]
    out["ladder_median_parts_s"] = {k: med(out["ladder"], k) for k in ("collect_s", "plan_s", "advance_s", "solve_s")}
    out["host_sampled_median_parts_s"] = {k: med(out["host_sampled"], k) for k in ("add_reads_s", "solve_s")}
    out["plan_median_gpu_ms"] = {k: med(out["plan"], k) for k in out["plan"][0]}
    out["plan_gpu_ms"] = float(sum(out["plan_median_gpu_ms"].values()))
    out["copy_gb_per_s"] = 2.0 * info["n_kept_bases"] / out["plan_median_gpu_ms"]["copy_gpu_ms"] / 1e6
    out["top_level_advance_median_ms"] = med(top, "advance_all_bands_ms")
    out["top_level_add_reads_median_ms"] = med(top, "add_reads_with_upload_ms")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("ladder", "host_sampled", "plan", "top_level_score")}))
    ctx.close()


if __name__ == "__main__":
    main()
