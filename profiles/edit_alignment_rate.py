#!/usr/bin/env python3
"""Rate of phi_edit_alignments at the reference harness' scale; prints one JSON line.

The workloads of profiles/edit_distance_rate.py (the same seeds): the MHC-CHM13 truth (4.92 Mbp) against copies with
2 x 10^4 planted single-base edits,
  (a) one pair;
  (b) 245 such pairs in one call (the 49 x 5 matrix of data/get_edit_stats.sh).
The distances come from phi_edit_distances first (not timed); then per case: seconds per phi_edit_alignments call with
the CIGARs (host clock around the synchronous call, median of --reps after a warm-up), the checkpoint bytes per pair
(the formula of edit_path.hip), and, with --stats-csv (the kernel_stats.csv of a separate `rocprofv3 --kernel-trace
--stats` run of `--case a` / `--case b`), the summed time of the checkpoint, recompute and walk kernels.

    python profiles/edit_alignment_rate.py [--case a|b|both] [--reps 3] [--stats-csv a.csv,b.csv]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

KERNELS = {"checkpoint": "phi_edit_ckpt_kernel", "recompute": "phi_edit_rows_kernel", "walk": "phi_edit_walk_kernel",
           "distance": "phi_edit_band_kernel"}


def checkpoint_bytes(la, lb, d):
    """bytes of checkpoints of one pair (edit_path.hip): per 64-row block of the shorter sequence its band's deltas
    at 2 bits a column (+ one word) and one top value; the stripes' row of deltas"""
    m, n = min(la, lb), max(la, lb)
    delta = n - m
    e = max(1, (d - delta) // 2)
    width = min(n, 64 + delta + 2 * e)
    nb = (m + 63) // 64
    return 4 * (nb * ((width + 15) // 16 + 1) + nb + n // 16 + 2)


def kernel_ms(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for key, name in KERNELS.items():
                if name in row.get("Name", ""):
                    out[key + "_ms"] = round(float(row["TotalDurationNs"]) / 1e6, 3)
                    out[key + "_calls"] = int(row["Calls"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="both", choices=["a", "b", "both"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats-csv", default="")
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    from edit_distance_rate import planted
    from phi_amd.eval_log import read_fasta
    import phi_amd
    truth = read_fasta(os.path.join(ROOT, "tests", "golden", "data", "MHC-CHM13.0.fa.gz"))
    ctx = phi_amd.Context(0)
    res = {"truth_bases": len(truth), "edits_planted": 20000, "seed": args.seed, "timer": "host clock around the synchronous call"}
    stats = dict(zip(["a", "b"], args.stats_csv.split(","))) if args.stats_csv else {}
    for case in (["a", "b"] if args.case == "both" else [args.case]):
        n_pairs = 1 if case == "a" else 245
        queries = [planted(truth, 20000, args.seed + i) for i in range(n_pairs)]
        a_list = [truth] * n_pairs
        d = ctx.edit_distances(a_list, queries)
        first = ctx.edit_alignments(a_list, queries, dist=d)                      # warm-up
        times = []
        for _ in range(args.reps):
            t = time.perf_counter()
            again = ctx.edit_alignments(a_list, queries, dist=d)
            times.append(time.perf_counter() - t)
            assert again.cigar == first.cigar
        ck = [checkpoint_bytes(len(truth), len(q), int(x)) for q, x in zip(queries, d)]
        r = {"pairs": n_pairs, "s_per_call_median": round(statistics.median(times), 4), "s_per_call_all": [round(x, 4) for x in times],
             "distance_min": int(d.min()), "distance_max": int(d.max()),
             "identity_min": round(float(first.identity.min()), 4), "identity_max": round(float(first.identity.max()), 4),
             "cigar_bytes_max": max(len(c) for c in first.cigar),
             "checkpoint_bytes_per_pair_max": max(ck), "checkpoint_bytes_total": sum(ck)}
        if case in stats and os.path.exists(stats[case]):
            r.update(kernel_ms(stats[case]))
        res[case] = r
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
