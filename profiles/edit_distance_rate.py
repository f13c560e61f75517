#!/usr/bin/env python3
"""Rate of phi_edit_distances at the reference harness' scale; prints one JSON line.

Inputs from a seed: the MHC-CHM13 truth (4.92 Mbp) against copies of it with planted edits (single-base
substitutions, insertions and deletions at uniform positions):
  (a) one pair at 2 x 10^4 edits;
  (b) 245 such pairs (each its own seed) in one call: the 49 x 5 matrix of data/get_edit_stats.sh.
For each: seconds per call (host clock around the synchronous call, median of 5 after a warm-up), and the final band's
block updates per second (columns x 64-row blocks of the band that proved the distance: the least work the banded
algorithm does; failed narrower passes come on top).  With --stats-csv (the kernel_stats.csv of a separate
`rocprofv3 --kernel-trace --stats` run of `--case a` / `--case b`) the edit kernel's summed time is added.  For (a) the
O(ND) test reference (tests/edit_ref.c) is timed on the same pair.

    python profiles/edit_distance_rate.py [--case a|b|both] [--reps 5] [--stats-csv a.csv,b.csv]
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def planted(truth, n_edits, seed):
    """truth with n_edits single-base edits at sorted uniform positions: 1/2 substitutions, 1/4 insertions, 1/4 deletions"""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(len(truth) - 20, n_edits, replace=False))
    kind = rng.integers(0, 4, n_edits)
    bases = np.frombuffer(b"ACGT", np.uint8)
    out, last = [], 0
    for p, k in zip(pos.tolist(), kind.tolist()):
        if p < last:
            continue
        out.append(truth[last:p])
        if k <= 1:                                        # substitution
            c = truth[p]
            out.append(bytes([bases[(int(np.where(bases == c)[0][0]) + 1) % 4] if c in b"ACGT" else 65]))
            last = p + 1
        elif k == 2:                                      # insertion
            out.append(bases[rng.integers(0, 4, 1)].tobytes())
            last = p
        else:                                             # deletion
            last = p + 1
    out.append(truth[last:])
    return b"".join(out)


def band_updates(n, m, d):
    """columns x blocks of the first doubled band that holds d (k = max(64, |n - m| + 64) * 2^i >= d)"""
    delta = abs(n - m)
    k = max(64, delta + 64)
    while k < d:
        k *= 2
    e = max(1, (k - delta) // 2)
    return max(n, m) * min((delta + 2 * e + 63) // 64 + 1, (min(n, m) + 63) // 64)


def kernel_ms(path):
    with open(path) as f:
        for row in csv.DictReader(f):
            if "phi_edit_band_kernel" in row.get("Name", ""):
                return float(row["TotalDurationNs"]) / 1e6, int(row["Calls"])
    return None, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="both", choices=["a", "b", "both"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stats-csv", default="")
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    from phi_amd.eval_log import read_fasta
    import phi_amd
    truth = read_fasta(os.path.join(ROOT, "tests", "golden", "data", "MHC-CHM13.0.fa.gz"))
    ctx = phi_amd.Context(0)
    res = {"truth_bases": len(truth), "edits_planted": 20000, "seed": args.seed, "timer": "host clock around the synchronous call"}
    stats = dict(zip(["a", "b"], args.stats_csv.split(","))) if args.stats_csv else {}
    cases = ["a", "b"] if args.case == "both" else [args.case]
    for case in cases:
        n_pairs = 1 if case == "a" else 245
        queries = [planted(truth, 20000, args.seed + i) for i in range(n_pairs)]
        a_list = [truth] * n_pairs
        d = ctx.edit_distances(a_list, queries)          # warm-up
        times = []
        for _ in range(args.reps):
            t = time.perf_counter()
            again = ctx.edit_distances(a_list, queries)
            times.append(time.perf_counter() - t)
            assert np.array_equal(again, d)
        sec = statistics.median(times)
        upd = sum(band_updates(len(truth), len(q), int(x)) for q, x in zip(queries, d))
        r = {"pairs": n_pairs, "s_per_call_median": round(sec, 4), "s_per_call_all": [round(x, 4) for x in times],
             "distance_min": int(d.min()), "distance_max": int(d.max()),
             "final_band_block_updates": upd, "final_band_block_updates_per_s": round(upd / sec, 0)}
        if case in stats and os.path.exists(stats[case]):
            ms, calls = kernel_ms(stats[case])
            r["rocprof_kernel_ms_total"] = ms
            r["rocprof_kernel_calls"] = calls
        if case == "a":
            with tempfile.TemporaryDirectory() as tmp:
                so = os.path.join(tmp, "libedit_ref.so")
                subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "edit_ref.c")])
                import ctypes as C
                L = C.CDLL(so)
                L.ond_edit_distance.restype = C.c_int64
                L.ond_edit_distance.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.c_int64]
                t = time.perf_counter()
                ref = L.ond_edit_distance(truth, len(truth), queries[0], len(queries[0]), -1)
                r["cpu_ond_reference_s"] = round(time.perf_counter() - t, 3)
                assert ref == int(d[0]), (ref, int(d[0]))
        res[case] = r
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
