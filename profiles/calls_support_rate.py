"""The read support of every call (phi_calls_support, calls_support.hip; no reference counterpart), on MHC_4
(tests/golden/data, path of the CHM13 reads against walk HG002.1) and on C2 (49 walks, path of its reads against walk 0).
Writes profiles/calls_support_rate.json, everything taken in one run, medians of --repeats runs behind one warm-up:

  (i)   per graph the GPU milliseconds of phi_calls_support by HIP events and its wall time around the call (the copies of the
        four arrays to the host included), the gpu_ms of the phi_calls_path in front of it in the same run, the items, entries
        visited, class records, witnesses and the bytes it moved by DESIGN.md 4.16's own count
  (ii)  the host alternative for the same witnesses: phi_walk_minimizers of the walks the path follows and of the reference walk
        (each a device expansion and a copy to the host) plus the recount in numpy (tests/calls_support_ref.py); alt_n and ref_n
        are compared.  The alternative does not recount the hits -- that would need the hit vector and the minimiser table on
        the host as well -- so its time is a lower bound
  (iii) the wall time of the stage "calls (device) + VCF write" of one `PHI --calls` command on the same input with and
        without --calls-support, and of the stage "calls support (device)", from the [phi timing] marks; the two commands are
        run alternately

    python profiles/calls_support_rate.py [--repeats 5] [--no-cli] [--out FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401  (its HIP runtime initialises first, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import phi_amd                                                  # noqa: E402
from phi_amd import ilp_index as H                              # noqa: E402
from phi_amd import synth                                       # noqa: E402
from calls_support_ref import path_support_ref_numpy            # noqa: E402

PHI = os.path.join(ROOT, "phi_amd", "PHI")
DATA = os.path.join(ROOT, "tests", "golden", "data")
STAGE = re.compile(r"\[phi timing\] main: stage (.+?)\s+[\d.]+ ->\s+[\d.]+ s\s+\(\s*([\d.]+) ms\)")


def median(rows, key):
    return float(np.median([r[key] for r in rows]))


def measure(name, A, reads, ref_walk, repeats):
    ctx = phi_amd.Context(0)
    ctx.set_params(k=31, w=25, threshold=1.0, recombination=100)
    ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])
    ctx.add_reads(reads)
    res = ctx.solve()
    row = {"graph": name, "n_vtx": len(A["seq_off"]) - 1, "n_walks": len(A["walk_off"]) - 1, "ref_walk": ref_walk, "n_path": int(res["n_path"]),
           "recombination_count": int(res["recombination_count"]), "runs": []}
    got = None
    for rep in range(repeats + 1):
        calls = ctx.calls(ref_walk)
        ctx.device_synchronize()
        t0 = time.perf_counter()
        got = ctx.calls_support()
        t1 = time.perf_counter()
        st = ctx.calls_support_stats()
        if rep:                                                 # (the first call is the warm-up)
            row["runs"].append(dict(st, wall_ms=(t1 - t0) * 1e3, calls_path_gpu_ms=calls["gpu_ms"]))
    row["median"] = {key: median(row["runs"], key) for key in ("gpu_ms", "wall_ms", "calls_path_gpu_ms")}
    row.update({key: int(row["runs"][0][key]) for key in ("n_calls", "n_items", "n_visited", "n_records", "n_witnesses", "bytes_moved")})
    row.update({key: int(got[key]) for key in ("alt_hit_total", "alt_n_total", "ref_hit_total", "ref_n_total")})
    row["median"]["gb_per_s_of_counted_bytes"] = row["bytes_moved"] / max(row["median"]["gpu_ms"], 1e-9) / 1e6
    # the host alternative
    woff, wvtx = np.asarray(A["walk_off"]), np.asarray(A["walk_vtx"])
    walks = [wvtx[woff[h]:woff[h + 1]] for h in range(len(woff) - 1)]
    vlen = np.diff(np.asarray(A["seq_off"]))
    alt = []
    for rep in range(repeats + 1):
        ctx.device_synchronize()
        t0 = time.perf_counter()
        mins = {int(h): ctx.walk_minimizers(int(h)) for h in set(res["path_hap"].tolist()) | {ref_walk}}
        t1 = time.perf_counter()
        want = path_support_ref_numpy(31, res["path_vtx"], res["path_hap"], walks, vlen, lambda h: mins[h], ref_walk)
        t2 = time.perf_counter()
        assert np.array_equal(want["alt_n"], got["alt_n"]) and np.array_equal(want["ref_n"], got["ref_n"])
        if rep:
            alt.append({"walk_minimizers_ms": (t1 - t0) * 1e3, "numpy_recount_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3})
    row["alternative"] = {"runs": alt, "walks_expanded": len(mins), "minimizers_copied": int(sum(len(m[0]) for m in mins.values())), "hits_recounted": False,
                          "median": {key: median(alt, key) for key in ("walk_minimizers_ms", "numpy_recount_ms", "total_ms")}}
    ctx.close()
    return row


def cli_stages(args, repeats):
    """the command with and without --calls-support, alternately"""
    runs = {"plain": [], "support": []}
    for rep in range(repeats + 1):
        for which, extra in (("plain", []), ("support", ["--calls-support"])):
            r = subprocess.run([PHI] + args + extra, capture_output=True, text=True, timeout=900, env=dict(os.environ, PHI_TIMING="1"))
            assert r.returncode == 0, r.stderr[-2000:]
            ms = {m.group(1).strip(): float(m.group(2)) for m in STAGE.finditer(r.stderr)}
            if rep:
                runs[which].append({"calls_and_vcf_write_ms": ms["calls (device) + VCF write"], "calls_support_ms": ms.get("calls support (device)", 0.0)})
    return {"runs": runs, "median": {which: {key: median(rows, key) for key in rows[0]} for which, rows in runs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calls_support_rate.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "graphs": []}
    g = H.Graph(os.path.join(DATA, "MHC_4.gfa.gz"))
    A = dict(seq_concat=g.seq_concat, seq_off=g.seq_off, adj_off=g.adj_off, adj=g.adj, walk_off=g.walk_off, walk_vtx=g.walk_vtx, top_rank=g.top_order_map)
    bases, off, _ = H.read_reads(os.path.join(DATA, "CHM13_reads.fq.gz"))
    out["graphs"].append(measure("MHC_4", A, (bases, off), g.hap_id2name.index("HG002.1"), a.repeats))
    print(json.dumps(out["graphs"][-1]["median"]), json.dumps(out["graphs"][-1]["alternative"]["median"]), flush=True)
    gk, rk = synth.CONFIGS["C2"]
    s = synth.make_graph(**gk)
    sb, so, _ = synth.make_reads(s, **rk)
    out["graphs"].append(measure("C2", s.arrays(), (sb, so), 0, a.repeats))
    print(json.dumps(out["graphs"][-1]["median"]), json.dumps(out["graphs"][-1]["alternative"]["median"]), flush=True)
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as d:
            out["graphs"][0]["cli"] = cli_stages(["-g", os.path.join(DATA, "MHC_4.gfa.gz"), "-r", os.path.join(DATA, "CHM13_reads.fq.gz"), "-o", os.path.join(d, "m.fa"),
                                                  "--calls", os.path.join(d, "m.vcf"), "--calls-ref", "HG002.1"], a.repeats)
            gfa, rd = os.path.join(d, "c2.gfa"), os.path.join(d, "c2_reads.fa")
            synth.write_gfa(s, gfa)
            synth.write_reads(sb, so, rd)
            out["graphs"][1]["cli"] = cli_stages(["-g", gfa, "-r", rd, "-o", os.path.join(d, "c.fa"), "--calls", os.path.join(d, "c.vcf"), "--calls-ref", s.hap_names[0]],
                                                 a.repeats)
        print(json.dumps([x["cli"]["median"] for x in out["graphs"]]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
