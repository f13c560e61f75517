"""The inferred path written as variant calls against a reference walk (phi_calls_path, calls.hip; no reference
counterpart), on MHC_4 (tests/golden/data, path of the CHM13 reads against walk HG002.1) and on C2 (49 walks,
path of its reads against walk 0).  Writes profiles/calls_rate.json, everything taken in one run:

  (i)   per graph the GPU milliseconds of phi_calls_path by HIP events (gpu_ms of phi_calls, and per stage from
        phi_calls_stats), its wall time around the call (copies to the host included), and the bytes it moved by DESIGN.md
        4.16's own count (bytes_moved of phi_calls_stats)
  (ii)  the wall time of the stages "FASTA write" and "calls (device) + VCF write" of one `PHI --calls` command on the same
        input, from its [phi timing] marks
  (iii) for the same C2 call the alternative it replaces: a device-to-host copy of the walk entries (phi_walk_entries: the
        accessor copies them all, the reference walk's among them) plus the rule restated in numpy (tests/calls_ref.py); the
        two results are compared

    python profiles/calls_rate.py [--repeats 5] [--no-cli] [--out FILE]
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
from calls_ref import calls_ref_numpy, digest                   # noqa: E402

PHI = os.path.join(ROOT, "phi_amd", "PHI")
DATA = os.path.join(ROOT, "tests", "golden", "data")
STAGE = re.compile(r"\[phi timing\] main: stage (.+?)\s+[\d.]+ ->\s+[\d.]+ s\s+\(\s*([\d.]+) ms\)")


def measure(name, A, reads, ref_walk, repeats, alternative):
    ctx = phi_amd.Context(0)
    ctx.set_params(k=31, w=25, threshold=1.0, recombination=100)
    ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])
    ctx.add_reads(reads)
    res = ctx.solve()
    row = {"graph": name, "n_vtx": len(A["seq_off"]) - 1, "n_walks": len(A["walk_off"]) - 1, "ref_walk": ref_walk, "n_path": int(res["n_path"]),
           "recombination_count": int(res["recombination_count"]), "runs": []}
    got = None
    for rep in range(repeats + 1):
        ctx.device_synchronize()
        t0 = time.perf_counter()
        got = ctx.calls(ref_walk)
        t1 = time.perf_counter()
        st = ctx.calls_stats()
        if rep:                                                 # (the first call is the warm-up)
            row["runs"].append(dict(st, wall_ms=(t1 - t0) * 1e3))
    med = lambda key: float(np.median([r[key] for r in row["runs"]]))   # noqa: E731
    row["median"] = {key: med(key) for key in ("gpu_ms", "table_gpu_ms", "shared_gpu_ms", "pairs_gpu_ms", "fill_gpu_ms", "wall_ms")}
    row.update({key: int(row["runs"][0][key]) for key in ("n_query", "n_ref", "n_shared", "n_calls", "ref_bytes", "alt_bytes", "bytes_moved")})
    row["median"]["gb_per_s_of_counted_bytes"] = row["bytes_moved"] / row["median"]["gpu_ms"] / 1e6
    if alternative:
        alt = []
        for rep in range(repeats + 1):
            ctx.device_synchronize()
            t0 = time.perf_counter()
            ent = ctx.walk_entries()
            t1 = time.perf_counter()
            woff = A["walk_off"]
            want = calls_ref_numpy(res["path_vtx"], ent[woff[ref_walk]:woff[ref_walk + 1]], np.asarray(A["seq_off"]), bytes(A["seq_concat"]))
            t2 = time.perf_counter()
            assert digest(want) == digest(got)
            if rep:
                alt.append({"entries_d2h_ms": (t1 - t0) * 1e3, "numpy_rule_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3})
        row["alternative"] = {"runs": alt, "entries_copied": int(len(ent)),
                              "median": {key: float(np.median([r[key] for r in alt])) for key in ("entries_d2h_ms", "numpy_rule_ms", "total_ms")}}
    ctx.close()
    return row


def cli_stages(args):
    r = subprocess.run([PHI] + args, capture_output=True, text=True, timeout=900, env=dict(os.environ, PHI_TIMING="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    ms = {m.group(1).strip(): float(m.group(2)) for m in STAGE.finditer(r.stderr)}
    return {"fasta_write_ms": ms["FASTA write"], "calls_and_vcf_write_ms": ms["calls (device) + VCF write"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calls_rate.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "graphs": []}
    g = H.Graph(os.path.join(DATA, "MHC_4.gfa.gz"))
    A = dict(seq_concat=g.seq_concat, seq_off=g.seq_off, adj_off=g.adj_off, adj=g.adj, walk_off=g.walk_off, walk_vtx=g.walk_vtx, top_rank=g.top_order_map)
    bases, off, _ = H.read_reads(os.path.join(DATA, "CHM13_reads.fq.gz"))
    out["graphs"].append(measure("MHC_4", A, (bases, off), g.hap_id2name.index("HG002.1"), a.repeats, False))
    print(json.dumps(out["graphs"][-1]["median"]), flush=True)
    gk, rk = synth.CONFIGS["C2"]
    s = synth.make_graph(**gk)
    sb, so, _ = synth.make_reads(s, **rk)
    out["graphs"].append(measure("C2", s.arrays(), (sb, so), 0, a.repeats, True))
    print(json.dumps(out["graphs"][-1]["median"]), json.dumps(out["graphs"][-1]["alternative"]["median"]), flush=True)
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as d:
            out["graphs"][0]["cli"] = cli_stages(["-g", os.path.join(DATA, "MHC_4.gfa.gz"), "-r", os.path.join(DATA, "CHM13_reads.fq.gz"), "-o", os.path.join(d, "m.fa"),
                                                  "--calls", os.path.join(d, "m.vcf"), "--calls-ref", "HG002.1"])
            gfa, rd = os.path.join(d, "c2.gfa"), os.path.join(d, "c2_reads.fa")
            synth.write_gfa(s, gfa)
            synth.write_reads(sb, so, rd)
            out["graphs"][1]["cli"] = cli_stages(["-g", gfa, "-r", rd, "-o", os.path.join(d, "c.fa"), "--calls", os.path.join(d, "c.vcf"), "--calls-ref", s.hap_names[0]])
        print(json.dumps([x["cli"] for x in out["graphs"]]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
