"""Panels of the C2 graph (49 walks, one sample each) with nested panels of 3, 7, 13 and 25 walks (phi_set_graph_panel, panel.hip;
the reference: data/chop_graph.sh:46-66, data/run_batch_9.py to run_batch_13.py).  Writes profiles/panel_rate.json.

  (i)   per panel the GPU milliseconds of mark, scan and remap (HIP events on the context's stream, phi_panel_stats) and their
        GB/s -- mark: 4 B read per kept entry; remap: 4 B read + 4 B written per kept entry; gathers not counted --, beside
        the chop's count + scan + expand (phi_chop_stats, N = 15 on the whole graph: 4 B read per entry + 4 B written per piece)
  (ii)  the host seconds of the array reduction and of Kahn (phi_panel_stats)
  (iii) whole set-graph seconds: set_graph(keep=mask) against the only way there was before -- induced_subgraph in numpy
        (phi_amd/panel.py) plus plain set_graph, the preparation included; the two results are compared
  (iv)  `PHI --panels 3,7,13,25` in one command against four plain commands on reduced GFA files (written before the clock
        starts), spawn to exit, as bench.py defines end_to_end_one_process_s; the FASTA files are compared

    python profiles/panel_rate.py [--repeats 3] [--no-cli]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import phi_amd                                                  # noqa: E402
from phi_amd import panel as rule                               # noqa: E402
from phi_amd import synth                                       # noqa: E402

SIZES = [3, 7, 13, 25]
SEED = 1
PHI = os.path.join(ROOT, "phi_amd", "PHI")


def set_arrays(ctx, A, **kw):
    return ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A.get("top_rank"), **kw)


def sub_graph(g, S, kept):
    s = synth.SynGraph()
    s.seq_concat = np.frombuffer(S["seq_concat"], np.uint8)
    s.seq_off, s.adj_off, s.adj, s.walk_off, s.walk_vtx, s.top_rank = S["seq_off"], S["adj_off"], S["adj"], S["walk_off"], S["walk_vtx"], S["top_rank"]
    s.n_vtx, s.n_walks = len(s.seq_off) - 1, len(kept)
    s.hap_names = [g.hap_names[h] for h in kept.tolist()]
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_rate.json"))
    a = ap.parse_args()
    gk, rk = synth.CONFIGS["C2"]
    g = synth.make_graph(**gk)
    bases, off, _ = synth.make_reads(g, **rk)
    A = g.arrays()
    samples = rule.samples_in_order(g.hap_names)
    panels = rule.nested_panels(samples, SIZES, SEED)
    masks = [rule.keep_mask(g.hap_names, keep_samples=p) for p in panels]
    assert [int(m.sum()) for m in masks] == SIZES
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    out = {"config": "C2", "n_walks": g.n_walks, "n_vtx": g.n_vtx, "n_entries": int(A["walk_off"][-1]), "sizes": SIZES, "seed": SEED, "panels": []}

    def fresh():
        ctx = phi_amd.Context(0)
        ctx.set_params(k=31, w=25, threshold=1.0, recombination=100)
        ctx.set_stream(stream.cuda_stream)
        return ctx
    for n, m in zip(SIZES, masks):
        row = {"walks": n, "device": [], "numpy": []}
        for rep in range(a.repeats + 1):
            ctx = fresh()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            set_arrays(ctx, A, keep=m)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ps = ctx.panel_stats()
            ent = ctx.walk_entries()
            ctx.close()
            ctx = fresh()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            S, origin, kept = rule.induced_arrays(A, m)
            t3 = time.perf_counter()
            set_arrays(ctx, S)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            assert np.array_equal(ent, ctx.walk_entries()) and ps["n_vtx_out"] == len(origin)
            ctx.close()
            if rep == 0:
                continue                                            # (warm-up)
            k = ps["n_entries_out"]
            ps.update(set_graph_panel_s=t1 - t0, mark_gbps=4 * k / ps["mark_gpu_ms"] / 1e6, remap_gbps=8 * k / ps["remap_gpu_ms"] / 1e6)
            row["device"].append(ps)
            row["numpy"].append({"induced_subgraph_s": t3 - t2, "set_graph_s": t4 - t3, "total_s": t4 - t2})
        med = lambda rows, key: float(np.median([r[key] for r in rows]))   # noqa: E731
        row["median"] = {key: med(row["device"], key) for key in ("mark_gpu_ms", "scan_gpu_ms", "remap_gpu_ms", "mark_gbps", "remap_gbps", "reduce_host_s",
                                                                  "kahn_host_s", "set_graph_panel_s")}
        row["median"].update({"numpy_" + key: med(row["numpy"], key) for key in ("induced_subgraph_s", "set_graph_s", "total_s")})
        row["median"].update({key: row["device"][0][key] for key in ("n_vtx_out", "n_edges_out", "n_entries_out")})
        out["panels"].append(row)
        print(n, row["median"], flush=True)
    # the chop's expansion of the whole graph's entries, for scale
    ctx = fresh()
    set_arrays(ctx, A, chop=15)
    torch.cuda.synchronize()
    cs = ctx.chop_stats()
    ctx.close()
    cs["gbps"] = 4 * (cs["n_entries_in"] + cs["n_entries_out"]) / cs["expand_gpu_ms"] / 1e6
    out["chop_15"] = cs
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as d:
            os.makedirs(os.path.join(d, "full"))
            full = os.path.join(d, "full", "g.gfa")
            synth.write_gfa(g, full)
            rd = os.path.join(d, "reads.fa")
            synth.write_reads(bases, off, rd)
            reduced = []
            for n, m in zip(SIZES, masks):
                S, origin, kept = rule.induced_arrays(A, m)
                os.makedirs(os.path.join(d, f"p{n}"))
                reduced.append(os.path.join(d, f"p{n}", "g.gfa"))
                synth.write_gfa(sub_graph(g, S, kept), reduced[-1])
            cli = {"panels_one_command_s": [], "four_commands_s": []}
            for rep in range(a.repeats + 1):
                t0 = time.perf_counter()
                r = subprocess.run([PHI, "--panels", ",".join(str(n) for n in SIZES), "--panel-seed", str(SEED), "-g", full, "-r", rd, "-o", os.path.join(d, "o.{panel}.fa")],
                                   capture_output=True, text=True, timeout=600)
                t1 = time.perf_counter()
                assert r.returncode == 0, r.stderr[-2000:]
                for n, path in zip(SIZES, reduced):
                    r = subprocess.run([PHI, "-g", path, "-r", rd, "-o", os.path.join(d, f"q.{n}.fa")], capture_output=True, text=True, timeout=600)
                    assert r.returncode == 0, r.stderr[-2000:]
                t2 = time.perf_counter()
                for n in SIZES:
                    assert open(os.path.join(d, f"o.{n}.fa"), "rb").read() == open(os.path.join(d, f"q.{n}.fa"), "rb").read(), n
                if rep:
                    cli["panels_one_command_s"].append(t1 - t0)
                    cli["four_commands_s"].append(t2 - t1)
            cli["panels_one_command_median_s"] = float(np.median(cli["panels_one_command_s"]))
            cli["four_commands_median_s"] = float(np.median(cli["four_commands_s"]))
            cli["speedup"] = cli["four_commands_median_s"] / cli["panels_one_command_median_s"]
            out["cli"] = cli
            print(cli, flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
