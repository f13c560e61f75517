"""The panel chosen from the reads (phi_scout_graph, phi_scout_scores, phi_scout_choose) on a native-generator
graph of 2 000 walks over 5 Mbp with reads at C3's coverage (10x, 150 bp).  Writes profiles/panel_auto_rate.json.  Not a test.

  (i)   the three passes of phi_scout_scores by HIP events (phi_scout_info), the entry pass beside phi_walk_sum_kernel<true>
        over the same entries in the same call (PHI_SCOUT_REF): both read 4 B per walk entry plus a per-class gather; the
        score pass has the per-(walk, block) flushes on top and is given up to twice that time
  (ii)  the seconds of phi_scout_graph beside phi_index_stats' GPU milliseconds, and the host seconds of the choice
        (phi_scout_choose: the matrix' copy + phi_panel_choose)
  (iii) --cli: `PHI --panel-auto N` end to end against `PHI --keep-samples <the chosen set>` on the same files, spawn to exit:
        the difference is the price of the scout

Every GPU step is a child process under a time limit of its own; a step that fails or runs out of time ends the script.

    python profiles/panel_auto_rate.py [--walks 2000] [--backbone 5000000] [--want 200] [--repeats 3] [--cli]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PHI = os.path.join(ROOT, "phi_amd", "PHI")


def make(a):
    from phi_amd import synth
    g = synth.NativeGraph(backbone_len=a.backbone, n_walks=a.walks, seed=20001)
    truth = g.sample(4901, 3)
    n = g.n_reads(10.0)
    return g, truth, n


def step_kernels(a):
    """(i) and (ii), in this process"""
    import numpy as np
    import torch                                                # noqa: F401  (its HIP runtime first, as bench.py has it)
    import phi_amd
    os.environ["PHI_SCOUT_REF"] = "1"
    t0 = time.perf_counter()
    g, truth, n_reads = make(a)
    bases, off = g.reads(4903, 0, n_reads)
    gen_s = time.perf_counter() - t0
    ctx = phi_amd.Context(0)
    ctx.set_params()
    out = dict(n_walks=g.n_walks, n_vtx=g.n_vtx, n_entries=int(g.walk_off[-1]), n_reads=int(n_reads), generate_s=gen_s, truth_walks=truth["walks"], runs=[])
    for rep in range(a.repeats):
        t0 = time.perf_counter()
        ctx.scout_graph(g.seq_concat, g.seq_off, g.adj_off, g.adj, g.walk_off, g.walk_vtx if rep == 0 else None, g.top_rank)
        scout_s = time.perf_counter() - t0
        st = ctx.index_stats()
        t0 = time.perf_counter()
        ctx.collect_reads((bases, off))
        ctx.collect_score()
        reads_s = time.perf_counter() - t0
        _, info = ctx.scout_scores(a.blocks, copy=False)
        t0 = time.perf_counter()
        keep, round_of = ctx.scout_choose(a.want)
        choose_s = time.perf_counter() - t0
        entered = round_of[(round_of >= 0) & (round_of < len(round_of))]
        out["runs"].append(dict(scout_graph_s=scout_s, from_retained_entries=rep > 0, index_gpu_ms=st["sketch_gpu_ms"], n_classes=st["n_classes"],
                                collect_and_score_s=reads_s, choose_host_s=choose_s, rounds=int(entered.max()) + 1 if len(entered) else 0,
                                truth_walks_round=[int(round_of[h]) for h in truth["walks"]],
                                entry_over_walk_sum=info["entry_gpu_ms"] / info["walk_sum_gpu_ms"] if info["walk_sum_gpu_ms"] else None,
                                entry_gbps_4B_per_entry=4e-6 * out["n_entries"] / info["entry_gpu_ms"] if info["entry_gpu_ms"] else None, **info))
    out["kept"] = [g.hap_names[h] for h in np.flatnonzero(keep).tolist()]
    ctx.close()
    print(json.dumps(out))


def step_cli(a):
    """(iii): files written before the clock starts"""
    g, truth, n_reads = make(a)
    d = tempfile.mkdtemp(prefix="panel_auto_")
    gfa, fq = os.path.join(d, "g.gfa"), os.path.join(d, "reads.fa")
    g.write_gfa(gfa)
    g.write_reads(fq, 4903, 0, n_reads)
    out = dict(gfa_bytes=os.path.getsize(gfa), reads_bytes=os.path.getsize(fq), runs=[])
    for rep in range(a.repeats):
        t0 = time.perf_counter()
        r = subprocess.run([PHI, "--panel-auto", str(a.want), "-g", gfa, "-r", fq, "-o", os.path.join(d, "auto.fa")], capture_output=True, text=True, timeout=a.limit)
        auto_s = time.perf_counter() - t0
        if r.returncode not in (0, 3):
            raise SystemExit(f"PHI --panel-auto failed ({r.returncode}):\n" + r.stderr[-2000:])
        m = re.search(r"Panel \(from the reads\): kept \d+ of \d+ walks in (\d+) rounds over (\d+) blocks: (\S+)$", r.stderr, re.M)
        if m is None:
            raise SystemExit("PHI --panel-auto printed no 'Panel (from the reads)' line:\n" + r.stderr[-2000:])
        samples = sorted({n.rsplit(".", 1)[0] for n in m.group(3).split(",")})
        names = os.path.join(d, "names.txt")
        open(names, "w").write("\n".join(samples) + "\n")
        t0 = time.perf_counter()
        r2 = subprocess.run([PHI, "--keep-samples", "@" + names, "-g", gfa, "-r", fq, "-o", os.path.join(d, "keep.fa")], capture_output=True, text=True, timeout=a.limit)
        keep_s = time.perf_counter() - t0
        if r2.returncode not in (0, 3):                         # (3: the path is not proven optimal; anything else ends the script, nothing further is started)
            raise SystemExit(f"PHI --keep-samples failed ({r2.returncode}):\n" + r2.stderr[-2000:])
        # (the generator names two walks per sample: --keep-samples keeps both, so the two FASTA files may differ)
        out["runs"].append(dict(panel_auto_s=auto_s, keep_samples_s=keep_s, keep_samples_rc=r2.returncode, rounds=int(m.group(1)), blocks=int(m.group(2)),
                                n_samples_kept=len(samples)))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", type=int, default=2000)
    ap.add_argument("--backbone", type=int, default=5_000_000)
    ap.add_argument("--want", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=480, help="seconds every child step may take")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--step", choices=["kernels", "cli"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_auto_rate.json"))
    a = ap.parse_args()
    if a.step:
        return (step_kernels if a.step == "kernels" else step_cli)(a)
    result = dict(config=dict(walks=a.walks, backbone=a.backbone, want=a.want, blocks=a.blocks, repeats=a.repeats, reads="10x of 150 bp, read set 4903"))
    for step in ["kernels"] + (["cli"] if a.cli else []):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--walks", str(a.walks), "--backbone", str(a.backbone), "--want", str(a.want),
               "--blocks", str(a.blocks), "--repeats", str(a.repeats), "--limit", str(a.limit)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit * (1 if step == "kernels" else 2 * a.repeats + 1))
        if r.returncode:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"step {step} failed ({r.returncode}): nothing further is started")
        result[step] = json.loads(r.stdout.strip().splitlines()[-1])
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "config"})[:3000])


if __name__ == "__main__":
    main()
