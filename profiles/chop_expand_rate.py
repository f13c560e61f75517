"""Rate of the device-side chop of the walk entries (phi_set_graph_chopped, chop.hip) against a device-to-device copy of
the same number of output bytes on the same stream in the same process, and the C2 index time with and without an
identity chop.  Writes profiles/chop_expand_rate.json.

The graph (NOT the native generator's own output, which one call cannot build at this size: a stand-in of its shape, made
in numpy -- say so where the figure is quoted): --sites bi-allelic sites; a backbone segment of --seg-len random bases
before each site and after the last, two allele segments of 1 .. 60 bases per site; each of --walks walks takes every
backbone segment and one allele per site, chosen at random per walk and site, so the walks differ.  At N = 30 a backbone
entry becomes ceil(seg_len / 30) entries.  The defaults give about 10^9 chopped entries and a first[] table of 11 MB.

    python profiles/chop_expand_rate.py [--sites 900000 --seg-len 2400 --walks 14 --chop 30 --repeats 3] [--no-c2]
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
from phi_amd import synth                                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=900_000)
    ap.add_argument("--seg-len", type=int, default=2400)
    ap.add_argument("--walks", type=int, default=14)
    ap.add_argument("--chop", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-c2", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "chop_expand_rate.json"))
    a = ap.parse_args()
    S, L, nw, N = a.sites, a.seg_len, a.walks, a.chop
    rng = np.random.default_rng(1)
    # vertices in topological order: backbone 3i, alleles 3i + 1 and 3i + 2, ..., the last backbone 3S
    n = 3 * S + 1
    vlen = np.empty(n, np.int64)
    vlen[0::3] = L
    vlen[1::3] = rng.integers(1, 61, size=S)
    vlen[2::3] = rng.integers(1, 61, size=S)
    seq_off = np.concatenate([[0], np.cumsum(vlen)]).astype(np.int64)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(seq_off[-1]), dtype=np.uint8)]
    deg = np.ones(n, np.int64)
    deg[0::3] = 2
    deg[-1] = 0
    adj_off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    adj = np.empty(int(adj_off[-1]), np.int32)
    b = np.arange(S, dtype=np.int64) * 3
    adj[adj_off[b]] = b + 1
    adj[adj_off[b] + 1] = b + 2
    adj[adj_off[b + 1]] = b + 3
    adj[adj_off[b + 2]] = b + 3
    walk_off = np.arange(nw + 1, dtype=np.int64) * (2 * S + 1)
    walk_vtx = np.empty(nw * (2 * S + 1), np.int32)
    for h in range(nw):
        wv = walk_vtx[h * (2 * S + 1):(h + 1) * (2 * S + 1)]
        wv[0::2] = np.arange(S + 1) * 3
        wv[1::2] = b + 1 + rng.integers(0, 2, size=S)
    top_rank = np.arange(n, dtype=np.int32)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    out = {"graph": f"{S} bi-allelic sites between backbone segments of {L} random bases, alleles of 1..60 bases, {nw} walks that choose "
                    f"their allele at random per site ({n} vertices, {int(seq_off[-1])} bases)", "max_len": N, "first_table_bytes": 4 * (n + 1), "runs": []}
    for _ in range(a.repeats):
        ctx = phi_amd.Context(0)
        ctx.set_params(k=31, w=25)
        ctx.set_stream(stream.cuda_stream)
        t0 = time.perf_counter()
        ctx.set_graph(seq, seq_off, adj_off, adj, walk_off, walk_vtx, top_rank, chop=N)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        cs = ctx.chop_stats()
        ctx.close()
        n_out = cs["n_entries_out"]
        src = torch.empty(n_out, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(src)
        src.zero_()
        dst.copy_(src)                                          # (first touch)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        dst.copy_(src)                                          # hipMemcpyAsync, device to device, on the context's stream
        e1.record(stream)
        torch.cuda.synchronize()
        copy_ms = e0.elapsed_time(e1)
        del src, dst
        out["runs"].append({"entries_in": cs["n_entries_in"], "entries_out": n_out, "vertices_in": cs["n_vtx_in"], "vertices_out": cs["n_vtx_out"],
                            "expand_gpu_ms": cs["expand_gpu_ms"], "copy_d2d_ms": copy_ms, "factor": cs["expand_gpu_ms"] / copy_ms,
                            "set_graph_chopped_wall_s": wall})
        print(out["runs"][-1], flush=True)
    best = min(out["runs"], key=lambda r: r["expand_gpu_ms"])
    out["expand_gpu_ms"], out["copy_d2d_ms"] = best["expand_gpu_ms"], min(r["copy_d2d_ms"] for r in out["runs"])
    out["factor"] = out["expand_gpu_ms"] / out["copy_d2d_ms"]
    out["expand_gentries_per_s"] = best["entries_out"] / best["expand_gpu_ms"] / 1e6
    if not a.no_c2:
        gk, _ = synth.CONFIGS["C2"]
        g = synth.make_graph(**gk)
        A = g.arrays()
        c2 = {"plain_s": [], "identity_chop_s": []}
        for i in range(2 * 5):
            ctx = phi_amd.Context(0)
            ctx.set_params(k=31, w=25)
            ctx.set_stream(stream.cuda_stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"], chop=(1 << 30) if i % 2 else None)
            torch.cuda.synchronize()
            c2["identity_chop_s" if i % 2 else "plain_s"].append(time.perf_counter() - t0)
            ctx.close()
        c2["plain_median_s"] = float(np.median(c2["plain_s"]))
        c2["identity_chop_median_s"] = float(np.median(c2["identity_chop_s"]))
        out["c2_index"] = c2
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))


if __name__ == "__main__":
    main()
