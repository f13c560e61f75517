"""The record splitter of FASTQ text on the device (phi_add_reads_text, reads_text.hip) on its own: a FASTQ of
150-base reads the script writes, fed in pieces from host memory against the reference's MHC_4 graph; the wall time covers the
copies to the device, the text kernels and the sketch of the records they find, the device waited for before the clock stops.
Run by hand on the MI355X, alone or under `rocprofv3 --kernel-trace --stats -- python3 profiles/reads_text_rate.py` for the
phi_text_* kernels one by one; writes profiles/reads_text_rate.json.

    python profiles/reads_text_rate.py [--mbytes 256] [--piece-mbytes 32] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (its HIP runtime initialises first, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import phi_amd                                                  # noqa: E402
from phi_amd import ilp_index as H                              # noqa: E402

READ = 150


def fastq(n_bytes, seed=5):
    """records of one layout: a 12-byte header line, READ bases, '+', READ quality bytes"""
    rng = np.random.default_rng(seed)
    rec = 12 + READ + 1 + 2 + READ + 1
    n = max(1, n_bytes // rec)
    t = np.empty((n, rec), np.uint8)
    t[:, :12] = np.frombuffer(b"@read......\n", np.uint8)
    t[:, 5:11] = np.frombuffer(b"0123456789", np.uint8)[(np.arange(n)[:, None] // 10 ** np.arange(5, -1, -1)) % 10]
    t[:, 12:12 + READ] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, READ))]
    t[:, 12 + READ:12 + READ + 3] = np.frombuffer(b"\n+\n", np.uint8)
    t[:, 12 + READ + 3:rec - 1] = ord("I")
    t[:, rec - 1] = ord("\n")
    return t.reshape(-1), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbytes", type=int, default=256)
    ap.add_argument("--piece-mbytes", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reads_text_rate.json"))
    a = ap.parse_args()
    text, n_reads = fastq(a.mbytes << 20)
    piece = a.piece_mbytes << 20
    g = H.Graph(os.path.join(ROOT, "tests", "golden", "data", "MHC_4.gfa.gz"))
    ctx = phi_amd.Context(0)
    ctx.set_params(k=31, w=25, threshold=0.9, recombination=10000)
    ctx.set_graph(g.seq_concat, g.seq_off, g.adj_off, g.adj, g.walk_off, g.walk_vtx, g.top_order_map)
    runs = []
    for rep in range(a.repeats + 1):
        ctx.reset_reads()
        ctx.reads_text_begin(piece)
        t0 = time.perf_counter()
        for i in range(0, len(text), piece):
            assert not ctx.add_reads_text(text[i:i + piece])
        pending, taken = ctx.reads_text_end()
        torch.cuda.synchronize()                                # (the sketch of the last piece's records is inside the clock)
        dt = time.perf_counter() - t0
        st = ctx.reads_stats()
        assert n_reads - 1 <= st["n_reads"] <= n_reads and st["n_bases"] == st["n_reads"] * READ, (st, taken, len(pending))
        if rep:                                                 # (the first turn is the warm-up)
            runs.append(dt)
    out = {"device": torch.cuda.get_device_name(0), "text_bytes": int(len(text)), "reads": int(n_reads), "piece_bytes": piece, "wall_s": runs,
           "median_wall_s": statistics.median(runs), "median_text_gb_per_s": len(text) / statistics.median(runs) / 1e9}
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
