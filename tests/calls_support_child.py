"""Child of tests/test_gpu_calls_support.py: MHC_4 with the CHM13 reads, walk argv[1] against walk argv[2] on a fresh context
under whatever PHI_DEVICE_POISON / PHI_DEVICE_POOL_MIN the parent set; prints {"digest": ...} of the four support arrays."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import conftest  # noqa: F401  (torch initialises first, as in the parent)
    import numpy as np
    import phi_amd
    from phi_amd import ilp_index as H
    data = os.path.join(ROOT, "tests", "golden", "data")
    g = H.Graph(os.path.join(data, "MHC_4.gfa.gz"))
    ctx = phi_amd.Context(0)
    ctx.set_params(k=31, w=25, threshold=1.0, recombination=100)
    ctx.set_graph(g.seq_concat, g.seq_off, g.adj_off, g.adj, g.walk_off, g.walk_vtx, g.top_order_map)
    bases, off, _ = H.read_reads(os.path.join(data, "CHM13_reads.fq.gz"))
    ctx.add_reads((bases, off))
    ctx.calls(1, walk=2)                                   # (buffers of another size go to the pool first)
    ctx.calls_support()
    ctx.calls(int(sys.argv[2]), walk=int(sys.argv[1]))
    s = ctx.calls_support()
    print(json.dumps({"digest": b"".join(np.ascontiguousarray(s[n]).tobytes() for n in ("alt_hit", "alt_n", "ref_hit", "ref_n")).hex()}))
    ctx.close()


if __name__ == "__main__":
    main()
