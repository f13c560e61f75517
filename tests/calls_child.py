"""Child of tests/test_gpu_calls.py: MHC_4, walk argv[1] against walk argv[2] on a fresh context under whatever
PHI_DEVICE_POISON / PHI_DEVICE_POOL_MIN the parent set; prints {"digest": ...} of the calls' arrays (no time, no address)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import conftest  # noqa: F401  (torch initialises first, as in the parent)
    import phi_amd
    from phi_amd import ilp_index as H
    from calls_ref import digest
    g = H.Graph(os.path.join(ROOT, "tests", "golden", "data", "MHC_4.gfa.gz"))
    ctx = phi_amd.Context(0)
    ctx.set_params(k=31, w=25, threshold=1.0, recombination=100)
    ctx.set_graph(g.seq_concat, g.seq_off, g.adj_off, g.adj, g.walk_off, g.walk_vtx, g.top_order_map)
    ctx.calls(1, walk=2)                                   # (buffers of another size go to the pool first)
    c = ctx.calls(int(sys.argv[2]), walk=int(sys.argv[1]))
    print(json.dumps({"digest": digest(c)}))
    ctx.close()


if __name__ == "__main__":
    main()
