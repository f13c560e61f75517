"""A panel, a chopped panel and a retained ladder of panels, run as a CHILD PROCESS by tests/test_gpu_panel.py: plain, under
PHI_DEVICE_POISON (every device buffer starts out full of a byte) and under PHI_DEVICE_POOL_MIN=256 (every buffer comes back with
an earlier owner's contents).  Every case is asserted here against the numpy rule (phi_amd.panel.induced_subgraph, and
test_cpu_chop.chop_numpy behind it); the last line printed is one JSON object of integers and array hashes -- never a time,
never an address -- which the parent compares exactly between the three runs."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def _h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _digest(ctx, res):
    d = {k: int(res[k]) for k in ("objective", "n_covered", "n_path", "recombination_count", "hap_len", "spectrum_size", "filtered", "n_in_model")}
    d.update(entries=_h(ctx.walk_entries()), path_vtx=_h(res["path_vtx"]), path_hap=_h(res["path_hap"]), n_minimizers=_h(res["n_minimizers"]),
             n_anchors=_h(res["n_anchors"]), anchors="|".join(_h(x) for x in ctx.kept_anchors()),
             seq=hashlib.sha256(ctx.path_sequence(res["hap_len"])).hexdigest()[:16])
    ps = ctx.panel_stats()
    d.update({k: int(v) for k, v in ps.items() if not k.endswith("_ms") and not k.endswith("_s")})
    return d


def main():
    import conftest  # noqa: F401  (torch initialises before libphi_amd.so is loaded, as in the suite)
    import phi_amd
    from graphgen import mosaic_reads, random_graph
    from phi_amd.panel import induced_subgraph
    from test_cpu_chop import chop_numpy
    rng = np.random.default_rng(507)
    g = random_graph(rng, n_sites=40, n_walks=5, seg_len=(1, 400), alt_len=(1, 40), p_del=0.3)
    reads = mosaic_reads(rng, g, n_reads=60, read_len=70, n_seg=2, err=0.01)
    A = g.arrays()
    out = {}

    def run(ctx, keep, chop, walk_vtx, retain):
        sub, origin = induced_subgraph(g, keep)
        want = chop_numpy(sub, chop)[0] if chop else sub
        woff = ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], walk_vtx, None, keep=keep, chop=chop, retain=retain)
        W = want.arrays()
        assert np.array_equal(woff, W["walk_off"]) and np.array_equal(ctx.walk_entries(), W["walk_vtx"])
        assert np.array_equal(ctx.panel_origin(np.arange(sub.n_vtx)), origin)
        ctx.add_reads(reads)
        res = ctx.solve()
        assert res["optimal"] == 1
        return _digest(ctx, res)

    every_other = np.arange(5) % 2 == 0
    ctx = phi_amd.Context(0)
    ctx.set_params(k=9, w=4, threshold=1.0, recombination=3)
    out["panel"] = run(ctx, every_other, None, A["walk_vtx"], False)
    out["chopped"] = run(ctx, every_other, 7, A["walk_vtx"], False)
    masks = [np.array([1, 0, 0, 0, 0], bool), np.array([1, 0, 1, 0, 0], bool), np.array([1, 1, 1, 0, 1], bool)]
    for step, j in enumerate([0, 1, 2, 1, 0]):
        out[f"ladder{step}"] = run(ctx, masks[j], 30 if step == 3 else None, A["walk_vtx"] if step == 0 else None, True)
    ctx.panel_release()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
