"""A panel of a graph's haplotypes (phi_set_graph_panel, phi_amd/csrc/panel.hip), the parts that need no GPU: the rule restated
in numpy (phi_amd.panel.induced_subgraph: what tests/test_gpu_panel.py holds the library against) pinned to the host reader
and to oracle.parse_gfa on GFA files reduced by plain text handling, the choice of nested panels, the kernels' resources and
the new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from graphgen import random_graph

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def gfa_text(g):
    out = ["H\tVN:Z:1.1\n"]
    for i, s in enumerate(g.node_seq):
        out.append(f"S\ts{i + 1}\t{s.decode()}\n")
    for u, a in enumerate(g.adj):
        for v in a:
            out.append(f"L\ts{u + 1}\t+\ts{v + 1}\t+\t0M\n")
    for h, p in enumerate(g.paths):
        smp, hap = g.hap_names[h].rsplit(".", 1)
        out.append(f"W\t{smp}\t{hap}\tchr\t0\t1\t" + "".join(f">s{v + 1}" for v in p) + "\n")
    return "".join(out)


def reduced_gfa_text(text, keep):
    """The GFA minus the W-lines of the dropped walks and minus the S- and L-lines nothing uses any more: text handling only."""
    lines = text.splitlines(keepends=True)
    w_lines = [ln for ln in lines if ln.startswith("W\t")]
    kept_w = [ln for ln, k in zip(w_lines, keep) if k]
    names, steps = set(), set()
    for ln in kept_w:
        walk = ln.rstrip("\n").split("\t")[6].split(">")[1:]
        names.update(walk)
        steps.update(zip(walk, walk[1:]))
    out = []
    for ln in lines:
        f = ln.rstrip("\n").split("\t")
        if f[0] == "S" and f[1] not in names:
            continue
        if f[0] == "L" and (f[1], f[3]) not in steps:
            continue
        if f[0] == "W" and ln not in kept_w:
            continue
        out.append(ln)
    return "".join(out)


def vacuity_graph():
    return random_graph(np.random.default_rng(507), n_sites=40, n_walks=5, seg_len=(1, 400), alt_len=(1, 40), p_del=0.3)


def _masks(n):
    every_other = np.arange(n) % 2 == 0
    without_first = np.ones(n, bool); without_first[0] = False
    first_only = ~without_first
    return {"every other": every_other, "without walk 0": without_first, "walk 0 alone": first_only}


def n_edges(g):
    return sum(len(a) for a in g.adj)


def hand_graph():
    """Compressed old ranks differ from Kahn's on the subgraph (found by enumeration, argued by hand in the test).
      edges 0->1, 0->2, 0->3, 1->2, 2->4, 3->4; walks 0 3 4 | 0 1 2 4 | 0 2 4
    Full graph: 0 releases 1 and 3 (2 still waits for 1), so the queue runs 0 1 3 2 4 and 3 comes BEFORE 2.  Without the
    middle walk vertex 1 and the edge 1->2 go: 2's early in-edge 0->2 is the only one left, 0 releases 2 and 3 in id order,
    and 2 comes before 3."""
    from oracle import oracle as O
    node_seq = [b"ACGTA", b"CC", b"GGT", b"TTA", b"CAG"]
    adj = [[1, 2, 3], [2], [4], [4], []]
    paths = [[0, 3, 4], [0, 1, 2, 4], [0, 2, 4]]
    g = O.Graph(seg_names=[f"s{i + 1}" for i in range(len(node_seq))], node_seq=node_seq, adj=adj, paths=paths,
                hap_names=[f"h{i}.0" for i in range(len(paths))])
    O.kahn(g)
    return g


def _check_rule(oracle, tmp_path, g, keep, tag):
    from phi_amd import ilp_index as H
    from phi_amd.panel import induced_subgraph
    sub, origin = induced_subgraph(g, keep)
    path = tmp_path / f"{tag}.gfa"
    path.write_text(reduced_gfa_text(gfa_text(g), keep))
    o = oracle.parse_gfa(str(path))
    assert o.node_seq == sub.node_seq and o.adj == sub.adj and o.paths == sub.paths and o.hap_names == sub.hap_names
    assert list(o.top_rank) == list(sub.top_rank)
    assert o.seg_names == [g.seg_names[v] for v in origin.tolist()]
    r = H.Graph(str(path))
    A = sub.arrays()
    assert r.n_vtx == sub.n_vtx and r.num_walks == sub.n_walks
    assert np.array_equal(r.seq_off, A["seq_off"]) and r.seq_concat.tobytes() == A["seq_concat"]
    assert np.array_equal(r.adj_off, A["adj_off"]) and np.array_equal(r.adj, A["adj"])
    assert np.array_equal(r.walk_off, A["walk_off"]) and np.array_equal(r.walk_vtx, A["walk_vtx"])
    assert np.array_equal(r.top_order_map, A["top_rank"])
    assert r.hap_id2name == sub.hap_names
    return sub, origin


def test_rule_equals_the_readers_on_the_reduced_gfa(oracle, tmp_path):
    g = vacuity_graph()
    lost = {}
    for name, keep in _masks(g.n_walks).items():
        sub, origin = _check_rule(oracle, tmp_path, g, keep, name.replace(" ", "_"))
        lost[name] = (g.n_vtx - sub.n_vtx, n_edges(g) - n_edges(sub))
        # not vacuous: the mask drops at least one vertex and one edge, or keeps a single walk
        assert (lost[name][0] >= 1 and lost[name][1] >= 1) or keep.sum() == 1, name
    assert lost["every other"] == (7, 17) and lost["without walk 0"] == (2, 7)
    assert lost["walk 0 alone"][0] * 3 >= g.n_vtx - 2                  # a third of the vertices


def test_rule_is_applied_with_every_walk_kept(oracle, tmp_path):
    g = random_graph(np.random.default_rng(107), n_sites=4, n_walks=3, seg_len=(1, 400), alt_len=(1, 40), p_del=0.3)
    sub, _ = _check_rule(oracle, tmp_path, g, np.ones(3, bool), "all")
    assert (g.n_vtx, sub.n_vtx, n_edges(g), n_edges(sub)) == (10, 9, 13, 11)


def test_ranks_are_kahns_on_the_panel_not_the_old_ones_compressed(oracle, tmp_path):
    g = hand_graph()
    keep = np.array([True, False, True])
    sub, origin = _check_rule(oracle, tmp_path, g, keep, "hand")
    old = np.asarray(g.top_rank)[origin]
    compressed = np.argsort(np.argsort(old))
    assert not np.array_equal(compressed, np.asarray(sub.top_rank))    # (the case is not vacuous)
    assert g.top_rank == [0, 1, 3, 2, 4] and origin.tolist() == [0, 2, 3, 4]
    assert sub.adj == [[1, 2], [3], [3], []] and sub.top_rank == [0, 1, 2, 3] and compressed.tolist() == [0, 2, 1, 3]


def test_rule_by_hand():
    from phi_amd.panel import induced_subgraph
    from oracle import oracle as O
    #   0 -> {1, 2} -> 3, 4 on no walk, an edge 0 -> 3 no walk uses
    g = O.Graph(seg_names=["a", "b", "c", "d", "e"], node_seq=[b"AAAAA", b"cc", b"GGNG", b"T", b"ACAC"],
                adj=[[1, 2, 3], [3], [3], [], []], paths=[[0, 1, 3], [0, 2, 3], [0, 2, 3]], hap_names=["x.1", "y.1", "y.2"])
    O.kahn(g)
    sub, origin = induced_subgraph(g, [0, 1, 1])
    assert origin.tolist() == [0, 2, 3] and sub.node_seq == [b"AAAAA", b"GGNG", b"T"] and sub.adj == [[1], [2], []]
    assert sub.paths == [[0, 1, 2], [0, 1, 2]] and sub.hap_names == ["y.1", "y.2"] and sub.top_rank == [0, 1, 2] and sub.seg_names == ["a", "c", "d"]
    sub, origin = induced_subgraph(g, [1, 1, 1])
    assert origin.tolist() == [0, 1, 2, 3] and sub.adj == [[1, 2], [3], [3], []]
    A, origin = induced_subgraph(g.arrays(), [1, 0, 0])
    assert origin.tolist() == [0, 1, 3] and A["walk_vtx"].tolist() == [0, 1, 2] and A["seq_concat"] == b"AAAAAccT" and A["top_rank"].tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        induced_subgraph(g, [0, 0, 0])
    with pytest.raises(ValueError):
        induced_subgraph(g, [1, 1])


def test_nested_panels():
    from phi_amd.panel import keep_mask, nested_panels, sample_of, samples_in_order
    assert sample_of("HG002.1") == "HG002" and sample_of("a.b.2") == "a.b" and sample_of("REF.0") == "REF"
    haps = ["REF.0"] + [f"S{i}.{j}" for i in range(24) for j in (1, 2)]
    samples = samples_in_order(haps)
    assert samples == ["REF"] + [f"S{i}" for i in range(24)]
    sizes = [1, 3, 6, 12, 24]
    p = nested_panels(samples, sizes, seed=3, always=["REF"])
    assert [len(x) for x in p] == [n + 1 for n in sizes]
    for a, b in zip(p, p[1:]):
        assert a == b[:len(a)]                                             # nested, in one order
    assert all(x[0] == "REF" and len(set(x)) == len(x) for x in p)
    assert set(p[-1]) == set(samples)
    assert nested_panels(samples, sizes, seed=3, always=["REF"]) == p
    assert nested_panels(samples, sizes, seed=4, always=["REF"])[2] != p[2]
    # the key is splitmix64(seed, ordinal) over the samples not in `always`, ties by ordinal
    from phi_amd.ladder import splitmix64
    rest = samples[1:]
    keys = splitmix64(3, np.arange(len(rest)))
    want = [rest[i] for i in sorted(range(len(rest)), key=lambda i: (int(keys[i]), i))]
    assert p[-1][1:] == want
    assert nested_panels(samples, [2], seed=3)[0] == [samples[i] for i in sorted(range(25), key=lambda i: (int(splitmix64(3, np.arange(25))[i]), i))][:2]
    for bad in ([3, 2], [25], [-1]):
        with pytest.raises(ValueError):
            nested_panels(samples, bad, seed=0, always=["REF"])
    with pytest.raises(ValueError, match="nobody"):
        nested_panels(samples, [1], seed=0, always=["nobody"])
    m = keep_mask(haps, keep_samples=["REF", "S3"])
    assert np.flatnonzero(m).tolist() == [0, 7, 8]
    assert np.array_equal(keep_mask(haps, drop_samples=["REF", "S3"]), ~m)
    with pytest.raises(ValueError, match="S99, T1"):
        keep_mask(haps, drop_samples=["S1", "S99", "T1"])


def test_vacuity_of_many_walks_over_few_sites():
    """Why the equality tests use few walks over many sites: with dozens of walks over a handful of sites every vertex stays
    on some kept walk."""
    from phi_amd.panel import induced_subgraph
    g = random_graph(np.random.default_rng(9), n_sites=6, n_walks=70, seg_len=(1, 40), alt_len=(1, 9), p_del=0.3)
    sub, _ = induced_subgraph(g, np.arange(70) % 2 == 0)
    assert sub.n_vtx == g.n_vtx and n_edges(sub) == n_edges(g)


def test_panel_kernels_use_no_scratch_and_the_lds_they_declare(tmp_path):
    """panel.hip for gfx950: no kernel spills or touches scratch; mark and remap stage two arrays of PANEL_TILE entries of 4
    bytes each (and the few words the workgroup-wide counts take), four workgroups to a CU; the small kernels use no LDS."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "phi_amd", "csrc", "panel.hip")
    out = tmp_path / "panel.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), src], stderr=subprocess.DEVNULL)
    asm = out.read_text()
    tile = int(re.search(r"#define PANEL_TILE (\d+)", open(src).read()).group(1))
    seen = {}
    for e in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        m = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", e)}
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        seen[name] = m
    assert len(seen) == 4, list(seen)
    for n, m in seen.items():
        if "panel_mark_kernel" in n or "panel_remap_kernel" in n:
            assert 2 * 4 * tile <= m["group_segment_fixed_size"] <= 2 * 4 * tile + 512, (n, m)
            assert 4 * m["group_segment_fixed_size"] <= 160 * 1024
            assert m["vgpr_count"] <= 64, (n, m)                           # (eight waves per SIMD)
        else:
            assert m["group_segment_fixed_size"] == 0, (n, m)


def test_panel_symbols_are_declared_bound_and_exported():
    from phi_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "phi_amd.h")).read()
    names = ("phi_set_graph_panel", "phi_panel_origin", "phi_panel_walks", "phi_panel_stats", "phi_panel_release")
    for name in names:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _capi.SYMBOLS
    for cite in (r"data/chop_graph\.sh:46-66", r"data/get_ids\.py", r"data/get_ids_2\.py", r"data/run_batch_9\.py to run_batch_13\.py"):
        assert re.search(cite, hdr), cite
    lib = os.path.join(ROOT, "phi_amd", "libphi_amd.so")
    if os.path.exists(lib):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for name in names:
            assert re.search(r" T " + name + r"\b", syms), name
