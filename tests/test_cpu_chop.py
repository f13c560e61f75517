"""Chopping a graph into segments of at most N bases (phi_set_graph_chopped, phi_amd/csrc/chop.hip), the parts that need no GPU:
the rule restated in numpy (chop_numpy: what tests/test_gpu_chop.py holds the library against) pinned by hand-written cases,
the new kernels' resources, and the new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def chop_numpy(g, N):
    """The rule of include/phi_amd.h phi_set_graph_chopped on an oracle Graph: (chopped Graph, orig_vtx, orig_off).
    A vertex of L bases becomes max(1, ceil(L / N)) pieces, full pieces first; the pieces of v are first[v] + j; edges
    piece j -> j + 1 and last piece of u -> first piece of v; rank = counts summed in topological order + j."""
    from oracle import oracle as O
    n = g.n_vtx
    L = np.array([len(s) for s in g.node_seq], np.int64)
    cnt = np.maximum(1, -(-L // N))
    first = np.concatenate([[0], np.cumsum(cnt)])
    nv = int(first[-1])
    orig_vtx = np.repeat(np.arange(n), cnt)
    piece = np.arange(nv) - first[orig_vtx]
    orig_off = piece * N
    node_seq = [g.node_seq[v][o:o + N] for v, o in zip(orig_vtx.tolist(), orig_off.tolist())]
    adj = [[] for _ in range(nv)]
    for v in range(n):
        for j in range(int(cnt[v]) - 1):
            adj[first[v] + j] = [int(first[v] + j + 1)]
        adj[first[v + 1] - 1] = [int(first[u]) for u in g.adj[v]]
    rank = np.asarray(g.top_rank, np.int64)
    order = np.argsort(rank)
    rank0 = np.zeros(n, np.int64)
    rank0[order] = np.concatenate([[0], np.cumsum(cnt[order])[:-1]])
    top_rank = rank0[orig_vtx] + piece
    paths = [np.concatenate([np.arange(first[v], first[v + 1]) for v in p]).tolist() for p in g.paths]
    out = O.Graph(seg_names=[f"s{i + 1}" for i in range(nv)], node_seq=node_seq, adj=adj, paths=paths, hap_names=list(g.hap_names),
                  top_order=np.argsort(top_rank).tolist(), top_rank=top_rank.tolist())
    return out, orig_vtx.astype(np.int32), orig_off.astype(np.int32)


def _graph(node_seq, adj, paths, top_rank=None):
    from oracle import oracle as O
    g = O.Graph(seg_names=[f"s{i + 1}" for i in range(len(node_seq))], node_seq=node_seq, adj=adj, paths=paths,
                hap_names=[f"h{i}.0" for i in range(len(paths))])
    if top_rank is None:
        O.kahn(g)
    else:
        g.top_rank = list(top_rank)
        g.top_order = np.argsort(top_rank).tolist()
    return g


def test_chop_numpy_chain_by_hand():
    # 7, 3 and 6 bases at N = 3: 3 + 1 + 2 pieces; an exact multiple (6), a multiple plus one (7)
    g = _graph([b"ACGTACG", b"TTT", b"GGGCCC"], [[1], [2], []], [[0, 1, 2], [1, 2]])
    c, ov, oo = chop_numpy(g, 3)
    assert c.node_seq == [b"ACG", b"TAC", b"G", b"TTT", b"GGG", b"CCC"]
    assert c.adj == [[1], [2], [3], [4], [5], []]
    assert c.paths == [[0, 1, 2, 3, 4, 5], [3, 4, 5]]
    assert c.top_rank == [0, 1, 2, 3, 4, 5]
    assert ov.tolist() == [0, 0, 0, 1, 2, 2] and oo.tolist() == [0, 3, 6, 0, 0, 3]


def test_chop_numpy_bubble_by_hand():
    # 0 -> {1, 2} -> 3 with vertex 2 BEFORE vertex 1 in topological order, an empty vertex 4 on no walk
    g = _graph([b"AAAAA", b"CC", b"GGGG", b"T", b""], [[1, 2], [3], [3], [], []], [[0, 1, 3], [0, 2, 3]], top_rank=[0, 2, 1, 3, 4])
    c, ov, oo = chop_numpy(g, 2)
    #            0: AA AA A | 1: CC | 2: GG GG | 3: T | 4: ""
    assert c.node_seq == [b"AA", b"AA", b"A", b"CC", b"GG", b"GG", b"T", b""]
    assert c.adj == [[1], [2], [3, 4], [6], [5], [6], [], []]          # out-edges of the last piece in the vertex's order
    assert c.paths == [[0, 1, 2, 3, 6], [0, 1, 2, 4, 5, 6]]
    assert c.top_rank == [0, 1, 2, 5, 3, 4, 6, 7]                      # vertex 2's pieces (ranks 3, 4) before vertex 1's (5)
    assert ov.tolist() == [0, 0, 0, 1, 2, 2, 3, 4] and oo.tolist() == [0, 2, 4, 0, 0, 2, 0, 0]


def test_chop_numpy_identity_by_hand():
    g = _graph([b"ACGT", b"AC", b"G"], [[1, 2], [2], []], [[0, 1, 2], [0, 2]])
    for N in (4, 5, 10000):
        c, ov, oo = chop_numpy(g, N)
        assert c.node_seq == g.node_seq and c.adj == g.adj and c.paths == g.paths and c.top_rank == list(g.top_rank)
        assert ov.tolist() == [0, 1, 2] and oo.tolist() == [0, 0, 0]
    c, _, _ = chop_numpy(g, 1)
    assert c.n_vtx == 7 and c.paths[1] == [0, 1, 2, 3, 6]


def test_chop_kernels_use_no_scratch_and_the_lds_they_declare(tmp_path):
    """chop.hip for gfx950: no kernel spills or touches scratch; the expansion's static LDS is its two staged arrays
    (CHOP_TILE entries of 4 bytes each) and the few words the workgroup-wide counts take, four workgroups to a CU."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "phi_amd", "csrc", "chop.hip")
    out = tmp_path / "chop.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), src], stderr=subprocess.DEVNULL)
    asm = out.read_text()
    tile = int(re.search(r"#define CHOP_TILE (\d+)", open(src).read()).group(1))
    entries = asm.split("  - .agpr_count:")[1:]
    seen = {}
    for e in entries:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        m = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", e)}
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        seen[name] = m
    expand = [m for n, m in seen.items() if "chop_expand_kernel" in n]
    assert len(expand) == 1 and len(seen) == 3, list(seen)
    assert 2 * 4 * tile <= expand[0]["group_segment_fixed_size"] <= 2 * 4 * tile + 512
    assert 4 * expand[0]["group_segment_fixed_size"] <= 160 * 1024
    assert expand[0]["vgpr_count"] <= 64                               # (eight waves per SIMD)
    for n, m in seen.items():
        if "chop_expand_kernel" not in n:
            assert m["group_segment_fixed_size"] == 0, (n, m)


def test_chop_symbols_are_declared_bound_and_exported():
    from phi_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "phi_amd.h")).read()
    for name in ("phi_set_graph_chopped", "phi_chop_origin", "phi_chop_stats"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _capi.SYMBOLS
    assert len(re.findall(r"data/chop_graph\.sh:3", hdr)) >= 3         # every entry cites what it replaces
    lib = os.path.join(ROOT, "phi_amd", "libphi_amd.so")
    if os.path.exists(lib):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for name in ("phi_set_graph_chopped", "phi_chop_origin", "phi_chop_stats"):
            assert re.search(r" T " + name + r"\b", syms), name
