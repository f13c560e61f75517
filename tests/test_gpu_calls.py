"""Variant calls of a walk or of the inferred path against a reference walk, made on the device (phi_calls_walk,
phi_calls_path; calls.hip), against the plain-Python restatement of the rule in tests/calls_ref.py: every array element for
element, and the consensus of the calls (phi_amd.calls.apply) against the query's own sequence.

The case "no shared vertex" uses a graph of two disjoint walks, which phi_set_graph accepts."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from calls_ref import calls_ref, calls_ref_numpy, digest
from conftest import DATA, ROOT
from graphgen import mosaic_reads, random_graph, walk_sequence
from test_cpu_chop import chop_numpy

pytestmark = pytest.mark.gpu

K, W = 5, 2
ARRAYS = ("pos", "anchor", "ref_off", "alt_off")
SCALARS = ("n_calls", "n_shared", "n_query", "n_ref", "ref_bytes", "alt_bytes", "ref_span", "query_span")


def _set(ctx, g, **kw):
    A = g.arrays()
    return ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"], **kw)


def _same(got, want):
    for k in SCALARS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert got["gpu_ms"] > 0


def _check_pair(ctx, g, q, r):
    """walk q against walk r on graph g (an oracle-style graph: what the context was set with)"""
    from phi_amd.calls import apply
    got = ctx.calls(r, walk=q)
    want = calls_ref(g.paths[q], g.paths[r], g.node_seq)
    _same(got, want)
    qs = walk_sequence(g, q)
    assert apply(walk_sequence(g, r), got) == qs[got["query_span"][0]:got["query_span"][1]]
    return got


def _hand_graph(node_seq, edges, paths):
    from oracle import oracle as O
    adj = [[] for _ in node_seq]
    for u, v in edges:
        adj[u].append(v)
    g = O.Graph(seg_names=[f"s{i + 1}" for i in range(len(node_seq))], node_seq=list(node_seq), adj=[sorted(a) for a in adj],
                paths=[list(p) for p in paths], hap_names=[f"hap{h}.{h}" for h in range(len(paths))])
    O.kahn(g)
    return g


# ------------------------------------------------------------------ 1. random graphs, every ordered pair of walks

@pytest.mark.parametrize("seed", range(36))
def test_random_graphs_every_ordered_pair(oracle, ctx_factory, seed):
    rng = np.random.default_rng(7000 + seed)
    g = random_graph(rng, n_sites=seed % 13, n_walks=4, seg_len=(K + 1, 12), p_del=0.4 if seed % 2 else 0.0)
    ctx = _ctx(ctx_factory)
    _set(ctx, g)
    n_padded = 0
    for q in range(4):
        for r in range(4):
            got = _check_pair(ctx, g, q, r)
            if q == r or g.paths[q] == g.paths[r]:
                assert got["n_calls"] == 0 and got["ref_off"][-1] == 0 and got["alt_off"][-1] == 0      # (the total of allele bytes is 0)
                assert got["n_shared"] == len(g.paths[q])
            ro, ao = got["ref_off"], got["alt_off"]
            for k in range(got["n_calls"]):                # padded calls: one allele is the one base of the anchor
                n_padded += (ro[k + 1] - ro[k] == 1 or ao[k + 1] - ao[k] == 1) and got["ref_bytes"][ro[k]] == got["alt_bytes"][ao[k]]
    if seed % 2 and seed % 13 >= 6:
        assert n_padded > 0                                # (p_del = 0.4 over six sites and more: some walk skips an allele another takes)


@functools.lru_cache(maxsize=None)
def _ctx_cached(factory):
    return factory(k=K, w=W, threshold=1.0, recombination=3)


def _ctx(ctx_factory):
    return _ctx_cached(ctx_factory)


def test_insertion_behind_a_one_base_vertex_and_adjacent_bubbles(oracle, ctx_factory):
    ctx = _ctx(ctx_factory)
    # 0 -> 1 ("G", one base, shared) -> [2, an insertion] -> 3
    g = _hand_graph([b"ACGTACGA", b"G", b"TTT", b"CAGTCATC"], [(0, 1), (1, 2), (1, 3), (2, 3)], [[0, 1, 3], [0, 1, 2, 3]])
    _set(ctx, g)
    ins = _check_pair(ctx, g, 1, 0)
    assert (ins["n_calls"], ins["ref_bytes"], ins["alt_bytes"], ins["pos"].tolist(), ins["anchor"].tolist()) == (1, b"G", b"GTTT", [8], [1])
    dele = _check_pair(ctx, g, 0, 1)
    assert (dele["n_calls"], dele["ref_bytes"], dele["alt_bytes"], dele["pos"].tolist()) == (1, b"GTTT", b"G", [8])
    # two bubbles with no plain vertex between them: 0 -> (1 | 2) -> (3 | 4) -> 5
    g = _hand_graph([b"ACGTACGA", b"a", b"CC", b"GGG", b"t", b"CAGTCATC"],
                    [(0, 1), (0, 2), (1, 3), (1, 4), (2, 3), (2, 4), (3, 5), (4, 5)], [[0, 1, 3, 5], [0, 2, 4, 5], [0, 1, 4, 5], [0, 2, 3, 5]])
    _set(ctx, g)
    both = _check_pair(ctx, g, 1, 0)
    assert (both["n_calls"], both["ref_bytes"], both["alt_bytes"], both["pos"].tolist()) == (1, b"aGGG", b"CCt", [8])     # (case kept)
    for q in range(4):
        for r in range(4):
            _check_pair(ctx, g, q, r)


# ------------------------------------------------------------------ 2. borders

@pytest.mark.parametrize("n_sites", [1500, 3000, 5000])
def test_queries_longer_than_the_scan_and_compaction_workgroups(oracle, ctx_factory, n_sites):
    """More than 2 048 entries (a workgroup of the compaction), more than 4 096 (the single-workgroup scan's tile) and more
    than 8 192 (where the 64-bit scan goes from one workgroup to three phases)."""
    rng = np.random.default_rng(n_sites)
    g = random_graph(rng, n_sites=n_sites, n_walks=3, seg_len=(1, 9), p_del=0.3)
    assert min(len(p) for p in g.paths) > {1500: 2048, 3000: 4096, 5000: 8192}[n_sites]
    ctx = _ctx(ctx_factory)
    _set(ctx, g)
    for q, r in ((0, 1), (1, 0), (2, 1)):
        assert _check_pair(ctx, g, q, r)["n_calls"] > n_sites // 8


@pytest.mark.parametrize("n_pairs", [1024, 2048])
def test_shared_pairs_an_exact_multiple_of_the_workgroup(oracle, ctx_factory, n_pairs):
    rng = np.random.default_rng(n_pairs)
    seqs, edges, p0, p1 = [], [], [], []

    def node(n):
        seqs.append(bytes(rng.choice(list(b"ACGT"), size=n).tolist()))
        return len(seqs) - 1
    prev = node(8)
    p0.append(prev)
    p1.append(prev)
    for i in range(n_pairs):
        nxt = None
        if i % 3 == 0:                                     # a bubble: walk 0 takes one allele, walk 1 the other
            a, b = node(int(rng.integers(1, 5))), node(int(rng.integers(1, 5)))
            nxt = node(int(rng.integers(1, 9)))
            edges += [(prev, a), (prev, b), (a, nxt), (b, nxt)]
            p0.append(a)
            p1.append(b)
        else:
            nxt = node(int(rng.integers(1, 9)))
            edges.append((prev, nxt))
        p0.append(nxt)
        p1.append(nxt)
        prev = nxt
    g = _hand_graph(seqs, edges, [p0, p1])
    ctx = _ctx(ctx_factory)
    _set(ctx, g)
    got = _check_pair(ctx, g, 1, 0)
    assert got["n_shared"] - 1 == n_pairs and got["n_calls"] == (n_pairs + 2) // 3


def test_an_allele_of_many_pieces_longer_than_the_fill_tile(oracle, ctx_factory):
    """A 10 000-base insertion on a graph set with chop=25: 400 pieces, ten tiles of the fill; the ids are the chopped graph's."""
    rng = np.random.default_rng(25)
    g = _hand_graph([b"ACGTACGTAC", bytes(rng.choice(list(b"ACGT"), size=10000).tolist()), b"TTGACCGATA"], [(0, 1), (0, 2), (1, 2)],
                    [[0, 2], [0, 1, 2]])
    c, _, _ = chop_numpy(g, 25)
    ctx = _ctx(ctx_factory)
    _set(ctx, g, chop=25)
    ins = _check_pair(ctx, c, 1, 0)
    assert ins["n_calls"] == 1 and ins["alt_off"][-1] == 10001 and ins["ref_bytes"] == b"C" and ins["n_query"] == 402
    dele = _check_pair(ctx, c, 0, 1)
    assert dele["n_calls"] == 1 and dele["ref_off"][-1] == 10001 and dele["alt_bytes"] == b"C"


# ------------------------------------------------------------------ 3. MHC_4

@pytest.fixture(scope="module")
def mhc(ctx_factory):
    from phi_amd import ilp_index as H
    g = H.Graph(os.path.join(DATA, "MHC_4.gfa.gz"))
    ctx = ctx_factory(k=31, w=25, threshold=1.0, recombination=100)
    ctx.set_graph(g.seq_concat, g.seq_off, g.adj_off, g.adj, g.walk_off, g.walk_vtx, g.top_order_map)
    seq = bytes(g.seq_concat)
    walks = [np.asarray(g.walk_vtx[g.walk_off[h]:g.walk_off[h + 1]]) for h in range(g.num_walks)]
    flat = np.frombuffer(seq, np.uint8)
    vlen = np.diff(g.seq_off)
    seqs = []
    for wv in walks:
        base = np.concatenate([[0], np.cumsum(vlen[wv])])
        seqs.append(flat[np.repeat(g.seq_off[wv] - base[:-1], vlen[wv]) + np.arange(base[-1])].tobytes())
    return dict(ctx=ctx, g=g, seq=seq, walks=walks, seqs=seqs, names=list(g.hap_id2name))


def _digest(c):
    return digest(c)


@pytest.mark.parametrize("ref_name", ["CHM13.0", "HG002.1"])
def test_mhc_every_walk_against_a_reference_walk(mhc, ref_name):
    from phi_amd.calls import apply
    r = mhc["names"].index(ref_name)
    n_same = n_short = 0
    for q in range(len(mhc["walks"])):
        got = mhc["ctx"].calls(r, walk=q)
        want = calls_ref_numpy(mhc["walks"][q], mhc["walks"][r], mhc["g"].seq_off, mhc["seq"])
        _same(got, want)
        assert apply(mhc["seqs"][r], got) == mhc["seqs"][q][got["query_span"][0]:got["query_span"][1]]
        if q == r:
            assert got["n_calls"] == 0
            continue
        assert got["n_calls"] > 10000 and np.all(np.diff(got["pos"]) > 0)
        assert max(np.diff(got["ref_off"]).max(), np.diff(got["alt_off"]).max()) > 8000          # alleles of many tiles of the fill
        ro, ao = got["ref_off"], got["alt_off"]
        n_same += sum(got["ref_bytes"][ro[k]:ro[k + 1]] == got["alt_bytes"][ao[k]:ao[k + 1]] for k in range(got["n_calls"]))
        n_short += got["ref_span"][1] < len(mhc["seqs"][r]) or got["query_span"][1] < len(mhc["seqs"][q])
    assert n_short > 0                                     # walks that end on an interior vertex: the called span ends before the walk
    if ref_name == "CHM13.0":
        assert n_same > 0                                  # a bubble whose two sides spell the same bytes


# ------------------------------------------------------------------ 4. the path

def test_calls_of_the_path(oracle, ctx_factory):
    from phi_amd import PHI_ERR_STATE, PhiError
    from phi_amd.calls import apply, ph_names
    n_recomb_with_calls = 0
    for seed in range(1, 9):
        rng = np.random.default_rng(100 * seed + 11)
        g = random_graph(rng, n_sites=12, n_walks=4, seg_len=(1, 400), alt_len=(1, 40), p_del=0.3)
        reads = mosaic_reads(rng, g, n_reads=60, read_len=70, n_seg=2, err=0.01)
        ctx = ctx_factory(k=9, w=4, threshold=1.0, recombination=3)
        _set(ctx, g)
        with pytest.raises(PhiError) as e:                 # no solved path yet
            ctx.calls(0)
        assert e.value.status == PHI_ERR_STATE
        ctx.add_reads(reads)
        res = ctx.solve()
        path = res["path_vtx"].tolist()
        hap_seq = ctx.path_sequence(res["hap_len"])
        for r in range(g.n_walks):
            got = ctx.calls(r)
            _same(got, calls_ref(path, g.paths[r], g.node_seq))
            assert apply(walk_sequence(g, r), got) == hap_seq[got["query_span"][0]:got["query_span"][1]]
            ph = ph_names(got, res["path_hap"], g.hap_names)
            assert ph == [g.hap_names[res["path_hap"][i + 1]] for i in got["anchor"].tolist()]
            # the tags change where the report's labels change: collapsed, they are a subsequence of the collapsed labels
            labels = [g.hap_names[h] for j, h in enumerate(res["path_hap"].tolist()) if j == 0 or h != res["path_hap"][j - 1]]
            tags = [t for j, t in enumerate(ph) if j == 0 or t != ph[j - 1]]
            it = iter(labels)
            assert all(t in it for t in tags), (tags, labels)
            if res["recombination_count"] > 0 and got["n_calls"] > 0:
                n_recomb_with_calls += 1
        ctx.close()
    assert n_recomb_with_calls > 0


# ------------------------------------------------------------------ 5. a panel; refusals

def test_calls_on_a_panel_graph_and_refusals(oracle, ctx_factory):
    from phi_amd import PHI_ERR_INVALID, PHI_ERR_UNSUPPORTED, PhiError
    from phi_amd.panel import induced_subgraph
    rng = np.random.default_rng(55)
    g = random_graph(rng, n_sites=12, n_walks=5, seg_len=(K + 1, 12), p_del=0.3)
    keep = np.array([1, 0, 1, 1, 0], bool)
    sub, _ = induced_subgraph(g, keep)
    ctx = ctx_factory(k=K, w=W, threshold=1.0, recombination=3)
    _set(ctx, g, keep=keep)
    for q in range(3):
        for r in range(3):
            _check_pair(ctx, sub, q, r)
    for q, r in ((3, 0), (0, 3), (-1, 0), (0, -1), (4, 4)):     # the ids are the panel's: three walks
        with pytest.raises(PhiError) as e:
            ctx.calls(r, walk=q)
        assert e.value.status == PHI_ERR_INVALID
    _check_pair(ctx, sub, 2, 1)                            # usable afterwards
    # no shared vertex: two disjoint walks
    d = _hand_graph([b"ACGTACGTAC", b"TTGACCGATA", b"GGATCCATGC", b"CATGCATTAG"], [(0, 1), (2, 3)], [[0, 1], [2, 3]])
    _set(ctx, d)
    with pytest.raises(PhiError) as e:
        ctx.calls(0, walk=1)
    assert e.value.status == PHI_ERR_UNSUPPORTED and "share no vertex" in e.value.detail
    _check_pair(ctx, d, 0, 0)
    _set(ctx, g)
    _check_pair(ctx, g, 4, 1)


# ------------------------------------------------------------------ 6. repeatability

def test_the_same_call_gives_the_same_bytes(mhc):
    ctx = mhc["ctx"]
    a = _digest(ctx.calls(0, walk=1))
    assert _digest(ctx.calls(0, walk=1)) == a
    other = _digest(ctx.calls(1, walk=3))
    assert other != a
    assert _digest(ctx.calls(0, walk=1)) == a
    st = ctx.calls_stats()
    assert st["n_calls"] > 10000 and st["bytes_moved"] > 0 and st["gpu_ms"] > 0


def test_mhc_calls_on_dirty_device_memory(mhc):
    """The MHC_4 case on a context whose every device buffer starts out poisoned and comes back from the pool with an earlier
    owner's contents, the way tests/test_gpu_dirty_memory.py dirties memory: the same digest as on clean memory."""
    from test_gpu_dirty_memory import VARIANTS
    want = _digest(mhc["ctx"].calls(0, walk=3))
    env = {k: v for k, v in os.environ.items() if k not in ("PHI_DEVICE_POISON", "PHI_DEVICE_POOL_MIN", "PHI_DEVICE_POOL")}
    env.update(VARIANTS["ff"])
    env.update(VARIANTS["pooled"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "calls_child.py"), "3", "0"], capture_output=True, text=True, timeout=240,
                       cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-300:] + r.stderr)[-3000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["digest"] == want
