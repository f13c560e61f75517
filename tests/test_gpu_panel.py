"""A panel of a graph's haplotypes inside "set graph" (phi_set_graph_panel: data/chop_graph.sh:46-66 done by the library, the kept
walk entries marked and renamed on the device by phi_amd/csrc/panel.hip) against the rule restated in numpy
(phi_amd.panel.induced_subgraph, pinned to the host reader by tests/test_cpu_panel.py) and, through it, against the CPU oracle on
the panel graph.  Every comparison is exact."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from graphgen import mosaic_reads, random_graph
from test_cpu_chop import chop_numpy
from test_gpu_chop import _dirty, _same_run, _write_gfa
from test_gpu_parity import _check_against_oracle

pytestmark = pytest.mark.gpu

PANEL_TILE = 4096                                          # phi_amd/csrc/panel.hip
K, W, T, R = 9, 4, 1.0, 3


def _n_edges(g):
    return sum(len(a) for a in g.adj)


def _with_private_walks(rng, g):
    """A private allele on a new first and a new last walk, and one allele on no walk at all: whatever mask drops the first
    or the last walk loses a vertex and two edges, and every mask -- "all" included -- loses the unused allele."""
    from oracle import oracle as O

    def add(a, b):
        v = len(g.node_seq)
        g.node_seq.append(bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(1, 41))).tolist()))
        g.seg_names.append(f"s{v + 1}")
        g.adj.append([b])
        g.adj[a].append(v)                                 # (the largest id: the list stays sorted)
        return v
    p, q = g.paths[0], g.paths[-1]
    first = p[:1] + [add(p[0], p[1])] + p[1:]
    last = q[:-1] + [add(q[-2], q[-1])] + q[-1:]
    add(p[1], p[2])
    g.paths = [first] + g.paths + [last]
    g.hap_names = [f"hap{h}.{h}" for h in range(len(g.paths))]
    O.kahn(g)
    return g


# (walks, sites): 3 walks (brute force), few walks over many sites (what loses vertices by itself), 9 walks, 70 walks (the
# blocks' rows on class lanes)
GRAPHS = [(1, 3, 4), (2, 5, 40), (3, 9, 6), (4, 70, 5)]
MASKS = ["all", "every_other", "first_only", "last_only", "without_first", "without_last"]


def _mask(name, n):
    m = np.ones(n, bool)
    if name == "every_other":
        m = np.arange(n) % 2 == 0
    elif name == "first_only":
        m[1:] = False
    elif name == "last_only":
        m[:-1] = False
    elif name == "without_first":
        m[0] = False
    elif name == "without_last":
        m[-1] = False
    return m


@functools.lru_cache(maxsize=None)
def _graph_and_reads(seed, n_walks, n_sites):
    rng = np.random.default_rng(100 * seed + 11)
    g = random_graph(rng, n_sites=n_sites, n_walks=n_walks - 2, seg_len=(1, 400), alt_len=(1, 40), p_del=0.3)
    _with_private_walks(rng, g)
    _dirty(rng, g)
    return g, mosaic_reads(rng, g, n_reads=60, read_len=70, n_seg=2, err=0.01)


def _set(ctx, g, **kw):
    A = g.arrays()
    return ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"], **kw)


def _reference(g, keep, chop):
    """(the graph context a is set with, old vertex of each of its vertices, the induced subgraph)"""
    from phi_amd.panel import induced_subgraph
    sub, origin = induced_subgraph(g, keep)
    # not vacuous: the mask drops at least one vertex and one edge, or keeps a single walk
    assert int(np.sum(keep)) == 1 or (g.n_vtx - sub.n_vtx >= 1 and _n_edges(g) - _n_edges(sub) >= 1)
    if chop is None:
        return sub, origin, sub, None
    c, ov, _ = chop_numpy(sub, chop)
    return c, origin[ov], sub, ov


def _check_panel_accessors(b, g, keep, sub, origin_of_set, path_vtx, chop):
    pv = b.chop_origin(path_vtx)[0] if chop is not None else path_vtx
    assert np.array_equal(b.panel_origin(pv), origin_of_set[path_vtx])
    assert np.array_equal(b.panel_walks(), np.flatnonzero(keep))
    ps = b.panel_stats()
    assert (ps["n_walks_in"], ps["n_walks_out"], ps["n_vtx_in"], ps["n_vtx_out"]) == (g.n_walks, sub.n_walks, g.n_vtx, sub.n_vtx)
    assert (ps["n_edges_in"], ps["n_edges_out"]) == (_n_edges(g), _n_edges(sub))
    assert (ps["n_entries_in"], ps["n_entries_out"]) == (sum(len(p) for p in g.paths), sum(len(p) for p in sub.paths))
    assert ps["mark_gpu_ms"] > 0 and ps["remap_gpu_ms"] > 0 and ps["scan_gpu_ms"] > 0


# ------------------------------------------------------------------ 1. equals setting the induced subgraph

@pytest.mark.parametrize("chop", [None, 7, 30])
@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("seed,n_walks,n_sites", GRAPHS)
def test_panel_equals_setting_the_induced_subgraph(oracle, ctx_factory, seed, n_walks, n_sites, mask_name, chop):
    g, reads = _graph_and_reads(seed, n_walks, n_sites)
    keep = _mask(mask_name, g.n_walks)
    c, origin_of_set, sub, _ = _reference(g, keep, chop)
    a = ctx_factory(k=K, w=W, threshold=T, recombination=R)
    b = ctx_factory(k=K, w=W, threshold=T, recombination=R)
    try:
        _set(a, c)
        a.add_reads(reads)
        st, res_a, m = _check_against_oracle(oracle, a, c, reads, K, W, T, R)     # the yardstick: the oracle on the panel graph
        if g.n_walks <= 3:
            assert res_a["objective"] == m.brute_force()[0]
        woff = _set(b, g, keep=keep, chop=chop)
        assert np.array_equal(woff, c.arrays()["walk_off"])
        b.add_reads(reads)
        rb = _same_run(a, b, c.n_walks, res_a)
        _check_panel_accessors(b, g, keep, sub, origin_of_set, rb["path_vtx"], chop)
        if chop is None:
            with pytest.raises(Exception):
                b.chop_stats()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 2. walks on the device

@pytest.mark.parametrize("chop", [None, 7])
@pytest.mark.parametrize("mask_name", ["every_other", "without_first", "last_only"])
def test_panel_of_walks_resolved_on_the_device(oracle, ctx_factory, tmp_path, mask_name, chop):
    from phi_amd import ilp_index as H
    g, reads = _graph_and_reads(2, 5, 40)
    keep = _mask(mask_name, g.n_walks)
    c, origin_of_set, sub, _ = _reference(g, keep, chop)
    path = _write_gfa(g, tmp_path / "full.gfa")
    a = ctx_factory(k=K, w=W, threshold=T, recombination=R)
    b = ctx_factory(k=K, w=W, threshold=T, recombination=R)
    try:
        dg = H.DeferredGraph(path)
        assert dg.resolve_on_device(b) and dg.walk_vtx is None
        assert dg.seq_off.tolist() == g.arrays()["seq_off"].tolist() and dg.adj.tolist() == g.arrays()["adj"].tolist()
        _set(a, c)
        a.add_reads(reads)
        st, res_a, m = _check_against_oracle(oracle, a, c, reads, K, W, T, R)
        woff = dg.set_graph(b, keep=keep, chop=chop)
        A = c.arrays()
        assert np.array_equal(woff, A["walk_off"]) and np.array_equal(b.walk_entries(), A["walk_vtx"])
        b.add_reads(reads)
        rb = _same_run(a, b, c.n_walks, res_a)
        _check_panel_accessors(b, g, keep, sub, origin_of_set, rb["path_vtx"], chop)
        # the device-resident walks were consumed, and nothing was retained
        import phi_amd
        with pytest.raises(phi_amd.PhiError) as e:
            dg.set_graph(b, keep=keep)
        assert e.value.status == phi_amd.PHI_ERR_STATE
        _set(b, g)                                                      # the context takes host entries next, as a whole graph
        assert np.array_equal(b.walk_entries(), g.arrays()["walk_vtx"])
        with pytest.raises(phi_amd.PhiError):
            b.panel_stats()
    finally:
        a.close()
        b.close()


def _reads_of_arrays(rng, A, n=40, length=60):
    seq, so, wo, wv = np.frombuffer(A["seq_concat"], np.uint8), A["seq_off"], A["walk_off"], A["walk_vtx"]
    out = []
    for _ in range(n):
        h = int(rng.integers(0, len(wo) - 1))
        s = b"".join(seq[so[v]:so[v + 1]].tobytes() for v in wv[wo[h]:wo[h + 1]].tolist())
        at = int(rng.integers(0, max(1, len(s) - length)))
        out.append(s[at:at + length])
    return out


def _graph_arrays(g):
    return dict(seq_concat=g.seq_concat.tobytes(), seq_off=g.seq_off, adj_off=g.adj_off, adj=g.adj, walk_off=g.walk_off, walk_vtx=g.walk_vtx)


def _set_arrays(ctx, A, **kw):
    return ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A.get("top_rank"), **kw)


def test_panel_of_a_vcf(ctx_factory, tmp_path):
    """set_graph_vcf(keep_samples=...): the graph of ALL samples' records (vcf2gfa.build), then the induced subgraph."""
    from phi_amd.panel import induced_arrays, keep_mask, sample_of
    from test_gpu_vcf import _python_graph, _random_case
    rng = np.random.default_rng(11)
    done = 0
    for case in range(8):
        vcf, fa = _random_case(rng, tmp_path, case)
        g, _ = _python_graph(vcf, fa, tmp_path, 30)
        samples = list(dict.fromkeys(sample_of(n) for n in g.hap_id2name))
        if len(samples) < 4:
            continue
        names = ["REF"] + samples[1::3] if case % 2 else samples[2::2]           # (with and without the reference walk)
        keep = keep_mask(g.hap_id2name, keep_samples=names)
        S, origin, kept = induced_arrays(_graph_arrays(g), keep)
        a = ctx_factory(k=5, w=3, threshold=T, recombination=R)
        b = ctx_factory(k=5, w=3, threshold=T, recombination=R)
        try:
            _set_arrays(a, S)
            v = b.set_graph_vcf(vcf, fa, keep_samples=names)
            assert v.hap_id2name == [g.hap_id2name[h] for h in kept.tolist()] and np.array_equal(v.kept_haps, kept)
            assert np.array_equal(v.walk_off, S["walk_off"]) and np.array_equal(b.walk_entries(), S["walk_vtx"])
            assert np.array_equal(b.panel_origin(np.arange(len(origin))), origin)
            ps = b.panel_stats()
            assert (ps["n_walks_in"], ps["n_walks_out"], ps["n_vtx_in"], ps["n_vtx_out"]) == (len(kept), len(kept), g.n_vtx, len(origin))
            reads = _reads_of_arrays(rng, S)
            a.add_reads(reads)
            b.add_reads(reads)
            _same_run(a, b, len(kept))
            done += 1
        finally:
            a.close()
            b.close()
    assert done >= 3


# ------------------------------------------------------------------ 3. tiles

def _entries_equal(ctx_factory, g, keep, k=5, w=2):
    from phi_amd.panel import induced_subgraph
    sub, origin = induced_subgraph(g, keep)
    A = sub.arrays()
    ctx = ctx_factory(k=k, w=w)
    try:
        woff = _set(ctx, g, keep=keep)
        assert np.array_equal(woff, A["walk_off"])
        assert np.array_equal(ctx.walk_entries(), A["walk_vtx"])
        assert np.array_equal(ctx.panel_origin(np.arange(sub.n_vtx)), origin)
        ps = ctx.panel_stats()
        assert (ps["n_vtx_out"], ps["n_edges_out"], ps["n_entries_out"]) == (sub.n_vtx, _n_edges(sub), len(A["walk_vtx"]))
    finally:
        ctx.close()
    return len(A["walk_vtx"])


def test_a_kept_walk_longer_than_two_tiles(ctx_factory):
    rng = np.random.default_rng(5)
    g = random_graph(rng, n_sites=5600, n_walks=3, seg_len=(1, 3), alt_len=(1, 3), p_del=0.3)
    assert min(len(g.paths[0]), len(g.paths[2])) > 2 * PANEL_TILE
    _entries_equal(ctx_factory, g, np.array([True, False, True]))


@pytest.mark.parametrize("parity", [0, 1])
def test_more_kept_walks_in_a_tile_than_lanes(ctx_factory, parity):
    """1 100 walks of about a dozen entries, every other kept: some 340 kept walks start inside one tile, a dropped walk lies
    between any two kept ones, and (parity 1) the first walk is dropped, (parity 0) the last."""
    rng = np.random.default_rng(6)
    g = random_graph(rng, n_sites=7, n_walks=1100, seg_len=(1, 30), alt_len=(1, 9), p_del=0.3)
    assert max(len(p) for p in g.paths) * 256 < PANEL_TILE
    keep = np.arange(1100) % 2 == parity
    assert keep[0] != keep[-1]
    _entries_equal(ctx_factory, g, keep)


def test_kept_totals_of_every_residue_modulo_four(ctx_factory):
    rng = np.random.default_rng(8)
    g, _ = _graph_and_reads(3, 9, 6)
    lens = np.array([len(p) for p in g.paths])
    seen = {}
    for _ in range(200):
        keep = rng.random(g.n_walks) < 0.5
        if keep.any() and int(lens[keep].sum()) % 4 not in seen:
            seen[int(lens[keep].sum()) % 4] = keep
    assert sorted(seen) == [0, 1, 2, 3]
    for r, keep in seen.items():
        assert _entries_equal(ctx_factory, g, keep, k=K, w=W) % 4 == r


# ------------------------------------------------------------------ 4. the walk limit

def test_walk_limit_applies_to_the_kept_walks(oracle, ctx_factory):
    import phi_amd
    from phi_amd.panel import induced_subgraph
    rng = np.random.default_rng(21)
    g = random_graph(rng, n_sites=4, n_walks=1100, seg_len=(1, 90), alt_len=(1, 20), p_del=0.3)
    reads = mosaic_reads(rng, g, n_reads=40, read_len=50, n_seg=2, err=0.01)
    keep = np.arange(1100) % 2 == 0
    sub, origin = induced_subgraph(g, keep)
    a = ctx_factory(k=5, w=2, threshold=T, recombination=R)
    b = ctx_factory(k=5, w=2, threshold=T, recombination=R)
    try:
        with pytest.raises(phi_amd.PhiError) as e:
            _set(b, g)                                                 # the whole graph is refused as ever
        assert e.value.status == phi_amd.PHI_ERR_UNSUPPORTED and "more than 1022 walks" in str(e.value)
        many = np.ones(1100, bool)
        many[1023:] = False
        with pytest.raises(phi_amd.PhiError) as e:
            _set(b, g, keep=many)
        assert e.value.status == phi_amd.PHI_ERR_UNSUPPORTED and "more than 1022 walks" in str(e.value)
        _set(a, sub)
        a.add_reads(reads)
        res_a = a.solve()
        assert res_a["optimal"] == 1
        _set(b, g, keep=keep)                                          # the context takes the 550-walk panel next
        b.add_reads(reads)
        rb = _same_run(a, b, sub.n_walks, res_a)
        assert np.array_equal(b.panel_origin(rb["path_vtx"]), origin[rb["path_vtx"]])
        assert b.panel_stats()["n_walks_in"] == 1100 and b.panel_stats()["n_walks_out"] == 550
    finally:
        a.close()
        b.close()


def test_vcf_of_600_diploid_samples_with_300_kept(ctx_factory, tmp_path):
    import phi_amd
    from phi_amd.panel import induced_arrays, keep_mask
    from test_gpu_vcf import _python_graph, _write_case
    rng = np.random.default_rng(23)
    ref = bytes(rng.choice(list(b"ACGT"), size=400).tolist())
    samples = [f"S{i}" for i in range(600)]

    def other(b):
        return b"C" if b != b"C" else b"G"
    recs = [(p, ref[p:p + 1], [other(ref[p:p + 1])], [b"%d|%d" % (rng.integers(0, 2), rng.integers(0, 2)) for _ in samples]) for p in (50, 120, 200, 310)]
    vcf, fa = _write_case(tmp_path, "many", ref, samples, recs)
    ctx = ctx_factory(k=5, w=3)
    try:
        with pytest.raises(phi_amd.PhiError) as e:
            ctx.set_graph_vcf(vcf, fa)                                 # 1 201 haplotypes: refused as before
        assert e.value.status == phi_amd.PHI_ERR_UNSUPPORTED and "1022" in str(e.value)
        names = samples[::2]
        v = ctx.set_graph_vcf(vcf, fa, keep_samples=names)
        assert v.num_walks == 600
        g, _ = _python_graph(vcf, fa, tmp_path, 30)
        S, origin, kept = induced_arrays(_graph_arrays(g), keep_mask(g.hap_id2name, keep_samples=names))
        assert np.array_equal(v.walk_off, S["walk_off"]) and np.array_equal(ctx.walk_entries(), S["walk_vtx"])
        assert np.array_equal(ctx.panel_origin(np.arange(len(origin))), origin)
        ctx.add_reads(_reads_of_arrays(rng, S, n=20, length=40))
        assert ctx.solve()["optimal"] == 1
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. retain

def test_a_ladder_of_panels_from_one_upload(ctx_factory):
    import phi_amd
    from phi_amd.panel import induced_subgraph, keep_mask, nested_panels, samples_in_order
    g, reads = _graph_and_reads(3, 9, 6)
    A = g.arrays()
    samples = samples_in_order(g.hap_names)
    panels = nested_panels(samples, [1, 3, 6], seed=3, always=[samples[0]])
    masks = [keep_mask(g.hap_names, keep_samples=p) for p in panels]
    assert [int(m.sum()) for m in masks] == [2, 4, 7] and all((a <= b).all() for a, b in zip(masks, masks[1:]))
    fresh = []
    for m in masks:
        sub, _ = induced_subgraph(g, m)
        f = ctx_factory(k=K, w=W, threshold=T, recombination=R)
        _set(f, sub)
        f.add_reads(reads)
        fresh.append((f, sub, f.solve()))
    ctx = ctx_factory(k=K, w=W, threshold=T, recombination=R)
    try:
        with pytest.raises(phi_amd.PhiError) as e:                     # nothing resolved, nothing retained
            _set_arrays(ctx, dict(A, walk_vtx=None), keep=masks[0])
        assert e.value.status == phi_amd.PHI_ERR_STATE
        order = [0, 1, 2, 2, 1, 0]
        for step, j in enumerate(order):
            _set_arrays(ctx, A if step == 0 else dict(A, walk_vtx=None), keep=masks[j], retain=True)
            ctx.add_reads(reads)
            f, sub, res = fresh[j]
            _same_run(f, ctx, sub.n_walks, res)
        # a larger, different graph on the same context (not a panel), then a panel again from the retained entries
        big, big_reads = _graph_and_reads(2, 5, 40)
        _set(ctx, big)
        ctx.add_reads(big_reads)
        ctx.solve()
        _set_arrays(ctx, dict(A, walk_vtx=None), keep=masks[1], retain=True)
        ctx.add_reads(reads)
        _same_run(fresh[1][0], ctx, fresh[1][1].n_walks, fresh[1][2])
        # other walks than the retained ones are not taken for them
        with pytest.raises(phi_amd.PhiError) as e:
            B = big.arrays()
            _set_arrays(ctx, dict(B, walk_vtx=None), keep=np.ones(big.n_walks, bool))
        assert e.value.status == phi_amd.PHI_ERR_STATE
        ctx.panel_release()
        with pytest.raises(phi_amd.PhiError) as e:
            _set_arrays(ctx, dict(A, walk_vtx=None), keep=masks[0])
        assert e.value.status == phi_amd.PHI_ERR_STATE
        _set_arrays(ctx, A, keep=masks[0])                             # usable
        ctx.add_reads(reads)
        _same_run(fresh[0][0], ctx, fresh[0][1].n_walks, fresh[0][2])
    finally:
        ctx.close()
        for f, _, _ in fresh:
            f.close()


# ------------------------------------------------------------------ 6. refusals

def test_refusals_leave_the_context_usable(ctx_factory):
    import phi_amd
    g, reads = _graph_and_reads(3, 9, 6)
    A = g.arrays()
    keep = _mask("without_first", g.n_walks)
    ctx = ctx_factory(k=K, w=W, threshold=T, recombination=R)

    def usable():
        _set(ctx, g, keep=keep)
        ctx.add_reads(reads)
        assert ctx.solve()["optimal"] == 1
    try:
        with pytest.raises(phi_amd.PhiError) as e:
            _set(ctx, g, keep=np.zeros(g.n_walks, bool))
        assert e.value.status == phi_amd.PHI_ERR_INVALID and "no walk is kept" in str(e.value)
        usable()
        # a vertex out of range in a kept walk: the walk and the vertex are named ...
        wv = A["walk_vtx"].copy()
        at = int(A["walk_off"][2]) + 1
        wv[at] = g.n_vtx + 5
        with pytest.raises(phi_amd.PhiError) as e:
            _set_arrays(ctx, dict(A, walk_vtx=wv), keep=keep)
        assert e.value.status == phi_amd.PHI_ERR_WALK and f"walk 2 holds vertex {g.n_vtx + 5} out of range" in str(e.value)
        with pytest.raises(phi_amd.PhiError) as e:
            ctx.solve()
        assert e.value.status == phi_amd.PHI_ERR_STATE
        usable()
        # ... and the smallest such entry is the one reported
        wv2 = wv.copy()
        wv2[int(A["walk_off"][5])] = -3
        with pytest.raises(phi_amd.PhiError) as e:
            _set_arrays(ctx, dict(A, walk_vtx=wv2), keep=keep)
        assert f"walk 2 holds vertex {g.n_vtx + 5} out of range" in str(e.value)
        # in a dropped walk it is no error
        wv = A["walk_vtx"].copy()
        wv[1] = g.n_vtx + 5
        wv[2] = -1
        _set_arrays(ctx, dict(A, walk_vtx=wv), keep=keep)
        ctx.add_reads(reads)
        r1 = ctx.solve()
        usable()
        assert ctx.solve()["objective"] == r1["objective"]
        # a step without a graph edge: set_graph reports it on the panel graph
        wv = A["walk_vtx"].copy()
        wv[at] = wv[at - 1]
        with pytest.raises(phi_amd.PhiError) as e:
            _set_arrays(ctx, dict(A, walk_vtx=wv), keep=keep)
        assert e.value.status == phi_amd.PHI_ERR_WALK and "walk 1 steps" in str(e.value)    # (walk 2 is panel walk 1)
        usable()
        for bad in (np.ones(g.n_walks + 1, bool), np.ones(g.n_walks - 1, bool), np.ones((g.n_walks, 1), bool)):
            with pytest.raises(ValueError):
                _set(ctx, g, keep=bad)
        with pytest.raises(ValueError):
            _set(ctx, g, retain=True)
        usable()
        for call in (ctx.panel_stats, ctx.panel_walks, lambda: ctx.panel_origin([0])):
            call()
        with pytest.raises(phi_amd.PhiError) as e:
            ctx.panel_origin([10 ** 6])
        assert e.value.status == phi_amd.PHI_ERR_INVALID
        _set(ctx, g)                                                   # not a panel any more
        for call in (ctx.panel_stats, ctx.panel_walks, lambda: ctx.panel_origin([0])):
            with pytest.raises(phi_amd.PhiError) as e:
                call()
            assert e.value.status == phi_amd.PHI_ERR_STATE
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7. recycled memory

def test_recycled_device_memory_changes_nothing():
    """tests/panel_child.py -- a panel, a chopped panel and a retained ladder, each asserted against the numpy rule in the child
    -- once plain, once with every buffer poisoned, once with every buffer recycled through the pool: equal digests.  One
    child at a time; after a child that ends on a signal, with status 134 or 139 or at its limit nothing more is started."""
    import __graft_entry__
    __graft_entry__.ensure_built()
    digests = {}
    for name, extra in (("plain", {}), ("poison", {"PHI_DEVICE_POISON": "255"}), ("pool", {"PHI_DEVICE_POOL_MIN": "256"})):
        env = {k: v for k, v in os.environ.items() if k not in ("PHI_DEVICE_POISON", "PHI_DEVICE_POOL_MIN", "PHI_DEVICE_POOL")}
        env.update(extra)
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "panel_child.py")], capture_output=True, text=True, timeout=120,
                               cwd=ROOT, env=env)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"{name}: no end after {e.timeout} s; nothing more is started")
        tail = (r.stdout[-300:] + r.stderr)[-3000:]
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stdout + r.stderr:
            pytest.fail(f"{name}: exit status {r.returncode}; nothing more is started\n{tail}")
        assert r.returncode == 0, tail
        digests[name] = json.loads(r.stdout.strip().splitlines()[-1])
        assert digests[name] and all(digests[name].values())
    assert digests["poison"] == digests["plain"] and digests["pool"] == digests["plain"]
