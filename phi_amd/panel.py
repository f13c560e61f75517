"""A panel of a graph's haplotypes: the rule of include/phi_amd.h phi_set_graph_panel restated in numpy, and the choice of
nested panels by sample name.

The reference builds one graph from the full VCF, removes samples from the haplotype index (data/chop_graph.sh:46-61
`vg gbwt ... -R SAMPLE`), writes one GFA per panel (:62-66) and runs PHI once per panel (data/run_batch_9.py to
run_batch_13.py); the sample lists are drawn nested by data/get_ids.py and data/get_ids_2.py.  Not compared with `vg`.

The rule.  Given a graph and a flag per walk, the panel graph is the subgraph induced by the kept walks:
  vertices  those on at least one kept walk, in their old order (new id = the number of kept vertices before it)
  edges     the edges (u, v) some kept walk steps along, in their old order within u's list; an edge between two kept
            vertices that no kept walk uses is dropped
  walks     the kept walks in their old order, entries renamed
  ranks     Kahn's algorithm with a FIFO queue on the panel graph, sources in id order (ILP_index.cpp:115-154): not the old
            ranks compressed
With every walk kept, vertices and edges on no walk still go.
"""
from collections import deque

import numpy as np

from .ladder import splitmix64


def kahn_ranks(adj_off, adj):
    """Topological ranks by Kahn's algorithm with a FIFO queue, sources in id order; ValueError for a cycle."""
    n = len(adj_off) - 1
    indeg = np.bincount(np.asarray(adj, np.int64), minlength=n).tolist() if len(adj) else [0] * n
    q = deque(i for i in range(n) if indeg[i] == 0)
    rank = [0] * n
    head = 0
    off, tgt = np.asarray(adj_off).tolist(), np.asarray(adj).tolist()
    while q:
        u = q.popleft()
        rank[u] = head
        head += 1
        for x in range(off[u], off[u + 1]):
            v = tgt[x]
            indeg[v] -= 1
            if indeg[v] == 0:
                q.append(v)
    if head != n:
        raise ValueError(f"graph is not acyclic: {head} of {n} vertices sorted")
    return np.asarray(rank, np.int32)


def _as_arrays(g):
    if isinstance(g, dict):
        return g
    if hasattr(g, "arrays"):
        return g.arrays()
    return dict(seq_concat=g.seq_concat, seq_off=g.seq_off, adj_off=g.adj_off, adj=g.adj, walk_off=g.walk_off, walk_vtx=g.walk_vtx)


def induced_arrays(A, keep):
    """The rule on the flat arrays of phi_set_graph (a dict with seq_concat, seq_off, adj_off, adj, walk_off, walk_vtx):
    (arrays of the panel graph with top_rank, old vertex ids of its vertices, old walk ids of its walks)."""
    seq_off, adj_off = np.asarray(A["seq_off"], np.int64), np.asarray(A["adj_off"], np.int64)
    adj, walk_off, walk_vtx = np.asarray(A["adj"], np.int64), np.asarray(A["walk_off"], np.int64), np.asarray(A["walk_vtx"], np.int64)
    n_vtx, n_walks = len(seq_off) - 1, len(walk_off) - 1
    keep = np.asarray(keep).astype(bool)
    if keep.shape != (n_walks,):
        raise ValueError(f"keep must hold one flag per walk ({n_walks})")
    kept = np.flatnonzero(keep)
    if len(kept) == 0:
        raise ValueError("no walk is kept")
    lens = np.diff(walk_off)
    ent_keep = np.repeat(keep, lens)
    ent = walk_vtx[ent_keep]
    used_vtx = np.zeros(n_vtx, bool)
    used_vtx[ent] = True
    # the steps of the kept walks: entry e -> e + 1 inside one walk
    last = np.zeros(len(walk_vtx), bool)
    last[walk_off[1:] - 1] = True
    step = ent_keep & ~last
    su, sv = walk_vtx[np.flatnonzero(step)], walk_vtx[np.flatnonzero(step) + 1]
    eu = np.repeat(np.arange(n_vtx, dtype=np.int64), np.diff(adj_off))
    stepped = np.unique(su * n_vtx + sv)
    used_edge = np.isin(eu * n_vtx + adj, stepped)
    origin = np.flatnonzero(used_vtx)
    new_id = np.full(n_vtx, -1, np.int64)
    new_id[origin] = np.arange(len(origin))
    seq = np.frombuffer(bytes(A["seq_concat"]), np.uint8) if not isinstance(A["seq_concat"], np.ndarray) else A["seq_concat"]
    vlen = np.diff(seq_off)
    base_keep = np.repeat(used_vtx, vlen)
    seq_off2 = np.concatenate([[0], np.cumsum(vlen[origin])]).astype(np.int64)
    deg2 = np.bincount(eu[used_edge], minlength=n_vtx)[origin] if len(adj) else np.zeros(len(origin), np.int64)
    adj_off2 = np.concatenate([[0], np.cumsum(deg2)]).astype(np.int64)
    adj2 = new_id[adj[used_edge]].astype(np.int32)
    out = dict(seq_concat=seq[base_keep].tobytes(), seq_off=seq_off2, adj_off=adj_off2, adj=adj2,
               walk_off=np.concatenate([[0], np.cumsum(lens[kept])]).astype(np.int64), walk_vtx=new_id[ent].astype(np.int32))
    out["top_rank"] = kahn_ranks(adj_off2, adj2)
    return out, origin.astype(np.int32), kept.astype(np.int32)


def induced_subgraph(g, keep):
    """The rule on an oracle-style graph (node_seq, adj, paths, hap_names; the result is of the same class, with Kahn's
    ranks) or on a dict of the flat arrays (the result is a dict): (panel graph, old vertex ids of its vertices)."""
    if isinstance(g, dict) or not hasattr(g, "node_seq"):
        out, origin, _ = induced_arrays(_as_arrays(g), keep)
        return out, origin
    out, origin, kept = induced_arrays(g.arrays(), keep)
    off, tgt = out["adj_off"].tolist(), out["adj"].tolist()
    woff, wv = out["walk_off"].tolist(), out["walk_vtx"].tolist()
    rank = out["top_rank"]
    sub = type(g)(seg_names=[g.seg_names[v] for v in origin.tolist()], node_seq=[g.node_seq[v] for v in origin.tolist()],
                  adj=[tgt[off[j]:off[j + 1]] for j in range(len(origin))],
                  paths=[wv[woff[h]:woff[h + 1]] for h in range(len(kept))], hap_names=[g.hap_names[h] for h in kept.tolist()],
                  top_order=np.argsort(rank).tolist(), top_rank=rank.tolist())
    return sub, origin


def sample_of(hap_name):
    """The W-line's sample field of a haplotype name "<sample>.<haplotype index>" (a sample name may itself hold dots)."""
    return hap_name.rsplit(".", 1)[0] if "." in hap_name else hap_name


def samples_in_order(hap_names):
    """The distinct samples of the haplotype names, in the order of their first walk."""
    seen = {}
    for n in hap_names:
        seen.setdefault(sample_of(n), None)
    return list(seen)


def keep_mask(hap_names, keep_samples=None, drop_samples=None):
    """One flag per walk from a list of samples to keep, or to drop; ValueError listing the names the graph does not hold."""
    if (keep_samples is None) == (drop_samples is None):
        raise ValueError("give keep_samples or drop_samples, not both")
    names = list(keep_samples if keep_samples is not None else drop_samples)
    have = set(sample_of(n) for n in hap_names)
    missing = [n for n in names if n not in have]
    if missing:
        raise ValueError("the graph holds no sample named " + ", ".join(missing))
    chosen = set(names)
    m = np.array([sample_of(n) in chosen for n in hap_names], bool)
    return m if keep_samples is not None else ~m


def nested_panels(samples, sizes, seed, always=()):
    """Nested panels of samples, as data/get_ids.py and data/get_ids_2.py nest theirs: the samples that are not in `always`
    are keyed by splitmix64(seed, ordinal) -- the ordinal counted over those samples in their given order --, ties by ordinal;
    panel j is `always` (in the given order) plus the first sizes[j] of them.  sizes ascend."""
    always = list(always)
    missing = [a for a in always if a not in samples]
    if missing:
        raise ValueError("the graph holds no sample named " + ", ".join(missing))
    rest = [s for s in samples if s not in set(always)]
    sizes = [int(x) for x in sizes]
    if any(x < 0 or x > len(rest) for x in sizes) or any(b < a for a, b in zip(sizes, sizes[1:])):
        raise ValueError(f"panel sizes must ascend within 0 .. {len(rest)}")
    keys = splitmix64(seed, np.arange(len(rest)))
    order = sorted(range(len(rest)), key=lambda i: (int(keys[i]), i))
    return [always + [rest[i] for i in order[:n]] for n in sizes]
