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
    # (the host readers' graphs, a VcfGraph among them: their ranks are top_order_map; walk_vtx is None where the device holds the entries)
    out = dict(seq_concat=g.seq_concat, seq_off=g.seq_off, adj_off=g.adj_off, adj=g.adj, walk_off=g.walk_off, walk_vtx=getattr(g, "walk_vtx", None))
    rank = getattr(g, "top_rank", None)
    if rank is None:
        rank = getattr(g, "top_order_map", None)
    if rank is not None:
        out["top_rank"] = rank
    return out


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


def choose_panel(S, n_want, always=None):
    """The rule of phi_panel_choose (include/phi_host.h) restated in numpy: which n_want walks to keep, from S[block, walk] =
    read support per block of the graph and walk (Context.scout_scores).  It stands in for what `vg haplotypes` answers from
    the reads' k-mers (data/vg_haplotypes.py:21-29) and for the lists of names of data/chop_graph.sh:46-66; the rule is this
    project's own, it is not `vg haplotypes`' and has not been compared with it.
      1. the `always` walks are in (more of them than n_want: ValueError; 1 <= n_want <= min(walks, 1022))
      2. in block b the walks are ordered by (-S[b, h], h)
      3. round r: votes[h] = blocks whose r-th walk is h with S[b, h] > 0; walks with votes that are not yet in enter by
         (votes descending, total S[:, h].sum() descending, id ascending) until the panel holds n_want
      4. a round without votes ends the rounds; the rest is filled by (total descending, id ascending)
    Returns (keep uint8[walks], round_of int32[walks]: -1 always, r entered in round r, walks = the fill, -2 not chosen)."""
    S = np.asarray(S, np.int64)
    n_blocks, n_walks = S.shape
    keep = np.zeros(n_walks, np.uint8) if always is None else (np.asarray(always) != 0).astype(np.uint8)
    if keep.shape != (n_walks,):
        raise ValueError(f"always must hold one flag per walk ({n_walks})")
    if n_blocks < 1 or n_walks < 1 or not 1 <= n_want <= min(n_walks, 1022) or int(keep.sum()) > n_want:
        raise ValueError("choose_panel: n_want must lie in 1 .. min(walks, 1022) and hold the always-kept walks")
    round_of = np.where(keep != 0, -1, -2).astype(np.int32)
    total = S.sum(0)
    ids = np.arange(n_walks)
    order = np.argsort(-S, axis=1, kind="stable")               # (stable: equal scores stay in id order)
    n_in = int(keep.sum())
    for r in range(n_walks):
        if n_in >= n_want:
            break
        pick = order[:, r]
        pick = pick[S[np.arange(n_blocks), pick] > 0]
        if len(pick) == 0:
            break
        votes = np.bincount(pick, minlength=n_walks)
        cand = ids[(votes > 0) & (keep == 0)]
        cand = cand[np.lexsort((cand, -total[cand], -votes[cand]))][:n_want - n_in]
        keep[cand] = 1
        round_of[cand] = r
        n_in += len(cand)
    if n_in < n_want:
        rest = ids[keep == 0]
        rest = rest[np.lexsort((rest, -total[rest]))][:n_want - n_in]
        keep[rest] = 1
        round_of[rest] = n_walks
    return keep, round_of


def auto_panel(ctx, A, reads, n_want, always=None, n_blocks=0, chop=None, text=False):
    """The panel chosen from the reads, start to end, on one Context: a graph of thousands of walks in, the reads scored
    against a panel of n_want of them out (ctx.solve() follows).  In the place of `vg haplotypes` in front of the inference
    (data/vg_haplotypes.py:21-29) and of the panels by name of data/chop_graph.sh:46-66; the rule of the choice
    (choose_panel) is this project's own and has not been compared with `vg haplotypes`.
      1. scout    ctx.scout_graph: the index of every walk, no DP
      2. collect  the reads into a store on the device (ctx.collect_reads; text=True: pieces of FASTA / FASTQ text)
      3. score    ctx.collect_score: the hit vector of the full index
      4. scores   ctx.scout_scores(n_blocks): read support per block and walk, on the device
      5. choose   ctx.scout_choose(n_want, always)
      6. panel    ctx.set_graph(..., walk_vtx=None, keep=chosen, chop=chop, keep_reads=True) from the entries the scout retained
      7. score    ctx.collect_score: the same reads against the panel's index
    A: the arrays of set_graph as a dict (seq_concat, seq_off, adj_off, adj, walk_off, walk_vtx -- None for entries the device
    holds --, top_rank).  Returns a dict: keep, round_of, n_rounds, walk_off (the panel's), info (scout_scores'), n_reads,
    n_bases."""
    A = _as_arrays(A)
    ctx.scout_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A.get("walk_vtx"), A["top_rank"])
    n_reads, n_bases = ctx.collect_reads(reads, text=text)
    ctx.collect_score()
    _, info = ctx.scout_scores(n_blocks, copy=False)
    keep, round_of = ctx.scout_choose(n_want, always)
    walk_off = ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], None, None, chop=chop, keep=keep,
                             keep_reads=True)
    ctx.collect_score()
    entered = round_of[(round_of >= 0) & (round_of < len(round_of))]
    return dict(keep=keep, round_of=round_of, n_rounds=int(entered.max()) + 1 if len(entered) else 0, walk_off=walk_off, info=info,
                n_reads=n_reads, n_bases=n_bases)
