"""dp_ref.py -- the additive relaxation one DP run of the solve computes, stated plainly (test infrastructure).

Written from the transition list at the top of phi_amd/csrc/dp.hip and from Model.successors (oracle/solve_oracle.py), from no
kernel: no run-length classes, no tops, no steps, int64 throughout.

    state (h, i): walk h at its position i, on vertex v = paths[h][i]
    F[h][i] = best value of a path that ENTERS walk h at i:   0 if i == 0;  G[h'][j] - cost over the in-edges u -> v and the
              walks h' on u at a non-last position j with paths[h'][j + 1] != v (a recombination; h' == h is one too)
    G[h][i] = max over s <= i of  F[h][s] + #{anchors of h of weight 1 with s <= t0 and t1 <= i}
    ends[h] = G[h][last position of h];   value = max(ends);   end walk = the lowest h that attains it
    cost    = 2 * (R // 2)

Per walk one vector of run values, indexed by the position s the run entered at: an anchor (t0, t1) that ends at i adds its
weight to the prefix [: t0 + 1].  Several weight vectors go through together (one more axis, nothing else).
"""
import numpy as np

NONE = -(1 << 60)              # "no state"; values stay above NONE / 2 when a state exists


def dp_anchors(kept):
    """The dp anchors [(walk, t0, t1)] of Context.kept_anchors(): the kept anchors that span an edge, in kept order."""
    _, wk, t0, t1 = kept
    return [(int(h), int(a), int(b)) for h, a, b in zip(wk.tolist(), t0.tolist(), t1.tolist()) if b > a]


def repeat_weights(kept):
    """The solve's own first relaxation: 0 on every dp anchor of a minimiser that has two dp anchors on one walk, 1 elsewhere."""
    hs, wk, t0, t1 = kept
    rows = [(int(r), int(h)) for r, h, a, b in zip(hs.tolist(), wk.tolist(), t0.tolist(), t1.tolist()) if b > a]
    seen, repeated = set(), set()
    for rh in rows:
        if rh in seen:
            repeated.add(rh[0])
        seen.add(rh)
    return np.array([0 if r in repeated else 1 for r, _ in rows], np.uint8)


def dp_ref_many(paths, adj, top_rank, anchors, weights, cost):
    """weights: (n_vectors, n_anchors) of 0 / 1.  Returns ends as an int64 array (n_vectors, n_walks); NONE where no state exists."""
    W = np.atleast_2d(np.asarray(weights, np.int64))
    assert W.shape[1] == len(anchors), (W.shape, len(anchors))
    nv, cost = W.shape[0], int(cost)
    n_vtx = len(adj)
    ending = {}                                            # (h, t1) -> [(t0, anchor index)]
    for a, (h, t0, t1) in enumerate(anchors):
        assert 0 <= t0 < t1 < len(paths[h]), (h, t0, t1)
        ending.setdefault((h, t1), []).append((t0, a))
    on = [[] for _ in range(n_vtx)]                        # vertex -> [(h, i)]
    for h, p in enumerate(paths):
        for i, v in enumerate(p):
            on[v].append((h, i))
    pred = [[] for _ in range(n_vtx)]
    for u in range(n_vtx):
        for v in adj[u]:
            pred[v].append(u)
    run = [np.full((nv, len(p)), NONE, np.int64) for p in paths]
    leaving = [dict() for _ in range(n_vtx)]               # u -> {next vertex of the walk: best G of the walks on u that go there}
    ends = np.full((nv, len(paths)), NONE, np.int64)
    for v in sorted(range(n_vtx), key=lambda x: top_rank[x]):
        if not on[v]:
            continue
        entry = np.full(nv, NONE, np.int64)
        for u in pred[v]:
            for nxt, g in leaving[u].items():
                if nxt != v:                               # the walk's own edge is no recombination
                    entry = np.maximum(entry, g)
        entry = np.where(entry > NONE // 2, entry - cost, NONE)
        for h, i in on[v]:
            r = run[h]
            r[:, i] = np.maximum(entry, 0) if i == 0 else entry
            for t0, a in ending.get((h, i), ()):
                r[:, : t0 + 1] += W[:, a, None]
            g = r[:, : i + 1].max(axis=1)
            g = np.where(g > NONE // 2, g, NONE)
            if i == len(paths[h]) - 1:
                ends[:, h] = g                             # (a walk that ends here cannot leave)
            else:
                nxt = paths[h][i + 1]
                leaving[v][nxt] = np.maximum(leaving[v][nxt], g) if nxt in leaving[v] else g
    return ends


def dp_ref(paths, adj, top_rank, anchors, weights, cost):
    """One weight vector.  Returns (ends: list with None where no state exists, value, end walk)."""
    ends = dp_ref_many(paths, adj, top_rank, anchors, [weights], cost)[0]
    return summary(ends)


def summary(ends_row):
    ends = [None if e <= NONE // 2 else int(e) for e in ends_row.tolist()]
    have = [e for e in ends if e is not None]
    value = max(have) if have else None
    return ends, value, (ends.index(value) if have else None)


# ---------------------------------------------------------------------------------------------------------- the scorer
class _NoAnchors:
    a_r = a_h = a_t0 = a_t1 = np.zeros(0, np.int32)


class _G:
    def __init__(self, paths, adj):
        self.paths, self.adj, self.n_vtx = paths, adj, len(adj)


def feasibility_model(paths, adj):
    """Model (oracle/solve_oracle.py) over the graph alone: its objective() is the feasibility check of a state sequence."""
    from oracle import solve_oracle as S
    return S.Model(_G(paths, adj), _NoAnchors, 0)


def states_of_segments(paths, segs):
    return [(paths[h][i], h) for h, a, b in segs for i in range(a, b + 1)]


def path_cover(model, segs, anchors):
    """The dp anchors that lie wholly inside a segment of their own walk, and the number of switches.  Raises ValueError if the
    segments are no feasible s -> e flow (Model.objective's rules), or if two consecutive segments are joined by a walk's own
    edge (that is one segment, not a switch)."""
    for h, a, b in segs:
        if not 0 <= a <= b < len(model.paths[h]):
            raise ValueError(f"segment ({h}, {a}, {b}) leaves its walk")
    _, _, n_sw = model.objective(states_of_segments(model.paths, segs))
    if n_sw != len(segs) - 1:
        raise ValueError(f"{len(segs)} segments joined by {n_sw} switches")
    by_walk = {}
    for h, a, b in segs:
        by_walk.setdefault(h, []).append((a, b))
    covered = [x for x, (h, t0, t1) in enumerate(anchors) if any(a <= t0 and t1 <= b for a, b in by_walk.get(h, ()))]
    return covered, n_sw


def score_segments(model, segs, anchors, weights, cost):
    """The additive value of a path given as segments [(walk, first, last)]: weight-1 anchors inside a segment of their own
    walk, minus cost per switch."""
    covered, n_sw = path_cover(model, segs, anchors)
    w = np.ones(len(anchors), np.int64) if weights is None else np.asarray(weights, np.int64)
    return int(w[covered].sum()) - int(cost) * n_sw


def segments_of_states(model, states):
    """A state sequence [(v, h)] as segments: a new one wherever the step is not along the walk's own edge."""
    segs = []
    for v, h in states:
        i = model.idx[h][v]
        if segs and segs[-1][0] == h and segs[-1][2] + 1 == i:
            segs[-1][2] = i
        else:
            segs.append([h, i, i])
    return [tuple(s) for s in segs]


def enumerate_paths(model, limit=2_000_000):
    """Model.brute_force's recursion: every s -> e state sequence, as segments."""
    n = 0
    stack = [[(p[0], h)] for h, p in enumerate(model.paths)]
    while stack:
        st = stack.pop()
        v, h = st[-1]
        succ = model.successors(v, h)
        if not succ:
            n += 1
            if n > limit:
                raise RuntimeError("enumeration limit exceeded")
            yield segments_of_states(model, st)
            continue
        for v2, h2, _ in succ:
            stack.append(st + [(v2, h2)])


def check_probes(ctx, g, R, rng, key=None):
    """After ctx.solve(): Context.dp_probe with all weights 1 and with one Bernoulli 1/2 vector against the reference -- the value
    at the end of every walk, the value and end walk picked, a feasible path of exactly that value."""
    kept = ctx.kept_anchors()
    anchors = dp_anchors(kept)
    cost = 2 * (R // 2)
    vectors = [None, (rng.random(len(anchors)) < 0.5).astype(np.uint8)]
    ref = dp_ref_many(g.paths, g.adj, g.top_rank, anchors, [np.ones(len(anchors), np.uint8), vectors[1]], cost)
    model = feasibility_model(g.paths, g.adj)
    for wv, row in zip(vectors, ref):
        p = ctx.dp_probe(wv)
        ends, value, end_walk = summary(row)
        assert p["ends"] == ends and (p["value"], p["end_walk"]) == (value, end_walk), (key, p["value"], p["end_walk"], value, end_walk)
        assert score_segments(model, p["segs"], anchors, wv, cost) == value, key


# ---------------------------------------------------------------------------------------------------------- the tie-breaks
def dp_ref_path(paths, adj, top_rank, anchors, weights, cost):
    """The argmax path under the tie-breaks the DP states in words (dp_dev.h, dp.hip, dp_events.hip, dp_pick_end), for one weight
    vector: the end on the lowest walk that has the value; on a walk, ties keep the older run (the lowest entry position);
    into a vertex the recombination with the larger value, then from the lower walk, then from the vertex of lower topological
    rank.  Returns (ends, value, end walk, segments [(walk, first, last)])."""
    w = np.ones(len(anchors), np.int64) if weights is None else np.asarray(weights, np.int64)
    cost, n_vtx = int(cost), len(adj)
    ending = {}
    for a, (h, t0, t1) in enumerate(anchors):
        if w[a]:
            ending.setdefault((h, t1), []).append(t0)
    on = [[] for _ in range(n_vtx)]
    for h, p in enumerate(paths):
        for i, v in enumerate(p):
            on[v].append((h, i))
    pred = [[] for _ in range(n_vtx)]
    for u in range(n_vtx):
        for v in adj[u]:
            pred[v].append(u)
    run = [np.full(len(p), NONE, np.int64) for p in paths]
    G = [[NONE] * len(p) for p in paths]
    start = [[0] * len(p) for p in paths]                  # where the best run at (h, i) entered the walk
    source = [None] * n_vtx                                # the recombination that enters v: (walk, position) it leaves from
    for v in sorted(range(n_vtx), key=lambda x: top_rank[x]):
        best = None
        for u in pred[v]:
            for h2, j in on[u]:
                if j < len(paths[h2]) - 1 and paths[h2][j + 1] != v and G[h2][j] > NONE // 2:
                    key = (G[h2][j], -h2, -top_rank[u])
                    if best is None or key > best[0]:
                        best = (key, h2, j)
        entry = NONE
        if best is not None:
            entry, source[v] = best[0][0] - cost, (best[1], best[2])
        for h, i in on[v]:
            r = run[h]
            r[i] = 0 if i == 0 else entry                  # (every walk of the test graphs begins on a vertex without in-edges)
            for t0 in ending.get((h, i), ()):
                r[: t0 + 1] += 1
            s = int(np.argmax(r[: i + 1]))                 # the first maximum: the older run
            G[h][i], start[h][i] = (int(r[s]), s) if r[s] > NONE // 2 else (NONE, 0)
    ends_row = np.array([G[h][-1] for h in range(len(paths))], np.int64)
    ends, value, end_walk = summary(ends_row)
    segs, h, i = [], end_walk, len(paths[end_walk]) - 1
    while True:
        s = start[h][i]
        segs.append((h, s, i))
        if s == 0:
            break
        h, i = source[paths[h][s]]
    return ends, value, end_walk, segs[::-1]
