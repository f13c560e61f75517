"""CPU test of the DP reference itself (tests/dp_ref.py): on tiny graphs the recurrence equals exhaustive enumeration of every
s -> e state sequence, scored additively, per end walk; and where every minimiser has one dp anchor, its all-ones value is the
exact objective's maximum (Model.brute_force).  The GPU probe tests (test_gpu_dp_probe.py) rest on this."""
import types

import numpy as np
import pytest

import dp_ref
from graphgen import mosaic_reads, random_graph

N_GRAPHS = 240
RS = (0, 1, 3, 100)
SEED0 = 5100                   # (the seeds were picked here so that no graph has more than 150 000 state sequences)


def _tiny_case(oracle, seed):
    rng = np.random.default_rng(SEED0 + seed)
    n_walks, n_sites = int(rng.integers(2, 6)), int(rng.integers(3, 8))
    k, w = int(rng.integers(3, 6)), int(rng.integers(1, 4))
    g = random_graph(rng, n_sites=n_sites, n_walks=n_walks, seg_len=(1, 6), alt_len=(1, 4), p_del=0.25)
    was_cut = False
    if seed % 3 == 0:
        h = int(rng.integers(0, n_walks))
        cut = int(rng.integers(1, 4))
        if len(g.paths[h]) > cut + 1:
            g.paths[h] = g.paths[h][: len(g.paths[h]) - cut]        # ends inside the graph
            was_cut = True
    reads = mosaic_reads(rng, g, n_reads=30, read_len=k + w + 8, n_seg=2)
    st = oracle.run_stage12(g, reads, k, w, 1.0)
    return rng, g, st, was_cut


def _anchors(st):
    return [(int(h), int(a), int(b)) for h, a, b in zip(st.a_h.tolist(), st.a_t0.tolist(), st.a_t1.tolist()) if b > a]


def test_dp_ref_equals_enumeration_per_end_walk(oracle):
    """240 seeded graphs of 2-5 walks and 3-7 sites, a third with a walk cut short inside the graph; R in {0, 1, 3, 100};
    weights all 1, all 0 and Bernoulli 1/2: for every end walk the reference's value is the best additive score over all state
    sequences that end there (the enumeration is Model.brute_force's recursion, the score dp_ref's scorer)."""
    n_seq_total, n_with_anchors, n_cut, n_switching = 0, 0, 0, 0
    for seed in range(N_GRAPHS):
        rng, g, st, was_cut = _tiny_case(oracle, seed)
        anchors = _anchors(st)
        model = dp_ref.feasibility_model(g.paths, g.adj)
        W = np.stack([np.ones(len(anchors), np.int64), np.zeros(len(anchors), np.int64),
                      (rng.random(len(anchors)) < 0.5).astype(np.int64)])
        covers = []                                                 # per state sequence: end walk, switches, anchors covered
        for segs in dp_ref.enumerate_paths(model, limit=150_000):
            covered, n_sw = dp_ref.path_cover(model, segs, anchors)
            covers.append((segs[-1][0], n_sw, W[:, covered].sum(axis=1)))
        n_seq_total += len(covers)
        n_with_anchors += len(anchors) > 0
        n_cut += was_cut
        end_h = np.array([c[0] for c in covers])
        n_sw = np.array([c[1] for c in covers], np.int64)
        add = np.stack([c[2] for c in covers])                      # (sequences, weight vectors)
        for R in RS:
            cost = 2 * (R // 2)
            got = dp_ref.dp_ref_many(g.paths, g.adj, g.top_rank, anchors, W, cost)
            score = add - cost * n_sw[:, None]
            for h in range(g.n_walks):
                sel = end_h == h
                assert sel.any(), (seed, h)                         # (every walk can be followed from its start to its end)
                want = score[sel].max(axis=0)
                assert got[:, h].tolist() == want.tolist(), (seed, R, h, got[:, h], want)
            for x in range(3):
                ends, value, end_walk = dp_ref.dp_ref(g.paths, g.adj, g.top_rank, anchors, W[x], cost)
                assert ends == got[x].tolist() and value == score[:, x].max()
                assert end_walk == min(h for h in range(g.n_walks) if ends[h] == value)
            if R == 3:
                best = score[:, 0].argmax()
                n_switching += n_sw[best] > 0
    assert n_with_anchors >= 200 and n_cut >= 40 and n_switching >= 20, (n_with_anchors, n_cut, n_switching)
    assert n_seq_total > 100_000, n_seq_total


def test_scorer_refuses_what_is_no_path(oracle):
    rng, g, st, was_cut = _tiny_case(oracle, 1)
    anchors = _anchors(st)
    model = dp_ref.feasibility_model(g.paths, g.adj)
    whole = [(0, 0, len(g.paths[0]) - 1)]
    assert dp_ref.score_segments(model, whole, anchors, None, 7) == sum(h == 0 for h, _, _ in anchors)
    with pytest.raises(ValueError):
        dp_ref.score_segments(model, [(0, 1, len(g.paths[0]) - 1)], anchors, None, 0)            # starts inside the walk
    with pytest.raises(ValueError):
        dp_ref.score_segments(model, [(0, 0, len(g.paths[0]) - 2)], anchors, None, 0)            # ends inside the walk
    with pytest.raises(ValueError):
        dp_ref.score_segments(model, [(0, 0, 1), (0, 2, len(g.paths[0]) - 1)], anchors, None, 0)  # a walk's own edge is no switch
    with pytest.raises(ValueError):
        dp_ref.score_segments(model, [(0, 0, len(g.paths[0]))], anchors, None, 0)                 # leaves the walk


def test_one_anchor_per_minimiser_makes_the_relaxation_exact(oracle):
    """With one dp anchor per minimiser nothing can be counted twice: the additive all-ones value is the exact objective's
    maximum over all paths (Model.brute_force, which knows nothing of the DP)."""
    from oracle import solve_oracle as S
    n = 0
    for seed in range(60):
        rng, g, st, was_cut = _tiny_case(oracle, seed)
        first = {}
        for x, (r, a, b) in enumerate(zip(st.a_r.tolist(), st.a_t0.tolist(), st.a_t1.tolist())):
            if b > a:
                first.setdefault(r, x)
        keep = sorted(first.values())
        one = types.SimpleNamespace(a_r=st.a_r[keep], a_h=st.a_h[keep], a_t0=st.a_t0[keep], a_t1=st.a_t1[keep])
        R = RS[seed % 4]
        m = S.Model(g, one, R)
        assert all(len(v) == 1 for v in m.anchors.values())
        best, _ = m.brute_force(limit=150_000)
        _, value, _ = dp_ref.dp_ref(g.paths, g.adj, g.top_rank, _anchors(one), np.ones(len(keep), np.int64), 2 * (R // 2))
        assert value == best, (seed, R, value, best)
        n += len(keep) > 0
    assert n >= 50, n


def test_the_stated_tie_breaks_give_an_argmax_path(oracle):
    """dp_ref_path (the end on the lowest walk, the older run, the recombination from the lower walk and then the lower vertex)
    returns the recurrence's values and a feasible path that scores exactly the value -- on bubble chains and on braided
    graphs, where a vertex can be entered over two in-edges."""
    from graphgen import braided_graph
    n_switching = 0
    for seed in range(80):
        rng = np.random.default_rng(SEED0 + 1000 + seed)
        if seed % 2:
            g = braided_graph(rng, n_sites=int(rng.integers(4, 14)), n_walks=int(rng.integers(2, 7)))
        else:
            g = random_graph(rng, n_sites=int(rng.integers(4, 10)), n_walks=int(rng.integers(2, 7)), seg_len=(2, 8), alt_len=(1, 5))
        reads = mosaic_reads(rng, g, n_reads=40, read_len=20, n_seg=3)
        anchors = _anchors(oracle.run_stage12(g, reads, 5, 2, 1.0))
        model = dp_ref.feasibility_model(g.paths, g.adj)
        for R in RS:
            cost = 2 * (R // 2)
            wv = (rng.random(len(anchors)) < 0.6).astype(np.int64)
            ends, value, end_walk, segs = dp_ref.dp_ref_path(g.paths, g.adj, g.top_rank, anchors, wv, cost)
            assert (ends, value, end_walk) == dp_ref.dp_ref(g.paths, g.adj, g.top_rank, anchors, wv, cost), (seed, R)
            assert segs[-1][0] == end_walk and dp_ref.score_segments(model, segs, anchors, wv, cost) == value, (seed, R)
            n_switching += len(segs) > 1
    assert n_switching >= 80, n_switching
