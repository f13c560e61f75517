"""Single DP runs against a plain max-plus reference, per kernel instance.

phi_dp_probe runs the solve's own run_dp once, with weights the test gives, on the state the last solve left; tests/dp_ref.py
is the same relaxation in plain numpy (checked against enumeration in test_cpu_dp_ref.py).  For every case and weight vector:
the value at the end of EVERY walk, the value and end walk picked, a feasible path that scores exactly the value -- and the
probe's info must say that the instance the case was written for is the one that ran.  A case that reaches another instance
fails.  The recurrence defines no tie-breaks.  For those the strategies vouch for each other (same path, segment for
segment) -- and for nothing else: they have shared their step rules since dp_dev.h -- and dp_ref.dp_ref_path restates the
rules the kernels' comments state in words (lowest end walk, older run, entry from the lower walk, then the lower source
step), so that a rule changed in the one shared header still shows.
"""
import numpy as np
import pytest

import dp_ref
from graphgen import braided_graph, closed_stretch_case, mosaic_reads, random_graph

pytestmark = pytest.mark.gpu

HALVE, NO_SMALL, GIVE_UP, DENSE = 1, 2, 4, 8       # PHI_DP_RETRY_*
KNOBS = ("PHI_DP_DENSE", "PHI_DP_WAVES", "PHI_DP_NOBLOCKS", "PHI_DP_BLOCK_STEPS", "PHI_DP_ROWS_LARGE", "PHI_DP_STRICT",
         "PHI_DP_CHAIN_SEGMENTS", "PHI_DP_CHAIN_UNITS", "PHI_DP_QLIMIT")
RS = (0, 1, 3, 100)


def _set_graph(ctx, g):
    A = g.arrays()
    ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])


def _graph(seed, n_sites, n_walks, k, w, sparse=False, repeat=False, cut=False, distinct=None):
    """random_graph + mosaic reads; repeat: a repeated segment; cut: walk 1 (or 0) ends inside the graph; distinct: only that
    many different walks, the others copies of them (walks of one class wherever a block is cut)."""
    rng = np.random.default_rng(seed)
    rep = bytes(rng.choice(list(b"ACGT"), size=k + 4).tolist()) if repeat else None
    g = random_graph(rng, n_sites=n_sites, n_walks=distinct or n_walks, seg_len=(8, 40) if sparse else (3, 40), alt_len=(1, 10),
                     p_del=0.25, repeat=rep)
    if distinct:
        g.paths = [list(g.paths[h % distinct]) for h in range(n_walks)]
        g.hap_names = [f"hap{h}.{h}" for h in range(n_walks)]
    if cut:
        h = min(1, n_walks - 1)
        g.paths[h] = g.paths[h][: len(g.paths[h]) - 3]
    reads = mosaic_reads(rng, g, n_reads=300, read_len=k + w + 30, n_seg=3, err=0.01)
    return g, reads


def _weight_vectors(kept, anchors, seed):
    n = len(anchors)
    rng = np.random.default_rng(seed)
    one_walk = anchors[n // 2][0] if n else 0
    return [("ones", None),
            ("zeros", np.zeros(n, np.uint8)),
            ("bernoulli a", (rng.random(n) < 0.5).astype(np.uint8)),
            ("bernoulli b", (rng.random(n) < 0.5).astype(np.uint8)),
            ("one walk", np.array([h == one_walk for h, _, _ in anchors], np.uint8).reshape(n)),
            ("first relaxation", dp_ref.repeat_weights(kept).reshape(n))]


class Solved:
    """A context after set_graph, add_reads and solve(), with what the probes are compared against."""

    def __init__(self, ctx_factory, g, reads, k, w, R, budget=8, threshold=1.0):
        self.g, self.R, self.cost = g, R, 2 * (R // 2)
        self.ctx = ctx_factory(k=k, w=w, threshold=threshold, recombination=R)
        self.ctx.set_solve_budget(budget)
        _set_graph(self.ctx, g)
        self.ctx.add_reads(reads)
        self.res = self.ctx.solve()
        self.kept = self.ctx.kept_anchors()
        self.anchors = dp_ref.dp_anchors(self.kept)
        assert len(self.anchors) == self.ctx.solve_stats()["n_dp_anchors"] > 20
        self.vectors = _weight_vectors(self.kept, self.anchors, 99)
        W = np.stack([np.ones(len(self.anchors), np.uint8) if v is None else v for _, v in self.vectors])
        self.ref = dp_ref.dp_ref_many(g.paths, g.adj, g.top_rank, self.anchors, W, self.cost)     # once, for every probe
        self.model = dp_ref.feasibility_model(g.paths, g.adj)

    def probe(self, x, what):
        """Probe with weight vector x; everything the reference defines is asserted here.  Returns the probe."""
        name, wv = self.vectors[x]
        p = self.ctx.dp_probe(wv)
        info = {f: p[f] for f in ("dp_mode", "n_blocks", "blk_ring", "blk_max_len", "max_classes", "retries", "retries_since_solve")}
        print(f"[dp probe] {what}: {name}: value {p['value']} end walk {p['end_walk']} segments {len(p['segs'])} {info}")
        ends, value, end_walk = dp_ref.summary(self.ref[x])
        bad = [(h, a, b) for h, (a, b) in enumerate(zip(p["ends"], ends)) if a != b]
        assert not bad, (what, name, "ends differ (walk, probe, reference)", bad[:8], len(bad))
        assert (p["value"], p["end_walk"]) == (value, end_walk), (what, name, p["value"], p["end_walk"], value, end_walk)
        assert p["segs"][-1][0] == end_walk
        assert dp_ref.score_segments(self.model, p["segs"], self.anchors, wv, self.cost) == value, (what, name)
        if x in (0, 2):
            # the tie-breaks as the DP states them in words (dp_ref_path): the path itself, segment for segment
            want = dp_ref.dp_ref_path(self.g.paths, self.g.adj, self.g.top_rank, self.anchors, wv, self.cost)[3]
            assert p["segs"] == want, (what, name, "path differs from the stated tie-breaks", p["segs"][:6], want[:6])
        return p

    def probe_all(self, what, expect):
        out = []
        for x in range(len(self.vectors)):
            p = self.probe(x, what)
            expect(p, x)
            out.append(p)
        return out

    def solve_again_is_the_same(self):
        again = self.ctx.solve()
        for key, v in self.res.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, again[key]), key
            else:
                assert v == again[key], (key, v, again[key])


def _env(monkeypatch, env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)


def _expect(mode, ring=None, max_len=None, classes=False, min_blocks=0, since_solve=0):
    def check(p, x):
        assert p["dp_mode"] == mode and p["retries"] == 0 and p["retries_since_solve"] == since_solve, p
        if mode < 2:
            assert (p["n_blocks"], p["blk_ring"], p["blk_max_len"]) == (0, 0, 0), p
        else:
            assert p["n_blocks"] >= max(2, min_blocks) and p["blk_ring"] == ring, p
            lo, hi = max_len
            assert lo <= p["blk_max_len"] <= hi, p
        if classes:
            assert 1 <= p["max_classes"] <= 64, p
    return check


# ------------------------------------------------------------------------------------------- serial kernels
@pytest.mark.parametrize("n_walks,waves", [(1, None), (2, None), (63, None), (64, None), (65, None), (128, None), (129, None), (256, None),
                                           (257, None), (5, "16")])
def test_serial_every_vertex(ctx_factory, monkeypatch, n_walks, waves):
    """phi_dp_kernel<1|2|4|8> by the number of walks (257: eight waves), <16> forced onto 5 walks."""
    _env(monkeypatch, {"PHI_DP_DENSE": "1", **({"PHI_DP_WAVES": waves} if waves else {})})
    g, reads = _graph(6000 + n_walks, 40 if n_walks > 64 else 70, n_walks, 7, 3, repeat=n_walks in (2, 129), cut=n_walks in (5, 64, 257))
    R = {1: 3, 2: 0, 63: 100, 64: 1, 65: 3, 128: 100, 129: 0, 256: 3, 257: 100, 5: 3}[n_walks]
    s = Solved(ctx_factory, g, reads, 7, 3, R, threshold=1.5 if n_walks == 1 else 1.0)     # (one walk: every minimiser is in all walks)
    s.probe_all(f"every vertex, {n_walks} walks", _expect(0))
    s.solve_again_is_the_same()


@pytest.mark.parametrize("n_walks", [2, 64, 65, 128, 129, 256])
def test_serial_events(ctx_factory, monkeypatch, n_walks):
    """The whole event chain: phi_dp_events_pc_kernel up to 64 walks, phi_dp_events_kernel<2> up to 128, <4> up to 256."""
    _env(monkeypatch, {"PHI_DP_NOBLOCKS": "1"})
    g, reads = _graph(6100 + n_walks, 40 if n_walks > 64 else 70, n_walks, 7, 3, repeat=n_walks in (64, 128), cut=n_walks in (2, 65, 256))
    s = Solved(ctx_factory, g, reads, 7, 3, {2: 3, 64: 100, 65: 0, 128: 3, 129: 1, 256: 100}[n_walks])
    s.probe_all(f"events, {n_walks} walks", _expect(1))
    s.solve_again_is_the_same()


# ------------------------------------------------------------------------------------------- blocks on walk lanes
@pytest.mark.parametrize("n_walks", [3, 64])
@pytest.mark.parametrize("steps,rows_large", [("1", False), ("3", False), ("16", False), ("16", True), (None, False)])
def test_blocks_on_walk_lanes_ring_256(ctx_factory, monkeypatch, n_walks, steps, rows_large):
    """Ring 256 (sparse minimisers, w = 20: no lane of a block task holds more than 8 live runs).  Blocks of at most 64 steps
    take the small DP_ROW instance (ring 64, period 2), PHI_DP_ROWS_LARGE=1 or longer blocks the ring-256 one; DP_PATH<256>
    behind both.  Default steps: a block of more than 64 steps."""
    _env(monkeypatch, {**({"PHI_DP_BLOCK_STEPS": steps} if steps else {}), **({"PHI_DP_ROWS_LARGE": "1"} if rows_large else {})})
    k = 7 if n_walks == 3 else 5
    g, reads = _graph(6200 + n_walks, 110, n_walks, k, 20, cut=True)
    s = Solved(ctx_factory, g, reads, k, 20, RS[(n_walks + len(steps or "")) % 4])
    want_len = (65, 256) if steps is None else (1, 64)
    s.probe_all(f"walk lanes, {n_walks} walks, steps {steps}, rows large {rows_large}", _expect(2, 256, want_len, min_blocks=2 if steps is None else 8))
    s.solve_again_is_the_same()


@pytest.mark.parametrize("ring,n_sites", [(1024, 130), (2048, 450)])
def test_blocks_on_walk_lanes_long_rings(ctx_factory, monkeypatch, ring, n_sites):
    """A stretch that no cut may split of 257..1024 compact steps (130 sites), of more than 1 024 (450 sites): the DP_ROW and
    DP_PATH instances on rings of 1 024 and of 2 048 tops."""
    _env(monkeypatch, {})
    g, reads, k = closed_stretch_case(7800, n_sites, 6, 11, 0.9)
    s = Solved(ctx_factory, g, reads, k, 1, 3)
    s.probe_all(f"walk lanes, ring {ring}", _expect(2, ring, (ring // 4 + 1, ring)))
    s.solve_again_is_the_same()


# ------------------------------------------------------------------------------------------- blocks on class lanes
def _sparse(n_walks, **kw):
    return _graph(6300 + n_walks, 60, n_walks, 5, 20, sparse=True, **kw)


# (seed, sites, k, w) at which every weight vector of the case keeps every block of 2 steps within 64 classes
CLASS_LANE_CASES = {65: (0, 60, 4, 25), 128: (0, 60, 4, 25), 129: (1, 60, 4, 25), 256: (2, 60, 4, 25)}


def _class_lane_graph(n_walks):
    seed, n_sites, k, w = CLASS_LANE_CASES[n_walks]
    g, reads = _graph(6300 + n_walks + 1000 * seed, n_sites, n_walks, k, w, sparse=True, repeat=n_walks in (65, 129), cut=n_walks in (128, 129))
    return g, reads, k, w


@pytest.mark.parametrize("n_walks", [65, 128, 129, 256])
@pytest.mark.parametrize("chain", [None, ("3", None), ("100000", None), ("3", "1"), ("5", "2"), ("3", "4")])
def test_blocks_on_class_lanes_of_two_steps(ctx_factory, monkeypatch, n_walks, chain):
    """Sparse graphs (k = 4, w = 25), blocks of 2 steps under PHI_DP_STRICT: rows on class lanes, the chain on the device whole
    and cut into segments (3, 5, one per block; 1, 2, 3 and 4 unit vectors a workgroup), phi_launch_dp_block_paths_wide<2|4>."""
    env = {"PHI_DP_BLOCK_STEPS": "2", "PHI_DP_STRICT": "1"}
    if chain:
        env["PHI_DP_CHAIN_SEGMENTS"] = chain[0]
        if chain[1]:
            env["PHI_DP_CHAIN_UNITS"] = chain[1]
    _env(monkeypatch, env)
    g, reads, k, w = _class_lane_graph(n_walks)
    s = Solved(ctx_factory, g, reads, k, w, RS[(n_walks + len(chain or ())) % 4])
    s.probe_all(f"class lanes, {n_walks} walks, chain {chain}", _expect(3, 256, (1, 16), classes=True, min_blocks=6))
    s.solve_again_is_the_same()


def test_blocks_on_class_lanes_default_steps(ctx_factory, monkeypatch):
    """The default class target of 16 steps a block: 65 walks whose blocks stay within 64 classes at that length."""
    _env(monkeypatch, {"PHI_DP_STRICT": "1"})
    g, reads = _graph(6300 + 65 + 2000, 40, 65, 4, 25, sparse=True, repeat=True)
    s = Solved(ctx_factory, g, reads, 4, 25, 3)
    s.probe_all("class lanes, 65 walks, default steps", _expect(3, 256, (16, 64), classes=True))
    s.solve_again_is_the_same()


def test_blocks_on_class_lanes_ring_512(ctx_factory, monkeypatch):
    """Class-lane rows at ring 512.  256 walks of eight kinds, dense minimisers: the blocks placed at ring 256 overflow the
    8-deep queues of their tasks in the solve's first run, which places them again without that ring: the all-ones and the
    all-zero probe run there.  The first Bernoulli vector splits a block into more than 64 classes at any length: that probe
    halves the class target down to the whole chain, where the later ones stay."""
    _env(monkeypatch, {})
    g, reads = _graph(6400 + 256, 60, 256, 7, 3, distinct=8, repeat=True)
    s = Solved(ctx_factory, g, reads, 7, 3, 3)

    def expect(p, x):
        if x < 2:
            assert p["dp_mode"] == 3 and p["blk_ring"] == 512 and p["n_blocks"] >= 2 and 1 <= p["max_classes"] <= 64, p
            assert p["retries"] == 0 and p["retries_since_solve"] == NO_SMALL, p
        else:                                              # (the Bernoulli weights split a block into more than 64 classes, at any length)
            assert p["dp_mode"] == 1 and p["retries"] == (HALVE | GIVE_UP if x == 2 else 0) and p["retries_since_solve"] == NO_SMALL | HALVE | GIVE_UP, p
    s.probe_all("class lanes, ring 512", expect)


# ------------------------------------------------------------------------------------------- retries
def test_retry_from_the_event_chain_to_every_vertex(ctx_factory, monkeypatch):
    """DP_DENSE: 150 walks on the whole event chain; PHI_DP_QLIMIT=1 (read by every run) overflows the four-wave kernel's queues in
    the first probe, which finishes on the every-vertex kernel -- as do the probes after it, with nothing left to retry."""
    _env(monkeypatch, {"PHI_DP_NOBLOCKS": "1"})
    g, reads = _graph(6500, 60, 150, 7, 3, cut=True)
    s = Solved(ctx_factory, g, reads, 7, 3, 3)
    assert s.ctx.solve_stats()["dp_mode"] == 1
    monkeypatch.setenv("PHI_DP_QLIMIT", "1")

    def expect(p, x):
        assert p["dp_mode"] == 0 and p["retries"] == (DENSE if x == 0 else 0) and p["retries_since_solve"] == DENSE, p
    s.probe_all("retry: dense", expect)


def test_retries_from_class_lane_blocks_down_to_every_vertex(ctx_factory, monkeypatch):
    """DP_NO_SMALL_BLOCKS and DP_GIVE_UP_BLOCKS: 150 walks in class-lane blocks at ring 256; under PHI_DP_QLIMIT=1 the second pass
    (phi_dp_events_kernel<4, DP_PATH>) overflows its queues: blocks again without ring 256, the same again, the whole chain,
    which overflows as well (the limit holds for every run of that kernel), and every vertex: three retries in the first probe."""
    _env(monkeypatch, {"PHI_DP_BLOCK_STEPS": "2"})
    g, reads = _sparse(150, repeat=True)
    s = Solved(ctx_factory, g, reads, 5, 20, 3)
    st = s.ctx.solve_stats()
    assert st["dp_mode"] == 3, st
    monkeypatch.setenv("PHI_DP_QLIMIT", "1")

    def expect(p, x):
        assert p["dp_mode"] == 0 and p["retries"] == (NO_SMALL | GIVE_UP | DENSE if x == 0 else 0), p
        assert p["retries_since_solve"] == NO_SMALL | GIVE_UP | DENSE, p
    s.probe_all("retry: no small blocks, give up blocks, dense", expect)


def test_retry_without_small_blocks_on_walk_lanes(ctx_factory, monkeypatch):
    """DP_NO_SMALL_BLOCKS on its own and of its own accord: 3 walks, dense minimisers (w = 3), R = 3.  The solve's relaxation
    (repeats at weight 0) fits the 8-deep queues of the 256-step block tasks; with every weight 1 a lane holds more live runs,
    and the probe places the blocks again at ring 1 024."""
    _env(monkeypatch, {})
    g, reads = _graph(6203, 110, 3, 7, 3, cut=True)
    s = Solved(ctx_factory, g, reads, 7, 3, 3)

    def expect(p, x):
        assert p["dp_mode"] == 2 and p["blk_ring"] == 1024 and p["retries"] == (NO_SMALL if x == 0 else 0) and p["retries_since_solve"] == NO_SMALL, p
    s.probe_all("retry: no small blocks", expect)


def test_retry_gives_up_blocks_alone(ctx_factory, monkeypatch):
    """DP_GIVE_UP_BLOCKS on its own: 128 walks whose blocks of 2 steps (fixed by PHI_DP_BLOCK_STEPS: no halving) hold more than
    64 classes.  The solve's first run meets that, so the probes find the whole chain and nothing to retry; the probe reports
    what the runs since the solve began took."""
    _env(monkeypatch, {"PHI_DP_BLOCK_STEPS": "2"})
    g, reads = _graph(6300 + 128 + 2000, 40, 128, 5, 20, sparse=True, cut=True)
    s = Solved(ctx_factory, g, reads, 5, 20, 3)

    def expect(p, x):
        assert p["dp_mode"] == 1 and p["retries"] == 0 and p["retries_since_solve"] == GIVE_UP, p
    s.probe_all("retry: give up blocks", expect)


def test_retry_halves_the_class_target(ctx_factory, monkeypatch):
    """DP_HALVE_CLASS_TARGET: 256 walks whose blocks exceed 64 classes at the default target of 16 steps.  A block's classes
    depend on the weights of the run.  The solve's own runs halve once (read from retries_since_solve) and leave blocks that fit
    all-ones and all-zero weights; the first Bernoulli vector splits a block into more than 64 classes again: that probe halves
    down to the whole chain, where the later probes stay."""
    _env(monkeypatch, {})
    g, reads = _graph(6300 + 256, 60, 256, 5, 20, sparse=True)
    s = Solved(ctx_factory, g, reads, 5, 20, 3)

    def expect(p, x):
        if x < 2:
            assert p["dp_mode"] == 3 and p["blk_ring"] == 256 and 1 <= p["max_classes"] <= 64, p
            assert p["retries"] == 0 and p["retries_since_solve"] == HALVE, p
        else:
            assert p["dp_mode"] == 1 and p["retries"] == (HALVE | GIVE_UP if x == 2 else 0) and p["retries_since_solve"] == HALVE | GIVE_UP, p
    s.probe_all("retry: halve the class target", expect)


# ------------------------------------------------------------------------------------------- the tie-break contract
@pytest.mark.parametrize("n_walks,w", [(9, 3), (9, 20), (100, 20)])
def test_every_strategy_returns_the_same_path(ctx_factory, monkeypatch, n_walks, w):
    """dp_dev.h: the same transitions, tie-breaks and outputs in every kernel.  One graph, R = 1 (no switch costs: ties
    everywhere), all-ones and one Bernoulli weight vector: the path is the same, segment for segment, whatever strategy ran
    (9 walks, w = 3: the blocks end up at ring 1 024; w = 20: at ring 256; 100 walks: class lanes)."""
    if n_walks <= 64:
        k = 7
        g, reads = _graph(6700, 110, n_walks, k, w, repeat=True, cut=True)
        envs = {"every vertex": ({"PHI_DP_DENSE": "1"}, 0), "events": ({"PHI_DP_NOBLOCKS": "1"}, 1),
                "blocks of 1": ({"PHI_DP_BLOCK_STEPS": "1"}, 2), "blocks of 16": ({"PHI_DP_BLOCK_STEPS": "16"}, 2),
                "blocks of 16, rows large": ({"PHI_DP_BLOCK_STEPS": "16", "PHI_DP_ROWS_LARGE": "1"}, 2), "default blocks": ({}, 2)}
    else:
        k = 5
        g, reads = _sparse(n_walks, repeat=True, cut=True)
        envs = {"every vertex": ({"PHI_DP_DENSE": "1"}, 0), "events": ({"PHI_DP_NOBLOCKS": "1"}, 1),
                "class lanes": ({"PHI_DP_BLOCK_STEPS": "2", "PHI_DP_STRICT": "1"}, 3),
                "class lanes, 3 segments": ({"PHI_DP_BLOCK_STEPS": "2", "PHI_DP_STRICT": "1", "PHI_DP_CHAIN_SEGMENTS": "3"}, 3)}
    got = {}
    for name, (env, mode) in envs.items():
        _env(monkeypatch, env)
        s = Solved(ctx_factory, g, reads, k, w, 1)
        for x in (0, 2):
            p = s.probe(x, f"same path, {n_walks} walks, w {w}, {name}")
            assert p["dp_mode"] == mode, (name, p)
            got[(name, x)] = p["segs"]
        s.ctx.close()
    first = next(iter(envs))
    for (name, x), segs in got.items():
        assert segs == got[(first, x)], (name, x, segs[:6], got[(first, x)][:6])
    assert max(len(got[(first, 0)]), len(got[(first, 2)])) > 3             # (the paths do switch)


@pytest.mark.parametrize("n_walks", [9, 70, 150])
def test_tie_breaks_where_two_in_edges_compete(ctx_factory, monkeypatch, n_walks):
    """Braided graphs: every vertex has two in-edges with walks that leave the other way, so the entry rule's second and third
    key (the lower walk, the lower source step) decide; R = 1 makes every switch free.  Every serial kernel and the blocks
    return the path of the stated tie-breaks (asserted in Solved.probe), and the reference's values."""
    rng = np.random.default_rng(6900 + n_walks)
    g = braided_graph(rng, n_sites=50, n_walks=n_walks)
    g.paths[1] = g.paths[1][:-2]                           # ends inside the graph
    reads = mosaic_reads(rng, g, n_reads=300, read_len=40, n_seg=3, err=0.01)
    envs = {"every vertex": ({"PHI_DP_DENSE": "1"}, 0), "events": ({"PHI_DP_NOBLOCKS": "1"}, 1), "blocks": ({"PHI_DP_BLOCK_STEPS": "3"}, None)}
    n_switches = 0
    for name, (env, mode) in envs.items():
        _env(monkeypatch, env)
        for R in (1, 3):
            s = Solved(ctx_factory, g, reads, 7, 8, R)
            for x in (0, 2):
                p = s.probe(x, f"two in-edges, {n_walks} walks, R {R}, {name}")
                assert mode is None or p["dp_mode"] == mode, (name, p)
                n_switches += len(p["segs"]) - 1
            s.ctx.close()
    assert n_switches >= 12, n_switches


def test_probe_refuses_what_it_cannot_run(ctx_factory, monkeypatch):
    import phi_amd
    _env(monkeypatch, {})
    g, reads = _graph(6800, 30, 4, 7, 3)
    ctx = ctx_factory(k=7, w=3, threshold=1.0, recombination=3)
    _set_graph(ctx, g)
    ctx.add_reads(reads)
    with pytest.raises(phi_amd.PhiError) as e:
        ctx.dp_probe()
    assert e.value.status == phi_amd.PHI_ERR_STATE
    ctx.solve()
    n = ctx.solve_stats()["n_dp_anchors"]
    for bad in (np.ones(n + 1, np.uint8), np.ones(n - 1, np.uint8), np.full(n, 2, np.uint8)):
        with pytest.raises(phi_amd.PhiError) as e:
            ctx.dp_probe(bad)
        assert e.value.status == phi_amd.PHI_ERR_INVALID
    assert ctx.dp_probe()["value"] == ctx.dp_probe(np.ones(n, np.uint8))["value"]
    scout = ctx_factory(k=7, w=3, threshold=1.0, recombination=3)
    A = g.arrays()
    scout.scout_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])
    with pytest.raises(phi_amd.PhiError) as e:
        scout.dp_probe()
    assert e.value.status == phi_amd.PHI_ERR_STATE and "scout" in str(e.value)
