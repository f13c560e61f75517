"""The panel chosen from the reads (phi_scout_graph, phi_scout_scores in phi_amd/csrc/panel_score.hip, phi_scout_choose,
PHI_PANEL_KEEP_READS, phi_reads_collect_score, phi_vcf_walks_wide; phi_amd.panel.auto_panel): graphs of more walks than the
DP takes.

1. the score matrix against its definition restated in numpy: the oracle's sketch of every walk's sequence, the oracle's read
   spectrum, the vertex under a minimiser's first base from the walk's vertex lengths;
2. the choice on the device's matrix against phi_amd.panel.choose_panel;
3. auto_panel on one context against set_graph(keep=chosen) + add_reads on another: the route equals its parts;
4. a planted case from a VCF of 1 201 haplotypes: the two haplotypes the reads are a mosaic of lead every block, are chosen in
   round 0, and the inferred sequence is the mosaic;
5. states, refusals and limits.
Every comparison is exact."""
import functools
import os

import numpy as np
import pytest

from graphgen import mosaic_reads, random_graph, walk_sequence
from test_gpu_chop import _dirty, _same_run, _write_gfa
from test_gpu_vcf import _python_graph, _write_case

pytestmark = pytest.mark.gpu

KW = [(5, 2), (15, 5)]


# ------------------------------------------------------------------ the graphs and the definition

@functools.lru_cache(maxsize=None)
def _graph(name):
    """many: 1 100 walks of about 25 entries (a wave's row of 64 entries meets several walks); short: the same with segments
    of 1-4 bases (k-mers start vertices behind their window's entry: classes get flagged); long: 3 walks of at least 20 000
    entries (a walk longer than a wave's slice); single: walks of one entry; dirty: lower case and N in the segments."""
    rng = np.random.default_rng({"many": 1, "short": 2, "long": 3, "single": 4, "dirty": 5}[name])
    if name == "many":
        g = random_graph(rng, n_sites=12, n_walks=1100, seg_len=(1, 90), alt_len=(1, 6))
    elif name == "short":
        g = random_graph(rng, n_sites=12, n_walks=1100, seg_len=(1, 4), alt_len=(1, 6))
    elif name == "long":
        g = random_graph(rng, n_sites=12000, n_walks=3, seg_len=(1, 4), alt_len=(1, 3), p_del=0.1)
        assert min(len(p) for p in g.paths) >= 20000
    elif name == "single":
        g = random_graph(rng, n_sites=0, n_walks=2, seg_len=(40, 40))
        assert all(len(p) == 1 for p in g.paths)
    else:
        g = random_graph(rng, n_sites=30, n_walks=1030, seg_len=(1, 60), alt_len=(1, 9))
        _dirty(rng, g)
    return g


@functools.lru_cache(maxsize=None)
def _reads(name, which):
    g = _graph(name)
    rng = np.random.default_rng(1000 + 10 * which + len(name))
    if name == "long":
        return mosaic_reads(rng, g, n_reads=300, read_len=100, n_seg=2, err=0.01)
    return mosaic_reads(rng, g, n_reads=40, read_len=60 if name != "single" else 30, n_seg=2, err=0.01)


def _arrays_of(g):
    return g.arrays() if hasattr(g, "arrays") else dict(seq_concat=g.seq_concat.tobytes(), seq_off=g.seq_off, adj_off=g.adj_off, adj=g.adj, walk_off=g.walk_off,
                                                       walk_vtx=g.walk_vtx, top_rank=g.top_order_map)


_occ_cache = {}


def _occurrences(O, key, A, k, w):
    """Per walk: (hashes, rank of the vertex under each minimiser's first base), from the oracle's sketch of the walk's sequence."""
    if (key, k, w) not in _occ_cache:
        seq = np.frombuffer(A["seq_concat"], np.uint8)
        so, wo, wv, rank = A["seq_off"], A["walk_off"], A["walk_vtx"], np.asarray(A["top_rank"], np.int64)
        vlen = np.diff(so)
        out = []
        for h in range(len(wo) - 1):
            path = wv[wo[h]:wo[h + 1]]
            s = b"".join(seq[so[v]:so[v + 1]].tobytes() for v in path.tolist())
            starts = np.concatenate([[0], np.cumsum(vlen[path])])
            hs, ps = O.sketch(s, k, w)
            out.append((hs, rank[path[np.searchsorted(starts, ps, side="right") - 1]] if len(ps) else np.zeros(0, np.int64)))
        _occ_cache[(key, k, w)] = out
    return _occ_cache[(key, k, w)]


def _expected(O, key, A, reads, k, w, n_blocks):
    """S[b][h] by the definition."""
    n_vtx, n_walks = len(A["seq_off"]) - 1, len(A["walk_off"]) - 1
    off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    spectrum = O.read_spectrum([(b"".join(reads), off)], k, w)[0] if len(reads) else np.zeros(0, np.uint64)
    S = np.zeros((n_blocks, n_walks), np.int64)
    for h, (hs, ranks) in enumerate(_occurrences(O, key, A, k, w)):
        hit = np.isin(hs, spectrum)
        np.add.at(S[:, h], ranks[hit] * n_blocks // n_vtx, 1)
    return S


def _scout(ctx, A, walk_vtx="host"):
    ctx.scout_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"] if walk_vtx == "host" else None, A["top_rank"])


def _check_scores(O, ctx, name, A, k, w, which):
    reads = _reads(name, which)
    ctx.add_reads(reads)
    n_vtx = len(A["seq_off"]) - 1
    out = {}
    for nb in (1, 7, n_vtx):
        S, info = ctx.scout_scores(nb)
        want = _expected(O, name, A, reads, k, w, nb)
        assert S.shape == want.shape and np.array_equal(S, want), (name, k, w, nb, int(np.abs(S - want).sum()))
        assert (info["n_blocks"], info["n_walks"], info["n_nonzero"]) == (nb, S.shape[1], int(np.count_nonzero(want)))
        assert info["entry_gpu_ms"] > 0 and info["record_gpu_ms"] > 0 and info["class_gpu_ms"] > 0
        if nb == 1:
            assert info["n_classes_flagged"] == 0
        out[nb] = (S, info)
    # the column sums are the hit occurrences of every walk, whatever the blocks
    per_walk = out[1][0][0]
    assert np.array_equal(out[7][0].sum(0), per_walk) and np.array_equal(out[n_vtx][0].sum(0), per_walk)
    return out


# ------------------------------------------------------------------ 1. scores against the definition

@pytest.mark.parametrize("k,w", KW)
@pytest.mark.parametrize("name", ["many", "short", "long", "single"])
def test_scores_equal_the_definition(oracle, ctx_factory, name, k, w):
    g = _graph(name)
    A = g.arrays()
    ctx = ctx_factory(k=k, w=w)
    try:
        _scout(ctx, A)
        # the occurrences are the list walk_minimizers returns (a few walks: the first, the last, one in between)
        occ = _occurrences(oracle, name, A, k, w)
        for h in sorted({0, g.n_walks // 2, g.n_walks - 1}):
            hs, ps = ctx.walk_minimizers(h)
            assert np.array_equal(hs, occ[h][0]) and np.array_equal(hs, oracle.sketch(walk_sequence(g, h), k, w)[0]), h
        # without reads: all zero
        S, info = ctx.scout_scores(7)
        assert S.shape == (7, g.n_walks) and not S.any() and info["n_nonzero"] == 0
        first = _check_scores(oracle, ctx, name, A, k, w, 0)
        assert first[1][0].any()                                # the reads hit something
        if name == "short":
            assert first[len(A["seq_off"]) - 1][1]["n_classes_flagged"] > 0
        if name == "many":
            assert np.diff(A["walk_off"]).max() < 64            # a row of 64 entries meets several walks
        # other reads after reset_reads: that set's matrix (the call zeroes its buffer)
        ctx.reset_reads()
        second = _check_scores(oracle, ctx, name, A, k, w, 1)
        # (not vacuous at k = 15: the two sets hit different minimisers; at k = 5 every 5-mer of a long walk is in both)
        assert k == 5 or name == "single" or not np.array_equal(first[7][0], second[7][0])
    finally:
        ctx.close()


def test_scores_on_a_used_context_with_dirty_segments(oracle, ctx_factory):
    """A context that has set, scored and solved another graph before, its device buffers recycled; lower case and N in the
    segments; the scout set twice from the entries it retained."""
    k, w = 9, 4
    ctx = ctx_factory(k=k, w=w)
    try:
        small = _graph("single").arrays()
        ctx.set_graph(small["seq_concat"], small["seq_off"], small["adj_off"], small["adj"], small["walk_off"], small["walk_vtx"], small["top_rank"])
        ctx.add_reads(_reads("single", 0))
        ctx.solve()
        _scout(ctx, _graph("short").arrays())
        ctx.add_reads(_reads("short", 0))
        ctx.scout_scores(7)
        A = _graph("dirty").arrays()
        _scout(ctx, A)
        _check_scores(oracle, ctx, "dirty", A, k, w, 0)
        _scout(ctx, A, walk_vtx=None)                           # again, from the entries the scout holds
        assert np.array_equal(ctx.walk_entries(), A["walk_vtx"])
        _check_scores(oracle, ctx, "dirty", A, k, w, 1)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. the choice

@pytest.mark.parametrize("name", ["many", "short", "long"])
def test_choice_equals_the_restatement(ctx_factory, name):
    from phi_amd.panel import choose_panel
    import phi_amd
    g = _graph(name)
    A = g.arrays()
    k, w = KW[0]
    ctx = ctx_factory(k=k, w=w)
    try:
        _scout(ctx, A)
        with pytest.raises(phi_amd.PhiError) as e:              # no matrix yet
            ctx.scout_choose(2)
        assert e.value.status == phi_amd.PHI_ERR_STATE
        ctx.add_reads(_reads(name, 0))
        always = np.zeros(g.n_walks, np.uint8)
        always[[0, g.n_walks - 1]] = 1
        for nb in (1, 7, g.n_vtx):
            S, _ = ctx.scout_scores(nb)
            for n_want, alw in ((2, None), (min(64, g.n_walks), None), (min(1022, g.n_walks), always), (2, always)):
                keep, round_of = ctx.scout_choose(n_want, alw)
                wk, wr = choose_panel(S, n_want, alw)
                assert np.array_equal(keep, wk) and np.array_equal(round_of, wr), (name, nb, n_want)
                assert int(keep.sum()) == n_want
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. the route equals its parts

K3, W3, T3, R3 = 9, 4, 1.0, 3


def _fasta_pieces(reads):
    text = b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads))
    return [text[i:i + 997] for i in range(0, len(text), 997)]


@pytest.mark.parametrize("variant", ["host", "chop30", "device_walks", "text_reads"])
def test_route_equals_its_parts(ctx_factory, tmp_path, variant):
    from phi_amd import ilp_index as H
    from phi_amd.panel import auto_panel, choose_panel
    g = _graph("many")
    A = g.arrays()
    reads = _reads("many", 0)
    chop = 30 if variant == "chop30" else None
    a = ctx_factory(k=K3, w=W3, threshold=T3, recombination=R3)
    b = ctx_factory(k=K3, w=W3, threshold=T3, recombination=R3)
    try:
        B = dict(A)
        if variant == "device_walks":
            dg = H.DeferredGraph(_write_gfa(g, tmp_path / "full.gfa"))
            assert dg.resolve_on_device(a) and dg.walk_vtx is None and np.array_equal(dg.walk_off, A["walk_off"])
            B["walk_vtx"] = None
        out = auto_panel(a, B, _fasta_pieces(reads) if variant == "text_reads" else reads, 64, chop=chop, text=variant == "text_reads")
        keep = out["keep"]
        assert int(keep.sum()) == 64 and out["n_reads"] == len(reads) and out["n_rounds"] >= 1
        # the same choice from the matrix alone, on a third scout
        _set = lambda c, **kw: c.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"], **kw)
        woff = _set(b, keep=keep, chop=chop)
        assert np.array_equal(woff, out["walk_off"])
        b.add_reads(reads)
        assert a.reads_stats() == b.reads_stats()
        rb = _same_run(a, b, 64)
        assert np.array_equal(a.panel_walks(), np.flatnonzero(keep)) and np.array_equal(b.panel_walks(), np.flatnonzero(keep))
        pv = rb["path_vtx"]
        if chop is not None:
            assert np.array_equal(a.chop_origin(pv)[0], b.chop_origin(pv)[0])
            pv = b.chop_origin(pv)[0]
        assert np.array_equal(a.panel_origin(pv), b.panel_origin(pv))
        assert a.panel_stats()["n_walks_in"] == g.n_walks and a.panel_stats()["n_walks_out"] == 64
        # a second read set on the same context: the scout again from the retained entries, another panel
        if variant == "host":
            reads2 = _reads("many", 1)
            out2 = auto_panel(a, dict(A, walk_vtx=None), reads2, 40)
            c = ctx_factory(k=K3, w=W3, threshold=T3, recombination=R3)
            _scout(c, A)
            c.add_reads(reads2)
            S, _ = c.scout_scores()
            assert np.array_equal(out2["keep"], choose_panel(S, 40)[0])
            _set(c, keep=out2["keep"])
            c.add_reads(reads2)
            _same_run(a, c, 40)
            c.close()
    finally:
        a.close()
        b.close()


def test_keep_reads_flag_and_collect_score(ctx_factory):
    """Without the flag a store goes with its graph; with it the store survives the panel call and a plan does not; the
    scored store leaves the read state of the reads handed over directly, one read length or several."""
    import phi_amd
    g = _graph("dirty")
    A = g.arrays()
    keep = np.zeros(g.n_walks, np.uint8)
    keep[::40] = 1
    rng = np.random.default_rng(8)
    a = ctx_factory(k=K3, w=W3, threshold=T3, recombination=R3)
    b = ctx_factory(k=K3, w=W3, threshold=T3, recombination=R3)
    try:
        _set = lambda c, **kw: c.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], None, keep=keep, **kw)
        for reads in (mosaic_reads(rng, g, n_reads=50, read_len=64, n_seg=2), mosaic_reads(rng, g, n_reads=25, read_len=64, n_seg=2) + [b"ACGTTGCA" * 5, b""]):
            _set(a)
            with pytest.raises(phi_amd.PhiError) as e:
                a.collect_score()
            assert e.value.status == phi_amd.PHI_ERR_STATE
            a.collect_begin(0)
            a.add_reads(reads)
            with pytest.raises(phi_amd.PhiError) as e:          # while collecting
                a.collect_score()
            assert e.value.status == phi_amd.PHI_ERR_STATE
            assert a.collect_end()[0] == len(reads)
            a.ladder_plan(1, [0.5, 1.0])
            _set(a, keep_reads=True)
            with pytest.raises(phi_amd.PhiError):               # the plan went
                a.ladder_advance(0)
            assert a.reads_stats()["n_reads"] == 0              # the read state is reset as ever
            a.collect_score()
            _set(b)
            b.add_reads(reads)
            assert a.reads_stats() == b.reads_stats()
            _same_run(a, b, int(keep.sum()))
            _set(a)                                             # without the flag: the store goes
            with pytest.raises(phi_amd.PhiError) as e:
                a.collect_score()
            assert e.value.status == phi_amd.PHI_ERR_STATE
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 4. a planted case without ties

PLANT_K, PLANT_W, PLANT_BLOCKS = 11, 4, 8


@functools.lru_cache(maxsize=None)
def _planted(tmp):
    """600 diploid samples + REF.  Sites every ~45 bases: every third one a common SNP (random genotypes), the others private to
    truth haplotype T1 (S0, first column) or T2 (S1, second column) in turn: 12 bases replaced by 12 others.  The reads tile a
    mosaic -- T1's alleles at the records of the left half, T2's from the first record of the right half, which is private to
    T2 -- on both strands, error-free, every base covered five times.
    (Why 12 bases and why the join sits there: the model lets a path change walks only where the two part, and the k-mers
    that span the edge it changes on are lost to it.  Entering T2 on its own 12-base allele loses the 10 k-mers that reach
    into it; leaving T1 anywhere else gives up a whole private allele, 30 k-mers and more.  With SNPs the two cost about the
    same number of minimisers and the optimum is not unique.)"""
    import pathlib
    rng = np.random.default_rng(77)
    ref = bytes(rng.choice(list(b"ACGT"), size=4000).tolist())
    n_s = 600
    samples = ["S%d" % i for i in range(n_s)]
    other = lambda c: b"ACGT"[(b"ACGT".index(c) + 1 + int(rng.integers(0, 3))) % 4]
    recs, t1, t2 = [], [], []                                   # per record: T1's / T2's allele
    pos, i = 30, 0
    while pos < len(ref) - 60:
        n = 1 if i % 3 == 0 else 12
        r = ref[pos:pos + n]
        alt = bytes(other(c) for c in r)
        gt = np.zeros((n_s, 2), np.int64)
        if i % 3 == 0:
            gt = rng.integers(0, 2, size=(n_s, 2))
        elif i % 3 == 1:
            gt[0, 0] = 1
        else:
            gt[1, 1] = 1
        recs.append((pos, r, [alt], [b"%d|%d" % (x, y) for x, y in gt.tolist()]))
        t1.append(int(gt[0, 0])); t2.append(int(gt[1, 1]))
        pos += n + int(rng.integers(30, 50))
        i += 1
    half = len(recs) // 2
    assert half % 3 == 2                                        # the first record of the right half is private to T2
    mosaic = bytearray(ref)
    for j, (p, r, alts, _) in enumerate(recs):
        if (t1[j] if j < half else t2[j]):
            mosaic[p:p + len(r)] = alts[0]
    mosaic = bytes(mosaic)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    reads = []
    for at in range(0, len(mosaic) - 100 + 1, 20):
        r = mosaic[at:at + 100]
        reads.append(r if (at // 20) % 2 == 0 else r.translate(comp)[::-1])
    reads.append(mosaic[-100:])
    vcf, fa = _write_case(pathlib.Path(tmp), "planted", ref, samples, recs)
    return vcf, fa, reads, mosaic, half


def test_planted_haplotypes_lead_every_block(oracle, ctx_factory, tmp_path_factory):
    import phi_amd
    from phi_amd.panel import choose_panel
    tmp = tmp_path_factory.mktemp("planted")
    vcf, fa, reads, mosaic, half = _planted(str(tmp))
    # on the CPU first: the Python route's graph, the definition, and in every block one of the two strictly first
    g, _ = _python_graph(vcf, fa, tmp)
    A = _arrays_of(g)
    names = list(g.hap_id2name)
    assert len(names) == 1201
    # the two truth haplotypes among the host reader's walks: by their sequence
    T1 = T2 = None
    seq = np.frombuffer(A["seq_concat"], np.uint8)
    so, wo, wv = A["seq_off"], A["walk_off"], A["walk_vtx"]
    hap_seq = lambda h: b"".join(seq[so[v]:so[v + 1]].tobytes() for v in wv[wo[h]:wo[h + 1]].tolist())
    for h in range(len(names)):
        s = hap_seq(h)
        if s[:1500] == mosaic[:1500] and T1 is None:
            T1 = h
        if s[-1500:] == mosaic[-1500:] and T2 is None:
            T2 = h
    assert T1 is not None and T2 is not None and T1 != T2
    S = _expected(oracle, "planted", A, reads, PLANT_K, PLANT_W, PLANT_BLOCKS)
    order = np.argsort(-S, axis=1, kind="stable")
    for b in range(PLANT_BLOCKS):
        first, second = order[b, 0], order[b, 1]
        assert first in (T1, T2) and S[b, first] > S[b, second], (b, first, S[b, first], S[b, second])
    assert {int(order[b, 0]) for b in range(PLANT_BLOCKS)} == {T1, T2}
    wk, wr = choose_panel(S, 32)
    assert wr[T1] == 0 and wr[T2] == 0
    # the plain route is still refused
    ctx = ctx_factory(k=PLANT_K, w=PLANT_W, threshold=1.0, recombination=2)
    try:
        with pytest.raises(phi_amd.PhiError) as e:
            ctx.set_graph_vcf(vcf, fa)
        assert e.value.status == phi_amd.PHI_ERR_UNSUPPORTED and "1022" in str(e.value)
        v = ctx.set_graph_vcf(vcf, fa, auto_panel=32, reads=reads, n_blocks=PLANT_BLOCKS)
        assert np.array_equal(v.auto["keep"], wk) and np.array_equal(v.auto["round_of"], wr)
        assert v.auto["round_of"][T1] == 0 and v.auto["round_of"][T2] == 0
        assert v.num_walks == 32 and len(v.hap_id2name) == 32 and v.kept_haps.tolist() == np.flatnonzero(wk).tolist()
        res = ctx.solve()
        assert res["optimal"]
        assert ctx.path_sequence(res["hap_len"]) == mosaic
        # auto_panel takes the VCF graph object as it takes a dict of arrays
        from phi_amd.panel import auto_panel
        vg = ctx.vcf_graph(vcf, fa, wide=True)
        out = auto_panel(ctx, vg, reads, 32, n_blocks=PLANT_BLOCKS)
        assert np.array_equal(out["keep"], wk) and ctx.path_sequence(ctx.solve()["hap_len"]) == mosaic
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. state, refusals, limits

def test_states_and_refusals(ctx_factory):
    import phi_amd
    g = _graph("many")
    A = g.arrays()
    reads = _reads("many", 0)
    ctx = ctx_factory(k=K3, w=W3, threshold=T3, recombination=R3)

    def still_works():
        keep = np.zeros(g.n_walks, np.uint8)
        keep[:5] = 1
        ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], None, keep=keep)
        ctx.add_reads(reads)
        assert ctx.solve()["objective"] >= 0

    def refused(status, fn, *words):
        with pytest.raises(phi_amd.PhiError) as e:
            fn()
        assert e.value.status == status, str(e.value)
        for word in words:
            assert word in str(e.value), str(e.value)

    try:
        # scout_scores without a scout: no graph at all, then a set graph
        refused(phi_amd.PHI_ERR_STATE, lambda: ctx.scout_scores(), "scout")
        still_works()
        refused(phi_amd.PHI_ERR_STATE, lambda: ctx.scout_scores(), "scout")
        refused(phi_amd.PHI_ERR_STATE, lambda: ctx.scout_choose(3), "scout")
        still_works()
        # what needs the DP, on a scout
        _scout(ctx, A)
        ctx.add_reads(reads)
        for fn in (ctx.solve, ctx.kept_anchors, ctx.panel_stats, ctx.solve_stats, ctx.chop_stats, ctx.panel_walks, lambda: ctx.path_sequence(10)):
            refused(phi_amd.PHI_ERR_STATE, fn, "scout")
        # ... while the index's accessors and the reads routes work
        assert ctx.reads_stats()["n_reads"] == len(reads) and ctx.index_stats()["n_entries"] == len(A["walk_vtx"])
        assert len(ctx.walk_minimizers(3)[0]) > 0
        still_works()
        # the choice's limits
        _scout(ctx, A)
        ctx.add_reads(reads)
        ctx.scout_scores()
        refused(phi_amd.PHI_ERR_INVALID, lambda: ctx.scout_choose(1023))
        refused(phi_amd.PHI_ERR_INVALID, lambda: ctx.scout_choose(0))
        always = np.zeros(g.n_walks, np.uint8)
        always[:9] = 1
        refused(phi_amd.PHI_ERR_INVALID, lambda: ctx.scout_choose(8, always))
        assert int(ctx.scout_choose(9, always)[0].sum()) == 9
        # the matrix' limits
        refused(phi_amd.PHI_ERR_INVALID, lambda: ctx.scout_scores(65537))
        assert ctx.scout_scores(65536, copy=False)[1]["n_blocks"] == 65536       # 65 536 x 1 100 cells: below 2^31
        still_works()
        # collect_score without a store
        refused(phi_amd.PHI_ERR_STATE, ctx.collect_score)
        still_works()
        # 65 536 walks are refused, 65 535 are not the limit's business (refused later or not: not asked here)
        n = 65536
        one = _graph("single").arrays()
        woff = np.arange(n + 1, dtype=np.int64)
        refused(phi_amd.PHI_ERR_UNSUPPORTED, lambda: ctx.scout_graph(one["seq_concat"], one["seq_off"], one["adj_off"], one["adj"], woff,
                                                                    np.zeros(n, np.int32), one["top_rank"]), "65535")
        still_works()
        # the wide VCF walks: the same refusal one step up; the plain entry point keeps its own
        L = ctx._L
        uf = np.array([0, 1], np.int32)
        out = np.zeros(n + 2, np.int64)
        assert L.phi_vcf_walks_wide(ctx._h, uf.ctypes.data, 1, None, None, 0, None, n, out.ctypes.data) == phi_amd.PHI_ERR_UNSUPPORTED
        assert L.phi_vcf_walks(ctx._h, uf.ctypes.data, 1, None, None, 0, None, 1023, out.ctypes.data) == phi_amd.PHI_ERR_UNSUPPORTED
        assert L.phi_vcf_walks_wide(ctx._h, uf.ctypes.data, 1, None, None, 0, None, 1023, out.ctypes.data) == 0
        still_works()
        # walk_vtx=None with nothing on the device
        ctx.panel_release()
        refused(phi_amd.PHI_ERR_STATE, lambda: _scout(ctx, A, walk_vtx=None))
        still_works()
    finally:
        ctx.close()
