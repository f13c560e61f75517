"""Reads of one length scored in window space (phi_sketch_win_kernel) and in base space (phi_sketch_kernel /
phi_sketch_pool_kernel): the same batches both ways, forced by PHI_SKETCH_WINDOWS ("1": window space wherever the geometry
allows, "0": never), against each other and against the CPU oracle -- emitted and distinct read hashes, the read hashes
that are not walk minimisers as a set, and the hit flags.  Hits, counters and the spectrum do not depend on how windows
are grouped into waves."""
import numpy as np
import pytest

from graphgen import mosaic_reads, random_graph, walk_sequence

pytestmark = pytest.mark.gpu


def _set_graph(ctx, g):
    A = g.arrays()
    ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])


def _outputs(ctx):
    import torch
    from phi_amd import dist as pdist
    st = ctx.reads_stats()
    p, m = ctx.spectrum_export()
    missing = np.sort(torch.as_tensor(pdist.DevArray(p, m, "<i8"), device="cuda").clone().cpu().numpy().view(np.uint64)) if m else np.zeros(0, np.uint64)
    p, nu = ctx.hits_buffer()
    hits = torch.as_tensor(pdist.DevArray(p, nu), device="cuda").cpu().numpy().copy()
    return st, missing, hits


def _score(ctx_factory, monkeypatch, g, k, w, rounds, layout):
    """rounds: a list of read sets, each a list of batches (lists of reads); a reset between read sets.  Returns the
    outputs of the last read set."""
    monkeypatch.setenv("PHI_SKETCH_WINDOWS", layout)
    ctx = ctx_factory(k=k, w=w, threshold=1.0, recombination=5)
    _set_graph(ctx, g)
    for i, batches in enumerate(rounds):
        if i:
            ctx.reset_reads()
        for b in batches:
            ctx.add_reads(b)
    out = _outputs(ctx)
    monkeypatch.delenv("PHI_SKETCH_WINDOWS")
    ctx.close()
    return out


def _expect(oracle, g, k, w, reads):
    walk_hashes = set()
    for h in range(g.n_walks):
        walk_hashes.update(oracle.sketch(walk_sequence(g, h), k, w)[0].tolist())
    sk = [oracle.sketch(r, k, w)[0] for r in reads]
    allh = np.concatenate(sk) if sk else np.zeros(0, np.uint64)
    distinct = np.unique(allh)
    missing = np.array(sorted(set(distinct.tolist()) - walk_hashes), np.uint64)
    return len(allh), len(distinct), missing


def _check_both_ways(oracle, ctx_factory, monkeypatch, g, k, w, rounds):
    last = [r for b in rounds[-1] for r in b]
    n_emit, n_dist, missing = _expect(oracle, g, k, w, last)
    got = {lay: _score(ctx_factory, monkeypatch, g, k, w, rounds, lay) for lay in ("0", "1")}
    for lay, (st, miss, hits) in got.items():
        assert st["n_reads"] == len(last) and st["n_bases"] == sum(len(r) for r in last), lay
        assert st["n_emitted"] == n_emit and st["n_distinct"] == n_dist, (lay, st, n_emit, n_dist)
        assert np.array_equal(miss, missing), lay
        assert int(hits.sum()) == n_dist - len(missing), lay
    assert np.array_equal(got["0"][2], got["1"][2])


def _rand(rng, n, L, alphabet=b"ACGT"):
    return [bytes(rng.choice(list(alphabet), size=L).tolist()) for _ in range(n)]


@pytest.mark.parametrize("k,w", [(31, 25), (15, 10), (21, 11), (5, 200), (32, 12), (7, 3)])
def test_one_length_batches_both_layouts(oracle, ctx_factory, monkeypatch, k, w):
    """Every length from the one-length path's lower bound (32) and from k + w - 2 over every residue of V mod 8, up to
    and past 150, and 2 000 (base space whatever the switch says); batches of reads from the graph, novel reads, and a
    batch smaller than one wave."""
    rng = np.random.default_rng(31000 + 100 * k + w)
    g = random_graph(rng, n_sites=10, n_walks=4, seg_len=(30, 90), alt_len=(2, 9))
    span = k + w - 1
    lengths = sorted({32, 33, 64, 100, 149, 150, 151, 160, 250, 300, 600, 2000} | {max(32, span - 1 + v) for v in range(0, 10)})
    for L in lengths:
        reads = mosaic_reads(rng, g, n_reads=37, read_len=L, n_seg=2, err=0.01) if L <= 600 else []
        reads = [r for r in reads if len(r) == L]
        reads += _rand(rng, 23, L)
        small = _rand(rng, 3, L)
        _check_both_ways(oracle, ctx_factory, monkeypatch, g, k, w, [[reads, small]])


@pytest.mark.parametrize("k,w", [(31, 25), (15, 10), (5, 200)])
def test_bases_outside_acgt_at_read_ends_and_wave_seams(oracle, ctx_factory, monkeypatch, k, w):
    """N / n and other bytes at the first and last base of reads, on the reads that open and close a wave (in window space)
    and on reads that straddle two chunks (in base space), and scattered; lower case too."""
    rng = np.random.default_rng(32000 + 100 * k + w)
    g = random_graph(rng, n_sites=8, n_walks=3, seg_len=(30, 90), alt_len=(2, 9))
    for L in (150, 151, 100, k + w + 3, 300):
        L = max(L, 32)
        reads = [bytearray(r) for r in _rand(rng, 90, L, b"ACGTacgt")]
        for i, r in enumerate(reads):
            if i % 5 == 0:
                r[0] = ord("N")
            if i % 5 == 4:
                r[-1] = ord("n")
            if i % 7 == 3:
                r[int(rng.integers(0, L))] = ord("N")
            if i % 11 == 6:
                r[int(rng.integers(0, L))] = ord("X")
        reads[40][:] = b"N" * L                        # a read of nothing but N
        reads = [bytes(r) for r in reads]
        _check_both_ways(oracle, ctx_factory, monkeypatch, g, k, w, [[reads]])


def test_logs_that_overflow_and_read_sets_after_a_reset(oracle, ctx_factory, monkeypatch):
    """Chunk logs of four entries (PHI_NOV_SHIFT=2) and small w on novel sequence: most of a wave's novel hashes go to the
    overflow list.  Three read sets against one context, a reset between them: the first launch after a reset empties
    what the previous set filled, by the waves of the new layout."""
    monkeypatch.setenv("PHI_NOV_SHIFT", "2")
    rng = np.random.default_rng(33000)
    g = random_graph(rng, n_sites=8, n_walks=3, seg_len=(30, 90), alt_len=(2, 9))
    for (k, w) in ((31, 25), (11, 2), (15, 4)):
        rounds = [[_rand(rng, 300, 150)], [_rand(rng, 120, 151), _rand(rng, 5, 151)], [_rand(rng, 200, 150), _rand(rng, 64, 150)]]
        _check_both_ways(oracle, ctx_factory, monkeypatch, g, k, w, rounds)


def test_pooled_size_batch_both_layouts(ctx_factory, monkeypatch):
    """A batch of 24 576 chunks and more: window space by default and when forced, the pooled kernel when
    PHI_SKETCH_WINDOWS=0 -- the same outputs."""
    rng = np.random.default_rng(34000)
    g = random_graph(rng, n_sites=8, n_walks=3, seg_len=(30, 90), alt_len=(2, 9))
    n = 84000                                          # 12.6 Mbases of 150-bp reads
    codes = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n * 150)]
    reads = (codes, np.arange(n + 1, dtype=np.int64) * 150)
    got = {lay: _score(ctx_factory, monkeypatch, g, 31, 25, [[reads]], lay) for lay in ("0", "1")}
    ctx = ctx_factory(k=31, w=25, threshold=1.0, recombination=5)
    _set_graph(ctx, g)
    ctx.add_reads(reads)
    got["default"] = _outputs(ctx)
    ctx.close()
    for lay in ("1", "default"):
        assert got["0"][0] == got[lay][0]
        assert np.array_equal(got["0"][1], got[lay][1]) and np.array_equal(got["0"][2], got[lay][2])
