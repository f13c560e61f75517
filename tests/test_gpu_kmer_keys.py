"""The k-mer route of the 150-bp read kernel (sketch_rounds_kmer.inc: clean waves probe a k-mer table and log novel k-mers,
MurmurHash3 only at the flush) against the hash route (PHI_SKETCH_KMER_KEYS=0) and the CPU oracle: reads_stats, the sorted
spectrum_export and the hit flags must be identical -- for batches of 1, 4, 5, 6 and 11 reads, reads cut from walks, random
reads, a novel read twice, lower case, bases outside ACGTacgt in the reads (tagged and untagged chunks in one log) and in
the graph, batches with offsets beside one-length batches, two generations through a reset, chunk logs that spill into the
overflow list, a log that is flushed mid-set and an overflow list that runs full (the replay); and batches at the size
where the route changes (all waves resident at once: the k-mer route; one wave more: the hash route), each also with the
k-mer route forced (PHI_SKETCH_KMER_KEYS=2)."""
import numpy as np
import pytest

from graphgen import random_graph, walk_sequence

pytestmark = pytest.mark.gpu

K, W, L, R = 31, 25, 150, 5


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


def _score(ctx_factory, monkeypatch, g, generations, kmer_keys):
    """generations: a list of read sets, each a list of batches; a reset between them.  Outputs of the last set."""
    monkeypatch.setenv("PHI_SKETCH_WINDOWS", "1")
    monkeypatch.setenv("PHI_SKETCH_KMER_KEYS", kmer_keys)
    ctx = ctx_factory(k=K, w=W, threshold=1.0, recombination=5)
    _set_graph(ctx, g)
    for i, batches in enumerate(generations):
        if i:
            ctx.reset_reads()
        for b in batches:
            ctx.add_reads(b)
    out = _outputs(ctx)
    monkeypatch.delenv("PHI_SKETCH_WINDOWS")
    monkeypatch.delenv("PHI_SKETCH_KMER_KEYS")
    ctx.close()
    return out


def _expect(oracle, g, reads):
    walk_hashes = set()
    for h in range(g.n_walks):
        walk_hashes.update(oracle.sketch(walk_sequence(g, h), K, W)[0].tolist())
    allh = np.concatenate([oracle.sketch(r, K, W)[0] for r in reads])
    distinct = np.unique(allh)
    missing = np.array(sorted(set(distinct.tolist()) - walk_hashes), np.uint64)
    return len(allh), len(distinct), missing


def _check(oracle, ctx_factory, monkeypatch, g, generations):
    got = {f: _score(ctx_factory, monkeypatch, g, generations, f) for f in ("1", "0")}
    a, b = got["1"], got["0"]
    assert a[0] == b[0], (a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    last = [bytes(r) for batch in generations[-1] for r in batch]
    n_emit, n_dist, missing = _expect(oracle, g, last)
    st, miss, hits = a
    assert st["n_reads"] == len(last) and st["n_bases"] == sum(len(r) for r in last)
    assert st["n_emitted"] == n_emit and st["n_distinct"] == n_dist, (st, n_emit, n_dist)
    assert np.array_equal(miss, missing)
    assert int(hits.sum()) == n_dist - len(missing)
    return a


def _graph(seed):
    return random_graph(np.random.default_rng(seed), n_sites=10, n_walks=4, seg_len=(120, 300), alt_len=(2, 9))


def _random_read(rng):
    return bytearray(rng.choice(list(b"ACGT"), size=L).tolist())


def _mixed_reads(rng, g, n):
    """reads cut from the walks (their minimisers hit), every third in lower case, every fourth random (all novel), and one
    novel read twice"""
    out = []
    for i in range(n):
        if i % 4 == 3:
            out.append(_random_read(rng))
            continue
        s = walk_sequence(g, int(rng.integers(0, g.n_walks)))
        a = int(rng.integers(0, len(s) - L))
        r = bytearray(s[a:a + L])
        if i % 3 == 1:
            r = bytearray(r.lower())
        out.append(r)
    if n >= 4:
        out[0] = bytearray(out[3])            # the novel read once more, in another wave position
    return out


@pytest.mark.parametrize("n", [1, 4, 5, 6, 11])
def test_small_batches(oracle, ctx_factory, monkeypatch, n):
    rng = np.random.default_rng(61000 + n + 500)      # (not the graph's stream: a random read would spell its first segment)
    g = _graph(61000 + n)
    reads = _mixed_reads(rng, g, n)
    st, miss, hits = _check(oracle, ctx_factory, monkeypatch, g, [[[bytes(r) for r in reads]]])
    if n >= 4:
        assert len(miss) > 0 and hits.sum() > 0              # both kinds of lookup took place


def test_the_table_is_built_and_reported(ctx_factory, monkeypatch, capfd):
    """PHI_TIMING names the k-mer table, its size and the OVERFLOWED share of both tables: the route under test exists"""
    monkeypatch.setenv("PHI_TIMING", "1")
    g = _graph(61100)
    ctx = ctx_factory(k=K, w=W, threshold=1.0, recombination=5)
    _set_graph(ctx, g)
    ctx.close()
    err = capfd.readouterr().err
    assert "k-mer table of " in err and "OVERFLOWED buckets: read table " in err, err[-2000:]
    assert "no k-mer table for this graph" not in err


def test_bad_bases_in_reads_tagged_and_untagged_chunks(oracle, ctx_factory, monkeypatch):
    """An N at the first and at the last read of a wave; the other waves are clean: k-mer chunks and hash chunks in one log"""
    n = 5 * 6 + 3
    rng = np.random.default_rng(62000 + 500)      # (not the graph's stream: a random read would spell its first segment)
    g = _graph(62000)
    reads = _mixed_reads(rng, g, n)
    reads[R][0] = ord("N")                       # first read of wave 1, first base
    reads[4 * R - 1][L - 1] = ord("n")           # last read of wave 3, last base
    reads[n - 1][L // 2] = ord("N")              # the last (partial) wave
    _check(oracle, ctx_factory, monkeypatch, g, [[[bytes(r) for r in reads]]])


def test_bad_base_inside_a_graph_segment(oracle, ctx_factory, monkeypatch):
    """The minimisers over an N of the graph have no 2-bit k-mer and are absent from the k-mer table; reads cut across it
    (they carry the N: the hash route of their wave) and clean reads beside it still hit"""
    rng = np.random.default_rng(63000 + 500)      # (not the graph's stream: a random read would spell its first segment)
    g = _graph(63000)
    v = max(g.paths[0][3:-3], key=lambda u: len(g.node_seq[u]))   # a backbone segment (every walk goes through it), away from the ends
    s = bytearray(g.node_seq[v])
    s[len(s) // 2] = ord("N")
    g.node_seq[v] = bytes(s)
    walk = walk_sequence(g, 0)
    at = walk.index(b"N")
    reads = _mixed_reads(rng, g, 11)
    reads.append(bytearray(walk[at - 70:at - 70 + L]))      # across the N
    reads.append(bytearray(walk[at + 1:at + 1 + L]))        # clean, right behind it
    reads.append(bytearray(walk[at - L:at]))                # clean, right before it
    st, miss, hits = _check(oracle, ctx_factory, monkeypatch, g, [[[bytes(r) for r in reads]]])
    assert hits.sum() > 0


def test_offsets_batch_and_one_length_batch_in_one_generation(oracle, ctx_factory, monkeypatch):
    rng = np.random.default_rng(64000 + 500)      # (not the graph's stream: a random read would spell its first segment)
    g = _graph(64000)
    a = [bytes(r) for r in _mixed_reads(rng, g, 12)]
    b = [bytes(r) for r in _mixed_reads(rng, g, 7)]
    b[2] = b[2] + b"ACGTTGCA"                    # reads of several lengths: this batch goes in with its offsets
    c = [bytes(r) for r in _mixed_reads(rng, g, 6)]
    _check(oracle, ctx_factory, monkeypatch, g, [[a, b, c]])


def test_two_generations_through_a_reset(oracle, ctx_factory, monkeypatch):
    rng = np.random.default_rng(65000 + 500)      # (not the graph's stream: a random read would spell its first segment)
    g = _graph(65000)
    first = [bytes(_random_read(rng)) for _ in range(40)]
    reads = [bytes(r) for r in _mixed_reads(rng, g, 33)]
    _check(oracle, ctx_factory, monkeypatch, g, [[first], [reads[:20], reads[20:]]])


def test_small_chunk_logs_spill_into_the_overflow_list(oracle, ctx_factory, monkeypatch):
    """PHI_NOV_SHIFT=2: four entries a chunk; a wave with more novel k-mers hashes its chunk itself"""
    monkeypatch.setenv("PHI_NOV_SHIFT", "2")
    rng = np.random.default_rng(66000 + 500)      # (not the graph's stream: a random read would spell its first segment)
    g = _graph(66000)
    reads = [bytes(r) for r in _mixed_reads(rng, g, 5 * 7 + 2)]
    reads[5:10] = [walk_sequence(g, 1)[i * 40:i * 40 + L] for i in range(5)]   # a wave of walk reads: few novel k-mers, stays tagged
    _check(oracle, ctx_factory, monkeypatch, g, [[reads]])


def test_a_tiny_log_budget_flushes_mid_set(oracle, ctx_factory, monkeypatch):
    monkeypatch.setenv("PHI_NOVLOG_BUDGET", "4096")
    rng = np.random.default_rng(67000 + 500)      # (not the graph's stream: a random read would spell its first segment)
    g = _graph(67000)
    reads = [bytes(r) for r in _mixed_reads(rng, g, 60)]
    _check(oracle, ctx_factory, monkeypatch, g, [[reads[:25], reads[25:45], reads[45:]]])


def test_a_full_overflow_list_replays_the_batch(oracle, ctx_factory, monkeypatch):
    monkeypatch.setenv("PHI_NOV_SHIFT", "2")
    monkeypatch.setenv("PHI_OVLIST_CAP", "8")
    rng = np.random.default_rng(68000 + 500)      # (not the graph's stream: a random read would spell its first segment)
    g = _graph(68000)
    reads = [bytes(r) for r in _mixed_reads(rng, g, 41)]
    _check(oracle, ctx_factory, monkeypatch, g, [[reads[:30], reads[30:]]])


@pytest.mark.parametrize("extra", [0, 1])
def test_batches_at_the_size_where_the_route_changes(ctx_factory, monkeypatch, extra):
    """The k-mer route is taken by batches whose waves are all resident at once (seven a SIMD: 28 a CU).  The largest such
    batch, and one wave more (the hash route), with scattered N and lower case; each equals the hash route, and so does the
    k-mer route forced on both (PHI_SKETCH_KMER_KEYS=2).  (The oracle checks the same paths on the small batches above.)"""
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count * 28 * R + extra * R
    rng = np.random.default_rng(69000 + extra)
    g = _graph(69000)
    codes = np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, size=n * L)].copy()
    walk = np.frombuffer(bytes(walk_sequence(g, 0)), np.uint8)
    for i in range(0, n, 3):                   # every third read from a walk: hits
        a = int(rng.integers(0, len(walk) - L))
        codes[i * L:(i + 1) * L] = walk[a:a + L]
    codes[rng.integers(0, len(codes), size=n // 50)] = ord("N")
    reads = (codes, np.arange(n + 1, dtype=np.int64) * L)
    got = {f: _score(ctx_factory, monkeypatch, g, [[reads]], f) for f in ("1", "0", "2")}
    for f in ("1", "2"):
        assert got[f][0] == got["0"][0], (f, got[f][0], got["0"][0])
        assert np.array_equal(got[f][1], got["0"][1]) and np.array_equal(got[f][2], got["0"][2])
    assert got["0"][0]["n_reads"] == n and len(got["0"][1]) > 0 and got["0"][2].sum() > 0
