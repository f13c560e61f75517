"""The fixed-geometry window kernel (sketch_win_fixed.hip: 150-bp reads at k = 31, w = 25) against the generic window kernel
(PHI_SKETCH_WIN_FIXED=0) and the CPU oracle: counters, the read hashes that are not walk minimisers, and the hit flags --
for batches of 1, 4, 5, 6 and an odd number of reads, bases outside ACGTacgt at the edges of waves and reads, lower case,
a misaligned base pointer, large batches and two generations through a reset (clean_finish)."""
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


def _score(ctx_factory, monkeypatch, g, generations, fixed, feed=None):
    """generations: a list of read sets, each a list of batches; a reset between them.  Outputs of the last set."""
    monkeypatch.setenv("PHI_SKETCH_WINDOWS", "1")
    monkeypatch.setenv("PHI_SKETCH_WIN_FIXED", fixed)
    ctx = ctx_factory(k=K, w=W, threshold=1.0, recombination=5)
    _set_graph(ctx, g)
    for i, batches in enumerate(generations):
        if i:
            ctx.reset_reads()
        for b in batches:
            feed(ctx, b) if feed else ctx.add_reads(b)
    out = _outputs(ctx)
    monkeypatch.delenv("PHI_SKETCH_WINDOWS")
    monkeypatch.delenv("PHI_SKETCH_WIN_FIXED")
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


def _same(a, b):
    assert a[0] == b[0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _check(oracle, ctx_factory, monkeypatch, g, generations, feed=None):
    got = {f: _score(ctx_factory, monkeypatch, g, generations, f, feed) for f in ("1", "0")}
    _same(got["1"], got["0"])
    if oracle is not None:
        last = [bytes(r) for b in generations[-1] for r in b]
        n_emit, n_dist, missing = _expect(oracle, g, last)
        st, miss, hits = got["1"]
        assert st["n_reads"] == len(last) and st["n_bases"] == L * len(last)
        assert st["n_emitted"] == n_emit and st["n_distinct"] == n_dist, (st, n_emit, n_dist)
        assert np.array_equal(miss, missing)
        assert int(hits.sum()) == n_dist - len(missing)


def _graph(seed):
    return random_graph(np.random.default_rng(seed), n_sites=10, n_walks=4, seg_len=(120, 300), alt_len=(2, 9))


def _graph_reads(rng, g, n):
    """reads cut from the walks (many of their minimisers hit), every third in lower case"""
    out = []
    for i in range(n):
        s = walk_sequence(g, int(rng.integers(0, g.n_walks)))
        a = int(rng.integers(0, len(s) - L))
        r = bytearray(s[a:a + L])
        if i % 3 == 1:
            r = bytearray(r.lower())
        out.append(r)
    return out


@pytest.mark.parametrize("n", [1, 4, 5, 6, 13, 5 * 9 + 2])
def test_small_batches(oracle, ctx_factory, monkeypatch, n):
    rng = np.random.default_rng(52000 + n)
    g = _graph(52000 + n)
    reads = _graph_reads(rng, g, n)
    _check(oracle, ctx_factory, monkeypatch, g, [[[bytes(r) for r in reads]]])


@pytest.mark.parametrize("n", [6, 5 * 12 + 3])
def test_bad_bases_at_wave_and_read_edges(oracle, ctx_factory, monkeypatch, n):
    rng = np.random.default_rng(53000 + n)
    g = _graph(53000 + n)
    reads = _graph_reads(rng, g, n)
    reads[0][0] = ord("N")                       # first base of the first read of wave 0
    reads[R - 1 if n > R else n - 1][L - 1] = ord("n")   # last base of the last read of wave 0
    if n > 2 * R:
        reads[R][L - 1] = ord("N")               # last base of the first read of wave 1
        reads[2 * R - 1][0] = ord("X")           # first base of the last read of wave 1
        reads[3 * R][:3] = b"NNN"                # a run at the start of a wave
        reads[4 * R - 1][L - 4:] = b"NNNN"       # ... across the seam of two waves
        reads[4 * R][:2] = b"nn"
        reads[6 * R + 2][:] = b"N" * L           # a read of nothing but N
        for i in range(8 * R, 9 * R):            # every read of one wave, somewhere
            reads[i][int(rng.integers(0, L))] = ord("N")
        reads[n - 1][L // 2] = ord("N")          # the last (partial) wave
    _check(oracle, ctx_factory, monkeypatch, g, [[[bytes(r) for r in reads]]])


def test_two_generations_through_a_reset(oracle, ctx_factory, monkeypatch):
    """The first launch after a reset empties what the previous generation filled (clean_finish), by the waves of this kernel;
    small chunk logs (PHI_NOV_SHIFT=2) send most novel hashes to the overflow list."""
    monkeypatch.setenv("PHI_NOV_SHIFT", "2")
    rng = np.random.default_rng(54000)
    g = _graph(54000)
    rand = [bytes(rng.choice(list(b"ACGT"), size=L).tolist()) for _ in range(300)]
    reads = [bytes(r) for r in _graph_reads(rng, g, 203)]
    _check(oracle, ctx_factory, monkeypatch, g, [[rand], [reads[:120], reads[120:]]])


def test_misaligned_base_pointer(oracle, ctx_factory, monkeypatch):
    """Bases at an odd device address (phase 0 takes the byte-wise load), no offsets array: as the command line hands them."""
    import torch
    rng = np.random.default_rng(55000)
    g = _graph(55000)
    reads = [bytes(r) for r in _graph_reads(rng, g, 5 * 40 + 3)]
    reads[7] = b"N" + reads[7][1:]
    buf = np.frombuffer(b"x" * 3 + b"".join(reads), np.uint8).copy()
    d_b = torch.from_numpy(buf).cuda()

    def feed(ctx, batch):
        ctx.add_reads_device(d_b.data_ptr() + 3, None, len(batch), L * len(batch))
    _check(oracle, ctx_factory, monkeypatch, g, [[reads]], feed)


@pytest.mark.parametrize("n", [34386, 30720 + 7])
def test_large_batches(ctx_factory, monkeypatch, n):
    """C2-sized batches (6 880 waves) of random and walk reads with scattered bases outside ACGTacgt and lower case: the two
    kernels agree (the oracle checks the same paths on the small batches above)."""
    rng = np.random.default_rng(56000 + n)
    g = _graph(56000)
    codes = np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, size=n * L)].copy()
    walk = np.frombuffer(bytes(walk_sequence(g, 0)), np.uint8)
    for i in range(0, n, 7):                   # every seventh read from a walk: hits
        a = int(rng.integers(0, len(walk) - L))
        codes[i * L:(i + 1) * L] = walk[a:a + L]
    codes[rng.integers(0, len(codes), size=n // 20)] = ord("N")
    reads = (codes, np.arange(n + 1, dtype=np.int64) * L)
    _check(None, ctx_factory, monkeypatch, g, [[reads]])
