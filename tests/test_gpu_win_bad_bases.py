"""The window-space read kernel keeps no bitmap of bases outside ACGTacgt in LDS through its phases: a wave that holds such a
base stages the bitmap again, over a dead part of its region, before phase 3 and again before the byte-wise routine.
Batches of one length with such bases where that path is exercised hardest -- the first and last read of a wave, the
first and last base of a read, every read of one wave, runs across the boundary of two reads -- scored in window space
(PHI_SKETCH_WINDOWS=1) and in base space (=0), against each other and against the CPU oracle: emitted and distinct read
hashes, the read hashes that are not walk minimisers, and the hit flags."""
import numpy as np
import pytest

from graphgen import random_graph, walk_sequence

pytestmark = pytest.mark.gpu

Q = 8


def _reads_per_wave(k, w, L):
    """phi_sketch_win_reads without the LDS bound (it does not bind at these (k, w, L))"""
    V = L - (k + w - 1) + 1
    G = (V + Q - 1) // Q
    return min(64 // G, 928 // L)


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


def _score(ctx_factory, monkeypatch, g, k, w, reads, layout):
    monkeypatch.setenv("PHI_SKETCH_WINDOWS", layout)
    ctx = ctx_factory(k=k, w=w, threshold=1.0, recombination=5)
    _set_graph(ctx, g)
    ctx.add_reads(reads)
    out = _outputs(ctx)
    monkeypatch.delenv("PHI_SKETCH_WINDOWS")
    ctx.close()
    return out


def _check(oracle, ctx_factory, monkeypatch, g, k, w, reads):
    walk_hashes = set()
    for h in range(g.n_walks):
        walk_hashes.update(oracle.sketch(walk_sequence(g, h), k, w)[0].tolist())
    allh = np.concatenate([oracle.sketch(r, k, w)[0] for r in reads])
    distinct = np.unique(allh)
    missing = np.array(sorted(set(distinct.tolist()) - walk_hashes), np.uint64)
    got = {lay: _score(ctx_factory, monkeypatch, g, k, w, reads, lay) for lay in ("0", "1")}
    for lay, (st, miss, hits) in got.items():
        assert st["n_reads"] == len(reads) and st["n_bases"] == sum(len(r) for r in reads), lay
        assert st["n_emitted"] == len(allh) and st["n_distinct"] == len(distinct), (lay, st, len(allh), len(distinct))
        assert np.array_equal(miss, missing), lay
        assert int(hits.sum()) == len(distinct) - len(missing), lay
    assert np.array_equal(got["0"][2], got["1"][2])


def _graph_reads(rng, g, n, L):
    """reads cut from the walks (so that many of their minimisers hit), upper and lower case"""
    out = []
    for i in range(n):
        s = walk_sequence(g, int(rng.integers(0, g.n_walks)))
        a = int(rng.integers(0, len(s) - L))
        r = bytearray(s[a:a + L])
        if i % 3 == 1:
            r = bytearray(r.lower())
        out.append(r)
    return out


@pytest.mark.parametrize("k,w", [(31, 25), (15, 10), (7, 3)])
@pytest.mark.parametrize("L", [150, 96])
def test_bad_bases_at_wave_and_read_edges(oracle, ctx_factory, monkeypatch, k, w, L):
    rng = np.random.default_rng(41000 + 1000 * k + 10 * w + L)
    g = random_graph(rng, n_sites=10, n_walks=4, seg_len=(120, 300), alt_len=(2, 9))
    R = _reads_per_wave(k, w, L)
    n = 12 * R + 3
    reads = _graph_reads(rng, g, n, L)
    # wave 1: its first read's first base, its last read's last base
    reads[R][0] = ord("N")
    reads[2 * R - 1][L - 1] = ord("n")
    # wave 3: its first read's last base and its last read's first base
    reads[3 * R][L - 1] = ord("N")
    reads[4 * R - 1][0] = ord("N")
    # wave 5: a base outside ACGTacgt in every read, at a different place in each
    for i in range(5 * R, 6 * R):
        reads[i][int(rng.integers(0, L))] = ord("X" if i % 2 else "N")
    # wave 7: a run across the boundary of two reads inside the wave, and one across the boundary of two waves
    if R > 1:
        reads[7 * R][L - 3:] = b"NNN"
        reads[7 * R + 1][:4] = b"nnnn"
    reads[8 * R - 1][L - 5:] = b"NNNNN"
    reads[8 * R][:2] = b"NN"
    # wave 9: one read of nothing but N beside clean reads; the last (partial) wave: a scattered one
    reads[9 * R + R // 2][:] = b"N" * L
    reads[n - 2][L // 2] = ord("N")
    _check(oracle, ctx_factory, monkeypatch, g, k, w, [bytes(r) for r in reads])
