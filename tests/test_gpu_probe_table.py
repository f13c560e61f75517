"""The read table the read kernels probe (phi_launch_read_table, table.hip): aligned 32-byte buckets of two (key, id) slots,
home bucket key & (buckets - 1), linear probing over buckets, and a flag on a bucket when a key whose home it is lies in a
later bucket.  A lookup loads its whole home bucket and walks on only when that flag is set.

Read back after phi_set_graph, the table must hold every walk minimiser once with its dense id, each in its home bucket or
in the chain its home bucket's flag announces; and reads scored through it -- by the window-space, the base-space one-chunk
and the pooled kernel, with bases outside ACGTacgt that take the byte-wise routine -- must give the oracle's hit flags and
spectrum.  PHI_READ_TABLE_BUCKETS sets the first try's buckets: a high load with long overflow chains, and a table too small
for the keys, which raises the table-full flag and is built again at twice the buckets until the keys fit."""
import numpy as np
import pytest

import spectrum_check
from graphgen import mosaic_reads, random_graph, walk_sequence

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
LAYOUTS = {"window": {"PHI_SKETCH_WINDOWS": "1"},
           "base": {"PHI_SKETCH_WINDOWS": "0"},
           "pooled": {"PHI_SKETCH_WINDOWS": "0", "PHI_SKETCH_POOL_MIN": "1", "PHI_SKETCH_WAVES": "3"}}


def _set_graph(ctx, g):
    A = g.arrays()
    ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])


def _walk_minimisers(oracle, g, k, w):
    """distinct walk minimisers in dense-id order: first occurrence in walk position order"""
    walk_h = np.concatenate([oracle.sketch(walk_sequence(g, h), k, w)[0] for h in range(g.n_walks)])
    _, first = np.unique(walk_h, return_index=True)
    return walk_h[np.sort(first)]


def _read_table(ctx):
    import torch
    from phi_amd import dist as pdist
    p, nb = ctx.read_table()
    t = torch.as_tensor(pdist.DevArray(p, nb * 4, "<i8"), device="cuda").cpu().numpy().view(np.uint64).copy()
    return t.reshape(nb, 4), nb


def _lookup(t, nb, h):
    """the probe of sketch.hip restated: (id, buckets loaded) or (None, buckets loaded)"""
    b = int(h) & (nb - 1)
    for n in range(1, 4098):
        if t[b, 0] == h:
            return int(t[b, 1] & np.uint64(0xFFFFFFFF)), n
        if t[b, 2] == h:
            return int(t[b, 3] & np.uint64(0xFFFFFFFF)), n
        if n == 1 and not (int(t[b, 1]) >> 32) & 1:
            return None, n
        if n > 1 and t[b, 2] == EMPTY:
            return None, n
        b = (b + 1) & (nb - 1)
    return None, 4097


def _check_table(t, nb, uniq):
    assert nb & (nb - 1) == 0 and 2 * nb >= len(uniq)
    key0, key1 = t[:, 0], t[:, 2]
    assert not np.any((key0 == EMPTY) & (key1 != EMPTY)), "slot 1 taken before slot 0"
    assert np.all(t[key0 == EMPTY, 1] == 0) and np.all(t[key1 == EMPTY, 3] == 0)
    assert np.all(t[:, 3] >> np.uint64(32) == 0) and np.all(t[:, 1] >> np.uint64(33) == 0)
    keys = np.concatenate([key0, key1])
    ids = np.concatenate([t[:, 1], t[:, 3]]) & np.uint64(0xFFFFFFFF)
    bucket = np.concatenate([np.arange(nb), np.arange(nb)])
    held = keys != EMPTY
    assert held.sum() == len(uniq)
    keys, ids, bucket = keys[held], ids[held].astype(np.int64), bucket[held]
    assert np.array_equal(np.sort(ids), np.arange(len(uniq))) and np.array_equal(uniq[ids], keys)
    flag = (t[:, 1] >> np.uint64(32)) & np.uint64(1)
    full = key1 != EMPTY
    home = (keys & np.uint64(nb - 1)).astype(np.int64)
    displaced = bucket != home
    # a displaced key: its home bucket flagged, and every bucket from its home up to its own full
    assert np.all(flag[home[displaced]] == 1)
    for hb, b in zip(home[displaced], bucket[displaced]):
        span = (np.arange(hb, hb + ((b - hb) % nb)) % nb)
        assert np.all(full[span]), (hb, b)
    # a flag only where a key whose home that bucket is lies further on
    assert np.array_equal(np.flatnonzero(flag), np.unique(home[displaced]))
    for h, i in zip(uniq, range(len(uniq))):
        assert _lookup(t, nb, h)[0] == i
    return int(displaced.sum()), int(flag.sum())


def _graph_and_reads(rng, k, w):
    g = random_graph(rng, n_sites=40, n_walks=6, seg_len=(60, 240), alt_len=(2, 9))
    reads = mosaic_reads(rng, g, n_reads=400, read_len=150, n_seg=2, err=0.01)
    reads += [bytes(rng.choice(list(b"ACGT"), size=150).tolist()) for _ in range(200)]      # novel hashes: misses of the table
    reads = [bytearray(r) for r in reads]
    for i in range(0, len(reads), 7):                                                     # the byte-wise routine
        reads[i][int(rng.integers(0, 150))] = ord("N" if i % 2 else "x")
    for i in range(3, len(reads), 11):
        reads[i] = bytearray(reads[i].lower())
    return g, [bytes(r) for r in reads]


def _overrides(n_unique):
    """None: the table as built for the run; a load of 0.45 -- 0.9 of the slots; far too few buckets (table full, rebuilt)"""
    hi = 1
    while 2 * hi * 0.9 < n_unique:
        hi *= 2
    return {"default": None, "high_load": str(hi), "full": "4"}


@pytest.mark.parametrize("k,w", [(31, 25), (15, 10)])
def test_read_table_layout_and_hits_of_every_read_kernel(oracle, ctx_factory, monkeypatch, k, w):
    import torch
    from phi_amd import dist as pdist
    rng = np.random.default_rng(52000 + 100 * k + w)
    g, reads = _graph_and_reads(rng, k, w)
    uniq = _walk_minimisers(oracle, g, k, w)
    sk = [oracle.sketch(r, k, w)[0] for r in reads]
    read_h = np.unique(np.concatenate(sk))
    want_hits = np.isin(uniq, read_h).astype(np.uint8)
    want_missing = read_h[~np.isin(read_h, uniq)]
    assert 0 < want_hits.sum() < len(uniq) and len(want_missing) > 0
    seen = {}
    for name, buckets in _overrides(len(uniq)).items():
        if buckets is None:
            monkeypatch.delenv("PHI_READ_TABLE_BUCKETS", raising=False)
        else:
            monkeypatch.setenv("PHI_READ_TABLE_BUCKETS", buckets)
        hits_of = {}
        for lay, env in LAYOUTS.items():
            for v in ("PHI_SKETCH_WINDOWS", "PHI_SKETCH_POOL_MIN", "PHI_SKETCH_WAVES"):
                monkeypatch.delenv(v, raising=False)
            for kk, vv in env.items():
                monkeypatch.setenv(kk, vv)
            ctx = ctx_factory(k=k, w=w, threshold=1.0, recombination=5)
            _set_graph(ctx, g)
            if lay == "window":
                t, nb = _read_table(ctx)
                displaced, flagged = _check_table(t, nb, uniq)
                seen[name] = (nb, displaced, flagged)
            ctx.add_reads(reads)
            st = ctx.reads_stats()
            assert st["n_emitted"] == sum(len(x) for x in sk) and st["n_distinct"] == len(read_h), (name, lay)
            p, n = ctx.hits_buffer()
            assert n == len(uniq)
            hits_of[lay] = torch.as_tensor(pdist.DevArray(p, n), device="cuda").cpu().numpy().copy()
            p, m = ctx.spectrum_export()
            sp = torch.as_tensor(pdist.DevArray(p, m, "<i8"), device="cuda").clone().cpu().numpy().view(np.uint64)
            assert np.array_equal(np.sort(sp), want_missing), (name, lay)
            # the same through the vectorised helper of the chromosome-scale tests (its decode against _check_table's)
            keys, ids, _ = spectrum_check.check_context(ctx, read_h, sum(len(x) for x in sk), len(reads), sum(len(r) for r in reads), len(read_h))
            assert np.array_equal(uniq[ids], keys)
            ctx.close()
        for lay, hits in hits_of.items():
            assert np.array_equal(hits, want_hits), (name, lay)
    for v in ("PHI_READ_TABLE_BUCKETS", "PHI_SKETCH_WINDOWS", "PHI_SKETCH_POOL_MIN", "PHI_SKETCH_WAVES"):
        monkeypatch.delenv(v, raising=False)
    nb0 = seen["default"][0]
    assert nb0 * 3 >= 16 * len(uniq) and nb0 * 3 < 32 * len(uniq) + 192        # at most 3/16 key per bucket, the smallest power of two
    assert seen["high_load"][1] > 0 and seen["high_load"][2] > 0                # overflow chains
    assert seen["full"][0] >= len(uniq) / 2 and seen["full"][0] > 4             # built again until the keys fit
