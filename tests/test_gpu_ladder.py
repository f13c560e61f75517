"""A ladder of coverages from one read set (phi_reads_collect_*, phi_ladder_*; ladder.hip) against the rule of
phi_amd/ladder.py, which shares no code with the device: the partition read by read and byte by byte, the read state of
every level against a fresh context handed that level's reads, the state errors, and a band that overflows the list of
novel hashes."""
import numpy as np
import pytest

from graphgen import mosaic_reads, random_graph

from phi_amd import _capi
from phi_amd import ladder as rule
from phi_amd.context import PhiError

pytestmark = pytest.mark.gpu


def _set_graph(ctx, g):
    A = g.arrays()
    ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])


@pytest.fixture(scope="module")
def small_ctx(ctx_factory):
    rng = np.random.default_rng(11)
    g = random_graph(rng, n_sites=6, n_walks=3, seg_len=(8, 20), alt_len=(1, 4))
    ctx = ctx_factory(k=7, w=4, threshold=1.0, recombination=3)
    _set_graph(ctx, g)
    return ctx


def _rand_reads(rng, lens):
    return [bytes(rng.choice(list(b"ACGTN"), size=int(n)).tolist()) for n in lens]


def _check_partition(ctx, batches, seed, fractions, first_ordinal=0):
    """collect the batches, plan, and compare every band with the rule: ordinals, bases, offsets, info"""
    reads = [r for b in batches for r in b]
    # add_reads hands a batch of one read length (>= 32) over without offsets: a store of such batches, all of the same
    # length, is "of one read length"
    lens = {len(r) for r in reads}
    one_length = lens.pop() if len(lens) == 1 and min(lens) >= 32 else 0
    ctx.collect_begin(first_ordinal)
    for b in batches:
        ctx.add_reads(b)
    nr, nb = ctx.collect_end()
    assert (nr, nb) == (len(reads), sum(len(r) for r in reads))
    info = ctx.ladder_plan(seed, fractions)
    L = len(fractions)
    ordinals = (np.arange(len(reads), dtype=np.uint64) + np.uint64(first_ordinal)).astype(np.uint64)
    band = rule.bands(seed, ordinals, fractions) if len(reads) else np.zeros(0, np.int32)
    assert info["n_levels"] == L and info["n_reads"] == nr and info["n_bases"] == nb
    assert info["one_length"] == one_length
    assert info["threshold"] == [int(t) for t in rule.thresholds(fractions)]
    kept = 0
    for j in range(L):
        idx = np.flatnonzero(band == j)
        ords, bases, off = ctx.ladder_band(j, data=True)
        assert np.array_equal(ords.view(np.uint64), ordinals[idx]), (j, len(ords), len(idx))
        want = [reads[i] for i in idx]
        want_off = np.zeros(len(want) + 1, np.int64)
        np.cumsum([len(r) for r in want], out=want_off[1:])
        assert np.array_equal(off, want_off), j
        assert bases.tobytes() == b"".join(want), j
        assert info["band_reads"][j] == len(idx) and info["band_bases"][j] == want_off[-1]
        kept += len(idx)
    assert info["n_kept_reads"] == kept
    return info, band


MIXED = [0, 1, 15, 16, 17, 150]
FOUR = [0.0, 0.3, 0.3, 1.0]                     # a 0, two equal neighbours (an empty band), a 1


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_partition_of_mixed_lengths_equals_the_rule(small_ctx, n):
    rng = np.random.default_rng(100 + n)
    lens = rng.choice(MIXED, size=n)
    if n >= 63:
        lens[n // 3] = 5000                                      # one long read
    _check_partition(small_ctx, [_rand_reads(rng, lens)], seed=n, fractions=FOUR)


@pytest.mark.parametrize("n", [1, 65, 1000])
def test_partition_of_one_read_length_keeps_the_property(small_ctx, n):
    rng = np.random.default_rng(200 + n)
    info, _ = _check_partition(small_ctx, [_rand_reads(rng, [150] * n)], seed=5, fractions=[0.2, 0.5, 0.9])
    assert info["one_length"] == 150                             # phi_ladder_advance passes such bands without offsets


@pytest.mark.parametrize("fractions", [[0.4], [1.0], [i / 16 for i in range(1, 17)], [0.0] * 16])
def test_partition_with_one_and_sixteen_levels(small_ctx, fractions):
    rng = np.random.default_rng(300 + len(fractions))
    _check_partition(small_ctx, [_rand_reads(rng, rng.choice(MIXED, size=700))], seed=9, fractions=fractions)


def test_all_reads_dropped_and_an_empty_store(small_ctx):
    rng = np.random.default_rng(400)
    info, band = _check_partition(small_ctx, [_rand_reads(rng, rng.choice(MIXED, size=300))], seed=1, fractions=[0.0, 0.0])
    assert info["n_kept_reads"] == 0 and (band == 2).all()
    info, _ = _check_partition(small_ctx, [], seed=1, fractions=FOUR)
    assert info["n_reads"] == 0 and info["n_kept_reads"] == 0
    small_ctx.reset_reads()
    small_ctx.ladder_advance(3)                                  # nothing to score
    assert small_ctx.reads_stats()["n_reads"] == 0


def test_ordinals_continue_across_batches_and_start_where_told(small_ctx):
    rng = np.random.default_rng(500)
    batches = [_rand_reads(rng, rng.choice(MIXED, size=n)) for n in (130, 1, 400)]
    _check_partition(small_ctx, batches, seed=77, fractions=FOUR)
    _check_partition(small_ctx, batches, seed=77, fractions=[0.1, 0.6], first_ordinal=2 ** 33 + 5)
    # batches of one length each, but not the same one: not a store of one length
    _check_partition(small_ctx, [_rand_reads(rng, [150] * 70), _rand_reads(rng, [100] * 70)], seed=3, fractions=[0.5, 1.0])


def test_bad_fractions_are_refused(small_ctx):
    small_ctx.collect_begin()
    small_ctx.add_reads([b"ACGTACGTACGT"])
    small_ctx.collect_end()
    for bad in ([0.5, 0.4], [-0.1], [], [0.1] * 17, [float("nan")]):
        with pytest.raises(PhiError) as e:
            small_ctx.ladder_plan(0, bad)
        assert e.value.status == _capi.PHI_ERR_INVALID
    assert small_ctx.ladder_plan(0, [0.5, 7.0])["threshold"] == [1 << 31, 1 << 32]


# --------------------------------------------------------------------------- the read state of every level

KEYS = ("spectrum_size", "filtered", "n_in_model", "objective")


def _level_case(k, w):
    rng = np.random.default_rng(1000 + k)
    if k == 31:
        g = random_graph(rng, n_sites=30, n_walks=4, seg_len=(40, 90), alt_len=(1, 8), p_del=0.2)
        reads = mosaic_reads(rng, g, n_reads=400, read_len=150, n_seg=3, err=0.01)
        reads = [r for r in reads if len(r) == 150]
        assert len(reads) > 300
    else:
        g = random_graph(rng, n_sites=int(rng.integers(10, 40)), n_walks=4, seg_len=(4, 30), alt_len=(1, 8), p_del=0.2)
        reads = mosaic_reads(rng, g, n_reads=300, read_len=40, n_seg=3, err=0.02)
        reads += [bytes(rng.choice(list(b"ACGTN"), size=200).tolist()) for _ in range(3)]
    return rng, g, reads


def _same_state(got_stats, got, want_stats, want):
    assert got_stats == want_stats, (got_stats, want_stats)
    for key in KEYS:
        assert got[key] == want[key], (key, got[key], want[key])
    assert np.array_equal(got["path_vtx"], want["path_vtx"]) and np.array_equal(got["path_hap"], want["path_hap"])


@pytest.mark.parametrize("k,w", [(7, 4), (31, 25)])
def test_level_state_equals_a_fresh_context(ctx_factory, k, w):
    """After ladder_advance(j) -- add, solve, add, solve on one context -- the read state and the solve equal those of a
    fresh context given the rule's level-j reads in shuffled order."""
    rng, g, reads = _level_case(k, w)
    fractions = [0.1, 0.35, 0.7, 1.0]
    seed = 42
    ctx = ctx_factory(k=k, w=w, threshold=1.0, recombination=5)
    _set_graph(ctx, g)
    ctx.collect_begin()
    ctx.add_reads(reads[:100])
    ctx.add_reads(reads[100:])
    ctx.collect_end()
    info = ctx.ladder_plan(seed, fractions)
    assert info["one_length"] == (150 if k == 31 else 0)
    band = rule.bands(seed, np.arange(len(reads)), fractions)
    assert 0 < (band == 0).sum() and (band <= 3).all()
    ctx.reset_reads()
    want = []
    for j in range(4):
        level = [reads[i] for i in np.flatnonzero(band <= j)]
        fresh = ctx_factory(k=k, w=w, threshold=1.0, recombination=5)
        _set_graph(fresh, g)
        fresh.add_reads([level[i] for i in rng.permutation(len(level))])
        want.append((fresh.reads_stats(), fresh.solve()))
        fresh.close()
        ctx.ladder_advance(j)
        _same_state(ctx.reads_stats(), ctx.solve(), *want[j])
    # a rewind keeps the plan
    ctx.reset_reads()
    ctx.ladder_advance(0)
    _same_state(ctx.reads_stats(), ctx.solve(), *want[0])
    ctx.ladder_advance(2)                                        # two bands in one call
    _same_state(ctx.reads_stats(), ctx.solve(), *want[2])


def test_coverage_ladder_yields_one_result_per_level(ctx_factory):
    rng, g, reads = _level_case(7, 4)
    ctx = ctx_factory(k=7, w=4, threshold=1.0, recombination=5)
    _set_graph(ctx, g)
    total = sum(len(r) for r in reads)
    coverages, genome = [0.5, 1, 2, 400], total // 4             # fractions 1/8, 1/4, 1/2, clipped at 1
    fr = rule.fractions_from_coverage(coverages, genome, total)
    assert fr[3] == 1.0
    band = rule.bands(3, np.arange(len(reads)), fr)
    text = b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads))
    for kind in ("list", "text"):
        src = reads if kind == "list" else [text[:len(text) // 2], text[len(text) // 2:]]
        out = list(ctx.coverage_ladder(src, coverages, genome, seed=3, text=kind == "text"))
        assert [r["coverage"] for r in out] == coverages
        for j, r in enumerate(out):
            level = [reads[i] for i in np.flatnonzero(band <= j)]
            assert (r["n_reads"], r["n_bases"]) == (len(level), sum(len(x) for x in level))
            fresh = ctx_factory(k=7, w=4, threshold=1.0, recombination=5)
            _set_graph(fresh, g)
            fresh.add_reads(level)
            want = fresh.solve()
            fresh.close()
            for key in KEYS:
                assert r[key] == want[key], (kind, j, key)
            assert np.array_equal(r["path_vtx"], want["path_vtx"])


# --------------------------------------------------------------------------- state errors

def test_state_errors_leave_the_context_usable(ctx_factory):
    rng, g, reads = _level_case(7, 4)
    ctx = ctx_factory(k=7, w=4, threshold=1.0, recombination=5)

    def refused(fn, *a):
        with pytest.raises(PhiError) as e:
            fn(*a)
        assert e.value.status == _capi.PHI_ERR_STATE, e.value

    refused(ctx.collect_begin)                                   # before set_graph
    _set_graph(ctx, g)
    refused(ctx.collect_end)                                     # without begin
    refused(ctx.ladder_advance, 0)                               # before plan
    refused(ctx.ladder_plan, 1, [0.5])                           # without a store
    ctx.collect_begin()
    refused(ctx.collect_begin)                                   # twice
    ctx.add_reads(reads)
    assert ctx.reads_stats()["n_reads"] == 0                     # collected, not scored
    refused(ctx.ladder_plan, 1, [0.5])                           # while collecting
    assert ctx.collect_end() == (len(reads), sum(len(r) for r in reads))
    ctx.ladder_plan(1, [0.3, 0.6, 1.0])
    ctx.ladder_advance(1)
    refused(ctx.ladder_advance, 0)                               # below a level already scored
    ctx.ladder_advance(1)                                        # (the same level again: nothing to do)
    ctx.ladder_advance(2)
    fresh = ctx_factory(k=7, w=4, threshold=1.0, recombination=5)
    _set_graph(fresh, g)
    fresh.add_reads(reads)
    _same_state(ctx.reads_stats(), ctx.solve(), fresh.reads_stats(), fresh.solve())
    # a new graph drops store and plan
    _set_graph(ctx, g)
    refused(ctx.ladder_advance, 0)
    refused(ctx.ladder_plan, 1, [0.5])
    ctx.add_reads(reads)
    _same_state(ctx.reads_stats(), ctx.solve(), fresh.reads_stats(), fresh.solve())


# --------------------------------------------------------------------------- a band that overflows the list of novel hashes

def test_a_band_that_overflows_the_novel_hash_list_is_replayed(ctx_factory, monkeypatch):
    rng = np.random.default_rng(606)
    g = random_graph(rng, n_sites=10, n_walks=3, seg_len=(30, 60), alt_len=(2, 8))
    k, w = 15, 10
    reads = [bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(60, 140))).tolist()) for _ in range(3000)]
    reads += mosaic_reads(rng, g, n_reads=40, read_len=60, n_seg=2)
    monkeypatch.setenv("PHI_NOV_SHIFT", "2")
    monkeypatch.setenv("PHI_OVLIST_CAP", "50")
    fractions = [0.3, 1.0]
    band = rule.bands(8, np.arange(len(reads)), fractions)
    ctx = ctx_factory(k=k, w=w, threshold=1.0, recombination=3)
    _set_graph(ctx, g)
    ctx.collect_begin()
    ctx.add_reads(reads)
    ctx.collect_end()
    ctx.ladder_plan(8, fractions)
    ctx.reset_reads()
    for j in range(2):
        fresh = ctx_factory(k=k, w=w, threshold=1.0, recombination=3)
        _set_graph(fresh, g)
        fresh.add_reads([reads[i] for i in np.flatnonzero(band <= j)])
        want_stats, want = fresh.reads_stats(), fresh.solve()
        fresh.close()
        ctx.ladder_advance(j)
        got_stats, got = ctx.reads_stats(), ctx.solve()
        assert got_stats == want_stats and want_stats["n_distinct"] > 10000
        assert got["spectrum_size"] == want["spectrum_size"]
