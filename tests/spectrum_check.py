"""The read side of a context against the oracle's read spectrum, element for element (test infrastructure).

What a context holds after its reads were scored: a hit flag per distinct walk minimiser (dense id order), the read hashes
that are no walk minimiser (the novel list), and the read table that maps a walk minimiser to its dense id.  Hit keys plus
novel list is the GPU's read spectrum; check_read_side asserts that it equals the oracle's sorted spectrum S as a set, not
only in size.  Everything is vectorised numpy: the table of the chromosome-scale configuration holds tens of millions of
keys in 2^27 and more buckets, and is decoded in pieces of buckets.

The table (phi_launch_read_table, table.hip): 32-byte buckets of two (key, id word) slots, home bucket key & (buckets - 1),
linear probing over buckets.  A slot's id is the low 32 bits of its second word; bit 32 of a bucket's FIRST id word flags
the bucket as the home of a key that lies further on."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
LOW32 = np.uint64(0xFFFFFFFF)
MAX_PROBE = 4096                        # buckets a key may lie past its home (PHI_MAX_PROBE)


def _show(a, n=4):
    return [hex(int(x)) for x in a[:n]]


def _is_member(sorted_set, x):
    """x[i] in sorted_set, for a sorted duplicate-free uint64 array"""
    if len(sorted_set) == 0:
        return np.zeros(len(x), bool)
    i = np.searchsorted(sorted_set, x)
    i[i == len(sorted_set)] = 0
    return sorted_set[i] == x


def decode_read_table(pieces, nb):
    """pieces: (rows, 4) uint64 arrays that together are the nb buckets in order.  Asserts the table's structure and
    returns (keys, ids, info): the held keys with their dense ids, info = displaced keys, flagged buckets, longest chain.

    Structure: slot 1 never taken before slot 0; empty slots zeroed; nothing but the id and the flag bit in the id words;
    every displaced key's home bucket flagged and every bucket from its home up to its own full (what makes the probe of
    sketch.hip find it); flags only where a displaced key has its home."""
    assert nb > 0 and nb & (nb - 1) == 0, nb
    flag, full = np.zeros(nb, bool), np.zeros(nb, bool)
    keys, ids, bucket = [], [], []
    at = 0
    for t in pieces:
        t = np.asarray(t).view(np.uint64).reshape(-1, 4)
        n = len(t)
        k0, w0, k1, w1 = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
        e0, e1 = k0 == EMPTY, k1 == EMPTY
        assert not np.any(e0 & ~e1), "slot 1 taken before slot 0"
        assert not np.any(w0[e0]) and not np.any(w1[e1]), "an empty slot's id word is not zero"
        assert not np.any(w1 >> np.uint64(32)) and not np.any(w0 >> np.uint64(33)), "stray bits in an id word"
        flag[at:at + n] = (w0 >> np.uint64(32)) & np.uint64(1)
        full[at:at + n] = ~e1
        for k, w, e in ((k0, w0, e0), (k1, w1, e1)):
            held = np.flatnonzero(~e)
            keys.append(k[held])
            ids.append((w[held] & LOW32).astype(np.int64))
            bucket.append(held + at)
        at += n
    assert at == nb, (at, nb)
    keys = np.concatenate(keys) if keys else np.zeros(0, np.uint64)
    ids = np.concatenate(ids) if ids else np.zeros(0, np.int64)
    bucket = np.concatenate(bucket) if bucket else np.zeros(0, np.int64)
    home = (keys & np.uint64(nb - 1)).astype(np.int64)
    disp = np.flatnonzero(bucket != home)
    hb, dist = home[disp], (bucket[disp] - home[disp]) % nb
    assert np.all(flag[hb]), "a displaced key's home bucket is not flagged"
    assert np.array_equal(np.flatnonzero(flag), np.unique(hb)), "a flag where no displaced key has its home"
    assert not len(dist) or int(dist.max()) <= MAX_PROBE, int(dist.max())
    n_full = np.zeros(nb + 1, np.int64)
    np.cumsum(full, out=n_full[1:])
    end = hb + dist
    between = n_full[np.minimum(end, nb)] - n_full[hb] + np.where(end > nb, n_full[np.maximum(end - nb, 0)], 0)
    assert np.array_equal(between, dist), "a bucket with a free slot between a displaced key and its home"
    return keys, ids, dict(n_displaced=len(disp), n_flagged=int(flag.sum()), longest=int(dist.max()) if len(dist) else 0)


def check_read_side(S, n_emitted, n_reads, n_bases, stats, spectrum_size, novel, hits, keys, ids):
    """S, n_emitted: oracle.read_spectrum of the reads that were fed (n_reads reads, n_bases bases).  From the context:
    stats = reads_stats(), spectrum_size = solve()["spectrum_size"], novel = the list of spectrum_export() (any order),
    hits = the flags of hits_buffer(), (keys, ids) = the read table's pairs.  Returns the number of hit keys."""
    S = np.asarray(S, np.uint64)
    assert np.all(S[1:] > S[:-1]), "the oracle's spectrum is not sorted and duplicate-free"
    assert stats["n_reads"] == n_reads and stats["n_bases"] == n_bases, (stats, n_reads, n_bases)
    assert stats["n_emitted"] == n_emitted, (stats["n_emitted"], n_emitted)
    assert stats["n_distinct"] == spectrum_size == len(S), (stats["n_distinct"], spectrum_size, len(S))
    keys, ids, hits = np.asarray(keys, np.uint64), np.asarray(ids, np.int64), np.asarray(hits)
    nu = len(keys)
    # every key once, ids a permutation of 0 .. nu - 1, one hit flag per id
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    assert np.all(ks[1:] != ks[:-1]), f"a key twice in the table: {_show(ks[1:][ks[1:] == ks[:-1]])}"
    assert nu == len(hits) == len(ids), (nu, len(hits), len(ids))
    assert nu == 0 or (int(ids.min()) >= 0 and int(ids.max()) < nu), "an id outside 0 .. nu - 1"
    seen = np.zeros(nu, bool)
    seen[ids] = True
    assert seen.all(), f"ids are no permutation: {int((~seen).sum())} of {nu} never occur"
    # the novel list: duplicate-free, no walk minimiser, a subset of S
    M = np.sort(np.asarray(novel, np.uint64))
    assert np.all(M[1:] != M[:-1]), f"a hash twice in the novel list: {_show(M[1:][M[1:] == M[:-1]])}"
    in_table = _is_member(ks, M)
    assert not in_table.any(), f"{int(in_table.sum())} novel hashes are keys of the table: {_show(M[in_table])}"
    in_S = _is_member(S, M)
    assert in_S.all(), f"{int((~in_S).sum())} novel hashes outside the oracle's spectrum: {_show(M[~in_S])}"
    # hit keys == S minus M, as sets
    got = ks[hits[ids[order]] != 0]
    want = S[~_is_member(M, S)]
    if not np.array_equal(got, want):
        extra, missing = got[~_is_member(want, got)], want[~_is_member(got, want)]
        raise AssertionError(f"hit keys differ from spectrum minus novel list: {len(got)} against {len(want)}; "
                             f"{len(extra)} flagged outside it {_show(extra)}, {len(missing)} not flagged {_show(missing)}")
    assert len(got) + len(M) == len(S)
    return len(got)


# ------------------------------------------------------------------------------------------------ from a context (GPU)

def table_pieces(ctx, rows=1 << 22):
    """The context's read table as host pieces of at most `rows` buckets, and its bucket count."""
    import torch
    from phi_amd import dist as pdist
    p, nb = ctx.read_table()
    dev = torch.as_tensor(pdist.DevArray(p, nb * 4, "<i8"), device="cuda")

    def pieces():
        for a in range(0, nb, rows):
            b = min(nb, a + rows)
            yield dev[a * 4:b * 4].cpu().numpy().view(np.uint64).reshape(b - a, 4)
    return pieces(), nb


def context_read_side(ctx):
    """(novel list, hit flags) of a context, as host arrays."""
    import torch
    from phi_amd import dist as pdist
    p, m = ctx.spectrum_export()
    novel = torch.as_tensor(pdist.DevArray(p, m, "<i8"), device="cuda").cpu().numpy().view(np.uint64).copy() if m else np.zeros(0, np.uint64)
    p, nu = ctx.hits_buffer()
    hits = torch.as_tensor(pdist.DevArray(p, nu), device="cuda").cpu().numpy().copy() if nu else np.zeros(0, np.uint8)
    return novel, hits


def check_context(ctx, S, n_emitted, n_reads, n_bases, spectrum_size, table=None):
    """check_read_side with everything taken from the context; table = (keys, ids) of an earlier decode of the same
    graph's table (it does not change with the reads).  Returns (keys, ids, number of hit keys)."""
    if table is None:
        pieces, nb = table_pieces(ctx)
        keys, ids, _ = decode_read_table(pieces, nb)
    else:
        keys, ids = table
    novel, hits = context_read_side(ctx)
    n_hit = check_read_side(S, n_emitted, n_reads, n_bases, ctx.reads_stats(), spectrum_size, novel, hits, keys, ids)
    return keys, ids, n_hit
