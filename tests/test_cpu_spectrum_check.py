"""tests/spectrum_check.py on made-up "GPU outputs": what the chromosome-scale GPU tests rely on to fail when a read
kernel or the read table is subtly wrong.  The outputs are built from a small oracle run (walk minimisers -> a read table
laid out by the rules of table.hip, hit flags, novel list); exact outputs pass, and every planted single fault raises."""
import numpy as np
import pytest

import spectrum_check as sc


def _fake_table(uniq, nb):
    """keys uniq[i] with dense id i in nb buckets of two slots: home bucket, else the next bucket with a free slot, the
    home flagged.  (nb, 4) uint64."""
    t = np.zeros((nb, 4), np.uint64)
    t[:, 0] = t[:, 2] = sc.EMPTY
    for i, key in enumerate(uniq.tolist()):
        home = b = key & (nb - 1)
        while t[b, 2] != sc.EMPTY:
            b = (b + 1) & (nb - 1)
        if b != home:
            t[home, 1] |= np.uint64(1 << 32)
        slot = 0 if t[b, 0] == sc.EMPTY else 2
        t[b, slot] = np.uint64(key)
        t[b, slot + 1] |= np.uint64(i)
    return t


@pytest.fixture(scope="module")
def outputs(oracle):
    from phi_amd import synth
    gk, rk = synth.CONFIGS["tiny"]
    g = synth.make_graph(**gk)
    bases, off, _ = synth.make_reads(g, **rk)
    k, w = 31, 25
    S, n_emitted = oracle.read_spectrum([(bases, off)], k, w)
    st = oracle.run_stage12_arrays(g.arrays(), bases, off, k, w, 1.0)
    _, first = np.unique(st.m_hash, return_index=True)
    uniq = st.m_hash[np.sort(first)]                                   # dense ids: first occurrence in walk order
    nb = 1
    while 2 * nb * 0.8 < len(uniq):                                    # a high load: displaced keys and flags
        nb *= 2
    table = _fake_table(uniq, nb)
    hits = np.isin(uniq, S).astype(np.uint8)
    novel = S[~np.isin(S, uniq)]
    rng = np.random.default_rng(9)
    novel = novel[rng.permutation(len(novel))]                         # the device's list is in no order
    assert 0 < hits.sum() < len(uniq) and len(novel) > 10
    stats = dict(n_reads=len(off) - 1, n_bases=int(off[-1]), n_emitted=n_emitted, n_distinct=len(S))
    return dict(S=S, n_emitted=n_emitted, stats=stats, fed=(len(off) - 1, int(off[-1])), novel=novel, hits=hits, table=table, nb=nb, uniq=uniq)


def _run(o, **change):
    d = dict(o, **change)
    pieces = np.array_split(d["table"], 3)                             # decoded in pieces, as the large tables are
    keys, ids, info = sc.decode_read_table(pieces, d["nb"])
    if "keys_ids" in d:
        keys, ids = d["keys_ids"](keys, ids)
    n_hit = sc.check_read_side(d["S"], d["n_emitted"], d["fed"][0], d["fed"][1], d["stats"],
                               d.get("spectrum_size", len(d["S"])), d["novel"], d["hits"], keys, ids)
    return keys, ids, info, n_hit


def test_exact_outputs_pass(outputs):
    keys, ids, info, n_hit = _run(outputs)
    assert np.array_equal(outputs["uniq"][ids], keys)
    assert info["n_displaced"] > 0 and info["n_flagged"] > 0 and info["longest"] >= 1
    assert n_hit == int(outputs["hits"].sum()) == len(outputs["S"]) - len(outputs["novel"])
    sc.decode_read_table([outputs["table"]], outputs["nb"])             # and in one piece


def _foreign(o):
    h = np.uint64(0x0123456789ABCDEF)
    assert h not in o["S"] and h not in o["uniq"]
    return h


FAULTS = ["hit_flag_cleared", "flag_set_outside_S", "hash_dropped_from_novel", "S_hash_duplicated_in_novel",
          "foreign_hash_in_novel", "n_emitted_off_by_one", "two_keys_share_an_id"]


@pytest.mark.parametrize("fault", FAULTS)
def test_single_fault_is_caught(outputs, fault):
    o = outputs
    change = {}
    if fault == "hit_flag_cleared":
        hits = o["hits"].copy()
        hits[np.flatnonzero(hits)[len(hits) // 7]] = 0
        change = dict(hits=hits)
    elif fault == "flag_set_outside_S":
        hits = o["hits"].copy()
        hits[np.flatnonzero(hits == 0)[3]] = 1
        change = dict(hits=hits)
    elif fault == "hash_dropped_from_novel":
        change = dict(novel=np.delete(o["novel"], 5))
    elif fault == "S_hash_duplicated_in_novel":
        change = dict(novel=np.append(o["novel"], o["novel"][2]))
    elif fault == "foreign_hash_in_novel":
        change = dict(novel=np.append(o["novel"], _foreign(o)))
    elif fault == "n_emitted_off_by_one":
        change = dict(stats=dict(o["stats"], n_emitted=o["n_emitted"] + 1))
    elif fault == "two_keys_share_an_id":
        def share(keys, ids):
            ids = ids.copy()
            ids[7] = ids[8]
            return keys, ids
        change = dict(keys_ids=share)
    with pytest.raises(AssertionError):
        _run(o, **change)


def test_more_single_faults_are_caught(outputs):
    """What the issue's list does not name but the helper also promises: counts, a walk minimiser in the novel list, a key
    twice, an S hash that is a hit key swapped into the novel list."""
    o = outputs
    hit_key = o["uniq"][np.flatnonzero(o["hits"])[0]]
    cases = [dict(stats=dict(o["stats"], n_reads=o["stats"]["n_reads"] - 1)),
             dict(stats=dict(o["stats"], n_bases=o["stats"]["n_bases"] + 150)),
             dict(stats=dict(o["stats"], n_distinct=len(o["S"]) + 1)),
             dict(spectrum_size=len(o["S"]) - 1),
             dict(novel=np.append(o["novel"], hit_key)),
             dict(hits=o["hits"][:-1]),
             dict(S=np.delete(o["S"], 11))]
    for change in cases:
        with pytest.raises(AssertionError):
            _run(o, **change)

    def twice(keys, ids):
        keys = keys.copy()
        keys[3] = keys[4]
        return keys, ids
    with pytest.raises(AssertionError):
        _run(o, keys_ids=twice)


def test_table_structure_faults_are_caught(outputs):
    o = outputs
    t0, nb = o["table"], o["nb"]
    flagged = np.flatnonzero((t0[:, 1] >> np.uint64(32)) & np.uint64(1))
    plain = np.flatnonzero(((t0[:, 1] >> np.uint64(32)) & np.uint64(1) == 0) & (t0[:, 0] != sc.EMPTY))
    both = np.flatnonzero(t0[:, 2] != sc.EMPTY)
    home = (t0[:, 0] & np.uint64(nb - 1)).astype(np.int64)
    moved = np.flatnonzero((t0[:, 0] != sc.EMPTY) & (home != np.arange(nb)))

    def broken(edit):
        t = t0.copy()
        edit(t)
        with pytest.raises(AssertionError):
            sc.decode_read_table([t], nb)

    def clear_flag(t):
        t[flagged[0], 1] &= sc.LOW32
    broken(clear_flag)

    def stray_flag(t):
        t[plain[0], 1] |= np.uint64(1 << 32)
    broken(stray_flag)

    def slot1_before_slot0(t):
        b = both[0]
        t[b, 0], t[b, 1] = sc.EMPTY, t[b, 1] & np.uint64(1 << 32)
    broken(slot1_before_slot0)

    def empty_not_zeroed(t):
        b = np.flatnonzero(t[:, 2] == sc.EMPTY)[0]
        t[b, 3] = np.uint64(5)
    broken(empty_not_zeroed)

    def stray_bits(t):
        t[both[0], 3] |= np.uint64(1 << 32)
    broken(stray_bits)

    def gap_in_a_chain(t):
        # a displaced key's home bucket loses its second key: the probe would stop there
        b = moved[0]
        h = int(home[b])
        t[h, 2], t[h, 3] = sc.EMPTY, np.uint64(0)
    broken(gap_in_a_chain)
    with pytest.raises(AssertionError):
        sc.decode_read_table([t0[:-1]], nb)
