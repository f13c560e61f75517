"""CPU tests: the oracle (test infrastructure) against the golden vectors and reference counters.

These pin the checker itself: MurmurHash3 known answers from the reference's own MurmurHash3.cpp,
the counters the reference logged on its own fixtures, the reference parser's view
of its GFA fixtures, the reference's model sizes, and HiGHS objectives of the restated program.
"""
import hashlib
import json
import os

import numpy as np

from conftest import DATA, GOLDEN


def test_murmur_known_answers(oracle):
    vec = json.load(open(os.path.join(GOLDEN, "murmur_vectors.json")))
    assert len(vec) > 100
    for v in vec:
        assert oracle.hash128_to_64(bytes.fromhex(v["hex"])) == int(v["hash"])


def test_murmur_matches_reference_build_when_present(oracle):
    # random bytes of every length 0 .. 69 with what the reference's own MurmurHash3.cpp returned for them
    # (tests/golden/make_golden.py); where oracle/_ref is built, against that build itself as well
    vec = json.load(open(os.path.join(GOLDEN, "murmur_random_vectors.json")))
    rng = np.random.default_rng(3)
    assert len(vec) == 70
    for n, v in enumerate(vec):
        b = bytes(rng.integers(0, 256, size=n, dtype=np.uint8).tolist())
        assert bytes.fromhex(v["hex"]) == b
        assert oracle.hash128_to_64(b) == int(v["hash"])
        if oracle.ref_available():
            assert oracle.ref().ref_hash128_to_64(b, n) == int(v["hash"])


def test_sketch_tiny_by_hand(oracle):
    # k=3, w=2 on ATCGATC: canonical 3-mers ATC,CGA(TCG->CGA),CGA? computed independently below
    seq = b"ATCGATCATACTTACCATG"
    k, w = 3, 2
    comp = bytes.maketrans(b"ACGT", b"TGCA")

    def canon(i):
        f = seq[i:i + k]
        r = f.translate(comp)[::-1]
        return min(f, r)
    prev, out = None, []
    for i in range(w - 1, len(seq) - k + 1):
        win = [(canon(j), j) for j in range(i - w + 1, i + 1)]
        best = min(win, key=lambda t: (t[0], -t[1]))          # smallest k-mer, rightmost on ties
        h = oracle.hash128_to_64(best[0])
        if h != prev:
            out.append((h, best[1]))
            prev = h
    h, p = oracle.sketch(seq, k, w)
    assert list(zip(h.tolist(), p.tolist())) == out


def test_sketch_edge_cases(oracle):
    assert len(oracle.sketch(b"", 31, 25)[0]) == 0
    assert len(oracle.sketch(b"ACGT" * 13 + b"AC", 31, 25)[0]) == 0          # 54 < w+k-1 = 55
    assert len(oracle.sketch(b"ACGT" * 13 + b"ACG", 31, 25)[0]) == 1         # exactly one window
    # case-insensitive, N kept as a byte that sorts between G and T
    a = oracle.sketch(b"acgtnacgtacgtagctagctagcatcgatcg", 5, 3)
    b = oracle.sketch(b"ACGTNACGTACGTAGCTAGCTAGCATCGATCG", 5, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_gfa_restatement_matches_reference_parser(oracle):
    gold = json.load(open(os.path.join(GOLDEN, "gfa_flatten.json")))
    g = oracle.parse_gfa(os.path.join(DATA, "test.gfa"))
    t = gold["test.gfa"]
    assert g.seg_names == t["seg_names"]
    assert [s.decode() for s in g.node_seq] == t["node_seq"]
    assert [sorted(a) for a in g.adj] == t["adj"]
    assert g.paths == t["paths"] and g.hap_names == t["hap_names"]
    g = oracle.parse_gfa(os.path.join(DATA, "MHC_4.gfa.gz"))
    m = gold["MHC_4.gfa.gz"]
    A = g.arrays()
    assert g.n_vtx == m["n_vtx"] and int(A["adj_off"][-1]) == m["n_edges"]
    assert g.hap_names == m["hap_names"] and [len(p) for p in g.paths] == m["walk_len"]
    assert hashlib.sha256(A["seq_concat"]).hexdigest() == m["sha256_seq"]
    assert hashlib.sha256(A["walk_vtx"].tobytes()).hexdigest() == m["sha256_walk_vtx"]
    assert hashlib.sha256(json.dumps([sorted(a) for a in g.adj]).encode()).hexdigest() == m["sha256_adj_sorted"]
    # Kahn order is a valid topological order
    for u, a in enumerate(g.adj):
        for v in a:
            assert g.top_rank[u] < g.top_rank[v]


def test_hap_name_golden(oracle):
    for c in json.load(open(os.path.join(GOLDEN, "hap_names.json"))):
        assert oracle.hap_name(c["gfa"], c["reads"]) == c["name"]


def test_reference_counters_toy(oracle):
    from oracle import solve_oracle as S
    gold = json.load(open(os.path.join(GOLDEN, "counters.json")))["test_gfa_k3_w2"]
    g = oracle.parse_gfa(os.path.join(DATA, "test.gfa"))
    reads = oracle.read_reads(os.path.join(DATA, "read.fa"))
    assert reads == [(b"test_read_1", b"ATCGATCATACTTACCATG")]
    st = oracle.run_stage12(g, reads, 3, 2, 1.0)
    assert st.n_minimizers.tolist() == gold["n_minimizers"]
    assert len(st.spectrum) == gold["spectrum_size"]
    assert st.n_anchors.tolist() == gold["n_anchors"]
    assert st.filtered == gold["filtered"] and st.n_in_model == gold["n_in_model"]
    assert "%.2f/%.2f" % (st.filtered / len(st.spectrum) * 100, st.retained / len(st.spectrum) * 100) == gold["filtered_retained_pct"]
    m = S.Model(g, st, 100)
    n_vars, n_rows = m.model_size()
    n_single = int((st.a_t1 == st.a_t0).sum())       # z_ijk created then skipped (ILP_index.cpp:794-795)
    assert n_vars + n_single == gold["model_vars"] and n_rows == gold["model_lin_rows_ilp"]
    best, arg = m.brute_force()
    val, _, _ = m.milp_solve()
    assert best == val == 4
    for states in arg:
        assert m.objective(states)[0] == best


def test_reference_counters_config1(oracle):
    """test/MHC_4.gfa.gz + test/CHM13_reads.fq.gz: every counter the reference logs."""
    from oracle import solve_oracle as S
    gold = json.load(open(os.path.join(GOLDEN, "counters.json")))["mhc4_chm13_k31_w25"]
    g = oracle.parse_gfa(os.path.join(DATA, "MHC_4.gfa.gz"))
    reads = oracle.read_reads(os.path.join(DATA, "CHM13_reads.fq.gz"))
    assert len(reads) == 16401 and sum(len(s) for _, s in reads) == 2460150
    st = oracle.run_stage12(g, reads, 31, 25, 1.0)
    assert g.hap_names == gold["hap_names"]
    assert st.n_minimizers.tolist() == gold["n_minimizers"]
    assert len(st.spectrum) == gold["spectrum_size"]
    assert st.n_anchors.tolist() == gold["n_anchors"]
    assert st.n_in_model == gold["n_in_model"]
    assert "%.2f/%.2f" % (np.float32(st.filtered) / np.float32(len(st.spectrum)) * 100,
                          np.float32(st.retained) / np.float32(len(st.spectrum)) * 100) == gold["filtered_retained_pct"]
    assert "%.2f" % (st.n_in_model * 100.0 / len(st.spectrum)) == gold["pct_in_model"]
    m = S.Model(g, st, 100)
    n_vars, n_rows = m.model_size()
    assert n_vars + int((st.a_t1 == st.a_t0).sum()) == gold["model_vars"]
    assert n_rows == gold["model_lin_rows_ilp"]


def test_milp_restatement_vs_brute_force_random(oracle):
    from graphgen import mosaic_reads, random_graph
    from oracle import solve_oracle as S
    for seed in range(6):
        rng = np.random.default_rng(100 + seed)
        k, w = int(rng.integers(3, 7)), int(rng.integers(1, 4))
        rep = bytes(rng.choice(list(b"ACGT"), size=k + 3).tolist()) if seed % 2 else None
        g = random_graph(rng, n_sites=4, n_walks=3, repeat=rep)
        reads = mosaic_reads(rng, g, n_reads=20, read_len=k + w + 6)
        R = int(rng.choice([0, 2, 3, 100]))
        st = oracle.run_stage12(g, reads, k, w, 1.0)
        m = S.Model(g, st, R)
        best, _ = m.brute_force()
        val, _, _ = m.milp_solve()
        assert best == val, (seed, best, val)


def test_highs_golden_tiny_is_reproducible(oracle):
    """The committed HiGHS objectives can be regenerated (tiny cases only: seconds)."""
    from oracle import solve_oracle as S
    from phi_amd import synth
    gold = [c for c in json.load(open(os.path.join(GOLDEN, "solve_golden.json"))) if c["config"] == "tiny"]
    assert gold
    gk, rk = synth.CONFIGS["tiny"]
    g = synth.make_graph(**gk)
    bases, off, _ = synth.make_reads(g, **rk)
    G = oracle.Graph(seg_names=[str(i) for i in range(g.n_vtx)],
                     node_seq=[bytes(g.seq_concat[g.seq_off[v]:g.seq_off[v + 1]]) for v in range(g.n_vtx)],
                     adj=[g.adj[g.adj_off[v]:g.adj_off[v + 1]].tolist() for v in range(g.n_vtx)],
                     paths=[g.walk_vtx[g.walk_off[h]:g.walk_off[h + 1]].tolist() for h in range(g.n_walks)],
                     hap_names=g.hap_names)
    oracle.kahn(G)
    reads = [bytes(bases[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    st = oracle.run_stage12(G, reads, 31, 25, 1.0)
    for c in gold[:1]:
        val, _, _ = S.Model(G, st, c["R"]).milp_solve()
        assert val == c["objective"] and len(st.spectrum) == c["spectrum_size"]


def _spectrum_cases():
    """(name, graph arrays, bases, offsets): the generator's tiny and small read sets, and a set with lower case and with
    bases outside ACGTacgt (reads of several lengths, some shorter than one window, one empty)."""
    from phi_amd import synth
    for name in ("tiny", "small"):
        gk, rk = synth.CONFIGS[name]
        g = synth.make_graph(**gk)
        bases, off, _ = synth.make_reads(g, **rk)
        yield name, g.arrays(), bases, off
    gk, rk = synth.CONFIGS["tiny"]
    g = synth.make_graph(**gk)
    bases, off, _ = synth.make_reads(g, **dict(rk, seed=77))
    rng = np.random.default_rng(78)
    bases = bases.copy()
    low = rng.random(len(off) - 1) < 0.3
    for r in np.flatnonzero(low):
        bases[off[r]:off[r + 1]] |= 0x20                               # a whole read in lower case
    odd = rng.integers(0, len(bases), size=len(bases) // 200)
    bases[odd] = rng.choice(np.frombuffer(b"NnxRY-*.", np.uint8), size=len(odd))
    extra = [b"", b"ACGT" * 13 + b"AC", b"acgtn" * 11, bytes(rng.choice(list(b"ACGTacgtN"), size=333).tolist())]
    lens = np.r_[np.diff(off), [len(e) for e in extra]]
    off2 = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off2[1:])
    yield "mixed", g.arrays(), np.concatenate([bases, np.frombuffer(b"".join(extra), np.uint8)]), off2


def test_read_spectrum_in_batches_equals_the_full_run(oracle):
    """oracle.read_spectrum (stage 1b alone, through the accumulator) against the spectrum orc_run builds inside a full
    run, in one batch, in three and in three reversed; against the union of oracle.sketch over the reads as a Python set;
    the emitted count against orc_sketch_reads."""
    k, w = 31, 25
    for name, A, bases, off in _spectrum_cases():
        want = oracle.run_stage12_arrays(A, bases, off, k, w, 1.0, want_minimizers=False).spectrum
        assert len(want) > 100 and np.all(want[1:] > want[:-1])
        n = len(off) - 1
        cuts = [0, n // 3, 2 * n // 3, n]
        parts = [(bases[off[a]:off[b]], off[a:b + 1] - off[a]) for a, b in zip(cuts[:-1], cuts[1:])]
        emitted = oracle.sketch_reads_count(bases, off, k, w)
        assert emitted > len(want)
        for label, batches in (("one", [(bases, off)]), ("three", parts), ("reversed", parts[::-1])):
            got, n_emitted = oracle.read_spectrum(batches, k, w)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (name, label)
            assert n_emitted == emitted, (name, label)
        raw = bases.tobytes()
        as_set = set()
        for r in range(n):
            as_set.update(oracle.sketch(raw[off[r]:off[r + 1]], k, w)[0].tolist())
        assert as_set == set(want.tolist()), name
    # bytes in place of arrays, no reads at all, and a batch large enough for the partitioned sort
    got, n_emitted = oracle.read_spectrum([(raw, off)], k, w)
    assert np.array_equal(got, want) and n_emitted == emitted
    got, n_emitted = oracle.read_spectrum([], k, w)
    assert len(got) == 0 and n_emitted == 0
    got, n_emitted = oracle.read_spectrum([(b"", np.zeros(1, np.int64))], k, w)
    assert len(got) == 0 and n_emitted == 0


def test_read_spectrum_partitioned_sort(oracle):
    """A batch above the size where the accumulator sorts by ranges of the hash's top bits (65 536 emitted hashes), with
    many repeats, against numpy's sort."""
    rng = np.random.default_rng(5)
    k, w = 15, 4
    hap = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=40_000)
    starts = rng.integers(0, len(hap) - 200, size=4000)
    bases = np.concatenate([hap[s:s + 200] for s in starts])
    off = np.arange(len(starts) + 1, dtype=np.int64) * 200
    raw = bases.tobytes()
    every = np.concatenate([oracle.sketch(raw[off[r]:off[r + 1]], k, w)[0] for r in range(len(starts))])
    assert len(every) > (1 << 16) and len(np.unique(every)) < len(every) // 4
    before = oracle.lib().orc_max_threads()
    for threads in (1, 3, before):
        got, n_emitted = oracle.read_spectrum([(bases, off)], k, w, threads=threads)
        assert n_emitted == len(every) and np.array_equal(got, np.unique(every))
    assert oracle.lib().orc_max_threads() == before
    got, _ = oracle.read_spectrum([(bases[:off[2000]], off[:2001]), (bases[off[2000]:], off[2000:] - off[2000])], k, w)
    assert np.array_equal(got, np.unique(every))
