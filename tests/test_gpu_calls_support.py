"""The read support of every call (phi_calls_support, calls_support.hip) against the plain-Python restatement of the rule in
tests/calls_support_ref.py: all four arrays and their totals, exactly.  The occurrences the reference counts come from the CPU
oracle's sketch of the walk sequences, the read spectrum from its sketch of the upper-cased reads."""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import calls_support_ref as R
from conftest import DATA, ROOT
from graphgen import mosaic_reads, random_graph, walk_sequence
from test_cpu_chop import chop_numpy
from test_gpu_calls import _hand_graph, _set

pytestmark = pytest.mark.gpu

NAMES = ("alt_hit", "alt_n", "ref_hit", "ref_n")
K, W = 5, 2


def _same(got, want, n_calls):
    assert got["n_calls"] == n_calls and got["gpu_ms"] >= 0
    for n in NAMES:
        assert got[n].dtype == np.int32 and np.array_equal(got[n], want[n]), (n, got[n].tolist(), want[n].tolist())
        assert got[n + "_total"] == want[n + "_total"], n


def _check_walks(oracle, ctx, g, q, r, k, w, spectrum):
    c = ctx.calls(r, walk=q)
    got = ctx.calls_support()
    _same(got, R.walk_support_ref(oracle, g, q, r, k, w, spectrum), c["n_calls"])
    return c, got


# ------------------------------------------------------------------ 1. random graphs, every ordered pair of walks

def _one_random_case(oracle, ctx_factory, pi, seed):
    g, reads, k, w = R.random_case(pi, seed)
    ctx = ctx_factory(k=k, w=w, threshold=1.0, recombination=3)
    _set(ctx, g)
    ctx.add_reads(reads)
    spectrum = R.spectrum_of(oracle, reads, k, w)
    lens = [len(s) for s in g.node_seq]
    n_empty_alt = n_between = 0
    for q in range(4):
        for r in range(4):
            c, got = _check_walks(oracle, ctx, g, q, r, k, w, spectrum)
            qb = R.walk_bases(g.paths[q], lens)
            for j, (i, i2, _, _) in enumerate(R.anchors(g.paths[q], g.paths[r])):
                n_empty_alt += qb[i + 1] == qb[i2] and got["alt_n"][j] > 0
                n_between += 0 < got["alt_hit"][j] < got["alt_n"][j]
    ctx.close()
    return n_empty_alt, n_between


@pytest.mark.parametrize("pi", range(len(R.PARAMS)))
def test_random_graphs_every_ordered_pair(oracle, ctx_factory, pi):
    """(k, w) = (5, 2) on vertices longer than k, (9, 4) on vertices of 1 to 400 bases, (5, 8) on vertices of 1 to 3 bases: there
    a window starts several entries before the entry its minimiser lies in, and the walk back meets the walk's first entry.
    Over the seeds some deletion is witnessed by the k-mers that span it, and some allele is seen in part
    (tests/test_cpu_calls_support_host.py checks on the CPU that these seeds give both)."""
    n_empty_alt = n_between = 0
    for seed in R.SEEDS:
        a, b = _one_random_case(oracle, ctx_factory, pi, seed)
        n_empty_alt += a
        n_between += b
    assert n_empty_alt > 0 and n_between > 0


# ------------------------------------------------------------------ 2. hand graphs, the values written out

def _hand(oracle, ctx, node_seq, edges, paths, reads):
    g = _hand_graph(node_seq, edges, paths)
    _set(ctx, g)
    if reads:
        ctx.add_reads(reads)
    return g, R.spectrum_of(oracle, reads, K, W)


def _values(got):
    return tuple(got[n].tolist() for n in NAMES)


def test_hand_graphs(oracle, ctx_factory):
    ctx = ctx_factory(k=K, w=W, threshold=1.0, recombination=3)
    # 0 -> 1 ("G", one base, shared) -> [2, an insertion] -> 3; the reads are the longer walk.
    #   walk 1 = ACGTACGAG TTT CAGTCATC, minimisers at 0 2 4 6 7 8 10 11 13 14; ALT = [9, 12): those at 6 .. 11
    #   walk 0 = ACGTACGAG CAGTCATC, minimisers at 0 2 4 5 7 8 10 11; REF is empty at 9: the k-mers at 5, 7, 8 span the junction,
    #   and the reads hold none of them
    g, spec = _hand(oracle, ctx, [b"ACGTACGA", b"G", b"TTT", b"CAGTCATC"], [(0, 1), (1, 2), (1, 3), (2, 3)], [[0, 1, 3], [0, 1, 2, 3]],
                    [b"ACGTACGAGTTTCAGTCATC"])
    _, ins = _check_walks(oracle, ctx, g, 1, 0, K, W, spec)
    assert _values(ins) == ([5], [5], [0], [3])
    _, dele = _check_walks(oracle, ctx, g, 0, 1, K, W, spec)      # the mirror: a deletion, witnessed by the k-mers that span it
    assert _values(dele) == ([0], [3], [5], [5])
    # two adjacent bubbles, 0 -> (1 | 2) -> (3 | 4) -> 5; the reads are walk 1 = ACGTACGA CC t CAGTCATC (minimisers at
    # 0 2 4 6 7 8 10 12 13, ALT = [8, 11): 4 .. 10); walk 0 = ACGTACGA a GGG CAGTCATC (0 2 4 6 7 8 10 11 13 14, REF = [8, 12): 4 .. 11)
    ctx.reset_reads()
    g, spec = _hand(oracle, ctx, [b"ACGTACGA", b"a", b"CC", b"GGG", b"t", b"CAGTCATC"],
                    [(0, 1), (0, 2), (1, 3), (1, 4), (2, 3), (2, 4), (3, 5), (4, 5)], [[0, 1, 3, 5], [0, 2, 4, 5], [0, 1, 4, 5], [0, 2, 3, 5]],
                    [b"ACGTACGACCTCAGTCATC"])
    _, both = _check_walks(oracle, ctx, g, 1, 0, K, W, spec)
    assert _values(both) == ([5], [5], [0], [6])
    _, mixed = _check_walks(oracle, ctx, g, 2, 3, K, W, spec)
    assert _values(mixed) == ([1], [4], [1], [7])
    for q in range(4):
        for r in range(4):
            _check_walks(oracle, ctx, g, q, r, K, W, spec)
    # A0 - k lies before the walk's first base: walk 1 = AC TT CAGTCATCGGA, minimisers at 0 2 3 5 6 8 9, ALT = [2, 4): 0, 2, 3
    ctx.reset_reads()
    g, spec = _hand(oracle, ctx, [b"AC", b"G", b"TT", b"CAGTCATCGGA"], [(0, 1), (0, 2), (1, 3), (2, 3)], [[0, 1, 3], [0, 2, 3]], [b"ACTTCAGTCATCGGA"])
    _, early = _check_walks(oracle, ctx, g, 1, 0, K, W, spec)
    assert _values(early) == ([3], [3], [0], [2])
    # walks of 3 and 4 bases, shorter than w + k - 1 = 6: no occurrence, 0 of 0 on both sides; the third walk gives the
    # graph its minimisers, one of which (the k-mer at 0 of ACTCA...) spans the junction of the deletion
    ctx.reset_reads()
    g, spec = _hand(oracle, ctx, [b"A", b"C", b"GG", b"T", b"CAGTCATCGGATTACAGGCA"], [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4)],
                    [[0, 1, 3], [0, 2, 3], [0, 1, 3, 4]], [b"ACTCAGTCATCGGATTACAGGCA"])
    for q, r in ((1, 0), (0, 1)):
        c, short = _check_walks(oracle, ctx, g, q, r, K, W, spec)
        assert c["n_calls"] == 1 and _values(short) == ([0], [0], [0], [0])
    _, long_ref = _check_walks(oracle, ctx, g, 1, 2, K, W, spec)
    assert _values(long_ref) == ([0], [0], [1], [1])
    ctx.close()


# ------------------------------------------------------------------ 3. two properties

@pytest.mark.parametrize("pi", range(len(R.PARAMS)))
def test_no_reads_and_the_walk_itself_as_the_read(oracle, ctx_factory, pi):
    g, _, k, w = R.random_case(pi, 5)
    ctx = ctx_factory(k=k, w=w, threshold=1.0, recombination=3)
    _set(ctx, g)
    for q in range(4):                                     # no reads: nothing is seen, the witnesses are the reference's
        for r in range(4):
            _, got = _check_walks(oracle, ctx, g, q, r, k, w, set())
            assert not got["alt_hit"].any() and not got["ref_hit"].any()
    for q in range(4):                                     # the query walk's own sequence as the only read: every ALT witness is seen
        ctx.reset_reads()
        ctx.add_reads([walk_sequence(g, q)])
        spec = R.spectrum_of(oracle, [walk_sequence(g, q)], k, w)
        for r in range(4):
            _, got = _check_walks(oracle, ctx, g, q, r, k, w, spec)
            assert np.array_equal(got["alt_hit"], got["alt_n"])
    ctx.close()


# ------------------------------------------------------------------ 4. the path

def test_support_of_the_path(oracle, ctx_factory):
    """Set up as test_gpu_calls.py's test_calls_of_the_path.  Query index j sits on walk path_hap[j] at the entry that holds
    path_vtx[j]; in some seed the path switches walks inside a call or within k bases of one."""
    k, w = 9, 4
    n_switch_at_a_call = 0
    for seed in range(1, 9):
        rng = np.random.default_rng(100 * seed + 11)
        g = random_graph(rng, n_sites=12, n_walks=4, seg_len=(1, 400), alt_len=(1, 40), p_del=0.3)
        reads = mosaic_reads(rng, g, n_reads=60, read_len=70, n_seg=2, err=0.01)
        ctx = ctx_factory(k=k, w=w, threshold=1.0, recombination=3)
        _set(ctx, g)
        ctx.add_reads(reads)
        res = ctx.solve()
        spectrum = R.spectrum_of(oracle, reads, k, w)
        path, hap = res["path_vtx"].tolist(), res["path_hap"].tolist()
        lens = [len(s) for s in g.node_seq]
        qb = R.walk_bases(path, lens)
        switches = [int(qb[j]) for j in range(1, len(path)) if hap[j] != hap[j - 1]]
        for r in range(g.n_walks):
            c = ctx.calls(r)
            _same(ctx.calls_support(), R.path_support_ref(oracle, g, path, hap, r, k, w, spectrum), c["n_calls"])
            for i, i2, _, _ in R.anchors(path, g.paths[r]):
                n_switch_at_a_call += any(qb[i + 1] - k <= s <= qb[i2] + k for s in switches)
        ctx.close()
    assert n_switch_at_a_call > 0


# ------------------------------------------------------------------ 5. borders

@pytest.mark.parametrize("n_sites", [1500, 5000])
def test_items_beyond_a_workgroup_and_the_scan_tile(oracle, ctx_factory, n_sites):
    rng = np.random.default_rng(n_sites)
    g = random_graph(rng, n_sites=n_sites, n_walks=3, seg_len=(1, 9), p_del=0.3)
    reads = mosaic_reads(rng, g, n_reads=200, read_len=60, n_seg=2, err=0.0)
    ctx = ctx_factory(k=K, w=W, threshold=1.0, recombination=3)
    _set(ctx, g)
    ctx.add_reads(reads)
    spectrum = np.array(sorted(R.spectrum_of(oracle, reads, K, W)), np.uint64)
    lens = [len(s) for s in g.node_seq]
    sk = [oracle.sketch(walk_sequence(g, h), K, W) for h in range(3)]
    base = [R.walk_bases(g.paths[h], lens) for h in range(3)]
    for q, r in ((0, 1), (1, 0), (2, 1)):
        c = ctx.calls(r, walk=q)
        got = ctx.calls_support()
        want = R.support_ref_numpy(K, sk[q][0], sk[q][1], base[q], sk[r][0], sk[r][1], base[r], R.anchors(g.paths[q], g.paths[r]), spectrum)
        _same(got, want, c["n_calls"])
        st = ctx.calls_support_stats()
        assert got["n_items"] == st["n_items"] > 2 * c["n_calls"] > n_sites // 4 and got["alt_hit_total"] > 0
        assert st["n_witnesses"] == got["alt_n_total"] + got["ref_n_total"] and st["n_visited"] >= st["n_items"] and st["bytes_moved"] > 0
    ctx.close()


def test_an_allele_of_many_pieces_beside_one_base_alleles(oracle, ctx_factory):
    """test_gpu_calls.py's 10 000-base insertion on a graph set with chop=25 -- 400 target entries for one (call, side) -- with
    one-base alleles of a second bubble behind it: items of one call fill whole workgroups beside calls of one item."""
    rng = np.random.default_rng(25)
    big = bytes(rng.choice(list(b"ACGT"), size=10000).tolist())
    g = _hand_graph([b"ACGTACGTAC", big, b"TTGACCGATA", b"A", b"C", b"GATTACAGGCATTC"], [(0, 1), (0, 2), (1, 2), (2, 3), (2, 4), (3, 5), (4, 5)],
                    [[0, 2, 3, 5], [0, 1, 2, 4, 5]])
    c, _, _ = chop_numpy(g, 25)
    reads = [big[100:400], big[5000:5200], b"TTGACCGATACGATTACAGGCATTC"]
    ctx = ctx_factory(k=K, w=W, threshold=1.0, recombination=3)
    _set(ctx, g, chop=25)
    ctx.add_reads(reads)
    spec = R.spectrum_of(oracle, reads, K, W)
    for q, r in ((1, 0), (0, 1)):
        cl, got = _check_walks(oracle, ctx, c, q, r, K, W, spec)
        assert cl["n_calls"] == 2 and got["n_items"] > 400
        side = "alt" if q == 1 else "ref"
        assert 0 < got[side + "_hit"][0] < got[side + "_n"][0] and got[side + "_n"][0] > 2000
    ctx.close()


# ------------------------------------------------------------------ 6. MHC_4

@pytest.fixture(scope="module")
def mhc(oracle, ctx_factory):
    from phi_amd import ilp_index as H
    g = H.Graph(os.path.join(DATA, "MHC_4.gfa.gz"))
    ctx = ctx_factory(k=31, w=25, threshold=1.0, recombination=100)
    ctx.set_graph(g.seq_concat, g.seq_off, g.adj_off, g.adj, g.walk_off, g.walk_vtx, g.top_order_map)
    bases, off, _ = H.read_reads(os.path.join(DATA, "CHM13_reads.fq.gz"))
    ctx.add_reads((bases, off))
    raw = bases.tobytes().upper()
    spectrum = set()
    for i in range(len(off) - 1):
        spectrum.update(oracle.sketch(raw[off[i]:off[i + 1]], 31, 25)[0].tolist())
    return dict(ctx=ctx, g=g, names=list(g.hap_id2name), spectrum=np.array(sorted(spectrum), np.uint64))


def _mhc_walk(oracle, g, h):
    wv = np.asarray(g.walk_vtx[g.walk_off[h]:g.walk_off[h + 1]])
    vlen = np.diff(g.seq_off)
    base = np.concatenate([[0], np.cumsum(vlen[wv])]).astype(np.int64)
    flat = np.frombuffer(bytes(g.seq_concat), np.uint8)
    seq = flat[np.repeat(g.seq_off[wv] - base[:-1], vlen[wv]) + np.arange(base[-1])].tobytes()
    return wv, base, oracle.sketch(seq, 31, 25)


def _digest(s):
    return b"".join(np.ascontiguousarray(s[n]).tobytes() for n in NAMES)


@pytest.mark.parametrize("ref_name", ["CHM13.0", "HG002.1"])
def test_mhc_a_walk_against_a_reference_walk(oracle, mhc, ref_name):
    g, ctx = mhc["g"], mhc["ctx"]
    r = mhc["names"].index(ref_name)
    q = next(h for h in range(len(mhc["names"])) if h != r and mhc["names"][h] not in ("CHM13.0", "HG002.1"))
    qv, qb, qs = _mhc_walk(oracle, g, q)
    rv, rb, rs = _mhc_walk(oracle, g, r)
    c = ctx.calls(r, walk=q)
    got = ctx.calls_support()
    want = R.support_ref_numpy(31, qs[0], qs[1], qb, rs[0], rs[1], rb, R.anchors(qv.tolist(), rv.tolist()), mhc["spectrum"])
    _same(got, want, c["n_calls"])
    assert c["n_calls"] > 10000 and got["n_items"] > 2 * c["n_calls"] and 0 < got["ref_hit_total"] < got["ref_n_total"]
    ctx.calls(r, walk=q)                                   # twice: the same bytes
    assert _digest(ctx.calls_support()) == _digest(got)


def test_mhc_support_on_dirty_device_memory(mhc):
    """Every device buffer poisoned and handed back from the pool with an earlier owner's contents, set up as
    test_gpu_calls.py's test_mhc_calls_on_dirty_device_memory: the same counts as on clean memory."""
    from test_gpu_dirty_memory import VARIANTS
    ctx = mhc["ctx"]
    ctx.calls(0, walk=3)
    want = _digest(ctx.calls_support()).hex()
    env = {k: v for k, v in os.environ.items() if k not in ("PHI_DEVICE_POISON", "PHI_DEVICE_POOL_MIN", "PHI_DEVICE_POOL")}
    env.update(VARIANTS["ff"])
    env.update(VARIANTS["pooled"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "calls_support_child.py"), "3", "0"], capture_output=True, text=True, timeout=240,
                       cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-300:] + r.stderr)[-3000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["digest"] == want


# ------------------------------------------------------------------ 7. state and refusals

def test_state_and_refusals(oracle, ctx_factory):
    from phi_amd import PHI_ERR_STATE, PhiError
    g, reads, k, w = R.random_case(0, 3)
    ctx = ctx_factory(k=k, w=w, threshold=1.0, recombination=3)
    _set(ctx, g)
    ctx.add_reads(reads)
    spec = R.spectrum_of(oracle, reads, k, w)
    for call in (ctx.calls_support, ctx.calls_support_stats):    # no calls yet
        with pytest.raises(PhiError) as e:
            call()
        assert e.value.status == PHI_ERR_STATE
    _check_walks(oracle, ctx, g, 1, 0, k, w, spec)
    assert ctx.calls_support_stats()["n_calls"] == ctx.calls_stats()["n_calls"]
    ctx.solve()                                            # the solve invalidates the calls, and their support with them
    with pytest.raises(PhiError) as e:
        ctx.calls_support()
    assert e.value.status == PHI_ERR_STATE and "phi_calls" in e.value.detail
    _check_walks(oracle, ctx, g, 2, 1, k, w, spec)         # after the refusal the context works as before
    _set(ctx, g)                                           # a new graph: the calls are gone
    with pytest.raises(PhiError) as e:
        ctx.calls_support()
    assert e.value.status == PHI_ERR_STATE
    _check_walks(oracle, ctx, g, 3, 0, k, w, set())        # (the new graph has no reads yet)
    ctx.close()


# ------------------------------------------------------------------ 8. the command line

SUPPORT_LINE = re.compile(r"Call support: (\d+) calls, (\d+) of (\d+) ALT and (\d+) of (\d+) REF witness minimisers seen")


def test_cli_calls_support(tmp_path):
    import phi_amd
    from phi_amd import ilp_index as H
    from phi_amd.calls import read_support, read_vcf
    from test_gpu_chop import _run_cli
    gfa, rd = os.path.join(DATA, "test.gfa"), os.path.join(DATA, "read.fa")
    base = ["-g", gfa, "-r", rd, "-k", "3", "-w", "2"]
    vcf, vcfz, plain = tmp_path / "x.vcf", tmp_path / "x.vcf.gz", tmp_path / "p.vcf"
    r = _run_cli(base + ["-o", str(tmp_path / "x.fa"), "--calls", str(vcf), "--calls-ref", "test_hap_1.0", "--calls-support"], tmp_path, env={"PHI_TIMING": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    m = SUPPORT_LINE.search(r.stderr)
    assert m and re.search(r"stage calls support \(device\)", r.stderr), r.stderr[-3000:]
    # the same calls from Python
    G = H.Graph(gfa)
    ctx = phi_amd.Context(0)
    ctx.set_params(k=3, w=2, threshold=1.0, recombination=100)
    ctx.set_graph(G.seq_concat, G.seq_off, G.adj_off, G.adj, G.walk_off, G.walk_vtx, G.top_order_map)
    bases, off, _ = H.read_reads(rd)
    ctx.add_reads((bases, off))
    ctx.solve()
    c = ctx.calls(list(G.hap_id2name).index("test_hap_1.0"))
    sup = ctx.calls_support()
    ctx.close()
    assert [int(x) for x in m.groups()] == [c["n_calls"]] + [sup[n + "_total"] for n in NAMES]
    ro, ao = c["ref_off"], c["alt_off"]
    kept = np.array([c["ref_bytes"][ro[j]:ro[j + 1]] != c["alt_bytes"][ao[j]:ao[j + 1]] for j in range(c["n_calls"])], bool)
    got = read_support(str(vcf))
    assert c["n_calls"] > 0 and len(got["alt_n"]) == kept.sum() == len(read_vcf(str(vcf))[2]["pos"])
    for n in NAMES:
        assert np.array_equal(got[n], sup[n][kept]), n
    # without the flag: the same file minus the two header lines and the two columns
    r = _run_cli(base + ["-o", str(tmp_path / "p.fa"), "--calls", str(plain), "--calls-ref", "test_hap_1.0"], tmp_path)
    assert r.returncode == 0 and "Call support" not in r.stderr
    stripped = [re.sub(r"\tGT:AK:RK\t1:\S+$", "\tGT\t1", ln) for ln in vcf.read_text().split("\n") if not ln.startswith(("##FORMAT=<ID=AK", "##FORMAT=<ID=RK"))]
    assert "\n".join(stripped) == plain.read_text() != vcf.read_text()
    # --bgzf: the inflated file has the same text
    r = _run_cli(["--bgzf"] + base + ["-o", str(tmp_path / "x.fa.gz"), "--calls", str(vcfz), "--calls-ref", "test_hap_1.0", "--calls-support"], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    assert gzip.decompress(vcfz.read_bytes()) == vcf.read_bytes() and SUPPORT_LINE.search(r.stderr).groups() == m.groups()
    # --calls-support alone is refused before any work
    r = _run_cli(base + ["-o", str(tmp_path / "n.fa"), "--calls-support"], tmp_path)
    assert r.returncode != 0 and "--calls-support goes with --calls" in r.stderr and not (tmp_path / "n.fa").exists()
    assert "Graph has" not in r.stderr
