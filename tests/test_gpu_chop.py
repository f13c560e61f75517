"""Chopping inside "set graph" (phi_set_graph_chopped: data/chop_graph.sh:3 `hal2vg --chop 30` done by the library, the walk
entries expanded on the device by phi_amd/csrc/chop.hip) against the rule restated in numpy (test_cpu_chop.chop_numpy) and,
through it, against the CPU oracle on the chopped graph."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT
from graphgen import mosaic_reads, random_graph
from test_cpu_chop import chop_numpy
from test_gpu_parity import _check_against_oracle

pytestmark = pytest.mark.gpu

PHI = os.path.join(ROOT, "phi_amd", "PHI")
SOLVE_KEYS = ("objective", "upper_bound", "optimal", "n_dp_runs", "n_covered", "n_path", "recombination_count", "n_switches", "hap_len",
              "n_walks", "spectrum_size", "filtered", "retained", "n_in_model")


def _set(ctx, g, chop=None):
    A = g.arrays()
    return ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"], chop=chop)


def _same_run(a, b, n_walks, res_a=None):
    """contexts a and b hold the same index and give the same solve, element for element; returns b's result"""
    assert np.array_equal(a.walk_entries(), b.walk_entries())
    for h in range(n_walks):
        (ha, pa), (hb, pb) = a.walk_minimizers(h), b.walk_minimizers(h)
        assert np.array_equal(ha, hb) and np.array_equal(pa, pb), h
    ra = res_a if res_a is not None else a.solve()
    rb = b.solve()
    for key in SOLVE_KEYS:
        assert ra[key] == rb[key], key
    for key in ("path_vtx", "path_hap", "n_minimizers", "n_anchors"):
        assert np.array_equal(ra[key], rb[key]), key
    for x, y in zip(a.kept_anchors(), b.kept_anchors()):
        assert np.array_equal(x, y)
    assert a.path_sequence(ra["hap_len"]) == b.path_sequence(rb["hap_len"])
    return rb


def _dirty(rng, g):
    """lower case and N inside some segments"""
    for v in rng.choice(g.n_vtx, size=max(2, g.n_vtx // 5), replace=False).tolist():
        s = bytearray(g.node_seq[v])
        if len(s) > 3 and v % 2:
            s[len(s) // 2] = ord("N")
            g.node_seq[v] = bytes(s)
        else:
            g.node_seq[v] = bytes(s).lower()


def _write_gfa(g, path):
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "wt") as f:
        f.write("H\tVN:Z:1.1\n")
        for i, s in enumerate(g.node_seq):
            f.write(f"S\ts{i + 1}\t{s.decode()}\n")
        for u, a in enumerate(g.adj):
            for v in a:
                f.write(f"L\ts{u + 1}\t+\ts{v + 1}\t+\t0M\n")
        for h, p in enumerate(g.paths):
            smp, hap = g.hap_names[h].rsplit(".", 1)
            f.write(f"W\t{smp}\t{hap}\tchr\t0\t1\t" + "".join(f">s{v + 1}" for v in p) + "\n")
    return str(path)


# 3 .. 70 walks: up to 64 the blocks' rows run on walk lanes, beyond on class lanes
GRAPHS = [(1, 3, 4), (2, 9, 6), (3, 70, 5)]


def _graph_and_reads(seed, n_walks, n_sites):
    """long segments, deletions, lower case and N in segments; reads of a two-segment mosaic"""
    rng = np.random.default_rng(100 * seed + 7)
    g = random_graph(rng, n_sites=n_sites, n_walks=n_walks, seg_len=(1, 400), alt_len=(1, 40), p_del=0.3)
    _dirty(rng, g)
    return g, mosaic_reads(rng, g, n_reads=60, read_len=70, n_seg=2, err=0.01)


@pytest.mark.parametrize("seed,n_walks,n_sites", GRAPHS)
@pytest.mark.parametrize("N", [1, 7, 30, 64, 10000])
def test_chop_equals_setting_the_chopped_graph(oracle, ctx_factory, seed, n_walks, n_sites, N):
    g, reads = _graph_and_reads(seed, n_walks, n_sites)
    k, w, T, R = 9, 4, 1.0, 3
    c, ov, oo = chop_numpy(g, N)
    a = ctx_factory(k=k, w=w, threshold=T, recombination=R)
    _set(a, c)
    a.add_reads(reads)
    # the yardstick: the oracle on the chopped graph
    st, res_a, m = _check_against_oracle(oracle, a, c, reads, k, w, T, R)
    if n_walks <= 3:
        assert res_a["objective"] == m.brute_force()[0]
    b = ctx_factory(k=k, w=w, threshold=T, recombination=R)
    woff = _set(b, g, chop=N)
    assert np.array_equal(woff, c.arrays()["walk_off"])
    b.add_reads(reads)
    rb = _same_run(a, b, n_walks, res_a)
    got_v, got_o = b.chop_origin(rb["path_vtx"])
    assert np.array_equal(got_v, ov[rb["path_vtx"]]) and np.array_equal(got_o, oo[rb["path_vtx"]])
    cs = b.chop_stats()
    assert (cs["n_vtx_in"], cs["n_vtx_out"], cs["max_len"]) == (g.n_vtx, c.n_vtx, N)
    assert (cs["n_entries_in"], cs["n_entries_out"]) == (sum(len(p) for p in g.paths), sum(len(p) for p in c.paths))


def test_chopping_is_what_brings_the_anchors_into_the_model(oracle, ctx_factory):
    """Segments of 200 .. 600 bases at k = 31: unchopped, most minimisers lie inside one vertex and drop out of the model;
    chopped to 30 every 31-mer spans two vertices or more.  Orderings, not thresholds."""
    rng = np.random.default_rng(31)
    g = random_graph(rng, n_sites=8, n_walks=5, seg_len=(200, 600), alt_len=(1, 40), p_del=0.2)
    reads = mosaic_reads(rng, g, n_reads=300, read_len=150, n_seg=2, err=0.0)
    k, w, T, R = 31, 25, 1.0, 100
    plain = ctx_factory(k=k, w=w, threshold=T, recombination=R)
    _set(plain, g)
    plain.add_reads(reads)
    r0 = plain.solve()
    ch = ctx_factory(k=k, w=w, threshold=T, recombination=R)
    _set(ch, g, chop=30)
    ch.add_reads(reads)
    r1 = ch.solve()
    _, _, t0, t1 = ch.kept_anchors()
    assert len(t0) > 0 and np.all(t1 > t0)
    c, _, _ = chop_numpy(g, 30)
    st = oracle.run_stage12(c, reads, k, w, T)
    assert r1["n_in_model"] == st.n_in_model
    assert r1["n_in_model"] > r0["n_in_model"]
    assert r1["objective"] >= r0["objective"]


@pytest.mark.parametrize("seed,n_walks,n_sites", GRAPHS)
@pytest.mark.parametrize("N", [1, 7, 30, 64, 10000])
def test_chop_of_walks_resolved_on_the_device(oracle, ctx_factory, tmp_path, seed, n_walks, n_sites, N):
    """The graphs of test_chop_equals_setting_the_chopped_graph written as W-line text -> phi_walk_text_upload / _resolve ->
    set_graph(walk_vtx=None, chop=N): the entries are expanded where they lie.  Equal, element for element, to context A of
    that test -- chop_numpy's graph through plain set_graph, itself held against the oracle --, with the topological ranks
    the GFA reader gives the file."""
    from phi_amd import ilp_index as H
    g, reads = _graph_and_reads(seed, n_walks, n_sites)
    k, w, T, R = 9, 4, 1.0, 3
    path = _write_gfa(g, tmp_path / "long.gfa")
    b = ctx_factory(k=k, w=w, threshold=T, recombination=R)
    dg = H.DeferredGraph(path)
    assert dg.resolve_on_device(b) and dg.walk_vtx is None
    # (the reader numbers the segments in file order: g's ids; its ranks are what the library is handed)
    assert dg.seq_off.tolist() == g.arrays()["seq_off"].tolist() and dg.adj_off.tolist() == g.arrays()["adj_off"].tolist()
    g.top_rank = dg.top_order_map.tolist()
    g.top_order = np.argsort(dg.top_order_map).tolist()
    c, ov, oo = chop_numpy(g, N)
    a = ctx_factory(k=k, w=w, threshold=T, recombination=R)
    _set(a, c)
    a.add_reads(reads)
    st, res_a, m = _check_against_oracle(oracle, a, c, reads, k, w, T, R)
    woff = dg.set_graph(b, chop=N)
    A = c.arrays()
    assert np.array_equal(woff, A["walk_off"]) and np.array_equal(b.walk_entries(), A["walk_vtx"])
    b.add_reads(reads)
    rb = _same_run(a, b, n_walks, res_a)
    got_v, got_o = b.chop_origin(rb["path_vtx"])
    assert np.array_equal(got_v, ov[rb["path_vtx"]]) and np.array_equal(got_o, oo[rb["path_vtx"]])
    cs = b.chop_stats()
    assert (cs["n_vtx_in"], cs["n_vtx_out"], cs["n_entries_out"]) == (g.n_vtx, c.n_vtx, len(A["walk_vtx"]))
    # the context takes host entries next, unchopped: the device-resident walks were consumed
    _set(b, g)
    assert np.array_equal(b.walk_entries(), g.arrays()["walk_vtx"])
    with pytest.raises(Exception):
        b.chop_stats()


def _arrays_graph(oracle, node_seq, adj, paths):
    g = oracle.Graph(seg_names=[f"s{i + 1}" for i in range(len(node_seq))], node_seq=node_seq, adj=adj, paths=paths,
                     hap_names=[f"h{i}.0" for i in range(len(paths))])
    oracle.kahn(g)
    return g


def test_expansion_borders(oracle, ctx_factory):
    rng = np.random.default_rng(4)

    def rseq(n):
        return bytes(rng.choice(list(b"ACGT"), size=n).tolist())
    # one entry -> 10^6 between two 1-bp vertices, N = 1; a walk of a single vertex; an empty vertex on no walk
    # (every walk starts at the source: the library refuses walks that both start and end inside the graph)
    g = _arrays_graph(oracle, [b"A", rseq(1_000_000), b"C", b""], [[1], [2], [], []], [[0, 1, 2], [0], [0, 1]])
    ctx = ctx_factory(k=9, w=4)
    woff = _set(ctx, g, chop=1)
    first = np.array([0, 1, 1_000_001, 1_000_002, 1_000_003])
    want = np.concatenate([np.arange(first[v], first[v + 1]) for p in g.paths for v in p]).astype(np.int32)
    assert woff.tolist() == [0, 1_000_002, 1_000_003, 2_000_004]
    assert np.array_equal(ctx.walk_entries(), want)
    assert ctx.chop_origin([0, 1, 1_000_000, 1_000_001, 1_000_002])[0].tolist() == [0, 1, 1, 2, 3]
    # exact multiples of N, multiples plus one, N around the expansion's tile size
    g = _arrays_graph(oracle, [rseq(4096 * 3), rseq(4096 * 3 + 1), rseq(4095), rseq(1)], [[1], [2], [3], []], [[0, 1, 2, 3], [0, 1], [0], [0, 1, 2]])
    for N in (1, 3, 4095, 4096, 4097):
        ctx = ctx_factory(k=9, w=4)
        woff = _set(ctx, g, chop=N)
        c, _, _ = chop_numpy(g, N)
        A = c.arrays()
        assert np.array_equal(woff, A["walk_off"]) and np.array_equal(ctx.walk_entries(), A["walk_vtx"]), N
        ctx.close()
    # 1 022 walks
    g = random_graph(rng, n_sites=4, n_walks=1022, seg_len=(1, 90), alt_len=(1, 20), p_del=0.3)
    ctx = ctx_factory(k=5, w=2)
    woff = _set(ctx, g, chop=7)
    A = chop_numpy(g, 7)[0].arrays()
    assert np.array_equal(woff, A["walk_off"]) and np.array_equal(ctx.walk_entries(), A["walk_vtx"])


def test_identity_chop(ctx_factory):
    rng = np.random.default_rng(12)
    g = random_graph(rng, n_sites=7, n_walks=6, seg_len=(5, 60), alt_len=(1, 9))
    longest = max(len(s) for s in g.node_seq)
    reads = mosaic_reads(rng, g, n_reads=60, read_len=50, n_seg=2, err=0.01)
    a = ctx_factory(k=9, w=4, threshold=1.0, recombination=3)
    _set(a, g)
    a.add_reads(reads)
    for N in (longest, longest + 1, 1 << 30):
        b = ctx_factory(k=9, w=4, threshold=1.0, recombination=3)
        woff = _set(b, g, chop=N)
        assert np.array_equal(woff, g.arrays()["walk_off"])
        cs = b.chop_stats()
        assert cs["n_vtx_in"] == cs["n_vtx_out"] == g.n_vtx and cs["n_entries_in"] == cs["n_entries_out"]
        b.add_reads(reads)
        rb = _same_run(a, b, g.n_walks)
        ov, oo = b.chop_origin(rb["path_vtx"])
        assert np.array_equal(ov, rb["path_vtx"]) and not oo.any()
        b.close()


def test_limits(ctx_factory):
    import phi_amd
    rng = np.random.default_rng(3)
    # 62 vertices of 70 000 bases in a chain, 1 000 identical walks: 1 000 x 62 x 70 000 = 4 340 000 000 > 2^32 - 64 at N = 1
    n, L, nw = 62, 70_000, 1000
    seq = bytes(rng.choice(list(b"ACGT"), size=n * L).tolist())
    seq_off = np.arange(n + 1, dtype=np.int64) * L
    adj_off = np.minimum(np.arange(n + 1, dtype=np.int64), n - 1)
    adj = np.arange(1, n, dtype=np.int32)
    walk_off = np.arange(nw + 1, dtype=np.int64) * n
    walk_vtx = np.tile(np.arange(n, dtype=np.int32), nw)
    ctx = ctx_factory(k=9, w=4, threshold=1.0, recombination=3)
    with pytest.raises(phi_amd.PhiError) as e:
        ctx.set_graph(seq, seq_off, adj_off, adj, walk_off, walk_vtx, np.arange(n, dtype=np.int32), chop=1)
    assert e.value.status == phi_amd.PHI_ERR_UNSUPPORTED and "4340000000" in str(e.value)
    with pytest.raises(phi_amd.PhiError) as e:
        ctx.solve()
    assert e.value.status == phi_amd.PHI_ERR_STATE                  # the context holds no graph ...
    g = random_graph(rng, n_sites=5, n_walks=4, seg_len=(5, 40))
    reads = mosaic_reads(rng, g, n_reads=40, read_len=40, n_seg=2)
    _set(ctx, g)                                                    # ... and is usable
    ctx.add_reads(reads)
    r0 = ctx.solve()
    assert r0["optimal"] == 1
    with pytest.raises(phi_amd.PhiError) as e:
        ctx.chop_origin(r0["path_vtx"])
    assert e.value.status == phi_amd.PHI_ERR_STATE
    with pytest.raises(phi_amd.PhiError) as e:
        ctx.chop_stats()
    assert e.value.status == phi_amd.PHI_ERR_STATE
    for bad in (0, -5):
        with pytest.raises(phi_amd.PhiError) as e:
            _set(ctx, g, chop=bad)
        assert e.value.status == phi_amd.PHI_ERR_INVALID
    # what phi_set_graph refuses is refused the same way: an entry out of range, a walk off the edges
    A = g.arrays()
    wv = A["walk_vtx"].copy(); wv[3] = g.n_vtx + 5
    with pytest.raises(phi_amd.PhiError) as e:
        ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], wv, A["top_rank"], chop=4)
    assert e.value.status == phi_amd.PHI_ERR_WALK and f"holds vertex {g.n_vtx + 5} out of range" in str(e.value)
    wv = A["walk_vtx"].copy(); wv[1] = wv[0]
    with pytest.raises(phi_amd.PhiError) as e:
        ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], wv, A["top_rank"], chop=4)
    assert e.value.status == phi_amd.PHI_ERR_WALK
    _set(ctx, g, chop=4)
    ctx.add_reads(reads)
    assert ctx.solve()["optimal"] == 1
    # a refused call leaves no graph behind, chopped or not: nothing answers for the graph that was there
    with pytest.raises(phi_amd.PhiError):
        _set(ctx, g, chop=0)
    for call in (ctx.solve, ctx.chop_stats, lambda: ctx.chop_origin([0])):
        with pytest.raises(phi_amd.PhiError) as e:
            call()
        assert e.value.status == phi_amd.PHI_ERR_STATE


# --------------------------------------------------------------------------- command line

def _run_cli(args, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([PHI] + args, capture_output=True, text=True, cwd=str(cwd), timeout=600, env=e)


def _counter_lines(log):
    """the log lines that carry counters (per-walk tables, spectrum, filter, model, recombinations), without time stamps"""
    out = []
    for line in log.splitlines():
        line = re.sub(r"^\[M::\w+::[\d.]+\*[\d.]+\] ", "", line)
        if re.search(r" : \d+$|spectrum size|Filtered/Retained|Minimizers are in ILP|Recombination count|Recombined haplotypes|Haplotype of size: \d+", line):
            out.append(re.sub(r" written to: .*", "", line))
    return out


CHOP_LINE = re.compile(r"Graph chopped to (\d+) bases: (\d+) -> (\d+) vertices, (\d+) -> (\d+) walk entries")


def _cli_pair(tmp_path, g, N, reads_path, name, extra=(), env=None):
    """PHI --chop N on g's GFA against PHI on the GFA chop_numpy wrote (same file name, so the FASTA header is the same)"""
    c, _, _ = chop_numpy(g, N)
    (tmp_path / "long").mkdir(exist_ok=True)
    (tmp_path / "chopped").mkdir(exist_ok=True)
    long_gfa = _write_gfa(g, tmp_path / "long" / name)
    chopped_gfa = _write_gfa(c, tmp_path / "chopped" / name)
    fa1, fa2 = tmp_path / "long.fa", tmp_path / "chopped.fa"
    r1 = _run_cli(["--chop", str(N), "-g", long_gfa, "-r", reads_path, "-o", str(fa1)] + list(extra), tmp_path, env)
    r2 = _run_cli(["-g", chopped_gfa, "-r", reads_path, "-o", str(fa2)] + list(extra), tmp_path, env)
    assert r1.returncode == 0, r1.stderr
    assert r2.returncode == 0, r2.stderr
    assert fa1.read_bytes() == fa2.read_bytes()
    assert _counter_lines(r1.stderr) == _counter_lines(r2.stderr) and len(_counter_lines(r1.stderr)) > 2 * g.n_walks
    m = CHOP_LINE.search(r1.stderr)
    assert m and not CHOP_LINE.search(r2.stderr)
    assert [int(x) for x in m.groups()] == [N, g.n_vtx, c.n_vtx, sum(len(p) for p in g.paths), sum(len(p) for p in c.paths)]
    assert f"Graph has {g.n_vtx} vertices" in r1.stderr
    return r1, r2


@pytest.mark.parametrize("route", ["host", "walk_text", "gzip_split"])
def test_cli_chop_on_long_segments(tmp_path, route):
    rng = np.random.default_rng(77)
    g = random_graph(rng, n_sites=8, n_walks=5, seg_len=(200, 600), alt_len=(1, 40), p_del=0.2)
    reads = mosaic_reads(rng, g, n_reads=300, read_len=150, n_seg=2, err=0.0)
    rd = tmp_path / "reads.fa"
    rd.write_text("".join(f">r{i}\n{r.decode()}\n" for i, r in enumerate(reads)))
    env = {"walk_text": {"PHI_WALK_TEXT_MIN": "0"}, "gzip_split": {"PHI_GFA_INFLATE_MIN": "0"}}.get(route)
    name = "g.gfa.gz" if route == "gzip_split" else "g.gfa"
    r1, _ = _cli_pair(tmp_path, g, 30, str(rd), name, extra=["-R", "50", "-d1"] if route == "host" else ["-R", "50"], env=env)
    if route != "host":
        e = dict(env); e["PHI_TIMING"] = "1"
        r = _run_cli(["--chop", "30", "-g", str(tmp_path / "long" / name), "-r", str(rd), "-o", str(tmp_path / "t.fa"), "-R", "50"], tmp_path, e)
        assert r.returncode == 0 and ("resolved on the device" in r.stderr or "walks kept on the device" in r.stderr), r.stderr
        assert (tmp_path / "t.fa").read_bytes() == (tmp_path / "long.fa").read_bytes()


def test_cli_chop_on_the_reference_fixture(oracle, tmp_path):
    """tests/golden/data/MHC_4.gfa.gz is a 30-bp graph already: --chop 10 makes it chop."""
    g = oracle.parse_gfa(os.path.join(DATA, "MHC_4.gfa.gz"))
    _cli_pair(tmp_path, g, 10, os.path.join(DATA, "CHM13_reads.fq.gz"), "MHC_4.gfa.gz", extra=["-t32"])


def test_python_mirror_with_chop_agrees_with_the_cli(tmp_path):
    """ILP_index.chop = N (and `python -m phi_amd.ilp_index --chop N`): the FASTA, the counter lines, the recombination
    report in output coordinates and the extra line of `PHI --chop N`."""
    import io
    from phi_amd import ilp_index as H
    rng = np.random.default_rng(78)
    g = random_graph(rng, n_sites=8, n_walks=5, seg_len=(200, 600), alt_len=(1, 40), p_del=0.2)
    reads = mosaic_reads(rng, g, n_reads=300, read_len=150, n_seg=2, err=0.0)
    rd = tmp_path / "reads.fa"
    rd.write_text("".join(f">r{i}\n{r.decode()}\n" for i, r in enumerate(reads)))
    gfa = _write_gfa(g, tmp_path / "g.gfa")
    fa = tmp_path / "cli.fa"
    r = _run_cli(["--chop", "30", "-g", gfa, "-r", str(rd), "-o", str(fa), "-R", "20"], tmp_path)
    assert r.returncode == 0, r.stderr
    log = io.StringIO()
    idx = H.ILP_index(gfa, log=log)
    idx.read_gfa()
    idx.recombination, idx.chop = 20, 30
    idx.hap_file = str(tmp_path / "py.fa")
    idx.hap_name = H.get_hap_name(gfa, str(rd))
    rr = []
    idx.read_ip_reads(rr, str(rd))
    res = idx.ILP_function(rr)
    assert open(idx.hap_file, "rb").read() == fa.read_bytes()
    assert _counter_lines(log.getvalue()) == _counter_lines(r.stderr)
    assert any(l.startswith("Recombined haplotypes: >(") for l in _counter_lines(log.getvalue()))
    assert CHOP_LINE.search(log.getvalue()).groups() == CHOP_LINE.search(r.stderr).groups()
    c, ov, oo = chop_numpy(g, 30)
    assert np.array_equal(res["path_orig_vtx"], ov[res["path_vtx"]]) and np.array_equal(res["path_orig_off"], oo[res["path_vtx"]])
    # the module's own command line
    import subprocess as sp
    import sys
    p = sp.run([sys.executable, "-m", "phi_amd.ilp_index", "--chop", "30", "-g", gfa, "-r", str(rd), "-o", str(tmp_path / "py2.fa"), "-R", "20"],
               capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "py2.fa").read_bytes() == fa.read_bytes() and CHOP_LINE.search(p.stderr)
    # and without chop the mirror says nothing of it
    log0 = io.StringIO()
    idx0 = H.ILP_index(gfa, log=log0)
    idx0.read_gfa()
    idx0.recombination = 20
    idx0.hap_file, idx0.hap_name = str(tmp_path / "py0.fa"), idx.hap_name
    res0 = idx0.ILP_function(rr)
    assert "chopped" not in log0.getvalue() and "path_orig_vtx" not in res0


def test_cli_without_chop_is_unchanged(tmp_path):
    """No --chop: the log and the FASTA tests/test_gpu_cli.py::test_cli_config1_logs_and_fasta pins, and no line of the chop."""
    import json
    from conftest import GOLDEN
    gold = json.load(open(os.path.join(GOLDEN, "counters.json")))["mhc4_chm13_k31_w25"]
    out = tmp_path / "CHM13.fa"
    r = _run_cli(["-t32", "-g", os.path.join(DATA, "MHC_4.gfa.gz"), "-r", os.path.join(DATA, "CHM13_reads.fq.gz"), "-o", str(out)], tmp_path)
    assert r.returncode == 0, r.stderr
    log = r.stderr
    assert "chopped" not in log and not CHOP_LINE.search(log)
    assert "Graph has 111805 vertices, 5 walks and read has 16401 reads" in log
    for name, n in zip(gold["hap_names"], gold["n_minimizers"]):
        assert f"{name} : {n}\n" in log
    assert f"Indexed reads with spectrum size: {gold['spectrum_size']}\n" in log
    for name, n in zip(gold["hap_names"], gold["n_anchors"]):
        assert f"{name} : {n}\n" in log
    assert f"Filtered/Retained Minimizers: {gold['filtered_retained_pct']}%\n" in log
    assert f"{gold['pct_in_model']}% Minimizers are in ILP\n" in log
    assert "Recombination count: 0\n" in log
    m = re.search(r"Recombined haplotypes: >\(CHM13\.0,\[0,(\d+)\]\)\n", log)
    assert m
    txt = out.read_text().split("\n")
    mm = re.match(r">MHC_4\.gfa_CHM13_reads\.fq LN:(\d+)$", txt[0])
    assert mm and int(mm.group(1)) == int(m.group(1)) + 1
    seq = "".join(txt[1:])
    assert len(seq) == int(mm.group(1)) and all(len(x) == 80 for x in txt[1:-2])
    assert f"Haplotype of size: {len(seq)} written to: {out}" in log
    r = _run_cli(["--chop", "0", "-g", "x", "-r", "y", "-o", "z"], tmp_path)
    assert r.returncode == 1 and "--chop" in r.stderr
