""" "Set graph" from a phased VCF + reference FASTA (include/phi_amd.h phi_vcf_genotypes / phi_vcf_walks, phi_amd/csrc/vcf.hip;
host side phi_amd/csrc/host/vcf_reader.cpp) against the Python route it replaces: phi_amd/vcf2gfa.py writing a GFA and the
host reader reading it back.  The genotype kernel against the scalar parser and the Python's own lines; every array of the whole
route, the walk entries on the device included; MHC_4 through both routes down to the inferred sequence; the refusals; the
command line."""
import gzip
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

PHI = os.path.join(ROOT, "phi_amd", "PHI")
SHAPES = [b"0|1", b"1/0", b".", b".|.", b"1", b"10|2", b"0|1|2", b"a|1", b"", b"3|", b".|2", b"007|1", b"9999|65", b"1x|+2"]


def _py_field(field, gi):
    """vcf2gfa.read_vcf's lines for one sample field"""
    g = field.split(b":")[gi].replace(b"/", b"|").split(b"|")
    ploidy = min(2, sum(1 for x in g if x != b"."))
    g = [int(x) if x.isdigit() else 0 for x in g] + [0, 0]
    return (min(g[0], 65535), min(g[1], 65535)), ploidy


def _shape_tables():
    """per field variant (gi = 0 bare, gi = 0 with a second part, gi = 1) and shape: the field's bytes and what the Python's lines
    make of it -- the expected matrix is then indexed, not parsed field by field in the interpreter"""
    fields = np.empty((3, len(SHAPES)), object)
    vals = np.zeros((3, len(SHAPES), 2), np.uint16)
    pls = np.zeros((3, len(SHAPES)), np.int32)
    for k, gt in enumerate(SHAPES):
        for v, (f, gi) in enumerate(((gt, 0), (gt + b":7", 0), (b"35:" + gt + b":PASS", 1))):
            fields[v, k] = f
            vals[v, k], pls[v, k] = _py_field(f, gi)
    return fields, vals, pls


def _genotype_text(rng, n_rec, n_s, pad_first=0, big_at=None, force_gi0=False):
    """sample-column slices laid out as phi_vcf_read lays them out, with the Python's matrix and ploidy"""
    fields, vals, pls = _shape_tables()
    gi = rng.integers(0, 2, size=n_rec).astype(np.int32)
    if force_gi0:
        gi[0] = 1
    pick = rng.integers(0, len(SHAPES), size=(n_rec, n_s))
    variant = np.where(gi[:, None] == 1, 2, ((np.arange(n_rec)[:, None] + np.arange(n_s)[None, :]) % 3 == 0).astype(np.int64))
    want = vals[variant, pick]
    ploidy = pls[variant, pick].max(axis=0).astype(np.int32)
    cells = fields[variant, pick]
    lines = [b"\t".join(row) + b"\n" for row in cells.tolist()]
    if pad_first:                                              # (gi[0] == 1: the padding goes into the FORMAT part before GT)
        assert gi[0] == 1 and lines[0].startswith(b"35:")
        lines[0] = b"35" + b"x" * pad_first + lines[0][2:]
    if big_at is not None:                                     # beyond the matrix width: the kernel must flag the record
        r, s_ = big_at
        row = cells[r].tolist()
        row[s_] = b"35:1|99999999999:PASS" if gi[r] else b"1|99999999999"
        lines[r] = b"\t".join(row) + b"\n"
        want[r, s_] = _py_field(row[s_], int(gi[r]))[0]
        ploidy[s_] = max(ploidy[s_], 2)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.int64)
    return np.frombuffer(b"".join(lines), np.uint8), off, gi, want, ploidy


def _device_genotypes(ctx, text, off, gi, n_s):
    import ctypes as C
    n_rec = len(off) - 1
    gt = np.full((n_rec, n_s, 2), 7, np.uint16)
    ploidy = np.full(n_s, 9, np.int32)
    flagged = np.full(max(n_rec, 1), 9, np.uint8)
    ctx._chk(ctx._L.phi_vcf_genotypes(ctx._h, text.ctypes.data, len(text), off.ctypes.data, gi.ctypes.data, n_rec, n_s,
                                      gt.ctypes.data, ploidy.ctypes.data, flagged.ctypes.data))
    return gt, ploidy, flagged[:n_rec]


@pytest.mark.parametrize("n_s", [1, 2, 63, 64, 65, 257, 1100])
def test_genotype_kernel_equals_scalar_parser_and_python(ctx_factory, n_s):
    from phi_amd import ilp_index as H
    ctx = ctx_factory()
    rng = np.random.default_rng(100 + n_s)
    for n_rec in (1, 3000):
        text, off, gi, want, want_pl = _genotype_text(rng, n_rec, n_s)
        gt, ploidy, flagged = _device_genotypes(ctx, text, off, gi, n_s)
        assert not flagged.any()
        hgt, hpl = H.parse_gt(text, off, gi, n_s)
        assert np.array_equal(hgt, want) and np.array_equal(hpl, want_pl)
        assert np.array_equal(gt, want) and np.array_equal(ploidy, want_pl)
        st = ctx.vcf_stats()
        assert (st["text_bytes"], st["n_records"], st["n_samples"], st["n_flagged"]) == (len(text), n_rec, n_s, 0) and st["genotype_gpu_ms"] > 0


def test_genotype_kernel_at_tile_borders_and_with_a_flagged_record(ctx_factory):
    """A record whose slice begins in the last 15 bytes of a 16-byte-aligned 4-KB tile, a field that straddles the border, and one
    allele too large for the matrix: flagged, filled by the scalar parser, equal to the Python's."""
    from phi_amd import ilp_index as H
    ctx = ctx_factory()
    rng = np.random.default_rng(5)
    n_s, n_rec = 3, 900
    for target in range(4096 - 15, 4097):
        # the first record's first field is padded (in a FORMAT part before GT) so that record 1 begins at `target`
        probe = _genotype_text(np.random.default_rng(target), n_rec, n_s, force_gi0=True)
        pad = target - int(probe[1][1])
        text, off, gi, want, want_pl = _genotype_text(np.random.default_rng(target), n_rec, n_s, pad_first=pad, force_gi0=True)
        assert pad > 0 and off[1] == target and len(text) > 4096 + 16
        gt, ploidy, flagged = _device_genotypes(ctx, text, off, gi, n_s)
        assert not flagged.any() and np.array_equal(gt, want) and np.array_equal(ploidy, want_pl), target
    # some field straddles a tile border in a long text; one record carries an allele beyond 16 bits
    n_s, n_rec = 40, 700
    text, off, gi, want, want_pl = _genotype_text(rng, n_rec, n_s, big_at=(351, 17))
    delim = np.flatnonzero((text == 9) | (text == 10))
    assert len(text) > 3 * 4096 and not np.isin(np.arange(4096, len(text), 4096) - 1, delim).all()
    gt, ploidy, flagged = _device_genotypes(ctx, text, off, gi, n_s)
    assert np.flatnonzero(flagged).tolist() == [351] and ctx.vcf_stats()["n_flagged"] == 1
    keep = np.ones(n_rec, bool); keep[351] = False
    assert np.array_equal(gt[keep], want[keep])
    H.parse_gt(text, off, gi, n_s, 351, 352, gt, ploidy)       # the fallback
    assert np.array_equal(gt, want) and np.array_equal(ploidy, want_pl) and gt[351, 17].tolist() == [1, 65535]
    # fewer fields than samples, fewer ':' parts than GT's index: flagged, and an error of the fallback
    for bad in (b"0|1\t1|1\n", b"3:0|1\t7\t3:1|0\n"):
        text = np.frombuffer(b"0|1\t0|0\t1|1\n" + bad, np.uint8)
        off = np.array([0, 12, len(text)], np.int64)
        gi = np.array([0, 1 if b":" in bad else 0], np.int32)
        gt, ploidy, flagged = _device_genotypes(ctx, text, off, gi, 3)
        assert flagged.tolist() == [0, 1] and gt[0].tolist() == [[0, 1], [0, 0], [1, 1]]
        with pytest.raises(H.HostError):
            H.parse_gt(text, off, gi, 3, 1, 2, gt, ploidy)
    # a layout that is not the reader's is refused, the context stays usable
    import phi_amd
    text = np.frombuffer(b"0|1\n0|0\n", np.uint8)
    with pytest.raises(phi_amd.PhiError):
        _device_genotypes(ctx, text, np.array([0, 8], np.int64), np.array([0], np.int32), 1)
    gt, _, _ = _device_genotypes(ctx, text, np.array([0, 4, 8], np.int64), np.array([0, 0], np.int32), 1)
    assert gt[:, 0].tolist() == [[0, 1], [0, 0]]


def _write_case(tmp_path, name, ref, samples, recs):
    """recs: (pos0, ref bytes, [alt bytes], [GT field bytes per sample])"""
    vcf, fa = tmp_path / (name + ".vcf"), tmp_path / (name + ".fa")
    with open(vcf, "wb") as f:
        f.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + b"\t".join(s.encode() for s in samples) + b"\n")
        for (p, r, alts, gts) in recs:
            f.write(b"chr\t%d\t.\t%s\t%s\t60\t.\t.\tGT\t%s\n" % (p + 1, r, b",".join(alts), b"\t".join(gts)))
    fa.write_bytes(b">chr\n" + b"\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + b"\n")
    return str(vcf), str(fa)


def _random_case(rng, tmp_path, case):
    """test_cpu_vcf2gfa.py's generator, widened: up to 40 samples, some of them haploid"""
    ref = bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(300, 900))).tolist())
    n_s = int(rng.integers(1, 41))
    haploid = rng.random(n_s) < 0.25
    recs, pos = [], int(rng.integers(2, 20))
    while pos < len(ref) - 60:
        kind = rng.random()
        rl = 1 if kind < 0.5 else int(rng.integers(1, 40))
        r = ref[pos:pos + rl]
        alts = []
        for _ in range(int(rng.integers(1, 4))):
            al = int(rng.integers(1, 45)) if rng.random() < 0.6 else 1
            a = r[:1] + bytes(rng.choice(list(b"ACGT"), size=al - 1).tolist()) if rng.random() < 0.7 else bytes(rng.choice(list(b"ACGT"), size=al).tolist())
            if a != r and a not in alts:
                alts.append(a)
        if alts:
            gts = [b"%d" % rng.integers(0, len(alts) + 1) if haploid[s] else b"%d|%d" % (rng.integers(0, len(alts) + 1), rng.integers(0, len(alts) + 1))
                   for s in range(n_s)]
            recs.append((pos, r, alts, gts))
        step = rng.random()
        pos += 0 if step < 0.1 else (int(rng.integers(1, max(2, rl))) if step < 0.35 else rl + int(rng.integers(0, 60)))
    return _write_case(tmp_path, f"c{case}", ref, ["S%d" % i for i in range(n_s)], recs)


def _python_graph(vcf, fa, tmp_path, max_len=30):
    """the Python route: vcf2gfa to a GFA file, the host reader over it"""
    from phi_amd import ilp_index as H
    from phi_amd import vcf2gfa
    old = vcf2gfa.CHOP
    vcf2gfa.CHOP = max_len
    try:
        _, ref_seq = vcf2gfa.read_fasta_single(fa)
        ref_seq = ref_seq.upper()
        samples, recs, ploidy = vcf2gfa.read_vcf(vcf, ref_seq, warn=lambda m: None)
        segs, links, walks = vcf2gfa.build(ref_seq, samples, recs, ploidy)
    finally:
        vcf2gfa.CHOP = old
    p = tmp_path / (os.path.basename(vcf) + ".%d.gfa" % max_len)
    with open(p, "wb") as f:
        vcf2gfa.write_gfa(f, "REF#0", segs, links, walks)
    return H.Graph(str(p)), str(p)


def _same_graph(ctx, v, g):
    for f in ("seq_off", "seq_concat", "adj_off", "adj", "walk_off", "top_order_map"):
        assert np.array_equal(getattr(v, f), getattr(g, f)), f
    assert v.hap_id2name == g.hap_id2name
    assert np.array_equal(ctx.walk_entries(), g.walk_vtx)
    st = v.stats
    assert st["n_entries"] == len(g.walk_vtx) and st["n_units"] == v.n_units and st["walks_gpu_ms"] > 0


@pytest.mark.parametrize("max_len", [30, 7])
def test_whole_route_equals_the_python_route_on_random_cases(ctx_factory, tmp_path, max_len):
    ctx = ctx_factory(k=5, w=3)
    rng = np.random.default_rng(11)
    n_haploid = 0
    for case in range(30):
        vcf, fa = _random_case(rng, tmp_path, case)
        g, _ = _python_graph(vcf, fa, tmp_path, max_len)
        v = ctx.set_graph_vcf(vcf, fa, max_len=max_len)
        _same_graph(ctx, v, g)
        n_haploid += 1 + 2 * len(v.samples) - v.num_walks
    assert n_haploid > 0


def test_whole_route_on_the_shapes_that_matter(ctx_factory, tmp_path):
    ctx = ctx_factory(k=5, w=3)
    rng = np.random.default_rng(2)
    ref = bytes(rng.choice(list(b"ACGT"), size=500).tolist())

    def other(b):
        return b"C" if b != b"C" else b"G"
    cases = {
        # no site at all: one unit, every walk the backbone (a record nobody carries; and no record)
        "nosite": (["A", "B"], [(100, ref[100:101], [other(ref[100:101])], [b"0|0", b"0"])]),
        "norecord": (["A"], []),
        "onesite": (["A", "B"], [(100, ref[100:103], [b"T" + ref[101:102]], [b"0|1", b"1|0"])]),
        # the only non-reference haplotype is the last sample's second column
        "lastcolumn": (["S%d" % i for i in range(9)], [(50, ref[50:51], [other(ref[50:51])], [b"0|0"] * 8 + [b"0|1"]),
                                                        (300, ref[300:301], [other(ref[300:301])], [b"0|0"] * 8 + [b"0|1"])]),
    }
    # a site with more than 255 distinct alleles: 300 haploid samples, each with its own ALT of one multi-allelic record
    alts = []
    while len(alts) < 300:
        a = ref[200:201] + bytes(rng.choice(list(b"ACGT"), size=6).tolist())
        if a not in alts:
            alts.append(a)
    cases["manyalleles"] = (["H%d" % i for i in range(300)], [(200, ref[200:201], alts, [b"%d" % (i + 1) for i in range(300)])])
    for name, (samples, recs) in cases.items():
        vcf, fa = _write_case(tmp_path, name, ref, samples, recs)
        g, _ = _python_graph(vcf, fa, tmp_path)
        if name == "manyalleles":
            # 301 out-edges of one vertex: beyond what phi_set_graph takes of ANY graph (254, include/phi_amd.h), the Python
            # route's GFA included; the route up to there is checked all the same, and the context stays usable
            import phi_amd
            for route in (lambda: ctx.set_graph_vcf(vcf, fa), lambda: ctx.set_graph(g.seq_concat, g.seq_off, g.adj_off, g.adj, g.walk_off, g.walk_vtx, g.top_order_map)):
                with pytest.raises(phi_amd.PhiError) as e:
                    route()
                assert "more than 254 out-edges" in str(e.value)
            v = ctx.vcf_graph(vcf, fa)
        else:
            v = ctx.set_graph_vcf(vcf, fa)
        _same_graph(ctx, v, g)
        if name in ("nosite", "norecord"):
            assert v.n_units == 1 and v.n_real_sites == 0 and all(np.array_equal(g.walk_vtx[g.walk_off[h]:g.walk_off[h + 1]], np.arange(g.n_vtx)) for h in range(g.num_walks))
        if name == "manyalleles":
            assert v.n_units == 1 + 301 + 1 and v.num_walks == 301 and int(v.choice.max()) == 300


@pytest.fixture(scope="module")
def mhc4(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mhc4")
    vcf, fa = os.path.join(DATA, "MHC_4.vcf.gz"), os.path.join(DATA, "MHC-CHM13.0.fa.gz")
    g, gfa = _python_graph(vcf, fa, tmp)
    from phi_amd import ilp_index as H
    bases, off, _ = H.read_reads(os.path.join(DATA, "CHM13_reads.fq.gz"))
    return dict(vcf=vcf, fa=fa, graph=g, gfa=gfa, reads=(bases, off), tmp=tmp)


def test_mhc4_through_both_routes(ctx_factory, mhc4):
    g = mhc4["graph"]
    a, b = ctx_factory(), ctx_factory()
    a.set_params()
    b.set_params()
    v = a.set_graph_vcf(mhc4["vcf"], mhc4["fa"])
    _same_graph(a, v, g)
    assert v.hap_id2name == ["REF.0", "HG002.1", "HG002.2", "HG005.1", "HG005.2"] and v.stats["n_flagged"] == 0
    b.set_graph(g.seq_concat, g.seq_off, g.adj_off, g.adj, g.walk_off, g.walk_vtx, g.top_order_map)
    res = []
    for c in (a, b):
        c.add_reads(mhc4["reads"])
        res.append(c.solve())
    for key in ("objective", "optimal", "spectrum_size", "filtered", "retained", "n_in_model"):
        assert res[0][key] == res[1][key], key
    for key in ("n_minimizers", "n_anchors"):
        assert np.array_equal(res[0][key], res[1][key]), key
    assert a.path_sequence(res[0]["hap_len"]) == b.path_sequence(res[1]["hap_len"]) and res[0]["hap_len"] > 1000


def test_refusals_leave_the_context_usable(ctx_factory, tmp_path):
    from phi_amd import ilp_index as H
    ctx = ctx_factory(k=5, w=3)
    rng = np.random.default_rng(8)
    ref = bytes(rng.choice(list(b"ACGT"), size=400).tolist())
    alt = lambda p: [b"C" if ref[p:p + 1] != b"C" else b"G"]
    good = _write_case(tmp_path, "good", ref, ["A", "B"], [(100, ref[100:101], alt(100), [b"0|1", b"1"]), (250, ref[250:252], [b"T"], [b"1|0", b"0"])])
    first = _write_case(tmp_path, "first", ref, ["A"], [(0, ref[0:1], alt(0), [b"0|1"])])
    last = _write_case(tmp_path, "last", ref, ["A"], [(399, ref[399:400], alt(399), [b"0|1"])])
    two = tmp_path / "two.fa"
    two.write_bytes(b">chr\n" + ref + b"\n>chr2\nACGT\n")
    for (vcf, fa), phrase in ((first, "first base of the contig"), (last, "last base of the contig"), ((good[0], str(two)), "more than one record")):
        with pytest.raises(H.HostError) as e:
            ctx.set_graph_vcf(vcf, fa)
        assert phrase in str(e.value)
        g, _ = _python_graph(*good, tmp_path)
        v = ctx.set_graph_vcf(*good)
        _same_graph(ctx, v, g)
        ctx.reset_reads()
        ctx.add_reads([ref[80:200], ref[220:330]])
        res = ctx.solve()
        assert res["optimal"] and res["n_path"] > 0


def _run_cli(args, cwd):
    from __graft_entry__ import ensure_built
    ensure_built()
    return subprocess.run([PHI] + args, capture_output=True, text=True, cwd=str(cwd), timeout=300)


def test_cli_vcf_route_against_the_gfa_of_the_python_route(mhc4):
    from phi_amd import eval_log
    tmp = mhc4["tmp"]
    reads = os.path.join(DATA, "CHM13_reads.fq.gz")
    r1 = _run_cli(["--vcf", mhc4["vcf"], "--ref", mhc4["fa"], "-r", reads, "-o", "vcf.fa"], tmp)
    r2 = _run_cli(["-g", mhc4["gfa"], "-r", reads, "-o", "gfa.fa"], tmp)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-2000:], r2.stderr[-2000:])
    assert "Loaded graph from: " + mhc4["vcf"] in r1.stderr
    seq = lambda p: "".join(open(os.path.join(str(tmp), p)).read().split("\n")[1:])
    assert seq("vcf.fa") == seq("gfa.fa") and len(seq("vcf.fa")) > 1000
    from phi_amd import ilp_index as H
    assert open(os.path.join(str(tmp), "vcf.fa")).readline().startswith(">" + H.get_hap_name(mhc4["vcf"], reads) + " LN:")
    a, b = eval_log.parse_log(r1.stderr), eval_log.parse_log(r2.stderr)
    for key in a:
        if key not in ("real_time_s", "peak_rss_gb"):
            assert a[key] == b[key] and a[key] is not None, key
    r = _run_cli(["--vcf", mhc4["vcf"], "--ref", mhc4["fa"], "-g", mhc4["gfa"], "-r", reads, "-o", "x.fa"], tmp)
    assert r.returncode == 1 and "exclude each other" in r.stderr


def test_cli_vcf_route_refusals_chop_and_several_read_sets(tmp_path):
    rng = np.random.default_rng(4)
    ref = bytes(rng.choice(list(b"ACGT"), size=3000).tolist())
    alt = lambda p: [b"C" if ref[p:p + 1] != b"C" else b"G"]
    recs = [(p, ref[p:p + 1], alt(p), [b"0|1", b"1|0"]) for p in range(100, 2900, 97)]
    good = _write_case(tmp_path, "good", ref, ["A", "B"], recs)
    first = _write_case(tmp_path, "first", ref, ["A"], [(0, ref[0:1], alt(0), [b"0|1"])])
    two = tmp_path / "two.fa"
    two.write_bytes(b">chr\n" + ref + b"\n>chr2\nACGT\n")
    (tmp_path / "a.fa").write_bytes(b">r1\n" + ref[200:1500] + b"\n")
    (tmp_path / "b.fa").write_bytes(b">r1\n" + ref[900:2800] + b"\n")
    for vcf, fa, phrase in ((first[0], first[1], "first base of the contig"), (good[0], str(two), "more than one record")):
        r = _run_cli(["--vcf", vcf, "--ref", fa, "-r", "a.fa", "-o", "o.fa"], tmp_path)
        assert r.returncode == 1 and phrase in r.stderr, r.stderr[-1500:]
    g, gfa = _python_graph(*good, tmp_path, 11)
    r1 = _run_cli(["--vcf", good[0], "--ref", good[1], "--chop", "11", "-r", "a.fa", "-o", "va.fa", "-r", "b.fa", "-o", "vb.fa"], tmp_path)
    r2 = _run_cli(["-g", gfa, "-r", "a.fa", "-o", "ga.fa", "-r", "b.fa", "-o", "gb.fa"], tmp_path)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1500:], r2.stderr[-1500:])
    seq = lambda p: "".join((tmp_path / p).read_text().split("\n")[1:])
    assert seq("va.fa") == seq("ga.fa") and seq("vb.fa") == seq("gb.fa") and len(seq("va.fa")) > 100


def test_cli_vcf_route_prints_the_two_warnings_in_the_scripts_words(tmp_path, capsys):
    """A record of another contig and one whose REF is not the FASTA's: skipped, and stderr carries exactly the lines
    phi_amd.vcf2gfa.read_vcf writes for the same file."""
    from phi_amd import vcf2gfa
    rng = np.random.default_rng(6)
    ref = bytes(rng.choice(list(b"ACGT"), size=3000).tolist())
    alt = lambda p: [b"C" if ref[p:p + 1] != b"C" else b"G"]
    recs = [(p, ref[p:p + 1], alt(p), [b"0|1", b"1|0"]) for p in range(100, 2900, 97)]
    vcf, fa = _write_case(tmp_path, "warn", ref, ["A", "B"], recs)
    wrong = b"A" if ref[1500:1501] != b"A" else b"T"
    with open(vcf, "ab") as f:
        f.write(b"other\t20\t.\tA\tC\t60\t.\t.\tGT\t1|1\t1|1\n" * 2)
        f.write(b"chr\t1501\t.\t" + wrong + b"\tN\t60\t.\t.\tGT\t1|1\t1|1\n")
    (tmp_path / "a.fa").write_bytes(b">r1\n" + ref[200:1500] + b"\n")
    _, ref_seq = vcf2gfa.read_fasta_single(fa)
    vcf2gfa.read_vcf(vcf, ref_seq.upper())
    want = [l for l in capsys.readouterr().err.splitlines() if l.startswith("[W::vcf2gfa] ")]
    assert len(want) == 2 and "2 record(s) of other contigs than chr" in want[0] and "1 record(s) skipped" in want[1]
    r = _run_cli(["--vcf", vcf, "--ref", fa, "-r", "a.fa", "-o", "o.fa"], tmp_path)
    assert r.returncode == 0, r.stderr[-1500:]
    assert [l for l in r.stderr.splitlines() if l.startswith("[W::vcf2gfa] ")] == want
