"""The host side of the VCF route (phi_amd/csrc/host/vcf_reader.cpp: phi_vcf_read, phi_vcf_parse_gt, phi_vcf_build) against
its oracle, phi_amd/vcf2gfa.py: records and their order, skip counts, ploidy, segments, links, walks, names -- on the random
cases of test_cpu_vcf2gfa.py (generator copied), on its refusal and skip cases, at three segment lengths; the scalar genotype
parser on hand-written fields; and the whole of it under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone
program run as a child process."""
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HOSTDIR = os.path.join(ROOT, "phi_amd", "csrc", "host")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", HOSTDIR, "-s", os.path.join("..", "..", "libphi_host.so")])
    return True


def _random_case(rng, tmp_path, case):
    """One case of test_cpu_vcf2gfa.py's generator: overlapping, touching, multi-allelic and conflicting records."""
    ref = bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(300, 900))).tolist())
    n_s = int(rng.integers(1, 4))
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
            gts = [(int(rng.integers(0, len(alts) + 1)), int(rng.integers(0, len(alts) + 1))) for _ in range(n_s)]
            recs.append((pos, r, alts, gts))
        step = rng.random()
        pos += 0 if step < 0.1 else (int(rng.integers(1, max(2, rl))) if step < 0.35 else rl + int(rng.integers(0, 60)))
    vcf = tmp_path / f"c{case}.vcf"
    with open(vcf, "wb") as f:
        f.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + b"\t".join(b"S%d" % i for i in range(n_s)) + b"\n")
        for (p, r, alts, gts) in recs:
            f.write(b"chr\t%d\t.\t%s\t%s\t60\t.\t.\tGT\t%s\n" % (p + 1, r, b",".join(alts), b"\t".join(b"%d|%d" % g for g in gts)))
    fa = tmp_path / f"c{case}.fa"
    fa.write_bytes(b">chr\n" + b"\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + b"\n")
    return str(vcf), str(fa)


def _python_route(vcf, fa, tmp_path):
    """vcf2gfa's own result and the reader's arrays for the file write_gfa writes."""
    from phi_amd import ilp_index as H
    from phi_amd import vcf2gfa
    _, ref_seq = vcf2gfa.read_fasta_single(fa)
    ref_seq = ref_seq.upper()
    msgs = []
    samples, recs, ploidy = vcf2gfa.read_vcf(vcf, ref_seq, warn=msgs.append)
    segs, links, walks = vcf2gfa.build(ref_seq, samples, recs, ploidy)
    buf = io.BytesIO()
    vcf2gfa.write_gfa(buf, "REF#0", segs, links, walks)
    p = tmp_path / "py_route.gfa"
    p.write_bytes(buf.getvalue())
    return dict(samples=samples, recs=recs, ploidy=ploidy, segs=segs, links=links, walks=walks, msgs=msgs, graph=H.Graph(str(p)))


def _check_against_python(vcf, fa, tmp_path, max_len=30):
    from phi_amd import ilp_index as H
    want = _python_route(vcf, fa, tmp_path)
    v = H.VcfGraph(vcf, fa)
    # records and their order, skip counts (the warnings in the script's words), ploidy
    assert v.samples == want["samples"]
    assert v.warnings() == want["msgs"]
    gt, ploidy = v.parse_gt()
    assert ploidy.tolist() == want["ploidy"]
    assert v.n_records == len(want["recs"])
    for r, (s, e, alts, gts) in enumerate(want["recs"]):
        assert (int(v.rec_start[r]), int(v.rec_end[r])) == (s, e) and v.alts(r) == alts
        assert [tuple(x) for x in gt[r].tolist()] == [(min(a, 65535), min(b, 65535)) for a, b in gts]
    v.build(gt, ploidy, max_len)
    # segments, links, walks, names: the builder's arrays against vcf2gfa.build, and against the reader over write_gfa's file
    g = want["graph"]
    raw = v.seq_concat.tobytes()
    assert [raw[v.seq_off[i]:v.seq_off[i + 1]] for i in range(v.n_vtx)] == want["segs"]
    src = np.repeat(np.arange(v.n_vtx), np.diff(v.adj_off))
    assert list(zip(src.tolist(), v.adj.tolist())) == sorted(want["links"])
    walk_off, walk_vtx = v.host_walks()
    assert [walk_vtx[walk_off[h]:walk_off[h + 1]].tolist() for h in range(v.num_walks)] == [ids for _, _, ids in want["walks"]]
    assert v.hap_id2name == ["%s.%d" % (s, h) for s, h, _ in want["walks"]] == g.hap_id2name
    for f in ("seq_off", "seq_concat", "adj_off", "adj", "top_order_map"):
        assert np.array_equal(getattr(v, f), getattr(g, f)), f
    assert np.array_equal(walk_off, g.walk_off) and np.array_equal(walk_vtx, g.walk_vtx)
    v.close()
    return want


def test_reader_and_builder_equal_vcf2gfa_on_the_random_cases(built, tmp_path):
    rng = np.random.default_rng(3)
    n_sites_seen = 0
    for case in range(30):
        vcf, fa = _random_case(rng, tmp_path, case)
        want = _check_against_python(vcf, fa, tmp_path)
        n_sites_seen += len(want["recs"])
        assert all(1 <= len(s) <= 30 for s in want["segs"])
    assert n_sites_seen > 300


@pytest.mark.parametrize("max_len", [7, 1000])
def test_builder_at_other_segment_lengths(built, tmp_path, monkeypatch, max_len):
    from phi_amd import vcf2gfa
    monkeypatch.setattr(vcf2gfa, "CHOP", max_len)
    rng = np.random.default_rng(3)
    for case in range(30):
        vcf, fa = _random_case(rng, tmp_path, case)
        want = _check_against_python(vcf, fa, tmp_path, max_len)
        assert max(len(s) for s in want["segs"]) <= max_len and (max_len != 7 or max(len(s) for s in want["segs"]) == 7)


def test_reader_skips_and_refuses_what_vcf2gfa_does(built, tmp_path):
    from phi_amd import ilp_index as H
    ref = b"ACGTTGCAAGGCTTAACCGGATCGATCGGCTAAGCTTAGGCTA" * 3
    fa = tmp_path / "r.fa"
    fa.write_bytes(b">chr\n" + ref.lower()[:40] + b"\n" + ref[40:] + b"\n")
    hdr = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tD\tH\n"
    vcf = tmp_path / "v.vcf"
    vcf.write_bytes(hdr + b"chr\t11\t.\t" + ref[10:11] + b"\tT\t60\t.\t.\tGT\t0|1\t1\n"        # D diploid, H haploid
                    b"other\t20\t.\tA\tC\t60\t.\t.\tGT\t1|1\t1\n"                               # another contig
                    b"chr\t31\t.\tN\tC\t60\t.\t.\tGT\t1|1\t1\n"                                 # REF is not what the FASTA holds
                    b"chr\t41\t.\t" + ref[40:41] + b"\t<DEL>\t60\t.\t.\tGT\t1|1\t1\n"           # symbolic
                    b"chr\t42\t.\t" + ref[41:42] + b"\tA,*\t60\t.\t.\tGT\t1|1\t1\n"             # spanning deletion
                    b"chr\t43\t.\t" + ref[42:43] + b"\tA[chr:5[\t60\t.\t.\tGT\t1|1\t1\n"        # breakend
                    b"chr\t44\t.\t" + ref[43:44] + b"\tA,\t60\t.\t.\tGT\t1|1\t1\n"              # empty ALT
                    b"chr\t45\t.\t" + ref[44:45] + b"\tA\t60\t.\t.\tDP\t1|1\t1\n"               # no GT
                    b"chr\t%d\t.\t" % len(ref) + ref[-1:] + b"CC\tA\t60\t.\t.\tGT\t1|1\t1\n"     # reaches outside the contig
                    b"chr\t0\t.\tA\tC\t60\t.\t.\tGT\t1|1\t1\n"                                  # before the contig
                    b"chr\t51\tshort line\n\n")
    want = _check_against_python(str(vcf), str(fa), tmp_path)
    assert len(want["recs"]) == 1 and want["ploidy"] == [2, 1] and len(want["msgs"]) == 2
    assert [(s_, h) for s_, h, _ in want["walks"]] == [("REF", 0), ("D", 1), ("D", 2), ("H", 1)]
    # the refusals: the script's two messages; a FASTA with two records; what makes the Python raise
    first = tmp_path / "first.vcf"
    first.write_bytes(hdr + b"chr\t1\t.\t" + ref[0:1] + b"\tT\t60\t.\t.\tGT\t0|1\t1\n")
    last = tmp_path / "last.vcf"
    last.write_bytes(hdr + b"chr\t%d\t.\t" % len(ref) + ref[-1:] + b"\tG\t60\t.\t.\tGT\t0|1\t1\n")
    for path, phrase in ((first, "first base of the contig"), (last, "last base of the contig")):
        v = H.VcfGraph(str(path), str(fa))
        gt, ploidy = v.parse_gt()
        with pytest.raises(H.HostError) as e:
            v.build(gt, ploidy)
        assert phrase in str(e.value) and e.value.status == -4
    two = tmp_path / "two.fa"
    two.write_bytes(b">chr\n" + ref + b"\n>chr2\nACGT\n")
    with pytest.raises(H.HostError) as e:
        H.VcfGraph(str(vcf), str(two))
    assert "more than one record" in str(e.value)
    with pytest.raises(H.HostError) as e:
        H.VcfGraph(str(tmp_path / "missing.vcf"), str(fa))
    assert e.value.status == -1
    few = tmp_path / "few.vcf"
    few.write_bytes(hdr + b"chr\t11\t.\t" + ref[10:11] + b"\tT\t60\t.\t.\tGT\t0|1\n")          # ten columns, the header names eleven
    parts = tmp_path / "parts.vcf"
    parts.write_bytes(hdr + b"chr\t11\t.\t" + ref[10:11] + b"\tT\t60\t.\t.\tDP:GT\t3:0|1\t7\n")  # H's field has no second part
    for path in (few, parts):
        v = H.VcfGraph(str(path), str(fa))
        with pytest.raises(H.HostError):
            v.parse_gt()
    badpos = tmp_path / "badpos.vcf"
    badpos.write_bytes(hdr + b"chr\tx\t.\tA\tT\t60\t.\t.\tGT\t0|1\t1\n")
    with pytest.raises(H.HostError):
        H.VcfGraph(str(badpos), str(fa))
    # gzip and block gzip inputs give the records of the plain file
    import gzip
    (tmp_path / "v.vcf.gz").write_bytes(gzip.compress(vcf.read_bytes()))
    (tmp_path / "r.fa.gz").write_bytes(gzip.compress(fa.read_bytes()))
    a, b = H.VcfGraph(str(vcf), str(fa)), H.VcfGraph(str(tmp_path / "v.vcf.gz"), str(tmp_path / "r.fa.gz"))
    assert a.text.tobytes() == b.text.tobytes() and a.rec_start.tolist() == b.rec_start.tolist() and a.ref_seq.tobytes() == b.ref_seq.tobytes() == ref


def _py_field(field, gi):
    """vcf2gfa.read_vcf's lines for one sample field."""
    g = field.split(b":")[gi].replace(b"/", b"|").split(b"|")
    ploidy = min(2, sum(1 for x in g if x != b"."))
    g = [int(x) if x.isdigit() else 0 for x in g] + [0, 0]
    return (g[0], g[1]), ploidy


def test_scalar_genotype_parser_on_hand_written_fields(built):
    from phi_amd import ilp_index as H
    want = {b"0|1": ((0, 1), 2), b"1/0": ((1, 0), 2), b".": ((0, 0), 0), b".|.": ((0, 0), 0), b"1": ((1, 0), 1), b"10|2": ((10, 2), 2),
            b"0|1|2": ((0, 1), 2), b"a|1": ((0, 1), 2), b"": ((0, 0), 1), b".|3": ((0, 3), 1), b"7|": ((7, 0), 2), b"65534|65536": ((65534, 65535), 2),
            b"12345678901234567890": ((65535, 0), 1), b"1x|+2": ((0, 0), 2)}
    for field, (gt_want, pl_want) in want.items():
        py_gt, py_pl = _py_field(field, 0)
        assert (tuple(min(x, 65535) for x in py_gt), py_pl) == (gt_want, pl_want), field      # the table is the Python's
        gt, ploidy = H.parse_gt(field + b"\n", [0, len(field) + 1], [0], 1)
        assert (tuple(gt[0, 0].tolist()), int(ploidy[0])) == (gt_want, pl_want), field
    # GT second in FORMAT; every field shape in one record, each sample's ploidy its own; a CR LF line end is stripped by the reader
    fields = list(want)
    gt, ploidy = H.parse_gt(b"\t".join(fields) + b"\n", [0, sum(len(f) + 1 for f in fields)], [0], len(fields))
    assert [tuple(x) for x in gt[0].tolist()] == [want[f][0] for f in fields] and ploidy.tolist() == [want[f][1] for f in fields]
    gt, ploidy = H.parse_gt(b"35:0|1:PASS\t.:1/2\n", [0, 18], [1], 2)
    assert gt[0].tolist() == [[0, 1], [1, 2]] and ploidy.tolist() == [2, 2]
    with pytest.raises(H.HostError):
        H.parse_gt(b"35:0|1:PASS\t7\n", [0, 14], [1], 2)
    with pytest.raises(H.HostError):
        H.parse_gt(b"0|1\n", [0, 4], [0], 2)
    # ploidy is a maximum over records; more fields than samples are ignored
    gt, ploidy = H.parse_gt(b"1\t.|.\t9\n0|1\t.\n", [0, 8, 14], [0, 0], 2)
    assert gt.tolist() == [[[1, 0], [0, 0]], [[0, 1], [0, 0]]] and ploidy.tolist() == [2, 0]


def test_reader_strips_cr_lf_and_takes_gt_where_format_puts_it(built, tmp_path):
    from phi_amd import ilp_index as H
    ref = b"ACGTTGCAAGGCTTAACCGGATCGATCGGCTAAGCTTAGGCTA" * 2
    fa = tmp_path / "r.fa"
    fa.write_bytes(b">chr desc\r\n" + ref[:30] + b"\r\n" + ref[30:] + b"\r\n")
    vcf = tmp_path / "v.vcf"
    vcf.write_bytes(b"##x\r\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\r\n"
                    b"chr\t31\t.\t" + ref[30:32] + b"\tT,TTT\t60\t.\t.\tDP:GT:FT\t35:0|2:PASS\t.:1/0:x\r\n"
                    b"chr\t11\t.\t" + ref[10:11] + b"\tg\t60\t.\t.\tGT\t1|0\t.|.")                # sorted in front; lower-case ALT; no final line feed
    want = _check_against_python(str(vcf), str(fa), tmp_path)
    assert want["samples"] == ["A", "B"] and [r[0] for r in want["recs"]] == [10, 30]
    v = H.VcfGraph(str(vcf), str(fa))
    assert v.text.tobytes() == b"1|0\t.|.\n35:0|2:PASS\t.:1/0:x\n" and v.gt_index.tolist() == [0, 1] and v.alts(0) == [b"G"]


def test_host_side_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """phi_amd/csrc/host/vcf_selftest.cpp: reader, scalar parser and builder over a generated VCF, a truncated last line, a line
    with too few sample columns and a zero-length file, in a stand-alone program built with -fsanitize=address,undefined."""
    subprocess.check_call(["make", "-C", HOSTDIR, "-s", "vcf_sanitize"])
    exe = os.path.join(ROOT, "build", "sanitize", "vcf_selftest_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.split(" ", 1) for l in r.stdout.splitlines())
    assert lines["full"].startswith("ok ") and lines["empty"].startswith("ok ") and lines["cut_fixed"].startswith("ok ")
    assert lines["cut"] == "error -4" and lines["few"] == "error -4" and lines["two_records"] == "error -4" and lines["missing"] == "error -1"
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
