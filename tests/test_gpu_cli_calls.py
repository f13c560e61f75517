"""`PHI --calls FILE [--calls-ref NAME] [--calls-contig NAME]`: the inferred haplotype written as variant calls against a
reference walk.  Every file is read back: header, ascending POS, no REF = ALT record, REF equal to the reference at POS, and the
consensus of the records over the logged span equal to the FASTA the same command wrote."""
import gzip
import os
import re

import numpy as np
import pytest

from conftest import DATA
from graphgen import mosaic_reads, random_graph, walk_sequence
from test_cpu_panel import gfa_text
from test_gpu_chop import _run_cli

pytestmark = pytest.mark.gpu

CALLS_LINE = re.compile(r"Calls: (\d+) written to (\S+), (\d+) dropped as REF = ALT; called span \[(\d+),(\d+)\) of (\S+) \((\d+) bases\), \[(\d+),(\d+)\) of the haplotype")


def _fasta(path):
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "rb") as f:
        lines = f.read().split(b"\n")
    return lines[0][1:].split()[0].decode(), b"".join(lines[1:])


def _check(log, vcf_path, fa_path, ref_seq, contig, contig_len, min_records=1):
    """the log's Calls line for vcf_path and the file itself; returns (records, dropped, INFO strings)"""
    from phi_amd.calls import apply, read_vcf
    m = [m for m in CALLS_LINE.finditer(log) if m.group(2) == str(vcf_path)]
    assert len(m) == 1, log[-2000:]
    n_written, n_dropped, r0, r1, ref_bases, q0, q1 = (int(m[0].group(i)) for i in (1, 3, 4, 5, 7, 8, 9))
    name, hap = _fasta(fa_path)
    header, sample, calls, infos = read_vcf(vcf_path)
    assert header[0] == "##fileformat=VCFv4.2" and header[1].startswith("##source=")
    assert header[2] == f"##contig=<ID={contig},length={contig_len}>"
    assert header[3].startswith("##INFO=<ID=PH,Number=1,Type=String,") and header[4].startswith("##FORMAT=<ID=GT,Number=1,Type=String,")
    assert header[5] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + name and len(header) == 6 and sample == name
    with open(vcf_path) as f:
        for ln in f:
            if not ln.startswith("#"):
                c = ln.rstrip("\n").split("\t")
                assert len(c) == 10 and c[0] == contig and c[2] == "." and c[5] == "." and c[6] == "PASS" and c[8] == "GT" and c[9] == "1"
                assert c[3] != c[4] and c[3] and c[4] and c[7].startswith("PH=")
    n = len(calls["pos"])
    assert n == n_written >= min_records and n_dropped >= 0
    assert np.all(np.diff(calls["pos"]) > 0)
    assert ref_bases == len(ref_seq) and 0 <= r0 < r1 <= ref_bases and 0 <= q0 < q1 <= len(hap)
    # apply() checks REF against the reference at every POS and that no two records overlap
    assert apply(ref_seq, calls, span=(r0, r1)) == hap[q0:q1]
    return n, n_dropped, infos


@pytest.fixture(scope="module")
def mhc(tmp_path_factory):
    """MHC_4 and reads tiled from its walk HG002.1: a path that is not the reference walk of the VCF route"""
    from phi_amd import ilp_index as H
    tmp = tmp_path_factory.mktemp("cli_calls")
    g = H.Graph(os.path.join(DATA, "MHC_4.gfa.gz"))
    flat, vlen = np.frombuffer(bytes(g.seq_concat), np.uint8), np.diff(g.seq_off)
    seqs = {}
    for h, name in enumerate(g.hap_id2name):
        wv = np.asarray(g.walk_vtx[g.walk_off[h]:g.walk_off[h + 1]])
        base = np.concatenate([[0], np.cumsum(vlen[wv])])
        seqs[name] = flat[np.repeat(g.seq_off[wv] - base[:-1], vlen[wv]) + np.arange(base[-1])].tobytes()
    s = seqs["HG002.1"].upper()
    rd = tmp / "hg002_reads.fa"
    with open(rd, "wb") as f:
        f.write(b"".join(b">r%d\n%s\n" % (i, s[a:a + 150]) for i, a in enumerate(range(0, len(s) - 150, 100))))
    return dict(tmp=tmp, seqs=seqs, reads=str(rd), gfa=os.path.join(DATA, "MHC_4.gfa.gz"), vcf=os.path.join(DATA, "MHC_4.vcf.gz"),
                fa=os.path.join(DATA, "MHC-CHM13.0.fa.gz"))


def test_vcf_route(mhc):
    tmp = mhc["tmp"]
    out, vcf = tmp / "v.fa", tmp / "v.vcf"
    r = _run_cli(["--vcf", mhc["vcf"], "--ref", mhc["fa"], "-r", mhc["reads"], "-o", str(out), "--calls", str(vcf), "--drop-samples", "HG005"], tmp,
                 env={"PHI_TIMING": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    _, ref = _fasta(mhc["fa"])
    with gzip.open(mhc["vcf"], "rt") as f:
        contig = next(ln for ln in f if not ln.startswith("#")).split("\t")[0]
    n, _, infos = _check(r.stderr, vcf, out, ref, contig, len(ref), min_records=1000)
    assert set(infos) <= {"PH=REF.0", "PH=HG002.1", "PH=HG002.2"} and "PH=HG002.1" in infos
    assert re.search(r"stage calls \(device\) \+ VCF write", r.stderr) and re.search(r"stage FASTA write", r.stderr)


def test_gfa_route(mhc):
    tmp = mhc["tmp"]
    out, vcf = tmp / "g.fa", tmp / "g.vcf"
    reads = os.path.join(DATA, "CHM13_reads.fq.gz")
    r = _run_cli(["-g", mhc["gfa"], "-r", reads, "-o", str(out), "--calls", str(vcf), "--calls-ref", "HG002.1"], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    ref = mhc["seqs"]["HG002.1"]
    _check(r.stderr, vcf, out, ref, "HG002.1", len(ref), min_records=1000)
    # --calls-contig names the contig; the length stays the walk's
    vcf2 = tmp / "g2.vcf"
    r = _run_cli(["-g", mhc["gfa"], "-r", reads, "-o", str(out), "--calls", str(vcf2), "--calls-ref", "HG002.1", "--calls-contig", "chr6"], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    _check(r.stderr, vcf2, out, ref, "chr6", len(ref), min_records=1000)
    assert open(vcf).read().replace("HG002.1\t", "chr6\t").replace("ID=HG002.1,", "ID=chr6,") == open(vcf2).read()


def _small(tmp_path):
    rng = np.random.default_rng(507)
    g = random_graph(rng, n_sites=40, n_walks=6, seg_len=(1, 400), alt_len=(1, 40), p_del=0.3)
    g.hap_names = ["hap0.1", "hap0.2", "hap1.1", "hap2.1", "hap3.1", "hap4.1"]
    files = []
    for tag in "ab":
        reads = mosaic_reads(rng, g, n_reads=200, read_len=100, n_seg=2, err=0.005)
        rd = tmp_path / f"reads_{tag}.fa"
        rd.write_text("".join(f">r{i}\n{r.decode()}\n" for i, r in enumerate(reads)))
        files.append(str(rd))
    full = tmp_path / "g.gfa"
    full.write_text(gfa_text(g))
    return g, str(full), files


def test_refusals(tmp_path):
    g, gfa, (ra, rb) = _small(tmp_path)
    base = ["-g", gfa, "-r", ra, "-o", str(tmp_path / "o.fa"), "-R", "30"]
    r = _run_cli(base + ["--calls", str(tmp_path / "o.vcf")], tmp_path)
    assert r.returncode == 1 and "--calls-ref" in r.stderr and "needs" in r.stderr
    r = _run_cli(base + ["--calls", str(tmp_path / "o.vcf"), "--calls-ref", "hap1.1", "--drop-samples", "hap1"], tmp_path)
    assert r.returncode == 1 and "--panel-always" in r.stderr and "does not keep" in r.stderr and not (tmp_path / "o.vcf").exists()
    r = _run_cli(base + ["--calls", str(tmp_path / "o.vcf"), "--calls-ref", "nobody.1"], tmp_path)
    assert r.returncode == 1 and "no walk of that name" in r.stderr
    r = _run_cli(base + ["-r", rb, "-o", str(tmp_path / "p.fa"), "--calls", str(tmp_path / "o.vcf"), "--calls-ref", "hap0.1"], tmp_path)
    assert r.returncode == 1 and "1 --calls but 2 -o" in r.stderr
    r = _run_cli(base + ["--calls", str(tmp_path / "o.vcf.gz"), "--calls-ref", "hap0.1"], tmp_path)
    assert r.returncode == 1 and ".gz" in r.stderr and "deflate" in r.stderr and not (tmp_path / "o.vcf.gz").exists()
    r = _run_cli(base + ["--calls-ref", "hap0.1"], tmp_path)
    assert r.returncode == 1 and "go with --calls" in r.stderr
    r = _run_cli(["-g", gfa, "-r", ra, "-o", str(tmp_path / "o.{panel}.fa"), "--panels", "1,2", "--panel-always", "hap0", "--calls", str(tmp_path / "o.vcf"),
                  "--calls-ref", "hap0.1"], tmp_path)
    assert r.returncode == 1 and "--calls must contain {panel}" in r.stderr


def test_two_read_sets_write_two_files(tmp_path):
    g, gfa, (ra, rb) = _small(tmp_path)
    fa, fb, va, vb = (tmp_path / n for n in ("a.fa", "b.fa", "a.vcf", "b.vcf"))
    r = _run_cli(["-g", gfa, "-R", "30", "--calls-ref", "hap2.1", "-r", ra, "-o", str(fa), "--calls", str(va), "-r", rb, "-o", str(fb), "--calls", str(vb)], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    ref = walk_sequence(g, 3)
    na, _, _ = _check(r.stderr, va, fa, ref, "hap2.1", len(ref))
    nb, _, _ = _check(r.stderr, vb, fb, ref, "hap2.1", len(ref))
    assert fa.read_bytes() != fb.read_bytes() and va.read_bytes() != vb.read_bytes()


def test_one_file_per_panel(tmp_path):
    g, gfa, (ra, _) = _small(tmp_path)
    r = _run_cli(["-g", gfa, "-R", "30", "-r", ra, "-o", str(tmp_path / "o.{panel}.fa"), "--calls", str(tmp_path / "o.{panel}.vcf"), "--calls-ref", "hap0.2",
                  "--panels", "1,3", "--panel-always", "hap0"], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    ref = walk_sequence(g, 1)
    for p in ("1", "3"):
        _, _, infos = _check(r.stderr, tmp_path / f"o.{p}.vcf", tmp_path / f"o.{p}.fa", ref, "hap0.2", len(ref), min_records=0)
        assert all(i[3:] in g.hap_names for i in infos)
