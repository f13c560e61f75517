"""`PHI --bgzf`: every -o and --calls file of the command formatted in memory, compressed into BGZF blocks on the command's device
and written under the name as given.  The compressed files are split and checked member by member (bgzf_util), inflate byte for
byte to what the same command writes without the flag, and the log states their sizes."""
import gzip
import os
import re

import pytest

import bgzf_util
from conftest import DATA
from test_gpu_chop import _run_cli

pytestmark = pytest.mark.gpu

BGZF_LINE = re.compile(r"BGZF: (\d+) bytes written to (\S+), (\d+) bytes of text in (\d+) blocks \((\d+) stored\); ([\d.]+) ms on device (\d+)")
GFA, READS = os.path.join(DATA, "test.gfa"), os.path.join(DATA, "read.fa")
BASE = ["-g", GFA, "-r", READS, "-k", "3", "-w", "2"]


def _logged(log, path):
    """the numbers of the log's BGZF line for path: (output bytes, text bytes, blocks)"""
    m = [m for m in BGZF_LINE.finditer(log) if m.group(2) == str(path)]
    assert len(m) == 1, log[-3000:]
    return int(m[0].group(1)), int(m[0].group(3)), int(m[0].group(4))


def _check_file(log, path, plain):
    data = path.read_bytes()
    assert bgzf_util.text_of(data) == plain and gzip.decompress(data) == plain
    assert _logged(log, path) == (len(data), len(plain), -(-len(plain) // bgzf_util.BLOCK))


def test_compressed_files_inflate_to_the_plain_ones(tmp_path):
    fa, vcf, faz, vcfz = (tmp_path / n for n in ("o.fa", "o.vcf", "o.fa.gz", "o.vcf.gz"))
    plain = _run_cli(BASE + ["-o", str(fa), "--calls", str(vcf), "--calls-ref", "test_hap_1.0"], tmp_path, env={"PHI_TIMING": "1"})
    assert plain.returncode == 0, plain.stderr[-3000:]
    assert "BGZF:" not in plain.stderr
    r = _run_cli(["--bgzf"] + BASE + ["-o", str(faz), "--calls", str(vcfz), "--calls-ref", "test_hap_1.0"], tmp_path, env={"PHI_TIMING": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert fa.read_bytes().startswith(b">test_read LN:") and vcf.read_bytes().startswith(b"##fileformat=VCFv4.2\n")
    _check_file(r.stderr, faz, fa.read_bytes())
    _check_file(r.stderr, vcfz, vcf.read_bytes())
    # the stages keep their names and the Calls line its wording
    for log in (plain.stderr, r.stderr):
        assert re.search(r"stage FASTA write", log) and re.search(r"stage calls \(device\) \+ VCF write", log)
    calls_line = re.compile(r"Calls: (\d+) written to \S+, (\d+) dropped as REF = ALT; called span (.*)")
    assert calls_line.search(plain.stderr).groups() == calls_line.search(r.stderr).groups()
    # the project's own inflater closes the round trip
    import phi_amd
    assert phi_amd.inflate(faz.read_bytes())[0] == fa.read_bytes()
    # Python's writer gives the command line's bytes
    from phi_amd.calls import read_vcf, write_vcf
    header, sample, calls, infos = read_vcf(str(vcf))
    contig, length = re.fullmatch(r"##contig=<ID=(.+),length=(\d+)>", header[2]).groups()
    py = tmp_path / "py.vcf.gz"
    ph = [i[3:] if i.startswith("PH=") else "" for i in infos]
    assert write_vcf(str(py), calls, contig, int(length), sample, ph=ph, bgzf=True) == (len(calls["pos"]), 0)
    assert py.read_bytes() == vcfz.read_bytes()
    # and so does the Python mirror of the command where it writes the FASTA
    import io
    from phi_amd import ilp_index as H
    idx = H.ILP_index(GFA, log=io.StringIO())
    idx.read_gfa()
    idx.k_mer, idx.window, idx.bgzf = 3, 2, True
    idx.hap_file, idx.hap_name = str(tmp_path / "py.fa.gz"), H.get_hap_name(GFA, READS)
    reads = []
    idx.read_ip_reads(reads, READS)
    idx.ILP_function(reads)
    assert (tmp_path / "py.fa.gz").read_bytes() == faz.read_bytes()


def test_names_are_taken_as_given_and_nothing_changes_without_the_flag(tmp_path):
    # --bgzf adds no suffix: a name without .gz holds BGZF all the same
    out = tmp_path / "named.fasta"
    r = _run_cli(["--bgzf"] + BASE + ["-o", str(out)], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("named")) == ["named.fasta"]
    text = bgzf_util.text_of(out.read_bytes())
    assert text.startswith(b">test_read LN:")
    # without it, -o x.fa.gz is text as before and --calls x.vcf.gz is refused before any work
    gz = tmp_path / "plain.fa.gz"
    r = _run_cli(BASE + ["-o", str(gz)], tmp_path)
    assert r.returncode == 0 and gz.read_bytes() == text and "BGZF:" not in r.stderr
    r = _run_cli(BASE + ["-o", str(tmp_path / "r.fa"), "--calls", str(tmp_path / "r.vcf.gz"), "--calls-ref", "test_hap_1.0"], tmp_path)
    assert r.returncode == 1 and ".gz" in r.stderr and "deflate" in r.stderr and "--bgzf" in r.stderr
    assert not (tmp_path / "r.vcf.gz").exists() and not (tmp_path / "r.fa").exists()


def test_one_valid_file_per_panel(tmp_path):
    args = BASE + ["--panels", "1,2", "--panel-always", "test_hap_1", "--calls-ref", "test_hap_1.0"]
    r = _run_cli(args + ["-o", str(tmp_path / "p.{panel}.fa"), "--calls", str(tmp_path / "p.{panel}.vcf")], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    z = _run_cli(["--bgzf"] + args + ["-o", str(tmp_path / "z.{panel}.fa.gz"), "--calls", str(tmp_path / "z.{panel}.vcf.gz")], tmp_path)
    assert z.returncode == 0, z.stderr[-3000:]
    for p in ("1", "2"):
        for ext in ("fa", "vcf"):
            _check_file(z.stderr, tmp_path / f"z.{p}.{ext}.gz", (tmp_path / f"p.{p}.{ext}").read_bytes())
    assert len(BGZF_LINE.findall(z.stderr)) == 4
