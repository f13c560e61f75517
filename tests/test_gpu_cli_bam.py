"""`PHI -r reads.bam`: the FASTA bytes and the scraped log lines of `PHI -r reads.fq` for the FASTQ that tests/bam_util.py writes
of the same reads -- on the toy graph and on MHC_4, through the park, under --coverage, with two read sets in one command --
under --panels -- and the refusals: several GPUs with a BAM, CRAM, SAM text, a truncated BAM.  Reads that come through a FIFO
are text as they always were: nothing is consumed from a pipe to find out what it holds.  Also the Python mirror's reads entry."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bam_util as B
from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

PHI = os.path.join(ROOT, "phi_amd", "PHI")
TOY_GFA = os.path.join(DATA, "test.gfa")
MHC_GFA = os.path.join(DATA, "MHC_4.gfa.gz")
TOY = ["-k3", "-w2", "-q0", "-m0", "-R", "10"]


def _run_cli(args, cwd, env=None):
    if not os.path.exists(PHI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host")])
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([PHI] + args, capture_output=True, text=True, cwd=str(cwd), timeout=300, env=e)


def _lines(log):
    """The log without its stamps and without what names the run: every line the reference's scripts scrape is among them."""
    return [re.sub(r"^\[M::[^\]]*\] ", "", l) for l in log.splitlines()
            if not (l.startswith("[phi timing]") or "Real time" in l or "CMD:" in l or "written to" in l or l.startswith("[M::main] BAM "))]


def _fasta_reads(text):
    recs = []
    for ln in text.decode().split("\n"):
        if ln.startswith(">"):
            recs.append(b"")
        elif ln:
            recs[-1] += ln.encode()
    return recs


def _write_pair(d, stem, reads, block_bytes=0xFF00, extra=()):
    """stem.bam and stem.fq of the same reads in directory d: every third read stored reverse-complemented with 0x10, records
    that give no read (`extra`) in between.  Both give the output the name `stem`."""
    recs = []
    for i, r in enumerate(reads):
        recs.append(B.record(b"q%d" % i, B.revcomp(r), flag=0x10 | 4) if i % 3 == 0 else B.record(b"q%d" % i, r, flag=4))
        if i % 5 == 0:
            recs.extend(extra)
    bam = B.header(b"@HD\tVN:1.6\tSO:unsorted\n") + b"".join(recs)
    assert B.decode(bam)[0] == list(reads)
    B.write_bam(str(d / (stem + ".bam")), bam, block_bytes)
    (d / (stem + ".fq")).write_bytes(B.fastq(reads))
    return bam


def _many_reads():
    rng = np.random.default_rng(5)
    base = b"ATCGATCATACTTACCATG"
    out = []
    for i in range(60):
        if i % 3 == 0:
            out.append(bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(5, 40))).tolist()))
        else:
            a = int(rng.integers(0, 8))
            out.append(base[a:a + int(rng.integers(6, 19))])
    return out


NO_READ = (B.record(b"sec", b"ACGTACGT", flag=0x100), B.record(b"sup", b"ACGT", flag=0x800 | 0x10), B.record(b"none", b"", flag=4))


def _same_run(tmp_path, gfa, stem, opts, env=None, bam_env=None):
    a = _run_cli(["-g", gfa, "-r", stem + ".fq", "-o", "fq.fa"] + opts, tmp_path, env)
    b = _run_cli(["-g", gfa, "-r", stem + ".bam", "-o", "bam.fa"] + opts, tmp_path, dict(env or {}, **(bam_env or {})))
    assert a.returncode == 0 and b.returncode == 0, a.stderr[-2000:] + b.stderr[-2000:]
    assert (tmp_path / "fq.fa").read_bytes() == (tmp_path / "bam.fa").read_bytes()
    assert _lines(a.stderr) == _lines(b.stderr)
    assert any("read has" in l for l in _lines(b.stderr)) and any("Indexed reads with spectrum size" in l for l in _lines(b.stderr))
    return a, b


def test_cli_toy_bam_equals_its_fastq(tmp_path):
    reads = _fasta_reads(open(os.path.join(DATA, "read.fa"), "rb").read())
    _write_pair(tmp_path, "x", reads, extra=NO_READ)
    a, b = _same_run(tmp_path, TOY_GFA, "x", TOY)
    m = re.search(r"\[M::main\] BAM x\.bam: (\d+) records, (\d+) reads kept \((\d+) stored reverse\), (\d+) secondary/supplementary and (\d+) without sequence dropped", b.stderr)
    n = len(reads)
    k = len(range(0, n, 5))
    assert m and [int(x) for x in m.groups()] == [n + 3 * k, n, len(range(0, n, 3)), 2 * k, k], b.stderr
    assert "BAM " not in a.stderr
    # more reads, BGZF blocks of 100 bytes (records straddle them), tiles of 64 bytes
    _write_pair(tmp_path, "many", _many_reads(), block_bytes=100, extra=NO_READ)
    _same_run(tmp_path, TOY_GFA, "many", TOY, bam_env={"PHI_BAM_TILE": "64", "PHI_READ_CHUNK": "300"})


@pytest.fixture(scope="module")
def mhc_reads():
    from phi_amd import ilp_index as H
    bases, off, _ = H.read_reads(os.path.join(DATA, "CHM13_reads.fq.gz"))
    raw = bytes(bases)
    return [raw[off[i]:off[i + 1]] for i in range(0, 16401, 2)][:7000]


def test_cli_mhc4_bam_equals_its_fastq_also_through_the_park(tmp_path, mhc_reads):
    _write_pair(tmp_path, "mhc", mhc_reads, extra=NO_READ[:1])
    env = {"PHI_TIMING": "1", "PHI_READ_CHUNK": "100000"}
    a, b = _same_run(tmp_path, MHC_GFA, "mhc", ["-t8"], env=dict(env, PHI_TEXT_PARK="0"))
    assert "waited in device memory" not in b.stderr
    assert f"read has {len(mhc_reads)} reads" in b.stderr
    p = _run_cli(["-t8", "-g", MHC_GFA, "-r", "mhc.bam", "-o", "parked.fa"], tmp_path, dict(env, PHI_TEXT_PARK_MIN="1"))
    assert p.returncode == 0, p.stderr[-2000:]
    m = re.search(r"main: (\d+) bytes of the reads text waited in device memory for the index", p.stderr)
    assert m and int(m.group(1)) >= 500_000, p.stderr[-2000:]
    assert _lines(p.stderr) == _lines(b.stderr)
    assert (tmp_path / "parked.fa").read_text().split("\n")[1:] == (tmp_path / "bam.fa").read_text().split("\n")[1:]
    # the BAM as ONE gzip stream (not BGZF): the device inflater's route, its text parked in pieces
    bam = gzip.decompress((tmp_path / "mhc.bam").read_bytes())
    (tmp_path / "single.bam").write_bytes(gzip.compress(bam, 1))
    s = _run_cli(["-t8", "-g", MHC_GFA, "-r", "single.bam", "-o", "single.fa"], tmp_path, dict(env, PHI_INFLATE_MIN="1"))
    assert s.returncode == 0, s.stderr[-2000:]
    assert "inflated on the device" in s.stderr
    assert (tmp_path / "single.fa").read_text().split("\n")[1:] == (tmp_path / "bam.fa").read_text().split("\n")[1:]


def test_cli_coverage_over_a_bam_equals_coverage_over_its_fastq(tmp_path):
    reads = _many_reads()
    _write_pair(tmp_path, "many", reads, extra=NO_READ)          # (dropped records get no ordinal: the draws follow the kept reads)
    total = sum(map(len, reads))
    outs = {}
    for kind in ("fq", "bam"):
        d = tmp_path / kind
        d.mkdir()
        r = _run_cli(["--coverage", "0.5,1,2", "--genome-size", str(total // 2), "--seed", "3", "-g", TOY_GFA, "-r", str(tmp_path / ("many." + kind)),
                      "-o", "out.{cov}x.fa"] + TOY, d)
        assert r.returncode == 0, r.stderr
        outs[kind] = ([(d / f"out.{c}x.fa").read_bytes() for c in ("0.5", "1", "2")], _lines(r.stderr))
    assert outs["fq"][0] == outs["bam"][0]
    assert outs["fq"][1] == outs["bam"][1]
    assert sum(l.startswith("Coverage ") for l in outs["bam"][1]) == 3


def test_cli_two_read_sets_one_bam_and_one_fastq(tmp_path):
    reads = _many_reads()
    _write_pair(tmp_path, "a", reads[:30], extra=NO_READ)
    _write_pair(tmp_path, "b", reads[30:])
    both = _run_cli(["-g", TOY_GFA, "-r", "a.bam", "-o", "a.fa", "-r", "b.fq", "-o", "b.fa"] + TOY, tmp_path)
    assert both.returncode == 0, both.stderr
    for stem, kind in (("a", "fq"), ("b", "bam")):               # each against a run of its own, from the other format
        one = _run_cli(["-g", TOY_GFA, "-r", f"{stem}.{kind}", "-o", f"{stem}_alone.fa"] + TOY, tmp_path)
        assert one.returncode == 0, one.stderr
        assert (tmp_path / f"{stem}.fa").read_bytes() == (tmp_path / f"{stem}_alone.fa").read_bytes()
    assert both.stderr.count("[M::main] BAM a.bam:") == 1 and "BAM b.fq" not in both.stderr


def test_cli_panels_over_a_bam_equal_panels_over_its_fastq(tmp_path):
    from graphgen import mosaic_reads, random_graph
    from test_cpu_panel import gfa_text
    rng = np.random.default_rng(507)
    g = random_graph(rng, n_sites=40, n_walks=6, seg_len=(1, 400), alt_len=(1, 40), p_del=0.3)
    g.hap_names = ["hap0.1", "hap0.2", "hap1.1", "hap2.1", "hap3.1", "hap4.1"]
    reads = [bytes(r) for r in mosaic_reads(rng, g, n_reads=200, read_len=100, n_seg=2, err=0.005)]
    (tmp_path / "g.gfa").write_text(gfa_text(g))
    _write_pair(tmp_path, "reads", reads, extra=NO_READ)
    outs = {}
    for kind in ("fq", "bam"):
        d = tmp_path / kind
        d.mkdir()
        r = _run_cli(["--panels", "2,4", "--panel-seed", "1", "-g", str(tmp_path / "g.gfa"), "-r", str(tmp_path / ("reads." + kind)), "-o", "out.{panel}.fa", "-R", "30"], d)
        assert r.returncode == 0, r.stderr
        outs[kind] = ([(d / f"out.{n}.fa").read_bytes() for n in ("2", "4")], _lines(r.stderr))
    assert outs["fq"][0] == outs["bam"][0] and outs["fq"][0][0] != outs["fq"][0][1]
    assert outs["fq"][1] == outs["bam"][1]
    assert sum(l.startswith("Panel: kept ") for l in outs["bam"][1]) == 2


def test_cli_reads_through_a_fifo_stay_text(tmp_path):
    """-r <(samtools fastq x.bam), the way around before BAM was read: the FASTQ arrives through a FIFO whose writer sees every
    byte taken exactly once -- the kind of a reads file is decided from regular files only."""
    import threading
    reads = _many_reads()
    fq = B.fastq(reads)
    (tmp_path / "file").mkdir()
    (tmp_path / "pipe").mkdir()
    (tmp_path / "file" / "x.fq").write_bytes(fq)
    fifo = tmp_path / "pipe" / "x.fq"
    os.mkfifo(str(fifo))
    state = {}

    def writer():
        try:
            with open(str(fifo), "wb") as f:                   # (blocks until the one reader opens)
                f.write(fq)
            state["ok"] = True
        except OSError as e:                                   # EPIPE: somebody opened, read a little and closed
            state["err"] = e
    t = threading.Thread(target=writer, daemon=True)
    t.start()
    a = _run_cli(["-g", TOY_GFA, "-r", str(fifo), "-o", "pipe.fa"] + TOY, tmp_path)
    t.join(10)
    assert not t.is_alive() and state.get("ok"), state
    b = _run_cli(["-g", TOY_GFA, "-r", str(tmp_path / "file" / "x.fq"), "-o", "file.fa"] + TOY, tmp_path)
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert (tmp_path / "pipe.fa").read_bytes() == (tmp_path / "file.fa").read_bytes()
    assert _lines(a.stderr) == _lines(b.stderr) and f"read has {len(reads)} reads" in a.stderr


def test_cli_refusals(tmp_path):
    reads = _many_reads()
    bam = _write_pair(tmp_path, "x", reads)
    r = _run_cli(["-g", TOY_GFA, "-r", "x.bam", "-o", "o.fa", "--devices", "0,0"] + TOY, tmp_path, {"PHI_ALLOW_SAME_DEVICE": "1"})
    assert r.returncode == 1 and "BAM" in r.stderr and "one GPU" in r.stderr and not (tmp_path / "o.fa").exists(), r.stderr
    (tmp_path / "c.cram").write_bytes(b"CRAM\x03\x00" + bytes(200))
    r = _run_cli(["-g", TOY_GFA, "-r", "c.cram", "-o", "o.fa"] + TOY, tmp_path)
    assert r.returncode == 1 and "CRAM" in r.stderr and not (tmp_path / "o.fa").exists(), r.stderr
    (tmp_path / "s.sam").write_bytes(b"@HD\tVN:1.6\tSO:unsorted\nq0\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n")
    r = _run_cli(["-g", TOY_GFA, "-r", "s.sam", "-o", "o.fa"] + TOY, tmp_path)
    assert r.returncode == 1 and "SAM text" in r.stderr and not (tmp_path / "o.fa").exists(), r.stderr
    # a FASTQ whose first read is merely NAMED like a SAM header tag is text, as it always was
    (tmp_path / "hd.fq").write_bytes(b"@HD\tsome read\nATCGATCATACTTACCATG\n+\nIIIIIIIIIIIIIIIIIII\n")
    r = _run_cli(["-g", TOY_GFA, "-r", "hd.fq", "-o", "hd.fa"] + TOY, tmp_path)
    assert r.returncode == 0 and "read has 1 reads" in r.stderr and (tmp_path / "hd.fa").exists(), r.stderr
    # a BAM whose inflated stream ends inside a record, and one that ends inside its header
    cut = len(bam) - 17
    with pytest.raises(B.BamInvalid) as e:
        B.decode(bam[:cut])
    B.write_bam(str(tmp_path / "cut.bam"), bam[:cut])
    r = _run_cli(["-g", TOY_GFA, "-r", "cut.bam", "-o", "o.fa"] + TOY, tmp_path)
    assert r.returncode == 1 and "ends inside the record" in r.stderr and f"byte offset {e.value.offset} " in r.stderr, r.stderr
    B.write_bam(str(tmp_path / "hdr.bam"), bam[:9])
    r = _run_cli(["-g", TOY_GFA, "-r", "hdr.bam", "-o", "o.fa"] + TOY, tmp_path)
    assert r.returncode == 1 and "ends inside its header" in r.stderr and not (tmp_path / "o.fa").exists(), r.stderr


def test_python_mirror_takes_a_bam_path(tmp_path):
    import io
    from phi_amd import ilp_index as H
    reads = _many_reads()
    _write_pair(tmp_path, "x", reads, extra=NO_READ)
    outs = {}
    for kind in ("fq", "bam"):
        log = io.StringIO()
        idx = H.ILP_index(TOY_GFA, log=log)
        idx.read_gfa()
        idx.k_mer, idx.window, idx.recombination, idx.is_qclp, idx.is_mixed = 3, 2, 10, 0, False
        idx.hap_file, idx.hap_name = str(tmp_path / f"py_{kind}.fa"), "x"
        ip = []
        idx.read_ip_reads(ip, str(tmp_path / ("x." + kind)))
        assert (len(ip) == 1 and isinstance(ip[0], H.BamReads)) if kind == "bam" else len(ip) == len(reads)
        res = idx.ILP_function(ip)
        outs[kind] = (res["objective"], res["spectrum_size"], res["path_vtx"].tolist(), open(idx.hap_file, "rb").read())
        assert f"read has {len(reads)} reads" in log.getvalue()
    assert outs["fq"] == outs["bam"]
