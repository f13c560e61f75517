"""`PHI --panel-auto N [--panel-blocks B] [--panel-always NAME,..]`: the panel chosen from the reads on the command line, against
`PHI --keep-samples <the chosen names>` on the same files: FASTA bytes and the scraped log counters are equal.  With -g (1 100
W-lines), with several read sets in one command, with --chop, with --vcf / --ref (1 201 haplotypes, the planted case of
test_gpu_panel_auto), with a graph of no more walks than asked for, and the refused option pairs."""
import re

import numpy as np
import pytest

from graphgen import mosaic_reads
from test_gpu_chop import _counter_lines, _run_cli, _write_gfa
from test_gpu_panel_auto import PLANT_BLOCKS, PLANT_K, PLANT_W, _graph, _planted, _reads

pytestmark = pytest.mark.gpu

AUTO_LINE = re.compile(r"Panel \(from the reads\): kept (\d+) of (\d+) walks in (\d+) rounds over (\d+) blocks: (\S+)$", re.M)
PANEL_LINE = re.compile(r"Panel: kept (\d+) of (\d+) walks")
KW = ["-k", "15", "-w", "5", "-R", "30"]


def _fasta(path, reads):
    path.write_text("".join(f">r{i}\n{r.decode()}\n" for i, r in enumerate(reads)))
    return str(path)


def _files(tmp_path):
    g = _graph("many")
    full = _write_gfa(g, tmp_path / "g.gfa")
    return g, full, _fasta(tmp_path / "a.fa", _reads("many", 0)), _fasta(tmp_path / "b.fa", _reads("many", 1))


def _same_as_keep_samples(tmp_path, log, fasta, names, full, rd, tag, extra=()):
    """the --keep-samples command with the chosen names gives the same FASTA and counters (a walk's sample is its name's head)"""
    out = tmp_path / f"{tag}.keep.fasta"
    r = _run_cli(["--keep-samples", ",".join(n.rsplit(".", 1)[0] for n in names), "-g", full, "-r", rd, "-o", str(out)] + KW + list(extra), tmp_path)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == fasta and len(fasta) > 100
    assert _counter_lines(log) == _counter_lines(r.stderr) and len(_counter_lines(log)) > 2 * len(names)
    rec = [ln for ln in log.splitlines() if ln.startswith("Recombined haplotypes")]
    assert rec and rec == [ln for ln in r.stderr.splitlines() if ln.startswith("Recombined haplotypes")]


@pytest.mark.parametrize("chop", [None, 30])
def test_panel_auto_equals_keep_samples_with_the_chosen_names(tmp_path, chop):
    g, full, rd_a, rd_b = _files(tmp_path)
    extra = ["--chop", str(chop)] if chop else []
    out = tmp_path / "auto.fasta"
    r = _run_cli(["--panel-auto", "40", "-g", full, "-r", rd_a, "-o", str(out)] + KW + extra, tmp_path)
    assert r.returncode == 0, r.stderr
    m = AUTO_LINE.search(r.stderr)
    assert m and (int(m.group(1)), int(m.group(2))) == (40, 1100) and int(m.group(3)) >= 1 and int(m.group(4)) == 1
    names = m.group(5).split(",")
    assert len(names) == 40 and set(names) <= set(g.hap_names)
    # the usual line follows it
    assert r.stderr.index("Panel (from the reads)") < PANEL_LINE.search(r.stderr).start()
    assert PANEL_LINE.search(r.stderr).groups() == ("40", "1100")
    _same_as_keep_samples(tmp_path, r.stderr, out.read_bytes(), names, full, rd_a, "a", extra)


def test_several_read_sets_blocks_and_always(tmp_path):
    """two read sets in one command: the scout is rebuilt from the retained entries, every set gets its own panel;
    --panel-blocks and --panel-always reach the choice"""
    g, full, rd_a, rd_b = _files(tmp_path)
    oa, ob = tmp_path / "oa.fasta", tmp_path / "ob.fasta"
    r = _run_cli(["--panel-auto", "24", "--panel-blocks", "7", "--panel-always", "hap1099,hap3", "-g", full, "-r", rd_a, "-o", str(oa), "-r", rd_b, "-o", str(ob)] + KW,
                 tmp_path)
    assert r.returncode == 0, r.stderr
    ms = list(AUTO_LINE.finditer(r.stderr))
    assert len(ms) == 2 and all(int(m.group(1)) == 24 and int(m.group(4)) == 7 for m in ms)
    parts = re.split(r"(?=^.*Panel \(from the reads\))", r.stderr, flags=re.M)[1:]
    assert len(parts) == 2
    chosen = [m.group(5).split(",") for m in ms]
    assert chosen[0] != chosen[1]                               # other reads, another panel
    for names, part, fa, rd, tag in zip(chosen, parts, (oa, ob), (rd_a, rd_b), "ab"):
        assert "hap3.3" in names and "hap1099.1099" in names
        _same_as_keep_samples(tmp_path, part, fa.read_bytes(), names, full, rd, tag)


def test_panel_auto_from_a_vcf(tmp_path):
    vcf, fa, reads, mosaic, _ = _planted(str(tmp_path))
    rd = _fasta(tmp_path / "reads.fa", reads)
    out = tmp_path / "v.fasta"
    args = ["--vcf", vcf, "--ref", fa, "-r", rd, "-o", str(out), "-k", str(PLANT_K), "-w", str(PLANT_W), "-R", "2"]
    r = _run_cli(args, tmp_path)                                # the plain route is still refused
    assert r.returncode == 1 and "more than 1022 walks" in r.stderr
    r = _run_cli(["--panel-auto", "32", "--panel-blocks", str(PLANT_BLOCKS)] + args, tmp_path)
    assert r.returncode == 0, r.stderr
    m = AUTO_LINE.search(r.stderr)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(4))) == (32, 1201, PLANT_BLOCKS)
    names = m.group(5).split(",")
    assert "S0.1" in names and "S1.2" in names, names          # the two truth haplotypes
    seq = "".join(out.read_text().splitlines()[1:]).encode()
    assert seq == mosaic


def test_no_more_walks_than_asked_for_and_refusals(tmp_path):
    g, full, rd_a, rd_b = _files(tmp_path)
    # a panel as large as the graph: the ordinary route, and it says so
    from graphgen import random_graph
    rng = np.random.default_rng(3)
    small = random_graph(rng, n_sites=8, n_walks=6, seg_len=(20, 90), alt_len=(1, 6))
    (tmp_path / "s").mkdir()
    sg = _write_gfa(small, tmp_path / "s" / "g.gfa")
    rd = _fasta(tmp_path / "s.fa", mosaic_reads(rng, small, n_reads=60, read_len=60, n_seg=2))
    o1, o2 = tmp_path / "s1.fasta", tmp_path / "s2.fasta"
    r1 = _run_cli(["--panel-auto", "6", "-g", sg, "-r", rd, "-o", str(o1)] + KW, tmp_path)
    r2 = _run_cli(["-g", sg, "-r", rd, "-o", str(o2)] + KW, tmp_path)
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
    assert "the ordinary route" in r1.stderr and "Panel" not in r1.stderr.replace("--panel-auto", "")
    assert o1.read_bytes() == o2.read_bytes() and _counter_lines(r1.stderr) == _counter_lines(r2.stderr)
    # the refused pairs: exit 1, a plain message, nothing written
    out = tmp_path / "never.fasta"
    base = ["-g", full, "-r", rd_a, "-o", str(out)] + KW
    for extra, word in ((["--panels", "2"], "--panels"), (["--keep-samples", "hap1"], "--keep-samples"), (["--drop-samples", "hap1"], "--drop-samples"),
                        (["--coverage", "1", "--genome-size", "1000"], "--coverage"), (["--devices", "0,1"], "--devices")):
        r = _run_cli(["--panel-auto", "40"] + extra + base, tmp_path)
        assert r.returncode == 1 and "--panel-auto" in r.stderr and word in r.stderr, r.stderr
        assert not out.exists()
    for bad in (["--panel-auto", "0"], ["--panel-auto", "1023"], ["--panel-blocks", "7"], ["--panel-auto", "40", "--panel-always", "nobody"]):
        r = _run_cli(bad + base, tmp_path)
        assert r.returncode == 1 and "[E::main]" in r.stderr and not out.exists(), r.stderr
