"""`PHI --keep-samples / --drop-samples / --panels` (a panel of the graph's haplotypes inside "set graph": data/chop_graph.sh:46-66,
data/run_batch_9.py to run_batch_13.py) against separate plain commands on the reduced GFA files the test writes by text
handling: FASTA bytes and the scraped log counters are equal."""
import os
import re

import numpy as np
import pytest

from graphgen import mosaic_reads, random_graph
from test_cpu_chop import chop_numpy
from test_cpu_panel import gfa_text, reduced_gfa_text
from test_gpu_chop import _counter_lines, _run_cli, _write_gfa

pytestmark = pytest.mark.gpu

PANEL_LINE = re.compile(r"Panel: kept (\d+) of (\d+) walks \((\d+) of (\d+) samples( \+ REF)?\): (\d+) -> (\d+) vertices, (\d+) -> (\d+) edges, (\d+) -> (\d+) walk entries")


def _case(tmp_path):
    """few walks over many sites, so that dropping a sample loses vertices and edges; two walks of one sample"""
    rng = np.random.default_rng(507)
    g = random_graph(rng, n_sites=40, n_walks=6, seg_len=(1, 400), alt_len=(1, 40), p_del=0.3)
    g.hap_names = ["hap0.1", "hap0.2", "hap1.1", "hap2.1", "hap3.1", "hap4.1"]
    reads = mosaic_reads(rng, g, n_reads=200, read_len=100, n_seg=2, err=0.005)
    rd = tmp_path / "reads.fa"
    rd.write_text("".join(f">r{i}\n{r.decode()}\n" for i, r in enumerate(reads)))
    (tmp_path / "full").mkdir()
    full = tmp_path / "full" / "g.gfa"
    full.write_text(gfa_text(g))
    return g, str(full), str(rd)


def _keep_of(g, samples):
    return np.array([n.rsplit(".", 1)[0] in samples for n in g.hap_names])


def _plain(tmp_path, g, keep, tag, rd, chop=None, extra=()):
    """the plain command on the reduced GFA (same file name: the FASTA header is the same); chopped by chop_numpy when asked"""
    from phi_amd.panel import induced_subgraph
    d = tmp_path / tag
    d.mkdir(exist_ok=True)
    if chop is None:
        (d / "g.gfa").write_text(reduced_gfa_text(gfa_text(g), keep))
    else:
        sub, _ = induced_subgraph(g, keep)
        _write_gfa(chop_numpy(sub, chop)[0], d / "g.gfa")
    fa = tmp_path / f"{tag}.fa"
    r = _run_cli(["-g", str(d / "g.gfa"), "-r", rd, "-o", str(fa), "-R", "30"] + list(extra), tmp_path)
    assert r.returncode == 0, r.stderr
    return r, fa.read_bytes()


def _check(log1, fa1, log2, fa2, g, keep, chop=None):
    from phi_amd.panel import induced_subgraph
    assert fa1 == fa2
    assert _counter_lines(log1) == _counter_lines(log2) and len(_counter_lines(log1)) > 2 * int(keep.sum())
    sub, _ = induced_subgraph(g, keep)
    m = PANEL_LINE.search(log1)
    assert m and not PANEL_LINE.search(log2)
    smp = [n.rsplit(".", 1)[0] for n in g.hap_names]
    want = [int(keep.sum()), g.n_walks, len(set(s for s, k in zip(smp, keep) if k)), len(set(smp)), g.n_vtx, sub.n_vtx,
            sum(len(a) for a in g.adj), sum(len(a) for a in sub.adj), sum(len(p) for p in g.paths), sum(len(p) for p in sub.paths)]
    assert [int(x) for i, x in enumerate(m.groups()) if i != 4] == want and m.group(5) is None
    if not keep.all():
        assert sub.n_vtx < g.n_vtx and want[7] < want[6]                   # (not vacuous)
    if chop is None:
        assert f"Graph has {sub.n_vtx} vertices, {sub.n_walks} walks" in log1 and f"Graph has {sub.n_vtx} vertices, {sub.n_walks} walks" in log2


@pytest.mark.parametrize("chop", [None, 30])
def test_drop_and_keep_samples(tmp_path, chop):
    g, full, rd = _case(tmp_path)
    extra = ["--chop", str(chop)] if chop else []
    keep = _keep_of(g, {"hap1", "hap2", "hap3", "hap4"})
    r2, fa2 = _plain(tmp_path, g, keep, "drop", rd, chop, extra=["-d1"])
    fa = tmp_path / "a.fa"
    r1 = _run_cli(["--drop-samples", "hap0", "-g", full, "-r", rd, "-o", str(fa), "-R", "30", "-d1"] + extra, tmp_path)
    assert r1.returncode == 0, r1.stderr
    _check(r1.stderr, fa.read_bytes(), r2.stderr, fa2, g, keep, chop)
    assert "hap0.1 :" not in r1.stderr and "hap1.1 :" in r1.stderr
    shared = [ln for ln in r1.stderr.splitlines() if ln.startswith("[Haplotypes: ")]
    assert len(shared) == 4 and shared == [ln for ln in r2.stderr.splitlines() if ln.startswith("[Haplotypes: ")]
    names = tmp_path / "names.txt"
    names.write_text("hap0\nhap3\n\nhap4\n")
    keep = _keep_of(g, {"hap0", "hap3", "hap4"})
    r2, fa2 = _plain(tmp_path, g, keep, "keep", rd, chop)
    fb = tmp_path / "b.fa"
    r1 = _run_cli(["--keep-samples", "@" + str(names), "-g", full, "-r", rd, "-o", str(fb), "-R", "30"] + extra, tmp_path)
    assert r1.returncode == 0, r1.stderr
    _check(r1.stderr, fb.read_bytes(), r2.stderr, fa2, g, keep, chop)


@pytest.mark.parametrize("chop", [None, 30])
def test_panels_in_one_command(tmp_path, chop):
    """chopped, the walks are resolved on the device (PHI_WALK_TEXT_MIN=0) and retained there; unchopped they come from the host"""
    from phi_amd.panel import nested_panels, samples_in_order
    g, full, rd = _case(tmp_path)
    extra = ["--chop", str(chop)] if chop else []
    panels = nested_panels(samples_in_order(g.hap_names), [1, 2, 4], seed=3, always=["hap0"])
    r1 = _run_cli(["--panels", "1,2,4", "--panel-seed", "3", "--panel-always", "hap0", "-g", full, "-r", rd, "-o", str(tmp_path / "o.{panel}.fa"), "-R", "30"] + extra,
                  tmp_path, {"PHI_WALK_TEXT_MIN": "0"} if chop else None)
    assert r1.returncode == 0, r1.stderr
    # the one log holds three runs' lines in turn: cut it at the "Panel:" lines
    parts = re.split(r"(?=^.*Panel: kept)", r1.stderr, flags=re.M)[1:]
    assert len(parts) == 3
    for size, p, part in zip([1, 2, 4], panels, parts):
        keep = _keep_of(g, set(p))
        assert int(keep.sum()) == size + 2
        r2, fa2 = _plain(tmp_path, g, keep, f"p{size}", rd, chop)
        _check(part, (tmp_path / f"o.{size}.fa").read_bytes(), r2.stderr, fa2, g, keep, chop)


def test_errors_and_refused_combinations(tmp_path):
    g, full, rd = _case(tmp_path)
    base = ["-g", full, "-r", rd, "-o", str(tmp_path / "x.fa")]
    r = _run_cli(["--drop-samples", "hap1,nobody,hap2,ghost"] + base, tmp_path)
    assert r.returncode == 1 and "the graph holds no sample named nobody, ghost" in r.stderr
    r = _run_cli(["--keep-samples", "hap1", "--drop-samples", "hap2"] + base, tmp_path)
    assert r.returncode == 1 and "exclude each other" in r.stderr
    r = _run_cli(["--panels", "1,2"] + base, tmp_path)
    assert r.returncode == 1 and "{panel}" in r.stderr
    r = _run_cli(["--panels", "2,1", "-g", full, "-r", rd, "-o", "o.{panel}.fa"], tmp_path)
    assert r.returncode == 1 and "ascend" in r.stderr
    r = _run_cli(["--panels", "1,9", "-g", full, "-r", rd, "-o", "o.{panel}.fa"], tmp_path)
    assert r.returncode == 1 and "the graph holds 5" in r.stderr
    r = _run_cli(["--panels", "1", "--coverage", "1", "--genome-size", "1000"] + base, tmp_path)
    assert r.returncode == 1 and "--coverage" in r.stderr
    r = _run_cli(["--panels", "1", "--devices", "0,1"] + base, tmp_path)
    assert r.returncode == 1 and "--devices" in r.stderr
    assert not os.path.exists(tmp_path / "x.fa")
