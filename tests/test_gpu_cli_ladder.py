"""`PHI --coverage ... --genome-size N --seed S`: one FASTA per coverage, each byte-identical to what a plain `PHI` run
writes for a file holding exactly the rule's reads of that level (phi_amd/ladder.py writes that file)."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

from phi_amd import ladder as rule

pytestmark = pytest.mark.gpu

PHI = os.path.join(ROOT, "phi_amd", "PHI")
GFA = os.path.join(DATA, "test.gfa")
TOY = ["-k3", "-w2", "-q0", "-m0", "-R", "10"]
COVS = ["0.5", "1", "2"]
SEED = 3


def _run_cli(args, cwd):
    if not os.path.exists(PHI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host")])
    return subprocess.run([PHI] + args, capture_output=True, text=True, cwd=str(cwd), timeout=300)


def _records(text):
    recs = []
    for ln in text.decode().split("\n"):
        if ln.startswith(">"):
            recs.append([ln, ""])
        elif ln:
            recs[-1][1] += ln
    return recs


def _level_lines(log):
    """per level: the ladder's line and the counts a plain run logs"""
    return re.findall(r"read has (\d+) reads|Indexed reads with spectrum size: (\d+)|(Coverage \S+x: fraction [\d.]+, \d+ reads, \d+ bases)", log)


def _many_reads():
    rng = np.random.default_rng(5)
    base = b"ATCGATCATACTTACCATG"
    out = []
    for i in range(60):
        if i % 3 == 0:
            s = bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(5, 40))).tolist())
        else:
            a = int(rng.integers(0, 8))
            s = base[a:a + int(rng.integers(6, 19))]
        out.append(b">r%d\n%s\n" % (i, s))
    return b"".join(out)


@pytest.mark.parametrize("case", ["golden", "many", "many_gz", "golden_gz"])
def test_cli_ladder_equals_plain_runs_on_the_levels(tmp_path, case):
    text = open(os.path.join(DATA, "read.fa"), "rb").read() if case.startswith("golden") else _many_reads()
    recs = _records(text)
    total = sum(len(s) for _, s in recs)
    genome = total if case.startswith("golden") else total // 2      # fractions 0.5, 1, 1 (clipped) / 0.25, 0.5, 1
    gz = case.endswith("_gz")
    name = "read.fa.gz" if gz else "read.fa"
    rd = tmp_path / name
    rd.write_bytes(gzip.compress(text) if gz else text)
    args = ["--coverage", ",".join(COVS), "--genome-size", str(genome), "--seed", str(SEED), "-g", GFA, "-r", str(rd)] + TOY
    r = _run_cli(args + ["-o", "out.{cov}x.fa"], tmp_path)
    assert r.returncode == 0, r.stderr
    fr = rule.fractions_from_coverage([float(c) for c in COVS], genome, total)
    band = rule.bands(SEED, np.arange(len(recs)), fr)
    lines = _level_lines(r.stderr)
    assert len(lines) == 9, r.stderr
    for j, cov in enumerate(COVS):
        out = tmp_path / f"out.{cov}x.fa"
        assert out.exists(), (cov, r.stderr)
        level = [recs[i] for i in np.flatnonzero(band <= j)]
        assert level, "the case is meant to keep reads at every level"
        # the level's reads in a file of the name the FASTA header is made from (the last extension goes)
        d = tmp_path / f"level{j}"
        d.mkdir()
        plain_rd = d / ("read.fa.fa" if gz else "read.fa")
        plain_rd.write_bytes("".join(f"{h}\n{s}\n" for h, s in level).encode())
        p = _run_cli(["-g", GFA, "-r", str(plain_rd), "-o", "plain.fa"] + TOY, d)
        assert p.returncode == 0, p.stderr
        assert out.read_bytes() == (d / "plain.fa").read_bytes(), (case, cov)
        n_bases = sum(len(s) for _, s in level)
        assert lines[3 * j][2] == f"Coverage {cov}x: fraction {fr[j]:.6f}, {len(level)} reads, {n_bases} bases"
        assert lines[3 * j + 1][0] == str(len(level))
        assert (lines[3 * j + 1][0], lines[3 * j + 2][1]) == tuple(x for t in _level_lines(p.stderr) for x in t if x)
        assert f"written to: out.{cov}x.fa" in r.stderr
    # two runs are identical
    r2 = _run_cli(args + ["-o", "again.{cov}x.fa"], tmp_path)
    assert r2.returncode == 0, r2.stderr
    for cov in COVS:
        assert (tmp_path / f"again.{cov}x.fa").read_bytes() == (tmp_path / f"out.{cov}x.fa").read_bytes()


def test_cli_ladder_for_several_read_sets_and_a_single_coverage(tmp_path):
    a, b = tmp_path / "a.fa", tmp_path / "b.fa"
    a.write_bytes(_many_reads())
    b.write_bytes(open(os.path.join(DATA, "read.fa"), "rb").read())
    r = _run_cli(["--coverage", "1,30", "--genome-size", "300", "-g", GFA, "-r", str(a), "-o", "a.{cov}.fa", "-r", str(b), "-o", "b.{cov}.fa"] + TOY, tmp_path)
    assert r.returncode == 0, r.stderr
    for n in ("a.1.fa", "a.30.fa", "b.1.fa", "b.30.fa"):
        assert (tmp_path / n).read_text().startswith(">test_" + n[0] + " LN:"), n
    p = _run_cli(["-g", GFA, "-r", str(b), "-o", "plain.fa"] + TOY, tmp_path)
    assert (tmp_path / "b.30.fa").read_text().split("\n")[1:] == (tmp_path / "plain.fa").read_text().split("\n")[1:]
    # one coverage: -o needs no {cov}
    r = _run_cli(["--coverage", "30", "--genome-size", "300", "-g", GFA, "-r", str(b), "-o", "single.fa"] + TOY, tmp_path)
    assert r.returncode == 0 and (tmp_path / "single.fa").read_bytes() == (tmp_path / "b.30.fa").read_bytes()


@pytest.mark.parametrize("args,word", [
    (["--coverage", "1,2", "-o", "x.{cov}.fa"], "--genome-size"),
    (["--coverage", "2,1", "--genome-size", "10", "-o", "x.{cov}.fa"], "ascend"),
    (["--coverage", "1,2", "--genome-size", "10", "--devices", "0,1", "-o", "x.{cov}.fa"], "--devices"),
    (["--coverage", "1,2", "--genome-size", "10", "-o", "x.fa"], "{cov}"),
    (["--coverage", "1,x", "--genome-size", "10", "-o", "x.{cov}.fa"], "--coverage"),
])
def test_cli_ladder_usage_errors(tmp_path, args, word):
    r = _run_cli(args + ["-g", GFA, "-r", os.path.join(DATA, "read.fa")], tmp_path)
    assert r.returncode != 0 and "[E::main]" in r.stderr and word in r.stderr, r.stderr
    assert not list(tmp_path.iterdir())
