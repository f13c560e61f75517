"""The command line's device route for single-stream gzip reads (PHI_INFLATE_MIN): every log line and the
FASTA of the host inflater's run (PHI_INFLATE=0)."""
import gzip
import os
import re
import subprocess

import pytest

from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

PHI = os.path.join(ROOT, "phi_amd", "PHI")
GFA = os.path.join(DATA, "MHC_4.gfa.gz")
READS = os.path.join(DATA, "CHM13_reads.fq.gz")
DEVICE = {"PHI_TIMING": "1", "PHI_INFLATE_MIN": "1", "PHI_READ_CHUNK": "100000"}
HOST = {"PHI_TIMING": "1", "PHI_INFLATE": "0", "PHI_READ_CHUNK": "100000"}


def run(args, tmp_path, env):
    if not os.path.exists(PHI):
        import __graft_entry__
        __graft_entry__.build()
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([PHI] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=300, env=e)


def lines(log):
    return [re.sub(r"^\[M::[^\]]*\] ", "", l) for l in log.splitlines()
            if not (l.startswith("[phi timing]") or "Real time" in l or "CMD:" in l or "written to" in l)]


def inflated(log):
    return max([int(m) for m in re.findall(r"main: (\d+) bytes inflated on the device", log)] or [0])


def fasta(path):
    return path.read_text().split("\n")[1:]


def test_golden_reads_inflated_on_the_device(tmp_path):
    host = run(["-t8", "-g", GFA, "-r", READS, "-o", str(tmp_path / "host.fa")], tmp_path, HOST)
    dev = run(["-t8", "-g", GFA, "-r", READS, "-o", str(tmp_path / "dev.fa")], tmp_path, DEVICE)
    assert host.returncode == 0 and dev.returncode == 0, host.stderr[-2000:] + dev.stderr[-2000:]
    assert inflated(host.stderr) == 0
    assert inflated(dev.stderr) > 5_000_000, dev.stderr[-2000:]
    assert lines(host.stderr) == lines(dev.stderr)
    assert "; 0 bases through the host reader" in dev.stderr
    assert fasta(tmp_path / "host.fa") == fasta(tmp_path / "dev.fa")
    # below the threshold (the default): today's path
    default = run(["-t8", "-g", GFA, "-r", READS, "-o", str(tmp_path / "default.fa")], tmp_path, {"PHI_TIMING": "1", "PHI_READ_CHUNK": "100000"})
    assert default.returncode == 0 and inflated(default.stderr) == 0


def test_irregular_text_is_fetched_back_for_the_host_reader(tmp_path):
    text = gzip.open(READS, "rb").read()
    recs = text.split(b"\n")
    mid = (len(recs) // 8) * 4
    wrapped = recs[:mid] + [recs[mid], recs[mid + 1][:70], recs[mid + 1][70:], recs[mid + 2], recs[mid + 3][:70], recs[mid + 3][70:]] + recs[mid + 4:]
    (tmp_path / "wrapped.fq.gz").write_bytes(gzip.compress(b"\n".join(wrapped), 6))
    args = ["-t8", "-g", GFA, "-r", str(tmp_path / "wrapped.fq.gz")]
    host = run(args + ["-o", str(tmp_path / "host.fa")], tmp_path, HOST)
    dev = run(args + ["-o", str(tmp_path / "dev.fa")], tmp_path, DEVICE)
    assert host.returncode == 0 and dev.returncode == 0, host.stderr[-2000:] + dev.stderr[-2000:]
    assert inflated(dev.stderr) > 5_000_000 and "host reader from the first byte not taken" in dev.stderr
    assert lines(host.stderr) == lines(dev.stderr)
    assert fasta(tmp_path / "host.fa") == fasta(tmp_path / "dev.fa")


def test_corrupt_reads_file_same_status_and_message(tmp_path):
    """the device refuses the stream and leaves it to the host inflater: whatever that reports, exit status included"""
    data = bytearray(open(READS, "rb").read())
    data[-6] ^= 0x40                                          # the trailer's CRC32
    (tmp_path / "bad.fq.gz").write_bytes(bytes(data))
    cut = open(READS, "rb").read()[: 900_000]
    (tmp_path / "cut.fq.gz").write_bytes(cut)
    for name in ("bad.fq.gz", "cut.fq.gz"):
        args = ["-t8", "-g", GFA, "-r", str(tmp_path / name)]
        host = run(args + ["-o", str(tmp_path / "host.fa")], tmp_path, HOST)
        dev = run(args + ["-o", str(tmp_path / "dev.fa")], tmp_path, DEVICE)
        assert host.returncode == dev.returncode, (name, host.returncode, dev.returncode, dev.stderr[-2000:])
        assert lines(host.stderr) == lines(dev.stderr), name
        assert inflated(dev.stderr) == 0


def test_two_jobs_in_one_command(tmp_path):
    text = gzip.open(READS, "rb").read()
    recs = text.split(b"\n")
    half = (len(recs) // 8) * 4
    (tmp_path / "b.fq.gz").write_bytes(gzip.compress(b"\n".join(recs[half:]), 6))
    jobs = ["-r", READS, "-o", "a.fa", "-r", str(tmp_path / "b.fq.gz"), "-o", "b.fa"]
    (tmp_path / "h").mkdir()
    (tmp_path / "d").mkdir()
    host = run(["-t8", "-g", GFA] + jobs, tmp_path / "h", HOST)
    dev = run(["-t8", "-g", GFA] + jobs, tmp_path / "d", DEVICE)
    assert host.returncode == 0 and dev.returncode == 0, host.stderr[-2000:] + dev.stderr[-2000:]
    assert inflated(dev.stderr) > len(text) > 5_000_000                       # both jobs' reads went through the device
    assert lines(host.stderr) == lines(dev.stderr)
    for f in ("a.fa", "b.fa"):
        assert fasta(tmp_path / "h" / f) == fasta(tmp_path / "d" / f)
