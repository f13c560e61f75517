"""CPU tests of the host side of the BAM reads route: phi_bam_header (include/phi_host.h, libphi_host.so) through ctypes, the
exported symbols of both libraries, the test writer and oracle of tests/bam_util.py against gzip.decompress, and the header
parser -- which reads untrusted bytes -- under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program
(phi_amd/csrc/host/bam_header_selftest.cpp, `make -C phi_amd/csrc/host bam_sanitize`) run as a child process."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_util as B
from conftest import ROOT

OK, INVALID, MORE = 0, -4, -6


@pytest.fixture(scope="module")
def H():
    from phi_amd import build
    build.build_host()
    from phi_amd import ilp_index
    return ilp_index


def _headers():
    refs = [(b"chr%d" % i + b"y" * (i % 9), 10 + i) for i in range(200)]
    return [B.header(), B.header(b"@HD\tVN:1.6\n"), B.header(b"", refs[:1]), B.header(b"@CO\tlong " + b"t" * 3000 + b"\n", refs)]


def test_valid_headers_and_every_truncation_point(H):
    for h in _headers():
        tail = h + B.record(b"r", b"ACGT")
        want = B.parse_header(tail)
        assert want[0] == len(h)
        for data in (h, tail):
            rc, start, n_ref, msg = H.bam_header(data)
            assert (rc, start, n_ref, msg) == (OK, want[0], want[1], "")
        for n in range(len(h)):
            rc, start, n_ref, msg = H.bam_header(tail[:n])
            assert rc == MORE and n < start <= len(h), (n, rc, start)      # "need more bytes", with a bound that makes progress
            with pytest.raises(B.BamInvalid):
                B.parse_header(tail[:n])


def test_what_is_not_a_bam_header(H):
    good = B.header(b"@CO\tx\n", [(b"chr1", 5), (b"chr2", 6)])
    for i in range(4):
        bad = bytearray(good)
        bad[i] ^= 1
        for n in range(i + 1, len(bad) + 1):
            rc, _, _, msg = H.bam_header(bytes(bad[:n]))
            assert rc == INVALID and f"byte {i} " in msg, (i, n, msg)
    for other in (b"CRAM\x03\x00", b"@HD\tVN:1.6\n", b"@r1\nACGT\n+\nIIII\n", b">r\nACGT\n", b"\x1f\x8b\x08\x04"):
        assert H.bam_header(other)[0] == INVALID
    at_text, at_nref, at_name = 4, 8 + 6, 8 + 6 + 4
    for at in (at_text, at_nref, at_name):
        for v in (-1, -4, -2 ** 31):
            bad = good[:at] + struct.pack("<i", v) + good[at + 4:]
            rc, _, _, msg = H.bam_header(bad)
            assert rc == INVALID and f"byte offset {at}" in msg, (at, v, msg)
            with pytest.raises(B.BamInvalid) as e:
                B.parse_header(bad)
            assert e.value.offset == at
        big = good[:at] + struct.pack("<i", 2 ** 31 - 1) + good[at + 4:]
        rc, start, _, _ = H.bam_header(big)
        assert rc == MORE and start > len(big)
    zero = good[:at_name] + struct.pack("<i", 0) + good[at_name + 4:]      # a name holds its NUL at least
    assert H.bam_header(zero)[0] == INVALID
    assert H.bam_header(b"")[0] == MORE and H.bam_header(b"BAM")[0] == MORE


def test_new_symbols_are_exported(H):
    from phi_amd import _capi
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in ("phi_reads_bam_begin", "phi_add_reads_bam", "phi_add_reads_bam_parked", "phi_reads_bam_end", "phi_reads_bam_last_batch"):
        assert name in have and name in _capi.SYMBOLS, name
    assert hasattr(H.host_lib(), "phi_bam_header") and "phi_bam_header" in H.HOST_SYMBOLS
    import phi_amd
    for m in ("reads_bam_begin", "add_reads_bam", "add_reads_bam_parked", "reads_bam_end", "reads_bam_last_batch"):
        assert callable(getattr(phi_amd.Context, m))


def _some_bam(rng, n=120):
    recs = []
    for i in range(n):
        ln = int(rng.choice([0, 1, 2, 33, 150, 151]))
        seq = bytes(rng.choice(np.frombuffer(B.CODES, np.uint8), ln))
        recs.append(B.record(b"q%d" % i, seq, flag=int(rng.choice([0, 4, 0x10, 0x100, 0x800, 0x910, 0x41, 0x91])), ref_id=int(rng.integers(-1, 3)),
                             n_cigar=int(rng.integers(0, 3)), aux=bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8))))
    return B.header(b"@HD\tVN:1.6\n", [(b"a", 9), (b"b", 9), (b"c", 9)]) + b"".join(recs)


def test_writer_and_oracle_round_trip(H, tmp_path):
    rng = np.random.default_rng(1)
    data = _some_bam(rng)
    for block, eof in ((0xFF00, True), (100, True), (37, False), (1, True)):
        gz = B.bgzf(data[:3000] if block == 1 else data, block, eof)
        want = data[:3000] if block == 1 else data
        assert gzip.decompress(gz) == want
        assert gz.endswith(B.EOF_BLOCK) == eof and gzip.decompress(B.EOF_BLOCK) == b""
        assert gz[12:14] == b"BC" and struct.unpack_from("<H", gz, 16)[0] + 1 == (len(gz) if len(want) <= block and not eof else gz.index(b"\x1f\x8b\x08\x04", 1))
    # the oracle on records written by hand: orientation, filter, codes
    assert B.revcomp(b"ACMGRSVTWYHKDBN=") == b"=NVHMDRWABSYCKGT"
    one = B.header() + B.record(b"f", b"AACGTN=", flag=0) + B.record(b"r", b"AACGTN=", flag=0x10) + B.record(b"s", b"ACGT", flag=0x100) + \
        B.record(b"p", b"ACGT", flag=0x800) + B.record(b"e", b"", flag=0) + B.record(b"m1", b"GG", flag=0x41) + B.record(b"m2", b"TT", flag=0x81)
    reads, info = B.decode(one)
    assert reads == [b"AACGTN=", b"=NACGTT", b"GG", b"TT"]
    assert (info["n_records"], info["n_kept"], info["n_secondary_supplementary"], info["n_empty"], info["n_reverse"], info["n_bases"]) == (7, 4, 2, 1, 1, 18)
    assert B.pack_seq(b"AACGT") == bytes([0x11, 0x24, 0x80])
    assert B.fastq(reads[:2]) == b"@r0\nAACGTN=\n+\nIIIIIII\n@r1\n=NACGTT\n+\nIIIIIII\n"
    # through the host pool the command line inflates BGZF with, and the content sniffing of the Python mirror
    p = str(tmp_path / "reads.anyname")
    B.write_bam(p, data, block_bytes=333, eof=False)
    assert b"".join(bytes(c) for c in H.text_chunks(p, 4096)) == data
    assert H.reads_file_kind(p) == "bam"
    for name, content, kind in (("a.bam", b"CRAM\x03\x00rest", "cram"), ("b.bam", b"@HD\tVN:1.6\n@SQ\tSN:x\tLN:5\n", "sam"), ("c.bam", b"@r\nACGT\n+\nIIII\n", "text"),
                                ("d.bam", gzip.compress(b">r\nACGT\n"), "text")):
        q = tmp_path / name
        q.write_bytes(content)
        assert H.reads_file_kind(str(q)) == kind
    # a FASTQ whose first read is merely named like a header tag; a missing file and a FIFO are left to the reader, unread
    (tmp_path / "hd.fq").write_bytes(b"@HD\tread one\nACGT\n+\nIIII\n")
    assert H.reads_file_kind(str(tmp_path / "hd.fq")) == "text"
    assert H.reads_file_kind(str(tmp_path / "no_such_file.fq")) == "text"
    with pytest.raises(H.HostError):
        H.ILP_index(os.path.join(ROOT, "tests", "golden", "data", "test.gfa")).read_ip_reads([], str(tmp_path / "no_such_file.fq"))
    os.mkfifo(str(tmp_path / "fifo.fq"))
    assert H.reads_file_kind(str(tmp_path / "fifo.fq")) == "text"      # (returns at once: nothing is opened)


def test_header_parser_under_the_sanitizers():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "bam_sanitize", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "build", "sanitize", "bam_header_selftest_asan")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("bam_header_selftest: ok ")
