"""CPU: the host side of `--bgzf`.  phi_format_fasta and phi_format_calls_vcf (libphi_host) hand out in memory exactly the bytes
phi_write_fasta and phi_write_calls_vcf write to their files; phi_deflate_bgzf_bound; the new symbols; and that nothing changes
without the flag: a .gz name is still refused by the plain writer."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

from conftest import DATA, ROOT
from test_cpu_calls_host import CALLS, EXPECTED


@pytest.fixture(scope="module")
def host():
    from phi_amd import build as B
    B.build_host()
    from phi_amd import ilp_index as H
    return H.host_lib()


def _format_fasta(L, name, seq):
    text, n = C.c_void_p(), C.c_int64()
    assert L.phi_format_fasta(name, seq, len(seq), C.byref(text), C.byref(n)) == 0
    try:
        return C.string_at(text, n.value)
    finally:
        L.phi_host_free_text(text)


def _format_calls(L, calls, contig, contig_len, sample, ph=None):
    n = len(calls["pos"])
    pos, ro, ao = (np.ascontiguousarray(calls[k], np.int64) for k in ("pos", "ref_off", "alt_off"))
    names = (C.c_char_p * max(n, 1))(*[s.encode() for s in ph]) if ph is not None else None
    text, size, nw, nd = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
    err = C.create_string_buffer(512)
    rc = L.phi_format_calls_vcf(contig.encode(), contig_len, sample.encode(), n, pos.ctypes.data, ro.ctypes.data, bytes(calls["ref_bytes"]), ao.ctypes.data,
                                bytes(calls["alt_bytes"]), names, C.byref(text), C.byref(size), C.byref(nw), C.byref(nd), err, 512)
    if rc:
        assert not text.value
        return rc, err.value.decode(), None, None
    try:
        return 0, C.string_at(text, size.value), nw.value, nd.value
    finally:
        L.phi_host_free_text(text)


def test_format_fasta_equals_the_written_file(host, tmp_path):
    with gzip.open(os.path.join(DATA, "MHC-CHM13.0.fa.gz"), "rb") as f:
        lines = f.read().split(b"\n")
    mhc = b"".join(lines[1:])
    assert len(mhc) > 4_000_000
    # lengths around the line width and the writer's blocks of 65 536 lines; the golden sequence whole
    for name, seq in ((b"empty", b""), (b"one", b"A"), (b"l79", mhc[:79]), (b"l80", mhc[:80]), (b"l81", mhc[:81]), (b"l160", mhc[:160]),
                      (b"blk", mhc[:65536 * 80]), (b"blk1", mhc[:65536 * 80 + 1]), (b"MHC-CHM13 x", mhc)):
        p = tmp_path / "w.fa"
        assert host.phi_write_fasta(os.fsencode(str(p)), name, seq, len(seq)) == 0
        assert _format_fasta(host, name, seq) == p.read_bytes(), name
    assert _format_fasta(host, b"n", b"ACGT") == b">n LN:4\nACGT\n"
    text, n = C.c_void_p(), C.c_int64()
    assert host.phi_format_fasta(None, b"A", 1, C.byref(text), C.byref(n)) != 0
    assert host.phi_format_fasta(b"n", None, 1, C.byref(text), C.byref(n)) != 0


def test_format_calls_equals_the_written_file(host, tmp_path):
    from phi_amd.calls import write_vcf
    ph = ["hapA.1", "hapA.1", "hapB.1", "hapC.2"]
    rc, text, nw, nd = _format_calls(host, CALLS, "chrT", 25, "sample_1", ph)
    assert (rc, nw, nd) == (0, 3, 1) and text == EXPECTED.encode()
    p = tmp_path / "c.vcf"
    for tags in (ph, None):
        assert write_vcf(str(p), CALLS, "chrT", 25, "sample_1", ph=tags) == (3, 1)
        assert _format_calls(host, CALLS, "chrT", 25, "sample_1", tags)[1] == p.read_bytes()
    empty = dict(pos=np.zeros(0, np.int64), ref_off=np.zeros(1, np.int64), alt_off=np.zeros(1, np.int64), ref_bytes=b"", alt_bytes=b"")
    assert write_vcf(str(p), empty, "chrT", 25, "sample_1", ph=[]) == (0, 0)
    assert _format_calls(host, empty, "chrT", 25, "sample_1", [])[1:] == (p.read_bytes(), 0, 0)
    # the same refusal, the same words
    bad = dict(CALLS, alt_off=np.array([0, 3, 3, 8, 9], np.int64))
    rc, msg, _, _ = _format_calls(host, bad, "chrT", 25, "s")
    assert rc != 0 and "empty allele" in msg and "call 1" in msg


def test_format_calls_on_records_of_the_golden_vcf(host, tmp_path):
    """the records of tests/golden/data/MHC_4.vcf.gz as calls (first ALT of every record whose REF and ALT are plain bases):
    thousands of records of every length through both routes"""
    from phi_amd.calls import write_vcf
    pos, refs, alts = [], [], []
    with gzip.open(os.path.join(DATA, "MHC_4.vcf.gz"), "rb") as f:
        for ln in f:
            if ln.startswith(b"#"):
                continue
            c = ln.split(b"\t", 6)
            alt = c[4].split(b",")[0]
            if re.fullmatch(rb"[ACGTNacgtn]+", c[3]) and re.fullmatch(rb"[ACGTNacgtn]+", alt):
                pos.append(int(c[1]) - 1), refs.append(c[3]), alts.append(alt)
    assert len(pos) > 5000 and all(r != a for r, a in zip(refs, alts))
    refs[7] = alts[7]                                              # one REF = ALT call: dropped by both
    ro, ao = np.zeros(len(pos) + 1, np.int64), np.zeros(len(pos) + 1, np.int64)
    np.cumsum([len(r) for r in refs], out=ro[1:])
    np.cumsum([len(a) for a in alts], out=ao[1:])
    calls = dict(pos=np.array(pos, np.int64), ref_off=ro, alt_off=ao, ref_bytes=b"".join(refs), alt_bytes=b"".join(alts))
    ph = ["w%d.1" % (k % 5) if k % 3 else "" for k in range(len(pos))]
    p = tmp_path / "g.vcf"
    assert write_vcf(str(p), calls, "chr6", 5_000_000, "HG", ph=ph) == (len(pos) - 1, 1)
    assert _format_calls(host, calls, "chr6", 5_000_000, "HG", ph) == (0, p.read_bytes(), len(pos) - 1, 1)


def test_without_bgzf_a_gz_name_is_still_refused(host, tmp_path):
    from phi_amd.calls import write_vcf
    from phi_amd.ilp_index import HostError
    with pytest.raises(HostError) as e:
        write_vcf(str(tmp_path / "calls.vcf.gz"), CALLS, "chrT", 25, "s")
    assert ".gz" in str(e.value) and "deflate" in str(e.value) and "bgzf" in str(e.value) and not (tmp_path / "calls.vcf.gz").exists()


def test_bound_is_monotone_and_covers_stored_blocks():
    import __graft_entry__
    __graft_entry__.ensure_built()
    from phi_amd import _capi
    L = _capi.load()
    B = _capi.PHI_BGZF_BLOCK
    assert B == 65280
    sizes = sorted({0, 1, 2, B - 1, B, B + 1, 2 * B, 2 * B + 1, 10 * B - 1, 10 * B, 10 * B + 1, 176_000_000, 1 << 33} | {int(x) for x in np.random.default_rng(5).integers(0, 1 << 24, 200)})
    bounds = [L.phi_deflate_bgzf_bound(n) for n in sizes]
    assert all(a <= b for a, b in zip(bounds, bounds[1:]))
    for n, b in zip(sizes, bounds):
        blocks = -(-n // B)
        assert b >= n + blocks * (18 + 5 + 8) + 28, (n, b)          # every block stored, and the EOF block
        assert b <= n + blocks * 64 + 64, (n, b)                    # and not a guess far above that
    assert L.phi_deflate_bgzf_bound(-5) == L.phi_deflate_bgzf_bound(0) == 28
    assert 18 + 5 + B + 8 <= 65536                                   # BSIZE fits 16 bits at the worst


def test_symbols_are_declared_bound_and_exported():
    from phi_amd import _capi
    from phi_amd import ilp_index as H
    import phi_amd
    hdr = open(os.path.join(ROOT, "include", "phi_amd.h")).read()
    for name in ("phi_deflate_bgzf", "phi_deflate_bgzf_alloc"):
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _capi.SYMBOLS, name
    assert re.search(r"\bint64_t phi_deflate_bgzf_bound\(", hdr) and re.search(r"\bvoid phi_deflate_free\(", hdr)
    assert {"phi_deflate_bgzf_bound", "phi_deflate_free"} <= set(_capi.SYMBOLS)
    for macro, value in (("PHI_BGZF_BLOCK", 65280), ("PHI_DEFLATE_NO_MATCH", 1), ("PHI_DEFLATE_NO_EOF", 2)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", hdr) and getattr(_capi, macro) == value, macro
    assert int(re.search(r"#define\s+PHI_DEFLATE_BATCH_DEFAULT\s+(\d+)", hdr).group(1)) == _capi.PHI_DEFLATE_BATCH_DEFAULT
    assert C.sizeof(_capi.PhiDeflateInfo) == 6 * 8 + 8 + 192
    host_hdr = open(os.path.join(ROOT, "include", "phi_host.h")).read()
    for name in ("phi_format_fasta", "phi_format_calls_vcf"):
        assert name in H.HOST_SYMBOLS and re.search(r"\bint " + name + r"\(", host_hdr), name
    assert "phi_host_free_text" in H.HOST_SYMBOLS and "no deflate writer" not in host_hdr
    assert callable(phi_amd.deflate_bgzf) and "deflate_bgzf" in phi_amd.__all__
