"""CPU: the parts of the BGZF indexes (phi_deflate_bgzf_indexed, PHI --bgzf-index) that need no GPU.  The new symbols in the
headers and the Python mirrors; phi_format_fasta_fai of libphi_host against the arithmetic of tests/tabix_ref.py's slice reader;
the plain host code of phi_amd/csrc/bgzf_index_host.h in a stand-alone program, phi_amd/csrc/host/bgzf_index_selftest.cpp, built
plain and with AddressSanitizer + UndefinedBehaviorSanitizer (`make -C phi_amd/csrc/host bgzf_index_sanitize`); and the helpers
the GPU tests rely on, checked against each other on a BGZF file that zlib wrote."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bgzf_index_cases as K
import bgzf_util
import tabix_ref as T
from conftest import ROOT

SAN = os.path.join(ROOT, "build", "sanitize")
BUILDS = ("plain", "asan")
OK = ("reg2bin", "gzi", "group_bins", "backfill", "names", "tbi_layout")


def test_symbols_and_mirrors():
    import phi_amd
    from phi_amd import _capi, ilp_index as H
    hdr = open(os.path.join(ROOT, "include", "phi_amd.h")).read()
    assert re.search(r"\bint phi_deflate_bgzf_indexed\(", hdr) and "phi_deflate_bgzf_indexed" in _capi.SYMBOLS
    for macro, value in (("PHI_BGZF_INDEX_GZI", 1), ("PHI_BGZF_INDEX_TBI_VCF", 2)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", hdr) and getattr(_capi, macro) == value, macro
    fields = re.search(r"typedef struct \{([^}]*)\} phi_bgzf_index_info;", hdr).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in re.sub(r"^\s*(int64_t|double|char)\s+", "", decl.strip()).split(",")]
    assert [re.sub(r"\[\d+\]", "", n) for n in names] == [n for n, _ in _capi.PhiBgzfIndexInfo._fields_]
    assert C.sizeof(_capi.PhiBgzfIndexInfo) == 7 * 8 + 8 + 192
    # the writer's own entries are what they were: flag 8 stays unknown
    assert re.search(r"#define\s+PHI_DEFLATE_NO_EOF\s+2\b", hdr) and not re.search(r"#define\s+PHI_DEFLATE_\w+\s+[48]\b", hdr)
    host_hdr = open(os.path.join(ROOT, "include", "phi_host.h")).read()
    assert re.search(r"\bint phi_format_fasta_fai\(", host_hdr) and "phi_format_fasta_fai" in H.HOST_SYMBOLS
    assert callable(phi_amd.deflate_bgzf_indexed) and "deflate_bgzf_indexed" in phi_amd.__all__
    from phi_amd.build import HIP_HEADERS, HIP_SOURCES
    assert "bgzf_index.hip" in HIP_SOURCES and "bgzf_index_host.h" in HIP_HEADERS
    src = open(os.path.join(ROOT, "phi_amd", "csrc", "bgzf_index.hip")).read()
    assert '#include "bgzf_index_host.h"' in src and '#include "phi_wave.h"' in src
    for fn in ("bgzfx::tbi_bytes", "bgzfx::gzi_bytes", "phi_compact_count", "phi_compact_write", "phi_scan_tiles", "phi_block_excl_scan"):
        assert fn + "(" in src or fn + "<" in src, fn


@pytest.mark.parametrize("length", [0, 1, 79, 80, 81, 160, 65199, 65280, 300000])
def test_fai_line_against_the_text_it_describes(length):
    from phi_amd.ilp_index import host_lib
    L = host_lib()
    rng = np.random.default_rng(length)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)].tobytes()
    name = b"hap_7 of sample\tx"
    t, n = C.c_void_p(), C.c_int64()
    assert L.phi_format_fasta(name, seq, length, C.byref(t), C.byref(n)) == 0
    text = C.string_at(t, n.value)
    L.phi_host_free_text(t)
    assert L.phi_format_fasta_fai(name, length, C.byref(t), C.byref(n)) == 0
    fai = C.string_at(t, n.value)
    L.phi_host_free_text(t)
    assert fai.endswith(b"\n") and fai.count(b"\n") == 1 and fai.count(b"\t") == 4
    got_name, got_len, offset, line_bases, line_width = T.fai_fields(fai)
    assert got_name == b"hap_7" and got_len == length and text[:offset] == b">" + name + b" LN:%d\n" % length
    assert (line_bases, line_width) == ((min(length, 80), min(length, 80) + 1) if length else (0, 0))
    for i in sorted({0, 1, 79, 80, 81, length // 2, length - 2, length - 1} & set(range(length))):
        assert text[T.fai_offset(fai, i)] == seq[i], i
    # through the slice reader, over a BGZF file that zlib wrote
    data = K.zlib_bgzf(text)
    gzi = T.gzi_bytes(T.member_offsets(data))
    for s, m in [(0, length)] + [(int(s), int(rng.integers(0, length - s + 1))) for s in rng.integers(0, max(length, 1), 10) if length]:
        assert T.fasta_slice(data, gzi, fai, s, m) == seq[s:s + m]
    assert L.phi_format_fasta_fai(None, 1, C.byref(t), C.byref(n)) != 0 and L.phi_format_fasta_fai(b"n", -1, C.byref(t), C.byref(n)) != 0


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "bgzf_index_sanitize", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return {b: subprocess.run([os.path.join(SAN, "bgzf_index_selftest_" + b)], capture_output=True, text=True, env=env, timeout=300) for b in BUILDS}


@pytest.mark.parametrize("build", BUILDS)
def test_host_rules_selftest(outputs, build):
    r = outputs[build]
    assert r.returncode == 0, (build, r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "FAILED" not in r.stdout
    lines = dict(l.split(" ", 1) for l in r.stdout.splitlines())
    for name in OK:
        assert lines[name].startswith("ok "), (name, lines[name])
    assert int(re.search(r"checked=(\d+)", lines["reg2bin"]).group(1)) > 900000
    assert outputs["plain"].stdout == outputs["asan"].stdout and len(r.stdout.splitlines()) == len(OK)


def test_the_reference_reader_finds_what_the_reference_writer_indexed():
    """tabix_ref's writer and reader against the brute-force filter, on the synthetic VCF in a BGZF file by zlib: the yardsticks
    of the GPU tests agree with each other before they judge the device"""
    text = K.synthetic_vcf("plain")
    K.check_corners(text)
    data = K.zlib_bgzf(text)
    assert bgzf_util.text_of(data) == text
    tbi, counts = T.tbi_bytes(text, T.member_offsets(data))
    assert counts["records"] > 6000 and counts["contigs"] == 2
    idx = T.parse_tbi(K.zlib_bgzf(tbi))
    cache = {}
    for name, lo, hi in K.draw_regions(text, 200, seed=9):
        assert T.query(data, idx, name, lo, hi, cache) == T.overlapping(text, name, lo, hi), (name, lo, hi)
