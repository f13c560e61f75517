"""The device inflater's host parts and its kernels' budget, checked without a GPU."""
import gzip
import os
import re
import struct
import subprocess
import zlib

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "phi_amd", "csrc", "inflate.hip")


@pytest.fixture(scope="module")
def phi():
    import __graft_entry__
    __graft_entry__.ensure_built()
    import phi_amd
    return phi_amd


def test_symbols_are_exported(phi):
    from phi_amd import _capi
    L = _capi.load()
    for name in ("phi_inflate", "phi_gzip_header", "phi_crc32_combine"):
        assert name in _capi.SYMBOLS and getattr(L, name)
    header = open(os.path.join(ROOT, "include", "phi_amd.h")).read()
    for name in ("phi_inflate(", "phi_gzip_header(", "phi_crc32_combine(", "phi_inflate_info"):
        assert name in header
    m = re.search(r"#define PHI_INFLATE_CHUNK_DEFAULT \((\d+) << (\d+)\)", header)
    assert m and int(m.group(1)) << int(m.group(2)) == _capi.PHI_INFLATE_CHUNK_DEFAULT


def test_crc32_combine_matches_zlib(phi):
    rng = __import__("random").Random(5)
    for la, lb in [(0, 0), (1, 0), (0, 1), (3, 5), (4096, 4096), (100_000, 12_345), (1, 1 << 20)]:
        a, b = rng.randbytes(la), rng.randbytes(lb)
        assert phi.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b), (la, lb)
    # a run of zero bytes far longer than any buffer: crc(a + 0^n) through the shift alone
    z = bytes(1 << 22)
    assert phi.crc32_combine(zlib.crc32(b"xyz"), zlib.crc32(z), len(z)) == zlib.crc32(b"xyz" + z)


def header(flags=0, extra=b"", name=b"", comment=b"", bad_hcrc=False):
    h = bytearray(b"\x1f\x8b\x08" + bytes([flags]) + b"\x00" * 4 + b"\x00\x03")
    if flags & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        h += name + b"\x00"
    if flags & 16:
        h += comment + b"\x00"
    if flags & 2:
        h += struct.pack("<H", (zlib.crc32(bytes(h)) ^ bad_hcrc) & 0xffff)
    return bytes(h)


def test_gzip_header_parsing(phi):
    from phi_amd import PhiError
    for flags, kw in [(0, {}), (8, {"name": b"reads.fq"}), (4, {"extra": b"BC\x02\x00\x10\x00"}), (16, {"comment": b"hi"}),
                      (2, {}), (2 | 4 | 8 | 16, {"extra": b"\x01" * 700, "name": b"a", "comment": b"b"})]:
        h = header(flags, **kw)
        data = b"pad" + h + b"\x03\x00"
        assert phi.gzip_header(data, 3) == 3 + len(h), flags
    g = gzip.compress(b"abc", mtime=0)
    assert phi.gzip_header(g) == 10
    for bad in [b"\x1f\x8b\x07" + b"\x00" * 7, b"\x1f\x8c\x08" + b"\x00" * 7, header(8, name=b"x")[:-1],
                header(4, extra=b"abcdef")[:-2], header(2, bad_hcrc=True), b"\x1f\x8b\x08\x20" + b"\x00" * 6, b"\x1f\x8b"]:
        with pytest.raises(PhiError):
            phi.gzip_header(bad)
    golden = open(os.path.join(ROOT, "tests", "golden", "data", "CHM13_reads.fq.gz"), "rb").read(4096)
    assert phi.gzip_header(golden) == golden.index(b"\x00", 10) + 1         # FNAME


@pytest.fixture(scope="module")
def inflate_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("asm") / "inflate.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), SRC],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


def _meta(asm, name):
    entries = asm.split("  - .agpr_count:")
    hits = [e for e in entries[1:] if re.search(r"\.name:\s+\S*" + re.escape(name), e)]
    assert len(hits) == 1, f"{len(hits)} metadata entries for {name}"
    return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", hits[0])}


# the decoder at most 96 VGPRs (five waves per SIMD) and 6 KB of LDS per wave (26 waves per CU), the
# finder at most 128 VGPRs and 16 KB of LDS; no kernel uses scratch
BUDGET = {"phi_inflate_decode_kernel": (96, 6 << 10), "phi_inflate_find_kernel": (128, 16 << 10),
          "phi_inflate_tail_kernel": (32, 0), "phi_inflate_resolve_kernel": (32, 0), "phi_inflate_crc_kernel": (32, 1024)}


@pytest.mark.parametrize("kernel", list(BUDGET))
def test_inflate_kernels_stay_within_budget(inflate_asm, kernel):
    m = _meta(inflate_asm, kernel)
    vgpr, lds = BUDGET[kernel]
    assert m["vgpr_count"] <= vgpr, m
    assert m["group_segment_fixed_size"] <= lds, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
