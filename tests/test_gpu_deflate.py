"""GPU: phi_deflate_bgzf (phi_amd.deflate_bgzf), the BGZF writer on the device.  Every output is split into its members and
checked field by field (bgzf_util: each member inflated on its own by zlib, so no copy may reach into the member before),
inflated by Python's gzip, and inflated by the project's own phi_amd.inflate; all three must give the input back.  The inputs
are the smallest at which the kernel can go wrong: the sizes around a block, one literal with copies that overlap themselves,
bytes that do not compress (stored blocks), copies at the far edge of the window and just beyond it, copies that would cross a
block, a code that needs its length limit, and the text the writer is meant for."""
import ctypes as C
import gzip
import os
import zlib

import numpy as np
import pytest

import bgzf_util
import deflate_writer as W
from conftest import DATA

pytestmark = pytest.mark.gpu

B = bgzf_util.BLOCK
FIB = [1, 1]
while len(FIB) < 22:
    FIB.append(FIB[-1] + FIB[-2])
assert sum(FIB) == 46367


@pytest.fixture(scope="module")
def phi():
    import __graft_entry__
    __graft_entry__.ensure_built()
    import phi_amd
    return phi_amd


@pytest.fixture(scope="module")
def vcf_text():
    with gzip.open(os.path.join(DATA, "MHC_4.vcf.gz"), "rb") as f:
        return f.read()


def _roundtrip(phi, data, match=True, eof=True):
    """compress, check the three ways back; returns (file, info, members)"""
    out, info = phi.deflate_bgzf(data, match=match, eof=eof, with_info=True)
    mem = bgzf_util.members(out, eof=eof)
    assert b"".join(t for _, t in mem) == data
    blocks = -(-len(data) // B)
    assert len(mem) == blocks + (1 if eof else 0)
    assert [len(t) for _, t in mem[:blocks]] == [B] * (blocks - 1) + ([len(data) - B * (blocks - 1)] if blocks else [])
    assert (info["in_bytes"], info["out_bytes"], info["blocks"]) == (len(data), len(out), blocks)
    assert 0 <= info["stored_blocks"] <= blocks and info["device_ms"] >= 0
    if out:
        assert gzip.decompress(out) == data
        text, inf = phi.inflate(out)
        assert text == data and inf["members"] == len(mem)
    return out, info, mem


def _walk(member):
    """the walker's statistics of one member's raw DEFLATE stream"""
    text, st, end = W.walk(member[18:-8])
    assert (end + 7) // 8 == len(member) - 26
    return text, st


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, B - 1, B, B + 1, 2 * B + 1])
def test_sizes_around_a_block(phi, n):
    data = W.fastq_like(max(n, 1), 3)[:n]
    out, info, mem = _roundtrip(phi, data)
    if n == 0:
        assert out == bgzf_util.EOF == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    if n in (0, 1):
        bare, _, _ = _roundtrip(phi, data, eof=False)
        assert bare + bgzf_util.EOF == out and (n or bare == b"")
    if n >= B - 1:
        assert info["stored_blocks"] == (1 if n in (B + 1, 2 * B + 1) else 0)       # (a block of one byte is stored: 6 bytes against 7 and more)
        # bases and qualities take about 2 bits a byte under a Huffman code and the header lines are digits: below half the
        # input even with no copy at all
        assert info["matches"] > 0 and len(out) < 0.5 * n


def test_one_literal_and_copies_that_overlap_themselves(phi):
    data = b"A" * B
    out, info, mem = _roundtrip(phi, data)
    assert len(out) <= 400, len(out)
    text, st = _walk(mem[0][0])
    assert text == data and st["blocks"] == {0: 0, 1: 0, 2: 1}
    assert st["one_code_dist_trees"] == 1 and st["one_code_dist_trees_used"] == 1 and st["max_distance"] == 1
    assert any(d < n for d, n in st["overlaps"]) and st["matches"] == info["matches"] and info["match_bytes"] == B - 1
    # one distinct literal and nothing to copy from: still two codes, the literal and end-of-block; no distance code at all
    out, info, mem = _roundtrip(phi, b"AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA", match=False)
    text, st = _walk(mem[0][0])
    assert st["blocks"][2] == 1 and st["zero_code_dist_trees"] == 1 and st["one_code_lit_trees"] == 0 and st["max_lit_bits"] == 1


def test_random_bytes_are_stored(phi):
    data = W.random_bytes(70000, 5)
    out, info, mem = _roundtrip(phi, data)
    assert info["stored_blocks"] == 2 and info["matches"] == 0
    for m, text in mem[:2]:
        assert len(m) <= len(text) + 31
        assert _walk(m)[1]["blocks"] == {0: 1, 1: 0, 2: 0}
    assert len(out) <= phi._capi.load().phi_deflate_bgzf_bound(len(data))


def test_the_far_edge_of_the_window(phi):
    period = W.random_bytes(32768, 6)
    data = (period * 2)[:B]
    out, info, mem = _roundtrip(phi, data)
    text, st = _walk(mem[0][0])
    assert st["max_distance"] == 32768 and info["matches"] > 0 and info["stored_blocks"] == 0
    assert st["matches"] == info["matches"] and len(out) < 0.6 * B
    # one byte further nothing lies within the window (LDS holds all 65 280 bytes: the format is what forbids the copy)
    period = W.random_bytes(32769, 7)
    data = (period * 2)[:B]
    out, info, mem = _roundtrip(phi, data)
    assert info["matches"] == 0 and info["stored_blocks"] == 1


def test_no_copy_crosses_a_block(phi):
    period = W.random_bytes(1000, 8)
    data = (period * 200)[:200_000]
    out, info, mem = _roundtrip(phi, data)                              # (each member is inflated alone in there)
    assert len(mem) == 5 and info["stored_blocks"] == 0
    print("period 1000: ratio %.4f, %d copies" % (len(out) / len(data), info["matches"]))
    assert len(out) <= 0.05 * len(data)
    for m, text in mem[:4]:
        assert len(m) >= 1000                                           # every block pays for its own first period


def test_huffman_side_alone_on_dna(phi):
    rng = np.random.default_rng(9)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 400_000)]
    lines = [seq[i:i + 60].tobytes() for i in range(0, len(seq), 60)]
    data = (b">random_dna\n" + b"\n".join(lines) + b"\n")[:400_000]
    out, info, mem = _roundtrip(phi, data, match=False)
    print("DNA, literals only: ratio %.4f" % (len(out) / len(data)))
    assert info["matches"] == 0 and info["stored_blocks"] == 0
    assert len(out) <= 0.30 * len(data)
    # and with copies allowed the parse must not pay more for them than for the literals
    out2, info2, _ = _roundtrip(phi, data)
    print("DNA, with copies: ratio %.4f, %d copies" % (len(out2) / len(data), info2["matches"]))
    assert len(out2) <= 0.30 * len(data)


def test_a_code_that_needs_its_length_limit(phi):
    rng = np.random.default_rng(10)
    data = np.concatenate([np.full(c, 40 + 3 * k, np.uint8) for k, c in enumerate(FIB)])
    rng.shuffle(data)
    data = data.tobytes()
    out, info, mem = _roundtrip(phi, data, match=False)
    text, st = _walk(mem[0][0])
    assert st["blocks"][2] == 1 and 12 <= st["max_lit_bits"] <= 15, st["max_lit_bits"]


def _zlib_blocks(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    total = 0
    for i in range(0, len(text), B):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        total += len(c.compress(text[i:i + B])) + len(c.flush()) + 26
    return total + 28


def test_vcf_text_beats_huffman_only_and_is_deterministic(phi, vcf_text):
    out, info, mem = _roundtrip(phi, vcf_text)
    huff = _zlib_blocks(vcf_text, 6, zlib.Z_HUFFMAN_ONLY)
    z1, z6 = _zlib_blocks(vcf_text, 1), _zlib_blocks(vcf_text, 6)
    n = len(vcf_text)
    # recorded, not asserted: the ratio beside zlib's levels 1 and 6 on the same blocks
    print("VCF text %d bytes: device %.4f (%.3f ms), zlib huffman-only %.4f, level 1 %.4f, level 6 %.4f; %d copies cover %d bytes"
          % (n, len(out) / n, info["device_ms"], huff / n, z1 / n, z6 / n, info["matches"], info["match_bytes"]))
    assert len(out) < huff
    assert info["stored_blocks"] == 0 and info["matches"] > 0
    # the same bytes from run to run, whatever ran in between
    other = W.fastq_like(300_000, 11)
    for _ in range(2):
        phi.deflate_bgzf(other)
        assert phi.deflate_bgzf(vcf_text) == out


def test_batches_do_not_change_the_bytes(phi):
    data = W.fastq_like(4 * B + 1000, 12)
    assert os.environ.get("PHI_DEFLATE_BATCH") is None
    want, info, _ = _roundtrip(phi, data)
    assert info["blocks"] == 5
    os.environ["PHI_DEFLATE_BATCH"] = "2"
    try:
        got, info2 = phi.deflate_bgzf(data, with_info=True)
    finally:
        del os.environ["PHI_DEFLATE_BATCH"]
    assert got == want and {k: v for k, v in info2.items() if k != "device_ms"} == {k: v for k, v in info.items() if k != "device_ms"}


def test_errors_and_capacity(phi):
    from phi_amd import _capi
    L = _capi.load()
    data = W.fastq_like(3000, 13)
    buf = np.frombuffer(data, np.uint8)
    out = np.full(8192, 0xEE, np.uint8)
    size, info = C.c_int64(-1), _capi.PhiDeflateInfo()
    call = lambda inp, n, cap, flags: L.phi_deflate_bgzf(0, inp, n, out.ctypes.data, cap, flags, C.byref(size), C.byref(info))
    INVALID = -1
    assert call(buf.ctypes.data, -1, 8192, 0) == INVALID and info.detail
    assert call(None, 10, 8192, 0) == INVALID
    assert call(buf.ctypes.data, 3000, 8192, 4) == INVALID and b"flags" in info.detail
    assert call(buf.ctypes.data, 3000, 8192, 0x100) == INVALID
    assert np.all(out == 0xEE)
    p = C.c_void_p(1)
    assert L.phi_deflate_bgzf_alloc(0, buf.ctypes.data, 3000, 8, C.byref(p), C.byref(size), C.byref(info)) == INVALID and not p.value
    with pytest.raises(phi.PhiError):
        phi.deflate_bgzf(data, device=-1)
    want = phi.deflate_bgzf(data)
    # one byte short: the size, and nothing copied
    assert call(buf.ctypes.data, 3000, len(want) - 1, 0) == 0 and size.value == len(want) and np.all(out == 0xEE)
    assert call(buf.ctypes.data, 3000, len(want), 0) == 0 and size.value == len(want)
    assert out[:len(want)].tobytes() == want and np.all(out[len(want):] == 0xEE)
    # n == 0 needs no input pointer
    assert call(None, 0, 8192, 0) == 0 and size.value == 28 and out[:28].tobytes() == bgzf_util.EOF
    assert call(None, 0, 0, 2) == 0 and size.value == 0
