"""gzip inflated on the GPU (phi_amd.inflate, include/phi_amd.h phi_inflate): every output byte for byte against zlib."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

SMALL = 4096                                     # a forced small chunk: thousands of chunks, every path of the chain


@pytest.fixture(scope="module")
def phi():
    import __graft_entry__
    __graft_entry__.ensure_built()
    import phi_amd
    return phi_amd


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    return c.compress(data) + c.flush()


def synth_fastq(n_bytes, seed):
    """reads sampled from a random backbone with substitutions, Illumina-like qualities: repeats at every distance"""
    rng = np.random.default_rng(seed)
    backbone = rng.choice(np.frombuffer(b"ACGT", np.uint8), 1 << 20)
    qual = np.frombuffer(b"#+2:FFF", np.uint8)
    out, size, i = [], 0, 0
    while size < n_bytes:
        p = int(rng.integers(0, len(backbone) - 150))
        r = backbone[p:p + 150].copy()
        sub = rng.random(150) < 0.01
        r[sub] = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(sub.sum()))
        q = qual[np.minimum(rng.geometric(0.6, 150), len(qual)) - 1]
        rec = b"@read_%d/1\n%s\n+\n%s\n" % (i, r.tobytes(), q.tobytes())
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)


def wrapped_fasta(n_bytes, seed):
    rng = np.random.default_rng(seed)
    seq = rng.choice(np.frombuffer(b"ACGTN", np.uint8), n_bytes, p=[0.29, 0.21, 0.21, 0.29, 0.0]).tobytes()
    seq = seq[: n_bytes // 2] * 2                                              # long repeats as well
    lines = [seq[i:i + 60] for i in range(0, len(seq), 60)]
    return b">chr_test synthetic\n" + b"\n".join(lines) + b"\n"


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(77)
    gfa = gzip.open(os.path.join(DATA, "MHC_4.gfa.gz")).read(8 << 20)
    period = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    return {
        "fastq": synth_fastq(8 << 20, 1),
        "fasta": wrapped_fasta(2 << 20, 2),
        "gfa": gfa,
        "random": rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes(),
        "one_byte": b"a" * (4 << 20),
        "period_32768": period * 64 + period[:1000],
    }


def test_golden_reads_fixture(phi):
    from phi_amd import _capi
    data = open(os.path.join(DATA, "CHM13_reads.fq.gz"), "rb").read()
    assert data[:4] == b"\x1f\x8b\x08\x08"                                   # FNAME, no FEXTRA: single-stream gzip
    want = gzip.decompress(data)
    for chunk in (0, SMALL):
        out, info = phi.inflate(data, chunk_bytes=chunk)
        assert out == want
        c = chunk or _capi.PHI_INFLATE_CHUNK_DEFAULT
        assert info["in_bytes"] == len(data) and info["out_bytes"] == len(want) and info["members"] == 1
        assert info["chunks"] == (len(data) + c - 1) // c
        assert info["confirmed"] + info["redecoded"] == info["chunks"] - 1
        assert info["confirmed"] >= min(10, info["chunks"] - 1)              # (a chunk smaller than a block may hold no start)
        assert info["marker_bytes"] > 0 and info["device_ms"] > 0


SETTINGS = {
    "stored": (0, zlib.Z_DEFAULT_STRATEGY), "l1": (1, zlib.Z_DEFAULT_STRATEGY), "l6": (6, zlib.Z_DEFAULT_STRATEGY),
    "l9": (9, zlib.Z_DEFAULT_STRATEGY), "filtered": (6, zlib.Z_FILTERED), "huffman_only": (6, zlib.Z_HUFFMAN_ONLY),
    "rle": (6, zlib.Z_RLE), "fixed": (6, zlib.Z_FIXED),
}


@pytest.mark.parametrize("kind", ["fastq", "fasta", "gfa", "random", "one_byte", "period_32768"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_matrix_matches_zlib_at_every_chunk_size(phi, inputs, kind, setting):
    text = inputs[kind]
    comp = gz(text, *SETTINGS[setting])
    small, info_s = phi.inflate(comp, chunk_bytes=SMALL)
    assert small == text, (kind, setting, len(small), len(text))
    assert info_s["out_bytes"] == len(text) and info_s["members"] == 1
    default, _ = phi.inflate(comp)
    assert default == text


def test_without_the_finder_every_chunk_goes_through_confirmation(phi, inputs):
    text = inputs["fastq"][: 2 << 20]
    comp = gz(text, 6)
    out, info = phi.inflate(comp, chunk_bytes=SMALL, finder=False)
    assert out == text
    assert info["confirmed"] == 0 and info["redecoded"] == info["chunks"] - 1 and info["chunks"] > 100


def test_sync_and_full_flush_points(phi, inputs):
    text = inputs["fastq"][: 3 << 20]
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    parts, step = [], 100_003
    for k, i in enumerate(range(0, len(text), step)):
        parts.append(c.compress(text[i:i + step]))
        parts.append(c.flush(zlib.Z_SYNC_FLUSH if k % 2 else zlib.Z_FULL_FLUSH))
    parts.append(c.flush())
    comp = b"".join(parts)
    assert gzip.decompress(comp) == text
    for chunk in (SMALL, 0):
        assert phi.inflate(comp, chunk_bytes=chunk)[0] == text


def test_decoders_that_outgrow_the_capacity_guess_decode_again(phi):
    """One member of 1 MiB of random bytes, then 8 MiB of zeros: ISIZE over the compressed size is about 9, so a decoder's
    symbol capacity is about 50 K, while a 4 KB chunk of the zeros inflates a thousandfold: its decoder overflows and runs
    a second time at its true size."""
    rng = np.random.default_rng(4)
    text = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes() + bytes(8 << 20)
    comp = gz(text, 6)
    assert 8 < len(text) / len(comp) < 10
    for chunk in (SMALL, 0):
        out, info = phi.inflate(comp, chunk_bytes=chunk)
        assert out == text
        assert info["members"] == 1 and info["out_bytes"] == len(text)


def member(payload, flags=0, extra=b"", name=b"", comment=b""):
    """one gzip member with a header built here (FTEXT aside, every flag RFC 1952 defines)"""
    h = bytearray(b"\x1f\x8b\x08" + bytes([flags]) + struct.pack("<I", 0) + b"\x00\x03")
    if flags & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        h += name + b"\x00"
    if flags & 16:
        h += comment + b"\x00"
    if flags & 2:
        h += struct.pack("<H", zlib.crc32(bytes(h)) & 0xffff)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return bytes(h) + c.compress(payload) + c.flush() + struct.pack("<II", zlib.crc32(payload), len(payload) & 0xffffffff)


def test_concatenated_members_with_every_header_field(phi, inputs):
    fq = inputs["fastq"]
    pieces = [fq[:1 << 20], b"", fq[1 << 20:(3 << 20) // 2], fq[(3 << 20) // 2:2 << 20], b"", b"x"]
    comp = (member(pieces[0], 4 | 8, extra=b"AB\x02\x00zz", name=b"reads.fq")
            + gzip.compress(pieces[1], mtime=0)
            + member(pieces[2], 16 | 2, comment=b"a comment")
            + member(pieces[3], 2 | 4 | 8 | 16, extra=b"\x00" * 300, name=b"n", comment=b"c")
            + member(pieces[4], 8, name=b"empty")
            + member(pieces[5]))
    want = b"".join(pieces)
    assert gzip.decompress(comp) == want
    for chunk in (SMALL, 0):
        out, info = phi.inflate(comp, chunk_bytes=chunk)
        assert out == want and info["members"] == 6


def test_bgzf_through_the_same_call(phi):
    data = open(os.path.join(DATA, "MHC_4.gfa.gz"), "rb").read()
    assert data[12:14] == b"BC"                                               # BGZF: many members with an FEXTRA
    want = gzip.decompress(data)
    out, info = phi.inflate(data)
    assert out == want and info["members"] > 10


def stray_distance_stream():
    """a fixed-Huffman block whose first symbol copies from distance 1: before the start of the stream"""
    bits = []

    def put(v, n, rev=False):
        if rev:
            bits.extend((v >> (n - 1 - k)) & 1 for k in range(n))
        else:
            bits.extend((v >> k) & 1 for k in range(n))
    put(1, 1)
    put(1, 2)                                     # BFINAL, BTYPE = 01
    put(0b0000001, 7, rev=True)                   # length symbol 257 (length 3)
    put(0, 5, rev=True)                           # distance symbol 0 (distance 1)
    put(0, 7, rev=True)                           # end of block
    bits += [0] * (-len(bits) % 8)
    raw = bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", zlib.crc32(b"\0\0\0"), 3)


def test_corrupt_streams_are_errors_and_the_process_goes_on(phi, inputs):
    from phi_amd import PHI_ERR_INVALID, PhiError
    text = inputs["fastq"][: 1 << 20]
    good = gz(text, 6)
    for bit in range(10 * 8 + 17, 10 * 8 + 200):                              # inside the first dynamic block's header
        flipped_header = bytearray(good)
        flipped_header[bit // 8] ^= 1 << (bit % 8)
        try:
            zlib.decompress(bytes(flipped_header), 31)
        except zlib.error:
            break
    bad = {
        "crc": good[:-8] + bytes([good[-8] ^ 1]) + good[-7:],
        "isize": good[:-4] + bytes([good[-4] ^ 1]) + good[-3:],
        "truncated_block": good[: len(good) // 2],
        "truncated_trailer": good[:-3],
        "huffman_header": bytes(flipped_header),
        "distance": stray_distance_stream(),
    }
    for name, data in bad.items():
        with pytest.raises(Exception):
            gzip.decompress(data)
        for chunk in (SMALL, 0):
            with pytest.raises(PhiError) as e:
                phi.inflate(data, chunk_bytes=chunk)
            assert e.value.status == PHI_ERR_INVALID, (name, e.value)
    assert phi.inflate(good, chunk_bytes=SMALL)[0] == text


def test_output_beyond_4_gib(phi):
    n = (4 << 30) + 12345
    c = zlib.compressobj(9, zlib.DEFLATED, 31)
    block = b"\x07" * (64 << 20)
    parts = [c.compress(block) for _ in range(n // len(block))] + [c.compress(block[: n % len(block)]), c.flush()]
    comp = b"".join(parts)
    assert len(comp) < 16 << 20
    out, info = phi.inflate(comp, chunk_bytes=64 << 10, as_array=True)
    assert len(out) == n == info["out_bytes"]
    assert zlib.crc32(out) == struct.unpack("<I", comp[-8:-4])[0]
    assert int(out[0]) == 7 and int(out[-1]) == 7


def test_distance_into_the_previous_member_found_across_pieces(phi, inputs):
    """A second member whose first block reaches back into the first member (deflated with the first member's tail as a
    preset dictionary), placed so that its deflate data starts exactly on a chunk: the chunk's decoder starts there and
    leaves markers, and resolution finds them reaching before their member."""
    from phi_amd import PHI_ERR_INVALID, PhiError
    a, b = inputs["fastq"][: 1 << 20], inputs["fastq"][(1 << 20) - 200_000: (1 << 20) + 300_000]
    m1 = member(a)
    xlen = -(len(m1) + 12) % SMALL
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, a[-32768:])
    body = c.compress(b) + c.flush()
    m2 = b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\x03" + struct.pack("<H", xlen) + b"\x00" * xlen
    assert (len(m1) + len(m2)) % SMALL == 0
    data = m1 + m2 + body + struct.pack("<II", zlib.crc32(b), len(b))
    with pytest.raises(Exception):
        gzip.decompress(data)
    with pytest.raises(PhiError) as e:
        phi.inflate(data, chunk_bytes=SMALL)
    assert e.value.status == PHI_ERR_INVALID and "reaches before the start of its member" in e.value.detail, e.value


def test_park_gzip_stream_pieces_and_parity_with_add_reads(phi, inputs):
    """Compressed slices of 1 byte, 7 KB and the rest into a park: the fetched pieces are the text, none larger than the
    piece size; taken by phi_add_reads_text_parked they give the reads_stats() and solve() of add_reads of the same text."""
    from oracle import oracle as O
    text = inputs["fastq"][: 3 << 20]
    text = text[: text.rfind(b"\n@") + 1]
    comp = gz(text, 6)
    piece = 256 << 10
    park = phi.TextPark(0)
    idx, info = park.add_gzip([comp[:1], comp[1:7169], comp[7169:]], piece)
    pieces = [park.fetch(i) for i in idx]
    assert b"".join(pieces) == text and max(map(len, pieces)) <= piece and len(idx) == -(-len(text) // piece)
    assert info["out_bytes"] == len(text) and info["members"] == 1

    g = O.parse_gfa(os.path.join(DATA, "test.gfa"))
    A = g.arrays()

    def context():
        ctx = phi.Context(0)
        ctx.set_params(k=3, w=2, threshold=1.0, recombination=100)
        ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])
        return ctx
    parked = context()
    parked.reads_text_begin(piece)
    for i in idx:
        assert not parked.add_reads_text_parked(park, i)
    rest, taken = parked.reads_text_end()
    assert taken + len(rest) == len(text)
    if rest:                                                  # (the last record, as the command line's host reader takes it)
        from phi_amd import ilp_index as H
        hb, ho = H.reads_of_text(rest, [], stream_offset=taken)
        parked.add_reads((hb, ho))
    plain = context()
    lines = text.split(b"\n")
    plain.add_reads([lines[i] for i in range(1, len(lines) - 1, 4)])
    assert parked.reads_stats() == plain.reads_stats()
    a, b = parked.solve(), plain.solve()
    assert a["objective"] == b["objective"] and np.array_equal(a["path_vtx"], b["path_vtx"]) and np.array_equal(a["path_hap"], b["path_hap"])
    parked.close()
    plain.close()
    # a corrupt stream: an error, no piece added, the park still works
    n_before = len(idx)
    with pytest.raises(phi.PhiError):
        park.add_gzip([comp[:-9] + bytes([comp[-9] ^ 1]) + comp[-8:]], piece)
    idx2, _ = park.add_gzip([comp], piece)
    assert idx2[0] == idx[-1] + 1 and len(idx2) == n_before
    park.close()
