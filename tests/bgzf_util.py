"""BGZF for the tests of the device's writer (phi_deflate_bgzf): a file split into its members by their BSIZE fields, every
field of the header checked, every member inflated on its own.  A helper, no test; nothing here shares code with phi_amd."""
import struct
import zlib

BLOCK = 65280                                            # input bytes per member, as htslib cuts them
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
assert len(EOF) == 28


def members(data, eof=True):
    """data as a list of (member bytes, its text).  Asserts for every member: ID1 ID2 CM = 1f 8b 08, FLG = 04 (FEXTRA alone),
    MTIME 0, XFL 0, OS ff, XLEN 6, the subfield 'B' 'C' of length 2, BSIZE = member size - 1 (so it fits 16 bits); the member
    holds ONE raw DEFLATE stream that zlib inflates with nothing before it (a copy reaching into the previous member would
    fail) and nothing left over, then CRC32 and ISIZE of that text; no text above BLOCK bytes.  With eof, the last member is
    the 28-byte EOF block, literally, and no earlier member is empty."""
    data = bytes(data)
    out, pos = [], 0
    while pos < len(data):
        assert pos + 18 <= len(data), "a member header is cut short"
        assert data[pos:pos + 4] == b"\x1f\x8b\x08\x04", (pos, data[pos:pos + 4])
        mtime, xfl, os_, xlen = struct.unpack_from("<IBBH", data, pos + 4)
        assert (mtime, xfl, os_, xlen) == (0, 0, 0xff, 6), (pos, mtime, xfl, os_, xlen)
        si1, si2, slen, bsize = struct.unpack_from("<BBHH", data, pos + 12)
        assert (si1, si2, slen) == (ord("B"), ord("C"), 2), (pos, si1, si2, slen)
        size = bsize + 1
        assert size >= 18 + 2 + 8 and pos + size <= len(data), (pos, size, len(data))
        m = data[pos:pos + size]
        d = zlib.decompressobj(-15)
        text = d.decompress(m[18:-8])
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", (pos, "the deflate stream does not end where the trailer begins")
        crc, isize = struct.unpack_from("<II", m, size - 8)
        assert crc == zlib.crc32(text) and isize == len(text) <= BLOCK, (pos, crc, zlib.crc32(text), isize, len(text))
        out.append((m, text))
        pos += size
    if eof:
        assert out and out[-1][0] == EOF, "the file does not end with the EOF block"
        assert all(len(t) > 0 for _, t in out[:-1]), "an empty member before the EOF block"
    return out


def text_of(data, eof=True):
    return b"".join(t for _, t in members(data, eof))
