"""BAM for the tests: a writer (struct + raw deflate in BGZF blocks), an independent sequential decoder used as the oracle,
and the FASTQ of the kept reads.  A plain module, stated from the SAM/BAM specification (sections 4.1 BGZF, 4.2 BAM); nothing
here shares code with phi_amd, and nothing was compared with samtools.

The reads of a BAM file: in file order, the sequences of the records with flag & 0x900 == 0 and l_seq > 0; a record with
flag & 0x10 holds the reverse complement of the read and is turned back.
"""
import struct
import zlib

CODES = b"=ACMGRSVTWYHKDBN"
_CODE_OF = {c: i for i, c in enumerate(CODES)}
_COMPLEMENT = dict(zip(b"ATCGMKRYVBHD=SWN", b"TAGCKMYRBVDH=SWN"))
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def revcomp(seq):
    return bytes(_COMPLEMENT[c] for c in reversed(seq))


def header(text=b"", refs=()):
    """magic, l_text, text, n_ref, n_ref x (l_name, name NUL, l_ref)."""
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        out += [struct.pack("<i", len(name) + 1), name, b"\x00", struct.pack("<i", length)]
    return b"".join(out)


def pack_seq(seq):
    """Two bases per byte, high nibble first."""
    codes = [_CODE_OF[c] for c in seq]
    if len(codes) & 1:
        codes.append(0)
    return bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))


def record(name, stored, flag=4, ref_id=-1, pos=-1, mapq=0, n_cigar=0, next_ref=-1, next_pos=-1, tlen=0, aux=b"", qual=None,
           block_size=None, l_seq=None):
    """One alignment record.  name: without its NUL (b"" gives l_read_name 1); stored: the sequence as the file holds it (the
    reverse complement of the read when flag & 0x10); the cigar is n_cigar operations `1M`.  block_size / l_seq override what
    is written in those fields (malformed records)."""
    n = len(stored)
    qual = bytes([30 + i % 11 for i in range(n)]) if qual is None else qual
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) + 1, mapq, 4680, n_cigar, flag, n if l_seq is None else l_seq,
                       next_ref, next_pos, tlen)
    body += name + b"\x00" + struct.pack("<I", 1 << 4) * n_cigar + pack_seq(stored) + qual + aux
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def aux_bytes(tag, data):
    """A `B` array of unsigned bytes: tag, 'B', 'C', count, the bytes."""
    return tag + b"BC" + struct.pack("<i", len(data)) + data


def bgzf(data, block_bytes=0xFF00, eof=True, level=6):
    """data in BGZF blocks of block_bytes inflated bytes each (<= 65 280): a gzip member with the BC extra field."""
    assert 1 <= block_bytes <= 0xFF00
    out = []
    for i in range(0, len(data), block_bytes):
        raw = data[i:i + block_bytes]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = co.compress(raw) + co.flush()
        bsize = len(comp) + 25
        out.append(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, bsize) + comp +
                   struct.pack("<II", zlib.crc32(raw) & 0xFFFFFFFF, len(raw)))
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def write_bam(path, inflated, block_bytes=0xFF00, eof=True):
    with open(path, "wb") as f:
        f.write(bgzf(inflated, block_bytes, eof))


class BamInvalid(Exception):
    """The stream is not valid BAM; offset: the byte offset in the inflated stream that says so (a wrong magic byte, the end of
    a stream cut inside its header, the first byte of a record that is not well-formed or that the stream ends in)."""

    def __init__(self, offset, why):
        super().__init__(f"{why} at byte offset {offset}")
        self.offset, self.why = offset, why


def parse_header(b):
    """(records_start, n_ref) of inflated bytes b."""
    for i in range(4):
        if i >= len(b):
            raise BamInvalid(len(b), "stream ends inside the header")
        if b[i] != b"BAM\x01"[i]:
            raise BamInvalid(i, "wrong magic")
    at = 4

    def i32(at):
        if at + 4 > len(b):
            raise BamInvalid(len(b), "stream ends inside the header")
        return struct.unpack_from("<i", b, at)[0]
    l_text = i32(at)
    if l_text < 0:
        raise BamInvalid(at, "negative l_text")
    at += 4 + l_text
    n_ref = i32(at)
    if n_ref < 0:
        raise BamInvalid(at, "negative n_ref")
    at += 4
    for _ in range(n_ref):
        l_name = i32(at)
        if l_name < 1:
            raise BamInvalid(at, "l_name below 1")
        at += 4 + l_name + 4
        if at > len(b):
            raise BamInvalid(len(b), "stream ends inside the header")
    return at, n_ref


def decode(b):
    """The oracle: a sequential walk of inflated BAM bytes.  Returns (reads, info): the kept reads as ASCII bytes in file
    order and the counters of phi_bam_info that do not depend on tiles.  Raises BamInvalid."""
    at, n_ref = parse_header(b)
    info = dict(n_records=0, n_kept=0, n_secondary_supplementary=0, n_empty=0, n_reverse=0, n_bases=0, n_ref=n_ref, header_bytes=at)
    reads = []
    while at < len(b):
        if at + 36 > len(b):
            raise BamInvalid(at, "stream ends inside a record")
        block_size, _ref, _pos, l_read_name, _mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiiBBHHHi", b, at)
        if l_read_name < 1 or l_seq < 0 or block_size < 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:
            raise BamInvalid(at, "record not well-formed")
        if at + 4 + block_size > len(b):
            raise BamInvalid(at, "stream ends inside a record")
        info["n_records"] += 1
        if flag & 0x900:
            info["n_secondary_supplementary"] += 1
        elif l_seq == 0:
            info["n_empty"] += 1
        else:
            s0 = at + 36 + l_read_name + 4 * n_cigar
            packed = b[s0:s0 + (l_seq + 1) // 2]
            seq = bytes(CODES[(packed[i >> 1] >> 4) if not i & 1 else (packed[i >> 1] & 15)] for i in range(l_seq))
            if flag & 0x10:
                seq = revcomp(seq)
                info["n_reverse"] += 1
            reads.append(seq)
            info["n_kept"] += 1
            info["n_bases"] += l_seq
        at += 4 + block_size
    lens = {len(r) for r in reads}
    info["one_length"] = lens.pop() if len(lens) == 1 else 0
    return reads, info


def fastq(reads, prefix=b"r"):
    """The FASTQ of the kept reads: four lines per record."""
    return b"".join(b"@" + prefix + str(i).encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
