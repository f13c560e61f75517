"""The BGZF indexes restated in plain Python, for the tests of phi_deflate_bgzf_indexed: a per-line writer of the .tbi rules of
include/phi_amd.h, a reader that answers region queries through a .tbi as the tabix specification describes it, and a reader of
FASTA slices through .gzi + .fai.  A helper, no test; nothing here shares code with phi_amd.  bcftools, tabix, samtools and
pysam are not at hand, so the yardstick is the specification, restated here."""
import bisect
import struct
import zlib

BLOCK = 65280
MAX_END = 1 << 29
LEVELS = ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1))
GZI, TBI_VCF = 1, 2


class Invalid(ValueError):
    """the text breaks a rule of the VCF preset (PHI_ERR_INVALID)"""


class Unsupported(ValueError):
    """the text needs what is not written (PHI_ERR_UNSUPPORTED)"""


# ------------------------------------------------------------------ shared: members, lines, records, bins

def member_offsets(data):
    """off[0..nb] of a BGZF file that ends with the EOF block: where every member begins, then where the EOF block does"""
    off, pos = [], 0
    while pos < len(data):
        off.append(pos)
        pos += struct.unpack_from("<H", data, pos + 16)[0] + 1
    assert pos == len(data) and len(off) >= 1
    return off


def virtual_offset(off, p):
    return (off[p // BLOCK] << 16) | (p % BLOCK)


def lines_of(text):
    """(start, next start, line without its newline) of every line; a last line without a newline counts"""
    out, pos = [], 0
    while pos < len(text):
        nl = text.find(b"\n", pos)
        end = len(text) if nl < 0 else nl
        out.append((pos, min(end + 1, len(text)), text[pos:end]))
        pos = end + 1
    return out


def _number(b):
    if not 1 <= len(b) <= 10 or not all(48 <= c <= 57 for c in b):
        return None
    return int(b)


def record_of(line):
    """(contig name, beg, end) of a record line, by the rules of the header"""
    f = line.split(b"\t")
    if len(f) < 8:
        raise Invalid("fewer than 8 fields")
    pos = _number(f[1])
    if pos is None:
        raise Invalid("POS")
    beg = max(pos - 1, 0)
    end = beg + len(f[3])
    for item in f[7].split(b";"):
        if item.startswith(b"END="):
            end = _number(item[4:])
            if end is None:
                raise Invalid("END")
            break
    if end <= beg:
        end = beg + 1
    if end > MAX_END:
        raise Unsupported("end beyond 2^29")
    if len(f[0]) > 1024:
        raise Unsupported("contig name")
    return f[0], beg, end


def reg2bin(beg, end):
    end -= 1
    for shift, first in LEVELS:
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    """every bin that can hold a record overlapping [beg, end)"""
    end -= 1
    bins = [0]
    for shift, first in reversed(LEVELS):
        bins.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


def overlapping(text, name, beg, end):
    """brute force: the record lines of contig `name` that overlap [beg, end), in file order"""
    out = []
    for _, _, line in lines_of(text):
        if not line.startswith(b"#"):
            c, b, e = record_of(line)
            if c == name and b < end and e > beg:
                out.append(line)
    return out


# ------------------------------------------------------------------ (b) the writer, line by line

def tbi_bytes(text, off):
    """the uncompressed bytes of the .tbi of text, whose BGZF members begin at off[0..nb]; and its counts"""
    contigs, n_rec, n_meta = [], 0, 0           # [name, [(bin, vbeg, vend)] chunks in file order, {window: offset}, max end]
    last = None                                 # (name, pos, bin) of the previous record
    for start, nxt, line in lines_of(text):
        if not line:
            raise Invalid("an empty line")
        if line.startswith(b"#"):
            n_meta += 1
            continue
        name, beg, end = record_of(line)
        pos = int(line.split(b"\t")[1])
        n_rec += 1
        b = reg2bin(beg, end)
        vbeg, vend = virtual_offset(off, start), virtual_offset(off, nxt)
        if last is None or last[0] != name:
            if any(c[0] == name for c in contigs):
                raise Invalid("a contig comes back")
            contigs.append([name, [], {}, 0])
            new_chunk = True
        else:
            if pos < last[1]:
                raise Invalid("POS goes back")
            new_chunk = b != last[2]
        c = contigs[-1]
        if new_chunk:
            c[1].append([b, vbeg, vend])
        else:
            c[1][-1][2] = vend
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            c[2][w] = min(c[2].get(w, vbeg), vbeg)
        c[3] = max(c[3], end)
        last = (name, pos, b)
    names = b"".join(c[0] + b"\0" for c in contigs)
    out = [b"TBI\1", struct.pack("<8i", len(contigs), 2, 1, 2, 0, ord("#"), 0, len(names)), names]
    counts = {"records": n_rec, "meta_lines": n_meta, "contigs": len(contigs), "bins": 0, "chunks": 0, "windows": 0}
    for _, chunks, windows, max_end in contigs:
        bins = sorted({k[0] for k in chunks})
        out.append(struct.pack("<i", len(bins)))
        for b in bins:
            mine = [k for k in chunks if k[0] == b]
            out.append(struct.pack("<Ii", b, len(mine)))
            out.extend(struct.pack("<QQ", k[1], k[2]) for k in mine)
        n_win = ((max_end - 1) >> 14) + 1
        lin, prev = [], 0
        for w in range(n_win):
            prev = windows.get(w, prev)
            lin.append(prev)
        out.append(struct.pack("<i", n_win) + struct.pack(f"<{n_win}Q", *lin))
        counts["bins"] += len(bins)
        counts["chunks"] += len(chunks)
        counts["windows"] += n_win
    out.append(struct.pack("<Q", 0))
    return b"".join(out), counts


def gzi_bytes(off):
    nb = len(off) - 1
    return struct.pack("<Q", max(nb - 1, 0)) + b"".join(struct.pack("<QQ", off[b], BLOCK * b) for b in range(1, nb))


# ------------------------------------------------------------------ (a) the reader

def inflate_member(data, pos):
    """(text, size) of the BGZF member at data[pos:]"""
    assert data[pos:pos + 4] == b"\x1f\x8b\x08\x04" and data[pos + 12:pos + 14] == b"BC", pos
    size = struct.unpack_from("<H", data, pos + 16)[0] + 1
    return zlib.decompress(data[pos + 18:pos + size - 8], -15), size


def inflate_all(data):
    out, pos = [], 0
    while pos < len(data):
        t, size = inflate_member(data, pos)
        out.append(t)
        pos += size
    return b"".join(out)


def parse_tbi(index_file):
    """a .tbi file (BGZF) -> {"names": [...], "bins": [{bin: [(beg, end)]}], "lin": [[...]], the header's fields}"""
    b = inflate_all(index_file)
    assert b[:4] == b"TBI\1"
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", b, 4)
    at = 36
    names = b[at:at + l_nm].split(b"\0")[:-1] if l_nm else []
    assert len(names) == n_ref and b[at:at + l_nm] == b"".join(n + b"\0" for n in names)
    at += l_nm
    bins, lin = [], []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", b, at)
        at += 4
        mine, order = {}, []
        for _ in range(n_bin):
            bn, n_chunk = struct.unpack_from("<Ii", b, at)
            at += 8
            assert bn not in mine and n_chunk > 0
            mine[bn] = [struct.unpack_from("<QQ", b, at + 16 * k) for k in range(n_chunk)]
            order.append(bn)
            at += 16 * n_chunk
        assert order == sorted(order)
        (n_intv,) = struct.unpack_from("<i", b, at)
        lin.append(list(struct.unpack_from(f"<{n_intv}Q", b, at + 4)))
        at += 4 + 8 * n_intv
        bins.append(mine)
    assert struct.unpack_from("<Q", b, at) == (0,) and at + 8 == len(b)
    return {"names": names, "bins": bins, "lin": lin, "format": fmt, "col_seq": col_seq, "col_beg": col_beg, "col_end": col_end,
            "meta": meta, "skip": skip}


def read_chunk(data, vbeg, vend, cache):
    """the bytes between two virtual offsets of a BGZF file, inflating only the members they touch"""
    out, pos, skip = [], vbeg >> 16, vbeg & 0xffff
    while pos < (vend >> 16):
        if pos not in cache:
            cache[pos] = inflate_member(data, pos)
        t, size = cache[pos]
        out.append(t[skip:])
        pos, skip = pos + size, 0
    if vend & 0xffff:
        if pos not in cache:
            cache[pos] = inflate_member(data, pos)
        out.append(cache[pos][0][skip:vend & 0xffff])
    return b"".join(out)


def query(data, tbi, name, beg, end, cache=None):
    """the record lines of contig `name` overlapping [beg, end), found through the index alone, in file order"""
    cache = {} if cache is None else cache
    if name not in tbi["names"] or end <= beg:
        return []
    c = tbi["names"].index(name)
    lin = tbi["lin"][c]
    if (beg >> 14) >= len(lin):
        return []                                   # beyond the last end of the contig
    least = lin[beg >> 14]
    chunks = sorted(k for b in reg2bins(beg, min(end, MAX_END)) for k in tbi["bins"][c].get(b, ()) if k[1] > least)
    out = []
    for vbeg, vend in chunks:
        for line in read_chunk(data, vbeg, vend, cache).split(b"\n"):
            if line and not line.startswith(b"#"):
                n, b, e = record_of(line)
                if n == name and b < end and e > beg:
                    out.append(line)
    return out


# ------------------------------------------------------------------ (c) FASTA slices through .gzi + .fai

def fai_fields(fai):
    name, length, offset, line_bases, line_width = fai.rstrip(b"\n").split(b"\t")
    return name, int(length), int(offset), int(line_bases), int(line_width)


def fai_offset(fai, i):
    """where base i stands in the uncompressed file"""
    _, _, offset, line_bases, line_width = fai_fields(fai)
    return offset + (i // line_bases) * line_width + i % line_bases


def fasta_slice(data, gzi, fai, s, n, touched=None):
    """bases [s, s + n) of the one sequence of a BGZF FASTA, inflating only the members that hold them"""
    if n == 0:
        return b""
    (count,) = struct.unpack_from("<Q", gzi, 0)
    pairs = [(0, 0)] + [struct.unpack_from("<QQ", gzi, 8 + 16 * k) for k in range(count)]
    assert len(gzi) == 8 + 16 * count
    u0, u1 = fai_offset(fai, s), fai_offset(fai, s + n - 1) + 1
    starts = [u for _, u in pairs]
    m = bisect.bisect_right(starts, u0) - 1
    out = []
    while m < len(pairs) and pairs[m][1] < u1:
        t, _ = inflate_member(data, pairs[m][0])
        if touched is not None:
            touched.add(m)
        lo = pairs[m][1]
        out.append(t[max(u0 - lo, 0):u1 - lo])
        m += 1
    return b"".join(out).replace(b"\n", b"")
