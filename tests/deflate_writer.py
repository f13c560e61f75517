"""DEFLATE for the tests, written bit by bit: a writer with every choice of RFC 1951 in the caller's hand (block type and
BFINAL, code lengths per symbol, HLIT / HDIST / HCLEN, the use of code-length symbols 16 / 17 / 18, matches as symbols
with their extra bits), a gzip wrapper (RFC 1952), a walker (a plain inflater that reports which features a stream
holds), and the stream families of tests/test_cpu_deflate_writer.py and tests/test_gpu_deflate_shapes.py.

A plain module stated from the two RFCs; nothing here shares code or tables with phi_amd.  The walker is no reference:
zlib's inflater is.  The walker only shows that a stream holds the feature its test is named for.
"""
import functools
import random
import struct
import zlib

# RFC 1951 3.2.5, from its rule and not from a table: eight lengths without extra bits, then four symbols for each count of
# extra bits 1..5, then 258; four distances without extra bits, then two symbols for each count 1..13
LEXT = [0] * 8 + [e for e in range(1, 6) for _ in range(4)] + [0]
LBASE = [3 + k for k in range(8)]
for _e in LEXT[8:28]:
    LBASE.append(LBASE[-1] + (1 << LEXT[len(LBASE) - 1]))
LBASE.append(258)
DEXT = [0] * 4 + [e for e in range(1, 14) for _ in range(2)]
DBASE = [1]
for _k in range(1, 30):
    DBASE.append(DBASE[-1] + (1 << DEXT[_k - 1]))
CLORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
assert LBASE[28] == 258 and LBASE[27] == 227 and DBASE[29] == 24577 and DBASE[29] + (1 << DEXT[29]) - 1 == 32768


def kraft(lens):
    """the code space the lengths take, in units of 2^-15: 32768 is a complete code"""
    return sum(1 << (15 - l) for l in lens if l)


def canonical(lens):
    """{symbol: (code, length)} by RFC 1951 3.2.2 (codes of an oversubscribed set are cut to their length)"""
    top = max(lens, default=0)
    count = [0] * (top + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, code = [0] * (top + 2), 0
    for b in range(1, top + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


def flat_lengths(symbols, n, pad=True):
    """a complete code over `symbols` (the first ones get the shorter codes) as a list of n lengths; one symbol alone is
    padded with a second, unused one (pad) or left as a single code of length 1"""
    symbols = list(dict.fromkeys(symbols))
    if len(symbols) == 1 and pad:
        symbols.append(next(s for s in range(n) if s != symbols[0]))
    lens = [0] * n
    m = len(symbols)
    if m == 1:
        lens[symbols[0]] = 1
    elif m > 1:
        k = (m - 1).bit_length()
        short = (1 << k) - m
        for i, s in enumerate(symbols):
            lens[s] = k - 1 if i < short else k
        assert kraft(lens) == 32768
    return lens


def length_symbol(length):
    for i in range(28, -1, -1):
        if LBASE[i] <= length < LBASE[i] + (1 << LEXT[i]):
            return 257 + i, length - LBASE[i]
    raise ValueError(length)


def dist_symbol(dist):
    for i in range(29, -1, -1):
        if DBASE[i] <= dist < DBASE[i] + (1 << DEXT[i]):
            return i, dist - DBASE[i]
    raise ValueError(dist)


def rle_lengths(seq, rle=True):
    """the code-length symbols (symbol, extra) of a run of code lengths, greedy over 16 / 17 / 18 (rle) or plain"""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if rle and v == 0 and run >= 3:
            r = min(run, 138)
            out.append((17, r - 3) if r <= 10 else (18, r - 11))
            i += r
        elif rle and i > 0 and seq[i - 1] == v and run >= 3:
            r = min(run, 6)
            out.append((16, r - 3))
            i += r
        else:
            out.append((v, 0))
            i += 1
    return out


def expand_lengths(cl_syms):
    seq = []
    for s, x in cl_syms:
        if s < 16:
            seq.append(s)
        elif s == 16:
            seq += [seq[-1]] * (3 + x)
        else:
            seq += [0] * ((3 if s == 17 else 11) + x)
    return seq


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.nb = bytearray(), 0, 0

    def bits(self, v, n):
        """n bits of v, least significant first (header fields, extra bits)"""
        assert 0 <= v < (1 << n)
        self.acc |= v << self.nb
        self.nb += n
        while self.nb >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.nb -= 8

    def code(self, c, n):
        """a Huffman code of n bits, most significant first"""
        for k in range(n - 1, -1, -1):
            self.bits((c >> k) & 1, 1)

    def align(self):
        if self.nb:
            self.bits(0, 8 - self.nb)

    def raw(self, b):
        assert self.nb == 0
        self.out += b

    def bitpos(self):
        return len(self.out) * 8 + self.nb


class Deflate:
    """One raw DEFLATE stream.  `text` follows what an inflater would write (track=False for streams that are invalid)."""

    def __init__(self, track=True):
        self.w, self.text, self.track = BitWriter(), bytearray(), track
        self.lit = self.dst = None
        self.starts = []                                   # the bit offset of every block header

    def head(self, final, btype):
        self.starts.append(self.w.bitpos())
        self.w.bits(final, 1)
        self.w.bits(btype, 2)

    def stored(self, payload, final=0, length=None, nlen=None):
        self.head(final, 0)
        self.w.align()
        n = len(payload) if length is None else length
        self.w.bits(n, 16)
        self.w.bits(~n & 0xffff if nlen is None else nlen, 16)
        self.w.raw(payload)
        self.text += payload

    def fixed(self, final=0):
        self.head(final, 1)
        self.lit, self.dst = canonical(FIXED_LIT), canonical(FIXED_DIST)

    def dynamic(self, lit_lens, dist_lens, final=0, hlit=None, hdist=None, hclen=None, cl_syms=None, cl_lens=None, rle=True,
                check=True):
        """the header of a dynamic block from its code lengths.  hlit / hdist: the counts written (default: up to the last
        coded symbol); cl_syms: the code-length symbols [(symbol, extra)] (default: rle_lengths); cl_lens: the lengths of
        the code-length code by symbol (default: a flat complete code over the symbols used); hclen: how many are written."""
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        if hlit is None:
            hlit = max([257] + [s + 1 for s, l in enumerate(lit_lens) if l])
        if hdist is None:
            hdist = max([1] + [s + 1 for s, l in enumerate(dist_lens) if l])
        lit_lens = (lit_lens + [0] * hlit)[:hlit]
        dist_lens = (dist_lens + [0] * hdist)[:hdist]
        seq = lit_lens + dist_lens
        if cl_syms is None:
            cl_syms = rle_lengths(seq, rle)
        if check:
            assert expand_lengths(cl_syms) == seq
        if cl_lens is None:
            freq = {}
            for s, _ in cl_syms:
                freq[s] = freq.get(s, 0) + 1
            cl_lens = flat_lengths(sorted(freq, key=lambda s: -freq[s]), 19)
        need = max([4] + [k + 1 for k in range(19) if cl_lens[CLORD[k]]])
        if hclen is None:
            hclen = need
        assert not check or hclen >= need
        self.head(final, 2)
        self.w.bits(hlit - 257, 5)
        self.w.bits(hdist - 1, 5)
        self.w.bits(hclen - 4, 4)
        for k in range(hclen):
            self.w.bits(cl_lens[CLORD[k]], 3)
        cc = canonical(cl_lens)
        for s, x in cl_syms:
            if s not in cc and not check:
                continue                                   # (a spoilt code-length code: its inflater has stopped by now)
            self.w.code(*cc[s])
            if s >= 16:
                self.w.bits(x, {16: 2, 17: 3, 18: 7}[s])
        self.lit, self.dst = canonical(lit_lens), canonical(dist_lens)

    def sym(self, s):
        self.w.code(*self.lit[s])

    def literal(self, b):
        self.sym(b)
        self.text.append(b)

    def match_sym(self, ls, le, ds, de):
        """a match as (length symbol, its extra bits' value, distance symbol, its extra bits' value)"""
        self.sym(ls)
        self.w.bits(le, LEXT[ls - 257])
        self.w.code(*self.dst[ds])
        self.w.bits(de, DEXT[ds])
        if self.track:
            t, n, d = self.text, LBASE[ls - 257] + le, DBASE[ds] + de
            assert d <= len(t), "distance before the start of the stream"
            at = len(t) - d
            for k in range(n):
                t.append(t[at + k])

    def match(self, length, dist):
        self.match_sym(*length_symbol(length), *dist_symbol(dist))

    def eob(self):
        self.sym(256)

    def token(self, t):
        if isinstance(t, int):
            self.literal(t)
        elif len(t) == 2:
            self.match(*t)
        else:
            self.match_sym(*t)

    def block(self, tokens, final=0, kind=2, dist="pad", **header):
        """a whole block of tokens (a literal byte, (length, distance) or (lsym, lextra, dsym, dextra)) over flat complete
        codes of the symbols it uses.  dist: 'pad' two distance codes at least (as zlib writes), 'natural' as many as used:
        none, or one of length 1."""
        if kind == 0:
            return self.stored(bytes(tokens), final)
        if kind == 1:
            self.fixed(final)
        else:
            lits, dsts = [256], []
            for t in tokens:
                if isinstance(t, int):
                    lits.append(t)
                else:
                    lits.append(length_symbol(t[0])[0] if len(t) == 2 else t[0])
                    dsts.append(dist_symbol(t[1])[0] if len(t) == 2 else t[2])
            lit_lens = flat_lengths(lits, 286)
            if dist == "pad":
                dist_lens = flat_lengths(dsts or [0], 30)
            else:
                dist_lens = flat_lengths(dsts, 30, pad=False) if dsts else [0]
            self.dynamic(lit_lens, dist_lens, final, **header)
        for t in tokens:
            self.token(t)
        self.eob()

    def finish(self):
        self.w.align()
        return bytes(self.w.out)


# ---------------------------------------------------------------------------------------------------------------- gzip

def gzip_header(total=10):
    """a member header of exactly `total` bytes (10, or 12 and more): the padding is an FEXTRA field, and an FCOMMENT
    beyond its 65535 bytes"""
    assert total == 10 or total >= 12
    if total == 10:
        return b"\x1f\x8b\x08\x00" + b"\x00" * 4 + b"\x00\x03"
    xlen = min(total - 12, 65535)
    rest = total - 12 - xlen
    if rest == 1:
        xlen, rest = xlen - 1, 2
    flags = 4 | (16 if rest else 0)
    h = b"\x1f\x8b\x08" + bytes([flags]) + b"\x00" * 4 + b"\x00\x03" + struct.pack("<H", xlen) + b"\x00" * xlen
    if rest:
        h += b"c" * (rest - 1) + b"\x00"
    assert len(h) == total
    return h


def member(raw, text, header_len=10):
    return gzip_header(header_len) + raw + struct.pack("<II", zlib.crc32(bytes(text)), len(text) & 0xffffffff)


def header_len_to_align(before, block_bit, align):
    """the header length that puts the block at bit `block_bit` of the raw stream on a multiple of `align` bytes, when
    `before` bytes precede the member"""
    assert block_bit % 8 == 0
    n = 10 + (-(before + 10 + block_bit // 8)) % align
    return n + align if n == 11 else n


def deflate_start(data, pos):
    """the offset of the deflate data of the member header at data[pos:]"""
    assert data[pos:pos + 3] == b"\x1f\x8b\x08"
    flg, q = data[pos + 3], pos + 10
    if flg & 4:
        q += 2 + struct.unpack_from("<H", data, q)[0]
    for f in (8, 16):
        if flg & f:
            q = data.index(b"\x00", q) + 1
    if flg & 2:
        q += 2
    return q


# -------------------------------------------------------------------------------------------------------------- walker

def _table(lens):
    top = max(lens, default=0)
    tab = [None] * (1 << top)
    for s, (c, l) in canonical(lens).items():
        rev = int(format(c, "0%db" % l)[::-1], 2)
        for r in range(rev, 1 << top, 1 << l):
            tab[r] = (s, l)
    return tab, top


def _check_code(lens, what, single_ok):
    k, n = kraft(lens), sum(1 for l in lens if l)
    if k > 32768:
        raise ValueError("oversubscribed %s code" % what)
    if k < 32768 and not (single_ok and (n == 0 or (n == 1 and max(lens) == 1))):
        raise ValueError("incomplete %s code" % what)


def new_stats():
    return {"blocks": {0: 0, 1: 0, 2: 0}, "max_distance": 0, "one_code_dist_trees": 0, "one_code_dist_trees_used": 0,
            "zero_code_dist_trees": 0, "one_code_lit_trees": 0, "len_pairs": set(), "dist_pairs": set(), "overlaps": set(),
            "matches": 0, "max_lit_bits": 0, "max_dist_bits": 0, "max_cl_bits": 0, "long_lit_symbols": 0,
            "long_dist_symbols": 0, "all_ones_15": set(), "shapes": set(), "hclen": set(), "cl_events": [],
            "empty": set(), "final_type": None, "min_block_out": None, "max_block_out": 0, "last_block_out": 0,
            "starts": [], "end_bit": 0, "blocks_reached": 0, "first_matches": [], "matches_to_first_byte": 0}


def walk(data, bit=0, st=None):
    """Inflate the raw DEFLATE stream at bit offset `bit` of data: (output, stats, the bit after the final block).
    stats (new_stats): blocks by type; the largest distance; distance trees with one code (and those whose code a match
    used) and with none; which (length symbol, extra) and (distance symbol, extra) pairs occurred; overlapping copies as
    (distance, length); the longest code lengths in use; (HLIT, HDIST) and HCLEN of the dynamic headers; the repeats of
    the code-length code as (symbol, count, first index, HLIT, symbol before); empty blocks as (type, final); the smallest
    and largest output of a block and that of the last; every block as (bit offset of its header, type, final); how many
    matches reach back into earlier blocks, how many reach exactly the stream's first byte, and the blocks whose first
    symbol is a match, as (bit offset, distance, length)."""
    st = st or new_stats()
    raw = bytes(data) + b"\x00" * 4
    nbits = len(data) * 8
    pos = bit
    out = bytearray()

    def peek(n):
        return (int.from_bytes(raw[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)

    def get(n):
        nonlocal pos
        v = peek(n)
        pos += n
        if pos > nbits:
            raise ValueError("truncated")
        return v

    def decode(tab, top):
        nonlocal pos
        e = tab[peek(top)] if top else None
        if e is None:
            raise ValueError("bits that are no code")
        pos += e[1]
        if pos > nbits:
            raise ValueError("truncated")
        return e

    final = 0
    while not final:
        at0 = pos
        final, btype = get(1), get(2)
        st["starts"].append((at0, btype, final))
        o0 = len(out)
        if btype == 3:
            raise ValueError("block type 3")
        if btype == 0:
            pos = (pos + 7) & ~7
            n, nn = get(16), get(16)
            if n != (~nn & 0xffff):
                raise ValueError("LEN != ~NLEN")
            if pos + 8 * n > nbits:
                raise ValueError("truncated")
            out += raw[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
        else:
            one_dist = False
            if btype == 1:
                lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
            else:
                hlit, hdist, hclen = get(5) + 257, get(5) + 1, get(4) + 4
                if hlit > 286 or hdist > 30:
                    raise ValueError("HLIT or HDIST too large")
                cl = [0] * 19
                for k in range(hclen):
                    cl[CLORD[k]] = get(3)
                _check_code(cl, "code-length", False)
                ctab, ctop = _table(cl)
                st["max_cl_bits"] = max(st["max_cl_bits"], ctop)
                st["shapes"].add((hlit, hdist))
                st["hclen"].add(hclen)
                lens, before = [], None
                while len(lens) < hlit + hdist:
                    s, _ = decode(ctab, ctop)
                    if s < 16:
                        lens.append(s)
                    else:
                        if s == 16 and not lens:
                            raise ValueError("repeat with nothing before it")
                        rep = (3 + get(2)) if s == 16 else (3 + get(3)) if s == 17 else (11 + get(7))
                        st["cl_events"].append((s, rep, len(lens), hlit, before))
                        lens += [lens[-1] if s == 16 else 0] * rep
                    before = s
                if len(lens) > hlit + hdist:
                    raise ValueError("repeat past HLIT + HDIST")
                lit_lens, dist_lens = lens[:hlit], lens[hlit:]
                if not lit_lens[256]:
                    raise ValueError("no end-of-block code")
                _check_code(lit_lens, "literal/length", True)
                _check_code(dist_lens, "distance", True)
                nd = sum(1 for l in dist_lens if l)
                one_dist = nd == 1
                st["one_code_dist_trees"] += one_dist
                st["zero_code_dist_trees"] += nd == 0
                st["one_code_lit_trees"] += sum(1 for l in lit_lens if l) == 1
            ltab, ltop = _table(lit_lens)
            dtab, dtop = _table(dist_lens)
            used_dist = False
            while True:
                s, l = decode(ltab, ltop)
                if btype == 2:
                    st["max_lit_bits"] = max(st["max_lit_bits"], l)
                    st["long_lit_symbols"] += l > 10
                    if l == 15 and _all_ones(raw, pos - 15):
                        st["all_ones_15"].add("lit")
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise ValueError("length symbol %d" % s)
                le = get(LEXT[s - 257])
                ds, dl = decode(dtab, dtop)
                if ds > 29:
                    raise ValueError("distance symbol %d" % ds)
                if btype == 2:
                    st["max_dist_bits"] = max(st["max_dist_bits"], dl)
                    st["long_dist_symbols"] += dl > 10
                    if dl == 15 and _all_ones(raw, pos - 15):
                        st["all_ones_15"].add("dist")
                de = get(DEXT[ds])
                n, d = LBASE[s - 257] + le, DBASE[ds] + de
                if d > len(out):
                    raise ValueError("distance before the start of the stream")
                st["len_pairs"].add((s, le))
                st["dist_pairs"].add((ds, de))
                st["max_distance"] = max(st["max_distance"], d)
                st["matches"] += 1
                if d < n:
                    st["overlaps"].add((d, n))
                if d > len(out) - o0:
                    st["blocks_reached"] += 1
                if d == len(out):
                    st["matches_to_first_byte"] += 1
                if len(out) == o0:
                    st["first_matches"].append((at0, d, n))
                used_dist = True
                at = len(out) - d
                for k in range(n):
                    out.append(out[at + k])
            st["one_code_dist_trees_used"] += one_dist and used_dist
        n = len(out) - o0
        st["blocks"][btype] += 1
        if n == 0:
            st["empty"].add((btype, final))
        st["min_block_out"] = n if st["min_block_out"] is None else min(st["min_block_out"], n)
        st["max_block_out"] = max(st["max_block_out"], n)
        st["last_block_out"] = n
        if final:
            st["final_type"] = btype
    st["end_bit"] = pos
    return bytes(out), st, pos


def _all_ones(raw, p):
    return (int.from_bytes(raw[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & 0x7fff == 0x7fff


def walk_gzip(data):
    """every member of a gzip file walked: (the whole output, the stats of all members together, per member the bit phase
    (0..7) at which its final block ended, its output size and that of its last block)"""
    st, out, ends, pos = new_stats(), [], [], 0
    while pos < len(data):
        q = deflate_start(data, pos)
        text, st, end = walk(data, q * 8, st)
        pos = (end + 7) // 8
        crc, isize = struct.unpack_from("<II", data, pos)
        assert crc == zlib.crc32(text) and isize == len(text) & 0xffffffff
        pos += 8
        out.append(text)
        ends.append((end % 8, len(text), st["last_block_out"]))
    return b"".join(out), st, ends


# ------------------------------------------------------------------------------------------------------------- sources

def random_bytes(n, seed):
    return random.Random(seed).randbytes(n)


def fastq_like(n, seed):
    rng = random.Random(seed)
    backbone = bytes(rng.choice(b"ACGT") for _ in range(20000))
    out, size, i = [], 0, 0
    while size < n:
        p = rng.randrange(len(backbone) - 150)
        r = bytearray(backbone[p:p + 150])
        for _ in range(rng.randrange(3)):
            r[rng.randrange(150)] = rng.choice(b"ACGT")
        q = bytes(rng.choice(b"##+2::FFFFFF") for _ in range(150))
        out.append(b"@read_%d/1\n%s\n+\n%s\n" % (i, bytes(r), q))
        size += len(out[-1])
        i += 1
    return b"".join(out)[:n]


def gfa_like(n, seed):
    """a GFA text: S-lines, L-lines and W-lines over the same few hundred segments, so that it repeats at every distance"""
    rng = random.Random(seed)
    nseg = 300
    out = [b"S\t%d\t%s\n" % (s, bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 30)))) for s in range(1, nseg + 1)]
    out += [b"L\t%d\t+\t%d\t+\t0M\n" % (s, s + 1) for s in range(1, nseg)]
    size, w = sum(map(len, out)), 0
    while size < n:
        a = rng.randint(1, nseg - 1)
        steps = range(a, min(nseg, a + rng.randint(1, 120)) + 1)
        out.append(b"W\ts%d\t%d\tchr\t0\t%d\t%s\n" % (w // 2, w % 2, len(steps), b"".join(b">%d" % s for s in steps)))
        size += len(out[-1])
        w += 1
    return b"".join(out)


# ------------------------------------------------------------------------------------------------------------ families

class Stream:
    """data: the gzip file; text: what it inflates to, as the writer followed it; aligned: the chunk sizes at which the
    block the family is about starts exactly on a chunk border"""

    def __init__(self, data, text, members=1, aligned=()):
        self.data, self.text, self.members, self.aligned = bytes(data), bytes(text), members, tuple(aligned)


ALIGN = 102400                                           # the least common multiple of the chunk sizes 64, 100 and 4096
FAR = range(32500, 32769)


def _far_tokens():
    return [(n, d) for d in FAR for n in (3, 258)]


def family_a_far():
    """32768 random bytes, then matches at every distance 32500..32768 with lengths 3 and 258"""
    d = Deflate()
    d.stored(random_bytes(32768, 11))
    d.block(_far_tokens(), final=1)
    return Stream(member(d.finish(), d.text), d.text)


def family_a_far_aligned():
    """the same in a block that starts on a chunk border, so that its decoder has nothing before it: the first match has
    distance 32768 (marker 256), the second reads the byte just before the piece (marker 256 + 32767), the third is 258
    long and begins 100 bytes before the piece"""
    d = Deflate()
    d.stored(random_bytes(32768, 12))
    d.block([(3, 32768), (258, 4), (258, 361)] + _far_tokens())
    d.block([], final=1, kind=1)
    raw = d.finish()
    return Stream(member(raw, d.text, header_len_to_align(0, d.starts[1], ALIGN)), d.text, aligned=(64, 100, 4096))


def family_a_member_start():
    """a second member whose match reaches exactly the member's first byte, first inside a piece, then (a block on a
    chunk border) from the piece after the one the member began in"""
    first = Deflate()
    first.block(list(fastq_like(3000, 13)), final=1)
    m1 = member(first.finish(), first.text)
    d = Deflate()
    lits = random_bytes(1000, 14)
    d.block(list(lits[:40]) + [(40, 40)])                       # reaches byte 0 of the member, inside the piece
    d.stored(lits[40:])
    d.block([(258, len(d.text))] + list(b"tail"))               # and again, as the first symbol of an aligned block
    d.block([], final=1, kind=1)
    raw = d.finish()
    m2 = member(raw, d.text, header_len_to_align(len(m1), d.starts[2], ALIGN))
    return Stream(m1 + m2, first.text + d.text, members=2, aligned=(64, 100, 4096))


LIT_LONG = [1, 2, 3, 4, 5, 6, 7] + [11] * 4 + [12] * 8 + [13] * 16 + [14] * 16 + [15] * 32
DIST_LONG = [1, 2, 3, 4, 5, 7, 8, 8] + [9] * 4 + [10] * 2 + [11] * 11 + [12, 13, 14, 15, 15]
assert kraft(LIT_LONG) == 32768 and kraft(DIST_LONG) == 32768 and len(DIST_LONG) == 30


def family_b_trees():
    """the trees and headers zlib's compressor never writes, one block each (see the comments)"""
    rng = random.Random(21)
    fq = fastq_like(4000, 22)
    d = Deflate()
    d.stored(random_bytes(32768, 23))
    # a literal-only block, HLIT = 257, HDIST = 1 and that one length 0; its zero run 85..255 takes symbol 18 with 138
    d.block([c for c in fq[:300] if c in b"ACGT\n"], dist="natural")
    # one distance code of length 1 (symbol 0), used by every match
    d.block(list(fq[300:340]) + [(5, 1), 65, (70, 1), (258, 1)], dist="natural")
    # the same with distance symbol 10 alone (distances 33..48): HDIST = 11
    d.block(list(fq[340:400]) + [(n, 33 + n % 16) for n in range(3, 40)], dist="natural")
    # a literal/length tree that holds end-of-block alone: an empty dynamic block
    d.dynamic([0] * 256 + [1], [0])
    d.eob()
    # HLIT = 286 and HDIST = 30, both last symbols used
    d.block(list(fq[400:420]) + [(258, 32768), (258, 24577), (3, 1)])
    # HCLEN = 5, the smallest a valid block can have (with 4, only 16, 17, 18 and 0 have a code, and no length is nonzero):
    # literals 1..256 on 8 bits each
    d.dynamic([0] + [8] * 256, [0])
    for c in fq[420:520]:
        d.literal(c)
    d.eob()
    # a code-length code with lengths 1..7: eight code-length symbols in use (0 and 1..7), no repeats
    lits = sorted(set(fq[520:]))[:7]
    lens = [0] * 257
    for c, l in zip(lits + [256], [1, 2, 3, 4, 5, 6, 7, 7]):
        lens[c] = l
    d.dynamic(lens, [0], rle=False, cl_lens=[1, 2, 3, 4, 5, 6, 7, 7] + [0] * 11)
    for c in fq[520:700]:
        if c in lits:
            d.literal(c)
    d.eob()
    # symbol 16 repeating zeros across the HLIT / HDIST border, right after a 17 (HLIT = 265) ...
    lit_lens = flat_lengths([256] + list(b"ACGT\n"), 257)
    cl = rle_lengths(lit_lens) + [(17, 1), (16, 3), (0, 0), (0, 0), (1, 0)]      # 257..260, 261..266, 267, 268, 269
    d.dynamic(lit_lens, [0, 0, 0, 0, 1], hlit=265, cl_syms=cl)
    for c in b"GATTACA\n":
        d.literal(c)
    d.eob()
    # ... and right after an 18 (HLIT = 276): 258..273, 274..278, then distance symbol 3 alone
    lit_lens = flat_lengths([256, 257] + list(b"ACGT\n"), 258)
    cl = rle_lengths(lit_lens) + [(18, 5), (16, 2), (1, 0)]
    d.dynamic(lit_lens, [0, 0, 0, 1], hlit=276, cl_syms=cl)
    for c in b"ACGT\n":
        d.literal(c)
    d.match_sym(257, 0, 3, 0)
    d.eob()
    # trees whose 11..15-bit codes carry most symbols (76 of 83, 16 of 30), the all-ones 15-bit code of both used:
    # literal/length symbol 268 (lengths 17, 18) and distance symbol 29; HCLEN = 19 (a length of 15 is coded)
    syms = list(range(70)) + list(range(256, 269))
    lens = [0] * 269
    for s, l in zip(syms, LIT_LONG):
        lens[s] = l
    d.dynamic(lens, DIST_LONG)
    for _ in range(600):
        d.literal(rng.randrange(70))
        if rng.random() < 0.4:
            ds = rng.randrange(30)
            d.match_sym(rng.randrange(257, 269), 0, ds, rng.randrange(1 << DEXT[ds]))
    d.match_sym(268, 1, 29, 8191)
    d.eob()
    d.block(list(b"end\n"), final=1)
    return Stream(member(d.finish(), d.text), d.text)


def family_c_sweep():
    """after 32 KB, one match for every length symbol at extra 0 and at its largest extra, crossed with every distance
    symbol at extra 0 and at its largest: 58 x 60 = 3480 matches, 284 + 31 among them"""
    d = Deflate()
    d.stored(random_bytes(32768, 31))
    tokens = [(ls, le, ds, de) for ls in range(257, 286) for le in (0, (1 << LEXT[ls - 257]) - 1)
              for ds in range(30) for de in (0, (1 << DEXT[ds]) - 1)]
    assert len(tokens) == 3480
    d.block(tokens)
    d.block([], final=1, kind=1)
    return Stream(member(d.finish(), d.text), d.text)


OVERLAP_LENGTHS = (3, 63, 64, 65, 66, 127, 128, 129, 257, 258)


def family_d_overlap():
    """every distance 1..66 with the lengths around the wave width, each after 70 fresh random literals, deep in a piece"""
    rng = random.Random(41)
    d = Deflate()
    d.block(list(rng.randbytes(500)))
    for dist in range(1, 67):
        tokens = []
        for n in OVERLAP_LENGTHS:
            tokens += list(rng.randbytes(70)) + [(n, dist)]
        d.block(tokens, kind=1 + dist % 2)
    d.block([], final=1, kind=1)
    return Stream(member(d.finish(), d.text), d.text)


def family_d_overlap_aligned():
    """the same with each match in a dynamic block of its own on a multiple of 64 bytes (stored blocks of random bytes fill
    up to it), so that at chunk size 64 each block's decoder has nothing before it: the match comes first (all of its
    source is markers) or after half a distance of literals (part of it is)"""
    rng = random.Random(42)
    d = Deflate()
    for dist in range(1, 67):
        for i, n in enumerate(OVERLAP_LENGTHS):
            payload_at = (d.w.bitpos() + 3 + 7) // 8 + 4
            d.stored(rng.randbytes(70 + (-(10 + payload_at + 70)) % 64))
            assert (10 + d.w.bitpos() // 8) % 64 == 0 and d.w.nb == 0
            d.block(list(rng.randbytes(dist // 2 if i % 2 else 0)) + [(n, dist)])
    d.block([], final=1, kind=1)
    return Stream(member(d.finish(), d.text), d.text, aligned=(64,))


def _small_blocks(text, rng, d, kinds=(0, 1, 1, 1, 2, 2), top=40):
    """text cut into blocks of 0..top output bytes of mixed types; matches from a table of earlier places of each 3 bytes"""
    seen, p = {}, 0

    def note(a, b):
        for i in range(max(a, 0), b):
            seen.setdefault(text[i:i + 3], []).append(i)

    while p < len(text):
        n = min(rng.randint(0, top), len(text) - p)
        kind = rng.choice(kinds)
        if kind == 0:
            d.stored(text[p:p + n])
        else:
            tokens, q = [], p
            while q < p + n:
                places = [c for c in seen.get(text[q:q + 3], ())[-6:] if q - c <= 32768]
                if places and p + n - q >= 3 and rng.random() < 0.85:
                    c = rng.choice(places)
                    m = 3
                    while m < min(p + n - q, 258) and text[c + m] == text[q + m]:
                        m += 1
                    tokens.append((m, q - c))
                    q += m
                else:
                    tokens.append(text[q])
                    q += 1
            d.block(tokens, kind=kind, dist=rng.choice(("pad", "natural")))
        note(p - 2, p + n - 2)
        p += n


def family_e_small_blocks():
    """about 20 000 blocks of 0..40 output bytes, stored, fixed and dynamic mixed by a seeded generator, the matches
    reaching back across many blocks; the text is a GFA"""
    d = Deflate()
    _small_blocks(gfa_like(400_000, 51), random.Random(52), d)
    d.block([], final=1, kind=1)
    return Stream(member(d.finish(), d.text), d.text)


def _with_empty_blocks(final):
    """data blocks with the three empty shapes between them, each non-final, and `final` as the last block"""
    fq = fastq_like(6000, 61)
    d = Deflate()

    def empty(kind, fin):
        if kind == 0:
            d.stored(b"", fin)
        elif kind == 1:
            d.block([], fin, kind=1)
        else:
            d.dynamic([0] * 256 + [1], [0], fin)
            d.eob()

    _small_blocks(fq[:2000], random.Random(62), d, top=300)
    for kind in (0, 1, 2):
        empty(kind, 0)
        _small_blocks(fq[2000 + 1000 * kind:3000 + 1000 * kind], random.Random(63 + kind), d, top=300)
    empty(0, 0), empty(1, 0), empty(2, 0), empty(2, 0), empty(1, 0), empty(0, 0)      # and in a row
    _small_blocks(fq[5000:], random.Random(66), d, top=300)
    if final == "stored":
        d.stored(b"the last block is stored\n", 1)
    else:
        empty(final, 1)
    return Stream(member(d.finish(), d.text), d.text)


def family_f_fixed_run():
    """300 non-final fixed-Huffman blocks in a row, about 100 compressed bytes each: longer than several chunks of 64, 100
    and 4096 bytes, and no chunk in it holds a start the finder looks for"""
    fq = fastq_like(45_000, 67)
    d = Deflate()
    d.block(list(fq[:200]))
    for i in range(300):
        d.block(list(fq[200 + 149 * i:200 + 149 * (i + 1)]), kind=1)
    d.block(list(b"end\n"), final=1)
    return Stream(member(d.finish(), d.text), d.text)


def family_g_decoy_deflate():
    """a stored block whose payload is a complete raw DEFLATE stream of FASTQ text in many small dynamic blocks: every
    header in it is a start that decodes cleanly, and none is a block of the stream"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 2)                  # memLevel 2: a block every 256 symbols
    fq = fastq_like(170_000, 71)
    payload = c.compress(fq) + c.flush()
    assert 50_000 < len(payload) <= 65535, len(payload)
    d = Deflate()
    d.block(list(fq[:500]))
    d.stored(payload)
    d.block(list(fq[500:900]) + [(100, 400)])
    d.block([], final=1, kind=1)
    return Stream(member(d.finish(), d.text), d.text), payload


def family_g_decoy_gzip():
    """a stored payload that holds the gzip magic and a whole valid member"""
    fq = fastq_like(60_000, 72)
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    payload = b"\x00" * 7 + c.compress(fq) + c.flush()
    d = Deflate()
    d.block(list(fq[:300]))
    d.stored(payload)
    d.block(list(fq[300:600]), final=1)
    return Stream(member(d.finish(), d.text), d.text), payload


def family_h_members():
    """twenty members whose last block is a few bytes (far too short to fill a chunk), empty members between them"""
    fq = fastq_like(40_000, 81)
    e = Deflate()
    e.block([], final=1, kind=1)
    empty = member(e.finish(), b"")
    parts, text, count = [], [], 0
    for i in range(20):
        d = Deflate()
        d.block(list(fq[2000 * i:2000 * i + 1990]), kind=1 + i % 2)
        d.block(list(fq[2000 * i + 1990:2000 * (i + 1)]), final=1, kind=(2, 1, 0)[i % 3])
        parts.append(member(d.finish(), d.text, 10 if i % 4 else 12 + i))
        text.append(bytes(d.text))
        count += 1
        for _ in range(i % 3):
            parts.append(empty)
            count += 1
    return Stream(b"".join(parts), b"".join(text), members=count)


def family_h_phases():
    """sixteen members: the final block of member i ends on bit phase i mod 8 (literals of 9 bits shift it by one each)"""
    parts, text = [], []
    for i in range(16):
        for extra in range(8):
            d = Deflate()
            d.block(list(b"member %d\n" % i), kind=1)
            d.block([200 + k for k in range(extra)] + list(b"end\n"), final=1, kind=1)
            if d.w.bitpos() % 8 == i % 8:
                break
        else:
            raise AssertionError("no phase %d" % i)
        parts.append(member(d.finish(), d.text))
        text.append(bytes(d.text))
    return Stream(b"".join(parts), b"".join(text), members=16)


@functools.lru_cache(maxsize=None)
def valid_streams():
    """{name: Stream} of every valid family (built once per process)"""
    s = {
        "A_far": family_a_far(), "A_far_aligned": family_a_far_aligned(), "A_member_start": family_a_member_start(),
        "B_trees": family_b_trees(), "C_sweep": family_c_sweep(),
        "D_overlap": family_d_overlap(), "D_overlap_aligned": family_d_overlap_aligned(),
        "E_small_blocks": family_e_small_blocks(),
        "F_final_empty_stored": _with_empty_blocks(0), "F_final_empty_fixed": _with_empty_blocks(1),
        "F_final_empty_dynamic": _with_empty_blocks(2), "F_final_stored": _with_empty_blocks("stored"),
        "F_fixed_run": family_f_fixed_run(),
        "G_decoy_deflate": family_g_decoy_deflate()[0], "G_decoy_gzip": family_g_decoy_gzip()[0],
        "H_members": family_h_members(), "H_phases": family_h_phases(),
    }
    assert list(s) == VALID
    return s


VALID = ["A_far", "A_far_aligned", "A_member_start", "B_trees", "C_sweep", "D_overlap", "D_overlap_aligned",
         "E_small_blocks", "F_final_empty_stored", "F_final_empty_fixed", "F_final_empty_dynamic", "F_final_stored",
         "F_fixed_run", "G_decoy_deflate", "G_decoy_gzip", "H_members", "H_phases"]


# ------------------------------------------------------------------------------------------------------------- invalid

_LINE = b"@read_1/1\nGATTACAGATTACA\n+\nFFFFFFFFFFFFFF\n"
INVALID_PREFIX = _LINE + (_LINE[-14:] * 2)[:20] + b"stored\n"       # what every invalid stream inflates to before it is wrong


def _invalid(spoil):
    """a member that begins with a good dynamic block and a good stored block; spoil(d) then writes what is wrong"""
    d = Deflate(track=False)
    d.block(list(_LINE) + [(20, 14)])
    d.stored(b"stored\n")
    spoil(d)
    d.w.align()
    return gzip_header() + bytes(d.w.out) + b"\x00" * 16


def _fixed_symbol(code, bits):
    def spoil(d):
        d.fixed()
        d.literal(65), d.literal(66)
        d.w.code(code, bits)
        d.w.bits(0, 16)
    return spoil


def _fixed_distance(ds):
    def spoil(d):
        d.fixed()
        d.literal(65), d.literal(66), d.literal(67)
        d.sym(257)
        d.w.code(ds, 5)
        d.w.bits(0, 16)
    return spoil


def _dynamic(lit=None, dist=None, tail=(), **kw):
    def spoil(d):
        d.dynamic(lit if lit is not None else flat_lengths([65, 66, 256, 257], 258), dist if dist is not None else [1, 1],
                  check=False, **kw)
        for bit in tail:
            d.w.bits(bit, 1)
        d.w.bits(0, 16)
    return spoil


def _lens(pairs, n=257):
    lens = [0] * n
    for s, l in pairs.items():
        lens[s] = l
    return lens


def _unassigned_bit(d):
    d.dynamic(flat_lengths([65, 66, 256, 257], 258), [1])
    d.literal(65), d.literal(66), d.literal(65)
    d.sym(257)
    d.w.bits(1, 1)                                               # the one distance code is "0"
    d.w.bits(0, 16)


_GOOD_LIT = flat_lengths([65, 66, 256, 257], 258)
_CL_01 = _lens({0: 1, 1: 1}, 19)

# name: (what spoils the stream, the message of zlib's inflater)
INVALID = {
    "block_type_3": (lambda d: (d.head(0, 3), d.w.bits(0, 29)), "invalid block type"),
    "fixed_literal_286": (_fixed_symbol(0b11000110, 8), "invalid literal/length code"),
    "fixed_literal_287": (_fixed_symbol(0b11000111, 8), "invalid literal/length code"),
    "fixed_distance_30": (_fixed_distance(30), "invalid distance code"),
    "fixed_distance_31": (_fixed_distance(31), "invalid distance code"),
    "hlit_287": (_dynamic(hlit=287), "too many length or distance symbols"),
    "hlit_288": (_dynamic(hlit=288), "too many length or distance symbols"),
    "hdist_31": (_dynamic(hdist=31), "too many length or distance symbols"),
    "hdist_32": (_dynamic(hdist=32), "too many length or distance symbols"),
    "code_length_code_oversubscribed": (_dynamic(cl_lens=_lens({0: 1, 1: 1, 2: 1}, 19)), "invalid code lengths set"),
    "code_length_code_incomplete": (_dynamic(cl_lens=_lens({0: 1, 1: 2, 2: 3}, 19)), "invalid code lengths set"),
    "repeat_16_first": (_dynamic(cl_syms=[(16, 0)] + rle_lengths(_GOOD_LIT[3:] + [1, 1]), cl_lens=_lens({0: 1, 2: 2, 16: 3, 18: 4, 1: 4}, 19)),
                        "invalid bit length repeat"),
    "repeat_past_the_end": (_dynamic(cl_syms=rle_lengths(_GOOD_LIT)[:-1] + [(18, 127)], cl_lens=_lens({0: 2, 2: 2, 17: 2, 18: 2}, 19)),
                            "invalid bit length repeat"),
    "no_end_of_block": (_dynamic(lit=flat_lengths([65, 66, 67, 257], 258)), "missing end-of-block"),
    "hclen_4_has_no_lengths": (_dynamic(lit=[0] * 257, dist=[0], cl_lens=_lens({0: 1, 18: 1}, 19), hclen=4), "missing end-of-block"),
    "lit_tree_oversubscribed": (_dynamic(lit=_lens({65: 1, 66: 1, 256: 1})), "invalid literal/lengths set"),
    "lit_tree_incomplete_two_codes": (_dynamic(lit=_lens({65: 2, 256: 2})), "invalid literal/lengths set"),
    "dist_tree_incomplete_two_codes": (_dynamic(dist=[2, 2]), "invalid distances set"),
    "dist_tree_one_code_of_length_2": (_dynamic(dist=[2]), "invalid distances set"),
    "one_code_dist_tree_unassigned_bit": (_unassigned_bit, "invalid distance code"),
    "stored_len_nlen": (lambda d: d.stored(b"abcdef", nlen=0x1234), "invalid stored block lengths"),
}


def invalid_stream(name):
    return _invalid(INVALID[name][0])
