"""Inputs for the tests of the BGZF indexes (phi_deflate_bgzf_indexed): a synthetic VCF of about 300 KB that meets the corners of
the .tbi rules on purpose, region draws for queries, and a BGZF writer on zlib so the reader of tabix_ref.py can be checked
without a GPU.  A helper, no test; nothing here shares code with phi_amd."""
import struct
import zlib

import numpy as np

import tabix_ref as T

BLOCK = T.BLOCK
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
VARIANTS = ("plain", "multiple_of_block", "no_final_newline")
LONG_REF = 40000
LONG_POS = 3 * 16384 + 1000 + 1             # beg = window 3 + 1000: the 40 000 bases overlap windows 3, 4 and 5


def zlib_bgzf(text):
    """text as a BGZF file by zlib, cut where the device's writer cuts: for the CPU tests of the reader"""
    out = []
    for at in range(0, len(text), BLOCK):
        t = text[at:at + BLOCK]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(t) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(body) + 8 - 1) + body +
                   struct.pack("<II", zlib.crc32(t), len(t)))
    return b"".join(out) + EOF


def _record(chrom, pos, ident=".", ref="A", alt="C", info=".", tail=""):
    return f"{chrom}\t{pos}\t{ident}\t{ref}\t{alt}\t.\tPASS\t{info}{tail}".encode()


def synthetic_vcf(variant="plain"):
    """The text, by construction:
      two contigs (chrA, chrB); meta lines, one of them after the first record; on chrA positions beyond 2^26 and one record
      across an edge of every level of the binning, so bins of all six levels occur; a REF of 40 000 bases over three windows
      whose line begins in block 0 and whose END= lies in block 1; END= at the start of INFO far beyond the REF; ;END= in
      mid-INFO; IDs "END=7" and "a;END=9", "SEND=" and "FRIEND=" keys, ";END=3" in a sample field (none of them counts);
      POS 0; a line that begins exactly at byte 2 * 65280 and a line whose newline is byte 3 * 65280.
    variant: "multiple_of_block" pads the last record so the length is a multiple of 65 280; "no_final_newline" drops the last byte."""
    rng = np.random.default_rng(20261021)
    bases = np.array(list("ACGT"))
    a = []                                                      # (pos, line) of chrA
    for i in range(800):
        a.append((100 + 60 * i, _record("chrA", 100 + 60 * i, f"a{i}", info=f"DP={i % 97}")))
    for i in range(2800):
        p = 60000 + 26000 * i + int(rng.integers(0, 20000))
        ref = "".join(bases[rng.integers(0, 4, int(rng.integers(1, 12)))])
        a.append((p, _record("chrA", p, f"b{i}", ref=ref, info=f"DP={i % 89};AF=0.5")))
    for shift in (14, 17, 20, 23, 26):                          # five bases over an edge of every level
        p = (1 << shift) - 2
        a.append((p, _record("chrA", p, f"edge{shift}", ref="ACGTA", info="EDGE")))
    long_ref = "".join(bases[rng.integers(0, 4, LONG_REF)])
    a.append((LONG_POS, _record("chrA", LONG_POS, "sv_long", ref=long_ref, alt="A", info=f"END={LONG_POS - 1 + LONG_REF};SVTYPE=DEL")))
    a.append((500000, _record("chrA", 500000, "sv_far", info="END=1200000;SVTYPE=DEL")))
    a.append((700000, _record("chrA", 700000, "sv_mid", info="SVTYPE=DEL;END=2000100;X=1")))
    a.append((800000, _record("chrA", 800000, "END=7", ref="ACG")))
    a.append((800100, _record("chrA", 800100, "a;END=9", ref="AC", info="SEND=5;FRIEND=3")))
    a.append((800200, _record("chrA", 800200, "fmt", info="DP=1", tail="\tGT\t1;END=3")))
    a.append((800300, _record("chrA", 800300, "short", ref="ACGT", info="END=5")))      # an END at or before beg: one base
    a.sort(key=lambda t: t[0])
    lines = [b"##fileformat=VCFv4.2", b"##contig=<ID=chrA>", b"##contig=<ID=chrB>", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO", a[0][1],
             b"##a meta line after the first record"] + [ln for _, ln in a[1:]]
    lines.append(_record("chrB", 0, "zero"))
    for i in range(2900):
        lines.append(_record("chrB", 1 + 37 * i, f"c{i}", info=f"DP={i % 83}"))
    # the two alignments: what follows a padded line begins at 2 * 65280; the newline of another is byte 3 * 65280
    out, at, wants = [], 0, [2 * BLOCK, 3 * BLOCK + 1]
    for ln in lines:
        if wants and wants[0] - 400 <= at + len(ln) + 1 <= wants[0] - 6 and not ln.startswith(b"#") and len(ln) < 200:
            ln += b";PAD=" + b"x" * (wants[0] - (at + len(ln) + 1) - 5)
            assert at + len(ln) + 1 == wants.pop(0)
        out.append(ln + b"\n")
        at += len(ln) + 1
    assert not wants
    text = b"".join(out)
    if variant == "multiple_of_block":
        pad = -len(text) % BLOCK
        text = text[:-1] + b";PAD=" + b"y" * (pad + BLOCK - 5 if pad < 5 else pad - 5) + b"\n"
        assert len(text) % BLOCK == 0
    elif variant == "no_final_newline":
        text = text[:-1]
    else:
        assert variant == "plain"
    return text


def check_corners(text):
    """that the synthetic text is what its docstring says (computed here, on the CPU, from the reference's own rules)"""
    lines = T.lines_of(text)
    recs = [(s, n, ln) + T.record_of(ln) for s, n, ln in lines if not ln.startswith(b"#")]
    assert len(text) >= 5 * BLOCK - BLOCK + 1 and {r[3] for r in recs} == {b"chrA", b"chrB"}
    first = next(i for i, (_, _, ln) in enumerate(lines) if not ln.startswith(b"#"))
    assert any(ln.startswith(b"#") for _, _, ln in lines[first:])
    levels = set()
    for r in recs:
        b = T.reg2bin(r[4], r[5])
        levels.add(sum(b >= first for _, first in T.LEVELS))
    assert levels == {0, 1, 2, 3, 4, 5} and max(r[5] for r in recs) > 1 << 26
    long_ = next(r for r in recs if len(r[2]) > LONG_REF)
    assert (long_[5] - 1 >> 14) - (long_[4] >> 14) == 2 and long_[0] // BLOCK == 0 and (long_[0] + long_[2].index(b"END=")) // BLOCK == 1
    by_id = {r[2].split(b"\t")[2]: r for r in recs}
    assert by_id[b"sv_far"][5] == 1200000 and by_id[b"sv_mid"][5] == 2000100
    assert by_id[b"END=7"][5] == by_id[b"END=7"][4] + 3 and by_id[b"a;END=9"][5] == by_id[b"a;END=9"][4] + 2
    assert by_id[b"fmt"][5] == by_id[b"fmt"][4] + 1 and by_id[b"short"][5] == by_id[b"short"][4] + 1 and by_id[b"zero"][4] == 0
    assert any(s == 2 * BLOCK for s, _, _ in lines) and any(s + len(ln) == 3 * BLOCK for s, _, ln in lines)
    return recs


def draw_regions(text, n, seed):
    """n regions (name, beg, end) around randomly chosen records of the text, the whole contigs and single bases at window edges
    among them; asserts on the brute-force side that at most a quarter of them hold no record"""
    rng = np.random.default_rng(seed)
    recs = [T.record_of(ln) for _, _, ln in T.lines_of(text) if not ln.startswith(b"#")]
    names = sorted({r[0] for r in recs})
    regions = [(nm, 0, T.MAX_END) for nm in names]
    picks = [max(recs, key=lambda r: r[2] - r[1])] + [recs[int(rng.integers(0, len(recs)))] for _ in range(n // 25 - 1)]
    for nm, b, e in picks:                                      # single bases on both sides of a window edge, the longest record's first
        edge = ((b >> 14) + 1) << 14
        regions += [(nm, edge - 1, edge), (nm, edge, edge + 1), (nm, b, b + 1), (nm, e - 1, e)]
    while len(regions) < n:
        nm, b, e = recs[int(rng.integers(0, len(recs)))]
        width = int(rng.choice([1, 10, 1000, 20000, 300000, 5000000]))
        lo = max(b - int(rng.integers(0, width)), 0)
        hi = min(max(e + int(rng.integers(0, width)) - int(rng.integers(0, 3)), lo + 1), T.MAX_END)
        regions.append((nm, lo, hi))
    regions = regions[:n]
    empty = sum(not any(r[0] == nm and r[1] < hi and r[2] > lo for r in recs) for nm, lo, hi in regions)
    assert 4 * empty <= len(regions), (empty, len(regions))
    return regions
