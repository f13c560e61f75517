"""Inputs for the tests of region reads (phi_region_*, phi_vcf_region_filter, set_graph_vcf(region=)): a phased three-contig VCF
with its reference, writers of the indexed files on zlib and tabix_ref.py, and a .tbi rewritten the way htslib lays one out.
A helper, no test; nothing here shares code with phi_amd."""
import struct

import numpy as np

import bgzf_index_cases as K
import tabix_ref as T

BLOCK = T.BLOCK
CONTIGS = (("chr1", 100000), ("chr10", 50000), ("ctgB", 40000))       # chr1 is a prefix of chr10
SAMPLES = tuple(f"S{i}" for i in range(6))
LONG_INFO = 70000
LINE = 60


def reference():
    """{name: bases} of the three contigs, some of them lower case in the file"""
    rng = np.random.default_rng(41)
    return {n: bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)]) for n, ln in CONTIGS}


def fasta_text(ref, lower=True):
    out = []
    for name, _ in CONTIGS:
        seq = ref[name]
        out.append(b">" + name.encode() + b" a description\n")
        for at in range(0, len(seq), LINE):
            row = seq[at:at + LINE]
            out.append((row.lower() if lower and (at // LINE) % 7 == 3 else row) + b"\n")
    return b"".join(out)


def fai_text(fasta):
    """the .fai of a FASTA text whose records have lines of one width (the last may be shorter), as samtools faidx writes it"""
    out, at, lines = [], 0, fasta.split(b"\n")
    name = None
    for ln in lines[:-1] if fasta.endswith(b"\n") else lines:
        if ln.startswith(b">"):
            if name is not None:
                out.append(b"%s\t%d\t%d\t%d\t%d\n" % (name, n, off, lb, lw))
            name, n, off, lb, lw = ln[1:].split()[0], 0, at + len(ln) + 1, 0, 0
        else:
            if not lb:
                lb, lw = len(ln), len(ln) + 1
            n += len(ln)
        at += len(ln) + 1
    out.append(b"%s\t%d\t%d\t%d\t%d\n" % (name, n, off, lb, lw))
    return b"".join(out)


def synthetic_vcf(ref, n_samples=len(SAMPLES)):
    """The text and its records [(name, beg, end, line)], by construction: about 2 000 records on three contigs, six phased
    samples (or n_samples); SNPs, deletions and insertions whose REF is the reference's; every 90th record a symbolic <DEL> with END= 400
    bases on; one record whose INFO holds 70 000 bytes, longer than a BGZF member; INFO padded so that the text is several
    members and lines cross their boundaries; no record within 150 bases of a contig's ends."""
    rng = np.random.default_rng(43)
    samples = tuple(f"S{i}" for i in range(n_samples))
    lines = [b"##fileformat=VCFv4.2"] + [b"##contig=<ID=%s,length=%d>" % (n.encode(), ln) for n, ln in CONTIGS]
    lines += [b'##INFO=<ID=END,Number=1,Type=Integer,Description="end">', b'##FORMAT=<ID=GT,Number=1,Type=String,Description="genotype">',
              ("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples)).encode()]
    k = 0
    for name, length in CONTIGS:
        seq, pos = ref[name], 150
        while True:
            pos += int(rng.integers(45, 135))
            if pos + 600 > length - 150:
                break
            k += 1
            kind = int(rng.integers(0, 10))
            info = b"DP=%d;PAD=%s" % (k % 97, b"p" * int(rng.integers(40, 160)))
            if k % 90 == 0:
                r, alts, info = seq[pos:pos + 1], [b"<DEL>"], b"SVTYPE=DEL;END=%d;" % (pos + 400) + info
            elif kind < 6:
                r = seq[pos:pos + 1]
                alts = [bytes([c]) for c in b"ACGT" if c != r[0]][:1 + int(rng.integers(0, 2))]
            elif kind < 8:
                r = seq[pos:pos + int(rng.integers(2, 7))]
                alts = [r[:1]]
            else:
                r = seq[pos:pos + 1]
                alts = [r + bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(rng.integers(1, 5)))])]
            if k == 700:
                info = b"LONG=" + b"x" * LONG_INFO
            gts = b"\t".join(b"%d|%d" % (int(rng.integers(0, len(alts) + 1)), int(rng.integers(0, len(alts) + 1))) for _ in samples)
            lines.append(b"%s\t%d\tr%d\t%s\t%s\t.\tPASS\t%s\tGT\t%s" % (name.encode(), pos + 1, k, r, b",".join(alts), info, gts))
    text = b"".join(ln + b"\n" for ln in lines)
    recs = [T.record_of(ln) + (ln,) for _, _, ln in T.lines_of(text) if not ln.startswith(b"#")]
    starts = {s for s, _, _ in T.lines_of(text)}
    assert len(text) > 5 * BLOCK and 1800 < len(recs) < 2600 and any(m * BLOCK not in starts for m in range(1, len(text) // BLOCK))
    assert sum(len(r[3]) > BLOCK for r in recs) == 1 and sum(b"END=" in r[3] for r in recs) > 10
    return text, recs


def indexed(text):
    """(the BGZF file, its .tbi file) by zlib and tabix_ref's per-line writer"""
    data = K.zlib_bgzf(text)
    raw, _ = T.tbi_bytes(text, T.member_offsets(data))
    return data, K.zlib_bgzf(raw)


def htslib_style(tbi_file, n_no_coor=5):
    """The same index laid out as htslib lays one out: within a bin, consecutive chunks of which one ends in the member
    where the next begins are merged into one (which then spans records of other bins); every contig gains pseudo-bin 37450
    with its two pairs of numbers; n_no_coor is not 0.  Returns (the .tbi file, the same with n_no_coor 0 for tabix_ref)."""
    idx = T.parse_tbi(tbi_file)
    names = b"".join(n + b"\0" for n in idx["names"])
    out = [b"TBI\1", struct.pack("<8i", len(idx["names"]), 2, 1, 2, 0, ord("#"), 0, len(names)), names]
    for bins, lin in zip(idx["bins"], idx["lin"]):
        out.append(struct.pack("<i", len(bins) + 1))
        lo, hi = min(c[0] for ch in bins.values() for c in ch), max(c[1] for ch in bins.values() for c in ch)
        for b in sorted(bins):
            merged = []
            for beg, end in bins[b]:
                if merged and merged[-1][1] >> 16 >= beg >> 16 and beg >= merged[-1][1]:
                    merged[-1][1] = end
                else:
                    merged.append([beg, end])
            out.append(struct.pack("<Ii", b, len(merged)) + b"".join(struct.pack("<QQ", *m) for m in merged))
        out.append(struct.pack("<Ii", 37450, 2) + struct.pack("<QQQQ", lo, hi, sum(len(c) for c in bins.values()), 0))
        out.append(struct.pack("<i", len(lin)) + struct.pack(f"<{len(lin)}Q", *lin))
    body = b"".join(out)
    return K.zlib_bgzf(body + struct.pack("<Q", n_no_coor)), K.zlib_bgzf(body + struct.pack("<Q", 0))


def write_files(tmp, text, ref, tbi=None):
    """the indexed VCF and the indexed BGZF FASTA under tmp: (vcf path, fasta path)"""
    data, t = indexed(text)
    vcf, fa = tmp / "syn.vcf.gz", tmp / "syn.fa.gz"
    vcf.write_bytes(data)
    (tmp / "syn.vcf.gz.tbi").write_bytes(t if tbi is None else tbi)
    fasta = fasta_text(ref)
    gz = K.zlib_bgzf(fasta)
    fa.write_bytes(gz)
    (tmp / "syn.fa.gz.fai").write_bytes(fai_text(fasta))
    (tmp / "syn.fa.gz.gzi").write_bytes(T.gzi_bytes(T.member_offsets(gz)))
    return str(vcf), str(fa)


def cut_files(tmp, tag, header, lines, bases, b):
    """the pre-cut files of a region: a plain VCF of the header and the lines with POS - b, a one-record plain FASTA"""
    out = [header]
    for ln in lines:
        f = ln.split(b"\t")
        f[1] = b"%d" % (int(f[1]) - b)
        out.append(b"\t".join(f) + b"\n")
    vcf, fa = tmp / f"{tag}.vcf", tmp / f"{tag}.fa"
    vcf.write_bytes(b"".join(out))
    fa.write_bytes(b">cut\n" + b"".join(bases[i:i + LINE] + b"\n" for i in range(0, len(bases), LINE)))
    return str(vcf), str(fa)


def header_of(text):
    at = text.index(b"#CHROM")
    return text[:text.index(b"\n", at) + 1]


def quiet_edges(recs, name, b, e):
    """[b, e) moved inwards until no record of the contig touches its first or last two bases (the graph route refuses a
    variant at the reference's first or last base)"""
    mine = [(rb, re) for n, rb, re, _ in recs if n == name]
    while any(rb <= b + 1 and re > b - 1 for rb, re in mine):
        b += 1
    while any(rb <= e and re >= e - 2 for rb, re in mine):
        e -= 1
    assert b < e
    return b, e
