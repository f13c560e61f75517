"""GPU: phi_deflate_bgzf_indexed (phi_amd.deflate_bgzf_indexed), the BGZF writer with an index built beside the file on the
device: a tabix .tbi (VCF preset) or bgzip's .gzi.  bcftools, tabix, samtools and pysam are not at hand, so the yardstick is the
specification as tests/tabix_ref.py restates it: a per-line writer of the rules of include/phi_amd.h, whose bytes the device's
index must equal exactly; a reader that answers region queries through the index alone, compared with a brute-force filter of
the lines; and a reader of FASTA slices through .gzi + .fai.  The file itself must be byte for byte what deflate_bgzf gives."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import bgzf_index_cases as K
import bgzf_util
import tabix_ref as T
from conftest import DATA

pytestmark = pytest.mark.gpu

B = bgzf_util.BLOCK
INVALID, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def phi():
    import __graft_entry__
    __graft_entry__.ensure_built()
    import phi_amd
    return phi_amd


@pytest.fixture(scope="module")
def synthetic():
    """variant -> (text, its records): built once, shared, never changed"""
    out = {}
    for v in K.VARIANTS:
        text = K.synthetic_vcf(v)
        out[v] = (text, K.check_corners(text))
    assert len(out["multiple_of_block"][0]) % B == 0 and not out["no_final_newline"][0].endswith(b"\n")
    return out


@pytest.fixture(scope="module")
def mhc_text():
    with gzip.open(os.path.join(DATA, "MHC_4.vcf.gz"), "rb") as f:
        return f.read()


def _indexed_vcf(phi, text):
    """the file and its .tbi, checked against the plain writer and the per-line writer; returns (file, tbi file, info)"""
    data, tbi, info = phi.deflate_bgzf_indexed(text, "tbi")
    assert data == phi.deflate_bgzf(text)
    mem = bgzf_util.members(tbi)
    want, counts = T.tbi_bytes(text, T.member_offsets(data))
    assert b"".join(t for _, t in mem) == want
    for k, v in counts.items():
        assert info[k] == v, (k, info[k], v)
    assert info["index_bytes"] == len(tbi) and info["device_ms"] >= 0 and (info["device_ms"] > 0) == (len(text) > 0)
    assert info["deflate"]["out_bytes"] == len(data) and info["deflate"]["in_bytes"] == len(text)
    return data, tbi, info


# ------------------------------------------------------------------ 1. the synthetic VCF, byte for byte

@pytest.mark.parametrize("variant", K.VARIANTS)
def test_synthetic_vcf_index_equals_the_per_line_writer(phi, synthetic, variant):
    text, recs = synthetic[variant]
    assert len(text) >= 4 * B + 1                                       # five blocks at the least
    data, tbi, info = _indexed_vcf(phi, text)
    assert info["records"] == len(recs) and info["contigs"] == 2 and info["meta_lines"] == 5
    assert bgzf_util.text_of(data) == text
    if variant == "multiple_of_block":                                  # the last chunk ends at the EOF block
        idx = T.parse_tbi(tbi)
        ends = max(e for chunks in idx["bins"][1].values() for _, e in chunks)
        assert ends == (len(data) - 28) << 16


# ------------------------------------------------------------------ 2. queries through the reader

def _check_queries(data, tbi, text, regions):
    idx = T.parse_tbi(tbi)
    assert (idx["format"], idx["col_seq"], idx["col_beg"], idx["col_end"], idx["meta"], idx["skip"]) == (2, 1, 2, 0, ord("#"), 0)
    recs = [(ln,) + T.record_of(ln) for _, _, ln in T.lines_of(text) if not ln.startswith(b"#")]
    cache, found = {}, 0
    for name, lo, hi in regions:
        want = [r[0] for r in recs if r[1] == name and r[2] < hi and r[3] > lo]
        assert T.query(data, idx, name, lo, hi, cache) == want, (name, lo, hi, len(want))
        found += bool(want)
    assert 4 * found >= 3 * len(regions)                                # (draw_regions asserted the same on its side)
    assert T.query(data, idx, b"no_such_contig", 0, 100) == []


def test_queries_on_the_synthetic_vcf(phi, synthetic):
    text, _ = synthetic["plain"]
    data, tbi, _ = phi.deflate_bgzf_indexed(text, "tbi")
    _check_queries(data, tbi, text, K.draw_regions(text, 200, seed=1))


def test_queries_on_the_mhc_vcf(phi, mhc_text):
    data, tbi, info = _indexed_vcf(phi, mhc_text)
    assert info["contigs"] == 1 and info["records"] > 30000
    _check_queries(data, tbi, mhc_text, K.draw_regions(mhc_text, 200, seed=2))


# ------------------------------------------------------------------ 3. batches

def test_batches_change_neither_file_nor_index(phi, synthetic):
    text, _ = synthetic["plain"]
    assert os.environ.get("PHI_DEFLATE_BATCH") is None
    want = phi.deflate_bgzf_indexed(text, "tbi")[:2]
    gzi = phi.deflate_bgzf_indexed(text, "gzi")[:2]
    try:
        for batch in ("1", "2"):                                        # at 1 the 40 000-base line and its END= straddle batches
            os.environ["PHI_DEFLATE_BATCH"] = batch
            assert phi.deflate_bgzf_indexed(text, "tbi")[:2] == want, batch
            assert phi.deflate_bgzf_indexed(text, "gzi")[:2] == gzi, batch
    finally:
        del os.environ["PHI_DEFLATE_BATCH"]


# ------------------------------------------------------------------ 4. refusals

HEAD = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def _rec(chrom=b"c1", pos=b"100", info=b".", ref=b"A"):
    return b"\t".join([chrom, pos, b".", ref, b"C", b".", b"PASS", info]) + b"\n"


REFUSALS = {
    "seven_fields": (HEAD + _rec() + b"c1\t200\t.\tA\tC\t.\tPASS\n", INVALID),
    "empty_line": (HEAD + _rec() + b"\n" + _rec(pos=b"200"), INVALID),
    "empty_line_first": (b"\n" + HEAD + _rec(), INVALID),
    "pos_empty": (HEAD + _rec(pos=b""), INVALID),
    "pos_not_digits": (HEAD + _rec(pos=b"12a"), INVALID),
    "pos_signed": (HEAD + _rec(pos=b"-5"), INVALID),
    "pos_eleven_digits": (HEAD + _rec(pos=b"00000000100"), INVALID),
    "end_empty": (HEAD + _rec(info=b"END=;X=1"), INVALID),
    "end_empty_last": (HEAD + _rec(info=b"X=1;END="), INVALID),
    "end_not_digits": (HEAD + _rec(info=b"X=1;END=12x"), INVALID),
    "end_eleven_digits": (HEAD + _rec(info=b"END=00000000200"), INVALID),
    "pos_goes_back": (HEAD + _rec(pos=b"100") + _rec(pos=b"200") + _rec(pos=b"199"), INVALID),
    "contig_comes_back": (HEAD + _rec(b"c1") + _rec(b"c2") + _rec(b"c1", b"500"), INVALID),
    "end_beyond_2_29_by_ref": (HEAD + _rec(pos=str(1 << 29).encode(), ref=b"AC"), UNSUPPORTED),
    "end_beyond_2_29_by_end": (HEAD + _rec(info=b"END=" + str((1 << 29) + 1).encode()), UNSUPPORTED),
    "pos_ten_digits": (HEAD + _rec(pos=b"9999999999"), UNSUPPORTED),
    "name_of_1025_bytes": (HEAD + _rec(chrom=b"n" * 1025), UNSUPPORTED),
}
ACCEPTED = {
    "end_at_2_29": HEAD + _rec(pos=str(1 << 29).encode()) + _rec(pos=str(1 << 29).encode(), info=b"END=" + str(1 << 29).encode()),
    "name_of_1024_bytes": HEAD + _rec(chrom=b"n" * 1024) + _rec(chrom=b"n" * 1023 + b"m"),
    "pos_repeats": HEAD + _rec() + _rec() + _rec(pos=b"0000000100"),
}


def _raw(phi, text, flags, kind):
    from phi_amd import _capi
    L = _capi.load()
    buf = np.frombuffer(text, np.uint8)
    p, size, q, qsize = C.c_void_p(1), C.c_int64(-1), C.c_void_p(1), C.c_int64(-1)
    info, iinfo = _capi.PhiDeflateInfo(), _capi.PhiBgzfIndexInfo()
    rc = L.phi_deflate_bgzf_indexed(0, buf.ctypes.data if len(buf) else None, len(buf), flags, kind, C.byref(p), C.byref(size), C.byref(q),
                                    C.byref(qsize), C.byref(info), C.byref(iinfo))
    if rc == 0:
        L.phi_deflate_free(p)
        L.phi_deflate_free(q)
    return rc, p.value, q.value, iinfo.detail.decode()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(phi, name):
    text, status = REFUSALS[name]
    with pytest.raises(T.Invalid if status == INVALID else T.Unsupported):      # the per-line writer refuses it for the same reason
        T.tbi_bytes(text, T.member_offsets(K.zlib_bgzf(text)))
    rc, p, q, detail = _raw(phi, text, 0, T.TBI_VCF)
    assert rc == status and p is None and q is None and detail, (rc, p, q, detail)
    if name not in ("contig_comes_back",):
        assert re.search(r"line \d+", detail), detail
    _indexed_vcf(phi, HEAD + _rec())                                    # a valid call afterwards in the same process
    assert len(phi.deflate_bgzf_indexed(text, "gzi")[1]) == 8          # the same text is fine where no VCF is read


def test_refused_arguments(phi):
    text = HEAD + _rec()
    for kind in (0, 3, -1, T.GZI | T.TBI_VCF, 4):
        rc, p, q, detail = _raw(phi, text, 0, kind)
        assert rc == INVALID and p is None and q is None and "index_kind" in detail, (kind, rc, detail)
    for kind in (T.GZI, T.TBI_VCF):
        rc, p, q, detail = _raw(phi, text, 2, kind)                     # PHI_DEFLATE_NO_EOF
        assert rc == INVALID and p is None and q is None and "NO_EOF" in detail
        rc, p, q, detail = _raw(phi, text, 8, kind)
        assert rc == INVALID and p is None and q is None and "flags" in detail
        assert _raw(phi, text, 0, kind)[0] == 0
        assert _raw(phi, text, 1, kind)[0] == 0                         # PHI_DEFLATE_NO_MATCH stays a flag of the writer
    _indexed_vcf(phi, text)


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_the_near_side_of_every_limit(phi, name):
    _indexed_vcf(phi, ACCEPTED[name])


# ------------------------------------------------------------------ 4b. END= across the borders of the marks' lanes

def _end_text(k, border, n_mod=None, final_newline=True):
    """A handful of records with END= in INFO, the ID of each padded so that a multiple of `border` lies in front of byte k of
    the five bytes (tab or ';', 'E', 'N', 'D', '='); then one more padded so that len(text) % 16 == n_mod"""
    text, pos = HEAD, 100
    for form in (b"END=%d", b"X=1;END=%d", b"END=%d;Y=2", b"SVTYPE=DEL;END=%d"):
        for pad in range(1, border + 1):
            r = b"\t".join([b"c1", b"%d" % pos, b"i" * pad, b"A", b"C", b".", b"PASS", form % (pos + 50)]) + b"\n"
            if (len(text) + r.index(b"END=") - 1 + k) % border == 0:
                break
        else:
            raise AssertionError("no padding found")
        text, pos = text + r, pos + 100
    if n_mod is not None:
        for pad in range(1, 17):
            r = b"\t".join([b"c1", b"%d" % pos, b"i" * pad, b"A", b"C", b".", b"PASS", b"END=%d" % (pos + 7)]) + b"\n"
            if (len(text) + len(r) - (not final_newline)) % 16 == n_mod:
                break
        text += r
    return text if final_newline else text[:-1]


END_CASES = {"lane_border_byte_%d" % k: (k, 16, None, True) for k in range(5)}
END_CASES.update({
    "workgroup_border": (1, 4096, None, True),          # the delimiter the last byte of a workgroup's 4096, END= in the next one's
    "n_mod_16_is_0": (2, 16, 0, True), "n_mod_16_is_1": (3, 16, 1, True), "n_mod_16_is_15": (4, 16, 15, True),
    "no_final_newline": (1, 16, 1, False),
})


@pytest.mark.parametrize("name", sorted(END_CASES))
def test_end_places_across_lane_and_workgroup_borders(phi, name):
    """The marks take the text 16 bytes a lane, 4096 a workgroup: "END=" with the tab or ';' in front of it split by a border
    at each of its bytes, texts that end 0, 1 and 15 bytes into a lane, one without its last line feed.  The index is the
    per-line writer's, whose ends here all come from END (POS + 50, not POS + len(REF))."""
    k, border, n_mod, final_newline = END_CASES[name]
    text = _end_text(k, border, n_mod, final_newline)
    assert text.endswith(b"\n") == final_newline and (n_mod is None or len(text) % 16 == n_mod)
    assert all((text.index(b"END=%d" % (p + 50)) - 1 + k) % border == 0 for p in (100, 200, 300, 400))
    recs = [T.record_of(ln) for _, _, ln in T.lines_of(text) if not ln.startswith(b"#")]
    assert [r[2] - r[1] for r in recs[:4]] == [51] * 4
    _, _, info = _indexed_vcf(phi, text)
    assert info["records"] == len(recs)


# ------------------------------------------------------------------ 5. empty inputs

def test_texts_without_a_record(phi):
    for text in (b"", HEAD, HEAD[:-1], b"#"):
        data, tbi, info = _indexed_vcf(phi, text)
        idx = T.parse_tbi(tbi)
        assert idx["names"] == [] and info["records"] == 0 and info["contigs"] == 0 and info["chunks"] == 0
        assert info["meta_lines"] == len(T.lines_of(text))
        data2, gzi, ginfo = phi.deflate_bgzf_indexed(text, "gzi")
        assert data2 == data and gzi == b"\0" * 8 and ginfo["index_bytes"] == 8


# ------------------------------------------------------------------ 6. .gzi + .fai

def _format_fasta(name, seq):
    from phi_amd.ilp_index import host_lib
    L = host_lib()
    out = []
    for call in (lambda t, n: L.phi_format_fasta(name, seq, len(seq), C.byref(t), C.byref(n)),
                 lambda t, n: L.phi_format_fasta_fai(name, len(seq), C.byref(t), C.byref(n))):
        t, n = C.c_void_p(), C.c_int64()
        assert call(t, n) == 0
        out.append(C.string_at(t, n.value))
        L.phi_host_free_text(t)
    return out


@pytest.mark.parametrize("length", [0, 1, 79, 80, 81, 65199, 65280, 300000])
def test_fasta_slices_through_gzi_and_fai(phi, length):
    rng = np.random.default_rng(length + 7)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)].tobytes()
    text, fai = _format_fasta(b"hap_1 sample", seq)
    data, gzi, info = phi.deflate_bgzf_indexed(text, "gzi")
    assert data == phi.deflate_bgzf(text) and bgzf_util.text_of(data) == text
    off = T.member_offsets(data)
    assert gzi == T.gzi_bytes(off) and len(gzi) == 8 + 16 * max(-(-len(text) // B) - 1, 0)
    assert info["index_bytes"] == len(gzi) and info["device_ms"] == 0 and info["records"] == 0
    assert T.fai_fields(fai) == (b"hap_1", length, len(b">hap_1 sample LN:%d\n" % length), min(length, 80), min(length, 80) + 1 if length else 0)
    if not length:
        return
    slices = [(0, length), (0, 1), (length - 1, 1)] + [(int(s), int(rng.integers(0, min(length - s, 500) + 1))) for s in rng.integers(0, length, 97)]
    for s, n in slices:
        touched = set()
        assert T.fasta_slice(data, gzi, fai, s, n, touched) == seq[s:s + n], (s, n)
        if n:                                                           # only the members that hold the slice were inflated
            u0, u1 = T.fai_offset(fai, s), T.fai_offset(fai, s + n - 1)
            assert touched == set(range(u0 // B, u1 // B + 1)), (s, n, touched)


# ------------------------------------------------------------------ 7. calls.write_vcf(..., bgzf=True, index=True)

def test_write_vcf_with_its_index(phi, oracle, ctx_factory, tmp_path):
    from graphgen import random_graph, walk_sequence
    from phi_amd.calls import write_vcf
    rng = np.random.default_rng(77)
    g = random_graph(rng, n_sites=60, n_walks=3, seg_len=(200, 900), alt_len=(1, 40), p_del=0.3)
    ctx = ctx_factory(k=9, w=4, threshold=1.0, recombination=3)
    A = g.arrays()
    ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])
    calls = ctx.calls(0, walk=1)
    ctx.close()
    assert calls["n_calls"] > 10
    ref_len = len(walk_sequence(g, 0))
    plain, packed, both = tmp_path / "c.vcf", tmp_path / "c.vcf.gz", tmp_path / "i.vcf.gz"
    n_written = write_vcf(str(plain), calls, "ctg", ref_len, "s1")
    assert write_vcf(str(packed), calls, "ctg", ref_len, "s1", bgzf=True) == n_written
    assert write_vcf(str(both), calls, "ctg", ref_len, "s1", bgzf=True, index=True) == n_written
    assert sorted(p.name for p in tmp_path.iterdir()) == ["c.vcf", "c.vcf.gz", "i.vcf.gz", "i.vcf.gz.tbi"]
    data, tbi, text = both.read_bytes(), (tmp_path / "i.vcf.gz.tbi").read_bytes(), plain.read_bytes()
    assert data == packed.read_bytes() and bgzf_util.text_of(data) == text
    bgzf_util.members(tbi)
    idx = T.parse_tbi(tbi)
    recs = [ln for ln in text.split(b"\n") if ln and not ln.startswith(b"#")]
    assert idx["names"] == [b"ctg"] and len(recs) == n_written[0]
    assert T.query(data, idx, b"ctg", 0, ref_len) == recs               # every record for the whole contig
    _check_queries(data, tbi, text, K.draw_regions(text, 40, seed=3))
    with pytest.raises(ValueError):
        write_vcf(str(tmp_path / "x.vcf"), calls, "ctg", ref_len, "s1", index=True)
    assert not (tmp_path / "x.vcf").exists() and not (tmp_path / "x.vcf.tbi").exists()


# ------------------------------------------------------------------ 8. the command line

INDEX_LINE = re.compile(r"BGZF index: (\d+) bytes written to (\S+), (\d+) records on (\d+) contigs, (\d+) chunks, (\d+) windows; ([\d.]+) ms on device (\d+)")


def test_command_line_writes_the_three_indexes(tmp_path):
    from test_gpu_chop import _run_cli
    gfa, reads = os.path.join(DATA, "test.gfa"), os.path.join(DATA, "read.fa")
    base = ["-g", gfa, "-r", reads, "-k", "3", "-w", "2", "--calls-ref", "test_hap_1.0"]
    r = _run_cli(["--bgzf-index"] + base + ["-o", str(tmp_path / "r.fa"), "--calls", str(tmp_path / "r.vcf")], tmp_path)
    assert r.returncode == 1 and "--bgzf-index" in r.stderr and "goes with --bgzf" in r.stderr and not [p.name for p in tmp_path.iterdir() if p.name.startswith("r.")]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    a = _run_cli(["--bgzf"] + base + ["-o", str(tmp_path / "a" / "o.fa.gz"), "--calls", str(tmp_path / "a" / "o.vcf.gz")], tmp_path)
    b = _run_cli(["--bgzf", "--bgzf-index"] + base + ["-o", str(tmp_path / "b" / "o.fa.gz"), "--calls", str(tmp_path / "b" / "o.vcf.gz")], tmp_path)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr[-2000:], b.stderr[-2000:])
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["o.fa.gz", "o.vcf.gz"] and "BGZF index:" not in a.stderr
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["o.fa.gz", "o.fa.gz.fai", "o.fa.gz.gzi", "o.vcf.gz", "o.vcf.gz.tbi"]
    for n in ("o.fa.gz", "o.vcf.gz"):
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes()
    logged = {os.path.basename(m.group(2)): m for m in INDEX_LINE.finditer(b.stderr)}
    assert sorted(logged) == ["o.fa.gz.fai", "o.fa.gz.gzi", "o.vcf.gz.tbi"]
    # the calls through their .tbi
    data, tbi = (tmp_path / "b" / "o.vcf.gz").read_bytes(), (tmp_path / "b" / "o.vcf.gz.tbi").read_bytes()
    text = bgzf_util.text_of(data)
    bgzf_util.members(tbi)
    idx = T.parse_tbi(tbi)
    recs = [ln for ln in text.split(b"\n") if ln and not ln.startswith(b"#")]
    assert len(recs) > 0 and len(idx["names"]) == 1 and T.query(data, idx, idx["names"][0], 0, T.MAX_END) == recs
    want, counts = T.tbi_bytes(text, T.member_offsets(data))
    assert bgzf_util.text_of(tbi) == want
    m = logged["o.vcf.gz.tbi"]
    assert (int(m.group(1)), int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6))) == (len(tbi), counts["records"], counts["contigs"], counts["chunks"], counts["windows"])
    for nm, lo, hi in K.draw_regions(text, 20, seed=4):
        assert T.query(data, idx, nm, lo, hi) == T.overlapping(text, nm, lo, hi)
    # the FASTA through .gzi + .fai
    fz, gzi, fai = ((tmp_path / "b" / n).read_bytes() for n in ("o.fa.gz", "o.fa.gz.gzi", "o.fa.gz.fai"))
    fasta = bgzf_util.text_of(fz)
    header, seq = fasta.split(b"\n", 1)
    seq = seq.replace(b"\n", b"")
    name, length, offset, _, _ = T.fai_fields(fai)
    assert (b">" + name, length, offset) == (header.split(b" ")[0], len(seq), len(header) + 1) and gzi == T.gzi_bytes(T.member_offsets(fz))
    for s in range(length):
        assert T.fasta_slice(fz, gzi, fai, s, length - s) == seq[s:]
    assert int(logged["o.fa.gz.gzi"].group(1)) == len(gzi) and int(logged["o.fa.gz.fai"].group(1)) == len(fai)
