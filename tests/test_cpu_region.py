"""CPU: the host side of a region read (PHI --region, set_graph_vcf(region=)) -- phi_amd/csrc/region_host.h through libphi_host.
The member plan against the index reader of tests/tabix_ref.py on a synthetic three-contig VCF and on MHC_4.vcf.gz, with the
per-line .tbi and with the same index laid out as htslib lays one out; FASTA slices through the .fai / .gzi that samtools and
bgzip wrote for the golden FASTA and through indexes written here; the refusals; phi_vcf_read against its split; and the
stand-alone program phi_amd/csrc/host/region_host_selftest.cpp, plain and under AddressSanitizer + UndefinedBehaviorSanitizer
(`make -C phi_amd/csrc/host region_host_sanitize`)."""
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_index_cases as K
import region_cases as R
import tabix_ref as T
from conftest import DATA, ROOT

SAN = os.path.join(ROOT, "build", "sanitize")
IO, INVALID, UNSUPPORTED = -1, -4, -5


@pytest.fixture(scope="module")
def H():
    import __graft_entry__
    __graft_entry__.ensure_built()
    from phi_amd import ilp_index
    return ilp_index


@pytest.fixture(scope="module")
def synthetic():
    ref = R.reference()
    text, recs = R.synthetic_vcf(ref)
    return ref, text, recs


@pytest.fixture(scope="module")
def mhc_text():
    with gzip.open(os.path.join(DATA, "MHC_4.vcf.gz"), "rb") as f:
        return f.read()


def _write(tmp_path, text, style):
    data, tbi = R.indexed(text)
    ref_tbi = tbi
    if style == "htslib":
        tbi, ref_tbi = R.htslib_style(tbi)
    path = tmp_path / "in.vcf.gz"
    path.write_bytes(data)
    (tmp_path / "in.vcf.gz.tbi").write_bytes(tbi)
    return str(path), data, T.parse_tbi(ref_tbi)


def _check_plan(H, path, data, idx, text, regions, merged=False):
    found = 0
    recs = [T.record_of(ln) + (ln,) for _, _, ln in T.lines_of(text) if not ln.startswith(b"#")]       # overlapping(), its records parsed once
    for name, b, e in regions:
        cache = {}
        got = T.query(data, idx, name, b, e, cache)
        want = [ln for n, rb, re, ln in recs if n == name and rb < e and re > b]
        # (merged chunks overlap the chunks of other bins and query() reads every chunk: it then finds a record more than once)
        assert set(got) == set(want) and len(got) >= len(want) if merged else got == want
        with H.RegionPlan(path, name.decode(), b, e) as p:
            assert set(p.member_at.tolist()) == set(cache), (name, b, e)
            assert p.header == R.header_of(text)
            inflated = T.inflate_all(p.gz) if p.gz else b""
            assert len(inflated) == p.member_text_off[-1] and len(p.gz) == sum(T.inflate_member(data, int(a))[1] for a in p.member_at)
            assert (np.diff(p.ranges.ravel()) >= 0).all() and (p.ranges[:, 1] > p.ranges[:, 0]).all()
            lines = []
            for p0, p1 in p.ranges.tolist():
                assert (p0 == 0 or p0 in p.member_text_off or inflated[p0 - 1:p0] == b"\n") and inflated[p1 - 1:p1] == b"\n"
                for ln in inflated[p0:p1].split(b"\n"):
                    if ln and not ln.startswith(b"#"):
                        n, rb, re = T.record_of(ln)
                        if n == name and rb < e and re > b:
                            lines.append(ln)
            assert lines == want, (name, b, e)
        found += bool(want)
    assert 4 * found >= 3 * len(regions)


@pytest.mark.parametrize("style", ["per_line", "htslib"])
def test_plan_on_the_synthetic_vcf(H, synthetic, tmp_path, style):
    _, text, _ = synthetic
    path, data, idx = _write(tmp_path, text, style)
    _check_plan(H, path, data, idx, text, K.draw_regions(text, 200, seed=11), merged=style == "htslib")


@pytest.mark.parametrize("style", ["per_line", "htslib"])
def test_plan_on_the_mhc_vcf(H, mhc_text, tmp_path, style):
    path, data, idx = _write(tmp_path, mhc_text, style)
    _check_plan(H, path, data, idx, mhc_text, K.draw_regions(mhc_text, 200, seed=12), merged=style == "htslib")


def test_plans_without_members(H, synthetic, tmp_path):
    _, text, recs = synthetic
    path, _, _ = _write(tmp_path, text, "htslib")
    last = max(r[2] for r in recs if r[0] == b"chr10")
    for name, b, e, known in (("chr10", ((last - 1 >> 14) + 1) << 14, 1 << 29, True), ("chr10", 1 << 29, (1 << 29) + 5, True), ("nope", 0, 1000, False),
                              ("chr1", 500, 500, True), ("chr1", 600, 500, True), ("chr", 0, 1 << 29, False)):
        with H.RegionPlan(path, name, b, e) as p:
            assert len(p.member_at) == 0 and len(p.ranges) == 0 and p.gz == b"" and p.in_index == known, (name, b, e)


def test_region_grammar(H):
    assert H.parse_region("chr6") == ("chr6", 1, None)
    assert H.parse_region("chr6:28,510,120-33,480,577") == ("chr6", 28510120, 33480577)
    assert H.parse_region("chr6:100") == ("chr6", 100, None) and H.parse_region("chr6:100-") == ("chr6", 100, None)
    assert H.parse_region("HLA-A*01:01:5-9") == ("HLA-A*01:01", 5, 9) and H.parse_region("a:b") == ("a:b", 1, None)
    assert H.parse_region("c:7-7") == ("c", 7, 7)
    for bad in ("", "chr1:", ":5-10", "chr1:10-5", "chr1:0-5", "chr1:1-2-3", "chr1:-5", "chr1:1234567890123456789", "chr1:,"):
        with pytest.raises(H.HostError) as ei:
            H.parse_region(bad)
        assert ei.value.status == INVALID and "region" in str(ei.value), bad


# ------------------------------------------------------------------ FASTA slices

def test_the_golden_fasta_through_the_real_index_files(H):
    fa = os.path.join(DATA, "MHC-CHM13.0.fa.gz")
    assert os.path.exists(fa + ".fai") and os.path.exists(fa + ".gzi")      # written by samtools faidx and bgzip -r
    with gzip.open(fa, "rb") as f:
        whole = f.read()
    name = whole[1:whole.index(b"\n")].split()[0].decode()
    seq = whole[whole.index(b"\n") + 1:].replace(b"\n", b"").upper()
    rng = np.random.default_rng(5)
    cuts = [(0, 1), (0, len(seq)), (len(seq) - 1, len(seq)), (59, 61), (60, 120)]
    while len(cuts) < 200:
        b = int(rng.integers(0, len(seq)))
        cuts.append((b, min(len(seq), b + int(rng.choice([1, 50, 61, 5000, 200000])))))
    for b, e in cuts:
        got, info = H.fasta_slice(fa, name, b, e, with_info=True)
        assert got == seq[b:e] and info["contig_len"] == len(seq), (b, e)
        assert 1 <= info["members"] <= (e - b) * 62 // 61 // 65280 + 3                                    # only the members that hold the range
    assert H.fasta_slice(fa, name, 1000) == seq[1000:] and H.fasta_slice(fa, name, 7, 7) == b""


@pytest.mark.parametrize("packed", [False, True])
def test_slices_of_a_multi_record_fasta(H, synthetic, tmp_path, packed):
    ref = synthetic[0]
    fasta = R.fasta_text(ref)
    path = tmp_path / ("m.fa.gz" if packed else "m.fa")
    gz = K.zlib_bgzf(fasta)
    path.write_bytes(gz if packed else fasta)
    (tmp_path / (path.name + ".fai")).write_bytes(R.fai_text(fasta))
    if packed:
        (tmp_path / (path.name + ".gzi")).write_bytes(T.gzi_bytes(T.member_offsets(gz)))
    rng = np.random.default_rng(6)
    for name, length in R.CONTIGS:
        cuts = [(0, length), (length - 1, length), (length - length % R.LINE - 1, length), (R.LINE - 1, R.LINE + 1), (0, R.LINE), (R.LINE, 2 * R.LINE)]
        while len(cuts) < 70:
            b = int(rng.integers(0, length))
            cuts.append((b, min(length, b + int(rng.choice([1, 59, 60, 61, 3000, 70000])))))
        for b, e in cuts:
            assert H.fasta_slice(str(path), name, b, e) == ref[name][b:e], (name, b, e)
    with pytest.raises(H.HostError) as ei:
        H.fasta_slice(str(path), "chr2", 0, 5)
    assert ei.value.status == INVALID and "chr2" in str(ei.value)


# ------------------------------------------------------------------ refusals

def test_refusals(H, synthetic, tmp_path):
    ref, text, _ = synthetic
    vcf, fa = R.write_files(tmp_path, text, ref)
    with H.RegionPlan.open(vcf, fa, "chr10:1,000-2,000") as p:
        assert (p.name, p.beg, p.end, p.contig_len) == ("chr10", 999, 2000, 50000) and p.ref == ref["chr10"][999:2000]
    with H.RegionPlan.open(vcf, fa, "ctgB:39000-99999999") as p:
        assert (p.beg, p.end) == (38999, 40000)

    def refused(code, word, fn, *a):
        with pytest.raises(H.HostError) as ei:
            fn(*a)
        assert ei.value.status == code and word in str(ei.value), str(ei.value)

    refused(INVALID, "inverted", H.RegionPlan.open, vcf, fa, "chr1:10-5")
    refused(INVALID, "empty", H.RegionPlan.open, vcf, fa, "chr1:100001")
    refused(INVALID, ".fai holds no record", H.RegionPlan.open, vcf, fa, "chrX:1-5")
    tbi = tmp_path / "syn.vcf.gz.tbi"
    keep = tbi.read_bytes()
    one = b"".join(ln + b"\n" for ln in text.split(b"\n") if ln and (ln.startswith(b"#") or ln.startswith(b"chr1\t")))
    tbi.write_bytes(R.indexed(one)[1])                                   # an index that names chr1 alone
    refused(INVALID, ".tbi holds no contig", H.RegionPlan.open, vcf, fa, "ctgB")
    os.remove(tbi)
    refused(IO, ".tbi", H.RegionPlan.open, vcf, fa, "chr1")
    (tmp_path / "syn.vcf.gz.csi").write_bytes(K.zlib_bgzf(b"CSI\1" + bytes(40)))
    refused(UNSUPPORTED, "CSI", H.RegionPlan.open, vcf, fa, "chr1")
    tbi.write_bytes(K.zlib_bgzf(b"CSI\1" + bytes(40)))
    refused(UNSUPPORTED, "CSI", H.RegionPlan, vcf, "chr1", 0, 100)
    raw = bytearray(T.inflate_all(keep))
    for at, value in ((8, 0), (8, 1), (12, 2), (16, 3), (24, ord("@"))):    # generic, SAM, another column, another meta character
        other = bytearray(raw)
        other[at:at + 4] = value.to_bytes(4, "little")
        tbi.write_bytes(K.zlib_bgzf(bytes(other)))
        refused(UNSUPPORTED, "preset", H.RegionPlan, vcf, "chr1", 0, 100)
    tbi.write_bytes(keep)
    plain_gz = tmp_path / "one.vcf.gz"
    plain_gz.write_bytes(gzip.compress(text))
    (tmp_path / "one.vcf.gz.tbi").write_bytes(keep)
    refused(UNSUPPORTED, "not BGZF", H.RegionPlan, str(plain_gz), "chr1", 0, 100)
    (tmp_path / "one.fa.gz").write_bytes(gzip.compress(R.fasta_text(ref)))
    (tmp_path / "one.fa.gz.fai").write_bytes((tmp_path / "syn.fa.gz.fai").read_bytes())
    refused(UNSUPPORTED, "not BGZF", H.fasta_slice, str(tmp_path / "one.fa.gz"), "chr1", 0, 10)
    os.remove(tmp_path / "syn.fa.gz.gzi")
    refused(IO, ".gzi", H.RegionPlan.open, vcf, fa, "chr1:5-50")
    os.remove(tmp_path / "syn.fa.gz.fai")
    refused(IO, ".fai", H.RegionPlan.open, vcf, fa, "chr1:5-50")


# ------------------------------------------------------------------ phi_vcf_read and its split

ARRAYS = ("ref_seq", "rec_start", "rec_end", "gt_index", "alt_off", "alt_pos", "alt_bytes", "site_off", "text_off", "text")


def test_phi_vcf_read_equals_the_rule_pass_over_the_same_text(H, mhc_text):
    vcf, fa = os.path.join(DATA, "MHC_4.vcf.gz"), os.path.join(DATA, "MHC-CHM13.0.fa.gz")
    with gzip.open(fa, "rb") as f:
        whole = f.read()
    seq = whole[whole.index(b"\n") + 1:].replace(b"\n", b"")
    a = H.VcfGraph(vcf, fa)
    b = H.VcfGraph(None, None, text=(mhc_text, seq, 0, None))
    assert a.n_records > 30000 and (a.origin, b.origin, a.region, b.region) == (0, 0, None, None)
    for n in ("samples", "contig", "n_records", "n_sites", "n_other_contig", "n_ref_mismatch", "n_outside"):
        assert getattr(a, n) == getattr(b, n), n
    for n in ARRAYS:
        assert getattr(a, n).tobytes() == getattr(b, n).tobytes(), n


def test_the_rule_pass_with_an_origin(H, synthetic):
    ref, text, recs = synthetic
    name, (b, e) = "chr1", (20000, 60000)
    lines = T.overlapping(text, name.encode(), b, e)
    cut = R.header_of(text) + b"".join(ln + b"\n" for ln in lines)
    v = H.VcfGraph(None, None, text=(cut, ref[name][b:e], b, name))
    whole = H.VcfGraph(None, None, text=(text, ref[name], 0, name))
    inside = [i for i in range(whole.n_records) if whole.rec_start[i] >= b and whole.rec_end[i] <= e]
    assert v.origin == b and v.n_records == len(inside) > 300 and v.n_ref_mismatch == 0
    assert (v.rec_start + b).tolist() == whole.rec_start[inside].tolist() and (v.rec_end + b).tolist() == whole.rec_end[inside].tolist()
    # the records that reach over an edge: counted, and no others
    assert v.n_outside == sum(1 for n, rb, re, ln in recs if n == name.encode() and rb < e and re > b and b"<DEL>" not in ln
                              and (rb < b or rb + len(ln.split(b"\t")[3]) > e))


# ------------------------------------------------------------------ the stand-alone program

@pytest.mark.parametrize("build", ["plain", "asan"])
def test_region_host_selftest(build):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "region_host_sanitize"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r =subprocess.run([os.path.join(SAN, "region_host_selftest_" + build)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    done = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert done == ["region_grammar", "tbi_parse", "chunk_selection", "htslib_style", "tbi_truncated", "fai_arithmetic", "member_plan"], r.stdout
