"""Region reads of an indexed VCF and FASTA on the GPU: phi_vcf_region_filter against tests/tabix_ref.py's overlapping() on the
synthetic three-contig VCF of tests/region_cases.py (its corners listed there and in test_filter_exactness), in one batch and
in batches of two members, through the per-line index and the htslib-style one; set_graph_vcf(region=) against the same call on
files cut in Python (the acceptance test); a contig by name alone; PHI --region with --calls in the contig's coordinates; and
that a refused call leaves the device as it found it."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bgzf_index_cases as K
import region_cases as R
import tabix_ref as T
from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu
PHI = os.path.join(ROOT, "phi_amd", "PHI")
INVALID = -1


@pytest.fixture(scope="module")
def phi():
    import __graft_entry__
    __graft_entry__.ensure_built()
    import phi_amd
    return phi_amd


@pytest.fixture(scope="module")
def syn(tmp_path_factory):
    """the synthetic VCF, its records, its files with the per-line index and with the htslib-style one: built once, never changed"""
    ref = R.reference()
    text, recs = R.synthetic_vcf(ref)
    a, b = tmp_path_factory.mktemp("per_line"), tmp_path_factory.mktemp("htslib")
    vcf, fa = R.write_files(a, text, ref)
    hts, _ = R.htslib_style((a / "syn.vcf.gz.tbi").read_bytes())
    vcf_h, fa_h = R.write_files(b, text, ref, tbi=hts)
    return dict(ref=ref, text=text, recs=recs, header=R.header_of(text), files={"per_line": (vcf, fa), "htslib": (vcf_h, fa_h)},
                tmp=tmp_path_factory.mktemp("cut"))


def _corner_regions(text, recs):
    """(name, b, e, records expected at least) -- every corner the filter can get wrong, found in the records themselves"""
    chr1 = [r for r in recs if r[0] == b"chr1"]
    dele = next(r for r in chr1 if r[2] - r[1] >= 3 and b"END=" not in r[3])            # a deletion: REF of three bases or more
    sv = next(r for r in chr1 if b"<DEL>" in r[3])                                         # END= 400 bases on
    long_ = next(r for r in recs if len(r[3]) > R.BLOCK)
    gap = next((p, n) for p, n in zip(chr1, chr1[1:]) if n[1] - p[2] > 30 and not any(r[1] < n[1] and r[2] > p[2] for r in chr1))
    starts = sorted(s for s, _, _ in T.lines_of(text))
    crossing = next(ln for s, n, ln in T.lines_of(text) if s // R.BLOCK != (n - 1) // R.BLOCK and not ln.startswith(b"#") and len(ln) < 1000)
    cross = T.record_of(crossing)
    assert starts
    out = [
        (b"chr1", dele[2], dele[2] + 20, 0), (b"chr1", dele[2] - 1, dele[2] + 20, 1),      # beg + len(REF) == b: out; == b + 1: in
        (b"chr1", dele[1] - 20, dele[1] + 1, 1), (b"chr1", dele[1] - 20, dele[1], 0),      # starts at e - 1: in; at e: out
        (b"chr1", sv[2] - 1, sv[2], 1), (b"chr1", sv[2], sv[2] + 1, 0), (b"chr1", sv[1] + 200, sv[1] + 201, 1),   # through END= alone
        (b"chr1", recs[0][1], recs[0][2], 1), (recs[-1][0], recs[-1][1], recs[-1][2], 1),  # the first and the last record of the file
        (b"chr1", gap[0][2], gap[1][1], 0),                                                # no record
        (b"chr1", 10000, 70000, 500), (b"chr1", 0, 1 << 29, len(chr1)),                    # several 16-kb windows; the contig
        (b"chr10", 0, 1 << 29, 300), (b"chr1", 16383, 16385, 0), (b"ctgB", 0, 100, 0),
        (long_[0], long_[1], long_[2], 1), (cross[0], cross[1], cross[2], 1),              # longer than a member; across a member boundary
        (b"chr", 0, 1 << 29, 0), (b"chr100", 0, 1 << 29, 0),
    ]
    return out


def test_filter_exactness(phi, syn, monkeypatch):
    from phi_amd import ilp_index as H
    from phi_amd.context import vcf_region_filter
    text, recs = syn["text"], syn["recs"]
    regions = _corner_regions(text, recs)
    regions += [(n, b, e, 0) for n, b, e in K.draw_regions(text, 60 - len(regions), seed=21)]
    assert len(regions) == 60
    for style in ("per_line", "htslib"):
        vcf = syn["files"][style][0]
        for batch in (None, "2"):
            if batch is None:
                monkeypatch.delenv("PHI_VCF_REGION_BATCH", raising=False)
            else:
                monkeypatch.setenv("PHI_VCF_REGION_BATCH", batch)
            spanned = 0
            for name, b, e, least in regions:
                want = [ln for n, rb, re, ln in recs if n == name and rb < e and re > b]
                assert len(want) >= least, (name, b, e)
                with H.RegionPlan(vcf, name.decode(), b, e) as p:
                    got, info = vcf_region_filter(p.gz, p.ranges, name, b, e)
                    assert got == b"".join(ln + b"\n" for ln in want), (style, batch, name, b, e, len(want))
                    assert info["members"] == len(p.member_at) and info["gz_bytes"] == len(p.gz) and info["text_bytes"] == p.member_text_off[-1]
                    assert info["lines_kept"] == len(want) <= info["lines_seen"]
                    per = 2 if batch else 256
                    assert (info["batches"] >= -(-len(p.member_at) // per)) and (info["batches"] > 0) == (len(p.ranges) > 0 and len(p.member_at) > 0)
                    if len(p.member_at):
                        assert info["inflate_ms"] > 0 and info["filter_ms"] > 0
                    spanned += info["reinflated_members"] > 0
            assert (spanned > 0) == (batch is not None), (style, batch, spanned)     # lines and ranges did span batches


def _graph_state(ctx, v):
    return dict(seq_concat=bytes(v.seq_concat), seq_off=v.seq_off.tolist(), adj_off=v.adj_off.tolist(), adj=v.adj.tolist(), walk_off=np.asarray(v.walk_off).tolist(),
                hap=list(v.hap_id2name), top=None if v.top_order_map is None else v.top_order_map.tolist(), entries=ctx.walk_entries().tolist(), mismatch=v.n_ref_mismatch)


def _reads_of(seq, n=120):
    return [seq[a:a + 150] for a in range(0, min(len(seq) - 150, 100 * n), 100)]


def _both_routes(ctx_factory, files, cut, region, reads, **kw):
    a, b = ctx_factory(), ctx_factory()
    a.set_params()
    b.set_params()
    auto = "auto_panel" in kw
    va = a.set_graph_vcf(files[0], files[1], region=region, **(dict(kw, reads=reads) if auto else kw))
    vb = b.set_graph_vcf(cut[0], cut[1], **(dict(kw, reads=reads) if auto else kw))
    sa, sb = _graph_state(a, va), _graph_state(b, vb)
    for key in sa:
        assert sa[key] == sb[key], (region, key)
    res = []
    for c in (a, b):
        if not auto:
            c.add_reads(reads)
        res.append(c.solve())
    for key in ("objective", "optimal", "spectrum_size", "filtered", "retained", "n_in_model", "hap_len"):
        assert res[0][key] == res[1][key], (region, key)
    assert a.path_sequence(res[0]["hap_len"]) == b.path_sequence(res[1]["hap_len"]) and res[0]["hap_len"] > 1000
    return va, vb


def _cut(syn, tag, name, b, e):
    lines = [ln for n, rb, re, ln in syn["recs"] if n == name.encode() and rb < e and re > b]
    return R.cut_files(syn["tmp"], tag, syn["header"], lines, syn["ref"][name][b:e], b), lines


@pytest.mark.parametrize("name,b,e", [("chr1", 20000, 60000), ("chr1", 0, 30000), ("chr10", 5000, 45000), ("ctgB", 10000, 30000), ("chr1", 60000, 100000)])
def test_region_graph_equals_the_graph_of_cut_files(ctx_factory, syn, name, b, e):
    b, e = R.quiet_edges(syn["recs"], name.encode(), b, e)
    cut, lines = _cut(syn, f"{name}_{b}", name, b, e)
    region = f"{name}:{b + 1:,}-{e:,}" if e < dict(R.CONTIGS)[name] else f"{name}:{b + 1}"
    va, vb = _both_routes(ctx_factory, syn["files"]["htslib" if name == "chr10" else "per_line"], cut, region, _reads_of(syn["ref"][name][b:e]))
    assert va.region == (name, b, e) and va.origin == b and vb.origin == 0 and vb.region is None and va.contig_len == dict(R.CONTIGS)[name]
    assert va.stats["lines_kept"] == len(lines) > 100 and va.stats["members"] > 0 and va.stats["filter_ms"] > 0 and "plan_s" in va.stats
    assert va.n_outside == vb.n_outside and va.n_records == vb.n_records > 100


def test_region_graph_with_a_panel_of_samples(ctx_factory, syn):
    name, (b, e) = "chr1", R.quiet_edges(syn["recs"], b"chr1", 30000, 70000)
    cut, _ = _cut(syn, "keep", name, b, e)
    va, _ = _both_routes(ctx_factory, syn["files"]["per_line"], cut, f"{name}:{b + 1}-{e}", _reads_of(syn["ref"][name][b:e]), keep_samples=["S1", "S4"])
    assert va.hap_id2name == ["S1.1", "S1.2", "S4.1", "S4.2"]


def test_region_graph_with_a_panel_chosen_from_the_reads(ctx_factory, tmp_path):
    ref = R.reference()
    text, recs = R.synthetic_vcf(ref, n_samples=20)                      # 41 haplotypes
    files = R.write_files(tmp_path, text, ref)
    name, (b, e) = "chr10", R.quiet_edges(recs, b"chr10", 8000, 40000)
    lines = [ln for n, rb, re, ln in recs if n == name.encode() and rb < e and re > b]
    cut = R.cut_files(tmp_path, "auto", R.header_of(text), lines, ref[name][b:e], b)
    va, vb = _both_routes(ctx_factory, files, cut, f"{name}:{b + 1}-{e}", _reads_of(ref[name][b:e], 300), auto_panel=8)
    assert va.auto is not None and va.num_walks == 8 and va.kept_haps.tolist() == vb.kept_haps.tolist()


def test_a_contig_by_name_alone(ctx_factory, syn):
    name = "ctgB"
    only = syn["tmp"] / "ctgB_only.vcf"
    only.write_bytes(syn["header"] + b"".join(ln + b"\n" for n, _, _, ln in syn["recs"] if n == b"ctgB"))
    fa = syn["tmp"] / "ctgB_only.fa"
    fa.write_bytes(b">ctgB\n" + syn["ref"][name] + b"\n")
    va, vb = _both_routes(ctx_factory, syn["files"]["per_line"], (str(only), str(fa)), name, _reads_of(syn["ref"][name]))
    assert va.region == (name, 0, 40000) and va.contig == vb.contig == name and va.n_other_contig == 0 and va.n_outside == 0


@pytest.fixture(scope="module")
def mhc(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mhc_region")
    with gzip.open(os.path.join(DATA, "MHC_4.vcf.gz"), "rb") as f:
        text = f.read()
    # the golden FASTA's record is named "0", the VCF's contig "CHM13#0#0": a region names one contig in both files, so the copy
    # that is indexed here takes the FASTA's name
    text = b"".join(ln if ln.startswith(b"#") else b"0" + ln[ln.index(b"\t"):] for ln in text.splitlines(keepends=True))
    data, tbi = R.indexed(text)
    (tmp / "mhc.vcf.gz").write_bytes(data)
    (tmp / "mhc.vcf.gz.tbi").write_bytes(tbi)
    with gzip.open(os.path.join(DATA, "MHC-CHM13.0.fa.gz"), "rb") as f:
        whole = f.read()
    seq = whole[whole.index(b"\n") + 1:].replace(b"\n", b"").upper()
    recs = [T.record_of(ln) + (ln,) for _, _, ln in T.lines_of(text) if not ln.startswith(b"#")]
    return dict(tmp=tmp, text=text, recs=recs, seq=seq, name=recs[0][0].decode(), vcf=str(tmp / "mhc.vcf.gz"), fa=os.path.join(DATA, "MHC-CHM13.0.fa.gz"))


@pytest.mark.parametrize("b,e", [(1000000, 1200000), (3000000, 3150000)])
def test_mhc_region_equals_the_graph_of_cut_files(ctx_factory, mhc, b, e):
    name = mhc["name"]
    b, e = R.quiet_edges(mhc["recs"], name.encode(), b, e)
    lines = [ln for n, rb, re, ln in mhc["recs"] if rb < e and re > b]
    cut = R.cut_files(mhc["tmp"], f"cut{b}", R.header_of(mhc["text"]), lines, mhc["seq"][b:e], b)
    va, _ = _both_routes(ctx_factory, (mhc["vcf"], mhc["fa"]), cut, f"{name}:{b + 1}-{e}", _reads_of(mhc["seq"][b:e]))
    assert va.stats["lines_kept"] == len(lines) > 100 and va.stats["fasta_members"] <= 6 and va.contig_len == len(mhc["seq"])


# ------------------------------------------------------------------ the command line

def _run_cli(args, cwd, env=None):
    return subprocess.run([PHI] + args, capture_output=True, text=True, cwd=str(cwd), timeout=300, env=dict(os.environ, **(env or {})))


def test_command_line(phi, syn, tmp_path):
    from phi_amd.calls import apply, read_vcf
    name, (b, e) = "chr1", R.quiet_edges(syn["recs"], b"chr1", 20000, 60000)
    cut, _ = _cut(syn, "cli", name, b, e)
    ref = syn["ref"][name]
    # reads of a haplotype that is not the reference: sample S2's first
    from phi_amd import ilp_index as H
    v = H.VcfGraph(cut[0], cut[1])
    gt, ploidy = v.parse_gt()
    v.build(gt, ploidy)
    wo, wv = v.host_walks()
    h = v.hap_id2name.index("S2.1")
    flat = np.frombuffer(bytes(v.seq_concat), np.uint8)
    hap = b"".join(flat[v.seq_off[x]:v.seq_off[x + 1]].tobytes() for x in wv[wo[h]:wo[h + 1]])
    reads = tmp_path / "reads.fa"
    reads.write_bytes(b"".join(b">r%d\n%s\n" % (i, hap[a:a + 150]) for i, a in enumerate(range(0, len(hap) - 150, 60))))
    vcf, fa = syn["files"]["per_line"]
    region = f"{name}:{b + 1}-{e}"
    # (the FASTA's header line is made of the graph file's and the reads file's names: the cut VCF takes the name that gives the same)
    os.mkdir(tmp_path / "cut")
    same_name = tmp_path / "cut" / (os.path.basename(vcf)[:-3] + ".vcf")
    same_name.write_bytes(open(cut[0], "rb").read())
    cut = (str(same_name), cut[1])
    r1 = _run_cli(["--vcf", vcf, "--ref", fa, "--region", region, "-r", str(reads), "-o", "a.fa", "--calls", "a.vcf"], tmp_path,
                  env={"PHI_TIMING": "1"})                                # (the stages are logged under PHI_TIMING)
    r2 = _run_cli(["--vcf", cut[0], "--ref", cut[1], "-r", str(reads), "-o", "b.fa", "--calls", "b.vcf"], tmp_path)
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr[-3000:] + r2.stderr[-2000:]
    assert (tmp_path / "a.fa").read_bytes() == (tmp_path / "b.fa").read_bytes()
    assert re.search(r"stage VCF region plan", r1.stderr) and re.search(r"stage VCF region filter", r1.stderr) and re.search(r"stage VCF \+ FASTA read \(region\)", r1.stderr)
    assert re.search(rf"^Region {name}:{b + 1}-{e} of {len(ref)} bases: \d+ BGZF members", r1.stderr, re.M) and "Region " not in r2.stderr
    header, _, calls, _ = read_vcf(tmp_path / "a.vcf")
    _, _, cut_calls, _ = read_vcf(tmp_path / "b.vcf")
    assert header[2] == f"##contig=<ID={name},length={len(ref)}>"
    n = len(calls["pos"])
    assert n == len(cut_calls["pos"]) > 20 and (np.asarray(calls["pos"]) == np.asarray(cut_calls["pos"]) + b).all()
    lines = [ln.split("\t") for ln in (tmp_path / "a.vcf").read_text().splitlines() if not ln.startswith("#")]
    for c in lines:                                                       # the contig's coordinates
        assert c[0] == name and ref[int(c[1]) - 1:int(c[1]) - 1 + len(c[3])].decode() == c[3]
    m = re.search(r"called span \[(\d+),(\d+)\) of \S+ \((\d+) bases\), \[(\d+),(\d+)\) of the haplotype", r2.stderr)
    r0, r1_, q0, q1 = int(m.group(1)), int(m.group(2)), int(m.group(4)), int(m.group(5))
    query = b"".join((tmp_path / "a.fa").read_bytes().split(b"\n")[1:])
    shifted = dict(calls, pos=np.asarray(calls["pos"]) - b)
    assert apply(ref[b:e], shifted, span=(r0, r1_)) == query[q0:q1]
    # --calls-contig still names the contig; --region needs --vcf and --ref
    r = _run_cli(["-g", os.path.join(DATA, "test.gfa"), "--region", region, "-r", str(reads), "-o", "c.fa"], tmp_path)
    assert r.returncode == 1 and "--region" in r.stderr and "--vcf" in r.stderr
    r = _run_cli(["--vcf", vcf, "--ref", fa, "--region", "chr1:10-5", "-r", str(reads), "-o", "c.fa"], tmp_path)
    assert r.returncode == 1 and "inverted" in r.stderr


# ------------------------------------------------------------------ errors leave things usable

def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_errors_leave_the_device_usable(phi, syn):
    from phi_amd import ilp_index as H
    from phi_amd.context import vcf_region_filter
    text, recs = syn["text"], syn["recs"]
    name, b, e = b"chr1", 10000, 70000
    want = b"".join(ln + b"\n" for n, rb, re, ln in recs if n == name and rb < e and re > b)
    with H.RegionPlan(syn["files"]["per_line"][0], "chr1", b, e) as p:
        gz, ranges = p.gz, p.ranges
    assert vcf_region_filter(gz, ranges, name, b, e)[0] == want           # (the first call settles what the runtime keeps)
    free = _free_bytes()
    corrupt = bytearray(gz)
    corrupt[len(gz) // 2] ^= 0x55                                         # inside a member's deflate data
    with pytest.raises(phi.PhiError) as ei:
        vcf_region_filter(bytes(corrupt), ranges, name, b, e)
    assert ei.value.status == INVALID
    # a POS that is no number, and a line of three fields, inside the range
    victim = next(ln for n, rb, re, ln in recs if n == name and rb > 30000)
    for bad, word in ((victim.replace(b"\t%d\t" % (T.record_of(victim)[1] + 1), b"\t12x4\t", 1), "POS"), (b"chr1\t30001\tshort", "fewer than 8 fields")):
        plan_text = text.replace(victim, bad, 1)
        members = K.zlib_bgzf(plan_text)[:-28]                            # every member, one range from the first record to the end
        assert len(T.member_offsets(members + K.EOF)) > 4
        whole = np.array([[plan_text.index(b"chr1\t"), len(plan_text)]], np.int64)
        with pytest.raises(phi.PhiError) as ei:
            vcf_region_filter(members, whole, name, b, e)
        assert ei.value.status == INVALID and word in str(ei.value) and f"offset {plan_text.index(bad)} " in str(ei.value), str(ei.value)
    assert vcf_region_filter(gz, ranges, name, b, e)[0] == want
    assert _free_bytes() == free
