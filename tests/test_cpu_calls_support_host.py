"""CPU: the VCF writer of the calls with the read support of every call (phi_format_calls_vcf_support, phi_write_calls_vcf_support
of libphi_host) against a Python formatter on the hand-made records of tests/test_cpu_calls_host.py with made-up counts, the plain
writer's text as the support text stripped, the writer under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone
program (phi_amd/csrc/host/calls_writer_selftest.cpp, `make -C phi_amd/csrc/host calls_writer_sanitize`) run as a child process,
the declarations, and the restatement of the rule the GPU test compares with (tests/calls_support_ref.py) on its own."""
import os
import re
import subprocess

import numpy as np
import pytest

import calls_support_ref as R
from conftest import ROOT
from test_cpu_calls_host import CALLS, EXPECTED

# made-up counts; call 2 is the REF = ALT call that is dropped, its counts with it
SUPPORT = dict(alt_hit=np.array([3, 0, 77, 2], np.int32), alt_n=np.array([5, 0, 99, 2147483647], np.int32),
               ref_hit=np.array([0, 1, 88, 0], np.int32), ref_n=np.array([4, 6, 99, 12], np.int32))
PH = ["hapA.1", "hapA.1", "hapB.1", "hapC.2"]
AK = '##FORMAT=<ID=AK,Number=2,Type=Integer,Description="ALT witness minimisers: seen in the reads, all">\n'
RK = '##FORMAT=<ID=RK,Number=2,Type=Integer,Description="REF witness minimisers: seen in the reads, all">\n'


@pytest.fixture(scope="module")
def built():
    from phi_amd import build as B
    B.build_host()
    return True


def _format(calls, contig, contig_len, sample, ph, sup):
    """the file's text, written from the description in include/phi_host.h"""
    out = [f"##fileformat=VCFv4.2\n##source=phi_amd\n##contig=<ID={contig},length={contig_len}>\n",
           '##INFO=<ID=PH,Number=1,Type=String,Description="Panel haplotype the inferred path follows through the call">\n',
           '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n', AK, RK,
           f"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t{sample}\n"]
    ro, ao = calls["ref_off"], calls["alt_off"]
    for k in range(len(calls["pos"])):
        ref, alt = calls["ref_bytes"][ro[k]:ro[k + 1]].decode(), calls["alt_bytes"][ao[k]:ao[k + 1]].decode()
        if ref == alt:
            continue
        info = f"PH={ph[k]}" if ph and ph[k] else "."
        out.append(f"{contig}\t{calls['pos'][k] + 1}\t.\t{ref}\t{alt}\t.\tPASS\t{info}\tGT:AK:RK\t"
                   f"1:{sup['alt_hit'][k]},{sup['alt_n'][k]}:{sup['ref_hit'][k]},{sup['ref_n'][k]}\n")
    return "".join(out)


def _strip(text):
    lines = [re.sub(r"\tGT:AK:RK\t1:[0-9,:]+$", "\tGT\t1", ln) for ln in text.split("\n") if ln + "\n" not in (AK, RK)]
    return "\n".join(lines)


def test_support_writer_byte_for_byte(built, tmp_path):
    from phi_amd.calls import read_support, read_vcf, write_vcf
    p, q = tmp_path / "s.vcf", tmp_path / "plain.vcf"
    assert write_vcf(str(p), CALLS, "chrT", 25, "sample_1", ph=PH, support=SUPPORT) == (3, 1)
    text = p.read_text()
    assert text == _format(CALLS, "chrT", 25, "sample_1", PH, SUPPORT)
    assert "1:3,5:0,4\n" in text and "1:2,2147483647:0,12\n" in text and "77" not in text and "hapB.1" not in text
    # the plain writer's output is unchanged, and is the support output without the two header lines and the two columns
    assert write_vcf(str(q), CALLS, "chrT", 25, "sample_1", ph=PH) == (3, 1)
    assert q.read_text() == EXPECTED == _strip(text)
    got = read_support(str(p))
    keep = [0, 1, 3]
    for n in SUPPORT:
        assert got[n].dtype == np.int32 and got[n].tolist() == SUPPORT[n][keep].tolist(), n
    assert read_vcf(str(p))[2]["pos"].tolist() == [2, 9, 15]                      # read_vcf reads such a file as it reads a plain one
    with pytest.raises(ValueError):
        read_support(str(q))
    # without tags; no call at all
    assert write_vcf(str(p), CALLS, "chrT", 25, "sample_1", support=SUPPORT) == (3, 1)
    assert p.read_text() == _format(CALLS, "chrT", 25, "sample_1", None, SUPPORT)
    empty = dict(pos=np.zeros(0, np.int64), ref_off=np.zeros(1, np.int64), alt_off=np.zeros(1, np.int64), ref_bytes=b"", alt_bytes=b"")
    none = {n: np.zeros(0, np.int32) for n in SUPPORT}
    assert write_vcf(str(p), empty, "chrT", 25, "sample_1", ph=[], support=none) == (0, 0)
    assert p.read_text() == _format(empty, "chrT", 25, "sample_1", [], none) and all(len(v) == 0 for v in read_support(str(p)).values())


def test_support_writer_refusals(built, tmp_path):
    from phi_amd.calls import write_vcf
    from phi_amd.ilp_index import HostError
    with pytest.raises(HostError) as e:
        write_vcf(str(tmp_path / "s.vcf.gz"), CALLS, "chrT", 25, "s", support=SUPPORT)
    assert ".gz" in str(e.value) and not (tmp_path / "s.vcf.gz").exists()
    bad = dict(CALLS, alt_off=np.array([0, 3, 3, 8, 9], np.int64))
    with pytest.raises(HostError) as e:
        write_vcf(str(tmp_path / "bad.vcf"), bad, "chrT", 25, "s", support=SUPPORT)
    assert "empty allele" in str(e.value) and not (tmp_path / "bad.vcf").exists()
    with pytest.raises(ValueError):                        # one count per call
        write_vcf(str(tmp_path / "x.vcf"), CALLS, "chrT", 25, "s", support={n: v[:3] for n, v in SUPPORT.items()})


def test_writer_under_the_sanitizers(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "calls_writer_sanitize", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = tmp_path / "selftest.vcf"
    r = subprocess.run([os.path.join(ROOT, "build", "sanitize", "calls_writer_selftest_asan"), str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("calls_writer_selftest: ok ")
    assert out.read_text() == _format(CALLS, "chrT", 25, "sample_1", PH, SUPPORT)   # the program's records are these


def test_support_symbols_are_declared_bound_and_documented():
    from phi_amd import _capi
    from phi_amd import ilp_index as H
    from phi_amd.build import HIP_SOURCES
    hdr = open(os.path.join(ROOT, "include", "phi_amd.h")).read()
    host = open(os.path.join(ROOT, "include", "phi_host.h")).read()
    for name in ("phi_calls_support", "phi_calls_support_stats"):
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _capi.SYMBOLS, name
    for name in ("phi_format_calls_vcf_support", "phi_write_calls_vcf_support"):
        assert re.search(r"\bint " + name + r"\(", host) and name in H.HOST_SYMBOLS, name
    assert "calls_support.hip" in HIP_SOURCES
    # the rule is stated, as this project's own and compared with no other tool's, where the calls' rule is
    for phrase in ("x < A1 and x \\+ k > A0", "THE RULE IS THIS PROJECT'S OWN: it is no other", "has not been compared with any other tool",
                   "CONTINUES ALONG THE WALK IT WAS SKETCHED ON"):
        assert re.search(phrase, re.sub(r"\s*\n \*\s*", " ", hdr)), phrase
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "phi_calls_support" in text and "--calls-support" in text and "not been compared with any other tool" in re.sub(r"\s+", " ", text), doc
    assert "per-call read support" not in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_support_kernels_use_no_scratch(tmp_path):
    """calls_support.hip for gfx950: two kernels, neither spills or touches scratch or declares LDS."""
    from phi_amd.build import HIPCC
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "phi_amd", "csrc", "calls_support.hip")
    out = tmp_path / "calls_support.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), src], stderr=subprocess.DEVNULL)
    seen = {}
    for e in out.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        m = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", e)}
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0 and m["vgpr_count"] <= 64, (name, m)
        seen[name] = m
    assert len(seen) == 2 and sum("support_item_kernel" in n for n in seen) == 1, list(seen)


# ------------------------------------------------------------------ the restatement of the rule on its own

def test_the_chosen_seeds_hold_a_witnessed_deletion_and_a_partly_seen_allele(oracle):
    """What tests/test_gpu_calls_support.py asserts over its seeds, checked here with the reference alone: in every parameter
    set some call has an empty ALT with witnesses, and some call's ALT is seen in part."""
    for pi in range(len(R.PARAMS)):
        n_empty_alt = n_between = 0
        for seed in R.SEEDS:
            g, reads, k, w = R.random_case(pi, seed)
            spec = R.spectrum_of(oracle, reads, k, w)
            lens = [len(s) for s in g.node_seq]
            for q in range(4):
                qb = R.walk_bases(g.paths[q], lens)
                for r in range(4):
                    s = R.walk_support_ref(oracle, g, q, r, k, w, spec)
                    for j, (i, i2, _, _) in enumerate(R.anchors(g.paths[q], g.paths[r])):
                        n_empty_alt += qb[i + 1] == qb[i2] and s["alt_n"][j] > 0
                        n_between += 0 < s["alt_hit"][j] < s["alt_n"][j]
        assert n_empty_alt > 0 and n_between > 0, pi


def test_the_two_restatements_agree_and_a_walk_is_its_own_path(oracle):
    for pi in range(len(R.PARAMS)):
        g, reads, k, w = R.random_case(pi, 3)
        spec = R.spectrum_of(oracle, reads, k, w)
        lens = [len(s) for s in g.node_seq]
        sk = [oracle.sketch(b"".join(g.node_seq[v] for v in p), k, w) for p in g.paths]
        base = [R.walk_bases(p, lens) for p in g.paths]
        for q in range(4):
            for r in range(4):
                a = R.walk_support_ref(oracle, g, q, r, k, w, spec)
                b = R.support_ref_numpy(k, sk[q][0], sk[q][1], base[q], sk[r][0], sk[r][1], base[r], R.anchors(g.paths[q], g.paths[r]), spec)
                c = R.path_support_ref(oracle, g, g.paths[q], [q] * len(g.paths[q]), r, k, w, spec)   # a path that follows one walk
                d = R.path_support_ref_numpy(k, g.paths[q], [q] * len(g.paths[q]), g.paths, np.array(lens), lambda h: sk[h], r, spec)
                assert R.anchors_numpy(g.paths[q], g.paths[r], len(lens)).tolist() == [list(t) for t in R.anchors(g.paths[q], g.paths[r])]
                for n in a:
                    assert np.array_equal(a[n], b[n]) and np.array_equal(a[n], c[n]) and np.array_equal(a[n], d[n]), (pi, q, r, n)
