"""CPU: the VCF writer of the calls (phi_write_calls_vcf of libphi_host) on hand-made arrays against the expected text byte for
byte, the consensus of the rule (phi_amd.calls.apply) on the same arrays, and the restatements the GPU tests compare with."""
import os
import re
import subprocess

import numpy as np
import pytest

from calls_ref import calls_ref, calls_ref_numpy
from conftest import ROOT
from graphgen import random_graph, walk_sequence


@pytest.fixture(scope="module")
def built():
    from phi_amd import build as B
    B.build_host()
    return True


#        0         1         2
#        0123456789012345678901234
REF = b"ACGTACGTTTGACCAgtcaTTGACA"
# a substitution, an insertion behind the base at 9 (padded), a REF = ALT call, a deletion (padded) with lower-case bytes kept
CALLS = dict(pos=np.array([2, 9, 12, 15], np.int64), ref_off=np.array([0, 2, 3, 5, 9], np.int64), alt_off=np.array([0, 3, 6, 8, 9], np.int64),
             ref_bytes=b"GT" + b"T" + b"CC" + b"gtca", alt_bytes=b"ccc" + b"TAA" + b"CC" + b"g")
EXPECTED = ("##fileformat=VCFv4.2\n##source=phi_amd\n##contig=<ID=chrT,length=25>\n"
            "##INFO=<ID=PH,Number=1,Type=String,Description=\"Panel haplotype the inferred path follows through the call\">\n"
            "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample_1\n"
            "chrT\t3\t.\tGT\tccc\t.\tPASS\tPH=hapA.1\tGT\t1\n"
            "chrT\t10\t.\tT\tTAA\t.\tPASS\tPH=hapA.1\tGT\t1\n"
            "chrT\t16\t.\tgtca\tg\t.\tPASS\tPH=hapC.2\tGT\t1\n")


def test_writer_byte_for_byte(built, tmp_path):
    from phi_amd.calls import read_vcf, write_vcf
    p = tmp_path / "calls.vcf"
    assert write_vcf(str(p), CALLS, "chrT", 25, "sample_1", ph=["hapA.1", "hapA.1", "hapB.1", "hapC.2"]) == (3, 1)
    assert p.read_text() == EXPECTED
    header, sample, calls, infos = read_vcf(str(p))
    assert sample == "sample_1" and infos == ["PH=hapA.1", "PH=hapA.1", "PH=hapC.2"] and calls["pos"].tolist() == [2, 9, 15]
    # without tags INFO is "."; no call at all is a header alone
    assert write_vcf(str(p), CALLS, "chrT", 25, "sample_1") == (3, 1)
    assert p.read_text() == EXPECTED.replace("PH=hapA.1", ".").replace("PH=hapC.2", ".")
    empty = dict(pos=np.zeros(0, np.int64), ref_off=np.zeros(1, np.int64), alt_off=np.zeros(1, np.int64), ref_bytes=b"", alt_bytes=b"")
    assert write_vcf(str(p), empty, "chrT", 25, "sample_1", ph=[]) == (0, 0)
    assert p.read_text() == "".join(ln + "\n" for ln in EXPECTED.split("\n")[:6])


def test_writer_refuses_gz_and_bad_arrays(built, tmp_path):
    from phi_amd.calls import write_vcf
    from phi_amd.ilp_index import HostError
    with pytest.raises(HostError) as e:
        write_vcf(str(tmp_path / "calls.vcf.gz"), CALLS, "chrT", 25, "s")
    assert ".gz" in str(e.value) and "deflate" in str(e.value) and not (tmp_path / "calls.vcf.gz").exists()
    bad = dict(CALLS, alt_off=np.array([0, 3, 3, 8, 9], np.int64))                  # an empty ALT: the rule never makes one
    with pytest.raises(HostError) as e:
        write_vcf(str(tmp_path / "bad.vcf"), bad, "chrT", 25, "s")
    assert "empty allele" in str(e.value) and not (tmp_path / "bad.vcf").exists()
    with pytest.raises(HostError):
        write_vcf(str(tmp_path / "no_such_dir" / "x.vcf"), CALLS, "chrT", 25, "s")
    with pytest.raises(ValueError):
        write_vcf(str(tmp_path / "x.vcf"), CALLS, "chrT", 25, "s", ph=["one"])


def test_calls_kernels_use_no_scratch_and_no_lds(tmp_path):
    """calls.hip for gfx950: seven kernels, none spills or touches scratch, none declares LDS, every one fits eight waves
    per SIMD -- they hide their gathers with resident waves, not with registers."""
    from phi_amd.build import HIP_SOURCES, HIPCC
    assert "calls.hip" in HIP_SOURCES
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "phi_amd", "csrc", "calls.hip")
    out = tmp_path / "calls.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), src], stderr=subprocess.DEVNULL)
    seen = {}
    for e in out.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        m = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", e)}
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0 and m["vgpr_count"] <= 64, (name, m)
        seen[name] = m
    assert len(seen) == 7 and sum("calls_fill_kernel" in n for n in seen) == 1, list(seen)


def test_calls_symbols_are_declared_bound_and_exported():
    from phi_amd import _capi
    from phi_amd import ilp_index as H
    hdr = open(os.path.join(ROOT, "include", "phi_amd.h")).read()
    for name in ("phi_calls_path", "phi_calls_walk", "phi_calls_stats"):
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _capi.SYMBOLS, name
    assert "phi_write_calls_vcf" in H.HOST_SYMBOLS and re.search(r"\bint phi_write_calls_vcf\(", open(os.path.join(ROOT, "include", "phi_host.h")).read())
    # no reference counterpart, the comparison it serves, and that the rule is not vg deconstruct's
    for phrase in ("No reference counterpart", r"data/run_PG\.py:54-60", "vg deconstruct"):
        assert re.search(phrase, hdr), phrase
    for doc in ("README.md", "DESIGN.md"):
        assert "vg deconstruct" in open(os.path.join(ROOT, doc)).read(), doc


def test_apply_on_the_same_arrays():
    from phi_amd.calls import apply
    want = b"AC" + b"ccc" + b"ACGTT" + b"TAA" + b"GA" + b"CC" + b"A" + b"g" + b"TTGACA"
    assert apply(REF, dict(CALLS, ref_span=(0, 25))) == want
    assert apply(REF, CALLS, span=(1, 20)) == want[1:-5]
    with pytest.raises(ValueError):                        # REF is not what the reference holds
        apply(REF.replace(b"gtca", b"GTCA"), CALLS, span=(0, 25))
    with pytest.raises(ValueError):                        # a call outside the span
        apply(REF, CALLS, span=(3, 25))
    with pytest.raises(ValueError):                        # overlapping calls
        apply(REF, dict(CALLS, pos=np.array([2, 3, 12, 15], np.int64)), span=(0, 25))


@pytest.mark.parametrize("seed", range(12))
def test_the_two_restatements_agree_and_apply_gives_the_query(oracle, seed):
    from phi_amd.calls import apply
    rng = np.random.default_rng(seed)
    g = random_graph(rng, n_sites=seed, n_walks=4, p_del=0.4)
    A = g.arrays()
    for q in range(4):
        for r in range(4):
            a = calls_ref(g.paths[q], g.paths[r], g.node_seq)
            b = calls_ref_numpy(g.paths[q], g.paths[r], A["seq_off"], bytes(A["seq_concat"]))
            assert a.keys() == b.keys()
            for k in a:
                assert np.array_equal(a[k], b[k]), k
            qs = walk_sequence(g, q)
            assert apply(walk_sequence(g, r), a) == qs[a["query_span"][0]:a["query_span"][1]]
            assert np.all(np.diff(a["pos"]) > 0) and np.all(a["pos"][1:] >= (a["pos"] + np.diff(a["ref_off"]))[:-1])
