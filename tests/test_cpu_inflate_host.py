"""CPU test: the rules of the device inflater that need no GPU (phi_amd/csrc/inflate_host.h: plain host code, no HIP) and the
gzip header parser its decode kernel calls, in a stand-alone program, phi_amd/csrc/host/inflate_host_selftest.cpp, built plain
and with AddressSanitizer + UndefinedBehaviorSanitizer (`make -C phi_amd/csrc/host inflate_host_sanitize`).

The program checks the header against serial restatements written from the rules' sentences: the chunk plan (sizes around a
chunk, the 64-byte floor, the environment's default, 2^30 chunks refused), the symbol capacity from the last ISIZE (a stream
shorter than a member, ratios below 4, between, above 1100), the job list, the chain of decoders (one job, every chunk
confirmed, no start but chunk 0, a false start dropped, an error at the first, a middle and the last chain job with its text
and byte position, results that cannot be followed refused instead of indexed, 2000 random instances), the second run (none,
one, all, a dropped job's overflow ignored, offsets and total, a second result that differs refused), the layout (member ends
on a piece boundary, inside a piece, across three pieces, empty members by record index, dropped jobs' records ignored, ends
that do not cover the output refused, 2000 random layouts), slabs and CRC segments around their sizes, the members' CRC32 and
ISIZE check on real bytes and on 2^32 + 7 zeros through the shift alone, the 64-bit CRC32 shift up to 2^40 bytes, and the gzip
header's flags, truncations and bad values, each buffer in an allocation of exactly its size.
Here: both builds exit 0, the sanitizers report nothing, and the two print the same lines."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SAN = os.path.join(ROOT, "build", "sanitize")
BUILDS = ("plain", "asan")
OK = ("chunk_n_around_C", "chunk_floor_64", "chunk_default_no_env", "chunk_default_env", "chunk_2pow30_refused",
      "cap_short_stream", "cap_empty_stream", "cap_ratio_below_4", "cap_ratio_between", "cap_ratio_above_1100", "cap_18_bytes_top_isize",
      "cap_ratio_exactly_1100", "jobs_from_starts", "member_capacity",
      "chain_single_job_end", "chain_every_chunk_confirmed", "chain_no_start_but_chunk_0", "chain_false_start_dropped",
      "chain_false_start_in_error_dropped", "chain_error_at_first", "chain_error_in_middle", "chain_error_at_last", "chain_error_code",
      "chain_error_header", "chain_error_unknown", "chain_malformed_stop_on_itself", "chain_malformed_stop_before_itself",
      "chain_malformed_stop_on_nch", "chain_malformed_stop_far_beyond", "chain_malformed_stop_negative",
      "chain_malformed_stop_on_chunk_without_job", "chain_random",
      "again_none", "again_one", "again_all", "again_dropped_job_ignored", "again_offsets_and_total", "again_second_run_agrees",
      "again_second_differs_in_length", "again_second_differs_in_status", "again_second_overflows_again",
      "layout_one_member_one_piece", "layout_end_on_piece_boundary", "layout_members_inside_one_piece", "layout_member_spans_three_pieces",
      "layout_empty_members_by_index", "layout_dropped_jobs_records_ignored", "layout_last_end_short_refused", "layout_last_end_beyond_refused",
      "layout_no_ends_refused", "layout_record_of_no_job_refused", "layout_random",
      "slabs_by_piece_length", "slabs_no_pieces", "segments_by_member_length", "segments_two_members_back_to_back", "segments_empty_members_between",
      "mcheck_short_members", "mcheck_3x4096_plus_5", "mcheck_wrong_crc", "mcheck_wrong_segment", "mcheck_wrong_isize", "mcheck_2pow32_plus_7_zeros",
      "crc_shift_64", "crc_combine_and_bitwise",
      "gzhdr_plain", "gzhdr_fname", "gzhdr_fextra", "gzhdr_fcomment", "gzhdr_fhcrc", "gzhdr_every_field", "gzhdr_bad_method", "gzhdr_bad_magic",
      "gzhdr_fname_unterminated", "gzhdr_fextra_cut", "gzhdr_bad_fhcrc", "gzhdr_reserved_flag", "gzhdr_two_bytes", "gzhdr_no_bytes",
      "gzhdr_fextra_65535", "gzhdr_fhcrc_covers_the_name")


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "inflate_host_sanitize", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return {b: subprocess.run([os.path.join(SAN, "inflate_host_selftest_" + b)], capture_output=True, text=True, env=env, timeout=300) for b in BUILDS}


@pytest.mark.parametrize("build", BUILDS)
def test_host_rules_equal_their_restatements(outputs, build):
    r = outputs[build]
    assert r.returncode == 0, (build, r.stdout[-3000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "FAILED" not in r.stdout
    lines = dict(l.split(" ", 1) for l in r.stdout.splitlines())
    for name in OK:
        assert lines[name].startswith("ok "), (name, lines[name])
    assert lines["cases_failed"] == "0"
    assert lines["chunk_n_around_C"].startswith("ok 0:4096,0 1:4096,1 4095:4096,1 4096:4096,1 4097:4096,2 ")
    assert lines["chunk_floor_64"].startswith("ok 63:64,1 64:64,1 65:64,2 ")
    assert " %d:64,%d %d:refused " % ((1 << 36) - 64, (1 << 30) - 1, (1 << 36) - 63) in lines["chunk_2pow30_refused"]
    assert lines["cap_ratio_between"] == "ok n=1000 isize=10000 cap=%d" % (4096 * 10 * 5 // 4 + 4096)
    assert lines["cap_ratio_above_1100"].endswith(" cap=%d" % (4096 * 1375 + 4096)) and lines["cap_short_stream"].endswith(" cap=%d" % (4096 * 5 + 4096))
    assert lines["chain_false_start_dropped"].startswith("ok rc=0 chain=0,2,3, ")
    assert lines["chain_error_in_middle"] == "ok rc=-1 chain=0,1,2, gzip stream corrupt: distance before the start of the member (near compressed byte 70000)"
    assert lines["chain_error_at_last"].endswith("gzip stream corrupt: truncated stream (near compressed byte %d)" % ((1 << 33) + 5))
    for name in OK:
        if name.startswith("chain_malformed_"):
            assert lines[name].startswith("ok rc=-3 "), (name, lines[name])                 # PHI_ERR_DEVICE, nothing indexed
    assert re.match(r"ok instances=2000 differ=0 ", lines["chain_random"])
    assert lines["again_all"] == "ok 0@0 1@601 2@1302 total=1303"
    assert lines["again_dropped_job_ignored"] == "ok 0@0 3@601 total=1402"
    assert lines["again_second_overflows_again"].endswith("phi_inflate: decoder of chunk 6 differs on its second run (internal error)")
    assert lines["layout_end_on_piece_boundary"] == "ok lo=0,100, ends=100#0,200#1, total=200"
    assert lines["layout_member_spans_three_pieces"] == "ok lo=0,50,50, ends=50#1,300#0, total=300"
    assert lines["layout_empty_members_by_index"] == "ok lo=0,100, ends=60#3,100#1,100#2,100#4,140#0, total=140"
    assert re.match(r"ok layouts=2000 differ=0 ", lines["layout_random"])
    assert lines["slabs_by_piece_length"].startswith("ok 0:0 1:0 32768:0 32769:1 98304:1 98305:2 ")
    assert lines["segments_by_member_length"].startswith("ok 0:0 1:1 4095:1 4096:1 4097:2 8192:2 ")
    assert re.match(r"ok gzip stream corrupt: CRC32 mismatch in member 1 \([0-9a-f]{8}, trailer [0-9a-f]{8}\)$", lines["mcheck_wrong_crc"])
    assert lines["mcheck_wrong_isize"] == "ok gzip stream corrupt: ISIZE mismatch in member 2 (9000, trailer 9001)"
    assert lines["crc_combine_and_bitwise"] == "ok differ=0 crc(123456789)=cbf43926"
    assert lines["gzhdr_every_field"] == "ok header=718 data_at=721 cuts_not_truncated=0"


def test_both_builds_print_the_same(outputs):
    assert outputs["plain"].stdout == outputs["asan"].stdout
    assert len(outputs["plain"].stdout.splitlines()) == len(OK) + 1


def test_the_library_calls_this_header():
    """inflate.hip and deflate.hip hold no copy of what the headers hold: records, CRC32 arithmetic, a run's scaffolding"""
    csrc = os.path.join(ROOT, "phi_amd", "csrc")
    inflate, deflate = (open(os.path.join(csrc, f)).read() for f in ("inflate.hip", "deflate.hip"))
    assert '#include "inflate_host.h"' in inflate and '#include "dev_run.h"' in inflate and '#include "dev_run.h"' in deflate
    for src in (inflate, deflate):
        assert not re.search(r"struct Dev\b|define DCHK|define DALLOC|\bint fail\(|EDB88320|CrcOps", src)
    assert not re.search(r"struct Inf(Job|Result|Member|Piece|Slab|Seg)\b|INF_E_CODE =|define INF_(SEG|WIN)", inflate)
    for fn in ("inf_chunk_plan", "inf_sym_capacity", "inf_job_list", "inf_chain", "inf_again_plan", "inf_again_check", "inf_layout", "inf_slabs",
               "inf_segments", "inf_member_check", "inf_gz_header", "inf_crc_combine"):
        assert re.search(r"\b" + fn + r"\(", inflate), fn
    from phi_amd.build import HIP_HEADERS
    assert {"inflate_host.h", "crc32_shift.h", "dev_run.h"} <= set(HIP_HEADERS)
