"""CPU test: the rules of the read path that need no GPU (phi_amd/csrc/reads_host.h: plain host code, no HIP) in a stand-alone
program, phi_amd/csrc/host/reads_host_selftest.cpp, built plain, with AddressSanitizer + UndefinedBehaviorSanitizer and with
ThreadSanitizer (`make -C phi_amd/csrc/host reads_host_sanitize`).

The program checks the header at PHI_HOST_THREADS 1 and 8 against serial restatements written from the rules' sentences: the
plan of a batch's part of the novel-hash log (an empty log, a batch that fits exactly, one entry over, the count buffer as
the limit, over budget with nothing logged and with chunks logged, doubling capped by the budget, the replay of the last
batch, 2^40 bases in 128-bit arithmetic, 2000 random states), the overflow list's bound (w of 1, 2, 3, 25, 255), its capacity
around the bound with the 65536 floor and what a replay keeps and grows to, the set's capacity and the reuse of another
generation's set, the offsets' check (sizes around 2^20, the one bad read at the first read, the last, and on either side
of a seam between two threads' pieces, empty reads, the first of several offenders against a serial scan), the one-length
decisions of the host and the device route, the fixed-point launch fields, the pool's best fit, and the text stream's sizes
and host carry.  Here: every build exits 0, no sanitizer reports anything, and the three print the same lines."""
import os
import subprocess

import pytest

from conftest import ROOT

SAN = os.path.join(ROOT, "build", "sanitize")
BUILDS = ("plain", "asan", "tsan")
OK = ("log_empty", "log_fits_exactly", "log_one_entry_over", "log_counts_are_the_limit", "log_over_budget_nothing_logged",
      "log_over_budget_flushes_first", "log_flushed_batch_fits_what_is_there", "log_doubling_capped_by_budget", "log_replay_same_plan",
      "log_2pow40_bases", "log_random",
      "ov_bound_by_w", "ov_capacity_around_the_bound", "ov_capacity_floor", "ov_replay_one_over", "ov_replay_ten_times",
      "set_capacity", "set_reuse",
      "offsets_monotone_sizes", "offsets_one_bad_read", "offsets_first_of_several", "offsets_empty_reads", "one_length_31_and_32",
      "one_length_product_agrees_reads_do_not", "device_one_length",
      "q32_inverse_length", "q32_reads_per_base",
      "pool_exact_fit", "pool_upper_end_taken", "pool_one_beyond_not_taken", "pool_smaller_of_two", "pool_none", "pool_random",
      "text_sizes_carry_from_env", "text_sizes_default_carry", "text_carry_update")


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "reads_host_sanitize", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="exitcode=66:halt_on_error=1")
    return {b: subprocess.run([os.path.join(SAN, "reads_host_selftest_" + b)], capture_output=True, text=True, env=env, timeout=600) for b in BUILDS}


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
    assert lines["log_empty"] == "ok base=0 flush=0 log=5120 cnt=84 keep=0,0"
    assert lines["log_fits_exactly"] == "ok base=30 flush=0 log=0 cnt=0 keep=0,0"
    assert lines["log_over_budget_flushes_first"] == "ok base=7 flush=1 log=51200 cnt=264 keep=0,0"
    assert lines["log_doubling_capped_by_budget"] == "ok base=100 flush=0 log=76800 cnt=364 keep=51200,200"
    assert " log=%d " % (1 << 44) in lines["log_2pow40_bases"] and "keep=%d,%d" % (1 << 43, 1 << 32) in lines["log_2pow40_bases"]
    assert lines["log_random"].startswith("ok states=2000 differ=0 ")
    assert lines["ov_bound_by_w"].startswith("ok w=1:5200016 w=2:5200016 w=3:3900016 ")
    assert lines["ov_capacity_around_the_bound"] == "ok below=100000 equal=100000 above=200000 far=300007"
    assert lines["ov_replay_one_over"] == "ok valid=50 cap=200"
    assert lines["ov_replay_ten_times"].startswith("ok valid=50 cap=1000 ")
    assert lines["set_capacity"].startswith("ok 0:65536 32768:65536 32769:131072 ")
    assert lines["set_reuse"] == "ok need=1 four=1 four_and_one=0 half=0 none=0"
    assert " 1048577@1048575 1048577@1048576 " in lines["offsets_one_bad_read"]
    assert lines["one_length_31_and_32"].startswith("ok 31:0 32:1 ")
    assert lines["device_one_length"] == "ok 1:offsets 31:offsets 32:computed 150:computed 2147483647:computed 2147483648:offsets "
    assert lines["q32_inverse_length"] == "ok 32:134217728 150:28633115 2147483647:2 "
    assert " 1/2:2147483648 1/1:2147483648 5/3:2147483648 " in lines["q32_reads_per_base"]
    assert lines["pool_one_beyond_not_taken"] == "ok index=-1" and lines["pool_smaller_of_two"] == "ok index=1"
    assert lines["text_sizes_carry_from_env"].startswith("ok 64:64 70:64 ")
    assert lines["text_carry_update"] == "ok 0:0 1:1 19:19 20:20 21:21 56:56 57:57 "


def test_the_three_builds_print_the_same(outputs):
    assert outputs["plain"].stdout == outputs["asan"].stdout == outputs["tsan"].stdout
    assert len(outputs["plain"].stdout.splitlines()) >= len(OK) + 1
