"""CPU test: the rules of phi_solve that need no GPU (phi_amd/csrc/solve_host.h: plain host code, no HIP) in a stand-alone
program, phi_amd/csrc/host/solve_host_selftest.cpp, built plain, with AddressSanitizer + UndefinedBehaviorSanitizer and with
ThreadSanitizer (`make -C phi_amd/csrc/host solve_host_sanitize`).

The program checks the header at PHI_HOST_THREADS 1 and 8 against serial restatements written from the definitions and
against brute force: the clusters of mutually exclusive anchors (one anchor, two on one walk, two apart, three that overlap
pairwise, a chain a-b-c, 200 random sets), the max-plus chain over up to 4 blocks of up to 3 walks against every walk
sequence, and its comparison with the second pass (a differing key, a key against "no run", two "no run" values), the host
anchor arrays (none, one, all spanning an edge, single-vertex anchors mixed in, 3 * 65536 + 17 anchors over 5 walks) with
their two refusals, the score bound, the block placement (one block, a closed stretch longer than the small ring, with and
without the small blocks ruled out, 300 random chains), the minimiser -> anchors map and the repeat set against O(n^2)
recounts, and the set tightening and branch choice of the exact search.  Here: every build exits 0, no sanitizer reports
anything, and the three print the same lines."""
import os
import subprocess

import pytest

from conftest import ROOT

SAN = os.path.join(ROOT, "build", "sanitize")
BUILDS = ("plain", "asan", "tsan")
OK = ("clusters_one", "clusters_same_walk", "clusters_disjoint", "clusters_three_overlap", "clusters_chain", "clusters_random",
      "chain_random", "chain_key_differs", "chain_key_against_no_run", "chain_both_no_run",
      "anchors_none", "anchors_one", "anchors_all_span", "anchors_mixed", "anchors_three_chunks", "score_bound_random",
      "blocks_below_target", "blocks_long_stretch", "blocks_long_stretch_no_small", "blocks_open", "blocks_open_no_small", "blocks_random",
      "csr_repeats_random",
      "tighten_nothing", "tighten_d_only", "tighten_z_only", "tighten_both", "tighten_revisit",
      "branch_lowest_first_anchor", "branch_tie", "branch_from_z", "branch_none")


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "solve_host_sanitize", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="exitcode=66:halt_on_error=1")
    return {b: subprocess.run([os.path.join(SAN, "solve_host_selftest_" + b)], capture_output=True, text=True, env=env, timeout=600) for b in BUILDS}


@pytest.mark.parametrize("build", BUILDS)
def test_host_rules_equal_their_restatements(outputs, build):
    r = outputs[build]
    assert r.returncode == 0, (build, r.stdout[-3000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "FAILED" not in r.stdout
    lines = dict(l.split(" ", 1) for l in r.stdout.splitlines())
    for name in OK:
        assert lines[name].startswith("ok "), (name, lines[name])
    assert lines["clusters_chain"].startswith("ok anchors=3 clusters=3 ")
    assert lines["clusters_three_overlap"].startswith("ok anchors=3 clusters=1 ")
    assert lines["chain_key_differs"] == "ok block 0 walk 1 got 4 want 5"
    assert lines["chain_both_no_run"] == "ok agree"
    assert " same_as_kept " in lines["anchors_all_span"] and " own_list " in lines["anchors_mixed"]
    assert "kept=%d " % (3 * 65536 + 17) in lines["anchors_three_chunks"]
    assert lines["anchors_span_rcap"] == "refused -3 an anchor spans 32 edges (at most 31 are supported)"
    assert lines["anchors_span_rcap_long_k"] == "refused -5 an anchor spans 32 edges (at most 31 are supported)"
    assert lines["anchors_unsorted_across_chunks"] == "refused -3 dp anchors not sorted by last entry (internal error)"
    assert " ring=256 blocks=1 " in lines["blocks_below_target"]
    assert " ring=1024 " in lines["blocks_long_stretch"] and " ring=1024 " in lines["blocks_long_stretch_no_small"]
    assert lines["csr_id_out_of_range"] == "refused id 3 of 3"
    assert lines["tighten_revisit"] == "ok stopped S={1,2} seen=1"
    assert lines["branch_tie"] == "ok branch on 1"
    assert lines["branch_none"] == "ok no branch"


def test_the_three_builds_print_the_same(outputs):
    assert outputs["plain"].stdout == outputs["asan"].stdout == outputs["tsan"].stdout
    assert len(outputs["plain"].stdout.splitlines()) >= len(OK) + 4
