"""CPU test: the host side of the k-mer keys (phi_amd/csrc/phi_dev.h: plain code, no HIP) in a stand-alone program,
phi_amd/csrc/host/kmer_keys_selftest.cpp, built plain and with AddressSanitizer + UndefinedBehaviorSanitizer
(`make -C phi_amd/csrc/host kmer_keys_sanitize`).

The program checks that phi_kmer_unmix inverts phi_kmer_mix, both ways, for 10^6 random values and at 0, 2^62 - 1 and ~0;
that the value mapping to the table sentinel is no k-mer (>= 2^62); that k-mers differing only in their first or only in their
last bases spread over the home buckets as random keys do; and the flush's rule on hand-made (hash, k-mer) pairs: a plain
entry, the same k-mer twice, and every class of MurmurHash3 collision -- novel and novel in consecutive entries, novel and
walk, both, the sentinel.  Here: both builds exit 0, the sanitizers report nothing, and the two print the same lines."""
import os
import subprocess

import pytest

from conftest import ROOT

SAN = os.path.join(ROOT, "build", "sanitize")
BUILDS = ("plain", "asan")
OK = ("inverse_random", "inverse_edges", "sentinel_preimage", "multiplier_inverse", "low_bits_mixed",
      "rule_plain_first", "rule_plain_prev_differs", "rule_same_kmer_twice", "rule_novel_novel", "rule_novel_novel_no_prev",
      "rule_novel_walk", "rule_both", "rule_sentinel", "rule_sentinel_first", "error_bits", "hash_of_value")


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "kmer_keys_sanitize", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return {b: subprocess.run([os.path.join(SAN, "kmer_keys_selftest_" + b)], capture_output=True, text=True, env=env, timeout=120) for b in BUILDS}


@pytest.mark.parametrize("build", BUILDS)
def test_mix_inverse_and_flush_rule(outputs, build):
    r = outputs[build]
    assert r.returncode == 0, (build, r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "FAILED" not in r.stdout
    lines = dict(l.split(" ", 1) for l in r.stdout.splitlines())
    for name in OK:
        assert lines[name].startswith("ok "), (name, lines[name])
    assert lines["inverse_random"] == "ok random=1000000 bad=0"
    pre = int(lines["sentinel_preimage"].split("preimage=")[1], 16)
    assert pre >= 1 << 62


def test_both_builds_print_the_same(outputs):
    assert outputs["plain"].stdout == outputs["asan"].stdout
    assert len(outputs["plain"].stdout.splitlines()) == len(OK)
