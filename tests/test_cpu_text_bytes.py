"""CPU test: the plain code of the text kernels' byte idioms (phi_amd/csrc/text_bytes.h: no HIP) in a stand-alone program,
phi_amd/csrc/host/text_bytes_selftest.cpp, built plain and with AddressSanitizer + UndefinedBehaviorSanitizer
(`make -C phi_amd/csrc/host text_bytes_sanitize`).

The program checks every function against byte-at-a-time code: the equality masks for every character over words whose bytes
are the character, its two neighbours, the character with the other high bit, 0x00, 0x7f, 0x80 and 0xff in every combination
(the borrow and high-bit cases), and over 16 bytes; the valid mask of the lanes at 0, 16 and 32 against every window
lo <= hi of [0, 48]; sixteen bytes at every shift of 32 all-distinct and random bytes; the two bisections for n = 1..70 over
strictly and non-strictly ascending lists, every x from a[0] to a[n - 1] + 1, with int and 64-bit indices, and their key
forms over the low half of a 64-bit element (reads_text.hip) and the first of two at a stride (vcf_region.hip).  Here: both
builds exit 0, the sanitizers report nothing, and the two print the same lines."""
import os
import subprocess

import pytest

from conftest import ROOT

SAN = os.path.join(ROOT, "build", "sanitize")
BUILDS = ("plain", "asan")
OK = ("eq4_neighbours", "eq16", "valid16", "shift16", "bisection", "bisection_key")


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "text_bytes_sanitize", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return {b: subprocess.run([os.path.join(SAN, "text_bytes_selftest_" + b)], capture_output=True, text=True, env=env, timeout=120) for b in BUILDS}


@pytest.mark.parametrize("build", BUILDS)
def test_every_function_against_bytewise_code(outputs, build):
    r = outputs[build]
    assert r.returncode == 0, (build, r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "FAILED" not in r.stdout
    lines = dict(l.split(" ", 1) for l in r.stdout.splitlines())
    for name in OK:
        assert lines[name].startswith("ok "), (name, lines[name])
        assert lines[name].endswith(" bad=0"), (name, lines[name])
    assert lines["eq4_neighbours"] == "ok cases=%d bad=0" % (256 * 8 ** 4)
    assert lines["valid16"] == "ok cases=%d bad=0" % (3 * 49 * 50 // 2 + 2)
    assert lines["shift16"] == "ok cases=%d bad=0" % (64 * 17)


def test_both_builds_print_the_same(outputs):
    assert outputs["plain"].stdout == outputs["asan"].stdout
    assert len(outputs["plain"].stdout.splitlines()) == len(OK)
