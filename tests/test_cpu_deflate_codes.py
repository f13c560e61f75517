"""CPU test: the plain code of the DEFLATE writer (phi_amd/csrc/deflate_codes.h: `__host__ __device__` functions the
compressor's kernel calls from single lanes) in a stand-alone program, phi_amd/csrc/host/deflate_codes_selftest.cpp, built
plain and with AddressSanitizer + UndefinedBehaviorSanitizer (`make -C phi_amd/csrc/host deflate_codes_sanitize`).

The program builds a length-limited code for every histogram with 0, 1 and 2 used symbols of the three alphabets (286 and 30
symbols at 15 bits, 19 at 7), flat histograms of 286 and 30 symbols, Fibonacci counts over 22 symbols (sum 46 367: Huffman's
code is 21 deep) at 15 bits and over 11 of the 19 code-length symbols at 7 bits, and 2 000 seeded random histograms.  For each:
no length above the limit, a Kraft sum of exactly 1 (or the degenerate forms: no code, one code of length 1), no rarer symbol
with the shorter code, a cost not above the fixed code's where one is defined, the run-length coding of the lengths expanded
back to the lengths, prefix-free canonical codes.  It also checks the symbols of every copy length and distance against
RFC 1951 3.2.5 and the CRC32 shift against the register run over zero bytes.
Here: both builds exit 0, the sanitizers report nothing, and the two print the same lines."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SAN = os.path.join(ROOT, "build", "sanitize")
BUILDS = ("plain", "asan")
OK = ("few_symbols", "flat_286", "flat_30", "fibonacci_22_limit_15", "fibonacci_11_limit_7", "random_2000", "copy_symbols", "crc_shift")


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "deflate_codes_sanitize", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return {b: subprocess.run([os.path.join(SAN, "deflate_codes_selftest_" + b)], capture_output=True, text=True, env=env, timeout=300) for b in BUILDS}


def _fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}


@pytest.mark.parametrize("build", BUILDS)
def test_codes_of_every_histogram(outputs, build):
    r = outputs[build]
    assert r.returncode == 0, (build, r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "FAILED" not in r.stdout
    lines = dict(l.split(" ", 1) for l in r.stdout.splitlines())
    for name in OK:
        assert lines[name].startswith("ok "), (name, lines[name])
    for name in OK[:6]:
        f = _fields(lines[name])
        assert all(f[k] == 0 for k in ("limit", "kraft", "order", "cost", "rle", "prefix")), (name, f)
    # 3 alphabets: the empty histogram, every single symbol at two counts, every pair at three
    assert _fields(lines["few_symbols"])["histograms"] == sum(1 + 2 * n + 3 * n * (n - 1) // 2 for n in (286, 30, 19))
    fib = _fields(lines["fibonacci_22_limit_15"])
    assert fib["depth"] == 21 and fib["longest"] == 15
    fib = _fields(lines["fibonacci_11_limit_7"])
    assert fib["depth"] == 10 and fib["longest"] == 7
    rnd = _fields(lines["random_2000"])
    assert rnd["histograms"] == 2000 and rnd["depth"] > 15 and rnd["longest"] <= 15     # the limit had work to do among them
    assert _fields(lines["copy_symbols"]) == {"lengths": 256, "distances": 32768, "bad": 0}


def test_both_builds_print_the_same(outputs):
    assert outputs["plain"].stdout == outputs["asan"].stdout
    assert len(outputs["plain"].stdout.splitlines()) == len(OK)


def test_the_kernel_calls_these_functions():
    """deflate.hip holds no code construction of its own: it includes the header and calls its functions"""
    src = open(os.path.join(ROOT, "phi_amd", "csrc", "deflate.hip")).read()
    assert '#include "deflate_codes.h"' in src
    for fn in ("dfl_build_lengths", "dfl_rle_lengths", "dfl_canonical_codes", "dfl_length_symbol", "dfl_dist_symbol", "dfl_crc_shift"):
        assert re.search(r"\b" + fn + r"\(", src), fn
    from phi_amd.build import HIP_HEADERS, HIP_SOURCES
    assert "deflate.hip" in HIP_SOURCES and "deflate_codes.h" in HIP_HEADERS
