"""CPU test: the DP step stream and the topology validation of phi_set_graph (phi_amd/csrc/dp_steps.h: plain host code on
all host threads, no HIP) in a stand-alone program, phi_amd/csrc/host/dp_steps_selftest.cpp, built plain, with
AddressSanitizer + UndefinedBehaviorSanitizer and with ThreadSanitizer (`make -C phi_amd/csrc/host dp_steps_sanitize`).

The program checks the header at PHI_HOST_THREADS 1 and 8 against a serial implementation of its own, written from the
definitions of the step records: one vertex, two vertices, one bi-allelic site (a pair), walks with interior ends, 4 live
in-edges (the first spill into in_packed), 255 (accepted) and 256 (refused), a rank array that is no permutation, a
backward edge, 300 random bubble chains of up to 40 vertices with extra forward edges, and one graph of 3 * 65536 + 17
vertices, where more than one chunk of vertices exists and the threaded paths run.  Here: every build exits 0, no sanitizer
reports anything, and the three print the same lines.

Not covered, as before: the refusal of an edge that spans 2^23 topological steps and more needs a graph of more than 8.4 M
vertices."""
import os
import subprocess

import pytest

from conftest import ROOT

SAN = os.path.join(ROOT, "build", "sanitize")
BUILDS = ("plain", "asan", "tsan")


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "dp_steps_sanitize", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="exitcode=66:halt_on_error=1")
    return {b: subprocess.run([os.path.join(SAN, "dp_steps_selftest_" + b)], capture_output=True, text=True, env=env, timeout=600) for b in BUILDS}


@pytest.mark.parametrize("build", BUILDS)
def test_step_stream_equals_the_serial_definition(outputs, build):
    r = outputs[build]
    assert r.returncode == 0, (build, r.stdout[-3000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "FAILED" not in r.stdout
    lines = dict(l.split(" ", 1) for l in r.stdout.splitlines())
    for name in ("one_vertex", "two_vertices", "one_site", "interior_ends", "four_in_edges", "255_in_edges", "random", "three_chunks"):
        assert lines[name].startswith("ok "), (name, lines[name])
    assert lines["256_in_edges"] == "refused -5 vertex 256 has more than 255 in-edges"
    assert lines["not_a_permutation"] == "refused -1 topo_rank is not a permutation (vertex 1): is the graph cyclic?"
    assert lines["backward_edge"] == "refused -1 edge 0->1 goes backwards in topo_rank: graph must be acyclic"
    assert "vertices=%d " % (3 * 65536 + 17) in lines["three_chunks"]


def test_the_three_builds_print_the_same(outputs):
    assert outputs["plain"].stdout == outputs["asan"].stdout == outputs["tsan"].stdout
    assert len(outputs["plain"].stdout.splitlines()) >= 13
