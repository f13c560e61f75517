"""CPU tests of the rule that picks a panel from the read support per block and walk: phi_panel_choose (include/phi_host.h,
libphi_host.so, phi_amd/csrc/host/panel_choose.h on the host threads) against its numpy restatement
phi_amd.panel.choose_panel, and the stand-alone program phi_amd/csrc/host/panel_choose_selftest.cpp built plain, with
AddressSanitizer + UndefinedBehaviorSanitizer and with ThreadSanitizer (`make -C phi_amd/csrc/host panel_choose_sanitize`),
run at 1 and 8 host threads.

The 202 cases are those of the program, made here from the same SplitMix64 values: matrices full of ties, all-zero
matrices, all-zero blocks, n_want == n_walks, more always-kept walks than n_want (refused), and two large ones (300 x 1500,
40 x 5000 with n_want = 1022) where the threaded passes and the lazy prefix sort run.  The program checks the header against
a serial restatement of its own; here its lines must also carry the hash of what choose_panel gives."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SAN = os.path.join(ROOT, "build", "sanitize")
BUILDS = ("plain", "asan", "tsan")
N_CASES = 202


def _case(c):
    from phi_amd.ladder import splitmix64
    seed = 0x5EED0000 + c
    v = lambda j: int(splitmix64(seed, j))
    if c >= 200:
        nb, nw, want = (300, 1500, 200) if c == 200 else (40, 5000, 1022)
        x = splitmix64(seed, 8 + np.arange(nb * nw))
        S = np.where(x % np.uint64(16) == 0, x % np.uint64(1000), 0).astype(np.int32).reshape(nb, nw)
        return S, np.zeros(nw, np.uint8), want
    kind = c % 5
    nb, nw = 1 + v(0) % 12, 1 + v(1) % 40
    if kind == 4 and nw < 2:
        nw = 2
    want = 1 + v(2) % nw
    x = splitmix64(seed, 8 + np.arange(nb * nw)).reshape(nb, nw)
    if kind == 0:
        S = x % np.uint64(6)
    elif kind == 1:
        S = np.zeros((nb, nw), np.uint64)
    elif kind == 2:
        S = x % np.uint64(50)
        S[splitmix64(seed + 0xB10C, np.arange(nb)) % np.uint64(2) == 0] = 0
    else:
        S = x % np.uint64(4)
    S = S.astype(np.int32)
    if kind == 4:
        return S, np.ones(nw, np.uint8), 1
    always = (splitmix64(seed + 0xA1, np.arange(nw)) % np.uint64(8) == 0).astype(np.uint8)
    if kind == 3:
        want = nw
    return S, always, max(want, int(always.sum()))


def _hash(keep, round_of):
    h = 0xCBF29CE484222325
    for k, r in zip(keep.tolist(), round_of.tolist()):
        h = ((h ^ k) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
        h = ((h ^ (r & 0xFFFFFFFF)) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.fixture(scope="module")
def expected():
    """Per case: None when the rule refuses it, else (keep, round_of) of choose_panel."""
    from phi_amd.panel import choose_panel
    out = []
    for c in range(N_CASES):
        S, always, want = _case(c)
        try:
            out.append(choose_panel(S, want, always))
        except ValueError:
            out.append(None)
    return out


def test_cases_cover_what_they_claim(expected):
    kinds = [_case(c) for c in range(200)]
    assert sum(e is None for e in expected) == 40 and all(expected[c] is None for c in range(4, 200, 5))
    assert any(not S.any() for S, _, _ in kinds) and any(S.any() and not S.all(1).all() and (S.sum(1) == 0).any() for S, _, _ in kinds)
    assert any(want == S.shape[1] and S.shape[1] > 1 for S, _, want in kinds)
    assert any(a.sum() > 0 for _, a, _ in kinds)
    # ties inside a block, the fill and several rounds all occur
    assert any(e is not None and (e[1] == len(e[1])).any() for e in expected)
    assert any(e is not None and e[1].max() >= 2 and e[1].max() < len(e[1]) for e in expected)
    for e, (S, always, want) in zip(expected, [_case(c) for c in range(N_CASES)]):
        if e is not None:
            assert int(e[0].sum()) == want and ((e[1] == -1) == (always != 0)).all() and ((e[1] == -2) == (e[0] == 0)).all()


def test_library_equals_the_restatement(expected):
    from phi_amd import ilp_index as H
    L = H.host_lib()
    for c in range(N_CASES):
        S, always, want = _case(c)
        S = np.ascontiguousarray(S, np.int32)
        keep, round_of = np.full(S.shape[1], 7, np.uint8), np.full(S.shape[1], 7, np.int32)
        rc = L.phi_panel_choose(S.ctypes.data, S.shape[0], S.shape[1], always.ctypes.data, want, keep.ctypes.data, round_of.ctypes.data)
        if expected[c] is None:
            assert rc == -4, c                                  # PHI_HOST_ERR_INVALID
            continue
        assert rc == 0, c
        assert np.array_equal(keep, expected[c][0]) and np.array_equal(round_of, expected[c][1]), c
    # always = NULL and round_of = NULL are allowed; n_want outside 1 .. min(walks, 1022) is refused
    S = np.ascontiguousarray(_case(0)[0], np.int32)
    keep = np.zeros(S.shape[1], np.uint8)
    assert L.phi_panel_choose(S.ctypes.data, S.shape[0], S.shape[1], None, 1, keep.ctypes.data, None) == 0 and keep.sum() == 1
    assert L.phi_panel_choose(S.ctypes.data, S.shape[0], S.shape[1], None, 0, keep.ctypes.data, None) == -4
    assert L.phi_panel_choose(S.ctypes.data, S.shape[0], S.shape[1], None, S.shape[1] + 1, keep.ctypes.data, None) == -4
    big = np.zeros((1, 2000), np.int32)
    keep = np.zeros(2000, np.uint8)
    assert L.phi_panel_choose(big.ctypes.data, 1, 2000, None, 1023, keep.ctypes.data, None) == -4
    assert L.phi_panel_choose(big.ctypes.data, 1, 2000, None, 1022, keep.ctypes.data, None) == 0 and keep[:1022].all() and not keep[1022:].any()


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "phi_amd", "csrc", "host"), "panel_choose_sanitize", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="exitcode=66:halt_on_error=1")
    return {(b, t): subprocess.run([os.path.join(SAN, "panel_choose_selftest_" + b), str(t)], capture_output=True, text=True, env=env, timeout=600)
            for b in BUILDS for t in (1, 8)}


@pytest.mark.parametrize("threads", (1, 8))
@pytest.mark.parametrize("build", BUILDS)
def test_selftest_agrees_with_its_serial_restatement(outputs, build, threads):
    r = outputs[(build, threads)]
    assert r.returncode == 0, (build, threads, r.stdout[-3000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "FAILED" not in r.stdout and len(r.stdout.splitlines()) == N_CASES


def test_every_build_and_thread_count_prints_the_restatement(outputs, expected):
    first = outputs[("plain", 1)].stdout
    for key, r in outputs.items():
        assert r.stdout == first, key
    for c, line in enumerate(first.splitlines()):
        assert line.startswith("case %d " % c)
        if expected[c] is None:
            assert line.endswith(" refused"), line
        else:
            assert line.endswith("hash=%016x" % _hash(*expected[c])), (c, line)


def test_symbols_are_declared():
    from phi_amd import _capi
    from phi_amd import ilp_index as H
    for name in ("phi_scout_graph", "phi_scout_scores", "phi_scout_choose", "phi_reads_collect_score", "phi_vcf_walks_wide"):
        assert name in _capi.SYMBOLS, name
    assert "phi_panel_choose" in H.HOST_SYMBOLS
