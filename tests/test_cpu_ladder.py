"""The sampling rule of the coverage ladder (phi_amd/ladder.py) by itself, the new symbols, and ladder.hip's
kernels' resources for gfx950 (no GPU needed: hipcc cross-compiles)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cpu_kernel_resources import HIPCC, _meta

from phi_amd import ladder as rule

NAMES = ("phi_reads_collect_begin", "phi_reads_collect_end", "phi_reads_collect_release", "phi_ladder_plan", "phi_ladder_advance",
         "phi_ladder_band")


def test_splitmix64_pins():
    """computed with plain Python integers when the rule was written down"""
    assert [int(z) for z in rule.splitmix64(0, np.arange(4))] == [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f, 0xf88bb8a8724c81ec]
    assert [int(u) for u in rule.draws(1234567, np.arange(4))] == [0x599ed017, 0x2c73f084, 0x883ebce5, 0x3fbef740]
    # the same with Python integers, for ordinals beyond 2^32 and a seed with its top bit set
    M = (1 << 64) - 1
    for seed, i in ((0, 0), (1234567, 3), (0xFEDCBA9876543210, (1 << 33) + 5), (M, M - 1)):
        x = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M
        z = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        assert int(rule.splitmix64(seed, np.array([i], np.uint64))[0]) == z
        assert int(rule.draws(seed, np.array([i], np.uint64))[0]) == z >> 32


def test_thresholds():
    assert [int(t) for t in rule.thresholds([0, 2.0 ** -32, 0.5, 1, 7])] == [0, 1, 1 << 31, 1 << 32, 1 << 32]
    for bad in ([0.5, 0.4], [-0.1], [], [0.1] * 17, [float("nan")]):
        with pytest.raises(ValueError):
            rule.thresholds(bad)


def test_levels_are_nested_and_bands_follow_the_thresholds():
    ordinals = np.arange(20000)
    fr = [0.0, 0.05, 0.05, 0.3, 0.8, 1.0]
    band = rule.bands(99, ordinals, fr)
    u, t = rule.draws(99, ordinals), rule.thresholds(fr)
    for i in range(0, 20000, 37):
        want = next((j for j in range(len(fr)) if int(u[i]) < int(t[j])), len(fr))
        assert band[i] == want
    assert not (band == 0).any() and not (band == 2).any() and (band <= 5).all()       # f = 0 takes nothing, f = 1 everything
    prev = np.zeros(len(ordinals), bool)
    for j in range(len(fr)):
        cur = rule.level_mask(99, ordinals, fr, j)
        assert not (prev & ~cur).any()                          # level j - 1 is a subset of level j
        prev = cur
    assert (rule.bands(99, ordinals, [0.3]) == 0).sum() == (band <= 3).sum()           # a level does not depend on the others


def test_kept_counts_are_binomial():
    """seed 7, 100 000 ordinals: 1030 / 9951 / 50189 kept at f = 0.01 / 0.1 / 0.5 (0.95 / 0.52 / 1.20 standard deviations
    from n f); the assertion is 5 sigma, sigma = sqrt(n f (1 - f))"""
    n = 100000
    band = rule.bands(7, np.arange(n), [0.01, 0.1, 0.5])
    for j, f in enumerate((0.01, 0.1, 0.5)):
        kept = int((band <= j).sum())
        print(f, kept, (kept - n * f) / math.sqrt(n * f * (1 - f)))
        assert abs(kept - n * f) <= 5 * math.sqrt(n * f * (1 - f)), (f, kept)


def test_fractions_from_coverage_clip_at_one():
    fr = rule.fractions_from_coverage([0.1, 1, 15, 30], 5000000, 75000000)
    assert fr[:2] == [0.1 * 5000000 / 75000000, 5000000 / 75000000] and fr[2:] == [1.0, 1.0]
    assert rule.fractions_from_coverage([1, 2], 100, 0) == [1.0, 1.0]


def test_ladder_symbols_are_declared_bound_and_exported():
    from phi_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "phi_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _capi.SYMBOLS
    # every entry cites what it replaces
    assert len(re.findall(r"data/preprocess\.py:83-107", hdr)) >= len(NAMES) and len(re.findall(r"data/run_batch_4\.py:38-58", hdr)) >= len(NAMES)
    assert "ladder.hip" in open(os.path.join(ROOT, "phi_amd", "build.py")).read()
    lib = os.path.join(ROOT, "phi_amd", "libphi_amd.so")
    if os.path.exists(lib):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(r" T " + name + r"\b", syms), name
    from phi_amd import Context
    for m in ("collect_begin", "collect_end", "ladder_plan", "ladder_advance", "ladder_band", "coverage_ladder"):
        assert callable(getattr(Context, m))


def test_ladder_kernels_compile_for_gfx950_without_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path / "ladder.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(ROOT, "phi_amd", "csrc", "ladder.hip")], stderr=subprocess.DEVNULL)
    asm = out.read_text()
    for kernel in ("ladder_append_kernel", "ladder_count_kernel", "ladder_scan_kernel", "ladder_scatter_kernel", "ladder_copy_kernel"):
        m = _meta(asm, kernel)
        print(kernel, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (kernel, m)
