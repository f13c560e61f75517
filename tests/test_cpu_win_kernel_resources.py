"""The window-space read kernel (phi_sketch_win_kernel: reads of one length) within the budget of six waves per SIMD, checked
where the code is built: at most 80 VGPRs, no spill, no scratch (`hipcc -S` metadata), and no more LDS per wave than the
base-space read kernel takes for the same (k, w) -- at (31, 25) and (10, 15) 24 waves per CU -- for every read length
phi_sketch_win_reads gives it."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "phi_amd", "csrc", "sketch.hip")
DEV = os.path.join(ROOT, "phi_amd", "csrc", "sketch_dev.h")            # constants, LDS geometry and helpers of the three sketch units
INSTANCES = ("phi_sketch_win_kernelILb1ELi31ELi25EE", "phi_sketch_win_kernelILb1ELi0ELi0EE", "phi_sketch_win_kernelILb0ELi0ELi0EE")


@pytest.fixture(scope="module")
def sketch_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("asm") / "sketch.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), SRC],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


def _meta(asm, mangled_part):
    entries = asm.split("  - .agpr_count:")
    hits = [e for e in entries[1:] if re.search(r"\.name:\s+\S*" + re.escape(mangled_part), e)]
    assert len(hits) == 1, f"{len(hits)} metadata entries for {mangled_part}"
    return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", hits[0])}


@pytest.mark.parametrize("name", INSTANCES)
def test_window_kernel_fits_six_waves_per_simd(sketch_asm, name):
    m = _meta(sketch_asm, name)
    assert m["vgpr_count"] <= 80, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m


# sketch_dev.h and sketch.hip restated: phi_wave_region_u64 (base space, items of 16 bits), phi_win_region_u64 / phi_sketch_win_reads
WCH, SWW, SBW, Q = 512, 32, 16, 8


def _items(w, k):
    return 1 + WCH + WCH // (w + k + 1) + 2


def _base_region(w, k):
    M = WCH + w
    P = (M + 63) // 64
    slots = ((M - 1) // P + 1) * P
    return ((slots + 8) * 9) // 8 + 8 + SWW + 2 * SBW + ((_items(w, k) + 4) * 2 + 7) // 8


def _win_region(R, s, w, k):
    return max(9 * R * s, 9 * 65 + ((_items(w, k) + 4) * 2 + 7) // 8) + SWW + SBW


def _win_reads(k, w, L):
    V = L - (k + w - 1) + 1
    if V < 1 or L > 928:
        return 0, 0
    G, s = (V + Q - 1) // Q, (V + Q - 1) // Q + (w + Q - 1) // Q
    if G > 64 or (L - k + 1 + G - 1) // G > 32:
        return 0, 0
    R = min(64 // G, 928 // L)
    while R > 0 and _win_region(R, s, w, k) > _base_region(w, k):
        R -= 1
    return R, s


def test_window_kernel_formulas_match_the_source():
    dev, src = open(DEV).read(), open(SRC).read()
    assert re.search(r"#define SWW 32\b", dev) and re.search(r"#define SBW 16\b", dev) and re.search(r"#define Q 8\b", dev)
    assert "const int kmers = 9 * R * s;" in dev and "const int minima = 9 * (64 + 1) + phi_win_items_u64(w, k);" in dev
    assert "if (R > 928 / L) R = (int)(928 / L);" in src


@pytest.mark.parametrize("k,w", [(31, 25), (10, 15), (15, 10), (21, 11), (5, 200), (32, 12), (7, 3)])
def test_window_kernel_lds_never_above_base_space(k, w):
    for L in range(32, 1001):
        R, s = _win_reads(k, w, L)
        if not R:
            continue
        assert R * ((L - (k + w - 1) + Q) // Q) <= 64                      # lanes
        assert R * L <= 928                                                # staged bases
        assert 9 * R * s + SWW + SBW <= _win_region(R, s, w, k)
        assert _win_region(R, s, w, k) <= _base_region(w, k), (L, R, s)
        if (k, w) in ((31, 25), (10, 15)):
            assert _win_region(R, s, w, k) * 8 * 24 <= 160 * 1024, (L, R)    # 24 waves per CU
    # the flagship's reads: five reads of 150 bases a wave, 6 144 B
    assert _win_reads(31, 25, 150) == (5, 16) and _win_region(5, 16, 25, 31) * 8 == 6144
