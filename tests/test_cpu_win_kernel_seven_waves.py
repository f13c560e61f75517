"""The window-space read kernel (phi_sketch_win_kernel) within the budget of SEVEN waves per SIMD, so that the 6 880 waves of
C2 (1 720 workgroups of four) are resident at once: at most 72 VGPRs, at most 96 SGPRs (256-thread workgroups per CU
<= 800 / (ceil(s / 16) 16 + 16)), no VGPR spill, no scratch (`hipcc -S` metadata), and at most 720 u64 of LDS per wave at
(31, 25), L = 150 -- the staged words and the bitmap of bases outside ACGTacgt no longer lie behind the k-mers."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "phi_amd", "csrc", "sketch.hip")
DEV = os.path.join(ROOT, "phi_amd", "csrc", "sketch_dev.h")            # constants, LDS geometry and helpers of the three sketch units
POOLED = os.path.join(ROOT, "phi_amd", "csrc", "sketch_pooled.hip")
FLAGSHIP = "phi_sketch_win_kernelILb1ELi31ELi25EE"
GENERIC = ("phi_sketch_win_kernelILb1ELi0ELi0EE", "phi_sketch_win_kernelILb0ELi0ELi0EE")


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
    keys = r"(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size)"
    return {k: int(v) for k, v in re.findall(r"\." + keys + r":\s+(\d+)", hits[0])}


def _blocks_per_cu(m):
    vg = (m["vgpr_count"] + 7) // 8 * 8
    by_vgpr = min(8, 512 // vg)                                     # waves per SIMD = 256-thread workgroups per CU
    by_sgpr = 800 // ((m["sgpr_count"] + 15) // 16 * 16 + 16)
    return min(by_vgpr, by_sgpr)


def test_flagship_instance_fits_seven_waves_per_simd(sketch_asm):
    m = _meta(sketch_asm, FLAGSHIP)
    assert m["vgpr_count"] <= 72 and m["sgpr_count"] <= 96, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    # SGPR spills go to lanes of a VGPR that the count above includes; the few left are on the byte-wise routine only
    assert m["sgpr_spill_count"] <= 4, m
    assert _blocks_per_cu(m) >= 7, m


@pytest.mark.parametrize("name", GENERIC)
def test_generic_instances_fit_seven_waves_per_simd(sketch_asm, name):
    m = _meta(sketch_asm, name)
    assert m["vgpr_count"] <= 72 and m["sgpr_count"] <= 96, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m


def test_only_the_window_kernel_declares_seven_waves():
    src = open(SRC).read()
    assert re.search(r"__launch_bounds__\(TPB, 7\) phi_sketch_win_kernel\(", src)
    assert re.search(r"__launch_bounds__\(TPB, 6\) phi_sketch_pool_kernel\(", open(POOLED).read())
    assert re.search(r"__launch_bounds__\(TPB, MODE == PHI_MODE_PROBE \? 6 : 1\) phi_sketch_kernel\(", src)


# sketch_dev.h and sketch.hip restated (see test_cpu_win_kernel_resources.py for the rest of the geometry)
WCH, SWW, SBW, Q = 512, 32, 16, 8


def _items(w, k):
    return 1 + WCH + WCH // (w + k + 1) + 2


def _base_region(w, k):
    M = WCH + w
    P = (M + 63) // 64
    slots = ((M - 1) // P + 1) * P
    return ((slots + 8) * 9) // 8 + 8 + SWW + 2 * SBW + ((_items(w, k) + 4) * 2 + 7) // 8


def _mp(R, s, w, k):
    return max(9 * R * s, 9 * 65 + ((_items(w, k) + 4) * 2 + 7) // 8)


def _old_region(R, s, w, k):
    return _mp(R, s, w, k) + SWW + SBW


def _new_region(R, s, w, k):
    return _mp(R, s, w, k)


def _win_reads(k, w, L):
    V = L - (k + w - 1) + 1
    if V < 1 or L > 928:
        return 0, 0
    G, s = (V + Q - 1) // Q, (V + Q - 1) // Q + (w + Q - 1) // Q
    if G > 64 or (L - k + 1 + G - 1) // G > 32:
        return 0, 0
    R = min(64 // G, 928 // L)
    while R > 0 and _new_region(R, s, w, k) + SWW + SBW > _base_region(w, k):
        R -= 1
    return R, s


def test_region_formula_matches_the_source():
    src = open(SRC).read()
    assert re.search(r"static inline int phi_win_region_u64\(int R, int s, int w, int k\) \{ return phi_win_mp_u64\(R, s, w, k\); \}", open(DEV).read())
    assert "while (R > 0 && phi_win_region_u64(R, s, w, k) + SWW + SBW > phi_wave_region_u64(w, k, false)) R--;" in src
    # the staged words and the bitmap alias the start of the wave's region
    assert "uint64_t *s_words = s_mp;" in src and "unsigned long long *s_bad = (unsigned long long *)s_mp;" in src


def test_flagship_region_fits_seven_workgroups():
    R, s = _win_reads(31, 25, 150)
    assert (R, s) == (5, 16)
    reg = _new_region(R, s, 25, 31)
    assert reg <= 720 and reg * 8 == 5760
    assert 7 * 4 * reg * 8 <= 163840


@pytest.mark.parametrize("k,w", [(31, 25), (10, 15), (15, 10), (21, 11), (5, 200), (32, 12), (7, 3)])
def test_region_never_larger_and_never_above_base_space(k, w):
    for L in range(32, 1001):
        R, s = _win_reads(k, w, L)
        if not R:
            continue
        assert _new_region(R, s, w, k) <= _old_region(R, s, w, k), (L, R)
        assert _new_region(R, s, w, k) <= _base_region(w, k), (L, R)
        assert SWW <= _new_region(R, s, w, k) and SBW <= 9 * 65          # staged words / bitmap inside the region
