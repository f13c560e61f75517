"""The fixed-geometry window kernel (sketch_win_fixed.hip: 150-bp reads at k = 31, w = 25) within the budget of seven waves
per SIMD, as the generic window kernel: at most 72 VGPRs and 96 SGPRs, no VGPR spill, no scratch (`hipcc -S` metadata),
seven 256-thread workgroups per CU, and the LDS region of the generic kernel at that geometry (720 u64 a wave)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "phi_amd", "csrc", "sketch_win_fixed.hip")
FIXED = "phi_sketch_winfix_kernelILi31ELi25ELi150EE"


@pytest.fixture(scope="module")
def fixed_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("asm") / "sketch_win_fixed.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), SRC],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


def _meta(asm, mangled_part):
    entries = asm.split("  - .agpr_count:")
    hits = [e for e in entries[1:] if re.search(r"\.name:\s+\S*" + re.escape(mangled_part), e)]
    assert len(hits) == 1, f"{len(hits)} metadata entries for {mangled_part}"
    keys = r"(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size)"
    return {k: int(v) for k, v in re.findall(r"\." + keys + r":\s+(\d+)", hits[0])}


def test_fixed_instance_fits_seven_waves_per_simd(fixed_asm):
    m = _meta(fixed_asm, FIXED)
    assert m["vgpr_count"] <= 72 and m["sgpr_count"] <= 96, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert m["sgpr_spill_count"] <= 4, m
    assert m["group_segment_fixed_size"] == 0, m                    # dynamic LDS only: the launch gives the region
    vg = (m["vgpr_count"] + 7) // 8 * 8
    by_vgpr = min(8, 512 // vg)
    by_sgpr = 800 // ((m["sgpr_count"] + 15) // 16 * 16 + 16)
    assert min(by_vgpr, by_sgpr) >= 7, m


def test_only_the_fixed_kernel_is_compiled_there(fixed_asm):
    """the helpers come from sketch_dev.h, which holds no kernel: no second copy of the kernels of sketch.hip (and of their host stubs)"""
    kernels = re.findall(r"^\s+\.amdhsa_kernel (\S+)", fixed_asm, re.M)
    assert len(kernels) == 1 and FIXED in kernels[0], kernels


def test_fixed_region_is_the_generic_one():
    """5 reads of s = 16 rows of 9 u64: 720 u64 = 5 760 B a wave, and the launcher takes exactly that geometry"""
    Q, k, w, L = 8, 31, 25, 150
    V = L - (k + w - 1) + 1
    G = (V + Q - 1) // Q
    s = G + (w + Q - 1) // Q
    assert (V, G, s, 64 // G, (L - k + 1) // G) == (96, 12, 16, 5, 10)
    assert 9 * 5 * s * 8 == 5760 and 7 * 4 * 5760 <= 163840
    src = open(SRC).read()
    assert "A.k == 31 && A.w == 25 && A.uniform_len == 150 && A.win_reads == 5" in src
    assert "phi_win_region_u64(R, s, w, k)" in src
