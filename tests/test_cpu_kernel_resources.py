"""The read kernel's occupancy budget, checked where the code is built (no GPU needed: hipcc cross-compiles).

`phi_sketch_kernel<PROBE, WIDE, 31, 25>` runs six waves per SIMD: at most 80 VGPRs (512 / 6, granule 8), no spill into
scratch (a build that spilled four VGPRs ran 35 % slower; five waves instead of six, 9 %) and at most
160 KB / 24 waves of LDS per wave.  A change that silently crosses one of these lines costs more than most
optimisations gain: this test fails instead."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "phi_amd", "csrc", "sketch.hip")
DEV = os.path.join(ROOT, "phi_amd", "csrc", "sketch_dev.h")            # constants, LDS geometry and helpers of the three sketch units


@pytest.fixture(scope="module")
def sketch_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("asm") / "sketch.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), SRC],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


def _meta(asm, mangled_part):
    """the amdhsa.kernels metadata entry of the kernel whose mangled name contains mangled_part"""
    entries = asm.split("  - .agpr_count:")
    hits = [e for e in entries[1:] if re.search(r"\.name:\s+\S*" + re.escape(mangled_part), e)]
    assert len(hits) == 1, f"{len(hits)} metadata entries for {mangled_part}"
    return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", hits[0])}


def test_read_kernel_fits_six_waves_per_simd(sketch_asm):
    m = _meta(sketch_asm, "phi_sketch_kernelILi2ELb1ELi31ELi25EE")          # MODE = PROBE, WIDE, k = 31, w = 25
    assert m["vgpr_count"] <= 80, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    # the generic read kernels (any k, w) must not use scratch either
    for name in ("phi_sketch_kernelILi2ELb1ELi0ELi0EE", "phi_sketch_kernelILi2ELb0ELi0ELi0EE"):
        g = _meta(sketch_asm, name)
        assert g["vgpr_count"] <= 80 and g["vgpr_spill_count"] == 0 and g["private_segment_fixed_size"] == 0, (name, g)


def test_read_kernel_lds_fits_twenty_four_waves_per_cu():
    # phi_wave_region_u64(w, k, pos = false) of sketch_dev.h, restated: dynamic LDS per wave of the read kernel
    WCH, SWW, SBW = 512, 32, 16
    src = open(DEV).read()
    assert re.search(r"#define SWW 32\b", src) and re.search(r"#define SBW 16\b", src) and "#define PHI_WCH 512" in open(os.path.join(ROOT, "phi_amd", "csrc", "phi_kernels.h")).read()

    def region_bytes(w, k):
        M = WCH + w
        P = (M + 63) // 64
        slots = ((M - 1) // P + 1) * P
        mp = ((slots + 8) * 9) // 8 + 8
        items = 1 + WCH + WCH // (w + k + 1) + 2
        return (mp + SWW + 2 * SBW + ((items + 4) * 2 + 7) // 8) * 8

    assert region_bytes(25, 31) * 24 <= 160 * 1024, region_bytes(25, 31)      # the default (k, w): six workgroups of four waves per CU
    assert region_bytes(10, 15) * 24 <= 160 * 1024


@pytest.fixture(scope="module")
def pooled_asm(tmp_path_factory):
    """sketch_pooled.hip as phi_amd/build.py compiles it (its extra flags included)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    from phi_amd import build as B
    out = tmp_path_factory.mktemp("asm") / "sketch_pooled.s"
    src = os.path.join(ROOT, "phi_amd", "csrc", "sketch_pooled.hip")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only"] + list(B.EXTRA_FLAGS.get("sketch_pooled.hip", []))
                          + ["-o", str(out), src], stderr=subprocess.DEVNULL)
    return out.read_text()


def test_pooled_read_kernel_fits_six_waves_per_simd(pooled_asm):
    """The pooled instances (batches of 12 Mbases and more: C3, C4, C5s, C5) live at exactly the 80-VGPR line -- the reason
    they have a translation unit of their own, compiled with machine LICM off; a spill there is the 35 % the one-chunk kernel once lost."""
    names = re.findall(r"\.name:\s+(\S*phi_sketch_pool_kernel\S*)", pooled_asm)
    assert names, "no pooled instance in sketch_pooled.hip"
    for name in sorted(set(n for n in names if not n.endswith(".kd"))):
        m = _meta(pooled_asm, name)
        assert m["vgpr_count"] <= 80 and m["vgpr_spill_count"] == 0, (name, m)
        # No vector register is spilled.  The k = 31 / w = 25 instance keeps a few SCALAR values (kernel arguments used once per
        # chunk) in 36 bytes of scratch per lane; the generic instances spill scalars into vector lanes, not into scratch: the state every measurement of rounds 3-4 was taken in (C3 499 Gbases/s);
        # more than that is a change to look at.
        assert m["private_segment_fixed_size"] <= 36, (name, m)


def test_only_the_pooled_instances_are_compiled_there(pooled_asm):
    """sketch_pooled.hip takes its helpers from sketch_dev.h: its code object holds the three pooled instances and no other
    kernel (a kernel that strayed into it would be compiled without machine LICM, and a second time)"""
    kernels = re.findall(r"^\s+\.amdhsa_kernel (\S+)", pooled_asm, re.M)
    assert len(kernels) == 3 and len(set(kernels)) == 3, kernels
    assert all("phi_sketch_pool_kernel" in k for k in kernels), kernels
    for inst in ("phi_sketch_pool_kernelILb1ELi31ELi25EE", "phi_sketch_pool_kernelILb1ELi0ELi0EE", "phi_sketch_pool_kernelILb0ELi0ELi0EE"):
        assert sum(inst in k for k in kernels) == 1, (inst, kernels)


def test_sixteen_wave_dense_dp_fits_the_lds(tmp_path):
    """phi_dp_kernel<16> (513..1022 walks): 1 024 lanes at no more than 128 VGPRs, no scratch, and its static LDS inside the
    160 KB of a CU (the difference ring alone is 128 KB)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path / "dp.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(ROOT, "phi_amd", "csrc", "dp.hip")], stderr=subprocess.DEVNULL)
    m = _meta(out.read_text(), "phi_dp_kernelILi16EE")
    assert m["vgpr_count"] <= 128 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert m["group_segment_fixed_size"] <= 160 * 1024, m


def test_scan_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """Every kernel of scan.hip (the three-phase pair in its three instances, the single-workgroup scan in its two, the
    compaction pair): no spill, no private segment."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path / "scan.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(ROOT, "phi_amd", "csrc", "scan.hip")], stderr=subprocess.DEVNULL)
    asm = out.read_text()
    kernels = sorted(set(re.findall(r"^\s+\.name:\s+(\S+)$", asm.split("amdhsa.kernels:")[1], flags=re.M)))
    kernels = [k for k in kernels if "kernel" in k]
    for part, count in (("phi_scan_blocksum_kernel", 3), ("phi_scan_apply_kernel", 3), ("phi_scan_tiles_kernel", 2), ("phi_flag_count_kernel", 1),
                        ("phi_flag_write_kernel", 1)):
        assert sum(part in k for k in kernels) == count, (part, kernels)
    for kernel in kernels:
        m = _meta(asm, kernel)
        print(kernel, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (kernel, m)


def test_event_dp_kernels_fit_the_tasks_per_cu_their_launchers_state(tmp_path):
    """dp_events.hip: the consumer + producers kernel uses no scratch in any instance (its consumer wave is the serial chain
    of the solve), and the static LDS of an instance leaves room for the workgroups per CU (160 KB of LDS) that the comments
    at its launchers count on: six for the rows of blocks of at most 64 steps (CK = 32), four / three for the rows / paths on
    a ring of 256 tops, two on a ring of 1 024.  Every instance, and the two- and four-wave kernel, fits one CU."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path / "dp_events.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(ROOT, "phi_amd", "csrc", "dp_events.hip")], stderr=subprocess.DEVNULL)
    asm = out.read_text()
    kernels = sorted(set(re.findall(r"^\s+\.name:\s+(\S+)$", asm.split("amdhsa.kernels:")[1], flags=re.M)))
    LDS = 160 * 1024
    DP_ROW, DP_PATH = 1, 2
    pc = [k for k in kernels if "phi_dp_events_pc_kernel" in k]
    assert len(pc) == 8, pc
    seen = set()
    for kernel in pc:
        npw, mode, p, ringt, qd, ck = map(int, re.search(r"pc_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE", kernel).groups())
        m = _meta(asm, kernel)
        print(kernel, m)
        assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (kernel, m)
        lds = m["group_segment_fixed_size"]
        assert lds <= LDS, (kernel, m)
        if ck == 32:
            seen.add("ck32")
            assert mode == DP_ROW and lds * 6 <= LDS, (kernel, m)
        elif ringt == 256 and mode == DP_ROW:
            seen.add("row256")
            assert lds * 4 <= LDS, (kernel, m)
        elif ringt == 256 and mode == DP_PATH:
            seen.add("path256")
            assert lds * 3 <= LDS, (kernel, m)
        elif ringt == 1024:
            seen.add(("ring1024", mode))
            assert lds * 2 <= LDS, (kernel, m)
    assert seen == {"ck32", "row256", "path256", ("ring1024", DP_ROW), ("ring1024", DP_PATH)}, seen
    wide = [k for k in kernels if "phi_dp_events_kernelILi" in k]
    assert len(wide) == 4 and all(re.search(r"kernelILi[24]ELi[02]EE", k) for k in wide), wide      # two or four waves, DP_SEQ or DP_PATH
    for kernel in wide:
        assert _meta(asm, kernel)["group_segment_fixed_size"] <= LDS, kernel
