"""phi_edit_distances without a GPU: the O(ND) test reference against eval_log's numpy DP, the ABI declaration and export,
and the edit kernel's resource budget in its gfx950 code object.

The reference (tests/edit_ref.c, Myers' diagonal transition) is compiled into a temporary directory at test time; the GPU
tests (test_gpu_edit_distance.py) use the same helper."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
REF_SRC = os.path.join(ROOT, "tests", "edit_ref.c")


def build_reference(tmpdir):
    """ctypes function ond(a: bytes, b: bytes, max_d=-1) -> distance or -1, built with cc -O2 into tmpdir."""
    so = os.path.join(str(tmpdir), "libedit_ref.so")
    subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-o", so, REF_SRC])
    L = C.CDLL(so)
    L.ond_edit_distance.restype = C.c_int64
    L.ond_edit_distance.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.c_int64]

    def ond(a, b, max_d=-1):
        return L.ond_edit_distance(a, len(a), b, len(b), max_d)
    return ond


@pytest.fixture(scope="module")
def ond(tmp_path_factory):
    return build_reference(tmp_path_factory.mktemp("edit_ref"))


def mutate(rng, s, n_edits, alphabet=b"ACGT"):
    """s with n_edits random substitutions, insertions and deletions"""
    s = bytearray(s)
    for _ in range(n_edits):
        op = rng.randrange(3)
        p = rng.randrange(len(s) + 1)
        if op == 0 and p < len(s):
            s[p] = alphabet[rng.randrange(len(alphabet))]
        elif op == 1:
            s.insert(p, alphabet[rng.randrange(len(alphabet))])
        elif p < len(s):
            del s[p]
    return bytes(s)


def test_reference_matches_numpy_dp_on_random_pairs(ond):
    from phi_amd.eval_log import edit_distance
    rng = random.Random(7)
    for i in range(200):
        la = rng.choice([0, 1, 2, 17, 64, 65, 300, rng.randrange(2000)])
        alphabet = [b"ACGT", b"AC", b"ACGTNacgt"][i % 3]
        a = bytes(alphabet[rng.randrange(len(alphabet))] for _ in range(la))
        b = mutate(rng, a, rng.randrange(0, 60), alphabet) if i % 5 else bytes(alphabet[rng.randrange(len(alphabet))] for _ in range(rng.randrange(1500)))
        want = edit_distance(a, b) if a and b else max(len(a), len(b))     # (the numpy DP wants both sides non-empty)
        assert ond(a, b) == want, (i, len(a), len(b))
        assert ond(b, a) == want
        assert ond(a, b, want) == want and (want == 0 or ond(a, b, want - 1) == -1)


def test_edit_distances_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "phi_amd.h")).read()
    assert re.search(r"int phi_edit_distances\(phi_ctx \*ctx, const char \*a, const int64_t \*a_off, const char \*b, "
                     r"const int64_t \*b_off,\s+int64_t n_pairs, int64_t max_distance, int64_t \*out\);", hdr)
    from phi_amd import _capi
    assert "phi_edit_distances" in _capi.SYMBOLS
    lib = _capi.LIB_PATH
    if not os.path.exists(lib):
        pytest.skip("libphi_amd.so not built")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT phi_edit_distances$", syms, re.M)


def test_edit_kernel_has_no_scratch_and_fits_its_budget(tmp_path):
    """at most 80 VGPRs (the kernel holds two 64-bit bit vectors, Eq and a few 64-bit column
    indices per lane), no scratch, and at most 136 KB of LDS: 128 KB of Peq, the staged columns and the carries."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path / "edit.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(out), os.path.join(ROOT, "phi_amd", "csrc", "edit.hip")],
                       capture_output=True, text=True, check=True)
    remarks = r.stderr
    assert "phi_edit_band_kernel" in remarks
    vgpr = int(re.search(r"VGPRs: (\d+)", remarks).group(1))
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", remarks).group(1))
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", remarks).group(1))
    assert vgpr <= 80 and scratch == 0 and lds <= 136 * 1024, (vgpr, scratch, lds)
    asm = out.read_text()
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", asm)
    assert "wave_shr:1" in asm           # the lane-to-lane carry is a DPP shift, not a round trip through LDS
