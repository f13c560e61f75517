"""phi_edit_alignments without a GPU: the traceback reference (tests/align_ref.c) against a full-matrix Python traceback,
eval_log's numpy traceback and the O(ND) distance; the ABI declaration and export; the resources of the kernels of
edit_path.hip; eval_log --identity and python -m phi_amd.edlib_edits on a machine without a device.

The reference is compiled into a temporary directory at test time; the GPU tests (test_gpu_edit_alignment.py) use the
same helper."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from test_cpu_edit_distance import HIPCC, build_reference, mutate

ALIGN_SRC = os.path.join(ROOT, "tests", "align_ref.c")
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


def build_align_reference(tmpdir):
    """ctypes function ref(a, b, band=-1) -> (M, X, I, D, cost, cigar), built with cc -O2 into tmpdir."""
    so = os.path.join(str(tmpdir), "libalign_ref.so")
    subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-o", so, ALIGN_SRC])
    L = C.CDLL(so)
    L.ref_align.restype = C.c_int64
    L.ref_align.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.c_int64, C.c_char_p, C.c_int64, C.c_void_p]

    def ref(a, b, band=-1):
        cap = 11 * (2 * (len(a) + len(b)) + 1) if band < 0 else 11 * (2 * band + 1)
        buf = C.create_string_buffer(cap)
        out = (C.c_int64 * 5)()
        n = L.ref_align(a, len(a), b, len(b), band, buf, cap, out)
        assert n >= 0, n
        return tuple(out) + (buf.raw[:n].decode(),)
    return ref


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_align_reference(tmp_path_factory.mktemp("align_ref"))


@pytest.fixture(scope="module")
def ond(tmp_path_factory):
    return build_reference(tmp_path_factory.mktemp("edit_ref"))


def full_traceback(a, b):
    """the rule on the whole matrix, plain Python: (M, X, I, D, cost, cigar)"""
    la, lb = len(a), len(b)
    H = [[0] * (lb + 1) for _ in range(la + 1)]
    for i in range(la + 1):
        for j in range(lb + 1):
            if i == 0 or j == 0:
                H[i][j] = i + j
            else:
                H[i][j] = min(H[i - 1][j - 1] + (a[i - 1] != b[j - 1]), H[i - 1][j] + 1, H[i][j - 1] + 1)
    i, j, ops = la, lb, []
    while i or j:
        v = H[i][j]
        if i and j and H[i - 1][j - 1] + (a[i - 1] != b[j - 1]) == v:
            ops.append("X" if a[i - 1] != b[j - 1] else "="); i -= 1; j -= 1
        elif i and H[i - 1][j] + 1 == v:
            ops.append("I"); i -= 1
        else:
            ops.append("D"); j -= 1
    ops.reverse()
    cig = "".join(f"{len(g.group(0))}{g.group(0)[0]}" for g in re.finditer(r"(=+|X+|I+|D+)", "".join(ops)))
    return ops.count("="), ops.count("X"), ops.count("I"), ops.count("D"), H[la][lb], cig


def replay(a, b, cigar):
    """-> (M, X, I, D) after checking that the CIGAR consumes a and b exactly, '=' on equal bytes and 'X' on others"""
    i = j = 0
    cnt = {"=": 0, "X": 0, "I": 0, "D": 0}
    for n, op in re.findall(r"(\d+)([=XID])", cigar):
        n = int(n)
        assert n > 0
        if op in "=X":
            for q in range(n):
                assert (a[i + q] == b[j + q]) == (op == "="), (i + q, j + q, op)
            i += n; j += n
        elif op == "I":
            i += n
        else:
            j += n
        cnt[op] += n
    assert re.fullmatch(r"(\d+[=XID])*", cigar)
    assert not re.search(r"([=XID])\d+\1", cigar), "adjacent runs of one operation"
    assert (i, j) == (len(a), len(b))
    return cnt["="], cnt["X"], cnt["I"], cnt["D"]


def test_reference_matches_a_full_traceback_and_the_distance(ref, ond):
    from phi_amd.eval_log import alignment
    rng = random.Random(11)
    for t in range(300):
        alphabet = [b"ACGT", b"AC", b"ACGTNacgt", b"CAG"][t % 4]
        la = rng.choice([0, 1, 2, 5, 17, 40, rng.randrange(90)])
        a = bytes(alphabet[rng.randrange(len(alphabet))] for _ in range(la))
        if t % 3 == 0:
            b = bytes(alphabet[rng.randrange(len(alphabet))] for _ in range(rng.randrange(90)))
        else:
            b = mutate(rng, a, rng.randrange(0, 12), alphabet)
        want = full_traceback(a, b)
        got = ref(a, b)
        assert got == want, (t, a, b)
        d = ond(a, b)
        assert got[4] == d and got[1] + got[2] + got[3] == d
        assert ref(a, b, d) == want                          # in Ukkonen's band for k = d: the same path
        assert replay(a, b, got[5]) == got[:4]
        assert alignment(a, b) == got[:4] + (got[5],)       # eval_log's numpy traceback


def test_reference_in_its_band_on_long_pairs(ref, ond):
    from phi_amd.eval_log import alignment
    rng = random.Random(12)
    a = bytes(b"ACGT"[rng.randrange(4)] for _ in range(3000))
    for n_edits in (0, 5, 60):
        b = mutate(rng, a, n_edits)
        d = ond(a, b)
        want = ref(a, b)
        assert ref(a, b, d) == want and want[4] == d
        assert ref(b, a, d)[4] == d
        assert alignment(a, b) == want[:4] + (want[5],)


def test_edit_alignments_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "phi_amd.h")).read()
    assert re.search(r"int phi_edit_alignments\(phi_ctx \*ctx, const char \*a, const int64_t \*a_off, const char \*b, "
                     r"const int64_t \*b_off,\s+int64_t n_pairs, const int64_t \*dist, int64_t \*counts, char \*cigar, "
                     r"const int64_t \*cigar_off\);", hdr)
    assert "data/edlib_edits.py:8-43" in hdr and "data/postprocessing_2_MIQP.py:21-39" in hdr
    from phi_amd import _capi
    assert "phi_edit_alignments" in _capi.SYMBOLS
    lib = _capi.LIB_PATH
    if not os.path.exists(lib):
        pytest.skip("libphi_amd.so not built")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT phi_edit_alignments$", syms, re.M)


# the budget of every kernel of edit_path.hip (VGPRs, static LDS bytes)
PATH_BUDGET = {"phi_edit_ckpt_kernel": (88, 136 * 1024), "phi_edit_rows_kernel": (96, 1024), "phi_edit_walk_kernel": (32, 0)}


def test_path_kernels_have_no_scratch_and_fit_their_budget(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path / "edit_path.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(out), os.path.join(ROOT, "phi_amd", "csrc", "edit_path.hip")],
                       capture_output=True, text=True, check=True)
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = {}
    for blk in blocks:
        name = next((k for k in PATH_BUDGET if k in blk.split()[0]), None)
        if name is None:
            continue
        seen[name] = (int(re.search(r"VGPRs: (\d+)", blk).group(1)), int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)),
                      int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1)))
    assert sorted(seen) == sorted(PATH_BUDGET), seen
    for name, (vgpr, scratch, lds) in seen.items():
        vmax, lmax = PATH_BUDGET[name]
        assert vgpr <= vmax and scratch == 0 and lds <= lmax, (name, vgpr, scratch, lds)
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", out.read_text())


def _fasta(path, name, seq, width=60):
    path.write_bytes(b">" + name + b" some description\n" + b"\n".join(seq[i:i + width] for i in range(0, len(seq), width)) + b"\n")


def test_eval_log_identity_without_a_device(tmp_path, ref):
    from phi_amd.eval_log import read_fasta
    rng = random.Random(13)
    truth = bytes(b"ACGT"[rng.randrange(4)] for _ in range(2500))
    query = mutate(rng, truth, 70)
    t, q, log = tmp_path / "truth.fa", tmp_path / "query.fa", tmp_path / "run.log"
    _fasta(t, b"t", truth)
    _fasta(q, b"q", query)
    log.write_text("Recombination count: 3\nReal time: 1.50 sec\n")
    base = [sys.executable, "-m", "phi_amd.eval_log", "--truth", str(t), "--query", str(q), str(log)]
    plain = subprocess.run(base, capture_output=True, text=True, cwd=ROOT, timeout=300, check=True, env=NO_DEVICE).stdout
    ident = subprocess.run(base + ["--identity"], capture_output=True, text=True, cwd=ROOT, timeout=300, check=True, env=NO_DEVICE).stdout
    rows_p, rows_i = [l.split(",") for l in plain.split()], [l.split(",") for l in ident.split()]
    assert rows_p[0][-1] == "edit_distance" and rows_i[0] == rows_p[0] + ["alignment_identity"]
    assert rows_i[1][:-1] == rows_p[1]
    m, x, i, d, cost, _ = ref(read_fasta(str(t)), read_fasta(str(q)))
    assert rows_p[1][-1] == str(cost)
    assert rows_i[1][-1] == f"{m * 100 / (m + x + i + d):.2f}"
    # without --truth/--query the flag adds nothing
    only = subprocess.run([sys.executable, "-m", "phi_amd.eval_log", "--identity", str(log)], capture_output=True, text=True,
                          cwd=ROOT, timeout=300, check=True, env=NO_DEVICE).stdout
    assert only.split()[0].split(",")[-1] == "pct_retained"


def test_eval_log_without_the_flag_is_unchanged(tmp_path):
    """the default CSV: the header and the row of the previous release's format, nothing appended"""
    rng = random.Random(14)
    truth = bytes(b"ACGT"[rng.randrange(4)] for _ in range(400))
    t, q, log = tmp_path / "truth.fa", tmp_path / "query.fa", tmp_path / "run.log"
    _fasta(t, b"t", truth)
    _fasta(q, b"q", mutate(rng, truth, 9))
    log.write_text("Peak RSS: 1.25 GB\n12.50% Minimizers are in ILP\n")
    out = subprocess.run([sys.executable, "-m", "phi_amd.eval_log", "--truth", str(t), "--query", str(q), str(log)],
                         capture_output=True, text=True, cwd=ROOT, timeout=300, check=True, env=NO_DEVICE).stdout
    from phi_amd.eval_log import FIELDS, edit_distance, read_fasta
    d = edit_distance(read_fasta(str(t)), read_fasta(str(q)))
    want = "log," + ",".join(FIELDS) + ",edit_distance\n" + f"{log},,,1.25,,12.5,,,{d}\n"     # (text mode: \r\n read as \n)
    assert out == want


def test_edlib_edits_command_line(tmp_path, ref):
    """the two lines of data/edlib_edits.py, parsed with the expressions of data/postprocessing_2_MIQP.py:27-28"""
    rng = random.Random(15)
    a = bytes(b"ACGTacgtN"[rng.randrange(9)] for _ in range(1200))
    b = mutate(rng, a, 40, b"ACGTacgtN")
    qa, qb = tmp_path / "query.fa", tmp_path / "reference.fa"
    _fasta(qa, b"first", a)
    qa.write_bytes(qa.read_bytes() + b">second\nACGT\n")                # only the first record counts
    _fasta(qb, b"ref", b)
    out = subprocess.run([sys.executable, "-m", "phi_amd.edlib_edits", str(qa), str(qb)], capture_output=True, text=True,
                         cwd=ROOT, timeout=300, check=True, env=NO_DEVICE).stdout
    m, x, i, d, cost, _ = ref(a, b)                                         # bytes as they are: case counts
    assert out == f"Edit distance: {cost}\nAlignment identity: {m * 100 / (m + x + i + d):.2f}%\n"
    dist = re.search(r"Edit distance:\s+(\d+)", out)
    ident = re.search(r"Alignment identity:\s+(\d+\.\d+)%", out)
    assert int(dist.group(1)) == cost and float(ident.group(1)) == round(m * 100 / (m + x + i + d), 2)
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b">e\n")
    out = subprocess.run([sys.executable, "-m", "phi_amd.edlib_edits", str(empty), str(empty)], capture_output=True, text=True,
                         cwd=ROOT, timeout=300, check=True, env=NO_DEVICE).stdout
    assert out == "Edit distance: 0\nAlignment identity: 0.00%\n"


def test_identity_bound_between_optimal_alignments(ref):
    """all optimal alignments share M - D, so identity moves by at most 100 d^2 / (2 max^2) points
    between them; checked on small pairs over the rule and its mirror (the traceback of (b, a), I and D swapped)."""
    rng = random.Random(16)
    for t in range(100):
        a = bytes(b"ACG"[rng.randrange(3)] for _ in range(rng.randrange(1, 60)))
        b = mutate(rng, a, rng.randrange(1, 15), b"ACG")
        if not b:
            continue
        m1, x1, i1, d1, cost, _ = ref(a, b)
        m2, x2, d2, i2, _, _ = ref(b, a)
        assert m1 - d1 == m2 - d2
        id1, id2 = m1 * 100 / (m1 + x1 + i1 + d1), m2 * 100 / (m2 + x2 + i2 + d2)
        assert abs(id1 - id2) <= 100 * cost ** 2 / (2 * max(len(a), len(b)) ** 2) + 1e-9
