"""phi_edit_distances on the MI355X against the O(ND) reference of tests/edit_ref.c (test_cpu_edit_distance.py builds
it): edge lengths, planted edits, band doublings and stripes, the cap, full-length MHC pairs, batching, independence of
the solve state, bad arguments, and the eval_log route with and without a device."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, ROOT
from test_cpu_edit_distance import build_reference, mutate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ond(tmp_path_factory):
    return build_reference(tmp_path_factory.mktemp("edit_ref"))


@pytest.fixture(scope="module")
def ctx(ctx_factory):
    return ctx_factory()


@pytest.fixture(scope="module")
def truth():
    from phi_amd.eval_log import read_fasta
    return read_fasta(os.path.join(DATA, "MHC-CHM13.0.fa.gz"))


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(alphabet[rng.randrange(len(alphabet))] for _ in range(n))


def check(ctx, ond, pairs):
    got = ctx.edit_distances([a for a, _ in pairs], [b for _, b in pairs])
    want = [ond(a, b) for a, b in pairs]
    assert got.dtype == np.int64
    bad = [(i, len(a), len(b), int(g), w) for i, ((a, b), g, w) in enumerate(zip(pairs, got, want)) if g != w]
    assert not bad, bad[:10]
    return got


LENGTHS = [0, 1, 63, 64, 65, 127, 128, 4095, 4096, 4097]


def test_edge_lengths_on_both_sides(ctx, ond):
    rng = random.Random(1)
    base = rand_seq(rng, 4200)
    pairs = []
    for la in LENGTHS:
        for lb in LENGTHS:
            a = base[:la]
            b = mutate(rng, base[:lb], min(lb, 40)) if lb else b""
            pairs.append((a, b[:lb] if len(b) > lb else b))
    got = check(ctx, ond, pairs)
    for (a, b), g in zip(pairs, got):
        if not a or not b:
            assert g == max(len(a), len(b))


def test_planted_edits(ctx, ond, truth):
    rng = random.Random(2)
    t = truth[1_000_000:1_200_000]
    subs = bytearray(t)
    for p in rng.sample(range(len(t)), 700):
        subs[p] = b"ACGT"[(b"ACGT".index(subs[p]) + 1) % 4] if subs[p] in b"ACGT" else ord("A")
    deletion = t[:90_000] + t[100_000:]                                   # one 10-kb deletion
    unit = b"CAGGT"
    rep = unit * 4000                                                      # 20 kb tandem repeat with indels inside it
    rep_edit = bytearray(rep)
    for _ in range(60):
        p = rng.randrange(len(rep_edit))
        if rng.random() < 0.5:
            del rep_edit[p:p + rng.randrange(1, 11)]
        else:
            rep_edit[p:p] = unit * rng.randrange(1, 3)
    far = mutate(rng, t[:8_000], 20)                                       # |n - m| = 32 kb, far above the rest
    pairs = [
        (t, bytes(subs)),
        (t, deletion),
        (t[:50_000] + rep + t[50_000:80_000], t[:50_000] + bytes(rep_edit) + t[50_000:80_000]),
        (t[:40_000], far),
        (b"N" * 5000, b"N" * 4100),                                        # all-N: N equals N
        (t[:20_000], t[:20_000].lower()),                                  # lower case against upper: 20 000 mismatches
        (t[:3000].lower(), mutate(rng, t[:3000], 30).lower()),
    ]
    got = check(ctx, ond, pairs)
    assert got[1] == 10_000 and got[4] == 900 and got[5] == 20_000


def test_band_doublings_and_stripes(ctx, ond, truth):
    """distances of ~3 000 over 150 kb: the band starts at 64 and doubles at least six times, and every pass runs the
    rows in stripes of at most the workgroup's lanes (far fewer than the 2 300 blocks); the unrelated 75 kb pair needs
    a band of more than 1 024 blocks, so stripes of the largest workgroup."""
    rng = random.Random(3)
    t = truth[2_000_000:2_150_000]
    pairs = [(t, mutate(rng, t, 3000)), (mutate(rng, t, 1500), mutate(rng, t, 1500))]
    got = check(ctx, ond, pairs)
    assert all(g > 512 for g in got)
    a, b = rand_seq(rng, 75_000), rand_seq(rng, 74_000)
    far = check(ctx, ond, [(a, b)])
    assert far[0] > 65_536 // 2


def test_max_distance(ctx, ond, truth):
    rng = random.Random(4)
    a = truth[3_000_000:3_040_000]
    b = mutate(rng, a, 400)
    d = ond(a, b)
    assert ctx.edit_distances([a], [b], max_distance=d)[0] == d
    assert ctx.edit_distances([a], [b], max_distance=d - 1)[0] == -1
    assert ctx.edit_distances([a], [a], max_distance=0)[0] == 0
    assert ctx.edit_distances([a[:100]], [a[:200]], max_distance=99)[0] == -1      # |n - m| alone exceeds the cap
    assert ctx.edit_distances([a], [b], max_distance=10**9)[0] == d


def _walks():
    from oracle import oracle as O
    g = O.parse_gfa(os.path.join(DATA, "MHC_4.gfa.gz"))
    A = g.arrays()
    sc, so = A["seq_concat"], A["seq_off"]
    return [b"".join(bytes(sc[so[v]:so[v + 1]]) for v in p).upper() for p in g.paths]


@pytest.fixture(scope="module")
def phi_fasta(tmp_path_factory):
    """the FASTA PHI writes for config 1 (CHM13 reads on MHC_4)"""
    from phi_amd.eval_log import read_fasta
    tmp = tmp_path_factory.mktemp("phi")
    phi = os.path.join(ROOT, "phi_amd", "PHI")
    out = tmp / "CHM13.fa"
    r = subprocess.run([phi, "-t32", "-g", os.path.join(DATA, "MHC_4.gfa.gz"), "-r", os.path.join(DATA, "CHM13_reads.fq.gz"),
                        "-o", str(out)], capture_output=True, text=True, cwd=str(tmp), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return read_fasta(str(out)), r.stderr, out


REF_MAX_D = 10_000      # the O(ND) reference's time grows about as D^2: 10 000 edits over 5 Mbp take it about a second


def test_full_length_mhc_pairs_and_one_batch(ctx, ond, truth, phi_fasta):
    """Every walk of MHC_4 and PHI's config-1 haplotype against the whole CHM13 MHC (4.92 Mbp), at full length, in one
    batch call, equal to the one-pair calls.  Against the O(ND) reference: a pair whose distance is at most 10 000 at full
    length is compared at full length; a larger one (the reference would need more than a minute) on the longest prefix
    of both sequences, halving from the full length, whose distance is at most 10 000 -- and every prefix on the way is
    compared with the cap set to 10 000 (-1 from both)."""
    queries = _walks() + [phi_fasta[0]]
    batch = ctx.edit_distances([truth] * len(queries), queries)
    single = [int(ctx.edit_distances([truth], [q])[0]) for q in queries]
    assert list(batch) == single
    for q, d in zip(queries, single):
        n = max(len(truth), len(q))
        while True:
            a, b = truth[:n], q[:n]
            dn = int(ctx.edit_distances([a], [b], max_distance=REF_MAX_D)[0])
            assert dn == ond(a, b, REF_MAX_D), (len(q), n)
            if dn >= 0:
                break
            n //= 2
        if n >= max(len(truth), len(q)):
            assert dn == d
        else:
            assert int(ctx.edit_distances([a], [b])[0]) == dn


def test_call_between_add_reads_and_solve_leaves_the_solve_alone(ctx_factory):
    from oracle import oracle as O
    g = O.parse_gfa(os.path.join(DATA, "test.gfa"))
    reads = [s for _, s in O.read_reads(os.path.join(DATA, "read.fa"))]
    A = g.arrays()
    res = []
    for between in (False, True):
        c = ctx_factory(k=3, w=2, threshold=1.0, recombination=100)
        c.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])
        c.add_reads(reads)
        if between:
            assert list(c.edit_distances([b"ACGTACGT", b"A" * 5000], [b"ACGAACGT", b"C" * 4000])) == [1, 5000]
        r = c.solve()
        res.append((r["objective"], r["path_vtx"].tolist(), r["path_hap"].tolist(), r["n_minimizers"].tolist(),
                    c.path_sequence(r["hap_len"])))
    assert res[0] == res[1]


def test_bad_arguments_are_invalid_and_the_context_survives(ctx):
    from phi_amd import _capi
    from phi_amd.context import _ptr
    L = _capi.load()
    out = np.zeros(2, np.int64)
    good = np.array([0, 4, 8], np.int64)
    back = np.array([0, 4, 3], np.int64)
    s = b"ACGTACGA"
    h = ctx._h
    assert L.phi_edit_distances(h, s, _ptr(good), s, _ptr(good), 2, -1, None) == _capi.PHI_ERR_INVALID
    assert L.phi_edit_distances(h, s, None, s, _ptr(good), 2, -1, _ptr(out)) == _capi.PHI_ERR_INVALID
    assert L.phi_edit_distances(h, None, _ptr(good), s, _ptr(good), 2, -1, _ptr(out)) == _capi.PHI_ERR_INVALID
    assert L.phi_edit_distances(h, s, _ptr(back), s, _ptr(good), 2, -1, _ptr(out)) == _capi.PHI_ERR_INVALID
    assert L.phi_edit_distances(h, s, _ptr(good), s, _ptr(back), 2, -1, _ptr(out)) == _capi.PHI_ERR_INVALID
    assert L.phi_edit_distances(None, s, _ptr(good), s, _ptr(good), 2, -1, _ptr(out)) == _capi.PHI_ERR_INVALID
    assert list(ctx.edit_distances([b"ACGT", b"ACGT"], [b"ACGT", b"ACGA"])) == [0, 1]


def test_eval_log_prints_the_same_csv_with_and_without_a_device(tmp_path, truth, ond, phi_fasta):
    _, log_text, _ = phi_fasta
    log = tmp_path / "run.log"
    log.write_text(log_text)
    t = tmp_path / "truth.fa"
    q = tmp_path / "query.fa"
    t.write_bytes(b">t\n" + truth[:20_000] + b"\n")
    rng = random.Random(5)
    q.write_bytes(b">q\n" + mutate(rng, truth[:20_000], 150) + b"\n")
    cmd = [sys.executable, "-m", "phi_amd.eval_log", "--truth", str(t), "--query", str(q), str(log)]
    gpu = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300, check=True).stdout
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")                   # no device visible: the numpy DP
    cpu = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300, check=True, env=env).stdout
    assert gpu == cpu
    d = ond(truth[:20_000], q.read_bytes().split(b"\n")[1])
    assert gpu.strip().split("\n")[1].endswith("," + str(d))
