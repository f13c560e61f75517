"""phi_edit_alignments on the MI355X against the traceback reference of tests/align_ref.c (test_cpu_edit_alignment.py
builds it): the CIGAR byte for byte on the edge-length grid in both orientations, planted and awkward edits, pairs over
several stripes, whole-MHC pairs (replayed, costed, repeatable, batch = single), bad input, independence of the solve
state, and eval_log --identity with and without a device."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_cpu_edit_alignment import build_align_reference, replay
from test_cpu_edit_distance import mutate
from test_gpu_edit_distance import LENGTHS, _walks, build_reference, phi_fasta, rand_seq, truth  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_align_reference(tmp_path_factory.mktemp("align_ref"))


@pytest.fixture(scope="module")
def ond(tmp_path_factory):
    return build_reference(tmp_path_factory.mktemp("edit_ref"))


@pytest.fixture(scope="module")
def ctx(ctx_factory):
    return ctx_factory()


def check(ctx, ref, pairs, band=False):
    """every pair's CIGAR and counts equal the reference's (run in its band at k = d when band)"""
    al = ctx.edit_alignments([a for a, _ in pairs], [b for _, b in pairs])
    assert al.counts.dtype == np.int64 and al.counts.shape == (len(pairs), 4)
    bad = []
    for q, (a, b) in enumerate(pairs):
        m, x, i, d, cost, cig = ref(a, b, int(al.distance[q]) if band else -1)
        if al.cigar[q] != cig or tuple(al.counts[q]) != (m, x, i, d) or al.distance[q] != cost:
            bad.append((q, len(a), len(b), cost, al.cigar[q][:80], cig[:80]))
        n = m + x + i + d
        assert al.identity[q] == (m * 100 / n if n else 0)
    assert not bad, bad[:5]
    return al


def test_edge_lengths_on_both_sides_and_both_orientations(ctx, ref):
    rng = random.Random(21)
    base = rand_seq(rng, 4200)
    pairs = []
    for la in LENGTHS:
        for lb in LENGTHS:
            a = base[:la]
            b = mutate(rng, base[:lb], min(lb, 40)) if lb else b""
            pairs.append((a, b[:lb]))
            pairs.append((b[:lb], a))
    check(ctx, ref, pairs)


def test_planted_and_awkward_edits(ctx, ref, truth):
    rng = random.Random(22)
    t = truth[1_000_000:1_030_000]
    unit = b"CAGGT"
    rep = unit * 1200
    rep_edit = bytearray(rep)
    for _ in range(40):
        p = rng.randrange(len(rep_edit))
        if rng.random() < 0.5:
            del rep_edit[p:p + rng.randrange(1, 11)]
        else:
            rep_edit[p:p] = unit * rng.randrange(1, 3)
    many = bytes(range(33, 33 + 40))                                     # 40 distinct bytes: the stripe's lanes shrink
    wide = bytes(many[rng.randrange(len(many))] for _ in range(9000))
    pairs = [
        (t, t[3000:]),                                                   # a long deletion at the very start
        (t, t[:-2500]),                                                  # ... and at the very end
        (t[1700:], t),                                                   # the same, a the shorter
        (t[:-900], t),
        (b"G" * 700 + t[:5000] + b"T" * 300, t[:5000]),                 # indels at both ends
        (t[:6000], t[:2000] + t[2000:6000] + t[:1000]),
        (t[:20_000] + rep + t[20_000:], t[:20_000] + bytes(rep_edit) + t[20_000:]),   # tandem repeats: ties abound
        (rep[:3000], rep[5:2400]),
        (t[:5000].lower(), mutate(rng, t[:5000], 30).lower()),           # lower case
        (t[:4000], t[:4000].lower()),                                    # lower against upper: all mismatches
        (t[:3000].replace(b"A", b"N"), mutate(rng, t[:3000], 25, b"ACGTN-*")),   # non-ACGT bytes
        (wide, mutate(rng, wide, 200, many)),
        (b"N" * 900, b"N" * 700),
    ]
    al = check(ctx, ref, pairs)
    assert list(al.distance[:4]) == [3000, 2500, 1700, 900]


def test_several_stripes(ctx, ref, truth):
    """50-200 kbp with a few hundred edits: the band is a few blocks wide, so a stripe (64 rows x the workgroup's lanes)
    is 4 096 rows and a pair spans up to 49 of them; edits sit right on stripe borders.  Against the reference in its
    band."""
    rng = random.Random(23)
    pairs = []
    for n in (50_000, 120_000, 200_000):
        t = truth[2_000_000:2_000_000 + n]
        b = bytearray(t)
        for border in range(4096 * ((n // 4096) - 1), 0, -4096):         # an edit on every stripe border (from the end)
            kind = rng.randrange(3)
            if kind == 0:
                b[border] = ord("A") if b[border] != ord("A") else ord("C")
            elif kind == 1:
                b[border:border] = b"G"
            else:
                del b[border - 1:border + 1]
        pairs.append((t, mutate(rng, bytes(b), 150)))
        pairs.append((mutate(rng, t, 100), t))
    check(ctx, ref, pairs, band=True)


def planted(truth, n_edits, seed):
    """truth with n_edits single-base edits at sorted uniform positions (as profiles/edit_distance_rate.py plants them)"""
    r = np.random.default_rng(seed)
    pos = np.sort(r.choice(len(truth) - 20, n_edits, replace=False))
    kind = r.integers(0, 4, n_edits)
    out, last = [], 0
    for p, k in zip(pos.tolist(), kind.tolist()):
        out.append(truth[last:p])
        c = truth[p:p + 1]
        if k <= 1:
            out.append(b"C" if c != b"C" else b"G")
        elif k == 2:
            out.append(b"T" + c)
        last = p + 1
    out.append(truth[last:])
    return b"".join(out)


def fast_replay(a, b, cigar):
    """replay of a whole-MHC CIGAR: '=' runs as slices"""
    i = j = 0
    cnt = [0, 0, 0, 0]
    for n, op in re.findall(r"(\d+)([=XID])", cigar):
        n = int(n)
        if op == "=":
            assert a[i:i + n] == b[j:j + n]
            i += n; j += n; cnt[0] += n
        elif op == "X":
            assert all(a[i + q] != b[j + q] for q in range(n))
            i += n; j += n; cnt[1] += n
        elif op == "I":
            i += n; cnt[2] += n
        else:
            j += n; cnt[3] += n
    assert (i, j) == (len(a), len(b))
    return cnt


def test_full_length_mhc_pairs(ctx, ond, truth, phi_fasta):
    queries = [planted(truth, 20_000, 2024)] + _walks() + [phi_fasta[0]]
    dist = ctx.edit_distances([truth] * len(queries), queries)
    assert ond(truth, queries[0], 25_000) == dist[0]
    batch = ctx.edit_alignments([truth] * len(queries), queries, dist=dist)
    for q, b in enumerate(queries):
        cnt = fast_replay(truth, b, batch.cigar[q])
        assert cnt == list(batch.counts[q]) and sum(cnt[1:]) == dist[q], q
    single = [ctx.edit_alignments([truth], [b], dist=dist[q:q + 1]) for q, b in enumerate(queries)]   # (a second call)
    assert [s.cigar[0] for s in single] == batch.cigar
    counts_only = ctx.edit_alignments([truth], queries[:1], dist=dist[:1], cigar=False)
    assert counts_only.cigar is None and np.array_equal(counts_only.counts[0], batch.counts[0])


def test_bad_input_is_rejected_and_the_context_survives(ctx, ref):
    from phi_amd import _capi
    from phi_amd.context import _ptr
    import ctypes as C
    L = _capi.load()
    h = ctx._h
    rng = random.Random(24)
    a = rand_seq(rng, 3000)
    b = mutate(rng, a, 30)
    d = int(ctx.edit_distances([a], [b])[0])
    for wrong in (d - 1, d + 1, d - 2, d + 7):
        with pytest.raises(Exception) as e:
            ctx.edit_alignments([a], [b], dist=[wrong])
        assert e.value.status == _capi.PHI_ERR_INVALID and "pair 0" in e.value.detail
    with pytest.raises(Exception) as e:
        ctx.edit_alignments([a, a], [a, b], dist=[0, len(a) + len(b)])    # above max(|a|, |b|)
    assert e.value.status == _capi.PHI_ERR_INVALID and "pair 1" in e.value.detail
    s = a + b
    off_a = np.array([0, len(a)], np.int64)
    off_b = np.array([len(a), len(s)], np.int64)
    dist = np.array([d], np.int64)
    counts = np.zeros(5, np.int64)
    short = np.array([0, 11 * (2 * d + 1) - 1], np.int64)
    buf = C.create_string_buffer(11 * (2 * d + 1))
    assert L.phi_edit_alignments(h, s, _ptr(off_a), s, _ptr(off_b), 1, _ptr(dist), _ptr(counts), buf, _ptr(short)) == _capi.PHI_ERR_INVALID
    assert not counts.any()                                               # no work was done
    ok = np.array([0, 11 * (2 * d + 1)], np.int64)
    back = np.array([len(a), 0], np.int64)
    assert L.phi_edit_alignments(h, s, _ptr(back), s, _ptr(off_b), 1, _ptr(dist), _ptr(counts), buf, _ptr(ok)) == _capi.PHI_ERR_INVALID
    assert L.phi_edit_alignments(h, s, _ptr(off_a), s, _ptr(off_b), 1, None, _ptr(counts), buf, _ptr(ok)) == _capi.PHI_ERR_INVALID
    assert L.phi_edit_alignments(h, s, _ptr(off_a), s, _ptr(off_b), 1, _ptr(dist), None, buf, _ptr(ok)) == _capi.PHI_ERR_INVALID
    assert L.phi_edit_alignments(h, s, _ptr(off_a), s, _ptr(off_b), 1, _ptr(dist), _ptr(counts), buf, None) == _capi.PHI_ERR_INVALID
    assert L.phi_edit_alignments(h, None, _ptr(off_a), s, _ptr(off_b), 1, _ptr(dist), _ptr(counts), buf, _ptr(ok)) == _capi.PHI_ERR_INVALID
    assert L.phi_edit_alignments(None, s, _ptr(off_a), s, _ptr(off_b), 1, _ptr(dist), _ptr(counts), buf, _ptr(ok)) == _capi.PHI_ERR_INVALID
    assert L.phi_edit_alignments(h, s, _ptr(off_a), s, _ptr(off_b), 1, _ptr(dist), _ptr(counts), buf, _ptr(ok)) == 0
    m, x, i, dd, cost, cig = ref(a, b)
    assert buf.raw[:counts[4]].decode() == cig and list(counts[:4]) == [m, x, i, dd]
    skipped = ctx.edit_alignments([a, b"", b"ACG", b""], [b, b"", b"", b"TT"], dist=[-1, 0, 3, 2])
    assert list(skipped.counts[0]) == [-1] * 4 and skipped.cigar[0] is None and np.isnan(skipped.identity[0])
    assert skipped.cigar[1:] == ["", "3I", "2D"] and list(skipped.identity[1:]) == [0, 0, 0]
    assert ctx.edit_alignments([b"ACGT"], [b"ACGA"]).cigar == ["3=1X"]


def test_call_between_add_reads_and_solve_leaves_the_solve_alone(ctx_factory):
    from oracle import oracle as O
    from conftest import DATA
    g = O.parse_gfa(os.path.join(DATA, "test.gfa"))
    reads = [s for _, s in O.read_reads(os.path.join(DATA, "read.fa"))]
    A = g.arrays()
    res = []
    for between in (False, True):
        c = ctx_factory(k=3, w=2, threshold=1.0, recombination=100)
        c.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])
        c.add_reads(reads)
        if between:
            al = c.edit_alignments([b"ACGTACGT", b"A" * 5000], [b"ACGAACGT", b"C" * 4000])
            assert al.cigar == ["3=1X4=", "1000I4000X"]
        r = c.solve()
        res.append((r["objective"], r["path_vtx"].tolist(), r["path_hap"].tolist(), r["n_minimizers"].tolist(),
                    c.path_sequence(r["hap_len"])))
    assert res[0] == res[1]


def test_eval_log_identity_with_and_without_a_device(tmp_path, truth, ref, phi_fasta):
    _, log_text, _ = phi_fasta
    log = tmp_path / "run.log"
    log.write_text(log_text)
    t, q = tmp_path / "truth.fa", tmp_path / "query.fa"
    rng = random.Random(25)
    a = truth[:6000]
    b = mutate(rng, a, 120)
    t.write_bytes(b">t\n" + a + b"\n")
    q.write_bytes(b">q\n" + b + b"\n")
    cmd = [sys.executable, "-m", "phi_amd.eval_log", "--truth", str(t), "--query", str(q), "--identity", str(log)]
    gpu = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300, check=True).stdout
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    cpu = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300, check=True, env=env).stdout
    assert gpu == cpu
    m, x, i, d, cost, _ = ref(a, b)
    assert gpu.strip().split("\n")[1].endswith(f",{cost},{m * 100 / (m + x + i + d):.2f}")
    ed = [sys.executable, "-m", "phi_amd.edlib_edits", str(t), str(q)]
    out_gpu = subprocess.run(ed, capture_output=True, text=True, cwd=ROOT, timeout=300, check=True).stdout
    out_cpu = subprocess.run(ed, capture_output=True, text=True, cwd=ROOT, timeout=300, check=True, env=env).stdout
    assert out_gpu == out_cpu == f"Edit distance: {cost}\nAlignment identity: {m * 100 / (m + x + i + d):.2f}%\n"


def test_replay_helper_agrees_with_counts(ref):
    """(the CPU replay used above, on a small pair: a sanity check of the helper itself)"""
    a, b = b"ACGTTGCA", b"ACTTGGCAA"
    m, x, i, d, _, cig = ref(a, b)
    assert replay(a, b, cig) == (m, x, i, d) and fast_replay(a, b, cig) == [m, x, i, d]
