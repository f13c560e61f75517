"""The smallest shapes that still reach every kernel family, run as a CHILD PROCESS by tests/test_gpu_dirty_memory.py under
PHI_DEVICE_POISON (every device buffer starts out full of a byte of the test's choosing), under PHI_DEVICE_POOL_MIN=256 (every
buffer comes back with an earlier owner's contents) and on contexts that have been used before.

    python tests/dirty_battery.py GROUP [--reference-only]        GROUP: one of GROUPS, or "all"

Every case builds its input from a fixed seed (tests/graphgen.py, tests/golden/data), computes the CPU reference the suite
already trusts for that operation (oracle/, the host readers, zlib, tests/edit_ref.c, tests/align_ref.c, phi_amd/ladder.py,
phi_amd/vcf2gfa.py, the numpy chop rule), runs the operation on the GPU, ASSERTS the result against that reference here, in the
child, asserts that it reached the code it is there for (solve_stats()["dp_mode"], info["one_length"], chop_stats(), ...) and
returns a digest: every integer result and a hash of every result array -- never a time, never an address.  The last line
printed is one JSON object {case: digest}; the parent compares it, exactly, with the digest of a run on clean memory.

--reference-only builds every case and runs only its CPU reference, without touching the GPU library: the cases stay honest
where no GPU is present (tests/test_cpu_dirty_battery.py).

A case that fails its assertion is reported and the next one runs; any other error (a device error among them) ends the child
at once: nothing more goes to a GPU that may have faulted."""
import contextlib
import gzip
import hashlib
import json
import os
import random
import sys
import tempfile
import time
import traceback
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

DATA = os.path.join(HERE, "golden", "data")
GROUPS = {}                                                # group -> [(case name, function)]


def case(group):
    def deco(fn):
        GROUPS.setdefault(group, []).append((fn.__name__, fn))
        return fn
    return deco


# --------------------------------------------------------------------------- plumbing

class Gpu:
    """What a case needs of the GPU side: contexts (closed at the end of the case), the helpers of the GPU test modules."""

    def __init__(self):
        import conftest  # noqa: F401  (torch initialises before libphi_amd.so is loaded, as in the suite)
        import phi_amd
        self.phi = phi_amd
        self.made = []

    def ctx(self, **params):
        c = self.phi.Context(0)
        if params:
            c.set_params(**params)
        self.made.append(c)
        return c

    def close_all(self):
        for c in self.made:
            c.close()
        self.made = []

    def device_u64(self, p, n):
        """sorted host copy of n 64-bit words at device address p"""
        import torch
        from phi_amd import dist as pdist
        if not n:
            return np.zeros(0, np.uint64)
        return np.sort(torch.as_tensor(pdist.DevArray(p, n, "<i8"), device="cuda").clone().cpu().numpy().view(np.uint64))

    def device_u8(self, p, n):
        import torch
        from phi_amd import dist as pdist
        return torch.as_tensor(pdist.DevArray(p, n), device="cuda").cpu().numpy().copy()


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def H(x):
    """hash of a result array / byte string / list of them"""
    h = hashlib.sha1()

    def feed(y):
        if isinstance(y, np.ndarray):
            h.update(str(y.dtype).encode() + str(y.shape).encode() + np.ascontiguousarray(y).tobytes())
        elif isinstance(y, (bytes, bytearray)):
            h.update(b"b%d:" % len(y) + bytes(y))
        elif isinstance(y, str):
            feed(y.encode())
        elif y is None:
            h.update(b"none")
        elif isinstance(y, (int, np.integer)):
            h.update(b"i%d;" % int(y))
        elif isinstance(y, (list, tuple)):
            h.update(b"l%d:" % len(y))
            for z in y:
                feed(z)
        else:
            raise TypeError(type(y))
    feed(x)
    return h.hexdigest()[:20]


def D(d):
    """a dict of results as a digest: integers as they are, arrays and byte strings hashed; times and floats left out"""
    out = {}
    for k, v in d.items():
        if k.endswith("_ms") or k.endswith("_s") or isinstance(v, float):
            continue
        if isinstance(v, (bool, int, np.integer)):
            out[k] = int(v)
        elif isinstance(v, dict):
            for kk, vv in D(v).items():
                out[f"{k}.{kk}"] = vv
        else:
            out[k] = H(v)
    return out


def set_graph(ctx, g, chop=None):
    A = g.arrays()
    return ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"], chop=chop)


def rseq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(list(alphabet), size=int(n)).tolist())


def same_result(a, b, what=""):
    """two solve() results (or any dicts of integers and arrays), field for field"""
    assert a.keys() == b.keys(), what
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), (what, key)
        else:
            assert a[key] == b[key], (what, key, a[key], b[key])


def write_gfa(g, path):
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "wt") as f:
        f.write("H\tVN:Z:1.1\n")
        for i, s in enumerate(g.node_seq):
            f.write(f"S\ts{i + 1}\t{s.decode()}\n")
        for u, a in enumerate(g.adj):
            for v in a:
                f.write(f"L\ts{u + 1}\t+\ts{v + 1}\t+\t0M\n")
        for h, p in enumerate(g.paths):
            smp, hap = g.hap_names[h].rsplit(".", 1)
            f.write(f"W\t{smp}\t{hap}\tchr\t0\t1\t" + "".join(f">s{v + 1}" for v in p) + "\n")
    return str(path)


_TMP = None


def tmpdir():
    global _TMP
    if _TMP is None:
        _TMP = tempfile.TemporaryDirectory(prefix="dirty_battery_")
    return _TMP.name


# --------------------------------------------------------------------------- the full path against the oracle

class FullCase:
    """graph + reads + parameters, the oracle's stages 1-2 and its restated model; check(): a context's solve against them
    (tests/test_gpu_parity.py _check_against_oracle, which also evaluates the decoded path with Model.objective)"""

    def __init__(self, g, reads, k, w, T, R, brute=False):
        from oracle import oracle as O
        from oracle import solve_oracle as S
        self.g, self.reads, self.k, self.w, self.T, self.R = g, reads, k, w, T, R
        self.st = O.run_stage12(g, reads, k, w, T)
        self.model = S.Model(g, self.st, R)
        self.best = self.model.brute_force()[0] if brute else None

    def context(self, gpu, budget=None):
        ctx = gpu.ctx(k=self.k, w=self.w, threshold=self.T, recombination=self.R)
        if budget is not None:
            ctx.set_solve_budget(budget)
        return ctx

    def check(self, ctx):
        from oracle import oracle as O
        from test_gpu_parity import _check_against_oracle
        st, res, m = _check_against_oracle(O, ctx, self.g, self.reads, self.k, self.w, self.T, self.R)
        if self.best is not None:
            assert res["objective"] == self.best, (res["objective"], self.best)
        return res

    def evaluate(self, res):
        """a solve that may have stopped at its budget: the path is feasible, has the reported value, below the bound"""
        from oracle import solve_oracle as S
        obj, cov, nsw = self.model.objective(S.states_from_path(res["path_vtx"], res["path_hap"]))
        assert obj == res["objective"] and obj <= res["upper_bound"], (obj, res["objective"], res["upper_bound"])
        assert (res["spectrum_size"], res["filtered"], res["n_in_model"]) == (len(self.st.spectrum), self.st.filtered, self.st.n_in_model)

    def run(self, gpu, budget=None, chop=None):
        ctx = self.context(gpu, budget)
        set_graph(ctx, self.g, chop)
        ctx.add_reads(self.reads)
        return ctx


def solve_digest(ctx, res):
    return dict(D(res), stats=D(ctx.solve_stats()))


# =========================================================================== reads

SKETCH_KW = [(31, 25), (3, 2), (32, 256), (45, 25)]


@case("reads")
def sketch(gpu):
    from oracle import oracle as O
    out = {}
    for k, w in SKETCH_KW:
        rng = np.random.default_rng(1000 * k + w)
        seqs = [rseq(rng, L) for L in (0, k - 1, k, k + w - 1, k + w, 4097)]
        bad = bytearray(rseq(rng, 700))
        for i in rng.choice(700, size=9, replace=False).tolist():
            bad[i] = int(rng.choice(list(b"NnRYx*-a")))
        seqs.append(bytes(bad))
        want = [O.sketch(q, k, w) for q in seqs]
        eh = np.concatenate([a for a, _ in want])
        ep = np.concatenate([b for _, b in want])
        es = np.concatenate([np.full(len(a), i, np.int32) for i, (a, _) in enumerate(want)])
        assert len(eh) > 0
        if gpu is None:
            continue
        h, p, s = gpu.ctx().sketch(seqs, k, w)
        assert np.array_equal(s, es) and np.array_equal(p, ep) and np.array_equal(h, eh), (k, w)
        out[f"k{k}w{w}"] = H([h, p, s])
    return out


def _scoring_case():
    from graphgen import mosaic_reads, random_graph
    rng = np.random.default_rng(9103)
    g = random_graph(rng, n_sites=12, n_walks=4, seg_len=(30, 80), alt_len=(2, 9))
    reads = mosaic_reads(rng, g, n_reads=160, read_len=150, n_seg=2, err=0.02)
    reads += [rseq(rng, rng.integers(1, 400), b"ACGTNacgtn") for _ in range(60)]
    reads += [rseq(rng, 150) for _ in range(531 - len(reads))]
    order = rng.permutation(len(reads))
    return g, [reads[i] for i in order]


def _score_against_oracle(gpu, ctx, g, st, n_reads, n_bases, n_emitted):
    """spectrum size, kept-anchor counters, the set of read hashes that are no walk minimisers, n_minimizers"""
    rs = ctx.reads_stats()
    assert (rs["n_reads"], rs["n_bases"]) == (n_reads, n_bases)
    assert rs["n_distinct"] == len(st.spectrum) and rs["n_emitted"] == n_emitted, (rs, len(st.spectrum), n_emitted)
    res = ctx.solve()
    assert res["spectrum_size"] == len(st.spectrum)
    assert (res["filtered"], res["retained"], res["n_in_model"]) == (st.filtered, st.retained, st.n_in_model)
    assert np.array_equal(res["n_anchors"], st.n_anchors) and np.array_equal(res["n_minimizers"], st.n_minimizers)
    absent = gpu.device_u64(*ctx.spectrum_export())
    assert np.array_equal(absent, st.spectrum[~np.isin(st.spectrum, np.unique(st.m_hash))])
    hits = gpu.device_u8(*ctx.hits_buffer())
    assert int(hits.sum()) == len(st.spectrum) - len(absent)
    return dict(D(rs), **D(res), absent=H(absent), hits=H(hits))


@case("reads")
def scoring(gpu):
    """one read set as one batch, as three batches of growing size (the log of novel hashes, the overflow list and the
    offsets grow and keep what they hold), and through the pooled kernel"""
    from oracle import oracle as O
    g, reads = _scoring_case()
    k, w = 15, 10
    st = O.run_stage12(g, reads, k, w, 1.0)
    n_emitted = sum(len(O.sketch(r, k, w)[0]) for r in reads)
    assert len(reads) == 531 and st.n_in_model > 0
    if gpu is None:
        return None
    out = {}
    routes = (("one_batch", [reads], {}), ("three_batches", [reads[:130], reads[130:131], reads[131:]], {}),
              ("pooled", [reads[:130], reads[130:131], reads[131:]], dict(PHI_SKETCH_POOL_MIN=1, PHI_SKETCH_WAVES=3)))
    for name, batches, e in routes:
        with env(**e):
            ctx = gpu.ctx(k=k, w=w, threshold=1.0, recombination=5)
            set_graph(ctx, g)
            for b in batches:
                ctx.add_reads(b)
            out[name] = _score_against_oracle(gpu, ctx, g, st, len(reads), sum(map(len, reads)), n_emitted)
    assert out["one_batch"] == out["three_batches"] == out["pooled"]
    return out


@case("reads")
def fixed_window_kernel(gpu):
    """150-bp reads at k = 31, w = 25, handed over without offsets: the fixed-geometry window kernel"""
    from graphgen import random_graph, walk_sequence
    from oracle import oracle as O
    rng = np.random.default_rng(52047)
    g = random_graph(rng, n_sites=10, n_walks=4, seg_len=(120, 300), alt_len=(2, 9))
    reads = []
    for i in range(47):
        s = walk_sequence(g, int(rng.integers(0, g.n_walks)))
        a = int(rng.integers(0, len(s) - 150))
        r = s[a:a + 150]
        reads.append(r.lower() if i % 3 == 1 else r)
    reads += [rseq(rng, 150) for _ in range(12)]
    bad = bytearray(reads[5]); bad[0] = ord("N"); bad[149] = ord("n"); reads[5] = bytes(bad)
    st = O.run_stage12(g, reads, 31, 25, 1.0)
    n_emitted = sum(len(O.sketch(r, 31, 25)[0]) for r in reads)
    if gpu is None:
        return None
    out = {}
    for fixed in ("1", "0"):
        with env(PHI_SKETCH_WINDOWS=1, PHI_SKETCH_WIN_FIXED=fixed):
            ctx = gpu.ctx(k=31, w=25, threshold=1.0, recombination=5)
            set_graph(ctx, g)
            ctx.add_reads(reads)                           # (one length >= 32: add_reads passes no offsets)
            out[fixed] = _score_against_oracle(gpu, ctx, g, st, len(reads), 150 * len(reads), n_emitted)
    assert out["1"] == out["0"]
    return out["1"]


@case("reads")
def novel_hash_log_spill(gpu):
    """chunk logs of four entries and an overflow list of 50: every chunk spills, the list runs full, is grown, the batch
    replayed (tests/test_gpu_ladder.py test_a_band_that_overflows_the_novel_hash_list_is_replayed, without the ladder)"""
    from graphgen import mosaic_reads, random_graph
    from oracle import oracle as O
    rng = np.random.default_rng(606)
    g = random_graph(rng, n_sites=10, n_walks=3, seg_len=(30, 60), alt_len=(2, 8))
    k, w = 15, 10
    reads = [rseq(rng, rng.integers(60, 140)) for _ in range(3000)]
    reads += mosaic_reads(rng, g, n_reads=40, read_len=60, n_seg=2)
    st = O.run_stage12(g, reads, k, w, 1.0)
    n_emitted = sum(len(O.sketch(r, k, w)[0]) for r in reads)
    assert len(st.spectrum) > 10000                            # far above what the chunk logs and a list of 50 hold
    if gpu is None:
        return None
    with env(PHI_NOV_SHIFT=2, PHI_OVLIST_CAP=50):
        ctx = gpu.ctx(k=k, w=w, threshold=1.0, recombination=3)
        set_graph(ctx, g)
        ctx.add_reads(reads)
        return _score_against_oracle(gpu, ctx, g, st, len(reads), sum(map(len, reads)), n_emitted)


# =========================================================================== solve

def _small_case(seed):
    """tests/test_gpu_parity.py test_random_small_graphs_vs_brute_force"""
    from graphgen import mosaic_reads, random_graph
    rng = np.random.default_rng(seed)
    k, w = int(rng.integers(3, 8)), int(rng.integers(1, 5))
    rep = rseq(rng, k + 3) if seed % 2 else None
    g = random_graph(rng, n_sites=int(rng.integers(3, 6)), n_walks=int(rng.integers(2, 5)), repeat=rep)
    reads = mosaic_reads(rng, g, n_reads=25, read_len=k + w + 8, n_seg=2)
    R = int(rng.choice([0, 1, 2, 3, 100]))
    T = float(rng.choice([1.0, 0.5, 2.0]))
    return FullCase(g, reads, k, w, T, R, brute=True)


@case("solve")
def small_graphs_vs_brute_force(gpu):
    out = {}
    for seed in (1, 2, 3):
        fc = _small_case(seed)
        if gpu is None:
            continue
        ctx = fc.run(gpu)
        out[f"seed{seed}"] = solve_digest(ctx, fc.check(ctx))
    return out


def _walk_lane_case():
    """tests/test_gpu_parity.py test_dp_blocks_in_parallel_equal_the_whole_chain, its seed 9 (the one of its odd seeds whose
    chain has clean cuts for blocks of three steps: the others keep the whole chain)"""
    from graphgen import mosaic_reads, random_graph
    seed = 9
    rng = np.random.default_rng(7700 + seed)
    k, w = int(rng.integers(5, 12)), int(rng.integers(1, 7))
    rep = rseq(rng, k + 4) if seed % 2 else None
    g = random_graph(rng, n_sites=int(rng.integers(30, 120)), n_walks=int(rng.integers(2, 40)), seg_len=(3, 40), alt_len=(1, 10), p_del=0.25, repeat=rep)
    reads = mosaic_reads(rng, g, n_reads=300, read_len=k + w + 30, n_seg=int(rng.integers(2, 6)), err=0.01)
    R = int(rng.choice([0, 1, 3, 10, 100]))
    return FullCase(g, reads, k, w, 1.0, R)


@case("solve")
def blocks_on_walk_lanes(gpu):
    fc = _walk_lane_case()
    assert fc.g.n_walks <= 64
    if gpu is None:
        return None
    out = {}
    for mode, e, dp_mode in (("blocks", dict(PHI_DP_BLOCK_STEPS=3), 2), ("whole", dict(PHI_DP_NOBLOCKS=1), 1)):
        with env(**e):
            ctx = fc.run(gpu, budget=64)
            res = ctx.solve()
            info = ctx.solve_stats()
        assert info["dp_mode"] == dp_mode and (info["n_blocks"] >= 2) == (mode == "blocks"), (mode, info)
        fc.evaluate(res)
        out[mode] = (res, solve_digest(ctx, res))
    a, b = out["blocks"][0], out["whole"][0]
    if a["optimal"] and b["optimal"]:
        assert a["objective"] == b["objective"]
    return {m: d for m, (_, d) in out.items()}


def _class_lane_case(n_walks, seed, params=None):
    """the sparse graphs of tests/test_gpu_parity.py test_dp_blocks_on_class_lanes_equal_the_whole_chain (few, short minimisers:
    many cuts that no anchor spans), at a number of walks of our choosing"""
    from graphgen import mosaic_reads, random_graph
    rng = np.random.default_rng(9100 + seed)
    k, w = int(rng.integers(4, 7)), int(rng.integers(14, 26))
    rng.choice([65, 70, 100, 128, 129, 200, 256])               # (the draw the test makes of its number of walks)
    rep = rseq(rng, k + 4) if seed % 2 else None
    g = random_graph(rng, n_sites=int(rng.integers(30, 90)), n_walks=n_walks, seg_len=(8, 40), alt_len=(1, 10), p_del=0.25, repeat=rep)
    if seed % 3 == 0:
        g.paths[1] = g.paths[1][: len(g.paths[1]) - 3]           # ends on an interior vertex
    reads = mosaic_reads(rng, g, n_reads=300, read_len=k + w + 30, n_seg=int(rng.integers(2, 6)), err=0.01)
    R = int(rng.choice([0, 1, 3, 10, 100]))
    if params is not None:                                       # (a context that is used again has ONE set of parameters)
        assert (k, w) == params[:2]
        R = params[2]
    return FullCase(g, reads, k, w, 1.0, R)


CLASS_LANE_SEEDS = {70: 7, 130: 4}                               # (seeds whose solves end proven optimal within the budget)
CLASS_LANE_ENV = dict(PHI_DP_BLOCK_STEPS=2, PHI_DP_STRICT=1)


def _class_lane_solve(fc, ctx, e=CLASS_LANE_ENV):
    """the blocks' rows on class lanes (the row table d_row_out): dp_mode 3, or the case did not reach what it is there for"""
    with env(**e):
        res = ctx.solve()
        info = ctx.solve_stats()
    assert info["dp_mode"] == 3 and info["n_blocks"] >= 4 and 1 <= info["max_classes"] <= 64, info
    fc.evaluate(res)
    return res


@case("solve")
def blocks_on_class_lanes(gpu):
    out = {}
    for n_walks, seed in CLASS_LANE_SEEDS.items():
        fc = _class_lane_case(n_walks, seed)
        assert fc.g.n_walks == n_walks
        if gpu is None:
            continue
        with env(**CLASS_LANE_ENV):
            ctx = fc.run(gpu, budget=32)
        a = _class_lane_solve(fc, ctx)
        with env(PHI_DP_NOBLOCKS=1):
            whole = fc.run(gpu, budget=32)
            b = whole.solve()
            assert whole.solve_stats()["dp_mode"] == 1
        fc.evaluate(b)
        if a["optimal"] and b["optimal"]:
            assert a["objective"] == b["objective"], (n_walks, a["objective"], b["objective"])
        out[f"walks{n_walks}"] = dict(blocks=solve_digest(ctx, a), whole=solve_digest(whole, b))
        if n_walks == 70:
            # the chain over the blocks cut into three segments: field for field what the one-workgroup chain gives
            with env(PHI_DP_CHAIN_SEGMENTS=3, **CLASS_LANE_ENV):
                seg = fc.run(gpu, budget=32)
                s = seg.solve()
                assert seg.solve_stats()["dp_mode"] == 3
            same_result(a, s, "chain segments")
            out["chain_segments"] = solve_digest(seg, s)
    return out


@case("solve")
def dense_dp(gpu):
    """PHI_DP_DENSE: the every-vertex kernel of dp.hip (tests/test_gpu_parity.py test_dense_and_event_dp_agree, R = 3)"""
    from graphgen import mosaic_reads, random_graph
    rng = np.random.default_rng(4242)
    g = random_graph(rng, n_sites=60, n_walks=9, seg_len=(4, 12), alt_len=(2, 6), p_del=0.25)
    reads = mosaic_reads(rng, g, n_reads=200, read_len=40, n_seg=4, err=0.01)
    fc = FullCase(g, reads, 7, 3, 0.8, 3)
    if gpu is None:
        return None
    out = {}
    for mode, e, dp_modes in (("dense", dict(PHI_DP_DENSE=1), (0,)), ("events", {}, (1, 2))):
        with env(**e):
            ctx = fc.run(gpu)
            res = fc.check(ctx)
            assert ctx.solve_stats()["dp_mode"] in dp_modes, (mode, ctx.solve_stats())
        out[mode] = (res, solve_digest(ctx, res))
    assert out["dense"][0]["objective"] == out["events"][0]["objective"]
    return {m: d for m, (_, d) in out.items()}


# =========================================================================== text

def _reads_text(rng, n, fastq):
    recs = []
    for i, L in enumerate(rng.integers(20, 160, size=n).tolist()):
        s = rseq(rng, L, b"ACGTacgtN")
        recs.append(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * L) if fastq else b">r%d some text\n%s\n" % (i, s))
    return b"".join(recs)


def _records(bases, off):
    raw = bytes(bases)
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _toy_graph():
    from oracle import oracle as O
    return O.parse_gfa(os.path.join(DATA, "test.gfa"))


@case("text")
def reads_as_text(gpu):
    """FASTA and FASTQ text split into records on the device (reads_text.hip) against the host reader; the counters against
    the oracle's sketch of the host reader's records"""
    from oracle import oracle as O
    from phi_amd import ilp_index as HR
    g = _toy_graph()
    out = {}
    for fastq in (False, True):
        rng = np.random.default_rng(31 + fastq)
        text = _reads_text(rng, 120, fastq)
        want = _records(*HR.reads_of_text(text))
        assert len(want) == 120
        sk = [O.sketch(r, 3, 2)[0] for r in want]
        if gpu is None:
            continue
        ctx = gpu.ctx(k=3, w=2, threshold=1.0, recombination=100)
        set_graph(ctx, g)
        ctx.reads_text_begin(4096)
        got = []
        for i in range(0, len(text), 3000):
            assert not ctx.add_reads_text(text[i:i + 3000])
            got += _records(*ctx.reads_text_last_batch())
        pending, taken = ctx.reads_text_end()
        assert taken + len(pending) == len(text)
        tail = _records(*HR.reads_of_text(pending, [], stream_offset=taken))
        assert got + tail == want and len(got) >= len(want) - 1
        if tail:
            ctx.add_reads(tail)
        rs = ctx.reads_stats()
        assert rs["n_reads"] == len(want) and rs["n_bases"] == sum(map(len, want))
        assert rs["n_emitted"] == sum(map(len, sk)) and rs["n_distinct"] == len(np.unique(np.concatenate(sk)))
        out["fastq" if fastq else "fasta"] = dict(D(rs), records=H(got), pending=H(pending), taken=taken)
    return out


@case("text")
def parked_text(gpu):
    """two pieces of unequal size through a text park: the second takes the buffer the first left behind"""
    from oracle import oracle as O
    from phi_amd import ilp_index as HR
    g = _toy_graph()
    rng = np.random.default_rng(77)
    text = _reads_text(rng, 90, True)
    cut = text.find(b"\n@", 2 * len(text) // 3) + 1
    pieces = [text[:cut], text[cut:]]
    want = _records(*HR.reads_of_text(text))
    sk = [O.sketch(r, 3, 2)[0] for r in want]
    assert len(pieces[0]) > len(pieces[1]) + 64 > 64
    if gpu is None:
        return None
    park = gpu.phi.TextPark(0)
    try:
        ctx = gpu.ctx(k=3, w=2, threshold=1.0, recombination=100)
        set_graph(ctx, g)
        ctx.reads_text_begin(len(pieces[0]))
        got = []
        for piece in pieces:
            idx = park.add(piece)
            assert park.fetch(idx) == piece
            assert not ctx.add_reads_text_parked(park, idx)
            got += _records(*ctx.reads_text_last_batch())
            park.release(idx)
        pending, taken = ctx.reads_text_end()
        assert pending == b"" and taken == len(text) and got == want
        rs = ctx.reads_stats()
        assert rs["n_emitted"] == sum(map(len, sk)) and rs["n_distinct"] == len(np.unique(np.concatenate(sk)))
    finally:
        park.close()
    return dict(D(rs), records=H(got))


def _text_graph():
    from graphgen import mosaic_reads, random_graph
    rng = np.random.default_rng(2024)
    g = random_graph(rng, n_sites=100, n_walks=6, seg_len=(8, 30), alt_len=(1, 6))
    reads = mosaic_reads(rng, g, n_reads=80, read_len=40, n_seg=3, err=0.01)
    return g, reads


def _same_host_graph(g, want):
    assert g.hap_id2name == want.hap_id2name
    for f in ("seq_off", "adj_off", "adj", "top_order_map", "walk_off"):
        assert np.array_equal(getattr(g, f), getattr(want, f)), f
    assert bytes(g.seq_concat) == bytes(want.seq_concat)


@case("text")
def walks_from_text(gpu):
    """the W-lines of a small GFA resolved on the device (walk_text.hip), from plain text and from a gzip file inflated and
    split on the device (inflate.hip, gfa_text.hip): the host reader's graph, and the solve of the same graph set from arrays"""
    from phi_amd import ilp_index as HR
    g, reads = _text_graph()
    fc = FullCase(g, reads, 7, 4, 1.0, 4)
    plain = write_gfa(g, os.path.join(tmpdir(), "walks.gfa"))
    zipped = write_gfa(g, os.path.join(tmpdir(), "walks.gfa.gz"))
    want = HR.Graph(plain)
    assert np.array_equal(want.walk_vtx, g.arrays()["walk_vtx"]) and 2000 < os.path.getsize(zipped) < 20000
    if gpu is None:
        return None
    arrays = fc.run(gpu)
    res_arrays = fc.check(arrays)
    out = {}
    for route in ("text", "gzip"):
        ctx = fc.context(gpu)
        if route == "text":
            dg = HR.DeferredGraph(plain)
            assert dg.resolve_on_device(ctx)
        else:
            dg = HR.DeferredGraph.from_gzip_on_device(zipped, ctx)
            assert dg.route == "device" and dg.split_info["n_walks"] == want.num_walks
        assert dg.walk_vtx is None
        _same_host_graph(dg, want)
        entries = ctx.walk_entries()
        assert np.array_equal(entries, want.walk_vtx)
        dg.set_graph(ctx)
        ctx.add_reads(reads)
        res = fc.check(ctx)
        same_result(res, res_arrays, route)
        out[route] = dict(D(res), entries=H(entries), walk_off=H(np.asarray(dg.walk_off)))
    return out


@case("text")
def gzip_reads(gpu):
    """a gzip reads file through the device inflater, whole and as parked pieces, against zlib"""
    rng = np.random.default_rng(5)
    text = _reads_text(rng, 400, True)
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    comp = c.compress(text) + c.flush()
    assert gzip.decompress(comp) == text
    if gpu is None:
        return None
    out = {}
    for chunk in (0, 4096):
        got, info = gpu.phi.inflate(comp, chunk_bytes=chunk)
        assert got == text and info["out_bytes"] == len(text) and info["members"] == 1
        out[f"chunk{chunk}"] = dict(D(info), text=H(got))
    park = gpu.phi.TextPark(0)
    try:
        idx, info = park.add_gzip([comp[:1], comp[1:3000], comp[3000:]], 16384)
        pieces = [park.fetch(i) for i in idx]
        assert b"".join(pieces) == text and max(map(len, pieces)) <= 16384 and len(idx) == -(-len(text) // 16384)
        out["parked"] = dict(D(info), pieces=H(pieces))
    finally:
        park.close()
    return out


# =========================================================================== graphs

def _chop_case():
    """tests/test_gpu_chop.py _graph_and_reads(2, 9, 6): long segments, deletions, lower case and N in segments"""
    from graphgen import mosaic_reads, random_graph
    rng = np.random.default_rng(100 * 2 + 7)
    g = random_graph(rng, n_sites=6, n_walks=9, seg_len=(1, 400), alt_len=(1, 40), p_del=0.3)
    for v in rng.choice(g.n_vtx, size=max(2, g.n_vtx // 5), replace=False).tolist():
        s = bytearray(g.node_seq[v])
        if len(s) > 3 and v % 2:
            s[len(s) // 2] = ord("N")
            g.node_seq[v] = bytes(s)
        else:
            g.node_seq[v] = bytes(s).lower()
    return g, mosaic_reads(rng, g, n_reads=60, read_len=70, n_seg=2, err=0.01)


def _chop_check(ctx, g, c, ov, oo, woff, res, N):
    assert np.array_equal(woff, c.arrays()["walk_off"])
    assert np.array_equal(ctx.walk_entries(), c.arrays()["walk_vtx"])
    got_v, got_o = ctx.chop_origin(res["path_vtx"])
    assert np.array_equal(got_v, ov[res["path_vtx"]]) and np.array_equal(got_o, oo[res["path_vtx"]])
    cs = ctx.chop_stats()
    assert (cs["n_vtx_in"], cs["n_vtx_out"], cs["max_len"]) == (g.n_vtx, c.n_vtx, N) and c.n_vtx > g.n_vtx
    assert (cs["n_entries_in"], cs["n_entries_out"]) == (sum(len(p) for p in g.paths), sum(len(p) for p in c.paths))
    return dict(D(res), woff=H(woff), origin=H([got_v, got_o]), chop=D(cs))


@case("graphs")
def chop(gpu):
    """set_graph(chop=N) against the numpy rule and the oracle on the chopped graph"""
    from test_cpu_chop import chop_numpy
    g, reads = _chop_case()
    out = {}
    for N in (7, 30):
        c, ov, oo = chop_numpy(g, N)
        fc = FullCase(c, reads, 9, 4, 1.0, 3)
        if gpu is None:
            continue
        ctx = fc.context(gpu)
        woff = set_graph(ctx, g, chop=N)
        ctx.add_reads(reads)
        out[f"N{N}"] = _chop_check(ctx, g, c, ov, oo, woff, fc.check(ctx), N)
    return out


def _python_vcf_graph(vcf, fa, name, max_len=30):
    """the Python route: vcf2gfa to a GFA file, the host reader over it (tests/test_gpu_vcf.py _python_graph)"""
    from phi_amd import ilp_index as HR
    from phi_amd import vcf2gfa
    old = vcf2gfa.CHOP
    vcf2gfa.CHOP = max_len
    try:
        _, ref_seq = vcf2gfa.read_fasta_single(fa)
        ref_seq = ref_seq.upper()
        samples, recs, ploidy = vcf2gfa.read_vcf(vcf, ref_seq, warn=lambda m: None)
        segs, links, walks = vcf2gfa.build(ref_seq, samples, recs, ploidy)
    finally:
        vcf2gfa.CHOP = old
    p = os.path.join(tmpdir(), name)
    with open(p, "wb") as f:
        vcf2gfa.write_gfa(f, "REF#0", segs, links, walks)
    return HR.Graph(p)


def _vcf_check(ctx, v, g):
    for f in ("seq_off", "seq_concat", "adj_off", "adj", "walk_off", "top_order_map"):
        assert np.array_equal(getattr(v, f), getattr(g, f)), f
    assert v.hap_id2name == g.hap_id2name
    entries = ctx.walk_entries()
    assert np.array_equal(entries, g.walk_vtx)
    st = v.stats
    assert st["n_entries"] == len(g.walk_vtx) and st["n_units"] == v.n_units and st["n_records"] > 0
    return dict(entries=H(entries), walk_off=H(np.asarray(v.walk_off)), stats=D(st))


GOLDEN_VCF = (os.path.join(DATA, "MHC_4.vcf.gz"), os.path.join(DATA, "MHC-CHM13.0.fa.gz"))


@case("vcf")
def vcf(gpu):
    """set_graph_vcf on the golden VCF (genotypes and walks on the device, vcf.hip) against vcf2gfa.py + the host reader"""
    g = _python_vcf_graph(*GOLDEN_VCF, "mhc4.gfa")
    assert g.num_walks == 5
    if gpu is None:
        return None
    ctx = gpu.ctx()
    ctx.set_params()
    v = ctx.set_graph_vcf(*GOLDEN_VCF)
    assert v.hap_id2name == ["REF.0", "HG002.1", "HG002.2", "HG005.1", "HG005.2"]
    return _vcf_check(ctx, v, g)


def _shared_walks_case():
    from graphgen import random_graph, walk_sequence
    rng = np.random.default_rng(808)
    g = random_graph(rng, n_sites=10, n_walks=12, seg_len=(6, 40), alt_len=(1, 8), p_del=0.2)
    return g, [walk_sequence(g, h) for h in range(g.n_walks)]


@case("graphs")
def class_tables(gpu):
    """walks that share most of their entries: the classes of contexts.hip; every walk's minimisers against the oracle's
    sketch of its sequence"""
    from oracle import oracle as O
    g, seqs = _shared_walks_case()
    out = {}
    for k, w in ((7, 4), (31, 25)):
        want = [O.sketch(s, k, w) for s in seqs]
        assert sum(len(h) for h, _ in want) > 0
        if gpu is None:
            continue
        ctx = gpu.ctx(k=k, w=w, threshold=1.0, recombination=3)
        set_graph(ctx, g)
        info = ctx.index_stats()
        assert info["n_entries"] == sum(len(p) for p in g.paths) and 0 < info["n_classes"] < info["n_entries"], info
        got = []
        for h in range(g.n_walks):
            gh, gp = ctx.walk_minimizers(h)
            assert np.array_equal(gh, want[h][0]) and np.array_equal(gp, want[h][1]), (k, w, h)
            got += [gh, gp]
        out[f"k{k}w{w}"] = dict(D(info), minimizers=H(got))
    return out


# =========================================================================== edit

EDIT_LENGTHS = [0, 1, 63, 64, 65, 4096, 4097]
_REFS = {}


def _edit_refs():
    if not _REFS:
        from test_cpu_edit_alignment import build_align_reference
        from test_cpu_edit_distance import build_reference
        _REFS["ond"] = build_reference(tmpdir())
        _REFS["align"] = build_align_reference(tmpdir())
    return _REFS["ond"], _REFS["align"]


def _edit_grid(seed=1):
    from test_cpu_edit_distance import mutate
    rng = random.Random(seed)
    base = bytes(b"ACGT"[rng.randrange(4)] for _ in range(4200))
    pairs = []
    for la in EDIT_LENGTHS:
        for lb in EDIT_LENGTHS:
            b = mutate(rng, base[:lb], min(lb, 40))[:lb] if lb else b""
            pairs.append((base[:la], b))
    return pairs


def _edit_check(ctx, pairs, want_d, want_a):
    a_list, b_list = [a for a, _ in pairs], [b for _, b in pairs]
    got = ctx.edit_distances(a_list, b_list)
    assert got.dtype == np.int64 and got.tolist() == want_d
    al = ctx.edit_alignments(a_list, b_list)
    for q, (m, x, i, d, cost, cig) in enumerate(want_a):
        assert al.cigar[q] == cig and tuple(al.counts[q]) == (m, x, i, d) and al.distance[q] == cost, (q, len(pairs[q][0]), len(pairs[q][1]))
    return dict(distances=H(got), counts=H(al.counts), cigars=H([c.encode() for c in al.cigar]))


@case("edit")
def edge_length_grid(gpu):
    ond, align = _edit_refs()
    pairs = _edit_grid()
    want_d = [ond(a, b) for a, b in pairs]
    want_a = [align(a, b) for a, b in pairs]
    assert [t[4] for t in want_a] == want_d and len(pairs) == 49
    if gpu is None:
        return None
    return _edit_check(gpu.ctx(), pairs, want_d, want_a)


@case("edit")
def long_pair(gpu):
    """50 kbp with 300 edits: several stripes, band doublings; max_distance at d and d - 1"""
    from test_cpu_edit_distance import mutate
    ond, align = _edit_refs()
    rng = random.Random(23)
    a = bytes(b"ACGT"[rng.randrange(4)] for _ in range(50_000))
    b = mutate(rng, a, 300)
    d = ond(a, b)
    want = align(a, b, d)
    assert 64 < d <= 300 and want[4] == d and ond(a, b, d - 1) == -1
    if gpu is None:
        return None
    ctx = gpu.ctx()
    out = _edit_check(ctx, [(a, b)], [d], [want])
    capped = [int(ctx.edit_distances([a], [b], max_distance=m)[0]) for m in (d, d - 1)]
    assert capped == [d, -1]
    return dict(out, d=d, capped=H(capped))


# =========================================================================== ladder

def _ladder_graph():
    """tests/test_gpu_ladder.py small_ctx"""
    from graphgen import random_graph
    return random_graph(np.random.default_rng(11), n_sites=6, n_walks=3, seg_len=(8, 20), alt_len=(1, 4))


def _ladder_reads(rng, lens):
    return [rseq(rng, n, b"ACGTN") for n in lens]


def _partition_inputs(n, one_length):
    rng = np.random.default_rng((200 if one_length else 100) + n)
    if one_length:
        return _ladder_reads(rng, [150] * n), 5, [i / 16 for i in range(1, 17)]
    lens = rng.choice([0, 1, 15, 16, 17, 150], size=n)
    lens[n // 3] = 5000                                      # one long read
    return _ladder_reads(rng, lens), n, [0.0, 0.3, 0.3, 1.0]


def _partition(ctx, reads, seed, fractions):
    """tests/test_gpu_ladder.py _check_partition compares every band with the rule of phi_amd/ladder.py; the digest: what the
    device holds of every band"""
    from test_gpu_ladder import _check_partition
    info, band = _check_partition(ctx, [reads], seed, fractions)
    bands = [ctx.ladder_band(j, data=True) for j in range(len(fractions))]
    return info, dict(D(info), bands=H([list(b) for b in bands]))


@case("ladder")
def partition(gpu):
    from phi_amd import ladder as rule
    g = _ladder_graph()
    out = {}
    if gpu is not None:
        ctx = gpu.ctx(k=7, w=4, threshold=1.0, recombination=3)
        set_graph(ctx, g)
    for n, one_length in ((65, False), (257, False), (65, True)):
        reads, seed, fractions = _partition_inputs(n, one_length)
        band = rule.bands(seed, np.arange(n, dtype=np.uint64), fractions)
        assert len(band) == n and band.max() <= len(fractions)
        if gpu is None:
            continue
        info, out[f"n{n}" + ("_one_length" if one_length else "")] = _partition(ctx, reads, seed, fractions)
        assert info["one_length"] == (150 if one_length else 0) and info["n_levels"] == len(fractions)
    return out


@case("ladder")
def level_state(gpu):
    """tests/test_gpu_ladder.py test_level_state_equals_a_fresh_context at (7, 4): after ladder_advance(j) the read state and
    the solve are those of a fresh context given the rule's level-j reads; the oracle on those reads gives the counters"""
    from graphgen import mosaic_reads, random_graph
    from oracle import oracle as O
    from phi_amd import ladder as rule
    k, w = 7, 4
    rng = np.random.default_rng(1000 + k)
    g = random_graph(rng, n_sites=int(rng.integers(10, 40)), n_walks=4, seg_len=(4, 30), alt_len=(1, 8), p_del=0.2)
    reads = mosaic_reads(rng, g, n_reads=300, read_len=40, n_seg=3, err=0.02)
    reads += [rseq(rng, 200, b"ACGTN") for _ in range(3)]
    fractions, seed = [0.1, 0.35, 0.7, 1.0], 42
    band = rule.bands(seed, np.arange(len(reads)), fractions)
    assert 0 < (band == 0).sum() and (band <= 3).all()
    levels = [[reads[i] for i in np.flatnonzero(band <= j)] for j in range(4)]
    sts = [O.run_stage12(g, lv, k, w, 1.0) for lv in levels]
    if gpu is None:
        return None
    from test_gpu_ladder import _same_state
    ctx = gpu.ctx(k=k, w=w, threshold=1.0, recombination=5)
    set_graph(ctx, g)
    ctx.collect_begin()
    ctx.add_reads(reads[:100])
    ctx.add_reads(reads[100:])
    ctx.collect_end()
    info = ctx.ladder_plan(seed, fractions)
    assert info["one_length"] == 0 and info["band_reads"] == [int((band == j).sum()) for j in range(4)]
    ctx.reset_reads()
    out, want = {}, []
    for j in range(4):
        fresh = gpu.ctx(k=k, w=w, threshold=1.0, recombination=5)
        set_graph(fresh, g)
        fresh.add_reads([levels[j][i] for i in rng.permutation(len(levels[j]))])
        want.append((fresh.reads_stats(), fresh.solve()))
        fresh.close()
        ctx.ladder_advance(j)
        rs, res = ctx.reads_stats(), ctx.solve()
        _same_state(rs, res, *want[j])
        assert (res["spectrum_size"], res["filtered"], res["n_in_model"]) == (len(sts[j].spectrum), sts[j].filtered, sts[j].n_in_model)
        assert np.array_equal(res["n_anchors"], sts[j].n_anchors)
        out[f"level{j}"] = dict(D(rs), **D(res))
    ctx.reset_reads()                                            # a rewind keeps the plan
    ctx.ladder_advance(2)
    _same_state(ctx.reads_stats(), ctx.solve(), *want[2])
    return out


# =========================================================================== reuse

REUSE = dict(k=4, w=16, T=1.0, R=100)                          # phi_set_params precedes the first phi_set_graph: one set per context


def _many_walks_case(n_walks):
    """the graphs of tests/test_gpu_parity.py test_more_than_64_walks_vs_highs"""
    from graphgen import mosaic_reads, random_graph
    rng = np.random.default_rng(1000 + n_walks)
    g = random_graph(rng, n_sites=8, n_walks=n_walks, seg_len=(6, 12), alt_len=(2, 5), p_del=0.3)
    reads = mosaic_reads(rng, g, n_reads=60, read_len=28, n_seg=4)
    return FullCase(g, reads, **REUSE)


def _truncated_vcf(n_records):
    """the first records of the golden VCF, and the reference up to a little behind the last of them"""
    from phi_amd import vcf2gfa
    vcf, fa = os.path.join(tmpdir(), "head.vcf"), os.path.join(tmpdir(), "head.fa")
    kept, last = 0, 0
    with gzip.open(GOLDEN_VCF[0], "rb") as f, open(vcf, "wb") as out:
        for line in f:
            out.write(line)
            if not line.startswith(b"#"):
                kept += 1
                last = int(line.split(b"\t", 2)[1])
            if kept >= n_records:
                break
    name, seq = vcf2gfa.read_fasta_single(GOLDEN_VCF[1])
    seq = seq[:last + 2000]
    name = name if isinstance(name, bytes) else name.encode()
    seq = seq if isinstance(seq, bytes) else seq.encode()
    with open(fa, "wb") as out:
        out.write(b">" + name + b"\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")
    return vcf, fa


@case("reuse")
def one_context_used_again(gpu):
    """Buffers a context keeps (phi_dev_ensure returns at once when the buffer is large enough): on ONE context, a second
    input after a different one, each equal -- field for field -- to the same input on a fresh context, which is checked
    against its CPU reference"""
    from phi_amd import ladder as rule
    from test_cpu_chop import chop_numpy
    big, small = _many_walks_case(130), _many_walks_case(20)
    cl70, cl130 = (_class_lane_case(n, 7, (REUSE["k"], REUSE["w"], REUSE["R"])) for n in (70, 130))
    ond, align = _edit_refs()
    grid = _edit_grid(2)
    edits_big = [p for p in grid if max(len(p[0]), len(p[1])) >= 4096][:6]
    edits_small = [p for p in grid if 0 < max(len(p[0]), len(p[1])) <= 65][:9]
    want_edits = [([ond(a, b) for a, b in ps], [align(a, b) for a, b in ps]) for ps in (edits_big, edits_small)]
    lg = _ladder_graph()
    l1000, seed1000, fr1000 = _partition_inputs(1000, False)
    l65, seed65, fr65 = _partition_inputs(65, False)
    assert len(rule.bands(seed65, np.arange(65, dtype=np.uint64), fr65)) == 65
    cg, creads = _chop_case()
    chopped, ov, oo = chop_numpy(cg, 7)
    fc_chopped, fc_plain = FullCase(chopped, creads, **REUSE), FullCase(cg, creads, **REUSE)
    head = _truncated_vcf(300)
    vg = _python_vcf_graph(*head, "head.gfa")
    tg, treads = _text_graph()
    fc_arrays = FullCase(tg, treads, **REUSE)
    if gpu is None:
        return None
    out = {}
    params = dict(k=REUSE["k"], w=REUSE["w"], threshold=REUSE["T"], recombination=REUSE["R"])
    used = gpu.ctx(**params)

    def on_used(fc, budget=4096):
        assert (fc.k, fc.w, fc.T, fc.R) == tuple(REUSE.values())
        used.set_solve_budget(budget)
        set_graph(used, fc.g)
        used.add_reads(fc.reads)
        return used

    # a larger solve, then a smaller one with fewer walks
    on_used(big).solve()
    fresh = small.run(gpu)
    want = small.check(fresh)
    got = on_used(small).solve()
    same_result(got, want, "130 -> 20 walks")
    assert used.solve_stats() == fresh.solve_stats()
    out["solve_130_then_20"] = solve_digest(used, got)

    # a small class-lane case in blocks of four steps, then a larger one in blocks of two: the row table (a row of 64 lanes
    # per block and class lane) grows with the number of blocks
    _class_lane_solve(cl70, on_used(cl70, 32), dict(PHI_DP_BLOCK_STEPS=4))
    n_blocks_before = used.solve_stats()["n_blocks"]
    fresh = cl130.run(gpu, budget=32)
    want = _class_lane_solve(cl130, fresh)
    got = _class_lane_solve(cl130, on_used(cl130, 32))
    same_result(got, want, "70 -> 130 walks on class lanes")
    assert used.solve_stats() == fresh.solve_stats() and used.solve_stats()["n_blocks"] > n_blocks_before
    out["class_lanes_70_then_130"] = solve_digest(used, got)
    used.set_solve_budget(4096)

    # a larger, then a smaller batch of alignments
    _edit_check(used, edits_big, *want_edits[0])
    want = _edit_check(gpu.ctx(), edits_small, *want_edits[1])
    got = _edit_check(used, edits_small, *want_edits[1])
    assert got == want
    out["edit_large_then_small"] = got

    # a ladder over 1000 reads, then over 65 on a new store
    set_graph(used, lg)
    _partition(used, l1000, seed1000, fr1000)
    fresh = gpu.ctx(**params)
    set_graph(fresh, lg)
    _, want = _partition(fresh, l65, seed65, fr65)
    used.reset_reads()
    _, got = _partition(used, l65, seed65, fr65)
    assert got == want
    out["ladder_1000_then_65"] = got
    used.reset_reads()

    # a chopped graph, then the same graph as it is
    woff = set_graph(used, cg, chop=7)
    used.add_reads(creads)
    _chop_check(used, cg, chopped, ov, oo, woff, fc_chopped.check(used), 7)
    fresh = fc_plain.run(gpu)
    want = fc_plain.check(fresh)
    got = on_used(fc_plain).solve()
    same_result(got, want, "chop -> plain")
    assert np.array_equal(used.walk_entries(), fresh.walk_entries())
    out["chop_then_plain"] = solve_digest(used, got)

    # a graph from a VCF, then one from arrays
    v = used.set_graph_vcf(*head)
    _vcf_check(used, v, vg)
    fresh = fc_arrays.run(gpu)
    want = fc_arrays.check(fresh)
    got = on_used(fc_arrays).solve()
    same_result(got, want, "vcf -> arrays")
    for h in range(tg.n_walks):
        for x, y in zip(used.walk_minimizers(h), fresh.walk_minimizers(h)):
            assert np.array_equal(x, y), h
    out["vcf_then_arrays"] = solve_digest(used, got)
    return out


# --------------------------------------------------------------------------- main

def poison_is_on(gpu):
    """A poisoned run that did not poison must not count as a pass: the hit vector of a small graph is allocated at the
    least size of a device buffer (256 bytes) and zeroed over its own few bytes only, so on a fresh context the rest of it
    still holds what the allocation held -- the byte of PHI_DEVICE_POISON, when that is set."""
    ctx = gpu.ctx(k=3, w=2, threshold=1.0, recombination=100)
    set_graph(ctx, _toy_graph())
    p, n = ctx.hits_buffer()
    assert 0 < n <= 128, n
    raw = gpu.device_u8(p, 256)
    assert not raw[:n].any()
    byte = os.environ.get("PHI_DEVICE_POISON")
    if byte is not None:
        assert (raw[192:] == int(byte, 0)).all(), (byte, raw.tolist())
    gpu.close_all()


def flat(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(flat(v, f"{prefix}{k}."))
        else:
            out[prefix + k] = v
    return out


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    reference_only = "--reference-only" in argv
    if len(args) != 1 or (args[0] != "all" and args[0] not in GROUPS):
        print(f"usage: dirty_battery.py ({' | '.join(GROUPS)} | all) [--reference-only]", file=sys.stderr)
        return 2
    groups = list(GROUPS) if args[0] == "all" else args
    gpu = None if reference_only else Gpu()
    if gpu is not None:
        poison_is_on(gpu)
    digest, failed = {}, []
    for group in groups:
        for name, fn in GROUPS[group]:
            t0 = time.perf_counter()
            try:
                d = fn(gpu)
                digest[f"{group}.{name}"] = flat(d) if d else {}
                assert reference_only or digest[f"{group}.{name}"], "a case without a digest"
            except AssertionError:
                traceback.print_exc()
                failed.append(f"{group}.{name}")
            finally:
                if gpu is not None:
                    gpu.close_all()
                print(f"[dirty_battery] {group}.{name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)
    for k in flat(digest):
        assert not k.endswith("_ms"), k
    if failed:
        print("FAILED:", " ".join(failed), file=sys.stderr)
    print(json.dumps(digest, sort_keys=True), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
