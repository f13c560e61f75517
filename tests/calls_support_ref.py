"""The rule of phi_calls_support (include/phi_amd.h) restated in plain Python: what the device's four arrays are compared
with, element for element (test infrastructure; the product never imports it).

Occurrences come from the CPU oracle's sketch of the walk sequences, the read spectrum is the set of its hashes over the
upper-cased reads.  support_ref is the rule as it reads, call by call and occurrence by occurrence; support_ref_numpy counts the
same intervals with two searches per call, for MHC_4."""
import numpy as np


def walk_bases(walk, node_len):
    """B(t): bases of the walk before its entry t, for t = 0 .. len(walk)."""
    b = np.zeros(len(walk) + 1, np.int64)
    np.cumsum([node_len[v] for v in walk], out=b[1:])
    return b


def anchors(query, ref):
    """Per call (rule 3 of the calls) the anchors' query indices i < i2 and indices on the reference walk p < p2."""
    pos_of = {int(v): p for p, v in enumerate(ref)}
    shared = [i for i, v in enumerate(query) if int(v) in pos_of]
    out = []
    for i, i2 in zip(shared, shared[1:]):
        p, p2 = pos_of[int(query[i])], pos_of[int(query[i2])]
        if not (i2 == i + 1 and p2 == p + 1):
            out.append((i, i2, p, p2))
    return out


def spectrum_of(oracle, reads, k, w):
    """The hashes the reads emit (upper-cased, as the read kernels take them)."""
    s = set()
    for r in reads:
        s.update(int(h) for h in oracle.sketch(bytes(r).upper(), k, w)[0])
    return s


def query_occurrences(where, minimizers, bases_of):
    """Rule 1.  where[j] = (walk h_j, entry t_j) of query index j; minimizers(h) = M(h) as (hash[], pos[]); bases_of(h) =
    B_h.  The occurrences of the query as a list of (x, hash) in query coordinates, and Q."""
    q = np.zeros(len(where) + 1, np.int64)
    occ = []
    for j, (h, t) in enumerate(where):
        b = bases_of(h)
        lo, hi = int(b[t]), int(b[t + 1])
        q[j + 1] = q[j] + (hi - lo)
        hs, ps = minimizers(h)
        for hh, p in zip(hs.tolist(), ps.tolist()):
            if lo <= p < hi:                               # the occurrence lies in entry t_j
                occ.append((int(q[j]) + (p - lo), hh))
    return occ, q


def _count(occ, a0, a1, k, spectrum):
    n = hit = 0
    for x, h in occ:
        if x < a1 and x + k > a0:                          # rule 3
            n += 1
            hit += h in spectrum
    return hit, n


def support_ref(k, q_occ, q_base, r_occ, r_base, calls, spectrum):
    """Rules 3 and 4.  q_occ, r_occ: (x, hash) lists; calls: anchors().  A dict of the four int32 arrays and their totals."""
    out = {n: np.zeros(len(calls), np.int32) for n in ("alt_hit", "alt_n", "ref_hit", "ref_n")}
    for c, (i, i2, p, p2) in enumerate(calls):
        out["alt_hit"][c], out["alt_n"][c] = _count(q_occ, int(q_base[i + 1]), int(q_base[i2]), k, spectrum)
        out["ref_hit"][c], out["ref_n"][c] = _count(r_occ, int(r_base[p + 1]), int(r_base[p2]), k, spectrum)
    return _with_totals(out)


def _with_totals(out):
    for n in ("alt_hit", "alt_n", "ref_hit", "ref_n"):
        out[n + "_total"] = int(out[n].sum(dtype=np.int64))
    return out


def walk_support_ref(oracle, g, q, r, k, w, spectrum):
    """phi_calls_walk(q, r) on an oracle-style graph g: M(walk) as it stands."""
    lens = [len(s) for s in g.node_seq]
    occ = {}
    for h in {q, r}:
        hs, ps = oracle.sketch(b"".join(g.node_seq[v] for v in g.paths[h]), k, w)
        occ[h] = list(zip(ps.tolist(), hs.tolist()))
    return support_ref(k, occ[q], walk_bases(g.paths[q], lens), occ[r], walk_bases(g.paths[r], lens), anchors(g.paths[q], g.paths[r]), spectrum)


def path_support_ref(oracle, g, path_vtx, path_hap, r, k, w, spectrum):
    """phi_calls_path(r): query index j sits on walk path_hap[j] at the entry that holds path_vtx[j] (which must lie there)."""
    lens = [len(s) for s in g.node_seq]
    where = []
    for v, h in zip(path_vtx, path_hap):
        assert int(v) in g.paths[int(h)], (v, h)
        where.append((int(h), g.paths[int(h)].index(int(v))))
    sk, bs = {}, {}

    def minimizers(h):
        if h not in sk:
            sk[h] = oracle.sketch(b"".join(g.node_seq[v] for v in g.paths[h]), k, w)
        return sk[h]

    def bases_of(h):
        if h not in bs:
            bs[h] = walk_bases(g.paths[h], lens)
        return bs[h]
    q_occ, q_base = query_occurrences(where, minimizers, bases_of)
    hs, ps = minimizers(r)
    return support_ref(k, q_occ, q_base, list(zip(ps.tolist(), hs.tolist())), bases_of(r), anchors([int(v) for v in path_vtx], g.paths[r]), spectrum)


def support_ref_numpy(k, q_hash, q_pos, q_base, r_hash, r_pos, r_base, calls, spectrum):
    """The same counts for a walk query of 10^5 entries: positions ascend, so the witnesses of an interval are a range."""
    spec = spectrum if isinstance(spectrum, np.ndarray) else np.array(sorted(spectrum), np.uint64)
    c = np.asarray(calls, np.int64).reshape(-1, 4)
    out = {}
    for side, hs, ps, base, lo, hi in (("alt", q_hash, q_pos, q_base, c[:, 0], c[:, 1]), ("ref", r_hash, r_pos, r_base, c[:, 2], c[:, 3])):
        ps = np.asarray(ps, np.int64)
        assert np.all(np.diff(ps) >= 0)
        seen = np.concatenate([[0], np.cumsum(np.isin(np.asarray(hs, np.uint64), spec))])
        a0, a1 = base[lo + 1], base[hi]
        first = np.searchsorted(ps, a0 - k, side="right")  # x + k > a0
        last = np.searchsorted(ps, a1, side="left")        # x < a1
        out[side + "_n"] = (last - first).astype(np.int32)
        out[side + "_hit"] = (seen[last] - seen[first]).astype(np.int32)
    return _with_totals(out)


def anchors_numpy(query, ref, n_vtx):
    """anchors() over int arrays, as an int64 array [n_calls, 4]."""
    query, ref = np.asarray(query, np.int64), np.asarray(ref, np.int64)
    pos_of = np.full(n_vtx, -1, np.int64)
    pos_of[ref] = np.arange(len(ref))
    sh = np.flatnonzero(pos_of[query] >= 0)
    i, i2 = sh[:-1], sh[1:]
    p, p2 = pos_of[query[i]], pos_of[query[i2]]
    is_call = ~((i2 == i + 1) & (p2 == p + 1))
    return np.stack([i[is_call], i2[is_call], p[is_call], p2[is_call]], axis=1)


def path_support_ref_numpy(k, path_vtx, path_hap, walks, vlen, minimizers, r, spectrum=None):
    """phi_calls_path(r) over flat arrays: walks[h] the vertices of walk h, vlen the vertices' lengths, minimizers(h) = M(h) as
    (hash[], pos[]).  Rule 1 walk by walk: every occurrence finds its entry, the entry its query index (-1: not on the path).
    spectrum None: the witnesses alone."""
    path_vtx, path_hap = np.asarray(path_vtx, np.int64), np.asarray(path_hap, np.int64)
    q_base = np.concatenate([[0], np.cumsum(vlen[path_vtx])]).astype(np.int64)
    n_vtx = len(vlen)
    xs, hs = [], []
    for h in np.unique(path_hap):
        wv = np.asarray(walks[h], np.int64)
        base = np.concatenate([[0], np.cumsum(vlen[wv])]).astype(np.int64)
        entry_of = np.full(n_vtx, -1, np.int64)
        entry_of[wv] = np.arange(len(wv))
        js = np.flatnonzero(path_hap == h)
        assert np.all(entry_of[path_vtx[js]] >= 0)         # the path's vertices lie on the walk they are labelled with
        j_of = np.full(len(wv), -1, np.int64)
        j_of[entry_of[path_vtx[js]]] = js
        hh, pos = minimizers(int(h))
        pos = np.asarray(pos, np.int64)
        ent = np.searchsorted(base, pos, side="right") - 1
        j = j_of[ent]
        on = j >= 0
        xs.append(q_base[j[on]] + (pos[on] - base[ent[on]]))
        hs.append(np.asarray(hh, np.uint64)[on])
    x, hq = np.concatenate(xs), np.concatenate(hs)
    order = np.argsort(x, kind="stable")
    rv = np.asarray(walks[r], np.int64)
    r_base = np.concatenate([[0], np.cumsum(vlen[rv])]).astype(np.int64)
    rh, rp = minimizers(int(r))
    return support_ref_numpy(k, hq[order], x[order], q_base, rh, rp, r_base, anchors_numpy(path_vtx, rv, n_vtx),
                             np.zeros(0, np.uint64) if spectrum is None else spectrum)


# ---------------------------------------------------------------------------- the random cases of the GPU test
# (k, w) and the graph's shape: vertices longer than k; vertices from one base to hundreds; vertices of one to three bases
# under w = 8, where a window starts several entries before the entry its minimiser lies in and the walk back meets the
# walk's first entry
PARAMS = (dict(k=5, w=2, read_len=24, graph=dict(seg_len=(6, 12))),
          dict(k=9, w=4, read_len=70, graph=dict(seg_len=(1, 400), alt_len=(1, 40))),
          dict(k=5, w=8, read_len=24, graph=dict(seg_len=(1, 3))))
SEEDS = range(8)


def random_case(pi, seed):
    """(graph, reads, k, w) of parameter set pi and seed: p_del = 0.4 on odd seeds."""
    from graphgen import mosaic_reads, random_graph
    P = PARAMS[pi]
    rng = np.random.default_rng(9000 + 100 * pi + seed)
    g = random_graph(rng, n_sites=(8 if pi == 2 else 3) + seed % 7, n_walks=4, p_del=0.4 if seed % 2 else 0.0, **P["graph"])
    reads = mosaic_reads(rng, g, n_reads=10, read_len=P["read_len"], n_seg=2, err=0.01)
    return g, reads, P["k"], P["w"]
