"""The rule of phi_calls_path / phi_calls_walk (include/phi_amd.h) restated in plain Python: what the device's arrays are
compared with, element for element (test infrastructure; the product never imports it)."""
import hashlib
import json

import numpy as np


class OrderError(Exception):
    pass


class NoSharedVertex(Exception):
    pass


def calls_ref(query, ref, node_seq):
    """query, ref: lists of vertex ids; node_seq: the vertices' sequences (bytes).  The dict of Context.calls() without gpu_ms."""
    pos_of = {v: p for p, v in enumerate(ref)}
    r_base = np.zeros(len(ref) + 1, np.int64)
    np.cumsum([len(node_seq[v]) for v in ref], out=r_base[1:])
    q_base = np.zeros(len(query) + 1, np.int64)
    np.cumsum([len(node_seq[v]) for v in query], out=q_base[1:])
    shared = [i for i, v in enumerate(query) if v in pos_of]
    if not shared:
        raise NoSharedVertex()
    pos, anchor, refs, alts = [], [], [], []
    for i, i2 in zip(shared, shared[1:]):
        p, p2 = pos_of[query[i]], pos_of[query[i2]]
        if p2 <= p:
            raise OrderError()
        if i2 == i + 1 and p2 == p + 1:
            continue
        r = b"".join(node_seq[v] for v in ref[p + 1:p2])
        a = b"".join(node_seq[v] for v in query[i + 1:i2])
        at = int(r_base[p + 1])
        if not r or not a:
            last = node_seq[query[i]][-1:]
            r, a, at = last + r, last + a, at - 1
        pos.append(at)
        anchor.append(i)
        refs.append(r)
        alts.append(a)
    ro, ao = np.zeros(len(pos) + 1, np.int64), np.zeros(len(pos) + 1, np.int64)
    np.cumsum([len(r) for r in refs], out=ro[1:])
    np.cumsum([len(a) for a in alts], out=ao[1:])
    i0, i1 = shared[0], shared[-1]
    return dict(n_calls=len(pos), pos=np.array(pos, np.int64), anchor=np.array(anchor, np.int32), ref_off=ro, alt_off=ao,
                ref_bytes=b"".join(refs), alt_bytes=b"".join(alts), n_shared=len(shared), n_query=len(query), n_ref=len(ref),
                ref_span=(int(r_base[pos_of[query[i0]]]), int(r_base[pos_of[query[i1]] + 1])),
                query_span=(int(q_base[i0]), int(q_base[i1 + 1])))


def calls_ref_numpy(query, ref, seq_off, seq):
    """The same rule with numpy over flat arrays, for graphs of 10^5 vertices and more (MHC_4): query, ref int32 arrays,
    seq_off int64[n_vtx + 1], seq the concatenated sequences (bytes)."""
    query, ref = np.asarray(query, np.int64), np.asarray(ref, np.int64)
    n_vtx = len(seq_off) - 1
    vlen = np.diff(seq_off)
    pos_of = np.full(n_vtx, -1, np.int64)
    pos_of[ref] = np.arange(len(ref))
    r_base = np.concatenate([[0], np.cumsum(vlen[ref])]).astype(np.int64)
    q_base = np.concatenate([[0], np.cumsum(vlen[query])]).astype(np.int64)
    sh = np.flatnonzero(pos_of[query] >= 0)
    if len(sh) == 0:
        raise NoSharedVertex()
    i, i2 = sh[:-1], sh[1:]
    p, p2 = pos_of[query[i]], pos_of[query[i2]]
    if np.any(p2 <= p):
        raise OrderError()
    is_call = ~((i2 == i + 1) & (p2 == p + 1))
    i, i2, p, p2 = i[is_call], i2[is_call], p[is_call], p2[is_call]
    rl, al = r_base[p2] - r_base[p + 1], q_base[i2] - q_base[i + 1]
    pad = ((rl == 0) | (al == 0)).astype(np.int64)
    pos = r_base[p + 1] - pad
    qpos = q_base[i + 1] - pad
    rl, al = rl + pad, al + pad
    ro = np.concatenate([[0], np.cumsum(rl)]).astype(np.int64)
    ao = np.concatenate([[0], np.cumsum(al)]).astype(np.int64)
    seq = np.frombuffer(seq, np.uint8)

    def flat(walk, base):                                  # the walk's whole sequence
        idx = np.repeat(seq_off[walk] - base[:-1], vlen[walk]) + np.arange(base[-1])
        return seq[idx]
    r_flat, q_flat = flat(ref, r_base), flat(query, q_base)

    def gather(flat_seq, start, length, off):
        idx = np.repeat(start - off[:-1], length) + np.arange(off[-1])
        return flat_seq[idx].tobytes()
    i0, i1 = sh[0], sh[-1]
    return dict(n_calls=len(pos), pos=pos, anchor=i.astype(np.int32), ref_off=ro, alt_off=ao,
                ref_bytes=gather(r_flat, pos, rl, ro), alt_bytes=gather(q_flat, qpos, al, ao),
                n_shared=len(sh), n_query=len(query), n_ref=len(ref),
                ref_span=(int(r_base[pos_of[query[i0]]]), int(r_base[pos_of[query[i1]] + 1])),
                query_span=(int(q_base[i0]), int(q_base[i1 + 1])))


def digest(c):
    """A hash of everything a calls dict holds but its times: equal digests, equal calls."""
    h = hashlib.sha256()
    for k in ("pos", "anchor", "ref_off", "alt_off"):
        h.update(np.ascontiguousarray(c[k]).tobytes())
    h.update(c["ref_bytes"])
    h.update(c["alt_bytes"])
    h.update(json.dumps([int(c[k]) for k in ("n_calls", "n_shared", "n_query", "n_ref")] + [int(x) for x in c["ref_span"] + c["query_span"]]).encode())
    return h.hexdigest()
