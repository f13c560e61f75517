"""Variant calls of the inferred path (or of a walk) against a reference walk: what goes with Context.calls().

The calls are made on the device by the rule of include/phi_amd.h (this project's own: not `vg deconstruct`'s, not
compared with it or with `bcftools`).  Here: the consensus of the rule (apply), the provenance tag of every call
(ph_names), the VCF writer over libphi_host (write_vcf), with the read support of every call where Context.calls_support()
is handed in, and readers of the files it writes (read_vcf, read_support).
"""
import ctypes as C
import os

import numpy as np


def apply(ref_seq, calls, span=None):
    """The consensus of the calls over the reference walk's sequence: ref_seq[span[0]:span[1]] with every call's REF replaced
    by its ALT (span: calls["ref_span"] when None).  By the rule this is the query's sequence over calls["query_span"].
    calls: the dict of Context.calls(), or of read_vcf().  ValueError where a call's REF is not what ref_seq holds at its POS,
    where calls overlap or leave the span."""
    lo, hi = (calls["ref_span"] if span is None else span)
    ref_seq = bytes(ref_seq)
    pos, ro, ao = calls["pos"], calls["ref_off"], calls["alt_off"]
    rb, ab = calls["ref_bytes"], calls["alt_bytes"]
    out, at = [], int(lo)
    for k in range(len(pos)):
        p, rn = int(pos[k]), int(ro[k + 1] - ro[k])
        if p < at or p + rn > hi:
            raise ValueError(f"call {k} at {p} overlaps its predecessor or leaves the span [{lo}, {hi})")
        if ref_seq[p:p + rn] != rb[ro[k]:ro[k + 1]]:
            raise ValueError(f"call {k}: REF is not the reference's bytes at {p}")
        out.append(ref_seq[at:p])
        out.append(ab[ao[k]:ao[k + 1]])
        at = p + rn
    out.append(ref_seq[at:int(hi)])
    return b"".join(out)


def ph_names(calls, path_hap, hap_names):
    """INFO/PH of every call: the name of the panel haplotype the path follows at query index anchor + 1 (the first vertex of
    ALT; where ALT is empty that is the right anchor).  path_hap: solve()'s labels; hap_names: the set graph's walk names."""
    return [hap_names[int(path_hap[int(i) + 1])] for i in calls["anchor"]]


SUPPORT_ARRAYS = ("alt_hit", "alt_n", "ref_hit", "ref_n")


def write_vcf(path, calls, contig, contig_len, sample, ph=None, bgzf=False, device=0, support=None, index=False, origin=0):
    """The calls as plain-text VCFv4.2 (phi_write_calls_vcf of include/phi_host.h): one haploid sample with genotype 1, POS
    1-based, PH=<ph[k]> in INFO where ph (a list of names, one per call) is given.  Calls whose REF and ALT are the same bytes
    are dropped.  Returns (records written, calls dropped).  A name ending in .gz is refused (HostError: this writer has no
    deflate of its own) unless bgzf is set: then the same text (phi_format_calls_vcf) is compressed into BGZF blocks on
    `device` (deflate_bgzf) and written under the name as given.  support: the dict of Context.calls_support() for these
    calls; the records then carry FORMAT/AK and RK (phi_write_calls_vcf_support), everything else is the same bytes.
    index (needs bgzf): a tabix index of the file, built on the device beside it (deflate_bgzf_indexed), as path + ".tbi";
    the file's bytes are the same with and without.
    origin: added to every POS -- calls against the reference of set_graph_vcf(region=) are written in the contig's
    coordinates with origin=v.origin, contig=v.region[0] and contig_len=v.contig_len; an index is that of the shifted positions."""
    from .ilp_index import HostError, host_lib
    L = host_lib()
    if index and not bgzf:
        raise ValueError("index=True needs bgzf=True: the index is one of a BGZF file")
    n = int(len(calls["pos"]))
    pos = np.ascontiguousarray(calls["pos"], np.int64) + int(origin)
    ro = np.ascontiguousarray(calls["ref_off"], np.int64)
    ao = np.ascontiguousarray(calls["alt_off"], np.int64)
    rb, ab = bytes(calls["ref_bytes"]), bytes(calls["alt_bytes"])
    names = None
    if ph is not None:
        if len(ph) != n:
            raise ValueError(f"ph must hold one name per call ({n}), not {len(ph)}")
        names = (C.c_char_p * max(n, 1))(*[s.encode() if isinstance(s, str) else s for s in ph])
    nw, nd = C.c_int64(), C.c_int64()
    err = C.create_string_buffer(512)
    sup, fmt, wr = (), L.phi_format_calls_vcf, L.phi_write_calls_vcf
    if support is not None:
        arrays = [np.ascontiguousarray(support[f], np.int32) for f in SUPPORT_ARRAYS]
        if any(len(a) != n for a in arrays):
            raise ValueError(f"support must hold one count per call ({n})")
        sup, fmt, wr = tuple(a.ctypes.data for a in arrays), L.phi_format_calls_vcf_support, L.phi_write_calls_vcf_support
    if bgzf:
        text, size = C.c_void_p(), C.c_int64()
        rc = fmt(contig.encode(), int(contig_len), sample.encode(), n, pos.ctypes.data, ro.ctypes.data, rb, ao.ctypes.data, ab,
                 names, *sup, C.byref(text), C.byref(size), C.byref(nw), C.byref(nd), err, 512)
        if rc:
            raise HostError(rc, err.value.decode())
        try:
            plain = C.string_at(text, size.value)
        finally:
            L.phi_host_free_text(text)
        from .context import deflate_bgzf, deflate_bgzf_indexed
        packed, tbi = deflate_bgzf_indexed(plain, "tbi", device=device)[:2] if index else (deflate_bgzf(plain, device=device), None)
        with open(path, "wb") as f:
            f.write(packed)
        if index:
            with open(os.fspath(path) + ".tbi", "wb") as f:
                f.write(tbi)
        return nw.value, nd.value
    rc = wr(os.fsencode(path), contig.encode(), int(contig_len), sample.encode(), n, pos.ctypes.data, ro.ctypes.data, rb,
            ao.ctypes.data, ab, names, *sup, C.byref(nw), C.byref(nd), err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
    return nw.value, nd.value


def read_vcf(path):
    """A file write_vcf wrote, back as (header lines, sample, calls dict of pos 0-based / ref_off / alt_off / ref_bytes /
    alt_bytes, list of INFO strings): for apply() and for checks.  Not a general VCF reader."""
    header, pos, refs, alts, infos, sample = [], [], [], [], [], None
    with open(path, "rb") as f:
        for ln in f.read().split(b"\n"):
            if not ln:
                continue
            if ln.startswith(b"##"):
                header.append(ln.decode())
            elif ln.startswith(b"#"):
                header.append(ln.decode())
                sample = ln.decode().split("\t")[9]
            else:
                c = ln.split(b"\t")
                pos.append(int(c[1]) - 1)
                refs.append(c[3])
                alts.append(c[4])
                infos.append(c[7].decode())
    ro, ao = np.zeros(len(pos) + 1, np.int64), np.zeros(len(pos) + 1, np.int64)
    np.cumsum([len(r) for r in refs], out=ro[1:])
    np.cumsum([len(a) for a in alts], out=ao[1:])
    calls = dict(pos=np.array(pos, np.int64), ref_off=ro, alt_off=ao, ref_bytes=b"".join(refs), alt_bytes=b"".join(alts))
    return header, sample, calls, infos


def read_support(path):
    """FORMAT/AK and RK of a file write_vcf(support=) wrote (plain text): a dict of alt_hit, alt_n, ref_hit, ref_n, int32 per
    record.  ValueError for a file without them."""
    cols = {f: [] for f in SUPPORT_ARRAYS}
    with open(path, "rb") as f:
        for ln in f.read().split(b"\n"):
            if not ln or ln.startswith(b"#"):
                continue
            c = ln.split(b"\t")
            if c[8] != b"GT:AK:RK":
                raise ValueError(f"{path}: a record without FORMAT GT:AK:RK")
            _, ak, rk = c[9].split(b":")
            for name, v in zip(SUPPORT_ARRAYS, ak.split(b",") + rk.split(b",")):
                cols[name].append(int(v))
    return {f: np.array(v, np.int32) for f, v in cols.items()}
