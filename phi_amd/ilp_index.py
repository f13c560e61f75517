"""Host-side mirror of the reference's operator interface for this path: class ILP_index
(src/ILP_index.h:48-94) as src/main.cpp:114-140 drives it -- same member names, same argument
meaning, same log lines and FASTA output -- with the work done by the two native libraries:

    read_gfa / read_ip_reads   -> libphi_host.so (include/phi_host.h)
    ILP_function               -> libphi_amd.so  (include/phi_amd.h: HIP kernels on one MI355X)

Nothing here computes on the CPU; without the HIP library or a GPU the calls raise.
"""
import ctypes as C
import os
import sys
import time

import numpy as np

from . import _capi
from .context import Context, PhiError

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "libphi_host.so")

HOST_SYMBOLS = [
    "phi_gfa_read", "phi_graph_free", "phi_graph_n_vtx", "phi_graph_n_walks", "phi_graph_n_edges",
    "phi_graph_seq_concat", "phi_graph_seq_off", "phi_graph_adj_off", "phi_graph_adj", "phi_graph_walk_off",
    "phi_graph_walk_vtx", "phi_graph_topo_rank", "phi_graph_hap_name", "phi_graph_seg_name", "phi_reads_read",
    "phi_reads_free", "phi_reads_count", "phi_reads_bases", "phi_reads_off", "phi_reads_name", "phi_hap_name",
    "phi_write_fasta", "phi_reads_stream_open", "phi_reads_stream_next", "phi_reads_stream_reads",
    "phi_reads_stream_bases", "phi_reads_stream_close", "phi_reads_stream_open_blocks",
    "phi_text_stream_open", "phi_text_stream_read", "phi_text_stream_close",
    "phi_gfa_read_deferred", "phi_graph_walks_deferred", "phi_graph_walk_texts", "phi_graph_name_index", "phi_graph_resolve_walks",
    "phi_graph_set_walk_off", "phi_gfa_read_deferred_text",
    "phi_vcf_read", "phi_vcf_free", "phi_vcf_n_samples", "phi_vcf_sample_name", "phi_vcf_contig", "phi_vcf_n_records", "phi_vcf_n_sites",
    "phi_vcf_n_other_contig", "phi_vcf_n_ref_mismatch", "phi_vcf_ref_len", "phi_vcf_ref_seq", "phi_vcf_rec_start", "phi_vcf_rec_end",
    "phi_vcf_rec_gt_index", "phi_vcf_rec_alt_off", "phi_vcf_alt_pos", "phi_vcf_alt_bytes", "phi_vcf_site_off", "phi_vcf_text", "phi_vcf_text_off",
    "phi_vcf_parse_gt", "phi_vcf_build", "phi_vcf_n_units", "phi_vcf_unit_first", "phi_vcf_n_real_sites", "phi_vcf_site_backbone",
    "phi_vcf_site_allele0", "phi_vcf_n_kept_haps", "phi_vcf_choice",
    "phi_region_parse", "phi_region_plan", "phi_region_open", "phi_region_free", "phi_region_name", "phi_region_beg", "phi_region_end",
    "phi_region_contig_len", "phi_region_in_index", "phi_region_n_members", "phi_region_member_at", "phi_region_member_text_off",
    "phi_region_n_ranges", "phi_region_ranges", "phi_region_gz", "phi_region_n_gz", "phi_region_header", "phi_region_n_header",
    "phi_region_ref", "phi_region_n_ref", "phi_region_fasta_members", "phi_fasta_slice", "phi_region_free_bases", "phi_vcf_read_text",
    "phi_vcf_read_region", "phi_vcf_origin", "phi_vcf_n_outside",
    "phi_bam_header", "phi_panel_choose", "phi_write_calls_vcf",
    "phi_format_fasta", "phi_format_fasta_fai", "phi_format_calls_vcf", "phi_host_free_text",
    "phi_write_calls_vcf_support", "phi_format_calls_vcf_support",
]
PHI_HOST_NEED_MORE = -6

WALK_TEXT_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int32)

TEXT_BLOCK_FN = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.POINTER(C.c_void_p))

_host = None


def host_lib():
    global _host
    if _host is not None:
        return _host
    if not os.path.exists(HOST_LIB_PATH):
        raise RuntimeError(f"{HOST_LIB_PATH} is missing: run `python -m phi_amd.build`")
    L = C.CDLL(HOST_LIB_PATH)
    vp = C.c_void_p
    L.phi_gfa_read.argtypes = [C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_graph_free.restype = None
    L.phi_graph_free.argtypes = [vp]
    L.phi_graph_n_vtx.restype = C.c_int32
    L.phi_graph_n_walks.restype = C.c_int32
    L.phi_graph_n_edges.restype = C.c_int64
    for n in ("n_vtx", "n_walks", "n_edges"):
        getattr(L, "phi_graph_" + n).argtypes = [vp]
    for n in ("seq_concat", "seq_off", "adj_off", "adj", "walk_off", "walk_vtx", "topo_rank"):
        f = getattr(L, "phi_graph_" + n)
        f.restype = vp
        f.argtypes = [vp]
    for n in ("hap_name", "seg_name"):
        f = getattr(L, "phi_graph_" + n)
        f.restype = C.c_char_p
        f.argtypes = [vp, C.c_int32]
    L.phi_reads_read.argtypes = [C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_reads_free.restype = None
    L.phi_reads_free.argtypes = [vp]
    L.phi_reads_count.restype = C.c_int64
    L.phi_reads_count.argtypes = [vp]
    for n in ("bases", "off"):
        f = getattr(L, "phi_reads_" + n)
        f.restype = vp
        f.argtypes = [vp]
    L.phi_reads_name.restype = C.c_char_p
    L.phi_reads_name.argtypes = [vp, C.c_int64]
    L.phi_reads_stream_open.argtypes = [C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_reads_stream_next.restype = C.c_int64
    L.phi_reads_stream_next.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.c_char_p, C.c_int]
    for n in ("reads", "bases"):
        f = getattr(L, "phi_reads_stream_" + n)
        f.restype = C.c_int64
        f.argtypes = [vp]
    L.phi_reads_stream_open_blocks.argtypes = [vp, C.c_int64, vp, vp, C.c_int64, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_text_stream_open.argtypes = [C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_text_stream_read.restype = C.c_int64
    L.phi_text_stream_read.argtypes = [vp, vp, C.c_int64, C.c_char_p, C.c_int]
    L.phi_text_stream_close.restype = None
    L.phi_text_stream_close.argtypes = [vp]
    L.phi_reads_stream_close.restype = None
    L.phi_reads_stream_close.argtypes = [vp]
    L.phi_gfa_read_deferred.argtypes = [C.c_char_p, C.POINTER(vp), vp, vp, C.c_char_p, C.c_int]
    L.phi_graph_walks_deferred.argtypes = [vp]
    L.phi_graph_walk_texts.argtypes = [vp, vp, C.c_int32]
    L.phi_graph_name_index.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.phi_graph_resolve_walks.argtypes = [vp, C.c_char_p, C.c_int]
    L.phi_graph_set_walk_off.argtypes = [vp, vp]
    L.phi_gfa_read_deferred_text.argtypes = [vp, C.c_int64, C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_hap_name.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    L.phi_vcf_read.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_vcf_free.restype = None
    L.phi_vcf_free.argtypes = [vp]
    for n, rt in (("n_samples", C.c_int32), ("n_kept_haps", C.c_int32), ("contig", C.c_char_p), ("n_records", C.c_int64), ("n_sites", C.c_int64),
                  ("n_other_contig", C.c_int64), ("n_ref_mismatch", C.c_int64), ("ref_len", C.c_int64), ("n_units", C.c_int64), ("n_real_sites", C.c_int64),
                  ("origin", C.c_int64), ("n_outside", C.c_int64)):
        f = getattr(L, "phi_vcf_" + n)
        f.restype = rt
        f.argtypes = [vp]
    for n in ("ref_seq", "rec_start", "rec_end", "rec_gt_index", "rec_alt_off", "alt_pos", "alt_bytes", "site_off", "text", "text_off",
              "unit_first", "site_backbone", "site_allele0", "choice"):
        f = getattr(L, "phi_vcf_" + n)
        f.restype = vp
        f.argtypes = [vp]
    L.phi_vcf_sample_name.restype = C.c_char_p
    L.phi_vcf_sample_name.argtypes = [vp, C.c_int32]
    L.phi_vcf_parse_gt.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, C.c_int32, vp, vp, C.c_char_p, C.c_int]
    L.phi_vcf_build.argtypes = [vp, vp, vp, C.c_int32, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_region_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.phi_region_plan.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_region_open.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_region_free.restype = None
    L.phi_region_free.argtypes = [vp]
    for n, rt in (("name", C.c_char_p), ("beg", C.c_int64), ("end", C.c_int64), ("contig_len", C.c_int64), ("in_index", C.c_int32), ("n_members", C.c_int64),
                  ("member_at", vp), ("member_text_off", vp), ("n_ranges", C.c_int32), ("ranges", vp), ("gz", vp), ("n_gz", C.c_int64), ("header", vp),
                  ("n_header", C.c_int64), ("ref", vp), ("n_ref", C.c_int64), ("fasta_members", C.c_int64)):
        f = getattr(L, "phi_region_" + n)
        f.restype = rt
        f.argtypes = [vp]
    L.phi_fasta_slice.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.phi_region_free_bases.restype = None
    L.phi_region_free_bases.argtypes = [vp]
    L.phi_vcf_read_text.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_char_p, C.c_int64, C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_vcf_read_region.argtypes = [vp, vp, C.c_int64, C.POINTER(vp), C.c_char_p, C.c_int]
    L.phi_write_fasta.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64]
    L.phi_write_calls_vcf.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, vp, vp, vp, vp, vp, vp,
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.phi_format_fasta.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.POINTER(vp), C.POINTER(C.c_int64)]
    L.phi_format_fasta_fai.argtypes = [C.c_char_p, C.c_int64, C.POINTER(vp), C.POINTER(C.c_int64)]
    L.phi_format_calls_vcf.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, vp, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.phi_write_calls_vcf_support.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.phi_format_calls_vcf_support.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp),
                                               C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.phi_host_free_text.restype = None
    L.phi_host_free_text.argtypes = [vp]
    L.phi_bam_header.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_char_p, C.c_int]
    L.phi_panel_choose.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int32, vp, vp]
    for n in HOST_SYMBOLS:
        getattr(L, n)
    _host = L
    return L


def stream_reads(path, bases_cap=64 << 20, reads_cap=1 << 20):
    """Chunks (uint8 bases, int64 offsets) of a FASTA/FASTQ file through phi_reads_stream_* -- the reader
    the command line feeds phi_add_reads with, chunk by chunk."""
    L = host_lib()
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = L.phi_reads_stream_open(os.fsencode(path), C.byref(h), err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
    bases = np.zeros(bases_cap, np.uint8)
    off = np.zeros(reads_cap + 1, np.int64)
    try:
        while True:
            n = L.phi_reads_stream_next(h, bases.ctypes.data, bases_cap, off.ctypes.data, reads_cap, err, 512)
            if n < 0:
                raise HostError(int(n), err.value.decode())
            if n == 0:
                break
            yield bases[:off[n]].copy(), off[:n + 1].copy()
    finally:
        L.phi_reads_stream_close(h)


def text_chunks(path, chunk_bytes=64 << 20):
    """The (inflated) text of a reads file, chunk by chunk, through phi_text_stream_*: what the command line hands to
    phi_add_reads_text."""
    L = host_lib()
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = L.phi_text_stream_open(os.fsencode(path), C.byref(h), err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
    buf = np.zeros(chunk_bytes, np.uint8)
    try:
        while True:
            n = L.phi_text_stream_read(h, buf.ctypes.data, chunk_bytes, err, 512)
            if n < 0:
                raise HostError(int(n), err.value.decode())
            if n == 0:
                break
            yield buf[:n].copy()
    finally:
        L.phi_text_stream_close(h)


def bam_header(data):
    """phi_bam_header on the first inflated bytes of a BAM stream: (status, records_start, n_ref, message); status 0,
    PHI_HOST_NEED_MORE (records_start: a lower bound of the bytes needed) or PHI_HOST_ERR_INVALID."""
    L = host_lib()
    buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
    start, n_ref = C.c_int64(), C.c_int32()
    err = C.create_string_buffer(256)
    rc = L.phi_bam_header(buf.ctypes.data if len(buf) else None, len(buf), C.byref(start), C.byref(n_ref), err, 256)
    return rc, start.value, n_ref.value, err.value.decode()


def reads_file_kind(path):
    """What the command line takes a reads file for, by content: "bam" (gzip whose inflated bytes begin with BAM\\1), "cram",
    "sam" (plain text that begins with a SAM header line and its first field) or "text" (FASTA / FASTQ, plain or gzip).  Only a
    regular file is looked at; a pipe, a missing or an unreadable file is "text", for the reader to take or to report."""
    import gzip
    try:
        if not os.path.isfile(path):
            return "text"
        with open(path, "rb") as f:
            head = f.read(7)
        if head[:4] == b"CRAM":
            return "cram"
        if head[:2] == b"\x1f\x8b":
            with gzip.open(path, "rb") as f:
                return "bam" if f.read(4) == b"BAM\x01" else "text"
    except (OSError, EOFError):
        return "text"
    return "sam" if head in (b"@HD\tVN:", b"@SQ\tSN:", b"@RG\tID:", b"@PG\tID:") else "text"


class BamReads:
    """A BAM reads file as an entry of ip_reads: its records are found and decoded on the device (Context.add_reads_bam) when
    ILP_function scores the reads; the file's BGZF layer is inflated by the host pool (text_chunks)."""

    def __init__(self, path, chunk_bytes=64 << 20):
        self.path, self.chunk_bytes, self.info = path, chunk_bytes, None

    def feed(self, ctx):
        ctx.reads_bam_begin(self.chunk_bytes)
        try:
            for chunk in text_chunks(self.path, self.chunk_bytes):
                ctx.add_reads_bam(chunk)
        except Exception:
            try:
                ctx.reads_bam_end()
            except PhiError:
                pass
            raise
        self.info = ctx.reads_bam_end()
        return self.info


def reads_of_text(prefix, blocks=(), bases_cap=64 << 20, reads_cap=1 << 20, stream_offset=0):
    """kseq's records (uint8 bases, int64 offsets) of the text `prefix` followed by the byte blocks `blocks`, through
    phi_reads_stream_open_blocks: the exact host state machine over text that is in memory (stream_offset: bytes of
    the stream before prefix[0])."""
    L = host_lib()
    it = iter(blocks)
    keep = []

    def nxt(_user, out):
        try:
            b = next(it)
        except StopIteration:
            return 0
        a = np.frombuffer(bytes(b), np.uint8)
        keep[:] = [a]
        out[0] = a.ctypes.data
        return len(a)
    cb = TEXT_BLOCK_FN(nxt)
    pre = np.frombuffer(bytes(prefix), np.uint8)
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = L.phi_reads_stream_open_blocks(pre.ctypes.data if len(pre) else None, len(pre), C.cast(cb, C.c_void_p), None, stream_offset, C.byref(h), err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
    bases = np.zeros(bases_cap, np.uint8)
    off = np.zeros(reads_cap + 1, np.int64)
    out_b, out_o = [], [np.zeros(1, np.int64)]
    try:
        while True:
            n = L.phi_reads_stream_next(h, bases.ctypes.data, bases_cap, off.ctypes.data, reads_cap, err, 512)
            if n < 0:
                raise HostError(int(n), err.value.decode())
            if n == 0:
                break
            out_b.append(bases[:off[n]].copy())
            out_o.append(off[1:n + 1] + out_o[-1][-1])
    finally:
        L.phi_reads_stream_close(h)
    return (np.concatenate(out_b) if out_b else np.zeros(0, np.uint8)), np.concatenate(out_o)


def _view(ptr, n, ctype, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,))


class HostError(RuntimeError):
    def __init__(self, status, detail):
        self.status = status
        super().__init__(f"host error {status}: {detail}")


def get_hap_name(gfa_name, reads_name):
    """get_hap_name (misc.cpp:58-87)."""
    buf = C.create_string_buffer(4096)
    n = host_lib().phi_hap_name(os.fsencode(gfa_name), os.fsencode(reads_name), buf, 4096)
    if n < 0:
        raise HostError(n, "name too long")
    return buf.value.decode()


class Graph:
    """gfa_t + the arrays ILP_index::read_gfa fills (adj_list, node_seq, paths, top_order_map, hap_id2name)."""

    def __init__(self, path):
        L = host_lib()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = L.phi_gfa_read(os.fsencode(path), C.byref(h), err, 512)
        if rc:
            raise HostError(rc, err.value.decode())
        try:
            self.n_vtx = L.phi_graph_n_vtx(h)
            self.num_walks = L.phi_graph_n_walks(h)
            ne = L.phi_graph_n_edges(h)
            self.seq_off = _view(L.phi_graph_seq_off(h), self.n_vtx + 1, C.c_int64, np.int64).copy()
            self.seq_concat = _view(L.phi_graph_seq_concat(h), int(self.seq_off[-1]), C.c_uint8, np.uint8).copy()
            self.adj_off = _view(L.phi_graph_adj_off(h), self.n_vtx + 1, C.c_int64, np.int64).copy()
            self.adj = _view(L.phi_graph_adj(h), ne, C.c_int32, np.int32).copy()
            self.walk_off = _view(L.phi_graph_walk_off(h), self.num_walks + 1, C.c_int64, np.int64).copy()
            self.walk_vtx = _view(L.phi_graph_walk_vtx(h), int(self.walk_off[-1]) if self.num_walks else 0, C.c_int32, np.int32).copy()
            self.top_order_map = _view(L.phi_graph_topo_rank(h), self.n_vtx, C.c_int32, np.int32).copy()
            self.hap_id2name = [L.phi_graph_hap_name(h, w).decode() for w in range(self.num_walks)]
            self.seg_names = [L.phi_graph_seg_name(h, v).decode() for v in range(self.n_vtx)]
        finally:
            L.phi_graph_free(h)


def parse_gt(text, text_off, gt_index, n_samples, rec_lo=0, rec_hi=None, gt=None, ploidy=None):
    """phi_vcf_parse_gt: the exact scalar genotype parser over sample-column slices (every slice followed by a line feed).
    -> (gt uint16 [records, n_samples, 2], ploidy int32 [n_samples]); rows outside [rec_lo, rec_hi) are left as passed in."""
    text = np.ascontiguousarray(np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else text)
    text_off = np.ascontiguousarray(text_off, np.int64)
    gt_index = np.ascontiguousarray(gt_index, np.int32)
    n_rec = len(text_off) - 1
    gt = np.zeros((n_rec, n_samples, 2), np.uint16) if gt is None else gt
    ploidy = np.zeros(n_samples, np.int32) if ploidy is None else ploidy
    err = C.create_string_buffer(512)
    rc = host_lib().phi_vcf_parse_gt(text.ctypes.data, text_off.ctypes.data, gt_index.ctypes.data, rec_lo, n_rec if rec_hi is None else rec_hi,
                                     n_samples, gt.ctypes.data, ploidy.ctypes.data, err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
    return gt, ploidy


def parse_region(region):
    """(name, BEG, END) of "NAME", "NAME:BEG" or "NAME:BEG-END": 1-based and inclusive as written, END None when absent
    (phi_region_parse; HostError for a string that is no region)."""
    L = host_lib()
    name, b, e, err = C.create_string_buffer(4096), C.c_int64(), C.c_int64(), C.create_string_buffer(1024)
    rc = L.phi_region_parse(os.fsencode(region), name, 4096, C.byref(b), C.byref(e), err, 1024)
    if rc:
        raise HostError(rc, err.value.decode())
    return name.value.decode(), b.value, None if e.value < 0 else e.value


def fasta_slice(fasta_path, name, beg, end=-1, with_info=False):
    """Bases [beg, end) (0-based; end < 0: to the record's end) of record `name` of an indexed FASTA, upper-cased
    (phi_fasta_slice: .fai, and .gzi for a BGZF file -- what `samtools faidx FILE REGION` prints, without its line ends)."""
    L = host_lib()
    p, n, ln, mem, err = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64(), C.create_string_buffer(1024)
    rc = L.phi_fasta_slice(os.fsencode(fasta_path), os.fsencode(name), beg, end, C.byref(p), C.byref(n), C.byref(ln), C.byref(mem), err, 1024)
    if rc:
        raise HostError(rc, err.value.decode())
    try:
        out = C.string_at(p, n.value)
    finally:
        L.phi_region_free_bases(p)
    return (out, {"contig_len": ln.value, "members": mem.value}) if with_info else out


class RegionPlan:
    """What the host decides about a region of an indexed BGZF VCF before a record is looked at (include/phi_host.h
    phi_region_plan / phi_region_open): the BGZF members the .tbi points at (member_at: their file offsets; gz: their bytes back
    to back), every merged chunk as a byte range of their inflated text (ranges [n, 2]; member_text_off), the header text,
    and from open() the reference slice ref and the contig's length.  RegionPlan(vcf, name, b, e) plans one 0-based
    half-open interval; RegionPlan.open(vcf, fasta, "NAME:BEG-END") is the whole host side of set_graph_vcf(region=)."""

    def __init__(self, vcf_path, name, beg, end, load=True, _open=None):
        L = host_lib()
        self._L = L
        self._h = C.c_void_p()
        err = C.create_string_buffer(1024)
        if _open is not None:
            rc = L.phi_region_open(os.fsencode(vcf_path), os.fsencode(_open[0]), os.fsencode(_open[1]), C.byref(self._h), err, 1024)
        else:
            rc = L.phi_region_plan(os.fsencode(vcf_path), os.fsencode(name), beg, end, 1 if load else 0, C.byref(self._h), err, 1024)
        if rc:
            raise HostError(rc, err.value.decode())
        h = self._h
        self.name = L.phi_region_name(h).decode()
        self.beg, self.end, self.contig_len = L.phi_region_beg(h), L.phi_region_end(h), L.phi_region_contig_len(h)
        self.in_index = bool(L.phi_region_in_index(h))
        m = L.phi_region_n_members(h)
        self.member_at = _view(L.phi_region_member_at(h), m, C.c_int64, np.int64).copy()
        self.member_text_off = _view(L.phi_region_member_text_off(h), m + 1, C.c_int64, np.int64).copy()
        self.ranges = _view(L.phi_region_ranges(h), 2 * L.phi_region_n_ranges(h), C.c_int64, np.int64).copy().reshape(-1, 2)
        self.gz = C.string_at(L.phi_region_gz(h), L.phi_region_n_gz(h)) if L.phi_region_n_gz(h) else b""
        self.header = C.string_at(L.phi_region_header(h), L.phi_region_n_header(h)) if L.phi_region_n_header(h) else b""
        self.ref = C.string_at(L.phi_region_ref(h), L.phi_region_n_ref(h)) if L.phi_region_n_ref(h) else b""
        self.fasta_members = L.phi_region_fasta_members(h)

    @classmethod
    def open(cls, vcf_path, fasta_path, region):
        return cls(vcf_path, None, 0, 0, _open=(fasta_path, region))

    def close(self):
        if self._h:
            self._L.phi_region_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VcfGraph:
    """A phased VCF + reference FASTA read by phi_vcf_read: the kept records (fixed columns), the sites and the sample-column
    text; build(gt, ploidy, max_len) makes the graph of phi_amd.vcf2gfa -- the attributes of Graph, with walk_off / walk_vtx
    None: Context.set_graph_vcf writes the walk entries on the device -- and the unit tables the device needs.
    region=RegionPlan (from RegionPlan.open) with lines=the record lines phi_vcf_region_filter kept: the same rule pass over
    header + lines against the plan's reference slice (phi_vcf_read_region); positions count from the region's first base
    (origin), region = (name, b, e), n_outside the records that reach over an edge of the region.
    text=(vcf text, reference bases, origin, contig or None): the rule pass over text in memory (phi_vcf_read_text)."""

    def __init__(self, vcf_path, fasta_path, region=None, lines=b"", text=None):
        L = host_lib()
        self._L = L
        self._h = C.c_void_p()
        err = C.create_string_buffer(1024)
        self.region = None
        if region is not None:
            rc = L.phi_vcf_read_region(region._h, lines, len(lines), C.byref(self._h), err, 1024)
            self.region = (region.name, region.beg, region.end)
            self.contig_len = region.contig_len
        elif text is not None:
            vt, ref, origin, contig = text
            rc = L.phi_vcf_read_text(vt, len(vt), ref, len(ref), None, origin, None if contig is None else os.fsencode(contig), C.byref(self._h), err, 1024)
        else:
            rc = L.phi_vcf_read(os.fsencode(vcf_path), os.fsencode(fasta_path), C.byref(self._h), err, 1024)
        if rc:
            raise HostError(rc, err.value.decode())
        h = self._h
        self.origin, self.n_outside = L.phi_vcf_origin(h), L.phi_vcf_n_outside(h)
        self.samples = [L.phi_vcf_sample_name(h, s).decode() for s in range(L.phi_vcf_n_samples(h))]
        self.contig = L.phi_vcf_contig(h).decode()
        self.n_records, self.n_sites = L.phi_vcf_n_records(h), L.phi_vcf_n_sites(h)
        self.n_other_contig, self.n_ref_mismatch = L.phi_vcf_n_other_contig(h), L.phi_vcf_n_ref_mismatch(h)
        n = self.n_records
        self.ref_seq = _view(L.phi_vcf_ref_seq(h), L.phi_vcf_ref_len(h), C.c_uint8, np.uint8)
        self.rec_start = _view(L.phi_vcf_rec_start(h), n, C.c_int64, np.int64)
        self.rec_end = _view(L.phi_vcf_rec_end(h), n, C.c_int64, np.int64)
        self.gt_index = _view(L.phi_vcf_rec_gt_index(h), n, C.c_int32, np.int32)
        self.alt_off = _view(L.phi_vcf_rec_alt_off(h), n + 1, C.c_int64, np.int64)
        self.alt_pos = _view(L.phi_vcf_alt_pos(h), int(self.alt_off[-1]) + 1, C.c_int64, np.int64)
        self.alt_bytes = _view(L.phi_vcf_alt_bytes(h), int(self.alt_pos[-1]), C.c_uint8, np.uint8)
        self.site_off = _view(L.phi_vcf_site_off(h), self.n_sites + 1, C.c_int64, np.int64)
        self.text_off = _view(L.phi_vcf_text_off(h), n + 1, C.c_int64, np.int64)
        self.text = _view(L.phi_vcf_text(h), int(self.text_off[-1]), C.c_uint8, np.uint8)

    def warnings(self):
        """The two warnings of vcf2gfa.read_vcf, in its words."""
        out = []
        if self.n_other_contig:
            out.append(f"{self.n_other_contig} record(s) of other contigs than {self.contig} skipped (vcf2gfa handles one contig)")
        if self.n_ref_mismatch:
            out.append(f"{self.n_ref_mismatch} record(s) skipped: their REF column is not what the FASTA holds at POS (another assembly?)")
        if self.region is not None and self.n_outside:
            out.append(f"{self.n_outside} record(s) skipped: they reach over an edge of the region {self.region[0]}:{self.region[1] + 1}-{self.region[2]}")
        return out

    def alts(self, r):
        raw = self.alt_bytes.tobytes()
        return [raw[self.alt_pos[a]:self.alt_pos[a + 1]] for a in range(int(self.alt_off[r]), int(self.alt_off[r + 1]))]

    def parse_gt(self, rec_lo=0, rec_hi=None, gt=None, ploidy=None):
        return parse_gt(self.text, self.text_off, self.gt_index, len(self.samples), rec_lo, rec_hi, gt, ploidy)

    def build(self, gt, ploidy, max_len=30):
        L, h = self._L, self._h
        gt = np.ascontiguousarray(gt, np.uint16)
        ploidy = np.ascontiguousarray(ploidy, np.int32)
        assert gt.size == self.n_records * len(self.samples) * 2 and len(ploidy) == len(self.samples)
        g = C.c_void_p()
        err = C.create_string_buffer(1024)
        rc = L.phi_vcf_build(h, gt.ctypes.data if gt.size else None, ploidy.ctypes.data if ploidy.size else None, max_len, C.byref(g), err, 1024)
        if rc:
            raise HostError(rc, err.value.decode())
        try:
            self.n_vtx = L.phi_graph_n_vtx(g)
            self.num_walks = L.phi_graph_n_walks(g)
            ne = L.phi_graph_n_edges(g)
            self.seq_off = _view(L.phi_graph_seq_off(g), self.n_vtx + 1, C.c_int64, np.int64).copy()
            self.seq_concat = _view(L.phi_graph_seq_concat(g), int(self.seq_off[-1]), C.c_uint8, np.uint8).copy()
            self.adj_off = _view(L.phi_graph_adj_off(g), self.n_vtx + 1, C.c_int64, np.int64).copy()
            self.adj = _view(L.phi_graph_adj(g), ne, C.c_int32, np.int32).copy()
            self.top_order_map = _view(L.phi_graph_topo_rank(g), self.n_vtx, C.c_int32, np.int32).copy()
            self.hap_id2name = [L.phi_graph_hap_name(g, w).decode() for w in range(self.num_walks)]
        finally:
            L.phi_graph_free(g)
        self.walk_off = self.walk_vtx = None
        self.n_units, self.n_real_sites = L.phi_vcf_n_units(h), L.phi_vcf_n_real_sites(h)
        assert L.phi_vcf_n_kept_haps(h) == self.num_walks
        self.unit_first = _view(L.phi_vcf_unit_first(h), self.n_units + 1, C.c_int32, np.int32).copy()
        self.site_backbone = _view(L.phi_vcf_site_backbone(h), self.n_real_sites, C.c_int32, np.int32).copy()
        self.site_allele0 = _view(L.phi_vcf_site_allele0(h), self.n_real_sites, C.c_int32, np.int32).copy()
        self.choice = _view(L.phi_vcf_choice(h), self.n_real_sites * self.num_walks, C.c_int32, np.int32).copy().reshape(self.n_real_sites, self.num_walks)
        return self

    def host_walks(self):
        """The walks the device writes, made here from the same tables (tests, and callers without a GPU): (walk_off, walk_vtx)."""
        uw = np.empty((self.num_walks, 2 * self.n_real_sites + 1), np.int64)
        uw[:, 0:-1:2] = self.site_backbone[None, :]
        uw[:, 1::2] = (self.site_allele0[:, None] + self.choice).T
        uw[:, -1] = self.n_units - 1
        cnt = np.diff(self.unit_first.astype(np.int64))[uw]
        walk_off = np.concatenate([[0], np.cumsum(cnt.sum(axis=1))]).astype(np.int64)
        flat_u, flat_c = uw.ravel(), cnt.ravel()
        start = np.repeat(self.unit_first[flat_u].astype(np.int64), flat_c)
        within = np.arange(int(flat_c.sum()), dtype=np.int64) - np.repeat(np.cumsum(flat_c) - flat_c, flat_c)
        return walk_off, (start + within).astype(np.int32)

    def close(self):
        if self._h:
            self._L.phi_vcf_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeferredGraph:
    """A GFA read with its walks left as TEXT (phi_gfa_read_deferred): resolve_on_device(ctx) sends the W-lines' walk fields
    to the context's GPU and resolves them there (include/phi_amd.h phi_walk_text_*); when the text is not of the kind
    the device takes -- or on request -- resolve_on_host() does what Graph does.  set_graph(ctx) hands the graph over."""

    def __init__(self, path, on_text=None, _text=None):
        L = host_lib()
        self._L = L
        self._h = C.c_void_p()
        err = C.create_string_buffer(512)
        self._cb = WALK_TEXT_FN(on_text) if on_text else None
        if _text is not None:                         # (address, bytes) of text in memory, borrowed: phi_gfa_read_deferred_text
            rc = L.phi_gfa_read_deferred_text(_text[0], _text[1], os.fsencode(path), C.byref(self._h), err, 512)
        else:
            rc = L.phi_gfa_read_deferred(os.fsencode(path), C.byref(self._h), C.cast(self._cb, C.c_void_p) if self._cb else None, None, err, 512)
        if rc:
            raise HostError(rc, err.value.decode())
        h = self._h
        self.n_vtx = L.phi_graph_n_vtx(h)
        self.num_walks = L.phi_graph_n_walks(h)
        ne = L.phi_graph_n_edges(h)
        self.seq_off = _view(L.phi_graph_seq_off(h), self.n_vtx + 1, C.c_int64, np.int64).copy()
        self.seq_concat = _view(L.phi_graph_seq_concat(h), int(self.seq_off[-1]), C.c_uint8, np.uint8).copy()
        self.adj_off = _view(L.phi_graph_adj_off(h), self.n_vtx + 1, C.c_int64, np.int64).copy()
        self.adj = _view(L.phi_graph_adj(h), ne, C.c_int32, np.int32).copy()
        self.top_order_map = _view(L.phi_graph_topo_rank(h), self.n_vtx, C.c_int32, np.int32).copy()
        self.hap_id2name = [L.phi_graph_hap_name(h, w).decode() for w in range(self.num_walks)]
        self.walk_off = None
        self.walk_vtx = None                          # stays None when the device resolved the walks
        self.on_device = False

    @classmethod
    def from_gzip_on_device(cls, path, ctx, chunk_bytes=0):
        """A gzip GFA through the device route of the command line: inflated and split on ctx's GPU
        (Context.gfa_gzip_split), the S-lines, L-lines and W-line heads read by the host reader from the split text, the
        walks resolved on the device from the fields that never left it.  Whatever that route does not finish -- a walk
        count that differs from the reader's, names not <prefix><number>, a W-line among the S-lines, irregular walk text --
        is read again from the file and resolved on the host; .route says which ("device" or the reason).  PhiError for a
        corrupt stream or a refused split (the file is then the caller's to read)."""
        p, n, info = ctx._gfa_gzip_split_raw(open(path, "rb").read(), chunk_bytes)
        try:
            g = cls(path, _text=(p.value, n))
            g.split_info = info
            if g.num_walks != info["n_walks"]:
                g.route = "walk count differs from the host reader's"
            elif g.resolve_on_device(ctx, upload=False):
                g.route = "device"
                return g
            else:
                g.route = "irregular walk text" if getattr(g, "irregular", 0) else "names not <prefix><number>, or a W-line among the S-lines"
            g.close()
        finally:
            ctx._L.phi_gfa_gzip_free(p)
        ctx._chk(ctx._L.phi_walk_text_upload(ctx._h, None, 0))
        h = cls(path)
        h.split_info, h.route = info, g.route
        h.resolve_on_host()
        return h

    def close(self):
        if self._h:
            self._L.phi_graph_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def walk_texts(self):
        """(address, bytes) of every walk field in the mapped file."""
        n = self._L.phi_graph_walk_texts(self._h, None, 0)
        buf = (C.c_int64 * (2 * max(n, 1)))()
        self._L.phi_graph_walk_texts(self._h, buf, n)
        return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]

    def resolve_on_device(self, ctx, upload=True):
        """True when the device resolved the walks; False when the text is irregular (then: resolve_on_host)."""
        L = self._L
        prefix, pn, tbl, nn = C.c_void_p(), C.c_int32(), C.c_void_p(), C.c_int64()
        if L.phi_graph_name_index(self._h, C.byref(prefix), C.byref(pn), C.byref(tbl), C.byref(nn)) != 0:
            return False
        n = self.num_walks
        if upload:
            buf = (C.c_int64 * (2 * max(n, 1)))()
            L.phi_graph_walk_texts(self._h, buf, n)
            ctx._chk(ctx._L.phi_walk_text_upload(ctx._h, buf, n))
        woff = np.zeros(n + 1, np.int64)
        irr = C.c_uint32()
        ctx._chk(ctx._L.phi_walk_text_resolve(ctx._h, C.cast(prefix, C.c_char_p), pn.value, tbl, nn.value, self.n_vtx, woff.ctypes.data, C.byref(irr)))
        self.irregular = irr.value
        if irr.value:
            return False
        self.walk_off = woff
        L.phi_graph_set_walk_off(self._h, woff.ctypes.data)
        self.on_device = True
        return True

    def resolve_on_host(self):
        err = C.create_string_buffer(512)
        rc = self._L.phi_graph_resolve_walks(self._h, err, 512)
        if rc:
            raise HostError(rc, err.value.decode())
        self.walk_off = _view(self._L.phi_graph_walk_off(self._h), self.num_walks + 1, C.c_int64, np.int64).copy()
        self.walk_vtx = _view(self._L.phi_graph_walk_vtx(self._h), int(self.walk_off[-1]) if self.num_walks else 0, C.c_int32, np.int32).copy()

    def set_graph(self, ctx, chop=None, keep=None, retain=False):
        return ctx.set_graph(self.seq_concat, self.seq_off, self.adj_off, self.adj, self.walk_off, self.walk_vtx, self.top_order_map, chop=chop,
                             keep=keep, retain=retain)


def read_reads(path):
    """(uint8 bases, int64 offsets, names) of a FASTA/FASTQ file (ILP_index::read_ip_reads)."""
    L = host_lib()
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = L.phi_reads_read(os.fsencode(path), C.byref(h), err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
    try:
        n = L.phi_reads_count(h)
        off = _view(L.phi_reads_off(h), n + 1, C.c_int64, np.int64).copy()
        bases = _view(L.phi_reads_bases(h), int(off[-1]), C.c_uint8, np.uint8).copy()
        names = [L.phi_reads_name(h, i).decode() for i in range(n)]
    finally:
        L.phi_reads_free(h)
    return bases, off, names


class ILP_index:
    """Mirror of class ILP_index.  Usage follows main.cpp:114-140:

        idx = ILP_index(gfa_path); idx.read_gfa()
        idx.k_mer, idx.window, idx.recombination, idx.threshold, idx.hap_file, idx.hap_name = ...
        reads = []; idx.read_ip_reads(reads, reads_path)
        idx.ILP_function(reads)
    """

    def __init__(self, g, device=0, log=sys.stderr):
        self.g = g                      # path of the GFA (the reference holds a parsed gfa_t*)
        self.device = device
        self.log = log
        # support variables with the reference's defaults (main.cpp:42-47, options.cpp:7-16)
        self.num_threads = 4
        self.hap_file = ""
        self.hap_name = ""
        self.debug = False
        self.k_mer = 31
        self.window = 25
        self.recombination = 100
        self.is_qclp = 1
        self.is_naive_exp = 0
        self.threshold = 1.0
        self.is_mixed = True
        self.max_occ = 5000
        self.bgzf = False               # the FASTA compressed into BGZF blocks on the device (the command line's --bgzf), the name as given
        self.chop = None                # N: segments are cut into pieces of at most N bases first (data/chop_graph.sh:3 `hal2vg --chop 30`)
        self.graph = None
        self.result = None
        self._t0 = time.time()

    # -- ILP_index::read_gfa (ILP_index.cpp:20-155)
    def read_gfa(self):
        self.graph = Graph(self.g)
        self.n_vtx = self.graph.n_vtx
        self.num_walks = self.graph.num_walks
        self.hap_id2name = self.graph.hap_id2name
        self.top_order_map = self.graph.top_order_map

    # -- ILP_index::read_ip_reads (ILP_index.cpp:313-328): appends (name, sequence) pairs
    #    A BAM file (by content, as the command line decides: reads_file_kind) becomes ONE entry, a BamReads: its reads are
    #    decoded on the device when ILP_function scores them, in the place of `samtools fastq` in front of this reader.
    def read_ip_reads(self, ip_reads, ip_reads_file):
        kind = reads_file_kind(ip_reads_file)
        if kind == "bam":
            ip_reads.append(BamReads(ip_reads_file))
            return
        if kind in ("cram", "sam"):
            raise HostError(-5, f"{ip_reads_file} is {kind.upper()}{' text' if kind == 'sam' else ''}: reads are taken from FASTA, FASTQ and BAM only")
        bases, off, names = read_reads(ip_reads_file)
        raw = bases.tobytes()
        for i, nm in enumerate(names):
            ip_reads.append((nm, raw[off[i]:off[i + 1]]))

    def _stamp(self, msg):
        w = time.time() - self._t0
        cpu = time.process_time()
        print(f"[M::ILP_function::{w:.3f}*{cpu / max(w, 1e-9):.2f}] {msg}", file=self.log)

    # -- ILP_index::ILP_function (ILP_index.cpp:528-1601)
    def ILP_function(self, ip_reads):
        if self.graph is None:
            raise PhiError(_capi.PHI_ERR_STATE, "ILP_function before read_gfa")
        G = self.graph
        bams = [r for r in ip_reads if isinstance(r, BamReads)]
        seqs = [r[1] if isinstance(r, tuple) else r for r in ip_reads if not isinstance(r, BamReads)]
        if not bams:
            self._stamp(f"Graph has {G.n_vtx} vertices, {G.num_walks} walks and read has {len(seqs)} reads")
        ctx = Context(self.device)
        try:
            flags = (_capi.PHI_FLAG_QCLP if self.is_qclp else 0) | (_capi.PHI_FLAG_MIXED if self.is_mixed else 0)
            ctx.set_params(k=self.k_mer, w=self.window, threshold=self.threshold, recombination=self.recombination, flags=flags)
            ctx.set_graph(G.seq_concat, G.seq_off, G.adj_off, G.adj, G.walk_off, G.walk_vtx, G.top_order_map, chop=self.chop)
            if self.chop is not None:
                cs = ctx.chop_stats()
                self._stamp(f"Graph chopped to {self.chop} bases: {cs['n_vtx_in']} -> {cs['n_vtx_out']} vertices, "
                            f"{cs['n_entries_in']} -> {cs['n_entries_out']} walk entries")
            ctx.add_reads(seqs)
            for b in bams:
                bi = b.feed(ctx)
                print(f"BAM {b.path}: {bi['n_records']} records, {bi['n_kept']} reads kept ({bi['n_reverse']} reverse), "
                      f"{bi['n_secondary_supplementary']} secondary/supplementary and {bi['n_empty']} without sequence dropped", file=self.log)
            if bams:
                self._stamp(f"Graph has {G.n_vtx} vertices, {G.num_walks} walks and read has {ctx.reads_stats()['n_reads']} reads")
            res = ctx.solve()
            if self.chop is not None:                          # the path in the caller's vertices: (segment, offset of the piece)
                res["path_orig_vtx"], res["path_orig_off"] = ctx.chop_origin(res["path_vtx"])
            hap = ctx.path_sequence(res["hap_len"])
            sharing = ctx.walk_sharing(G.num_walks) if self.debug else None
        finally:
            ctx.close()
        self.result = res
        print("Number of Minimizers", file=self.log)
        for h in range(G.num_walks):
            print(f"{G.hap_id2name[h]} : {int(res['n_minimizers'][h])}", file=self.log)
        if sharing is not None:                                # -d1 (ILP_index.cpp:591-604)
            hist, n_distinct = sharing
            print("Shared fraction of unique kmers by haplotypes", file=self.log)
            for i in range(1, G.num_walks + 1):
                print("[Haplotypes: %d, fraction of unique shared kmers: %.5f]" % (i, np.float32(hist[i]) / np.float32(n_distinct)), file=self.log)
        self._stamp("Haplotypes sketched")
        self._stamp(f"Indexed reads with spectrum size: {res['spectrum_size']}")
        print("Number of Anchors", file=self.log)
        for h in range(G.num_walks):
            print(f"{G.hap_id2name[h]} : {int(res['n_anchors'][h])}", file=self.log)
        sp = max(res["spectrum_size"], 1)
        self._stamp("Filtered/Retained Minimizers: %.2f/%.2f%%" % (np.float32(res["filtered"]) / np.float32(sp) * 100,
                                                                   np.float32(res["retained"]) / np.float32(sp) * 100))
        self._stamp("QP model started" if self.is_qclp else "ILP model started")
        self._stamp("%.2f%% Minimizers are in ILP" % (res["n_in_model"] * 100.0 / sp))
        self._stamp("Minimizer constraints added to the model")
        self._stamp("Using Mixed Integer Programming" if self.is_mixed else "Using Integer Programming")
        self._stamp("Optimized expanded graph constructed")
        self._stamp("Model optimized")
        print(f"Recombination count: {res['recombination_count']}", file=self.log)
        print("Recombined haplotypes: " + self.recombined_segments(res), file=self.log)
        L = host_lib()
        if self.bgzf:
            text, size = C.c_void_p(), C.c_int64()
            rc = L.phi_format_fasta(self.hap_name.encode(), hap, len(hap), C.byref(text), C.byref(size))
            if rc:
                raise HostError(rc, f"cannot format {self.hap_file}")
            try:
                from .context import deflate_bgzf
                packed = deflate_bgzf(np.ctypeslib.as_array(C.cast(text, C.POINTER(C.c_uint8)), shape=(size.value,)), device=self.device)
            finally:
                L.phi_host_free_text(text)
            with open(self.hap_file, "wb") as f:
                f.write(packed)
        else:
            rc = L.phi_write_fasta(os.fsencode(self.hap_file), self.hap_name.encode(), hap, len(hap))
            if rc:
                raise HostError(rc, f"cannot write {self.hap_file}")
        self._stamp(f"Haplotype of size: {len(hap)} written to: {self.hap_file}")
        return res

    def recombined_segments(self, res):
        """The '>(name,[start,end])' list of ILP_index.cpp:1508-1550 (output coordinates)."""
        G = self.graph
        out = []
        str_id = prev = 0
        vt, hp = res["path_vtx"], res["path_hap"]
        if len(vt) == 0:
            return ""
        prev_hap = int(hp[0])
        if "path_orig_vtx" in res:                             # chopped: the pieces' lengths
            ov, oo = res["path_orig_vtx"], res["path_orig_off"]
            lens = np.maximum(0, np.minimum(self.chop, (G.seq_off[ov + 1] - G.seq_off[ov]) - oo))
        else:
            lens = G.seq_off[vt + 1] - G.seq_off[vt]
        for i in range(len(vt)):
            str_id += int(lens[i])
            if i > 0 and int(hp[i]) != prev_hap:
                out.append(f">({G.hap_id2name[prev_hap]},[{prev},{str_id - 1}])")
                prev_hap, prev = int(hp[i]), str_id
        out.append(f">({G.hap_id2name[prev_hap]},[{prev},{str_id - 1}])")
        return "".join(out)


def main(argv=None):
    """`python -m phi_amd.ilp_index -g G -r R -o O [...]`: the reference's main.cpp flow in Python."""
    import argparse
    ap = argparse.ArgumentParser(prog="PHI")
    ap.add_argument("-g", required=True)
    ap.add_argument("-r", required=True)
    ap.add_argument("-o", required=True)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("-w", type=int, default=25)
    ap.add_argument("-R", type=int, default=100)
    ap.add_argument("-q", type=int, default=1)
    ap.add_argument("-m", type=int, default=1)
    ap.add_argument("-T", type=float, default=1.0)
    ap.add_argument("-t", type=int, default=4)
    ap.add_argument("-d", type=int, default=0)
    ap.add_argument("--chop", type=int, default=None)
    ap.add_argument("--bgzf", action="store_true")
    a = ap.parse_args(argv)
    idx = ILP_index(a.g)
    idx.read_gfa()
    idx.num_threads, idx.hap_file, idx.debug = a.t, a.o, bool(a.d)
    idx.hap_name = get_hap_name(a.g, a.r)
    idx.k_mer, idx.window, idx.recombination = a.k, a.w, a.R
    idx.is_qclp, idx.threshold, idx.is_mixed = a.q, a.T, bool(a.m)
    idx.chop = a.chop
    idx.bgzf = a.bgzf
    reads = []
    idx.read_ip_reads(reads, a.r)
    idx.ILP_function(reads)


if __name__ == "__main__":
    main()
