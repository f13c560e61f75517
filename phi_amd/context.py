"""Thin object wrapper over the C ABI: one Context == one phi_ctx (one GPU)."""
import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _capi


class PhiError(RuntimeError):
    def __init__(self, status, detail):
        self.status = status
        self.detail = detail
        super().__init__(f"{_capi.load().phi_strerror(status).decode()} ({status}): {detail}")


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


class Alignments(NamedTuple):
    """Context.edit_alignments: per pair the distance, the counts (M, X, I, D) as an (n, 4) int64 array, the extended
    CIGAR (str, or None) and the alignment identity M * 100 / (M + X + I + D) in percent (float64)."""
    distance: np.ndarray
    counts: np.ndarray
    cigar: list
    identity: np.ndarray


class Context:
    def __init__(self, device=0):
        self._L = _capi.load()
        self._h = C.c_void_p()
        rc = self._L.phi_ctx_create(device, C.byref(self._h))
        if rc:
            raise PhiError(rc, "phi_ctx_create failed (no HIP device?)")
        self.device = device

    def close(self):
        if self._h:
            self._L.phi_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise PhiError(rc, self._L.phi_last_error(self._h).decode())

    # ------------------------------------------------------------------ configuration
    def set_stream(self, hip_stream):
        """Run this context's work on the caller's HIP stream (its handle as an integer); None restores the
        context's private stream.  The null stream has handle 0 and cannot be named through the C ABI (NULL
        means "private stream" there), so 0 is refused instead of silently selecting a stream that is not
        ordered against the caller's work: create an explicit stream (torch.cuda.Stream()) and pass that."""
        if hip_stream is not None and int(hip_stream) == 0:
            raise ValueError("the null stream (handle 0) cannot be shared with a context: pass an explicit stream, or None for the private one")
        self._chk(self._L.phi_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_params(self, k=31, w=25, threshold=1.0, recombination=100, flags=_capi.PHI_FLAG_QCLP | _capi.PHI_FLAG_MIXED):
        self._chk(self._L.phi_set_params(self._h, k, w, C.c_float(threshold), recombination, flags))
        self.k, self.w = k, w

    def set_graph(self, seq_concat, seq_off, adj_off, adj, walk_off, walk_vtx, top_rank, chop=None, keep=None, retain=False, keep_reads=False):
        """Arrays of phi_set_graph: bytes + int64/int32 numpy arrays.  chop=N: every vertex is first cut into pieces of at
        most N bases (phi_set_graph_chopped: what `hal2vg --chop N` does in the reference's pipeline); returns the chopped
        walks' offsets, and path_vtx, kept_anchors ... then speak of the chopped graph (chop_origin maps back).
        keep=mask (one flag per walk): the graph is first reduced to the subgraph induced by the kept walks
        (phi_set_graph_panel, the rule of phi_amd.panel; top_rank is not used: the panel's ranks are made by the library),
        then chopped when chop is given; returns the panel's (chopped) walk offsets, and path_vtx, path_hap ... speak of the
        panel (panel_origin, panel_walks map back).  retain=True keeps the full walk entries on the device: a later call
        with walk_vtx=None and the same walk_off starts from them (panel_release lets them go); after scout_graph the
        entries are retained without it.  keep_reads=True (with keep=mask): a collected read store survives the call, for
        collect_score against the panel's index."""
        seq_off = np.ascontiguousarray(seq_off, np.int64)
        adj_off = np.ascontiguousarray(adj_off, np.int64)
        adj = np.ascontiguousarray(adj, np.int32)
        walk_off = np.ascontiguousarray(walk_off, np.int64)
        walk_vtx = np.ascontiguousarray(walk_vtx, np.int32) if walk_vtx is not None else None     # (None: resolved on the device, phi_walk_text_resolve)
        top_rank = np.ascontiguousarray(top_rank, np.int32) if top_rank is not None else None     # (not used with keep=mask)
        buf = np.frombuffer(seq_concat, np.uint8) if not isinstance(seq_concat, np.ndarray) else seq_concat
        self.n_vtx, self.n_walks = len(seq_off) - 1, len(walk_off) - 1
        if keep is not None:
            keep = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
            if keep.shape != (self.n_walks,):
                raise ValueError(f"keep must hold one flag per walk ({self.n_walks}), not {keep.shape}")
            walk_off_out = np.zeros(int(keep.sum()) + 1, np.int64)
            self._chk(self._L.phi_set_graph_panel(self._h, self.n_vtx, _ptr(buf), _ptr(seq_off), _ptr(adj_off), _ptr(adj),
                                                  self.n_walks, _ptr(walk_off), _ptr(walk_vtx), keep.ctypes.data,
                                                  int(chop) if chop is not None else 0,
                                                  (_capi.PHI_PANEL_RETAIN if retain else 0) | (_capi.PHI_PANEL_KEEP_READS if keep_reads else 0),
                                                  walk_off_out.ctypes.data))
            self.n_walks = len(walk_off_out) - 1
            return walk_off_out
        if retain or keep_reads:
            raise ValueError("retain=True and keep_reads=True go with keep=mask")
        if chop is not None:
            walk_off_out = np.zeros(self.n_walks + 1, np.int64)
            self._chk(self._L.phi_set_graph_chopped(self._h, self.n_vtx, _ptr(buf), _ptr(seq_off), _ptr(adj_off), _ptr(adj),
                                                    self.n_walks, _ptr(walk_off), _ptr(walk_vtx), _ptr(top_rank), int(chop),
                                                    _ptr(walk_off_out)))
            return walk_off_out
        self._chk(self._L.phi_set_graph(self._h, self.n_vtx, _ptr(buf), _ptr(seq_off), _ptr(adj_off), _ptr(adj),
                                        self.n_walks, _ptr(walk_off), _ptr(walk_vtx), _ptr(top_rank)))
        return None

    # ------------------------------------------------------------------ the panel chosen from the reads
    def scout_graph(self, seq_concat, seq_off, adj_off, adj, walk_off, walk_vtx, top_rank):
        """The index of a graph of up to 65 535 walks without the DP (phi_scout_graph): the arrays of set_graph; walk_vtx=None
        takes entries the device holds (walk text resolved there, vcf_graph(wide=True), or retained by a panel or an earlier
        scout with the same walk_off).  Afterwards the reads routes, collect_*, reads_stats, walk_minimizers ... work as on a
        set graph, solve() and what follows it raise PhiError (PHI_ERR_STATE); scout_scores, scout_choose and
        set_graph(..., walk_vtx=None, keep=mask) follow."""
        seq_off = np.ascontiguousarray(seq_off, np.int64)
        adj_off = np.ascontiguousarray(adj_off, np.int64)
        adj = np.ascontiguousarray(adj, np.int32)
        walk_off = np.ascontiguousarray(walk_off, np.int64)
        walk_vtx = np.ascontiguousarray(walk_vtx, np.int32) if walk_vtx is not None else None
        top_rank = np.ascontiguousarray(top_rank, np.int32)
        buf = np.frombuffer(seq_concat, np.uint8) if not isinstance(seq_concat, np.ndarray) else seq_concat
        n_vtx, n_walks = len(seq_off) - 1, len(walk_off) - 1
        self._chk(self._L.phi_scout_graph(self._h, n_vtx, _ptr(buf), _ptr(seq_off), _ptr(adj_off), _ptr(adj), n_walks, _ptr(walk_off),
                                          _ptr(walk_vtx), _ptr(top_rank)))
        self.n_vtx, self.n_walks = n_vtx, n_walks

    def scout_scores(self, n_blocks=0, copy=True):
        """Read support per block of the graph and per walk (phi_scout_scores) from the reads scored so far: (S int32
        [blocks, walks] -- None with copy=False --, info dict: n_blocks, n_walks, n_classes_flagged, n_nonzero, GPU
        milliseconds).  n_blocks=0: one block per 1024 vertices."""
        info = _capi.PhiScoutInfo()
        if not copy or not hasattr(self, "n_vtx"):              # (no graph was ever set: the library says so)
            self._chk(self._L.phi_scout_scores(self._h, int(n_blocks), None, C.byref(info)))
            return None, {n: getattr(info, n) for n, _ in info._fields_}
        nb = int(n_blocks) if n_blocks > 0 else min(65536, max(1, (self.n_vtx + 1023) // 1024))     # (the default of phi_scout_scores)
        S = np.zeros((nb, self.n_walks), np.int32)
        self._chk(self._L.phi_scout_scores(self._h, nb, S.ctypes.data, C.byref(info)))
        return S, {n: getattr(info, n) for n, _ in info._fields_}

    def scout_choose(self, n_want, always=None):
        """The rule of phi_amd.panel.choose_panel on the matrix of the last scout_scores (phi_scout_choose): (keep uint8
        [walks], round_of int32[walks])."""
        keep, round_of = np.zeros(self.n_walks, np.uint8), np.zeros(self.n_walks, np.int32)
        if always is not None:
            always = np.ascontiguousarray(np.asarray(always) != 0, np.uint8)
            if always.shape != (self.n_walks,):
                raise ValueError(f"always must hold one flag per walk ({self.n_walks}), not {always.shape}")
        self._chk(self._L.phi_scout_choose(self._h, always.ctypes.data if always is not None else None, int(n_want), keep.ctypes.data,
                                           round_of.ctypes.data))
        return keep, round_of

    def collect_reads(self, reads, text=False):
        """collect_begin, the reads through add_reads (a list of sequences or (concat, offsets)) or, with text=True, pieces of
        FASTA / FASTQ text through the text route (which must take all of it), collect_end: (reads, bases) in the store."""
        self.collect_begin(0)
        try:
            if text:
                self.reads_text_begin()
                for piece in reads:
                    if self.add_reads_text(piece):
                        raise ValueError("collect_reads: the reads text is irregular (parse it on the host and pass sequences)")
                pending, _ = self.reads_text_end()
                tail = _parse_reads_tail(pending)
                if tail:
                    self.add_reads(tail)
            else:
                self.add_reads(reads)
        finally:
            out = self.collect_end()
        return out

    def collect_score(self):
        """Scores the whole collected store where it lies (phi_reads_collect_score): the read state is then that of a
        context handed the same reads directly."""
        self._chk(self._L.phi_reads_collect_score(self._h))

    def set_graph_vcf(self, vcf_path, fasta_path, max_len=30, keep_samples=None, auto_panel=None, reads=None, always=None, n_blocks=0, text=False,
                      region=None):
        """ "Set graph" from a phased VCF + reference FASTA (the graph of phi_amd.vcf2gfa, no GFA in between): vcf_graph(), then
        phi_set_graph takes the walk entries from where the device left them.  Returns the host graph description (VcfGraph:
        hap_id2name, the arrays, walk_off, n_other_contig / n_ref_mismatch / warnings()) with .stats = vcf_stats() plus host
        seconds per stage.  What phi_set_graph refuses of any graph it refuses here (the context stays usable).
        keep_samples=[names]: a panel, with the reference's semantics (data/chop_graph.sh:46-66) -- the graph is built from
        ALL samples' records, only the kept samples' haplotypes are written as walks (the reference is the sample "REF"), and
        the panel step then removes what no kept walk uses.  v.hap_id2name, v.num_walks and v.walk_off then speak of the kept
        walks, v.kept_haps names them among all haplotypes; path_vtx speaks of the panel graph (panel_origin maps back to
        v's vertices).  The limit of 1022 haplotypes applies to the kept ones.
        auto_panel=N with reads=...: the panel of N haplotypes is chosen from the reads (phi_amd.panel.auto_panel: every
        haplotype's walk is written, up to 65 535, the reads are scored against the index of them all, and the N that lead
        the blocks of the graph are kept; always=[haplotype names] are kept whatever the reads say).  The reads are scored
        against the panel when the call returns: solve() follows.  v.auto holds what the choice did, the rest as with
        keep_samples.  A VCF of at most N haplotypes takes the ordinary route and the reads are added.
        region="NAME", "NAME:BEG" or "NAME:BEG-END" (1-based, inclusive, as tabix and samtools read it): the graph of that
        part of one contig of an indexed BGZF VCF (.tbi) and an indexed FASTA (.fai, .gzi), see vcf_graph; everything else as
        without it, in the region's coordinates (v.region = (name, b, e), 0-based half-open)."""
        import time
        if auto_panel is not None:
            if keep_samples is not None or reads is None:
                raise ValueError("auto_panel=N goes with reads=... and without keep_samples")
            from . import panel as _panel
            v = self.vcf_graph(vcf_path, fasta_path, max_len, wide=True, region=region)
            t4 = time.perf_counter()
            if v.num_walks <= int(auto_panel):
                self.set_graph(v.seq_concat, v.seq_off, v.adj_off, v.adj, v.walk_off, None, v.top_order_map)
                self.collect_reads(reads, text=text)
                self.collect_score()
                v.auto = None
            else:
                mask = None
                if always is not None:
                    missing = [a for a in always if a not in v.hap_id2name]
                    if missing:
                        raise ValueError("the VCF holds no haplotype named " + ", ".join(missing))
                    mask = np.array([n in set(always) for n in v.hap_id2name], np.uint8)
                A = dict(seq_concat=v.seq_concat, seq_off=v.seq_off, adj_off=v.adj_off, adj=v.adj, walk_off=v.walk_off, walk_vtx=None,
                         top_rank=v.top_order_map)
                v.auto = _panel.auto_panel(self, A, reads, int(auto_panel), always=mask, n_blocks=n_blocks, text=text)
                v.kept_haps = np.flatnonzero(v.auto["keep"]).astype(np.int32)
                v.hap_id2name = [v.hap_id2name[h] for h in v.kept_haps.tolist()]
                v.num_walks = len(v.kept_haps)
                v.walk_off = v.auto["walk_off"]
            v.stats["set_graph_s"] = time.perf_counter() - t4
            return v
        v = self.vcf_graph(vcf_path, fasta_path, max_len, keep_samples=keep_samples, region=region)
        t4 = time.perf_counter()
        if keep_samples is None:
            self.set_graph(v.seq_concat, v.seq_off, v.adj_off, v.adj, v.walk_off, None, v.top_order_map)
        else:
            v.walk_off = self.set_graph(v.seq_concat, v.seq_off, v.adj_off, v.adj, v.walk_off, None, None, keep=np.ones(v.num_walks, np.uint8))
        v.stats["set_graph_s"] = time.perf_counter() - t4
        return v

    def vcf_graph(self, vcf_path, fasta_path, max_len=30, keep_samples=None, wide=False, region=None):
        """The VCF route up to "set graph": the host reads the fixed columns and builds the per-vertex arrays
        (ilp_index.VcfGraph), the device parses the genotype text (phi_vcf_genotypes; records it flags go through the host's
        scalar parser) and writes the walk entries (phi_vcf_walks): walk_entries() returns them, set_graph(..., walk_vtx=None)
        takes them.  wide=True: up to 65 535 haplotypes (phi_vcf_walks_wide), for scout_graph.
        region: the host plans which BGZF members of the VCF the .tbi points at and slices the FASTA through .fai / .gzi
        (ilp_index.RegionPlan), the device inflates those members and keeps exactly the region's records
        (phi_vcf_region_filter), and the host's rule pass runs over header + kept lines with positions counted from the
        region's first base; v.stats then also holds phi_vcf_region_info and plan_s / filter_s."""
        import time
        from .ilp_index import VcfGraph
        t0 = time.perf_counter()
        extra = {}
        if region is None:
            v = VcfGraph(vcf_path, fasta_path)
        else:
            from .ilp_index import RegionPlan
            with RegionPlan.open(vcf_path, fasta_path, region) as plan:
                tp = time.perf_counter()
                lines, rinfo = vcf_region_filter(plan.gz, plan.ranges, plan.name, plan.beg, plan.end, device=self.device)
                tf = time.perf_counter()
                v = VcfGraph(None, None, region=plan, lines=lines)
            extra = dict(rinfo, plan_s=tp - t0, filter_s=tf - tp, fasta_members=plan.fasta_members)
        t1 = time.perf_counter()
        n_s, n_r = len(v.samples), v.n_records
        gt = np.zeros((n_r, n_s, 2), np.uint16)
        ploidy = np.zeros(n_s, np.int32)
        flagged = np.zeros(max(n_r, 1), np.uint8)
        self._chk(self._L.phi_vcf_genotypes(self._h, _ptr(v.text), len(v.text), _ptr(v.text_off), _ptr(v.gt_index), n_r, n_s,
                                            _ptr(gt), _ptr(ploidy), _ptr(flagged)))
        for r in np.flatnonzero(flagged[:n_r]).tolist():          # what the kernel left undecided: the exact scalar parser
            v.parse_gt(r, r + 1, gt, ploidy)
        t2 = time.perf_counter()
        v.build(gt, ploidy, max_len)
        t3 = time.perf_counter()
        if keep_samples is not None:                              # the choice columns of the kept haplotypes only
            from .panel import keep_mask
            v.kept_haps = np.flatnonzero(keep_mask(v.hap_id2name, keep_samples=keep_samples)).astype(np.int32)
            if len(v.kept_haps) == 0:
                raise ValueError("keep_samples keeps no haplotype")
            v.choice = np.ascontiguousarray(v.choice[:, v.kept_haps])
            v.hap_id2name = [v.hap_id2name[h] for h in v.kept_haps.tolist()]
            v.num_walks = len(v.kept_haps)
        walk_off = np.zeros(v.num_walks + 1, np.int64)
        choice = np.ascontiguousarray(v.choice, np.int32)
        self._chk((self._L.phi_vcf_walks_wide if wide else self._L.phi_vcf_walks)(self._h, _ptr(v.unit_first), v.n_units, _ptr(v.site_backbone), _ptr(v.site_allele0), v.n_real_sites,
                                        _ptr(choice), v.num_walks, _ptr(walk_off)))
        t4 = time.perf_counter()
        v.walk_off = walk_off
        v.stats = dict(self.vcf_stats(), read_s=t1 - t0, genotypes_s=t2 - t1, build_s=t3 - t2, walks_s=t4 - t3, set_graph_s=0.0, **extra)
        return v

    def vcf_stats(self):
        """What phi_vcf_genotypes / phi_vcf_walks did: bytes of genotype text, records, samples, flagged records, units, entries,
        GPU milliseconds of the two stages."""
        r = _capi.PhiVcfInfo()
        self._chk(self._L.phi_vcf_stats(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in _capi.PhiVcfInfo._fields_}

    def chop_origin(self, vtx):
        """Chopped vertex ids -> (vertex as passed to set_graph(chop=N), base offset of the piece inside it)."""
        vtx = np.ascontiguousarray(vtx, np.int32)
        ov, oo = np.zeros(len(vtx), np.int32), np.zeros(len(vtx), np.int32)
        self._chk(self._L.phi_chop_origin(self._h, _ptr(vtx), len(vtx), _ptr(ov), _ptr(oo)))
        return ov, oo

    def panel_origin(self, vtx):
        """Panel vertex ids -> the vertices as passed to set_graph(keep=mask) (after chop_origin when the panel was chopped)."""
        vtx = np.ascontiguousarray(vtx, np.int32)
        ov = np.zeros(len(vtx), np.int32)
        self._chk(self._L.phi_panel_origin(self._h, _ptr(vtx), len(vtx), _ptr(ov)))
        return ov

    def panel_walks(self):
        """Panel walk ids (path_hap, kept_anchors' walks) -> the walks as passed to set_graph(keep=mask)."""
        n = C.c_int32()
        self._chk(self._L.phi_panel_walks(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        self._chk(self._L.phi_panel_walks(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def panel_stats(self):
        """What set_graph(keep=mask) did: walks, vertices, edges and walk entries before and after, GPU milliseconds of mark,
        scan and remap, host seconds of the array reduction and of Kahn."""
        r = _capi.PhiPanelInfo()
        self._chk(self._L.phi_panel_stats(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in _capi.PhiPanelInfo._fields_}

    def panel_release(self):
        """Lets the full walk entries a set_graph(keep=mask, retain=True) kept on the device go."""
        self._chk(self._L.phi_panel_release(self._h))

    def chop_stats(self):
        """What set_graph(chop=N) did: vertices and walk entries before and after, N, GPU time of the expansion."""
        r = _capi.PhiChopInfo()
        self._chk(self._L.phi_chop_stats(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in _capi.PhiChopInfo._fields_}

    def index_stats(self):
        """Sizes of the de-duplicated walk index (classes of walk entries with equal context) and its GPU time."""
        r = _capi.PhiIndexInfo()
        self._chk(self._L.phi_index_stats(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in _capi.PhiIndexInfo._fields_}

    def solve_stats(self):
        """How the last solve ran its DP: mode (0 every vertex, 1 event chain, 2 blocks on walk lanes, 3 blocks with rows
        on class lanes), blocks, class lanes per block."""
        r = _capi.PhiSolveInfo()
        self._chk(self._L.phi_solve_stats(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in _capi.PhiSolveInfo._fields_}

    def dp_probe(self, weights=None):
        """(tests) One run of the solve's DP, after solve(), with one 0/1 weight per dp anchor (the kept anchors with
        t1 > t0, in kept order; None: all ones).  ends: per walk the best value of a path ending at its last vertex (None: no
        such path); value, end_walk: the best of them, the lowest walk that has it; segs: the argmax path as (walk, first,
        last position in the walk); dp_mode, n_blocks, blk_ring, blk_max_len, max_classes: the strategy of the attempt that
        finished; retries: the fallbacks taken on the way (PHI_DP_RETRY_* or-ed); retries_since_solve: those of every run since
        the last solve began, its own included."""
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, np.uint8)
        ends = np.zeros(max(self.n_walks, 1), np.int32)
        value, end_walk, n_seg = C.c_int64(), C.c_int32(), C.c_int64()
        info = _capi.PhiDpProbeInfo()
        cap = self.n_vtx + 1                                   # (one segment per vertex at most; a chopped graph has more vertices)
        while True:
            sw, s0, s1 = np.zeros(cap, np.int32), np.zeros(cap, np.int64), np.zeros(cap, np.int64)
            self._chk(self._L.phi_dp_probe(self._h, None if w is None else w.ctypes.data, 0 if w is None else len(w), _ptr(ends),
                                           C.byref(value), C.byref(end_walk), _ptr(sw), _ptr(s0), _ptr(s1), cap, C.byref(n_seg), C.byref(info)))
            if n_seg.value <= cap:
                break
            cap = n_seg.value                                  # (the run again, with room for its path)
        n = n_seg.value
        out = {"ends": [None if e == -2 ** 31 else int(e) for e in ends[:self.n_walks].tolist()], "value": value.value,
               "end_walk": end_walk.value, "segs": list(zip(sw[:n].tolist(), s0[:n].tolist(), s1[:n].tolist()))}
        out.update({name: getattr(info, name) for name, _ in _capi.PhiDpProbeInfo._fields_})
        return out

    # ------------------------------------------------------------------ reads
    def add_reads(self, seqs):
        """seqs: list of bytes, or (concat bytes/uint8 array, int64 offsets)."""
        if isinstance(seqs, tuple):
            concat, off = seqs
            concat = np.frombuffer(concat, np.uint8) if not isinstance(concat, np.ndarray) else concat
            off = np.ascontiguousarray(off, np.int64)
        else:
            off = np.zeros(len(seqs) + 1, np.int64)
            np.cumsum([len(s) for s in seqs], out=off[1:])
            concat = np.frombuffer(b"".join(seqs), np.uint8)
        self._chk(self._L.phi_add_reads(self._h, _ptr(concat), _ptr(off), len(off) - 1))

    def reads_text_begin(self, max_chunk_bytes=64 << 20):
        self._chk(self._L.phi_reads_text_begin(self._h, max_chunk_bytes))

    def add_reads_text(self, text):
        """The next bytes of a FASTA / FASTQ text; the records are found on the device.  True when the text is irregular
        (nothing more is taken: finish on the host reader with what reads_text_end hands back + the rest of the stream)."""
        buf = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else text
        irr = C.c_int32()
        self._chk(self._L.phi_add_reads_text(self._h, _ptr(buf), len(buf), C.byref(irr)))
        return bool(irr.value)

    def add_reads_text_parked(self, park, index):
        """add_reads_text with the index-th piece of a TextPark as its bytes."""
        irr = C.c_int32()
        self._chk(self._L.phi_add_reads_text_parked(self._h, park._h, index, C.byref(irr)))
        return bool(irr.value)

    def reads_text_end(self):
        """(bytes handed over but not taken, stream bytes taken as whole records)."""
        p, n, t = C.c_void_p(), C.c_int64(), C.c_int64()
        self._chk(self._L.phi_reads_text_end(self._h, C.byref(p), C.byref(n), C.byref(t)))
        return (C.string_at(p.value, n.value) if n.value else b""), t.value

    def reads_text_last_batch(self):
        """(uint8 bases, int64 offsets) of the records the device took from the last piece of text."""
        nr, nb = C.c_int64(), C.c_int64()
        self._chk(self._L.phi_reads_text_last_batch(self._h, None, 0, None, 0, C.byref(nr), C.byref(nb)))
        bases, off = np.zeros(nb.value, np.uint8), np.zeros(nr.value + 1, np.int64)
        if nr.value:
            self._chk(self._L.phi_reads_text_last_batch(self._h, _ptr(bases), nb.value, _ptr(off), nr.value, C.byref(nr), C.byref(nb)))
        return bases, off

    def reads_text_detach_carry(self):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self._L.phi_reads_text_detach_carry(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    # ------------------------------------------------------------------ reads from BAM: records found and decoded on the device
    def reads_bam_begin(self, max_chunk_bytes=64 << 20, tile_bytes=0):
        """Opens a BAM stream (phi_reads_bam_begin); tile_bytes <= 0: the default tile of the record finder."""
        self._chk(self._L.phi_reads_bam_begin(self._h, int(max_chunk_bytes), int(tile_bytes)))

    def add_reads_bam(self, data):
        """The next INFLATED bytes of a BAM stream, pieces of any size in stream order: the header is consumed, whole
        records are decoded on the device and scored (or collected), the unfinished rest waits for the next piece."""
        buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
        self._chk(self._L.phi_add_reads_bam(self._h, _ptr(buf) if len(buf) else None, len(buf)))

    def add_reads_bam_parked(self, park, index):
        """add_reads_bam with the index-th piece of a TextPark as its bytes."""
        self._chk(self._L.phi_add_reads_bam_parked(self._h, park._h, index))

    def reads_bam_end(self):
        """Closes the stream: the dict of phi_bam_info.  Raises PhiError -- with .info set -- when the stream ends inside its
        header or inside a record, or had failed."""
        info = _capi.PhiBamInfo()
        rc = self._L.phi_reads_bam_end(self._h, C.byref(info))
        d = {n: getattr(info, n) for n, _ in info._fields_}
        if rc:
            e = PhiError(rc, self._L.phi_last_error(self._h).decode())
            e.info = d
            raise e
        return d

    def reads_bam_last_batch(self):
        """(uint8 bases, int64 offsets) of the reads the last piece of the BAM stream gave."""
        nr, nb = C.c_int64(), C.c_int64()
        self._chk(self._L.phi_reads_bam_last_batch(self._h, None, 0, None, 0, C.byref(nr), C.byref(nb)))
        bases, off = np.zeros(nb.value, np.uint8), np.zeros(nr.value + 1, np.int64)
        if nr.value:
            self._chk(self._L.phi_reads_bam_last_batch(self._h, _ptr(bases), nb.value, _ptr(off), nr.value, C.byref(nr), C.byref(nb)))
        return bases, off

    def add_reads_device(self, d_bases, d_read_off, n_reads, n_bases):
        self._chk(self._L.phi_add_reads_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_read_off), n_reads, n_bases))

    def reset_reads(self):
        self._chk(self._L.phi_reset_reads(self._h))

    # ------------------------------------------------------------------ a ladder of coverages from one read set
    def collect_begin(self, first_ordinal=0):
        """From now on every reads route appends its batches to a store on the device instead of scoring them
        (phi_reads_collect_begin); first_ordinal: the ordinal of the first read collected."""
        self._chk(self._L.phi_reads_collect_begin(self._h, int(first_ordinal)))

    def collect_end(self):
        """Stops collecting: (reads, bases) in the store."""
        nr, nb = C.c_int64(), C.c_int64()
        self._chk(self._L.phi_reads_collect_end(self._h, C.byref(nr), C.byref(nb)))
        return nr.value, nb.value

    def collect_release(self):
        self._chk(self._L.phi_reads_collect_release(self._h))

    def ladder_plan(self, seed, fractions):
        """Partitions the collected store into the bands of phi_amd.ladder's rule (phi_ladder_plan); returns phi_ladder_info
        as a dict (band_reads, band_bases, threshold as lists of one entry per level)."""
        f = (C.c_double * len(fractions))(*[float(x) for x in fractions])
        info = _capi.PhiLadderInfo()
        self._chk(self._L.phi_ladder_plan(self._h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), f, len(fractions), C.byref(info)))
        d = {n: getattr(info, n) for n, _ in _capi.PhiLadderInfo._fields_}
        for key in ("band_reads", "band_bases", "threshold"):
            d[key] = list(d[key])[:info.n_levels]
        return d

    def ladder_advance(self, level):
        """Scores the bands up to `level` not scored since the last reset_reads: the read state is then that of a context
        handed exactly that level's reads."""
        self._chk(self._L.phi_ladder_advance(self._h, int(level)))

    def ladder_band(self, band, data=False):
        """The ordinals (int64) of a band's reads in stored order; data=True: (ordinals, uint8 bases, int64 offsets)."""
        n, nb = C.c_int64(), C.c_int64()
        self._chk(self._L.phi_ladder_band(self._h, band, None, 0, C.byref(n), None, 0, None, C.byref(nb)))
        ords = np.zeros(n.value, np.int64)
        bases, off = np.zeros(nb.value, np.uint8), np.zeros(n.value + 1, np.int64)
        self._chk(self._L.phi_ladder_band(self._h, band, _ptr(ords), n.value, C.byref(n), _ptr(bases) if data else None, nb.value,
                                          off.ctypes.data if data else None, C.byref(nb)))
        return (ords, bases, off) if data else ords

    def coverage_ladder(self, reads, coverages, genome_size, seed=0, text=False):
        """One read set inferred at a ladder of coverages (ascending; the reference: data/preprocess.py:83-107 +
        data/run_batch_4.py:38-58): the set is uploaded once, sampled on the device and every base scored once.  reads: a
        list of sequences (or (concat, offsets)) for add_reads, or with text=True an iterable of pieces of FASTA / FASTQ text
        for the text route (which must take all of it).  Yields one dict per level: solve()'s result plus coverage, fraction,
        n_reads and n_bases of the level; the context holds that level's state while the caller looks at it."""
        from . import ladder as _ladder
        self.reset_reads()
        self.collect_begin(0)
        try:
            if text:
                self.reads_text_begin()
                for piece in reads:
                    if self.add_reads_text(piece):
                        raise ValueError("coverage_ladder: the reads text is irregular (parse it on the host and pass sequences)")
                pending, _ = self.reads_text_end()
                tail = _parse_reads_tail(pending)                 # (the device leaves the last record: nothing told it that it had ended)
                if tail:
                    self.add_reads(tail)
            else:
                self.add_reads(reads)
        finally:
            _, total_bases = self.collect_end()
        fr = _ladder.fractions_from_coverage(coverages, genome_size, total_bases)
        info = self.ladder_plan(seed, fr)
        nr = nb = 0
        for j, cv in enumerate(coverages):
            self.ladder_advance(j)
            nr += info["band_reads"][j]
            nb += info["band_bases"][j]
            res = self.solve()
            res.update(coverage=cv, fraction=fr[j], n_reads=nr, n_bases=nb)
            yield res

    def reads_stats(self):
        a, b, e, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.phi_reads_stats(self._h, C.byref(a), C.byref(b), C.byref(e), C.byref(d)))
        return dict(n_reads=a.value, n_bases=b.value, n_emitted=e.value, n_distinct=d.value)

    # ------------------------------------------------------------------ multi-GPU hooks
    def hits_buffer(self):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self._L.phi_hits_buffer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def read_table(self):
        """Device pointer and bucket count of the read table the read kernels probe (phi_read_table)."""
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self._L.phi_read_table(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def spectrum_export(self):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self._L.phi_spectrum_export(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def spectrum_import(self, d_hashes, n):
        self._chk(self._L.phi_spectrum_import(self._h, C.c_void_p(d_hashes), n))

    def spectrum_set_size(self, n):
        self._chk(self._L.phi_spectrum_set_size(self._h, n))

    # ------------------------------------------------------------------ RCCL inside the library
    @staticmethod
    def comm_unique_id():
        """128 bytes (ncclUniqueId) made by one rank; the others receive them out of band."""
        L = _capi.load()
        buf = C.create_string_buffer(_capi.PHI_COMM_ID_BYTES)
        rc = L.phi_comm_unique_id(buf, _capi.PHI_COMM_ID_BYTES)
        if rc:
            raise PhiError(rc, "phi_comm_unique_id failed (librccl missing?)")
        return buf.raw

    def comm_init(self, uid, rank, n_ranks):
        assert len(uid) == _capi.PHI_COMM_ID_BYTES
        self._chk(self._L.phi_comm_init(self._h, C.c_char_p(uid), rank, n_ranks))

    def comm_info(self):
        r, n = C.c_int32(), C.c_int32()
        self._chk(self._L.phi_comm_info(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def comm_allreduce_hits(self):
        self._chk(self._L.phi_comm_allreduce_hits(self._h))

    def comm_exchange(self):
        self._chk(self._L.phi_comm_exchange(self._h))

    # ------------------------------------------------------------------ contexts of one process exchanging through peer-mapped memory
    @staticmethod
    def peers_create(n_ranks):
        g = C.c_void_p()
        rc = _capi.load().phi_peers_create(n_ranks, C.byref(g))
        if rc:
            raise PhiError(rc, "phi_peers_create")
        return g

    @staticmethod
    def peers_destroy(group):
        _capi.load().phi_peers_destroy(group)

    def peers_join(self, group, rank):
        self._chk(self._L.phi_peers_join(self._h, group, rank))

    def peers_allreduce_hits(self):
        self._chk(self._L.phi_peers_allreduce_hits(self._h))

    def peers_exchange(self):
        self._chk(self._L.phi_peers_exchange(self._h))

    # ------------------------------------------------------------------ processes of one node exchanging through mapped hit vectors
    @staticmethod
    def ipc_unique_id():
        """128 bytes (the name of a shared-memory block) made by one rank; the others receive them out of band."""
        L = _capi.load()
        buf = C.create_string_buffer(_capi.PHI_COMM_ID_BYTES)
        rc = L.phi_ipc_unique_id(buf, _capi.PHI_COMM_ID_BYTES)
        if rc:
            raise PhiError(rc, "phi_ipc_unique_id failed")
        return buf.raw

    def ipc_init(self, uid, rank, n_ranks):
        assert len(uid) == _capi.PHI_COMM_ID_BYTES
        self._chk(self._L.phi_ipc_init(self._h, C.c_char_p(uid), rank, n_ranks))

    def ipc_info(self):
        r, n = C.c_int32(), C.c_int32()
        self._chk(self._L.phi_ipc_info(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def ipc_allreduce_hits(self):
        self._chk(self._L.phi_ipc_allreduce_hits(self._h))

    def ipc_flush(self):
        self._chk(self._L.phi_ipc_flush(self._h))

    def ipc_exchange(self):
        self._chk(self._L.phi_ipc_exchange(self._h))

    def ipc_check(self):
        self._chk(self._L.phi_ipc_check(self._h))

    def ipc_destroy(self):
        self._chk(self._L.phi_ipc_destroy(self._h))

    def comm_destroy(self):
        self._chk(self._L.phi_comm_destroy(self._h))

    # ------------------------------------------------------------------ solve
    def set_solve_budget(self, max_dp_runs):
        """DP runs the exact search may use (<= 0: no limit, as the reference's model.optimize())."""
        self._chk(self._L.phi_set_solve_budget(self._h, int(max_dp_runs)))

    def solve(self):
        r = _capi.PhiResult()
        self._chk(self._L.phi_solve(self._h, C.byref(r)))
        nw, npth = r.n_walks, r.n_path
        out = {f: getattr(r, f) for f in ("objective", "upper_bound", "optimal", "n_dp_runs", "n_covered", "n_path",
                                           "recombination_count", "n_switches", "hap_len", "n_walks", "spectrum_size",
                                           "filtered", "retained", "n_in_model")}
        out["path_vtx"] = np.ctypeslib.as_array(r.path_vtx, shape=(npth,)).copy() if npth else np.zeros(0, np.int32)
        out["path_hap"] = np.ctypeslib.as_array(r.path_hap, shape=(npth,)).copy() if npth else np.zeros(0, np.int32)
        out["n_minimizers"] = np.ctypeslib.as_array(r.n_minimizers, shape=(nw,)).copy()
        out["n_anchors"] = np.ctypeslib.as_array(r.n_anchors, shape=(nw,)).copy()
        return out

    def path_sequence(self, hap_len):
        buf = C.create_string_buffer(max(int(hap_len), 1))
        self._chk(self._L.phi_path_sequence(self._h, buf, hap_len))
        return buf.raw[:hap_len]

    # ------------------------------------------------------------------ variant calls against a reference walk
    def calls(self, ref_walk, walk=None):
        """The path of the last solve() (walk=None: phi_calls_path) or walk `walk` of the set graph (phi_calls_walk) as
        variant calls against walk ref_walk, made on the device by the rule of include/phi_amd.h: a dict of n_calls, pos
        (int64, 0-based in bases of the reference walk), ref_off / alt_off (int64[n + 1]), ref_bytes / alt_bytes (bytes),
        anchor (int32: the query index of each call's left anchor), n_shared, n_query, n_ref, ref_span, query_span
        (tuples [first, behind last) in bases) and gpu_ms.  phi_amd.calls has apply() and write_vcf() over it."""
        r = _capi.PhiCalls()
        if walk is None:
            self._chk(self._L.phi_calls_path(self._h, int(ref_walk), C.byref(r)))
        else:
            self._chk(self._L.phi_calls_walk(self._h, int(walk), int(ref_walk), C.byref(r)))
        n = r.n_calls
        out = {f: getattr(r, f) for f in ("n_calls", "n_shared", "n_query", "n_ref", "gpu_ms")}
        out["pos"] = np.ctypeslib.as_array(r.pos, shape=(n,)).copy() if n else np.zeros(0, np.int64)
        out["anchor"] = np.ctypeslib.as_array(r.anchor, shape=(n,)).copy() if n else np.zeros(0, np.int32)
        out["ref_off"] = np.ctypeslib.as_array(r.ref_off, shape=(n + 1,)).copy()
        out["alt_off"] = np.ctypeslib.as_array(r.alt_off, shape=(n + 1,)).copy()
        out["ref_bytes"] = C.string_at(r.ref_bytes, int(out["ref_off"][n])) if out["ref_off"][n] else b""
        out["alt_bytes"] = C.string_at(r.alt_bytes, int(out["alt_off"][n])) if out["alt_off"][n] else b""
        out["ref_span"] = (r.ref_span[0], r.ref_span[1])
        out["query_span"] = (r.query_span[0], r.query_span[1])
        return out

    def calls_stats(self):
        """What the last calls() did (phi_calls_stats): sizes, the algorithmic bytes, GPU milliseconds per stage."""
        r = _capi.PhiCallsInfo()
        self._chk(self._L.phi_calls_stats(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in _capi.PhiCallsInfo._fields_}

    def calls_support(self):
        """The read support of every call of the last calls() (phi_calls_support, the rule of include/phi_amd.h): a dict of
        alt_hit, alt_n, ref_hit, ref_n (int32 per call: the minimiser occurrences that witness the allele, and those of them
        the reads have seen), their totals (<name>_total), n_calls, n_items and gpu_ms.  phi_amd.calls.write_vcf(support=)
        writes them as FORMAT/AK and RK."""
        r = _capi.PhiCallSupport()
        self._chk(self._L.phi_calls_support(self._h, C.byref(r)))
        n = r.n_calls
        out = {f: getattr(r, f) for f in ("n_calls", "alt_hit_total", "alt_n_total", "ref_hit_total", "ref_n_total", "n_items", "gpu_ms")}
        for f in ("alt_hit", "alt_n", "ref_hit", "ref_n"):
            out[f] = np.ctypeslib.as_array(getattr(r, f), shape=(n,)).copy() if n else np.zeros(0, np.int32)
        return out

    def calls_support_stats(self):
        """What the last calls_support() did (phi_calls_support_stats): items, entries visited, records, witnesses, the
        algorithmic bytes, GPU milliseconds."""
        r = _capi.PhiCallsSupportInfo()
        self._chk(self._L.phi_calls_support_stats(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in _capi.PhiCallsSupportInfo._fields_}

    # ------------------------------------------------------------------ evaluation
    def edit_distances(self, a_list, b_list, max_distance=-1):
        """edlib NW edit distance of every pair (a_list[i], b_list[i]) of byte strings on the GPU (phi_edit_distances):
        np.int64 array; -1 where max_distance >= 0 and the distance exceeds it."""
        if len(a_list) != len(b_list):
            raise ValueError("a_list and b_list differ in length")
        n = len(a_list)
        a_off, b_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        np.cumsum([len(s) for s in a_list], out=a_off[1:])
        np.cumsum([len(s) for s in b_list], out=b_off[1:])
        a, b = b"".join(a_list), b"".join(b_list)
        out = np.zeros(n, np.int64)
        self._chk(self._L.phi_edit_distances(self._h, a, _ptr(a_off), b, _ptr(b_off), n, int(max_distance), _ptr(out)))
        return out

    def edit_alignments(self, a_list, b_list, dist=None, cigar=True):
        """One optimal alignment of every pair (query a_list[i], target b_list[i]) on the GPU (phi_edit_alignments):
        Alignments(distance, counts, cigar, identity).  dist: the pairs' distances (phi_edit_distances runs first when
        None); a pair with dist -1 is skipped (counts -1, cigar None, identity nan).  cigar=False: counts only.  The
        identity of two empty sequences is 0, as data/edlib_edits.py gives it."""
        if len(a_list) != len(b_list):
            raise ValueError("a_list and b_list differ in length")
        n = len(a_list)
        if dist is None:
            dist = self.edit_distances(a_list, b_list)
        dist = np.ascontiguousarray(dist, np.int64)
        if dist.shape != (n,):
            raise ValueError("dist must hold one distance per pair")
        a_off, b_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        np.cumsum([len(s) for s in a_list], out=a_off[1:])
        np.cumsum([len(s) for s in b_list], out=b_off[1:])
        a, b = b"".join(a_list), b"".join(b_list)
        counts = np.zeros((n, 5), np.int64)
        buf, c_off = None, None
        if cigar:
            c_off = np.zeros(n + 1, np.int64)
            np.cumsum(np.where(dist >= 0, 11 * (2 * dist + 1), 0), out=c_off[1:])
            buf = C.create_string_buffer(max(int(c_off[-1]), 1))
        self._chk(self._L.phi_edit_alignments(self._h, a, _ptr(a_off), b, _ptr(b_off), n, _ptr(dist), _ptr(counts),
                                               buf, _ptr(c_off)))
        cig = None
        if cigar:
            raw = buf.raw
            cig = [raw[c_off[i]:c_off[i] + counts[i, 4]].decode() if dist[i] >= 0 else None for i in range(n)]
        total = counts[:, :4].sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            ident = np.where(dist < 0, np.nan, np.where(total > 0, counts[:, 0] * 100.0 / np.maximum(total, 1), 0.0))
        return Alignments(dist, counts[:, :4].copy(), cig, ident)

    # ------------------------------------------------------------------ introspection
    def sketch(self, seqs, k, w):
        """Stand-alone minimiser sketch: (hash[], pos[], seq[]) sorted by (seq, pos)."""
        off = np.zeros(len(seqs) + 1, np.int64)
        np.cumsum([len(s) for s in seqs], out=off[1:])
        concat = np.frombuffer(b"".join(seqs), np.uint8)
        n = C.c_int64()
        self._chk(self._L.phi_sketch(self._h, _ptr(concat), _ptr(off), len(seqs), k, w, None, None, None, 0, C.byref(n)))
        h = np.zeros(n.value, np.uint64)
        p = np.zeros(n.value, np.int64)
        s = np.zeros(n.value, np.int32)
        if n.value:
            self._chk(self._L.phi_sketch(self._h, _ptr(concat), _ptr(off), len(seqs), k, w, _ptr(h), _ptr(p), _ptr(s),
                                         n.value, C.byref(n)))
        return h, p, s

    def walk_minimizers(self, walk):
        n = C.c_int64()
        self._chk(self._L.phi_walk_minimizers(self._h, walk, None, None, 0, C.byref(n)))
        h = np.zeros(n.value, np.uint64)
        p = np.zeros(n.value, np.int64)
        if n.value:
            self._chk(self._L.phi_walk_minimizers(self._h, walk, _ptr(h), _ptr(p), n.value, C.byref(n)))
        return h, p

    def walk_sharing(self, n_walks):
        """-d1 histogram: hist[c] = distinct walk minimisers occurring in exactly c walks."""
        hist = np.zeros(n_walks + 1, np.int64)
        n = C.c_int64()
        self._chk(self._L.phi_walk_sharing(self._h, _ptr(hist), n_walks + 1, C.byref(n)))
        return hist, n.value

    def kept_anchors(self):
        n = C.c_int64()
        self._chk(self._L.phi_kept_anchors(self._h, None, None, None, None, 0, C.byref(n)))
        h = np.zeros(n.value, np.uint64)
        wk = np.zeros(n.value, np.int32)
        t0 = np.zeros(n.value, np.int32)
        t1 = np.zeros(n.value, np.int32)
        if n.value:
            self._chk(self._L.phi_kept_anchors(self._h, _ptr(h), _ptr(wk), _ptr(t0), _ptr(t1), n.value, C.byref(n)))
        return h, wk, t0, t1

    def walk_entries(self):
        """(tests) host copy of the walk entries on the device."""
        n = C.c_int64()
        self._chk(self._L.phi_walk_entries(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        if n.value:
            self._chk(self._L.phi_walk_entries(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def gfa_gzip_split(self, data, chunk_bytes=0):
        """A gzip GFA (bytes) inflated and split on this context's device (include/phi_amd.h phi_gfa_gzip_split): the walk
        fields stay there for phi_walk_text_resolve.  Returns (host_text, info): the text with every walk field cut out, as
        bytes, and phi_gfa_gzip_info as a dict (its inflate part a dict of phi_inflate_info).  PhiError(PHI_ERR_INVALID) for
        a corrupt stream, PhiError(PHI_ERR_UNSUPPORTED) when the split refuses."""
        p, n, info = self._gfa_gzip_split_raw(data, chunk_bytes)
        try:
            return C.string_at(p, n) if n else b"", info
        finally:
            self._L.phi_gfa_gzip_free(p)

    def _gfa_gzip_split_raw(self, data, chunk_bytes=0):
        """(pinned host text pointer, its bytes, info): the caller lets it go with phi_gfa_gzip_free."""
        buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
        p, n, info = C.c_void_p(), C.c_int64(), _capi.PhiGfaGzipInfo()
        self._chk(self._L.phi_gfa_gzip_split(self._h, _ptr(buf), len(buf), chunk_bytes, C.byref(p), C.byref(n), C.byref(info)))
        d = {k: getattr(info, k) for k in ("text_bytes", "host_bytes", "walk_bytes", "n_walks")}
        d["inflate"] = _info(info.inflate)
        return p, n.value, d

    def device_synchronize(self):
        self._chk(self._L.phi_device_synchronize(self._h))

    def prefix_sums(self, kind, d_in, n, d_out):
        """(tests) d_out[0 .. n] = exclusive prefix sums of d_in[0 .. n) over device memory given as addresses (include/phi_amd.h
        phi_prefix_sums): kind 0 uint8 -> int32, 1 int32 -> int32 (d_out may be d_in), 2 int32 -> int64."""
        self._chk(self._L.phi_prefix_sums(self._h, kind, C.c_void_p(d_in), n, C.c_void_p(d_out)))

    def prof_enable(self, on=True):
        self._chk(self._L.phi_prof_enable(self._h, int(on)))

    def prof_read(self):
        n, ms, b = C.c_int64(), C.c_double(), C.c_int64()
        self._chk(self._L.phi_prof_read(self._h, C.byref(n), C.byref(ms), C.byref(b)))
        return n.value, ms.value, b.value


def _parse_reads_tail(text):
    """The sequences of the few whole records a reads text ends with (FASTA, or FASTQ with four lines per record)."""
    lines = [ln.rstrip(b"\r") for ln in text.split(b"\n")]
    while lines and not lines[-1]:
        lines.pop()
    if not lines:
        return []
    if lines[0][:1] == b"@":
        if len(lines) % 4:
            raise ValueError("the reads text ends inside a FASTQ record")
        return lines[1::4]
    if lines[0][:1] != b">":
        raise ValueError("the reads text is neither FASTA nor FASTQ")
    seqs = []
    for ln in lines:
        if ln[:1] == b">":
            seqs.append([])
        else:
            seqs[-1].append(ln)
    return [b"".join(s) for s in seqs]


def _info(info):
    return {n: getattr(info, n) for n, _ in _capi.PhiInflateInfo._fields_ if n != "detail"}


def inflate(data, device=0, chunk_bytes=0, finder=True, as_array=False):
    """A gzip file (bytes; any number of members) inflated on `device` (include/phi_amd.h phi_inflate_alloc: one inflate,
    whatever the output's size).  Returns (text, info): text as bytes (a uint8 numpy array with as_array), info a dict of
    phi_inflate_info.  chunk_bytes (0: the default) and finder=False are test knobs.  PhiError(PHI_ERR_INVALID) for a
    corrupt stream."""
    L = _capi.load()
    buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
    flags = 0 if finder else _capi.PHI_INFLATE_NO_FINDER
    p, size, info = C.c_void_p(), C.c_int64(), _capi.PhiInflateInfo()
    rc = L.phi_inflate_alloc(device, _ptr(buf), len(buf), chunk_bytes, flags, C.byref(p), C.byref(size), C.byref(info))
    if rc:
        raise PhiError(rc, info.detail.decode())
    try:
        out = np.empty(size.value, np.uint8)
        if size.value:
            C.memmove(out.ctypes.data, p, size.value)
    finally:
        L.phi_inflate_free(p)
    return (out if as_array else out.tobytes()), _info(info)


def deflate_bgzf(data, device=0, match=True, eof=True, with_info=False):
    """data (bytes or a uint8 array) as a BGZF file written on `device` (include/phi_amd.h phi_deflate_bgzf_alloc): one gzip
    member per 65 280 input bytes, then the 28-byte EOF block (eof=False leaves it out, for outputs that are concatenated).
    match=False writes literals only (a test knob).  Returns the file as bytes, or (bytes, info) with with_info: info a
    dict of phi_deflate_info.  The bytes are a function of data and the two flags alone."""
    L = _capi.load()
    buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    flags = (0 if match else _capi.PHI_DEFLATE_NO_MATCH) | (0 if eof else _capi.PHI_DEFLATE_NO_EOF)
    p, size, info = C.c_void_p(), C.c_int64(), _capi.PhiDeflateInfo()
    rc = L.phi_deflate_bgzf_alloc(device, _ptr(buf) if len(buf) else None, len(buf), flags, C.byref(p), C.byref(size), C.byref(info))
    if rc:
        raise PhiError(rc, info.detail.decode())
    try:
        out = C.string_at(p, size.value) if size.value else b""
    finally:
        L.phi_deflate_free(p)
    if not with_info:
        return out
    return out, {n: getattr(info, n) for n, _ in _capi.PhiDeflateInfo._fields_ if n != "detail"}


def deflate_bgzf_indexed(data, kind, device=0):
    """data as a BGZF file with an index built beside it on `device` (include/phi_amd.h phi_deflate_bgzf_indexed).  kind:
    "gzi" (bgzip's .gzi: where every member begins) or "tbi" (a tabix index with the VCF preset; data is then VCF text), or
    the header's PHI_BGZF_INDEX_* value.  Returns (file, index, info): file is byte for byte deflate_bgzf(data), index the
    finished index file, info a dict of phi_bgzf_index_info with the writer's phi_deflate_info under "deflate".  PhiError
    for a text the index refuses (its detail says which line and why)."""
    L = _capi.load()
    kind = {"gzi": _capi.PHI_BGZF_INDEX_GZI, "tbi": _capi.PHI_BGZF_INDEX_TBI_VCF}.get(kind, kind)
    buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    p, size, q, qsize = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
    info, iinfo = _capi.PhiDeflateInfo(), _capi.PhiBgzfIndexInfo()
    rc = L.phi_deflate_bgzf_indexed(device, _ptr(buf) if len(buf) else None, len(buf), 0, int(kind), C.byref(p), C.byref(size),
                                    C.byref(q), C.byref(qsize), C.byref(info), C.byref(iinfo))
    if rc:
        assert not p.value and not q.value
        raise PhiError(rc, iinfo.detail.decode())
    try:
        out = C.string_at(p, size.value) if size.value else b""
        index = C.string_at(q, qsize.value) if qsize.value else b""
    finally:
        L.phi_deflate_free(p)
        L.phi_deflate_free(q)
    d = {n: getattr(iinfo, n) for n, _ in _capi.PhiBgzfIndexInfo._fields_ if n != "detail"}
    d["deflate"] = {n: getattr(info, n) for n, _ in _capi.PhiDeflateInfo._fields_ if n != "detail"}
    return out, index, d


def vcf_region_filter(gz, ranges, name, beg, end, device=0):
    """The record lines of contig `name` that overlap the 0-based half-open [beg, end), out of the BGZF members gz (bytes) and
    the byte ranges of their inflated text (int64 pairs) that ilp_index.RegionPlan holds: include/phi_amd.h
    phi_vcf_region_filter, what `tabix FILE REGION` prints below the header.  Returns (text, info)."""
    L = _capi.load()
    buf = np.frombuffer(gz, np.uint8) if not isinstance(gz, np.ndarray) else np.ascontiguousarray(gz, np.uint8)
    rng = np.ascontiguousarray(ranges, np.int64).ravel()
    p, size, info = C.c_void_p(), C.c_int64(), _capi.PhiVcfRegionInfo()
    rc = L.phi_vcf_region_filter(device, _ptr(buf) if len(buf) else None, len(buf), _ptr(rng) if len(rng) else None, len(rng) // 2,
                                 name if isinstance(name, bytes) else str(name).encode(), beg, end, C.byref(p), C.byref(size), C.byref(info))
    if rc:
        assert not p.value
        raise PhiError(rc, info.detail.decode())
    try:
        out = C.string_at(p, size.value) if size.value else b""
    finally:
        L.phi_vcf_region_free(p)
    return out, {n: getattr(info, n) for n, _ in _capi.PhiVcfRegionInfo._fields_ if n != "detail"}


def gzip_header(data, pos=0):
    """The offset of the deflate data of the gzip member header at data[pos:] (PhiError when there is none)."""
    L = _capi.load()
    buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
    q = C.c_int64()
    rc = L.phi_gzip_header(_ptr(buf), len(buf), pos, C.byref(q))
    if rc:
        raise PhiError(rc, "no gzip member header")
    return q.value


def crc32_combine(crc_a, crc_b, len_b):
    """zlib.crc32(a + b) from zlib.crc32(a), zlib.crc32(b) and len(b)."""
    return _capi.load().phi_crc32_combine(crc_a, crc_b, len_b)


class TextPark:
    """Pieces of a reads text in device memory before any context wants them (include/phi_amd.h phi_text_park_*)."""

    def __init__(self, device=0):
        self._L = _capi.load()
        self._h = C.c_void_p()
        rc = self._L.phi_text_park_create(device, C.byref(self._h))
        if rc:
            raise PhiError(rc, "phi_text_park_create failed")

    def add(self, text):
        buf = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else text
        idx = C.c_int32()
        rc = self._L.phi_text_park_add(self._h, _ptr(buf), len(buf), C.byref(idx))
        if rc:
            raise PhiError(rc, "phi_text_park_add failed")
        return idx.value

    def add_gzip(self, slices, piece_bytes):
        """A gzip stream given as compressed slices (bytes each), inflated on the park's device and parked as pieces of at
        most piece_bytes in stream order (phi_text_park_gzip_*).  Returns (indices, info)."""
        rc = self._L.phi_text_park_gzip_begin(self._h, piece_bytes)
        if rc:
            raise PhiError(rc, "phi_text_park_gzip_begin failed")
        for sl in slices:
            buf = np.frombuffer(sl, np.uint8) if not isinstance(sl, np.ndarray) else sl
            rc = self._L.phi_text_park_gzip_add(self._h, _ptr(buf), len(buf))
            if rc:
                raise PhiError(rc, "phi_text_park_gzip_add failed")
        first, count, info = C.c_int32(), C.c_int32(), _capi.PhiInflateInfo()
        rc = self._L.phi_text_park_gzip_end(self._h, C.byref(first), C.byref(count), C.byref(info))
        if rc:
            raise PhiError(rc, info.detail.decode())
        return list(range(first.value, first.value + count.value)), _info(info)

    def fetch(self, index):
        n = self._L.phi_text_park_bytes(self._h, index)
        if n < 0:
            raise PhiError(-1, "no such piece")
        out = np.zeros(n, np.uint8)
        rc = self._L.phi_text_park_fetch(self._h, index, _ptr(out), n)
        if rc:
            raise PhiError(rc, "phi_text_park_fetch failed")
        return out.tobytes()

    def release(self, index):
        rc = self._L.phi_text_park_release(self._h, index)
        if rc:
            raise PhiError(rc, "phi_text_park_release failed")

    def close(self):
        if self._h:
            self._L.phi_text_park_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
