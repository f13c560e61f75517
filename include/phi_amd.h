/*
 * phi_amd.h -- C ABI of the MI355X-native PHI hot path (libphi_amd.so).
 *
 * The reference (at-cg/PHI) has no FFI seam: its hot path is the C++ member function
 * ILP_index::ILP_function (src/ILP_index.cpp:528-1601) reading public fields that
 * ILP_index::read_gfa (src/ILP_index.cpp:20-155) fills.  This header is the seam a maintainer
 * binds instead (INTEGRATION.md shows the patch to src/main.cpp:114-140): plain pointers and
 * sizes, no C++ or torch types.  Every entry point cites the reference interface it replaces.
 *
 * Conventions
 *   - every function returns 0 (PHI_OK) or a negative phi_status; nothing calls exit();
 *   - host pointers are borrowed for the duration of the call and copied;
 *   - result buffers are owned by the context and stay valid until the next phi_solve /
 *     phi_ctx_destroy;
 *   - one context per process per GPU, calls serialised by the caller (the reference is not
 *     re-entrant either: src/main.cpp:136-140).
 *
 * Limits (PHI_ERR_UNSUPPORTED / PHI_ERR_INVALID beyond them): k <= 64 (k <= 32 on the fast 2-bit kernels; 33 .. 64 through
 * the exact byte-wise routine, and only while no k-mer covers more than 32 vertices), w <= 256, at most 1022 walks (one per lane of the largest workgroup: 513 and more run a slower instance of the dense DP kernel),
 * at most 2^32 - 64 walk entries (2.5 G solved: profiles/wide_entries.py), fewer than 2^31 minimisers of the distinct walk
 * contexts, anchors in the model and walk entries on vertices with recombination edges, at most
 * 254 out-edges and 255 recombination in-edges per vertex, no walk through a segment without
 * sequence, no graph whose walks both start and end at interior vertices.  phi_set_graph_chopped: the same limits hold
 * for the CHOPPED graph (at most 2^31 - 1 pieces, at most 2^32 - 64 chopped walk entries).  phi_vcf_genotypes / phi_vcf_walks:
 * one contig, fewer than 2^31 kept records, genotype text + matrix (4 bytes per record and sample) within device memory, fewer
 * than 65 535 ALT alleles per record, at most 1022 kept haplotypes (reference
 * included) and 2^32 - 64 walk entries, as for any graph.  phi_add_reads_bam: BAM alignment records only (CRAM and SAM text are
 * not read), a header of at most 1 GB, a record no longer than the stream's carry buffer (half of max_chunk_bytes, 16 MB at
 * least; PHI_ERR_UNSUPPORTED beyond), the default filter of `samtools fastq` (flag & 0x900 == 0) and no other; not compared
 * with samtools itself.  A BAM stream's device buffers -- two of (carry + max_chunk_bytes), twice that for the decoded bases and
 * about 0.7 of it in tables: some 450 MB at a 64-MB chunk -- stay with the context until phi_ctx_destroy, as the text stream's do.
 */
#ifndef PHI_AMD_H
#define PHI_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phi_ctx phi_ctx;

typedef enum {
    PHI_OK = 0,
    PHI_ERR_INVALID = -1,      /* bad argument (null pointer, k/w out of range, offsets not monotone) */
    PHI_ERR_NOMEM = -2,        /* host or device allocation failed */
    PHI_ERR_DEVICE = -3,       /* HIP runtime error, kernel fault, no gfx950 device */
    PHI_ERR_STATE = -4,        /* call order violated (e.g. phi_solve before phi_set_graph) */
    PHI_ERR_UNSUPPORTED = -5,  /* input the path does not handle: see phi_last_error() */
    PHI_ERR_WALK = -6,         /* walk does not follow graph edges / reverse-strand vertex:
                                  the reference exit(1)s at ILP_index.cpp:104-107, :1568-1572 */
    PHI_ERR_OVERFLOW = -7      /* an internal table overflowed its capacity */
} phi_status;

const char *phi_strerror(int status);
/* Human-readable detail of the last failure on this context ("" if none). */
const char *phi_last_error(const phi_ctx *ctx);

/* ILP_index::ILP_index(gfa_t*) (ILP_index.cpp:4-6).  device_id = HIP device ordinal.  Also pays the one-time costs of the
 * HIP runtime on this device (code objects of the kernels, staging of the first host copy: ~10 ms) so that they do not
 * fall into the first phi_set_graph / phi_solve: create the context while the graph file is being parsed. */
int phi_ctx_create(int device_id, phi_ctx **out);
void phi_ctx_destroy(phi_ctx *ctx);

/* Run all work of this context on the caller's HIP stream (hipStream_t passed as void*);
 * NULL restores the context's private stream, which is non-blocking: it is NOT ordered against
 * the null stream.  A caller that shares buffers with this context (phi_hits_buffer,
 * phi_add_reads_device, phi_spectrum_export) passes the stream its own work runs on, or
 * synchronises the device. */
int phi_set_stream(phi_ctx *ctx, void *hip_stream);

/* Flags of phi_set_params. */
#define PHI_FLAG_QCLP 1u       /* -q1 (main.cpp:66): accepted; both programs have the same optimum */
#define PHI_FLAG_MIXED 2u      /* -m1 (main.cpp:62): accepted; integral optimum of equal value exists */

/* main.cpp:118-131: k_mer, window, threshold, recombination, is_qclp/is_mixed.
 * k in [1,64] (33 .. 64: exact but slow, see the limits above), w in [1,256].  Must precede phi_set_graph. */
int phi_set_params(phi_ctx *ctx, int32_t k, int32_t w, float threshold, int32_t recombination,
                   uint32_t flags);

/*
 * ILP_index::read_gfa's outputs (ILP_index.h:53-61) as flat arrays, then stage 1a of
 * ILP_function (:559-573): the graph goes to HBM, every walk is sketched on the GPU and the
 * minimiser table is built.
 *   seq_concat/seq_off[n_vtx+1]  node_seq, original case
 *   adj_off[n_vtx+1]/adj         adj_list (forward strand)
 *   walk_off[n_walks+1]/walk_vtx paths
 *   topo_rank[n_vtx]             top_order_map
 */
int phi_set_graph(phi_ctx *ctx, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off,
                  const int64_t *adj_off, const int32_t *adj, int32_t n_walks,
                  const int64_t *walk_off, const int32_t *walk_vtx, const int32_t *topo_rank);

/*
 * The same with the graph chopped first (data/chop_graph.sh:3 `hal2vg --chop 30`, :62 `gfa2gbwt -m 30`: the reference's
 * pipeline never hands PHI a graph as the builder wrote it, since the model switches haplotypes at vertex borders only and
 * ignores anchors inside one vertex).  A vertex of L bases becomes max(1, ceil(L / max_len)) pieces, full pieces first;
 * the pieces of vertex v get the consecutive ids first[v] + j (first = exclusive prefix sum of the piece counts in vertex
 * order); edges piece j -> j + 1, and last piece of u -> first piece of v for every edge (u, v), a vertex's out-edges in
 * their order; topological rank = prefix sum of the counts in topological order + j; every walk entry is replaced by its
 * vertex's pieces.  The per-vertex arrays are chopped on the host, the walk entries on the device (chop.hip): walk_vtx may
 * be host entries (uploaded unchopped) or NULL after phi_walk_text_resolve (expanded where they lie).  walk_off_out
 * [n_walks + 1] (may be NULL) receives the chopped walks' offsets.  max_len < 1: PHI_ERR_INVALID.  More than 2^31 - 1
 * pieces or more than 2^32 - 64 chopped entries: PHI_ERR_UNSUPPORTED, decided from the counts before the chopped entries
 * are allocated; the context stays usable.  Whatever phi_set_graph refuses is refused the same way (vertex ids in such a
 * message are the chopped graph's); on failure the context holds no graph.  max_len >= the longest vertex: the graph as
 * passed in, same ids, same result as phi_set_graph.  Everything downstream (phi_solve's path_vtx, phi_kept_anchors, ...)
 * speaks of the chopped graph.
 */
int phi_set_graph_chopped(phi_ctx *ctx, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off,
                          const int64_t *adj_off, const int32_t *adj, int32_t n_walks,
                          const int64_t *walk_off, const int32_t *walk_vtx, const int32_t *topo_rank,
                          int32_t max_len, int64_t *walk_off_out);
/* data/chop_graph.sh:3,62 undone for reporting: chopped vertex id vtx[i] -> the vertex as passed to phi_set_graph_chopped
 * (orig_vtx[i]) and the base offset of the piece inside it (orig_off[i]); either output may be NULL.  PHI_ERR_STATE when
 * the context's graph was not set chopped, PHI_ERR_INVALID for an id outside the chopped graph. */
int phi_chop_origin(phi_ctx *ctx, const int32_t *vtx, int64_t n, int32_t *orig_vtx, int32_t *orig_off);
/* What the chop (data/chop_graph.sh:3,62) did: vertices and walk entries before and after, and expand_gpu_ms = count + scan +
 * expand of the walk entries by HIP events on the context's stream (0 when nothing had to be chopped).  PHI_ERR_STATE when
 * the context's graph was not set chopped. */
typedef struct {
    int64_t n_vtx_in, n_vtx_out;
    int64_t n_entries_in, n_entries_out;
    int32_t max_len;
    double expand_gpu_ms;
} phi_chop_info;
int phi_chop_stats(phi_ctx *ctx, phi_chop_info *out);

/*
 * "Set graph" against a PANEL: a chosen subset of the graph's haplotypes.  The reference builds one graph from the full VCF
 * (data/chop_graph.sh:46-50), removes samples from the haplotype index (data/chop_graph.sh:51-61 `vg gbwt ... -R SAMPLE`, the
 * sample lists drawn nested by data/get_ids.py and data/get_ids_2.py), writes one GFA per panel (data/chop_graph.sh:62-66) and
 * runs PHI once per panel (data/run_batch_9.py to run_batch_13.py); leave-one-out evaluation is the same operation.
 *
 * THE RULE.  Given a graph and a flag per walk (keep[h] != 0), the panel graph is the subgraph induced by the kept walks:
 *   vertices   those on at least one kept walk, in their old order; the new id is the number of kept vertices before it;
 *   edges      the edges (u, v) that at least one kept walk steps along, in their old order within u's list; an edge whose
 *              two ends are kept but which no kept walk uses is dropped (what a graph induced by a haplotype index holds);
 *   walks      the kept walks in their old order, renumbered from 0, their entries renamed;
 *   ranks      the topological ranks the host reader gives the panel graph -- Kahn's algorithm with a FIFO queue, sources in
 *              id order (ILP_index.cpp:115-154) --, NOT the old ranks compressed: the two can differ, and ranks break ties.
 * The rule is applied uniformly: with every walk kept, vertices and edges on no walk still go.  With these ranks the result
 * is what phi_set_graph gives for the GFA minus the W-lines of the dropped walks and the S- and L-lines nothing uses any
 * more.  Believed to be what `gfa2gbwt -d` writes after `vg gbwt -R`; not compared with `vg`.
 *
 *   phi_set_graph_panel  (data/chop_graph.sh:46-66) the arrays of phi_set_graph without topo_rank (the panel's ranks are made
 *                        here).  walk_vtx: host entries, or NULL for entries on the device -- freshly resolved there
 *                        (phi_walk_text_resolve, phi_vcf_walks) or retained by an earlier call.  The kept entries are marked
 *                        and renamed on the device (panel.hip), the per-vertex arrays reduced on the host.  max_len > 0 then
 *                        chops the PANEL graph (phi_set_graph_chopped: phi_chop_origin names (panel vertex, offset));
 *                        max_len <= 0: no chop.  walk_off_out[kept walks + 1] (may be NULL): the panel's (chopped) walk
 *                        offsets.  flags: PHI_PANEL_RETAIN keeps the FULL entries on the device after the call, so that a
 *                        later call with walk_vtx = NULL and the same walk_off starts from them (a ladder of panels from
 *                        one upload or one device-side resolve); they stay until phi_panel_release, a retaining call that
 *                        replaces them, or a call without the flag that starts from them.  walk_vtx = NULL with neither:
 *                        PHI_ERR_STATE.  No walk kept: PHI_ERR_INVALID; more than 1022 KEPT walks: PHI_ERR_UNSUPPORTED (the
 *                        input's walk count is not limited); both decided before anything is allocated, the context and
 *                        walks resolved on the device as they were.  A kept walk holding a vertex out of range:
 *                        PHI_ERR_WALK, naming the walk and the vertex as passed in (a dropped walk's entries are not looked
 *                        at).  A cycle: PHI_ERR_INVALID in the host reader's words.  Whatever phi_set_graph refuses of the
 *                        panel graph is refused the same way, ids in such a message being the panel graph's; on failure the
 *                        context holds no graph.  Everything downstream (phi_solve's path_vtx and path_hap,
 *                        phi_kept_anchors, phi_walk_minimizers, ...) speaks of panel vertices and panel walks.
 *   phi_panel_origin     (data/chop_graph.sh:51-66 undone for reporting) panel vertex vtx[i] -> the vertex as passed in.
 *   phi_panel_walks      (data/chop_graph.sh:51-61 undone for reporting) orig_walk[0, *n_kept): panel walk -> the walk as passed
 *                        in; nothing is copied when cap is too small.
 *   phi_panel_stats      (data/chop_graph.sh:46-66) walks, vertices, edges and walk entries before and after; the GPU
 *                        milliseconds of mark, scan and remap by HIP events on the context's stream; the host seconds of the
 *                        array reduction and of Kahn.
 *   phi_panel_release    (data/run_batch_9.py to run_batch_13.py: the ladder is over) lets retained entries go.
 * The three accessors give PHI_ERR_STATE when the context's graph was not set as a panel.
 */
#define PHI_PANEL_RETAIN 1u
typedef struct {
    int32_t n_walks_in, n_walks_out;
    int64_t n_vtx_in, n_vtx_out;
    int64_t n_edges_in, n_edges_out;
    int64_t n_entries_in, n_entries_out;
    double mark_gpu_ms, scan_gpu_ms, remap_gpu_ms;
    double reduce_host_s, kahn_host_s;
} phi_panel_info;
int phi_set_graph_panel(phi_ctx *ctx, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off,
                        const int64_t *adj_off, const int32_t *adj, int32_t n_walks,
                        const int64_t *walk_off, const int32_t *walk_vtx, const uint8_t *keep,
                        int32_t max_len, uint32_t flags, int64_t *walk_off_out);
int phi_panel_origin(phi_ctx *ctx, const int32_t *vtx, int64_t n, int32_t *orig_vtx);
int phi_panel_walks(phi_ctx *ctx, int32_t *orig_walk, int32_t cap, int32_t *n_kept);
int phi_panel_stats(phi_ctx *ctx, phi_panel_info *out);
int phi_panel_release(phi_ctx *ctx);
/* phi_set_graph_panel, further flag: a collected read store (phi_reads_collect_end done) survives the call, so that the same
 * reads can be scored against the panel's index with phi_reads_collect_score; a ladder plan is dropped and the read state is
 * reset as ever.  Without the flag the store goes with the graph it was collected under, as before. */
#define PHI_PANEL_KEEP_READS 2u

/*
 * THE PANEL CHOSEN FROM THE READS: graphs of more walks than the DP takes (1022).  The reference lists them as future work
 * and is compared with a tool that answers the question from the reads' k-mers before anything is inferred
 * (data/vg_haplotypes.py:21-29: `vg haplotypes` samples haplotypes by k-mer counts of the read set); its own panels are drawn
 * by name (data/chop_graph.sh:46-66).  The calls below stand in for that step: index the full graph without the DP, score the
 * reads once, count per stretch of the graph and per walk how many of the walk's minimiser occurrences the reads hit, choose
 * the walks that lead somewhere, and set the panel.  THE RULE OF THE CHOICE IS THIS PROJECT'S OWN: it is not `vg haplotypes`'
 * (no diploid sampling, no k-mer presence/absence scoring against a haplotype index) and has not been compared with it.
 *
 *   phi_scout_graph   (stands in for the index `vg haplotypes` reads, data/vg_haplotypes.py:21-29, and for the full graph of
 *                     data/chop_graph.sh:46-50)  The arrays of phi_set_graph; up to 65 535 walks.  Builds the index only
 *                     -- classes of walk entries, class records, walk-minimiser table, read table, hit vectors -- and none of
 *                     the DP's tables; no host copy of the walk entries is kept.  walk_vtx == NULL: the entries are on the
 *                     device, left there by phi_walk_text_resolve, phi_vcf_walks_wide or retained by a panel call (or an
 *                     earlier scout) with the same walk_off.  Afterwards the context is in state SCOUT and the full entries
 *                     count as retained (PHI_PANEL_RETAIN): phi_set_graph_panel(..., walk_vtx = NULL, ...) with the same
 *                     walk_off starts from them and keeps them.  On a scout every reads route, phi_reads_collect_*,
 *                     phi_reset_reads, phi_reads_stats, phi_hits_buffer, phi_index_stats, phi_walk_minimizers and
 *                     phi_walk_sharing work as on a set graph; phi_solve, phi_kept_anchors, phi_solve_stats,
 *                     phi_path_sequence, the phi_comm_ / phi_ipc_ / phi_peers_ exchanges and the panel and chop accessors
 *                     return PHI_ERR_STATE with a message that names the scout.  Any phi_set_graph* call ends the state.
 *                     More than 65 535 walks: PHI_ERR_UNSUPPORTED; whatever phi_set_graph refuses of the arrays, the topology
 *                     or the walks is refused the same way, except what only the DP's model forbids (walks that both start
 *                     and end at interior vertices).
 *   phi_scout_scores  (data/vg_haplotypes.py:21-29, the k-mer counting)  Vertex v lies in block (int64)topo_rank[v] *
 *                     n_blocks / n_vtx; n_blocks <= 0: min(65 536, max(1, ceil(n_vtx / 1024))).  S[b * n_walks + h] = the
 *                     number of minimiser occurrences (hash, pos) of walk h -- exactly the list phi_walk_minimizers(h)
 *                     returns -- whose hash has its hit flag set in the current read generation and whose base pos (the
 *                     k-mer's first base) lies in a vertex of block b.  The matrix is zeroed by the call, computed on the
 *                     device (panel_score.hip) and stays there for phi_scout_choose until the scout state ends (4 bytes a
 *                     cell, below 8 GB; any phi_set_graph* frees it); scores (host, may be NULL) receives a copy.  More than 65 536 blocks or n_blocks * n_walks >= 2^31: PHI_ERR_INVALID.  Not a scout:
 *                     PHI_ERR_STATE.
 *   phi_scout_choose  (data/vg_haplotypes.py:21-29 the sampling, data/chop_graph.sh:51-61 the list of names)  Copies the matrix
 *                     of the last phi_scout_scores to the host and applies phi_panel_choose (include/phi_host.h has the
 *                     rule): keep[n_walks], round_of[n_walks] (may be NULL).
 */
typedef struct {
    int32_t n_blocks, n_walks;
    int64_t n_classes_flagged;        /* classes with a record in another block than their first record's */
    int64_t n_nonzero;                /* cells of the matrix that are not 0 */
    double record_gpu_ms, class_gpu_ms, entry_gpu_ms;   /* HIP events on the context's stream */
    double walk_sum_gpu_ms;           /* with PHI_SCOUT_REF set (profiles): the per-walk minimiser count kernel over the same entries
                                         in the same call, which reads the same 4 bytes and one gather per entry; else 0 */
} phi_scout_info;
int phi_scout_graph(phi_ctx *ctx, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off,
                    const int64_t *adj_off, const int32_t *adj, int32_t n_walks,
                    const int64_t *walk_off, const int32_t *walk_vtx, const int32_t *topo_rank);
int phi_scout_scores(phi_ctx *ctx, int32_t n_blocks, int32_t *scores, phi_scout_info *info);
int phi_scout_choose(phi_ctx *ctx, const uint8_t *always, int32_t n_want, uint8_t *keep, int32_t *round_of);

/*
 * "Set graph" from a phased multi-sample VCF + reference FASTA (the reference's second input route, vcf2gfa.py:27-64: `vg construct
 * | vg gbwt | gfa2gbwt -m 30`, here the rule of phi_amd/vcf2gfa.py) without a GFA in between.  The host reads the small parts
 * and builds the per-vertex arrays (include/phi_host.h phi_vcf_read, phi_vcf_build); the device parses the genotype text, the
 * bulk of a VCF's bytes, and writes the walk entries, which at panel scale exist only in device memory:
 *   phi_vcf_genotypes   vcf2gfa.py:27-64, the GT columns.  text[n_text]: the sample columns of the kept records back to back,
 *                       record r's slice at [text_off[r], text_off[r + 1] - 1) with ONE line feed behind it (phi_vcf_text of
 *                       phi_host.h); gt_index[r] = index of GT in FORMAT.  Sample s's field stands behind the slice's s-th tab; its
 *                       GT part is the gt_index-th ':'-separated part; '/' reads as '|'; the first two '|'-separated parts give
 *                       gt[(r * n_samples + s) * 2 + {0, 1}] (uint16: a non-empty run of ASCII digits is its value, anything
 *                       else 0); ploidy[s] = max over records of min(2, parts other than ".").  flagged[r] != 0: the kernel did
 *                       not decide record r (a value of more than four digits, fewer fields than samples, fewer ':' parts than
 *                       gt_index + 1, a GT part of kilobytes) and nothing of its row is to be trusted: phi_vcf_parse_gt
 *                       (phi_host.h) over that row fills it and raises ploidy, or reports the error.  Nothing is guessed.
 *   phi_vcf_walks       vcf2gfa.py:27-64, the W-lines.  From phi_vcf_build's tables -- unit_first[n_units + 1], per site its
 *                       backbone unit and first allele unit, choice[site * n_haps + haplotype] -- every haplotype's walk over
 *                       units (2 * n_sites + 1 entries: backbone, allele, ..., last backbone = unit n_units - 1), expanded to
 *                       segment ids by the count / scan / expand of phi_set_graph_chopped (chop.hip).  The entries and
 *                       walk_off_out[n_haps + 1] are left where phi_walk_text_resolve leaves them: phi_set_graph(..., walk_vtx =
 *                       NULL, ...) and phi_walk_entries follow unchanged.  More than 1022 haplotypes or 2^32 - 64 entries:
 *                       PHI_ERR_UNSUPPORTED, decided before the entries are allocated; the context stays usable and walks
 *                       an earlier call left on the device are as they were.
 *   phi_vcf_stats       what the last two calls did; the GPU milliseconds by HIP events on the context's stream.
 */
typedef struct {
    int64_t text_bytes;               /* genotype text uploaded */
    int64_t n_records;
    int32_t n_samples;
    int64_t n_flagged;                /* records left to the host's scalar parser */
    int64_t n_units, n_entries;       /* phi_vcf_walks: units of the graph, walk entries written */
    double genotype_gpu_ms, walks_gpu_ms;
} phi_vcf_info;
int phi_vcf_genotypes(phi_ctx *ctx, const char *text, int64_t n_text, const int64_t *text_off, const int32_t *gt_index, int64_t n_records,
                      int32_t n_samples, uint16_t *gt, int32_t *ploidy, uint8_t *flagged);
int phi_vcf_walks(phi_ctx *ctx, const int32_t *unit_first, int64_t n_units, const int32_t *site_backbone, const int32_t *site_allele0,
                  int64_t n_sites, const int32_t *choice, int32_t n_haps, int64_t *walk_off_out);
/* phi_vcf_walks for every haplotype of a population VCF (the input of data/vg_haplotypes.py:21-29 and of the full graph of
 * data/chop_graph.sh:46-50): the same call with the limit of phi_scout_graph, 65 535 haplotypes, in the place of the DP's 1022.
 * The entries are left for phi_scout_graph or phi_set_graph_panel (walk_vtx = NULL). */
int phi_vcf_walks_wide(phi_ctx *ctx, const int32_t *unit_first, int64_t n_units, const int32_t *site_backbone, const int32_t *site_allele0,
                       int64_t n_sites, const int32_t *choice, int32_t n_haps, int64_t *walk_off_out);
int phi_vcf_stats(phi_ctx *ctx, phi_vcf_info *out);

/*
 * Stage 1b/2a of ILP_function (:617-655) for one batch of reads: sketch, spectrum insert,
 * match against the walk minimiser table.  Streaming: may be called repeatedly.
 * bases = raw ASCII (upper/lower case; any byte), read r = bases[read_off[r], read_off[r+1]).
 */
int phi_add_reads(phi_ctx *ctx, const char *bases, const int64_t *read_off, int64_t n_reads);
/* Same, with both arrays already resident in this GPU's HBM (n_bases = read_off[n_reads]).  d_read_off may be NULL for reads of
 * ONE length (n_bases / n_reads each, as sequencers write short reads): the kernel then computes the read starts and reads no offsets. */
int phi_add_reads_device(phi_ctx *ctx, const void *d_bases, const void *d_read_off, int64_t n_reads,
                         int64_t n_bases);
/*
 * The same stage fed with the reads file's TEXT (FASTA or FASTQ, already inflated), in pieces of any size in file order:
 * the records are found on the device (kseq's rules, src/kseq.h:192-233, ILP_index.cpp:313-328, for the two regular
 * layouts: FASTQ with four lines per record; FASTA, wrapped or not) instead of by a byte-at-a-time state machine on one
 * host core, and piece i + 1 crosses the link while piece i is sketched.
 *   phi_reads_text_begin   start a stream; max_chunk_bytes sizes the device buffers (a longer piece is cut)
 *   phi_add_reads_text     the next bytes of the stream.  The device takes the whole records it finds and keeps the
 *                          unfinished rest for the next call.  *irregular = 1: the text is not laid out in one of the
 *                          two regular ways (carriage returns, a wrapped FASTQ record, text before the first header,
 *                          a record longer than the buffers ...): nothing more is taken, further calls fail with
 *                          PHI_ERR_STATE, and the caller finishes the stream on the exact host reader (phi_host.h)
 *   phi_reads_text_end     ends the stream and hands back the bytes handed over but NOT taken (valid until the next
 *                          phi_reads_text_begin) -- after an irregular piece: everything from the first byte not taken
 *                          to the end of that call's bytes; at the end of a regular file: the last record, whose end
 *                          only the end of the file shows -- to be parsed by the host reader and added with
 *                          phi_add_reads; *n_taken = bytes of the stream taken as whole records.
 * Together the device-side records and the host-parsed rest are exactly kseq's records of the file.
 */
int phi_reads_text_begin(phi_ctx *ctx, int64_t max_chunk_bytes);
int phi_add_reads_text(phi_ctx *ctx, const char *text, int64_t n_bytes, int32_t *irregular);
int phi_reads_text_end(phi_ctx *ctx, const char **pending, int64_t *n_pending, int64_t *n_taken);
/* Introspection for the parity tests: the records the device took from the LAST piece handed to phi_add_reads_text (their
 * bases back to back and their offsets, off[0] = 0), copied to the host.  Sizes only when the buffers are too small. */
/*
 * Reads text that arrives BEFORE the graph is there (the command line: the reads file is read while the GFA is parsed and the
 * index built -- seconds at chromosome scale, with the link and 288 GB of HBM idle).  A park holds pieces of the stream in
 * device memory; it belongs to no context (its own stream and buffers), so a reader thread may fill it while phi_set_graph
 * runs on another thread.  phi_add_reads_text_parked is phi_add_reads_text with the index-th piece as its bytes (the pieces in
 * stream order, mixed freely with phi_add_reads_text calls); irregular text is handed back through phi_reads_text_end as ever,
 * and the host reads the pieces still parked with phi_text_park_fetch.
 *   phi_text_park_create / _destroy   on a device
 *   phi_text_park_pin                 page-locks a host buffer the pieces come from (unpinned by _destroy)
 *   phi_text_park_add                 copies n bytes to the device; returns when they are there (the host buffer is free again)
 *   phi_text_park_add_async / _wait   the same in two halves: the copy is issued / the host buffer may be written again (the next
 *                                     chunk is read into another buffer meanwhile)
 *   phi_text_park_bytes / _fetch      a piece's size; its bytes back on the host
 *   phi_text_park_release             the piece's device memory is let go (after phi_add_reads_text_parked took it)
 */
typedef struct phi_text_park phi_text_park;
int phi_text_park_create(int32_t device, phi_text_park **out);
int phi_text_park_pin(phi_text_park *park, void *host, size_t bytes);
int phi_text_park_add(phi_text_park *park, const char *text, int64_t n, int32_t *index);
int phi_text_park_add_async(phi_text_park *park, const char *text, int64_t n, int32_t *index);
int phi_text_park_wait(phi_text_park *park, int32_t index);
int64_t phi_text_park_bytes(phi_text_park *park, int32_t index);
int phi_text_park_fetch(phi_text_park *park, int32_t index, char *out, int64_t cap);
int phi_text_park_release(phi_text_park *park, int32_t index);
void phi_text_park_destroy(phi_text_park *park);
int phi_add_reads_text_parked(phi_ctx *ctx, phi_text_park *park, int32_t index, int32_t *irregular);
int phi_reads_text_last_batch(phi_ctx *ctx, char *bases, int64_t cap_bases, int64_t *off, int64_t cap_reads, int64_t *n_reads,
                              int64_t *n_bases);
/* For a stream whose chunks go to SEVERAL contexts in turn (one per GPU): hands out the bytes this context holds
 * unfinished (valid until its next phi_add_reads_text) and forgets them, so that the caller can put them in front of the
 * next chunk on whichever context takes it.  Does not wait for the sketch of the records already taken. */
int phi_reads_text_detach_carry(phi_ctx *ctx, const char **bytes, int64_t *n);
/* Forget all reads seen so far (graph index is kept).  The clearing itself may be folded into the
 * next batch's first launch; every call on this context that observes the spectrum, the counters
 * or the hit vector sees the reads forgotten.  A hit-vector pointer obtained earlier from
 * phi_hits_buffer must not be read between this call and the next phi_add_reads*: fetch it again. */
int phi_reset_reads(phi_ctx *ctx);
/* Totals since the last reset (waits for the stream): reads, bases, emitted read minimisers
 * (with multiplicity) and distinct read hashes so far. */
int phi_reads_stats(phi_ctx *ctx, int64_t *n_reads, int64_t *n_bases, int64_t *n_emitted, int64_t *n_distinct);

/*
 * Multi-GPU exchange (no reference counterpart: the reference is one process).  Each rank holds
 * a shard of the reads; before phi_solve the caller all-reduces (MAX) the hit vector in place
 * and tells every rank the size of the union spectrum.
 *   phi_hits_buffer     device pointer to uint8 hit[n], n = number of distinct walk minimisers;
 *                       index = dense minimiser id (rank of the hash's first occurrence in walk
 *                       position order), identical on every rank for the same graph; valid until
 *                       the next phi_reset_reads / phi_set_graph on this context
 *   phi_spectrum_export this rank's distinct read hashes that are NOT walk minimisers (those that
 *                       are, are exactly the set hit flags): device pointer to uint64[n] (valid
 *                       until the next call on this context)
 *   phi_spectrum_import merge another rank's exported hashes (a device buffer the caller owns): a
 *                       hash that is a walk minimiser sets its hit flag, any other joins the local
 *                       set; after the hit all-reduce and the imports |Sp_R| (ILP_index.cpp:641)
 *                       = flags set + set size is the same on every rank
 *   phi_spectrum_set_size  alternatively, override |Sp_R| used in the log counters
 */
int phi_hits_buffer(phi_ctx *ctx, void **d_hits, int64_t *n);
/* The read table the read kernels probe (diagnostics, tests): device pointer to n_buckets 32-byte buckets of two slots,
 * u64 words [key 0, id 0 | flags << 32, key 1, id 1] (empty key UINT64_MAX; flag 1: a key whose home bucket this is lies
 * in a later bucket), home bucket key & (n_buckets - 1); valid until the next phi_set_graph on this context. */
int phi_read_table(phi_ctx *ctx, void **d_table, int64_t *n_buckets);
int phi_spectrum_export(phi_ctx *ctx, void **d_hashes, int64_t *n);
int phi_spectrum_import(phi_ctx *ctx, const void *d_hashes, int64_t n);
int phi_spectrum_set_size(phi_ctx *ctx, int64_t global_size);

/*
 * The same exchange done by the library itself with RCCL over xGMI (librccl is loaded on first use).
 * One context per GPU -- one process per GPU, or one host thread per GPU in one process (the `PHI
 * --devices 0,1,..` mode) -- all holding the same graph and parameters, each fed its own shard of reads.
 *   phi_comm_unique_id      ncclGetUniqueId: 128 bytes made by one rank and handed to the others out of
 *                           band (a file, MPI, a torch.distributed store, shared memory between threads)
 *   phi_comm_init           ncclCommInitRank on the context's device: collective over the n_ranks contexts
 *   phi_comm_allreduce_hits step 1 alone: ncclAllReduce(MAX, uint8) of the hit vector in place, on the
 *                           context's stream, asynchronous (what a job times per read set)
 *   phi_comm_exchange       the whole exchange, once per job after the rank's last read batch: step 1, then
 *                           ncclAllGather of the sizes and of the padded lists of phi_spectrum_export, and
 *                           the import of every other rank's list.  Afterwards the hit vector, |Sp_R| and so
 *                           phi_solve's result are identical on every rank.
 *   phi_comm_destroy        also done by phi_ctx_destroy
 */
#define PHI_COMM_ID_BYTES 128
int phi_comm_unique_id(void *id_out, size_t cap);
int phi_comm_init(phi_ctx *ctx, const void *id, int32_t rank, int32_t n_ranks);
int phi_comm_info(const phi_ctx *ctx, int32_t *rank, int32_t *n_ranks);
int phi_comm_allreduce_hits(phi_ctx *ctx);
int phi_comm_exchange(phi_ctx *ctx);
int phi_comm_destroy(phi_ctx *ctx);

/*
 * The same exchange for the contexts of ONE process -- one host thread and one context per GPU, the `PHI --devices` mode --
 * without RCCL: every GPU ORs the peers' hit vectors into its own with one kernel that loads them across xGMI
 * (hipDeviceEnablePeerAccess), ordered by HIP events; the lists of the other read hashes are imported where they lie.
 * Meant for hit vectors of a few MB, where an 8-rank ncclAllReduce is latency (tens of microseconds: as long as one GPU
 * takes to score a whole MHC read set).  All calls but create / destroy are collective over the group's threads.
 *   phi_peers_create          a group for n_ranks contexts (at most 16)
 *   phi_peers_join            every rank's thread, after phi_set_graph: peer access, events
 *   phi_peers_allreduce_hits  step 1 alone, asynchronous on the contexts' streams
 *   phi_peers_exchange        steps 1 + 2: afterwards phi_solve gives the same result on every rank
 *   phi_peers_destroy         once, when no rank will call into the group again
 */
int phi_peers_create(int32_t n_ranks, void **group);
int phi_peers_join(phi_ctx *ctx, void *group, int32_t rank);
int phi_peers_allreduce_hits(phi_ctx *ctx);
int phi_peers_exchange(phi_ctx *ctx);
int phi_peers_destroy(void *group);

/*
 * The same exchange between PROCESSES of one node -- one process and one context per GPU, as bench.py runs under
 * torch.distributed.run -- without RCCL: every rank maps the other ranks' hit vectors (hipIpcGetMemHandle /
 * hipIpcOpenMemHandle; the loads travel over xGMI) and ORs them into its own with one kernel per read set.  The ranks
 * order themselves through flags in device memory; no host call takes part in an exchange, and the gather of read set i
 * runs on a stream of its own beside the scoring of read set i + 1 (the context keeps four hit vectors for that).  For hit
 * vectors of a few MB, where an 8-rank ncclAllReduce is all latency.  One exchange per read set (per phi_reset_reads), the
 * same sequence of calls on every rank.  HSA_ENABLE_IPC_MODE_LEGACY=0 where the host driver only shares memory by dmabuf.
 *   phi_ipc_unique_id        128 bytes (the name of a small shared-memory block) made by one rank, handed to the others out of band
 *   phi_ipc_init             collective, after phi_set_graph: handles published and mapped; phi_set_graph is refused from here on
 *   phi_ipc_allreduce_hits   step 1 alone, asynchronous: the gather starts once the read set is scored, which the context's NEXT
 *                            read launch tells it (no launch, event or host call in between); whatever observes the hit vector
 *                            through this library afterwards waits for it by itself
 *   phi_ipc_flush            behind a LAST exchange, before waiting on the device by other means (hipDeviceSynchronize,
 *                            torch.cuda.synchronize): lets the gather start without a further read launch.  Asynchronous
 *   phi_ipc_exchange         steps 1 + 2 (the lists of novel read hashes, through mapped buffers and a host barrier), once per job
 *   phi_ipc_check            waits for the gathers issued so far; PHI_ERR_DEVICE when one gave up on a peer (PHI_IPC_TIMEOUT_S, 20 s)
 *   phi_ipc_destroy          collective; also done by phi_ctx_destroy
 */
int phi_ipc_unique_id(void *id_out, size_t cap);
int phi_ipc_init(phi_ctx *ctx, const void *id, int32_t rank, int32_t n_ranks);
int phi_ipc_info(const phi_ctx *ctx, int32_t *rank, int32_t *n_ranks);
int phi_ipc_allreduce_hits(phi_ctx *ctx);
int phi_ipc_flush(phi_ctx *ctx);
int phi_ipc_exchange(phi_ctx *ctx);
int phi_ipc_check(phi_ctx *ctx);
int phi_ipc_destroy(phi_ctx *ctx);

typedef struct {
    /* ---- solve (ILP_index.cpp:776-1418) */
    int64_t objective;          /* max  #covered minimisers - 2*(R/2)*#recombinations          */
    int64_t upper_bound;        /* proven bound; optimal iff upper_bound == objective           */
    int32_t optimal;            /* 1 when proven optimal; 0 when the search ran out of its budget of DP runs
                                   (phi_set_solve_budget): the path is feasible, the bound proven */
    int32_t n_dp_runs;          /* DP launches used (1 = certificate closed at the root)        */
    int64_t n_covered;          /* minimisers with >=1 anchor fully traversed (sum of z_i)      */
    /* ---- decode (:1431-1525) */
    int64_t n_path;
    const int32_t *path_vtx;    /* [n_path] vertices in topological order                       */
    const int32_t *path_hap;    /* [n_path] haplotype label of each vertex                      */
    int32_t recombination_count;/* :1519 adjacent label changes                                 */
    int32_t n_switches;         /* w-node traversals (each costs 2*(R/2))                       */
    int64_t hap_len;            /* length of the inferred sequence                              */
    /* ---- log counters (:563, :641, :734, :738-743, :883) */
    int32_t n_walks;
    const int64_t *n_minimizers;/* [n_walks] "Number of Minimizers"                             */
    const int64_t *n_anchors;   /* [n_walks] "Number of Anchors" (after the filter)             */
    int64_t spectrum_size;      /* |Sp_R|                                                       */
    int64_t filtered;           /* minimisers dropped by the shared-anchor filter               */
    int64_t retained;           /* spectrum_size - filtered                                     */
    int64_t n_in_model;         /* minimisers with a z_i ("% Minimizers are in ILP")            */
} phi_result;

/* Budget of the exact search behind phi_solve, counted in DP runs (never in wall-clock time: the same
 * input gives the same result and the same `optimal` flag on every run).  The reference's
 * model.optimize() (ILP_index.cpp:1412-1418) sets no limit; max_dp_runs <= 0 means the same here.
 * Default 4096 (minutes at most on a 49-walk MHC graph, seconds on small ones).  Almost every input closes at the
 * root in 1-3 runs; what does not are graphs where short k-mers repeat all over (k <= 8). */
int phi_set_solve_budget(phi_ctx *ctx, int64_t max_dp_runs);

/* Stages 2b-3 of ILP_function (:670-1525): filter, exact solve, decode.  Replaces
 * model.optimize() (:1418) with a max-plus DP + optimality certificate. */
int phi_solve(phi_ctx *ctx, phi_result *out);

/* ILP_index.cpp:1577-1581: concatenated original-case node sequences of the path.
 * buf must hold result.hap_len bytes. */
int phi_path_sequence(phi_ctx *ctx, char *buf, int64_t cap);

/*
 * Introspection used by the parity tests (tests/ compare these with oracle/).
 * phi_sketch: stand-alone (w,k)-minimiser sketch of arbitrary sequences on the GPU
 * (compute_hashes / index_kmers minus the vertex map).  Records come back sorted by
 * (sequence, position).  Pass cap = 0 to query *n_out.
 */
int phi_sketch(phi_ctx *ctx, const char *bases, const int64_t *seq_off, int64_t n_seq, int32_t k,
               int32_t w, uint64_t *out_hash, int64_t *out_pos, int32_t *out_seq, int64_t cap,
               int64_t *n_out);
/*
 * What phi_set_graph built.  The reference sketches every walk on its own (ILP_index.cpp:559-573); here walk
 * entries with the same context (the base before, the vertex, the next w+k-2 bases of the walk) form a class
 * that is sketched once (graph-side de-duplication): n_classes classes laid out in class_bases bases of "class
 * space" stand for walk_bases bases of walks, n_class_records minimiser records for n_walk_minimizers.
 * sketch_gpu_ms = GPU time from the first class kernel to the last class record (HIP events on the stream).
 */
typedef struct {
    int64_t n_entries, walk_bases;
    int64_t n_classes, class_bases, n_class_records;
    int64_t n_walk_minimizers, n_distinct_minimizers;
    double sketch_gpu_ms;
} phi_index_info;
int phi_index_stats(phi_ctx *ctx, phi_index_info *out);

/*
 * How the last phi_solve ran its DP (no reference counterpart: the reference hands the model to Gurobi).
 * dp_mode: 0 = every vertex is a step (more than 256 walks, or the fallback of the event kernels), 1 = event
 * driven, one chain over the compact steps, 2 = blocks of steps in parallel on walk lanes (<= 64 walks),
 * 3 = blocks in parallel with their transfer rows on class lanes (65 .. 256 walks).  n_blocks = 0 unless 2 / 3;
 * max_classes / mean_classes: class lanes per block of the last DP run (mode 3).
 */
typedef struct {
    int64_t n_dp_anchors, n_events;
    int32_t n_steps, n_blocks, dp_mode, max_classes;
    double mean_classes;
} phi_solve_info;
int phi_solve_stats(phi_ctx *ctx, phi_solve_info *out);

/*
 * Test introspection: ONE run of the solve's DP with anchor weights the caller gives (no reference counterpart; the
 * search calls the same function once per relaxation).  Valid after phi_solve, on the state that solve left: the strategy
 * (dp_mode and the blocks phi_solve_stats reports), including what its fallbacks changed.  The run is the solve's own,
 * fallbacks included, and may change that state as a run inside a solve would; the next phi_solve starts over as ever.
 *
 * weights: one byte, 0 or 1, per dp anchor = per kept anchor that spans an edge (t1 > t0 in phi_kept_anchors), in kept
 * order; n_weights must be their number (phi_solve_info.n_dp_anchors).  NULL: every weight 1 (n_weights is not read).
 * The run maximises, over the walks-and-switches paths of the model, the weights of the anchors traversed whole minus
 * 2 * (recombination / 2) per switch.
 *
 * out_ends[h], h < n_walks: the best value of a path that ends at the last vertex of walk h (INT32_MIN: none).
 * *out_value, *out_end_walk: the largest of them and the lowest walk that has it.  The argmax path as segments in path
 * order -- walk, first and last position within the walk -- *n_seg of them; with seg_cap < *n_seg none is written.
 * info: the strategy of the attempt that finished (dp_mode, n_blocks, max_classes as in phi_solve_info; blk_ring = ring of
 * tops the blocks were placed for, blk_max_len = steps of the longest block; both 0 without blocks) and the fallbacks
 * taken on the way, PHI_DP_RETRY_* or-ed; retries_since_solve: those of every run since the last phi_solve began, its own
 * runs included (a solve whose first run falls back leaves nothing for a later run to fall back from).
 */
#define PHI_DP_RETRY_HALVE_CLASS_TARGET 1u   /* a block with more than 64 classes: shorter class-lane blocks */
#define PHI_DP_RETRY_NO_SMALL_BLOCKS 2u      /* a 256-step block task's queue overflowed: longer blocks */
#define PHI_DP_RETRY_GIVE_UP_BLOCKS 4u       /* the whole event chain from now on */
#define PHI_DP_RETRY_DENSE 8u                /* the event kernel's queue overflowed: every vertex a step from now on */
typedef struct {
    int32_t dp_mode, n_blocks, blk_ring, blk_max_len, max_classes;
    uint32_t retries, retries_since_solve;
} phi_dp_probe_info;
int phi_dp_probe(phi_ctx *ctx, const uint8_t *weights, int64_t n_weights, int32_t *out_ends, int64_t *out_value,
                 int32_t *out_end_walk, int32_t *out_seg_walk, int64_t *out_seg_first, int64_t *out_seg_last,
                 int64_t seg_cap, int64_t *n_seg, phi_dp_probe_info *info);

/* Minimisers of walk h found by phi_set_graph, sorted by position. */
int phi_walk_minimizers(phi_ctx *ctx, int32_t walk, uint64_t *out_hash, int64_t *out_pos,
                        int64_t cap, int64_t *n_out);
/*
 * The reference's -d1 report (ILP_index.cpp:565-604): hist[c], c = 1..n_walks, = number of distinct
 * walk minimisers that occur in exactly c walks (hist[0] = 0); *n_distinct = their total.  hist has
 * cap >= n_walks + 1 entries.  Valid after phi_set_graph.
 */
int phi_walk_sharing(phi_ctx *ctx, int64_t *hist, int32_t cap, int64_t *n_distinct);

/* Kept anchors after the filter (valid after phi_solve): hash, walk, first/last walk index. */
int phi_kept_anchors(phi_ctx *ctx, uint64_t *out_hash, int32_t *out_walk, int32_t *out_t0,
                     int32_t *out_t1, int64_t cap, int64_t *n_out);

/* Pin / unpin caller memory on this context's device (hipHostRegister): for host buffers handed to
 * phi_add_reads again and again, e.g. the chunk buffers of a streaming reads reader (phi_host.h), so
 * that the device copy is a direct DMA.  No reference counterpart. */
int phi_host_register(phi_ctx *ctx, void *p, size_t bytes);
int phi_host_unregister(phi_ctx *ctx, void *p);

/* Timing of the dominant kernel (the sketch kernel), measured with HIP events on the stream
 * the kernel is launched on.  phi_prof_enable(n), n >= 1, starts bracketing every n-th sketch launch
 * (a bracketed launch costs the stream a few microseconds more than a plain one, so a throughput
 * measurement samples: n = 8); phi_prof_enable(0) stops.  phi_prof_read returns the number of
 * bracketed launches, their summed duration and the bases they covered. */
int phi_prof_enable(phi_ctx *ctx, int on);
int phi_prof_read(phi_ctx *ctx, int64_t *n_launches, double *total_ms, int64_t *total_bases);

/*
 * The walks resolved ON THE DEVICE from the text of the GFA's W-lines (the reference: gfa-io.cpp:367-432 on one core, then
 * ILP_index.cpp:96-113).  At chromosome scale the walk text is the file (10.5 of config 5's 10.9 GB).
 *   phi_walk_text_upload    the walk field of every W-line (">s17>s18...", optional tags may follow), as it stands in the (mapped)
 *                           file, to the device through pinned staging; returns when the last piece is on its way -- call it
 *                           on a thread of its own while the host still reads the S- and L-lines
 *   phi_walk_text_resolve   names <prefix><canonical decimal> -> num2id[number] (the direct index of the host reader's name table,
 *                           include/phi_host.h phi_graph_name_index); walk_off_out[n_walks + 1].  *irregular != 0 (a reverse step:
 *                           the reference flips such walks by majority strand; a name of another form, or naming no segment: the
 *                           reference leaves such steps out): nothing was resolved, fall back to the host reader
 *   phi_set_graph(..., walk_vtx = NULL, ...)  then takes the walk entries from where phi_walk_text_resolve left them
 *   phi_walk_entries        (tests) a host copy of the walk entries on the device
 */
typedef struct { const char *text; int64_t n; } phi_walk_text;
int phi_walk_text_upload(phi_ctx *ctx, const phi_walk_text *walks, int32_t n_walks);
int phi_walk_text_resolve(phi_ctx *ctx, const char *prefix, int32_t prefix_n, const int32_t *num2id, int64_t n_num, int32_t n_seg,
                          int64_t *walk_off_out, uint32_t *irregular);
int phi_walk_entries(phi_ctx *ctx, int32_t *out, int64_t cap, int64_t *n);

/* Wait for everything this process has put on the context's device, on every stream, and report the device's error
 * state: a fault raised by an earlier asynchronous launch surfaces here (diagnostics; no reference counterpart). */
int phi_device_synchronize(phi_ctx *ctx);

/* (tests; no reference counterpart) The prefix sums every count / scan / write pass of the library is built on, on device
 * memory of the caller: d_out[0 .. n] = exclusive prefix sums of d_in[0 .. n), d_out[n] = the total.  kind 0: uint8 in,
 * int32 out; 1: int32 in, int32 out, d_out may be d_in; 2: int32 in, int64 out.  d_out holds n + 1 items and nothing behind
 * them is written.  n < 0, another kind, d_out = NULL or d_in = NULL with n > 0: PHI_ERR_INVALID, nothing launched.  Runs on
 * the context's stream and returns when d_out is filled. */
int phi_prefix_sums(phi_ctx *ctx, int32_t kind, const void *d_in, int64_t n, void *d_out);

/* data/edlib_edits.py:24-27, data/postprocessing_2_MIQP.py:21-42, data/get_edit_stats.sh: edlib NW edit distance of
 * pair i = (a[a_off[i]..a_off[i+1]), b[b_off[i]..b_off[i+1])), one workgroup per pair.  out[i] = distance, or -1 when
 * max_distance >= 0 and the distance exceeds it.  Needs no phi_set_params / phi_set_graph and leaves graph, reads and
 * result state untouched.  Bytes compare exactly (case-sensitive, no wildcards); each sequence < 2^31 bytes
 * (PHI_ERR_UNSUPPORTED beyond).  Runs on the context's stream and returns when out is filled. */
int phi_edit_distances(phi_ctx *ctx, const char *a, const int64_t *a_off, const char *b, const int64_t *b_off,
                       int64_t n_pairs, int64_t max_distance, int64_t *out);

/* data/edlib_edits.py:8-43, data/postprocessing_2_MIQP.py:21-39: one optimal global alignment (unit costs, bytes compared
 * exactly) of each pair of phi_edit_distances' layout, query a and target b as in edlib.align(a, b), given its distance
 * dist[i] (as phi_edit_distances returned it; -1: the pair is skipped and its counts are -1).  counts[5i .. 5i+4] = M
 * ('='), X (mismatch), I (a byte of a only), D (a byte of b only) and the CIGAR's length in bytes; identity =
 * M * 100 / (M + X + I + D).  The path is the traceback from (|a|, |b|) that takes at each cell the first step keeping the
 * optimal value: diagonal, then I, then D.  cigar may be NULL (counts only); otherwise pair i's extended CIGAR ('=', 'X',
 * 'I', 'D' runs, no terminator) goes to cigar[cigar_off[i] .. cigar_off[i+1]), which must hold 11 (2 dist[i] + 1) bytes
 * (PHI_ERR_INVALID before any work otherwise).  PHI_ERR_INVALID, naming the pair, when no alignment costs dist[i];
 * PHI_ERR_NOMEM when a pair's checkpoints do not fit in free device memory.  Needs no phi_set_params / phi_set_graph and
 * leaves graph, reads and result state untouched.  Runs on the context's stream and returns when counts are filled. */
int phi_edit_alignments(phi_ctx *ctx, const char *a, const int64_t *a_off, const char *b, const int64_t *b_off,
                        int64_t n_pairs, const int64_t *dist, int64_t *counts, char *cigar, const int64_t *cigar_off);


/* gzip (RFC 1952, any number of members) inflated on a device, DESIGN.md 4.8.  in[0, n): the whole file; the output goes
 * to out[0, cap) when it fits.  *out_size = the inflated size in every successful call: when it exceeds cap nothing is
 * copied (call again with a larger buffer).  chunk_bytes: the compressed bytes per chunk (<= 0: PHI_INFLATE_CHUNK from the
 * environment, else PHI_INFLATE_CHUNK_DEFAULT).  flags: PHI_INFLATE_NO_FINDER searches no chunk for a block start (every
 * chunk is then decoded by its predecessor: serial speed, for tests).  Every member's CRC32 and ISIZE are checked; an
 * invalid code, a distance before the start of its member, truncation or a CRC / ISIZE mismatch is PHI_ERR_INVALID and
 * claims no output.  info (may be NULL) is filled, its detail text on any error.  Needs no phi_ctx. */
#define PHI_INFLATE_CHUNK_DEFAULT (64 << 10)
#define PHI_INFLATE_NO_FINDER 1
typedef struct {
    int64_t in_bytes;          /* compressed bytes */
    int64_t out_bytes;         /* inflated bytes */
    int64_t members;           /* gzip members */
    int64_t chunks;            /* chunks the stream was cut into */
    int64_t confirmed;         /* chunks whose decoder's output was used (confirmed at their found start), chunk 0 aside */
    int64_t redecoded;         /* chunks decoded by a predecessor instead (start missing or false) */
    int64_t marker_bytes;      /* output bytes that referred to an earlier chunk's window and were resolved afterwards */
    double device_ms;          /* span from the uploaded input to the checked output (upload and download excluded; the host's
                                  work between kernels included: an upper bound of the device time) */
    char detail[192];
} phi_inflate_info;
int phi_inflate(int32_t device, const void *in, int64_t n, void *out, int64_t cap, int64_t chunk_bytes, int32_t flags,
                int64_t *out_size, phi_inflate_info *info);
/* phi_inflate with the output in a host buffer it allocates (*out, *out_size bytes; free it with phi_inflate_free): one
 * inflate whatever the output's size (phi_inflate needs a second call when cap is too small) */
int phi_inflate_alloc(int32_t device, const void *in, int64_t n, int64_t chunk_bytes, int32_t flags, void **out, int64_t *out_size,
                      phi_inflate_info *info);
void phi_inflate_free(void *p);
/* A gzip stream into a park: _begin, the compressed bytes in slices of any size through _add (gathered on the
 * host), then _end inflates them on the park's device and parks the text as *count pieces of at most piece_bytes, indices
 * *first .. *first + *count - 1 in stream order, which phi_add_reads_text_parked and phi_text_park_fetch take as they are.
 * _end's status is phi_inflate's (PHI_ERR_INVALID for a corrupt stream: no piece is added), info its detail. */
int phi_text_park_gzip_begin(phi_text_park *park, int64_t piece_bytes);
int phi_text_park_gzip_add(phi_text_park *park, const void *data, int64_t n);
int phi_text_park_gzip_end(phi_text_park *park, int32_t *first, int32_t *count, phi_inflate_info *info);
/* the gzip member header at byte pos of data[0, n): *deflate_start = the offset of its deflate data (FEXTRA, FNAME,
 * FCOMMENT skipped, FHCRC checked); PHI_ERR_INVALID when it is no header or is cut short */
int phi_gzip_header(const void *data, int64_t n, int64_t pos, int64_t *deflate_start);
/* CRC32 (the gzip one) of A followed by B, from crc(A), crc(B) and |B| */
uint32_t phi_crc32_combine(uint32_t crc_a, uint32_t crc_b, int64_t len_b);

/* BGZF written on a device, DESIGN.md 4.17: in[0, n) cut into runs of PHI_BGZF_BLOCK bytes (the last may be shorter), each
 * compressed by one workgroup into one gzip member with the BGZF extra field (1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6,
 * "BC" 02 00, BSIZE = member size - 1; one raw DEFLATE stream; CRC32, ISIZE), then the 28-byte EOF block.  A block holds
 * LZ77 copies (lengths up to 258, distances up to 32768, none reaching before the block's first byte) under a dynamic
 * Huffman code built on the device from the block's own histogram, or is a stored block where that would not be smaller.
 * The output is a function of the input and the flags alone.  cap, *out_size and "nothing copied when it does not fit" as
 * for phi_inflate; phi_deflate_bgzf_bound(n) always fits.  n == 0 is valid (the EOF block alone, or nothing with
 * PHI_DEFLATE_NO_EOF).  PHI_ERR_INVALID, with nothing launched, for n < 0, in == NULL with n > 0, or unknown flags.  Inputs
 * beyond a batch of blocks (PHI_DEFLATE_BATCH from the environment, else PHI_DEFLATE_BATCH_DEFAULT) go through the device in
 * batches, so device memory stays bounded.  info (may be NULL) is filled, its detail text on any error.  Needs no phi_ctx. */
#define PHI_BGZF_BLOCK 65280           /* input bytes per block, as htslib cuts them */
#define PHI_DEFLATE_NO_MATCH 1         /* literals only (tests: isolates the Huffman side) */
#define PHI_DEFLATE_NO_EOF   2         /* leave out the 28-byte EOF block (outputs that are concatenated) */
#define PHI_DEFLATE_BATCH_DEFAULT 512  /* blocks per batch */
typedef struct {
    int64_t in_bytes, out_bytes, blocks;
    int64_t stored_blocks;             /* blocks written as stored because the Huffman form was not smaller */
    int64_t matches, match_bytes;      /* LZ77 copies and the input bytes they cover (of the blocks not stored) */
    double  device_ms;                 /* uploaded input -> finished output, as phi_inflate_info.device_ms, summed over the batches */
    char    detail[192];
} phi_deflate_info;
int64_t phi_deflate_bgzf_bound(int64_t n);        /* the output never exceeds this */
int phi_deflate_bgzf(int32_t device, const void *in, int64_t n, void *out, int64_t cap, int32_t flags,
                     int64_t *out_size, phi_deflate_info *info);
int phi_deflate_bgzf_alloc(int32_t device, const void *in, int64_t n, int32_t flags, void **out, int64_t *out_size,
                           phi_deflate_info *info);   /* freed with phi_deflate_free */
void phi_deflate_free(void *p);

/* The same file with an index built beside it on the device, DESIGN.md 4.18.  *out[0, *out_size) is byte for byte what
 * phi_deflate_bgzf_alloc gives for in, n and flags; *index[0, *index_size) is the finished index file; both are freed with
 * phi_deflate_free.  index_kind is exactly one of the two values below (anything else: PHI_ERR_INVALID, nothing launched), and
 * so is PHI_DEFLATE_NO_EOF with an index.  On any error both outputs are NULL and iinfo->detail says why.  Needs no phi_ctx.
 *
 * Virtual offsets: with off[0..nb] the file offsets of the members (off[nb] the EOF block's), uncompressed byte p in [0, n] is
 * (off[p / PHI_BGZF_BLOCK] << 16) | (p % PHI_BGZF_BLOCK); so p == n with n a multiple of the block size points at the EOF block.
 *
 * PHI_BGZF_INDEX_GZI: little-endian uint64 count nb - 1 (0 for nb <= 1), then for the members 1 .. nb-1 the pair (off[b],
 * PHI_BGZF_BLOCK * b).  Built on the host from the members' sizes; no kernel runs for it.
 *
 * PHI_BGZF_INDEX_TBI_VCF: a tabix index with the VCF preset, itself BGZF.  The text is lines ended by '\n' (a last line without
 * one counts); a line beginning with '#' is a meta line wherever it stands, every other line a record of at least the 8 fields
 * CHROM POS ID REF ALT QUAL FILTER INFO.  Contigs are numbered by first appearance.  beg = POS - 1 (at least 0), end = beg +
 * len(REF), or the value of the first key END of INFO (the field begins with "END=" or holds ";END="); an end <= beg becomes
 * beg + 1.  bin = reg2bin(beg, end) of the SAM/tabix specification (5 levels, 14 bits).  A chunk is a maximal run of records
 * consecutive in the file that share contig and bin, from the virtual offset of its first record's first byte to that of the
 * byte after its last record's line; within a contig bins ascend, within a bin chunks keep file order; no merging of chunks,
 * no pseudo-bin 37450.  The linear index of a contig has ((max end - 1) >> 14) + 1 windows, window w the smallest virtual
 * offset of a record start among the records overlapping [w << 14, (w + 1) << 14); an empty window takes its predecessor's
 * value, leading ones 0.  Header: "TBI\1", n_ref, format 2, col_seq 1, col_beg 2, col_end 0, meta '#', skip 0, l_nm, the
 * NUL-terminated names; per contig n_bin, the bins, n_intv, the offsets; then n_no_coor = 0 (uint64).  A text without a record
 * (n_ref 0) and n == 0 are valid.
 * PHI_ERR_INVALID: a record with fewer than 8 fields; an empty line; a POS or END value that is empty, not all digits or longer
 * than 10 digits; a POS smaller than the previous record's on the same contig; a contig name that comes back after another
 * contig.  PHI_ERR_UNSUPPORTED: an end above 2^29 (CSI would be needed and is not written); a contig name above 1024 bytes; more
 * than 2^31 - 2 lines.  PHI_ERR_NOMEM: the text does not fit the device beside a batch's buffers.
 *
 * These rules are stated here and checked against themselves (a per-line writer and an index reader in tests/tabix_ref.py): the
 * bytes are NOT compared with those of `tabix -p vcf` or `bgzip -i`, which merge chunks and add a pseudo-bin. */
#define PHI_BGZF_INDEX_GZI     1       /* bgzip's .gzi: where every member begins, compressed and uncompressed */
#define PHI_BGZF_INDEX_TBI_VCF 2       /* tabix .tbi with the VCF preset, itself BGZF-compressed */
typedef struct {
    int64_t records, meta_lines, contigs;   /* of the text (TBI); 0 for GZI */
    int64_t bins, chunks, windows;          /* written to the index (TBI); for GZI chunks = the member entries written */
    int64_t index_bytes;                    /* *index_size */
    double  device_ms;                      /* GPU time of the index kernels alone, by HIP events (0 for GZI) */
    char    detail[192];
} phi_bgzf_index_info;
int phi_deflate_bgzf_indexed(int32_t device, const void *in, int64_t n, int32_t flags, int32_t index_kind, void **out,
                             int64_t *out_size, void **index, int64_t *index_size, phi_deflate_info *info,
                             phi_bgzf_index_info *iinfo);

/* The records of one region of a BGZF VCF, DESIGN.md 4.19: what `tabix FILE REGION` prints below the header.  gz[0, n_gz): the
 * BGZF members a .tbi points at for the region, back to back (a multi-member gzip stream); range[2 * n_ranges]: byte ranges
 * [p0, p1) of their inflated concatenation, ascending and disjoint, each beginning at a line's first byte and ending behind a
 * line feed -- both as phi_region_plan of include/phi_host.h leaves them (phi_region_gz, phi_region_ranges), passed unchanged.
 * *text[0, *n_text) (NUL behind it, freed with phi_vcf_region_free) holds, in file order, exactly the lines that start inside one
 * of the ranges, do not begin with '#', whose CHROM equals name byte for byte, and whose interval overlaps [beg, end) (0-based,
 * half-open: rec_beg < end and rec_end > beg); each line is followed by one line feed.  The interval is the .tbi writer's, stated
 * above for PHI_BGZF_INDEX_TBI_VCF: rec_beg = max(POS - 1, 0), rec_end = rec_beg + len(REF) or the value of the first key END of
 * INFO, and a rec_end <= rec_beg becomes rec_beg + 1.  (tests/tabix_ref.py: overlapping(), and what query() finds through the index.)
 * A range's first byte begins a line even where no line feed stands before it: planned members need not be neighbours in the file.
 * PHI_ERR_INVALID: inside a range, a line that is no meta line and has fewer than 8 fields (an empty line too), or whose POS or
 * END is empty, not all digits or longer than 10 digits -- of any contig; the detail text names the line's offset in the inflated
 * members; bytes that are no chain of BGZF members; ranges that are empty, out of order or beyond the text; members whose text is
 * not as long as their ISIZE says.  A corrupt member is phi_inflate's error, with its detail.  PHI_ERR_UNSUPPORTED: a record of
 * 2^31 bytes or more.  On any error *text is NULL and nothing stays allocated on the device.
 * The members go through the device in batches of PHI_VCF_REGION_BATCH members (environment; else the default below, a starting
 * value, not measured), so device memory stays bounded by a batch whatever the region.  A batch that ends inside a line starts
 * the next at the member that holds that line's first byte (inflated a second time: reinflated_members), with twice the members
 * when that is the batch's own first member; a line is looked at once, in the batch that holds its line feed, so nothing is kept
 * twice and nothing is lost.  Needs no phi_ctx. */
#define PHI_VCF_REGION_BATCH_DEFAULT 256   /* members per batch: 16 MiB of text at most; a starting value, not measured */
typedef struct {
    int64_t members, gz_bytes;         /* the members read and their compressed bytes */
    int64_t text_bytes;                /* their inflated bytes */
    int64_t lines_seen, lines_kept;    /* lines that start inside a range; lines written to *text */
    int64_t batches;
    int64_t reinflated_members;        /* members inflated again because a batch ended inside a line */
    double  inflate_ms, filter_ms;     /* GPU milliseconds by HIP events: phi_inflate_info.device_ms summed; marks, lines, offsets, copy */
    char    detail[192];
} phi_vcf_region_info;
int phi_vcf_region_filter(int32_t device, const void *gz, int64_t n_gz, const int64_t *range, int32_t n_ranges, const char *name,
                          int64_t beg, int64_t end, char **text, int64_t *n_text, phi_vcf_region_info *info);
void phi_vcf_region_free(char *text);

/* A gzip GFA split on the device: the file (RFC 1952, any number of members) is inflated on the context's
 * device, the walk field of every W-line -- everything after its 6th tab, tags included, by the host reader's line rules
 * (include/phi_host.h) -- stays there, laid out as phi_walk_text_upload lays it out (phi_walk_text_resolve follows as after
 * an upload), and *host_text receives the rest: the file with every walk field cut out (a W-line then ends right after its
 * 6th tab), *host_n bytes, NUL-terminated, in pinned memory the caller lets go with phi_gfa_gzip_free once the host reader
 * is done with it (phi_gfa_read_deferred_text borrows it).  The inflated text is freed before the call returns.
 * chunk_bytes as for phi_inflate.  PHI_ERR_INVALID for a corrupt stream (info->inflate.detail says why); PHI_ERR_UNSUPPORTED
 * when the split refuses (more W-lines than it lists: PHI_GFA_SPLIT_CAP, default 2^20); nothing is kept on either error.
 * info (may be NULL): the inflate's detail, the text's bytes, the bytes returned to the host, the walk bytes kept and the
 * number of walks. */
typedef struct {
    int64_t text_bytes;        /* inflated bytes */
    int64_t host_bytes;        /* bytes of *host_text */
    int64_t walk_bytes;        /* bytes of walk fields left on the device */
    int32_t n_walks;
    phi_inflate_info inflate;
} phi_gfa_gzip_info;
int phi_gfa_gzip_split(phi_ctx *ctx, const void *gz, int64_t n, int64_t chunk_bytes, char **host_text, int64_t *host_n,
                       phi_gfa_gzip_info *info);
void phi_gfa_gzip_free(char *host_text);

/*
 * A ladder of coverages from ONE read set, sampled on the device.  Replaces data/preprocess.py:83-107 (seven
 * `seqkit sample` files per sample) and data/run_batch_4.py:38-58 (one PHI process per (sample, coverage) pair): the read
 * set is uploaded once, partitioned into nested bands by a per-read draw, and every base is scored once.
 *
 * The rule.  Read i (its 0-based ordinal in the order the reads reach the context) draws u_i = the upper 32 bits of output
 * i + 1 of SplitMix64 seeded with `seed`.  Level j of fraction f_j has the threshold t_j = min(2^32, floor(f_j * 2^32)); the
 * band of read i is the smallest j with u_i < t_j (none: the read is dropped); level j = bands 0..j.  A per-read Bernoulli
 * draw, as `seqkit sample -p`: level sizes are not exact counts.
 *
 *   phi_reads_collect_begin    (data/preprocess.py:83-107, data/run_batch_4.py:38-58) from now on every reads route -- phi_add_reads,
 *                              phi_add_reads_device, the text and the parked route -- appends its batches to a store on the device
 *                              instead of scoring them: no read counter moves.  first_ordinal: the ordinal of the first read
 *                              collected (shards of one read set; tests).  PHI_ERR_STATE while collecting or before phi_set_graph.
 *   phi_reads_collect_end      (data/preprocess.py:83-107, data/run_batch_4.py:38-58) stops collecting; reads and bases in the store.
 *                              PHI_ERR_STATE when not collecting.
 *   phi_reads_collect_release  (data/preprocess.py:83-107, data/run_batch_4.py:38-58) frees the store and the plan.
 *   phi_ladder_plan            (data/preprocess.py:83-107, data/run_batch_4.py:38-58) partitions the store, stably, into band order:
 *                              band-major, inside a band by ordinal.  1 <= n_levels <= PHI_LADDER_MAX_LEVELS, fractions ascending and
 *                              not negative (PHI_ERR_INVALID otherwise); PHI_ERR_STATE while collecting or without a store.
 *   phi_ladder_advance         (data/preprocess.py:83-107, data/run_batch_4.py:38-58) scores the bands up to `level` that have not been
 *                              scored since the last phi_reset_reads: the read state is then that of a context handed exactly
 *                              level `level`'s reads.  PHI_ERR_STATE without a plan or for a level below one already scored.
 *                              phi_reset_reads rewinds to "no band scored" and keeps the plan; phi_set_graph* drops store and plan.
 *   phi_ladder_band            (data/preprocess.py:83-107, data/run_batch_4.py:38-58; tests) the ordinals of a band's reads in stored
 *                              order into ordinals_out[0, cap) and, when not NULL, the band's bases and its reads + 1 offsets
 *                              (from 0).  *n = the band's reads, *n_bases its bases, whatever cap is (nothing is copied to a
 *                              buffer that is too small).
 */
#define PHI_LADDER_MAX_LEVELS 16
typedef struct {
    int32_t n_levels;
    int32_t one_length;                              /* the store is of one read length (> 0: that length; 0: it is not) */
    int64_t n_reads, n_bases;                        /* the store */
    int64_t n_kept_reads, n_kept_bases;              /* all bands */
    int64_t band_reads[PHI_LADDER_MAX_LEVELS], band_bases[PHI_LADDER_MAX_LEVELS];
    uint64_t threshold[PHI_LADDER_MAX_LEVELS];
    double count_gpu_ms, scan_gpu_ms, scatter_gpu_ms, copy_gpu_ms;   /* by events */
} phi_ladder_info;
int phi_reads_collect_begin(phi_ctx *ctx, int64_t first_ordinal);
int phi_reads_collect_end(phi_ctx *ctx, int64_t *n_reads, int64_t *n_bases);
int phi_reads_collect_release(phi_ctx *ctx);
/* The same reads twice (the panel chosen from the reads: scored once against the scout's index to choose, once against the
 * panel's index to infer; it stands in for running the reads through `vg haplotypes`, data/vg_haplotypes.py:21-29, and then
 * through PHI on the reduced graph, data/chop_graph.sh:46-66): scores the whole collected store in stored order where it
 * lies -- no ladder plan, no copy, no offsets read when the store is of one read length.  The read state afterwards is that
 * of a context handed the same reads directly.  PHI_ERR_STATE while collecting, without a store, or without a graph. */
int phi_reads_collect_score(phi_ctx *ctx);
int phi_ladder_plan(phi_ctx *ctx, uint64_t seed, const double *fractions, int32_t n_levels, phi_ladder_info *info);
int phi_ladder_advance(phi_ctx *ctx, int32_t level);
int phi_ladder_band(phi_ctx *ctx, int32_t band, int64_t *ordinals_out, int64_t cap, int64_t *n,
                    char *bases_out, int64_t bases_cap, int64_t *offsets_out, int64_t *n_bases);

/*
 * Reads from BAM: the records of the INFLATED BAM byte stream are found and decoded on the device.  Stands in
 * for `samtools fastq` in front of ILP_index.cpp:313-328: the reads of a BAM file are, in file order, the sequences of the
 * records with flag & 0x900 == 0 (secondary and supplementary alignments left out, both mates of a pair kept) and l_seq > 0, a
 * record with flag & 0x10 reverse-complemented back to the read as sequenced, upper case, codes =ACMGRSVTWYHKDBN.  Dropped
 * records get no ordinal (phi_reads_collect_*).  Rules from the SAM/BAM specification; not compared with samtools.
 *
 *   phi_reads_bam_begin        (ILP_index.cpp:313-328 fed by `samtools fastq`) opens the stream.  max_chunk_bytes: the largest
 *                              piece the device takes at once (larger calls are cut); tile_bytes: bytes per tile of the record
 *                              finder, 64 .. 49 152, <= 0 for the default (32 768).  PHI_ERR_STATE before phi_set_graph.
 *   phi_add_reads_bam          (ILP_index.cpp:313-328 fed by `samtools fastq`) the next n >= 1 inflated bytes of the stream, pieces of
 *                              any size, in stream order.  The header (magic, text, references) is consumed by the stream itself;
 *                              whole records are decoded and go where phi_add_reads_device's go, the unfinished rest of a piece
 *                              waits on the device for the next one.  PHI_ERR_INVALID, with the byte offset in the inflated stream
 *                              in phi_last_error(), for a wrong magic, a header that is no header, and a record on the chain that
 *                              is not well-formed (l_read_name >= 1, l_seq >= 0, block_size >= 32 + l_read_name + 4 n_cigar_op +
 *                              (l_seq + 1) / 2 + l_seq): nothing of the failing piece is taken, what earlier pieces gave stays, the
 *                              stream is failed and every further call on it is PHI_ERR_STATE.  PHI_ERR_UNSUPPORTED for a record
 *                              longer than the carry buffer.
 *   phi_add_reads_bam_parked   (ILP_index.cpp:313-328 fed by `samtools fastq`) the same with a parked piece (phi_text_park_add,
 *                              phi_text_park_gzip_end) as the bytes; the piece stays the caller's to release.
 *   phi_reads_bam_end          (ILP_index.cpp:313-328 fed by `samtools fastq`) closes the stream; info (may be NULL) is filled whatever
 *                              the status.  A stream that ends inside the header or inside a record: PHI_ERR_INVALID with the
 *                              offset; a failed stream: PHI_ERR_STATE.  A new stream may begin afterwards either way.
 *   phi_reads_bam_last_batch   (ILP_index.cpp:313-328 fed by `samtools fastq`; tests) the reads the last piece gave, as
 *                              phi_reads_text_last_batch.
 */
typedef struct {
    int64_t n_records;                               /* records on the chain */
    int64_t n_kept;                                  /* reads handed on */
    int64_t n_secondary_supplementary;               /* dropped: flag & 0x900 */
    int64_t n_empty;                                 /* dropped: l_seq == 0 (of those not dropped above) */
    int64_t n_reverse;                               /* kept records with flag & 0x10 */
    int64_t n_bases;
    int64_t header_bytes;                            /* offset of the first record */
    int64_t tiles, tiles_confirmed, tiles_rewalked;  /* tiles_confirmed: speculative lists the true chain used as they were */
    int64_t batches, batches_without_offsets;        /* decoded batches handed to the sketch; those of one read length (>= 32) */
    int32_t n_ref;
    int32_t one_length;                              /* > 0: every kept read has that length; 0: several lengths, or no read */
} phi_bam_info;
int phi_reads_bam_begin(phi_ctx *ctx, int64_t max_chunk_bytes, int64_t tile_bytes);
int phi_add_reads_bam(phi_ctx *ctx, const void *bytes, int64_t n);
int phi_add_reads_bam_parked(phi_ctx *ctx, phi_text_park *park, int32_t index);
int phi_reads_bam_end(phi_ctx *ctx, phi_bam_info *info);
int phi_reads_bam_last_batch(phi_ctx *ctx, char *bases, int64_t cap_bases, int64_t *off, int64_t cap_reads, int64_t *n_reads, int64_t *n_bases);

/*
 * VARIANT CALLS of the inferred path, or of any walk, against a reference walk of the set graph, made on the device
 * (DESIGN.md 4.16).  No reference counterpart: the reference's one product is a FASTA (ILP_index.cpp:1577-1581).  The
 * comparison the calls serve is the one the reference makes the other way round -- PanGenie's VCF turned into a FASTA with
 * `bcftools consensus` (data/run_PG.py:54-60) so that it can be set beside PHI's output at all -- and any comparison with a
 * truth VCF.  THE RULE IS THIS PROJECT'S OWN: it is not `vg deconstruct`'s and has not been compared with it or `bcftools`.
 *
 * The rule.  The set graph is the one phi_set_graph* was given (after a chop the pieces, after a panel the panel graph); all
 * ids are its ids.  The query is the path of the last phi_solve or a walk; r is a walk.
 *   1. A vertex is SHARED when it lies on the query and on walk r.  The graph is acyclic, so shared vertices come in the same
 *      order on both; where they do not: PHI_ERR_WALK.  No shared vertex at all: PHI_ERR_UNSUPPORTED.
 *   2. Calls cover the part between the first and the last shared vertex, both included; what either has outside it is not
 *      called.  ref_span / query_span give that part in bases of walk r and of the query's sequence ([first, behind last)).
 *   3. Consecutive shared vertices a, b (query indices i < i', indices on r p < p'): no call when i' = i + 1 and p' = p + 1,
 *      else one call: REF = the sequences of r's vertices p + 1 .. p' - 1, ALT = those of the query's i + 1 .. i' - 1, POS = the
 *      0-based base offset of REF's first byte along walk r.  If REF or ALT is empty both get the last base of a in front and
 *      POS moves one back.
 *   4. Nothing is normalised: no common prefix or suffix is trimmed, nothing is left-aligned (`bcftools norm` does that), the
 *      bytes are the graph's own in their original case.  Calls come in ascending POS and do not overlap.
 *   5. A call whose REF and ALT are the same bytes (other vertices, the same sequence) is returned like any other;
 *      phi_write_calls_vcf (phi_host.h) drops it and counts it.
 *   6. anchor[k] = the query index i of call k's left anchor a.
 *
 *   phi_calls_path   (no reference counterpart; for the comparison of data/run_PG.py:54-60) the path of the last phi_solve
 *                    against walk ref_walk.  PHI_ERR_STATE without a solved path.
 *   phi_calls_walk   (no reference counterpart; for the comparison of data/run_PG.py:54-60) walk `walk` against walk ref_walk:
 *                    a leave-one-out truth -- the dropped sample's own calls -- is made by the same code.
 *   phi_calls_stats  (no reference counterpart) what the last successful call did: sizes, the algorithmic bytes as DESIGN.md
 *                    4.16 counts them, GPU milliseconds per stage by HIP events on the context's stream.
 * The buffers behind phi_calls are owned by the context and stay valid until the next phi_calls_path / phi_calls_walk, phi_solve, phi_set_graph*
 * or phi_ctx_destroy.  Limits: fewer than 2^31 calls, a query and a reference walk of fewer than 2^31 - 1 entries each, an
 * allele of fewer than 2^31 bytes (PHI_ERR_UNSUPPORTED beyond); byte offsets are 64-bit.  walk or ref_walk outside the set
 * graph's walks (after a panel: the kept ones, renumbered): PHI_ERR_INVALID.  Before phi_set_graph or on a scout:
 * PHI_ERR_STATE.  After any refusal the context stays usable: graph, reads and result are as they were.
 */
typedef struct {
    int64_t n_calls;
    const int64_t *pos;                              /* [n_calls] 0-based, in bases of the reference walk */
    const int64_t *ref_off, *alt_off;                /* [n_calls + 1] call k's REF = ref_bytes[ref_off[k], ref_off[k + 1]) */
    const char *ref_bytes, *alt_bytes;
    const int32_t *anchor;                           /* [n_calls] rule 6 */
    int64_t n_shared, n_query, n_ref;                /* shared vertices; vertices of the query and of the reference walk */
    int64_t ref_span[2], query_span[2];              /* rule 2 */
    double gpu_ms;                                   /* first launch to last kernel, by HIP events */
} phi_calls;
typedef struct {
    int64_t n_query, n_ref, n_shared, n_pairs, n_calls;
    int64_t ref_bytes, alt_bytes;
    int64_t ref_bases, query_bases;                  /* bases of the whole reference walk and of the whole query */
    int64_t bytes_moved;                             /* the algorithmic bytes of all kernels */
    double table_gpu_ms, shared_gpu_ms, pairs_gpu_ms, fill_gpu_ms, gpu_ms;
} phi_calls_info;
int phi_calls_path(phi_ctx *ctx, int32_t ref_walk, phi_calls *out);
int phi_calls_walk(phi_ctx *ctx, int32_t walk, int32_t ref_walk, phi_calls *out);
int phi_calls_stats(phi_ctx *ctx, phi_calls_info *out);

/*
 * READ SUPPORT OF EVERY CALL: how many minimisers witness each call's ALT and REF, and how many of those the reads have seen
 * (calls_support.hip).  No reference counterpart: the reference writes no calls.  It is the per-record evidence
 * a genotyper's VCF carries (PanGenie, `bcftools`): at 0.1x to 2x most of the path is imputed from the panel, and INFO/PH alone
 * does not tell a call with ten witnessed minimisers from one with none.  THE RULE IS THIS PROJECT'S OWN: it is no other
 * tool's count and has not been compared with any other tool.
 *
 * The rule.  k and w are the context's parameters.  M(h) is the list phi_walk_minimizers(h) returns: occurrences (hash, pos),
 * pos in bases of walk h.  Entry t of walk h covers the bases [B_h(t), B_h(t + 1)); an occurrence LIES IN the entry that holds
 * its pos.  Q(j) is the number of bases of the query before query index j, R(p) that of walk r before its index p.
 *   1. Occurrences of the query.  Query index j sits on walk h_j at entry t_j: for phi_calls_walk h_j = walk and t_j = j; for
 *      the path h_j is the walk of the stretch that holds j (the result's path_hap[j]) and t_j that vertex's index on it.
 *      Index j contributes the occurrences of M(h_j) that lie in entry t_j, at the query coordinate
 *      x = Q(j) + (pos - B_{h_j}(t_j)).  For a walk that is M(walk) as it stands.  For the path it is a union per entry: THE
 *      K-MER OF AN OCCURRENCE WITHIN k + w - 2 BASES BEFORE A SWITCH CONTINUES ALONG THE WALK IT WAS SKETCHED ON, NOT ALONG
 *      THE PATH, and the windows are that walk's.  This is not corrected.
 *   2. Occurrences of the reference walk r: M(r), in its own coordinates.
 *   3. Witnesses.  Call k has its anchors at query indices i < i' and at indices p < p' on r (rule 3 of the calls).  The
 *      unpadded ALT is the interval [A0, A1) = [Q(i + 1), Q(i')) of the query, the unpadded REF is [R(p + 1), R(p')) of r;
 *      either may be empty.  An occurrence at x WITNESSES an interval when x < A1 and x + k > A0.  For a non-empty interval the
 *      k-mer holds at least one base of the allele; for an empty one (A0 = A1 = J) it holds both bases at the junction, so a
 *      deletion is witnessed by the k-mers that span it.
 *   4. Counts.  alt_n[k] and ref_n[k] are the witnesses of call k, as occurrences and not as distinct hashes.  alt_hit[k] and
 *      ref_hit[k] are those whose minimiser has its flag set in the context's CURRENT hit vector: after a solve the vector the
 *      solve read; several read sets, a ladder level, an exchanged multi-GPU vector are whatever is current.  0 of 0 is a
 *      valid answer (a walk shorter than w + k - 1 bases has no occurrence at all).
 *
 *   phi_calls_support        (no reference counterpart) the four counts of every call of the last successful phi_calls_path /
 *                            phi_calls_walk, their totals, the (call, side, entry) items the device worked through and its
 *                            GPU milliseconds by HIP events.  (The struct is phi_call_support: C has one name space for
 *                            both.)  The arrays are owned by the context and stay valid exactly as long as the buffers
 *                            behind phi_calls do.  PHI_ERR_STATE without a current calls result or on a scout; after a
 *                            refusal the context is as it was, the calls included.
 *   phi_calls_support_stats  (no reference counterpart) what the last successful phi_calls_support did: items, entries
 *                            visited, class records looked at, witnesses, the algorithmic bytes as DESIGN.md 4.16 counts
 *                            them, GPU milliseconds.
 * Limits: fewer than 2^39 items (PHI_ERR_UNSUPPORTED beyond).
 */
typedef struct {
    int64_t n_calls;
    const int32_t *alt_hit, *alt_n, *ref_hit, *ref_n; /* [n_calls] rule 4 */
    int64_t alt_hit_total, alt_n_total, ref_hit_total, ref_n_total;
    int64_t n_items;                                 /* (call, side, target entry) triples */
    double gpu_ms;                                   /* first fill to last kernel, by HIP events */
} phi_call_support;
typedef struct {
    int64_t n_calls, n_items;
    int64_t n_visited, n_records, n_witnesses;       /* walk entries whose class was read; class records looked at; witnesses */
    int64_t bytes_moved;                             /* the algorithmic bytes of the stage */
    double gpu_ms;
} phi_calls_support_info;
int phi_calls_support(phi_ctx *ctx, phi_call_support *out);
int phi_calls_support_stats(phi_ctx *ctx, phi_calls_support_info *out);

#ifdef __cplusplus
}
#endif
#endif
