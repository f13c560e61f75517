/*
 * phi_host.h -- C ABI of the host-side feeders of the hot path (libphi_host.so, CPU only).
 *
 * These are the steps on either side of the GPU path (SURVEY.md section 8f "next"):
 *   phi_gfa_read     gfa_read() + ILP_index::read_gfa()   src/gfa-io.cpp:462-508, src/ILP_index.cpp:20-155
 *   phi_reads_read   ILP_index::read_ip_reads()           src/ILP_index.cpp:313-328 (kseq FASTA/FASTQ, gz)
 *   phi_reads_stream_*  the same records in chunks, for files larger than one buffer; phi_reads_stream_open_blocks: over text
 *                       in memory + blocks a callback hands over (the rest of a stream whose beginning the device has taken)
 *   phi_text_stream_*   the (inflated) text of a reads file as it is, for phi_add_reads_text (phi_amd.h): the records are
 *                       found on the device, no host core parses a regular FASTA / FASTQ file
 *   phi_vcf_*        vcf2gfa.py (VCF + FASTA -> graph)              vcf2gfa.py:27-64, without vg / gfa2gbwt
 *   phi_hap_name     get_hap_name()                       src/misc.cpp:58-87
 *   phi_write_fasta  the FASTA writer                     src/ILP_index.cpp:1590-1598
 *   phi_format_*     the FASTA and the calls as text in memory (for phi_deflate_bgzf of phi_amd.h)
 * The arrays phi_gfa_read returns are exactly the arguments of phi_set_graph (phi_amd.h).
 * All functions return 0 or a negative code and never call exit(); *err receives a message.
 */
#ifndef PHI_HOST_H
#define PHI_HOST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phi_graph phi_graph;
typedef struct phi_reads phi_reads;

enum {
    PHI_HOST_OK = 0,
    PHI_HOST_ERR_IO = -1,       /* file cannot be opened / read (main.cpp:102-105 returns 1) */
    PHI_HOST_ERR_WALK = -2,     /* a walk holds a reverse-strand vertex (ILP_index.cpp:104-107 exits) */
    PHI_HOST_ERR_CYCLE = -3,    /* Kahn's algorithm did not reach every vertex: graph is not acyclic */
    PHI_HOST_ERR_INVALID = -4,
    PHI_HOST_ERR_UNSUPPORTED = -5,/* a link onto the reverse strand of its target: the reference's own adjacency for it depends on
                                     the line's place in the file (gfa-base.cpp:269-303): refused, not guessed */
    PHI_HOST_NEED_MORE = -6       /* phi_bam_header: the bytes given are a prefix of a header that may still be valid */
};

/* Parse S/L/W lines (plain or gzip), flip walks as gfa_walk_flip does, complete arcs with their
 * complements, keep forward-strand arcs, build walks / names / Kahn topological order. */
int phi_gfa_read(const char *path, phi_graph **out, char *err, int err_cap);
/* The same with the walks left as TEXT, for a caller that resolves them on the device (include/phi_amd.h phi_walk_text_*: at
 * chromosome scale the W-lines are 96 % of the file and resolving them was the reader's largest stage).  on_text (optional) is
 * called on a thread of the reader's own as soon as the walk fields are known -- before the segment names are --, with slices
 * of the mapped file (valid until the walks are resolved either way); it is joined before the call returns.
 *   phi_graph_walks_deferred   1 while the walks are text
 *   phi_graph_walk_texts       the walk fields again (optional tags may follow a walk); returns their number
 *   phi_graph_name_index       the name table's direct index: names are <prefix><canonical decimal> -> num2id[number];
 *                              PHI_HOST_ERR_UNSUPPORTED when some name is of another form or a W-line stands before an S-line
 *                              (the device path does not take such a file: phi_graph_resolve_walks)
 *   phi_graph_resolve_walks    the host path after all, with the reference's rules (steps naming no segment left out, walks
 *                              flipped by majority strand, a reverse vertex left over is PHI_HOST_ERR_WALK)
 *   phi_graph_set_walk_off     the device resolved them: their offsets [n_walks + 1]; the text is let go
 * phi_graph_walk_vtx stays NULL for walks resolved on the device. */
typedef struct { const char *text; int64_t n; } phi_host_walk_text;
typedef void (*phi_walk_text_fn)(void *user, const phi_host_walk_text *walks, int32_t n_walks);
int phi_gfa_read_deferred(const char *path, phi_graph **out, phi_walk_text_fn on_text, void *user, char *err, int err_cap);
/* phi_gfa_read_deferred on text already in memory, e.g. phi_gfa_gzip_split's host text (phi_amd.h): the graph, hap names, name
 * index and walks are those phi_gfa_read_deferred returns for a file holding text[0, n) (a W-line cut right after its 6th tab
 * has an empty walk field).  The text is BORROWED, not copied: it must stay valid and unchanged until the walks are resolved
 * (phi_graph_set_walk_off, phi_graph_resolve_walks) or the graph is freed, whichever comes first; the caller frees it.
 * name_for_messages (may be NULL) stands for the file in messages. */
int phi_gfa_read_deferred_text(const char *text, int64_t n, const char *name_for_messages, phi_graph **out, char *err, int err_cap);
int phi_graph_walks_deferred(const phi_graph *g);
int phi_graph_walk_texts(const phi_graph *g, phi_host_walk_text *out, int32_t cap);
int phi_graph_name_index(const phi_graph *g, const char **prefix, int32_t *prefix_n, const int32_t **num2id, int64_t *n_num);
int phi_graph_resolve_walks(phi_graph *g, char *err, int err_cap);
int phi_graph_set_walk_off(phi_graph *g, const int64_t *walk_off);
void phi_graph_free(phi_graph *g);

int32_t phi_graph_n_vtx(const phi_graph *g);
int32_t phi_graph_n_walks(const phi_graph *g);
int64_t phi_graph_n_edges(const phi_graph *g);
const char *phi_graph_seq_concat(const phi_graph *g);      /* node_seq, original case */
const int64_t *phi_graph_seq_off(const phi_graph *g);      /* [n_vtx+1] */
const int64_t *phi_graph_adj_off(const phi_graph *g);      /* [n_vtx+1] */
const int32_t *phi_graph_adj(const phi_graph *g);
const int64_t *phi_graph_walk_off(const phi_graph *g);     /* [n_walks+1] */
const int32_t *phi_graph_walk_vtx(const phi_graph *g);
const int32_t *phi_graph_topo_rank(const phi_graph *g);    /* top_order_map */
const char *phi_graph_hap_name(const phi_graph *g, int32_t walk);   /* sample + "." + hap (:98) */
const char *phi_graph_seg_name(const phi_graph *g, int32_t vtx);

/* A phased multi-sample VCF + a reference FASTA as the graph (the reference's second input route, vcf2gfa.py:27-64), without a
 * GFA in between.  The graph is exactly the one phi_amd/vcf2gfa.py writes (read_fasta_single, read_vcf, build, write_gfa, its
 * CHOP a parameter) and phi_gfa_read reads back: vertices, adjacency (out-edges ascending), walks, hap names, Kahn ranks.
 *   phi_vcf_read      the FASTA record (upper-cased; more than one record: PHI_HOST_ERR_INVALID) and the VCF (plain, gzip, BGZF):
 *                     the record rules on the FIXED columns -- first contig seen (others counted: phi_vcf_n_other_contig), REF
 *                     against the FASTA (phi_vcf_n_ref_mismatch), GT in FORMAT, sequence ALTs only, inside the contig --, the
 *                     stable sort by (start, end), the sites (phi_vcf_site_off[n_sites + 1]: records of every maximal run that
 *                     overlaps or touches).  The SAMPLE columns of the kept records are not parsed: phi_vcf_text holds them back
 *                     to back, record r's slice (from the byte after the line's 9th tab to its end, CR / LF stripped) at
 *                     [text_off[r], text_off[r + 1] - 1) with ONE LINE FEED behind it, ready for one upload (phi_vcf_genotypes
 *                     of phi_amd.h).  ALT a of record r: alt_bytes[alt_pos[alt_off[r] + a], alt_pos[alt_off[r] + a + 1]).
 *   phi_vcf_parse_gt  the exact scalar genotype parser over those slices, rows [rec_lo, rec_hi): what the device kernel computes
 *                     and its fallback.  gt[(r * n_samples + s) * 2 + column] (65 535 = that index or more; a record holds fewer
 *                     ALTs), ploidy[s] raised to min(2, GT parts other than ".").  PHI_HOST_ERR_INVALID where the Python raises.
 *   phi_vcf_build     genotype matrix -> graph with the walks left out (as phi_gfa_read_deferred leaves them; free it with
 *                     phi_graph_free) + the tables phi_vcf_walks (phi_amd.h) makes the walk entries from: unit_first[n_units + 1]
 *                     (units are backbone, alleles, backbone, ... and hold consecutive segment ids), per real site its backbone
 *                     unit and first allele unit, choice[site * n_kept_haps + kept haplotype] = allele index.  The two refusals
 *                     ("first base of the contig", "last base of the contig") are PHI_HOST_ERR_INVALID.  At most 16 threads.
 * Errors occur wherever the Python raises, and in two places where it does not: a #CHROM line that names samples behind kept data
 * lines (the script starts a new sample list there and then indexes the earlier records with it), and a POS that is not an
 * optionally signed run of decimal digits (Python's int() also takes forms such as "1_0"). */
typedef struct phi_vcf phi_vcf;
int phi_vcf_read(const char *vcf_path, const char *fasta_path, phi_vcf **out, char *err, int err_cap);
void phi_vcf_free(phi_vcf *v);
int32_t phi_vcf_n_samples(const phi_vcf *v);
const char *phi_vcf_sample_name(const phi_vcf *v, int32_t s);
const char *phi_vcf_contig(const phi_vcf *v);
int64_t phi_vcf_n_records(const phi_vcf *v);
int64_t phi_vcf_n_sites(const phi_vcf *v);
int64_t phi_vcf_n_other_contig(const phi_vcf *v);
int64_t phi_vcf_n_ref_mismatch(const phi_vcf *v);
int64_t phi_vcf_ref_len(const phi_vcf *v);
const char *phi_vcf_ref_seq(const phi_vcf *v);
const int64_t *phi_vcf_rec_start(const phi_vcf *v);        /* [n_records], 0-based */
const int64_t *phi_vcf_rec_end(const phi_vcf *v);
const int32_t *phi_vcf_rec_gt_index(const phi_vcf *v);     /* index of GT in FORMAT */
const int64_t *phi_vcf_rec_alt_off(const phi_vcf *v);      /* [n_records + 1] */
const int64_t *phi_vcf_alt_pos(const phi_vcf *v);
const char *phi_vcf_alt_bytes(const phi_vcf *v);
const int64_t *phi_vcf_site_off(const phi_vcf *v);
const char *phi_vcf_text(const phi_vcf *v);
const int64_t *phi_vcf_text_off(const phi_vcf *v);         /* [n_records + 1] */
int phi_vcf_parse_gt(const char *text, const int64_t *text_off, const int32_t *gt_index, int64_t rec_lo, int64_t rec_hi, int32_t n_samples,
                     uint16_t *gt, int32_t *ploidy, char *err, int err_cap);
int phi_vcf_build(phi_vcf *v, const uint16_t *gt, const int32_t *ploidy, int32_t max_len, phi_graph **out, char *err, int err_cap);
int64_t phi_vcf_n_units(const phi_vcf *v);                 /* these after phi_vcf_build */
const int32_t *phi_vcf_unit_first(const phi_vcf *v);
int64_t phi_vcf_n_real_sites(const phi_vcf *v);
const int32_t *phi_vcf_site_backbone(const phi_vcf *v);
const int32_t *phi_vcf_site_allele0(const phi_vcf *v);
int32_t phi_vcf_n_kept_haps(const phi_vcf *v);
const int32_t *phi_vcf_choice(const phi_vcf *v);

/* A region of an indexed VCF and FASTA: what `tabix FILE REGION` and `samtools faidx FILE REGION` do before a
 * record is looked at, so that a chromosome's VCF is neither inflated nor walked as a whole.  None of it needs a GPU.
 *   phi_region_parse   NAME, NAME:BEG or NAME:BEG-END, 1-based and inclusive as tabix and samtools read them, commas allowed in
 *                      the numbers; *end1 = -1 without END.  PHI_HOST_ERR_INVALID: empty, no name, BEG 0, END before BEG, a
 *                      number of more than 18 digits.
 *   phi_region_plan    the BGZF members of vcf_path that can hold a record of contig `name` overlapping the 0-based half-open
 *                      [beg, end), through vcf_path + ".tbi" (VCF preset only; a .csi and any other preset:
 *                      PHI_HOST_ERR_UNSUPPORTED; a gzip that is not BGZF too): reg2bins over 5 levels of 14 bits, chunks that end
 *                      at or before the linear index's value for window beg >> 14 dropped (a window beyond the list: no records),
 *                      the rest sorted and merged where they touch or overlap; a chunk (vbeg, vend) takes the members from
 *                      vbeg >> 16 on, through the one at vend >> 16 when vend & 0xffff is not 0, followed by BSIZE with pread --
 *                      nothing is inflated but the header: phi_region_header is every ## line and the #CHROM line.
 *                      phi_region_gz[n_gz] is the members' compressed bytes back to back (load != 0), a valid multi-member gzip
 *                      stream; phi_region_ranges[2 * n_ranges] every merged chunk as [p0, p1) of their inflated concatenation
 *                      (member m's text begins at phi_region_member_text_off[m], from the ISIZEs); both go unchanged to
 *                      phi_vcf_region_filter (phi_amd.h).  A contig the index does not name, an empty interval and a window
 *                      beyond the list give no members (phi_region_in_index tells the first).  Reads what htslib writes: several
 *                      chunks per bin, merged chunks, pseudo-bin 37450 (skipped), n_no_coor of any value or absent.
 *   phi_fasta_slice    bases [beg, end) (end < 0 or beyond: the record's length) of record `name` of a FASTA through
 *                      fasta_path + ".fai" (NAME LEN OFFSET LINEBASES LINEWIDTH, any number of records), upper-cased, line ends
 *                      removed, NUL behind them; freed with phi_region_free_bases.  A plain file: one pread.  A BGZF file: the
 *                      members that hold the range, found through fasta_path + ".gzi" (pairs as phi_amd.h describes them) and
 *                      inflated on the host.  A missing .fai or .gzi is PHI_HOST_ERR_IO and named; gzip that is not BGZF is
 *                      PHI_HOST_ERR_UNSUPPORTED.
 *   phi_region_open    all of it for PHI --region: parse, the contig's length from the .fai (a missing END or one beyond it
 *                      becomes that length; an empty interval and a name the .fai or the .tbi does not hold are refused), the
 *                      plan, the reference slice (phi_region_ref).
 *   phi_vcf_read_text  phi_vcf_read's rule pass over text in memory: ref[ref_len] is the reference from base `origin` of the
 *                      contig on, a record's position is POS - 1 - origin, so that the rule "inside the reference" drops the
 *                      records that reach over either edge (counted: phi_vcf_n_outside); contig: the one contig read (NULL: the
 *                      first seen).  phi_vcf_read is this with the whole files, origin 0 and NULL.
 *   phi_vcf_read_region   that over phi_region_header followed by the lines phi_vcf_region_filter kept. */
typedef struct phi_region phi_region;
int phi_region_parse(const char *region, char *name, int name_cap, int64_t *beg1, int64_t *end1, char *err, int err_cap);
int phi_region_plan(const char *vcf_path, const char *name, int64_t beg, int64_t end, int32_t load, phi_region **out, char *err, int err_cap);
int phi_region_open(const char *vcf_path, const char *fasta_path, const char *region, phi_region **out, char *err, int err_cap);
void phi_region_free(phi_region *r);
const char *phi_region_name(const phi_region *r);
int64_t phi_region_beg(const phi_region *r);               /* 0-based, half-open */
int64_t phi_region_end(const phi_region *r);
int64_t phi_region_contig_len(const phi_region *r);        /* the .fai's (phi_region_open) */
int32_t phi_region_in_index(const phi_region *r);
int64_t phi_region_n_members(const phi_region *r);
const int64_t *phi_region_member_at(const phi_region *r);        /* [n_members] file offsets */
const int64_t *phi_region_member_text_off(const phi_region *r);  /* [n_members + 1] */
int32_t phi_region_n_ranges(const phi_region *r);
const int64_t *phi_region_ranges(const phi_region *r);
const char *phi_region_gz(const phi_region *r);
int64_t phi_region_n_gz(const phi_region *r);
const char *phi_region_header(const phi_region *r);
int64_t phi_region_n_header(const phi_region *r);
const char *phi_region_ref(const phi_region *r);
int64_t phi_region_n_ref(const phi_region *r);
int64_t phi_region_fasta_members(const phi_region *r);     /* BGZF members inflated for the slice */
int phi_fasta_slice(const char *fasta_path, const char *name, int64_t beg, int64_t end, char **bases, int64_t *n_bases, int64_t *contig_len,
                    int64_t *members_read, char *err, int err_cap);
void phi_region_free_bases(char *p);
int phi_vcf_read_text(const char *text, int64_t n_text, const char *ref, int64_t ref_len, const char *ref_name, int64_t origin, const char *contig,
                      phi_vcf **out, char *err, int err_cap);
int phi_vcf_read_region(const phi_region *rg, const char *lines, int64_t n_lines, phi_vcf **out, char *err, int err_cap);
int64_t phi_vcf_origin(const phi_vcf *v);                  /* where phi_vcf_ref_seq begins on the contig */
int64_t phi_vcf_n_outside(const phi_vcf *v);               /* records with GT that reach beyond the reference (a region's edges) */

/* FASTA/FASTQ reader with kseq's record rules (multi-line FASTA, '+' quality blocks). */
int phi_reads_read(const char *path, phi_reads **out, char *err, int err_cap);
void phi_reads_free(phi_reads *r);
int64_t phi_reads_count(const phi_reads *r);
const char *phi_reads_bases(const phi_reads *r);           /* concatenated sequences */
const int64_t *phi_reads_off(const phi_reads *r);          /* [count+1] */
const char *phi_reads_name(const phi_reads *r, int64_t i);

/* The same reader, streaming: phi_reads_stream_next parses the next records into the
 * caller's buffers -- bases[bases_cap] (e.g. pinned memory the device copy reads while the next chunk
 * is parsed) and off[reads_cap + 1], off[0] = 0 -- never splitting a record, and returns their number:
 * 0 at the end of the file, negative on error (a single read longer than bases_cap). */
typedef struct phi_reads_stream phi_reads_stream;
int phi_reads_stream_open(const char *path, phi_reads_stream **out, char *err, int err_cap);
int64_t phi_reads_stream_next(phi_reads_stream *s, char *bases, int64_t bases_cap, int64_t *off, int64_t reads_cap,
                              char *err, int err_cap);
int64_t phi_reads_stream_reads(const phi_reads_stream *s);  /* records / bases returned so far */
int64_t phi_reads_stream_bases(const phi_reads_stream *s);
void phi_reads_stream_close(phi_reads_stream *s);

/* The same records from text that is already in memory followed by blocks a callback hands over: the way to finish, on
 * this exact state machine, a stream whose beginning the device has taken (phi_add_reads_text, phi_amd.h).  next returns
 * the length of the next block and its address (valid until the next call), 0 at the end, negative on error; it may be NULL. */
typedef int64_t (*phi_text_block_fn)(void *user, const char **block);
/* stream_offset = bytes of the stream before prefix[0] (what the device took: *n_taken of phi_reads_text_end): kseq reads in
 * blocks of 65 536 bytes and what it makes of a file's very last bytes depends on the file's size modulo that (kseq.h:81,113,242). */
int phi_reads_stream_open_blocks(const char *prefix, int64_t n_prefix, phi_text_block_fn next, void *user, int64_t stream_offset,
                                 phi_reads_stream **out, char *err, int err_cap);

/* The (inflated) text of a reads file as it is -- no parsing on the host: the bytes go to phi_add_reads_text, which finds the
 * records on the device.  phi_text_stream_read fills buf with the next bytes (plain files: several preads at once, so that
 * a pinned buffer fills at more than one core's copy rate) and returns their number: 0 at the end, negative on error. */
typedef struct phi_text_stream phi_text_stream;
int phi_text_stream_open(const char *path, phi_text_stream **out, char *err, int err_cap);
int64_t phi_text_stream_read(phi_text_stream *s, char *buf, int64_t cap, char *err, int err_cap);
void phi_text_stream_close(phi_text_stream *s);

/* The header of a BAM stream (SAM/BAM specification 4.2: magic BAM\1, l_text, text, n_ref, n_ref x (l_name, name, l_ref), all
 * little-endian) from the first n INFLATED bytes of the stream: what stands in front of the records that phi_add_reads_bam
 * (phi_amd.h) decodes, in the place of `samtools fastq` in front of ILP_index.cpp:313-328.
 *   PHI_HOST_OK           *records_start = offset of the first alignment record, *n_ref = reference sequences
 *   PHI_HOST_NEED_MORE    a valid prefix that ends inside the header; *records_start = a lower bound (> n) of the bytes needed
 *   PHI_HOST_ERR_INVALID  not a BAM header (wrong magic, a negative l_text or n_ref, an l_name below 1); err names the byte offset
 * Untrusted bytes: nothing outside bytes[0, n) is read, whatever the lengths in it say. */
int phi_bam_header(const void *bytes, int64_t n, int64_t *records_start, int32_t *n_ref, char *err, int err_cap);

/* The panel chosen from the reads: which walks of a graph of thousands to keep for the DP, from S[n_blocks * n_walks] =
 * read support per block of the graph and walk (phi_scout_scores, phi_amd.h).  It stands in for what `vg haplotypes` answers
 * from the reads' k-mers (data/vg_haplotypes.py:21-29) and for the lists of names of data/chop_graph.sh:46-66.  The rule is
 * this project's own; it is not `vg haplotypes`' and has not been compared with it:
 *   1. the walks with always[h] != 0 (always may be NULL) are in; more of them than n_want: PHI_HOST_ERR_INVALID, as is an
 *      n_want below 1 or above min(n_walks, 1022)
 *   2. in block b the walks are ordered by (-S[b][h], h)
 *   3. round r = 0, 1, ...: votes[h] = the number of blocks whose r-th walk is h with S[b][h] > 0; the walks with votes that
 *      are not yet in enter in the order (votes descending, total = sum over b of S[b][h] descending, id ascending) until the
 *      panel holds n_want walks
 *   4. a round that brings no votes ends the rounds; the rest is filled by (total descending, id ascending)
 * keep[n_walks] receives the flags (exactly n_want of them set); round_of[n_walks] (may be NULL): -1 an always walk, r entered
 * in round r, n_walks entered in the fill, -2 not chosen.  All host threads; the result does not depend on their number. */
int phi_panel_choose(const int32_t *S, int32_t n_blocks, int32_t n_walks, const uint8_t *always, int32_t n_want, uint8_t *keep,
                     int32_t *round_of);

/* Record id of the output: basename(gfa) minus extension + "_" + basename(reads), minus the last
 * extension of the whole string.  Returns the length or -1 if cap is too small. */
int phi_hap_name(const char *gfa_path, const char *reads_path, char *out, int cap);

/* ">" name " LN:" len, then the sequence in 80-column lines. */
int phi_write_fasta(const char *path, const char *name, const char *seq, int64_t len);

/* The calls of phi_calls_path / phi_calls_walk (phi_amd.h; no reference counterpart, the file serves the comparison of
 * data/run_PG.py:54-60) as plain-text VCFv4.2: ##fileformat, ##source, ##contig=<ID=contig,length=contig_len>, the INFO line
 * of PH and the FORMAT line of GT, the column line with one sample, then per call
 *     contig  pos + 1  .  REF  ALT  .  PASS  PH=<ph[k]>  GT  1
 * (tabs; INFO is "." where ph is NULL or ph[k] is NULL or empty; the bytes of REF and ALT as they are, case kept).  A call
 * whose REF and ALT are the same bytes is not written and counted in *n_dropped; *n_written = the records written (either
 * may be NULL).  PHI_HOST_ERR_INVALID, with a message, for a path that ends in ".gz" (this writer writes plain text and has no
 * deflate of its own: nothing is written; compressed calls are the text of phi_format_calls_vcf through phi_deflate_bgzf of
 * phi_amd.h, which is what PHI --bgzf and write_vcf(bgzf=True) do) and for a call with an empty allele; PHI_HOST_ERR_IO when
 * the file cannot be written. */
int phi_write_calls_vcf(const char *path, const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos,
                        const int64_t *ref_off, const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph,
                        int64_t *n_written, int64_t *n_dropped, char *err, int err_cap);

/* The same two texts in memory, for the BGZF writer on the device (phi_deflate_bgzf, phi_amd.h): *out[0, *n) holds exactly the
 * bytes phi_write_fasta / phi_write_calls_vcf write to their file; free it with phi_host_free_text.  phi_format_calls_vcf has
 * phi_write_calls_vcf's refusals (the file name's aside) and its count of dropped REF = ALT calls. */
int phi_format_fasta(const char *name, const char *seq, int64_t len, char **out, int64_t *n);
/* The one-line .fai of the file phi_format_fasta makes for this name and length (PHI --bgzf-index, beside the .gzi of
 * phi_deflate_bgzf_indexed): NAME \t LEN \t OFFSET \t LINEBASES \t LINEWIDTH \n, with NAME the header up to its first blank,
 * OFFSET the header line's length (where the sequence begins), LINEBASES = min(len, 80) and LINEWIDTH = LINEBASES + 1, both 0
 * for len == 0.  Free it with phi_host_free_text.  Written from the format's description; NOT compared with `samtools faidx`. */
int phi_format_fasta_fai(const char *name, int64_t len, char **out, int64_t *n);
int phi_format_calls_vcf(const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos, const int64_t *ref_off,
                         const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph, char **out, int64_t *n,
                         int64_t *n_written, int64_t *n_dropped, char *err, int err_cap);
void phi_host_free_text(char *p);

/* The same file with the read support of every call (phi_calls_support of phi_amd.h: alt_hit, alt_n, ref_hit, ref_n, [n_calls]
 * each).  Two more header lines behind the FORMAT line of GT,
 *     ##FORMAT=<ID=AK,Number=2,Type=Integer,Description="ALT witness minimisers: seen in the reads, all">
 * and the same for RK and REF, and every record ends  GT:AK:RK  1:alt_hit,alt_n:ref_hit,ref_n .  Everything else is byte for byte
 * what phi_write_calls_vcf / phi_format_calls_vcf give, their refusals and the dropped REF = ALT calls included (the counts of a
 * dropped call go with it).  The counts follow this project's own rule and are no other tool's. */
int phi_write_calls_vcf_support(const char *path, const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos,
                                const int64_t *ref_off, const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph,
                                const int32_t *alt_hit, const int32_t *alt_n, const int32_t *ref_hit, const int32_t *ref_n, int64_t *n_written,
                                int64_t *n_dropped, char *err, int err_cap);
int phi_format_calls_vcf_support(const char *contig, int64_t contig_len, const char *sample, int64_t n_calls, const int64_t *pos, const int64_t *ref_off,
                                 const char *ref_bytes, const int64_t *alt_off, const char *alt_bytes, const char *const *ph, const int32_t *alt_hit,
                                 const int32_t *alt_n, const int32_t *ref_hit, const int32_t *ref_n, char **out, int64_t *n, int64_t *n_written,
                                 int64_t *n_dropped, char *err, int err_cap);

#ifdef __cplusplus
}
#endif
#endif
