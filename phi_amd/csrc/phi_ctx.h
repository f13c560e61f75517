// phi_ctx.h -- the context behind the opaque phi_ctx handle of include/phi_amd.h.
#pragma once
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <future>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/phi_amd.h"
#include "phi_kernels.h"
#include "phi_host_par.h"          // phi_host_threads, phi_parallel_chunks, PhiHostError (no HIP: shared with dp_steps.h)
#include "solve_host.h"            // PhiAnchorHost, PhiAnchorSpan and the solve's host rules (no HIP: shared with its stand-alone check)
#include "reads_host.h"            // the read path's host rules: log, overflow list, set, offsets, text sizes (no HIP: shared with its stand-alone check)

// growable device buffer
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    uint32_t gen = 0;        // bumped by phi_dev_ensure whenever the memory behind p changes hands (a new allocation, a buffer from the pool)
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// host array that is NOT value-initialised on allocation: the threads that fill it touch its pages
// first (a std::vector would zero 38 MB on one thread before the threaded pass starts)
template <class T> struct PhiRawBuf {
    T *p = nullptr;
    size_t n = 0;
    PhiRawBuf() = default;
    PhiRawBuf(const PhiRawBuf &) = delete;
    PhiRawBuf &operator=(const PhiRawBuf &) = delete;
    ~PhiRawBuf() { free(p); }
    bool resize(size_t m)
    {
        free(p);
        p = m ? static_cast<T *>(malloc(m * sizeof(T))) : nullptr;
        n = p ? m : 0;
        return m == 0 || p != nullptr;
    }
    size_t size() const { return n; }
    T *data() const { return p; }
    T &operator[](size_t i) const { return p[i]; }
};

struct PhiComm;               // phi_comm.hip: the RCCL communicator of a multi-GPU job
struct PhiIpc;                // phi_ipc.hip: a group of PROCESSES of one node that map each other's hit vectors
#define PHI_HIT_RING 4        // hit buffers of a context in such a group (two otherwise)
struct PhiPeers;              // phi_comm.hip: the contexts of one process that exchange through peer-mapped memory

struct phi_ctx {
    int device = 0;
    PhiComm *comm = nullptr;
    PhiPeers *peers = nullptr;
    int peer_rank = 0;
    PhiIpc *ipc = nullptr;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t aux_stream = nullptr;    // the host thread's copies inside phi_set_graph, while the GPU thread works on `stream`
    std::string last_error;
    std::mutex err_mu;                                // guards last_error

    // params (main.cpp:118-131)
    int32_t k = 31, w = 25, recombination = 100;
    float threshold = 1.0f;
    uint32_t flags = PHI_FLAG_QCLP | PHI_FLAG_MIXED;
    int64_t solve_budget = 4096;                      // DP runs the exact search may use (phi_set_solve_budget); <= 0 = no limit

    // ---- graph, host side (decode, validation)
    bool have_graph = false;
    int32_t n_vtx = 0, n_walks = 0;
    std::vector<char> h_seq;
    std::vector<int64_t> h_seq_off, h_adj_off, h_walk_off, h_walk_base;   // h_walk_base: flat base offset of each walk
    std::vector<int32_t> h_adj, h_topo_rank, h_topo;
    PhiRawBuf<int32_t> h_walk_vtx;                    // host copy of the walk entries
    int64_t n_entries = 0, walk_bases = 0;

    // ---- the walks resolved on the device from the text of the W-lines (walk_text.hip): the text while it is being uploaded and
    //      resolved; afterwards d_walk_vtx holds the entries and phi_set_graph(walk_vtx = NULL) takes them from there
#define WT_TILE 4096                                  // bytes per tile; every walk's text starts on a tile boundary of d_text
    struct PhiWalkText {
        bool ready = false;
        int32_t n_walks = 0;
        std::vector<int64_t> tile0, t_len;            // first 4-KB tile and bytes of every walk's text in d_text
        std::vector<int32_t> ends;                    // first and last vertex of every walk (what phi_set_graph's host pass looks at)
        DevBuf d_text;
    } wtext;
    bool walks_on_device = false;
    int64_t walks_on_device_n = 0;
    // ---- the graph was set chopped (phi_set_graph_chopped): the vertices the solve names are pieces of the caller's
    struct PhiChop {
        bool on = false;
        std::vector<int32_t> first;                   // [vertices as passed in + 1] first piece of every vertex
        phi_chop_info info{};
    } chop;
    // ---- the graph was set as a panel of its walks (phi_set_graph_panel): the vertices and walks the solve names are the panel's
    struct PhiPanel {
        bool on = false;
        std::vector<int32_t> origin;                  // [panel vertices] the vertex as passed in
        std::vector<int32_t> kept;                    // [panel walks] the walk as passed in
        phi_panel_info info{};
        DevBuf d_full;                                // PHI_PANEL_RETAIN: the full graph's walk entries, for the next panel
        std::vector<int64_t> full_off;                // their walk offsets (empty: nothing retained)
    } panel;
    // ---- the scout (phi_scout_graph, set_graph.hip): the index of a graph of up to 65 535 walks without the DP's tables.  have_graph
    //      is set, so the reads routes and the index's accessors work; what needs the DP asks phi_refuse_scout first.  The
    //      full entries are d_walk_vtx and count as retained: panel.full_off names them, phi_set_graph_panel moves them to
    //      panel.d_full
    struct PhiScout {
        bool on = false;
        DevBuf d_scores;                              // [n_blocks * n_walks] read support per block and walk (panel_score.hip)
        int32_t n_blocks = 0;                         // 0: no phi_scout_scores yet on this scout
    } scout;
    // ---- "set graph" from a phased VCF (phi_vcf_genotypes, phi_vcf_walks): what the last calls did
    struct PhiVcf {
        bool have = false;
        phi_vcf_info info{};
    } vcf;

    // ---- graph, device side
    DevBuf d_seq, d_seq_off, d_walk_vtx, d_walk_off, d_topo, d_in_off, d_in_src;
    DevBuf d_e_out, d_st_rec, d_st_mask, d_in_packed;  // DP step stream (dp.hip)
    int dp_nw = 1;                                    // waves of the DP workgroup
    DevBuf d_wwords, d_wstarts, d_wbad, d_wascii;     // class space (contexts.hip): packed bases, start bitmap, non-ACGT mask, flat ASCII (only if needed)
    // graph-side de-duplication: walk entries of equal context form a class that is sketched once
    DevBuf d_vlen;                                    // bases of every vertex
    DevBuf d_ent_cls;                                 // class of every walk entry
    DevBuf d_cls_rep, d_cls_left, d_cls_mult, d_cls_base, d_cls_rec_off;   // per class: representative entry, has a left base, entries, first base in class space, first record
    int64_t n_cls = 0, cls_bases = 0;
    double index_gpu_ms = 0.0;                        // GPU time of the walk sketch (classes, class-space sketch, table): phi_index_stats
    // class records: (hash, class, position relative to the vertex, first / last entry of the representative under the k-mer, table slot)
    DevBuf d_rec_hash, d_rec_pos, d_rec_cls, d_rec_rel, d_rec_slot, d_rec_e0, d_rec_e1;
    int64_t n_rec = 0;
    DevBuf d_u_keys, d_u_rep, d_u_uid, d_u_replist;   // walk-minimiser table: keys, first record, dense id; dense id -> first record
    DevBuf d_rt;                                      // the same keys with their ids as the read table of the read probes (phi_launch_read_table)
    uint64_t rt_buckets = 0, rt_mask = 0;             // its 32-byte buckets (a power of two) and the mask of the bucket index
    // The k-mer table (set_graph.hip build_kmer_table; k <= 31): the same bucket format and dense ids under the keys
    // phi_kmer_mix(canonical k-mer) of the walk minimisers, for the clean waves of the 150-bp read kernel (sketch_rounds_kmer.inc).
    // kt_mask = 0: this graph has none (k = 32 and beyond, or two walk k-mers of one hash).
    DevBuf d_kt;
    uint64_t kt_buckets = 0, kt_mask = 0;
    // The batches that take it: those whose waves are all resident at once (seven a SIMD).  Such a launch lasts as long as one
    // wave's dependent chain, which the route shortens (C2: 10.9 -> 10.4 us); a launch of many rounds of waves is bound by the
    // table's random loads, and there the route measured 3 - 9 % SLOWER in spite of 30 % fewer vector instructions (C3, C5s:
    // profiles/kmer_keys_bench_ab.json).  PHI_SKETCH_KMER_KEYS=0: no batch; =2: every batch.
    int64_t kt_max_chunks = 0;
    void *h_stage[2] = {nullptr, nullptr};            // pinned staging buffers of large uploads from pageable memory (dev_mem.hip upload_staged)
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    DevBuf d_wpre;                                    // per DP run: prefix sums of the anchor weights (dp_events.hip)
    DevBuf d_rowdiag;                                 // class-lane blocks: the rows' own columns (dp_events.hip DP_ROW)
    DevBuf d_in_s, d_last_walk;                       // solve on the device copy of the anchors: a flag / the last walk per minimiser
    int64_t n_unique = 0;                             // distinct walk minimisers
    uint64_t u_cap = 0;
    DevBuf d_hit;                                     // uint8 per distinct walk minimiser
    // In a group of processes (phi_ipc.hip) the hit vector exists FOUR times and phi_reset_reads rotates d_hit <- alt.hit <-
    // hit_extra[0] <- hit_extra[1] <- d_hit: the peers read the vector of read set g while this rank scores read set g + 1,
    // and it is zeroed two read sets later.  hit_idx = which buffer of the ring (in the order the peers mapped them) d_hit is.
    DevBuf hit_extra[PHI_HIT_RING - 2];
    int hit_n = 2, hit_idx = 0;

    // ---- reads
    // The reference's read spectrum Sp_R (ILP_index.cpp:622-635) = the hit flags (read hashes that are walk minimisers, d_hit)
    // + the NOVEL read hashes.  The read kernels only LOG the novel ones, coalesced: d_novlog holds 1 << nov_shift entries per
    // 512-window chunk of every batch since the last flush (d_novcnt of them valid), d_ovlist what those entries could not
    // hold and what the byte-wise routine found.  phi_sp_flush (read_batches.hip) enters what has been logged into the set d_sp_keys
    // when something asks for |Sp_R| or for the list (phi_reads_stats, phi_solve, phi_spectrum_export / _import): once per
    // read set, with every lane of the launch an insert, instead of a dependent atomic behind each probe of the scoring wave.
    // The sizes of all three are rules of reads_host.h.
    struct PhiSpectrumSet {
        DevBuf d_sp_keys;                             // the set (open addressing), valid for generation sp_set_gen
        uint64_t sp_cap = 0;
        DevBuf d_sp_cnt;                              // [PHI_STRIPES][8] u64: keys in the set
        DevBuf d_export;                              // the set's keys as a list (a set that grows, phi_spectrum_export)
        int64_t sp_set_gen = -1;                      // the generation of reads whose hashes the set holds (another one: emptied before use)
        int64_t sp_gen = 0;                           // the generation of reads the context is in
        void new_generation() { sp_gen++; }           // (the set stays the ended generation's until the new one first needs it)
        void new_graph() { sp_set_gen = -1; }         // no generation's: emptied before use
    } spset;
    struct PhiReadLog {
        DevBuf d_novlog, d_novcnt;
        int32_t nov_shift = 6;
        int64_t log_chunks = 0, log_done = 0;         // chunks in the log; of those, already in the set
        int64_t logged_done = 0;                      // the n_logged stripes' sum at the last flush
        int64_t last_log_chunks = 0;                  // log chunks of the last batch (a replay rewinds the log by them)
        DevBuf d_ovlist;
        int64_t ov_cap = 0, ov_done = 0, ov_bound = 0;   // overflow list: capacity; entries already in the set; what the batches so far may have sent there at most
        bool async_batches = false;                   // batches went in without a wait behind them (phi_add_reads_device): their overflow shows at the next check
        bool next_flag_zeroed = false;                // a launch of this generation has zeroed the overflow counter of the next one
        DevBuf d_roff_made;                           // offsets made for a batch of one length the kernel does not take without (below 32)
        // what the log and the list held is in the set (phi_sp_flush): both start over within the generation.  The caller
        // zeroes the generation's overflow counter on the device.
        void flushed() { log_chunks = log_done = 0; ov_done = 0; ov_bound = 0; }
        // a new generation of reads starts both over; its overflow counter is another one (zeroed by the caller unless a launch has)
        void new_generation() { flushed(); logged_done = 0; last_log_chunks = 0; next_flag_zeroed = false; }
    } rlog;
    int64_t reads_bases = 0, reads_count = 0;
    int64_t spectrum_override = -1;
    DevBuf d_rbases, d_roff, d_peer_send;
    // device scalars: [0] err(u32 in low half) [1] n_bad ... [8..10] three rotating overflow counters (generation g: g % 3)
    DevBuf d_scalars;
    DevBuf d_stripes;                                 // [2][PHI_STRIPES][8] u64: novel hashes logged (with duplicates), emitted records
    // Double buffers: what a generation of reads accumulates in place (d_hit, d_stripes) exists twice.  phi_reset_reads swaps
    // the two on the host; what the ended generation filled is zeroed by the waves of the next read launch (sketch.hip
    // clean_finish), ready for the generation after: no reset launch.  The log needs none of it: a generation starts it over.
    struct PhiReadBufs {
        DevBuf hit, stripes;
        bool needs_clean = false;                     // filled by the ended generation, not zeroed yet
    } alt;

    uint32_t *h_err = nullptr;                        // pinned copy of the device error word, fetched behind a batch's last kernel
    // ---- reads as raw text (phi_add_reads_text, reads_text.hip): the device finds the records
    struct PhiTextStream {
        bool active = false, irregular = false, started = false, detached = false;
        bool carry_stale = false;                     // the carry is on the device only (pieces from parked text): h_carry is made when asked for
        int mode = 0;                                 // 0 FASTA, 1 FASTQ with four lines per record
        int64_t fed = 0, taken = 0;                   // stream bytes handed over / taken as whole records
        uint32_t carry_cap = 0, chunk_cap = 0, line_cap = 0;
        DevBuf text[2], bases[2], roff[2], tile_cnt, ls, pre, blk, sum;   // two slots: chunk i + 1 is copied while chunk i is sketched
        int slot = 0;                                 // slot of the last chunk
        uint32_t carry_len = 0, carry_at = 0;         // the carry: text[slot][carry_at, carry_at + carry_len)
        std::vector<char> h_carry;                    // the same bytes on the host (what phi_reads_text_end hands back)
        PhiTextSummary *h_sum = nullptr;              // pinned
        hipEvent_t ev_copy = nullptr;
        int last_slot = -1;                           // the chunk whose sketch may still be running: replayed if the spectrum set overflowed
        int64_t last_reads = 0, last_bases = 0;
        bool last_uniform = false;
        int dbg_slot = 0;                             // what the last piece took (phi_reads_text_last_batch: the parity tests)
        int64_t dbg_reads = 0, dbg_bases = 0;
        uint32_t why = 0, first_bad = 0;
    } text;

    // ---- reads from BAM (phi_add_reads_bam, bam.hip): the device finds the records of the inflated byte stream and decodes them
    struct PhiBamStream {
        bool active = false, failed = false, header_done = false;
        int32_t n_ref = 0;
        uint32_t tile = 0, list_cap = 0, max_tiles = 0, max_rec = 0;   // bytes per tile; record starts a tile's list holds; table sizes
        uint32_t carry_cap = 0, chunk_cap = 0;
        std::vector<unsigned char> h_hdr;             // the stream's first bytes, until they hold the whole header
        int64_t fed = 0;                              // bytes of the stream handed to the device so far, header included
        DevBuf text[2];                               // [carry | piece]: the carry of piece i is copied in front of piece i + 1 in the other slot
        DevBuf bases, roff, sum;                      // the decoded batch; the device summary
        DevBuf t_first, t_exit, t_status, t_cnt, t_skip, t_list, t_has, t_has_pre, t_use, t_base;   // per tile
        DevBuf rec_pos, rec_keep, kidx, klen, kseq, krev;                                             // per record / per kept record
        int slot = 0;
        uint32_t carry_len = 0, carry_at = 0;         // the carry: text[slot][carry_at, carry_at + carry_len)
        void *h_sum = nullptr;                        // pinned
        hipEvent_t ev_copy = nullptr;                 // the piece's copy (aux_stream) has landed
        int64_t one_len = -1;                         // -1 no read yet, -2 several lengths, else the one length
        int64_t dbg_reads = 0, dbg_bases = 0;         // what the last piece gave (phi_reads_bam_last_batch)
        phi_bam_info info{};
    } bam;

    // ---- a ladder of coverages from one read set (ladder.hip): the collected store, and its partition into bands
    struct PhiLadder {
        bool collecting = false, have_store = false, have_plan = false;
        int64_t first_ordinal = 0;
        int64_t n_reads = 0, n_bases = 0;             // the store
        int64_t one_len = -1;                         // -1 nothing collected yet, -2 reads of several lengths, else the one length
        DevBuf d_bases, d_off;                        // the store: bases in arrival order, n_reads + 1 offsets (64-bit)
        // the plan: bases band-major (every band starts on a 256-byte border), per band reads + 1 offsets from 0, and per
        // kept read its index in the store and where its bases lie there
        DevBuf d_pbases, d_poff, d_pidx, d_psrc, d_wg, d_tab;
        int64_t band_read0[PHI_LADDER_MAX_LEVELS + 1] = {0}, band_pos[PHI_LADDER_MAX_LEVELS + 1] = {0};
        int32_t scored = 0;                           // bands scored since the last phi_reset_reads
        phi_ladder_info info{};
    } ladder;

    // ---- scratch for sketch passes and compaction
    DevBuf d_blk_cnt, d_blk_off, d_flags, d_flags2, d_list, d_list2, d_list3, d_walk_last;
    DevBuf d_sel_off, d_sel_tri;                       // the filter's selected class records, packed per class (phi_solve: the anchors are expanded from these)
    DevBuf d_adj_off, d_adj, d_topo_rank, d_cnt_edge, d_walk_err;   // the walk-entry pass on the GPU (phi_walk_edges_kernel)
    DevBuf d_sa_cnt, d_sa_cur, d_sa_off, d_sa_idx;    // minimiser -> anchors CSR, built on the GPU

    // ---- solve state
    DevBuf d_m_rec, d_m_group, d_g_keys, d_g_rep, d_g_cnt, d_slot_maxcnt, d_slot_multi;
    DevBuf d_a_e1, d_g_off, d_g_span, d_a_weight;
    DevBuf d_dmax, d_bstart, d_top, d_ent, d_word;
    // event-driven DP (dp_events.hip)
    bool dp_dense_ready = false;                      // the every-vertex stream of dp.hip is on the device (fallback of the 4-wave event kernel)
    bool dp_events = false;
    int32_t n_k = 0;                                  // compact steps
    int64_t n_ev = 0;                                 // events
    std::vector<int32_t> h_cstep, h_kstep;            // topological step -> compact step (-1) and back
    // blocks of compact steps solved in parallel (dp_events.hip DP_ROW / DP_PATH, <= 64 walks): per graph, the steps a cut
    // may not sit before (a recombination edge would cross it / it would split a pair of allele steps); per solve, the cuts
    std::vector<int32_t> h_k_cut_ok;                  // [n_k + 1]: 1 = structurally a cut may sit before step k
    bool dp_blocks = false;
    int32_t n_blk = 0, blk_ring = 1024, blk_max_len = 0;
    std::vector<int32_t> h_blk_lo;
    DevBuf d_blk_lo, d_blk_ev, d_blk_S, d_row_out, d_rowend, d_blk_keys, d_blk_carry, d_cov, d_cov2, d_stepdiff;
    // more than 64 walks: the blocks' rows run on class lanes (dp_events.hip), regrouped per DP run
    bool dp_cls = false;
    int32_t blk_cls_target = 16;        // class-lane blocks: steps per block aimed at (halved when a block holds more than 64 classes)
    bool blk_no_small = false;          // this solve met a block task with more than 8 live runs on a lane: no 256-step blocks
    int32_t blk_ls = 64;                // row length of the per-(block, walk) tables
    uint32_t dp_retries = 0;            // the fallbacks DP runs have taken since the last solve began (PHI_DP_RETRY_*: phi_dp_probe reports them)
    DevBuf d_lane_walk, d_walk_lane, d_coff, d_blk_ncls, d_rownew, d_blk_bad;
    DevBuf d_seg_lo, d_seg_row, d_seg_S;  // the chain over the blocks cut into segments (dp_blocks.hip)
    DevBuf d_k_rec, d_k_in, d_cvtx, d_ev_e, d_ev_off, d_ev, d_off_end, d_off_start, d_scan_blk, d_scan_blk64, d_scan_blkoff;
    // The kept anchors as triples (minimiser id, first entry, last entry) in HBM, and whether the host has its copy:
    // a large model whose anchors all span an edge is solved on the device copy (solve_dev.hip); h_kept / h_dp are then
    // empty until something needs them (branch and bound, phi_kept_anchors: phi_host_anchors fetches them).
    DevBuf d_anchors, d_cov_all, d_cov_w, d_slots, d_slots2, d_segs, d_ctr, d_vmax;
    int64_t n_kept = 0, n_dp = 0;
    bool anchors_host = false;
    PhiAnchorSpan h_kept, h_dp;                       // kept anchors (in h_pin); dp anchors (span >= 1 edge: h_kept itself or h_dp_own)
    std::vector<PhiAnchorHost> h_dp_own;
    void *h_pin = nullptr;                            // pinned host buffer the kept anchors are downloaded into
    size_t h_pin_cap = 0;
    std::future<void> pin_future;                     // its allocation, started by phi_set_graph on a thread of its own
    std::future<int> dp_alloc_future;                 // the DP's entry-sized buffers of a chromosome-scale graph, allocated beside phi_set_graph's host pass
    std::vector<uint64_t> h_kept_hash;
    std::vector<int32_t> h_path_vtx, h_path_hap;
    std::vector<int64_t> h_n_minimizers, h_n_anchors;
    phi_result result{};
    bool solved = false;
    // the path of the last solve as stretches of walk entries (walk h, entries es .. ee of d_walk_vtx): what phi_calls_path
    // expands on the device (calls.hip)
    struct PhiPathSeg { int32_t h; int64_t es, ee; };
    std::vector<PhiPathSeg> path_segs;
    struct PhiCallSrc {      // where an allele's bytes lie on its walk: first base (in bases of the walk), vertex indices [v0, v1)
        int64_t base;
        int32_t v0, v1;
    };
    // ---- variant calls of the path or of a walk against a reference walk (calls.hip): the host copies phi_calls points into
    struct PhiCalls {
        bool have = false;
        std::vector<int64_t> pos, ref_off, alt_off;
        std::vector<int32_t> anchor;
        std::vector<char> ref_bytes, alt_bytes;
        int64_t span[4] = {0, 0, 0, 0};
        phi_calls_info info{};
        // what phi_calls_support (calls_support.hip) counts from, left on the device by the calls: the base offsets of the
        // reference walk's and the query's entries, per call the left anchor's query index and where the alleles lie on their
        // walks; on the host the query as stretches of walk entries ([0, n]: where every stretch starts in the query; behind:
        // its first walk entry; behind: the first entry of its walk) and the reference walk
        DevBuf d_r_base, d_q_base, d_anchor, d_ref_src, d_alt_src;
        std::vector<int64_t> stretches;
        int32_t ref_walk = 0;
        // the read support of the calls above: the host copies phi_call_support points into
        struct PhiSupport {
            bool have = false;
            std::vector<int32_t> cnt;                 // [4][n_calls]: alt_hit, alt_n, ref_hit, ref_n
            phi_call_support out{};
            phi_calls_support_info info{};
        } support;
    } calls;

    // ---- profiling of the sketch kernel
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    int prof_period = 1;                              // every prof_period-th sketch launch is bracketed
    uint64_t prof_seq = 0;
    size_t prof_used = 0;
    int64_t prof_bases = 0;
    double prof_ms_done = 0.0;
    int64_t prof_n_done = 0;
};

// PHI_TIMING=1: stage timings of phi_set_graph / phi_solve on stderr
struct PhiStageTimer {
    bool on;
    const char *what;
    std::chrono::steady_clock::time_point t0;
    explicit PhiStageTimer(const char *w) : on(getenv("PHI_TIMING") != nullptr), what(w), t0(std::chrono::steady_clock::now()) {}
    void lap(const char *stage)
    {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[phi timing] %s: %-28s %8.3f ms\n", what, stage, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

// Blocking copies / fills ON THE CONTEXT'S STREAM.  hipMemcpy / hipMemset would go through the null stream, whose hardware
// queue the runtime creates at first use (~20 ms, and as much again when the process ends) for nothing: every other
// piece of work of a context runs on its own streams.
static inline hipError_t phi_copy_sync(phi_ctx *c, void *dst, const void *src, size_t n, hipMemcpyKind kind)
{
    const hipError_t e = hipMemcpyAsync(dst, src, n, kind, c->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}
static inline hipError_t phi_memset_sync(phi_ctx *c, void *dst, int v, size_t n)
{
    const hipError_t e = hipMemsetAsync(dst, v, n, c->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

// walk of a walk entry
static inline int32_t phi_entry_walk(const phi_ctx *c, int64_t e)
{
    return phi_walk_of_entry(c->h_walk_off.data(), (int32_t)c->h_walk_off.size() - 1, e);
}

// phi_solve.cpp: host orchestration of the exact solve on top of the DP kernel
int phi_solve_impl(phi_ctx *c);
// one batch of reads the device can address; replay: the same batch again after the spectrum set was regrown
int phi_add_reads_device_impl(phi_ctx *c, const void *d_bases, const void *d_read_off, int64_t n_reads, int64_t n_bases, bool replay);
// replay of the batch at (d_bases, d_off) while the overflow list of novel hashes ran full under it (read_batches.hip; err = the
// device error word read behind the batch, after the stream was waited for)
int replay_if_full(phi_ctx *c, uint32_t err, const void *d_bases, const void *d_off, int64_t n_reads, int64_t n_bases);
// helpers of phi_abi.hip (errors) and dev_mem.hip (device memory) shared with every unit of host glue
int phi_fail(phi_ctx *c, int code, const char *fmt, ...);
#define HIPCHK(call) do { int rc_ = phi_hip_check(c, (call), #call); if (rc_) return rc_; } while (0)
#define PHICHK(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)
int phi_dev_ensure(phi_ctx *c, DevBuf &b, size_t bytes);
int phi_dev_grow_keep(phi_ctx *c, DevBuf &b, size_t bytes, size_t keep);   // grows and KEEPS the first `keep` bytes
void phi_dev_free(DevBuf &b);                          // to the pool of large buffers or back to the driver (waits for the device)
// the scout state ends (any phi_set_graph*, a new scout): its score matrix, up to 8 GB, goes with it
static inline void phi_scout_end(phi_ctx *c)
{
    c->scout.on = false; c->scout.n_blocks = 0;
    phi_dev_free(c->scout.d_scores);
}
// temporaries of one call: let go, through phi_dev_free, when the scope ends
struct PhiDevGuard {
    std::vector<DevBuf *> b;
    ~PhiDevGuard() { for (DevBuf *x : b) phi_dev_free(*x); }
};
// scalar slots in d_scalars (8 bytes each)
enum { S_ERR = 0, S_NBAD = 1, S_BATCHBAD = 2, S_NEMIT = 3, S_FILTERED = 4, S_INMODEL = 5, S_EXPORT = 6, S_BATCHBAD2 = 7,
       S_OVCNT = 8 /* .. 10: three rotating counters of the overflow list, generation g uses g % 3 */, S_N = 11 };
static inline uint64_t *scalar(phi_ctx *c, int i) { return c->d_scalars.as<uint64_t>() + i; }
#define STRIPE_BYTES ((size_t)PHI_STRIPES * 8 * 8)
// n bytes from host memory into b (grown to hold them) on `st`, the context's stream if null; not waited for.  256 MB and more
// from pageable memory go through the context's pinned staging buffers, given back by stage_release.
int phi_upload_bytes(phi_ctx *c, DevBuf &b, const void *src, size_t bytes, hipStream_t st);
template <class T> static inline int upload(phi_ctx *c, DevBuf &b, const T *src, size_t n, hipStream_t st = nullptr)
{
    return phi_upload_bytes(c, b, src, n * sizeof(T), st);
}
void stage_release(phi_ctx *c);                        // the pinned staging buffers given back
// count pass -> scan -> ordered write of the minimiser records of one packed flat sequence (phi_abi.hip)
int sketch_records(phi_ctx *c, const uint64_t *words, const unsigned long long *starts, int64_t n_bases, int32_t k, int32_t w,
                   const uint8_t *ascii_if_bad, DevBuf &out_hash, DevBuf &out_pos, int64_t *n_out);
// set_graph.hip: the body of phi_set_graph, and of phi_set_graph_chopped once the graph is chopped; what both check first
int set_graph_check_args(phi_ctx *c, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off, const int64_t *adj_off,
                         const int32_t *adj, int32_t n_walks, const int64_t *walk_off, const int32_t *walk_vtx, const int32_t *topo_rank);
int set_graph_check_offsets(phi_ctx *c, int32_t n_vtx, const int64_t *seq_off, const int64_t *adj_off, int32_t n_walks, const int64_t *walk_off);
int set_graph_impl(phi_ctx *c, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off, const int64_t *adj_off,
                   const int32_t *adj, int32_t n_walks, const int64_t *walk_off, const int32_t *walk_vtx, const int32_t *topo_rank);
// chop.hip: count / 64-bit scan / tiled expand of walk entries on the device (phi_set_graph_chopped, phi_vcf_walks)
int chop_expand_entries(phi_ctx *c, const int32_t *d_in, int64_t n_in, const int32_t *first, int32_t n_vtx, const int64_t *walk_off,
                        int32_t n_walks, int32_t max_len, DevBuf &d_out, std::vector<int64_t> &walk_off2, std::vector<int32_t> &ends,
                        int64_t *n_out_p, double *gpu_ms);
// PHI_DEVICE_POISON=<0..255> (tests; read once at load, -1 = unset): every device buffer is filled with that byte over its whole
// capacity when it gets a new owner, and the fill is complete on the device before the buffer is handed on.  Called wherever
// device memory changes hands: phi_dev_ensure, the text park's pieces, the inflater's buffers.  Not meant for groups of
// processes (phi_ipc.hip): their mailbox is not poisoned.
extern const int phi_device_poison;
int phi_dev_poison_fill(void *p, size_t bytes);         // 0 = filled
static inline int phi_dev_poison(void *p, size_t bytes) { return phi_device_poison < 0 ? 0 : phi_dev_poison_fill(p, bytes); }
// bam.hip
void phi_bam_drop(phi_ctx *c);                         // the stream's buffers let go (the context's end)
// a parked piece's bytes on `device`, landed (text_park.hip owns the park): PHI_ERR_INVALID when there is no such piece there
int phi_text_park_piece_dev(phi_text_park *p, int32_t index, int device, const void **d, int64_t *n, char *first = nullptr);   // *first (optional): the piece's first byte
// ladder.hip
int phi_ladder_collect(phi_ctx *c, const void *d_bases, const void *d_read_off, int64_t n_reads, int64_t n_bases);   // the hook of phi_add_reads_device_impl
void phi_ladder_drop(phi_ctx *c);                      // store and plan let go (a new graph, the context's end)
// PHI_PANEL_KEEP_READS: a collected store taken out of the context (its plan dropped) before the graph is set anew, and put back
void phi_ladder_detach(phi_ctx *c, phi_ctx::PhiLadder &out);
void phi_ladder_attach(phi_ctx *c, phi_ctx::PhiLadder &in);
// a batch whose data stays where it is: scored, waited for, and replayed if the overflow list of novel hashes ran full
int phi_score_resident_batch(phi_ctx *c, const void *d_bases, const void *d_read_off, int64_t n_reads, int64_t n_bases);
void phi_pool_bypass(bool on);                         // dev_mem.hip: what this thread lets go from now on goes back to the driver, not to the pool (a context that ends)
void phi_pool_flush(int device);                    // the pool of large device buffers let go (dev_mem.hip) back to the driver
int phi_hip_check(phi_ctx *c, hipError_t e, const char *what);
int phi_sync_check(phi_ctx *c);
// PHI_ERR_STATE naming the scout when the context holds one (phi_scout_graph: an index without the DP), else PHI_OK
static inline int phi_refuse_scout(phi_ctx *c, const char *what)
{
    return c->scout.on ? phi_fail(c, PHI_ERR_STATE, "%s on a scout graph (phi_scout_graph builds the index without the DP: phi_set_graph_panel sets the chosen panel)", what) : PHI_OK;
}
// pinned host buffer of at least `bytes` (contents are not kept)
int phi_pin_ensure(phi_ctx *c, size_t bytes);
int phi_dp_probe_impl(phi_ctx *c, const uint8_t *weights, int32_t *out_ends, int64_t *out_value, int32_t *out_end_walk,   // phi_solve.hip
                      int32_t *out_seg_walk, int64_t *out_seg_first, int64_t *out_seg_last, int64_t seg_cap, int64_t *n_seg, uint32_t *retries);
int phi_host_anchors(phi_ctx *c);                      // the host copy of the kept anchors, fetched if it is not there
// phi_ipc.hip
int phi_ipc_wait_pending(phi_ctx *c);                  // the context's stream waits for the last gather (every observer of the hit vector: phi_flush_reset)
int phi_ipc_before_generation(phi_ctx *c, int64_t gen); // phi_reset_reads, two resets in a row: before a hit buffer is zeroed by a launch of its own
void phi_ipc_launch_args(phi_ctx *c, PhiSketchArgs &A);  // every read launch: the flags its waves publish / look at
// sums of the striped counters (waits for the stream): novel hashes logged (with duplicates), emitted records
int phi_read_counts(phi_ctx *c, uint64_t *n_logged, uint64_t *n_emitted);
int phi_spectrum_count(phi_ctx *c, uint64_t *n_distinct);
// scan.hip: off[0..n] = exclusive prefix sums of cnt[0..n), off[n] = the total.  On the context's stream, not waited for; the
// scratch is the context's (d_scan_blk, d_scan_blk64, d_scan_blkoff), sized inside: one scan of a context at a time.
int phi_scan(phi_ctx *c, const uint8_t *cnt, int64_t n, int32_t *off);
int phi_scan(phi_ctx *c, const int32_t *cnt, int64_t n, int32_t *off);   // off may be cnt
int phi_scan(phi_ctx *c, const int32_t *cnt, int64_t n, int64_t *off);   // one workgroup up to 8192 items, three phases beyond
// flags[n] (0/1) -> ascending list of flagged indices (int32) in out (waits for the stream)
int phi_compact(phi_ctx *c, const uint8_t *flags, int64_t n, DevBuf &out, int64_t *n_out);
// The same kernels for a run that has no context (bgzf_index.hip): launches on the caller's stream over the caller's scratch,
// nothing waited for.  phi_scan_tiles: the one-workgroup scan, any n.  phi_compact_count: blk_cnt[phi_compact_blocks(n)] and
// blk_off[.. + 1], whose last entry is the number of flagged items; phi_compact_write: their indices, ascending.
int64_t phi_compact_blocks(int64_t n);
void phi_scan_tiles(hipStream_t st, const int32_t *cnt, int64_t n, int64_t *off);
void phi_compact_count(hipStream_t st, const uint8_t *flags, int64_t n, int32_t *blk_cnt, int64_t *blk_off);
void phi_compact_write(hipStream_t st, const uint8_t *flags, int64_t n, const int64_t *blk_off, int32_t *out);
