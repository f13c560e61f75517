// read_batches.hip -- the read path of the C ABI: batches of reads scored against the index (from host memory, from device
// memory, resident), the generations of reads (phi_reset_reads), and what is made of the novel hashes they log: the
// read-spectrum set, its size, its export and import.  No kernel: the launches are those of sketch.hip and table.hip.  The sizes
// of the log, the overflow list and the set, the offsets' check and the fixed-point launch fields are rules of reads_host.h.
#include <string.h>
#include "phi_ctx.h"
#include "phi_dev.h"

static unsigned long long *logged_stripes(phi_ctx *c) { return c->d_stripes.as<unsigned long long>(); }
static unsigned long long *emit_stripes(phi_ctx *c) { return c->d_stripes.as<unsigned long long>() + PHI_STRIPES * 8; }

// Called by everything that observes the read state.  A reset leaves nothing pending (phi_reset_reads swaps the context's
// double buffers, see phi_ctx.h); in a group of processes the last gather of the hit vectors runs on a stream of its own
// (phi_ipc.hip): the context's stream waits for it here.
int phi_flush_reset(phi_ctx *c) { return c && c->ipc ? phi_ipc_wait_pending(c) : PHI_OK; }

static void swap_read_bufs(phi_ctx *c)
{
    if (c->hit_n == PHI_HIT_RING) {
        // a group of processes: the ended read set's vector stays readable for the peers (it is zeroed two read sets later)
        const DevBuf old = c->d_hit;
        c->d_hit = c->alt.hit; c->alt.hit = c->hit_extra[0]; c->hit_extra[0] = c->hit_extra[1]; c->hit_extra[1] = old;
        c->hit_idx = (c->hit_idx + 1) % PHI_HIT_RING;
    } else {
        std::swap(c->d_hit, c->alt.hit);
    }
    std::swap(c->d_stripes, c->alt.stripes);
}

static int sum_stripes(phi_ctx *c, const void *d, int n_sets, uint64_t *out)
{
    std::vector<uint64_t> h((size_t)n_sets * PHI_STRIPES * 8);
    int rc = phi_hip_check(c, phi_copy_sync(c, h.data(), d, (size_t)n_sets * STRIPE_BYTES, hipMemcpyDeviceToHost), "D2H counters");
    if (rc) return rc;
    for (int s_ = 0; s_ < n_sets; s_++) {
        uint64_t a = 0;
        for (int i = 0; i < PHI_STRIPES; i++) a += h[((size_t)s_ * PHI_STRIPES + i) * 8];
        out[s_] = a;
    }
    return PHI_OK;
}

int phi_read_counts(phi_ctx *c, uint64_t *n_logged, uint64_t *n_emitted)
{
    int frc = phi_flush_reset(c);
    if (frc) return frc;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return phi_fail(c, PHI_ERR_DEVICE, "stream synchronize failed");
    uint64_t v[2];
    int rc = sum_stripes(c, c->d_stripes.p, 2, v);
    if (rc) return rc;
    if (n_logged) *n_logged = v[0];
    if (n_emitted) *n_emitted = v[1];
    return PHI_OK;
}

static int sp_set_size(phi_ctx *c, uint64_t *n)
{
    auto &S = c->spset;
    *n = 0;
    if (S.sp_cap == 0 || S.sp_set_gen != S.sp_gen) return PHI_OK;
    return sum_stripes(c, S.d_sp_cnt.p, 1, n);
}

static int sp_clear(phi_ctx *c, uint64_t cap)
{
    auto &S = c->spset;
    if (cap != S.sp_cap || !S.d_sp_keys.p) {
        phi_dev_free(S.d_sp_keys);
        S.sp_cap = 0;
        PHICHK(phi_dev_ensure(c, S.d_sp_keys, cap * 8));
        S.sp_cap = cap;
    }
    PHICHK(phi_dev_ensure(c, S.d_sp_cnt, STRIPE_BYTES));
    phi_launch_fill_u64(c->stream, S.d_sp_keys.as<uint64_t>(), (int64_t)cap, PHI_EMPTY_KEY);
    HIPCHK(hipMemsetAsync(S.d_sp_cnt.p, 0, STRIPE_BYTES, c->stream));
    return PHI_OK;
}

// room in the set for `more` further keys (load factor <= 0.5): a set that has to grow is listed, emptied at its new
// size and filled again
static int sp_reserve(phi_ctx *c, uint64_t in_set, uint64_t more)
{
    auto &S = c->spset;
    const uint64_t need = phi_set_capacity(in_set, more);
    if (S.sp_set_gen != S.sp_gen) {                         // the set of another generation of reads: nothing of it is kept
        PHICHK(sp_clear(c, phi_set_reusable(S.sp_cap, need) ? S.sp_cap : need));
        S.sp_set_gen = S.sp_gen;
        return PHI_OK;
    }
    if (need <= S.sp_cap) return PHI_OK;
    PHICHK(phi_dev_ensure(c, S.d_export, (size_t)std::max<uint64_t>(in_set, 1) * 8));
    HIPCHK(hipMemsetAsync(scalar(c, S_EXPORT), 0, 8, c->stream));
    phi_launch_spectrum_export(c->stream, S.d_sp_keys.as<uint64_t>(), (int64_t)S.sp_cap, S.d_export.as<uint64_t>(),
                               (unsigned long long *)scalar(c, S_EXPORT));
    HIPCHK(hipStreamSynchronize(c->stream));
    PHICHK(sp_clear(c, need));
    phi_launch_spectrum_insert(c->stream, S.d_export.as<uint64_t>(), (int64_t)in_set, S.d_sp_keys.as<uint64_t>(), S.sp_cap - 1,
                               S.d_sp_cnt.as<unsigned long long>(), nullptr, 0, nullptr, nullptr, (uint32_t *)scalar(c, S_ERR));
    return PHI_OK;
}

// The set made current: every novel hash this generation of reads has logged so far is entered (the log's chunks since
// the last flush, the overflow list's entries since then).  Waits for the stream.  *n_in_set (optional) = the set's size.
int phi_sp_flush(phi_ctx *c, uint64_t *n_in_set)
{
    auto &S = c->spset;
    auto &L = c->rlog;
    PHICHK(phi_sync_check(c));                                // (also: an overflow list that ran full under an unwaited batch)
    L.async_batches = false;
    uint64_t logged = 0, in_set = 0;
    PHICHK(phi_read_counts(c, &logged, nullptr));
    unsigned long long ov_now = 0;
    HIPCHK(phi_copy_sync(c, &ov_now, scalar(c, S_OVCNT + (int)(S.sp_gen % 3)), 8, hipMemcpyDeviceToHost));
    if ((int64_t)ov_now > L.ov_cap) ov_now = (unsigned long long)L.ov_cap;
    const bool pending = L.log_chunks > L.log_done || (int64_t)ov_now > L.ov_done;
    PHICHK(sp_set_size(c, &in_set));
    if (pending) {
        const uint64_t more = logged > (uint64_t)L.logged_done ? logged - (uint64_t)L.logged_done : 0;
        PHICHK(sp_reserve(c, in_set, more));
        if (L.log_chunks > L.log_done)
            phi_launch_spectrum_flush(c->stream, L.d_novlog.as<uint64_t>(), L.d_novcnt.as<uint16_t>(), L.log_done, L.log_chunks, L.nov_shift,
                                      S.d_sp_keys.as<uint64_t>(), S.sp_cap - 1, S.d_sp_cnt.as<unsigned long long>(), c->k, c->d_u_keys.as<uint64_t>(),
                                      c->u_cap - 1, (uint32_t *)scalar(c, S_ERR));
        if ((int64_t)ov_now > L.ov_done)
            phi_launch_spectrum_insert(c->stream, L.d_ovlist.as<uint64_t>() + L.ov_done, (int64_t)ov_now - L.ov_done, S.d_sp_keys.as<uint64_t>(),
                                       S.sp_cap - 1, S.d_sp_cnt.as<unsigned long long>(), nullptr, 0, nullptr, nullptr, (uint32_t *)scalar(c, S_ERR));
        HIPCHK(hipGetLastError());
        L.log_done = L.log_chunks; L.ov_done = (int64_t)ov_now; L.logged_done = (int64_t)logged;
        PHICHK(phi_sync_check(c));
        PHICHK(sp_set_size(c, &in_set));
    }
    if (n_in_set) *n_in_set = in_set;
    return PHI_OK;
}

// |Sp_R| = hit flags set (read hashes that are walk minimisers) + size of the set of the others
int phi_spectrum_count(phi_ctx *c, uint64_t *n_distinct)
{
    uint64_t in_set = 0, flagged = 0;
    PHICHK(phi_sp_flush(c, &in_set));
    if (c->n_unique > 0) {
        HIPCHK(hipMemsetAsync(scalar(c, S_EXPORT), 0, 8, c->stream));
        phi_launch_count_flags(c->stream, c->d_hit.as<uint8_t>(), c->n_unique, (unsigned long long *)scalar(c, S_EXPORT));
        HIPCHK(hipMemcpyAsync(&flagged, scalar(c, S_EXPORT), 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    *n_distinct = in_set + flagged;
    return PHI_OK;
}

// wait for the stream and translate the device error word
int phi_sync_check(phi_ctx *c)
{
    PHICHK(phi_flush_reset(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    uint64_t s[S_N];
    HIPCHK(phi_copy_sync(c, s, c->d_scalars.p, sizeof s, hipMemcpyDeviceToHost));
    const uint32_t err = (uint32_t)s[S_ERR];
    if (err & PHI_KERR_TABLE_FULL) return phi_fail(c, PHI_ERR_OVERFLOW, "open-addressed table overflow (probe bound %d), or the overflow list of novel read hashes ran full under a batch handed over with phi_add_reads_device", PHI_MAX_PROBE);
    if (err & PHI_KERR_SENTINEL) return phi_fail(c, PHI_ERR_UNSUPPORTED, "a minimiser hashes to UINT64_MAX (table sentinel)");
    if (err & PHI_KERR_HASH_COLLISION) return phi_fail(c, PHI_ERR_UNSUPPORTED, "two different k-mers of the reads and walks share a MurmurHash3 value: the k-mer route cannot reproduce the reference's result for this read set (set PHI_SKETCH_KMER_KEYS=0 and run again)");
    return PHI_OK;
}

extern "C" {

int phi_add_reads_device(phi_ctx *c, const void *d_bases, const void *d_read_off, int64_t n_reads, int64_t n_bases)
{
    const int rc = phi_add_reads_device_impl(c, d_bases, d_read_off, n_reads, n_bases, false);
    if (c && rc == PHI_OK) c->rlog.async_batches = true;            // nobody waits behind this batch: an overflow list that ran full shows at the next check
    return rc;
}

}  // extern "C"

// replay: the same batch again after the overflow list of novel hashes was grown (its first pass filled the list):
// everything a batch does is idempotent (hit flags, the log's entries: the replay rewrites the same ones) except the
// counts of emitted minimisers and of logged hashes, which are not repeated
int phi_add_reads_device_impl(phi_ctx *c, const void *d_bases, const void *d_read_off, int64_t n_reads, int64_t n_bases, bool replay)
{
    if (!c) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_add_reads before phi_set_graph");
    if (n_reads < 0 || n_bases < 0 || (n_bases > 0 && !d_bases)) return phi_fail(c, PHI_ERR_INVALID, "phi_add_reads: bad arguments");
    if (__builtin_expect(c->ladder.collecting, 0)) return phi_ladder_collect(c, d_bases, d_read_off, n_reads, n_bases);   // phi_reads_collect_begin: kept, not scored
    auto &L = c->rlog;
    // no offsets: reads of one length, n_bases / n_reads each
    int64_t uniform_len = 0;
    if (!d_read_off && n_reads > 0 && n_bases > 0) {
        if (n_bases % n_reads) return phi_fail(c, PHI_ERR_INVALID, "phi_add_reads_device without offsets: %lld bases are not %lld reads of one length", (long long)n_bases, (long long)n_reads);
        const PhiOneLength one = phi_device_one_length(n_reads, n_bases);
        if (one.make_offsets) {
            PHICHK(phi_dev_ensure(c, L.d_roff_made, (size_t)(n_reads + 1) * 8));
            phi_launch_iota_i64(c->stream, L.d_roff_made.as<int64_t>(), n_reads + 1, one.step);
            d_read_off = L.d_roff_made.p;
        }
        uniform_len = one.uniform_len;
    }
    if (n_reads == 0 || n_bases == 0) { if (!replay) c->reads_count += n_reads; return PHI_OK; }
    HIPCHK(hipSetDevice(c->device));
    c->solved = false;
    // this batch's part of the log of novel hashes, behind the chunks logged so far (phi_log_plan of reads_host.h: the log
    // grows -- keeping what it holds -- up to 1 GB; beyond that what it holds is entered into the set and the log starts over)
    const int64_t n_log_chunks = phi_sketch_read_chunks(c->k, c->w, uniform_len, n_reads, n_bases);
    {
        size_t budget = (size_t)1 << 30;
        if (const char *e = getenv("PHI_NOVLOG_BUDGET")) budget = (size_t)std::max<long long>(atoll(e), 1);      // tests: a log that starts over
        const PhiLogPlan P = phi_log_plan(L.log_chunks, L.last_log_chunks, replay, n_log_chunks, L.nov_shift, L.d_novlog.cap, L.d_novcnt.cap, budget);
        L.log_chunks = P.base;                                 // (a replay: the same entries again)
        if (P.flush_first) {
            PHICHK(phi_sp_flush(c, nullptr));
            L.flushed();
            // (the overflow list starts over with the log: what it held is in the set)
            HIPCHK(hipMemsetAsync(scalar(c, S_OVCNT + (int)(c->spset.sp_gen % 3)), 0, 8, c->stream));
        }
        if (P.log_bytes) {
            PHICHK(phi_dev_grow_keep(c, L.d_novlog, P.log_bytes, P.keep_log));
            PHICHK(phi_dev_grow_keep(c, L.d_novcnt, P.cnt_bytes, P.keep_cnt));
        }
        // The overflow list: room for everything this batch can send there (phi_ov_batch_bound), since a batch handed over with
        // phi_add_reads_device has nobody behind it to grow the list and replay (phi_add_reads and the text path do:
        // replay_if_full).  Memory that is reserved, not touched: 0.9 bytes per base at w = 25.
        if (!replay) {
            L.ov_bound += phi_ov_batch_bound(n_bases, c->w);
            const char *e = getenv("PHI_OVLIST_CAP");                                                                     // tests: a list that runs full (provokes the replay)
            if (e && !L.d_ovlist.p) {
                L.ov_cap = std::max<long long>(atoll(e), 1);
                PHICHK(phi_dev_ensure(c, L.d_ovlist, (size_t)L.ov_cap * 8));
            } else if (const int64_t cap = phi_ov_capacity(L.ov_bound, L.ov_cap); !e && cap != L.ov_cap) {
                PHICHK(phi_dev_grow_keep(c, L.d_ovlist, (size_t)cap * 8, (size_t)L.ov_cap * 8));
                L.ov_cap = cap;
            }
        }
    }
    // ONE launch per batch: every wave stages its chunk straight from the ASCII bases (2-bit pack, bases outside
    // ACGTacgt, read starts from the offsets), sketches, hashes and probes; windows touching a base outside ACGT
    // take the exact byte-wise routine inside the same wave
    PhiSketchArgs A{};
    A.ascii = (const uint8_t *)d_bases;
    A.read_off = (const int64_t *)d_read_off; A.n_reads = n_reads;
    A.uniform_len = (int32_t)uniform_len; A.inv_len = uniform_len ? 1.0 / (double)uniform_len : 0.0;
    A.inv_len_q32 = phi_inv_len_q32(uniform_len); A.reads_per_base_q32 = phi_reads_per_base_q32(n_reads, n_bases);
    A.allslow = c->k > PHI_MAX_K_PACKED;                       // longer k-mers: the byte-wise routine for every window
    A.n_bases = n_bases; A.k = c->k; A.w = c->w;
    A.n_logged = replay ? nullptr : logged_stripes(c);
    A.n_emitted = replay ? nullptr : emit_stripes(c);
    A.u_rt = c->d_rt.as<uint64_t>(); A.u_bmask = c->rt_mask;
    A.hit = c->d_hit.as<uint8_t>();
    A.err = (uint32_t *)scalar(c, S_ERR);
    if (c->kt_mask) {
        // the k-mer route of the clean 150-bp waves, for a batch whose waves are resident at once (phi_ctx.h kt_max_chunks;
        // PHI_SKETCH_KMER_KEYS=0: the hash route for every batch, =2: the k-mer route for every batch)
        const char *e = getenv("PHI_SKETCH_KMER_KEYS");
        const int mode = e ? atoi(e) : 1;
        if (mode >= 2 || (mode == 1 && n_log_chunks <= c->kt_max_chunks)) { A.k_rt = c->d_kt.as<uint64_t>(); A.k_bmask = c->kt_mask; }
    }
    A.nov_log = L.d_novlog.as<uint64_t>(); A.nov_cnt = L.d_novcnt.as<uint16_t>(); A.log_base = L.log_chunks; A.nov_shift = L.nov_shift;
    A.ov_list = L.d_ovlist.as<uint64_t>(); A.ov_cap = L.ov_cap;
    A.ov_count = (unsigned long long *)scalar(c, S_OVCNT + (int)(c->spset.sp_gen % 3));
    L.log_chunks += n_log_chunks; L.last_log_chunks = n_log_chunks;
    if (c->alt.needs_clean) {
        // the first launch since the reset: its waves zero what the ended generation filled (the other half of the
        // double buffers) for the generation after this one, and that generation's overflow counter
        A.q_clean = 1;
        A.ov_zero = (unsigned long long *)scalar(c, S_OVCNT + (int)((c->spset.sp_gen + 1) % 3));
        A.q_hit_words = c->alt.hit.as<uint64_t>(); A.q_n_hit_words = c->n_unique / 8 + 1;
        A.q_stripes = c->alt.stripes.as<uint64_t>(); A.q_n_stripe_words = 2 * PHI_STRIPES * 8;
        c->alt.needs_clean = false;
        L.next_flag_zeroed = true;
    }
    phi_ipc_launch_args(c, A);                                 // (a context in a group of processes: the flags of its exchanges)
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (c->prof && c->prof_period > 0 && (c->prof_seq++ % c->prof_period) == 0) {
        if (c->prof_used == c->prof_events.size()) {
            hipEvent_t a, b;
            HIPCHK(hipEventCreate(&a));
            HIPCHK(hipEventCreate(&b));
            c->prof_events.emplace_back(a, b);
        }
        t0 = c->prof_events[c->prof_used].first; t1 = c->prof_events[c->prof_used].second;
        c->prof_used++;
        c->prof_bases += n_bases;
    }
    phi_launch_sketch(c->stream, PHI_MODE_PROBE, A, t0, t1);
    HIPCHK(hipGetLastError());
    if (!replay) { c->reads_bases += n_bases; c->reads_count += n_reads; }
    return PHI_OK;
}


// After the stream has been waited for: if the overflow list of novel hashes ran full under the batch whose data still
// sits at (d_bases, d_off) -- chunks that emit far more than random sequence does; the reference's std::map has no such
// limit, ILP_index.cpp:622-635 -- grow the list (keeping what it holds: everything below its old capacity is valid) and
// replay that batch.  err = the device error word as read behind the batch.
int replay_if_full(phi_ctx *c, uint32_t err, const void *d_bases, const void *d_off, int64_t n_reads, int64_t n_bases)
{
    for (int attempt = 0; attempt < 8 && (err & PHI_KERR_TABLE_FULL); attempt++) {
        unsigned long long *cnt = (unsigned long long *)scalar(c, S_OVCNT + (int)(c->spset.sp_gen % 3));
        unsigned long long wanted = 0;
        HIPCHK(phi_copy_sync(c, &wanted, cnt, 8, hipMemcpyDeviceToHost));
        const PhiOvReplay R = phi_ov_replay(wanted, c->rlog.ov_cap);
        PHICHK(phi_dev_grow_keep(c, c->rlog.d_ovlist, (size_t)R.cap * 8, (size_t)R.valid * 8));
        c->rlog.ov_cap = R.cap;
        HIPCHK(phi_copy_sync(c, cnt, &R.valid, 8, hipMemcpyHostToDevice));
        err &= ~PHI_KERR_TABLE_FULL;
        HIPCHK(phi_copy_sync(c, scalar(c, S_ERR), &err, 4, hipMemcpyHostToDevice));
        PHICHK(phi_add_reads_device_impl(c, d_bases, d_off, n_reads, n_bases, true));
        HIPCHK(phi_copy_sync(c, &err, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost));
    }
    return PHI_OK;
}

// A batch whose data stays at (d_bases, d_read_off) until this returns: scored, the error word fetched behind its kernel, one
// wait for everything, and the replay if the overflow list ran full.  tm (optional): the caller's laps.
static int score_wait_replay(phi_ctx *c, const void *d_bases, const void *d_read_off, int64_t n_reads, int64_t n_bases, PhiStageTimer *tm)
{
    PHICHK(phi_add_reads_device_impl(c, d_bases, d_read_off, n_reads, n_bases, false));
    HIPCHK(hipMemcpyAsync(c->h_err, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (tm) tm->lap("H2D + sketch + probe");
    if (*c->h_err & PHI_KERR_TABLE_FULL) {
        PHICHK(replay_if_full(c, *c->h_err, d_bases, d_read_off, n_reads, n_bases));
        if (tm) tm->lap("overflow list grown, batch replayed");
    }
    return PHI_OK;
}

int phi_score_resident_batch(phi_ctx *c, const void *d_bases, const void *d_read_off, int64_t n_reads, int64_t n_bases)
{
    if (c->rlog.async_batches) { PHICHK(phi_sync_check(c)); c->rlog.async_batches = false; }   // (a replay below must only ever concern THIS batch)
    if (!c->h_err) HIPCHK(hipHostMalloc((void **)&c->h_err, 64, hipHostMallocDefault));
    return score_wait_replay(c, d_bases, d_read_off, n_reads, n_bases, nullptr);
}

extern "C" {

int phi_add_reads(phi_ctx *c, const char *bases, const int64_t *read_off, int64_t n_reads)
{
    if (!c) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_add_reads before phi_set_graph");
    if (n_reads < 0 || (n_reads > 0 && !read_off)) return phi_fail(c, PHI_ERR_INVALID, "phi_add_reads: bad arguments");
    if (n_reads == 0) return PHI_OK;
    if (read_off[0] != 0) return phi_fail(c, PHI_ERR_INVALID, "read_off must start at 0");
    const int64_t first_bad = phi_offsets_first_bad(read_off, n_reads, false, 0);
    if (first_bad >= 0) return phi_fail(c, PHI_ERR_INVALID, "read_off not monotone at read %lld", (long long)first_bad);
    const int64_t n_bases = read_off[n_reads];
    if (n_bases > 0 && !bases) return phi_fail(c, PHI_ERR_INVALID, "phi_add_reads: bases is null");
    // reads of one length (>= 32): their offsets are r * length -- they need not cross the link, nor be read by the kernel
    const bool uniform = phi_reads_one_length(read_off, n_reads);
    HIPCHK(hipSetDevice(c->device));
    PhiStageTimer tm("add_reads");
    // (every call ends with a wait for the stream: nothing of an earlier batch still reads the staging buffers)
    if (c->rlog.async_batches) { PHICHK(phi_sync_check(c)); c->rlog.async_batches = false; }   // (a replay below must only ever concern THIS batch)
    PHICHK(phi_dev_ensure(c, c->d_roff, (size_t)(n_reads + 1) * 8));
    if (!c->h_err) HIPCHK(hipHostMalloc((void **)&c->h_err, 64, hipHostMallocDefault));
    tm.lap("buffers");
    // One staged copy, then the kernel, on one stream.  What was measured on the MI355X box before settling for it
    // (profiles/r03_h2d_experiments.txt; C2 = 5.2 MB per batch, the link moves 52-57 GB/s):
    //   * pieces of the batch copied on a second stream while the piece before is sketched: every copy-engine -> compute
    //     dependency (event record + stream wait) costs ~50 us, more than the kernel of a 1-MB piece: 300 us per batch
    //     with 1-MB pieces, 262 with 2-MB, against 177 for the single copy (C3: 2245 / 1810 / 1277 us);
    //   * the kernel reading pinned bases in place across the link (every base is loaded exactly once): shader reads of
    //     host memory reach 25-32 GB/s, half the copy engine's rate: 190 us (C3: 1673 us).
    PHICHK(phi_dev_ensure(c, c->d_rbases, (size_t)std::max<int64_t>(n_bases, 1)));
    if (!uniform) HIPCHK(hipMemcpyAsync(c->d_roff.p, read_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n_bases) HIPCHK(hipMemcpyAsync(c->d_rbases.p, bases, (size_t)n_bases, hipMemcpyHostToDevice, c->stream));
    // (host buffers are borrowed for the call only: the wait behind the kernel is the wait for the copies as well)
    return score_wait_replay(c, c->d_rbases.p, uniform ? nullptr : c->d_roff.p, n_reads, n_bases, &tm);
}

int phi_reset_reads(phi_ctx *c)
{
    if (!c) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_reset_reads before phi_set_graph");
    HIPCHK(hipSetDevice(c->device));
    // The buffers this generation filled go to the back (the next read launch zeroes them), the other half
    // comes to the front: no launch, no wait.  The log of novel hashes starts over; the set made from it belongs to the
    // ended generation (sp_set_gen) and is emptied when the new one first needs it.
    const bool front_dirty = c->alt.needs_clean;               // two resets with no read launch in between
    swap_read_bufs(c);
    c->alt.needs_clean = true;
    if (front_dirty) {
        PHICHK(phi_ipc_before_generation(c, c->spset.sp_gen + 1));   // (a group of processes: the peers are done with what is about to be zeroed)
        // nothing zeroed the half that comes to the front: do it now
        phi_launch_reset_reads(c->stream, c->d_hit.as<uint64_t>(), c->d_hit.p ? c->n_unique / 8 + 1 : 0, c->d_stripes.as<uint64_t>(), 2 * PHI_STRIPES * 8);
        HIPCHK(hipGetLastError());
    }
    c->spset.new_generation();
    if (!c->rlog.next_flag_zeroed) HIPCHK(hipMemsetAsync(scalar(c, S_OVCNT + (int)(c->spset.sp_gen % 3)), 0, 8, c->stream));   // the new generation's overflow counter
    c->rlog.new_generation();
    c->reads_bases = 0; c->reads_count = 0; c->spectrum_override = -1;
    c->solved = false;
    c->ladder.scored = 0;                                      // (phi_ladder_advance starts over; the plan stays)
    return PHI_OK;
}

int phi_reads_stats(phi_ctx *c, int64_t *n_reads, int64_t *n_bases, int64_t *n_emitted, int64_t *n_distinct)
{
    if (!c) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_reads_stats before phi_set_graph");
    HIPCHK(hipSetDevice(c->device));
    PHICHK(phi_sync_check(c));
    uint64_t nd = 0, ne = 0;
    PHICHK(phi_read_counts(c, nullptr, &ne));
    PHICHK(phi_spectrum_count(c, &nd));
    if (n_reads) *n_reads = c->reads_count;
    if (n_bases) *n_bases = c->reads_bases;
    if (n_emitted) *n_emitted = (int64_t)ne;
    if (n_distinct) *n_distinct = (int64_t)nd;
    return PHI_OK;
}

int phi_hits_buffer(phi_ctx *c, void **d_hits, int64_t *n)
{
    if (!c || !d_hits || !n) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_hits_buffer before phi_set_graph");
    HIPCHK(hipSetDevice(c->device));
    PHICHK(phi_flush_reset(c));
    *d_hits = c->d_hit.p;
    *n = c->n_unique;
    return PHI_OK;
}

int phi_read_table(phi_ctx *c, void **d_table, int64_t *n_buckets)
{
    if (!c || !d_table || !n_buckets) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_read_table before phi_set_graph");
    *d_table = c->d_rt.p;
    *n_buckets = (int64_t)c->rt_buckets;
    return PHI_OK;
}

int phi_spectrum_export(phi_ctx *c, void **d_hashes, int64_t *n)
{
    if (!c || !d_hashes || !n) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_spectrum_export before phi_set_graph");
    HIPCHK(hipSetDevice(c->device));
    *d_hashes = nullptr; *n = 0;
    uint64_t cnt = 0;
    PHICHK(phi_sp_flush(c, &cnt));                            // waits for the stream
    PHICHK(phi_dev_ensure(c, c->spset.d_export, (size_t)std::max<uint64_t>(cnt, 1) * 8));      // (an empty list still has an address)
    if (cnt) {
        HIPCHK(hipMemsetAsync(scalar(c, S_EXPORT), 0, 8, c->stream));
        phi_launch_spectrum_export(c->stream, c->spset.d_sp_keys.as<uint64_t>(), (int64_t)c->spset.sp_cap, c->spset.d_export.as<uint64_t>(),
                                   (unsigned long long *)scalar(c, S_EXPORT));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    *d_hashes = c->spset.d_export.p;
    *n = (int64_t)cnt;
    return PHI_OK;
}

int phi_spectrum_import(phi_ctx *c, const void *d_hashes, int64_t n)
{
    if (!c || n < 0 || (n > 0 && !d_hashes)) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_spectrum_import before phi_set_graph");
    if (n == 0) return PHI_OK;
    HIPCHK(hipSetDevice(c->device));
    if (d_hashes == c->spset.d_export.p) return phi_fail(c, PHI_ERR_INVALID, "phi_spectrum_import: pass a copy, not the export buffer");
    uint64_t in_set = 0;
    PHICHK(phi_sp_flush(c, &in_set));                         // the set made current first: what is imported goes straight into it
    PHICHK(sp_reserve(c, in_set, (uint64_t)n));
    phi_launch_spectrum_insert(c->stream, (const uint64_t *)d_hashes, n, c->spset.d_sp_keys.as<uint64_t>(), c->spset.sp_cap - 1,
                               c->spset.d_sp_cnt.as<unsigned long long>(), c->d_u_keys.as<uint64_t>(), c->u_cap - 1, c->d_u_uid.as<uint32_t>(),
                               c->d_hit.as<uint8_t>(), (uint32_t *)scalar(c, S_ERR));
    HIPCHK(hipGetLastError());
    c->solved = false;
    return PHI_OK;
}

int phi_spectrum_set_size(phi_ctx *c, int64_t global_size)
{
    if (!c || global_size < 0) return PHI_ERR_INVALID;
    c->spectrum_override = global_size;
    return PHI_OK;
}

}  // extern "C"
