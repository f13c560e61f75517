// phi_abi.hip -- C ABI of include/phi_amd.h: errors, the context, the solve's entry, the stand-alone sketch and the statistics
// and anchor accessors.  (Device memory and its pool: dev_mem.hip; read batches: read_batches.hip; reads as text:
// text_stream.hip, text_park.hip; phi_set_graph: set_graph.hip; the chopped and the VCF routes: chop.hip, vcf.hip, each beside
// its kernels.)  Host-side orchestration only; all per-base work runs in the kernels of sketch.hip, table.hip,
// anchors.hip and dp.hip.  There is no CPU fallback: without a HIP device every entry point
// that needs one returns PHI_ERR_DEVICE.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <future>
#include "phi_ctx.h"
#include "phi_dev.h"

int phi_fail(phi_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) {
        std::lock_guard<std::mutex> g(c->err_mu);            // phi_set_graph runs a GPU thread beside the caller's: both may fail
        c->last_error = buf;
    }
    return code;
}

int phi_hip_check(phi_ctx *c, hipError_t e, const char *what)
{
    if (e == hipSuccess) return PHI_OK;
    const int code = (e == hipErrorOutOfMemory) ? PHI_ERR_NOMEM : PHI_ERR_DEVICE;
    return phi_fail(c, code, "%s: %s", what, hipGetErrorString(e));
}

extern "C" {

const char *phi_strerror(int status)
{
    switch (status) {
    case PHI_OK: return "ok";
    case PHI_ERR_INVALID: return "invalid argument";
    case PHI_ERR_NOMEM: return "out of memory";
    case PHI_ERR_DEVICE: return "HIP device error";
    case PHI_ERR_STATE: return "call order violated";
    case PHI_ERR_UNSUPPORTED: return "unsupported input";
    case PHI_ERR_WALK: return "walk does not follow the graph";
    case PHI_ERR_OVERFLOW: return "internal table overflow";
    default: return "unknown status";
    }
}

const char *phi_last_error(const phi_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int phi_ctx_create(int device_id, phi_ctx **out)
{
    if (!out) return PHI_ERR_INVALID;
    *out = nullptr;
    PhiStageTimer tm("ctx_create");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return PHI_ERR_DEVICE;
    tm.lap("runtime start (hipInit)");
    if (device_id < 0 || device_id >= n_dev) return PHI_ERR_INVALID;
    if (hipSetDevice(device_id) != hipSuccess) return PHI_ERR_DEVICE;
    phi_ctx *c = new (std::nothrow) phi_ctx();
    if (!c) return PHI_ERR_NOMEM;
    c->device = device_id;
    // What a context costs is the runtime's one-time work, all of it latency: a stream is a hardware queue (~20 ms each),
    // the kernels' code objects load at the first launch of their translation unit (~13 ms), and the first host copies of
    // every kind -- large through the copy engines' staging buffers, small through the runtime's own copy kernels -- set up
    // what they go through (~20 ms).  Two threads: this one makes the context's stream and loads the code objects, the other
    // makes the second stream (the host thread's copies inside phi_set_graph) and warms the copy paths on it.  Nothing
    // touches the null stream, whose queue would cost as much again (phi_copy_sync / phi_memset_sync in phi_ctx.h).
    std::future<hipError_t> aux = std::async(std::launch::async, [c, device_id]() {
        hipError_t e = hipSetDevice(device_id);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
        void *d = nullptr;
        std::vector<char> h((size_t)1 << 20, 0);
        if (hipMalloc(&d, h.size()) == hipSuccess) {
            (void)phi_dev_poison(d, h.size());
            (void)hipMemcpyAsync(d, h.data(), h.size(), hipMemcpyHostToDevice, c->aux_stream);
            (void)hipMemcpyAsync(h.data(), d, h.size(), hipMemcpyDeviceToHost, c->aux_stream);
            (void)hipMemcpyAsync(d, h.data(), 64, hipMemcpyHostToDevice, c->aux_stream);
            (void)hipMemcpyAsync(h.data(), d, 64, hipMemcpyDeviceToHost, c->aux_stream);
            (void)hipMemsetAsync(d, 0, 4096, c->aux_stream);
            (void)hipStreamSynchronize(c->aux_stream);
            (void)hipFree(d);
        }
        return hipSuccess;
    });
    auto bail = [&](int code) {
        if (aux.valid()) (void)aux.get();
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
        if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
        phi_dev_free(c->d_scalars); phi_dev_free(c->d_stripes); phi_dev_free(c->alt.stripes);
        delete c;
        return code;
    };
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) return bail(PHI_ERR_DEVICE);
    c->stream = c->own_stream;
    tm.lap("stream");
    if (phi_dev_ensure(c, c->d_scalars, S_N * 8) || hipMemsetAsync(c->d_scalars.p, 0, S_N * 8, c->stream) != hipSuccess ||
        phi_dev_ensure(c, c->d_stripes, 2 * STRIPE_BYTES) || hipMemsetAsync(c->d_stripes.p, 0, 2 * STRIPE_BYTES, c->stream) != hipSuccess ||
        phi_dev_ensure(c, c->alt.stripes, 2 * STRIPE_BYTES) || hipMemsetAsync(c->alt.stripes.p, 0, 2 * STRIPE_BYTES, c->stream) != hipSuccess)
        return bail(PHI_ERR_DEVICE);
    // the kernels' code objects are loaded lazily, per translation unit, at their first launch: do that here, once
    if (tm.on && getenv("PHI_TIMING_UNITS")) {
        // (diagnostics: what each unit's code object costs to load)
        (void)hipStreamSynchronize(c->stream); tm.lap("  scalars");
        phi_warm_sketch(c->stream); (void)hipStreamSynchronize(c->stream); tm.lap("  code object: sketch");
        phi_warm_table(c->stream); (void)hipStreamSynchronize(c->stream); tm.lap("  code object: table");
        phi_warm_anchors(c->stream); (void)hipStreamSynchronize(c->stream); tm.lap("  code object: anchors");
        phi_warm_contexts(c->stream); (void)hipStreamSynchronize(c->stream); tm.lap("  code object: contexts");
        phi_warm_dp(c->stream); (void)hipStreamSynchronize(c->stream); tm.lap("  code object: dp");
        phi_warm_dp_events(c->stream); (void)hipStreamSynchronize(c->stream); tm.lap("  code object: dp_events");
        phi_warm_dp_blocks(c->stream); (void)hipStreamSynchronize(c->stream); tm.lap("  code object: dp_blocks");
        phi_warm_solve_dev(c->stream); (void)hipStreamSynchronize(c->stream); tm.lap("  code object: solve_dev");
        phi_warm_reads_text(c->stream); (void)hipStreamSynchronize(c->stream); tm.lap("  code object: reads_text");
        phi_warm_scan(c->stream); (void)hipStreamSynchronize(c->stream); tm.lap("  code object: scan");
    }
    phi_warm_sketch(c->stream); phi_warm_table(c->stream); phi_warm_anchors(c->stream); phi_warm_contexts(c->stream);
    phi_warm_dp(c->stream); phi_warm_dp_events(c->stream); phi_warm_dp_blocks(c->stream); phi_warm_solve_dev(c->stream); phi_warm_reads_text(c->stream);
    phi_warm_walk_text(c->stream); phi_warm_scan(c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return bail(PHI_ERR_DEVICE);
    tm.lap("scalars + code objects");
    if (aux.get() != hipSuccess) { c->aux_stream = nullptr; return bail(PHI_ERR_DEVICE); }
    c->last_error.clear();
    tm.lap("wait for the second stream + first host copies");
    *out = c;
    return PHI_OK;
}

void phi_ctx_destroy(phi_ctx *c)
{
    if (c && c->pin_future.valid()) c->pin_future.wait();
    if (c && c->dp_alloc_future.valid()) (void)c->dp_alloc_future.get();
    if (c && c->h_pin) { (void)hipSetDevice(c->device); (void)hipHostFree(c->h_pin); c->h_pin = nullptr; }
    if (c) { (void)hipSetDevice(c->device); stage_release(c); }
    if (!c) return;
    (void)phi_comm_destroy(c);
    (void)phi_ipc_destroy(c);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    phi_ladder_drop(c);
    DevBuf *all[] = {&c->d_anchors, &c->d_cov_all, &c->d_cov_w, &c->d_slots, &c->d_slots2, &c->d_segs, &c->d_ctr, &c->d_vmax, &c->d_lane_walk, &c->d_walk_lane, &c->d_coff, &c->d_blk_ncls, &c->d_rownew, &c->d_blk_bad, &c->d_seg_lo, &c->d_seg_row, &c->d_seg_S, &c->wtext.d_text, &c->panel.d_full, &c->scout.d_scores, &c->d_sel_off, &c->d_sel_tri, &c->d_blk_lo, &c->d_blk_ev, &c->d_blk_S, &c->d_row_out, &c->d_rowend, &c->d_blk_keys, &c->d_blk_carry, &c->d_cov, &c->d_cov2, &c->d_stepdiff, &c->alt.hit, &c->hit_extra[0], &c->hit_extra[1], &c->alt.stripes, &c->spset.d_sp_cnt, &c->rlog.d_novlog, &c->rlog.d_novcnt, &c->rlog.d_ovlist, &c->d_vlen, &c->d_ent_cls, &c->d_cls_rep, &c->d_cls_left, &c->d_cls_mult, &c->d_cls_base, &c->d_cls_rec_off, &c->d_rec_cls, &c->d_rec_rel, &c->d_u_replist, &c->d_adj_off, &c->d_adj, &c->d_topo_rank, &c->d_cnt_edge, &c->d_walk_err, &c->d_sa_cnt, &c->d_sa_cur, &c->d_sa_off, &c->d_sa_idx, &c->d_seq, &c->d_seq_off, &c->d_walk_vtx, &c->d_walk_off, &c->d_topo, &c->d_in_off,
                     &c->d_in_src, &c->d_e_out, &c->d_st_rec, &c->d_st_mask, &c->d_in_packed, &c->d_word, &c->d_wwords, &c->d_wbad,
                     &c->d_wascii, &c->d_wstarts, &c->d_rec_hash, &c->d_rec_pos, &c->d_rec_slot,
                     &c->d_rec_e0, &c->d_rec_e1, &c->d_u_keys, &c->d_u_rep, &c->d_u_uid, &c->d_rt, &c->d_kt, &c->d_in_s, &c->d_last_walk, &c->d_rowdiag, &c->d_wpre, &c->d_hit, &c->spset.d_sp_keys, &c->d_rbases,
                     &c->d_roff, &c->rlog.d_roff_made, &c->d_peer_send, &c->spset.d_export, &c->d_scalars, &c->d_stripes, &c->d_blk_cnt,
                     &c->d_blk_off, &c->d_flags, &c->d_flags2, &c->d_list, &c->d_list2, &c->d_list3, &c->d_walk_last, &c->d_m_rec, &c->d_m_group,
                     &c->d_g_keys, &c->d_g_rep, &c->d_g_cnt, &c->d_slot_maxcnt, &c->d_slot_multi, &c->d_a_e1,
                     &c->d_g_off, &c->d_g_span, &c->d_a_weight, &c->d_dmax, &c->d_bstart, &c->d_k_rec, &c->d_k_in, &c->d_cvtx, &c->d_ev_e, &c->d_ev_off, &c->d_ev,
                     &c->d_off_end, &c->d_off_start, &c->d_scan_blk, &c->d_scan_blk64, &c->d_scan_blkoff, &c->d_top,
                     &c->d_ent, &c->calls.d_r_base, &c->calls.d_q_base, &c->calls.d_anchor, &c->calls.d_ref_src, &c->calls.d_alt_src};
    phi_pool_flush(c->device);
    phi_pool_bypass(true);                                 // (a context that goes gives its memory back to the driver)
    struct Bypass { ~Bypass() { phi_pool_bypass(false); } } bypass_guard;
    for (DevBuf *b : all) phi_dev_free(*b);
    for (auto &pr : c->prof_events) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    if (c->h_err) (void)hipHostFree(c->h_err);
    {
        auto &T = c->text;
        for (int i = 0; i < 2; i++) { phi_dev_free(T.text[i]); phi_dev_free(T.bases[i]); phi_dev_free(T.roff[i]); }
        phi_dev_free(T.tile_cnt); phi_dev_free(T.ls); phi_dev_free(T.pre); phi_dev_free(T.blk); phi_dev_free(T.sum);
        if (T.h_sum) (void)hipHostFree(T.h_sum);
        if (T.ev_copy) (void)hipEventDestroy(T.ev_copy);
    }
    phi_bam_drop(c);
    (void)hipStreamDestroy(c->own_stream);
    (void)hipStreamDestroy(c->aux_stream);
    delete c;
}

int phi_set_stream(phi_ctx *c, void *hip_stream)
{
    if (!c) return PHI_ERR_INVALID;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return PHI_OK;
}

int phi_set_params(phi_ctx *c, int32_t k, int32_t w, float threshold, int32_t recombination, uint32_t flags)
{
    if (!c) return PHI_ERR_INVALID;
    if (c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_set_params must precede phi_set_graph");
    if (k < 1 || k > PHI_MAX_K) return phi_fail(c, PHI_ERR_INVALID, "k=%d outside [1,%d]", k, PHI_MAX_K);
    if (w < 1 || w > PHI_MAX_W) return phi_fail(c, PHI_ERR_INVALID, "w=%d outside [1,%d]", w, PHI_MAX_W);
    if (recombination < 0) return phi_fail(c, PHI_ERR_INVALID, "recombination penalty must be >= 0");
    c->k = k; c->w = w; c->threshold = threshold; c->recombination = recombination; c->flags = flags;
    return PHI_OK;
}

}  // extern "C" (helpers below are C++)

// count pass -> scan -> ordered write of the minimiser records of one packed flat sequence
int sketch_records(phi_ctx *c, const uint64_t *words, const unsigned long long *starts, int64_t n_bases,
                   int32_t k, int32_t w, const uint8_t *ascii_if_bad, DevBuf &out_hash, DevBuf &out_pos,
                   int64_t *n_out)
{
    *n_out = 0;
    const int64_t nb = phi_sketch_num_blocks(n_bases);
    if (nb == 0) return PHI_OK;
    PHICHK(phi_dev_ensure(c, c->d_blk_cnt, (size_t)nb * 4));
    PHICHK(phi_dev_ensure(c, c->d_blk_off, (size_t)(nb + 1) * 8));
    PhiSketchArgs A{};
    A.words = words; A.starts = starts; A.n_bases = n_bases; A.k = k; A.w = w;
    // sequences with bases outside ACGT take the exact byte-wise path for every window, so that the
    // ordered write stays in position order
    A.ascii = ascii_if_bad; A.allslow = ascii_if_bad ? 1 : 0; A.badbits = nullptr;
    A.block_cnt = c->d_blk_cnt.as<int32_t>();
    A.err = (uint32_t *)scalar(c, S_ERR);
    if (A.allslow) phi_launch_sketch_bytes(c->stream, PHI_MODE_COUNT, A, nullptr);
    else phi_launch_sketch(c->stream, PHI_MODE_COUNT, A);
    PHICHK(phi_scan(c, c->d_blk_cnt.as<int32_t>(), nb, c->d_blk_off.as<int64_t>()));
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, c->d_blk_off.as<int64_t>() + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    PHICHK(phi_dev_ensure(c, out_hash, (size_t)std::max<int64_t>(total, 1) * 8));
    PHICHK(phi_dev_ensure(c, out_pos, (size_t)std::max<int64_t>(total, 1) * 8));
    A.block_off = c->d_blk_off.as<int64_t>();
    A.out_hash = out_hash.as<uint64_t>();
    A.out_pos = out_pos.as<int64_t>();
    if (A.allslow) phi_launch_sketch_bytes(c->stream, PHI_MODE_WRITE, A, nullptr);
    else phi_launch_sketch(c->stream, PHI_MODE_WRITE, A);
    HIPCHK(hipGetLastError());
    *n_out = total;
    return PHI_OK;
}

extern "C" {

int phi_set_solve_budget(phi_ctx *c, int64_t max_dp_runs)
{
    if (!c) return PHI_ERR_INVALID;
    c->solve_budget = max_dp_runs > 0x7FFFFFFF ? 0x7FFFFFFF : max_dp_runs;
    c->solved = false;
    return PHI_OK;
}

int phi_solve(phi_ctx *c, phi_result *out)
{
    if (!c || !out) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_solve before phi_set_graph");
    PHICHK(phi_refuse_scout(c, "phi_solve"));
    HIPCHK(hipSetDevice(c->device));
    const int rc = phi_solve_impl(c);
    phi_pool_flush(c->device);                              // (what the index build and this solve let go and nobody took again)
    if (rc) return rc;
    *out = c->result;
    return PHI_OK;
}

int phi_path_sequence(phi_ctx *c, char *buf, int64_t cap)
{
    if (!c || (!buf && cap > 0)) return PHI_ERR_INVALID;
    PHICHK(phi_refuse_scout(c, "phi_path_sequence"));
    if (!c->solved) return phi_fail(c, PHI_ERR_STATE, "phi_path_sequence before phi_solve");
    if (cap < c->result.hap_len) return phi_fail(c, PHI_ERR_INVALID, "buffer too small: need %lld bytes", (long long)c->result.hap_len);
    // (where every vertex of the path lands, then the copies by all host threads: 5.8 M vertices and 176 MB at chromosome scale)
    const int64_t np = (int64_t)c->h_path_vtx.size();
    std::vector<int64_t> at((size_t)np + 1, 0);
    for (int64_t i = 0; i < np; i++) { const int32_t v = c->h_path_vtx[(size_t)i]; at[(size_t)i + 1] = at[(size_t)i] + (c->h_seq_off[v + 1] - c->h_seq_off[v]); }
    phi_parallel_chunks(np, 1 << 15, [&](int64_t lo, int64_t hi, int) {
        for (int64_t i = lo; i < hi; i++) {
            const int32_t v = c->h_path_vtx[(size_t)i];
            memcpy(buf + at[(size_t)i], c->h_seq.data() + c->h_seq_off[v], (size_t)(at[(size_t)i + 1] - at[(size_t)i]));      // original case, :1580
        }
    });
    return PHI_OK;
}

int phi_sketch(phi_ctx *c, const char *bases, const int64_t *seq_off, int64_t n_seq, int32_t k, int32_t w,
               uint64_t *out_hash, int64_t *out_pos, int32_t *out_seq, int64_t cap, int64_t *n_out)
{
    if (!c || !n_out || n_seq < 0 || (n_seq > 0 && !seq_off)) return PHI_ERR_INVALID;
    if (k < 1 || k > PHI_MAX_K || w < 1 || w > PHI_MAX_W) return phi_fail(c, PHI_ERR_INVALID, "k or w out of range");
    *n_out = 0;
    if (n_seq == 0) return PHI_OK;
    for (int64_t r = 0; r < n_seq; r++)
        if (seq_off[r + 1] < seq_off[r]) return phi_fail(c, PHI_ERR_INVALID, "seq_off not monotone");
    const int64_t n_bases = seq_off[n_seq] - seq_off[0];
    if (n_bases == 0) return PHI_OK;
    if (!bases) return PHI_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    DevBuf dB, dO, dW, dS, dH, dP;
    int rc = PHI_OK;
    std::vector<int64_t> off(seq_off, seq_off + n_seq + 1);
    for (auto &o : off) o -= seq_off[0];
    do {
        if ((rc = phi_dev_ensure(c, dB, (size_t)n_bases + 64))) break;
        if ((rc = phi_dev_ensure(c, dO, (size_t)(n_seq + 1) * 8))) break;
        const int64_t n_words = (n_bases + 31) / 32;
        if ((rc = phi_dev_ensure(c, dW, (size_t)(n_words + 2) * 8))) break;
        const size_t n_sw = (size_t)(n_bases / 64 + 2);
        if ((rc = phi_dev_ensure(c, dS, n_sw * 8))) break;
        if ((rc = phi_hip_check(c, hipMemcpyAsync(dB.p, bases + seq_off[0], (size_t)n_bases, hipMemcpyHostToDevice, c->stream), "H2D bases"))) break;
        if ((rc = phi_hip_check(c, hipMemcpyAsync(dO.p, off.data(), (size_t)(n_seq + 1) * 8, hipMemcpyHostToDevice, c->stream), "H2D offsets"))) break;
        if ((rc = phi_hip_check(c, hipMemsetAsync(dW.as<uint64_t>() + n_words, 0, 16, c->stream), "memset"))) break;
        if ((rc = phi_hip_check(c, hipMemsetAsync(dS.p, 0, n_sw * 8, c->stream), "memset"))) break;
        if ((rc = phi_hip_check(c, hipMemsetAsync(scalar(c, S_NBAD), 0, 8, c->stream), "memset"))) break;
        phi_launch_mark_starts(c->stream, dO.as<int64_t>(), n_seq, dS.as<unsigned long long>());
        phi_launch_pack_ascii(c->stream, dB.as<uint8_t>(), n_bases, dW.as<uint64_t>(), n_words, nullptr,
                              (unsigned long long *)scalar(c, S_NBAD));
        if ((rc = phi_hip_check(c, hipStreamSynchronize(c->stream), "sync"))) break;
        uint64_t n_bad = 0;
        if ((rc = phi_hip_check(c, phi_copy_sync(c, &n_bad, scalar(c, S_NBAD), 8, hipMemcpyDeviceToHost), "D2H"))) break;
        int64_t total = 0;
        if ((rc = sketch_records(c, dW.as<uint64_t>(), dS.as<unsigned long long>(), n_bases, k, w,
                                 (n_bad || k > PHI_MAX_K_PACKED) ? dB.as<uint8_t>() : nullptr, dH, dP, &total))) break;
        if ((rc = phi_sync_check(c))) break;
        *n_out = total;
        if (cap >= total && total > 0) {
            std::vector<int64_t> gpos((size_t)total);
            if (out_hash && (rc = phi_hip_check(c, phi_copy_sync(c, out_hash, dH.p, (size_t)total * 8, hipMemcpyDeviceToHost), "D2H hash"))) break;
            if ((rc = phi_hip_check(c, phi_copy_sync(c, gpos.data(), dP.p, (size_t)total * 8, hipMemcpyDeviceToHost), "D2H pos"))) break;
            int64_t s = 0;
            for (int64_t i = 0; i < total; i++) {
                while (off[s + 1] <= gpos[i]) s++;
                if (out_pos) out_pos[i] = gpos[i] - off[s];
                if (out_seq) out_seq[i] = (int32_t)s;
            }
        }
    } while (0);
    phi_dev_free(dB); phi_dev_free(dO); phi_dev_free(dW); phi_dev_free(dS); phi_dev_free(dH); phi_dev_free(dP);
    // a failed stand-alone sketch must not poison later calls on this context
    (void)phi_memset_sync(c, c->d_scalars.p, 0, 16);
    return rc;
}

int phi_walk_minimizers(phi_ctx *c, int32_t walk, uint64_t *out_hash, int64_t *out_pos, int64_t cap, int64_t *n_out)
{
    if (!c || !n_out) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_walk_minimizers before phi_set_graph");
    if (walk < 0 || walk >= c->n_walks) return phi_fail(c, PHI_ERR_INVALID, "walk out of range");
    HIPCHK(hipSetDevice(c->device));
    const int64_t n = c->h_n_minimizers[walk];
    *n_out = n;
    if (cap < n || n == 0) return PHI_OK;
    // the records of a walk are never stored: expand the classes of its entries, in entry order
    const int64_t e_lo = c->h_walk_off[walk], e_hi = c->h_walk_off[walk + 1], ne = e_hi - e_lo;
    DevBuf lens, base, oh, op;
    struct Guard { DevBuf &a, &b, &d, &e; ~Guard() { phi_dev_free(a); phi_dev_free(b); phi_dev_free(d); phi_dev_free(e); } } guard{lens, base, oh, op};
    PHICHK(phi_dev_ensure(c, lens, (size_t)ne * 4));
    PHICHK(phi_dev_ensure(c, base, (size_t)(ne + 1) * 8));
    PHICHK(phi_dev_ensure(c, oh, (size_t)n * 8));
    PHICHK(phi_dev_ensure(c, op, (size_t)n * 8));
    phi_launch_entry_len_range(c->stream, c->d_walk_vtx.as<int32_t>(), c->d_vlen.as<int32_t>(), e_lo, ne, lens.as<int32_t>());
    PHICHK(phi_scan(c, lens.as<int32_t>(), ne, base.as<int64_t>()));
    PhiExpandArgs X{};
    X.ent_cls = c->d_ent_cls.as<int32_t>(); X.e_lo = e_lo; X.e_hi = e_hi;
    X.cls_rec_off = c->d_cls_rec_off.as<int32_t>(); X.cls_rep = c->d_cls_rep.as<phi_ent_t>();
    X.rec_hash = c->d_rec_hash.as<uint64_t>(); X.rec_rel = c->d_rec_rel.as<int32_t>(); X.ent_base = base.as<int64_t>();
    X.out_hash = oh.as<uint64_t>(); X.out_pos = op.as<int64_t>();
    const int64_t nb = phi_expand_num_blocks(ne);
    PHICHK(phi_dev_ensure(c, c->d_blk_cnt, (size_t)nb * 4));
    PHICHK(phi_dev_ensure(c, c->d_blk_off, (size_t)(nb + 1) * 8));
    X.block_cnt = c->d_blk_cnt.as<int32_t>(); X.block_off = c->d_blk_off.as<int64_t>();
    phi_launch_expand_count(c->stream, X);
    PHICHK(phi_scan(c, c->d_blk_cnt.as<int32_t>(), nb, c->d_blk_off.as<int64_t>()));
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, c->d_blk_off.as<int64_t>() + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (total != n) return phi_fail(c, PHI_ERR_DEVICE, "walk %d expands to %lld records, counted %lld (internal error)", walk, (long long)total, (long long)n);
    phi_launch_expand_write(c->stream, X, 0);
    HIPCHK(hipGetLastError());
    if (out_hash) HIPCHK(hipMemcpyAsync(out_hash, oh.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    if (out_pos) HIPCHK(hipMemcpyAsync(out_pos, op.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PHI_OK;
}

int phi_index_stats(phi_ctx *c, phi_index_info *out)
{
    if (!c || !out) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_index_stats before phi_set_graph");
    out->n_entries = c->n_entries; out->walk_bases = c->walk_bases;
    out->n_classes = c->n_cls; out->class_bases = c->cls_bases; out->n_class_records = c->n_rec;
    out->n_walk_minimizers = 0;
    for (int64_t m : c->h_n_minimizers) out->n_walk_minimizers += m;
    out->n_distinct_minimizers = c->n_unique;
    out->sketch_gpu_ms = c->index_gpu_ms;
    return PHI_OK;
}

int phi_solve_stats(phi_ctx *c, phi_solve_info *out)
{
    if (!c || !out) return PHI_ERR_INVALID;
    PHICHK(phi_refuse_scout(c, "phi_solve_stats"));
    if (!c->solved) return phi_fail(c, PHI_ERR_STATE, "phi_solve_stats before phi_solve");
    memset(out, 0, sizeof *out);
    out->n_dp_anchors = c->n_dp;
    out->n_events = c->dp_events ? c->n_ev : c->n_entries;
    out->n_steps = c->dp_events ? c->n_k : c->n_vtx;
    out->dp_mode = !c->dp_events ? 0 : !c->dp_blocks ? 1 : c->dp_cls ? 3 : 2;
    out->n_blocks = c->dp_events && c->dp_blocks ? c->n_blk : 0;
    if (out->dp_mode == 3 && c->n_blk > 0) {
        HIPCHK(hipSetDevice(c->device));
        std::vector<int32_t> n((size_t)c->n_blk);
        HIPCHK(phi_copy_sync(c, n.data(), c->d_blk_ncls.p, n.size() * 4, hipMemcpyDeviceToHost));
        int64_t sum = 0;
        for (int32_t v : n) { sum += v; out->max_classes = std::max(out->max_classes, v); }
        out->mean_classes = (double)sum / (double)n.size();
    }
    return PHI_OK;
}

int phi_dp_probe(phi_ctx *c, const uint8_t *weights, int64_t n_weights, int32_t *out_ends, int64_t *out_value, int32_t *out_end_walk,
                 int32_t *out_seg_walk, int64_t *out_seg_first, int64_t *out_seg_last, int64_t seg_cap, int64_t *n_seg, phi_dp_probe_info *info)
{
    if (!c || !out_ends || !out_value || !out_end_walk || !n_seg || !info) return PHI_ERR_INVALID;
    if (seg_cap > 0 && (!out_seg_walk || !out_seg_first || !out_seg_last)) return PHI_ERR_INVALID;
    PHICHK(phi_refuse_scout(c, "phi_dp_probe"));
    if (!c->solved) return phi_fail(c, PHI_ERR_STATE, "phi_dp_probe before phi_solve");
    if (weights) {
        if (n_weights != c->n_dp) return phi_fail(c, PHI_ERR_INVALID, "phi_dp_probe: %lld weights for %lld dp anchors", (long long)n_weights, (long long)c->n_dp);
        for (int64_t a = 0; a < n_weights; a++)
            if (weights[a] > 1) return phi_fail(c, PHI_ERR_INVALID, "phi_dp_probe: weight %lld is %d, not 0 or 1", (long long)a, (int)weights[a]);
    }
    HIPCHK(hipSetDevice(c->device));
    memset(info, 0, sizeof *info);
    PHICHK(phi_dp_probe_impl(c, weights, out_ends, out_value, out_end_walk, out_seg_walk, out_seg_first, out_seg_last, seg_cap, n_seg, &info->retries));
    phi_solve_info st;
    PHICHK(phi_solve_stats(c, &st));                             // (the strategy as the run left it: the attempt that finished)
    info->dp_mode = st.dp_mode; info->n_blocks = st.n_blocks; info->max_classes = st.max_classes;
    if (st.dp_mode >= 2) { info->blk_ring = c->blk_ring; info->blk_max_len = c->blk_max_len; }
    info->retries_since_solve = c->dp_retries;
    return PHI_OK;
}

int phi_walk_sharing(phi_ctx *c, int64_t *hist, int32_t cap, int64_t *n_distinct)
{
    if (!c || !hist) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_walk_sharing before phi_set_graph");
    if (cap < c->n_walks + 1) return phi_fail(c, PHI_ERR_INVALID, "phi_walk_sharing: hist needs n_walks + 1 entries");
    HIPCHK(hipSetDevice(c->device));
    DevBuf last, cnt, dh;
    int rc = PHI_OK;
    do {
        if ((rc = phi_dev_ensure(c, last, c->u_cap * 4))) break;
        if ((rc = phi_dev_ensure(c, cnt, c->u_cap * 4))) break;
        if ((rc = phi_dev_ensure(c, dh, (size_t)(c->n_walks + 1) * 8))) break;
        phi_launch_fill_u32(c->stream, last.as<uint32_t>(), (int64_t)c->u_cap, 0xFFFFFFFFu);
        if ((rc = phi_hip_check(c, hipMemsetAsync(cnt.p, 0, c->u_cap * 4, c->stream), "memset"))) break;
        if ((rc = phi_hip_check(c, hipMemsetAsync(dh.p, 0, (size_t)(c->n_walks + 1) * 8, c->stream), "memset"))) break;
        for (int32_t h = 0; h < c->n_walks; h++)
            phi_launch_share_count_cls(c->stream, c->d_ent_cls.as<int32_t>(), c->h_walk_off[h], c->h_walk_off[h + 1], c->d_cls_rec_off.as<int32_t>(),
                                       c->d_rec_slot.as<uint32_t>(), h, last.as<int32_t>(), cnt.as<int32_t>());
        phi_launch_share_hist(c->stream, c->d_u_keys.as<uint64_t>(), (int64_t)c->u_cap, cnt.as<int32_t>(),
                              dh.as<unsigned long long>());
        if ((rc = phi_hip_check(c, hipGetLastError(), "launch"))) break;
        if ((rc = phi_hip_check(c, hipStreamSynchronize(c->stream), "synchronize"))) break;
        std::vector<unsigned long long> hh(c->n_walks + 1);
        if ((rc = phi_hip_check(c, phi_copy_sync(c, hh.data(), dh.p, hh.size() * 8, hipMemcpyDeviceToHost), "D2H"))) break;
        for (int32_t i = 0; i <= c->n_walks; i++) hist[i] = (int64_t)hh[i];
        if (n_distinct) *n_distinct = c->n_unique;
    } while (0);
    phi_dev_free(last); phi_dev_free(cnt); phi_dev_free(dh);
    return rc;
}

int phi_kept_anchors(phi_ctx *c, uint64_t *out_hash, int32_t *out_walk, int32_t *out_t0, int32_t *out_t1, int64_t cap,
                     int64_t *n_out)
{
    if (!c || !n_out) return PHI_ERR_INVALID;
    PHICHK(phi_refuse_scout(c, "phi_kept_anchors"));
    if (!c->solved) return phi_fail(c, PHI_ERR_STATE, "phi_kept_anchors before phi_solve");
    const int64_t n = c->n_kept;
    if (cap >= n) PHICHK(phi_host_anchors(c));                 // (a large model is solved on the device copy alone)
    *n_out = n;
    if (cap < n) return PHI_OK;
    if (out_hash && n && (int64_t)c->h_kept_hash.size() != n) {
        // the hashes stayed on the device (phi_solve does not need them): fetch them now
        HIPCHK(hipSetDevice(c->device));
        c->h_kept_hash.resize(n);
        // hash of a dense minimiser id = hash of its first class record
        std::vector<uint64_t> id_hash((size_t)c->n_unique);
        PHICHK(phi_dev_ensure(c, c->d_list2, (size_t)std::max<int64_t>(c->n_unique, 1) * 8));
        phi_launch_gather_u64(c->stream, c->d_rec_hash.as<uint64_t>(), c->d_u_replist.as<int32_t>(), c->n_unique, c->d_list2.as<uint64_t>());
        HIPCHK(hipMemcpyAsync(id_hash.data(), c->d_list2.p, (size_t)c->n_unique * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int64_t i = 0; i < n; i++) c->h_kept_hash[i] = id_hash[c->h_kept[i].slot];
    }
    for (int64_t i = 0; i < n; i++) {
        const PhiAnchorHost &a = c->h_kept[i];
        const int32_t h = phi_entry_walk(c, a.e0);
        if (out_hash) out_hash[i] = c->h_kept_hash[i];
        if (out_walk) out_walk[i] = h;
        if (out_t0) out_t0[i] = (int32_t)((int64_t)a.e0 - c->h_walk_off[h]);
        if (out_t1) out_t1[i] = (int32_t)((int64_t)a.e1 - c->h_walk_off[h]);
    }
    return PHI_OK;
}

int phi_device_synchronize(phi_ctx *c)
{
    if (!c) return PHI_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipGetLastError());
    return PHI_OK;
}

int phi_prof_enable(phi_ctx *c, int on)
{
    if (!c) return PHI_ERR_INVALID;
    c->prof = on != 0;
    c->prof_period = on > 0 ? on : 1;                   // on = n: every n-th sketch launch is bracketed
    c->prof_seq = 0;
    if (c->prof) {
        // create the event pairs of the next launches now, not inside the region being timed
        HIPCHK(hipSetDevice(c->device));
        while (c->prof_events.size() < c->prof_used + 256) {
            hipEvent_t a, b;
            HIPCHK(hipEventCreate(&a));
            HIPCHK(hipEventCreate(&b));
            c->prof_events.emplace_back(a, b);
        }
    }
    return PHI_OK;
}

int phi_prof_read(phi_ctx *c, int64_t *n_launches, double *total_ms, int64_t *total_bases)
{
    if (!c) return PHI_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < c->prof_used; i++) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->prof_events[i].first, c->prof_events[i].second));
        c->prof_ms_done += ms;
        c->prof_n_done++;
    }
    c->prof_used = 0;
    if (n_launches) *n_launches = c->prof_n_done;
    if (total_ms) *total_ms = c->prof_ms_done;
    if (total_bases) *total_bases = c->prof_bases;
    c->prof_n_done = 0; c->prof_ms_done = 0.0; c->prof_bases = 0;
    return PHI_OK;
}

}  // extern "C"
