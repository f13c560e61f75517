// text_stream.hip -- reads as raw text (FASTA / FASTQ): the stream's pieces are copied to the device, where reads_text.hip
// finds the records, and scored as batches; what a piece leaves unfinished is carried into the next.  No kernel.  The
// stream's sizes and the update of the host carry are rules of reads_host.h.
#include "phi_ctx.h"

extern "C" {

// ---- reads as raw text: the records are found on the device (reads_text.hip)

int phi_reads_text_begin(phi_ctx *c, int64_t max_chunk_bytes)
{
    if (!c) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_reads_text_begin before phi_set_graph");
    if (max_chunk_bytes <= 0) return phi_fail(c, PHI_ERR_INVALID, "phi_reads_text_begin: bad chunk size");
    HIPCHK(hipSetDevice(c->device));
    PHICHK(phi_sync_check(c));                                // (batches handed over without a wait: their overflow shows here, not in a replay of ours)
    c->rlog.async_batches = false;
    auto &T = c->text;
    const PhiTextSizes Z = phi_text_sizes(max_chunk_bytes, getenv("PHI_TEXT_CARRY"));
    const uint32_t chunk = Z.chunk, carry = Z.carry, line_cap = Z.line_cap;
    for (int i = 0; i < 2; i++) {
        PHICHK(phi_dev_ensure(c, T.text[i], (size_t)carry + chunk + 64));
        PHICHK(phi_dev_ensure(c, T.bases[i], (size_t)carry + chunk + 64));
        PHICHK(phi_dev_ensure(c, T.roff[i], ((size_t)line_cap + 2) * 8));
    }
    PHICHK(phi_dev_ensure(c, T.tile_cnt, ((size_t)phi_text_num_tiles(0, carry + chunk + 64) + 2) * 4));
    PHICHK(phi_dev_ensure(c, T.ls, ((size_t)line_cap + 2) * 4));
    PHICHK(phi_dev_ensure(c, T.pre, ((size_t)line_cap + 2) * 8));
    PHICHK(phi_dev_ensure(c, T.blk, ((size_t)phi_text_scan_blocks(line_cap) + 1) * 8));
    PHICHK(phi_dev_ensure(c, T.sum, sizeof(PhiTextSummary)));
    if (!T.h_sum) HIPCHK(hipHostMalloc((void **)&T.h_sum, 64 + sizeof(PhiTextSummary), hipHostMallocDefault));
    if (!T.ev_copy) HIPCHK(hipEventCreateWithFlags(&T.ev_copy, hipEventDisableTiming));
    T.carry_cap = carry; T.chunk_cap = chunk; T.line_cap = line_cap;
    T.active = true; T.irregular = false; T.started = false; T.mode = 0;
    T.fed = 0; T.taken = 0; T.slot = 0; T.carry_len = 0; T.carry_at = carry; T.h_carry.clear();
    T.last_slot = -1; T.why = 0; T.first_bad = 0; T.detached = false; T.carry_stale = false;
    return PHI_OK;
}

}  // extern "C"

// the sketch of the chunk before may have filled the overflow list of novel hashes: its bases and offsets are still in their slot
static int text_replay_last(phi_ctx *c, uint32_t err)
{
    auto &T = c->text;
    if (T.last_slot < 0 || !(err & PHI_KERR_TABLE_FULL)) return PHI_OK;
    return replay_if_full(c, err, T.bases[T.last_slot].p, T.last_uniform ? nullptr : T.roff[T.last_slot].p, T.last_reads, T.last_bases);
}

// the carry's host copy, when the pieces came from device memory (parked text: nobody had their bytes on the host)
static int text_carry_to_host(phi_ctx *c)
{
    auto &T = c->text;
    if (!T.carry_stale) return PHI_OK;
    T.h_carry.resize(T.carry_len);
    if (T.carry_len) HIPCHK(phi_copy_sync(c, T.h_carry.data(), T.text[T.slot].as<uint8_t>() + T.carry_at, T.carry_len, hipMemcpyDeviceToHost));
    T.carry_stale = false;
    return PHI_OK;
}

// one piece of the stream: m bytes at p (host memory) -- or at d_src (device memory, p = NULL; first = the piece's first byte)
static int text_piece(phi_ctx *c, const char *p, uint32_t m, int32_t *irregular, const void *d_src = nullptr, char first = 0)
{
    auto &T = c->text;
    T.dbg_reads = 0; T.dbg_bases = 0;
    if (p) first = p[0];
    if (!T.started) {
        T.started = true;
        // the layout is decided by the first byte of the stream; text before the first header is the host reader's business
        if (first == '@') T.mode = 1;
        else if (first == '>') T.mode = 0;
        else { T.irregular = true; T.why = PHI_TEXT_IRREGULAR_LAYOUT; T.first_bad = 0; *irregular = 1; return PHI_OK; }
    }
    if (p) PHICHK(text_carry_to_host(c));
    if (T.detached) { T.h_carry.clear(); T.detached = false; }
    const int slot = T.slot ^ 1;
    const uint32_t C = T.carry_cap, start = C - T.carry_len, end = C + m;
    uint8_t *buf = T.text[slot].as<uint8_t>();
    // chunk i + 1 crosses the link while chunk i is sketched: the copy runs on aux_stream, everything else on `stream`
    HIPCHK(hipMemcpyAsync(buf + C, p ? (const void *)p : d_src, m, p ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->aux_stream));
    HIPCHK(hipEventRecord(T.ev_copy, c->aux_stream));
    if (T.carry_len)
        HIPCHK(hipMemcpyAsync(buf + start, T.text[T.slot].as<uint8_t>() + T.carry_at, T.carry_len, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamWaitEvent(c->stream, T.ev_copy, 0));
    HIPCHK(hipMemsetAsync(T.sum.p, 0, sizeof(PhiTextSummary), c->stream));
    HIPCHK(hipMemsetAsync(&T.sum.as<PhiTextSummary>()->first_bad, 0xFF, 4, c->stream));
    PhiTextArgs A{};
    A.buf = buf; A.start = start; A.end = end; A.mode = T.mode; A.line_cap = T.line_cap;
    A.tile_cnt = T.tile_cnt.as<uint32_t>(); A.ls = T.ls.as<uint32_t>(); A.pre = T.pre.as<uint64_t>(); A.blk = T.blk.as<uint64_t>();
    A.read_off = T.roff[slot].as<int64_t>(); A.bases = T.bases[slot].as<uint8_t>(); A.sum = T.sum.as<PhiTextSummary>();
    phi_launch_reads_text(c->stream, A);
    HIPCHK(hipGetLastError());
    uint32_t *h_err = (uint32_t *)((char *)T.h_sum + sizeof(PhiTextSummary));
    HIPCHK(hipMemcpyAsync(T.h_sum, T.sum.p, sizeof(PhiTextSummary), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h_err, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                 // also ends the sketch of the chunk before, and the copy of this one
    PHICHK(text_replay_last(c, *h_err));
    T.last_slot = -1;
    T.dbg_reads = 0; T.dbg_bases = 0;
    const PhiTextSummary S = *T.h_sum;
    const uint32_t tail = end - S.cons_end;
    if (S.err || tail > C) {
        // nothing of this chunk is taken: the caller parses the pending bytes (phi_reads_text_end) and this chunk on the host
        T.irregular = true; T.why = S.err ? S.err : PHI_TEXT_IRREGULAR_LINES; T.first_bad = S.first_bad; *irregular = 1;
        return PHI_OK;
    }
    if (S.n_rec) {
        // records of one length (>= 32): the sketch kernel computes the read starts, no offsets
        const bool uni = !S.not_uniform && S.n_bases % S.n_rec == 0 && S.n_bases / S.n_rec >= 32;
        T.last_uniform = uni;
        PHICHK(phi_add_reads_device_impl(c, T.bases[slot].p, uni ? nullptr : T.roff[slot].p, (int64_t)S.n_rec, (int64_t)S.n_bases, false));
        T.last_slot = slot; T.last_reads = (int64_t)S.n_rec; T.last_bases = (int64_t)S.n_bases;
        T.dbg_slot = slot; T.dbg_reads = (int64_t)S.n_rec; T.dbg_bases = (int64_t)S.n_bases;
    }
    // the bytes not taken, on the host as well: the last `tail` bytes of (carry before + this chunk)
    if (!p) T.carry_stale = true;                            // (fetched from the device when somebody asks: text_carry_to_host)
    else phi_text_carry_update(T.h_carry, p, m, tail);
    T.taken += (int64_t)(S.cons_end - start);
    T.fed += m;
    T.carry_len = tail; T.carry_at = S.cons_end; T.slot = slot;
    return PHI_OK;
}

extern "C" {

int phi_add_reads_text(phi_ctx *c, const char *text, int64_t n_bytes, int32_t *irregular)
{
    if (!c || !irregular || n_bytes < 0 || (n_bytes > 0 && !text)) return PHI_ERR_INVALID;
    *irregular = 0;
    auto &T = c->text;
    if (!T.active) return phi_fail(c, PHI_ERR_STATE, "phi_add_reads_text before phi_reads_text_begin");
    if (T.irregular) return phi_fail(c, PHI_ERR_STATE, "phi_add_reads_text after an irregular chunk: finish the stream on the host reader");
    HIPCHK(hipSetDevice(c->device));
    for (int64_t at = 0; at < n_bytes; ) {
        const uint32_t m = (uint32_t)std::min<int64_t>(n_bytes - at, T.chunk_cap);
        PHICHK(text_piece(c, text + at, m, irregular));
        if (*irregular) {
            // what the device has not taken = the carry + the rest of this call's bytes: all of it is handed back by
            // phi_reads_text_end, the caller goes on with the bytes of the stream AFTER this call's
            T.h_carry.insert(T.h_carry.end(), text + at, text + n_bytes);
            break;
        }
        at += m;
    }
    return PHI_OK;
}

int phi_add_reads_text_parked(phi_ctx *c, phi_text_park *p, int32_t index, int32_t *irregular)
{
    if (!c || !irregular) return PHI_ERR_INVALID;
    *irregular = 0;
    // (the piece's bytes on this context's device, landed: the park's own accessor waits for their copy)
    const void *d_piece = nullptr;
    int64_t n_piece = 0;
    char first = 0;
    const int prc = phi_text_park_piece_dev(p, index, c->device, &d_piece, &n_piece, &first);
    if (prc == PHI_ERR_INVALID) return phi_fail(c, PHI_ERR_INVALID, "phi_add_reads_text_parked: no such piece on this context's device");
    if (prc) return phi_fail(c, prc, "phi_add_reads_text_parked: the wait for the piece's bytes failed");
    auto &T = c->text;
    if (!T.active) return phi_fail(c, PHI_ERR_STATE, "phi_add_reads_text_parked before phi_reads_text_begin");
    if (T.irregular) return phi_fail(c, PHI_ERR_STATE, "phi_add_reads_text_parked after an irregular chunk: finish the stream on the host reader");
    HIPCHK(hipSetDevice(c->device));
    const char *d_text = static_cast<const char *>(d_piece);
    for (int64_t at = 0; at < n_piece; ) {
        const uint32_t m = (uint32_t)std::min<int64_t>(n_piece - at, T.chunk_cap);
        PHICHK(text_piece(c, nullptr, m, irregular, d_text + at, first));      // (the first byte matters to the stream's first piece only)
        if (*irregular) {
            // as phi_add_reads_text: what the device has not taken = the carry + the rest of this piece, handed back by phi_reads_text_end
            PHICHK(text_carry_to_host(c));
            const size_t had = T.h_carry.size();
            T.h_carry.resize(had + (size_t)(n_piece - at));
            HIPCHK(phi_copy_sync(c, T.h_carry.data() + had, d_text + at, (size_t)(n_piece - at), hipMemcpyDeviceToHost));
            break;
        }
        at += m;
    }
    return PHI_OK;
}

int phi_reads_text_last_batch(phi_ctx *c, char *bases, int64_t cap_bases, int64_t *off, int64_t cap_reads, int64_t *n_reads, int64_t *n_bases)
{
    if (!c || !n_reads || !n_bases) return PHI_ERR_INVALID;
    auto &T = c->text;
    *n_reads = T.dbg_reads; *n_bases = T.dbg_bases;
    if (T.dbg_reads == 0 || cap_reads < T.dbg_reads || cap_bases < T.dbg_bases || !off) return PHI_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (T.dbg_bases && bases) HIPCHK(phi_copy_sync(c, bases, T.bases[T.dbg_slot].p, (size_t)T.dbg_bases, hipMemcpyDeviceToHost));
    HIPCHK(phi_copy_sync(c, off, T.roff[T.dbg_slot].p, (size_t)(T.dbg_reads + 1) * 8, hipMemcpyDeviceToHost));
    return PHI_OK;
}

int phi_reads_text_detach_carry(phi_ctx *c, const char **bytes, int64_t *n)
{
    if (!c || !bytes || !n) return PHI_ERR_INVALID;
    auto &T = c->text;
    if (!T.active || T.irregular) return phi_fail(c, PHI_ERR_STATE, "phi_reads_text_detach_carry: no regular text stream is open");
    HIPCHK(hipSetDevice(c->device));
    PHICHK(text_carry_to_host(c));
    *bytes = T.h_carry.data(); *n = (int64_t)T.h_carry.size();
    T.carry_len = 0; T.detached = true;                       // (the host copy is dropped by the next piece: the pointer stays valid until then)
    return PHI_OK;
}

int phi_reads_text_end(phi_ctx *c, const char **pending, int64_t *n_pending, int64_t *n_taken)
{
    if (!c) return PHI_ERR_INVALID;
    auto &T = c->text;
    if (!T.active) return phi_fail(c, PHI_ERR_STATE, "phi_reads_text_end before phi_reads_text_begin");
    HIPCHK(hipSetDevice(c->device));
    uint32_t err = 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(phi_copy_sync(c, &err, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost));
    PHICHK(text_replay_last(c, err));
    T.last_slot = -1;
    T.active = false;
    if (!T.irregular) PHICHK(text_carry_to_host(c));
    if (T.detached) { T.h_carry.clear(); T.detached = false; }      // (handed out already)
    if (pending) *pending = T.h_carry.data();
    if (n_pending) *n_pending = (int64_t)T.h_carry.size();
    if (n_taken) *n_taken = T.taken;
    return PHI_OK;
}

}  // extern "C"
