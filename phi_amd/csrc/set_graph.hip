// set_graph.hip -- phi_set_graph: the index of a graph and its walks, and the DP step stream.
// Host-side orchestration only.  The per-base work runs in the kernels of contexts.hip, sketch.hip, table.hip and anchors.hip
// (build_classes, build_minimizer_table, build_read_table below); the step stream that dp.hip and dp_events.hip consume is
// plain host code (dp_steps.h).  set_graph_impl at the end of the file is the schedule: which thread runs what, and what is
// joined where.
#include <string.h>
#include <algorithm>
#include <future>
#include <memory>
#include "phi_ctx.h"
#include "phi_dev.h"
#include "dp_steps.h"

// The read table of the read probes (phi_launch_read_table) from the walk-minimiser table's keys and dense ids.  At most
// 3/16 key per bucket: a read probe then takes a second trip when the key it looks for sits past its home bucket (0.25 %
// of the keys at C2's 0.127 a bucket, 0.54 % at 3/16) or when a novel hash's home bucket has overflowed (3e-4 / 1e-3 of
// the buckets); C2's 533 074 keys get 2^22 buckets, the 134 MB the one-slot table of pairs had.  A key that finds no
// room within PHI_MAX_PROBE buckets: built again at twice the buckets.  PHI_READ_TABLE_BUCKETS (tests): the first try's
// buckets -- high loads, overflow chains, the full table.
static int build_read_table(phi_ctx *c)
{
    uint64_t nb = pow2_at_least(std::max<uint64_t>(64, (16 * (uint64_t)c->n_unique + 2) / 3));
    if (const char *e = getenv("PHI_READ_TABLE_BUCKETS")) nb = pow2_at_least(std::max<long long>(atoll(e), 1));
    uint32_t err0 = 0;                                  // (a table overflow raised before this one: reported by phi_sync_check)
    HIPCHK(hipMemcpyAsync(&err0, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int attempt = 0;; attempt++) {
        PHICHK(phi_dev_ensure(c, c->d_rt, nb * 32));
        phi_launch_read_table(c->stream, c->d_u_keys.as<uint64_t>(), c->d_u_uid.as<uint32_t>(), (int64_t)c->u_cap,
                              c->d_rt.as<uint64_t>(), (int64_t)nb, (uint32_t *)scalar(c, S_ERR));
        uint32_t err = 0;
        HIPCHK(hipMemcpyAsync(&err, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if ((err0 & PHI_KERR_TABLE_FULL) || !(err & PHI_KERR_TABLE_FULL)) break;
        if (attempt >= 40) return phi_fail(c, PHI_ERR_OVERFLOW, "read table overflow at %llu buckets (internal error)", (unsigned long long)nb);
        err &= ~PHI_KERR_TABLE_FULL;
        HIPCHK(phi_copy_sync(c, scalar(c, S_ERR), &err, 4, hipMemcpyHostToDevice));
        nb *= 2;
    }
    c->rt_buckets = nb; c->rt_mask = nb - 1;
    return PHI_OK;
}

// The k-mer table beside it (phi_ctx.h d_kt): for every class record the canonical k-mer under it, from the class-space
// text, checked against the record's hash; its phi_kmer_mix under the record's slot of the walk-minimiser table; then the
// read table's build over those keys and the same dense ids, at the read table's buckets.  A record whose k-mer holds a base
// outside ACGTacgt has no 2-bit value and is skipped: no clean read carries its k-mer.  Two records of one hash and
// different k-mers -- a MurmurHash3 collision inside the graph -- leave the graph without a k-mer table: the reads then take
// the hash route, which treats the two as the reference does.  k <= 31: a 32-mer has no value to spare for the sentinel.
static int build_kmer_table(phi_ctx *c)
{
    c->kt_buckets = 0; c->kt_mask = 0;
    if (c->k > 31 || c->n_rec <= 0 || c->n_unique <= 0) return PHI_OK;
    PhiStageTimer tg("set_graph");
    DevBuf kkeys, ctr;
    PhiDevGuard guard{{&kkeys, &ctr}};
    PHICHK(phi_dev_ensure(c, kkeys, c->u_cap * 8));
    PHICHK(phi_dev_ensure(c, ctr, 5 * 8));
    phi_launch_fill_u64(c->stream, kkeys.as<uint64_t>(), (int64_t)c->u_cap, PHI_EMPTY_KEY);
    HIPCHK(hipMemsetAsync(ctr.p, 0, 5 * 8, c->stream));
    phi_launch_kmer_keys(c->stream, c->d_rec_cls.as<int32_t>(), c->d_rec_rel.as<int32_t>(), c->d_rec_hash.as<uint64_t>(), c->d_rec_slot.as<uint32_t>(),
                         c->n_rec, c->d_cls_base.as<int64_t>(), c->d_cls_left.as<uint8_t>(), c->d_wwords.as<uint64_t>(), c->d_wbad.as<uint32_t>(),
                         c->k, kkeys.as<uint64_t>(), ctr.as<unsigned long long>());
    uint64_t n[5] = {0, 0, 0, 0, 0};
    HIPCHK(phi_copy_sync(c, n, ctr.p, 3 * 8, hipMemcpyDeviceToHost));
    if (n[1]) return phi_fail(c, PHI_ERR_DEVICE, "k-mer table: %llu class records whose k-mer in class space does not hash to the record's hash (internal error)", (unsigned long long)n[1]);
    if (n[2]) {
        if (tg.on) fprintf(stderr, "[phi timing] set_graph: %llu walk minimisers share a hash with another k-mer: no k-mer table for this graph\n", (unsigned long long)n[2]);
        return PHI_OK;
    }
    uint64_t nb = c->rt_buckets;
    uint32_t err0 = 0;                                  // (a table overflow raised before this one: reported by phi_sync_check)
    HIPCHK(phi_copy_sync(c, &err0, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost));
    if (err0 & PHI_KERR_TABLE_FULL) return PHI_OK;
    for (int attempt = 0;; attempt++) {
        PHICHK(phi_dev_ensure(c, c->d_kt, nb * 32));
        phi_launch_read_table(c->stream, kkeys.as<uint64_t>(), c->d_u_uid.as<uint32_t>(), (int64_t)c->u_cap, c->d_kt.as<uint64_t>(), (int64_t)nb,
                              (uint32_t *)scalar(c, S_ERR));
        uint32_t err = 0;
        HIPCHK(phi_copy_sync(c, &err, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost));
        if (!(err & PHI_KERR_TABLE_FULL)) break;
        if (attempt >= 40) return phi_fail(c, PHI_ERR_OVERFLOW, "k-mer table overflow at %llu buckets (internal error)", (unsigned long long)nb);
        err &= ~PHI_KERR_TABLE_FULL;
        HIPCHK(phi_copy_sync(c, scalar(c, S_ERR), &err, 4, hipMemcpyHostToDevice));
        nb *= 2;
    }
    c->kt_buckets = nb; c->kt_mask = nb - 1;
    int n_cu = 0;
    HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device));
    c->kt_max_chunks = (int64_t)n_cu * 4 * 7;           // (waves resident at once: four SIMDs a CU, seven waves of the read kernel each)
    if (tg.on) {
        phi_launch_rt_overflowed(c->stream, c->d_rt.as<uint64_t>(), (int64_t)c->rt_buckets, ctr.as<unsigned long long>() + 3);
        phi_launch_rt_overflowed(c->stream, c->d_kt.as<uint64_t>(), (int64_t)nb, ctr.as<unsigned long long>() + 4);
        HIPCHK(phi_copy_sync(c, n + 3, ctr.as<uint64_t>() + 3, 2 * 8, hipMemcpyDeviceToHost));
        fprintf(stderr, "[phi timing] set_graph: k-mer table of %llu buckets (%.1f MB) beside the read table's %llu; %llu class records with a base outside ACGT skipped; "
                        "OVERFLOWED buckets: read table %.2e, k-mer table %.2e\n", (unsigned long long)nb, (double)nb * 32 / 1e6, (unsigned long long)c->rt_buckets,
                (unsigned long long)n[0], (double)n[3] / (double)c->rt_buckets, (double)n[4] / (double)nb);
        tg.lap("[gpu thread]   k-mer table");
    }
    return PHI_OK;
}

// Classes of walk entries with equal context, their sketch in class space and the class records
// (contexts.hip).  Leaves d_vlen, d_ent_cls, d_cls_*, d_rec_{hash,cls,rel,e0,e1}, n_cls, n_rec,
// h_walk_base / walk_bases.  Runs on the context's stream; called by the GPU thread of phi_set_graph.
static int build_classes(phi_ctx *c, int32_t n_vtx, int32_t n_walks, int64_t n_entries)
{
    PhiStageTimer tg("set_graph");
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    HIPCHK(hipEventCreate(&ev0));
    HIPCHK(hipEventCreate(&ev1));
    struct EvGuard { hipEvent_t a, b; ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } evg{ev0, ev1};
    HIPCHK(hipEventRecord(ev0, c->stream));
    PHICHK(phi_dev_ensure(c, c->d_vlen, (size_t)n_vtx * 4));
    phi_launch_vlen(c->stream, c->d_seq_off.as<int64_t>(), n_vtx, c->d_vlen.as<int32_t>());
    // bases of every walk (flat base offset of each walk: the positions phi_walk_minimizers reports are walk-relative)
    PHICHK(phi_dev_ensure(c, c->d_list, (size_t)(n_walks + 1) * 8));
    HIPCHK(hipMemsetAsync(c->d_list.p, 0, (size_t)(n_walks + 1) * 8, c->stream));
    phi_launch_walk_bases(c->stream, c->d_walk_vtx.as<int32_t>(), c->d_vlen.as<int32_t>(), c->d_walk_off.as<int64_t>(), n_walks, n_entries,
                          c->d_list.as<unsigned long long>());
    c->h_walk_base.assign(n_walks + 1, 0);
    HIPCHK(hipMemcpyAsync(c->h_walk_base.data() + 1, c->d_list.p, (size_t)n_walks * 8, hipMemcpyDeviceToHost, c->stream));

    tg.lap("[gpu thread]     events, vlen, walk bases");
    // ---- classes: table of context fingerprints, verified entry by entry
    PHICHK(phi_dev_ensure(c, c->d_ent_cls, (size_t)n_entries * 4));
    PHICHK(phi_dev_ensure(c, c->d_flags, (size_t)n_entries));
    DevBuf t_keys, t_rep, t_mult;
    PhiDevGuard guard{{&t_keys, &t_rep, &t_mult}};
    PhiClassArgs A{};
    A.walk_vtx = c->d_walk_vtx.as<int32_t>(); A.walk_off = c->d_walk_off.as<int64_t>(); A.n_walks = n_walks; A.n_entries = n_entries;
    A.vlen = c->d_vlen.as<int32_t>(); A.seq = c->d_seq.as<uint8_t>(); A.seq_off = c->d_seq_off.as<int64_t>();
    A.tail_need = c->w + c->k - 2;
    A.ent_slot = c->d_ent_cls.as<uint32_t>();
    A.err = (uint32_t *)scalar(c, S_ERR);
    // a pangenome has a few contexts per vertex; walks that share nothing have one per entry
    const uint64_t cap_max = pow2_at_least(std::max<uint64_t>(1024, 2 * (uint64_t)n_entries));
    uint64_t cap = std::min(cap_max, pow2_at_least(std::max<uint64_t>(1024, 4 * (uint64_t)n_vtx)));
    tg.lap("[gpu thread]     entry buffers");
    for (int attempt = 0;; attempt++) {
        PHICHK(phi_dev_ensure(c, t_keys, cap * 8));
        PHICHK(phi_dev_ensure(c, t_rep, cap * 4));
        PHICHK(phi_dev_ensure(c, t_mult, cap * 4));
        A.t_keys = t_keys.as<uint64_t>(); A.t_rep = t_rep.as<uint32_t>(); A.t_mult = t_mult.as<uint32_t>(); A.t_mask = cap - 1;
        A.seed = 0x13198A2E03707344ull + 0x9E3779B97F4A7C15ull * (uint64_t)attempt;
        phi_launch_fill_u64(c->stream, A.t_keys, (int64_t)cap, PHI_EMPTY_KEY);
        phi_launch_fill_u32(c->stream, A.t_rep, (int64_t)cap, 0xFFFFFFFFu);
        HIPCHK(hipMemsetAsync(A.t_mult, 0, cap * 4, c->stream));
        phi_launch_class_insert(c->stream, A);
        uint32_t err = 0;
        HIPCHK(hipMemcpyAsync(&err, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (err & PHI_KERR_TABLE_FULL) {
            if (cap == cap_max) return phi_fail(c, PHI_ERR_OVERFLOW, "walk-context table overflow (internal error)");
            cap = std::min(cap_max, cap * 8);
            err &= ~PHI_KERR_TABLE_FULL;
            HIPCHK(phi_copy_sync(c, scalar(c, S_ERR), &err, 4, hipMemcpyHostToDevice));
            attempt--;
            continue;
        }
        phi_launch_class_verify(c->stream, A, c->d_flags.as<uint8_t>());
        HIPCHK(hipMemcpyAsync(&err, scalar(c, S_ERR), 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (!(err & PHI_KERR_FP_COLLISION)) break;
        if (attempt >= 7) return phi_fail(c, PHI_ERR_DEVICE, "walk-context fingerprints collide under 8 seeds (internal error)");
        err &= ~PHI_KERR_FP_COLLISION;
        HIPCHK(phi_copy_sync(c, scalar(c, S_ERR), &err, 4, hipMemcpyHostToDevice));
    }
    tg.lap("[gpu thread]     table insert + verify");
    for (int32_t h = 0; h < n_walks; h++) c->h_walk_base[h + 1] += c->h_walk_base[h];
    c->walk_bases = c->h_walk_base[n_walks];
    // classes in the order of their representatives (smallest entry): the same on every rank
    PHICHK(phi_compact(c, c->d_flags.as<uint8_t>(), n_entries, c->d_cls_rep, &c->n_cls));
    const int64_t nc = c->n_cls;
    tg.lap("[gpu thread]     compact representatives");
    PHICHK(phi_dev_ensure(c, c->d_cls_mult, (size_t)nc * 4));
    PHICHK(phi_dev_ensure(c, c->d_cls_left, (size_t)nc));
    PHICHK(phi_dev_ensure(c, c->d_cls_base, (size_t)(nc + 1) * 8));
    PHICHK(phi_dev_ensure(c, c->d_cls_rec_off, (size_t)(nc + 1) * 4));
    // (the rep slot array t_rep is reused as slot -> class id)
    phi_launch_class_ids(c->stream, c->d_cls_rep.as<phi_ent_t>(), nc, A.ent_slot, n_entries, A.t_mult, A.t_rep, c->d_cls_mult.as<int32_t>(),
                         c->d_ent_cls.as<int32_t>());
    PHICHK(phi_dev_ensure(c, c->d_list3, (size_t)nc * 4));
    phi_launch_class_len(c->stream, A, c->d_cls_rep.as<phi_ent_t>(), nc, c->d_list3.as<int32_t>(), c->d_cls_left.as<uint8_t>());
    PHICHK(phi_scan(c, c->d_list3.as<int32_t>(), nc, c->d_cls_base.as<int64_t>()));
    int64_t run = 0;
    HIPCHK(hipMemcpyAsync(&run, c->d_cls_base.as<int64_t>() + nc, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->cls_bases = run;
    if (tg.on) fprintf(stderr, "[phi timing] set_graph: %lld entries in %lld classes, %lld bases of class space for %lld bases of walks\\n",
                       (long long)n_entries, (long long)nc, (long long)run, (long long)c->walk_bases);
    tg.lap("[gpu thread]   classes");

    // ---- class space: packed bases, start bitmap, sketch
    const int64_t n_words = (run + 31) / 32;
    PHICHK(phi_dev_ensure(c, c->d_wwords, (size_t)(n_words + 2) * 8));
    PHICHK(phi_dev_ensure(c, c->d_wbad, (size_t)(n_words + 6) * 4));
    auto pack = [&](uint8_t *ascii) {
        phi_launch_pack_classes(c->stream, c->d_seq.as<uint8_t>(), c->d_seq_off.as<int64_t>(), c->d_walk_vtx.as<int32_t>(), c->d_vlen.as<int32_t>(),
                                c->d_cls_rep.as<phi_ent_t>(), c->d_cls_left.as<uint8_t>(), c->d_cls_base.as<int64_t>(), nc,
                                c->d_wwords.as<uint64_t>(), n_words, c->d_wbad.as<uint32_t>(), ascii, (unsigned long long *)scalar(c, S_NBAD));
    };
    pack(nullptr);
    // bases outside ACGTacgt in the graph: keep a flat ASCII copy of class space for the byte-wise path
    const uint8_t *cls_ascii = nullptr;
    {
        uint64_t n_bad = 0;
        HIPCHK(hipMemcpyAsync(&n_bad, scalar(c, S_NBAD), 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (n_bad || c->k > PHI_MAX_K_PACKED) {                 // (k > 32: the byte-wise path for every window)
            PHICHK(phi_dev_ensure(c, c->d_wascii, (size_t)run + 64));
            HIPCHK(hipMemsetAsync(scalar(c, S_NBAD), 0, 8, c->stream));
            pack(c->d_wascii.as<uint8_t>());
            cls_ascii = c->d_wascii.as<uint8_t>();
        }
    }
    const size_t n_sw = (size_t)(run / 64 + 2);
    PHICHK(phi_dev_ensure(c, c->d_wstarts, n_sw * 8));
    HIPCHK(hipMemsetAsync(c->d_wstarts.p, 0, n_sw * 8, c->stream));
    phi_launch_mark_starts(c->stream, c->d_cls_base.as<int64_t>(), nc, c->d_wstarts.as<unsigned long long>());
    int64_t n_raw = 0;
    DevBuf raw_hash;
    PhiDevGuard guard1{{&raw_hash}};
    PHICHK(sketch_records(c, c->d_wwords.as<uint64_t>(), c->d_wstarts.as<unsigned long long>(), run, c->k, c->w, cls_ascii, raw_hash,
                          c->d_rec_pos, &n_raw));
    if (n_raw >= (int64_t)1 << 31) return phi_fail(c, PHI_ERR_UNSUPPORTED, "more than 2^31 minimisers in the distinct walk contexts");
    tg.lap("[gpu thread]   class-space pack + sketch");

    // ---- raw records -> class records (the left base's own window dropped)
    const int64_t nr0 = std::max<int64_t>(n_raw, 1);
    DevBuf r_cls, r_rel, r_e0, r_e1;
    PhiDevGuard guard4{{&r_cls, &r_rel, &r_e0, &r_e1}};
    PHICHK(phi_dev_ensure(c, r_cls, (size_t)nr0 * 4));
    PHICHK(phi_dev_ensure(c, r_rel, (size_t)nr0 * 4));
    PHICHK(phi_dev_ensure(c, r_e0, (size_t)nr0 * 4));
    PHICHK(phi_dev_ensure(c, r_e1, (size_t)nr0 * 4));
    PHICHK(phi_dev_ensure(c, c->d_flags, (size_t)std::max<int64_t>(nr0, n_entries)));
    phi_launch_class_rec(c->stream, c->d_rec_pos.as<int64_t>(), n_raw, c->d_cls_base.as<int64_t>(), nc, c->d_cls_rep.as<phi_ent_t>(),
                         c->d_cls_left.as<uint8_t>(), c->d_walk_vtx.as<int32_t>(), c->d_vlen.as<int32_t>(), c->k, c->d_flags.as<uint8_t>(),
                         r_cls.as<int32_t>(), r_rel.as<int32_t>(), r_e0.as<phi_ent_t>(), r_e1.as<phi_ent_t>());
    PHICHK(phi_compact(c, c->d_flags.as<uint8_t>(), n_raw, c->d_list2, &c->n_rec));
    const int64_t nr = std::max<int64_t>(c->n_rec, 1);
    PHICHK(phi_dev_ensure(c, c->d_rec_hash, (size_t)nr * 8));
    PHICHK(phi_dev_ensure(c, c->d_rec_cls, (size_t)nr * 4));
    PHICHK(phi_dev_ensure(c, c->d_rec_rel, (size_t)nr * 4));
    PHICHK(phi_dev_ensure(c, c->d_rec_e0, (size_t)nr * 4));
    PHICHK(phi_dev_ensure(c, c->d_rec_e1, (size_t)nr * 4));
    phi_launch_class_rec_gather(c->stream, c->d_list2.as<int32_t>(), c->n_rec, raw_hash.as<uint64_t>(), r_cls.as<int32_t>(), r_rel.as<int32_t>(),
                                r_e0.as<phi_ent_t>(), r_e1.as<phi_ent_t>(), c->d_rec_hash.as<uint64_t>(), c->d_rec_cls.as<int32_t>(),
                                c->d_rec_rel.as<int32_t>(), c->d_rec_e0.as<phi_ent_t>(), c->d_rec_e1.as<phi_ent_t>());
    phi_launch_class_rec_off(c->stream, c->d_rec_cls.as<int32_t>(), c->n_rec, nc, c->d_cls_rec_off.as<int32_t>());
    HIPCHK(hipEventRecord(ev1, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                  // the temporaries above go out of scope
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    c->index_gpu_ms = ms;
    HIPCHK(hipGetLastError());
    return PHI_OK;
}

// What phi_set_graph and phi_set_graph_chopped check before anything else, with the same words: the arguments, the state
// the device-resident walks need (this clears the graph the context held), then the offset arrays both index with.
int set_graph_check_args(phi_ctx *c, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off, const int64_t *adj_off,
                         const int32_t *adj, int32_t n_walks, const int64_t *walk_off, const int32_t *walk_vtx, const int32_t *topo_rank)
{
    // walk_vtx == NULL: the entries are on the device already, resolved there from the W-lines' text (phi_walk_text_resolve)
    const bool dev_walks = walk_vtx == nullptr;
    if (dev_walks && c && walk_off && n_walks > 0 && !(c->walks_on_device && c->walks_on_device_n == walk_off[n_walks] && (int32_t)(c->wtext.ends.size() / 2) == n_walks))
        return phi_fail(c, PHI_ERR_STATE, "phi_set_graph without walk_vtx: phi_walk_text_resolve must have resolved exactly these walks on this context");
    if (n_vtx <= 0 || n_walks <= 0 || !seq_concat || !seq_off || !adj_off || !walk_off || !topo_rank)
        return phi_fail(c, PHI_ERR_INVALID, "phi_set_graph: null pointer or empty graph");
    if (adj_off[n_vtx] > 0 && !adj) return phi_fail(c, PHI_ERR_INVALID, "phi_set_graph: adj is null");
    HIPCHK(hipSetDevice(c->device));
    if (c->ipc) return phi_fail(c, PHI_ERR_STATE, "phi_set_graph on a context in a group of processes: phi_ipc_destroy first (the peers have this context's hit vectors mapped)");
    c->have_graph = false;
    c->chop.on = false;
    c->panel.on = false;
    phi_scout_end(c);
    c->solved = false;
    c->calls.have = false;
    phi_ladder_drop(c);                                        // (a collected read set and its bands belong to the graph they were collected under)
    return PHI_OK;
}
int set_graph_check_offsets(phi_ctx *c, int32_t n_vtx, const int64_t *seq_off, const int64_t *adj_off, int32_t n_walks, const int64_t *walk_off)
{
    if (seq_off[0] != 0 || adj_off[0] != 0 || walk_off[0] != 0) return phi_fail(c, PHI_ERR_INVALID, "offset arrays must start at 0");
    for (int32_t v = 0; v < n_vtx; v++)
        if (seq_off[v + 1] < seq_off[v] || adj_off[v + 1] < adj_off[v]) return phi_fail(c, PHI_ERR_INVALID, "offsets not monotone at vertex %d", v);
    for (int32_t h = 0; h < n_walks; h++)
        if (walk_off[h + 1] <= walk_off[h]) return phi_fail(c, PHI_ERR_INVALID, "walk %d is empty", h);
    if (walk_off[n_walks] > PHI_MAX_ENTRIES) return phi_fail(c, PHI_ERR_UNSUPPORTED, "more than 2^32 - 64 walk entries");
    return PHI_OK;
}

// ---- phi_set_graph as a schedule ----------------------------------------------------------------------------------
// Everything one call of set_graph_impl shares between its stages and its threads, on set_graph_impl's stack.  The call
// runs up to four jobs beside the calling thread -- the uploads of the graph arrays, the host copy of the walk entries, the
// GPU thread (gpu_thread below) and, through the context, the pinning and the DP-buffer futures -- and all but the last two
// reference this object.  What holds, here and for whoever changes a stage:
//   * nothing the threads reference dies before they end: the destructor waits for the GPU thread, then for the host walk
//     copy, then for the uploads, and only then do the members go.  Every early return of set_graph_impl passes through it;
//   * no kernel indexes with the graph arrays before validate_topology has passed: the uploads started before it are copies
//     only, and the GPU thread is started after it;
//   * after a walk error (walk_err[0]) the GPU thread builds nothing further: the calling thread reports it;
//   * the host thread waiting for the edge counts is released whatever happens on the GPU thread (PromiseGuard);
//   * the step-stream vectors (steps: k_rec, k_in, cvtx are uploaded without a wait) live until the final phi_sync_check;
//   * c->dp_alloc_future is joined before the call returns successfully, and stage_release runs at the end;
//   * the calling thread's uploads go on c->stream like the GPU thread's work (a second stream was tried: slower, see
//     build_step_stream); only the device-to-host copy of walks resolved on the device uses c->aux_stream.
struct SetGraph {
    phi_ctx *const c;
    // the inputs, and the sizes once set_graph_check_offsets has passed
    const int32_t n_vtx;
    const char *const seq_concat;
    const int64_t *const seq_off, *const adj_off;
    const int32_t *const adj;
    const int32_t n_walks;
    const int64_t *const walk_off;
    const int32_t *const walk_vtx, *const topo_rank;
    int64_t n_edges = 0, n_entries = 0;
    const bool dev_walks;                                  // walk_vtx == NULL: the entries are on the device already
    bool want_masks = false;                               // the every-vertex stream of dp.hip is wanted
    bool keep_host_walks = false;
    PhiStageTimer tm{"set_graph"};
    std::vector<int64_t> indeg;                            // validate_topology
    std::vector<int32_t> cnt_edge;                         // walks per edge: written by the GPU thread, read after edges_future
    int32_t walk_err[4] = {0, 0, 0, 0};                    // likewise: code, walk, vertex, vertex
    std::vector<int32_t> ends_own;                         // host walks: first and last vertex of every walk
    const int32_t *walk_ends = nullptr;                    // [2 * n_walks]: ends_own, or c->wtext.ends for walks on the device
    PhiDpSteps steps;
    std::promise<int> edges_promise;                       // the walk-entry pass is done: its status
    std::future<int> edges_future = edges_promise.get_future();
    std::future<int> uploads, gpu;
    std::future<void> wv_copy;

    SetGraph(phi_ctx *c_, int32_t n_vtx_, const char *seq_concat_, const int64_t *seq_off_, const int64_t *adj_off_, const int32_t *adj_,
             int32_t n_walks_, const int64_t *walk_off_, const int32_t *walk_vtx_, const int32_t *topo_rank_)
        : c(c_), n_vtx(n_vtx_), seq_concat(seq_concat_), seq_off(seq_off_), adj_off(adj_off_), adj(adj_), n_walks(n_walks_), walk_off(walk_off_),
          walk_vtx(walk_vtx_), topo_rank(topo_rank_), dev_walks(walk_vtx_ == nullptr) {}
    ~SetGraph()
    {
        if (gpu.valid()) gpu.wait();
        if (wv_copy.valid()) wv_copy.wait();
        if (uploads.valid()) uploads.wait();
    }
};

// the solve downloads its kept anchors (12 bytes each, a fraction of the walk entries) into pinned
// memory; pinning tens of MB takes 5-30 ms, so it happens on a thread of its own, from now on
static void start_pinning(SetGraph &S)
{
    phi_ctx *c = S.c;
    if (c->pin_future.valid()) c->pin_future.wait();
    int64_t ne = S.walk_off[S.n_walks];                      // not validated yet: clamp
    ne = ne < 0 ? 0 : (ne > PHI_MAX_ENTRIES ? PHI_MAX_ENTRIES : ne);
    const size_t want = ((size_t)ne / 4 + 4096) * sizeof(PhiAnchorHost);
    // (only for graphs whose solve is likely to take the host copy of the anchors: a model of 2^16 anchors or more
    //  stays on the device, solve_dev.hip, and pinning tens of MB here holds up the other threads' HIP calls)
    if (want > c->h_pin_cap && ne / 4 < ((int64_t)1 << 16) && !getenv("PHI_PREPIN")) {
        c->h_kept = PhiAnchorSpan{}; c->h_dp = PhiAnchorSpan{}; c->anchors_host = false;
        c->pin_future = std::async(std::launch::async, [c, want]() {
            (void)hipSetDevice(c->device);
            if (c->h_pin) (void)hipHostFree(c->h_pin);
            c->h_pin = nullptr; c->h_pin_cap = 0;
            void *p = nullptr;
            if (hipHostMalloc(&p, want, hipHostMallocDefault) == hipSuccess) { c->h_pin = p; c->h_pin_cap = want; }
        });
    }
}

// The DP's per-entry buffers of a chromosome-scale graph (5 x 4-8 bytes per walk entry: 26 GB at 1.3 G entries) are
// allocated now, on a thread of their own: the driver clears device memory as it hands it out (tens of GB/s), which
// otherwise shows up as half a second at the start of phi_solve.  Joined before set_graph_impl returns.
static void start_dp_buffers(SetGraph &S)
{
    phi_ctx *c = S.c;
    if (c->dp_alloc_future.valid()) (void)c->dp_alloc_future.get();
    if (S.n_entries >= ((int64_t)1 << 24) && S.n_walks <= PHI_DP_EVENT_MAX_WALKS) {
        c->dp_alloc_future = std::async(std::launch::async, [c, n_entries = S.n_entries]() -> int {
            if (hipSetDevice(c->device) != hipSuccess) return PHI_ERR_DEVICE;
            const size_t ne = (size_t)n_entries;
            PHICHK(phi_dev_ensure(c, c->d_g_off, (ne + 1) * 8));
            PHICHK(phi_dev_ensure(c, c->d_dmax, ne * 4));
            PHICHK(phi_dev_ensure(c, c->d_bstart, ne * 4));
            PHICHK(phi_dev_ensure(c, c->d_off_end, (ne + 3) * 4));
            PHICHK(phi_dev_ensure(c, c->d_off_start, (ne + 3) * 4));
            return PHI_OK;
        });
    }
}

// The graph arrays go to the device while the calling thread validates them (copies from the caller's pageable arrays:
// 52 MB and 3 ms at C2).  Only copies: no kernel indexes with them before the validation has passed.
// (joined by the GPU thread, or by ~SetGraph on an early return)
static void start_uploads(SetGraph &S)
{
    S.uploads = std::async(std::launch::async, [&S]() -> int {
        phi_ctx *c = S.c;
        HIPCHK(hipSetDevice(c->device));
        PHICHK(upload(c, c->d_seq, S.seq_concat, (size_t)S.seq_off[S.n_vtx]));
        PHICHK(upload(c, c->d_seq_off, S.seq_off, (size_t)S.n_vtx + 1));
        if (!S.dev_walks) PHICHK(upload(c, c->d_walk_vtx, S.walk_vtx, (size_t)S.n_entries));
        PHICHK(upload(c, c->d_walk_off, S.walk_off, (size_t)S.n_walks + 1));
        PHICHK(upload(c, c->d_adj_off, S.adj_off, (size_t)S.n_vtx + 1));
        if (S.n_edges == 0) PHICHK(phi_dev_ensure(c, c->d_adj, 4));
        else PHICHK(upload(c, c->d_adj, S.adj, (size_t)S.n_edges));
        PHICHK(upload(c, c->d_topo_rank, S.topo_rank, (size_t)S.n_vtx));
        return PHI_OK;
    });
}

// topological order from the ranks; every edge must go forward (dp_steps.h).  All host threads: at chromosome scale these
// are 8.4 M + 11 M random accesses that every kernel of the index build waits for.
// (the walk entries are range-checked by the first kernel that reads them: phi_walk_edges_kernel, code 4 of report_walk_errors)
static int validate_topology(SetGraph &S)
{
    phi_ctx *c = S.c;
    PhiHostError verr;
    S.indeg.assign((size_t)S.n_vtx, 0);
    if (phi_topo_from_ranks(S.n_vtx, S.topo_rank, c->h_topo, verr) ||
        phi_check_edges(S.n_vtx, S.adj_off, S.adj, S.topo_rank, S.indeg.data(), verr))
        return phi_fail(c, verr.code, "%s", verr.msg.c_str());
    return PHI_OK;
}

// host copy of the walk entries for the solve (38 MB at C2, 4 ms of page faults): a few threads of their own, joined
// before set_graph_impl returns.  NOT for a chromosome-scale graph (5.3 GB at 1.3 G entries, beside the caller's own copy):
// what the solve looks up there -- a few entries per recombination of the backtrack, the stretches of the decoded path --
// it reads from the device copy (phi_solve.hip walk_vtx_*); the branch and bound proper fetches the array if it ever starts.
static int start_host_walk_copy(SetGraph &S)
{
    phi_ctx *c = S.c;
    int64_t host_walks_max = (int64_t)1 << 26;
    if (const char *e = getenv("PHI_HOST_WALKS_MAX")) host_walks_max = atoll(e);                     // tests: no host copy at any size
    S.keep_host_walks = S.n_entries <= host_walks_max;
    if (!c->h_walk_vtx.resize(S.keep_host_walks ? S.n_entries : 0)) return phi_fail(c, PHI_ERR_NOMEM, "host allocation failed");
    if (!S.keep_host_walks) return PHI_OK;
    S.wv_copy = std::async(std::launch::async, [c, dev_walks = S.dev_walks, n_entries = S.n_entries, walk_vtx = S.walk_vtx]() {
        int32_t *dst = c->h_walk_vtx.data();
        if (dev_walks) {                                       // (resolved on the device: the host copy comes from there)
            (void)hipSetDevice(c->device);
            if (n_entries && hipMemcpyAsync(dst, c->d_walk_vtx.p, (size_t)n_entries * 4, hipMemcpyDeviceToHost, c->aux_stream) == hipSuccess)
                (void)hipStreamSynchronize(c->aux_stream);
            return;
        }
        const int nt = 4;
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++)
            th.emplace_back([=]() {
                const int64_t lo = n_entries * t / nt, hi = n_entries * (t + 1) / nt;
                memcpy(dst + lo, walk_vtx + lo, (size_t)(hi - lo) * 4);
            });
        for (auto &x : th) x.join();
    });
    return PHI_OK;
}

// the walk-entry pass (out-edge of every entry, walks per edge, walks per vertex): walks follow edges of forward vertices
// (ILP_index.cpp:104-107 exits on reverse strand; an edge-less step would leave an anchor's edge variables unconstrained,
// :799-815).  Its edge counts and its error go to the host, the rest stays on the device.
static int walk_entry_pass(SetGraph &S)
{
    phi_ctx *c = S.c;
    const int nw64 = c->dp_nw;
    PHICHK(phi_dev_ensure(c, c->d_e_out, (size_t)S.n_entries));
    PHICHK(phi_dev_ensure(c, c->d_cnt_edge, S.cnt_edge.size() * 4));
    PHICHK(phi_dev_ensure(c, c->d_walk_err, 16));
    HIPCHK(hipMemsetAsync(c->d_cnt_edge.p, 0, S.cnt_edge.size() * 4, c->stream));
    HIPCHK(hipMemsetAsync(c->d_walk_err.p, 0, 16, c->stream));
    if (S.want_masks) {
        PHICHK(phi_dev_ensure(c, c->d_st_mask, (size_t)S.n_vtx * nw64 * 8));
        HIPCHK(hipMemsetAsync(c->d_st_mask.p, 0, (size_t)S.n_vtx * nw64 * 8, c->stream));
    }
    phi_launch_walk_edges(c->stream, c->d_walk_vtx.as<int32_t>(), c->d_walk_off.as<int64_t>(), S.n_walks, S.n_entries, S.n_vtx,
                          c->d_adj_off.as<int64_t>(), c->d_adj.as<int32_t>(), c->d_seq_off.as<int64_t>(),
                          c->d_topo_rank.as<int32_t>(), c->d_e_out.as<uint8_t>(), c->d_cnt_edge.as<int32_t>(),
                          S.want_masks ? c->d_st_mask.as<unsigned long long>() : nullptr, nw64, c->d_walk_err.as<int32_t>());
    HIPCHK(hipMemcpyAsync(S.cnt_edge.data(), c->d_cnt_edge.p, S.cnt_edge.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(S.walk_err, c->d_walk_err.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PHI_OK;
}

// The walk-minimiser table, built over the class records (nearly all distinct) at twice their number, then re-inserted at
// 8x the distinct keys (load ~12 %).  Leaves d_u_keys, d_u_uid, d_u_replist, d_rec_slot, u_cap, n_unique.  The read probes
// go to the read table built from it (build_read_table).
static int build_minimizer_table(phi_ctx *c)
{
    const int64_t nr = std::max<int64_t>(c->n_rec, 1);
    PHICHK(phi_dev_ensure(c, c->d_rec_slot, (size_t)nr * 4));
    const uint64_t cap_full = pow2_at_least(std::max<uint64_t>(1024, 2 * (uint64_t)c->n_rec));
    const uint64_t UMULT = 8;
    PHICHK(phi_dev_ensure(c, c->d_flags, (size_t)nr));
    c->u_cap = cap_full;
    PHICHK(phi_dev_ensure(c, c->d_u_keys, c->u_cap * 8));
    PHICHK(phi_dev_ensure(c, c->d_u_rep, c->u_cap * 4));
    phi_launch_fill_u64(c->stream, c->d_u_keys.as<uint64_t>(), (int64_t)c->u_cap, PHI_EMPTY_KEY);
    phi_launch_fill_u32(c->stream, c->d_u_rep.as<uint32_t>(), (int64_t)c->u_cap, 0xFFFFFFFFu);
    phi_launch_table_build(c->stream, c->d_rec_hash.as<uint64_t>(), c->n_rec, c->d_u_keys.as<uint64_t>(),
                           c->d_u_rep.as<uint32_t>(), c->u_cap - 1, c->d_rec_slot.as<uint32_t>(),
                           (uint32_t *)scalar(c, S_ERR));
    // dense, rank-independent minimiser ids: rank of the first class record of each hash
    phi_launch_rep_flags(c->stream, c->d_rec_slot.as<uint32_t>(), c->n_rec, c->d_u_rep.as<uint32_t>(),
                         c->d_flags.as<uint8_t>());
    PHICHK(phi_compact(c, c->d_flags.as<uint8_t>(), c->n_rec, c->d_u_replist, &c->n_unique));   // waits for the stream
    // wanted capacity: 8x the distinct keys; re-insert them (and look every record up again) when
    // the table is more than a factor two away from it
    const uint64_t want = pow2_at_least(std::max<uint64_t>(1024, UMULT * (uint64_t)c->n_unique));
    if (c->u_cap > 2 * want || 2 * c->u_cap < want) {
        DevBuf keys2, uid2;
        PhiDevGuard guard{{&keys2, &uid2}};                // error paths below
        PHICHK(phi_dev_ensure(c, keys2, want * 8));
        PHICHK(phi_dev_ensure(c, uid2, want * 4));
        phi_launch_fill_u64(c->stream, keys2.as<uint64_t>(), (int64_t)want, PHI_EMPTY_KEY);
        phi_launch_table_compact(c->stream, c->d_u_replist.as<int32_t>(), c->n_unique, c->d_rec_hash.as<uint64_t>(), c->n_rec,
                                 keys2.as<uint64_t>(), uid2.as<uint32_t>(), want - 1, c->d_rec_slot.as<uint32_t>(),
                                 (uint32_t *)scalar(c, S_ERR));
        HIPCHK(hipStreamSynchronize(c->stream));
        phi_dev_free(c->d_u_keys); phi_dev_free(c->d_u_uid); phi_dev_free(c->d_u_rep);
        c->d_u_keys = keys2; c->d_u_uid = uid2;
        keys2 = DevBuf{}; uid2 = DevBuf{};                 // ownership moved
        c->u_cap = want;
    } else {
        PHICHK(phi_dev_ensure(c, c->d_u_uid, c->u_cap * 4));
        phi_launch_slot_uid(c->stream, c->d_u_replist.as<int32_t>(), c->n_unique, c->d_rec_slot.as<uint32_t>(),
                            c->d_u_uid.as<uint32_t>());
    }
    return PHI_OK;
}

// ---- the GPU side of the index (walk-entry pass, classes, walk sketch, minimiser table) runs on its own host thread while
//      the calling thread builds the DP step stream: the calling thread needs the edge counts of the first pass, no more
static int gpu_thread(SetGraph &S)
{
    phi_ctx *c = S.c;
    // whatever happens, the host thread waiting for the edge counts is released
    struct PromiseGuard { std::promise<int> &p; bool done = false; ~PromiseGuard() { if (!done) p.set_value(PHI_ERR_DEVICE); } } pg{S.edges_promise};
    HIPCHK(hipSetDevice(c->device));
    PhiStageTimer tg("set_graph");
    PHICHK(S.uploads.get());                                   // (the graph arrays: on their way since before the validation)
    {
        const int rc = walk_entry_pass(S);
        S.edges_promise.set_value(rc);
        pg.done = true;
        if (rc) return rc;
        if (tg.on) tg.lap("[gpu thread] uploads + walk-entry pass");
    }
    if (S.walk_err[0]) return PHI_OK;                          // the main thread reports it; nothing below may index with such walks
    // ---- stage 1a on the GPU (ILP_index.cpp:559-573), de-duplicated: classes of walk entries with equal
    //      context, one sketch per class, the minimiser table from the class records (contexts.hip)
    HIPCHK(hipMemsetAsync(c->d_scalars.p, 0, S_N * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->d_stripes.p, 0, 2 * STRIPE_BYTES, c->stream));
    PHICHK(build_classes(c, S.n_vtx, S.n_walks, S.n_entries));
    c->h_kept = PhiAnchorSpan{}; c->h_dp = PhiAnchorSpan{}; c->anchors_host = false;
    if (tg.on) (void)hipStreamSynchronize(c->stream);
    tg.lap("[gpu thread] classes + class sketch");
    PHICHK(build_minimizer_table(c));
    PHICHK(build_read_table(c));
    PHICHK(build_kmer_table(c));
    // records of each walk ("Number of Minimizers", ILP_index.cpp:563) = sum over its entries of their class's records
    PHICHK(phi_dev_ensure(c, c->d_list2, (size_t)(S.n_walks + 1) * 8));
    HIPCHK(hipMemsetAsync(c->d_list2.p, 0, (size_t)(S.n_walks + 1) * 8, c->stream));
    phi_launch_walk_rec_counts(c->stream, c->d_ent_cls.as<int32_t>(), c->d_cls_rec_off.as<int32_t>(), c->d_walk_off.as<int64_t>(),
                               S.n_walks, S.n_entries, c->d_list2.as<unsigned long long>());
    c->h_n_minimizers.assign(S.n_walks, 0);
    HIPCHK(hipMemcpyAsync(c->h_n_minimizers.data(), c->d_list2.p, (size_t)S.n_walks * 8, hipMemcpyDeviceToHost, c->stream));
    // the hit vectors of both read generations
    PHICHK(phi_dev_ensure(c, c->d_hit, (size_t)(c->n_unique / 8 + 1) * 8));
    HIPCHK(hipMemsetAsync(c->d_hit.p, 0, (size_t)(c->n_unique / 8 + 1) * 8, c->stream));
    PHICHK(phi_dev_ensure(c, c->alt.hit, (size_t)(c->n_unique / 8 + 1) * 8));
    HIPCHK(hipMemsetAsync(c->alt.hit.p, 0, (size_t)(c->n_unique / 8 + 1) * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->alt.stripes.p, 0, 2 * STRIPE_BYTES, c->stream));
    HIPCHK(hipGetLastError());
    PHICHK(phi_sync_check(c));
    tg.lap("[gpu thread] walk sketch + table");
    return PHI_OK;
}

// ---- host copies of the graph, while the GPU thread uploads
// (each array on a thread of its own: at chromosome scale they are 0.45 GB of first-touched pages, 130 ms one after the other)
static void copy_graph_to_host(SetGraph &S)
{
    phi_ctx *c = S.c;
    std::thread t1([&]() { c->h_seq.assign(S.seq_concat, S.seq_concat + S.seq_off[S.n_vtx]); });
    std::thread t2([&]() { c->h_seq_off.assign(S.seq_off, S.seq_off + S.n_vtx + 1); });
    std::thread t3([&]() { c->h_adj_off.assign(S.adj_off, S.adj_off + S.n_vtx + 1); c->h_adj.assign(S.adj, S.adj + S.n_edges); });
    c->h_walk_off.assign(S.walk_off, S.walk_off + S.n_walks + 1);
    c->h_topo_rank.assign(S.topo_rank, S.topo_rank + S.n_vtx);
    t1.join(); t2.join(); t3.join();
}

// what the walk-entry pass on the GPU found wrong with the walks (after edges_future)
static int report_walk_errors(SetGraph &S)
{
    phi_ctx *c = S.c;
    const int32_t *walk_err = S.walk_err;
    if (walk_err[0] == 4) return phi_fail(c, PHI_ERR_WALK, "walk %d holds vertex %d out of range", walk_err[1], walk_err[2]);
    if (walk_err[0] == 1) return phi_fail(c, PHI_ERR_UNSUPPORTED, "walk %d passes through empty segment %d", walk_err[1], walk_err[2]);
    if (walk_err[0] == 2) return phi_fail(c, PHI_ERR_WALK, "walk %d steps %d->%d without a graph edge", walk_err[1], walk_err[2], walk_err[3]);
    if (walk_err[0] == 3) return phi_fail(c, PHI_ERR_UNSUPPORTED, "vertex %d has more than 254 out-edges", walk_err[2]);
    return PHI_OK;
}

// The first and the last vertex of every walk are all the host pass looks at of the walk entries: for host walks gathered
// here, once the entries are known to be in range (a few thousand ints), in the layout c->wtext.ends has for walks on the device.
static int refuse_interior_ends(SetGraph &S)
{
    if (S.dev_walks) S.walk_ends = S.c->wtext.ends.data();
    else {
        S.ends_own.resize((size_t)S.n_walks * 2);
        for (int32_t h = 0; h < S.n_walks; h++) {
            S.ends_own[(size_t)h * 2] = S.walk_vtx[S.walk_off[h]];
            S.ends_own[(size_t)h * 2 + 1] = S.walk_vtx[S.walk_off[h + 1] - 1];
        }
        S.walk_ends = S.ends_own.data();
    }
    bool start_interior = false, end_interior = false;
    for (int32_t h = 0; h < S.n_walks; h++) {
        if (S.indeg[(size_t)S.walk_ends[(size_t)h * 2]] > 0) start_interior = true;
        const int32_t last = S.walk_ends[(size_t)h * 2 + 1];
        if (S.adj_off[last + 1] > S.adj_off[last]) end_interior = true;
    }
    if (start_interior && end_interior)
        return phi_fail(S.c, PHI_ERR_UNSUPPORTED, "walks both start and end at interior vertices: the reference model "
                        "admits flow leak/spawn artefacts there (ILP_index.cpp:1330) that are not emulated");
    return PHI_OK;
}

// The DP step stream (dp_steps.h) on the host threads, then the compact stream's arrays on their way to the device.
static int build_step_stream(SetGraph &S)
{
    phi_ctx *c = S.c;
    PhiStageTimer &tm = S.tm;
    const PhiDpGraph g{S.n_vtx, S.n_walks, S.adj_off, S.adj, S.topo_rank, c->h_topo.data(), S.cnt_edge.data(), S.walk_ends};
    PhiDpSteps &st = S.steps;
    PhiHostError err;
    if (phi_dp_steps_dense(g, st, err)) return phi_fail(c, err.code, "%s", err.msg.c_str());
    tm.lap("  dense step records");
    c->dp_events = S.n_walks <= PHI_DP_EVENT_MAX_WALKS && !getenv("PHI_DP_DENSE");
    c->n_k = 0; c->n_ev = 0;
    if (c->dp_events) {
        if (phi_dp_steps_compact(g, st, err)) return phi_fail(c, err.code, "%s", err.msg.c_str());
        c->n_k = st.n_k;
        if (tm.on) {
            int64_t n_tops = 0, n_entry = 0;
            for (int32_t k = 0; k < c->n_k; k++) { n_tops += (st.k_rec[(size_t)k * 8] & PHI_DP_NEED_TOPS) != 0; n_entry += (st.k_rec[(size_t)k * 8] & PHI_DP_NEED_ENTRY) != 0; }
            fprintf(stderr, "[phi timing] set_graph: %d compact steps: %lld with TOPS, %lld with ENTRY, %lld pairs\n", c->n_k, (long long)n_tops, (long long)n_entry, (long long)st.n_pairs);
        }
        tm.lap("  compact records");
        phi_dp_steps_cuts(st);
        // (the context keeps these three; the stream's other vectors stay with S until the end of the call)
        c->h_cstep.swap(st.cstep); c->h_kstep.swap(st.kstep); c->h_k_cut_ok.swap(st.cut_ok);
        // (tried on a stream of this thread's own, so that these copies do not queue behind the GPU thread's kernels:
        //  0.8 ms slower -- the pageable copies of a second stream do not share the first one's staging)
        PHICHK(upload(c, c->d_k_rec, st.k_rec.data(), st.k_rec.size()));
        PHICHK(upload(c, c->d_k_in, st.k_in.data(), st.k_in.size()));
        PHICHK(upload(c, c->d_cvtx, st.cvtx.data(), st.cvtx.size()));
        // (no wait: a synchronisation here would also wait for whatever the GPU thread has queued on the stream; the
        //  vectors live until phi_sync_check at the end of the call)
    }
    return PHI_OK;
}

// ---- device copies of what the host pass made, and the events of every walk: its entries on the compact steps
static int late_uploads_and_events(SetGraph &S)
{
    phi_ctx *c = S.c;
    c->dp_dense_ready = S.want_masks;
    if (S.want_masks) {                                        // the every-vertex stream serves dp.hip only
        PHICHK(upload(c, c->d_st_rec, S.steps.st_rec.get(), (size_t)S.n_vtx * 8));
        PHICHK(upload(c, c->d_in_packed, S.steps.in_packed.data(), S.steps.in_packed.size()));
    }
    if (c->dp_events) {
        PHICHK(phi_dev_ensure(c, c->d_flags, (size_t)S.n_entries));
        phi_launch_event_flags(c->stream, c->d_walk_vtx.as<int32_t>(), S.n_entries, c->d_cvtx.as<int32_t>(), c->d_flags.as<uint8_t>());
        PHICHK(phi_compact(c, c->d_flags.as<uint8_t>(), S.n_entries, c->d_ev_e, &c->n_ev));
        // (event indices are 32-bit signed in the block tables and on the DP lanes; events are the entries on vertices where a
        //  recombination can enter or leave or a walk begins or ends: 18 % of the entries of a chromosome-scale graph)
        if (c->n_ev >= (int64_t)1 << 31) return phi_fail(c, PHI_ERR_UNSUPPORTED, "more than 2^31 walk entries on vertices with recombination edges");
        PHICHK(phi_dev_ensure(c, c->d_ev_off, (size_t)(S.n_walks + 1) * 8));
        phi_launch_event_off(c->stream, c->d_ev_e.as<phi_ent_t>(), c->n_ev, c->d_walk_off.as<int64_t>(), S.n_walks,
                             c->d_ev_off.as<int64_t>());
    }
    HIPCHK(hipGetLastError());
    PHICHK(phi_sync_check(c));
    if (S.tm.on) fprintf(stderr, "[phi timing] set_graph: %d vertices, %d compact steps, %lld entries, %lld events\n", S.n_vtx, c->n_k, (long long)S.n_entries, (long long)c->n_ev);
    return PHI_OK;
}

// a new graph: no reads yet
static void reset_read_state(phi_ctx *c)
{
    c->reads_bases = 0; c->reads_count = 0; c->spectrum_override = -1;
    c->spset.new_graph(); c->rlog.new_generation(); c->rlog.async_batches = false;   // (set_graph zeroed all scalars, the overflow counters among them)
    c->walks_on_device = false;                                // (consumed: a later phi_set_graph brings its own walks)
    c->rlog.nov_shift = phi_nov_shift(c->w);
    if (const char *e = getenv("PHI_NOV_SHIFT")) c->rlog.nov_shift = std::max(0, std::min(9, atoi(e)));   // tests: chunk logs of a few entries, so that ordinary reads spill into the overflow list
    c->alt.needs_clean = false;
}

// the body of phi_set_graph, and of phi_set_graph_chopped once the graph is chopped: the schedule of the stages above
int set_graph_impl(phi_ctx *c, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off, const int64_t *adj_off,
                   const int32_t *adj, int32_t n_walks, const int64_t *walk_off, const int32_t *walk_vtx,
                   const int32_t *topo_rank)
{
    if (!c) return PHI_ERR_INVALID;
    PHICHK(set_graph_check_args(c, n_vtx, seq_concat, seq_off, adj_off, adj, n_walks, walk_off, walk_vtx, topo_rank));
    SetGraph S(c, n_vtx, seq_concat, seq_off, adj_off, adj, n_walks, walk_off, walk_vtx, topo_rank);
    PhiStageTimer &tm = S.tm;
    start_pinning(S);
    PHICHK(set_graph_check_offsets(c, n_vtx, seq_off, adj_off, n_walks, walk_off));
    S.n_edges = adj_off[n_vtx]; S.n_entries = walk_off[n_walks];
    start_dp_buffers(S);
    c->n_vtx = n_vtx; c->n_walks = n_walks; c->n_entries = S.n_entries;
    start_uploads(S);
    PHICHK(validate_topology(S));
    tm.lap("validate graph, copies");
    if (n_walks > PHI_DP_MAX_WALKS) return phi_fail(c, PHI_ERR_UNSUPPORTED, "more than %d walks", PHI_DP_MAX_WALKS);
    c->dp_nw = phi_dp_num_waves(n_walks);
    PHICHK(start_host_walk_copy(S));
    S.cnt_edge.assign((size_t)std::max<int64_t>(S.n_edges, 1), 0);
    // the every-vertex stream of dp.hip: beyond 256 walks, when asked for, and as the fallback of the
    // four-wave event kernel (129-256 walks) whose per-lane queues are shallower than the worst case
    S.want_masks = !(n_walks <= PHI_DP_EVENT_SAFE_WALKS && !getenv("PHI_DP_DENSE"));
    S.gpu = std::async(std::launch::async, [&S]() { return gpu_thread(S); });
    // ---- meanwhile, on this thread (every return from here on waits for the GPU thread: ~SetGraph)
    copy_graph_to_host(S);
    tm.lap("host copies");
    PHICHK(S.edges_future.get());                              // the edge counts and the walk error of the walk-entry pass
    PHICHK(report_walk_errors(S));
    tm.lap("walk entries: pass on the GPU");
    PHICHK(refuse_interior_ends(S));
    PHICHK(build_step_stream(S));
    tm.lap("DP step stream");
    // ---- the GPU side has been running meanwhile
    PHICHK(S.gpu.get());
    tm.lap("wait for the GPU thread");
    PHICHK(late_uploads_and_events(S));
    tm.lap("late uploads + event list");
    reset_read_state(c);
    stage_release(c);
    if (c->dp_alloc_future.valid()) {
        PHICHK(c->dp_alloc_future.get());
        tm.lap("wait for the DP buffers");
    }
    c->have_graph = true;
    return PHI_OK;
}

extern "C" int phi_set_graph(phi_ctx *c, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off, const int64_t *adj_off,
                             const int32_t *adj, int32_t n_walks, const int64_t *walk_off, const int32_t *walk_vtx,
                             const int32_t *topo_rank)
{
    return set_graph_impl(c, n_vtx, seq_concat, seq_off, adj_off, adj, n_walks, walk_off, walk_vtx, topo_rank);
}

// ---- phi_scout_graph: a second schedule over the stages above, for graphs of more walks than the DP takes.  It runs the
// checks, the uploads, validate_topology and the GPU thread as it is (walk-entry pass without masks, classes, minimiser
// table, read table, per-walk minimiser counts, hit vectors), then reset_read_state; it leaves out everything that serves
// the DP alone -- start_pinning, start_dp_buffers, the host copy of the walk entries, refuse_interior_ends (a refusal of the
// DP's model), build_step_stream, late_uploads_and_events.  Nothing of the index holds a walk id in a fixed-size field:
// the classes, their records and both tables are keyed by context and hash, the per-walk counts are 64-bit sums over
// contiguous entry ranges, and the walk-entry pass without masks only searches walk_off.  The limit of 65 535 walks is the
// one panel_score.hip's matrix and the choice work with.
// The full entries stay in d_walk_vtx (the index reads them) and count as retained: panel.full_off names them, and
// phi_set_graph_panel(walk_vtx = NULL) with the same offsets moves them to panel.d_full before it starts.
extern "C" int phi_scout_graph(phi_ctx *c, int32_t n_vtx, const char *seq_concat, const int64_t *seq_off, const int64_t *adj_off,
                               const int32_t *adj, int32_t n_walks, const int64_t *walk_off, const int32_t *walk_vtx,
                               const int32_t *topo_rank)
{
    if (!c) return PHI_ERR_INVALID;
    if (n_vtx <= 0 || n_walks <= 0 || !seq_concat || !seq_off || !adj_off || !walk_off || !topo_rank)
        return phi_fail(c, PHI_ERR_INVALID, "phi_scout_graph: null pointer or empty graph");
    if (adj_off[n_vtx] > 0 && !adj) return phi_fail(c, PHI_ERR_INVALID, "phi_scout_graph: adj is null");
    if (n_walks > PHI_SCOUT_MAX_WALKS) return phi_fail(c, PHI_ERR_UNSUPPORTED, "phi_scout_graph: more than %d walks", PHI_SCOUT_MAX_WALKS);
    HIPCHK(hipSetDevice(c->device));
    if (c->ipc || c->peers || c->comm) return phi_fail(c, PHI_ERR_STATE, "phi_scout_graph on a context that exchanges with others (a scout graph is one GPU's: leave the group first)");
    PHICHK(set_graph_check_offsets(c, n_vtx, seq_off, adj_off, n_walks, walk_off));
    auto &P = c->panel;
    enum { FROM_HOST, IN_PLACE, FROM_RETAINED } from = FROM_HOST;
    if (!walk_vtx) {
        const bool same_off = P.full_off.size() == (size_t)n_walks + 1 && std::equal(P.full_off.begin(), P.full_off.end(), walk_off);
        if (c->walks_on_device && c->walks_on_device_n == walk_off[n_walks] && (int32_t)(c->wtext.ends.size() / 2) == n_walks) from = IN_PLACE;
        else if (c->scout.on && same_off) from = IN_PLACE;
        else if (P.d_full.p && same_off) from = FROM_RETAINED;
        else return phi_fail(c, PHI_ERR_STATE, "phi_scout_graph without walk_vtx: these walks are neither freshly resolved on this context nor retained by an earlier panel or scout");
    }
    c->have_graph = false;
    c->chop.on = false;
    P.on = false;
    phi_scout_end(c);
    c->solved = false;
    c->calls.have = false;
    phi_ladder_drop(c);
    // (on failure below the context holds no graph and retains nothing)
    if (from == FROM_RETAINED) { phi_dev_free(c->d_walk_vtx); std::swap(c->d_walk_vtx, P.d_full); }
    else phi_dev_free(P.d_full);
    P.full_off.clear();

    SetGraph S(c, n_vtx, seq_concat, seq_off, adj_off, adj, n_walks, walk_off, walk_vtx, topo_rank);
    PhiStageTimer &tm = S.tm;
    S.n_edges = adj_off[n_vtx]; S.n_entries = walk_off[n_walks];
    if (c->dp_alloc_future.valid()) (void)c->dp_alloc_future.get();
    c->n_vtx = n_vtx; c->n_walks = n_walks; c->n_entries = S.n_entries;
    start_uploads(S);
    PHICHK(validate_topology(S));
    tm.lap("scout: validate graph, copies");
    c->dp_nw = 1;                                              // (no masks: the walk-entry pass does not look at it)
    if (!c->h_walk_vtx.resize(0)) return phi_fail(c, PHI_ERR_NOMEM, "host allocation failed");
    S.cnt_edge.assign((size_t)std::max<int64_t>(S.n_edges, 1), 0);
    S.want_masks = false;
    S.gpu = std::async(std::launch::async, [&S]() { return gpu_thread(S); });
    copy_graph_to_host(S);                                     // (the per-vertex arrays and walk_off: phi_walk_minimizers, phi_walk_sharing)
    PHICHK(S.edges_future.get());
    PHICHK(report_walk_errors(S));
    PHICHK(S.gpu.get());
    tm.lap("scout: index on the GPU thread");
    c->dp_events = false; c->dp_dense_ready = false; c->n_k = 0; c->n_ev = 0;
    reset_read_state(c);
    stage_release(c);
    P.full_off.assign(walk_off, walk_off + n_walks + 1);
    c->scout.on = true;
    c->have_graph = true;
    return PHI_OK;
}
