// ladder.hip -- a ladder of coverages from ONE read set: the set is collected on the device, partitioned into nested bands
// by a per-read draw, and scored band by band (include/phi_amd.h phi_reads_collect_*, phi_ladder_*).
//
// The reference's evaluation cuts every sample's FASTQ into seven files with `seqkit sample` (data/preprocess.py:83-107) and
// starts one PHI process per (sample, coverage) pair (data/run_batch_4.py:38-58): 33.6x of bases uploaded and scored for a
// 15x read set.  Read state is order-independent (the hit vector is a running OR, the spectrum a set, the counters sums),
// so with NESTED samples every base is uploaded and scored once: score the reads a level adds, solve, score the next band.
//
// The rule: read i (ordinal, 64-bit) draws u_i = the upper 32 bits of output i + 1 of SplitMix64(seed); its band is the
// smallest j with u_i < t_j, t_j = min(2^32, floor(f_j 2^32)); none: dropped.  Level j = bands 0..j.
//
// The partition is a stable counting sort of the reads by band, in four launches:
//     count    one lane per read: draw, band, length; per workgroup the reads and bases of every band, written BAND-MAJOR
//     scan     64-bit exclusive scan over (band, workgroup) -- band-major, so a read's place is behind every read of a lower
//              band and behind the same band's reads of earlier workgroups: stable -- and the table of band starts
//     scatter  the band recomputed; the rank among the workgroup's reads of the same band from ballots and mbcnt, a prefix of
//              their lengths: every kept read gets its place, its source and its destination offset
//     copy     one lane per 16 destination bytes: finds its read by a search in the band's offsets (a division for a store
//              of one read length), assembles the 16 bytes from aligned source dwords with a byte funnel shift and stores
//              them at once; a chunk that crosses a read's end, or the band's, goes byte by byte
// Every band's bases start on a 256-byte border (the read kernels load 16 aligned bytes per lane), its offsets start at 0.
// A store of one read length keeps that property per band: phi_ladder_advance hands such a band over WITHOUT offsets, which
// is what selects the fixed-geometry window kernel for 150-bp reads.
// Bound: HBM.  Per read 8 bytes of offsets twice, 24 bytes of lists; per kept base one byte read and one written.
#include <math.h>
#include <string.h>
#include "phi_ctx.h"
#include "phi_wave.h"

#define LAD_TPB 256
#define LAD_MAXL PHI_LADDER_MAX_LEVELS
#define LAD_ALIGN 256
// the table of band starts the scan leaves: reads before band b, bases before it, where its bases start in the plan
#define LAD_TAB_R 0
#define LAD_TAB_B (LAD_MAXL + 1)
#define LAD_TAB_P (2 * (LAD_MAXL + 1))
#define LAD_TAB_N (3 * (LAD_MAXL + 1))

namespace {

struct LadThr { uint64_t t[LAD_MAXL]; };       // thresholds; beyond the last level: never reached

__device__ __forceinline__ uint32_t lad_draw(uint64_t seed, uint64_t ordinal)
{
    uint64_t z = seed + (ordinal + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z >> 32);
}

// thresholds ascend: the smallest j with u < t_j = the number of j with u >= t_j (n_levels: dropped)
__device__ __forceinline__ int lad_band(uint32_t u, const LadThr &T)
{
    int b = 0;
#pragma unroll
    for (int j = 0; j < LAD_MAXL; j++) b += (uint64_t)u >= T.t[j];
    return b;
}

// the store's offsets of one batch: off[r] = base + (the batch's own offset of read r, or r * uniform_len), r = 0 .. n;
// kept inside [base, base + n_bases] whatever the batch's offsets say
__global__ void __launch_bounds__(LAD_TPB) ladder_append_kernel(int64_t *__restrict__ off, const int64_t *__restrict__ src, int64_t uniform_len,
                                                                int64_t n, int64_t base, int64_t n_bases)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += stride) {
        int64_t v = src ? src[r] : r * uniform_len;
        v = v < 0 ? 0 : (v > n_bases ? n_bases : v);
        off[r] = base + v;
    }
}

__global__ void __launch_bounds__(LAD_TPB) ladder_count_kernel(const int64_t *__restrict__ off, int64_t n, uint64_t seed, uint64_t ord0, LadThr T,
                                                               int L, int64_t nwg, int64_t *__restrict__ wg_reads, int64_t *__restrict__ wg_bases)
{
    __shared__ unsigned long long s_r[LAD_MAXL], s_b[LAD_MAXL];
    const int tid = threadIdx.x;
    if (tid < LAD_MAXL) { s_r[tid] = 0; s_b[tid] = 0; }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * LAD_TPB + tid;
    if (i < n) {
        const int b = lad_band(lad_draw(seed, ord0 + (uint64_t)i), T);
        if (b < L) {
            const int64_t len = max((int64_t)0, off[i + 1] - off[i]);
            atomicAdd(&s_r[b], 1ull);
            atomicAdd(&s_b[b], (unsigned long long)len);
        }
    }
    __syncthreads();
    if (tid < L) {
        wg_reads[(int64_t)tid * nwg + blockIdx.x] = (int64_t)s_r[tid];
        wg_bases[(int64_t)tid * nwg + blockIdx.x] = (int64_t)s_b[tid];
    }
}

// a[0, M), b[0, M) -> their exclusive prefix sums, in place (one workgroup, a tile of 1024 items a turn), and the table
__global__ void __launch_bounds__(1024) ladder_scan_kernel(int64_t *__restrict__ a, int64_t *__restrict__ b, int64_t M, int64_t nwg, int L,
                                                           int64_t *__restrict__ tab)
{
    __shared__ long long s_a[16], s_b[16], s_R[LAD_MAXL + 1], s_B[LAD_MAXL + 1];
    const int tid = threadIdx.x;
    long long ca = 0, cb = 0;
    for (int64_t t0 = 0; t0 < M; t0 += 1024) {
        const int64_t i = t0 + tid;
        const long long va = i < M ? (long long)a[i] : 0, vb = i < M ? (long long)b[i] : 0;
        long long ta, tb;
        const long long pa = phi_block_excl_scan<16>(va, s_a, &ta), pb = phi_block_excl_scan<16>(vb, s_b, &tb);
        if (i < M) {
            const long long ea = ca + pa, eb = cb + pb;
            a[i] = ea; b[i] = eb;
            if (i % nwg == 0) { s_R[i / nwg] = ea; s_B[i / nwg] = eb; }     // the first workgroup of a band: where the band starts
        }
        ca += ta; cb += tb;
        __syncthreads();
    }
    if (tid == 0) {
        s_R[L] = ca; s_B[L] = cb;
        long long p = 0;
        for (int j = 0; j <= L; j++) {
            tab[LAD_TAB_R + j] = s_R[j];
            tab[LAD_TAB_B + j] = s_B[j];
            tab[LAD_TAB_P + j] = p;
            if (j < L) p = (p + (s_B[j + 1] - s_B[j]) + LAD_ALIGN - 1) / LAD_ALIGN * LAD_ALIGN;
        }
    }
}

__global__ void __launch_bounds__(LAD_TPB) ladder_scatter_kernel(const int64_t *__restrict__ off, int64_t n, uint64_t seed, uint64_t ord0, LadThr T,
                                                                 int L, int64_t nwg, const int64_t *__restrict__ wg_reads,
                                                                 const int64_t *__restrict__ wg_bases, const int64_t *__restrict__ tab,
                                                                 int64_t *__restrict__ poff, int64_t *__restrict__ pidx, int64_t *__restrict__ psrc)
{
    __shared__ long long s_wr[LAD_TPB / 64][LAD_MAXL], s_wb[LAD_TPB / 64][LAD_MAXL];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * LAD_TPB + tid;
    int band = L;
    long long len = 0, src = 0;
    if (i < n) {
        band = min(L, lad_band(lad_draw(seed, ord0 + (uint64_t)i), T));
        src = off[i];
        len = max((long long)0, (long long)(off[i + 1] - src));
    }
    long long my_rank = 0, my_pre = 0;
    for (int j = 0; j < L; j++) {
        const bool mine = band == j;
        const unsigned long long m = __ballot(mine);
        long long x = 0;
        if (m) {                                              // (wave-uniform)
            x = phi_wave_incl_scan(mine ? len : 0);
            if (mine) {
                my_rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                my_pre = x - len;
            }
        }
        if (lane == 63) { s_wr[wv][j] = __popcll(m); s_wb[wv][j] = x; }
    }
    __syncthreads();
    if (band < L) {
        long long r = my_rank, d = my_pre;
        for (int v = 0; v < wv; v++) { r += s_wr[v][band]; d += s_wb[v][band]; }
        const int64_t R0 = tab[LAD_TAB_R + band], R1 = tab[LAD_TAB_R + band + 1];
        r += wg_reads[(int64_t)band * nwg + blockIdx.x] - R0;
        d += wg_bases[(int64_t)band * nwg + blockIdx.x] - tab[LAD_TAB_B + band];
        const int64_t slot = R0 + r;
        pidx[slot] = i;
        psrc[slot] = src;
        poff[slot + band] = d;                                // (band j's run of reads + 1 offsets starts at R0 + j)
        if (r == R1 - R0 - 1) poff[slot + band + 1] = d + len;
    }
}

__global__ void __launch_bounds__(LAD_TPB) ladder_copy_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int64_t *__restrict__ tab,
                                                              const int64_t *__restrict__ poff, const int64_t *__restrict__ psrc, int L, int64_t one_len)
{
    const int64_t p = ((int64_t)blockIdx.x * LAD_TPB + threadIdx.x) * 16;
    if (p >= tab[LAD_TAB_P + L]) return;
    int b = 0;
    for (int j = 1; j < L; j++) b = p >= tab[LAD_TAB_P + j] ? j : b;
    const int64_t x = p - tab[LAD_TAB_P + b];
    const int64_t nb = tab[LAD_TAB_B + b + 1] - tab[LAD_TAB_B + b];
    if (x >= nb) return;                                      // (the padding behind a band)
    const int64_t R0 = tab[LAD_TAB_R + b], nr = tab[LAD_TAB_R + b + 1] - R0;
    const int64_t *__restrict__ o = poff + R0 + b;
    const int64_t *__restrict__ so = psrc + R0;
    int64_t q, o0, o1;
    if (one_len > 0) {
        q = (x >> 32) == 0 && (one_len >> 32) == 0 ? (int64_t)((uint32_t)x / (uint32_t)one_len) : x / one_len;
        o0 = q * one_len; o1 = o0 + one_len;
    } else {
        // the last read that starts at or before x (empty reads share their start with the read behind them: never chosen)
        int64_t lo = 0, hi = nr;
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (o[mid] <= x) lo = mid; else hi = mid;
        }
        q = lo; o0 = o[q]; o1 = o[q + 1];
    }
    uint8_t *out = dst + p;
    if (x + 16 <= o1) {
        const int64_t s = so[q] + (x - o0);
        const uint32_t sh = (uint32_t)s & 3u;
        const uint32_t *__restrict__ w = reinterpret_cast<const uint32_t *>(src + (s - sh));
        const uint32_t d0 = w[0], d1 = w[1], d2 = w[2], d3 = w[3];
        const uint32_t d4 = sh ? w[4] : 0u;                   // (the store is padded: the dword behind the last base exists)
        *reinterpret_cast<uint4 *>(out) = make_uint4(__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                                                     __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh));
    } else {
        int64_t sb = so[q];
        for (int t = 0; t < 16; t++) {
            const int64_t xb = x + t;
            if (xb >= nb) break;
            while (xb >= o1 && q + 1 < nr) { q++; o0 = o1; o1 = one_len > 0 ? o0 + one_len : o[q + 1]; sb = so[q]; }
            out[t] = src[sb + (xb - o0)];
        }
    }
}

}  // namespace

int phi_ladder_collect(phi_ctx *c, const void *d_bases, const void *d_read_off, int64_t n_reads, int64_t n_bases)
{
    auto &S = c->ladder;
    if (n_reads == 0) return PHI_OK;
    int64_t len = 0;
    if (!d_read_off) {
        if (n_bases % n_reads) return phi_fail(c, PHI_ERR_INVALID, "phi_add_reads_device without offsets: %lld bases are not %lld reads of one length", (long long)n_bases, (long long)n_reads);
        len = n_bases / n_reads;
    }
    HIPCHK(hipSetDevice(c->device));
    // (16 bytes behind the last base: the copy kernel reads whole aligned dwords)
    const size_t need_b = (size_t)(S.n_bases + n_bases) + 64, need_o = (size_t)(S.n_reads + n_reads + 1) * 8;
    if (need_b > S.d_bases.cap || !S.d_bases.p) PHICHK(phi_dev_grow_keep(c, S.d_bases, std::max(need_b, 2 * S.d_bases.cap), (size_t)S.n_bases));
    if (need_o > S.d_off.cap || !S.d_off.p) PHICHK(phi_dev_grow_keep(c, S.d_off, std::max(need_o, 2 * S.d_off.cap), (size_t)(S.n_reads + 1) * 8));
    if (n_bases) HIPCHK(hipMemcpyAsync(S.d_bases.as<uint8_t>() + S.n_bases, d_bases, (size_t)n_bases, hipMemcpyDeviceToDevice, c->stream));
    const unsigned nb = (unsigned)std::min<int64_t>((n_reads + 1 + LAD_TPB - 1) / LAD_TPB, 4096);
    hipLaunchKernelGGL(ladder_append_kernel, dim3(nb), dim3(LAD_TPB), 0, c->stream, S.d_off.as<int64_t>() + S.n_reads, (const int64_t *)d_read_off, len,
                       n_reads, S.n_bases, n_bases);
    HIPCHK(hipGetLastError());
    if (d_read_off) S.one_len = -2;
    else if (S.one_len == -1) S.one_len = len;
    else if (S.one_len != len) S.one_len = -2;
    S.n_reads += n_reads; S.n_bases += n_bases;
    return PHI_OK;
}

static void ladder_drop_plan(phi_ctx *c)
{
    auto &S = c->ladder;
    for (DevBuf *b : {&S.d_pbases, &S.d_poff, &S.d_pidx, &S.d_psrc, &S.d_wg, &S.d_tab}) phi_dev_free(*b);
    S.have_plan = false; S.scored = 0;
}

void phi_ladder_drop(phi_ctx *c)
{
    auto &S = c->ladder;
    if (!S.d_bases.p && !S.d_off.p && !S.d_pbases.p && !S.d_tab.p && !S.collecting && !S.have_store) return;
    (void)hipStreamSynchronize(c->stream);
    ladder_drop_plan(c);
    phi_dev_free(S.d_bases); phi_dev_free(S.d_off);
    S.collecting = S.have_store = false;
    S.n_reads = S.n_bases = 0; S.one_len = -1;
}

// PHI_PANEL_KEEP_READS (panel.hip): the finished store leaves the context -- without its plan, whose bands belong to nothing
// after the call -- so that the phi_ladder_drop of the set-graph stages finds nothing, and comes back once the panel is set
void phi_ladder_detach(phi_ctx *c, phi_ctx::PhiLadder &out)
{
    auto &S = c->ladder;
    out = phi_ctx::PhiLadder{};
    if (!S.have_store || S.collecting) return;
    (void)hipStreamSynchronize(c->stream);
    ladder_drop_plan(c);
    std::swap(out, S);
}

void phi_ladder_attach(phi_ctx *c, phi_ctx::PhiLadder &in)
{
    if (!in.have_store) return;
    phi_ladder_drop(c);
    std::swap(c->ladder, in);
}

extern "C" {

int phi_reads_collect_begin(phi_ctx *c, int64_t first_ordinal)
{
    if (!c) return PHI_ERR_INVALID;
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_reads_collect_begin before phi_set_graph");
    auto &S = c->ladder;
    if (S.collecting) return phi_fail(c, PHI_ERR_STATE, "phi_reads_collect_begin: already collecting");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    ladder_drop_plan(c);                                      // (a new store: the old one's bands go; its buffers are reused)
    S.n_reads = S.n_bases = 0; S.one_len = -1; S.have_store = false;
    S.first_ordinal = first_ordinal;
    S.collecting = true;
    return PHI_OK;
}

int phi_reads_collect_end(phi_ctx *c, int64_t *n_reads, int64_t *n_bases)
{
    if (!c) return PHI_ERR_INVALID;
    auto &S = c->ladder;
    if (!S.collecting) return phi_fail(c, PHI_ERR_STATE, "phi_reads_collect_end without phi_reads_collect_begin");
    HIPCHK(hipSetDevice(c->device));
    S.collecting = false; S.have_store = true;
    PHICHK(phi_sync_check(c));                                // (the batches' buffers are the caller's again)
    if (n_reads) *n_reads = S.n_reads;
    if (n_bases) *n_bases = S.n_bases;
    return PHI_OK;
}

int phi_reads_collect_release(phi_ctx *c)
{
    if (!c) return PHI_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    phi_ladder_drop(c);
    return PHI_OK;
}

int phi_reads_collect_score(phi_ctx *c)
{
    if (!c) return PHI_ERR_INVALID;
    auto &S = c->ladder;
    if (S.collecting) return phi_fail(c, PHI_ERR_STATE, "phi_reads_collect_score while collecting: phi_reads_collect_end first");
    if (!S.have_store) return phi_fail(c, PHI_ERR_STATE, "phi_reads_collect_score without a collected read set");
    if (!c->have_graph) return phi_fail(c, PHI_ERR_STATE, "phi_reads_collect_score before phi_set_graph");
    HIPCHK(hipSetDevice(c->device));
    if (S.n_reads == 0) return PHI_OK;
    // the store as one resident batch, where it lies; one read length: no offsets, as phi_ladder_advance hands its bands over
    const void *d_off = S.one_len > 0 && S.one_len <= 0x7FFFFFFF ? nullptr : S.d_off.p;
    return phi_score_resident_batch(c, S.d_bases.p, d_off, S.n_reads, S.n_bases);
}

int phi_ladder_plan(phi_ctx *c, uint64_t seed, const double *fractions, int32_t n_levels, phi_ladder_info *info)
{
    if (!c) return PHI_ERR_INVALID;
    auto &S = c->ladder;
    if (S.collecting) return phi_fail(c, PHI_ERR_STATE, "phi_ladder_plan while collecting: phi_reads_collect_end first");
    if (!S.have_store) return phi_fail(c, PHI_ERR_STATE, "phi_ladder_plan without a collected read set");
    if (!fractions || n_levels < 1 || n_levels > LAD_MAXL) return phi_fail(c, PHI_ERR_INVALID, "phi_ladder_plan: 1 to %d levels", LAD_MAXL);
    LadThr T;
    phi_ladder_info I{};
    const int L = n_levels;
    for (int j = 0; j < LAD_MAXL; j++) T.t[j] = ~0ull;
    for (int j = 0; j < L; j++) {
        const double f = fractions[j];
        if (!(f >= 0.0) || (j > 0 && f < fractions[j - 1])) return phi_fail(c, PHI_ERR_INVALID, "phi_ladder_plan: fraction %d is negative or below the one before it", j);
        T.t[j] = f >= 1.0 ? (uint64_t)1 << 32 : (uint64_t)floor(f * 4294967296.0);
        I.threshold[j] = T.t[j];
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    ladder_drop_plan(c);
    const int64_t N = S.n_reads, NB = S.n_bases;
    I.n_levels = L; I.n_reads = N; I.n_bases = NB;
    I.one_length = S.one_len > 0 && S.one_len <= 0x7FFFFFFF ? (int32_t)S.one_len : 0;
    memset(S.band_read0, 0, sizeof S.band_read0);
    memset(S.band_pos, 0, sizeof S.band_pos);
    if (N > 0) {
        const int64_t nwg = (N + LAD_TPB - 1) / LAD_TPB, M = nwg * L;
        if (nwg > 0x7FFFFFFF) return phi_fail(c, PHI_ERR_UNSUPPORTED, "phi_ladder_plan: more than 2^39 reads");
        const int64_t n_chunks = (NB + (int64_t)LAD_ALIGN * L) / 16 + 1, copy_blocks = (n_chunks + LAD_TPB - 1) / LAD_TPB;
        if (copy_blocks > 0x7FFFFFFF) return phi_fail(c, PHI_ERR_UNSUPPORTED, "phi_ladder_plan: more than 2^43 bases");
        PHICHK(phi_dev_ensure(c, S.d_wg, (size_t)M * 16));
        PHICHK(phi_dev_ensure(c, S.d_tab, LAD_TAB_N * 8));
        PHICHK(phi_dev_ensure(c, S.d_poff, (size_t)(N + L) * 8));
        PHICHK(phi_dev_ensure(c, S.d_pidx, (size_t)N * 8));
        PHICHK(phi_dev_ensure(c, S.d_psrc, (size_t)N * 8));
        PHICHK(phi_dev_ensure(c, S.d_pbases, (size_t)(n_chunks * 16) + 64));
        int64_t *wg_r = S.d_wg.as<int64_t>(), *wg_b = wg_r + M, *tab = S.d_tab.as<int64_t>();
        const int64_t *off = S.d_off.as<int64_t>();
        const uint64_t ord0 = (uint64_t)S.first_ordinal;
        hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int i = 0; i < 5; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
        for (int i = 0; i < 5; i++) HIPCHK(hipEventCreate(&ev[i]));
        HIPCHK(hipMemsetAsync(S.d_poff.p, 0, (size_t)(N + L) * 8, c->stream));       // (an empty band's single offset)
        HIPCHK(hipEventRecord(ev[0], c->stream));
        hipLaunchKernelGGL(ladder_count_kernel, dim3((unsigned)nwg), dim3(LAD_TPB), 0, c->stream, off, N, seed, ord0, T, L, nwg, wg_r, wg_b);
        HIPCHK(hipEventRecord(ev[1], c->stream));
        hipLaunchKernelGGL(ladder_scan_kernel, dim3(1), dim3(1024), 0, c->stream, wg_r, wg_b, M, nwg, L, tab);
        HIPCHK(hipEventRecord(ev[2], c->stream));
        hipLaunchKernelGGL(ladder_scatter_kernel, dim3((unsigned)nwg), dim3(LAD_TPB), 0, c->stream, off, N, seed, ord0, T, L, nwg, (const int64_t *)wg_r,
                           (const int64_t *)wg_b, (const int64_t *)tab, S.d_poff.as<int64_t>(), S.d_pidx.as<int64_t>(), S.d_psrc.as<int64_t>());
        HIPCHK(hipEventRecord(ev[3], c->stream));
        hipLaunchKernelGGL(ladder_copy_kernel, dim3((unsigned)copy_blocks), dim3(LAD_TPB), 0, c->stream, S.d_bases.as<uint8_t>(), S.d_pbases.as<uint8_t>(),
                           (const int64_t *)tab, (const int64_t *)S.d_poff.p, (const int64_t *)S.d_psrc.p, L, (int64_t)I.one_length);
        HIPCHK(hipEventRecord(ev[4], c->stream));
        HIPCHK(hipGetLastError());
        int64_t h_tab[LAD_TAB_N];
        HIPCHK(phi_copy_sync(c, h_tab, tab, sizeof h_tab, hipMemcpyDeviceToHost));
        float ms[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < 4; i++) HIPCHK(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
        I.count_gpu_ms = ms[0]; I.scan_gpu_ms = ms[1]; I.scatter_gpu_ms = ms[2]; I.copy_gpu_ms = ms[3];
        for (int j = 0; j <= L; j++) { S.band_read0[j] = h_tab[LAD_TAB_R + j]; S.band_pos[j] = h_tab[LAD_TAB_P + j]; }
        for (int j = 0; j < L; j++) {
            I.band_reads[j] = h_tab[LAD_TAB_R + j + 1] - h_tab[LAD_TAB_R + j];
            I.band_bases[j] = h_tab[LAD_TAB_B + j + 1] - h_tab[LAD_TAB_B + j];
        }
        I.n_kept_reads = h_tab[LAD_TAB_R + L]; I.n_kept_bases = h_tab[LAD_TAB_B + L];
    }
    S.info = I;
    S.have_plan = true; S.scored = 0;
    if (info) *info = I;
    return PHI_OK;
}

int phi_ladder_advance(phi_ctx *c, int32_t level)
{
    if (!c) return PHI_ERR_INVALID;
    auto &S = c->ladder;
    if (!S.have_plan) return phi_fail(c, PHI_ERR_STATE, "phi_ladder_advance before phi_ladder_plan");
    if (level < 0 || level >= S.info.n_levels) return phi_fail(c, PHI_ERR_INVALID, "phi_ladder_advance: level %d of %d", level, S.info.n_levels);
    if (level + 1 < S.scored) return phi_fail(c, PHI_ERR_STATE, "phi_ladder_advance: level %d is below level %d, scored already (phi_reset_reads rewinds)", level, S.scored - 1);
    HIPCHK(hipSetDevice(c->device));
    for (int b = S.scored; b <= level; b++) {
        const int64_t nr = S.info.band_reads[b], nb = S.info.band_bases[b];
        if (nr > 0) {
            // a store of one read length: no offsets (the read kernels compute the read starts; 150-bp reads take the fixed-geometry kernel)
            const void *d_off = S.info.one_length > 0 ? nullptr : (const void *)(S.d_poff.as<int64_t>() + S.band_read0[b] + b);
            PHICHK(phi_score_resident_batch(c, S.d_pbases.as<uint8_t>() + S.band_pos[b], d_off, nr, nb));
        }
        S.scored = b + 1;
    }
    return PHI_OK;
}

int phi_ladder_band(phi_ctx *c, int32_t band, int64_t *ordinals_out, int64_t cap, int64_t *n, char *bases_out, int64_t bases_cap,
                    int64_t *offsets_out, int64_t *n_bases)
{
    if (!c) return PHI_ERR_INVALID;
    auto &S = c->ladder;
    if (!S.have_plan) return phi_fail(c, PHI_ERR_STATE, "phi_ladder_band before phi_ladder_plan");
    if (band < 0 || band >= S.info.n_levels) return phi_fail(c, PHI_ERR_INVALID, "phi_ladder_band: band %d of %d", band, S.info.n_levels);
    const int64_t nr = S.info.band_reads[band], nb = S.info.band_bases[band];
    if (n) *n = nr;
    if (n_bases) *n_bases = nb;
    HIPCHK(hipSetDevice(c->device));
    if (ordinals_out && cap >= nr && nr > 0) {
        HIPCHK(phi_copy_sync(c, ordinals_out, S.d_pidx.as<int64_t>() + S.band_read0[band], (size_t)nr * 8, hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < nr; r++) ordinals_out[r] = (int64_t)((uint64_t)ordinals_out[r] + (uint64_t)S.first_ordinal);
    }
    if (offsets_out && cap >= nr) {
        if (S.n_reads > 0) HIPCHK(phi_copy_sync(c, offsets_out, S.d_poff.as<int64_t>() + S.band_read0[band] + band, (size_t)(nr + 1) * 8, hipMemcpyDeviceToHost));
        else offsets_out[0] = 0;
    }
    if (bases_out && bases_cap >= nb && nb > 0)
        HIPCHK(phi_copy_sync(c, bases_out, S.d_pbases.as<uint8_t>() + S.band_pos[band], (size_t)nb, hipMemcpyDeviceToHost));
    return PHI_OK;
}

}  // extern "C"
