// gfa_text.hip -- a gzip GFA inflated on the device and split there: the walk fields of its W-lines stay in HBM, in the tile
// layout phi_walk_text_resolve reads, and only the rest of the text -- S-lines, L-lines, W-line heads -- goes to the host.
//
// At chromosome scale the W-lines are the file (config 5: 10.4 of 10.9 GB).  phi_inflate_to_device (inflate.hip) leaves the
// text in device memory; three kernels then find the walk fields with the host reader's own line rules (gfa_reader.cpp
// scan_slice / split_tabs), so that both sides agree on every line:
//   lines    split at '\n'; one '\r' before the line's end is not part of it; the last line may lack its '\n'
//   W-line   at least 3 bytes, byte 0 'W', byte 1 '\t'; a WALK when it holds at least 6 tabs; its walk field is everything
//            after the 6th tab up to the line's end, tags included (walk_text.hip stops at a tab inside it)
// Kernels:
//   scan     one workgroup per 64-KB tile, 16 bytes per lane: the tile's first '\n', and every "\nW\t" (and a text that
//            starts with "W\t") appended to a list of CANDIDATE line starts, one atomic per wave
//   line     one wave per candidate: its line's end (the next '\n' inside its tile, else the first tile after it that holds
//            one: 64 tiles per step of the wave) and its 6th tab, bounded by that end
//   copy     every walk field to the tile layout of phi_walk_text_upload (each walk on a 4-KB tile boundary), 16 bytes per lane
// The list of candidates has a fixed capacity: a file with more W-lines is refused (PHI_ERR_UNSUPPORTED), as is one whose
// walks a caller's host reader would count differently -- the command line then reads the file as it always has.
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "phi_ctx.h"
#include "phi_wave.h"
#include "text_bytes.h"

#define GT_TILE ((int64_t)64 << 10)     // bytes per workgroup of the scan
#define GT_CAP_DEFAULT (1 << 20)        // candidate W-lines at most (PHI_GFA_SPLIT_CAP)

extern "C" int phi_inflate_to_device(int32_t device, const void *in, int64_t n, int64_t chunk_bytes, int32_t flags, void **d_out,
                                     int64_t *out_size, phi_inflate_info *info);      // inflate.hip

namespace {

__global__ void __launch_bounds__(256) phi_gfa_split_scan_kernel(const uint8_t *__restrict__ text, int64_t n, int64_t n_tiles,
                                                                 int64_t *__restrict__ tile_nl, int64_t *__restrict__ cand, int32_t cap,
                                                                 unsigned int *__restrict__ n_cand)
{
    __shared__ unsigned long long s_nl;
    const int lane = threadIdx.x & 63;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        if (threadIdx.x == 0) s_nl = ~0ull;
        __syncthreads();
        unsigned long long first = ~0ull;
        const int64_t lo = t * GT_TILE, hi = min(n, lo + GT_TILE);
        for (int64_t p = lo + 16 * (int64_t)threadIdx.x; p - 16 * (int64_t)threadIdx.x < hi; p += 16 * 256) {
            uint32_t nl = 0, w = 0, tab = 0;
            if (p < hi) {
                const PhiText16 v = phi_load16(text, p);
                const uint32_t x4 = p + 16 < n ? *reinterpret_cast<const uint32_t *>(text + p + 16) : 0u;   // look-ahead: bytes 16..19
                nl = phi_eq16(v, '\n');
                w = phi_eq16(v, 'W') | (phi_eq4(x4, 'W') << 16);
                tab = phi_eq16(v, '\t') | (phi_eq4(x4, '\t') << 16);
                const int64_t room = n - p;                                   // bytes of the text from p on
                if (room < 20) { const uint32_t ok = (1u << room) - 1u; nl &= ok; w &= ok; tab &= ok; }
                nl &= 0xffffu;
                if (nl) first = min(first, (unsigned long long)(p + __ffs((int)nl) - 1));
            }
            // "\nW\t" at bit k: a candidate line starts at p + k + 1; and the text's first line
            uint32_t m = nl & (w >> 1) & (tab >> 2);
            int nc = __popc(m) + ((p == 0 && (w & 1u) && (tab & 2u)) ? 1 : 0);
            if (__ballot(nc > 0)) {
                const int inc = phi_wave_incl_scan(nc);
                const int total = __shfl(inc, 63, 64);
                unsigned int base = 0;
                if (lane == 0) base = atomicAdd(n_cand, (unsigned int)total);
                base = __shfl(base, 0, 64);
                unsigned int at = base + (unsigned int)(inc - nc);
                if (p == 0 && (w & 1u) && (tab & 2u)) { if (at < (unsigned int)cap) cand[at] = 0; at++; }
                while (m) {
                    const int k = __ffs((int)m) - 1;
                    m &= m - 1;
                    if (at < (unsigned int)cap) cand[at] = p + k + 1;
                    at++;
                }
            }
        }
        if (first != ~0ull) atomicMin(&s_nl, first);
        __syncthreads();
        if (threadIdx.x == 0) tile_nl[t] = s_nl == ~0ull ? -1 : (int64_t)s_nl;
        __syncthreads();
    }
}

// one wave per candidate line start s: its line's end e (after the '\r' rule) and the start b of its walk field (-1: not a walk)
__global__ void __launch_bounds__(256) phi_gfa_split_line_kernel(const uint8_t *__restrict__ text, int64_t n, int64_t n_tiles,
                                                                 const int64_t *__restrict__ tile_nl, const int64_t *__restrict__ cand, int32_t n_cand,
                                                                 int64_t *__restrict__ walk_b, int64_t *__restrict__ line_e)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_cand) return;
    const int64_t s = cand[i];
    // the line's end: the next '\n' in s's tile, 1 KB per step of the wave ...
    const int64_t t = s / GT_TILE, tile_hi = min(n, (t + 1) * GT_TILE);
    int64_t e = -1;
    for (int64_t base = s & ~(int64_t)15; base < tile_hi; base += 1024) {
        const int64_t p = base + 16 * lane;
        const uint32_t m = p < n ? phi_eq16(phi_load16(text, p), '\n') & phi_valid16(p, s, n) : 0u;      // (a line feed of [s, n))
        const unsigned long long b = __ballot(m != 0);
        if (b) {
            const int l = __ffsll((long long)b) - 1;
            const int64_t q = p + __ffs((int)m) - 1;
            e = __shfl(q, l, 64);
            break;
        }
    }
    // ... else the first newline of a later tile (a walk of 60 MB spans a thousand tiles with none), 64 tiles per step
    for (int64_t k0 = t + 1; e < 0 && k0 < n_tiles; k0 += 64) {
        const int64_t v = k0 + lane < n_tiles ? tile_nl[k0 + lane] : -1;
        const unsigned long long b = __ballot(v >= 0);
        if (b) e = __shfl(v, __ffsll((long long)b) - 1, 64);
    }
    if (e < 0) e = n;                                                     // the last line, without its '\n'
    if (e > s && text[e - 1] == '\r') e--;
    // the 6th tab of [s, e)
    int64_t b6 = -1;
    if (e - s >= 3) {
        int need = 6;
        for (int64_t base = s & ~(int64_t)15; base < e; base += 1024) {
            const int64_t p = base + 16 * lane;
            uint32_t m = p < e ? phi_eq16(phi_load16(text, p), '\t') & phi_valid16(p, s, e) : 0u;
            const int cnt = __popc(m);
            const int inc = phi_wave_incl_scan(cnt);
            const int total = __shfl(inc, 63, 64);
            if (total >= need) {
                int64_t q = -1;
                if (inc >= need && inc - cnt < need) {
                    for (int r = need - (inc - cnt); r > 1; r--) m &= m - 1;     // the (need - before)-th tab of this lane
                    q = p + __ffs((int)m) - 1;
                }
                const unsigned long long hit = __ballot(q >= 0);
                b6 = __shfl(q, __ffsll((long long)hit) - 1, 64) + 1;
                break;
            }
            need -= total;
        }
    }
    if (lane == 0) { walk_b[i] = b6; line_e[i] = e; }
}

// the walk fields to their tiles: job j copies walk w's bytes [off, off + len) of one 4-KB tile, 16 bytes per lane
struct GtCopy { int64_t src, dst, len; };

__global__ void __launch_bounds__(256) phi_gfa_split_copy_kernel(const uint8_t *__restrict__ text, const GtCopy *__restrict__ walks, int32_t n_walks,
                                                                 const int64_t *__restrict__ tile0, int64_t n_tiles, uint8_t *__restrict__ out)
{
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int w = phi_last_le(tile0, n_walks, t);                     // walk of the tile: tile0[w] <= t < tile0[w + 1]
        const GtCopy W = walks[w];
        const int64_t off = (t - tile0[w]) * WT_TILE + 16 * (int64_t)threadIdx.x;
        if (off >= W.len) continue;
        const int64_t k = min((int64_t)16, W.len - off);
        uint8_t *d = out + W.dst + off;
        if (k == 16) {
            // (an unaligned source takes a second aligned word, the one that holds the walk's byte off + 15: inside the text or its slack)
            const PhiText16 v = phi_load16_unaligned(text, W.src + off);
            *reinterpret_cast<uint4 *>(d) = make_uint4(v.x, v.y, v.z, v.w);
            continue;
        }
        const uint8_t *s = text + W.src + off;
        for (int64_t j = 0; j < k; j++) d[j] = s[j];
    }
}

}  // namespace

extern "C" {

int phi_gfa_gzip_split(phi_ctx *c, const void *gz, int64_t n, int64_t chunk_bytes, char **host_text, int64_t *host_n, phi_gfa_gzip_info *info)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!c || !host_text || !host_n || n < 0 || (n > 0 && !gz)) return PHI_ERR_INVALID;
    *host_text = nullptr;
    *host_n = 0;
    auto &W = c->wtext;
    W.ready = false;
    PhiStageTimer tm("gfa split");
    phi_inflate_info inf;
    memset(&inf, 0, sizeof inf);
    void *d_raw = nullptr;
    int64_t total = 0;
    const int irc = phi_inflate_to_device(c->device, gz, n, chunk_bytes, 0, &d_raw, &total, &inf);
    if (info) info->inflate = inf;
    if (irc) return phi_fail(c, irc, "%s", inf.detail);
    HIPCHK(hipSetDevice(c->device));
    struct Raw { void *p; ~Raw() { if (p) (void)hipFree(p); } } raw{d_raw};  // (the inflated text goes before this call returns)
    const uint8_t *text = static_cast<const uint8_t *>(d_raw);
    tm.lap("inflate");

    // ---- candidates and tiles' first newlines, then every candidate's line
    const int64_t cap = getenv("PHI_GFA_SPLIT_CAP") ? std::max<int64_t>(1, atoll(getenv("PHI_GFA_SPLIT_CAP"))) : GT_CAP_DEFAULT;
    const int64_t n_tiles = (total + GT_TILE - 1) / GT_TILE;
    DevBuf d_nl, d_cand, d_cnt, d_b, d_e;
    struct Guard { std::vector<DevBuf *> b; ~Guard() { for (DevBuf *x : b) if (x->p) (void)hipFree(x->p); } } guard{{&d_nl, &d_cand, &d_cnt, &d_b, &d_e}};
    PHICHK(phi_dev_ensure(c, d_nl, (size_t)std::max<int64_t>(n_tiles, 1) * 8));
    PHICHK(phi_dev_ensure(c, d_cand, (size_t)cap * 8));
    PHICHK(phi_dev_ensure(c, d_cnt, 64));
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, 64, c->stream));
    if (n_tiles > 0)
        hipLaunchKernelGGL(phi_gfa_split_scan_kernel, dim3((unsigned)std::min<int64_t>(n_tiles, 8192)), dim3(256), 0, c->stream, text, total, n_tiles,
                           d_nl.as<int64_t>(), d_cand.as<int64_t>(), (int32_t)cap, d_cnt.as<unsigned int>());
    HIPCHK(hipGetLastError());
    unsigned int nc_dev = 0;
    HIPCHK(phi_copy_sync(c, &nc_dev, d_cnt.p, 4, hipMemcpyDeviceToHost));
    if ((int64_t)nc_dev > cap) return phi_fail(c, PHI_ERR_UNSUPPORTED, "phi_gfa_gzip_split: %u W-lines, more than the %lld the split takes (PHI_GFA_SPLIT_CAP)", nc_dev, (long long)cap);
    const int32_t n_cand = (int32_t)nc_dev;
    std::vector<int64_t> cand((size_t)n_cand), b((size_t)n_cand), e((size_t)n_cand);
    if (n_cand > 0) {
        PHICHK(phi_dev_ensure(c, d_b, (size_t)n_cand * 8));
        PHICHK(phi_dev_ensure(c, d_e, (size_t)n_cand * 8));
        hipLaunchKernelGGL(phi_gfa_split_line_kernel, dim3((unsigned)((n_cand + 3) / 4)), dim3(256), 0, c->stream, text, total, n_tiles,
                           d_nl.as<int64_t>(), d_cand.as<int64_t>(), n_cand, d_b.as<int64_t>(), d_e.as<int64_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(cand.data(), d_cand.p, (size_t)n_cand * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(b.data(), d_b.p, (size_t)n_cand * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(e.data(), d_e.p, (size_t)n_cand * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    tm.lap("W-lines found");

    // ---- the walks in file order: their tiles, as phi_walk_text_upload lays them out
    std::vector<int32_t> ord((size_t)n_cand);
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return cand[(size_t)x] < cand[(size_t)y]; });
    std::vector<GtCopy> walks;
    for (int32_t i : ord)
        if (b[(size_t)i] >= 0) walks.push_back(GtCopy{b[(size_t)i], 0, e[(size_t)i] - b[(size_t)i]});
    if (walks.size() >= ((size_t)1 << 31)) return phi_fail(c, PHI_ERR_UNSUPPORTED, "phi_gfa_gzip_split: too many walks");
    const int32_t n_walks = (int32_t)walks.size();
    W.n_walks = n_walks;
    W.tile0.assign((size_t)n_walks + 1, 0);
    W.t_len.assign((size_t)n_walks, 0);
    int64_t walk_bytes = 0;
    for (int32_t w = 0; w < n_walks; w++) {
        W.t_len[(size_t)w] = walks[(size_t)w].len;
        W.tile0[(size_t)w + 1] = W.tile0[(size_t)w] + (walks[(size_t)w].len + WT_TILE - 1) / WT_TILE;
        walks[(size_t)w].dst = W.tile0[(size_t)w] * WT_TILE;
        walk_bytes += walks[(size_t)w].len;
    }
    const int64_t w_tiles = W.tile0[(size_t)n_walks];
    if (n_walks > 0) {
        PHICHK(phi_dev_ensure(c, W.d_text, (size_t)w_tiles * WT_TILE + 256));
        if (w_tiles > 0) {
            DevBuf d_walks, d_tile0;
            struct G2 { DevBuf &a, &b; ~G2() { if (a.p) (void)hipFree(a.p); if (b.p) (void)hipFree(b.p); } } g2{d_walks, d_tile0};
            PHICHK(phi_dev_ensure(c, d_walks, (size_t)n_walks * sizeof(GtCopy)));
            PHICHK(phi_dev_ensure(c, d_tile0, ((size_t)n_walks + 1) * 8));
            HIPCHK(hipMemcpyAsync(d_walks.p, walks.data(), (size_t)n_walks * sizeof(GtCopy), hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d_tile0.p, W.tile0.data(), ((size_t)n_walks + 1) * 8, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(phi_gfa_split_copy_kernel, dim3((unsigned)std::min<int64_t>(w_tiles, 256 * 64)), dim3(256), 0, c->stream, text,
                               d_walks.as<GtCopy>(), n_walks, d_tile0.as<int64_t>(), w_tiles, W.d_text.as<uint8_t>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    }
    tm.lap("walks to their tiles");

    // ---- the rest of the text to the host: every byte outside the walk fields, at most n_walks + 1 ranges
    const int64_t keep = total - walk_bytes;
    char *h = nullptr;
    HIPCHK(hipHostMalloc((void **)&h, (size_t)keep + 1, hipHostMallocDefault));
    int64_t at = 0, from = 0;
    hipError_t err = hipSuccess;
    for (int32_t w = 0; w <= n_walks && err == hipSuccess; w++) {
        const int64_t to = w < n_walks ? walks[(size_t)w].src : total;
        if (to > from) err = hipMemcpyAsync(h + at, text + from, (size_t)(to - from), hipMemcpyDeviceToHost, c->stream);
        at += to - from;
        if (w < n_walks) from = walks[(size_t)w].src + walks[(size_t)w].len;
    }
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) { (void)hipHostFree(h); return phi_hip_check(c, err, "the host text"); }
    h[keep] = 0;
    tm.lap("host text down");
    W.ready = true;
    *host_text = h;
    *host_n = keep;
    if (info) {
        info->text_bytes = total;
        info->host_bytes = keep;
        info->walk_bytes = walk_bytes;
        info->n_walks = n_walks;
    }
    return PHI_OK;
}

void phi_gfa_gzip_free(char *host_text) { if (host_text) (void)hipHostFree(host_text); }

}  // extern "C"
