// scan.hip -- the stand-alone prefix sums and the ordered compaction of the device code.
//
//   phi_scan      off[0..n] = exclusive prefix sums of cnt[0..n), off[n] = the total
//                   uint8 -> int32   (the anchor weights of a DP run)
//                   int32 -> int32   (counts per entry / class / minimiser id; may run in place)
//                   int32 -> int64   (flat base offsets, block counts of the two-pass kernels)
//   phi_compact   flags[0..n) -> the ascending list of the flagged indices
//
// All of it is integer addition with a fixed place for every output: no result depends on the order of the additions.
// The entry points run on the context's stream and own their scratch (d_scan_blk, d_scan_blk64, d_scan_blkoff, d_blk_cnt,
// d_blk_off): calls on one context follow one another on that stream, from one host thread at a time.
// A run without a context (bgzf_index.hip) launches the same kernels on its own stream over its own scratch: phi_scan_tiles,
// phi_compact_count, phi_compact_write (phi_ctx.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "phi_ctx.h"
#include "phi_kernels.h"
#include "phi_wave.h"

// ------------------------------------------------------------------ three phases, 1024 items per workgroup
// block sums -> their scan in one workgroup (phi_scan_tiles_kernel) -> every workgroup again, from its offset.
// Workgroup n / 1024 owns off[n], the total: one workgroup more than the items need when n is a multiple of 1024.
#define SCAN_WG_ITEMS 1024
static inline int64_t scan_num_blocks(int64_t n) { return (n + 1 + SCAN_WG_ITEMS - 1) / SCAN_WG_ITEMS; }

template <class In, class Acc>
__global__ void __launch_bounds__(256) phi_scan_blocksum_kernel(const In *__restrict__ cnt, int64_t n, Acc *__restrict__ blk)
{
    __shared__ Acc s_w[4];
    const int64_t base = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    Acc c = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) if (base + j < n) c += cnt[base + j];
    c = phi_wave_sum(c);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// (off may be cnt itself where both are int32: a thread reads its four counts before it writes its four sums, and nobody
//  else's -- so neither pointer is __restrict__)
template <class In, class Acc>
__global__ void __launch_bounds__(256) phi_scan_apply_kernel(const In *cnt, int64_t n, const int64_t *__restrict__ blk_off, Acc *off)
{
    __shared__ Acc s_w[4];
    const int64_t base = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    Acc v[4], c = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) { v[j] = (base + j < n) ? cnt[base + j] : 0; c += v[j]; }
    Acc run = (Acc)blk_off[blockIdx.x] + phi_block_excl_scan<4>(c, s_w);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (base + j < n) off[base + j] = run;
        run += v[j];
    }
    if (base <= n && n < base + 4) off[n] = run;       // total (the items past n are zero)
}

// ------------------------------------------------------------------ one workgroup, tiles of 4096
// single-workgroup exclusive scan of per-block counts (off[n] = total): phi_carry_scan (phi_wave.h), whose tiles keep the loads
// coalesced whatever n is -- a chromosome-scale graph scans 1.3 M block counts here, six times per solve
// (a thread summing its own contiguous share of the array, as before, read with a stride of 5 KB between lanes: 4.4 ms a call).
template <class In>
__global__ void __launch_bounds__(1024) phi_scan_tiles_kernel(const In *__restrict__ cnt, int64_t n, int64_t *__restrict__ off)
{
    __shared__ int64_t s_w[16];
    const int64_t total = phi_carry_scan(cnt, n, off, s_w);
    if (threadIdx.x == 0) off[n] = total;
}

template <class In>
static void launch_scan_tiles(hipStream_t st, const In *cnt, int64_t n, int64_t *off)
{
    hipLaunchKernelGGL(phi_scan_tiles_kernel<In>, dim3(1), dim3(1024), 0, st, cnt, n, off);
}

template <class In, class Acc>
static int scan_three_phase(phi_ctx *c, const In *cnt, int64_t n, Acc *off)
{
    const int64_t nb = scan_num_blocks(n);
    DevBuf &d_blk = sizeof(Acc) == 8 ? c->d_scan_blk64 : c->d_scan_blk;
    PHICHK(phi_dev_ensure(c, d_blk, (size_t)nb * sizeof(Acc)));
    PHICHK(phi_dev_ensure(c, c->d_scan_blkoff, (size_t)(nb + 1) * 8));
    Acc *blk = d_blk.as<Acc>();
    int64_t *blk_off = c->d_scan_blkoff.as<int64_t>();
    hipLaunchKernelGGL((phi_scan_blocksum_kernel<In, Acc>), dim3((unsigned)nb), dim3(256), 0, c->stream, cnt, n, blk);
    launch_scan_tiles(c->stream, blk, nb, blk_off);
    hipLaunchKernelGGL((phi_scan_apply_kernel<In, Acc>), dim3((unsigned)nb), dim3(256), 0, c->stream, cnt, n, blk_off, off);
    return PHI_OK;
}

int phi_scan(phi_ctx *c, const uint8_t *cnt, int64_t n, int32_t *off) { return scan_three_phase(c, cnt, n, off); }
int phi_scan(phi_ctx *c, const int32_t *cnt, int64_t n, int32_t *off) { return scan_three_phase(c, cnt, n, off); }
// one workgroup for a few thousand items, the three phases beyond (the per-chunk counts of 250 Mbases of walks are half a
// million items: 1 ms in one workgroup)
int phi_scan(phi_ctx *c, const int32_t *cnt, int64_t n, int64_t *off)
{
    if (n <= 8192) { launch_scan_tiles(c->stream, cnt, n, off); return PHI_OK; }
    return scan_three_phase(c, cnt, n, off);
}

// ------------------------------------------------------------------ ordered compaction
// flags[n] (0/1) -> ascending list of the flagged indices.  2048 items per workgroup.
#define CMP_ITEMS 8
__global__ void __launch_bounds__(256) phi_flag_count_kernel(const uint8_t *__restrict__ flags, int64_t n,
                                                             int32_t *__restrict__ block_cnt)
{
    __shared__ int s_w[4];
    const int64_t base = ((int64_t)blockIdx.x * 256 + threadIdx.x) * CMP_ITEMS;
    int c = 0;
#pragma unroll
    for (int j = 0; j < CMP_ITEMS; j++)
        if (base + j < n) c += flags[base + j] != 0;
    c = phi_wave_sum(c);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ void __launch_bounds__(256) phi_flag_write_kernel(const uint8_t *__restrict__ flags, int64_t n,
                                                             const int64_t *__restrict__ block_off,
                                                             int32_t *__restrict__ out)
{
    __shared__ int s_w[4];
    const int64_t base = ((int64_t)blockIdx.x * 256 + threadIdx.x) * CMP_ITEMS;
    uint32_t f = 0;
#pragma unroll
    for (int j = 0; j < CMP_ITEMS; j++)
        if (base + j < n && flags[base + j]) f |= 1u << j;
    int64_t o = block_off[blockIdx.x] + phi_block_excl_scan<4>((int)__popc(f), s_w);
#pragma unroll
    for (int j = 0; j < CMP_ITEMS; j++)
        if (f & (1u << j)) out[o++] = (int32_t)(base + j);
}

// flags[n] -> ascending indices in out; *n_out = count (waits for the stream)
int phi_compact(phi_ctx *c, const uint8_t *flags, int64_t n, DevBuf &out, int64_t *n_out)
{
    *n_out = 0;
    const int64_t nb = (n + 256 * CMP_ITEMS - 1) / (256 * CMP_ITEMS);
    if (nb <= 0) return PHI_OK;
    PHICHK(phi_dev_ensure(c, c->d_blk_cnt, (size_t)nb * 4));
    PHICHK(phi_dev_ensure(c, c->d_blk_off, (size_t)(nb + 1) * 8));
    hipLaunchKernelGGL(phi_flag_count_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, flags, n, c->d_blk_cnt.as<int32_t>());
    PHICHK(phi_scan(c, c->d_blk_cnt.as<int32_t>(), nb, c->d_blk_off.as<int64_t>()));
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, c->d_blk_off.as<int64_t>() + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    PHICHK(phi_dev_ensure(c, out, (size_t)std::max<int64_t>(total, 1) * 4));
    hipLaunchKernelGGL(phi_flag_write_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, flags, n, c->d_blk_off.as<int64_t>(),
                       out.as<int32_t>());
    *n_out = total;
    return PHI_OK;
}

// ------------------------------------------------------------------ the same for a run without a context (phi_ctx.h)
int64_t phi_compact_blocks(int64_t n) { return (n + 256 * CMP_ITEMS - 1) / (256 * CMP_ITEMS); }
void phi_scan_tiles(hipStream_t st, const int32_t *cnt, int64_t n, int64_t *off) { launch_scan_tiles(st, cnt, n, off); }
void phi_compact_count(hipStream_t st, const uint8_t *flags, int64_t n, int32_t *blk_cnt, int64_t *blk_off)
{
    const int64_t nb = phi_compact_blocks(n);
    if (nb > 0) hipLaunchKernelGGL(phi_flag_count_kernel, dim3((unsigned)nb), dim3(256), 0, st, flags, n, blk_cnt);
    launch_scan_tiles(st, blk_cnt, nb, blk_off);
}
void phi_compact_write(hipStream_t st, const uint8_t *flags, int64_t n, const int64_t *blk_off, int32_t *out)
{
    const int64_t nb = phi_compact_blocks(n);
    if (nb > 0) hipLaunchKernelGGL(phi_flag_write_kernel, dim3((unsigned)nb), dim3(256), 0, st, flags, n, blk_off, out);
}

// ------------------------------------------------------------------ the exported entry (include/phi_amd.h)
int phi_prefix_sums(phi_ctx *c, int32_t kind, const void *d_in, int64_t n, void *d_out)
{
    if (!c) return PHI_ERR_INVALID;
    if (n < 0 || kind < 0 || kind > 2 || !d_out || (n > 0 && !d_in)) return phi_fail(c, PHI_ERR_INVALID, "phi_prefix_sums: bad argument");
    HIPCHK(hipSetDevice(c->device));
    if (kind == 0) PHICHK(phi_scan(c, static_cast<const uint8_t *>(d_in), n, static_cast<int32_t *>(d_out)));
    else if (kind == 1) PHICHK(phi_scan(c, static_cast<const int32_t *>(d_in), n, static_cast<int32_t *>(d_out)));
    else PHICHK(phi_scan(c, static_cast<const int32_t *>(d_in), n, static_cast<int64_t *>(d_out)));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return PHI_OK;
}

// (the code object of this translation unit, loaded by phi_ctx_create: see phi_warm_sketch)
__global__ void phi_warm_scan_kernel() {}
void phi_warm_scan(hipStream_t st) { hipLaunchKernelGGL(phi_warm_scan_kernel, dim3(1), dim3(64), 0, st); }
