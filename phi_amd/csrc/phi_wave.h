// Sums across the 64 lanes of a wave and across the waves of a workgroup: the one copy of the two idioms every scan,
// compaction and counter of the device code is made of, and the scan of a whole array by one workgroup.  Device code only;
// workgroups are one-dimensional (the lane is threadIdx.x & 63).  Integer sums only: the order of the additions is not part
// of the result.
// (The sketch and DP kernels keep their own DPP scans and reductions, tuned to a register count: sketch_dev.h, dp_dev.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

// the shuffles take (unsigned) int and (unsigned) long long: int64_t / uint64_t go through the latter
template <class T>
using phi_shfl_t = std::conditional_t<sizeof(T) == 8, std::conditional_t<std::is_signed<T>::value, long long, unsigned long long>, T>;

// inclusive prefix sum over the lanes: lane l returns x of lanes 0..l
template <class T>
__device__ __forceinline__ T phi_wave_incl_scan(T x)
{
    static_assert(std::is_integral<T>::value && (sizeof(T) == 4 || sizeof(T) == 8), "int, uint32_t, int64_t, uint64_t");
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = (T)__shfl_up((phi_shfl_t<T>)x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// the sum over all 64 lanes, in every lane
template <class T>
__device__ __forceinline__ T phi_wave_sum(T x)
{
    static_assert(std::is_integral<T>::value && (sizeof(T) == 4 || sizeof(T) == 8), "int, uint32_t, int64_t, uint64_t");
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += (T)__shfl_xor((phi_shfl_t<T>)x, d, 64);
    return x;
}

// Exclusive prefix sum over a workgroup of NW waves: returns the sum of `mine` over the threads before this one, and in
// *total (optional) the sum over all of them.  s_w[NW] is LDS of the caller; one __syncthreads, which every thread of the
// workgroup must reach.  A caller that comes back (a loop over tiles) puts a barrier of its own before the next call.
template <int NW, class T>
__device__ __forceinline__ T phi_block_excl_scan(T mine, T *s_w, T *total = nullptr)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const T inc = phi_wave_incl_scan(mine);
    if (lane == 63) s_w[wid] = inc;
    __syncthreads();
    T woff = 0;
    for (int i = 0; i < wid; i++) woff += s_w[i];
    if (total) {
        T t = 0;
#pragma unroll
        for (int i = 0; i < NW; i++) t += s_w[i];
        *total = t;
    }
    return woff + inc - mine;
}

// Exclusive prefix sums by ONE workgroup of 1024 threads: out[i] = in[0] + .. + in[i - 1] for i < n; returns the total, in every
// thread.  Tiles of 4096 items, four consecutive per thread -- the loads are coalesced whatever n is -- and a running carry.
// out may be in itself: a thread reads its four items before it writes its four sums, and nobody else's (so neither pointer is
// __restrict__ here).  s_w[16] is LDS of the caller.
template <class In, class Out>
__device__ __forceinline__ Out phi_carry_scan(const In *in, int64_t n, Out *out, Out *s_w)
{
    Out carry = 0;                                        // everything before the tile
    for (int64_t base = 0; base < n; base += 4096) {
        const int64_t i0 = base + 4 * (int64_t)threadIdx.x;
        In v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = i0 + j < n ? in[i0 + j] : 0;
        const Out c = (Out)v[0] + v[1] + v[2] + v[3];
        Out tile;
        Out run = carry + phi_block_excl_scan<16>(c, s_w, &tile);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (i0 + j < n) out[i0 + j] = run;
            run += v[j];
        }
        carry += tile;
        __syncthreads();                                  // (s_w is written again in the next turn)
    }
    return carry;
}
