// dev_run.h -- what a stand-alone device run (inflate.hip, deflate.hip: calls that take no context) keeps for its duration:
// a stream, two events and the buffers it allocated, all released when the run ends; and how such a run fails: a status and
// a line of text in its info's `detail`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../../include/phi_amd.h"
#include "phi_ctx.h"

namespace {

struct Dev {
    std::vector<void *> bufs;
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~Dev()
    {
        if (st) (void)hipStreamSynchronize(st);
        for (void *p : bufs) (void)hipFree(p);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
    template <class T> T *alloc(size_t bytes)
    {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        bufs.push_back(p);
        if (phi_dev_poison(p, std::max<size_t>(bytes, 16))) return nullptr;
        return (T *)p;
    }
};

// info: a phi_inflate_info or a phi_deflate_info (may be null)
template <class Info> int fail(Info *info, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
template <class Info> int fail(Info *info, int code, const char *fmt, ...)
{
    if (info) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(info->detail, sizeof(info->detail), fmt, ap);
        va_end(ap);
    }
    return code;
}

}  // namespace

// deflate.hip: the BGZF writer's run for the indexed entry (bgzf_index.hip).  The file of src[0, n) into dst[0,
// phi_deflate_bgzf_bound(n)); d_src (may be null): the same bytes already on the device, 64 readable bytes behind them, from
// which the batches then read; member_off (may be null): off[0..blocks], where every member and the EOF block begin
int phi_deflate_run(int32_t device, const uint8_t *src, const uint8_t *d_src, int64_t n, int32_t flags, uint8_t *dst, int64_t *out_size,
                    phi_deflate_info *info, std::vector<int64_t> *member_off);

// inside a function with `info` (and, for DALLOC, a Dev `dev`) in scope that returns a status
#define DCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(info, PHI_ERR_DEVICE, "%s: %s", #call, hipGetErrorString(e_)); } while (0)
#define DALLOC(var, T, bytes) T *var = dev.alloc<T>(bytes); if (!var) return fail(info, PHI_ERR_NOMEM, "device allocation of %zu bytes failed", (size_t)(bytes))
