// dev_mem.hip -- device memory of a context: growable buffers and the per-device pool of large ones, the poison fill of the
// tests, uploads (staged through pinned buffers when large and pageable), the pinned download buffer, host registration.
// No kernel.  The pool's best-fit choice is a rule of reads_host.h.
#include <string.h>
#include "phi_ctx.h"

// Large device buffers that are let go are kept for the next taker of about their size instead of going back to the driver:
// the driver clears device memory before it hands it out again (measured on this pool: ~28 us per MB once the freed memory is
// what the next hipMalloc gets -- 60 ms for the 2.1 GB of a DP run's prefix sums at config 5, 0.25 s of phi_solve when the 10 GB
// of walk text were freed before it, and every allocation of a process that starts right behind another one's end), and
// phi_set_graph's temporaries are the sizes phi_solve asks for next (4 bytes per walk entry, several times).  The pool is per
// device, emptied when a solve is done, when a context goes, and when an allocation fails.  PHI_DEVICE_POOL=0: off.
namespace {
struct DevPool { std::mutex mu; std::vector<DevBuf> bufs; };
DevPool g_pool[64];
// (PHI_DEVICE_POOL_MIN=bytes: tests pool everything, so that every buffer comes back with an earlier owner's contents;
//  PHI_DEVICE_POISON=0..255: tests fill every buffer with that byte when it gets a new owner -- phi_dev_poison of phi_ctx.h,
//  tests/test_gpu_dirty_memory.py runs the small shapes of every kernel family under both.  Not for groups of processes:
//  the mailbox of phi_ipc.hip is left alone)
const size_t POOL_MIN = getenv("PHI_DEVICE_POOL_MIN") ? (size_t)atoll(getenv("PHI_DEVICE_POOL_MIN")) : ((size_t)16 << 20);
thread_local bool t_pool_bypass = false;
bool pool_on()
{
    static const bool on = !(getenv("PHI_DEVICE_POOL") && atoi(getenv("PHI_DEVICE_POOL")) == 0);
    return on && !t_pool_bypass;
}
int cur_device() { int d = 0; return hipGetDevice(&d) == hipSuccess && d >= 0 && d < 64 ? d : -1; }
bool pool_take(int dev, size_t want, DevBuf &b)
{
    if (dev < 0) return false;
    DevPool &P = g_pool[dev];
    std::lock_guard<std::mutex> lk(P.mu);
    std::vector<size_t> caps;
    for (const DevBuf &x : P.bufs) caps.push_back(x.cap);
    const int best = phi_pool_best_fit(caps.data(), (int)caps.size(), want);
    if (best < 0) return false;
    b = P.bufs[(size_t)best];
    P.bufs.erase(P.bufs.begin() + best);
    return true;
}
int poison_from_env()
{
    const char *e = getenv("PHI_DEVICE_POISON");
    if (!e || !*e) return -1;
    char *end = nullptr;
    const long v = strtol(e, &end, 0);
    return (*end || v < 0 || v > 255) ? -1 : (int)v;
}
}  // namespace
void phi_pool_bypass(bool on) { t_pool_bypass = on; }
const int phi_device_poison = poison_from_env();
// (the null stream, and a wait for it: the mode is for tests, and the buffer has no other user yet)
int phi_dev_poison_fill(void *p, size_t bytes)
{
    if (!p || !bytes) return 0;
    if (hipMemset(p, phi_device_poison, bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) { (void)hipGetLastError(); return 1; }
    return 0;
}
void phi_pool_flush(int dev)
{
    if (dev < 0 || dev >= 64) return;
    std::vector<DevBuf> v;
    { std::lock_guard<std::mutex> lk(g_pool[dev].mu); v.swap(g_pool[dev].bufs); }
    for (DevBuf &x : v) if (x.p) (void)hipFree(x.p);
}
void phi_dev_free(DevBuf &b)
{
    if (!b.p) { b.cap = 0; return; }
    int dev = -1;
    if (b.cap >= POOL_MIN && pool_on()) {
        // (the device the buffer lives on -- not the calling thread's current one: a thread that has not chosen a device is on device 0)
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, b.p) == hipSuccess && at.device >= 0 && at.device < 64 && at.device == cur_device()) dev = at.device;
        else (void)hipGetLastError();
    }
    if (dev >= 0) {
        (void)hipDeviceSynchronize();                      // (what hipFree does before it lets memory go: nobody still works on it)
        std::lock_guard<std::mutex> lk(g_pool[dev].mu);
        g_pool[dev].bufs.push_back(b);
    } else {
        (void)hipFree(b.p);
    }
    b.p = nullptr; b.cap = 0;
}

int phi_dev_ensure(phi_ctx *c, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap && b.p) return PHI_OK;
    const uint32_t gen = b.gen + 1;                        // (the memory behind b changes hands below, whatever address it gets)
    phi_dev_free(b);
    size_t want = bytes < 256 ? 256 : bytes;
    if (want >= POOL_MIN && pool_on() && pool_take(c->device, want, b)) {
        b.gen = gen;
        if (phi_dev_poison(b.p, b.cap)) return phi_fail(c, PHI_ERR_DEVICE, "PHI_DEVICE_POISON: the fill of %zu bytes failed", b.cap);
        return PHI_OK;
    }
    static const bool timing = getenv("PHI_TIMING_ALLOC") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(&b.p, want);
    if (e == hipErrorOutOfMemory) {                        // what the pool holds may be what is missing
        (void)hipGetLastError();
        phi_pool_flush(c->device);
        e = hipMalloc(&b.p, want);
    }
    if (timing) {
        static std::atomic<long long> total_ns{0}, calls{0};
        const long long ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        total_ns += ns; calls++;
        fprintf(stderr, "[phi alloc] %10zu bytes %8.1f us (total %lld calls, %.3f ms)\n", want, ns / 1e3, (long long)calls, total_ns / 1e6);
    }
    if (e != hipSuccess) { b.p = nullptr; return phi_fail(c, PHI_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e)); }
    b.cap = want;
    b.gen = gen;
    if (phi_dev_poison(b.p, b.cap)) return phi_fail(c, PHI_ERR_DEVICE, "PHI_DEVICE_POISON: the fill of %zu bytes failed", b.cap);
    return PHI_OK;
}

// (the pinned staging buffers serve phi_set_graph's uploads only: given back when it is done)
void stage_release(phi_ctx *c)
{
    for (int i = 0; i < 2; i++) {
        if (c->stage_ev[i]) { (void)hipEventSynchronize(c->stage_ev[i]); (void)hipEventDestroy(c->stage_ev[i]); }
        if (c->h_stage[i]) (void)hipHostFree(c->h_stage[i]);
        c->h_stage[i] = nullptr; c->stage_ev[i] = nullptr;
    }
}

// A large array from the caller's PAGEABLE memory (the walk entries of a chromosome-scale graph: 5 GB): the runtime stages such
// a copy through its own pinned buffers with one thread, 7 GB/s -- most of phi_set_graph at that size.  Here: two pinned
// buffers of the context, filled by four threads, each sent while the other is filled.
static int upload_staged(phi_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t st)
{
    constexpr size_t PIECE = (size_t)64 << 20;
    if (!c->h_stage[0]) {
        // both buffers and both events, or none: a context never holds half of them
        void *b[2] = {nullptr, nullptr};
        hipEvent_t ev[2] = {nullptr, nullptr};
        hipError_t e = hipSuccess;
        for (int i = 0; i < 2 && e == hipSuccess; i++) {
            e = hipHostMalloc(&b[i], PIECE, hipHostMallocDefault);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        }
        if (e != hipSuccess) {
            for (int i = 0; i < 2; i++) { if (b[i]) (void)hipHostFree(b[i]); if (ev[i]) (void)hipEventDestroy(ev[i]); }
            return phi_hip_check(c, e, "pinned staging buffers");
        }
        for (int i = 0; i < 2; i++) { c->h_stage[i] = b[i]; c->stage_ev[i] = ev[i]; }
    }
    int k = 0;
    for (size_t off = 0; off < bytes; off += PIECE, k ^= 1) {
        const size_t n = std::min(PIECE, bytes - off);
        HIPCHK(hipEventSynchronize(c->stage_ev[k]));          // (the copy that last read this buffer; a fresh event is complete)
        {
            const int nt = 4;
            std::vector<std::thread> th;
            char *d = static_cast<char *>(c->h_stage[k]);
            const char *s = static_cast<const char *>(src) + off;
            for (int t = 1; t < nt; t++) th.emplace_back([=]() { memcpy(d + n * t / nt, s + n * t / nt, n * (t + 1) / nt - n * t / nt); });
            memcpy(d, s, n / nt);
            for (auto &x : th) x.join();
        }
        HIPCHK(hipMemcpyAsync(static_cast<char *>(dst) + off, c->h_stage[k], n, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(c->stage_ev[k], st));
    }
    return PHI_OK;
}

int phi_upload_bytes(phi_ctx *c, DevBuf &b, const void *src, size_t bytes, hipStream_t st)
{
    PHICHK(phi_dev_ensure(c, b, bytes ? bytes : 1));
    if (!st) st = c->stream;
    if (bytes >= ((size_t)256 << 20) && !getenv("PHI_NO_STAGED_UPLOAD")) {
        hipPointerAttribute_t at{};
        const bool pinned = hipPointerGetAttributes(&at, src) == hipSuccess && at.type == hipMemoryTypeHost;
        (void)hipGetLastError();                               // (an unregistered pointer is an error of that call, not of ours)
        if (!pinned) return upload_staged(c, b.p, src, bytes, st);
    }
    if (bytes) HIPCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
    return PHI_OK;
}

// a device buffer that grows and KEEPS its first `keep` bytes
int phi_dev_grow_keep(phi_ctx *c, DevBuf &b, size_t bytes, size_t keep)
{
    if (bytes <= b.cap && b.p) return PHI_OK;
    DevBuf nb;
    nb.gen = b.gen;                                        // (b's generation goes on counting through the exchange below)
    int rc = phi_dev_ensure(c, nb, bytes);
    if (rc) return rc;
    if (b.p && keep) {
        rc = phi_hip_check(c, phi_copy_sync(c, nb.p, b.p, std::min(keep, b.cap), hipMemcpyDeviceToDevice), "copy into the grown buffer");
        if (rc) { phi_dev_free(nb); return rc; }
    } else if (b.p) {
        rc = phi_hip_check(c, hipStreamSynchronize(c->stream), "stream synchronize");      // an earlier launch may still write the old buffer
        if (rc) { phi_dev_free(nb); return rc; }
    }
    phi_dev_free(b);
    b = nb;
    return PHI_OK;
}

int phi_pin_ensure(phi_ctx *c, size_t bytes)
{
    if (c->pin_future.valid()) c->pin_future.wait();          // an allocation started by phi_set_graph
    if (bytes <= c->h_pin_cap) return PHI_OK;
    if (c->h_pin) (void)hipHostFree(c->h_pin);
    c->h_pin = nullptr; c->h_pin_cap = 0;
    c->h_kept = PhiAnchorSpan{}; c->h_dp = PhiAnchorSpan{}; c->anchors_host = false;
    const size_t want = bytes + bytes / 4;
    if (hipHostMalloc(&c->h_pin, want, hipHostMallocDefault) != hipSuccess) { c->h_pin = nullptr; return phi_fail(c, PHI_ERR_NOMEM, "pinned host allocation of %zu bytes failed", want); }
    c->h_pin_cap = want;
    return PHI_OK;
}

extern "C" {

int phi_host_register(phi_ctx *c, void *p, size_t bytes)
{
    if (!c || !p || !bytes) return PHI_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipHostRegister(p, bytes, hipHostRegisterPortable));   // every GPU of a --devices run copies from it
    return PHI_OK;
}

int phi_host_unregister(phi_ctx *c, void *p)
{
    if (!c || !p) return PHI_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipHostUnregister(p));
    return PHI_OK;
}

}  // extern "C"
