// text_park.hip -- text that arrives before the graph is there waits in device memory: the park, its pieces, and a gzip
// stream gathered and inflated into pieces.  No kernel.
#include <deque>
#include <string.h>
#include "phi_ctx.h"

extern "C" {

/* Text that arrives before the graph is there waits in device memory (include/phi_amd.h): a park is no part of any context's
 * state -- its own stream, its own buffers --, so that a reader thread fills it while phi_set_graph runs on another. */
struct phi_text_park {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    struct Piece { DevBuf d; int64_t n = 0; char first = 0; hipEvent_t ev = nullptr; };      // ev: the copy of the bytes has landed
    std::deque<Piece> pieces;                                  // (a deque: references stay valid while pieces are added)
    std::vector<DevBuf> spare;                                 // buffers of released pieces
    std::vector<void *> pinned;
    std::vector<char> gz;                                      // a gzip stream being gathered (phi_text_park_gzip_*)
    int64_t gz_piece = 0;
    bool gz_on = false;
};

int phi_text_park_create(int32_t device, phi_text_park **out)
{
    if (!out) return PHI_ERR_INVALID;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return PHI_ERR_DEVICE;
    phi_text_park *p = new phi_text_park();
    p->device = device;
    if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess) { delete p; return PHI_ERR_DEVICE; }
    *out = p;
    return PHI_OK;
}

int phi_text_park_pin(phi_text_park *p, void *host, size_t bytes)
{
    if (!p || !host) return PHI_ERR_INVALID;
    if (hipSetDevice(p->device) != hipSuccess || hipHostRegister(host, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return PHI_ERR_DEVICE; }
    p->pinned.push_back(host);
    return PHI_OK;
}

// A buffer of `want` bytes for a new piece: one a released piece left behind, if one is large enough (pieces are of one size
// but the last), else a new one; poisoned under PHI_DEVICE_POISON.  On failure d holds nothing.
static int park_take_buffer(phi_text_park *p, size_t want, DevBuf &d)
{
    {
        std::lock_guard<std::mutex> lk(p->mu);
        for (size_t i = 0; i < p->spare.size(); i++)
            if (p->spare[i].cap >= want) { d = p->spare[i]; p->spare.erase(p->spare.begin() + (ptrdiff_t)i); break; }
    }
    if (!d.p) {
        if (hipMalloc(&d.p, want) != hipSuccess) { (void)hipGetLastError(); d.p = nullptr; return PHI_ERR_NOMEM; }
        d.cap = want;
    }
    if (phi_dev_poison(d.p, d.cap)) { (void)hipFree(d.p); d = DevBuf{}; return PHI_ERR_DEVICE; }
    return PHI_OK;
}

// the copy is ISSUED when this returns; phi_text_park_wait says when the host buffer may be written again (whoever takes the
// piece -- phi_add_reads_text_parked, phi_text_park_fetch -- waits for it by itself)
int phi_text_park_add_async(phi_text_park *p, const char *text, int64_t n, int32_t *index)
{
    if (!p || !text || n <= 0 || !index) return PHI_ERR_INVALID;
    if (hipSetDevice(p->device) != hipSuccess) return PHI_ERR_DEVICE;
    phi_text_park::Piece pc;
    if (const int rc = park_take_buffer(p, (size_t)n + 64, pc.d)) return rc;
    pc.n = n; pc.first = text[0];
    if (hipEventCreateWithFlags(&pc.ev, hipEventDisableTiming) != hipSuccess ||
        hipMemcpyAsync(pc.d.p, text, (size_t)n, hipMemcpyHostToDevice, p->stream) != hipSuccess || hipEventRecord(pc.ev, p->stream) != hipSuccess) {
        (void)hipGetLastError(); (void)hipStreamSynchronize(p->stream);
        if (pc.ev) (void)hipEventDestroy(pc.ev);
        (void)hipFree(pc.d.p); return PHI_ERR_DEVICE;
    }
    std::lock_guard<std::mutex> lk(p->mu);
    p->pieces.push_back(pc);
    *index = (int32_t)p->pieces.size() - 1;
    return PHI_OK;
}

static phi_text_park::Piece *park_piece(phi_text_park *p, int32_t index)
{
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(p->mu);
    return index >= 0 && (size_t)index < p->pieces.size() && p->pieces[(size_t)index].d.p ? &p->pieces[(size_t)index] : nullptr;
}

int phi_text_park_wait(phi_text_park *p, int32_t index)
{
    phi_text_park::Piece *pc = park_piece(p, index);
    if (!pc) return PHI_ERR_INVALID;
    if (pc->ev && hipEventSynchronize(pc->ev) != hipSuccess) { (void)hipGetLastError(); return PHI_ERR_DEVICE; }
    return PHI_OK;
}

int phi_text_park_add(phi_text_park *p, const char *text, int64_t n, int32_t *index)
{
    const int rc = phi_text_park_add_async(p, text, n, index);
    return rc ? rc : phi_text_park_wait(p, *index);
}

int64_t phi_text_park_bytes(phi_text_park *p, int32_t index) { phi_text_park::Piece *pc = park_piece(p, index); return pc ? pc->n : -1; }

int phi_text_park_fetch(phi_text_park *p, int32_t index, char *out, int64_t cap)
{
    phi_text_park::Piece *pc = park_piece(p, index);
    if (!pc || !out || cap < pc->n) return PHI_ERR_INVALID;
    if (hipSetDevice(p->device) != hipSuccess) return PHI_ERR_DEVICE;
    if (pc->ev) (void)hipEventSynchronize(pc->ev);
    if (hipMemcpyAsync(out, pc->d.p, (size_t)pc->n, hipMemcpyDeviceToHost, p->stream) != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess) { (void)hipGetLastError(); return PHI_ERR_DEVICE; }
    return PHI_OK;
}

int phi_text_park_release(phi_text_park *p, int32_t index)
{
    phi_text_park::Piece *pc = park_piece(p, index);
    if (!pc) return PHI_ERR_INVALID;
    // The buffer stays with the park (the next piece takes it; phi_text_park_destroy frees them all): a hipFree per piece would
    // wait for the device each time -- between the chunks of a stream whose sketches are meant to overlap -- and 165 of them at
    // the end of config 5's reads are time inside whatever runs next.
    if (pc->ev) { (void)hipEventSynchronize(pc->ev); (void)hipEventDestroy(pc->ev); pc->ev = nullptr; }
    std::lock_guard<std::mutex> lk(p->mu);
    p->spare.push_back(pc->d);
    pc->d = DevBuf{};
    return PHI_OK;
}

void phi_text_park_destroy(phi_text_park *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->stream);
    for (auto &pc : p->pieces) { if (pc.ev) (void)hipEventDestroy(pc.ev); if (pc.d.p) (void)hipFree(pc.d.p); }
    for (auto &d : p->spare) if (d.p) (void)hipFree(d.p);
    for (void *h : p->pinned) (void)hipHostUnregister(h);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

extern "C" int phi_inflate_to_device(int32_t device, const void *in, int64_t n, int64_t chunk_bytes, int32_t flags, void **d_out,
                                     int64_t *out_size, phi_inflate_info *info);      // inflate.hip

int phi_text_park_gzip_begin(phi_text_park *p, int64_t piece_bytes)
{
    if (!p || piece_bytes <= 0) return PHI_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    p->gz.clear();
    p->gz_piece = piece_bytes;
    p->gz_on = true;
    return PHI_OK;
}

int phi_text_park_gzip_add(phi_text_park *p, const void *data, int64_t n)
{
    if (!p || !p->gz_on || n < 0 || (n > 0 && !data)) return PHI_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    p->gz.insert(p->gz.end(), (const char *)data, (const char *)data + n);
    return PHI_OK;
}

// the gathered stream inflated on the park's device (phi_inflate), its text cut into pieces of at most gz_piece bytes
int phi_text_park_gzip_end(phi_text_park *p, int32_t *first, int32_t *count, phi_inflate_info *info)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!p || !p->gz_on || !first || !count) return PHI_ERR_INVALID;
    *first = -1;
    *count = 0;
    p->gz_on = false;
    std::vector<char> gz;
    gz.swap(p->gz);
    void *d = nullptr;
    int64_t total = 0;
    int rc = phi_inflate_to_device(p->device, gz.data(), (int64_t)gz.size(), 0, 0, &d, &total, info);
    if (rc) return rc;
    std::vector<char>().swap(gz);
    if (hipSetDevice(p->device) != hipSuccess) { (void)hipFree(d); return PHI_ERR_DEVICE; }
    for (int64_t at = 0; at < total && !rc; at += p->gz_piece) {
        const int64_t n = std::min<int64_t>(p->gz_piece, total - at);
        phi_text_park::Piece pc;
        if ((rc = park_take_buffer(p, (size_t)n + 64, pc.d))) break;
        pc.n = n;
        if (hipMemcpy(&pc.first, (char *)d + at, 1, hipMemcpyDeviceToHost) != hipSuccess ||
            hipEventCreateWithFlags(&pc.ev, hipEventDisableTiming) != hipSuccess ||
            hipMemcpyAsync(pc.d.p, (char *)d + at, (size_t)n, hipMemcpyDeviceToDevice, p->stream) != hipSuccess ||
            hipEventRecord(pc.ev, p->stream) != hipSuccess) {
            (void)hipGetLastError();
            if (pc.ev) (void)hipEventDestroy(pc.ev);
            (void)hipFree(pc.d.p);
            rc = PHI_ERR_DEVICE;
            break;
        }
        std::lock_guard<std::mutex> lk(p->mu);
        p->pieces.push_back(pc);
        if (*first < 0) *first = (int32_t)p->pieces.size() - 1;
        (*count)++;
    }
    (void)hipStreamSynchronize(p->stream);                    // (the pieces' copies read d)
    (void)hipFree(d);
    return rc;
}

}  // extern "C"

// a parked piece's device bytes for the streams that take parked pieces (text_stream.hip, bam.hip): waits until they have landed
int phi_text_park_piece_dev(phi_text_park *p, int32_t index, int device, const void **d, int64_t *n, char *first)
{
    phi_text_park::Piece *pc = park_piece(p, index);
    if (!pc || p->device != device) return PHI_ERR_INVALID;
    if (pc->ev && hipEventSynchronize(pc->ev) != hipSuccess) { (void)hipGetLastError(); return PHI_ERR_DEVICE; }
    *d = pc->d.p; *n = pc->n;
    if (first) *first = pc->first;
    return PHI_OK;
}
