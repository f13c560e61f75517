// bam_header.h -- the header of a BAM stream (SAM/BAM specification, section 4.2), parsed on the host from a prefix of the
// inflated bytes: plain C++, no allocation, every read checked against the bytes at hand.  One copy, used by
// phi_bam_header (include/phi_host.h, libphi_host.so: the command line, the Python mirror) and by the device stream of
// bam.hip, which needs the place where the records start before any kernel runs.
//
//   magic "BAM\1" | l_text int32 | text[l_text] | n_ref int32 | n_ref x ( l_name int32 | name[l_name] | l_ref int32 )
//
// All integers little-endian.  The header's size is known only once l_text and every l_name have been read.
#pragma once
#include <stdint.h>
#include <stdio.h>

enum { PHI_BAM_HDR_OK = 0, PHI_BAM_HDR_MORE = 1, PHI_BAM_HDR_BAD = -1 };

static inline int32_t phi_bam_le32(const unsigned char *p)
{
    return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}

// OK: *records_start = the first record's offset, *n_ref.  MORE: the n bytes are a prefix of a header that may still be
// valid; *records_start = a lower bound of the bytes needed (> n).  BAD: not a BAM header; err names the byte offset.
static inline int phi_bam_header_parse(const void *bytes, int64_t n, int64_t *records_start, int32_t *n_ref, char *err, int err_cap)
{
    const unsigned char *b = (const unsigned char *)bytes;
    static const unsigned char magic[4] = {'B', 'A', 'M', 1};
    if (err && err_cap > 0) err[0] = 0;
    if (records_start) *records_start = 0;
    if (n_ref) *n_ref = 0;
    if (n < 0 || (n > 0 && !b)) { if (err) snprintf(err, (size_t)err_cap, "BAM header: bad arguments"); return PHI_BAM_HDR_BAD; }
    for (int64_t i = 0; i < 4 && i < n; i++)
        if (b[i] != magic[i]) {
            if (err) snprintf(err, (size_t)err_cap, "not a BAM stream: byte %lld is 0x%02x, the magic is BAM\\1", (long long)i, (unsigned)b[i]);
            return PHI_BAM_HDR_BAD;
        }
    int64_t at = 4;
    auto more = [&](int64_t need) { if (records_start) *records_start = need; return (int)PHI_BAM_HDR_MORE; };
    if (n < at + 4) return more(at + 4);
    const int32_t l_text = phi_bam_le32(b + at);
    if (l_text < 0) { if (err) snprintf(err, (size_t)err_cap, "BAM header: l_text = %d at byte offset %lld", (int)l_text, (long long)at); return PHI_BAM_HDR_BAD; }
    at += 4 + (int64_t)l_text;
    if (n < at + 4) return more(at + 4);
    const int32_t nr = phi_bam_le32(b + at);
    if (nr < 0) { if (err) snprintf(err, (size_t)err_cap, "BAM header: n_ref = %d at byte offset %lld", (int)nr, (long long)at); return PHI_BAM_HDR_BAD; }
    at += 4;
    for (int32_t r = 0; r < nr; r++) {
        // what is still to come is at least 9 bytes per reference (an l_name of 1)
        if (n < at + 4) return more(at + 9 * (int64_t)(nr - r));
        const int32_t l_name = phi_bam_le32(b + at);
        if (l_name < 1) { if (err) snprintf(err, (size_t)err_cap, "BAM header: l_name = %d of reference %d at byte offset %lld", (int)l_name, (int)r, (long long)at); return PHI_BAM_HDR_BAD; }
        at += 4 + (int64_t)l_name + 4;
        if (n < at) return more(at + 9 * (int64_t)(nr - r - 1));
    }
    if (records_start) *records_start = at;
    if (n_ref) *n_ref = nr;
    return PHI_BAM_HDR_OK;
}
