// bam_header.cpp -- phi_bam_header of include/phi_host.h: the header of a BAM stream from a prefix of its inflated bytes
// (../bam_header.h holds the parser; the device stream of bam.hip compiles the same copy).
#include "../../../include/phi_host.h"
#include "../bam_header.h"

extern "C" int phi_bam_header(const void *bytes, int64_t n, int64_t *records_start, int32_t *n_ref, char *err, int err_cap)
{
    const int r = phi_bam_header_parse(bytes, n, records_start, n_ref, err, err_cap);
    return r == PHI_BAM_HDR_OK ? PHI_HOST_OK : r == PHI_BAM_HDR_MORE ? PHI_HOST_NEED_MORE : PHI_HOST_ERR_INVALID;
}
