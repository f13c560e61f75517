// crc32_shift.h -- the CRC32 of gzip (RFC 1952) as arithmetic modulo its polynomial: the one place the polynomial is written.
// A register is a polynomial over GF(2) in the reflected form: bit 31 is x^0.  __host__ __device__: the kernels of deflate.hip
// and inflate.hip build their byte tables and shift their segments' registers with these, the host combines members with them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DFL_HD __host__ __device__ inline
#else
#define DFL_HD inline
#endif

#define DFL_CRC_POLY 0xEDB88320u

// the register c after one more zero byte: c * x^8 mod P.  For c < 256 this is entry c of the byte table.
DFL_HD uint32_t dfl_crc_byte(uint32_t c)
{
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (DFL_CRC_POLY & (0u - (c & 1u)));
    return c;
}

// a * b mod P
DFL_HD uint32_t dfl_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 31; k >= 0; k--) {
        if ((a >> k) & 1u) p ^= b;
        b = (b >> 1) ^ (DFL_CRC_POLY & (0u - (b & 1u)));       // b * x
    }
    return p;
}

// the register c (zero initial value, no final inversion) after nbytes more zero bytes: c * x^(8 nbytes) mod P
DFL_HD uint32_t dfl_crc_shift(uint32_t c, uint32_t nbytes)
{
    uint32_t sq = 0x00800000u;                                  // x^8
    for (int k = 0; k < 32 && nbytes; k++, nbytes >>= 1) {
        if (nbytes & 1u) c = dfl_crc_mul(c, sq);
        sq = dfl_crc_mul(sq, sq);
    }
    return c;
}
