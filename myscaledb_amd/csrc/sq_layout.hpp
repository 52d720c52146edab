// sq_layout.hpp -- the stored order of an IVFSQ row (sq_ivf_kernels.hpp, sq_index.hip) for its three code widths: plain C++, shared by
// the encoder, the scan, export / serialize / load and the host test.
//
// A row is ld = round_up(dim, 16) columns.  The scan gives lane g of a 16-lane group the float4 columns g, g + 16, ... (column c =
// natural columns 4 c .. 4 c + 3) and fetches 16 bytes per lane at a time; inside every WHOLE block of 256 stored bytes the codes
// are permuted so that the 16 bytes at offset 256 b + 16 g are E of lane g's own columns in its accumulation order:
//   bits  8 : E = 4, a block is 256 columns: byte 4 e + i of the lane's 16 = component i of column 64 b + g + 16 e;
//   bits  4 : E = 8, a block is 512 columns: byte 4 w + i of the lane's 16 holds component i of column 128 b + g + 16 (2 w) in its
//             low nibble and of column 128 b + g + 16 (2 w + 1) in its high nibble (w & 0x0f0f0f0f and (w >> 4) & 0x0f0f0f0f are
//             two words of four byte-codes each);
//   bits 16 : E = 2, a block is 128 columns: half 4 e + i of the lane's 8 = component i of column 32 b + g + 16 e.
// The tail (the columns beyond the last whole block) stays in natural order: code j in byte j (8), in byte j / 2, low nibble for
// even j (4), in half j (16).  Blocks are counted by ld, so every column of a block exists in the padded query and centroid rows.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MSVS_HD __host__ __device__
#else
#ifndef MSVS_HD
#define MSVS_HD
#endif
#endif

namespace msvs
{

/// 16-byte words of a stored row of ld columns: ld bytes (8), round_up(ld / 2, 16) = round_up(ceil(dim / 2), 16) bytes (4), 2 ld bytes (16)
MSVS_HD inline uint32_t sq_row_words(uint32_t bits, uint32_t ld) { return bits == 4 ? (ld + 31) >> 5 : (bits == 16 ? ld >> 3 : ld >> 4); }

/// bits 8: byte of natural column j (< ld) inside a stored row of ld bytes
MSVS_HD inline uint32_t sq_stored_pos(uint32_t j, uint32_t ldc)
{
    if (j >= (ldc & ~255u))
        return j;
    const uint32_t c = (j & 255u) >> 2; // float4 column inside the block
    return (j & ~255u) + ((c & 15u) << 4) + ((c >> 4) << 2) + (j & 3u);
}

/// bits 4: NIBBLE of natural column j (< ld) inside a stored row: nibble p is the low (p even) or high (p odd) half of byte p / 2
MSVS_HD inline uint32_t sq4_stored_pos(uint32_t j, uint32_t ld)
{
    if (j >= (ld & ~511u))
        return j;
    const uint32_t c = (j & 511u) >> 2, e = c >> 4; // float4 column inside the block; which of the lane's eight
    const uint32_t byte = ((j & ~511u) >> 1) + ((c & 15u) << 4) + ((e >> 1) << 2) + (j & 3u);
    return 2 * byte + (e & 1u);
}

/// bits 4: the natural columns whose codes stored byte p (< 16 sq_row_words(4, ld)) holds in its low and high nibble; a column >= ld
/// is padding (tail bytes beyond ld / 2)
MSVS_HD inline void sq4_stored_cols(uint32_t p, uint32_t ld, uint32_t & lo, uint32_t & hi)
{
    if (p >= ((ld & ~511u) >> 1))
    {
        lo = 2 * p;
        hi = 2 * p + 1;
        return;
    }
    const uint32_t g = (p >> 4) & 15u, w = (p >> 2) & 3u;
    lo = ((p & ~255u) << 1) + ((g + 32 * w) << 2) + (p & 3u);
    hi = lo + 64;
}

/// bits 16: half of natural column j (< ld) inside a stored row of ld halves
MSVS_HD inline uint32_t sq16_stored_pos(uint32_t j, uint32_t ld)
{
    if (j >= (ld & ~127u))
        return j;
    const uint32_t c = (j & 127u) >> 2;
    return (j & ~127u) + ((c & 15u) << 3) + ((c >> 4) << 2) + (j & 3u);
}

}
