// sq_index.hpp -- what the two translation units of the IVFSQ index share: the index itself.  sq_index.hip: geometry, quantiser, add,
// build, the canonical search, export and files; sq_candidates.hip: the int8 matrix-core candidate search (sq_cand_kernels.hpp).
#pragma once

#include "coded_ivf.hpp"

namespace msvs
{
constexpr const char * SQ = "IVFSQ";
}

struct msvs_sq_index : msvs::CodedIvf // ld = round_up(dim, 16), row_bytes = 16 sq_row_words(bits, ld); codes: max(n, 1) rows, not zeroed
{
    uint32_t bits = 8;                 // 4, 8 or 16
    std::vector<float> h_vmin, h_vmax; // dim
    msvs::DevBuf<float> d_vmin, d_step; // ld each, zero padded (bits 16: none, the range enters no arithmetic)
    // prepare_candidates (bits 8 only; device only, never in a file): empty until then
    bool cand_ready = false;
    msvs::DevBuf<float> d_erow; // L2: max(n, 1) row terms E_row, list-major
};
