// match_path_groups.h -- the scratch of a vbz_gpu_match_path_batch call (match.hip): how many words of direction bits one pair takes, and
// how many pairs the host runs per group so that the bit-matrix stays under a cap.  Decided on the host from max_width, ref_stride and the
// cap alone.  Plain host code with no HIP in it: tests/host/match_path_groups_main.cpp sweeps it under the sanitizers.
#pragma once
#include <cstdint>

namespace vbzhip {

// Rows of the cost matrix a lane owns for a reference of `rows` levels: the smallest of 1, 2, 4, 8, 16, 32 with 64 c >= rows (rows <= 2048).
inline uint32_t match_rows_per_lane(uint32_t rows)
{
    uint32_t c = 1;
    while (c < 32u && UINT64_C(64) * c < rows) c *= 2;
    return c;
}

// One pair's bit-matrix in 32-bit words.  A cell is two bits; a lane packs its c cells of a step, step after step, into words of 16 cells,
// and word g of lane l stands at g * 64 + l.  A pair runs at most max_width + 63 steps and its reference has at most ref_stride rows:
// 64 * ceil((max_width + 63) c / 16) words, about 16 c max_width bytes.
inline uint64_t match_path_pair_words(uint32_t max_width, uint32_t ref_stride)
{
    const uint64_t cells = (UINT64_C(63) + max_width) * match_rows_per_lane(ref_stride);
    return UINT64_C(64) * ((cells + 15u) / 16u);
}

// Pairs per group: as many as fit `cap_bytes` of direction bits, at least one (a pair larger than the cap runs alone), at most n_pairs.
inline uint32_t match_path_group_pairs(uint32_t n_pairs, uint32_t max_width, uint32_t ref_stride, uint64_t cap_bytes)
{
    const uint64_t fit = cap_bytes / (match_path_pair_words(max_width, ref_stride) * 4u);
    const uint64_t g = fit < 1u ? 1u : fit;
    return g < n_pairs ? (uint32_t)g : (n_pairs < 1u ? 1u : n_pairs);
}

constexpr uint64_t MATCH_PATH_CAP_DEFAULT = UINT64_C(1) << 32;   // bytes of direction bits a group may take ("The path")

}  // namespace vbzhip
