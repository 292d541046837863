// match_select.h -- which kernel a *_match_span_batch call runs (match.hip), decided on the host from query_len and ref_stride alone.
// Plain host code with no HIP in it: tests/host/match_select_main.cpp sweeps it under the sanitizers.
#pragma once
#include <cstdint>

namespace vbzhip {

// The start field of a packed key: sb = ceil(log2 N), so every start 0 ... N - 1 fits (N >= 1).
inline uint32_t match_span_start_bits(uint32_t N)
{
    uint32_t sb = 0;
    while ((UINT64_C(1) << sb) < N) ++sb;
    return sb;
}

// The packed kernel keeps a cell as cost << sb | start in one 32-bit word, its far value at bit 31.  It is sound when
//     255 ref_stride < 2^(31 - sb)   and   sb <= 16
// (the proof: match.hip, at match_span_kernel).  Everything else inside the header's limits runs the wide kernel.
inline bool match_span_packed(uint32_t N, uint32_t ref_stride)
{
    const uint32_t sb = match_span_start_bits(N);
    return sb <= 16u && UINT64_C(255) * ref_stride < (UINT64_C(1) << (31u - sb));
}

}  // namespace vbzhip
