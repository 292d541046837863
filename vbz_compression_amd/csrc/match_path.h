// match_path.h -- what the kernels of match.hip and locate.hip share: the quantiser, the ladder over rows per lane, the keys (cost, start)
// of a cell, a path kernel's pair and the traceback over a pair's direction bits.  Device code; both files include it inside their own
// translation unit.
#pragma once
#include <type_traits>

#include "vbz_kernels.h"

// A lambda handed to with_rows is part of the kernel's one body, like a __forceinline__ function: stated after its parameters.
#define VBZ_LAMBDA_INLINE __attribute__((always_inline))

namespace vbzhip {
namespace {

// The rule's quantisation of one converted sample: the level k + 128, 1 ... 255 (NaN: level 0, the byte 128).  match.hip streams it as the
// cell's query word, match_level; locate.hip keeps it in the lanes.
__device__ __forceinline__ uint32_t align_level(float z, float quant)
{
    const float v = z * quant;
    const float r = fminf(fmaxf(rintf(v), -127.0f), 127.0f);   // (NaN: fmaxf gives -127; taken out below)
    return v != v ? 128u : (uint32_t)((int)r + 128);
}
__device__ __forceinline__ uint32_t match_level(float z, float quant) { return align_level(z, quant) | 0x100u; }

// The ladder over rows per lane: f(std::integral_constant<int, C>) for the smallest C of 1, 2, 4, 8, 16, 32 with 64 C >= len (len <= 2048).
// tests/locate_ref.py states the thresholds again as the reference.  match_kernel, match_span_body and locate_span_kernel keep the
// ladder written out: through with_rows the compiler emits the same instructions for them in another order and with other scalar
// registers (profiles/align_restate_isa.txt), and this header was to leave every code object as it was.
template <typename F>
__device__ __forceinline__ void with_rows(uint32_t len, F&& f)
{
    if (len <= 64u) f(std::integral_constant<int, 1>{});
    else if (len <= 128u) f(std::integral_constant<int, 2>{});
    else if (len <= 256u) f(std::integral_constant<int, 4>{});
    else if (len <= 512u) f(std::integral_constant<int, 8>{});
    else if (len <= 1024u) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 32>{});
}


// The cell's cost is one v_msad_u8: the sum over the four bytes of |a - b|, skipping the bytes where the REFERENCE operand is 0, plus
// an accumulator.  Query level k (-127 ... 127) is the word {k + 128, 1, 0, 0}; reference level r >= -127 is {r + 128, 0, 0, 0}, so its
// byte 0 is 1 ... 255 and counts, byte 1 does not; r = -128 is {1, 2, 0, 0}: |k + 127| + 1.  A row behind the reference's end is the word 0:
// every cell of it costs nothing, so it holds the running minimum of the row above it -- the last row of lane la is then the running
// minimum of D[M - 1][.] whatever M is, and the answer is tracked on a fixed register.
__device__ __forceinline__ uint32_t match_ref_word(int r) { return r == -128 ? 0x0201u : (uint32_t)(r + 128); }

// PackedKey: cost << sb | start in one word, sb = ceil(log2 N) from the host; the far value is bit 31.  The cell's cost has to land in the
// cost field, where v_msad_u8 cannot add it; v_sad_u32 over levels shifted by sb can: a cell is v_min3_u32 and v_sad_u32, two instructions
// as in match_pair (v_msad_u8 with accumulator 0 and v_lshl_add_u32 was three: 10 + 3 c a step against 10 + 2 c, 1.36 - 1.47 against
// 1.01 - 1.03 times match_kernel's time).  v_sad_u32 has no mask, so rows behind the reference's end cost something: they are SINKS -- a
// row reads rows above it alone, so no true cell and not the answer depends on them, whatever they hold or wrap to -- and the tracked row is
// row (M - 1) mod C of lane la itself, chosen once by a scalar switch over C instantiations of the loop (match_span_rows) where C - 1
// selects a step would have cost what the third instruction did.  The rule (match_select.h):
//     255 ref_stride < 2^(31 - sb)   and   sb <= 16.
// Proof that nothing wraps and that far stays far, for rows 0 ... M - 1.  (a) A true cell D[i][j] is <= 255 (i + 1) <= 255 M <=
// 255 ref_stride and a start is < 2^sb, so a true key is < (255 ref_stride + 1) 2^sb <= 2^31: below the far value.  (b) A lane that has not met sample 0 computes on far
// values alone (its rows, its diag, and the `up` of a lane in the same state; lane 0 is never in it): every value is >= 2^31 and a row
// grows by at most 255 2^sb a step, since a cell is <= its `left` plus one cost.  That state lasts at most 63 steps, so these values stay
// below 2^31 + 63 * 255 * 2^16 < 2^32.  D[.][-1], which is such a row when sample 0 arrives, is therefore above every true key, and the
// minimum of a true key and one of these is the true key.  (c) A lane that has passed sample n - 1 computes on whatever it is handed (lane
// 0's `up` is then a step number >= n, which may not fit the start field), and may wrap: only lanes in the same state read that, and the
// lane that holds the answer never is in it -- its last sample is the last step.
// WideKey: the pair in two registers as one 64-bit key, cost << 32 | start, far at bit 62: v_msad_u8 adds the cost straight into the high
// word and nothing comes near a wrap.  For calls outside the packed rule; held to correctness only.
struct PackedKey
{
    using T = uint32_t;
    static constexpr bool FREE_ROWS = false;
    uint32_t sb;
    __device__ __forceinline__ T far() const { return 1u << 31; }
    __device__ __forceinline__ T prev_lane(T v, uint32_t j) const { return (T)__builtin_amdgcn_update_dpp((int)j, (int)v, 0x138, 0xF, 0xF, false); }
    // levels as words in the cost field: r + 128 and k + 128, 0 ... 255 (-128 needs no case of its own here)
    __device__ __forceinline__ uint32_t ref_word(int r) const { return (uint32_t)(r + 128) << sb; }
    __device__ __forceinline__ uint32_t query_word(uint32_t level) const { return (level & 0xFFu) << sb; }
    __device__ __forceinline__ T cell(uint32_t k, uint32_t r, T d, T u, T left) const
    {
        return (k > r ? k - r : r - k) + min(min(d, u), left);   // v_min3_u32, v_sad_u32
    }
    __device__ __forceinline__ T uniform(T v, uint32_t lane) const { return (T)__builtin_amdgcn_readlane((int)v, (int)lane); }
    __device__ __forceinline__ uint32_t cost(T key) const { return key >> sb; }
    __device__ __forceinline__ uint32_t start(T key) const { return key & ((1u << sb) - 1u); }
};
struct WideKey
{
    using T = uint64_t;
    static constexpr bool FREE_ROWS = true;
    __device__ __forceinline__ T far() const { return (T)1 << 62; }
    __device__ __forceinline__ T prev_lane(T v, uint32_t j) const
    {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)j, (int)(uint32_t)v, 0x138, 0xF, 0xF, false);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x138, 0xF, 0xF, false);
        return (T)hi << 32 | lo;
    }
    __device__ __forceinline__ uint32_t ref_word(int r) const { return match_ref_word(r); }
    __device__ __forceinline__ uint32_t query_word(uint32_t level) const { return level; }
    __device__ __forceinline__ T cell(uint32_t k, uint32_t r, T d, T u, T left) const
    {
        const T m = min(min(d, u), left);
        return (T)__builtin_amdgcn_msad_u8(k, r, (uint32_t)(m >> 32)) << 32 | (uint32_t)m;
    }
    __device__ __forceinline__ T uniform(T v, uint32_t lane) const
    {
        return (T)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)lane) << 32 |
               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane);
    }
    __device__ __forceinline__ uint32_t cost(T key) const { return (uint32_t)(key >> 32); }
    __device__ __forceinline__ uint32_t start(T key) const { return (uint32_t)key; }
};

// a direction bit is the sign of a difference (match.hip, at match_path_forward)
__device__ __forceinline__ uint32_t match_sign_less(uint32_t a, uint32_t b) { return a - b; }                       // bit 31: a < b
__device__ __forceinline__ uint32_t match_sign_less(uint64_t a, uint64_t b) { return (uint32_t)((a - b) >> 32); }

// Pair pi = first + w of a path launch (AlignPathArgs: vbz_kernels.h), uniform: {read, ref or target, begin, end}
__device__ __forceinline__ uint4 path_pair(const AlignPathArgs& p, size_t pi)
{
    const uint4 pl = p.pairs[pi];
    return make_uint4(__builtin_amdgcn_readfirstlane(pl.x), __builtin_amdgcn_readfirstlane(pl.y), __builtin_amdgcn_readfirstlane(pl.z),
                      __builtin_amdgcn_readfirstlane(pl.w));
}

// The traceback of one pair, by its whole wavefront: the walk over the bit-matrix a forward pass left (match.hip, at match_path_forward:
// the layout), which does not know which operand sat in the lanes.  M >= 1: the rows of the cost matrix, the operand in the lanes, c rows
// a lane by M; a: the window's first column; W >= 1 its width; bits: the pair's words; rows: the pair's M entries.  It writes rows
// 0 ... M - 1 and returns the column where the path starts.  The walk cannot leave the pair's words or run on whatever the bits hold:
// every step lowers i or j, and j == 0 forces up.  The walk itself is one dependent chain whoever walks it, so the whole wavefront
// walks it in scalar registers; what the wavefront adds is the fetch: the 64 words of lane l's stream that end at the word the walk needs are loaded
// by one instruction, lane k taking word g - k, and a step reads its word out of that register by v_readlane.  Inside a lane's stream
// the walk only moves to smaller cell numbers (up: one cell, left: c cells), so a fetch serves 1 024 cells -- 1 024 / c columns -- or lasts
// until the walk crosses into the lane above.  Rows leave 64 at a time: lane i mod 64 keeps row i, and the 64 lanes store a 512-byte
// stretch when the walk leaves row 64 k.
__device__ __forceinline__ uint32_t match_path_walk(uint32_t M, uint32_t a, uint32_t W, const uint32_t* __restrict__ bits, uint2* __restrict__ rows)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lc = 0;   // log2 c
    with_rows(M, [&](auto C) VBZ_LAMBDA_INLINE { lc = (uint32_t)__builtin_ctz((unsigned)C()); });
    uint32_t i = M - 1u, j = W - 1u, end = j + 1u;
    uint32_t have_l = 0xFFFFFFFFu, top = 0, cache = 0;   // lane k holds word top - k of lane have_l's stream
    uint2 mine = make_uint2(0u, 0u);
    for (;;) {
        uint32_t dir = 2u;   // 0, 1: diagonal; 2: up (row 0: stop); 3: left.  Column a: up
        if (j != 0) {
            const uint32_t l = i >> lc, cell = ((j + l) << lc) + (i & ((1u << lc) - 1u)), g = cell >> 4;
            if (l != have_l || g > top || g + 63u < top) {
                have_l = l, top = g;
                cache = lane <= g ? bits[(size_t)(g - lane) * 64u + l] : 0u;
            }
            const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)cache, (int)(top - g));
            dir = (word >> (30u - 2u * (cell & 15u))) & 3u;
            if (i == 0) dir |= 2u;   // (row 0 has no diagonal step: b1 alone)
        }
        if (dir == 3u) {
            --j;
            continue;
        }
        if (i == 0) break;
        if (lane == (i & 63u)) mine = make_uint2(a + j, a + end);
        if ((i & 63u) == 0 && i + lane < M) rows[i + lane] = mine;   // rows i ... i + 63 are walked
        --i;
        if (dir < 2u) --j;
        end = j + 1u;
    }
    if (lane == 0) mine = make_uint2(a + j, a + end);
    if (lane < M) rows[lane] = mine;
    return a + j;
}

}  // namespace
}  // namespace vbzhip
