// squiggle_bases.h -- what the kernels of squiggle.hip and pile.hip share: the cut of a squiggle row over lanes, a row's length under an
// untrusted seq_len, a lane's 24 strand bases and the roll of the k-mer index over them, and the test that makes a pair of the levels
// arena valid.  Device code; both files include it inside their own translation unit.
#pragma once
#include "vbz_kernels.h"

namespace vbzhip {
namespace {

// The cut.  A lane makes SQ_LANE = 16 consecutive positions of a row, a wavefront's tile is 1 024 positions, a workgroup's 4 096.
constexpr uint32_t SQ_KMAX = 9, SQ_LANE = 16, SQ_WAVE = 64u * SQ_LANE, SQ_BLOCK = 4u * SQ_WAVE;

// the strand's length and the row's L under an untrusted seq_len
__device__ __forceinline__ uint32_t squiggle_len(const uint32_t* seq_len, uint32_t seq_stride, uint32_t k, uint32_t target_stride, uint32_t s, uint32_t& n)
{
    n = seq_len[s];
    if (n > seq_stride) n = 0;   // (no address is formed from it)
    const uint32_t L = n >= k ? n - k + 1u : 0u;
    return L > target_stride ? 0u : L;
}

// Four bases of a dword as codes A 0, C 1, G 2, T/U 3 in the bytes' low bits ((b >> 1) & 3 is A 0, C 1, T/U 2, G 3: x ^ (x >> 1) puts G
// and T right), complemented for the reverse strand; whether a byte IS one of the ten letters is asked per byte below.
__device__ __forceinline__ uint32_t base_codes(uint32_t w, bool rc)
{
    const uint32_t c = (w >> 1) & 0x03030303u;
    return c ^ ((c >> 1) & 0x01010101u) ^ (rc ? 0x03030303u : 0u);
}
__device__ __forceinline__ uint32_t base_invalid(uint32_t byte)
{
    const uint32_t i = (byte | 0x20u) - 0x61u;   // a 0, c 2, g 6, t 19, u 20; both bytes that give one of these are letters
    return i <= 20u ? (~(0x180045u >> i)) & 1u : 1u;
}

// The bases.  A lane's 16 k-mers are p = lo ... lo + 15 in STRAND order (lo = j0, or L - 16 - j0 with REVERSED), and they need the strand
// bases lo ... lo + 14 + k.  The lane loads the seven aligned dwords that cover its 24 bytes -- each only when it lies inside the row's
// seq_stride bytes, 0 otherwise -- and v_alignbyte_b32 shifts them into place; the reverse strand then swaps the bytes and the dwords
// (base_codes complements them).  Byte 0 of the 24 is strand base lo - (9 - k), so that byte i >= 8 closes k-mer lo + i - 8 whatever k is.
// -> lo; v: the 24 bytes in strand order.  lo may be negative and bytes at and behind n are the caller's junk: both reach only k-mers
// outside [0, L), which squiggle_roll_step never hands on.
__device__ __forceinline__ int32_t squiggle_bases(const uint8_t* seq, uint32_t seq_stride, uint32_t s, uint32_t n, uint32_t k, uint32_t L, uint32_t j0, bool rc,
                                                  bool reversed, uint32_t (&v)[6])
{
    const int32_t lo = reversed ? (int32_t)L - (int32_t)SQ_LANE - (int32_t)j0 : (int32_t)j0;   // (>= -15)
    const int32_t b0 = lo - (int32_t)(SQ_KMAX - k);                                            // the strand base of byte 0 (>= -23)
    const int32_t at = rc ? (int32_t)n - 1 - b0 - 23 : b0;                                     // the first of the 24 bytes in seq
    const int32_t d0 = at >> 2;                                                                // (floor)
    const uint32_t shift = (uint32_t)at & 3u, n_words = seq_stride / 4u;
    const uint32_t* const words = reinterpret_cast<const uint32_t*>(seq + (size_t)s * seq_stride);
    uint32_t w[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const uint32_t d = (uint32_t)(d0 + i);   // (a negative dword is a large one)
        w[i] = d < n_words ? words[d] : 0u;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], shift);
    if (rc) {   // the same bytes from the other end
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t x = __builtin_bswap32(v[i]);
            v[i] = __builtin_bswap32(v[5 - i]);
            v[5 - i] = x;
        }
    }
    return lo;
}

// The roll, one byte of it.  index = (index << 2 | code) & (4^k - 1); bad = (bad << 1 | invalid) & (2^k - 1): after k bases both describe
// exactly the last k, whatever came before (index_mask = 4^k - 1, bad_mask = 2^k - 1).  Byte i >= 8 closes the k-mer at p = lo + i - 8:
// -> whether it lies inside [0, L); index < 4^k by the mask, bad != 0 when it holds an invalid base.  The callers' loops over i = 0 ... 23
// are unrolled over constants, so entry e = i - 8 of a lane's registers is one in every turn.
__device__ __forceinline__ bool squiggle_roll_step(const uint32_t (&v)[6], uint32_t i, bool rc, uint32_t index_mask, uint32_t bad_mask, int32_t lo, uint32_t L,
                                                   uint32_t& index, uint32_t& bad)
{
    const uint32_t byte = (v[i / 4u] >> (8u * (i % 4u))) & 0xFFu, code = (base_codes(v[i / 4u], rc) >> (8u * (i % 4u))) & 3u;
    index = (index << 2 | code) & index_mask;
    bad = (bad << 1 | base_invalid(byte)) & bad_mask;
    if (i < SQ_KMAX - 1u) return false;
    const int32_t p = lo + (int32_t)(i - (SQ_KMAX - 1u));
    return p >= 0 && (uint32_t)p < L;
}

// A pair of the levels arena ({read, ref, begin, end}, hit {cost, end, start, n}, W = n_levels[p]) is valid -- its rows are target levels
// [start, end) of row ref -- by this test and no other; no address is formed from an unchecked value.
__device__ __forceinline__ bool levels_pair_valid(const uint4& pr, const uint4& h, uint32_t W, uint32_t n_reads, uint32_t G, uint32_t target_stride,
                                                  uint32_t max_width, const uint32_t* target_len)
{
    const uint32_t read = pr.x, ref = pr.y, end = h.y, start = h.z;
    bool valid = read < n_reads && ref < G && W != 0u && W <= max_width && end > start && end - start == W;
    if (valid) {
        const uint32_t Lg = target_len[ref];
        valid = Lg != 0u && Lg <= target_stride && end <= Lg;
    }
    return valid;
}

}  // namespace
}  // namespace vbzhip
