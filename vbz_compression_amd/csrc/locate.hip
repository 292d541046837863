// locate.hip -- signal locate (vbz_gpu_*_locate_batch; the rule: include/vbz_gpu.h): every read's whole quantised prefix aligned to a
// stretch of every row of a matrix of long int8 target squiggles, one wavefront per (read, target) pair.  match.hip with the operands
// exchanged: the DP is symmetric, so schedule and cell are match_pair's.
//
// Layout.  The lanes of a wavefront are the QUERY: lane l owns rows l C ... l C + C - 1 of the cost matrix, C the smallest of 1, 2, 4, 8,
// 16, 32 with 64 C >= n (one kernel; a wavefront picks its instantiation by its read's n, which only the device knows).  Each lane
// quantises its own C floats once, before the loop.  The four wavefronts of a workgroup take four reads against ONE target row: the
// stream is fetched once per workgroup from memory and three times from cache.
// Schedule.  Systolic: at step t lane l takes target level j = t - l.  A step is two wave_shr:1 DPP moves -- the lane below's last row
// for this level, and the level itself -- and then C cells down the lane's rows in registers: v_min3_u32 of {diagonal, above, left},
// v_msad_u8 for |k - g| + min.  No LDS, no barrier, no atomics.
// The cell's cost.  v_msad_u8 sums |a - b| over the four bytes, skipping the bytes where the LANE-RESIDENT operand is 0, plus an
// accumulator.  A query level k (-127 ... 127, never -128) is the word k + 128: byte 0 is 1 ... 255 and counts.  A streamed level g is
// the byte g + 128, 0 ... 255: -128 is byte 0, which needs no case of its own because the mask is not taken from the streamed operand.
// A row at or behind n is the word 0: every cell of it costs nothing, so it holds the running minimum of the row above it -- the last row
// of lane la, the lane of row n - 1, is then the running minimum of D[n - 1][.] whatever n is, tracked on one register with a strict <,
// which keeps the first j.
// The stream is int8: a dword a lane is 256 steps, requested a block ahead; the level of step t goes to lane 0 by v_readlane under a
// scalar index (one for four steps) and a scalar field extraction.
// Boundaries fall out of the initial values, as in match_pair.  Lane 0's incoming pair is the DPP's 0: row 0 is c(0, j), the free start.
// Every D[.][-1] starts at 2^30.  Nothing wraps, for L + la <= 2^30 + 63 steps: (a) a true value is D[i][j] <= 255 (i + 1) <= 255 n < 2^20
// however long the stream is -- a path may leave row i along column j alone.  (b) A lane that has not yet met level 0 (t < l) computes
// on far values alone; that state lasts at most 63 steps and a value grows by at most 255 a step, so far values stay inside
// [2^30, 2^30 + 63 * 255]: above every true value, and a minimum of a true value and a far one is the true one.  (c) A lane that has
// passed level L - 1 computes on whatever it is handed -- bytes behind L, or 0x80 behind the row -- for at most 63 steps more, from values
// below 2^20; only lanes in the same state read that, and lane la never is in it: its last level is the last step.  (d) The step counter
// reaches L + 63 <= 2^30 + 63 and end <= 2^30: both fit 32 bits.
// VALU instructions in the disassembly (profiles/locate_kernel_resources.txt).  A turn of the loop is four steps, one dword of the stream:
// 8 DPP moves, 1 v_readlane, 4 v_min_u32 / v_cmp / v_cndmask of the running minimum, 12 v_mov_b32, and v_min3_u32 + v_msad_u8 per row
// and step -- 41, 49, 65, 97, 161, 289 a turn for C = 1, 2, 4, 8, 16, 32: 8.25 + 2 C a step against match_pair's 9 + 2 C.
#include "vbz_kernels.h"

namespace vbzhip {
namespace {

constexpr uint32_t LOCATE_FAR = 1u << 30;   // D[.][-1]

// the match rule's quantisation of one converted sample, as the cell's lane-resident word: k + 128, 1 ... 255 (NaN: level 0)
__device__ __forceinline__ uint32_t locate_level(float z, float quant)
{
    const float v = z * quant;
    const float r = fminf(fmaxf(rintf(v), -127.0f), 127.0f);   // (NaN: fmaxf gives -127; taken out below)
    return v != v ? 128u : (uint32_t)((int)r + 128);
}

// One pair.  q: the read's query row, n >= 1 its valid samples, 64 C >= n; row: the target row (16-byte aligned), L >= 1 levels, and
// (L + 3) / 4 dwords of it may be read (L <= target_stride, a multiple of 16).
template <int C>
__device__ __forceinline__ uint2 locate_pair(const float* __restrict__ q, uint32_t n, float quant, const int8_t* __restrict__ row, uint32_t L)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t la = (n - 1u) / (uint32_t)C;   // the lane that holds row n - 1
    uint32_t k[C], cur[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const uint32_t r = lane * (uint32_t)C + (uint32_t)i;
        k[i] = r < n ? locate_level(q[r], quant) : 0u;   // (no address behind n)
        cur[i] = LOCATE_FAR;
    }
    uint32_t diag = lane == 0 ? 0u : LOCATE_FAR;   // D[l C - 1][j - 1]: what `up` was a step ago
    uint32_t g = 0;                                // this lane's level
    // Lane la's last row, step by step: far while t < la, then the running minimum of D[n - 1][0 ... t - la]; its last level is the last
    // step.  A strict < therefore keeps the first step that attains the minimum, and no step needs a mask.
    uint32_t best = 0xFFFFFFFFu, best_t = 0;
    const uint32_t steps = L + la;   // level L - 1 reaches lane la at step L - 1 + la
    const uint32_t* const words = reinterpret_cast<const uint32_t*>(row);
    const uint32_t n_words = (L + 3u) / 4u;
    uint32_t w = lane < n_words ? words[lane] : 0u;
    for (uint32_t t0 = 0; t0 < steps; t0 += 256u) {
        const uint32_t lv = w ^ 0x80808080u;   // four levels + 128
        const uint32_t next = t0 / 4u + 64u + lane;
        w = next < n_words ? words[next] : 0u;   // (in flight while this block is walked)
        const uint32_t block = steps - t0 < 256u ? steps - t0 : 256u;
        // (an even number of steps a turn, as in match_pair: one step leaves every row in another register, the next brings them back)
        auto step = [&](uint32_t s, uint32_t g0) {
            const uint32_t up = wave_prev_lane_u32(cur[C - 1]);   // D[l C - 1][j]; lane 0: 0
            g = (uint32_t)__builtin_amdgcn_update_dpp((int)g0, (int)g, 0x138, 0xF, 0xF, false);   // the lane below's level; lane 0: level t
            uint32_t d = diag, u = up;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const uint32_t left = cur[i];
                u = __builtin_amdgcn_msad_u8(g, k[i], min(min(d, u), left));
                d = left;
                cur[i] = u;
            }
            diag = up;
            const bool less = u < best;
            best = less ? u : best;
            best_t = less ? t0 + s : best_t;
        };
        uint32_t s = 0;
        for (; s + 4u <= block; s += 4u) {
            const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)lv, (int)(s >> 2));
            step(s, x & 0xFFu);
            step(s + 1u, (x >> 8) & 0xFFu);
            step(s + 2u, (x >> 16) & 0xFFu);
            step(s + 3u, x >> 24);
        }
        for (; s < block; ++s) {
            const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)lv, (int)(s >> 2));
            step(s, (x >> (8u * (s & 3u))) & 0xFFu);
        }
    }
    // lane la holds the answer: every lane gets it
    const uint32_t cost = (uint32_t)__builtin_amdgcn_readlane((int)best, (int)la);
    const uint32_t end = (uint32_t)__builtin_amdgcn_readlane((int)best_t, (int)la) - la + 1u;
    return make_uint2(cost, end);
}

// grid (ceil(n_reads / 4), G); wavefront w of a workgroup: read 4 blockIdx.x + w against target blockIdx.y
__global__ __launch_bounds__(256) void locate_kernel(uint32_t n_reads, const float* __restrict__ query, const uint32_t* __restrict__ valid, uint32_t N,
                                                     float quant, const int8_t* __restrict__ target, const uint32_t* __restrict__ target_len, uint32_t G,
                                                     uint32_t target_stride, uint2* __restrict__ out)
{
    const uint32_t read = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t tg = blockIdx.y;
    if (read >= n_reads) return;
    const uint32_t n0 = valid[read], n = __builtin_amdgcn_readfirstlane(n0 < N ? n0 : N);
    const uint32_t L = __builtin_amdgcn_readfirstlane(target_len[tg]);
    uint2 hit = make_uint2(0xFFFFFFFFu, 0u);
    if (n != 0 && L != 0 && L <= target_stride) {   // (no address from a length that fails here; N <= 2048: 32 rows a lane hold every n)
        const float* const q = query + (size_t)read * N;
        const int8_t* const row = target + (size_t)tg * target_stride;
        if (n <= 64u) hit = locate_pair<1>(q, n, quant, row, L);
        else if (n <= 128u) hit = locate_pair<2>(q, n, quant, row, L);
        else if (n <= 256u) hit = locate_pair<4>(q, n, quant, row, L);
        else if (n <= 512u) hit = locate_pair<8>(q, n, quant, row, L);
        else if (n <= 1024u) hit = locate_pair<16>(q, n, quant, row, L);
        else hit = locate_pair<32>(q, n, quant, row, L);
    }
    if ((threadIdx.x & 63u) == 0) out[(size_t)read * G + tg] = hit;   // (one 8-byte vector store)
}

}  // namespace

hipError_t launch_locate(uint32_t n_reads, const float* query, const uint32_t* valid, uint32_t N, float quant, const int8_t* target,
                         const uint32_t* target_len, uint32_t G, uint32_t target_stride, void* out, hipStream_t s)
{
    if (n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(locate_kernel, dim3((n_reads + 3u) / 4u, G), dim3(256), 0, s, n_reads, query, valid, N, quant, target, target_len, G, target_stride,
                       reinterpret_cast<uint2*>(out));
    return hipGetLastError();
}

}  // namespace vbzhip
