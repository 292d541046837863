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

// ---- the start of the stretch (vbz_gpu_*_locate_span_batch) -------------------------------------------------------------------------------
// Phase 2, the walk back.  locate_pair gave (cost, end); the start is the SMALLEST s over the paths of that cost that end at column
// end - 1.  In reversed coordinates i' = n - 1 - i, j' = end - 1 - j that is the same systolic schedule with the query REVERSED in the lanes,
// the target streamed BACKWARDS from level end - 1, and an ANCHORED start: D'[-1][-1] = 0, every other D'[-1][.] and D'[.][-1] far -- lane
// 0's diag is 0 at step 0 and its incoming `up` is far at every step (the DPP leaves lane 0 its old value).  D'[i'][j'] is then the least cost
// of a path from that cell to (n - 1, end - 1), sits on the query's first level included, and
//     start = end - 1 - (the LARGEST j' with D'[n - 1][j'] == cost):
// an equality, tracked by lane la with v_cmp_eq / v_cndmask, the last hit kept.  D'[n - 1][j'] >= cost everywhere: it is the cost of an
// alignment of the whole query that ends at end - 1, and cost is the least of those.
// Padded rows.  Row n - 1 is register (n - 1) mod C of lane la, chosen by C - 1 selects a step under a scalar condition (the cheaper form to
// write: phase 2 is short).  A row behind n holds the word 0x100 here, not 0: byte 0 is skipped and byte 1 costs |0 - 1| = 1 against
// every streamed level (whose upper bytes are 0), so such a cell is 1 + a minimum over cells of row n - 1 and of padded rows: >= cost + 1
// by induction.  Padded rows feed no row in front of them and can never hold `cost`, which keeps them out of the stopping test unmasked.
// The stream.  Virtual step v = t + skip, skip = 3 - (end - 1) % 4: v = 0 is the top byte of the dword of level end - 1, so a block of 256
// virtual steps is 64 aligned dwords, descending, byte-swapped once a block so that step v takes byte v % 4; the first block starts at
// v = skip.  A dword index below 0 is not loaded.
// Stopping.  A lane's cell at step t is in column t - l.  Along a path the quantity f = j' + lane(i') grows by 0, 1 or 2 a step (right: 1;
// down: 0 or 1; diagonal: 1 or 2), starting from f = 0 at the anchor's cell.  So every path to a cell with f >= t + 2 passes through a cell
// with f = t or f = t + 1: a cell of the front of step t or of step t + 1, in a row < n and a column inside [0, end).  Costs are >= 0, so a
// path's cost is at least D' of any cell on it.  If every such cell of the two fronts exceeds `cost`, every later cell does, the tracked
// row's among them, and the walk ends: tested once a block behind its last two steps (a minimum over the lane's registers after each, one
// compare, one ballot).  Cells that have not met column 0 hold far values and cells of padded rows exceed `cost`, as the rule wants them;
// cells in front of the target's first level (lanes below la, for at most la steps, on zero dwords) can only delay the stop, and nothing
// they hold reaches a column inside the target.  The walk also ends at the target's first level: end + la steps.
// Nothing wraps.  (a) A true D' can be large here -- row 0 sums its costs along the whole walk -- so once a block every register is
// clamped to 2^30: a value grows by at most 255 a step (a cell is at most 255 + its left), so inside a block values stay below
// 2^30 + 256 * 255 < 2^31.  min and + are monotone: a computed value lies between min(true, 2^30) and true, so every value below 2^30 --
// all that can equal cost <= 255 n < 2^20 -- is exact.  (b) Far values start at 2^30 and obey the same bound.  (c) t <= end + 63 <= 2^30 + 63,
// start < end <= 2^30.
// VALU instructions in the disassembly (profiles/locate_span_kernel_resources.txt).  A turn of four steps: 8 DPP moves, 1 v_readlane, 4
// v_cmp_eq / v_cndmask of the last hit, 12 v_mov_b32, per row and step v_min3_u32 + v_msad_u8, and the C - 1 selects a step -- 37, 49, 73,
// 121, 217 a turn for C = 1 ... 16: 6.25 + 3 C a step against phase 1's 8.25 + 2 C; at C = 32 the compiler branches over half of the
// selects, 346 or 406 a turn.  Both phases in one kernel need 141 VGPRs as the compiler allocates them by itself; held to four wavefronts a
// SIMD it allocates 128 with no spill.
template <int C>
__device__ __forceinline__ uint32_t locate_back(const float* __restrict__ q, uint32_t n, float quant, const int8_t* __restrict__ row, uint32_t cost,
                                                uint32_t end)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t la = (n - 1u) / (uint32_t)C;        // the lane that holds reversed row n - 1 ...
    const uint32_t track = (n - 1u) % (uint32_t)C;     // ... in this register
    uint32_t k[C], cur[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const uint32_t r = lane * (uint32_t)C + (uint32_t)i;
        k[i] = r < n ? locate_level(q[n - 1u - r], quant) : 0x100u;   // (no address behind n)
        cur[i] = LOCATE_FAR;
    }
    uint32_t diag = lane == 0 ? 0u : LOCATE_FAR;   // D'[-1][-1]
    uint32_t g = 0;
    const uint32_t skip = 3u - ((end - 1u) & 3u);
    uint32_t last = skip + la;                     // the virtual step of the last D'[n - 1][.] == cost (lane la's alone means anything)
    const uint32_t vend = skip + end + la;         // level 0 reaches lane la at step end - 1 + la
    const uint32_t* const words = reinterpret_cast<const uint32_t*>(row);
    const int32_t top = (int32_t)((end - 1u) >> 2);
    int32_t at = top - (int32_t)lane;
    uint32_t w = at >= 0 ? words[at] : 0u;
    for (uint32_t v0 = 0; v0 < vend; v0 += 256u) {
        const uint32_t lv = __builtin_bswap32(w) ^ 0x80808080u;   // four levels + 128, the highest first
        at -= 64;
        w = at >= 0 ? words[at] : 0u;   // (in flight while this block is walked)
        const uint32_t block = vend - v0 < 256u ? vend - v0 : 256u;
        auto step = [&](uint32_t s, uint32_t g0) {
            const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp((int)LOCATE_FAR, (int)cur[C - 1], 0x138, 0xF, 0xF, false);   // lane 0: far
            g = (uint32_t)__builtin_amdgcn_update_dpp((int)g0, (int)g, 0x138, 0xF, 0xF, false);
            uint32_t d = diag, u = up;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const uint32_t left = cur[i];
                u = __builtin_amdgcn_msad_u8(g, k[i], min(min(d, u), left));
                d = left;
                cur[i] = u;
            }
            diag = up;
            uint32_t x = cur[0];
#pragma unroll
            for (int i = 1; i < C; ++i) x = track == (uint32_t)i ? cur[i] : x;
            last = x == cost ? v0 + s : last;
        };
        auto single = [&](uint32_t s) {
            const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)lv, (int)(s >> 2));
            step(s, (x >> (8u * (s & 3u))) & 0xFFu);
        };
        auto front = [&]() {
            uint32_t m = cur[0];
#pragma unroll
            for (int i = 1; i < C; ++i) m = min(m, cur[i]);
            return m;
        };
        uint32_t s = v0 == 0 ? skip : 0u;
        for (; (s & 3u) != 0 && s < block; ++s) single(s);
        const uint32_t turns = block < 252u ? block : 252u;   // (a whole block leaves its last four steps to the loop that looks at the fronts)
        for (; s + 4u <= turns; s += 4u) {
            const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)lv, (int)(s >> 2));
            step(s, x & 0xFFu);
            step(s + 1u, (x >> 8) & 0xFFu);
            step(s + 2u, (x >> 16) & 0xFFu);
            step(s + 3u, x >> 24);
        }
        uint32_t m0 = 0, m1 = 0;   // the least cell of the lane behind the block's last two steps
        for (; s < block; ++s) {
            single(s);
            m0 = m1, m1 = front();
        }
        if (block == 256u && __builtin_amdgcn_ballot_w64(min(m0, m1) <= cost) == 0) break;
#pragma unroll
        for (int i = 0; i < C; ++i) cur[i] = min(cur[i], LOCATE_FAR);
        diag = min(diag, LOCATE_FAR);
    }
    // `last` counts virtual steps: column j' = last - skip - la
    const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)last, (int)la);
    return end - 1u - (t - skip - la);
}

// Both phases of one pair, in one wavefront: phase 2's registers are phase 1's, used again.
template <int C>
__device__ __forceinline__ uint4 locate_span_pair(const float* __restrict__ q, uint32_t n, float quant, const int8_t* __restrict__ row, uint32_t L)
{
    const uint2 hit = locate_pair<C>(q, n, quant, row, L);
    return make_uint4(hit.x, hit.y, locate_back<C>(q, n, quant, row, hit.x, hit.y), 0u);
}

// grid and wavefronts as locate_kernel; out: vbz_gpu_match_span
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void locate_span_kernel(uint32_t n_reads, const float* __restrict__ query, const uint32_t* __restrict__ valid, uint32_t N,
                                                          float quant, const int8_t* __restrict__ target, const uint32_t* __restrict__ target_len,
                                                          uint32_t G, uint32_t target_stride, uint4* __restrict__ out)
{
    const uint32_t read = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t tg = blockIdx.y;
    if (read >= n_reads) return;
    const uint32_t n0 = valid[read], n = __builtin_amdgcn_readfirstlane(n0 < N ? n0 : N);
    const uint32_t L = __builtin_amdgcn_readfirstlane(target_len[tg]);
    uint4 hit = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
    if (n != 0 && L != 0 && L <= target_stride) {   // (as locate_kernel)
        const float* const q = query + (size_t)read * N;
        const int8_t* const row = target + (size_t)tg * target_stride;
        if (n <= 64u) hit = locate_span_pair<1>(q, n, quant, row, L);
        else if (n <= 128u) hit = locate_span_pair<2>(q, n, quant, row, L);
        else if (n <= 256u) hit = locate_span_pair<4>(q, n, quant, row, L);
        else if (n <= 512u) hit = locate_span_pair<8>(q, n, quant, row, L);
        else if (n <= 1024u) hit = locate_span_pair<16>(q, n, quant, row, L);
        else hit = locate_span_pair<32>(q, n, quant, row, L);
    }
    if ((threadIdx.x & 63u) == 0) out[(size_t)read * G + tg] = hit;   // (one 16-byte vector store)
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

hipError_t launch_locate_span(uint32_t n_reads, const float* query, const uint32_t* valid, uint32_t N, float quant, const int8_t* target,
                              const uint32_t* target_len, uint32_t G, uint32_t target_stride, void* out, hipStream_t s)
{
    if (n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(locate_span_kernel, dim3((n_reads + 3u) / 4u, G), dim3(256), 0, s, n_reads, query, valid, N, quant, target, target_len, G,
                       target_stride, reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

}  // namespace vbzhip
