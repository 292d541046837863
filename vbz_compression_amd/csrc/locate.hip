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
#include "match_path.h"
#include "match_select.h"
#include "vbz_kernels.h"

namespace vbzhip {
namespace {

constexpr uint32_t LOCATE_FAR = 1u << 30;   // D[.][-1]

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
        k[i] = r < n ? align_level(q[r], quant) : 0u;   // (no address behind n)
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
        with_rows(n, [&](auto C) VBZ_LAMBDA_INLINE { hit = locate_pair<decltype(C)::value>(q, n, quant, row, L); });
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
        k[i] = r < n ? align_level(q[n - 1u - r], quant) : 0x100u;   // (no address behind n)
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

// ---- the path (vbz_gpu_locate_path_batch) --------------------------------------------------------------------------------------------------
// The warping path of listed pairs in target coordinates: match.hip's two path launches with the operands exchanged.  A pair names a read,
// a target and a window [a, b) of TARGET levels; the rows of the cost matrix are the query's n levels, in the lanes as in locate_pair (c
// rows a lane by the pair's own n), the columns the window's W = b - a levels, streamed.
// A pair of the untrusted table: the rows of its read, n = min(valid, N), when every condition of the header holds, 0 otherwise -- and
// then no address was formed from the pair beyond valid[read] and target_len[target] of a read and a target inside the call.
__device__ __forceinline__ uint32_t locate_path_open(const AlignPathArgs& p, uint4 pr)
{
    if (pr.x >= p.n_reads || pr.y >= p.n_levels || pr.z >= pr.w) return 0u;
    const uint32_t n0 = p.valid[pr.x], n = n0 < p.N ? n0 : p.N;
    const uint32_t L = p.levels_len[pr.y];
    if (L == 0 || L > p.levels_stride || pr.w > L || pr.w - pr.z > p.max_width) return 0u;
    return n;   // (0: nothing to align)
}

// The forward pass of one pair over its window: match_path_forward's cells, keys, direction bits and bit layout (match.hip; starts
// relative to a, sb = ceil(log2 max_width)) under locate_pair's schedule -- the query quantised once into the lanes, the window streamed
// as int8, a dword a lane per block of 256 steps, one v_readlane per four steps.  W + la steps; the answer is row n - 1 of lane la at the
// last step, read off the lane's rows behind the loop.  Rows behind n are sinks for both keys.
// The byte stream.  The window starts at an arbitrary byte a and ends at an arbitrary byte b of the row.  Only aligned dwords are
// loaded: for the block that starts at step t0 lane l loads dwords a / 4 + t0 / 4 + l and the one behind it, each only when it lies in
// front of dword (b + 3) / 4 <= (L + 3) / 4 of the row (0 otherwise), and v_alignbyte_b32 shifts the pair right by a % 4 bytes: the lane
// then holds levels a + t0 + 4 l ... + 3, step t takes byte t % 4 of "dword" t / 4 as if the window began at a dword, and a word of
// direction bits closes at the same steps as in match_path_forward.  Bytes in front of a are shifted out; bytes at and behind b (the
// rest of the last dword, junk behind L, or zeros) reach lanes at steps >= W + l alone, which have left the window.
// Nothing wraps and far stays far, for rows 0 ... n - 1 (PackedKey, under match_select.h's rule with max_width in N's place and
// query_len in ref_stride's: 255 query_len < 2^(31 - sb), sb <= 16; WideKey's far value at bit 62 is out of every sum's reach).
// (a) A true cell is D[i][j] <= 255 (i + 1) <= 255 query_len however wide the window is -- a path may enter row 0 at column j and leave
// row i along that column alone -- and a start is < W <= 2^sb, so a true key is < (255 query_len + 1) 2^sb <= 2^31: below the far value.
// (b) Lanes ahead of the window (t < l) compute on far values alone -- their rows, their diag and the `up` of a lane in the same state;
// lane 0 never is in it: every value is >= 2^31, a row grows by at most 255 2^sb a step (a cell is at most its `left` plus one cost),
// and the state lasts at most 63 steps: below 2^31 + 63 * 255 * 2^16 < 2^32.  So D[.][a - 1], which is such a row when level a arrives,
// is above every true key, and a minimum of a true key and one of these is the true key.  (c) Lanes behind the window (t >= W + l)
// compute on whatever they are handed -- bytes behind b, lane 0's `up` a step number >= W that may not fit the start field -- and may
// wrap: only lanes in the same state read that (a lane reads the lane below it alone, which left the window a step earlier), and lane
// la never is in it: its last level is the last step.  (d) The sign of a difference is the comparison for the operands of every cell
// the traceback reads -- (i, j) with j > a, whose left, up and (above row 0) diag are true cells, below the far value, half the range.
template <int C, typename Key>
__device__ __forceinline__ uint32_t locate_path_forward(const Key key, const float* __restrict__ q, uint32_t n, float quant, const int8_t* __restrict__ row,
                                                        uint32_t a, uint32_t b, uint32_t* __restrict__ bits)
{
    using T = typename Key::T;
    constexpr int SPD = C <= 16 ? 16 / C : 1;   // steps per word (C = 32: two words a step)
    constexpr int UN = SPD < 4 ? 4 : SPD;       // steps a turn: whole dwords of the stream and whole words of bits
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t la = (n - 1u) / (uint32_t)C;   // the lane that holds row n - 1
    const T far = key.far();
    uint32_t k[C];
    T cur[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const uint32_t r = lane * (uint32_t)C + (uint32_t)i;
        k[i] = r < n ? key.query_word(align_level(q[r], quant)) : 0u;   // (no address behind n)
        cur[i] = far;
    }
    const T far0 = lane == 0 ? far : (T)0;   // lane 0's diag stays far
    T diag = far;
    uint32_t g = 0;   // this lane's level
    uint32_t acc = 0;
    uint32_t* const out = bits + lane;
    const uint32_t W = b - a, steps = W + la;
    const uint32_t* const words = reinterpret_cast<const uint32_t*>(row);
    const uint32_t first = a >> 2, shift = a & 3u, n_words = (b + 3u) >> 2;
    auto load = [&](uint32_t t0) {
        const uint32_t at = first + t0 / 4u + lane;
        const uint32_t lo = at < n_words ? words[at] : 0u;
        const uint32_t hi = at + 1u < n_words ? words[at + 1u] : 0u;
        return __builtin_amdgcn_alignbyte(hi, lo, shift);   // levels a + t0 + 4 lane ... + 3
    };
    uint32_t w = load(0u);
    for (uint32_t t0 = 0; t0 < steps; t0 += 256u) {
        const uint32_t lv = w ^ 0x80808080u;   // four levels + 128
        w = load(t0 + 256u);                   // (in flight while this block is walked)
        const uint32_t block = steps - t0 < 256u ? steps - t0 : 256u;
        auto step = [&](uint32_t s, uint32_t level, bool close) {   // close: the step fills the lane's word (C <= 16)
            const T up = key.prev_lane(cur[C - 1], t0 + s);   // D[l C - 1][j]; lane 0: the key (0, j), j = t0 + s relative to a
            g = (uint32_t)__builtin_amdgcn_update_dpp((int)key.query_word(level), (int)g, 0x138, 0xF, 0xF, false);   // the lane below's level; lane 0: level t
            T d = diag, u = up;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const T left = cur[i];
                const T m = min(min(d, u), left);
                acc = __builtin_amdgcn_alignbit(acc, match_sign_less(m, d), 31);      // acc << 1 | (m < d)
                acc = __builtin_amdgcn_alignbit(acc, match_sign_less(left, u), 31);   // acc << 1 | (left < u)
                u = key.cell(g, k[i], m, m, m);   // (the mask of v_msad_u8 is the lane-resident operand's: the query's)
                d = left;
                cur[i] = u;
                if (C == 32 && i % 16 == 15) out[((t0 + s) * 2u + (uint32_t)(i / 16)) * 64u] = acc;
            }
            diag = up | far0;
            if (C <= 16 && close) out[((t0 + s) / (uint32_t)SPD) * 64u] = acc;
        };
        uint32_t s = 0;   // (t0 is a multiple of 256, 256 and UN of SPD: a word closes at the steps e with (e + 1) % SPD == 0 of a turn)
        for (; s + (uint32_t)UN <= block; s += (uint32_t)UN) {
#pragma unroll
            for (int e = 0; e < UN; e += 4) {
                const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)lv, (int)((s + (uint32_t)e) >> 2));
                step(s + (uint32_t)e, x & 0xFFu, (e + 1) % SPD == 0);
                step(s + (uint32_t)e + 1u, (x >> 8) & 0xFFu, (e + 2) % SPD == 0);
                step(s + (uint32_t)e + 2u, (x >> 16) & 0xFFu, (e + 3) % SPD == 0);
                step(s + (uint32_t)e + 3u, x >> 24, (e + 4) % SPD == 0);
            }
        }
        for (; s < block; ++s) {
            const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)lv, (int)(s >> 2));
            step(s, (x >> (8u * (s & 3u))) & 0xFFu, (s + 1u) % (uint32_t)SPD == 0);
        }
    }
    if (C <= 16 && steps % (uint32_t)SPD != 0)   // the open word: its cells to the top
        out[(steps / (uint32_t)SPD) * 64u] = acc << (32u - 2u * (uint32_t)C * (steps % (uint32_t)SPD));
    // row n - 1 of lane la at its last step, the last step of all
    const uint32_t sel = (n - 1u) % (uint32_t)C;
    T x = cur[0];
#pragma unroll
    for (int i = 1; i < C; ++i) x = sel == (uint32_t)i ? cur[i] : x;
    return key.cost(key.uniform(x, la));
}

// grid ceil(count / 4) workgroups of four wavefronts, a wavefront a pair.  Besides the pass, the wavefront writes what the traceback
// does not: the rows behind n as {0, 0}, and of a pair that fails locate_path_open the empty verdict and every row.
template <typename Key>
__device__ __forceinline__ void locate_path_forward_body(const Key key, const AlignPathArgs& p)
{
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    if (w >= p.count) return;
    const size_t pi = (size_t)p.first + w;
    const uint4 pr = path_pair(p, pi);
    const uint32_t n = __builtin_amdgcn_readfirstlane(locate_path_open(p, pr));
    uint2* const rows = p.rows + pi * p.N;
    for (uint32_t i = n + lane; i < p.N; i += 64u) rows[i] = make_uint2(0u, 0u);
    if (n == 0) {
        if (lane == 0) p.hit[pi] = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
        return;
    }
    const float* const q = p.query + (size_t)pr.x * p.N;
    const int8_t* const row = p.levels + (size_t)pr.y * p.levels_stride;
    uint32_t* const bits = p.bits + (size_t)w * p.pair_words;
    uint32_t cost;
    with_rows(n, [&](auto C) VBZ_LAMBDA_INLINE { cost = locate_path_forward<decltype(C)::value>(key, q, n, p.quant, row, pr.z, pr.w, bits); });
    if (lane == 0) p.cost[w] = cost;
}

__global__ __launch_bounds__(256) void locate_path_forward_kernel(const AlignPathArgs p, uint32_t sb) { locate_path_forward_body(PackedKey{ sb }, p); }
__global__ __launch_bounds__(256) void locate_path_forward_wide_kernel(const AlignPathArgs p) { locate_path_forward_body(WideKey{}, p); }

// The traceback, one wavefront per pair: match_path_walk (match_path.h) over the query's n rows.  It writes rows 0 ... n - 1 and the hit
// (one 16-byte store) of the pairs that pass locate_path_open; the forward launch wrote the rest.
__global__ __launch_bounds__(256) void locate_path_trace_kernel(const AlignPathArgs p)
{
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    if (w >= p.count) return;
    const size_t pi = (size_t)p.first + w;
    const uint4 pr = path_pair(p, pi);
    const uint32_t n = __builtin_amdgcn_readfirstlane(locate_path_open(p, pr));
    if (n == 0) return;
    const uint32_t start = match_path_walk(n, pr.z, pr.w - pr.z, p.bits + (size_t)w * p.pair_words, p.rows + pi * p.N);
    if (lane == 0) p.hit[pi] = make_uint4(p.cost[w], pr.w, start, n);
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

hipError_t launch_locate_path_forward(const AlignPathArgs& a, hipStream_t s)
{
    if (a.count == 0) return hipSuccess;
    const dim3 grid((a.count + 3u) / 4u);
    if (match_span_packed(a.max_width, a.N))
        hipLaunchKernelGGL(locate_path_forward_kernel, grid, dim3(256), 0, s, a, match_span_start_bits(a.max_width));
    else
        hipLaunchKernelGGL(locate_path_forward_wide_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_locate_path_trace(const AlignPathArgs& a, hipStream_t s)
{
    if (a.count == 0) return hipSuccess;
    hipLaunchKernelGGL(locate_path_trace_kernel, dim3((a.count + 3u) / 4u), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace vbzhip
