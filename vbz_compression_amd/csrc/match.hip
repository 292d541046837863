// match.hip -- signal match (vbz_gpu_*_match_batch; the rule: include/vbz_gpu.h): subsequence DTW of every read's quantised prefix against
// every reference row, one wavefront per (read, reference) pair.
//
// Layout.  The lanes of a wavefront are the reference: lane l owns rows l C ... l C + C - 1 of the cost matrix, C the smallest of
// 1, 2, 4, 8, 16, 32 with 64 C >= M (one kernel; a wavefront picks its instantiation by its reference's length, which only the device
// knows).  The four wavefronts of a workgroup take four references of ONE read: the query row is fetched once per workgroup from memory
// and three times from cache.
// Schedule.  Systolic: at step t lane l takes query sample j = t - l.  A step is two wave_shr:1 DPP moves -- the lane below's last row
// for this sample, and the sample itself -- and then C cells down the lane's rows in registers: v_min3_u32 of {diagonal, above, left},
// v_msad_u8 for |r - k| + min (below).  No LDS, no barrier, no atomics.
// Boundaries fall out of the initial values.  Lane 0's incoming pair is the DPP's 0: row 0 is c(0, j), the free start.  Every D[.][-1]
// starts at 2^30.  A lane that has not yet met sample 0 (t < l) computes on these, and its values stay >= 2^30; one that has passed sample
// n - 1 computes on whatever it is handed, and only lanes in the same state ever read that.  True values are < 2^20 and the junk grows by
// at most 255 a step for at most 65 536 + 64 steps: nothing wraps, and a minimum of a true value and junk is the true value.
// The answer.  Row M - 1 lies in lane la; the rows behind it cost nothing and carry its running minimum to the lane's last row, where a
// strict < keeps the first j.
// The query is loaded 64 floats at a time (the next block is requested while this one is walked), quantised on load, and sample t is handed
// to lane 0 by v_readlane under a scalar index.
#include "match_path.h"
#include "match_select.h"
#include "vbz_kernels.h"

namespace vbzhip {
namespace {

constexpr uint32_t MATCH_FAR = 1u << 30;   // D[.][-1]

// The cell's cost is one v_msad_u8 over the words of match_path.h (match_ref_word): a row behind the reference's end is the word 0 and costs
// nothing.

// One pair.  q: the read's query row; n >= 1 its valid samples; ref: the reference row, M >= 1 entries, 64 C >= M.
template <int C>
__device__ __forceinline__ uint2 match_pair(const float* __restrict__ q, uint32_t n, float quant, const int8_t* __restrict__ ref, uint32_t M)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t la = (M - 1u) / (uint32_t)C;   // the lane that holds row M - 1
    uint32_t r[C], cur[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const uint32_t row = lane * (uint32_t)C + (uint32_t)i;
        r[i] = row < M ? match_ref_word(ref[row]) : 0u;   // (no address behind M)
        cur[i] = MATCH_FAR;
    }
    uint32_t diag = lane == 0 ? 0u : MATCH_FAR;   // D[l C - 1][j - 1]: what `up` was a step ago
    uint32_t k = 0x180u;                          // this lane's sample
    // Lane la's last row, step by step: junk >= 2^30 while t < la, then the running minimum of D[M - 1][0 ... t - la]; its last sample
    // is the last step.  A strict < therefore keeps the first step that attains the minimum, and no step needs a mask.
    uint32_t best = 0xFFFFFFFFu, best_t = 0;
    const uint32_t steps = n + la;   // the last sample reaches lane la at step n - 1 + la
    float z = lane < n ? q[lane] : 0.0f;
    for (uint32_t t0 = 0; t0 < steps; t0 += 64u) {
        const uint32_t kq = match_level(z, quant);
        const uint32_t next = t0 + 64u + lane;
        z = next < n ? q[next] : 0.0f;   // (in flight while this block is walked)
        const uint32_t block = steps - t0 < 64u ? steps - t0 : 64u;
        // (two steps a turn: a row's new value cannot take the register of its old one, which the row below still reads, so one step
        // leaves every row in another register; the second brings them back and the loop carries no copies)
        auto step = [&](uint32_t s) {
            const uint32_t up = wave_prev_lane_u32(cur[C - 1]);   // D[l C - 1][j]; lane 0: 0
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)kq, (int)s);
            k = (uint32_t)__builtin_amdgcn_update_dpp((int)k0, (int)k, 0x138, 0xF, 0xF, false);   // the lane below's sample; lane 0: sample t
            uint32_t d = diag, u = up;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const uint32_t left = cur[i];
                u = __builtin_amdgcn_msad_u8(k, r[i], min(min(d, u), left));
                d = left;
                cur[i] = u;
            }
            diag = up;
            const bool less = u < best;
            best = less ? u : best;
            best_t = less ? t0 + s : best_t;
        };
        uint32_t s = 0;
        for (; s + 2u <= block; s += 2u) {
            step(s);
            step(s + 1u);
        }
        if (s < block) step(s);
    }
    // lane la holds the answer: every lane gets it
    const uint32_t cost = (uint32_t)__builtin_amdgcn_readlane((int)best, (int)la);
    const uint32_t end = (uint32_t)__builtin_amdgcn_readlane((int)best_t, (int)la) - la + 1u;
    return make_uint2(cost, end);
}

// grid (n_reads, ceil(R / 4)); wavefront w of a workgroup: reference 4 blockIdx.y + w of read blockIdx.x
__global__ __launch_bounds__(256) void match_kernel(const float* __restrict__ query, const uint32_t* __restrict__ valid, uint32_t N, float quant,
                                                    const int8_t* __restrict__ ref, const uint32_t* __restrict__ ref_len, uint32_t R, uint32_t ref_stride,
                                                    uint2* __restrict__ out)
{
    const uint32_t read = blockIdx.x;
    const uint32_t rf = __builtin_amdgcn_readfirstlane(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (rf >= R) return;
    const uint32_t n0 = valid[read], n = __builtin_amdgcn_readfirstlane(n0 < N ? n0 : N);
    const uint32_t M = __builtin_amdgcn_readfirstlane(ref_len[rf]);
    uint2 hit = make_uint2(0xFFFFFFFFu, 0u);
    if (n != 0 && M != 0 && M <= ref_stride) {   // (ref_stride <= 2048: no address from a length that fails here)
        const float* const q = query + (size_t)read * N;
        const int8_t* const row = ref + (size_t)rf * ref_stride;
        if (M <= 64u) hit = match_pair<1>(q, n, quant, row, M);
        else if (M <= 128u) hit = match_pair<2>(q, n, quant, row, M);
        else if (M <= 256u) hit = match_pair<4>(q, n, quant, row, M);
        else if (M <= 512u) hit = match_pair<8>(q, n, quant, row, M);
        else if (M <= 1024u) hit = match_pair<16>(q, n, quant, row, M);
        else hit = match_pair<32>(q, n, quant, row, M);
    }
    if ((threadIdx.x & 63u) == 0) out[(size_t)read * R + rf] = hit;   // (one 8-byte vector store)
}

// ---- the span calls (vbz_gpu_*_match_span_batch): the same DP over pairs (cost, start), ordered by cost first and then by start -----------
// A cell is a KEY whose unsigned order is that order, so the minimum of three keys is the lexicographic minimum, and adding the cell's
// cost to the key's cost field keeps the order of the three candidates: schedule, lanes and registers are match_pair's.
// Row 0.  Lane 0's incoming `up` at the step of sample j is the key (0, j) -- the DPP move's `old` operand, which lane 0 keeps -- and its
// `diag` is the far value for ever: (0, j - 1) would beat (0, j) there and claim a sample the path does not contain.  Row 0's own `left`
// is the path that sat on row 0: it wins against (0, j) exactly when its cost is 0, and then its start is the smaller one.
// The answer.  The first column that attains the minimum cost also holds the smallest start of all columns that attain it
// (include/vbz_gpu.h), so a strict < on the keys of row M - 1, step by step, stops where match_pair's does.  The same holds for the running
// LEXICOGRAPHIC minimum of that row, which is what rows that cost nothing hold behind the reference's end (WideKey).
//
// The keys.  PackedKey (cost << sb | start in one word, the far value at bit 31, v_min3_u32 and v_sad_u32 a cell; rows behind the reference's
// end are sinks) and WideKey (two registers, far at bit 62, free rows): match_path.h, with the rule and the proof that nothing wraps.

// One pair, as match_pair: {cost, end, start, 0}.  SEL: the lane's row that is tracked -- row (M - 1) mod C of lane la
template <int C, int SEL, typename Key>
__device__ __forceinline__ uint4 match_span_pair(const Key key, const float* __restrict__ q, uint32_t n, float quant, const int8_t* __restrict__ ref, uint32_t M)
{
    using T = typename Key::T;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t la = (M - 1u) / (uint32_t)C;   // the lane that holds row M - 1
    const T far = key.far();
    uint32_t r[C];
    T cur[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const uint32_t row = lane * (uint32_t)C + (uint32_t)i;
        r[i] = row < M ? key.ref_word(ref[row]) : 0u;   // (no address behind M)
        cur[i] = far;
    }
    const T far0 = lane == 0 ? far : (T)0;   // lane 0's diag stays far
    T diag = far;                             // D[l C - 1][j - 1]: what `up` was a step ago
    uint32_t k = key.query_word(0x180u);      // this lane's sample
    T best = ~(T)0;                           // lane la's last row, tracked as in match_pair
    uint32_t best_t = 0;
    const uint32_t steps = n + la;
    float z = lane < n ? q[lane] : 0.0f;
    for (uint32_t t0 = 0; t0 < steps; t0 += 64u) {
        const uint32_t kq = key.query_word(match_level(z, quant));
        const uint32_t next = t0 + 64u + lane;
        z = next < n ? q[next] : 0.0f;   // (in flight while this block is walked)
        const uint32_t block = steps - t0 < 64u ? steps - t0 : 64u;
        auto step = [&](uint32_t s) {
            const T up = key.prev_lane(cur[C - 1], t0 + s);   // D[l C - 1][j]; lane 0: the key (0, j), j = t0 + s
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)kq, (int)s);
            k = (uint32_t)__builtin_amdgcn_update_dpp((int)k0, (int)k, 0x138, 0xF, 0xF, false);   // the lane below's sample; lane 0: sample t
            T d = diag, u = up;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const T left = cur[i];
                u = key.cell(k, r[i], d, u, left);
                d = left;
                cur[i] = u;
            }
            diag = up | far0;
            const T a = cur[SEL];
            const bool less = a < best;
            best = less ? a : best;
            best_t = less ? t0 + s : best_t;
        };
        uint32_t s = 0;
        for (; s + 2u <= block; s += 2u) {   // (two steps a turn, as in match_pair)
            step(s);
            step(s + 1u);
        }
        if (s < block) step(s);
    }
    const T hit = key.uniform(best, la);
    const uint32_t end = (uint32_t)__builtin_amdgcn_readlane((int)best_t, (int)la) - la + 1u;
    return make_uint4(key.cost(hit), end, key.start(hit), 0u);
}

// The tracked row.  WideKey's rows behind the reference's end cost nothing, so the lane's last row is tracked whatever M is.  PackedKey's
// cost something (v_sad_u32 has no mask): they are sinks that nothing reads, and the tracked row is row (M - 1) mod C itself -- chosen by a
// scalar switch over C instantiations of the loop, not by C - 1 selects a step.
template <int C, int SEL, typename Key>
__device__ __forceinline__ uint4 match_span_rows(const Key key, const float* __restrict__ q, uint32_t n, float quant, const int8_t* __restrict__ ref, uint32_t M)
{
    if constexpr (Key::FREE_ROWS) return match_span_pair<C, C - 1>(key, q, n, quant, ref, M);
    else if constexpr (SEL == C - 1) return match_span_pair<C, SEL>(key, q, n, quant, ref, M);
    else return (M - 1u) % (uint32_t)C == (uint32_t)SEL ? match_span_pair<C, SEL>(key, q, n, quant, ref, M) : match_span_rows<C, SEL + 1>(key, q, n, quant, ref, M);
}

// grid and wavefronts as match_kernel; the scalar switch over the rows per lane
template <typename Key>
__device__ __forceinline__ void match_span_body(const Key key, const float* __restrict__ query, const uint32_t* __restrict__ valid, uint32_t N, float quant,
                                                const int8_t* __restrict__ ref, const uint32_t* __restrict__ ref_len, uint32_t R, uint32_t ref_stride,
                                                uint4* __restrict__ out)
{
    const uint32_t read = blockIdx.x;
    const uint32_t rf = __builtin_amdgcn_readfirstlane(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (rf >= R) return;
    const uint32_t n0 = valid[read], n = __builtin_amdgcn_readfirstlane(n0 < N ? n0 : N);
    const uint32_t M = __builtin_amdgcn_readfirstlane(ref_len[rf]);
    uint4 hit = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
    if (n != 0 && M != 0 && M <= ref_stride) {   // (ref_stride <= 2048: no address from a length that fails here)
        const float* const q = query + (size_t)read * N;
        const int8_t* const row = ref + (size_t)rf * ref_stride;
        if (M <= 64u) hit = match_span_rows<1, 0>(key, q, n, quant, row, M);
        else if (M <= 128u) hit = match_span_rows<2, 0>(key, q, n, quant, row, M);
        else if (M <= 256u) hit = match_span_rows<4, 0>(key, q, n, quant, row, M);
        else if (M <= 512u) hit = match_span_rows<8, 0>(key, q, n, quant, row, M);
        else if (M <= 1024u) hit = match_span_rows<16, 0>(key, q, n, quant, row, M);
        else hit = match_span_rows<32, 0>(key, q, n, quant, row, M);
    }
    if ((threadIdx.x & 63u) == 0) out[(size_t)read * R + rf] = hit;   // (one 16-byte vector store)
}

__global__ __launch_bounds__(256) void match_span_kernel(const float* __restrict__ query, const uint32_t* __restrict__ valid, uint32_t N, float quant,
                                                         const int8_t* __restrict__ ref, const uint32_t* __restrict__ ref_len, uint32_t R,
                                                         uint32_t ref_stride, uint32_t sb, uint4* __restrict__ out)
{
    match_span_body(PackedKey{ sb }, query, valid, N, quant, ref, ref_len, R, ref_stride, out);
}

__global__ __launch_bounds__(256) void match_span_wide_kernel(const float* __restrict__ query, const uint32_t* __restrict__ valid, uint32_t N, float quant,
                                                              const int8_t* __restrict__ ref, const uint32_t* __restrict__ ref_len, uint32_t R,
                                                              uint32_t ref_stride, uint4* __restrict__ out)
{
    match_span_body(WideKey{}, query, valid, N, quant, ref, ref_len, R, ref_stride, out);
}

// ---- the path calls (vbz_gpu_match_best_batch, vbz_gpu_match_path_batch) -------------------------------------------------------------------
// The winners' table.  One wavefront per read, whatever R is: the lanes stride over the read's row of the span arena (16-byte loads, a
// row of R = 24 is one load a lane), keep the least cost << 32 | ref each, and five xor-shuffles leave the wavefront's least in every lane
// -- least cost first, then the smallest reference.  (One lane per read would walk R dependent 16-byte loads at a stride of 16 R bytes.)
__global__ __launch_bounds__(256) void match_best_kernel(uint32_t n_reads, const uint4* __restrict__ spans, uint32_t R, uint32_t max_cost,
                                                         uint4* __restrict__ pairs)
{
    const uint32_t read = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (read >= n_reads) return;
    const uint4* const row = spans + (size_t)read * R;
    uint64_t best = ~UINT64_C(0);
    for (uint32_t r = lane; r < R; r += 64u) {
        const uint32_t cost = row[r].x;
        const uint64_t key = (uint64_t)cost << 32 | r;
        if (cost != 0xFFFFFFFFu && cost <= max_cost && key < best) best = key;
    }
    for (int o = 32; o != 0; o >>= 1) {
        const uint64_t other = __shfl_xor(best, o);
        best = other < best ? other : best;
    }
    uint4 out = make_uint4(read, 0xFFFFFFFFu, 0u, 0u);
    if (best != ~UINT64_C(0)) {   // (a cost of 0xFFFFFFFF never became a key)
        const uint4 h = row[(uint32_t)best];
        out = make_uint4(read, (uint32_t)best, h.z, h.y);
    }
    if (lane == 0) pairs[read] = out;   // (one 16-byte vector store)
}

// A pair of the untrusted table: the length of its reference when every condition of the header holds, 0 otherwise -- and then no address
// was formed from the pair beyond valid[read] and ref_len[ref] of a read and a reference inside the call.
__device__ __forceinline__ uint32_t match_path_open(const AlignPathArgs& p, uint4 pr)
{
    if (pr.x >= p.n_reads || pr.y >= p.n_levels || pr.z >= pr.w) return 0u;
    const uint32_t n0 = p.valid ? p.valid[pr.x] : p.N, n = n0 < p.N ? n0 : p.N;
    if (pr.w > n || pr.w - pr.z > p.max_width) return 0u;
    const uint32_t M = p.levels_len[pr.y];
    return M <= p.levels_stride ? M : 0u;
}

// The forward pass of one pair over its window: match_span_pair's schedule over the W columns q[0 ... W), W + la steps, starts relative to
// the window.  The answer is no running minimum: it is row M - 1 at the last step of lane la, read off the lane's rows once, behind the
// loop.  Rows behind the reference's end are sinks for both keys here (WideKey's free rows would hold a running minimum nobody wants).
// Directions.  Behind v_min3_u32, a cell emits two bits: b0 = (min < diag), b1 = (left < up).  b0 == 0 is the diagonal step, the first
// of the three; otherwise the minimum is min(up, left) and up goes first unless left is strictly smaller.  (b1 means nothing when b0 is 0,
// and the traceback does not look at it.)  Row 0: lane 0's diag is far, a diagonal step does not exist and the traceback does not look at
// b0 there; its `up` is the key (0, j), which its left beats exactly when the left's cost is 0 -- b1 there is the sit on row 0, no b1 the
// stop.  A bit is the sign of a difference, and v_alignbit_b32 shifts it into the lane's accumulator: a subtraction and an alignbit a
// bit, 4 VALU instructions a cell more than the span kernel's two (compares and selects -- v_cmp, v_cndmask, v_lshl_or a bit -- were 6
// more: DESIGN.md 4.22 "The path").  The sign is the comparison for operands below half the range, which the keys of every cell the
// traceback reads are: it reads (i, j) with j > 0 alone, where left, up and (above row 0) diag are true cells, below the far value.
// Layout.  A lane's cells, step after step and its C rows down, fill words of 16 cells, the first cell in the top bits: cell (t, i) of
// lane l is cell number t C + i mod C of its stream, word g = number / 16 stands at bits[g * 64 + l].  Every lane closes word g at the same
// step, so a store is one 256-byte line.  Lanes that have not met the window yet, or have left it, and sink rows store junk that the
// traceback never reads: it reads (i, j) at step j + l of lane l <= la alone, and steps 0 ... W - 1 + la are all stored.  No LDS.
template <int C, typename Key>
__device__ __forceinline__ uint32_t match_path_forward(const Key key, const float* __restrict__ q, uint32_t W, float quant, const int8_t* __restrict__ ref,
                                                       uint32_t M, uint32_t* __restrict__ bits)
{
    using T = typename Key::T;
    constexpr int SPD = C <= 16 ? 16 / C : 1;   // steps per word (C = 32: two words a step)
    constexpr int UN = SPD < 2 ? 2 : SPD;       // steps a turn: even, as in match_pair
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t la = (M - 1u) / (uint32_t)C;
    const T far = key.far();
    uint32_t r[C];
    T cur[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const uint32_t row = lane * (uint32_t)C + (uint32_t)i;
        r[i] = row < M ? key.ref_word(ref[row]) : 0u;   // (no address behind M)
        cur[i] = far;
    }
    const T far0 = lane == 0 ? far : (T)0;
    T diag = far;
    uint32_t k = key.query_word(0x180u);
    uint32_t acc = 0;
    uint32_t* const out = bits + lane;
    const uint32_t steps = W + la;
    float z = lane < W ? q[lane] : 0.0f;
    for (uint32_t t0 = 0; t0 < steps; t0 += 64u) {
        const uint32_t kq = key.query_word(match_level(z, quant));
        const uint32_t next = t0 + 64u + lane;
        z = next < W ? q[next] : 0.0f;
        const uint32_t block = steps - t0 < 64u ? steps - t0 : 64u;
        auto step = [&](uint32_t s, bool close) {   // close: the step fills the lane's word (C <= 16)
            const T up = key.prev_lane(cur[C - 1], t0 + s);
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)kq, (int)s);
            k = (uint32_t)__builtin_amdgcn_update_dpp((int)k0, (int)k, 0x138, 0xF, 0xF, false);
            T d = diag, u = up;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const T left = cur[i];
                const T m = min(min(d, u), left);
                acc = __builtin_amdgcn_alignbit(acc, match_sign_less(m, d), 31);      // acc << 1 | (m < d)
                acc = __builtin_amdgcn_alignbit(acc, match_sign_less(left, u), 31);   // acc << 1 | (left < u)
                u = key.cell(k, r[i], m, m, m);
                d = left;
                cur[i] = u;
                if (C == 32 && i % 16 == 15) out[((t0 + s) * 2u + (uint32_t)(i / 16)) * 64u] = acc;
            }
            diag = up | far0;
            if (C <= 16 && close) out[((t0 + s) / (uint32_t)SPD) * 64u] = acc;
        };
        uint32_t s = 0;   // (t0 is a multiple of 64, 64 and UN of SPD: a word closes at the steps e with (e + 1) % SPD == 0 of a turn)
        for (; s + (uint32_t)UN <= block; s += (uint32_t)UN) {
#pragma unroll
            for (int e = 0; e < UN; ++e) step(s + (uint32_t)e, (e + 1) % SPD == 0);
        }
        for (; s < block; ++s) step(s, (s + 1u) % (uint32_t)SPD == 0);
    }
    if (C <= 16 && steps % (uint32_t)SPD != 0)   // the open word: its cells to the top
        out[(steps / (uint32_t)SPD) * 64u] = acc << (32u - 2u * (uint32_t)C * (steps % (uint32_t)SPD));
    // row M - 1 of lane la at its last step, the last step of all
    const uint32_t sel = (M - 1u) % (uint32_t)C;
    T a = cur[0];
#pragma unroll
    for (int i = 1; i < C; ++i) a = sel == (uint32_t)i ? cur[i] : a;
    return key.cost(key.uniform(a, la));
}

// grid ceil(count / 4) workgroups of four wavefronts, a wavefront a pair.  Besides the pass, the wavefront writes what the traceback
// does not: the rows behind the reference's end as {0, 0}, and of a pair that fails match_path_open the empty verdict and every row.
template <typename Key>
__device__ __forceinline__ void match_path_forward_body(const Key key, const AlignPathArgs& p)
{
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    if (w >= p.count) return;
    const size_t pi = (size_t)p.first + w;
    const uint4 pr = path_pair(p, pi);
    const uint32_t M = __builtin_amdgcn_readfirstlane(match_path_open(p, pr));
    uint2* const rows = p.rows + pi * p.levels_stride;
    for (uint32_t i = M + lane; i < p.levels_stride; i += 64u) rows[i] = make_uint2(0u, 0u);
    if (M == 0) {
        if (lane == 0) p.hit[pi] = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
        return;
    }
    const float* const q = p.query + (size_t)pr.x * p.N + pr.z;
    const int8_t* const row = p.levels + (size_t)pr.y * p.levels_stride;
    uint32_t* const bits = p.bits + (size_t)w * p.pair_words;
    const uint32_t W = pr.w - pr.z;
    uint32_t cost;
    with_rows(M, [&](auto C) VBZ_LAMBDA_INLINE { cost = match_path_forward<decltype(C)::value>(key, q, W, p.quant, row, M, bits); });
    if (lane == 0) p.cost[w] = cost;
}

__global__ __launch_bounds__(256) void match_path_forward_kernel(const AlignPathArgs p, uint32_t sb) { match_path_forward_body(PackedKey{ sb }, p); }
__global__ __launch_bounds__(256) void match_path_forward_wide_kernel(const AlignPathArgs p) { match_path_forward_body(WideKey{}, p); }

// The traceback, one wavefront per pair: at most W + M dependent steps (match_path.h: match_path_walk, stated once for this call and for
// the locate path).  It writes rows 0 ... M - 1 and the hit (one 16-byte store) of the pairs that pass match_path_open; the forward launch
// wrote the rest.
__global__ __launch_bounds__(256) void match_path_trace_kernel(const AlignPathArgs p)
{
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    if (w >= p.count) return;
    const size_t pi = (size_t)p.first + w;
    const uint4 pr = path_pair(p, pi);
    const uint32_t M = __builtin_amdgcn_readfirstlane(match_path_open(p, pr));
    if (M == 0) return;
    const uint32_t start = match_path_walk(M, pr.z, pr.w - pr.z, p.bits + (size_t)w * p.pair_words, p.rows + pi * p.levels_stride);
    if (lane == 0) p.hit[pi] = make_uint4(p.cost[w], pr.w, start, M);
}

// valid[i] of the fused calls: min(T', N) from the read's verdict (T x 4 bytes on success) and the range tables; an error: 0
__global__ void match_valid_kernel(uint32_t n, const uint32_t* __restrict__ result, const uint32_t* __restrict__ rbegin, const uint32_t* __restrict__ rend,
                                   uint32_t N, uint32_t* __restrict__ valid)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t res = result[i];
    uint32_t v = 0;
    if (res < E_FIRST) {
        const uint32_t T = res / 4u;
        const uint32_t e0 = rend ? rend[i] : T, e = e0 < T ? e0 : T;
        const uint32_t b0 = rbegin ? rbegin[i] : 0u, b = b0 < e ? b0 : e;
        v = e - b < N ? e - b : N;
    }
    valid[i] = v;
}

// the library's own window tables of the fused calls: read i owns row i, which starts at sample 0
__global__ void match_windows_kernel(uint32_t n, uint64_t* __restrict__ first, int32_t* __restrict__ start)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) first[i] = i;
    if (i < n) start[i] = 0;
}

}  // namespace

hipError_t launch_match(uint32_t n_reads, const float* query, const uint32_t* valid, uint32_t N, float quant, const int8_t* ref, const uint32_t* ref_len,
                        uint32_t R, uint32_t ref_stride, void* out, hipStream_t s)
{
    if (n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(match_kernel, dim3(n_reads, (R + 3u) / 4u), dim3(256), 0, s, query, valid, N, quant, ref, ref_len, R, ref_stride,
                       reinterpret_cast<uint2*>(out));
    return hipGetLastError();
}

hipError_t launch_match_span(uint32_t n_reads, const float* query, const uint32_t* valid, uint32_t N, float quant, const int8_t* ref, const uint32_t* ref_len,
                             uint32_t R, uint32_t ref_stride, void* out, hipStream_t s)
{
    if (n_reads == 0) return hipSuccess;
    const dim3 grid(n_reads, (R + 3u) / 4u);
    if (match_span_packed(N, ref_stride))
        hipLaunchKernelGGL(match_span_kernel, grid, dim3(256), 0, s, query, valid, N, quant, ref, ref_len, R, ref_stride, match_span_start_bits(N),
                           reinterpret_cast<uint4*>(out));
    else
        hipLaunchKernelGGL(match_span_wide_kernel, grid, dim3(256), 0, s, query, valid, N, quant, ref, ref_len, R, ref_stride, reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

hipError_t launch_match_best(uint32_t n_reads, const void* spans, uint32_t R, uint32_t max_cost, void* pairs, hipStream_t s)
{
    if (n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(match_best_kernel, dim3((n_reads + 3u) / 4u), dim3(256), 0, s, n_reads, reinterpret_cast<const uint4*>(spans), R, max_cost,
                       reinterpret_cast<uint4*>(pairs));
    return hipGetLastError();
}

hipError_t launch_match_path_forward(const AlignPathArgs& a, hipStream_t s)
{
    if (a.count == 0) return hipSuccess;
    const dim3 grid((a.count + 3u) / 4u);
    if (match_span_packed(a.max_width, a.levels_stride))
        hipLaunchKernelGGL(match_path_forward_kernel, grid, dim3(256), 0, s, a, match_span_start_bits(a.max_width));
    else
        hipLaunchKernelGGL(match_path_forward_wide_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_match_path_trace(const AlignPathArgs& a, hipStream_t s)
{
    if (a.count == 0) return hipSuccess;
    hipLaunchKernelGGL(match_path_trace_kernel, dim3((a.count + 3u) / 4u), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_match_valid(uint32_t n, const uint32_t* result, const uint32_t* rbegin, const uint32_t* rend, uint32_t N, uint32_t* valid, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(match_valid_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, result, rbegin, rend, N, valid);
    return hipGetLastError();
}

hipError_t launch_match_windows(uint32_t n, uint64_t* first, int32_t* start, hipStream_t s)
{
    hipLaunchKernelGGL(match_windows_kernel, dim3(n / 256 + 1), dim3(256), 0, s, n, first, start);
    return hipGetLastError();
}

}  // namespace vbzhip
