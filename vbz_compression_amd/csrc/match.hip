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
#include "match_select.h"
#include "vbz_kernels.h"

namespace vbzhip {
namespace {

constexpr uint32_t MATCH_FAR = 1u << 30;   // D[.][-1]

// The cell's cost is one v_msad_u8: the sum over the four bytes of |a - b|, skipping the bytes where the REFERENCE operand is 0, plus
// an accumulator.  Query level k (-127 ... 127) is the word {k + 128, 1, 0, 0}; reference level r >= -127 is {r + 128, 0, 0, 0}, so its
// byte 0 is 1 ... 255 and counts, byte 1 does not; r = -128 is {1, 2, 0, 0}: |k + 127| + 1.  A row behind the reference's end is the word 0:
// every cell of it costs nothing, so it holds the running minimum of the row above it -- the last row of lane la is then the running
// minimum of D[M - 1][.] whatever M is, and the answer is tracked on a fixed register.
__device__ __forceinline__ uint32_t match_ref_word(int r) { return r == -128 ? 0x0201u : (uint32_t)(r + 128); }

// the rule's quantisation of one converted sample, as the cell's query word
__device__ __forceinline__ uint32_t match_level(float z, float quant)
{
    const float v = z * quant;
    const float r = fminf(fmaxf(rintf(v), -127.0f), 127.0f);   // (NaN: fmaxf gives -127; taken out below)
    return (v != v ? 128u : (uint32_t)((int)r + 128)) | 0x100u;
}

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
