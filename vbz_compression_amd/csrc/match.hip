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
