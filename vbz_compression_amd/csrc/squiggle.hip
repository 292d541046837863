// squiggle.hip -- the two ends of the event-space chain (the rules: include/vbz_gpu.h; in numpy: tests/squiggle_ref.py).
//   vbz_gpu_squiggle_batch:   bases and a k-mer table -> the int8 target arena the locate calls take (and the float32 levels behind it), both
//                             strands, 5'->3' or 3'->5': a rolling k-mer index, one gather a level, the query's own quantiser.
//   vbz_gpu_levels_fit_batch: a vbz_gpu_level arena and the target levels of each pair's stretch -> least-squares {offset, scale} per pair,
//                             from five exact integer sums and a float64 formula with no fused operation.
// No LDS, no barrier, no atomics, no private scratch: lanes talk through shuffles alone (the squiggle's wavefronts leave one word each in a
// buffer of the context for the second launch).
#include "match_path.h"
#include "squiggle_bases.h"

#pragma clang fp contract(off)

namespace vbzhip {
namespace {

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (uint32_t o = 32u; o != 0u; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- vbz_gpu_squiggle_batch -------------------------------------------------------------------------------------------------------------
// The cut.  A lane makes SQ_LANE = 16 consecutive output positions: one 16-byte store of int8 and four of float32.  A wavefront's tile is
// 1 024 positions, a workgroup's 4 096; blockIdx.y is the output row.  Every lane of the grid in front of target_stride stores, so a row is
// written whole; lanes at and behind L store zeros and load nothing.
// The bases.  Output position j holds the k-mer at p = j, or L - 1 - j with REVERSED, of the row's strand; a lane's 16 k-mers are
// p = lo ... lo + 15 in STRAND order (lo = j0, or L - 16 - j0: the lane turns them round before it stores), and they need the
// 16 + k - 1 <= 24 strand bases lo ... lo + 14 + k.  On the strand as given those are the bytes seq[lo ...]; on the reverse complement strand base i is the complement
// of seq[n - 1 - i], so they are the 24 bytes that END at n - 1 - lo, read the other way round.  Either way a lane loads the seven aligned
// dwords that cover its 24 bytes -- each only when it lies inside the row's seq_stride bytes, 0 otherwise -- and v_alignbyte_b32 shifts
// them into place; the reverse strand then swaps the bytes and the dwords and complements the codes.  lo may be negative (the last lane of a
// reversed row) and bytes at and behind n are the caller's junk: both reach only k-mers outside [0, L), which are never gathered or stored.
// Byte 0 of the 24 is strand base lo - (9 - k), so that byte i >= 8 closes k-mer lo + i - 8 whatever k is: the roll (squiggle_bases.h, shared with pile.hip) is unrolled over
// constants, and the 9 - k bases in front of the first k-mer have left both windows when it closes.
// The roll.  index = (index << 2 | code) & (4^k - 1); bad = (bad << 1 | invalid) & (2^k - 1): after k bases both describe exactly the
// last k, whatever came before.  A k-mer inside [0, L) with bad == 0 gathers model[index] (index < 4^k by the mask); with bad != 0 it
// is counted, and holds int8 0 and float +0.
// The count.  A wavefront adds its lanes' counts by shuffles and stores ONE word, part[row][wavefront]: every word of part is stored by
// every call, so nothing is zeroed in front and no atomic is needed; squiggle_masked_kernel, one wavefront a row, adds them up.
struct SquiggleArgs
{
    uint32_t k, rows, seq_stride, target_stride, flags, waves_per_row;
    float quant;
    const uint8_t* seq;
    const uint32_t* seq_len;
    const uint32_t* model;   // the 32 bits of each float
    uint4* target;           // [rows, target_stride / 16]
    uint32_t* target_len;
    uint4* level;            // [rows, target_stride / 4] or nullptr
    uint32_t* part;          // [rows, waves_per_row]
};

__global__ __launch_bounds__(256) void squiggle_kernel(SquiggleArgs a)
{
    const uint32_t row = blockIdx.y, wave = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t j0 = wave * SQ_WAVE + lane * SQ_LANE;
    const bool both = (a.flags & 1u) != 0, reversed = (a.flags & 2u) != 0;
    const uint32_t s = both ? row >> 1 : row;
    const bool rc = both && (row & 1u) != 0;
    uint32_t n = 0;
    const uint32_t L = squiggle_len(a.seq_len, a.seq_stride, a.k, a.target_stride, s, n);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.target_len[row] = L;

    uint32_t q[4] = { 0u, 0u, 0u, 0u }, m[SQ_LANE];
#pragma unroll
    for (uint32_t e = 0; e < SQ_LANE; ++e) m[e] = 0u;
    uint32_t masked = 0;
    if (j0 < L) {
        uint32_t v[6];
        const int32_t lo = squiggle_bases(a.seq, a.seq_stride, s, n, a.k, L, j0, rc, reversed, v);
        const uint32_t index_mask = (1u << (2u * a.k)) - 1u, bad_mask = (1u << a.k) - 1u;
        uint32_t index = 0, bad = 0;
#pragma unroll
        for (uint32_t i = 0; i < 24u; ++i) {
            if (!squiggle_roll_step(v, i, rc, index_mask, bad_mask, lo, L, index, bad)) continue;
            const uint32_t e = i - (SQ_KMAX - 1u);   // byte i closes the k-mer at p = lo + e, inside [0, L)
            if (bad != 0) ++masked;
            else {
                m[e] = a.model[index];
                const float val = __uint_as_float(m[e]) * a.quant;
                const float r = fminf(fmaxf(rintf(val), -127.0f), 127.0f);
                q[e / 4u] |= (val != val ? 0u : (uint32_t)(int)r & 0xFFu) << (8u * (e % 4u));
            }
        }
        if (reversed) {   // strand order -> output order
#pragma unroll
            for (uint32_t e = 0; e < SQ_LANE / 2u; ++e) {
                const uint32_t x = m[e];
                m[e] = m[SQ_LANE - 1u - e];
                m[SQ_LANE - 1u - e] = x;
            }
            const uint32_t x0 = __builtin_bswap32(q[0]), x1 = __builtin_bswap32(q[1]);
            q[0] = __builtin_bswap32(q[3]), q[1] = __builtin_bswap32(q[2]), q[2] = x1, q[3] = x0;
        }
    }
    masked = wave_sum(masked);
    if (lane == 0) a.part[(size_t)row * a.waves_per_row + wave] = masked;
    if (j0 >= a.target_stride) return;
    a.target[(size_t)row * (a.target_stride / 16u) + j0 / 16u] = make_uint4(q[0], q[1], q[2], q[3]);
    if (a.level) {
        uint4* const lv = a.level + (size_t)row * (a.target_stride / 4u) + j0 / 4u;
#pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) lv[t] = make_uint4(m[4u * t], m[4u * t + 1u], m[4u * t + 2u], m[4u * t + 3u]);
    }
}

__global__ __launch_bounds__(256) void squiggle_masked_kernel(uint32_t rows, uint32_t waves_per_row, const uint32_t* __restrict__ part,
                                                              uint32_t* __restrict__ masked)
{
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (row >= rows) return;
    const uint32_t* const p = part + (size_t)row * waves_per_row;
    uint32_t sum = 0;
    for (uint32_t i = lane; i < waves_per_row; i += 64u) sum += p[i];
    sum = wave_sum(sum);
    if (lane == 0) masked[row] = sum;
}

// ---- vbz_gpu_levels_fit_batch -----------------------------------------------------------------------------------------------------------
// One wavefront a pair, four to a workgroup, 64 levels a turn: a lane loads its 32-byte record by two 16-byte loads and its target level
// from the aligned dword that holds byte start + t -- t < W and start + W == end <= L_g, so that dword lies in front of dword
// (L_g + 3) / 4 of the row -- and keeps the five sums K, Sg, Sgg, Sq, Sgq in registers; they are added across the wavefront once, behind
// the last turn, and lane 0 does the float64 arithmetic and the stores.  Integer sums do not depend on their order.
struct FitArgs
{
    uint32_t n_pairs, n_reads, G, target_stride, max_width, min_samples, max_entries;
    float quant;
    const int8_t* target;
    const uint32_t* target_len;
    const uint4* pairs;        // {read, ref, begin, end}
    const uint4* hit;          // {cost, end, start, n}
    const uint32_t* n_levels;
    const uint4* levels;       // [n_pairs, max_width] of two 16-byte halves
    const float2* prior;       // [n_reads] {shift, scale} or nullptr
    uint4* out;                // {offset, scale, used, ok}
    float* offset;
    float* scale;
    int64_t* sums;             // [n_pairs, 4] or nullptr
};

__global__ __launch_bounds__(256) void levels_fit_kernel(FitArgs a)
{
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (p >= a.n_pairs) return;
    const uint4 pr = a.pairs[p], h = a.hit[p];
    const uint32_t read = pr.x, ref = pr.y, start = h.z, W = a.n_levels[p];
    const bool valid = levels_pair_valid(pr, h, W, a.n_reads, a.G, a.target_stride, a.max_width, a.target_len);
    uint32_t K = 0;
    int64_t Sg = 0, Sgg = 0, Sq = 0, Sgq = 0;
    if (valid) {
        const uint4* const lv = a.levels + 2u * (size_t)p * a.max_width;
        const uint32_t* const words = reinterpret_cast<const uint32_t*>(a.target + (size_t)ref * a.target_stride);
        const uint32_t least = a.min_samples > 1u ? a.min_samples : 1u;
        for (uint32_t base = 0; base < W; base += 64u) {
            const uint32_t t = base + lane;
            if (t >= W) continue;
            const uint4 r0 = lv[2u * (size_t)t], r1 = lv[2u * (size_t)t + 1u];
            const uint32_t at = start + t;
            const int32_t g = (int32_t)(int8_t)(words[at >> 2] >> (8u * (at & 3u)));
            const uint32_t ns = r0.z, ne = r0.w;
            if (ns < least || (a.max_entries != 0u && ne > a.max_entries)) continue;
            const double mean = (double)(int64_t)((uint64_t)r1.y << 32 | r1.x) / (double)ns;
            if (!(fabs(mean) <= 32768.0)) continue;
            const int64_t q = (int64_t)rint(mean * 64.0);   // (a power of two: exact)
            ++K;
            Sg += g;
            Sgg += g * g;
            Sq += q;
            Sgq += g * q;
        }
        K = wave_sum(K);
        Sg = wave_sum(Sg);
        Sgg = wave_sum(Sgg);
        Sq = wave_sum(Sq);
        Sgq = wave_sum(Sgq);
    }
    if (lane != 0) return;
    float offset = 0.0f, scale = 1.0f;   // the prior's constants: what a pair without a good fit keeps
    if (a.prior && read < a.n_reads) {
        const float2 ss = a.prior[read];
        offset = -ss.x;
        scale = (float)(1.0 / (double)ss.y);
    }
    uint32_t ok = 0;
    const int64_t num = (int64_t)K * Sgq - Sg * Sq, den = (int64_t)K * Sgg - Sg * Sg;
    if (valid && K >= 2u && den > 0 && num > 0) {
        const double A = (double)num / (double)den;
        const double B = __dsub_rn((double)Sq, __dmul_rn(A, (double)Sg)) / (double)K;
        const double sa = A / 64.0, sb = B / 64.0;
        const float fs = (float)(1.0 / __dmul_rn(sa, (double)a.quant)), fo = (float)(-sb);
        if (fs > 0.0f && fs <= 3.402823466e+38f && fabsf(fo) <= 3.402823466e+38f) offset = fo, scale = fs, ok = 1u;
    }
    a.out[p] = make_uint4(__float_as_uint(offset), __float_as_uint(scale), K, ok);
    a.offset[p] = offset;
    a.scale[p] = scale;
    if (a.sums) {
        int64_t* const sm = a.sums + 4u * (size_t)p;
        sm[0] = Sg, sm[1] = Sgg, sm[2] = Sq, sm[3] = Sgq;
    }
}

}  // namespace

uint32_t squiggle_part_words(uint32_t rows, uint32_t target_stride) { return rows * (((target_stride + SQ_BLOCK - 1u) / SQ_BLOCK) * 4u); }

hipError_t launch_squiggle(uint32_t k, uint32_t rows, uint32_t seq_stride, uint32_t target_stride, uint32_t flags, float quant, const uint8_t* seq,
                           const uint32_t* seq_len, const float* model, int8_t* target, uint32_t* target_len, uint32_t* masked, float* level, uint32_t* part,
                           hipStream_t s)
{
    SquiggleArgs a;
    const uint32_t blocks = (target_stride + SQ_BLOCK - 1u) / SQ_BLOCK;
    a.k = k, a.rows = rows, a.seq_stride = seq_stride, a.target_stride = target_stride, a.flags = flags, a.waves_per_row = blocks * 4u;
    a.quant = quant;
    a.seq = seq, a.seq_len = seq_len, a.model = reinterpret_cast<const uint32_t*>(model);
    a.target = reinterpret_cast<uint4*>(target), a.target_len = target_len, a.level = reinterpret_cast<uint4*>(level), a.part = part;
    hipLaunchKernelGGL(squiggle_kernel, dim3(blocks, rows), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(squiggle_masked_kernel, dim3((rows + 3u) / 4u), dim3(256), 0, s, rows, a.waves_per_row, part, masked);
    return hipGetLastError();
}

hipError_t launch_levels_fit(uint32_t n_pairs, uint32_t n_reads, uint32_t G, uint32_t target_stride, float quant, const int8_t* target,
                             const uint32_t* target_len, const void* pairs, const void* hit, const uint32_t* n_levels, const void* levels, uint32_t max_width,
                             uint32_t min_samples, uint32_t max_entries, const float* prior, void* out, float* offset, float* scale, int64_t* sums,
                             hipStream_t s)
{
    if (n_pairs == 0) return hipSuccess;
    FitArgs a;
    a.n_pairs = n_pairs, a.n_reads = n_reads, a.G = G, a.target_stride = target_stride, a.max_width = max_width, a.min_samples = min_samples;
    a.max_entries = max_entries, a.quant = quant;
    a.target = target, a.target_len = target_len;
    a.pairs = reinterpret_cast<const uint4*>(pairs), a.hit = reinterpret_cast<const uint4*>(hit), a.n_levels = n_levels;
    a.levels = reinterpret_cast<const uint4*>(levels), a.prior = reinterpret_cast<const float2*>(prior);
    a.out = reinterpret_cast<uint4*>(out), a.offset = offset, a.scale = scale, a.sums = sums;
    hipLaunchKernelGGL(levels_fit_kernel, dim3((n_pairs + 3u) / 4u), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace vbzhip
