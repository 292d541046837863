// pile.hip -- the pile-up across reads (the rules: include/vbz_gpu_pile.h; in numpy: tests/pile_ref.py).
//   vbz_gpu_levels_pile_batch:    every kept level of every pair added into its target position's cell: a fixed-point value, so integer adds
//                                 that do not depend on their order.
//   vbz_gpu_squiggle_kmers_batch: the k-mer index under every target position, by the squiggle call's own base loading and roll.
//   vbz_gpu_pile_kmers_batch:     the position cells added into the cells of their k-mers; small tables are summed in LDS first.
//   vbz_gpu_model_update_batch:   mean and sd per k-mer from the sums, the prior where there are too few observations.
// A pile is four planes of 64-bit words over cells: plane q of cell c is pile[q * n_cells + c]; 0 the count word n + 2^32 skipped, 1
// n_samples, 2 sum, 3 sumsq.  64 lanes on consecutive cells make one contiguous 512-byte atomic instruction per plane.
#include "squiggle_bases.h"

// Every float64 operation of the rules is rounded and none is fused.  The plain operators of this file say so under this pragma; the
// __dmul_rn / __dsub_rn of the HIP headers are inline operators compiled under the headers' own contraction, and a product feeding a
// difference through them came out as one v_fma_f64 (the k-mer variance, a cancellation, then differed from the rule in float32).
#pragma clang fp contract(off)

namespace vbzhip {
namespace {

__device__ __forceinline__ void pile_add(uint64_t* p, uint64_t v)   // no return, at the memory side, modulo 2^64
{
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the arena's clear --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pile_clear_kernel(uint4* __restrict__ pile, uint64_t n16)
{
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n16; i += step) pile[i] = make_uint4(0u, 0u, 0u, 0u);
}

hipError_t pile_clear(uint64_t* pile, uint64_t n_cells, hipStream_t s)
{
    const uint64_t n16 = n_cells * 2u;   // four planes of 8 bytes a cell
    if (n16 == 0) return hipSuccess;
    const uint64_t blocks = (n16 + 1023u) / 1024u;   // four stores a thread while the grid is below its cap
    hipLaunchKernelGGL(pile_clear_kernel, dim3((uint32_t)(blocks < 65536u ? blocks : 65536u)), dim3(256), 0, s, reinterpret_cast<uint4*>(pile), n16);
    return hipGetLastError();
}

// ---- vbz_gpu_levels_pile_batch ----------------------------------------------------------------------------------------------------------
// levels_fit_kernel's shape: one wavefront a pair, four to a workgroup, 64 levels a turn; a lane loads its 32-byte record by two 16-byte
// loads, does the float64 arithmetic and issues four adds (a skipped level one).  Lanes of a turn hit consecutive cells -- start + t < end
// <= L_g <= target_stride, so cell g * target_stride + start + t lies inside row g of the arena -- and pairs collide with each other at the
// coverage depth.
struct PileArgs
{
    uint32_t n_pairs, n_reads, G, target_stride, max_width, min_samples, max_entries, require_ok;
    double fix;
    const uint32_t* target_len;
    const uint4* pairs;        // {read, ref, begin, end}
    const uint4* hit;          // {cost, end, start, n}
    const uint32_t* n_levels;
    const uint4* levels;       // [n_pairs, max_width] of two 16-byte halves
    const uint4* fit;          // {offset, scale, used, ok} or nullptr
    uint64_t* pile;            // four planes of n_cells words
    uint64_t n_cells;
};

__global__ __launch_bounds__(256) void levels_pile_kernel(PileArgs a)
{
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (p >= a.n_pairs) return;
    const uint4 pr = a.pairs[p], h = a.hit[p];
    const uint32_t W = a.n_levels[p];
    if (!levels_pair_valid(pr, h, W, a.n_reads, a.G, a.target_stride, a.max_width, a.target_len)) return;
    double o = 0.0, s = 1.0;
    if (a.fit) {
        const uint4 f = a.fit[p];
        if (a.require_ok && f.w == 0u) return;
        o = (double)__uint_as_float(f.x), s = (double)__uint_as_float(f.y);
    }
    const uint4* const lv = a.levels + 2u * (size_t)p * a.max_width;
    uint64_t* const cell = a.pile + (size_t)pr.y * a.target_stride + h.z;
    const uint32_t least = a.min_samples > 1u ? a.min_samples : 1u;
    for (uint32_t base = 0; base < W; base += 64u) {
        const uint32_t t = base + lane;
        if (t >= W) continue;
        const uint4 r0 = lv[2u * (size_t)t], r1 = lv[2u * (size_t)t + 1u];
        const uint32_t ns = r0.z, ne = r0.w;
        bool keep = ns >= least && (a.max_entries == 0u || ne <= a.max_entries);
        int64_t u = 0;
        if (keep) {
            const double m = (double)(int64_t)((uint64_t)r1.y << 32 | r1.x) / (double)ns;
            const double w = ((m + o) * s) * a.fix;   // (each rounded, none fused: see the pragma above)
            keep = fabs(w) <= 16777216.0;   // (NaN: left out)
            if (keep) u = (int64_t)rint(w);
        }
        pile_add(cell + t, keep ? 1ull : 1ull << 32);
        if (!keep) continue;
        pile_add(cell + a.n_cells + t, (uint64_t)ns);
        pile_add(cell + 2u * a.n_cells + t, (uint64_t)u);
        pile_add(cell + 3u * a.n_cells + t, (uint64_t)(u * u));
    }
}

// ---- vbz_gpu_squiggle_kmers_batch -------------------------------------------------------------------------------------------------------
// squiggle_kernel's cut, bases and roll (squiggle_bases.h); where that kernel gathers the model this one keeps the index: 16 words a lane,
// four 16-byte stores, the mark for a masked k-mer and at and behind L.  Every lane of the grid in front of target_stride stores.
struct KmersArgs
{
    uint32_t k, rows, seq_stride, target_stride, flags;
    const uint8_t* seq;
    const uint32_t* seq_len;
    uint4* kmer;             // [rows, target_stride / 4]
    uint32_t* target_len;
};

__global__ __launch_bounds__(256) void squiggle_kmers_kernel(KmersArgs a)
{
    const uint32_t row = blockIdx.y, wave = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t j0 = wave * SQ_WAVE + lane * SQ_LANE;
    const bool both = (a.flags & 1u) != 0, reversed = (a.flags & 2u) != 0;
    const uint32_t s = both ? row >> 1 : row;
    const bool rc = both && (row & 1u) != 0;
    uint32_t n = 0;
    const uint32_t L = squiggle_len(a.seq_len, a.seq_stride, a.k, a.target_stride, s, n);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.target_len[row] = L;
    if (j0 >= a.target_stride) return;

    uint32_t m[SQ_LANE];
#pragma unroll
    for (uint32_t e = 0; e < SQ_LANE; ++e) m[e] = 0xFFFFFFFFu;
    if (j0 < L) {
        uint32_t v[6];
        const int32_t lo = squiggle_bases(a.seq, a.seq_stride, s, n, a.k, L, j0, rc, reversed, v);
        const uint32_t index_mask = (1u << (2u * a.k)) - 1u, bad_mask = (1u << a.k) - 1u;
        uint32_t index = 0, bad = 0;
#pragma unroll
        for (uint32_t i = 0; i < 24u; ++i) {
            if (!squiggle_roll_step(v, i, rc, index_mask, bad_mask, lo, L, index, bad)) continue;
            if (bad == 0) m[i - (SQ_KMAX - 1u)] = index;
        }
        if (reversed) {   // strand order -> output order
#pragma unroll
            for (uint32_t e = 0; e < SQ_LANE / 2u; ++e) {
                const uint32_t x = m[e];
                m[e] = m[SQ_LANE - 1u - e];
                m[SQ_LANE - 1u - e] = x;
            }
        }
    }
    uint4* const out = a.kmer + (size_t)row * (a.target_stride / 4u) + j0 / 4u;
#pragma unroll
    for (uint32_t t = 0; t < 4u; ++t) out[t] = make_uint4(m[4u * t], m[4u * t + 1u], m[4u * t + 2u], m[4u * t + 3u]);
}

// ---- vbz_gpu_pile_kmers_batch -----------------------------------------------------------------------------------------------------------
// A workgroup takes PK_TILE consecutive positions of one row (blockIdx.y), a thread PK_TILE / 256 of them, 256 apart: coalesced loads of the
// key and of the four planes.  At k = 1 every position of the call lands on four cells, so with LDS a workgroup keeps a private table of
// 4^k cells, adds into it with LDS 64-bit adds and at its end adds the table's non-zero words into global memory: 4 * 4^k adds at the most
// in place of 4 * PK_TILE.  Without LDS (tables beyond PILE_KMERS_LDS_KMAX) every non-zero cell makes four global adds.
constexpr uint32_t PK_TILE = 4096u;

struct PileKmersArgs
{
    uint32_t k, rows, target_stride;
    const uint32_t* target_len;
    const uint32_t* kmer;      // [rows, target_stride]
    const uint64_t* pile;      // four planes of rows * target_stride words
    uint64_t* kmer_pile;       // four planes of 4^k words
};

template <bool LDS>
__global__ __launch_bounds__(256) void pile_kmers_kernel(PileKmersArgs a)
{
    extern __shared__ uint64_t pk_table[];   // [4][4^k] with LDS
    const uint32_t row = blockIdx.y, cells = 1u << (2u * a.k);
    uint32_t L = a.target_len[row];
    if (L > a.target_stride) L = 0;   // (no address is formed from it)
    const uint32_t j_first = blockIdx.x * PK_TILE;
    if (j_first >= L) return;   // (the whole workgroup: nothing in the table)
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < 4u * cells; i += 256u) pk_table[i] = 0;
        __syncthreads();
    }
    const uint64_t n_cells = (uint64_t)a.rows * a.target_stride;
    const size_t at = (size_t)row * a.target_stride;
    const uint32_t j_end = j_first + PK_TILE < L ? j_first + PK_TILE : L;
    for (uint32_t j = j_first + threadIdx.x; j < j_end; j += 256u) {
        const uint32_t idx = a.kmer[at + j];
        if (idx >= cells) continue;   // (the mark, or a key of another k)
        uint64_t w[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) w[q] = a.pile[q * n_cells + at + j];
        if ((w[0] | w[1] | w[2] | w[3]) == 0) continue;
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            if (LDS) (void)__hip_atomic_fetch_add(&pk_table[q * cells + idx], w[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else pile_add(a.kmer_pile + (size_t)q * cells + idx, w[q]);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 4u * cells; i += 256u) {   // (the table's layout is the arena's)
            const uint64_t w = pk_table[i];
            if (w != 0) pile_add(a.kmer_pile + i, w);
        }
    }
}

// ---- vbz_gpu_model_update_batch ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void model_update_kernel(uint32_t cells, uint32_t min_obs, double fix, const uint64_t* __restrict__ kmer_pile,
                                                           const uint32_t* prior, uint32_t* model, uint32_t* sd)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cells) return;
    const uint32_t n = (uint32_t)kmer_pile[i], least = min_obs > 1u ? min_obs : 1u;
    uint32_t m = prior[i], d = 0u;   // (read before model[i] is written: prior may be model)
    if (n >= least) {
        const double mean = (double)(int64_t)kmer_pile[2u * (size_t)cells + i] / (double)n;
        const double mm = mean * mean;   // (rounded: see the pragma above)
        const double var = (double)kmer_pile[3u * (size_t)cells + i] / (double)n - mm;
        m = __float_as_uint(__double2float_rn(mean / fix));
        d = __float_as_uint(__double2float_rn(__dsqrt_rn(var > 0.0 ? var : 0.0) / fix));
    }
    model[i] = m;
    if (sd) sd[i] = d;
}

}  // namespace

hipError_t launch_levels_pile(uint32_t n_pairs, uint32_t n_reads, uint32_t G, uint32_t target_stride, const uint32_t* target_len, const void* pairs,
                              const void* hit, const uint32_t* n_levels, const void* levels, uint32_t max_width, uint32_t min_samples, uint32_t max_entries,
                              bool require_ok, bool clear, float fix, const void* fit, uint64_t* pile, hipStream_t s)
{
    const uint64_t n_cells = (uint64_t)G * target_stride;
    if (clear) {
        const hipError_t e = pile_clear(pile, n_cells, s);
        if (e != hipSuccess) return e;
    }
    if (n_pairs == 0) return hipSuccess;
    PileArgs a;
    a.n_pairs = n_pairs, a.n_reads = n_reads, a.G = G, a.target_stride = target_stride, a.max_width = max_width, a.min_samples = min_samples;
    a.max_entries = max_entries, a.require_ok = require_ok ? 1u : 0u, a.fix = (double)fix;
    a.target_len = target_len, a.pairs = reinterpret_cast<const uint4*>(pairs), a.hit = reinterpret_cast<const uint4*>(hit), a.n_levels = n_levels;
    a.levels = reinterpret_cast<const uint4*>(levels), a.fit = reinterpret_cast<const uint4*>(fit), a.pile = pile, a.n_cells = n_cells;
    hipLaunchKernelGGL(levels_pile_kernel, dim3((n_pairs + 3u) / 4u), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_squiggle_kmers(uint32_t k, uint32_t rows, uint32_t seq_stride, uint32_t target_stride, uint32_t flags, const uint8_t* seq,
                                 const uint32_t* seq_len, uint32_t* kmer, uint32_t* target_len, hipStream_t s)
{
    KmersArgs a;
    a.k = k, a.rows = rows, a.seq_stride = seq_stride, a.target_stride = target_stride, a.flags = flags;
    a.seq = seq, a.seq_len = seq_len, a.kmer = reinterpret_cast<uint4*>(kmer), a.target_len = target_len;
    hipLaunchKernelGGL(squiggle_kmers_kernel, dim3((target_stride + SQ_BLOCK - 1u) / SQ_BLOCK, rows), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pile_kmers(uint32_t k, uint32_t rows, uint32_t target_stride, bool clear, bool direct, const uint32_t* target_len, const uint32_t* kmer,
                             const uint64_t* pile, uint64_t* kmer_pile, hipStream_t s)
{
    const uint32_t cells = 1u << (2u * k);
    if (clear) {
        const hipError_t e = pile_clear(kmer_pile, cells, s);
        if (e != hipSuccess) return e;
    }
    PileKmersArgs a;
    a.k = k, a.rows = rows, a.target_stride = target_stride, a.target_len = target_len, a.kmer = kmer, a.pile = pile, a.kmer_pile = kmer_pile;
    const dim3 grid((target_stride + PK_TILE - 1u) / PK_TILE, rows);
    if (k <= PILE_KMERS_LDS_KMAX && !direct) {
        if (32u * cells > 65536u) {   // (a table beyond 64 KB of dynamic LDS is asked for by name)
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pile_kmers_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)(32u << (2u * PILE_KMERS_LDS_KMAX)));
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(pile_kmers_kernel<true>, grid, dim3(256), 32u * cells, s, a);
    }
    else hipLaunchKernelGGL(pile_kmers_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_model_update(uint32_t k, uint32_t min_obs, float fix, const uint64_t* kmer_pile, const float* prior, float* model, float* sd, hipStream_t s)
{
    const uint32_t cells = 1u << (2u * k);
    hipLaunchKernelGGL(model_update_kernel, dim3((cells + 255u) / 256u), dim3(256), 0, s, cells, min_obs, (double)fix, kmer_pile,
                       reinterpret_cast<const uint32_t*>(prior), reinterpret_cast<uint32_t*>(model), reinterpret_cast<uint32_t*>(sd));
    return hipGetLastError();
}

}  // namespace vbzhip
