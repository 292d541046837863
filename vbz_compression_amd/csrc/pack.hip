// pack.hip -- dense arenas of a batch (include/vbz_gpu.h: vbz_gpu_pack_batch, vbz_gpu_decompressed_size_batch).
//
// Layout: every read gets a byte count (its result, or the raw size its sized header states) or an error code, and a packed offset:
// the exclusive scan of the counts, each rounded up to `align`, error entries taking nothing; off[n] = the total.  The scan is
// reduce-then-scan in three short launches (per 1024-read tile: sum; the tile sums; the tile's own scan), O(n) loads at any n.  The
// tile sums travel in the offset table itself, at off[t * 1024], which only tile t's last launch overwrites.
//
// Gather: one wavefront per unit of 8 KB of the DESTINATION (eight rows of 64 lanes x 16 bytes, every store a whole aligned dwordx4),
// grid-stride over the units.  A wave finds the read that holds its unit's first byte by a 64-ary search in the packed offsets, keeps
// 64 consecutive reads' offsets, sizes and source addresses in LDS, and every lane finds its chunk's read there.  A chunk inside one
// read's bytes is loaded as aligned dwords and shifted with v_alignbit_b32; a chunk inside padding is zeros; a chunk at a read's edge
// (or holding several reads) is put together byte by byte.  Every load lies inside a read's own bytes [src, src + size): no address
// outside a slot the layout launch accepted is formed.
#include "vbz_kernels.h"

namespace vbzhip {

namespace {

constexpr uint32_t TILE = 1024;           // reads per workgroup of the scan launches
constexpr uint32_t ROWS = 8;              // rows of 64 x 16 bytes per gather unit
constexpr uint32_t UNIT = ROWS * 1024;    // destination bytes per unit (one wavefront)
constexpr uint32_t GATHER_WAVES = 4;      // wavefronts per gather workgroup
constexpr uint32_t GATHER_MAX_WGS = 16384;

__device__ __forceinline__ uint64_t round_up(uint32_t v, uint32_t align) { return ((uint64_t)v + align - 1) & ~(uint64_t)(align - 1); }
__device__ __forceinline__ uint32_t bytes_of(uint32_t s) { return s >= E_FIRST ? 0u : s; }   // error entries occupy no bytes

// sum of v over the 1024 threads, in thread 0
__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t* wsum)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if (lane == 0) wsum[w] = v;
    __syncthreads();
    uint64_t t = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < 16; ++k) t += wsum[k];
    return t;
}

// exclusive prefix of v over the 1024 threads; total = the sum
__device__ __forceinline__ uint64_t block_excl_scan_u64(uint64_t v, uint64_t* wsum, uint64_t& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t pre = 0, tot = 0;
    for (int k = 0; k < 16; ++k) {
        const uint64_t s = wsum[k];
        pre += k < w ? s : 0;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return pre + inc - v;
}

// ---- layout, launch 1: per-read byte counts and the tile sums -------------------------------------------------------------------
// pack: the result table is untrusted; a count takes space only when it fits its slot and the slot lies inside [0, dst_bytes).
__global__ __launch_bounds__(1024) void pack_sizes_kernel(uint32_t n, const uint32_t* result, const uint64_t* dst_off, const uint32_t* dst_cap,
                                                          uint64_t dst_bytes, uint32_t align, uint64_t* off, uint32_t* size)
{
    __shared__ uint64_t wsum[16];
    const uint32_t i = blockIdx.x * TILE + threadIdx.x;
    uint64_t take = 0;
    if (i < n) {
        const uint32_t r = result[i];
        uint32_t s = r;
        if (r < E_FIRST) {
            const uint64_t o = dst_off[i];
            const uint32_t cap = dst_cap[i];
            if (r > cap || o > dst_bytes || (uint64_t)cap > dst_bytes - o) s = E_INPUT_SIZE;
            else take = round_up(r, align);
        }
        size[i] = s;
    }
    const uint64_t t = block_sum_u64(take, wsum);
    if (threadIdx.x == 0) off[blockIdx.x * TILE] = t;
}

// sized buffers: raw_size[i] = what vbz_decompressed_size returns (the 4-byte little-endian header; VBZ_INPUT_SIZE_ERROR for a buffer
// shorter than 4 bytes or outside [0, src_bytes))
__global__ __launch_bounds__(1024) void sized_sizes_kernel(uint32_t n, const uint8_t* src, const uint64_t* src_off, const uint32_t* src_size,
                                                           uint64_t src_bytes, uint32_t align, uint64_t* off, uint32_t* size)
{
    __shared__ uint64_t wsum[16];
    const uint32_t i = blockIdx.x * TILE + threadIdx.x;
    uint64_t take = 0;
    if (i < n) {
        const uint64_t o = src_off[i];
        const uint32_t sz = src_size[i];
        uint32_t s = E_INPUT_SIZE;
        if (o <= src_bytes && (uint64_t)sz <= src_bytes - o && sz >= 4) {
            const uint8_t* p = src + o;
            s = p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            take = s >= E_FIRST ? 0 : round_up(s, align);
        }
        size[i] = s;
    }
    const uint64_t t = block_sum_u64(take, wsum);
    if (threadIdx.x == 0) off[blockIdx.x * TILE] = t;
}

// chunk layout (vbz_gpu_chunk_layout_batch): the counts are the reads' chunk counts (align 1 in the launches behind)
__global__ __launch_bounds__(1024) void chunk_counts_kernel(uint32_t n, const uint32_t* samples, uint32_t L, uint32_t S, uint64_t* off, uint32_t* count)
{
    __shared__ uint64_t wsum[16];
    const uint32_t i = blockIdx.x * TILE + threadIdx.x;
    uint64_t take = 0;
    if (i < n) {
        const uint32_t t = samples[i];
        const uint32_t k = t >= 0x80000000u ? 0u : chunk_count(t, L, S);   // (an error code of the size query: no chunks)
        count[i] = k;
        take = k;
    }
    const uint64_t t = block_sum_u64(take, wsum);
    if (threadIdx.x == 0) off[blockIdx.x * TILE] = t;
}

// ---- launch 2: the exclusive scan of the tile sums (one workgroup); off[n] = the total
__global__ __launch_bounds__(1024) void pack_scan_tiles_kernel(uint32_t n, uint64_t* off)
{
    __shared__ uint64_t wsum[16];
    const uint32_t tiles = (n + TILE - 1) / TILE;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < tiles; base += 1024) {
        const uint32_t t = base + threadIdx.x;
        const uint64_t v = t < tiles ? off[(uint64_t)t * TILE] : 0;
        uint64_t sum;
        const uint64_t pre = block_excl_scan_u64(v, wsum, sum);
        if (t < tiles) off[(uint64_t)t * TILE] = carry + pre;
        carry += sum;
    }
    if (threadIdx.x == 0) off[n] = carry;
}

// ---- launch 3: every tile's own scan from its prefix
__global__ __launch_bounds__(1024) void pack_scan_reads_kernel(uint32_t n, uint32_t align, const uint32_t* size, uint64_t* off)
{
    __shared__ uint64_t wsum[16];
    __shared__ uint64_t prefix;
    const uint32_t i = blockIdx.x * TILE + threadIdx.x;
    if (threadIdx.x == 0) prefix = off[blockIdx.x * TILE];
    const uint64_t take = i < n ? round_up(bytes_of(size[i]), align) : 0;
    __syncthreads();
    uint64_t sum;
    const uint64_t pre = block_excl_scan_u64(take, wsum, sum);
    if (i < n) off[i] = prefix + pre;
}

// ---- gather -------------------------------------------------------------------------------------------------------------------
struct WaveCache  // 64 consecutive reads j .. j+63 of the layout (reads at or beyond n: offset = the total, no bytes)
{
    uint64_t lo[65];   // packed offsets of reads j .. j+64
    uint64_t src[64];  // dst_off of each read (its bytes' source)
    uint32_t sz[64];   // bytes of each read
};

// largest k in [0, n) with off[k] <= x (off[0] = 0 <= x): a 64-ary search by the whole wave
__device__ uint32_t wave_find(const uint64_t* off, uint32_t n, uint64_t x)
{
    const uint32_t lane = threadIdx.x & 63;
    uint32_t lo = 0, len = n;
    while (len > 1) {
        const uint32_t step = (len + 63) / 64;
        const uint64_t idx = (uint64_t)lo + (uint64_t)lane * step;
        const bool ok = idx < (uint64_t)lo + len && off[idx] <= x;
        const uint64_t m = __ballot(ok);
        const uint32_t l = 63 - __builtin_clzll(m);
        const uint32_t nlo = lo + l * step;
        len = min(step, lo + len - nlo);
        lo = nlo;
    }
    return lo;
}

// lane-local binary search: largest k in [lo, n) with off[k] <= x, given off[lo] <= x
__device__ uint32_t lane_find(const uint64_t* off, uint32_t lo, uint32_t n, uint64_t x)
{
    uint32_t hi = n;   // off[hi] > x or hi == n
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void wave_fill(WaveCache& c, uint32_t j, uint32_t n, const uint64_t* off, const uint32_t* size, const uint8_t* dst,
                                          const uint64_t* dst_off, uint64_t& my_lo)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t k = (uint64_t)j + lane;
    wave_lds_sync();   // (the lanes' last reads of the previous cache come first)
    my_lo = off[k < n ? k : n];
    c.lo[lane] = my_lo;
    c.sz[lane] = k < n ? bytes_of(size[k]) : 0u;
    c.src[lane] = k < n ? dst_off[k] : 0ull;
    if (lane == 63) c.lo[64] = off[k + 1 < n ? k + 1 : n];
    wave_lds_sync();
}

template <typename T>
__device__ __forceinline__ T table_load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__global__ __launch_bounds__(256) void pack_gather_kernel(uint32_t n, const uint8_t* __restrict__ dst, const uint64_t* __restrict__ dst_off,
                                                          const uint64_t* __restrict__ off, const uint32_t* __restrict__ size,
                                                          uint8_t* __restrict__ packed, uint64_t packed_cap, uint64_t units)
{
    __shared__ WaveCache caches[GATHER_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    WaveCache& c = caches[w];
    const uint64_t total = off[n];
    if (total > packed_cap) return;   // the whole arena or nothing
    // chunk boundaries are 16-byte aligned ADDRESSES: position p of the arena is packed + p, units start at -a0
    const int64_t a0 = (int64_t)((uintptr_t)packed & 15);
    const uint64_t stride = (uint64_t)gridDim.x * GATHER_WAVES;
    for (uint64_t g = (uint64_t)blockIdx.x * GATHER_WAVES + w; g < units; g += stride) {
        const int64_t P = (int64_t)(g * UNIT) - a0;
        if (P >= (int64_t)total) break;
        uint32_t j = wave_find(off, n, (uint64_t)(P > 0 ? P : 0));
        uint64_t my_lo;
        wave_fill(c, j, n, off, size, dst, dst_off, my_lo);

        uint32_t v[ROWS][5];
        uint32_t mode[ROWS];   // 0: nothing to store, 1: shifted copy, 2: ready in v[r][0..3]
        uint32_t shift[ROWS];
#pragma unroll
        for (uint32_t r = 0; r < ROWS; ++r) {
            mode[r] = 0;
            shift[r] = 0;
            const int64_t rs = P + (int64_t)r * 1024;
            if (rs >= (int64_t)total) continue;   // (wave-uniform)
            // the row runs past the cached reads: move the cache up to the read that holds the row's first byte
            if ((uint64_t)(rs + 1024) > c.lo[64] && c.lo[64] < total) {
                const uint64_t m = __ballot(my_lo <= (uint64_t)(rs > 0 ? rs : 0));
                const uint32_t l = 63 - __builtin_clzll(m);
                if (l > 0) {
                    j += l;
                    wave_fill(c, j, n, off, size, dst, dst_off, my_lo);
                }
            }
            const int64_t p = rs + (int64_t)lane * 16;
            if (p >= (int64_t)total) continue;
            const uint64_t x0 = p > 0 ? (uint64_t)p : 0;
            // the read that holds the chunk's first byte
            uint32_t k;
            if (x0 < c.lo[64]) {
                uint32_t a = 0;
#pragma unroll
                for (uint32_t s = 32; s > 0; s >>= 1)
                    if (c.lo[a + s] <= x0) a += s;
                k = j + a;
            } else {
                k = lane_find(off, j + 63 < n ? j + 63 : n - 1, n, x0);
            }
            // (reads past the cache come from the tables themselves; a relaxed atomic load there keeps hipcc from merging the two loads
            // into one flat load from a selected address)
            auto lo_of = [&](uint32_t q) -> uint64_t { return q - j <= 64 ? c.lo[q - j] : table_load(off + (q < n ? q : n)); };
            auto sz_of = [&](uint32_t q) -> uint32_t { return q - j < 64 ? c.sz[q - j] : bytes_of(table_load(size + q)); };
            auto src_of = [&](uint32_t q) -> uint64_t { return q - j < 64 ? c.src[q - j] : table_load(dst_off + q); };
            const uint64_t lo = lo_of(k), end = lo + sz_of(k);
            const bool whole = p >= 0 && (uint64_t)p + 16 <= total;
            if (whole && (uint64_t)p >= end && (uint64_t)p + 16 <= lo_of(k + 1)) {   // padding
                mode[r] = 2;
                v[r][0] = v[r][1] = v[r][2] = v[r][3] = 0;
                continue;
            }
            if (whole && (uint64_t)p + 16 <= end) {
                const uint64_t s0 = src_of(k), s = s0 + ((uint64_t)p - lo), sa = s & ~3ull;
                const uint32_t sh = (uint32_t)(s & 3);
                if (sa >= s0 && sa + (sh ? 20 : 16) <= s0 + (end - lo)) {   // aligned dwords inside the read's bytes
                    const u32x4_a4 q = *reinterpret_cast<const u32x4_a4*>(dst + sa);
                    v[r][0] = q.x;
                    v[r][1] = q.y;
                    v[r][2] = q.z;
                    v[r][3] = q.w;
                    v[r][4] = sh ? *reinterpret_cast<const uint32_t*>(dst + sa + 16) : 0u;
                    shift[r] = sh * 8;
                    mode[r] = 1;
                    continue;
                }
            }
            // byte by byte: read edges, several reads in one chunk, the arena's own ends
            uint32_t d[4] = { 0, 0, 0, 0 };
            uint32_t q = k;
            uint64_t qlo = lo, qend = end, qhi = lo_of(k + 1), qsrc = src_of(k);
#pragma unroll
            for (uint32_t b = 0; b < 16; ++b) {
                const int64_t x = p + (int64_t)b;
                if (x < 0 || (uint64_t)x >= total) continue;
                while ((uint64_t)x >= qhi) {
                    ++q;
                    qlo = qhi;
                    qend = qlo + sz_of(q);
                    qhi = lo_of(q + 1);
                    qsrc = src_of(q);
                }
                if ((uint64_t)x < qend) d[b >> 2] |= (uint32_t)dst[qsrc + ((uint64_t)x - qlo)] << (8 * (b & 3));
            }
            v[r][0] = d[0];
            v[r][1] = d[1];
            v[r][2] = d[2];
            v[r][3] = d[3];
            mode[r] = 2;
        }
#pragma unroll
        for (uint32_t r = 0; r < ROWS; ++r) {
            if (!mode[r]) continue;
            const int64_t p = P + (int64_t)r * 1024 + (int64_t)lane * 16;
            uint4 o;
            if (mode[r] == 1) {
                const uint32_t sh = shift[r];
                o.x = __builtin_amdgcn_alignbit(v[r][1], v[r][0], sh);
                o.y = __builtin_amdgcn_alignbit(v[r][2], v[r][1], sh);
                o.z = __builtin_amdgcn_alignbit(v[r][3], v[r][2], sh);
                o.w = __builtin_amdgcn_alignbit(v[r][4], v[r][3], sh);
            } else {
                o = make_uint4(v[r][0], v[r][1], v[r][2], v[r][3]);
            }
            if (p >= 0 && (uint64_t)p + 16 <= total) {
                *reinterpret_cast<uint4*>(packed + p) = o;
            } else {
                const uint32_t ow[4] = { o.x, o.y, o.z, o.w };
#pragma unroll
                for (uint32_t b = 0; b < 16; ++b) {
                    const int64_t x = p + (int64_t)b;
                    if (x >= 0 && (uint64_t)x < total) packed[x] = (uint8_t)(ow[b >> 2] >> (8 * (b & 3)));
                }
            }
        }
    }
}

// ---- signal windows: the window check (vbz_kernels.h launch_window_check) -------------------------------------------------------------
// launch 1: every read's row count -- 0 unless its two entries of wfirst are rows of the arena -- and the tile sums.  Reads of a batch:
// the constants' table too, and a pair that fails closes the read's gate; POD5 reads: the plan has looked at the pairs.
__global__ __launch_bounds__(1024) void window_counts_kernel(ReadBatch b, Pod5Reads pr, const float* offset, const float* scale, uint64_t* off, uint32_t* count)
{
    __shared__ uint64_t wsum[16];
    const bool reads = pr.reads != nullptr;
    const uint32_t n = reads ? pr.n_reads : b.n_reads;
    const uint32_t i = blockIdx.x * TILE + threadIdx.x;
    uint64_t take = 0;
    if (i < n) {
        if (reads) {
            if (!*pr.bad && !(pr.reads[i].flags & POD5_READ_FAIL)) take = b.sig.wfirst[i + 1] - b.sig.wfirst[i];
        } else {
            uint32_t* gate = const_cast<uint32_t*>(b.gate);
            const_cast<float2*>(b.sig.cal)[i] = make_float2(offset ? offset[i] : 0.0f, scale ? scale[i] : 1.0f);
            if (gate[i] < GATE_SKIP) {
                const uint64_t a = b.sig.wfirst[i], z = b.sig.wfirst[i + 1];
                if (a > z || z > b.sig.wrows || z - a > WINDOW_READ_ROWS_MAX) gate[i] = E_DESTINATION_SIZE;
                else take = z - a;
            }
        }
        count[i] = (uint32_t)take;
    }
    const uint64_t t = block_sum_u64(take, wsum);
    if (threadIdx.x == 0) off[blockIdx.x * TILE] = t;
}

// launch 4 (behind the scan): the j-th counted row -> its read (scan_find) and its row c of the arena; a pair start[c] > start[c + 1]
// inside a read's rows closes the read.  Every start read here belongs to a read whose pair has passed.
__global__ __launch_bounds__(256) void window_sorted_kernel(ReadBatch b, Pod5Reads pr, const uint64_t* scan)
{
    const bool reads = pr.reads != nullptr;
    const uint32_t n = reads ? pr.n_reads : b.n_reads;
    const uint64_t total = scan[n];
    uint32_t* gate = const_cast<uint32_t*>(b.gate);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j + 1 < total; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = scan_find(scan, n, j);
        if (j + 1 >= scan[i + 1]) continue;   // the read's last row
        const uint64_t c = b.sig.wfirst[i] + (j - scan[i]);
        if (b.sig.wstart[c] <= b.sig.wstart[c + 1]) continue;
        if (!reads) {
            gate[i] = E_DESTINATION_SIZE;
            continue;
        }
        // a POD5 read: closed as the plan closes a read that fails its check -- POD5_READ_FAIL, its rows' gates, its statistics finished.
        // The plan also zeroes the read's T and range and its rows' flags; they stay here (the plan has passed them: a window call sets no
        // POD5_ROW_PAD, and every kernel behind this one looks at POD5_READ_FAIL or the rows' gates before it looks at T or the range)
        atomicOr(&pr.reads[i].flags, POD5_READ_FAIL);
        for (uint32_t r = pr.first_row[i]; r < pr.first_row[i + 1]; ++r) gate[r] = E_DESTINATION_SIZE;
        if (b.sig.norm.st) b.sig.norm.st[i].phase = NORM_DONE;
    }
}

// the same pass of an event call (SignalOut::events): an event's start is unsigned (a window's may be negative), nothing else differs --
// a kernel of its own, so that the windows' keeps its code
__global__ __launch_bounds__(256) void event_sorted_kernel(ReadBatch b, Pod5Reads pr, const uint64_t* scan)
{
    const bool reads = pr.reads != nullptr;
    const uint32_t n = reads ? pr.n_reads : b.n_reads;
    const uint64_t total = scan[n];
    const uint32_t* start = reinterpret_cast<const uint32_t*>(b.sig.wstart);
    uint32_t* gate = const_cast<uint32_t*>(b.gate);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j + 1 < total; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = scan_find(scan, n, j);
        if (j + 1 >= scan[i + 1]) continue;   // the read's last row
        const uint64_t c = b.sig.wfirst[i] + (j - scan[i]);
        if (start[c] <= start[c + 1]) continue;
        if (!reads) {
            gate[i] = E_DESTINATION_SIZE;
            continue;
        }
        atomicOr(&pr.reads[i].flags, POD5_READ_FAIL);   // (a POD5 read: closed as window_sorted_kernel closes it)
        for (uint32_t r = pr.first_row[i]; r < pr.first_row[i + 1]; ++r) gate[r] = E_DESTINATION_SIZE;
        if (b.sig.norm.st) b.sig.norm.st[i].phase = NORM_DONE;
    }
}

hipError_t scan_launches(uint32_t n, uint32_t align, const uint32_t* size, uint64_t* off, hipStream_t s)
{
    hipLaunchKernelGGL(pack_scan_tiles_kernel, dim3(1), dim3(1024), 0, s, n, off);
    hipLaunchKernelGGL(pack_scan_reads_kernel, dim3((n + TILE - 1) / TILE), dim3(1024), 0, s, n, align, size, off);
    return hipGetLastError();
}

// ---- signal segmentation: the maps' layout in front of the pass, and count, scan, emit behind it (vbz_kernels.h SegmentOut) ----------
// the map of a read of T samples: one bit a position, whole bytes (the scan rounds them up to 4)
__global__ __launch_bounds__(1024) void segment_sizes_kernel(ReadBatch b, Pod5Reads pr, uint64_t* off, uint32_t* size)
{
    __shared__ uint64_t wsum[16];
    const bool reads = pr.reads != nullptr;
    const uint32_t n = reads ? pr.n_reads : b.n_reads;
    const uint32_t i = blockIdx.x * TILE + threadIdx.x;
    uint64_t take = 0;
    if (i < n) {
        uint32_t T = 0;
        if (reads) T = *pr.bad ? 0u : pr.reads[i].T;
        else if (!(b.gate && b.gate[i] >= GATE_SKIP)) T = b.dst_cap[i] >> 1;
        size[i] = (T + 7u) >> 3;
        take = round_up(size[i], 4);
    }
    const uint64_t t = block_sum_u64(take, wsum);
    if (threadIdx.x == 0) off[blockIdx.x * TILE] = t;
}

// whether read i passed (result[] is read first: a read whose stream failed mid-pass counts 0), and its samples
__device__ __forceinline__ bool segment_passed(const ReadBatch& b, const Pod5Reads& pr, uint32_t i, uint32_t* T)
{
    if (pr.reads) {
        for (uint32_t r = pr.first_row[i]; r < pr.first_row[i + 1]; ++r)
            if (b.result[r] >= E_FIRST) return false;
        *T = pr.reads[i].T;
        return !(pr.reads[i].flags & POD5_READ_FAIL);
    }
    *T = b.result[i] >> 1;
    return b.result[i] < E_FIRST;
}

__global__ __launch_bounds__(1024) void segment_counts_kernel(ReadBatch b, Pod5Reads pr, const uint32_t* rows, uint64_t* off, uint32_t* count)
{
    __shared__ uint64_t wsum[16];
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    const uint32_t i = blockIdx.x * TILE + threadIdx.x;
    uint64_t take = 0;
    if (i < n && !(pr.reads && *pr.bad)) {
        uint32_t T;
        if (segment_passed(b, pr, i, &T) && T != 0) take = rows[i];   // (a read without samples never reached its sink)
        count[i] = (uint32_t)take;
    }
    const uint64_t t = block_sum_u64(take, wsum);
    if (threadIdx.x == 0) off[blockIdx.x * TILE] = t;
}

// one workgroup per read: its entry of event_first and, rank by rank, its starts -- 4 096 bytes of the map a trip, a word a thread
__global__ __launch_bounds__(1024) void segment_emit_kernel(ReadBatch b, Pod5Reads pr, SegmentOut so, const uint32_t* count, const uint64_t* scan,
                                                            uint64_t* event_first, uint32_t* start, uint64_t start_cap)
{
    __shared__ uint64_t wsum[16];
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    if (pr.reads && *pr.bad) return;
    const uint32_t i = blockIdx.x;
    const uint64_t a = scan[i], z = scan[i + 1];
    if (threadIdx.x == 0) {
        event_first[i] = a;
        if (i + 1 == n) event_first[n] = z;
    }
    const uint32_t rows = count[i];
    if (rows == 0 || start == nullptr) return;
    if (z > start_cap) {   // the read does not fit: not one word of start
        if (pr.reads) {
            for (uint32_t r = pr.first_row[i] + threadIdx.x; r < pr.first_row[i + 1]; r += 1024) b.result[r] = E_DESTINATION_SIZE;
            if (threadIdx.x == 0 && pr.read_result) pr.read_result[i] = E_DESTINATION_SIZE;
        } else if (threadIdx.x == 0) {
            b.result[i] = E_DESTINATION_SIZE;
        }
        return;
    }
    if (threadIdx.x == 0) start[a] = 0;
    const uint32_t* map = reinterpret_cast<const uint32_t*>(so.map + so.map_off[i]);
    const uint32_t nbytes = (uint32_t)((so.map_off[i + 1] - so.map_off[i]));   // (rounded up to 4; the bytes behind the map's last hold anything)
    uint32_t T;
    (void)segment_passed(b, pr, i, &T);
    if (!pr.reads) {   // the signal: the read's clamped range
        uint32_t rb, re;
        sample_range(b.sig, i, T, &rb, &re);
        T = re - rb;
    } else if (b.sig.ranged()) {
        T = pr.range[i].y - pr.range[i].x;
    }
    uint64_t rank = a + 1;
    for (uint32_t w0 = 0; w0 < nbytes / 4u; w0 += 1024) {
        const uint32_t w = w0 + threadIdx.x;
        uint32_t bits = w < nbytes / 4u ? map[w] : 0u;
        const uint64_t q0 = 32ull * w;
        if (q0 + 32u > T) bits = q0 >= T ? 0u : bits & (0xFFFFFFFFu >> (32u - (uint32_t)(T - q0)));   // (positions behind the signal: no writer)
        uint64_t tot;
        uint64_t at = rank + block_excl_scan_u64((uint64_t)__popc(bits), wsum, tot);
        while (bits) {
            const uint32_t j = (uint32_t)__ffs((int)bits) - 1u;
            bits &= bits - 1u;
            if (at < z) start[at] = (uint32_t)q0 + j;   // (at < z always: the map's bits are the sink's count)
            ++at;
        }
        rank += tot;
    }
}

// ---- signal spans: count, scan, emit behind the span pass (vbz_kernels.h SpanOut; the rule: include/vbz_gpu.h) ------------------------------
// running maximum of v over the 1024 threads in front of this one (0 in front of thread 0); total = the maximum of all
__device__ __forceinline__ uint32_t block_excl_max_u32(uint32_t v, uint32_t* wmax, uint32_t& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc = inc > t ? inc : t;
    }
    uint32_t ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0;
    if (lane == 63) wmax[w] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
    for (int k = 0; k < 16; ++k) {
        const uint32_t s = wmax[k];
        pre = k < w && s > pre ? s : pre;
        tot = s > tot ? s : tot;
    }
    __syncthreads();
    total = tot;
    return pre > ex ? pre : ex;
}

// The one statement of the walk, by the whole workgroup: the spans of the map's bits at positions [rb, re) of the read -- in-positions at
// most D apart merged, spans shorter than m dropped -- counted (the return, workgroup-uniform) and, EMIT, written as pairs {begin, end}
// in positions of the signal (p - rb) from edge[0] on, in order, `cap` pairs at the most (the count launch's: nothing is written beyond
// them).  A word a thread, 32 768 positions a trip.  Positions travel as p + 1 (0: none).  Two running maxima carry what a thread must
// know of the walk in front of it: the last in-position (whether the thread's first in-position opens a span: more than D positions lie
// between) and the begin of the span that is open there.  A span is complete at its last in-position, which is known where the next
// span opens -- there its length is tested -- or at the walk's end.  A thread loops over the span BEGINS of its word, not over its
// in-positions (a plateau is words of 32 set bits and one begin): the begins are the bits with no set bit in the min(D + 1, 32)
// positions below them inside the word, the word's lowest set bit being judged against the last in-position in front of the word.
template <bool EMIT>
__device__ __forceinline__ uint32_t span_walk(const uint32_t* map, uint32_t rb, uint32_t re, uint32_t D, uint32_t m, uint32_t* wmax, uint64_t* wsum,
                                              uint32_t* edge, uint32_t cap)
{
    uint32_t last_in = 0, open_at = 0;   // (workgroup-uniform, p + 1) behind the trips so far: the last in-position, the open span's begin
    uint64_t rank = 0;                   // complete spans that passed the length test so far
    const uint32_t wend = (re + 31u) >> 5;
    const uint32_t reach = D + 1u < 32u ? D + 1u : 32u;
    for (uint32_t w0 = rb >> 5; w0 < wend && rb < re; w0 += 1024) {
        const uint32_t w = w0 + threadIdx.x, p0 = 32u * w;
        uint32_t bits = w < wend ? map[w] : 0u;
        if (p0 < rb) bits &= 0xFFFFFFFFu << (rb - p0);                                         // (rb - p0 < 32: the walk begins in rb's word)
        if (w < wend && re - p0 < 32u) bits &= 0xFFFFFFFFu >> (32u - (re - p0));                // (positions behind the range: other bits, or no writer)
        uint32_t tot_in, tot_open;
        const uint32_t prev0 = max(last_in, block_excl_max_u32(bits ? p0 + 32u - (uint32_t)__clz((int)bits) : 0u, wmax, tot_in));
        // this thread's span begins: an in-position with no in-position in the D + 1 positions in front of it
        uint32_t near = bits << 1;   // bit j: an in-position lies 1 ... `have` positions below j, inside the word
        for (uint32_t have = 1; have < reach;) {
            const uint32_t step = have < reach - have ? have : reach - have;
            near |= near << step;
            have += step;
        }
        uint32_t opens = bits & ~near;   // (the word's lowest set bit among them)
        if (bits && prev0 != 0 && p0 + (uint32_t)__ffs((int)bits) - 1u - prev0 <= D) opens &= opens - 1u;   // ... which the walk in front of the word may reach
        const uint32_t open0 = max(open_at, block_excl_max_u32(opens ? p0 + 32u - (uint32_t)__clz((int)opens) : 0u, wmax, tot_open));
        // every begin but the read's first completes the span in front of it: [cur - 1, prev), prev behind the last in-position below the
        // begin -- kept when it has m positions
        auto spans_of = [&](auto&& take) {
            uint32_t cur = open0;
            for (uint32_t rest = opens; rest; rest &= rest - 1u) {
                const uint32_t j = (uint32_t)__ffs((int)rest) - 1u, below = bits & ((1u << j) - 1u);
                const uint32_t prev = below ? p0 + 32u - (uint32_t)__clz((int)below) : prev0;
                if (prev != 0 && prev - cur + 1u >= m) take(cur, prev);
                cur = p0 + j + 1u;
            }
        };
        uint32_t cnt = 0;
        spans_of([&](uint32_t, uint32_t) { ++cnt; });
        uint64_t tot;
        uint64_t at = rank + block_excl_scan_u64((uint64_t)cnt, wsum, tot);
        if (EMIT && cnt)
            spans_of([&](uint32_t cur, uint32_t prev) {
                if (at < cap) {
                    edge[2 * at] = cur - 1u - rb;
                    edge[2 * at + 1] = prev - rb;
                }
                ++at;
            });
        rank += tot;
        last_in = max(last_in, tot_in);
        open_at = max(open_at, tot_open);
    }
    if (last_in != 0 && last_in - open_at + 1u >= m) {   // the span that is open at the walk's end
        if (EMIT && threadIdx.x == 0 && rank < cap) {
            edge[2 * rank] = open_at - 1u - rb;
            edge[2 * rank + 1] = last_in - rb;
        }
        ++rank;
    }
    return (uint32_t)rank;
}

// the signal of read i of T samples: its clamped range, in positions of the read (segment_emit_kernel's)
__device__ __forceinline__ void span_range(const ReadBatch& b, const Pod5Reads& pr, uint32_t i, uint32_t T, uint32_t* rb, uint32_t* re)
{
    *rb = 0, *re = T;
    if (!pr.reads) sample_range(b.sig, i, T, rb, re);
    else if (b.sig.ranged()) *rb = pr.range[i].x, *re = pr.range[i].y;
}

// the count launch, one workgroup per read: rows[i] = twice the read's spans -- result[] is read first, and the map of a read that did
// not pass is not looked at (the sink cannot count: spans cross lanes, tiles and segments)
__global__ __launch_bounds__(1024) void span_count_kernel(ReadBatch b, Pod5Reads pr, SpanOut so, uint32_t* rows)
{
    __shared__ uint64_t wsum[16];
    __shared__ uint32_t wmax[16];
    if (pr.reads && *pr.bad) return;
    const uint32_t i = blockIdx.x;
    uint32_t T = 0, spans = 0;
    if (segment_passed(b, pr, i, &T) && T != 0) {
        uint32_t rb, re;
        span_range(b, pr, i, T, &rb, &re);
        spans = span_walk<false>(reinterpret_cast<const uint32_t*>(so.map + so.map_off[i]), rb, re, so.D, so.m, wmax, wsum, nullptr, 0u);
    }
    if (threadIdx.x == 0) rows[i] = 2u * spans;
}

// the emit launch, one workgroup per read: its entry of edge_first and, where its pairs end at or in front of edge_cap, the pairs
__global__ __launch_bounds__(1024) void span_emit_kernel(ReadBatch b, Pod5Reads pr, SpanOut so, const uint32_t* count, const uint64_t* scan,
                                                         uint64_t* edge_first, uint32_t* edge, uint64_t edge_cap)
{
    __shared__ uint64_t wsum[16];
    __shared__ uint32_t wmax[16];
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    if (pr.reads && *pr.bad) return;
    const uint32_t i = blockIdx.x;
    const uint64_t a = scan[i], z = scan[i + 1];
    if (threadIdx.x == 0) {
        edge_first[i] = a;
        if (i + 1 == n) edge_first[n] = z;
    }
    if (count[i] == 0 || edge == nullptr) return;
    if (z > edge_cap) {   // the read does not fit: not one word of edge
        if (pr.reads) {
            for (uint32_t r = pr.first_row[i] + threadIdx.x; r < pr.first_row[i + 1]; r += 1024) b.result[r] = E_DESTINATION_SIZE;
            if (threadIdx.x == 0 && pr.read_result) pr.read_result[i] = E_DESTINATION_SIZE;
        } else if (threadIdx.x == 0) {
            b.result[i] = E_DESTINATION_SIZE;
        }
        return;
    }
    uint32_t T, rb, re;
    (void)segment_passed(b, pr, i, &T);
    span_range(b, pr, i, T, &rb, &re);
    (void)span_walk<true>(reinterpret_cast<const uint32_t*>(so.map + so.map_off[i]), rb, re, so.D, so.m, wmax, wsum, edge + a, count[i] / 2u);   // (count[i] words: the same walk counted them)
}

}  // namespace

hipError_t launch_span_emit(const ReadBatch& b, const Pod5Reads& pr, const SpanOut& so, const SegmentScratch& sc, uint64_t* edge_first, uint32_t* edge,
                            uint64_t edge_cap, hipStream_t s)
{
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    if (n == 0) return hipMemsetAsync(edge_first, 0, 8, s);
    hipLaunchKernelGGL(span_count_kernel, dim3(n), dim3(1024), 0, s, b, pr, so, sc.rows);
    hipLaunchKernelGGL(segment_counts_kernel, dim3((n + TILE - 1) / TILE), dim3(1024), 0, s, b, pr, sc.rows, sc.scan, sc.count);
    const hipError_t e = scan_launches(n, 1, sc.count, sc.scan, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(span_emit_kernel, dim3(n), dim3(1024), 0, s, b, pr, so, sc.count, sc.scan, edge_first, edge, edge_cap);
    return hipGetLastError();
}

hipError_t launch_segment_layout(const ReadBatch& b, const Pod5Reads& pr, const SegmentScratch& sc, hipStream_t s)
{
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    if (n == 0) return hipMemsetAsync(sc.map_off, 0, 8, s);
    hipLaunchKernelGGL(segment_sizes_kernel, dim3((n + TILE - 1) / TILE), dim3(1024), 0, s, b, pr, sc.map_off, sc.size);
    return scan_launches(n, 4, sc.size, sc.map_off, s);
}

hipError_t launch_segment_emit(const ReadBatch& b, const Pod5Reads& pr, const SegmentOut& so, const SegmentScratch& sc, uint64_t* event_first,
                               uint32_t* start, uint64_t start_cap, hipStream_t s)
{
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    if (n == 0) return hipMemsetAsync(event_first, 0, 8, s);
    hipLaunchKernelGGL(segment_counts_kernel, dim3((n + TILE - 1) / TILE), dim3(1024), 0, s, b, pr, sc.rows, sc.scan, sc.count);
    const hipError_t e = scan_launches(n, 1, sc.count, sc.scan, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(segment_emit_kernel, dim3(n), dim3(1024), 0, s, b, pr, so, sc.count, sc.scan, event_first, start, start_cap);
    return hipGetLastError();
}

hipError_t launch_window_check(const ReadBatch& b, const Pod5Reads& pr, const float* offset, const float* scale, const WindowScratch& w, hipStream_t s)
{
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(window_counts_kernel, dim3((n + TILE - 1) / TILE), dim3(1024), 0, s, b, pr, offset, scale, w.scan, w.count);
    const hipError_t e = scan_launches(n, 1, w.count, w.scan, s);
    if (e != hipSuccess || b.sig.wrows < 2) return e;
    const uint64_t wgs = (b.sig.wrows + 255) / 256;
    const dim3 grid((uint32_t)(wgs < 4096u ? wgs : 4096u));
    if (b.sig.events) hipLaunchKernelGGL(event_sorted_kernel, grid, dim3(256), 0, s, b, pr, w.scan);   // (the event check: the starts are unsigned)
    else hipLaunchKernelGGL(window_sorted_kernel, grid, dim3(256), 0, s, b, pr, w.scan);
    return hipGetLastError();
}

hipError_t launch_pack_layout(uint32_t n, const uint32_t* result, const uint64_t* dst_off, const uint32_t* dst_cap, uint64_t dst_bytes, uint32_t align,
                              uint64_t* packed_off, uint32_t* packed_size, hipStream_t s)
{
    if (n == 0) return hipMemsetAsync(packed_off, 0, 8, s);
    hipLaunchKernelGGL(pack_sizes_kernel, dim3((n + TILE - 1) / TILE), dim3(1024), 0, s, n, result, dst_off, dst_cap, dst_bytes, align, packed_off,
                       packed_size);
    return scan_launches(n, align, packed_size, packed_off, s);
}

hipError_t launch_sized_layout(uint32_t n, const uint8_t* src, const uint64_t* src_off, const uint32_t* src_size, uint64_t src_bytes, uint32_t align,
                               uint32_t* raw_size, uint64_t* raw_off, hipStream_t s)
{
    if (n == 0) return hipMemsetAsync(raw_off, 0, 8, s);
    hipLaunchKernelGGL(sized_sizes_kernel, dim3((n + TILE - 1) / TILE), dim3(1024), 0, s, n, src, src_off, src_size, src_bytes, align, raw_off, raw_size);
    return scan_launches(n, align, raw_size, raw_off, s);
}

// row c of the layout -> its read (the last k with chunk_first[k] <= c: reads without chunks share their successor's offset) and start
__global__ __launch_bounds__(256) void chunk_info_kernel(uint32_t n, const uint32_t* samples, uint32_t L, uint32_t S, uint32_t mode, uint32_t end_align,
                                                         const uint64_t* chunk_first, uint32_t* info, uint64_t info_cap)
{
    const uint64_t total = chunk_first[n];
    if (total > info_cap) return;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = lane_find(chunk_first, 0, n, c);
        const uint32_t T = samples[r];
        const uint32_t K = chunk_count(T, L, S), k = (uint32_t)(c - chunk_first[r]);
        info[2 * c] = r;
        info[2 * c + 1] = k + 1 < K ? k * S : chunk_last_start(T, K, L, S, mode, end_align);
    }
}

hipError_t launch_chunk_layout(uint32_t n, const uint32_t* samples, uint32_t L, uint32_t S, uint32_t* count, uint64_t* chunk_first, hipStream_t s)
{
    if (n == 0) return hipMemsetAsync(chunk_first, 0, 8, s);
    hipLaunchKernelGGL(chunk_counts_kernel, dim3((n + TILE - 1) / TILE), dim3(1024), 0, s, n, samples, L, S, chunk_first, count);
    return scan_launches(n, 1, count, chunk_first, s);
}

hipError_t launch_chunk_info(uint32_t n, const uint32_t* samples, uint32_t L, uint32_t S, uint32_t mode, uint32_t end_align, const uint64_t* chunk_first,
                             uint32_t* info, uint64_t info_cap, hipStream_t s)
{
    if (n == 0 || info == nullptr) return hipSuccess;
    hipLaunchKernelGGL(chunk_info_kernel, dim3(2048), dim3(256), 0, s, n, samples, L, S, mode, end_align, chunk_first, info, info_cap);
    return hipGetLastError();
}

hipError_t launch_pack_gather(uint32_t n, const uint8_t* dst, const uint64_t* dst_off, const uint64_t* packed_off, const uint32_t* packed_size,
                              uint8_t* packed, uint64_t packed_cap, hipStream_t s)
{
    if (n == 0 || packed_cap == 0) return hipSuccess;
    const uint64_t units = (packed_cap + 15 + UNIT - 1) / UNIT;   // (+15: the unit in front of an unaligned arena's first line)
    const uint64_t wgs = (units + GATHER_WAVES - 1) / GATHER_WAVES;
    hipLaunchKernelGGL(pack_gather_kernel, dim3((uint32_t)(wgs < GATHER_MAX_WGS ? wgs : GATHER_MAX_WGS)), dim3(64 * GATHER_WAVES), 0, s, n, dst, dst_off,
                       packed_off, packed_size, packed, packed_cap, units);
    return hipGetLastError();
}

}  // namespace vbzhip
