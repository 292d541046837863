// xxh64.hip -- the zstd content checksum on the device: XXH64 (seed 0) of many buffers at once, the check of the checksums of decoded
// frames, and the checksum writer behind the entropy stage.
//
// XXH64 keeps four accumulators, one per 8-byte lane of a 32-byte stripe; they are independent of each other, and within one the rounds
// are a serial chain (a 64-bit multiply and a rotation: nothing to reassociate).  So a buffer is hashed by a QUAD of lanes, one
// accumulator each, and a wavefront hashes 16 buffers.  Lane k of a quad reads the k-th 8 bytes of every stripe: one load instruction of
// the quad covers 32 contiguous bytes, and XXH_GROUP loads are in flight ahead of the chain (a ring: see quad_xxh64).
// The serial statement of the same steps, which the kernel must agree with, is xxh64.h.
#include "vbz_kernels.h"
#include "xxh64.h"
#include "zstd_frame.h"

namespace vbzhip {

namespace {

constexpr int XXH_GROUP = 16;   // stripes whose loads are in flight ahead of the chain (a ring of 32 VGPRs)

__device__ __forceinline__ uint64_t quad_shfl64(uint64_t v, int src_lane)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src_lane, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src_lane, 64);
    return ((uint64_t)hi << 32) | lo;
}

// XXH64 of p[0..len) on the four lanes of a quad (k = the lane's place in it, all four active); every lane returns the hash
__device__ uint64_t quad_xxh64(const uint8_t* p, uint64_t len, uint32_t k)
{
    const uint64_t stripes = len >> 5;
    uint64_t h = XXH_P5;
    if (stripes) {
        uint64_t v = xxh64_init((int)k);
        const uint8_t* q = p + 8u * k;
        const uint64_t groups = stripes / XXH_GROUP;
        // a ring of XXH_GROUP stripes: the load of stripe s + XXH_GROUP is issued right after round s has used stripe s out of slot
        // s % XXH_GROUP, so XXH_GROUP - 1 loads are in flight while a round waits for the oldest alone (vmcnt(XXH_GROUP - 1)).  The loads beyond the last whole group re-read that group's stripes (in bounds, never used): every
        // trip issues the same loads, which keeps the wait counts exact.  The scheduling barriers keep the compiler from gathering a
        // trip's loads at its top and from rotating the ring through copies at the loop's end (a copy waits for every load in flight).
        if (groups) {
            uint64_t ring[XXH_GROUP];
#pragma unroll
            for (int i = 0; i < XXH_GROUP; ++i) {
                ring[i] = xxh_read64(q + 32 * i);
                __builtin_amdgcn_sched_barrier(0);   // (issued in slot order, as the loop issues them)
            }
            const uint8_t* last = q + (groups - 1) * (32ull * XXH_GROUP);
            for (uint64_t g = 0; g < groups; ++g) {
                const uint8_t* nx = g + 1 < groups ? q + (g + 1) * (32ull * XXH_GROUP) : last;
#pragma unroll
                for (int i = 0; i < XXH_GROUP; ++i) {
                    v = xxh64_round(v, ring[i]);
                    __builtin_amdgcn_sched_barrier(0);   // (the slot's old value is dead before its load: the same register, no copies)
                    ring[i] = xxh_read64(nx + 32 * i);
                }
            }
        }
        for (uint64_t st = groups * XXH_GROUP; st < stripes; ++st) v = xxh64_round(v, xxh_read64(q + 32 * st));
        const int base = (int)(threadIdx.x & ~3u);
        const uint64_t v1 = quad_shfl64(v, base), v2 = quad_shfl64(v, base + 1), v3 = quad_shfl64(v, base + 2), v4 = quad_shfl64(v, base + 3);
        h = xxh64_converge(v1, v2, v3, v4);
    }
    return xxh64_finish(h, p + (stripes << 5), (uint32_t)(len & 31), len);
}

// out[i] = XXH64 of buffer i; len[i] >= E_FIRST (a verdict, not a length), gate[i] >= GATE_SKIP or skip[i] >= E_FIRST: left alone
__global__ __launch_bounds__(256) void xxh64_batch_kernel(const uint8_t* src, const uint64_t* off, const uint32_t* len, const uint32_t* gate,
                                                          const uint32_t* skip, uint32_t n, uint64_t* out)
{
    const uint32_t r = (blockIdx.x * 256u + threadIdx.x) >> 2;   // (the whole quad takes the same branches)
    if (r >= n) return;
    if ((gate && gate[r] >= GATE_SKIP) || (skip && skip[r] >= E_FIRST)) return;
    const uint32_t l = len[r];
    if (l >= E_FIRST) return;
    const uint64_t h = quad_xxh64(src + off[r], l, threadIdx.x & 3u);
    if ((threadIdx.x & 3u) == 0) out[r] = h;
}

// where the checksum of a frame stands: the end of its last block (RFC 8878 3.1.1); 0 when the header or a block header does not fit
// in n bytes.  The frames this is asked about have been decoded or written already: the walk only steps over the blocks.
__device__ uint32_t frame_blocks_end(const uint8_t* f, uint32_t n)
{
    if (n < 6) return 0;
    auto at = [&](uint32_t i) { return (uint32_t)f[i]; };
    ZFrameHeader h;
    zstd_frame_header(at, n, &h);
    for (uint32_t pos = h.len;;) {
        if ((uint64_t)pos + 3 > n) return 0;
        const ZBlockHeader bk = zstd_block_header(at(pos) | (at(pos + 1) << 8) | (at(pos + 2) << 16));
        const uint64_t next = (uint64_t)pos + 3 + bk.src;
        if (next > n) return 0;
        pos = (uint32_t)next;
        if (bk.last) return pos;
    }
}

// decode: a frame that carries Content_Checksum_flag and whose content (b.dst + b.dst_off[r], b.result[r] bytes) does not hash to the
// stored value gets E_ZSTD, as libzstd's checksum_wrong makes the reference's vbz_decompress return VBZ_ZSTD_ERROR (vbz/vbz.cpp:258-266)
__global__ __launch_bounds__(256) void xxh64_verify_kernel(ReadBatch b)
{
    const uint32_t r = (blockIdx.x * 256u + threadIdx.x) >> 2;
    if (r >= b.n_reads) return;
    if (b.gate && b.gate[r] >= GATE_SKIP) return;
    const uint32_t res = b.result[r], n = b.src_size[r];
    if (res >= E_FIRST || n >= E_FIRST || n < 6) return;
    const uint8_t* f = b.src + b.src_off[r];
    if (!(f[4] & 4u)) return;   // (every frame without the flag: one byte looked at)
    const uint32_t end = frame_blocks_end(f, n);
    if (end == 0 || (uint64_t)end + 4 > n) return;   // (the decoder has accepted the frame: cannot happen)
    const uint32_t stored = f[end] | ((uint32_t)f[end + 1] << 8) | ((uint32_t)f[end + 2] << 16) | ((uint32_t)f[end + 3] << 24);
    const uint64_t h = quad_xxh64(b.dst + b.dst_off[r], res, threadIdx.x & 3u);
    if ((threadIdx.x & 3u) == 0 && (uint32_t)h != stored) b.result[r] = E_ZSTD;
}

__device__ __forceinline__ uint64_t zstd_bound64(uint64_t n)   // ZSTD_COMPRESSBOUND
{
    return n + (n >> 8) + (n < (128u << 10) ? (((128u << 10) - n) >> 11) : 0);
}

// encode: one wavefront per read.  The frame at b.dst + b.dst_off[r] + hdr (b.result[r] bytes with the sized header) gets
// Content_Checksum_flag and the low 32 bits of hash[r] behind its last block; the skippable trailers behind it move up by four bytes.
// The result stays within the slot and within vbz_max_compressed_size of the raw read (raw_size, integer_size; raw_size == nullptr:
// the slot alone): a frame that would not fit with its trailers loses the trailers, which are hints only; one that does not fit even
// without them (a slot below the bound) gets E_DESTINATION_SIZE -- the caller asked for checksums, and a frame without one is not returned.
__global__ __launch_bounds__(256) void checksum_insert_kernel(ReadBatch b, const uint64_t* hash, uint32_t hdr, const uint32_t* raw_size,
                                                              uint32_t integer_size)
{
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (r >= b.n_reads) return;
    if (b.gate && b.gate[r] >= GATE_SKIP) return;
    const uint32_t res = b.result[r];
    if (res >= E_FIRST || res < hdr + 6) return;
    uint8_t* f = b.dst + b.dst_off[r] + hdr;
    const uint32_t n = res - hdr;
    if (f[4] & 4u) return;
    const uint32_t end = frame_blocks_end(f, n);
    if (end == 0) return;
    uint64_t limit = b.dst_cap[r];
    if (raw_size) {
        const uint64_t raw = raw_size[r];
        const uint64_t cnt = integer_size ? raw / integer_size : 0;
        const uint64_t svb = integer_size ? (cnt + 3) / 4 + 4 * cnt : raw;
        const uint64_t bound = zstd_bound64(svb) + 4;
        if (bound < limit) limit = bound;
    }
    uint32_t trail = n - end;
    if ((uint64_t)res + 4 > limit) trail = 0;
    if ((uint64_t)hdr + end + 4 + trail > limit) {   // (never within vbz_max_compressed_size; a tight slot of the stage entry point)
        if (lane == 0) b.result[r] = E_DESTINATION_SIZE;
        return;
    }
    // the trailers up by four bytes, from the top down: a chunk's loads have completed before its stores, and the next (lower) chunk
    // writes nothing that a later load reads
    for (uint32_t top = trail; top > 0;) {
        const uint32_t lo = top > 64 ? top - 64 : 0;
        const uint32_t i = lo + lane;
        uint8_t v = 0;
        if (i < top) v = f[end + i];
        __builtin_amdgcn_wave_barrier();
        if (i < top) f[end + 4 + i] = v;
        top = lo;
    }
    if (lane == 0) {
        const uint32_t h = (uint32_t)hash[r];
        f[end] = (uint8_t)h;
        f[end + 1] = (uint8_t)(h >> 8);
        f[end + 2] = (uint8_t)(h >> 16);
        f[end + 3] = (uint8_t)(h >> 24);
        f[4] = (uint8_t)(f[4] | 4u);
        b.result[r] = hdr + end + 4 + trail;
    }
}

}  // namespace

hipError_t launch_xxh64_batch(const uint8_t* src, const uint64_t* off, const uint32_t* len, const uint32_t* gate, const uint32_t* skip, uint32_t n,
                              uint64_t* out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    xxh64_batch_kernel<<<dim3((n + 63) / 64), dim3(256), 0, s>>>(src, off, len, gate, skip, n, out);
    return hipGetLastError();
}

hipError_t launch_xxh64_verify(const ReadBatch& b, hipStream_t s)
{
    if (b.n_reads == 0) return hipSuccess;
    xxh64_verify_kernel<<<dim3((b.n_reads + 63) / 64), dim3(256), 0, s>>>(b);
    return hipGetLastError();
}

hipError_t launch_checksum_insert(const ReadBatch& b, const uint64_t* hash, uint32_t hdr, const uint32_t* raw_size, uint32_t integer_size, hipStream_t s)
{
    if (b.n_reads == 0) return hipSuccess;
    checksum_insert_kernel<<<dim3((b.n_reads + 3) / 4), dim3(256), 0, s>>>(b, hash, hdr, raw_size, integer_size);
    return hipGetLastError();
}

}  // namespace vbzhip
