// xxh64.h -- XXH64 with seed 0, the content checksum of a zstd frame (RFC 8878 3.1.1: the low 32 bits, little-endian, behind the
// last block when the frame header descriptor has Content_Checksum_flag).
//
// The serial statement of the hash, written from the public XXH64 specification, compiled for gfx950 and under g++ (the CPU test:
// tests/test_xxh64_host.py).  The batched kernel (xxh64.hip) splits the same steps over the four lanes of a quad -- one accumulator
// each -- and must give the same 64 bits.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VBZ_XXH_HD __host__ __device__ __forceinline__
#else
#define VBZ_XXH_HD inline
#endif

namespace vbzhip {

constexpr uint64_t XXH_P1 = 0x9E3779B185EBCA87ull;
constexpr uint64_t XXH_P2 = 0xC2B2AE3D27D4EB4Full;
constexpr uint64_t XXH_P3 = 0x165667B19E3779F9ull;
constexpr uint64_t XXH_P4 = 0x85EBCA77C2B2AE63ull;
constexpr uint64_t XXH_P5 = 0x27D4EB2F165667C5ull;

VBZ_XXH_HD uint64_t xxh_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

VBZ_XXH_HD uint64_t xxh_read64(const uint8_t* p)  // little-endian, any alignment
{
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

VBZ_XXH_HD uint32_t xxh_read32(const uint8_t* p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// one 8-byte lane of a 32-byte stripe into accumulator acc
VBZ_XXH_HD uint64_t xxh64_round(uint64_t acc, uint64_t input)
{
    acc += input * XXH_P2;
    acc = xxh_rotl(acc, 31);
    return acc * XXH_P1;
}

// accumulator k (0..3) before the first stripe
VBZ_XXH_HD uint64_t xxh64_init(int k)
{
    return k == 0 ? XXH_P1 + XXH_P2 : (k == 1 ? XXH_P2 : (k == 2 ? 0ull : 0ull - XXH_P1));
}

VBZ_XXH_HD uint64_t xxh64_merge(uint64_t h, uint64_t v)
{
    h ^= xxh64_round(0, v);
    return h * XXH_P1 + XXH_P4;
}

// the four accumulators after the last whole stripe -> the running hash (inputs of 32 bytes and more)
VBZ_XXH_HD uint64_t xxh64_converge(uint64_t v1, uint64_t v2, uint64_t v3, uint64_t v4)
{
    uint64_t h = xxh_rotl(v1, 1) + xxh_rotl(v2, 7) + xxh_rotl(v3, 12) + xxh_rotl(v4, 18);
    h = xxh64_merge(h, v1);
    h = xxh64_merge(h, v2);
    h = xxh64_merge(h, v3);
    return xxh64_merge(h, v4);
}

// h: the converged accumulators (or P5 for an input shorter than 32 bytes); p, rest: the bytes behind the last whole stripe (< 32);
// total: the input's length
VBZ_XXH_HD uint64_t xxh64_finish(uint64_t h, const uint8_t* p, uint32_t rest, uint64_t total)
{
    h += total;
    while (rest >= 8) {
        h ^= xxh64_round(0, xxh_read64(p));
        h = xxh_rotl(h, 27) * XXH_P1 + XXH_P4;
        p += 8;
        rest -= 8;
    }
    if (rest >= 4) {
        h ^= (uint64_t)xxh_read32(p) * XXH_P1;
        h = xxh_rotl(h, 23) * XXH_P2 + XXH_P3;
        p += 4;
        rest -= 4;
    }
    while (rest > 0) {
        h ^= (uint64_t)*p * XXH_P5;
        h = xxh_rotl(h, 11) * XXH_P1;
        ++p;
        --rest;
    }
    h ^= h >> 33;
    h *= XXH_P2;
    h ^= h >> 29;
    h *= XXH_P3;
    return h ^ (h >> 32);
}

// XXH64(p[0..len), seed 0)
VBZ_XXH_HD uint64_t xxh64(const uint8_t* p, uint64_t len)
{
    uint64_t h = XXH_P5;
    const uint64_t stripes = len / 32;
    if (stripes) {
        uint64_t v1 = xxh64_init(0), v2 = xxh64_init(1), v3 = xxh64_init(2), v4 = xxh64_init(3);
        for (uint64_t s = 0; s < stripes; ++s, p += 32) {
            v1 = xxh64_round(v1, xxh_read64(p));
            v2 = xxh64_round(v2, xxh_read64(p + 8));
            v3 = xxh64_round(v3, xxh_read64(p + 16));
            v4 = xxh64_round(v4, xxh_read64(p + 24));
        }
        h = xxh64_converge(v1, v2, v3, v4);
    }
    return xxh64_finish(h, p, (uint32_t)(len & 31), len);
}

}  // namespace vbzhip
