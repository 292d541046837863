// svb_store.h -- the output side of the svb decoder (svb_kernels.hip): the sinks its decode loops store through, and what only they use.
// A sink is what svb_decode_range, I16DecPairs::run and svb16_decode_row (`class Store`) hand their values to:
//   static constexpr uint32_t BYTES   bytes per value in result[]
//   begin_row(s)                      (the sinks that walk a POD5 read's rows in turn) the values handed to put() from here on begin at s of the read
//   aligned()                         whole 16-byte lines may be stored: the tile loop's lanes of VPL values, and I16DecPairs at all
//   put(i0, valid, base, s)           one lane's values i0 ... i0 + valid - 1 of the workgroup's (base + s[k]), every lane at the same point
//   finish()                          once per read, by the whole workgroup (svb_decode_range: the range at the read's start)
//   done()                            once per workgroup, after its values, by the whole workgroup
// (a hook a sink has no use for is an empty body).  A sink keeps its own output's state alone and is built ready to use in one step.  A
// new output is one more sink and one more line of the selection at the end of this file.
#pragma once
#include "vbz_kernels.h"

namespace vbzhip {
namespace {

constexpr int WG = 256;

template <int ELEM>
struct Vpl
{
    static constexpr int value = (ELEM == 4) ? 4 : 8;  // values per lane per tile
};

__device__ __forceinline__ int32_t load_elem(const uint8_t* p, int elem)
{
    if (elem == 1) return (int8_t)p[0];
    if (elem == 2) {
        uint16_t v;
        __builtin_memcpy(&v, p, 2);
        return (int16_t)v;
    }
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return (int32_t)v;
}

__device__ __forceinline__ void store_elem(uint8_t* p, int elem, uint32_t v)
{
    if (elem == 1) p[0] = (uint8_t)v;
    else if (elem == 2) {
        uint16_t t = (uint16_t)v;
        __builtin_memcpy(p, &t, 2);
    } else __builtin_memcpy(p, &v, 4);
}

// ---- typed store (SignalOut): a decoded int16 sample -> ((float)x + offset) * scale, rounded once (RNE) to the output type ----------
// OUT = SIG_* (0: the int16 store itself).  The read's constants are workgroup-uniform (one scalar load per workgroup).
template <int OUT>
struct OutBytes
{
    static constexpr int value = (OUT & 3) == SIG_F32 ? 4 : 2;   // (OUT & SIG_CHUNK: the chunk store of the same type)
};
struct SigK
{
    float o = 0.0f, s = 1.0f;
    uint32_t bias = 0;   // 0: the low 16 bits are an int16; 0x8000: a uint16
};

__device__ __forceinline__ SigK sig_constants(const ReadBatch& b, uint32_t r)
{
    const float2 c = b.sig.cal[r];
    SigK k;
    k.o = c.x;
    k.s = c.y;
    k.bias = b.sig.bias;
    return k;
}

__device__ __forceinline__ float sig_f32(uint32_t v, const SigK& k)
{
#pragma clang fp contract(off)
    // (sign-extend v ^ bias, add the bias back: the int16 or the uint16 value of the low 16 bits; exact in float)
    const int32_t x = ((int32_t)((v ^ k.bias) << 16) >> 16) + (int32_t)k.bias;
    return ((float)x + k.o) * k.s;   // add, then multiply, each rounded (no FMA)
}

template <int OUT>
__device__ __forceinline__ uint32_t sig_pack2(float a, float b)
{
    if (OUT == SIG_F16) {
        // (the float32 values are pinned in registers: hipcc folds a multiply and the conversion behind it into v_fma_mixlo_f16, one
        // rounding straight to float16, whatever the contraction setting -- y must be rounded to float32 first)
        asm("" : "+v"(a), "+v"(b));   // v_cvt_f16_f32: round to nearest even (not v_cvt_pkrtz_f16_f32)
        const _Float16 ha = (_Float16)a, hb = (_Float16)b;
        uint16_t ua, ub;
        __builtin_memcpy(&ua, &ha, 2);
        __builtin_memcpy(&ub, &hb, 2);
        return (uint32_t)ua | ((uint32_t)ub << 16);
    } else {                // v_cvt_pk_bf16_f32: round to nearest even
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        const bf16x2 h = __builtin_convertvector((f32x2){ a, b }, bf16x2);
        uint32_t u;
        __builtin_memcpy(&u, &h, 4);
        return u;
    }
}

// eight consecutive samples base + s[0 .. 7] to p (16-byte aligned): two dwordx4 stores of float32, one of float16 / bfloat16
template <int OUT>
__device__ __forceinline__ void sig_store8(uint8_t* p, uint32_t base, const uint32_t s[8], const SigK& k)
{
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = sig_f32(base + s[j], k);
    if (OUT == SIG_F32) {
        *reinterpret_cast<uint4*>(p) = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
        *reinterpret_cast<uint4*>(p + 16) = make_uint4(__float_as_uint(f[4]), __float_as_uint(f[5]), __float_as_uint(f[6]), __float_as_uint(f[7]));
    } else {
        *reinterpret_cast<uint4*>(p) = make_uint4(sig_pack2<OUT>(f[0], f[1]), sig_pack2<OUT>(f[2], f[3]), sig_pack2<OUT>(f[4], f[5]), sig_pack2<OUT>(f[6], f[7]));
    }
}

template <int OUT>
__device__ __forceinline__ void sig_store1(uint8_t* p, uint32_t v, const SigK& k)
{
    const float f = sig_f32(v, k);
    if (OUT == SIG_F32) {
        __builtin_memcpy(p, &f, 4);
    } else {
        const uint16_t h = (uint16_t)sig_pack2<OUT>(f, f);
        __builtin_memcpy(p, &h, 2);
    }
}

// ---- chunk store (SignalOut::row; OUT = SIG_* | SIG_CHUNK): the typed samples into fixed-length chunks --------------------------------
// Chunk k of the read is row k of the read's rows (ChunkK::base), row-major, L * E bytes (16-byte aligned: L is a multiple of 8).  The
// chunks on the grid k * S start at multiples of 8, so a lane's eight samples i0 ... i0 + 7 (i0 a multiple of 8) lie wholly inside or
// outside each of them and go out as whole 16-byte stores, one per chunk that holds them (at most ceil(L / S) + 1).  The END chunk starts
// at `last`, d = last % 8 samples past a multiple of 8: its 8-sample line starting at sample i0 + d is put together from the lane's
// samples d ... 7 and the next lane's 0 ... d - 1 (one shuffle per dword) and stored whole -- except where the next group belongs to
// another wavefront (lane 63) or to the next row of a POD5 read: there the two lanes store their parts element by element (disjoint
// bytes).  Positions past the read's end take the pad value: in a line that holds samples, the lane storing the line puts it there; the
// lines that hold none are written by chunk_pad.  No two stores of a launch write the same bytes (the argument: DESIGN.md 4.11).
struct ChunkK
{
    uint8_t* base = nullptr;   // the read's first row
    uint64_t row_bytes = 0;    // L * E
    uint32_t T = 0, L = 0, S = 0, K = 0, last = 0;   // samples, chunk length, step, chunks, the last chunk's start
    uint32_t nG = 0;           // chunks on the grid k * S (END with K >= 2: all but the last)
    uint32_t inv = 0;          // floor(2^32 / S): k = floor(i0 / S) by one multiply-high and a correction
    uint32_t padw = 0;         // the pad value's bits in the output type
    bool extra = false;        // END with K >= 2: the last chunk is the pulled-back one at `last`
};

// the chunks of a signal of T samples whose chunk 0 is row first_row of the arena (a read: b.sig.row[r]; a POD5 read: the plan's)
template <int OUT>
__device__ __forceinline__ ChunkK chunk_constants(const ReadBatch& b, uint32_t T, uint64_t first_row)
{
    constexpr uint32_t OB = OutBytes<OUT>::value;
    ChunkK c;
    c.T = T;
    c.L = b.sig.chunk_len;
    c.S = b.sig.step;
    c.K = chunk_count(T, c.L, c.S);
    c.last = chunk_last_start(T, c.K, c.L, c.S, b.sig.mode, b.sig.end_align);
    c.extra = b.sig.mode == CHUNK_END && c.K >= 2;
    c.nG = c.extra ? c.K - 1 : c.K;
    c.row_bytes = (uint64_t)c.L * OB;
    c.base = b.dst + first_row * c.row_bytes;
    c.inv = (uint32_t)(0x100000000ull / c.S);
    if (OB == 4) c.padw = __float_as_uint(b.sig.pad);
    else c.padw = sig_pack2<OUT & 3>(b.sig.pad, b.sig.pad) & 0xFFFFu;
    return c;
}

// e[0 .. 7]: the output type's bits of eight consecutive positions (16-bit types in the low halves) -> p, 16-byte aligned
template <int OUT>
__device__ __forceinline__ void chunk_put8(uint8_t* p, const uint32_t e[8])
{
    if (OutBytes<OUT>::value == 4) {
        *reinterpret_cast<uint4*>(p) = make_uint4(e[0], e[1], e[2], e[3]);
        *reinterpret_cast<uint4*>(p + 16) = make_uint4(e[4], e[5], e[6], e[7]);
    } else {
        *reinterpret_cast<uint4*>(p) = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
    }
}

template <int OUT>
__device__ __forceinline__ void chunk_put1(uint8_t* p, uint32_t e)
{
    if (OutBytes<OUT>::value == 4) {
        __builtin_memcpy(p, &e, 4);
    } else {
        const uint16_t h = (uint16_t)e;
        __builtin_memcpy(p, &h, 2);
    }
}

template <int D>
__device__ __forceinline__ void chunk_shift(const uint32_t a[8], const uint32_t n[8], uint32_t o[8])
{
#pragma unroll
    for (int m = 0; m < 8; ++m) o[m] = m + D < 8 ? a[m + D] : n[m + D - 8];
}

// e[0 .. 7]: the output type's bits of a lane's eight samples base + s[j], the pad value behind the first `valid` of them
template <int OUT>
__device__ __forceinline__ void chunk_elems8(const ChunkK& ck, int valid, uint32_t base, const uint32_t s[8], const SigK& sk, uint32_t e[8])
{
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = sig_f32(base + s[j], sk);
    if (OutBytes<OUT>::value == 4) {
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = __float_as_uint(f[j]);
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const uint32_t w = sig_pack2<OUT & 3>(f[2 * m], f[2 * m + 1]);
            e[2 * m] = w & 0xFFFFu;
            e[2 * m + 1] = w >> 16;
        }
    }
    if (valid < 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j >= valid) e[j] = ck.padw;
    }
}

// the grid chunks that hold position p of the signal: put(q), q the address of position p, in k = floor(p / S) (at most the grid's last)
// and in every chunk before it that still reaches p
template <int OUT, class Put>
__device__ __forceinline__ void chunk_walk(const ChunkK& ck, uint32_t p, Put put)
{
    constexpr uint32_t OB = OutBytes<OUT>::value;
    uint32_t k = __umulhi(p, ck.inv);
    if (p - k * ck.S >= ck.S) ++k;
    if (k > ck.nG - 1u) k = ck.nG - 1u;
    uint32_t off = p - k * ck.S;
    uint8_t* q = ck.base + (uint64_t)k * ck.row_bytes + (size_t)off * OB;
    const int64_t back = (int64_t)ck.S * OB - (int64_t)ck.row_bytes;   // one chunk back: the same sample S positions further on
    while (off < ck.L) {
        put(q);
        if (k == 0) break;
        --k;
        off += ck.S;
        q += back;
    }
}

// the sample at position p of the signal (its bits e in the output type) into every chunk that holds it
template <int OUT>
__device__ __forceinline__ void chunk_put_sample(const ChunkK& ck, uint32_t p, uint32_t e)
{
    chunk_walk<OUT>(ck, p, [&](uint8_t* q) { chunk_put1<OUT>(q, e); });
    if (ck.extra && p >= ck.last && p - ck.last < ck.L)
        chunk_put1<OUT>(ck.base + (uint64_t)(ck.K - 1u) * ck.row_bytes + (size_t)(p - ck.last) * OutBytes<OUT>::value, e);
}

// one lane's eight consecutive samples i0 ... i0 + 7 of the signal (i0 a multiple of 8), the first `valid` of them decoded (base + s[j]),
// into every chunk that holds them.  Every lane of the workgroup calls it at the same point (the END chunk's lines take a cross-lane
// shuffle).  ROWS: the workgroup's samples may end at re in front of the signal's end, the next workgroup (a POD5 read's next row) going on
// from there.  A lane then stores whole lines only where all eight positions are this workgroup's samples or lie behind the signal's end;
// its last group, when the next row goes on in the same line, and the END chunk's lines that reach into the next row are stored element by
// element, each workgroup its own samples.  Without ROWS (a read, or a segment of one: segments end at multiples of 8 * 64) re is not
// looked at.
template <int OUT, bool ROWS>
__device__ __forceinline__ void chunk_store8(const ChunkK& ck, uint32_t i0, int valid, uint32_t re, uint32_t base, const uint32_t s[8], const SigK& sk)
{
    constexpr uint32_t OB = OutBytes<OUT>::value;
    uint32_t e[8];
    chunk_elems8<OUT>(ck, valid, base, s, sk, e);
    const bool tail = ROWS && re < ck.T;                   // samples of later rows follow
    const bool partial = tail && valid > 0 && valid < 8;   // ... in this lane's line
    if (partial) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < valid) chunk_put_sample<OUT>(ck, i0 + (uint32_t)j, e[j]);
    } else if (valid > 0) {
        chunk_walk<OUT>(ck, i0, [&](uint8_t* q) { chunk_put8<OUT>(q, e); });
    }
    if (!ck.extra) return;
    // the END chunk (a partial lane has stored its samples there already)
    const uint32_t sl = ck.last, d = sl & 7u, g0 = sl - d;
    uint8_t* row = ck.base + (uint64_t)(ck.K - 1u) * ck.row_bytes;
    if (d == 0) {
        if (!partial && valid > 0 && i0 >= sl && i0 - sl < ck.L) chunk_put8<OUT>(row + (size_t)(i0 - sl) * OB, e);
        return;
    }
    const int lane = threadIdx.x & 63;
    // the line that starts at sample i0 + d (behind the signal's end it holds no sample: chunk_pad's)
    const bool in = !partial && valid > 0 && i0 >= g0 && i0 - g0 < ck.L && i0 + d < ck.T;
    const bool in0 = !partial && lane == 0 && valid > 0 && i0 >= g0 + 8u && i0 - 8u - g0 < ck.L;   // lane 0: the line that starts in the group before
    if (!__any(in || in0)) return;
    uint32_t n[8];
    if (OB == 4) {
#pragma unroll
        for (int j = 0; j < 8; ++j) n[j] = (uint32_t)__shfl_down((int)e[j], 1, 64);
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const uint32_t w = (uint32_t)__shfl_down((int)(e[2 * m] | (e[2 * m + 1] << 16)), 1, 64);
            n[2 * m] = w & 0xFFFFu;
            n[2 * m + 1] = w >> 16;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (i0 + 8u + (uint32_t)j >= ck.T) n[j] = ck.padw;
    if (in) {
        // whole: the next group is behind the signal's end, or the next lane's and all of it this workgroup's
        if (i0 + 8u >= ck.T || (lane != 63 && !(tail && i0 + 16u > re))) {
            uint32_t o[8];
            switch (d) {
            case 1: chunk_shift<1>(e, n, o); break;
            case 2: chunk_shift<2>(e, n, o); break;
            case 3: chunk_shift<3>(e, n, o); break;
            case 4: chunk_shift<4>(e, n, o); break;
            case 5: chunk_shift<5>(e, n, o); break;
            case 6: chunk_shift<6>(e, n, o); break;
            default: chunk_shift<7>(e, n, o); break;
            }
            chunk_put8<OUT>(row + (size_t)(i0 - g0) * OB, o);
        } else {   // (the rest of the line is stored by whoever holds the next group: lane 0 below, a partial lane, the next row)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((uint32_t)j >= d) chunk_put1<OUT>(row + (size_t)(i0 - g0 + (uint32_t)j - d) * OB, e[j]);
        }
    }
    if (in0) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if ((uint32_t)j < d) chunk_put1<OUT>(row + (size_t)(i0 + (uint32_t)j - sl) * OB, e[j]);
    }
}

// the pad behind the signal's last sample, by the whole workgroup: the last chunk's lines that hold no sample and, with `elems` (the line
// of the last sample was stored sample by sample), the positions between that sample and the first such line
template <int OUT>
__device__ __forceinline__ void chunk_pad(const ChunkK& ck, bool elems)
{
    if (ck.K == 0) return;
    constexpr uint32_t OB = OutBytes<OUT>::value;
    uint8_t* row = ck.base + (uint64_t)(ck.K - 1u) * ck.row_bytes;
    const uint32_t p0 = ck.T - ck.last, l0 = (p0 + 7u) >> 3;   // the first pad position, the first line of nothing else
    if (elems && p0 + threadIdx.x < l0 * 8u) chunk_put1<OUT>(row + (size_t)(p0 + threadIdx.x) * OB, ck.padw);
    uint32_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = ck.padw;
    for (uint32_t j = l0 + threadIdx.x; j < (ck.L >> 3); j += WG) chunk_put8<OUT>(row + (size_t)j * 8u * OB, e);
}

// The chunk sink of one workgroup (the contract: this file's head): its values are the samples s0 ... re - 1 of a read whose samples [rb, rend) are the signal that is
// chunked (ck is that signal's; OUT & SIG_RANGE, else the whole read).  A whole read on one workgroup is s0 = 0, rb = 0, rend = re = T; a
// segment of the large-read path the same (put() gets positions in the read); a row of a POD5 read (ROWS) lies at s0.
template <int OUT, bool ROWS>
struct ChunkStore
{
    static constexpr bool RANGED = (OUT & SIG_RANGE) != 0;
    static constexpr uint32_t BYTES = OutBytes<OUT>::value;
    ChunkK ck;
    SigK sk;
    const uint8_t* arena = nullptr;   // aligned(): the chunk arena (ROWS: not looked at)
    uint32_t s0 = 0, re = 0;      // ROWS (else 0 and not looked at)
    uint32_t rb = 0, rend = 0;    // RANGED
    bool pad_elems = false;       // finish(): the line of the signal's last sample is stored sample by sample (ROWS: by whichever row holds it)

    // one lane's values i0 ... i0 + valid - 1 of the workgroup's (base + s[k]), every lane of the workgroup at the same point.  A lane that
    // starts at a multiple of 8 of the signal stores lines (`valid` cut at the range's ends; a lane outside still takes part in the END
    // chunk's shuffle), any other every sample on its own
    __device__ __forceinline__ void put(uint32_t i0, int valid, uint32_t base, const uint32_t s[8]) const
    {
        const uint32_t first = ROWS ? s0 : 0u, b0 = RANGED ? rb : 0u;
        const uint32_t p = first + i0;   // the lane's first sample in the read
        if (((first - b0) & 7u) == 0) {
            int v = valid;
            uint32_t end = re;   // where the workgroup's samples end in the signal
            if constexpr (RANGED) {
                v = (p < rb || p >= rend) ? 0 : (rend - p < (uint32_t)valid ? (int)(rend - p) : valid);
                const uint32_t rowend = re < rend ? re : rend;
                end = rowend > rb ? rowend - rb : 0u;
            }
            chunk_store8<OUT, ROWS>(ck, p - b0, v, end, base, s, sk);
        } else {
            uint32_t e[8];
            chunk_elems8<OUT>(ck, valid, base, s, sk, e);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < valid && (!RANGED || p + (uint32_t)j - rb < rend - rb)) chunk_put_sample<OUT>(ck, p + (uint32_t)j - b0, e[j]);
        }
    }

    // the signal's pad, by the whole workgroup, once per read
    __device__ __forceinline__ void finish() const { chunk_pad<OUT>(ck, (ROWS || RANGED) && pad_elems); }
    __device__ __forceinline__ void done() const {}
    __device__ __forceinline__ bool aligned() const { return (((uintptr_t)arena) & 15u) == 0; }
};

// ---- window store (SignalOut::wfirst; OUT = SIG_* | SIG_CHUNK | SIG_WINDOW): the typed samples into caller-listed windows ------------
// Row w of the read's n rows holds positions start[w] ... start[w] + L - 1 of the signal (the read's samples [rb, rb + T)); the starts are
// sorted (the window check), so the windows are sorted by their ends too.  A lane holds eight consecutive samples at signal position q0.
// The windows that hold one of them are consecutive in the list: from the first whose end lies behind the lane's first sample to the last
// that starts in front of its last one.  Into each of them the lane stores one whole line when all eight are samples of the signal and lie
// at a multiple of 8 of the window, wholly inside it; otherwise its samples inside the window one by one.  Only positions that hold a
// sample are ever written here: every other position of the rows is window_pad_kernel's.  No cross-lane exchange: the
// rule is the same for a read, a segment, a POD5 row and a range.
struct WindowK
{
    uint8_t* base = nullptr;          // the read's first row
    const int32_t* start = nullptr;   // its rows' starts
    uint64_t row_bytes = 0;           // L * E
    uint32_t n = 0, L = 0;            // rows, samples per row
    uint32_t rb = 0, T = 0;           // the signal: samples [rb, rb + T) of the read
};

// the windows of the read whose entry of SignalOut::wfirst is i (the window check has passed: the entries are rows of the arena -- a pair
// that is not gives no row, so no address is formed from it whatever comes in)
template <int OUT>
__device__ __forceinline__ WindowK window_constants(const ReadBatch& b, uint32_t i, uint32_t rb, uint32_t rend)
{
    WindowK w;
    const uint64_t a = b.sig.wfirst[i], z = b.sig.wfirst[i + 1];
    const bool ok = a <= z && z <= b.sig.wrows && z - a <= WINDOW_READ_ROWS_MAX;
    w.n = ok ? (uint32_t)(z - a) : 0u;
    w.L = b.sig.chunk_len;
    w.row_bytes = (uint64_t)w.L * OutBytes<OUT>::value;
    w.base = b.dst + (ok ? a : 0ull) * w.row_bytes;
    w.start = b.sig.wstart + (ok ? a : 0ull);
    w.rb = rb;
    w.T = rend - rb;
    return w;
}

// The window sink of one workgroup (the contract: this file's head): its values lie at s0 of the read (ROWS: a row of a POD5 read; else 0 -- put() gets positions in the
// read).  Every lane of the workgroup calls put() at the same point with i0 = the tile's first value + 8 x its thread number (the tile
// loops of svb_decode_range, I16DecPairs and svb16_decode_row), so the tile's samples [ta, tb) of the signal are workgroup-uniform, and
// so is the bracket [lo, hi) of its candidates: lo the first window that still reaches ta, hi the first that starts at or behind tb.
// The windows are sorted by start, hence by end, and a workgroup's tiles only move forward: both ends only advance, 64 windows a step
// (one load per lane and a ballot; every wavefront of the workgroup comes to the same values).  One binary search, at the workgroup's
// first tile that holds samples (a segment and a POD5 row start in the middle of the list; also if a tile ever lay in front of the one
// before).  A lane then walks the bracket alone, the same window in every lane at the same time.
template <int OUT, bool ROWS>
struct WindowStore
{
    static constexpr uint32_t UNSET = 0xFFFFFFFFu, BYTES = OutBytes<OUT>::value;
    WindowK wk;
    SigK sk;
    const uint8_t* arena = nullptr;   // aligned(): the window arena (ROWS: not looked at)
    uint32_t s0 = 0;
    mutable uint32_t lo = UNSET, hi = 0, at = 0;   // the bracket, and the first sample of the tile it was made for

    __device__ __forceinline__ int64_t end_of(uint32_t w) const { return (int64_t)wk.start[w] + (int64_t)wk.L; }
    // the first window that ends behind position q (n: none): wave-uniform arguments, wave-uniform result
    __device__ __forceinline__ uint32_t first_behind(int64_t q) const
    {
        uint32_t a = 0, z = wk.n;
        while (a < z) {
            const uint32_t mid = a + ((z - a) >> 1);
            if (end_of(mid) > q) z = mid;
            else a = mid + 1u;
        }
        return a;
    }
    // the first window at or behind c at which pred fails (n: none), pred holding on a prefix of [c, n): by the whole wavefront
    template <class P>
    __device__ __forceinline__ uint32_t advance(uint32_t c, P pred) const
    {
        const uint32_t lane = threadIdx.x & 63u;
        for (;;) {
            const uint32_t w = c + lane;
            const uint64_t m = __ballot(w < wk.n && pred(w) ? 1 : 0);
            const uint32_t k = m == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~m);
            c += k;
            if (k < 64u) return c;
        }
    }

    __device__ __forceinline__ void put(uint32_t i0, int valid, uint32_t base, const uint32_t s[8]) const
    {
        constexpr uint32_t OB = OutBytes<OUT>::value;
        if (wk.n == 0) return;
        // the tile (workgroup-uniform): values t0 ... t0 + 8 WG - 1 of the workgroup's, samples [ta, tb) of the signal
        const uint32_t t0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(i0 - 8u * threadIdx.x));
        const int64_t tq = (int64_t)(ROWS ? s0 : 0u) + (int64_t)t0 - (int64_t)wk.rb;
        const int64_t ta = tq < 0 ? 0 : tq, tb = tq + 8 * WG < (int64_t)wk.T ? tq + 8 * WG : (int64_t)wk.T;
        if (ta >= tb) return;   // no sample of the signal in the tile
        uint32_t a = lo, z = hi;
        if (a == UNSET || ta < (int64_t)at) {
            a = first_behind(ta);
            z = a;
        } else {
            a = advance(a, [&](uint32_t w) { return end_of(w) <= ta; });
        }
        z = advance(z > a ? z : a, [&](uint32_t w) { return (int64_t)wk.start[w] < tb; });
        a = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
        z = (uint32_t)__builtin_amdgcn_readfirstlane((int)z);
        lo = a;
        hi = z;
        at = (uint32_t)ta;
        // the lane: values jl ... jh - 1 of its eight are samples of the signal, at positions [qa, qb)
        const int64_t q0 = tq + 8 * (int64_t)threadIdx.x;
        const int64_t l0 = q0 < 0 ? -q0 : 0, h0 = (int64_t)wk.T - q0;
        const int jl = l0 < (int64_t)valid ? (int)l0 : valid, jh = h0 < (int64_t)valid ? (h0 < 0 ? 0 : (int)h0) : valid;
        if (jl >= jh || a >= z) return;
        const int64_t qa = q0 + jl, qb = q0 + jh;
        uint32_t e[8];
        chunk_elems8<OUT>(ChunkK(), 8, base, s, sk, e);
        const bool whole = jl == 0 && jh == 8;
        for (uint32_t c = a; c < z; ++c) {
            const int64_t st = wk.start[c];
            if (st >= qb) break;
            if (st + (int64_t)wk.L <= qa) continue;
            const int64_t d = q0 - st;   // the lane's first value in the window
            uint8_t* row = wk.base + (uint64_t)c * wk.row_bytes;
            if (whole && d >= 0 && d <= (int64_t)wk.L - 8 && (d & 7) == 0) {
                chunk_put8<OUT>(row + (size_t)d * OB, e);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int64_t pos = d + j;
                    if (j >= jl && j < jh && pos >= 0 && pos < (int64_t)wk.L) chunk_put1<OUT>(row + (size_t)pos * OB, e[j]);
                }
            }
        }
    }
    __device__ __forceinline__ void finish() const {}   // (the windows' pad: window_pad_kernel)
    __device__ __forceinline__ void done() const {}
    __device__ __forceinline__ bool aligned() const { return (((uintptr_t)arena) & 15u) == 0; }
};

// ---- event sink (SignalOut::events; OUT = SIG_EVENT [| SIG_RANGE]): per-event exact moments, no sample stored ---------------------------
// Event c of the read's n rows holds the positions start[c] <= q < start[c + 1] of the signal (the read's samples [rb, rb + T); the last
// event runs to T; positions in front of start[0] belong to no event).  The starts are sorted (the event check), so a lane's eight
// consecutive samples lie in consecutive events: the lane adds up each run of samples that share an event -- sum x in 32 bits, sum x^2 in
// 64, exact -- and adds the run to the event's two 64-bit words of moments when the run ends (no-return global adds: integer sums, so the
// order of the additions does not matter).  The words were zeroed by a launch in front (launch_event_zero).  The rule is the same for a
// read, a segment, a POD5 row and a range; no cross-lane exchange.
struct EventK
{
    unsigned long long* mom = nullptr;   // the read's first row's moments (two words a row)
    const uint32_t* start = nullptr;     // its rows' starts
    uint32_t n = 0;                      // rows
    uint32_t rb = 0, T = 0;              // the signal: samples [rb, rb + T) of the read
    uint32_t bias = 0;                   // SigK::bias
};

// the events of the read whose entry of SignalOut::wfirst is i (as window_constants: a pair that is not rows of the arena gives no row)
__device__ __forceinline__ EventK event_constants(const ReadBatch& b, uint32_t i, uint32_t rb, uint32_t rend)
{
    EventK k;
    const uint64_t a = b.sig.wfirst[i], z = b.sig.wfirst[i + 1];
    const bool ok = a <= z && z <= b.sig.wrows && z - a <= WINDOW_READ_ROWS_MAX;
    k.n = ok ? (uint32_t)(z - a) : 0u;
    k.mom = b.sig.event_moments(b.dst) + 2ull * (ok ? a : 0ull);
    k.start = reinterpret_cast<const uint32_t*>(b.sig.wstart) + (ok ? a : 0ull);
    k.rb = rb;
    k.T = rend - rb;
    k.bias = b.sig.bias;
    return k;
}

// The event sink of one workgroup (the contract: this file's head): its values lie at s0 of the read (a row of a POD5 read: begin_row();
// else 0 -- put() gets positions in the read).  As for the window sink the tile's samples [ta, tb) of the signal are workgroup-uniform,
// and so is the bracket [lo, hi) of the starts that lie inside the tile: lo the first start behind ta, hi the first at or behind tb.
// Both ends only advance, 64 starts a ballot step, with one binary search at the workgroup's first tile that holds samples.  The event of
// a lane's first sample is the last start at or in front of it: all of those lie in front of lo or inside the bracket, so the lane
// bisects the bracket alone (at most log2 of the tile's starts + 1 steps), then walks forward sample by sample.
struct EventStore
{
    static constexpr uint32_t UNSET = 0xFFFFFFFFu, BYTES = 2;   // (result[] is the int16 decode's)
    EventK ek;
    uint32_t s0 = 0;
    mutable uint32_t lo = UNSET, hi = 0, at = 0;   // the bracket, and the first sample of the tile it was made for

    __device__ __forceinline__ void begin_row(uint32_t s) { s0 = s; }
    __device__ __forceinline__ bool aligned() const { return true; }   // (nothing is stored)
    // the first start behind position q (n: none): wave-uniform arguments, wave-uniform result
    __device__ __forceinline__ uint32_t first_behind(uint32_t q) const
    {
        uint32_t a = 0, z = ek.n;
        while (a < z) {
            const uint32_t mid = a + ((z - a) >> 1);
            if (ek.start[mid] > q) z = mid;
            else a = mid + 1u;
        }
        return a;
    }
    // the first row at or behind c at which pred fails (n: none), pred holding on a prefix of [c, n): by the whole wavefront
    template <class P>
    __device__ __forceinline__ uint32_t advance(uint32_t c, P pred) const
    {
        const uint32_t lane = threadIdx.x & 63u;
        for (;;) {
            const uint32_t w = c + lane;
            const uint64_t m = __ballot(w < ek.n && pred(w) ? 1 : 0);
            const uint32_t k = m == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~m);
            c += k;
            if (k < 64u) return c;
        }
    }
    // a run of samples of row c: its sums into the row's moments
    __device__ __forceinline__ void add(uint32_t c, int32_t s1, uint64_t s2) const
    {
        atomicAdd(ek.mom + 2ull * c, (unsigned long long)(long long)s1);
        atomicAdd(ek.mom + 2ull * c + 1u, (unsigned long long)s2);
    }

    __device__ __forceinline__ void put(uint32_t i0, int valid, uint32_t base, const uint32_t s[8]) const
    {
        if (ek.n == 0) return;
        // the tile (workgroup-uniform): values t0 ... t0 + 8 WG - 1 of the workgroup's, samples [ta, tb) of the signal
        const uint32_t t0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(i0 - 8u * threadIdx.x));
        const int64_t tq = (int64_t)s0 + (int64_t)t0 - (int64_t)ek.rb;
        const int64_t ta = tq < 0 ? 0 : tq, tb = tq + 8 * WG < (int64_t)ek.T ? tq + 8 * WG : (int64_t)ek.T;
        if (ta >= tb) return;   // no sample of the signal in the tile
        uint32_t a = lo, z = hi;
        if (a == UNSET || ta < (int64_t)at) {
            a = first_behind((uint32_t)ta);
            z = a;
        } else {
            a = advance(a, [&](uint32_t w) { return (int64_t)ek.start[w] <= ta; });
        }
        z = advance(z > a ? z : a, [&](uint32_t w) { return (int64_t)ek.start[w] < tb; });
        a = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
        z = (uint32_t)__builtin_amdgcn_readfirstlane((int)z);
        lo = a;
        hi = z;
        at = (uint32_t)ta;
        // the lane: values jl ... jh - 1 of its eight are samples of the signal, the first of them at position qa
        const int64_t q0 = tq + 8 * (int64_t)threadIdx.x;
        const int64_t l0 = q0 < 0 ? -q0 : 0, h0 = (int64_t)ek.T - q0;
        const int jl = l0 < (int64_t)valid ? (int)l0 : valid, jh = h0 < (int64_t)valid ? (h0 < 0 ? 0 : (int)h0) : valid;
        if (jl >= jh) return;
        const uint32_t qa = (uint32_t)(q0 + jl);
        // c: the first row whose start lies behind qa -- row c - 1 is open (c == 0: none yet)
        uint32_t c = a, ce = z;
        while (c < ce) {
            const uint32_t mid = c + ((ce - c) >> 1);
            if (ek.start[mid] > qa) ce = mid;
            else c = mid + 1u;
        }
        uint32_t next = c < ek.n ? ek.start[c] : UNSET;   // (UNSET: the last row is open; no sample lies at 2^32 - 1)
        int32_t s1 = 0;
        uint64_t s2 = 0;
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < jl || j >= jh) continue;
            const uint32_t q = qa + (uint32_t)(j - jl);
            if (q >= next) {   // the run ends: rows with equal starts in between stay empty
                if (m != 0 && c != 0) add(c - 1u, s1, s2);
                s1 = 0;
                s2 = 0;
                m = 0;
                do {
                    ++c;
                    next = c < ek.n ? ek.start[c] : UNSET;
                } while (q >= next);
            }
            const uint32_t v = base + s[j];
            const int32_t x = ((int32_t)((v ^ ek.bias) << 16) >> 16) + (int32_t)ek.bias;   // (as sig_f32: the int16 or the uint16 value)
            s1 += x;
            s2 += (uint32_t)x * (uint32_t)x;   // (|x| < 2^16: the square fits 32 bits)
            ++m;
        }
        if (m != 0 && c != 0) add(c - 1u, s1, s2);
    }
    __device__ __forceinline__ void finish() const {}
    __device__ __forceinline__ void done() const {}
};

// ---- normalisation statistics (OUT = SIG_COUNT; vbz_kernels.h NormRead) -------------------------------------------------------------
// The counting pass histograms a read's keys into the windows of its NormRead in LDS; the select turns the counts into ranks.  A read on
// one workgroup is selected at the end of its pass with the counts still in LDS; on the large-read path every segment adds its counts to
// the read's slab (no-return atomics) and norm_select_kernel selects from there in a launch of its own.
struct NormLds
{
    uint32_t h[NORM_WINDOWS * NORM_BINS];   // the windows' bins (the select turns each window into its inclusive prefix sums)
    uint32_t below[NORM_WINDOWS];           // keys below each window (anchored: below window 0 only)
    uint32_t tot[NORM_WINDOWS];             // keys in each window
    uint32_t az[2 * NORM_WINDOWS];          // the targets' new brackets
};
__device__ __forceinline__ NormLds* norm_lds()
{
    __shared__ __attribute__((aligned(16))) NormLds L;
    return &L;
}

// the smallest x in [lo, hi] with pred(x), pred monotone and true at hi: 64 candidates a round, every lane of the wave (wave-uniform)
template <class P>
__device__ __forceinline__ uint32_t wave_search(uint32_t lo, uint32_t hi, P pred)
{
    const uint32_t lane = threadIdx.x & 63u;
    while (lo < hi) {
        const uint32_t step = (hi - lo + 64u) >> 6;
        const uint32_t e0 = lo + (lane + 1u) * step - 1u, e = e0 < hi ? e0 : hi;
        const uint64_t m = __ballot(pred(e) ? 1 : 0);
        const uint32_t f = m ? (uint32_t)__ffsll((unsigned long long)m) - 1u : 63u;   // (m == 0 only if the caller's promise fails)
        const uint32_t nhi = lo + (f + 1u) * step - 1u;
        lo += f * step;
        hi = nhi < hi ? nhi : hi;
    }
    return lo;
}

// the ranks (0-based, in sorted order) whose values a stage wants: MED_MAD the two middle ones (both stages); QUANTILE floor(q (T - 1))
// and the one above it, for both quantiles.  T >= 1.
__device__ __forceinline__ double norm_h(float q, uint32_t T) { return __dmul_rn((double)q, (double)(T - 1u)); }
__device__ __forceinline__ void norm_ranks(const NormOut& no, uint32_t T, uint32_t R[NORM_WINDOWS])
{
    if (no.method == NORM_MED_MAD) {
        R[0] = (T - 1u) >> 1;
        R[1] = R[2] = R[3] = T >> 1;
    } else {
        const uint32_t ja = (uint32_t)floor(norm_h(no.qa, T)), jb = (uint32_t)floor(norm_h(no.qb, T));
        R[0] = ja;
        R[1] = ja + 1u < T ? ja + 1u : T - 1u;
        R[2] = jb;
        R[3] = jb + 1u < T ? jb + 1u : T - 1u;
    }
}

// numpy's quantile (method "linear") from the two values around rank h = q (T - 1), in float64 without contraction
__device__ __forceinline__ double norm_quantile(float q, uint32_t T, double a, double b)
{
    const double h = norm_h(q, T), t = __dsub_rn(h, floor(h)), d = __dsub_rn(b, a);
    return t < 0.5 ? __dadd_rn(a, __dmul_rn(d, t)) : __dsub_rn(b, __dmul_rn(d, __dsub_rn(1.0, t)));
}

// c, w -> shift = max(shift_min, shift_mul c), scale = max(scale_min, scale_mul w) (float64, rounded once to float32); the store's
// constants {-shift, float32(1 / float64(scale))}
__device__ __forceinline__ void norm_finish(const ReadBatch& b, uint32_t r, double c, double w)
{
    const NormOut& no = b.sig.norm;
    const double sd = fmax((double)no.shift_min, __dmul_rn((double)no.shift_mul, c));
    const double kd = fmax((double)no.scale_min, __dmul_rn((double)no.scale_mul, w));
    const float shift = __double2float_rn(sd), scale = __double2float_rn(kd);
    const_cast<float2*>(b.sig.cal)[r] = make_float2(-shift, __double2float_rn(__ddiv_rn(1.0, (double)scale)));
    no.ss[no.map ? no.map[r] : r] = make_float2(shift, scale);
}

// the windows of the next pass: one per unresolved bracket (equal brackets share one), wide enough to hold it whole
__device__ __forceinline__ void norm_windows(NormRead* sp, const uint32_t A[NORM_WINDOWS], const uint32_t Z[NORM_WINDOWS])
{
#pragma unroll
    for (int t = 0; t < (int)NORM_WINDOWS; ++t) {
        bool off = A[t] == Z[t];
#pragma unroll
        for (int v = 0; v < t; ++v) off = off || (A[v] == A[t] && Z[v] == Z[t]);
        uint32_t s = 0;
        while ((NORM_BINS << s) < Z[t] - A[t] + 1u) ++s;
        sp->lo[t] = A[t];
        sp->sh[t] = off ? NORM_OFF : s;
        sp->a[t] = A[t];
        sp->z[t] = Z[t];
    }
    sp->anchored = 0;
}

// The select, by the whole workgroup, from the counts of read r (T >= 1 values) in L: every target's bracket is narrowed; when all are
// found the stage ends (the value stage of MED_MAD hands over to the MAD's, which the first pass's adjacent windows often answer at once),
// and the read's constants are written.  L->h is overwritten.  xoff: key - value (0x8000 for int16, 0 for uint16).
__device__ __forceinline__ void norm_select(NormLds* L, const ReadBatch& b, uint32_t r, uint32_t T, uint32_t xoff)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const NormOut& no = b.sig.norm;
    NormRead* sp = no.st + r;
    {   // wave w: the inclusive prefix sums of window w, in place
        uint32_t* h = L->h + wv * NORM_BINS + lane * 16;
        uint32_t v[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint4 q = *reinterpret_cast<const uint4*>(h + 4 * j);
            v[4 * j] = q.x;
            v[4 * j + 1] = q.y;
            v[4 * j + 2] = q.z;
            v[4 * j + 3] = q.w;
        }
        uint32_t sum = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) sum += v[j];
        const uint32_t inc = wave_incl_scan_u32(sum);
        uint32_t run = inc - sum;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            run += v[j];
            v[j] = run;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<uint4*>(h + 4 * j) = make_uint4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
        if (lane == 63) L->tot[wv] = inc;
    }
    wg_lds_barrier();
    const uint32_t phase = sp->phase, anchored = sp->anchored;
    uint32_t lo[NORM_WINDOWS], sh[NORM_WINDOWS], below[NORM_WINDOWS], cum[NORM_WINDOWS], R[NORM_WINDOWS];
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < (int)NORM_WINDOWS; ++w) {
        lo[w] = sp->lo[w];
        sh[w] = sp->sh[w];
        cum[w] = c;   // (anchored: keys in the windows before w)
        below[w] = anchored ? L->below[0] + c : L->below[w];
        c += L->tot[w];
    }
    norm_ranks(no, T, R);
    {   // wave t: target t
        const int t = wv;
        uint32_t a = sp->a[t], z = sp->z[t];
        if (a != z) {
#pragma unroll
            for (int w = 0; w < (int)NORM_WINDOWS; ++w) {
                if (sh[w] == NORM_OFF) continue;
                const uint32_t B = below[w], tw = L->tot[w], end = lo[w] + (NORM_BINS << sh[w]);
                if (R[t] >= B && R[t] - B < tw) {   // in window w: the bin where the prefix sums pass the rank
                    const uint32_t g = R[t] - B;
                    const uint32_t* P = L->h + w * NORM_BINS;
                    const uint32_t bin = wave_search(0u, NORM_BINS - 1u, [&](uint32_t x) { return P[x] > g; });
                    const uint32_t a1 = lo[w] + (bin << sh[w]), z1 = a1 + (1u << sh[w]) - 1u;
                    a = a1 > a ? a1 : a;
                    z = z1 < z ? z1 : z;
                    break;
                }
                if (R[t] < B) {
                    if (lo[w] != 0 && lo[w] - 1u < z) z = lo[w] - 1u;
                } else if (end > a) {
                    a = end;
                }
            }
            if (a > z) a = z;   // (only a stream whose counts disagree with its length comes here: it gets an error verdict)
        }
        if (lane == 0) {
            L->az[t] = a;
            L->az[NORM_WINDOWS + t] = z;
        }
    }
    wg_lds_barrier();
    if (wv != 0) return;
    uint32_t A[NORM_WINDOWS], Z[NORM_WINDOWS];
    bool all = true;
#pragma unroll
    for (int t = 0; t < (int)NORM_WINDOWS; ++t) {
        A[t] = L->az[t];
        Z[t] = L->az[NORM_WINDOWS + t];
        all = all && A[t] == Z[t];
    }
    auto x = [&](uint32_t u) { return (double)((int32_t)u - (int32_t)xoff); };
    if (!all) {
        if (lane == 0) norm_windows(sp, A, Z);
        return;
    }
    if (phase == NORM_DEV) {   // |x - c| = d / 2: the MAD is (d0 + d1) / 4, exactly
        if (lane == 0) {
            norm_finish(b, r, (double)((int32_t)(sp->c2) - 2 * (int32_t)xoff) * 0.5, (double)(A[0] + A[1]) * 0.25);
            sp->phase = NORM_DONE;
        }
        return;
    }
    if (no.method == NORM_QUANTILE) {
        if (lane == 0) {
            const double qa = norm_quantile(no.qa, T, x(A[0]), x(A[1])), qb = norm_quantile(no.qb, T, x(A[2]), x(A[3]));
            norm_finish(b, r, __dadd_rn(qa, qb), __dsub_rn(qb, qa));
            sp->phase = NORM_DONE;
        }
        return;
    }
    // MED_MAD: the median is known; the MAD's ranks of d = |2u - c2| straight from the first pass's 4 x NORM_BINS adjacent keys, when
    // the band they need lies inside them
    const uint32_t c2 = A[0] + A[1];
    if (anchored && c2 >= 2u * lo[0] && c2 <= 2u * (lo[0] + NORM_WINDOWS * NORM_BINS - 1u)) {   // (always so, unless counts disagree)
        const uint32_t L0 = lo[0], Dmax = min(c2 - 2u * L0, 2u * L0 + 2u * NORM_WINDOWS * NORM_BINS - 1u - c2);
        auto G = [&](uint32_t u) -> uint32_t {   // keys <= u, for u in [L0 - 1, L0 + 4095]
            if (u + 1u == L0) return below[0];
            const uint32_t i = u - L0, w = i / NORM_BINS;
            return below[0] + cum[w] + L->h[i];
        };
        auto cnt = [&](uint32_t D) { return G((c2 + D) >> 1) - G(((c2 - D + 1u) >> 1) - 1u); };   // deviations d <= D
        if (cnt(Dmax) > R[1]) {
            const uint32_t d0 = wave_search(0u, Dmax, [&](uint32_t D) { return cnt(D) > R[0]; });
            const uint32_t d1 = wave_search(0u, Dmax, [&](uint32_t D) { return cnt(D) > R[1]; });
            if (lane == 0) {
                norm_finish(b, r, __dadd_rn(x(A[0]), x(A[1])) * 0.5, (double)(d0 + d1) * 0.25);
                sp->phase = NORM_DONE;
            }
            return;
        }
    }
    if (lane == 0) {
        uint32_t A2[NORM_WINDOWS], Z2[NORM_WINDOWS];
#pragma unroll
        for (int t = 0; t < (int)NORM_WINDOWS; ++t) {
            A2[t] = 0;
            Z2[t] = 2u * 0xFFFFu;
        }
        norm_windows(sp, A2, Z2);
        sp->c2 = c2;
        sp->phase = NORM_DEV;
    }
}

// the counting store's state: the read's windows (workgroup-uniform) and this lane's counts of keys below them
struct NormK
{
    NormLds* L = nullptr;
    const ReadBatch* b = nullptr;
    uint32_t r = 0, T = 0, kx = 0, c2 = 0, lo0 = 0;
    bool dev = false, anchored = false;
    uint32_t lo[NORM_WINDOWS] = {}, sh[NORM_WINDOWS] = {};
};

// ---- signal trim (OUT = SIG_TRIM; vbz_kernels.h TrimOut; the rule: include/vbz_gpu.h) ---------------------------------------------------
// The trim store's state, per read and workgroup-uniform.  A sample is high when float64(x) > thr; on the key u the counting pass forms
// (x = u - kx) that is u >= hk, hk the smallest high key, clamped to [0, 65536] (65536: no sample is high).  Window k = (p - t0) / W of
// the nW windows in front of `end` = t0 + nW W <= N = min(M, T); word k of the counting passes' bins (NormLds::h; the large-read path:
// the read's slab) counts the window's high samples, and its bit 31 says that the window's last sample is high.
struct TrimK
{
    NormLds* L = nullptr;
    uint32_t* out = nullptr;    // the read's entry of TrimOut::begin
    uint32_t* slab = nullptr;   // large-read path: the read's words in scratch (the segments add theirs up there), else nullptr
    uint32_t hk = 0x10000u, kx = 0;
    uint32_t t0 = 0, W = 1, m = 0, flags = 0, T = 0, N = 0, nW = 0, span = 0, end = 0;   // span = nW W
    uint32_t mul = 0, sh = 0;   // d / W = d mul >> sh for d < 2^28 (span <= TRIM_MAX_WINDOWS x 65536 = 2^28)
    float max_fraction = 1.0f;
};

// the state of read r of T samples whose statistics are final (its {shift, scale} in NormOut::ss)
__device__ __forceinline__ TrimK trim_state(const ReadBatch& b, const TrimOut& tr, uint32_t r, uint32_t T)
{
    const NormOut& no = b.sig.norm;
    const uint32_t i = no.map ? no.map[r] : r;
    TrimK k;
    k.out = tr.begin + i;
    k.kx = b.sig.bias ^ 0x8000u;
    k.t0 = tr.t0;
    k.W = tr.W;
    k.m = tr.m;
    k.flags = tr.flags;
    k.max_fraction = tr.max_fraction;
    k.T = T;
    k.N = tr.M < T ? tr.M : T;
    k.nW = k.N > k.t0 ? (k.N - k.t0) / k.W : 0u;
    if (k.nW > TRIM_MAX_WINDOWS) k.nW = TRIM_MAX_WINDOWS;   // (the host refuses such a trim: no word is formed outside the bins whatever comes in)
    k.span = k.nW * k.W;
    k.end = k.nW ? k.t0 + k.span : 0u;
    uint32_t l = 0;
    while ((1u << l) < k.W) ++l;   // d < 2^28 and W <= 2^l: ceil(2^(28 + l) / W) <= 2^29 gives the exact quotient
    k.sh = 28u + l;
    k.mul = (uint32_t)((((uint64_t)1 << k.sh) + k.W - 1u) / k.W);
    if (k.nW) {
        const float2 ss = no.ss[i];
        const double thr = __dadd_rn((double)ss.x, __dmul_rn((double)tr.f, (double)ss.y));   // (multiply, then add: no FMA)
        const double h = floor(thr) + 1.0 + (double)k.kx;   // the smallest key above thr (exact: |thr| beyond 2^52 only where it is clamped)
        k.hk = !(thr == thr) ? 0x10000u : (h >= 65536.0 ? 0x10000u : (h > 0.0 ? (uint32_t)h : 0u));
    }
    return k;
}

// The scan of a read's nW window words h[], by one wavefront (wave-uniform): the first window with more than m high samples opens the
// peak, the first window at or behind it whose last sample is not high ends it, and that window's end is the answer unless one of the
// two rejections sends it back to min(t0, T) -- as no peak and a peak that never comes down do.  Lane 0 writes the read's begin entry.
__device__ __forceinline__ void trim_scan(const uint32_t* h, const TrimK& k)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t ans = k.t0 < k.T ? k.t0 : k.T;
    bool seen = false;
    for (uint32_t base = 0; base < k.nW; base += 64u) {
        const bool valid = base + lane < k.nW;
        const uint32_t v = valid ? h[base + lane] : 0u;
        uint64_t from = ~0ull;
        if (!seen) {
            const uint64_t mo = __ballot(valid && (v & 0x7FFFFFFFu) > k.m ? 1 : 0);
            if (!mo) continue;
            seen = true;
            from <<= (uint32_t)__ffsll((unsigned long long)mo) - 1u;
        }
        const uint64_t ms = __ballot(valid && !(v >> 31) ? 1 : 0) & from;
        if (ms) {
            const uint32_t e = k.t0 + (base + (uint32_t)__ffsll((unsigned long long)ms)) * k.W;   // the stopping window's end
            const bool reject = ((k.flags & TRIM_REJECT_AT_END) && e >= k.N) || (double)e > __dmul_rn((double)k.max_fraction, (double)k.T);
            if (!reject) ans = e;
            break;
        }
    }
    if (lane == 0) *k.out = ans;
}

// OUT = SIG_NONE: the ELEM-byte values into the read's slot (dst + dst_off[r])
template <int ELEM>
struct RawStore
{
    static constexpr int VPL = Vpl<ELEM>::value;
    static constexpr uint32_t BYTES = ELEM;
    uint8_t* out;   // the read's slot
    __device__ __forceinline__ bool aligned() const { return (((uintptr_t)out) & 15u) == 0; }
    __device__ __forceinline__ void put(uint32_t i0, int valid, uint32_t base, const uint32_t s[VPL]) const
    {
        if (valid == VPL && aligned()) {
            uint32_t w[4];
            if (ELEM == 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) w[k] = base + s[k % VPL];
            } else if (ELEM == 2) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    w[k] = ((base + s[(2 * k) % VPL]) & 0xFFFFu) | ((base + s[(2 * k + 1) % VPL]) << 16);
            } else {
                w[2] = w[3] = 0;
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    w[k] = ((base + s[(4 * k) % VPL]) & 0xFFu) | (((base + s[(4 * k + 1) % VPL]) & 0xFFu) << 8) |
                           (((base + s[(4 * k + 2) % VPL]) & 0xFFu) << 16) | ((base + s[(4 * k + 3) % VPL]) << 24);
            }
            if (ELEM == 1) {
                *reinterpret_cast<uint2*>(out + (size_t)i0) = make_uint2(w[0], w[1]);
            } else {
                *reinterpret_cast<uint4*>(out + (size_t)i0 * ELEM) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < VPL; ++k)
                if (k < valid) store_elem(out + (size_t)(i0 + k) * ELEM, ELEM, base + s[k]);
        }
    }
    __device__ __forceinline__ void finish() const {}
    __device__ __forceinline__ void done() const {}
};

// OUT = SIG_F32 / F16 / BF16: the typed samples into the read's typed slot (dst + dst_off[r] / 2 * E: dst_off is the int16 layout's)
template <int OUT>
struct TypedStore
{
    static constexpr uint32_t BYTES = OutBytes<OUT>::value;
    uint8_t* out;   // the read's slot
    SigK sk;
    __device__ __forceinline__ bool aligned() const { return (((uintptr_t)out) & 15u) == 0; }
    __device__ __forceinline__ void put(uint32_t i0, int valid, uint32_t base, const uint32_t s[8]) const
    {
        if (valid == 8 && aligned()) {
            sig_store8<OUT>(out + (size_t)i0 * BYTES, base, s, sk);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < valid) sig_store1<OUT>(out + (size_t)(i0 + k) * BYTES, base + s[k], sk);
        }
    }
    __device__ __forceinline__ void finish() const {}
    __device__ __forceinline__ void done() const {}
};

// OUT = SIG_COUNT [| SIG_RANGE]: the counting pass of a normalising decode -- nothing is stored; every value's key goes to its bin in LDS.
// RANGED: only the positions [rb, rend) of the read are counted -- the others are decoded (the delta chain needs them) and skipped.
template <bool RANGED>
struct CountStore
{
    static constexpr uint32_t BYTES = 2;   // (a counting pass that writes result[] writes the int16 decode's)
    NormK nk;
    mutable uint32_t nbelow[NORM_WINDOWS] = {};   // this lane's keys below each window
    uint32_t rb = 0, rend = 0, s0 = 0;            // RANGED (else not looked at): the range; where put()'s values begin in the read (a POD5 read: row by row)
    // read r of `count` samples, by all threads of the workgroup: the bins are zeroed here
    __device__ __forceinline__ CountStore(const ReadBatch* b, uint32_t r, uint32_t count) : rend(count)
    {
        if constexpr (RANGED) sample_range(b->sig, r, count, &rb, &rend);   // the store's read is the range
        const NormRead* sp = b->sig.norm.st + r;
        nk.L = norm_lds();
        nk.b = b;
        nk.r = r;
        nk.T = rend - rb;
        nk.kx = b->sig.bias ^ 0x8000u;
        nk.dev = sp->phase == NORM_DEV;
        nk.anchored = sp->anchored != 0;
        nk.c2 = sp->c2;
#pragma unroll
        for (int w = 0; w < (int)NORM_WINDOWS; ++w) {
            nk.lo[w] = sp->lo[w];
            nk.sh[w] = sp->sh[w];
        }
        nk.lo0 = nk.lo[0];
        uint4* h = reinterpret_cast<uint4*>(nk.L->h);
        for (uint32_t i = threadIdx.x; i < NORM_WINDOWS * NORM_BINS / 4; i += WG) h[i] = make_uint4(0u, 0u, 0u, 0u);
        if (threadIdx.x < NORM_WINDOWS) nk.L->below[threadIdx.x] = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void begin_row(uint32_t s) { s0 = s; }
    __device__ __forceinline__ bool aligned() const { return true; }   // (nothing is stored)
    // one LDS increment per value: its key's bin
    __device__ __forceinline__ void put(uint32_t i0, int valid, uint32_t base, const uint32_t s[8]) const
    {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k >= valid) continue;
            if constexpr (RANGED) {
                if (s0 + i0 + (uint32_t)k - rb >= rend - rb) continue;   // (outside [rb, rend))
            }
            const uint32_t u = ((base + s[k]) ^ nk.kx) & 0xFFFFu;
            const uint32_t key = nk.dev ? (uint32_t)abs((int32_t)(2u * u) - (int32_t)nk.c2) : u;
            if (nk.anchored) {   // four adjacent windows of width 1
                const uint32_t d = key - nk.lo0;
                if (d < NORM_WINDOWS * NORM_BINS) atomicAdd(&nk.L->h[d], 1u);
                else if (key < nk.lo0) ++nbelow[0];
            } else {
#pragma unroll
                for (int w = 0; w < (int)NORM_WINDOWS; ++w) {
                    if (nk.sh[w] == NORM_OFF) continue;
                    const uint32_t d = key - nk.lo[w];
                    if ((d >> nk.sh[w]) < NORM_BINS) atomicAdd(&nk.L->h[w * NORM_BINS + (d >> nk.sh[w])], 1u);
                    else if (key < nk.lo[w]) ++nbelow[w];
                }
            }
        }
    }
    __device__ __forceinline__ void finish() const {}
    // the counts are complete -- a read on one workgroup is selected from LDS, a segment of the large-read path adds them to the read's slab
    __device__ __forceinline__ void done() const
    {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int w = 0; w < (int)NORM_WINDOWS; ++w) {
            const uint32_t t = wave_incl_scan_u32(nbelow[w]);
            if (lane == 63 && t != 0) atomicAdd(&nk.L->below[w], t);
        }
        __syncthreads();
        const NormOut& no = nk.b->sig.norm;
        if (no.slab) {
            uint32_t* slab = no.slab + (size_t)nk.r * NORM_SLAB;
            for (uint32_t i = threadIdx.x; i < NORM_WINDOWS * NORM_BINS; i += WG) {
                const uint32_t v = nk.L->h[i];
                if (v) atomicAdd(slab + i, v);
            }
            if (threadIdx.x < NORM_WINDOWS && nk.L->below[threadIdx.x]) atomicAdd(slab + NORM_WINDOWS * NORM_BINS + threadIdx.x, nk.L->below[threadIdx.x]);
        } else if (RANGED && nk.T == 0) {   // (an empty range of a read that has samples: c = w = 0, as norm_init_read says for an empty read)
            if (threadIdx.x == 0) {
                norm_finish(*nk.b, nk.r, 0.0, 0.0);
                no.st[nk.r].phase = NORM_DONE;
            }
        } else {
            norm_select(nk.L, *nk.b, nk.r, nk.T, nk.kx);
        }
    }
};

// OUT = SIG_TRIM: the trim pass -- nothing is stored; the high samples of the read's prefix are counted per window
struct TrimStore
{
    static constexpr uint32_t BYTES = 2;
    TrimK tk;
    uint32_t s0 = 0;   // where the values handed to put() begin in the read (a POD5 read: row by row)
    // k: the read's state (trim_state), by all threads of the workgroup: its window words are zeroed here
    __device__ __forceinline__ explicit TrimStore(const TrimK& k) : tk(k)
    {
        tk.L = norm_lds();
        for (uint32_t i = threadIdx.x; i < tk.nW; i += WG) tk.L->h[i] = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void begin_row(uint32_t s) { s0 = s; }
    __device__ __forceinline__ bool aligned() const { return true; }   // (nothing is stored)
    // one LDS increment per HIGH value of the prefix: its window's word (most values are not high)
    __device__ __forceinline__ void put(uint32_t i0, int valid, uint32_t base, const uint32_t s[8]) const
    {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t u = ((base + s[k]) ^ tk.kx) & 0xFFFFu, d = s0 + i0 + (uint32_t)k - tk.t0;
            if (k < valid && u >= tk.hk && d < tk.span) {
                const uint32_t w = (uint32_t)(((uint64_t)d * tk.mul) >> tk.sh);
                atomicAdd(&tk.L->h[w], d - w * tk.W == tk.W - 1u ? 0x80000001u : 1u);   // (bit 31: the window's last sample)
            }
        }
    }
    __device__ __forceinline__ void finish() const {}
    // a read on one workgroup is scanned from LDS by one wavefront; a segment adds its non-zero words to the read's slab (added, never
    // stored: a window may straddle two segments; bit 31 comes from one sample only, so the sums do not carry into it)
    __device__ __forceinline__ void done() const
    {
        __syncthreads();
        if (tk.slab) {
            for (uint32_t i = threadIdx.x; i < tk.nW; i += WG) {
                const uint32_t v = tk.L->h[i];
                if (v) atomicAdd(tk.slab + i, v);
            }
        } else if (threadIdx.x < 64) {
            trim_scan(tk.L->h, tk);
        }
    }
};

// ---- signal segmentation (vbz_kernels.h SegmentOut; the rule: include/vbz_gpu.h) --------------------------------------------------------
// The first sink that needs a neighbourhood of each sample: a position's verdict depends on the H = max(w1, w2) + r samples on either
// side of it.  The sink's workgroup walks its read's whole signal in order (one workgroup per read on every path: DESIGN.md 4.20), so the
// halo is a matter of LDS alone.  put() stages the tile's samples in a ring indexed by signal position; behind one barrier the workgroup
// scores every position whose two windows are staged by now (a lane takes eight consecutive positions and slides the four window sums),
// the scores going to a second ring; behind a second barrier a lane takes a group of eight positions whose scores of [8k - r, 8k + 8 + r]
// are all there, applies the boundary test and writes the group's byte of the read's map.  Both rings hold 4 096 positions: a tile of
// 2 048, the halo on both sides and the up to 15 positions a group waits for.  The put that stages the signal's last sample also flushes
// what was waiting for samples past the end (the scores there are 0 by the rule).
// Ring hazards: staging writes ring positions no score phase reads before the barrier behind it, and the barrier between the score and
// the boundary phase keeps the next put's staging behind this put's ring reads; the next put's scores are written behind its staging
// barrier, which every lane reaches only after its boundary phase.
constexpr uint32_t SEGMENT_RING = 4096;
#ifndef VBZ_SEGMENT_PRETEST
#define VBZ_SEGMENT_PRETEST 1   // (0: both divisions at every position -- the build that measures what the pre-test saves)
#endif
struct SegmentLds
{
    double score[SEGMENT_RING];
    uint16_t ring[SEGMENT_RING];
    uint32_t hi, bits;   // positions [0, hi) of the signal are staged; the boundaries found
};
__device__ __forceinline__ SegmentLds* segment_lds()
{
    __shared__ __attribute__((aligned(16))) SegmentLds L;
    return &L;
}

// the scores of positions [qa, qe) of a signal of T samples into the score ring, by the whole workgroup: s = max(s_1, s_2),
// s_d = (float64(N) / float64(D)) / (float64(t) float64(t)) where w <= q <= T - w, else 0, N and D exact integers.  A score below 1 can
// neither be a boundary nor suppress one, so it is stored as 0 and the two divisions are only made where N >= 0.99 D t^2 in float64 --
// the three roundings of the exact expression move it by less than one part in 2^50.  The window sums slide: the values that enter at
// positions outside the signal are whatever the ring holds there and leave again unchanged (integer sums), and no score is taken from them.
__device__ __forceinline__ void segment_scores(SegmentLds* L, const SegmentOut& so, uint32_t bias, uint32_t qa, uint32_t qe, uint32_t T)
{
#pragma clang fp contract(off)
    auto X = [&](uint32_t q) -> int64_t {   // (as sig_f32: the int16 or the uint16 value)
        const uint32_t v = L->ring[q & (SEGMENT_RING - 1u)];
        return (int64_t)(((int32_t)((v ^ bias) << 16) >> 16) + (int32_t)bias);
    };
    for (uint32_t q0 = qa + 8u * threadIdx.x; q0 < qe; q0 += 8u * WG) {
        double sc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) sc[j] = 0.0;
        for (int d = 0; d < 2; ++d) {
            const uint32_t w = d ? so.w2 : so.w1;
            if (w == 0) continue;
            const double kk = d ? so.k2 : so.k1;
            int64_t A = 0, B = 0, A2 = 0, B2 = 0;
            for (uint32_t j = 0; j < w; ++j) {
                const int64_t a = X(q0 - w + j), c = X(q0 + j);
                A += a;
                A2 += a * a;
                B += c;
                B2 += c * c;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t q = q0 + (uint32_t)j;
                if (q < qe && q >= w && q + w <= T) {
                    const int64_t dm = A - B, N = (int64_t)w * dm * dm;
                    int64_t D = (int64_t)w * (A2 + B2) - A * A - B * B;
                    if (D < 1) D = 1;
                    const double nd = (double)N, dd = (double)D;
                    if (!VBZ_SEGMENT_PRETEST || nd >= 0.99 * (dd * kk)) {
                        const double s = (nd / dd) / kk;
                        if (s > sc[j]) sc[j] = s;
                    }
                }
                const int64_t xm = X(q - w), x0 = X(q), xp = X(q + w);
                A += x0 - xm;
                A2 += x0 * x0 - xm * xm;
                B += xp - x0;
                B2 += xp * xp - x0 * x0;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (q0 + (uint32_t)j < qe) L->score[(q0 + (uint32_t)j) & (SEGMENT_RING - 1u)] = sc[j] >= 1.0 ? sc[j] : 0.0;
    }
}

// The segmentation sink of one workgroup (the contract: this file's head): its values lie at s0 of the read (a row of a POD5 read:
// begin_row(); else 0), the signal is the read's samples [rb, rb + T).  Built by all threads of the workgroup.
struct SegmentStore
{
    static constexpr uint32_t BYTES = 2;   // (result[] is the int16 decode's)
    SegmentLds* L;
    SegmentOut so;
    uint8_t* map;      // the read's
    uint32_t* rows;    // the read's entry of SegmentOut::rows
    uint32_t rb, T, bias, H, wmax;
    uint32_t s0 = 0;
    mutable uint32_t scored = 0, lo = 0, nb = 0;   // scores of [0, scored) and groups [0, lo) are done (workgroup-uniform); this lane's boundaries

    __device__ __forceinline__ SegmentStore(const SegmentOut& o, uint32_t i, uint32_t rb_, uint32_t T_, uint32_t bias_)
        : L(segment_lds()), so(o), map(o.map + o.map_off[i]), rows(o.rows + i), rb(rb_), T(T_), bias(bias_)
    {
        wmax = so.w1 > so.w2 ? so.w1 : so.w2;
        H = wmax + so.r;
        if (threadIdx.x == 0) {
            L->hi = 0;
            L->bits = 0;
        }
        __syncthreads();
    }
    __device__ __forceinline__ void begin_row(uint32_t s) { s0 = s; }
    __device__ __forceinline__ bool aligned() const { return true; }   // (nothing is stored)

    // the groups [lo, khi) of eight positions: the boundary test on the scores, one byte of the map per lane and group
    __device__ __forceinline__ void pick(uint32_t khi) const
    {
        const uint32_t r = so.r;
        auto S = [&](uint32_t q) { return L->score[q & (SEGMENT_RING - 1u)]; };
        for (uint32_t k = lo + threadIdx.x; k < khi; k += WG) {
            uint32_t byte = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t q = 8u * k + (uint32_t)j;
                if (q < 1u || q >= T) continue;
                const double v = S(q);
                if (!(v >= 1.0)) continue;
                bool ok = true;
                for (uint32_t u = q > r ? q - r : 0u; u < q && ok; ++u) ok = v > S(u);
                const uint32_t jh = q + r < T ? q + r : T;
                for (uint32_t u = q + 1u; u <= jh && ok; ++u) ok = v >= S(u);
                if (ok) byte |= 1u << j;
            }
            map[k] = (uint8_t)byte;
            nb += (uint32_t)__popc(byte);
        }
    }

    __device__ __forceinline__ void put(uint32_t i0, int valid, uint32_t base, const uint32_t s[8]) const
    {
        // stage: the lane's samples at their positions of the signal; the wavefront's last lane that has samples says how far they reach
        const uint32_t p = s0 + i0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t q = p + (uint32_t)j - rb;
            if (j < valid && q < T) L->ring[q & (SEGMENT_RING - 1u)] = (uint16_t)(base + s[j]);
        }
        const uint64_t m = __ballot(valid > 0 ? 1 : 0);
        if (m != 0 && (threadIdx.x & 63u) == 63u - (uint32_t)__builtin_clzll(m)) {
            const uint32_t e = p + (uint32_t)valid;
            atomicMax(&L->hi, e <= rb ? 0u : (e - rb < T ? e - rb : T));
        }
        wg_lds_barrier();
        const uint32_t hi = L->hi;
        const bool last = hi >= T;
        const uint32_t shi = last ? T + 1u : (hi >= wmax ? hi - wmax + 1u : 0u);   // scores of [0, shi) can be taken now
        if (shi > scored) segment_scores(L, so, bias, scored, shi, T);
        wg_lds_barrier();
        const uint32_t khi = last ? (T + 7u) >> 3 : (shi >= so.r + 8u ? (shi - so.r) >> 3 : 0u);
        if (khi > lo) {
            pick(khi);
            lo = khi;
        }
        if (shi > scored) scored = shi;
    }
    __device__ __forceinline__ void finish() const {}
    // the read's row count: its boundaries and row 0 (an empty signal: none)
    __device__ __forceinline__ void done() const
    {
        const uint32_t t = wave_incl_scan_u32(nb);
        if ((threadIdx.x & 63u) == 63u && t != 0) atomicAdd(&L->bits, t);
        __syncthreads();
        if (threadIdx.x == 0) *rows = T ? L->bits + 1u : 0u;
    }
};

// ---- signal spans (vbz_kernels.h SpanOut; the rule: include/vbz_gpu.h) -------------------------------------------------------------------
// The cheap sink: a position's bit depends on that sample alone -- no neighbourhood, no LDS, no barrier, no float arithmetic per sample.
// Once per read the threshold becomes a pair of key bounds as trim_state makes hk (x = u - kx on the key u): ABOVE, float64(x) > thr is
// u >= floor(thr) + 1 + kx; BELOW, float64(x) < thr is u < ceil(thr) + kx; each clamped to [0, 65536], a NaN thr giving the empty set.  Both
// directions are one unsigned compare, u - lo < n.
// The map is indexed by the sample's position in the READ (not in its range), so that a lane's eight samples are one byte wherever the
// lane's values begin at a multiple of 8 of the read: on the one-workgroup walk (i0 = 8 x lane from 0) and in every segment of the
// large-read path (segments begin at multiples of 16 384).  The invariant: every byte of a passing read's map has a defined value after
// the pass, whatever the order in which workgroups run --
//   SHARED == false (int16 reads on both paths; a POD5 row as a read): byte p / 8 has exactly one writer in the whole launch, the lane
//   whose values begin at p, which stores it plainly, zeros too; the walk reaches the read's last sample, so ceil(T / 8) bytes are
//   written and nothing zeroes the map in front.  The bits of a last byte behind T, and those outside [b + p0, e), are stored as 0.
//   SHARED == true (POD5 reads of several rows, one workgroup per READ walking its rows: svb16_pass_reads): a row that begins at
//   s0 % 8 != 0 makes every lane's bits straddle two bytes, so no lane owns one.  The read's workgroup zeroes the read's map words
//   itself, and behind a barrier the lanes OR their non-zero bits into the words (32-bit atomics: the map begins at a multiple of 4 and
//   is rounded up to 4).  Only that workgroup touches the read's map, so the order of workgroups does not matter here either.
// The emit launch masks the words to the range again, so the up to 3 bytes behind a map's last byte may hold anything.
struct SpanK
{
    uint8_t* map = nullptr;   // the read's
    uint32_t lo = 0, n = 0;   // in: u - lo < n
    uint32_t kx = 0;
    uint32_t pb = 0, pe = 0;  // the positions of the read that can be in: [b + p0, e), pb <= pe
};

// the state of read r (entry i of the call's tables) of samples [rb, re) whose constants are final
__device__ __forceinline__ SpanK span_state(const ReadBatch& b, const SpanOut& so, uint32_t r, uint32_t i, uint32_t rb, uint32_t re)
{
    const NormOut& no = b.sig.norm;
    SpanK k;
    k.map = so.map + so.map_off[i];
    k.kx = b.sig.bias ^ 0x8000u;
    k.pe = re;
    k.pb = so.p0 < re - rb ? rb + so.p0 : re;
    const float2 aw = so.level ? so.level[i] : no.ss[no.map ? no.map[r] : r];
    const double thr = __dadd_rn((double)aw.x, __dmul_rn((double)so.f, (double)aw.y));   // (multiply, then add: no FMA)
    const double h = (so.below ? ceil(thr) : floor(thr) + 1.0) + (double)k.kx;   // the first key not below / above thr (exact where it is not clamped)
    const uint32_t key = h >= 65536.0 ? 0x10000u : (h > 0.0 ? (uint32_t)h : 0u);
    if (thr == thr) {
        k.lo = so.below ? 0u : key;
        k.n = so.below ? key : 0x10000u - key;
    }
    return k;
}

template <bool SHARED>
struct SpanStore
{
    static constexpr uint32_t BYTES = 2;   // (result[] is the int16 decode's)
    SpanK sk;
    uint32_t s0 = 0;   // where the values handed to put() begin in the read (a POD5 read: row by row)
    __device__ __forceinline__ explicit SpanStore(const SpanK& k) : sk(k) {}
    __device__ __forceinline__ void begin_row(uint32_t s) { s0 = s; }
    __device__ __forceinline__ bool aligned() const { return true; }   // (a byte a lane: any position)
    __device__ __forceinline__ void put(uint32_t i0, int valid, uint32_t base, const uint32_t s[8]) const
    {
        if (valid <= 0) return;
        uint32_t bits = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t u = ((base + s[k]) ^ sk.kx) & 0xFFFFu;
            bits |= (u - sk.lo < sk.n ? 1u : 0u) << k;
        }
        const uint32_t p = s0 + i0;   // the position of bit 0 in the read
        uint32_t keep = 0xFFu >> (8 - valid);
        if (p < sk.pb) keep &= sk.pb - p >= 8u ? 0u : 0xFFu << (sk.pb - p);
        if (p + 8u > sk.pe) keep &= sk.pe > p ? 0xFFu >> (8u - (sk.pe - p)) : 0u;
        bits &= keep;
        if constexpr (!SHARED) {
            sk.map[p >> 3] = (uint8_t)bits;   // (p % 8 == 0: the lane's own byte)
        } else if (bits) {
            uint32_t* const w = reinterpret_cast<uint32_t*>(sk.map) + (p >> 5);
            const uint64_t v = (uint64_t)bits << (p & 31u);
            if ((uint32_t)v) atomicOr(w, (uint32_t)v);
            if ((uint32_t)(v >> 32)) atomicOr(w + 1, (uint32_t)(v >> 32));   // (set bits lie in front of pe <= T: inside the map)
        }
    }
    __device__ __forceinline__ void finish() const {}
    __device__ __forceinline__ void done() const {}
};

// The selection and the builder in one: the sink of read r of `count` values for the whole-read and segment kernels' OUT.  | SIG_RANGE (the
// chunk and window sinks and SIG_COUNT): the read is its samples [b, e).  b: the batch, for the typed stores only -- SIG_NONE gets nullptr
// and the batch's fields (a reference to the kernel's ReadBatch argument would cost its loads their scalar form).  cr: whose constants
// (b->sig.cal) the typed store takes -- a POD5 row decoded with its read's
template <int ELEM, int OUT>
__device__ __forceinline__ auto dec_store(uint8_t* dst, const uint64_t* dst_off, const ReadBatch* b, uint32_t r, uint32_t count, uint32_t cr)
{
    static_assert(OUT == SIG_NONE || ELEM == 2, "the typed stores are for int16 samples");
    static_assert(!(OUT & SIG_RANGE) || (OUT & (SIG_CHUNK | SIG_COUNT | SIG_EVENT)) != 0, "ranges: the chunk, window and event sinks and the counting pass");
    static_assert(!(OUT & SIG_TRIM), "the trim sink is built from the read's TrimK");
    static_assert(!(OUT & SIG_EVENT) || (OUT & ~(SIG_EVENT | SIG_RANGE)) == 0, "the event sink stores no sample: no output type");
    if constexpr (OUT == SIG_NONE) return RawStore<ELEM>{ dst + dst_off[r] };
    else if constexpr ((OUT & SIG_EVENT) != 0) {
        uint32_t rb = 0, rend = count;
        if constexpr ((OUT & SIG_RANGE) != 0) sample_range(b->sig, r, count, &rb, &rend);   // the sink's read is the range
        return EventStore{ event_constants(*b, b->sig.wmap ? b->sig.wmap[r] : r, rb, rend) };
    }
    else if constexpr ((OUT & SIG_COUNT) != 0) return CountStore<(OUT & SIG_RANGE) != 0>(b, r, count);
    else if constexpr ((OUT & SIG_CHUNK) == 0) return TypedStore<OUT>{ dst + (dst_off[r] >> 1) * OutBytes<OUT>::value, sig_constants(*b, cr) };
    else {
        uint32_t rb = 0, rend = count;
        if constexpr ((OUT & SIG_RANGE) != 0) sample_range(b->sig, r, count, &rb, &rend);   // the store's read is the range
        if constexpr ((OUT & SIG_WINDOW) != 0) return WindowStore<OUT, false>{ window_constants<OUT>(*b, b->sig.wmap ? b->sig.wmap[r] : r, rb, rend), sig_constants(*b, r), dst };
        else {
            ChunkStore<OUT, false> st;
            st.arena = dst;
            st.ck = chunk_constants<OUT>(*b, rend - rb, b->sig.row[r]);
            st.sk = sig_constants(*b, r);
            st.re = count;
            st.rb = rb;
            st.rend = rend;
            st.pad_elems = (rb & 7u) != 0;
            return st;
        }
    }
}
template <int ELEM, int OUT>
__device__ __forceinline__ auto dec_store(uint8_t* dst, const uint64_t* dst_off, const ReadBatch* b, uint32_t r, uint32_t count) { return dec_store<ELEM, OUT>(dst, dst_off, b, r, count, r); }
template <int ELEM, int OUT>
using DecStore = decltype(dec_store<ELEM, OUT>(nullptr, nullptr, nullptr, 0u, 0u));
}  // namespace
}  // namespace vbzhip
