// svb_kernels.hip -- delta + zig-zag + streamvbyte stage of the VBZ path as HIP kernels for gfx950.
//
// Replaces (reference file:line):
//   StreamVByteWorkerV0<int16_t,true>::compress / ::decompress   vbz/v0/vbz_streamvbyte_impl_sse3.h:406-466, 468-580
//   StreamVByteWorkerV0<T,ZigZag>::compress / ::decompress       vbz/v0/vbz_streamvbyte_impl.h:18-73
//   (dispatch: vbz/v0/vbz_streamvbyte.cpp:20-108, vbz/v1/vbz_streamvbyte.cpp:22-113)
//
// Design (MI355X-first, not a translation of the SSSE3 loop):
//   * one 256-thread workgroup per read; the read is walked in tiles of 256 lanes x VPL values, every
//     lane loading 16 contiguous bytes (global_load_dwordx4, 1 KiB per wave instruction);
//   * the variable-length byte scatter/gather is turned into a prefix sum: per-lane byte counts ->
//     wave scan (cross-lane shuffles) -> workgroup scan through 4 LDS words -> running carry per read;
//   * data bytes are staged through LDS so that HBM only ever sees 16-byte aligned, coalesced
//     dwordx4 stores/loads, whatever the byte alignment of the data section;
//   * the int16 wrap-around delta chain and its inverse (inclusive prefix sum mod 2^16) use the same
//     scan primitives; the previous sample comes from the neighbouring lane by a shuffle.
// Algorithmic HBM bytes per int16 sample: encode 2 read + ~1.26 written; decode the reverse.
#include "svb_store.h"

namespace vbzhip {

namespace {

// ------------------------------------------------------------------------------------------------
// encode
// ------------------------------------------------------------------------------------------------
// Per-read validation shared by the one-workgroup-per-read kernel and the segmented kernels: 0 = go on, or the error.
template <int ELEM, bool I16ZZ>
__device__ __forceinline__ uint32_t svb_encode_check(uint32_t size, uint32_t cap, uint32_t hdr, uint32_t strict_cap)
{
    if (size % ELEM != 0) return E_INPUT_SIZE;  // vbz/v0/vbz_streamvbyte.cpp:28-31
    const uint32_t n = size / ELEM;
    const uint32_t keyLen = (n + 3u) >> 2;
    // the reference requires the destination to hold the worst case (vbz/vbz.cpp:171-174); the
    // library's own scratch slots (strict_cap == 0) are sized for what this kernel can really emit
    const uint64_t worst = (uint64_t)keyLen + ((I16ZZ && !strict_cap) ? 2ull : 4ull) * n + hdr;
    if (worst > cap) return worst > 0xFFFFFFF0ull ? E_INPUT_SIZE : E_DESTINATION_SIZE;
    return 0;
}

// Read r of an encode launch, opened: the gate (read_gate), then the check above.  true: code it -- *e holds its samples, its slot and its
// sizes; false: *verdict is the read's result (GATE_SKIP: none to write).  The three launch shapes (one workgroup per read, segments with
// self-summed prefixes, segments with scan launches) all open a read here.
struct SvbEnc
{
    const uint8_t* in;
    uint8_t* out;   // the read's slot (the sized header's place, when there is one)
    uint32_t size, n, keyLen;
};
template <int ELEM, bool I16ZZ>
__device__ __forceinline__ bool svb_enc_open(const ReadBatch& b, uint32_t r, uint32_t hdr, uint32_t strict_cap, SvbEnc* e, uint32_t* verdict)
{
    *verdict = read_gate(b, r, false);
    if (*verdict) return false;
    e->size = b.src_size[r];
    *verdict = svb_encode_check<ELEM, I16ZZ>(e->size, b.dst_cap[r], hdr, strict_cap);
    if (*verdict) return false;
    e->n = e->size / ELEM;
    e->keyLen = (e->n + 3u) >> 2;
    e->in = b.src + b.src_off[r];
    e->out = b.dst + b.dst_off[r];
    return true;
}

// The result of a read of the large-read path, by one thread, from what svb_enc_open said of it (open, e, verdict) and the data bytes its
// segments counted in all: whether one is to be written, and *res.  A read that is coded also gets its sized header here.
__device__ __forceinline__ bool svb_seg_enc_result(bool open, const SvbEnc& e, uint32_t verdict, uint32_t hdr, uint64_t total, uint32_t* res)
{
    *res = open ? hdr + e.keyLen + (uint32_t)total : verdict;
    if (open && hdr) {
        for (int j = 0; j < 4; ++j) e.out[j] = (uint8_t)(e.size >> (8 * j));
    }
    return open || verdict != GATE_SKIP;
}

// ---- probe for a long repeat distance in the data bytes (consumed by zstd_encode.hip's long-repeat coder) -------------
// libzstd's match finder (on at every level of the reference: vbz/vbz.cpp:194-207) turns signal that cycles a template --
// the reference's own perf generator does, vbz/perf/test_data_generator.h:61-67 -- into a few long matches: the data bytes
// of such a read repeat at ONE distance D.  Finding D must cost a read without one next to nothing, and this kernel has
// every data byte in LDS once anyway.  The sixteen dwords that start at data bytes p0 .. p0 + 15 are the probes; whatever D
// is, exactly one of them comes to lie, D bytes further down, on the first dword of a 16-byte chunk of the flush loop.  So
// the flush looks up the first dword of every chunk it writes in a small hash table (value -> probe number; an empty cell
// holds a value that does not hash to it, so nothing matches it): a multiply, a shift, one LDS read and a compare per 16
// data bytes.  A hit whose 16 bytes equal the 16 bytes behind the probe proposes D = position - (p0 + probe number); the
// smallest proposal is left in hint[r] (0: none), and the entropy stage checks it before it relies on it.
constexpr uint32_t PROBE_TABLE = 512, PROBE_P0 = 256, PROBE_MIN_D = 64, PROBE_TRIES = 4, PROBE_SHIFT = 80;
struct PeriodProbe
{
    uint32_t val[PROBE_TABLE];
    uint8_t idx[PROBE_TABLE];
    uint32_t ctx[12];   // the 32 + 16 data bytes from p0 on (dword k = bytes p0 + 4k ...)
    uint32_t best;      // smallest distance proposed so far
    uint32_t lost;      // table construction: a probe collided
};
__device__ __forceinline__ uint32_t probe_hash(uint32_t w) { return (w * 0x9E3779B1u) >> 23; }

// ---- the data bytes' histogram on the way (CNT; int16 zig-zag reads into library scratch) -------------------------------------------
// The entropy stage builds the data-byte region's Huffman table from a histogram of one kilobyte in four (region_histogram of
// zstd_encode.hip) -- a pass of its own over bytes this kernel has just had in LDS.  Here exactly that sample (the unaligned ends and
// every fourth stripe of 64 aligned 16-byte chunks; everything, in two parts, for reads so short that the region may have to be counted
// exactly) is counted by LDS atomics while the bytes are flushed, and left in the read's plan (EncPlan::hist_mode): the same counts, so
// the frames are byte for byte what they were, and the entropy stage's planning never reads the data bytes.
// Round 5 also moved the control bytes' TOKENISER in here, twice -- every wavefront deciding its own 128 control bytes per tile with
// wave-uniform scalar arithmetic (a CU has ONE scalar unit: 2.3 x the kernel's time), then tokenise_runs' own arithmetic as "trips" of
// one wavefront over an LDS ring of control bytes (bit-exact, and + 45 % on this kernel for - 11 % on the planning launch: a trip's
// latency, ~5 000 cycles, sits on the workgroup's barrier-synchronised critical path) -- and took it out again: profiles/r05_experiments.md.
constexpr uint32_t CNT_MIN_VALUES = 1640;            // n + ceil(n / 4) >= 2048: the entropy stage then cuts the stream into its two regions
constexpr uint32_t CNT_HIST_SAMPLE_FROM = 32u << 10; // region_histogram samples regions of this size and more (HIST_SAMPLE_FROM)

struct CntLds
{
    uint32_t hA[4][256];      // data bytes of the sample, one copy per wavefront (atomics on a shared bin serialise)
    uint32_t hB[256];         // the other data bytes (hist_mode 2)
};

__device__ __forceinline__ void cnt_count16(uint32_t* h, const uint4& v)
{
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(&h[(w[k] >> (8 * j)) & 0xFFu], 1u);
    }
}

// ---- pairs of whole int16 zig-zag tiles (round 6) --------------------------------------------------------------------------------------
// The tile loop of svb_encode_range issues ~185 wave-level VALU instructions per 512 samples of a wavefront, most of them the 4-cycle
// kind (tools/valu_rate.hip: compares, selects, v_bfe, DPP), and four workgroup barriers per tile: the kernel sat on instruction issue
// at 4.6 ms per 65 536 reads where its 21.4 GB would take 3.5 at a copy's rate.  Whole tiles of int16 samples -- all but the ends of a
// read -- now go through this loop, two tiles (4096 samples) per trip:
//   * the samples stay PACKED (two per register) from the load to the byte stores: delta and zig-zag as before (v_pk_*), then the eight
//     high bytes of a lane's values are gathered into two registers (v_perm_b32) and "is this byte non-zero" is byte-parallel
//     arithmetic on four values at once -- (((h & 0x7f7f7f7f) + 0x7f7f7f7f) | h) & 0x80808080 --; one multiplication turns the four
//     flags into the key byte (bits 0, 2, 4, 6), another into their prefix sums (a byte each: where each value's bytes go, and the
//     lane's byte count), instead of eight compares and a dozen selects;
//   * ONE workgroup scan for both tiles: their byte counts ride in the two halves of one register (a tile has at most 4096 bytes);
//   * byte emission as before (two ds_write_b8 per value, a one-byte value's zero high byte overwritten by the next value's low byte),
//     but straight from the packed registers (ds_write_b8_d16_hi for the odd values) at offsets cut out of the prefix-sum register;
//   * two stage buffers used in turn, so that the bytes that do not fill a 16-byte chunk move to the OTHER buffer while this one is
//     being flushed: two barriers per trip (eight before, for two tiles), and every thread of the workgroup has a chunk to flush.
// Same bytes, same probe and histogram hand-over (the flush is the old one); tests/test_gpu_parity.py holds both to the oracle.
template <bool PROBE, bool CNT>
struct I16Pairs
{
    // one stage buffer: the kept bytes + two tiles at 3/2 bytes per value (signal: 1.01; all of 2 would be 8 KB, and a workgroup's LDS
    // decides how many of them a CU holds).  A pair that does not fit ends the loop: the tile loop of svb_encode_range codes the rest.
#ifndef VBZ_ENC_BUF_BYTES
#define VBZ_ENC_BUF_BYTES (2 * WG * 8 * 3 / 2 + 32)
#endif
    static constexpr uint32_t TILE = WG * 8, BUF = VBZ_ENC_BUF_BYTES;
    const uint8_t* in;
    uint8_t* keys;
    uint8_t* gal;
    uint8_t* stage;      // two buffers of BUF bytes; [0] is the one the caller's own loop uses
    uint32_t* wsum;      // 8 words
    uint16_t* kb16;      // 2 x 512 halfwords: the control bytes of a pair on their way out (two sets used in turn)
    PeriodProbe* pp;
    CntLds* CL;
    uint32_t A, hmode;
    bool cnt_on;
    uint32_t probe_p0;

    // zig-zag of the wrap-around deltas of a lane's eight samples, packed (sse3.h:432-440); pw's top half = the sample in front
    static __device__ __forceinline__ void zz4(const uint4& q, uint32_t pw, uint32_t Z[4])
    {
        typedef short s16x2 __attribute__((ext_vector_type(2)));
        const uint32_t w[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t prevw = __builtin_amdgcn_alignbit(w[k], k ? w[k - 1] : pw, 16);
            const s16x2 d = __builtin_bit_cast(s16x2, w[k]) - __builtin_bit_cast(s16x2, prevw);
            Z[k] = __builtin_bit_cast(uint32_t, (s16x2)((d << (s16x2)1) ^ (d >> (s16x2)15)));
        }
    }
    // flags (bit 0 of every byte) "value j of four needs two bytes", from the packed values Za (values 0, 1) and Zb (values 2, 3)
    static __device__ __forceinline__ uint32_t flags4(uint32_t Za, uint32_t Zb)
    {
        const uint32_t h = __builtin_amdgcn_perm(Zb, Za, 0x07050301u);   // the four high bytes
        return ((((h & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | h) & 0x80808080u) >> 7;
    }
    // a lane's 8 .. 16 data bytes at s (LDS): both bytes of every value are written, a one-byte value's zero high byte is overwritten by
    // the next value's low byte (a later instruction of this lane); only the lane's LAST value must not touch the byte behind it
    static __device__ __forceinline__ void emit8(uint8_t* s, const uint32_t Z[4], uint32_t ps0, uint32_t ps1)
    {
        const uint32_t Y0 = Z[0] >> 8, Y1 = Z[1] >> 8, Y2 = Z[2] >> 8, Y3 = Z[3] >> 8;
        s[1] = (uint8_t)Y0;
        uint8_t* t = s + (ps0 & 0xFFu);
        t[1] = (uint8_t)(Z[0] >> 16);
        s[0] = (uint8_t)Z[0];   // (behind a store that may alias s[1]: the two are not to be fused into one unaligned 16-bit store, which is slow)
        t[2] = (uint8_t)(Y0 >> 16);
        t = s + ((ps0 >> 8) & 0xFFu);
        t[2] = (uint8_t)Z[1];
        t[3] = (uint8_t)Y1;
        t = s + ((ps0 >> 16) & 0xFFu);
        t[3] = (uint8_t)(Z[1] >> 16);
        t[4] = (uint8_t)(Y1 >> 16);
        uint8_t* const s4 = s + (ps0 >> 24);
        s4[4] = (uint8_t)Z[2];
        s4[5] = (uint8_t)Y2;
        t = s4 + (ps1 & 0xFFu);
        t[5] = (uint8_t)(Z[2] >> 16);
        t[6] = (uint8_t)(Y2 >> 16);
        t = s4 + ((ps1 >> 8) & 0xFFu);
        t[6] = (uint8_t)Z[3];
        t[7] = (uint8_t)Y3;
        t = s4 + ((ps1 >> 16) & 0xFFu);
        t[7] = (uint8_t)(Z[3] >> 16);
        if (Z[3] >> 24) t[8] = (uint8_t)(Y3 >> 16);
    }

    // one 16-byte chunk of the stage leaves for gal + F + 16 c (the flush of svb_encode_range, chunk by chunk)
    __device__ __forceinline__ void flush_chunk(const uint8_t* buf, uint64_t F, uint32_t c, int wv)
    {
        uint8_t* g = gal + F + 16ull * c;
        if (F == 0 && c == 0 && A != 0) {
            for (uint32_t j = A; j < 16; ++j) g[j] = buf[j];
            if (CNT && cnt_on)
                for (uint32_t j = A; j < 16; ++j) atomicAdd(&CL->hA[wv][buf[j]], 1u);
            return;
        }
        const uint4 v = *reinterpret_cast<const uint4*>(buf + 16u * c);
        *reinterpret_cast<uint4*>(g) = v;
        if (CNT && cnt_on) {
            const uint32_t cq = (uint32_t)(F >> 4) + c - (A ? 1u : 0u);
            if (((cq >> 6) & 3u) == 0u) cnt_count16(CL->hA[wv], v);
            else if (hmode == 2u) cnt_count16(CL->hB, v);
        }
        if (PROBE && probe_p0) {
            const uint32_t h = probe_hash(v.x);
            if (pp->val[h] == v.x) {
                const uint64_t rel = F + 16ull * c - A;
                const uint32_t j = pp->idx[h], k = j >> 2, sh = j & 3u;
                const uint32_t c0 = __builtin_amdgcn_alignbyte(pp->ctx[k + 1], pp->ctx[k], sh), c1 = __builtin_amdgcn_alignbyte(pp->ctx[k + 2], pp->ctx[k + 1], sh);
                const uint32_t c2 = __builtin_amdgcn_alignbyte(pp->ctx[k + 3], pp->ctx[k + 2], sh), c3 = __builtin_amdgcn_alignbyte(pp->ctx[k + 4], pp->ctx[k + 3], sh);
                if (rel >= (uint64_t)probe_p0 + j + PROBE_MIN_D && rel < 0xFFFFFFFFull && c0 == v.x && c1 == v.y && c2 == v.z && c3 == v.w)
                    atomicMin(&pp->best, (uint32_t)rel - (probe_p0 + j));
            }
        }
    }

    // tiles t0, t0 + TILE, ... while two whole ones are left; the bytes [F, P) the caller holds at the head of stage buffer 0 are
    // taken over and handed back the same way.  Returns the first value not coded.  All 256 threads; the caller's next barrier
    // orders the last LDS writes.
    static __device__ __forceinline__ uint64_t uniform64(uint64_t v)
    {
        return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) | ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
    }
    __device__ __forceinline__ uint32_t run(uint32_t t0_in, uint32_t end_in, uint64_t& F_io, uint64_t& P_io)
    {
        const int tid = threadIdx.x, lane = tid & 63;
        // workgroup-uniform state, held in scalar registers
        uint32_t t0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)t0_in);
        const uint32_t end = (uint32_t)__builtin_amdgcn_readfirstlane((int)end_in);
        uint64_t F = uniform64(F_io), P = uniform64(P_io);
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        const uint32_t m0 = wv > 0 ? 0xFFFFFFFFu : 0u, m1 = wv > 1 ? 0xFFFFFFFFu : 0u, m2 = wv > 2 ? 0xFFFFFFFFu : 0u;
        uint32_t cur = 0;   // the stage buffer this trip writes
        const uint8_t* ip = in + ((size_t)t0 + (size_t)tid * 8) * 2;
        uint8_t* kp0 = keys + (t0 >> 2);   // the pair's control bytes: 1 KB from here
        // lane 0 of a wavefront: the aligned dword in front of its samples -- its top half is the sample in front (samples start 16-byte
        // aligned here, and the read's very first value has nothing in front of it)
        auto prev_of = [&](const uint8_t* p, bool first_value) -> uint32_t {
            return (lane == 0 && !first_value) ? *reinterpret_cast<const uint32_t*>(p - 4) : 0u;
        };
        uint4 na = *reinterpret_cast<const uint4*>(ip), nb = *reinterpret_cast<const uint4*>(ip + TILE * 2);
        uint32_t npa = prev_of(ip, t0 == 0 && tid == 0), npb = prev_of(ip + TILE * 2, false);
        uint32_t par = 0;
        while (end - t0 >= 2u * TILE) {
            const uint4 qa = na, qb = nb;
            const uint32_t pa = npa, pb = npb;
            if (end - t0 >= 4u * TILE) {   // the next pair's samples are requested a trip ahead
                na = *reinterpret_cast<const uint4*>(ip + TILE * 4);
                nb = *reinterpret_cast<const uint4*>(ip + TILE * 6);
                npa = prev_of(ip + TILE * 4, false);
                npb = prev_of(ip + TILE * 6, false);
            }
            uint32_t ZA[4], ZB[4];
            {
                uint32_t pw = wave_prev_lane_u32(qa.w);
                if (lane == 0) pw = pa;
                zz4(qa, pw, ZA);
                pw = wave_prev_lane_u32(qb.w);
                if (lane == 0) pw = pb;
                zz4(qb, pw, ZB);
            }
            const uint32_t fa0 = flags4(ZA[0], ZA[1]), fa1 = flags4(ZA[2], ZA[3]), fb0 = flags4(ZB[0], ZB[1]), fb1 = flags4(ZB[2], ZB[3]);
            // key bytes: flag j of four to bit 2 j (codes 0 / 1 only); prefix sums of the flags, a byte each
            const uint32_t ka = ((fa0 * 0x01041040u) >> 24) | (((fa1 * 0x01041040u) >> 24) << 8);
            const uint32_t kb = ((fb0 * 0x01041040u) >> 24) | (((fb1 * 0x01041040u) >> 24) << 8);
            const uint32_t pa0 = fa0 * 0x01010101u, pa1 = fa1 * 0x01010101u, pb0 = fb0 * 0x01010101u, pb1 = fb1 * 0x01010101u;
            // control bytes: a lane's two bytes per tile go to LDS, and behind the barrier ONE wavefront stores the pair's kilobyte of them
            // as 16 bytes per lane (two 2-byte stores per lane of every wavefront measured 0.36 ms of the kernel's 4.2: 1.6 GB in 128-byte
            // requests)
            kb16[par * 128 + (uint32_t)tid] = (uint16_t)ka;
            kb16[par * 128 + 256u + (uint32_t)tid] = (uint16_t)kb;
            // one scan for both tiles: tile A's byte count in the low half, tile B's in the high half
            const uint32_t L = (8u + (pa0 >> 24) + (pa1 >> 24)) | ((8u + (pb0 >> 24) + (pb1 >> 24)) << 16);
            const uint32_t inc = wave_incl_scan_u32(L);
            uint32_t* ws = wsum + par;
            if (lane == 63) ws[wv] = inc;
            wg_lds_barrier();   // (also: the previous trip's kept bytes stand in this trip's buffer, its flush has read the other one)
            if (tid < 64) {
                const uint4 kv = *reinterpret_cast<const uint4*>(kb16 + par * 128 + 8u * (uint32_t)tid);
                __builtin_memcpy(kp0 + 16u * (uint32_t)tid, &kv, 16);
            }
            const uint4 s4 = *reinterpret_cast<const uint4*>(ws);
            const uint32_t tot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(s4.x + s4.y + s4.z + s4.w));
            const uint32_t ex = (s4.x & m0) + (s4.y & m1) + (s4.z & m2) + inc - L;
            const uint32_t R = (uint32_t)(P - F), totA = tot & 0xFFFFu, totB = tot >> 16;
            if (R + totA + totB + 1u > BUF) break;   // (workgroup-uniform; nothing of this pair is in the stage -- its control bytes are written again)
            uint8_t* const buf = stage + cur * BUF;
            emit8(buf + R + (ex & 0xFFFFu), ZA, pa0, pa1);
            emit8(buf + R + totA + (ex >> 16), ZB, pb0, pb1);
            wg_lds_barrier();
            const uint32_t endidx = R + totA + totB, nch = endidx >> 4, rem = endidx & 15u;
            if ((uint32_t)tid < nch) flush_chunk(buf, F, (uint32_t)tid, wv);
            if ((uint32_t)tid + WG < nch) flush_chunk(buf, F, (uint32_t)tid + WG, wv);
            if ((uint32_t)tid + 2 * WG < nch) flush_chunk(buf, F, (uint32_t)tid + 2 * WG, wv);   // (only when most values take two bytes)
            if ((uint32_t)tid < rem) stage[(cur ^ 1u) * BUF + tid] = buf[16u * nch + tid];   // the bytes short of a chunk: to the other buffer
            F += 16ull * nch;
            P += totA + totB;
            cur ^= 1u;
            par ^= 4u;
            t0 += 2u * TILE;
            ip += TILE * 4;
            kp0 += TILE / 2;
        }
        wg_lds_barrier();   // the last flush has read its buffer, the kept bytes stand in stage[cur]
        if (cur != 0) {
            if ((uint32_t)tid < (uint32_t)(P - F)) stage[tid] = stage[BUF + tid];
        }
        F_io = F;
        P_io = P;
        return t0;
    }
};

// Values [first, end) of a read of n values (first a multiple of the tile size): control bytes to keys[first/4 ...),
// data bytes to data[0 ...) -- `data` is where this range's data bytes start, any alignment; only bytes of the range
// are touched.  COUNT_ONLY: nothing is written, the data byte count is all that is wanted.  Returns the data bytes
// (workgroup-uniform).  All 256 threads.
// PROBE (one-workgroup-per-read kernel only, data starts at first == 0): see PeriodProbe; *hint_out gets the distance.
// CNT (one-workgroup-per-read kernel, first == 0): hmode != 0 = the data bytes' sample is counted on the way into *CL (see CntLds;
// hmode: EncPlan::hist_mode).
template <int ELEM, bool ZZ, bool I16ZZ, bool COUNT_ONLY, bool PROBE = false, bool CNT = false>
__device__ __forceinline__ uint64_t svb_encode_range(const uint8_t* in, uint32_t first, uint32_t end, uint8_t* keys, uint8_t* data,
                                                     uint8_t* stage, uint32_t* wsum, PeriodProbe* pp = nullptr, uint32_t* hint_out = nullptr,
                                                     CntLds* CL = nullptr, uint32_t hmode = 0)
{
    constexpr int VPL = Vpl<ELEM>::value;
    constexpr int TILE = WG * VPL;
    static_assert(!CNT || !COUNT_ONLY, "counting rides on the flush");
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const bool cnt_on = CNT && hmode != 0;      // the data bytes' sample is counted on the way
    (void)wv;
    const uint32_t A = (uint32_t)((uintptr_t)data & 15u);
    uint8_t* gal = data - A;  // 16-byte aligned address space of the data section
    const bool in_aligned = (((uintptr_t)in) & 15u) == 0;

    uint64_t F = 0;  // bytes of the aligned space already flushed (multiple of 16)
    uint64_t P = A;  // next byte position in the aligned space; stage[] holds [F, P)
    uint32_t probe_p0 = 0;   // != 0: the probe table stands, with its probes at data bytes probe_p0 ...
    bool probe_runs = false; // the probes could not be placed: the distance 1 ("a run") is proposed (zstd_encode.hip: RUN_D)
    if (PROBE) {
        for (uint32_t i = tid; i < PROBE_TABLE; i += WG) pp->val[i] = i == 0 ? 1u : 0u;   // hash(0) = 0, hash(1) != 0
        if (tid == 0) {
            pp->best = 0xFFFFFFFFu;
            pp->lost = 0;
        }
        // (the scan of the first tile holds the barrier that orders these writes)
    }

    // the next tile's 16 bytes per lane are requested before this tile is processed (one load always in flight)
    uint4 qnext = make_uint4(0u, 0u, 0u, 0u);
    {
        const uint32_t i0 = first + (uint32_t)tid * VPL;
        if (in_aligned && i0 < end && end - i0 >= (uint32_t)VPL) qnext = *reinterpret_cast<const uint4*>(in + (size_t)i0 * ELEM);
    }
    constexpr bool FAST = I16ZZ && !COUNT_ONLY;   // pairs of whole int16 tiles take svb_i16zz_pairs (below)
    bool fast_done = !FAST || !in_aligned;
    for (uint32_t t0 = first; t0 < end; t0 += TILE) {
        if (FAST && !fast_done && (!PROBE || t0 != first)) {
            // (with PROBE the read's first tile goes through the loop below, which builds the probe table from it)
            fast_done = true;
            if (end - t0 >= 2u * (uint32_t)TILE) {
                I16Pairs<PROBE, CNT> fp = { in, keys, gal, stage, wsum, reinterpret_cast<uint16_t*>(stage + 2 * I16Pairs<PROBE, CNT>::BUF), pp, CL, A, hmode, cnt_on, probe_p0 };
                t0 = fp.run(t0, end, F, P);
                if (t0 >= end) break;
                const uint32_t i0 = t0 + (uint32_t)tid * VPL;
                qnext = make_uint4(0u, 0u, 0u, 0u);
                if (i0 < end && end - i0 >= (uint32_t)VPL) qnext = *reinterpret_cast<const uint4*>(in + (size_t)i0 * ELEM);
            }
        }
        const uint32_t i0 = t0 + (uint32_t)tid * VPL;
        const int valid = i0 >= end ? 0 : (end - i0 >= (uint32_t)VPL ? VPL : (int)(end - i0));
        const bool full = in_aligned && end - t0 >= (uint32_t)TILE;
        const uint4 q = qnext;
        {
            const uint32_t i1 = i0 + TILE;
            if (in_aligned && i1 < end && end - i1 >= (uint32_t)VPL) qnext = *reinterpret_cast<const uint4*>(in + (size_t)i1 * ELEM);
        }
        uint32_t u[VPL];
        if (I16ZZ && full) {
            // full int16 tile: wrap-around delta and 16-bit zig-zag (sse3.h:432-440) on two samples per instruction
            typedef short s16x2 __attribute__((ext_vector_type(2)));
            const uint32_t w[4] = { q.x, q.y, q.z, q.w };
            uint32_t pw = wave_prev_lane_u32(w[3]);  // its top half: the sample in front of this lane's first
            if (lane == 0) pw = i0 == 0 ? 0u : ((uint32_t)(uint16_t)load_elem(in + (size_t)(i0 - 1) * ELEM, ELEM) << 16);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t prevw = __builtin_amdgcn_alignbit(w[k], k ? w[k - 1] : pw, 16);
                const s16x2 d = __builtin_bit_cast(s16x2, w[k]) - __builtin_bit_cast(s16x2, prevw);
                const uint32_t zz = __builtin_bit_cast(uint32_t, (s16x2)((d << (s16x2)1) ^ (d >> (s16x2)15)));
                u[(2 * k) % VPL] = zz & 0xFFFFu;
                u[(2 * k + 1) % VPL] = zz >> 16;
            }
        } else {
        int32_t x[VPL];
        if (valid == VPL && in_aligned) {
            const uint32_t w[4] = { q.x, q.y, q.z, q.w };
            if (ELEM == 4) {
#pragma unroll
                for (int k = 0; k < VPL; ++k) x[k] = (int32_t)w[k & 3];
            } else if (ELEM == 2) {
#pragma unroll
                for (int k = 0; k < VPL; ++k) x[k] = (int16_t)(w[(k >> 1) & 3] >> (16 * (k & 1)));
            } else {
#pragma unroll
                for (int k = 0; k < VPL; ++k) x[k] = (int8_t)(w[(k >> 2) & 3] >> (8 * (k & 3)));
            }
        } else {
#pragma unroll
            for (int k = 0; k < VPL; ++k) x[k] = k < valid ? load_elem(in + (size_t)(i0 + k) * ELEM, ELEM) : 0;
        }
        if (ZZ) {
            // previous sample: neighbouring lane's last value; wave lane 0 re-reads it from memory
            int32_t prev = (int32_t)wave_prev_lane_u32((uint32_t)x[VPL - 1]);
            if (lane == 0) prev = (i0 == 0 || valid == 0) ? 0 : load_elem(in + (size_t)(i0 - 1) * ELEM, ELEM);
#pragma unroll
            for (int k = 0; k < VPL; ++k) {
                if (I16ZZ) {
                    // wrap-around int16 delta, 16-bit zig-zag (sse3.h:432-440)
                    uint32_t d = ((uint32_t)x[k] - (uint32_t)prev) & 0xFFFFu;
                    u[k] = ((d << 1) ^ (0u - (d >> 15))) & 0xFFFFu;
                } else {
                    uint32_t d = (uint32_t)x[k] - (uint32_t)prev;  // streamvbyte zigzag_delta_encode
                    u[k] = (d << 1) ^ (uint32_t)((int32_t)d >> 31);
                }
                prev = x[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < VPL; ++k) u[k] = (uint32_t)x[k];
        }
        }
        uint32_t keybits = 0, L = 0;
        if (I16ZZ && full) {  // full tile of one- or two-byte values
#pragma unroll
            for (int k = 0; k < VPL; ++k) {
                const uint32_t code = u[k] >> 8 ? 1u : 0u;
                keybits |= code << (2 * k);
                L += code;
            }
            L += VPL;
            if (!COUNT_ONLY) {
                const uint16_t kk = (uint16_t)keybits;
                __builtin_memcpy(keys + (i0 >> 2), &kk, 2);
            }
        } else {
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            uint32_t code = (u[k] > 0xFFu) + (u[k] > 0xFFFFu) + (u[k] > 0xFFFFFFu);
            if (k < valid) {
                keybits |= code << (2 * k);
                L += code + 1;
            }
        }
        }
        // control bytes: VPL/4 per lane, contiguous across the wave
        if (!COUNT_ONLY && !(I16ZZ && full) && valid > 0) {
            uint8_t* kp = keys + (i0 >> 2);
            if (VPL == 8 && valid > 4) {
                uint16_t kk = (uint16_t)keybits;
                __builtin_memcpy(kp, &kk, 2);
            } else {
                kp[0] = (uint8_t)keybits;
            }
        }
        uint32_t tot;
        const uint32_t ex = block_excl_scan_u32(L, wsum, tot);
        if (COUNT_ONLY) {
            P += tot;
            continue;
        }
        uint32_t o = (uint32_t)(P - F) + ex;
        if (I16ZZ && full) {
            // full tile, one or two bytes per value: both bytes are always written and a one-byte value's second
            // byte is overwritten by the lane's next value (a later instruction) -- no branches; only the lane's
            // last value must not touch the next lane's first byte
#pragma unroll
            for (int k = 0; k < VPL - 1; ++k) {
                stage[o] = (uint8_t)u[k];
                stage[o + 1] = (uint8_t)(u[k] >> 8);
                o += 1u + (u[k] > 0xFFu ? 1u : 0u);
            }
            stage[o] = (uint8_t)u[VPL - 1];
            if (u[VPL - 1] > 0xFFu) stage[o + 1] = (uint8_t)(u[VPL - 1] >> 8);
        } else {
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            if (k < valid) {
                uint32_t v = u[k];
                stage[o++] = (uint8_t)v;
                if (v > 0xFFu) stage[o++] = (uint8_t)(v >> 8);
                if (!I16ZZ) {
                    if (v > 0xFFFFu) stage[o++] = (uint8_t)(v >> 16);
                    if (v > 0xFFFFFFu) stage[o++] = (uint8_t)(v >> 24);
                }
            }
        }
        }
        wg_lds_barrier();
        const uint32_t endidx = (uint32_t)(P - F) + tot;
        const uint32_t nch = endidx >> 4;
        if (PROBE && t0 == 0 && endidx >= A + PROBE_P0 + PROBE_TRIES * PROBE_SHIFT + 48u) {
            // the first tile holds the probes: sixteen distinct dwords in sixteen different cells, else another place
            uint32_t p0 = PROBE_P0;
            for (uint32_t attempt = 0; attempt < PROBE_TRIES; ++attempt, p0 += PROBE_SHIFT) {
                uint32_t pw = 0, h = 0;
                if (tid < 16) {
                    const uint8_t* q = stage + A + p0 + tid;
                    pw = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
                    h = probe_hash(pw);
                    pp->val[h] = pw;
                    pp->idx[h] = (uint8_t)tid;
                }
                wg_lds_barrier();
                if (tid < 16 && (pp->val[h] != pw || pp->idx[h] != (uint8_t)tid)) pp->lost = 1;   // two probes in one cell (or equal)
                wg_lds_barrier();
                const bool lost = pp->lost != 0;
                wg_lds_barrier();
                if (!lost) {
                    probe_p0 = p0;
                    break;
                }
                if (tid < 16) pp->val[h] = h == 0 ? 1u : 0u;
                if (tid == 0) pp->lost = 0;
                wg_lds_barrier();
            }
            if (!probe_p0) probe_runs = true;   // (no sixteen distinct dwords at any of the places tried: bytes that are all alike -- a run is proposed)
            if (probe_p0 && tid < 12) {
                const uint8_t* q = stage + A + probe_p0 + 4 * tid;
                pp->ctx[tid] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
            }
            wg_lds_barrier();
        }
        for (uint32_t c = tid; c < nch; c += WG) {
            uint8_t* g = gal + F + 16ull * c;
            if (F == 0 && c == 0 && A != 0) {
                for (uint32_t j = A; j < 16; ++j) g[j] = stage[j];
                if (CNT && cnt_on)   // the unaligned head of the data bytes is part of the sample
                    for (uint32_t j = A; j < 16; ++j) atomicAdd(&CL->hA[wv][stage[j]], 1u);
            } else {
                const uint4 v = *reinterpret_cast<const uint4*>(stage + 16u * c);
                *reinterpret_cast<uint4*>(g) = v;
                if (CNT && cnt_on) {
                    // region_histogram's sample: 16-byte chunks are numbered from the first aligned one, 64 of them are a stripe, every
                    // fourth stripe is counted (hist_mode 2: the others too, apart)
                    const uint32_t cq = (uint32_t)(F >> 4) + c - (A ? 1u : 0u);
                    if (((cq >> 6) & 3u) == 0u) cnt_count16(CL->hA[wv], v);
                    else if (hmode == 2u) cnt_count16(CL->hB, v);
                }
                if (PROBE && probe_p0) {
                    const uint32_t h = probe_hash(v.x);
                    if (pp->val[h] == v.x) {   // rare: compare the chunk with the 16 bytes behind that probe
                        const uint64_t rel = F + 16ull * c - A;   // data byte of the chunk's first byte
                        const uint32_t j = pp->idx[h], k = j >> 2, sh = j & 3u;
                        const uint32_t c0 = __builtin_amdgcn_alignbyte(pp->ctx[k + 1], pp->ctx[k], sh), c1 = __builtin_amdgcn_alignbyte(pp->ctx[k + 2], pp->ctx[k + 1], sh);
                        const uint32_t c2 = __builtin_amdgcn_alignbyte(pp->ctx[k + 3], pp->ctx[k + 2], sh), c3 = __builtin_amdgcn_alignbyte(pp->ctx[k + 4], pp->ctx[k + 3], sh);
                        if (rel >= (uint64_t)probe_p0 + j + PROBE_MIN_D && rel < 0xFFFFFFFFull && c0 == v.x && c1 == v.y && c2 == v.z && c3 == v.w)
                            atomicMin(&pp->best, (uint32_t)rel - (probe_p0 + j));
                    }
                }
            }
        }
        const uint32_t rem = endidx & 15u;
        uint8_t keep = 0;
        if ((uint32_t)tid < rem) keep = stage[16u * nch + tid];
        wg_lds_barrier();
        if (nch > 0 && (uint32_t)tid < rem) stage[tid] = keep;
        F += 16ull * nch;
        P += tot;
        // the scan at the top of the next tile contains the barrier that orders these LDS writes
    }
    if (COUNT_ONLY) return P - A;
    wg_lds_barrier();
    if (PROBE && tid == 0) *hint_out = pp->best == 0xFFFFFFFFu ? (probe_runs ? 1u : 0u) : pp->best;
    {   // tail: bytes [F, P) still in LDS
        const uint32_t rem = (uint32_t)(P - F);
        const uint32_t lo = (F == 0) ? A : 0u;
        if ((uint32_t)tid >= lo && (uint32_t)tid < rem) {
            gal[F + tid] = stage[tid];
            if (CNT && cnt_on) atomicAdd(&CL->hA[0][stage[tid]], 1u);   // (the unaligned end: part of the sample too)
        }
    }
    return P - A;
}

template <int ELEM, bool I16ZZ>
struct EncStage
{
    // (int16 zig-zag: the two buffers of I16Pairs; the tile loop of svb_encode_range uses the head of the first, one tile's worst case)
    static constexpr int value = I16ZZ ? 2 * (int)I16Pairs<false, false>::BUF + 2048 : WG * Vpl<ELEM>::value * 4 + 32;   // (+ the control bytes' 2 x 1 KB)
};

template <bool CNT> struct CntLdsOf { typedef CntLds type; };
template <> struct CntLdsOf<false> { struct type { uint32_t none; }; };

#ifndef VBZ_SVBENC_WAVES
#define VBZ_SVBENC_WAVES 1
#endif
template <int ELEM, bool ZZ, bool I16ZZ, bool PROBE, bool CNT = false>
__global__ __launch_bounds__(WG, VBZ_SVBENC_WAVES) void svb_encode_kernel(ReadBatch b, uint32_t hdr, uint32_t strict_cap, uint32_t* period_hint, EncPlan* pre)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[EncStage<ELEM, I16ZZ>::value];
    __shared__ __attribute__((aligned(16))) uint32_t wsum[8];   // (I16Pairs uses two sets of four in turn)
    __shared__ PeriodProbe probe;   // (only the PROBE instantiations refer to it)
    __shared__ __attribute__((aligned(16))) typename CntLdsOf<CNT>::type cntl[1];   // (only the CNT instantiations have one)

    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x;
    if (PROBE && tid == 0) period_hint[r] = 0;
    if (CNT && tid == 0) pre[r].hist_mode = 0;   // whatever becomes of the read, the entropy stage finds a verdict of this launch in its plan
    SvbEnc e;
    uint32_t verdict;
    if (!svb_enc_open<ELEM, I16ZZ>(b, r, hdr, strict_cap, &e, &verdict)) return read_closed(b, r, verdict);
    const uint32_t n = e.n, keyLen = e.keyLen;
    const uint8_t* in = e.in;
    uint8_t* out = e.out;
    if (hdr) {
        if (tid < 4) out[tid] = (uint8_t)(e.size >> (8 * tid));
        out += 4;
    }
    CntLds* const CL = reinterpret_cast<CntLds*>(&cntl[0]);
    uint32_t hmode = 0;
    if (CNT && hdr == 0 && n >= CNT_MIN_VALUES) {
        // (a read of fewer values may give a stream the entropy stage does not cut into regions; a read of 32 K values and more has a
        // data-byte region that is always sampled first: the other bytes are then not counted here -- if the sample turns out not to
        // show enough byte values, the entropy stage counts the region itself)
        hmode = n >= CNT_HIST_SAMPLE_FROM ? 1u : 2u;
        uint32_t* z = &CL->hA[0][0];   // hA and hB are contiguous
        for (uint32_t i = tid; i < 5u * 256u; i += WG) z[i] = 0;
        // (the scan of the first tile holds the barrier that orders these writes)
    }
    const uint64_t bytes = svb_encode_range<ELEM, ZZ, I16ZZ, false, PROBE, CNT>(in, 0, n, out, out + keyLen, stage, wsum, PROBE ? &probe : nullptr,
                                                                                PROBE ? period_hint + r : nullptr, CL, hmode);
    if (tid == 0) b.result[r] = hdr + keyLen + (uint32_t)bytes;
    if (CNT && hmode) {
        wg_lds_barrier();   // the tail's atomics
        EncPlan* P = pre + r;
        P->reg[1].ctable[tid] = CL->hA[0][tid] + CL->hA[1][tid] + CL->hA[2][tid] + CL->hA[3][tid];
        if (hmode == 2u) P->histB[tid] = CL->hB[tid];
        if (tid == 0) P->hist_mode = hmode;
    }
}

// ---- one read on many workgroups ("segments"): for batches of few, large reads --------------------------------------
// A segment is SEG_TILES tiles of values.  seg_first[r] (exclusive scan of the reads' segment counts, seg_first[n_reads] =
// total) maps a workgroup to its (read, segment).  Pass 1 counts the data bytes of every segment, a scan turns the
// counts into data offsets (and gives the read's result), pass 2 encodes every segment at its offset.
constexpr int SEG_TILES = 8;

__device__ __forceinline__ bool seg_locate(const uint32_t* seg_first, uint32_t n_reads, uint32_t g, uint32_t& r, uint32_t& k)
{
    if (g >= seg_first[n_reads]) return false;
    uint32_t lo = 0, hi = n_reads;  // the last read with seg_first[r] <= g
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg_first[mid] <= g) lo = mid; else hi = mid;
    }
    r = lo;
    k = g - seg_first[lo];
    return true;
}

// SELF (calls whose segment tables are small: self_max): no scan launch between the passes -- a workgroup adds up what the segments
// of its read in front of it have announced by itself (a few loads per thread, the values sit in the L2), and a read's first
// workgroup does what the scan kernel's first thread does (the read's result).  A call of few reads is a chain of short dependent
// launches: each one saved is 4.5 us.  The loads grow with the square of the table (1024 segments: 4 MB out of the L2 per pass).
// The bound is the caller's (self_max of the launchers: SVB_SEG_SELF_MAX in vbz_kernels.h, or what the context read from
// VBZ_HIP_SEG_SELF_MAX when it was created; 0: always the scan launches).

// all 256 threads: { sum of arr[lo .. mid), sum of arr[lo .. hi) }, lo <= mid <= hi
__device__ __forceinline__ void seg_sums(const uint32_t* arr, uint32_t lo, uint32_t mid, uint32_t hi, uint64_t* sums_s, uint64_t& before, uint64_t& total)
{
    uint64_t a = 0, t = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += WG) {
        const uint32_t v = arr[i];
        t += v;
        a += i < mid ? v : 0u;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        a += __shfl_xor(a, d, 64);
        t += __shfl_xor(t, d, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        sums_s[2 * (threadIdx.x >> 6)] = a;
        sums_s[2 * (threadIdx.x >> 6) + 1] = t;
    }
    __syncthreads();
    before = sums_s[0] + sums_s[2] + sums_s[4] + sums_s[6];
    total = sums_s[1] + sums_s[3] + sums_s[5] + sums_s[7];
}

template <int ELEM, bool ZZ, bool I16ZZ, bool COUNT_ONLY, bool SELF = false>
__global__ __launch_bounds__(WG) void svb_seg_encode_kernel(ReadBatch b, uint32_t hdr, uint32_t strict_cap, const uint32_t* seg_first,
                                                            uint32_t* seg_bytes, const uint64_t* seg_off)
{
    constexpr int SEG = WG * Vpl<ELEM>::value * SEG_TILES;
    __shared__ __attribute__((aligned(16))) uint8_t stage[COUNT_ONLY ? 16 : EncStage<ELEM, I16ZZ>::value];
    __shared__ __attribute__((aligned(16))) uint32_t wsum[8];   // (I16Pairs uses two sets of four in turn)
    __shared__ uint64_t sums_s[8];
    uint32_t r, k;
    if (!seg_locate(seg_first, b.n_reads, blockIdx.x, r, k)) return;
    const int tid = threadIdx.x;
    if (COUNT_ONLY && tid == 0) seg_bytes[blockIdx.x] = 0;
    SvbEnc e;
    uint32_t verdict;
    const bool open = svb_enc_open<ELEM, I16ZZ>(b, r, hdr, strict_cap, &e, &verdict);
    uint64_t self_off = 0;
    if (SELF && !COUNT_ONLY) {
        // the data offset of this segment, and (first workgroup of the read) the read's result: svb_seg_encode_scan_kernel's work
        uint64_t total;
        seg_sums(seg_bytes, seg_first[r], blockIdx.x, seg_first[r + 1], sums_s, self_off, total);
        uint32_t res;
        if (k == 0 && tid == 0 && svb_seg_enc_result(open, e, verdict, hdr, total, &res)) b.result[r] = res;
    }
    if (!open) return;   // (the scan, or the read's first workgroup, writes the verdict)
    const uint32_t n = e.n, keyLen = e.keyLen;
    const uint32_t first = k * (uint32_t)SEG;
    const uint32_t end = n - first > (uint32_t)SEG ? first + SEG : n;
    if (first >= n) return;  // the single (empty) segment of an empty read
    const uint8_t* in = e.in;
    uint8_t* out = e.out + hdr;
    if (COUNT_ONLY) {
        const uint64_t bytes = svb_encode_range<ELEM, ZZ, I16ZZ, true>(in, first, end, nullptr, nullptr, stage, wsum);
        if (tid == 0) seg_bytes[blockIdx.x] = (uint32_t)bytes;
    } else {
        (void)svb_encode_range<ELEM, ZZ, I16ZZ, false>(in, first, end, out, out + keyLen + (SELF ? self_off : seg_off[blockIdx.x]), stage, wsum);
    }
}

// one workgroup per read: data offsets of its segments (exclusive scan of their byte counts) and the read's result
template <int ELEM, bool I16ZZ>
__global__ __launch_bounds__(WG) void svb_seg_encode_scan_kernel(ReadBatch b, uint32_t hdr, uint32_t strict_cap, const uint32_t* seg_first,
                                                                 const uint32_t* seg_bytes, uint64_t* seg_off)
{
    __shared__ uint32_t wsum[4];
    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t s0 = seg_first[r], s1 = seg_first[r + 1];
    uint64_t carry = 0;
    for (uint32_t base = s0; base < s1; base += WG) {
        const uint32_t i = base + (uint32_t)tid;
        const uint32_t v = i < s1 ? seg_bytes[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan_u32(v, wsum, tot);
        if (i < s1) seg_off[i] = carry + ex;
        carry += tot;
    }
    SvbEnc e;
    uint32_t verdict, res;
    const bool open = svb_enc_open<ELEM, I16ZZ>(b, r, hdr, strict_cap, &e, &verdict);
    if (tid == 0 && svb_seg_enc_result(open, e, verdict, hdr, carry, &res)) b.result[r] = res;
}

// ------------------------------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------------------------------
// ---- pairs of whole int16 zig-zag tiles, decoded two loads ahead (round 6) --------------------------------------------------------------
// The tile loop of svb_decode_range asks memory twice per tile, one request behind the other: the control bytes, then -- where the
// scan of their lengths says the tile's data bytes start -- the data bytes; with eight workgroups per CU that chain of round trips, not
// the 21.4 GB the launch moves, is what its 4.7 ms per 65 536 reads were (the fewer instructions and barriers of rounds 2 - 5 all
// measured +- 0).  Whole tiles of int16 values with one- and two-byte codes -- everything but the ends of a read this library or the
// reference wrote -- go through this loop, two tiles per trip, as a pipeline: a trip PLANS the pair after the one it decodes (scan of
// the lengths the control bytes announce: where its data bytes stand), REQUESTS that pair's data bytes into registers and the control
// bytes of the pair after it, then decodes the pair whose bytes the trip before left in LDS, and last moves the requested bytes into
// the other stage buffer.  Every request has a whole trip to arrive, and a trip has two barriers (ten before, for two tiles).  The
// lengths of both tiles ride in the halves of one register through one scan; the delta sums need a scan each (16-bit wrap-around).
// A pair that is not of that kind (3- or 4-byte codes, a stream shorter than announced, more bytes than a stage buffer holds) ends
// the loop before anything of it is touched, and the tile loop -- which decides every verdict -- goes on from there.
struct I16DecPairs
{
    static constexpr uint32_t TILE = WG * 8, BUF = 2 * WG * 8 * 3 / 2 + 48;   // a stage buffer: two tiles at 3/2 bytes per value + alignment slack
    static constexpr uint32_t WS_LEN = 0, WS_DELTA = 8, WS_FLAG = 24, WS_WORDS = 28;   // LDS words: 2 x 4 length sums, 2 x 8 delta sums, the flag
    const uint8_t* in;        // control bytes
    const uint8_t* data;
    uint32_t dataBytes;
    uint8_t* stage;           // two buffers of BUF bytes
    uint32_t* ws;             // WS_WORDS words, 16-byte aligned

    static __device__ __forceinline__ uint32_t announced(uint32_t k) { return 8u + (uint32_t)__popc(k & 0x5555u) + 2u * (uint32_t)__popc(k & 0xAAAAu); }

    // a lane's eight values (codes 0 / 1) from the bytes at buf[o ...]: inclusive sums of the un-zig-zagged deltas (mod 2^32; the caller keeps 16 bits)
    static __device__ __forceinline__ uint32_t decode8(const uint8_t* buf, uint32_t o, uint32_t keybits, uint32_t s[8])
    {
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t two = (keybits >> (2 * k)) & 1u;
            const uint32_t lo = buf[o], hi = buf[o + 1];
            uint32_t v = lo | (two ? hi << 8 : 0u);
            o += 1u + two;
            v = (v >> 1) ^ (0u - (v & 1u));   // sse3.h:516-523
            acc += v;
            s[k] = acc;
        }
        return acc;
    }

    // pairs from t0 on while two whole tiles are left; pos / run as in svb_decode_range.  Returns the first value not decoded (a multiple of
    // the tile size from t0).  All 256 threads; ends with a barrier.  st: the store, of whole lines (st.aligned()).
    template <class Store>
    __device__ __forceinline__ uint32_t run(const Store& st, uint32_t t0_in, uint32_t end_in, uint64_t& pos_io, uint32_t& run_io)
    {
        const int tid = threadIdx.x, lane = tid & 63;
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        const uint32_t m0 = wv > 0 ? 0xFFFFFFFFu : 0u, m1 = wv > 1 ? 0xFFFFFFFFu : 0u, m2 = wv > 2 ? 0xFFFFFFFFu : 0u;
        const uint32_t end = (uint32_t)__builtin_amdgcn_readfirstlane((int)end_in);
        uint32_t tn = (uint32_t)__builtin_amdgcn_readfirstlane((int)t0_in);   // the pair the next trip plans
        uint64_t posn = I16Pairs<false, false>::uniform64(pos_io);              // ... and where its data bytes start
        uint32_t rn = (uint32_t)__builtin_amdgcn_readfirstlane((int)run_io);
        auto load_keys = [&](uint32_t t, uint32_t& ka, uint32_t& kb) {
            const uint8_t* kp = in + ((t + (uint32_t)tid * 8u) >> 2);
            uint16_t a, b;
            __builtin_memcpy(&a, kp, 2);
            __builtin_memcpy(&b, kp + TILE / 4, 2);
            ka = a;
            kb = b;
        };
        bool more = end - tn >= 2u * TILE, have = false;
        uint32_t kna = 0, knb = 0;
        if (more) load_keys(tn, kna, knb);
        if (tid == 0) ws[WS_FLAG] = 0;
        wg_lds_barrier();   // the flag is cleared before any wavefront's first trip can set it (the control bytes stay in flight)
        uint32_t cur = 0, par = 0;
        uint32_t kca = 0, kcb = 0, exC = 0, totC = 0, misC = 0, tc = 0;   // the pair in the stage
        while (more || have) {
            uint32_t Ln = 0, incn = 0;
            if (more) {
                Ln = announced(kna) | (announced(knb) << 16);
                incn = wave_incl_scan_u32(Ln);
                if (lane == 63) ws[WS_LEN + par * 4 + wv] = incn;
                if (__any(((kna | knb) & 0xAAAAu) != 0) && lane == 0) ws[WS_FLAG] = 1;   // codes of 3 or 4 bytes: not for this loop
            }
            wg_lds_barrier();
            uint32_t exN = 0, totN = 0, misN = 0, kn2a = 0, kn2b = 0;
            uint4 d0 = make_uint4(0u, 0u, 0u, 0u), d1 = d0;
            bool more2 = false;
            if (more) {
                const uint4 s4 = *reinterpret_cast<const uint4*>(ws + WS_LEN + par * 4);
                totN = (uint32_t)__builtin_amdgcn_readfirstlane((int)(s4.x + s4.y + s4.z + s4.w));
                exN = (s4.x & m0) + (s4.y & m1) + (s4.z & m2) + incn - Ln;
                const uint32_t bad = (uint32_t)__builtin_amdgcn_readfirstlane((int)ws[WS_FLAG]);
                const uint32_t bytes = (totN & 0xFFFFu) + (totN >> 16);
                misN = (uint32_t)((uintptr_t)(data + posn) & 15u);
                if (bad || posn + bytes > dataBytes || misN + bytes + 16u > BUF) {
                    more = false;   // (workgroup-uniform) the tile loop takes it from here
                } else {
                    const uint8_t* ga = data + posn - misN;
                    const uint32_t nch = (misN + bytes + 15u) >> 4;
                    if ((uint32_t)tid < nch) d0 = *reinterpret_cast<const uint4*>(ga + 16u * (uint32_t)tid);
                    if ((uint32_t)tid + WG < nch) d1 = *reinterpret_cast<const uint4*>(ga + 16u * ((uint32_t)tid + WG));
                    more2 = end - tn >= 4u * TILE;
                    if (more2) load_keys(tn + 2u * TILE, kn2a, kn2b);
                }
            }
            uint32_t sA[8], sB[8], accA = 0, accB = 0, incA = 0, incB = 0;
            if (have) {
                const uint8_t* buf = stage + cur * BUF;
                accA = decode8(buf, misC + (exC & 0xFFFFu), kca, sA);
                accB = decode8(buf, misC + (totC & 0xFFFFu) + (exC >> 16), kcb, sB);
                incA = wave_incl_scan_u32(accA);
                incB = wave_incl_scan_u32(accB);
                if (lane == 63) {
                    ws[WS_DELTA + par * 8 + wv] = incA;
                    ws[WS_DELTA + par * 8 + 4 + wv] = incB;
                }
            }
            wg_lds_barrier();
            if (have) {
                const uint4 a4 = *reinterpret_cast<const uint4*>(ws + WS_DELTA + par * 8), b4 = *reinterpret_cast<const uint4*>(ws + WS_DELTA + par * 8 + 4);
                const uint32_t totA = a4.x + a4.y + a4.z + a4.w, totB = b4.x + b4.y + b4.z + b4.w;
                const uint32_t baseA = rn + (a4.x & m0) + (a4.y & m1) + (a4.z & m2) + incA - accA;
                const uint32_t baseB = rn + totA + (b4.x & m0) + (b4.y & m1) + (b4.z & m2) + incB - accB;
                st.put(tc + (uint32_t)tid * 8u, 8, baseA, sA);
                st.put(tc + TILE + (uint32_t)tid * 8u, 8, baseB, sB);
                rn = (uint32_t)__builtin_amdgcn_readfirstlane((int)(rn + totA + totB));
            }
            have = more;
            if (more) {   // the requested bytes into the other buffer: the next trip decodes them
                cur ^= 1u;
                uint8_t* nb = stage + cur * BUF;
                const uint32_t bytes = (totN & 0xFFFFu) + (totN >> 16), nch = (misN + bytes + 15u) >> 4;
                if ((uint32_t)tid < nch) *reinterpret_cast<uint4*>(nb + 16u * (uint32_t)tid) = d0;
                if ((uint32_t)tid + WG < nch) *reinterpret_cast<uint4*>(nb + 16u * ((uint32_t)tid + WG)) = d1;
                kca = kna;
                kcb = knb;
                exC = exN;
                totC = totN;
                misC = misN;
                tc = tn;
                posn += bytes;
                tn += 2u * TILE;
                kna = kn2a;
                knb = kn2b;
                more = more2;
            }
            par ^= 1u;
        }
        wg_lds_barrier();
        pos_io = posn;
        run_io = rn;
        return tn;
    }
};


// Per-read validation of the svb decoders (the one-workgroup kernel, the segmented kernels): returns true
// when the read is finished with `res`.
template <int ELEM, bool I16ZZ>
__device__ __forceinline__ bool svb_decode_check(uint32_t in_size, uint32_t out_size, uint32_t& res)
{
    if (out_size % ELEM != 0) {  // vbz/v0/vbz_streamvbyte.cpp:75-78
        res = E_DESTINATION_SIZE;
        return true;
    }
    const uint32_t count = out_size / ELEM;
    const uint32_t keyLen = (count + 3u) >> 2;
    if (I16ZZ) {
        if (count == 0) {  // sse3.h:472-476
            res = 0;
            return true;
        }
        if (in_size < keyLen) {  // sse3.h:478-482
            res = E_INPUT_SIZE;
            return true;
        }
    } else {
        // streamvbyte_validate_stream (vbz/v0/vbz_streamvbyte_impl.h:49-51)
        if (in_size == 0 || count == 0) {
            res = (in_size == count) ? 0u : E_STREAM;
            return true;
        }
        if (keyLen > in_size) {
            res = E_STREAM;
            return true;
        }
    }
    return false;
}

// Read r of a decode launch, opened: the gate and the previous stage's verdict (read_gate), then the check above.  true: walk the read --
// *rd holds its stream and its sizes; false: *verdict is the read's result (GATE_SKIP: none to write).  svb16_row_open's contract, and
// where every sink of this decoder starts from, on all three launch shapes (one workgroup per read, segments with self-summed prefixes,
// segments with scan launches).
struct SvbRead
{
    const uint8_t* in;
    uint32_t in_size, count, keyLen, dataBytes;
};
template <int ELEM, bool I16ZZ>
__device__ __forceinline__ bool svb_read_open(const ReadBatch& b, uint32_t r, SvbRead* rd, uint32_t* verdict)
{
    *verdict = read_gate(b, r, true);
    if (*verdict) return false;
    rd->in_size = b.src_size[r];
    const uint32_t out_size = b.dst_cap[r];   // exact decoded byte count
    if (svb_decode_check<ELEM, I16ZZ>(rd->in_size, out_size, *verdict)) return false;
    rd->count = out_size / ELEM;
    rd->keyLen = (rd->count + 3u) >> 2;
    rd->dataBytes = rd->in_size - rd->keyLen;
    rd->in = b.src + b.src_off[r];
    return true;
}

// The result of a read of the large-read path, from what svb_read_open said of it (open, rd, verdict) and the data bytes its segments'
// control bytes announced in all (the stream is good iff that total equals the data bytes present): whether one is to be written, and
// *res.  bytes_per_value: the store's.
__device__ __forceinline__ bool svb_seg_read_result(bool open, const SvbRead& rd, uint32_t verdict, uint64_t announced, uint32_t bytes_per_value,
                                                    uint32_t* res)
{
    *res = !open ? verdict : (announced == rd.dataBytes ? rd.count * bytes_per_value : E_STREAM);
    return open || verdict != GATE_SKIP;
}

// The svb decoder's LDS, declared once per kernel (`const SvbDecLds<..> lds;`).  PAIRS: the kernel runs I16DecPairs (the two stage buffers
// and the sums of that loop; the tile loop's 8240 bytes fit), else one tile's worst case.  (Two variables, as norm_lds() has one: a
// kernel pays for the ones it touches.)
template <int ELEM, bool PAIRS>
struct SvbDecLds
{
    static constexpr int STAGE = PAIRS ? 2 * (int)I16DecPairs::BUF : WG * Vpl<ELEM>::value * 4 + 48;
    static_assert(STAGE >= WG * Vpl<ELEM>::value * 4 + 48, "the tile loop's stage");
    uint8_t* stage;
    uint32_t* wsum;
    __device__ __forceinline__ SvbDecLds()
    {
        __shared__ __attribute__((aligned(16))) uint8_t s[STAGE];
        __shared__ __attribute__((aligned(16))) uint32_t w[PAIRS ? (int)I16DecPairs::WS_WORDS : 4];
        stage = s;
        wsum = w;
    }
};

// MODE 0: decode values [first, end) of a stream of `count` values whose data bytes start at data[pos] and whose delta
//         chain stands at `run`; store them.  MODE 1: only add up the data bytes the control bytes announce.
//         MODE 2: decode without storing (the total of the deltas is wanted).  pos / run are updated; returns false when
//         the stream is shorter than its control bytes claim.  All 256 threads.  st: the sink MODE 0 stores through (svb_store.h);
//         the MODE 0 range that starts at the read's first value (the whole read, or its first segment) also finishes it.
template <int ELEM, bool ZZ, bool I16ZZ, int MODE, class Store>
__device__ __forceinline__ bool svb_decode_range(const uint8_t* in, const uint8_t* data, uint32_t dataBytes, uint32_t count, uint32_t first,
                                                 uint32_t end, uint64_t& pos_io, uint32_t& run_io, const Store& st, uint8_t* stage, uint32_t* wsum)
{
    constexpr int VPL = Vpl<ELEM>::value;
    constexpr int TILE = WG * VPL;
    const int tid = threadIdx.x;
    const uint32_t* stage32 = reinterpret_cast<const uint32_t*>(stage);
    uint64_t pos = pos_io;   // data bytes consumed so far
    uint32_t run = run_io;   // running value of the delta chain
    bool good = true;
    uint32_t t_start = first;
    if (I16ZZ && MODE == 0 && st.aligned() && end - first >= 2u * (uint32_t)TILE) {   // pairs of whole tiles: I16DecPairs
        I16DecPairs dp = { in, data, dataBytes, stage, wsum };
        t_start = dp.run(st, first, end, pos, run);
    }
    for (uint32_t t0 = t_start; t0 < end; t0 += TILE) {
        const uint32_t i0 = t0 + (uint32_t)tid * VPL;
        const int valid = i0 >= end ? 0 : (end - i0 >= (uint32_t)VPL ? VPL : (int)(end - i0));
        uint32_t keybits = 0;
        if (valid > 0) {
            const uint8_t* kp = in + (i0 >> 2);
            keybits = kp[0];
            if (VPL == 8 && valid > 4) keybits |= (uint32_t)kp[1] << 8;
        }
        // bytes of the lane's values: each 2-bit code is length - 1; the sum of the 2-bit fields of a word is
        // (word & 0x5555) + ((word >> 1) & 0x5555) folded -- two population counts
        const uint32_t kb = valid == VPL ? keybits : (keybits & ((1u << (2 * valid)) - 1u));
        const uint32_t L = (uint32_t)valid + (uint32_t)__popc(kb & 0x5555u) + 2u * (uint32_t)__popc(kb & 0xAAAAu);
        uint32_t tot;
        const uint32_t ex = block_excl_scan_u32(L, wsum, tot);
        if (MODE == 1) {
            pos += tot;
            continue;
        }
        if (pos + tot > dataBytes) {  // stream shorter than its control bytes claim
            good = false;
            break;
        }
        // stage the tile's data bytes: aligned 16-byte chunks, coalesced
        const uint8_t* g0 = data + pos;
        const uint32_t mis = (uint32_t)((uintptr_t)g0 & 15u);
        const uint8_t* ga = g0 - mis;
        const uint32_t nch = (mis + tot + 15u) >> 4;
        for (uint32_t c = tid; c < nch; c += WG)
            *reinterpret_cast<uint4*>(stage + 16u * c) = *reinterpret_cast<const uint4*>(ga + 16ull * c);
        wg_lds_barrier();
        uint32_t o = mis + ex;
        // int16 zig-zag path: SIMD body vs scalar tail of the reference (sse3.h:494-540 vs 542-572)
        const bool body = I16ZZ && ((i0 >> 3) < (count >> 3)) && (dataBytes - (pos + ex) >= 32u);
        uint32_t s[VPL];
        uint32_t acc = 0;
        // full tile of one- and two-byte codes (what the encoder writes for int16): values stay below 2^16, where the
        // body and the tail of the reference agree, so the lane just picks up its bytes
        if (I16ZZ && end - t0 >= (uint32_t)TILE && !__any((keybits & 0xAAAAu) != 0)) {
#pragma unroll
            for (int k = 0; k < VPL; ++k) {
                const uint32_t two = (keybits >> (2 * k)) & 1u;
                const uint32_t lo = stage[o], hi = stage[o + 1];
                uint32_t v = lo | (two ? hi << 8 : 0u);
                o += 1u + two;
                v = (v >> 1) ^ (0u - (v & 1u));
                acc += v;
                s[k] = acc;
            }
        } else {
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            uint32_t v = 0;
            if (k < valid) {
                const uint32_t len = ((keybits >> (2 * k)) & 3u) + 1u;
                const uint32_t w0 = stage32[o >> 2];
                const uint32_t w1 = stage32[(o >> 2) + 1];
                v = (uint32_t)(((uint64_t)w1 << 32 | w0) >> (8u * (o & 3u)));
                v &= 0xFFFFFFFFu >> (32u - 8u * len);
                o += len;
            }
            if (ZZ) {
                if (I16ZZ && body) v &= 0xFFFFu;  // keep the low 16 bits (sse3.h:510-514)
                v = (v >> 1) ^ (0u - (v & 1u));
                acc += v;
                s[k] = acc;
            } else {
                s[k] = v;
            }
        }
        }
        uint32_t base = 0;
        if (ZZ) {
            uint32_t ttot;
            base = run + block_excl_scan_u32(acc, wsum, ttot);
            run += ttot;
        } else {
            wg_lds_barrier();  // stage is overwritten by the next tile
        }
        if (MODE == 2) {
            pos += tot;
            continue;
        }
        st.put(i0, valid, base, s);
        pos += tot;
    }
    if (MODE == 0 && first == 0) st.finish();   // (the read's first range: the whole read, or its first segment)
    if (MODE == 0) st.done();
    pos_io = pos;
    run_io = run;
    return good;
}

#ifndef VBZ_SVBDEC_WAVES
#define VBZ_SVBDEC_WAVES 1
#endif
// This kernel keeps its prologue and its LDS pair as its own text (svb_read_open's order, spelled out): opened through the shared
// statement, its float32 instantiation took 72 registers for 82 and measured 3 % slower, and the counting and window ones moved too.
template <int ELEM, bool ZZ, bool I16ZZ, int OUT = SIG_NONE>
__global__ __launch_bounds__(WG, VBZ_SVBDEC_WAVES) void svb_decode_kernel(ReadBatch b)
{
    constexpr int STAGE = I16ZZ ? 2 * (int)I16DecPairs::BUF : WG * Vpl<ELEM>::value * 4 + 48;   // (int16 zig-zag: the two buffers of I16DecPairs; the tile loop's 8240 bytes fit)
    static_assert(STAGE >= WG * Vpl<ELEM>::value * 4 + 48, "the tile loop's stage");
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE];
    __shared__ __attribute__((aligned(16))) uint32_t wsum[I16ZZ ? (int)I16DecPairs::WS_WORDS : 4];

    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x;
    if (b.gate && b.gate[r] >= GATE_SKIP) {
        if (tid == 0 && b.gate[r] != GATE_SKIP) b.result[r] = b.gate[r];
        return;
    }
    const uint32_t in_size = b.src_size[r];
    if (in_size >= E_FIRST) {  // the previous stage failed for this read
        if (tid == 0) b.result[r] = in_size;
        return;
    }
    const uint32_t out_size = b.dst_cap[r];  // exact decoded byte count
    uint32_t res;
    if (svb_decode_check<ELEM, I16ZZ>(in_size, out_size, res)) {
        if (tid == 0) b.result[r] = res;
        return;
    }
    if ((OUT & SIG_COUNT) && b.sig.norm.st[r].phase == NORM_DONE) return;   // (a later counting pass: the read is finished)
    const uint32_t count = out_size / ELEM;
    const uint32_t keyLen = (count + 3u) >> 2;
    const uint8_t* in = b.src + b.src_off[r];
    const uint32_t dataBytes = in_size - keyLen;
    uint64_t pos = 0;
    uint32_t run = 0;
    const DecStore<ELEM, OUT> st = dec_store<ELEM, OUT>(b.dst, b.dst_off, OUT == SIG_NONE ? nullptr : &b, r, count);
    const bool good = svb_decode_range<ELEM, ZZ, I16ZZ, 0>(in, in + keyLen, dataBytes, count, 0, count, pos, run, st, stage, wsum);
    if (tid == 0) b.result[r] = (!good || pos != dataBytes) ? E_STREAM : count * st.BYTES;
}

// ---- segmented decode: pass 1 adds up the data bytes each segment's control bytes announce; a scan gives every
// segment its data offset and decides the read's verdict (the stream is good iff the announced total equals the data
// bytes present -- the same predicate streamvbyte_validate_stream computes); zig-zag streams then need the delta total
// of every segment (pass 2, decode without storing) and a second scan before the storing pass.
// SELF (see svb_seg_encode_kernel): no scan launches -- MODE 2 / 0 workgroups add up the announced lengths (seg_val, left by MODE 1)
// in front of them and over the whole read (the verdict: good iff the total equals the bytes present), MODE 2 leaves its delta
// totals in seg_run_io and MODE 0 adds those up too; a read's first MODE 0 workgroup writes the read's result.
// OUT (MODE 0): the typed store.  Segments start at multiples of SEG samples: their typed offsets stay 16-byte aligned.
template <int ELEM, bool ZZ, bool I16ZZ, int MODE, bool SELF = false, int OUT = SIG_NONE>
__global__ __launch_bounds__(WG) void svb_seg_decode_kernel(ReadBatch b, const uint32_t* seg_first, uint32_t* seg_val, const uint64_t* seg_pos,
                                                            uint32_t* seg_run_io)
{
    static_assert(OUT == SIG_NONE || MODE == 0, "the typed stores are the storing pass's");
    const uint32_t* seg_run = seg_run_io;
    constexpr int SEG = WG * Vpl<ELEM>::value * SEG_TILES;
    // (not SvbDecLds: arrays of the kernel's own are dropped where a MODE stages nothing, and the LDS of those instantiations stays what it was)
    constexpr int STAGE = MODE == 1 ? 16 : ((I16ZZ && MODE == 0) ? 2 * (int)I16DecPairs::BUF : WG * Vpl<ELEM>::value * 4 + 48);
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE];
    __shared__ __attribute__((aligned(16))) uint32_t wsum[(I16ZZ && MODE == 0) ? (int)I16DecPairs::WS_WORDS : 4];
    __shared__ uint64_t sums_s[8];
    uint32_t r, k;
    if (!seg_locate(seg_first, b.n_reads, blockIdx.x, r, k)) return;
    const int tid = threadIdx.x;
    if (MODE != 0 && tid == 0) (SELF && MODE == 2 ? seg_run_io : seg_val)[blockIdx.x] = 0;
    SvbRead rd;
    uint32_t verdict;
    const bool open = svb_read_open<ELEM, I16ZZ>(b, r, &rd, &verdict);
    uint64_t self_pos = 0, self_total = 0, self_run = 0;
    if (SELF && MODE != 1) {
        seg_sums(seg_val, seg_first[r], blockIdx.x, seg_first[r + 1], sums_s, self_pos, self_total);
        if (MODE == 0 && ZZ) {
            uint64_t dummy;
            seg_sums(seg_run, seg_first[r], blockIdx.x, seg_first[r + 1], sums_s, self_run, dummy);
        }
        uint32_t res0;   // (svb_seg_decode_scan_kernel<.., VERDICT>'s first thread)
        if (MODE == 0 && k == 0 && tid == 0 && svb_seg_read_result(open, rd, verdict, self_total, DecStore<ELEM, OUT>::BYTES, &res0)) b.result[r] = res0;
    }
    if (!open) return;   // (the scan, or the read's first MODE 0 workgroup, writes the verdict)
    if (SELF) {
        if (MODE != 1 && self_total != (uint64_t)rd.dataBytes) return;   // the stream is malformed
    } else if (MODE != 1 && b.result[r] >= E_FIRST) return;  // the scan found the stream malformed
    if ((OUT & SIG_COUNT) && b.sig.norm.st[r].phase == NORM_DONE) return;
    const uint32_t count = rd.count;
    const uint32_t first = k * (uint32_t)SEG;
    if (first >= count) return;
    const uint32_t end = count - first > (uint32_t)SEG ? first + SEG : count;
    uint64_t pos = MODE == 1 ? 0 : (SELF ? self_pos : seg_pos[blockIdx.x]);
    uint32_t run = (MODE == 0 && ZZ) ? (SELF ? (uint32_t)self_run : seg_run[blockIdx.x]) : 0u;
    const uint64_t pos0 = pos;
    const DecStore<ELEM, OUT> st = dec_store<ELEM, OUT>(b.dst, b.dst_off, OUT == SIG_NONE ? nullptr : &b, r, count);
    (void)svb_decode_range<ELEM, ZZ, I16ZZ, MODE>(rd.in, rd.in + rd.keyLen, rd.dataBytes, count, first, end, pos, run, st, stage, wsum);
    if (MODE == 1 && tid == 0) seg_val[blockIdx.x] = (uint32_t)(pos - pos0);
    if (MODE == 2 && tid == 0) (SELF ? seg_run_io : seg_val)[blockIdx.x] = run;
}

// one workgroup per read.  VERDICT: exclusive scan of the announced data bytes -> seg_pos, and the read's result;
// otherwise: exclusive scan (mod 2^32) of the delta totals -> seg_run.  RES: bytes per value in the result (the typed store's).
template <int ELEM, bool I16ZZ, bool VERDICT, int RES = ELEM>
__global__ __launch_bounds__(WG) void svb_seg_decode_scan_kernel(ReadBatch b, const uint32_t* seg_first, const uint32_t* seg_val, uint64_t* seg_pos,
                                                                 uint32_t* seg_run)
{
    __shared__ uint32_t wsum[4];
    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t s0 = seg_first[r], s1 = seg_first[r + 1];
    uint64_t carry = 0;
    for (uint32_t base = s0; base < s1; base += WG) {
        const uint32_t i = base + (uint32_t)tid;
        const uint32_t v = i < s1 ? seg_val[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan_u32(v, wsum, tot);
        if (i < s1) {
            if (VERDICT) seg_pos[i] = carry + ex;
            else seg_run[i] = (uint32_t)carry + ex;
        }
        carry += tot;
    }
    SvbRead rd;
    uint32_t verdict, res;
    const bool open = svb_read_open<ELEM, I16ZZ>(b, r, &rd, &verdict);
    if (VERDICT && tid == 0 && svb_seg_read_result(open, rd, verdict, carry, RES, &res)) b.result[r] = res;
}

// ------------------------------------------------------------------------------------------------
// v1 nibble ("half") codec for 1-byte integers: reference vbz/v1/vbz_streamvbyte_impl.h:20-216
//   code 0: value 0, no data; 1: one nibble; 2: two nibbles; 3: four nibbles (low 16 bits of the value);
//   nibbles are appended low nibble first.  Same tiling as the byte codec, but offsets are in nibbles: a lane
//   assembles its <= 32 nibbles in registers and ORs them into a zeroed LDS stage (two lanes can share a byte).
// ------------------------------------------------------------------------------------------------
template <bool ZZ>
__global__ __launch_bounds__(WG) void svb_half_encode_kernel(ReadBatch b, uint32_t hdr)
{
    constexpr int VPL = 8;
    constexpr int TILE = WG * VPL;
    constexpr int STAGE_W = (TILE * 2 + 64) / 4;  // a tile emits at most 4 nibbles per value
    __shared__ __attribute__((aligned(16))) uint32_t stage[STAGE_W];
    __shared__ uint32_t wsum[4];

    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x;
    if (const uint32_t verdict = read_gate(b, r, false)) return read_closed(b, r, verdict);
    const uint32_t n = b.src_size[r];  // one byte per value
    const uint32_t cap = b.dst_cap[r];
    const uint32_t keyLen = (n + 3u) >> 2;
    {   // the reference requires the worst case of the byte codec (vbz/vbz.cpp:171-174)
        const uint64_t worst = (uint64_t)keyLen + 4ull * n + hdr;
        if (worst > cap) {
            if (tid == 0) b.result[r] = worst > 0xFFFFFFF0ull ? E_INPUT_SIZE : E_DESTINATION_SIZE;
            return;
        }
    }
    const uint8_t* in = b.src + b.src_off[r];
    uint8_t* out = b.dst + b.dst_off[r];
    if (hdr) {
        if (tid < 4) out[tid] = (uint8_t)(n >> (8 * tid));
        out += 4;
    }
    uint8_t* keys = out;
    uint8_t* data = out + keyLen;
    for (int i = tid; i < STAGE_W; i += WG) stage[i] = 0;
    wg_lds_barrier();

    uint64_t flushed = 0;  // data bytes already written
    uint32_t held = 0;     // nibbles held in stage[] (they start at nibble 0 of the stage)
    for (uint32_t t0 = 0; t0 < n; t0 += TILE) {
        const uint32_t i0 = t0 + (uint32_t)tid * VPL;
        const int valid = i0 >= n ? 0 : (n - i0 >= (uint32_t)VPL ? VPL : (int)(n - i0));
        int32_t prev = 0;
        if (ZZ && valid > 0 && i0 > 0) prev = load_elem(in + i0 - 1, 1);
        uint32_t keybits = 0, nibs = 0;
        unsigned __int128 acc = 0;
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            if (k < valid) {
                const int32_t x = load_elem(in + i0 + k, 1);
                uint32_t u = (uint32_t)x;
                if (ZZ) {
                    const uint32_t d = (uint32_t)x - (uint32_t)prev;  // streamvbyte zigzag_delta_encode
                    u = (d << 1) ^ (uint32_t)((int32_t)d >> 31);
                    prev = x;
                }
                const uint32_t code = u == 0 ? 0u : (u < 16u ? 1u : (u < 256u ? 2u : 3u));
                const uint32_t nn = (1u << code) >> 1;
                const uint32_t bits = nn == 4 ? (u & 0xFFFFu) : (u & ((1u << (4 * nn)) - 1u));
                acc |= (unsigned __int128)bits << (4 * nibs);
                nibs += nn;
                keybits |= code << (2 * k);
            }
        }
        if (valid > 0) {
            uint8_t* kp = keys + (i0 >> 2);
            kp[0] = (uint8_t)keybits;
            if (valid > 4) kp[1] = (uint8_t)(keybits >> 8);
        }
        uint32_t tot;
        const uint32_t ex = block_excl_scan_u32(nibs, wsum, tot);
        if (nibs) {
            const uint32_t o = held + ex;  // nibble offset in the stage
            const uint32_t sh = 4 * (o & 7);
            const unsigned __int128 lo = acc << sh;
            const uint32_t top = sh ? (uint32_t)(acc >> (128 - sh)) : 0u;
            const uint32_t w[5] = { (uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)(lo >> 64), (uint32_t)(lo >> 96), top };
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if (w[k]) atomicOr(&stage[(o >> 3) + k], w[k]);
        }
        wg_lds_barrier();
        // write the complete 16-byte chunks, keep the rest (including a half-filled byte) at the front
        const uint32_t endn = held + tot;
        const uint32_t nch = endn >> 5;  // 32 nibbles per chunk
        for (uint32_t c = tid; c < nch; c += WG) {
            const uint4 v = *reinterpret_cast<const uint4*>(stage + 4 * c);
            __builtin_memcpy(data + flushed + 16ull * c, &v, 16);
        }
        const uint32_t remw = ((endn & 31u) + 7u) >> 3;  // words still in use behind the chunks
        uint32_t keep = 0;
        if ((uint32_t)tid < remw) keep = stage[4 * nch + tid];
        wg_lds_barrier();
        for (uint32_t i = tid; i < ((endn + 7u) >> 3) + 1u && i < (uint32_t)STAGE_W; i += WG) stage[i] = 0;
        wg_lds_barrier();
        if ((uint32_t)tid < remw) stage[tid] = keep;
        flushed += 16ull * nch;
        held = endn & 31u;
        wg_lds_barrier();
    }
    const uint32_t tailBytes = (held + 1u) >> 1;
    if ((uint32_t)tid < tailBytes) data[flushed + tid] = (uint8_t)(stage[tid >> 2] >> (8 * (tid & 3)));
    if (tid == 0) b.result[r] = hdr + keyLen + (uint32_t)flushed + tailBytes;
}

template <bool ZZ>
__global__ __launch_bounds__(WG) void svb_half_decode_kernel(ReadBatch b)
{
    constexpr int VPL = 8;
    constexpr int TILE = WG * VPL;
    constexpr int STAGE = TILE * 2 + 64;
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE];
    __shared__ uint32_t wsum[4];

    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x;
    if (const uint32_t verdict = read_gate(b, r, true)) return read_closed(b, r, verdict);
    const uint32_t in_size = b.src_size[r];
    const uint32_t count = b.dst_cap[r];  // exact decoded byte count = value count
    // half validate_stream (vbz/v1/vbz_streamvbyte_impl.h)
    if (in_size == 0 || count == 0) {
        if (tid == 0) b.result[r] = (in_size == count) ? 0u : E_STREAM;
        return;
    }
    const uint32_t keyLen = (count + 3u) >> 2;
    if (keyLen > in_size) {
        if (tid == 0) b.result[r] = E_STREAM;
        return;
    }
    const uint8_t* in = b.src + b.src_off[r];
    const uint8_t* data = in + keyLen;
    uint8_t* out = b.dst + b.dst_off[r];
    const uint32_t dataBytes = in_size - keyLen;
    const uint32_t* stage32 = reinterpret_cast<const uint32_t*>(stage);

    uint64_t posn = 0;  // nibbles consumed so far
    uint32_t run = 0;   // running value of the delta chain
    bool bad = false;
    for (uint32_t t0 = 0; t0 < count; t0 += TILE) {
        const uint32_t i0 = t0 + (uint32_t)tid * VPL;
        const int valid = i0 >= count ? 0 : (count - i0 >= (uint32_t)VPL ? VPL : (int)(count - i0));
        uint32_t keybits = 0;
        if (valid > 0) {
            const uint8_t* kp = in + (i0 >> 2);
            keybits = kp[0];
            if (valid > 4) keybits |= (uint32_t)kp[1] << 8;
        }
        uint32_t nibs = 0;
#pragma unroll
        for (int k = 0; k < VPL; ++k)
            if (k < valid) nibs += (1u << ((keybits >> (2 * k)) & 3u)) >> 1;
        uint32_t tot;
        const uint32_t ex = block_excl_scan_u32(nibs, wsum, tot);
        if (((posn + tot + 1u) >> 1) > dataBytes) {  // stream shorter than its control bytes claim
            bad = true;
            break;
        }
        // stage the bytes that hold nibbles [posn, posn + tot): aligned 16-byte chunks, coalesced
        const uint8_t* g0 = data + (posn >> 1);
        const uint32_t mis = (uint32_t)((uintptr_t)g0 & 15u);
        const uint8_t* ga = g0 - mis;
        const uint32_t nbytes = (uint32_t)(((posn + tot + 1u) >> 1) - (posn >> 1));
        const uint32_t nch = (mis + nbytes + 15u) >> 4;
        for (uint32_t c = tid; c < nch; c += WG)
            *reinterpret_cast<uint4*>(stage + 16u * c) = *reinterpret_cast<const uint4*>(ga + 16ull * c);
        wg_lds_barrier();
        uint32_t o = 2u * mis + (uint32_t)(posn & 1u) + ex;  // nibble offset in the stage
        uint32_t s[VPL];
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            uint32_t v = 0;
            if (k < valid) {
                const uint32_t nn = (1u << ((keybits >> (2 * k)) & 3u)) >> 1;
                if (nn) {
                    const uint32_t w0 = stage32[o >> 3];
                    const uint32_t w1 = stage32[(o >> 3) + 1];
                    v = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (4u * (o & 7u)));
                    v &= 0xFFFFu >> (16u - 4u * nn);
                    o += nn;
                }
            }
            if (ZZ) {
                v = (v >> 1) ^ (0u - (v & 1u));
                acc += v;
                s[k] = acc;
            } else {
                s[k] = v;
            }
        }
        uint32_t base = 0;
        if (ZZ) {
            uint32_t ttot;
            base = run + block_excl_scan_u32(acc, wsum, ttot);
            run += ttot;
        } else {
            wg_lds_barrier();  // stage is overwritten by the next tile
        }
#pragma unroll
        for (int k = 0; k < VPL; ++k)
            if (k < valid) out[i0 + k] = (uint8_t)(base + s[k]);
        posn += tot;
    }
    if (tid == 0) b.result[r] = (bad || ((posn + 1u) >> 1) != dataBytes) ? E_STREAM : count;
}

// ------------------------------------------------------------------------------------------------
// svb16: the svb stage of POD5 signal rows (VBZ_GPU_VERSION_POD5; the format: include/vbz_gpu.h)
//   ceil(n / 8) key bytes, bit j % 8 of byte j / 8 set when zig-zag delta z_j takes two data bytes; then the data bytes, z_j as one
//   byte (z_j < 256) or two, little-endian.  Delta coding starts from 0 in every row, 16-bit wrap-around, as v0's int16 path.
// The one-workgroup-per-read shape of the byte codec above, one tile (256 lanes x 8 samples) per trip: at VPL = 8 a lane's samples
// are exactly one key byte, its data length is 8 + popcount(key), one workgroup scan gives the data offsets and a second one the
// delta sums; data bytes are staged through LDS so that HBM sees aligned 16-byte lines.  The decoder stores through DecStore<2, OUT>:
// the int16, typed, chunk and counting stores of v0's int16 decoder.  Both run on the large-read path too (one workgroup per read;
// DESIGN.md 4.13).
// ------------------------------------------------------------------------------------------------
constexpr int SVB16_TILE = WG * 8;
// the svb16 decoder's LDS, declared once per kernel (`const Svb16Lds lds;`): one tile's worst case of data bytes behind the bytes short of
// a line, and the scan's sums
struct Svb16Lds
{
    uint8_t* stage;
    uint32_t* wsum;
    __device__ __forceinline__ Svb16Lds()
    {
        __shared__ __attribute__((aligned(16))) uint8_t s[SVB16_TILE * 2 + 48];
        __shared__ __attribute__((aligned(16))) uint32_t w[4];
        stage = s;
        wsum = w;
    }
};

__global__ __launch_bounds__(WG) void svb16_encode_kernel(ReadBatch b, uint32_t* period_hint)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[SVB16_TILE * 2 + 32];   // the bytes short of a line + one tile's worst case
    __shared__ uint32_t wsum[4];

    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    if (period_hint && tid == 0) period_hint[r] = 0;   // (the svb16 stream is not probed: the entropy stage's matcher stays off)
    if (const uint32_t verdict = read_gate(b, r, false)) return read_closed(b, r, verdict);
    const uint32_t size = b.src_size[r];
    if (size & 1u) {
        if (tid == 0) b.result[r] = E_INPUT_SIZE;
        return;
    }
    const uint32_t n = size >> 1, K = (n + 7u) >> 3;
    const uint64_t worst = (uint64_t)K + 2ull * n;   // svb16_max(n)
    if (worst > b.dst_cap[r]) {
        if (tid == 0) b.result[r] = worst > 0xFFFFFFF0ull ? E_INPUT_SIZE : E_DESTINATION_SIZE;
        return;
    }
    const uint8_t* in = b.src + b.src_off[r];
    uint8_t* keys = b.dst + b.dst_off[r];
    uint8_t* data = keys + K;
    const uint32_t A = (uint32_t)((uintptr_t)data & 15u);
    uint8_t* gal = data - A;   // the 16-byte aligned address space of the data bytes
    const bool in_aligned = (((uintptr_t)in) & 15u) == 0;
    uint64_t F = 0;   // bytes of the aligned space flushed (a multiple of 16)
    uint64_t P = A;   // the next byte position; stage[] holds [F, P)
    for (uint32_t t0 = 0; t0 < n; t0 += SVB16_TILE) {
        const uint32_t i0 = t0 + (uint32_t)tid * 8u;
        const int valid = i0 >= n ? 0 : (n - i0 >= 8u ? 8 : (int)(n - i0));
        uint32_t x[8];
        if (valid == 8 && in_aligned) {
            const uint4 q = *reinterpret_cast<const uint4*>(in + (size_t)i0 * 2);
            const uint32_t w[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = k < valid ? (uint32_t)(uint16_t)load_elem(in + (size_t)(i0 + k) * 2, 2) : 0u;
        }
        // the sample in front: the lane below's last one; lane 0 of a wavefront reads it
        uint32_t prev = wave_prev_lane_u32(x[7]);
        if (lane == 0) prev = (i0 == 0 || valid == 0) ? 0u : (uint32_t)(uint16_t)load_elem(in + (size_t)(i0 - 1) * 2, 2);
        uint32_t z[8], key = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t d = (x[k] - prev) & 0xFFFFu;   // wrap-around delta, 16-bit zig-zag
            z[k] = ((d << 1) ^ (0u - (d >> 15))) & 0xFFFFu;
            prev = x[k];
            if (k < valid && z[k] > 0xFFu) key |= 1u << k;
        }
        if (valid > 0) keys[i0 >> 3] = (uint8_t)key;
        const uint32_t L = (uint32_t)valid + (uint32_t)__popc(key);
        uint32_t tot;
        const uint32_t ex = block_excl_scan_u32(L, wsum, tot);
        uint32_t o = (uint32_t)(P - F) + ex;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < valid) {
                stage[o++] = (uint8_t)z[k];
                if (z[k] > 0xFFu) stage[o++] = (uint8_t)(z[k] >> 8);
            }
        }
        wg_lds_barrier();
        const uint32_t endidx = (uint32_t)(P - F) + tot, nch = endidx >> 4;
        for (uint32_t c = tid; c < nch; c += WG) {
            uint8_t* g = gal + F + 16ull * c;
            if (F == 0 && c == 0 && A != 0) {
                for (uint32_t j = A; j < 16; ++j) g[j] = stage[j];
            } else {
                *reinterpret_cast<uint4*>(g) = *reinterpret_cast<const uint4*>(stage + 16u * c);
            }
        }
        const uint32_t rem = endidx & 15u;
        uint8_t keep = 0;
        if ((uint32_t)tid < rem) keep = stage[16u * nch + tid];
        wg_lds_barrier();
        if (nch > 0 && (uint32_t)tid < rem) stage[tid] = keep;
        F += 16ull * nch;
        P += tot;
        // (the scan at the top of the next tile holds the barrier that orders these LDS writes)
    }
    wg_lds_barrier();
    {   // the tail: bytes [F, P) still in LDS
        const uint32_t rem = (uint32_t)(P - F), lo = F == 0 ? A : 0u;
        if ((uint32_t)tid >= lo && (uint32_t)tid < rem) gal[F + tid] = stage[tid];
    }
    if (tid == 0) b.result[r] = K + (uint32_t)(P - A);
}

// One row's stream (in_size bytes at `in`, K <= in_size <= svb16_max(count)) through st.put(), a tile a trip, by the whole workgroup:
// whether the stream is exactly as long as its key bits announce.  stage / wsum: the kernel's LDS.  This is svb16_decode_kernel's tile
// loop for the kernels over reads; that kernel keeps its own text, which as a call of this function compiles to other registers.
// PREFIX (the trim pass): only the row's first min(stop, count) samples are walked, and the return says nothing about the stream's length.
template <bool PREFIX = false, class Store>
__device__ __forceinline__ bool svb16_decode_row(const uint8_t* in, uint32_t in_size, uint32_t count, const Store& st, uint8_t* stage, uint32_t* wsum,
                                                 uint32_t stop = 0)
{
    const int tid = threadIdx.x;
    const uint32_t K = (count + 7u) >> 3;
    const uint8_t* data = in + K;
    const uint32_t dataBytes = in_size - K;
    uint64_t pos = 0;   // data bytes consumed
    uint32_t run = 0;   // the delta chain's running value
    bool good = true;
    const uint32_t lim = PREFIX && stop < count ? stop : count;
    for (uint32_t t0 = 0; t0 < lim; t0 += SVB16_TILE) {
        const uint32_t i0 = t0 + (uint32_t)tid * 8u;
        const int valid = i0 >= lim ? 0 : (lim - i0 >= 8u ? 8 : (int)(lim - i0));
        const uint32_t key = valid > 0 ? (uint32_t)in[i0 >> 3] & ((1u << valid) - 1u) : 0u;   // (unused key bits ignored)
        const uint32_t L = (uint32_t)valid + (uint32_t)__popc(key);
        uint32_t tot;
        const uint32_t ex = block_excl_scan_u32(L, wsum, tot);
        if (pos + tot > dataBytes) {   // (workgroup-uniform) fewer data bytes than the key bits announce
            good = false;
            break;
        }
        const uint8_t* g0 = data + pos;
        const uint32_t mis = (uint32_t)((uintptr_t)g0 & 15u);
        const uint8_t* ga = g0 - mis;
        const uint32_t nch = (mis + tot + 15u) >> 4;
        for (uint32_t c = tid; c < nch; c += WG)
            *reinterpret_cast<uint4*>(stage + 16u * c) = *reinterpret_cast<const uint4*>(ga + 16ull * c);
        wg_lds_barrier();
        uint32_t o = mis + ex, s[8], acc = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t two = (key >> k) & 1u;
            uint32_t v = stage[o] | (two ? (uint32_t)stage[o + 1] << 8 : 0u);
            o += 1u + two;
            v = (v >> 1) ^ (0u - (v & 1u));
            acc += k < valid ? v : 0u;
            s[k] = acc;
        }
        uint32_t ttot;
        const uint32_t base = run + block_excl_scan_u32(acc, wsum, ttot);   // (its barriers also keep the next tile's staging behind these reads)
        run += ttot;
        st.put(i0, valid, base, s);
        pos += tot;
    }
    return good && pos == dataBytes;
}

// The verdicts of a POD5 row: content longer than svb16_max(n) is the zstd stage's (E_ZSTD), a stream whose length is not
// K + n + popcount(the first n key bits) -- bytes missing or left over -- E_STREAM.
// svb16_row_open: whether row r is to be decoded (*in_size, *count: its stream and its samples); else *verdict is its result (GATE_SKIP:
// none to write)
__device__ __forceinline__ bool svb16_row_open(const ReadBatch& b, uint32_t r, uint32_t* in_size, uint32_t* count, uint32_t* verdict)
{
    *verdict = read_gate(b, r, true);
    if (*verdict) return false;
    *in_size = b.src_size[r];
    const uint32_t out_size = b.dst_cap[r];
    *verdict = E_DESTINATION_SIZE;
    if (out_size & 1u) return false;
    *count = out_size >> 1;
    const uint32_t K = (*count + 7u) >> 3;
    *verdict = *in_size < K ? E_STREAM : E_ZSTD;
    if ((uint64_t)*in_size > (uint64_t)K + 2ull * *count || *in_size < K) return false;
    *verdict = 0;
    return *count != 0;   // (an empty stream: nothing to store or count)
}

template <int OUT>
__global__ __launch_bounds__(WG) void svb16_decode_kernel(ReadBatch b)
{
    const Svb16Lds lds;
    uint8_t* const stage = lds.stage;   // (the tile loop below keeps its own text)
    uint32_t* const wsum = lds.wsum;

    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x;
    uint32_t in_size = 0, count = 0, verdict;
    if (!svb16_row_open(b, r, &in_size, &count, &verdict)) return read_closed(b, r, verdict);   // (every pass gives the verdict)
    if ((OUT & SIG_COUNT) && b.sig.norm.st[r].phase == NORM_DONE) return;   // (a later counting pass: the read is finished)
    const uint32_t K = (count + 7u) >> 3;
    const uint8_t* in = b.src + b.src_off[r];
    const uint8_t* data = in + K;
    const uint32_t dataBytes = in_size - K;
    const DecStore<2, OUT> st = dec_store<2, OUT>(b.dst, b.dst_off, OUT == SIG_NONE ? nullptr : &b, r, count);
    uint64_t pos = 0;   // data bytes consumed
    uint32_t run = 0;   // the delta chain's running value
    bool good = true;
    for (uint32_t t0 = 0; t0 < count; t0 += SVB16_TILE) {
        const uint32_t i0 = t0 + (uint32_t)tid * 8u;
        const int valid = i0 >= count ? 0 : (count - i0 >= 8u ? 8 : (int)(count - i0));
        const uint32_t key = valid > 0 ? (uint32_t)in[i0 >> 3] & ((1u << valid) - 1u) : 0u;   // (unused key bits ignored)
        const uint32_t L = (uint32_t)valid + (uint32_t)__popc(key);
        uint32_t tot;
        const uint32_t ex = block_excl_scan_u32(L, wsum, tot);
        if (pos + tot > dataBytes) {   // (workgroup-uniform) fewer data bytes than the key bits announce
            good = false;
            break;
        }
        const uint8_t* g0 = data + pos;
        const uint32_t mis = (uint32_t)((uintptr_t)g0 & 15u);
        const uint8_t* ga = g0 - mis;
        const uint32_t nch = (mis + tot + 15u) >> 4;
        for (uint32_t c = tid; c < nch; c += WG)
            *reinterpret_cast<uint4*>(stage + 16u * c) = *reinterpret_cast<const uint4*>(ga + 16ull * c);
        wg_lds_barrier();
        uint32_t o = mis + ex, s[8], acc = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t two = (key >> k) & 1u;
            uint32_t v = stage[o] | (two ? (uint32_t)stage[o + 1] << 8 : 0u);
            o += 1u + two;
            v = (v >> 1) ^ (0u - (v & 1u));
            acc += k < valid ? v : 0u;
            s[k] = acc;
        }
        uint32_t ttot;
        const uint32_t base = run + block_excl_scan_u32(acc, wsum, ttot);   // (its barriers also keep the next tile's staging behind these reads)
        run += ttot;
        st.put(i0, valid, base, s);
        pos += tot;
    }
    st.finish();
    st.done();
    if (tid == 0) b.result[r] = (!good || pos != dataBytes) ? E_STREAM : count * st.BYTES;
}

// the raw byte count whose 32-bit key region ((x / 4 + 3) / 4 bytes: the entropy stage's key_elem = 4) is svb16's ceil(n / 8)
__global__ __launch_bounds__(WG) void svb16_key_raw_kernel(uint32_t n, const uint32_t* raw_size, uint32_t* key_raw)
{
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = ((uint64_t)(raw_size[i] >> 1) + 7u) >> 3;
    key_raw[i] = (uint32_t)std::min<uint64_t>(16u * k, 0xFFFFFFF0ull);
}

// the first pass's windows: NORM_WINDOWS x NORM_BINS adjacent keys around key a
__device__ __forceinline__ void norm_first_windows(NormRead* sp, uint32_t a)
{
    constexpr uint32_t SPAN = NORM_WINDOWS * NORM_BINS;
    uint32_t L0 = a < SPAN / 2 ? 0u : a - SPAN / 2;
    if (L0 > 0x10000u - SPAN) L0 = 0x10000u - SPAN;
    sp->phase = NORM_VALUE;
    sp->c2 = 0;
    sp->anchored = 1;
#pragma unroll
    for (int w = 0; w < (int)NORM_WINDOWS; ++w) {
        sp->lo[w] = L0 + (uint32_t)w * NORM_BINS;
        sp->sh[w] = 0;
        sp->a[w] = 0;
        sp->z[w] = 0xFFFFu;
    }
}

// ---- normalising decode: the reads' starting windows, and the select of the large-read path --------------------------------------------
// One thread per read: the first pass's windows are NORM_WINDOWS x NORM_BINS adjacent keys around the read's first sample, which the
// stream's first control and data bytes give (any anchor gives the same statistics; a good one saves the later passes).  A read of no
// samples is finished here (c = w = 0).  SVB16: the stream is svb16's (one key bit per sample).
template <bool SVB16>
__device__ __forceinline__ void norm_init_read(const ReadBatch& b, uint32_t zigzag)
{
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    if (r >= b.n_reads || read_gate(b, r, true)) return;
    const uint32_t in_size = b.src_size[r], out_size = b.dst_cap[r];
    if (out_size & 1u) return;
    const uint32_t T = out_size >> 1, keyLen = SVB16 ? (T + 7u) >> 3 : (T + 3u) >> 2;
    NormRead* sp = b.sig.norm.st + r;
    if (T == 0) {
        norm_finish(b, r, 0.0, 0.0);
        sp->phase = NORM_DONE;
        return;
    }
    uint32_t a = 0x8000u;
    if (in_size >= keyLen + 2u) {
        const uint8_t* in = b.src + b.src_off[r];
        uint32_t v = in[keyLen] | ((in[0] & (SVB16 ? 1u : 3u)) ? (uint32_t)in[keyLen + 1] << 8 : 0u);
        if (zigzag) v = (v >> 1) ^ (0u - (v & 1u));
        a = (v ^ b.sig.bias ^ 0x8000u) & 0xFFFFu;
    }
    norm_first_windows(sp, a);
}
__global__ __launch_bounds__(WG) void norm_init_kernel(ReadBatch b, uint32_t zigzag) { norm_init_read<false>(b, zigzag); }
__global__ __launch_bounds__(WG) void norm_init16_kernel(ReadBatch b) { norm_init_read<true>(b, 1u); }

// one workgroup per read: the counts the segments added to the read's slab (zeroed again for the next pass) -> the select
template <bool RANGED>
__device__ __forceinline__ void norm_select_read(const ReadBatch& b)
{
    const uint32_t r = blockIdx.x;
    if (read_gate(b, r, true)) return;
    const uint32_t out_size = b.dst_cap[r];
    if ((out_size & 1u) || out_size == 0 || b.sig.norm.st[r].phase == NORM_DONE) return;
    uint32_t T = out_size >> 1;
    if (RANGED) {   // the ranks are the range's
        uint32_t rb, re;
        sample_range(b.sig, r, T, &rb, &re);
        T = re - rb;
        if (T == 0) {   // (nothing was counted: c = w = 0, and the slab is zero as it was)
            if (threadIdx.x == 0) {
                norm_finish(b, r, 0.0, 0.0);
                b.sig.norm.st[r].phase = NORM_DONE;
            }
            return;
        }
    }
    NormLds* L = norm_lds();
    uint32_t* slab = b.sig.norm.slab + (size_t)r * NORM_SLAB;
    for (uint32_t i = threadIdx.x; i < NORM_WINDOWS * NORM_BINS; i += WG) {
        L->h[i] = slab[i];
        slab[i] = 0;
    }
    if (threadIdx.x < NORM_WINDOWS) {
        L->below[threadIdx.x] = slab[NORM_WINDOWS * NORM_BINS + threadIdx.x];
        slab[NORM_WINDOWS * NORM_BINS + threadIdx.x] = 0;
    }
    __syncthreads();
    norm_select(L, b, r, T, b.sig.bias ^ 0x8000u);
}
__global__ __launch_bounds__(WG) void norm_select_kernel(ReadBatch b) { norm_select_read<false>(b); }
__global__ __launch_bounds__(WG) void norm_select_range_kernel(ReadBatch b) { norm_select_read<true>(b); }

// ---- POD5 reads of several rows (vbz_kernels.h Pod5Reads) ----------------------------------------------------------------
// The batch's entries stay rows, one workgroup each in the store pass; the plan below tells every row where it lies in its read, and the
// chunk store and the counting passes then reason about the read: its T samples, its chunks, its constants.
__global__ __launch_bounds__(WG) void pod5_reads_check_kernel(uint32_t n_rows, Pod5Reads pr)
{
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i > pr.n_reads) return;
    const uint32_t v = pr.first_row[i];
    if ((i == 0 && v != 0) || (i == pr.n_reads ? v != n_rows : v > pr.first_row[i + 1])) *pr.bad = 1u;
}
__global__ __launch_bounds__(WG) void pod5_reads_bad_kernel(Pod5Reads pr, uint32_t* out)
{
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < pr.n_reads && *pr.bad) out[i] = E_INPUT_SIZE;
}
__global__ __launch_bounds__(WG) void pod5_read_samples_kernel(Pod5Reads pr, const uint32_t* row_samples, uint32_t* read_samples)
{
    const uint32_t k = blockIdx.x * WG + threadIdx.x;
    if (k >= pr.n_reads || *pr.bad) return;
    uint64_t T = 0;
    for (uint32_t j = pr.first_row[k]; j < pr.first_row[k + 1]; ++j) T += row_samples[j];
    read_samples[k] = T >> 31 ? E_DESTINATION_SIZE : (uint32_t)T;
}

// One thread per row and per read.  A bad table closes every row's gate with E_INPUT_SIZE (its result too) and nothing else happens.  Otherwise the read's
// thread walks its rows: their places (Pod5Row), T, the chunk check (chunk_first is untrusted; 2^31 samples and more fail too) -- a read
// that fails closes its rows' gates with E_DESTINATION_SIZE -- and the read's constants: the given ones, or (a normalising call) the
// first pass's windows around the first sample of its first row that has one.
// RANGED: the read's clamped range goes to pr.range, the chunk check is against the range's chunks, and the element-wise flag is about the
// row that holds the range's last sample (rows lie at s0 - b of the range's signal).
// WINDOWS (b.sig.wfirst; b.sig.row is NULL): the check is the first half of the window check -- the read's two entries of wfirst are rows of
// the arena; window_sorted_kernel looks at the starts behind this launch.
template <bool RANGED, bool WINDOWS = false>
__device__ __forceinline__ void pod5_reads_plan(const ReadBatch& b, const Pod5Reads& pr, const float* offset, const float* scale, uint64_t chunk_rows)
{
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    uint32_t* gate = const_cast<uint32_t*>(b.gate);
    if (*pr.bad) {
        if (i < b.n_reads) {
            gate[i] = b.result[i] = E_INPUT_SIZE;
            pr.rows[i] = Pod5Row{ 0u, 0u, 0u, 0u };
        }
        return;
    }
    if (i >= pr.n_reads) return;
    const uint32_t first = pr.first_row[i], end = pr.first_row[i + 1];
    uint64_t T64 = 0;
    uint32_t last_s0 = 0;   // where the last row that has samples begins
    for (uint32_t j = first; j < end; ++j) {
        const uint32_t n = b.dst_cap[j] >> 1;
        pr.rows[j] = Pod5Row{ (uint32_t)T64, i, j + 1u == end && b.sig.row ? POD5_ROW_PAD : 0u, 0u };
        if (n) last_s0 = (uint32_t)T64;
        T64 += n;
    }
    const uint32_t T = (uint32_t)T64;
    bool fail = (T64 >> 31) != 0;
    uint32_t rb = 0, re = T;
    if (RANGED && !fail) {
        sample_range(b.sig, i, T, &rb, &re);
        pr.range[i] = make_uint2(rb, re);
        last_s0 = 0;
        for (uint32_t j = first; j < end; ++j)   // the row that holds sample e - 1
            if (pr.rows[j].s0 < re && (b.dst_cap[j] >> 1) != 0) last_s0 = pr.rows[j].s0 - rb;
    }
    uint64_t c0 = 0;
    if constexpr (WINDOWS) {
        if (!fail) {
            c0 = b.sig.wfirst[i];
            const uint64_t c1 = b.sig.wfirst[i + 1];
            fail = c0 > c1 || c1 > b.sig.wrows || c1 - c0 > WINDOW_READ_ROWS_MAX;
        }
    } else if (b.sig.row && !fail) {
        c0 = b.sig.row[i];
        const uint64_t c1 = b.sig.row[i + 1];
        fail = c0 > c1 || c1 > chunk_rows || c1 - c0 != chunk_count(re - rb, b.sig.chunk_len, b.sig.step);
    }
    if (fail) {
        for (uint32_t j = first; j < end; ++j) {
            gate[j] = E_DESTINATION_SIZE;
            pr.rows[j].flags = 0;
        }
        if (RANGED) pr.range[i] = make_uint2(0u, 0u);
        pr.reads[i] = Pod5Read{ 0u, POD5_READ_FAIL, 0ull };
        if (b.sig.norm.st) b.sig.norm.st[i].phase = NORM_DONE;
        return;
    }
    pr.reads[i] = Pod5Read{ T, (last_s0 & 7u) ? POD5_READ_PAD_ELEMS : 0u, c0 };
    if (!b.sig.norm.st) {
        if (b.sig.cal) const_cast<float2*>(b.sig.cal)[i] = make_float2(offset ? offset[i] : 0.0f, scale ? scale[i] : 1.0f);
        return;
    }
    NormRead* sp = b.sig.norm.st + i;
    if (T == 0) {
        norm_finish(b, i, 0.0, 0.0);
        sp->phase = NORM_DONE;
        return;
    }
    uint32_t a = 0x8000u;
    for (uint32_t j = first; j < end; ++j) {
        uint32_t in_size, n, verdict;
        if (!svb16_row_open(b, j, &in_size, &n, &verdict)) continue;
        const uint32_t K = (n + 7u) >> 3;
        if (in_size >= K + 2u) {
            const uint8_t* in = b.src + b.src_off[j];
            uint32_t v = in[K] | ((in[0] & 1u) ? (uint32_t)in[K + 1] << 8 : 0u);
            v = (v >> 1) ^ (0u - (v & 1u));
            a = (v ^ b.sig.bias ^ 0x8000u) & 0xFFFFu;
        }
        break;
    }
    norm_first_windows(sp, a);
}
__global__ __launch_bounds__(WG) void pod5_reads_plan_kernel(ReadBatch b, Pod5Reads pr, const float* offset, const float* scale, uint64_t chunk_rows)
{
    pod5_reads_plan<false>(b, pr, offset, scale, chunk_rows);
}
__global__ __launch_bounds__(WG) void pod5_reads_plan_range_kernel(ReadBatch b, Pod5Reads pr, const float* offset, const float* scale, uint64_t chunk_rows)
{
    pod5_reads_plan<true>(b, pr, offset, scale, chunk_rows);
}

__global__ __launch_bounds__(WG) void pod5_reads_plan_window_kernel(ReadBatch b, Pod5Reads pr, const float* offset, const float* scale)
{
    pod5_reads_plan<false, true>(b, pr, offset, scale, 0);
}
__global__ __launch_bounds__(WG) void pod5_reads_plan_window_range_kernel(ReadBatch b, Pod5Reads pr, const float* offset, const float* scale)
{
    pod5_reads_plan<true, true>(b, pr, offset, scale, 0);
}

// the window store of a row of a read, from the plan: the row's samples lie at s0 of the read's signal
template <int OUT>
__device__ __forceinline__ WindowStore<OUT, true> row_window_store(const ReadBatch& b, const Pod5Reads& pr, const Pod5Row& rw)
{
    WindowStore<OUT, true> st;
    uint32_t rb = 0, rend = pr.reads[rw.read].T;
    if (OUT & SIG_RANGE) {
        const uint2 g = pr.range[rw.read];
        rb = g.x;
        rend = g.y;
    }
    st.wk = window_constants<OUT>(b, rw.read, rb, rend);
    st.sk = sig_constants(b, rw.read);
    st.s0 = rw.s0;
    return st;
}

// the event sink of a row of a read, from the plan: the row's samples lie at s0 of the read's signal
template <int OUT>
__device__ __forceinline__ EventStore row_event_store(const ReadBatch& b, const Pod5Reads& pr, const Pod5Row& rw)
{
    uint32_t rb = 0, rend = pr.reads[rw.read].T;
    if (OUT & SIG_RANGE) {
        const uint2 g = pr.range[rw.read];
        rb = g.x;
        rend = g.y;
    }
    EventStore st{ event_constants(b, rw.read, rb, rend) };
    st.begin_row(rw.s0);
    return st;
}

// Signal events (SignalOut::events), the two launches around the event pass: one thread per row of a read that passed the event check.
// scan: the exclusive scan of the passing reads' row counts (launch_window_check), which says whose row the j-th is; a read the sorted
// pass closed behind the scan (its gate; POD5: POD5_READ_FAIL) is passed over, so not one byte of its rows is written.
// *rb, *re: the signal of read i (its clamped range); false: the read is closed
__device__ __forceinline__ bool event_read_open(const ReadBatch& b, const Pod5Reads& pr, uint32_t i, uint32_t* rb, uint32_t* re)
{
    if (pr.reads) {
        if (pr.reads[i].flags & POD5_READ_FAIL) return false;
        *rb = 0;
        *re = pr.reads[i].T;
        if (b.sig.ranged()) {
            const uint2 g = pr.range[i];
            *rb = g.x;
            *re = g.y;
        }
        return true;
    }
    if (read_gate(b, i, false)) return false;
    sample_range(b.sig, i, b.dst_cap[i] >> 1, rb, re);
    return true;
}

__global__ __launch_bounds__(WG) void event_zero_kernel(ReadBatch b, Pod5Reads pr, const uint64_t* scan)
{
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    const uint64_t total = scan[n];
    for (uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x; j < total; j += (uint64_t)gridDim.x * WG) {
        const uint32_t i = scan_find(scan, n, j);
        uint32_t rb, re;
        if (!event_read_open(b, pr, i, &rb, &re)) continue;
        const uint64_t c = b.sig.wfirst[i] + (j - scan[i]);
        *reinterpret_cast<uint4*>(b.sig.event_moments(b.dst) + 2ull * c) = make_uint4(0u, 0u, 0u, 0u);
    }
}

// The record of an event of cnt >= 1 samples from its exact moments: m = S1 / n, v = S2 / n - m m clamped at 0, r = sqrt(v),
// mean = float32((m + o) s), sd = float32(r |s|) -- float64, every operation rounded once.  Contraction is off for this body: the
// _rn intrinsics of this compiler are the plain operators, and m m would be fused into the subtraction (one rounding less than numpy's;
// one sd in a few million then rounds the other way to float32).  The device's sqrt(double) is correctly rounded.
__device__ __forceinline__ void event_record(long long S1, unsigned long long S2, uint32_t cnt, float o, float s, float* mean, float* sd)
{
#pragma clang fp contract(off)
    const double nd = (double)cnt;
    const double m = (double)S1 / nd;
    const double q = (double)S2 / nd;
    const double mm = m * m;
    double v = q - mm;
    if (v < 0.0) v = 0.0;
    const double t = m + (double)o;
    *mean = __double2float_rn(t * (double)s);
    *sd = __double2float_rn(__dsqrt_rn(v) * fabs((double)s));
}

// The records of the rows (include/vbz_gpu.h: vbz_gpu_event): n = z - a from the starts and the signal's length alone, the rest by
// event_record.  One 16-byte store per row.
__global__ __launch_bounds__(WG) void event_finish_kernel(ReadBatch b, Pod5Reads pr, const float* offset, const float* scale, const uint64_t* scan, uint4* out)
{
    const unsigned long long* mom = b.sig.event_moments(b.dst);
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    const uint64_t total = scan[n];
    const uint32_t* start = reinterpret_cast<const uint32_t*>(b.sig.wstart);
    for (uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x; j < total; j += (uint64_t)gridDim.x * WG) {
        const uint32_t i = scan_find(scan, n, j);
        uint32_t rb, re;
        if (!event_read_open(b, pr, i, &rb, &re)) continue;
        const uint32_t T = re - rb;
        const uint64_t c = b.sig.wfirst[i] + (j - scan[i]);
        const uint32_t a0 = start[c], a = a0 < T ? a0 : T;
        uint32_t z = T;
        if (j + 1 < scan[i + 1]) {   // (not the read's last row)
            const uint32_t z0 = start[c + 1];
            z = z0 < T ? z0 : T;
        }
        const uint32_t cnt = z - a;   // (sorted starts: z >= a)
        float o = offset ? offset[i] : 0.0f, s = scale ? scale[i] : 1.0f;
        if (b.sig.norm.st) {   // the read's own statistics: the store's constants as norm_finish makes them
            const float2 ss = b.sig.norm.ss[i];
            o = -ss.x;
            s = __double2float_rn(__ddiv_rn(1.0, (double)ss.y));
        }
        float mean = 0.0f, sd = 0.0f;
        if (cnt != 0) event_record((long long)mom[2ull * c], mom[2ull * c + 1u], cnt, o, s, &mean, &sd);
        out[c] = make_uint4(__float_as_uint(mean), __float_as_uint(sd), cnt, 0u);
    }
}

// The pad of the windows (SignalOut::wfirst), behind the window check and independent of the decode: one wavefront per row of a read that
// passed.  scan: the exclusive scan of the passing reads' row counts (launch_window_check), which says whose row the j-th is.  Row c of a
// signal of T samples: positions p with start[c] + p < 0 or start[c] + p >= T take the pad value -- exactly the positions no sample
// store writes -- element by element up to the next line boundary and in whole lines beyond.  pr.reads (a call over POD5 reads): b's
// entries are rows, the reads' samples and ranges are the plan's, and a read that failed has no row in `scan`.
__global__ __launch_bounds__(WG) void window_pad_kernel(ReadBatch b, Pod5Reads pr, const uint64_t* scan)
{
    const bool reads = pr.reads != nullptr;
    const uint32_t n = reads ? pr.n_reads : b.n_reads, lane = threadIdx.x & 63u;
    const uint32_t OB = b.sig.type == SIG_F32 ? 4u : 2u, L = b.sig.chunk_len;
    const uint32_t padw = b.sig.type == SIG_F32   ? __float_as_uint(b.sig.pad)
                          : b.sig.type == SIG_F16 ? sig_pack2<SIG_F16>(b.sig.pad, b.sig.pad) & 0xFFFFu
                                                  : sig_pack2<SIG_BF16>(b.sig.pad, b.sig.pad) & 0xFFFFu;
    const uint4 line = OB == 4 ? make_uint4(padw, padw, padw, padw) : make_uint4(padw * 0x10001u, padw * 0x10001u, padw * 0x10001u, padw * 0x10001u);
    const uint64_t total = scan[n], waves = (uint64_t)gridDim.x * (WG / 64);
    for (uint64_t j = (uint64_t)blockIdx.x * (WG / 64) + (threadIdx.x >> 6); j < total; j += waves) {
        const uint32_t i = scan_find(scan, n, j);
        uint32_t rb = 0, re = 0;
        if (reads) {
            if (pr.reads[i].flags & POD5_READ_FAIL) continue;   // (the starts decreased)
            re = pr.reads[i].T;
            if (b.sig.ranged()) {
                const uint2 g = pr.range[i];
                rb = g.x;
                re = g.y;
            }
        } else {
            if (read_gate(b, i, false)) continue;
            sample_range(b.sig, i, b.dst_cap[i] >> 1, &rb, &re);
        }
        const uint64_t c = b.sig.wfirst[i] + (j - scan[i]);
        const int64_t st = b.sig.wstart[c], T = (int64_t)(re - rb);
        const uint32_t f = st >= 0 ? 0u : (-st < (int64_t)L ? (uint32_t)(-st) : L);                 // positions [0, f) lie in front of the signal
        const uint32_t g = T - st <= 0 ? 0u : (T - st < (int64_t)L ? (uint32_t)(T - st) : L);       // ... and [g, L) behind it (g >= f)
        uint8_t* row = b.dst + c * ((uint64_t)L * OB);
        auto put = [&](uint32_t m, uint32_t p0, uint32_t p1) {   // positions [p0, p1) of line m
            uint8_t* q = row + (size_t)m * 8u * OB;
            if (p1 - p0 == 8u) {
                *reinterpret_cast<uint4*>(q) = line;
                if (OB == 4) *reinterpret_cast<uint4*>(q + 16) = line;
            } else {
                for (uint32_t p = p0; p < p1; ++p) {
                    if (OB == 4) reinterpret_cast<uint32_t*>(q)[p] = padw;
                    else reinterpret_cast<uint16_t*>(q)[p] = (uint16_t)padw;
                }
            }
        };
        for (uint32_t m = lane; m < (f + 7u) >> 3; m += 64u) put(m, 0u, f - 8u * m < 8u ? f - 8u * m : 8u);
        for (uint32_t m = (g >> 3) + lane; m < (L >> 3); m += 64u) put(m, g > 8u * m ? g - 8u * m : 0u, 8u);
    }
}

// the chunk store of row r of a read, from the plan: the row's `count` samples lie at s0 of the read's signal
template <int OUT>
__device__ __forceinline__ ChunkStore<OUT, true> row_chunk_store(const ReadBatch& b, const Pod5Reads& pr, const Pod5Row& rw, uint32_t count)
{
    ChunkStore<OUT, true> st;
    const Pod5Read rd = pr.reads[rw.read];
    st.rend = rd.T;
    if (OUT & SIG_RANGE) {   // (the chunking is the range's)
        const uint2 g = pr.range[rw.read];
        st.rb = g.x;
        st.rend = g.y;
    }
    st.ck = chunk_constants<OUT>(b, st.rend - st.rb, rd.row);
    st.sk = sig_constants(b, rw.read);
    st.s0 = rw.s0;
    st.re = rw.s0 + count;
    st.pad_elems = (rd.flags & POD5_READ_PAD_ELEMS) != 0;
    return st;
}

// the sink of row r of a read: its window or chunk sink from the plan, or the typed sink of the row's slot with its read's constants
template <int OUT>
__device__ __forceinline__ auto row_store(const ReadBatch& b, const Pod5Reads& pr, const Pod5Row& rw, uint32_t r, uint32_t count)
{
    if constexpr ((OUT & SIG_EVENT) != 0) return row_event_store<OUT>(b, pr, rw);
    else if constexpr ((OUT & SIG_WINDOW) != 0) return row_window_store<OUT>(b, pr, rw);
    else if constexpr ((OUT & SIG_CHUNK) != 0) return row_chunk_store<OUT>(b, pr, rw, count);
    else return dec_store<2, OUT>(b.dst, b.dst_off, &b, r, count, rw.read);
}

// The store pass over reads: one workgroup per row, OUT a typed, a chunk or a window sink.  The read's pad positions are written here, once, by
// the workgroup of its last row -- before anything can send that workgroup home (an empty row, a closed gate, a failed stream).
template <int OUT>
__global__ __launch_bounds__(WG) void svb16_decode_rows_kernel(ReadBatch b, Pod5Reads pr)
{
    const Svb16Lds lds;

    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const Pod5Row rw = pr.rows[r];
    if ((OUT & SIG_CHUNK) && !(OUT & SIG_WINDOW) && (rw.flags & POD5_ROW_PAD)) row_chunk_store<OUT>(b, pr, rw, 0u).finish();
    uint32_t in_size = 0, count = 0, verdict;
    if (!svb16_row_open(b, r, &in_size, &count, &verdict)) return read_closed(b, r, verdict);
    const uint8_t* in = b.src + b.src_off[r];
    const auto st = row_store<OUT>(b, pr, rw, r, count);
    const bool good = svb16_decode_row(in, in_size, count, st, lds.stage, lds.wsum);
    if (tid == 0) b.result[r] = good ? count * st.BYTES : E_STREAM;
}

// ---- a POD5 read of several rows on one workgroup: what every kernel that walks a read's rows in turn is made of ---------------------------
// The rows [first, end) of a read through one sink, by the read's workgroup: the delta chain and the data position restart with every
// row, begin_row() places each in the read's signal and the sink's state carries on.  verdicts: every row's result is written here, the
// int16 decode's.  PREFIX (the trim pass): only the read's first `stop` samples are walked, up to the row that holds the last of them.
template <bool PREFIX = false, class Store>
__device__ __forceinline__ void svb16_walk_rows(const ReadBatch& b, const Pod5Reads& pr, uint32_t first, uint32_t end, Store& st, const Svb16Lds& lds,
                                                bool verdicts, uint32_t stop = 0)
{
    for (uint32_t r = first; r < end; ++r) {
        if constexpr (PREFIX)
            if (pr.rows[r].s0 >= stop) break;
        uint32_t in_size = 0, count = 0, verdict;
        if (!svb16_row_open(b, r, &in_size, &count, &verdict)) {   // (a closed gate, a failed stage, a refused size, an empty row)
            if (verdicts) read_closed(b, r, verdict);
            continue;
        }
        const uint32_t s0 = pr.rows[r].s0;
        st.begin_row(s0);   // (put() gets positions in the row)
        const bool good = svb16_decode_row<PREFIX>(b.src + b.src_off[r], in_size, count, st, lds.stage, lds.wsum, PREFIX ? stop - s0 : 0u);
        if (verdicts && threadIdx.x == 0) b.result[r] = good ? count * 2u : E_STREAM;
    }
}

// The rows' verdicts of a read that is not walked, a row a thread: what svb16_row_open says of the row, or -- where that is no error and
// `instead` is one (E_OOM: the read's map does not fit) -- `instead`
__device__ __forceinline__ void svb16_rows_closed(const ReadBatch& b, uint32_t first, uint32_t end, uint32_t instead)
{
    for (uint32_t r = first + threadIdx.x; r < end; r += WG) {
        uint32_t in_size, count, verdict;
        (void)svb16_row_open(b, r, &in_size, &count, &verdict);
        if (verdict != GATE_SKIP) b.result[r] = instead == 0 || verdict >= E_FIRST ? verdict : instead;
    }
}

// whether a row of the read has an error verdict in result[] (a pass behind the counting passes, which left them), by the read's workgroup
__device__ __forceinline__ bool svb16_rows_failed(const ReadBatch& b, uint32_t first, uint32_t end)
{
    int failed = 0;
    for (uint32_t r = first + threadIdx.x; r < end; r += WG) failed |= b.result[r] >= E_FIRST ? 1 : 0;
    return __syncthreads_or(failed) != 0;
}

// the samples [*rb, *re) of read k of T samples that a ranged call takes (the plan has clamped them), else all
__device__ __forceinline__ void pod5_read_range(const ReadBatch& b, const Pod5Reads& pr, uint32_t k, uint32_t T, uint32_t* rb, uint32_t* re)
{
    *rb = 0;
    *re = T;
    if (b.sig.ranged()) {
        const uint2 g = pr.range[k];
        *rb = g.x;
        *re = g.y;
    }
}

// A counting pass over reads: one workgroup per read walks its rows in turn -- the bins and the below-counts carry on from row to row --
// and selects with the read's histogram in LDS.  verdicts != 0 (the first pass of the statistics alone, which has no store pass): every
// row's result is written here.
template <int OUT>
__device__ __forceinline__ void svb16_count_reads(const ReadBatch& b, const Pod5Reads& pr, uint32_t verdicts)
{
    const Svb16Lds lds;

    if (*pr.bad) return;
    const uint32_t k = blockIdx.x;
    const uint32_t first = pr.first_row[k], end = pr.first_row[k + 1];
    if (b.sig.norm.st[k].phase == NORM_DONE) {   // finished (no sample, or failed): no row of it has samples to walk
        if (verdicts) svb16_rows_closed(b, first, end, 0u);
        return;
    }
    DecStore<2, OUT> st = dec_store<2, OUT>(nullptr, nullptr, &b, k, pr.reads[k].T);
    svb16_walk_rows(b, pr, first, end, st, lds, verdicts != 0);
    st.done();
}
__global__ __launch_bounds__(WG) void svb16_count_reads_kernel(ReadBatch b, Pod5Reads pr, uint32_t verdicts)
{
    svb16_count_reads<SIG_COUNT>(b, pr, verdicts);
}
__global__ __launch_bounds__(WG) void svb16_count_reads_range_kernel(ReadBatch b, Pod5Reads pr, uint32_t verdicts)
{
    svb16_count_reads<SIG_COUNT | SIG_RANGE>(b, pr, verdicts);
}

// ---- the signal passes behind the decoder: trim, spans, segmentation (DESIGN.md 4.27 has the table of walks and passes) -------------------
// TrimStore, SpanStore and SegmentStore store no sample and ride the decoder's walks.  Every stream form has ONE walk below, a function
// template over a pass policy, and every kernel is a thin instantiation of it: svb_pass_read (one workgroup per int16 read),
// svb_pass_segment (a segment of a large read: trim and spans), svb16_pass_row (a POD5 row as a read), svb16_pass_reads (a POD5 read of
// several rows).  A policy is a plain struct around the pass's *Out, a kernel argument by value, and says only what differs, in constants
// and inlined members, so that no pass pays for another's option: owes() -- whether this launch writes the int16 decode's verdicts;
// closed() -- a read whose stream was not opened; admit() / admit_rows() / admit_segment() -- whether an opened read (a POD5 read's rows,
// a segment) is walked, and its state, else what it gets instead is written; end() -- where the walk ends; sink<SHARED>() -- the sink
// from that state (SHARED: rows may begin inside a map byte); WAVES -- the one-workgroup int16 kernel's second launch bound (0: none).
// The sinks' done() is svb_decode_range's to call on the int16 walks and the walk's on the POD5 ones (SpanStore's is empty).  Every begin
// entry and every byte of a map has one writer: the read's workgroup, or on the large-read path the lanes that own whole bytes (spans)
// and trim_select_kernel (trim).

// begin 0: a read with an error verdict (entry: trim_state's)
__device__ __forceinline__ void trim_zero(const ReadBatch& b, const TrimOut& tr, uint32_t r)
{
    if (threadIdx.x == 0) tr.begin[b.sig.norm.map ? b.sig.norm.map[r] : r] = 0;
}
// the state of read r of T samples that has no error; a read with no window gets begin = min(t0, T) and false
__device__ __forceinline__ bool trim_windows(const ReadBatch& b, const TrimOut& tr, uint32_t r, uint32_t T, TrimK* k)
{
    *k = trim_state(b, tr, r, T);
    if (k->nW != 0) return true;
    if (threadIdx.x == 0) *k->out = k->t0 < k->T ? k->t0 : k->T;
    return false;
}

// The trim pass (OUT = SIG_TRIM), behind the last counting pass: it reads result[] and walks only the prefix [0, t0 + nW W) of every read
// that has no error -- whatever its NormRead::phase.
struct TrimPass
{
    using Read = TrimK;
    static constexpr int WAVES = VBZ_SVBDEC_WAVES;
    static constexpr bool PREFIX = true, ZEROED_MAP = false, SEG_VERDICT = false;
    TrimOut out;
    __device__ static constexpr bool owes() { return false; }
    __device__ __forceinline__ void closed(const ReadBatch& b, uint32_t r, uint32_t verdict) const
    {
        if (verdict != GATE_SKIP) trim_zero(b, out, r);   // (another launch group's read: nothing is written)
    }
    __device__ __forceinline__ bool admit(const ReadBatch& b, uint32_t r, uint32_t T, TrimK* k) const
    {
        if (b.result[r] < E_FIRST) return trim_windows(b, out, r, T, k);
        trim_zero(b, out, r);
        return false;
    }
    // (a read with a failing row gets 0)
    __device__ __forceinline__ bool admit_rows(const ReadBatch& b, const Pod5Reads&, uint32_t q, uint32_t first, uint32_t end, const Pod5Read& rd,
                                               TrimK* k) const
    {
        if (!svb16_rows_failed(b, first, end)) return trim_windows(b, out, q, rd.T, k);
        trim_zero(b, out, q);
        return false;
    }
    // (trim_select_kernel writes the read's 0 or min(t0, T), and scans the words the segments add to the read's slab)
    template <bool SELF>
    __device__ __forceinline__ bool admit_segment(const ReadBatch& b, uint32_t r, uint32_t, bool open, const SvbRead& rd, uint32_t, uint64_t,
                                                  TrimK* k) const
    {
        if (!open || b.result[r] >= E_FIRST) return false;
        *k = trim_state(b, out, r, rd.count);
        k->slab = b.sig.norm.slab + (size_t)r * NORM_SLAB;
        return true;
    }
    __device__ static uint32_t end(const TrimK& k, uint32_t) { return k.end; }
    template <bool SHARED>
    __device__ __forceinline__ TrimStore sink(const ReadBatch&, uint32_t, const TrimK& k) const { return TrimStore(k); }
};

// The two passes that leave a bit per position in the read's map (vbz_kernels.h ReadMaps): what they share.  Unlike the trim they walk
// every read to its end -- every byte of the map gets its writer.
struct MapRead
{
    uint32_t i, rb, re;   // the read's entry of the call's tables; its samples [rb, re)
};
template <class P>
struct MapPass
{
    using Read = MapRead;
    static constexpr bool PREFIX = false, SEG_VERDICT = true;
    __device__ __forceinline__ const P& self() const { return static_cast<const P&>(*this); }
    __device__ __forceinline__ void closed(const ReadBatch& b, uint32_t r, uint32_t verdict) const
    {
        if (self().owes()) read_closed(b, r, verdict);
    }
    __device__ __forceinline__ bool admit(const ReadBatch& b, uint32_t r, uint32_t T, MapRead* w) const
    {
        if (!self().owes() && b.result[r] >= E_FIRST) return false;
        w->i = self().out.entry(r);
        if (!self().out.fits(w->i, T)) {
            if (threadIdx.x == 0) b.result[r] = E_OOM;
            return false;
        }
        sample_range(b.sig, r, T, &w->rb, &w->re);
        return true;
    }
    // (a read the plan failed has its rows' gates closed: every row has or gets that verdict; a read with a failing row is not walked)
    __device__ __forceinline__ bool admit_rows(const ReadBatch& b, const Pod5Reads& pr, uint32_t k, uint32_t first, uint32_t end, const Pod5Read& rd,
                                               MapRead* w) const
    {
        const bool failed = (rd.flags & POD5_READ_FAIL) != 0, fits = self().out.fits(k, rd.T);
        if (failed || !fits) {
            if (self().owes() || !fits) svb16_rows_closed(b, first, end, failed ? 0u : E_OOM);
            return false;
        }
        if (!self().owes() && svb16_rows_failed(b, first, end)) return false;
        w->i = k;
        pod5_read_range(b, pr, k, rd.T, &w->rb, &w->re);
        return true;
    }
    // The read's verdict is svb_seg_decode_kernel's MODE 0: the scan launch's, or (SELF) written by the read's first workgroup from the
    // data bytes its segments announce (total).
    template <bool SELF>
    __device__ __forceinline__ bool admit_segment(const ReadBatch& b, uint32_t r, uint32_t sg, bool open, const SvbRead& rd, uint32_t verdict,
                                                  uint64_t total, MapRead* w) const
    {
        w->i = self().out.entry(r);
        const bool fits = !open || self().out.fits(w->i, rd.count);
        if (sg == 0 && threadIdx.x == 0) {   // the read's verdict: one writer
            uint32_t res0;
            if (!fits) b.result[r] = E_OOM;
            else if (SELF && svb_seg_read_result(open, rd, verdict, total, 2u, &res0)) b.result[r] = res0;
        }
        if (!open || !fits) return false;
        if (SELF ? total != (uint64_t)rd.dataBytes : b.result[r] >= E_FIRST) return false;   // malformed: these sums say so, or the scan (or a counting pass) did
        sample_range(b.sig, r, rd.count, &w->rb, &w->re);
        return true;
    }
    __device__ static uint32_t end(const MapRead&, uint32_t T) { return T; }
};

// The span pass (svb_store.h SpanStore), in two settings.  Behind the counting passes of a call with a normalisation (verdicts == 0) it
// owes no verdict and walks the reads that have none.  With the caller's constants no counting pass runs, and it writes them itself.
// A segment of the large-read path begins at a multiple of 16 384 samples, so its lanes own whole bytes of the map and store them plainly.
struct SpanPass : MapPass<SpanPass>
{
    static constexpr int WAVES = VBZ_SVBDEC_WAVES;
    static constexpr bool ZEROED_MAP = true;
    SpanOut out;
    uint32_t verdicts;
    __device__ bool owes() const { return verdicts != 0; }
    template <bool SHARED>
    __device__ __forceinline__ SpanStore<SHARED> sink(const ReadBatch& b, uint32_t r, const MapRead& w) const
    {
        return SpanStore<SHARED>(span_state(b, out, r, w.i, w.rb, w.re));
    }
    // a row may begin inside a map byte, so the read's workgroup zeroes the read's map and the lanes OR their bits in
    __device__ __forceinline__ void zero_map(const SpanStore<true>& st, uint32_t T) const
    {
        uint32_t* const m = reinterpret_cast<uint32_t*>(st.sk.map);
        const uint32_t words = (((T + 7u) >> 3) + 3u) >> 2;   // (map_off is a scan of sizes rounded up to 4: the words lie inside the read's map)
        for (uint32_t j = threadIdx.x; j < words; j += WG) m[j] = 0;
        __syncthreads();
    }
};

// The segmentation pass (svb_store.h SegmentStore): the sink needs each sample's neighbourhood, and a workgroup that walks the whole
// signal in order has it in LDS -- one workgroup per read on every path.  No seam lies between the rows of a POD5 read.
struct SegmentPass : MapPass<SegmentPass>
{
    static constexpr int WAVES = 0;
    static constexpr bool ZEROED_MAP = false;
    SegmentOut out;
    __device__ static constexpr bool owes() { return true; }
    template <bool SHARED>
    __device__ __forceinline__ SegmentStore sink(const ReadBatch& b, uint32_t, const MapRead& w) const
    {
        return SegmentStore(out, w.i, w.rb, w.re - w.rb, b.sig.bias);
    }
};

// one workgroup per int16 read: svb_decode_kernel's walk
template <bool ZZ, bool I16ZZ, class Pass>
__device__ __forceinline__ void svb_pass_read(const ReadBatch& b, const Pass& p)
{
    const SvbDecLds<2, I16ZZ> lds;

    const uint32_t r = blockIdx.x;
    SvbRead rd;
    uint32_t verdict;
    if (!svb_read_open<2, I16ZZ>(b, r, &rd, &verdict)) return p.closed(b, r, verdict);
    typename Pass::Read w;
    if (!p.admit(b, r, rd.count, &w)) return;
    uint64_t pos = 0;
    uint32_t run = 0;
    const auto st = p.template sink<false>(b, r, w);
    const bool good = svb_decode_range<2, ZZ, I16ZZ, 0>(rd.in, rd.in + rd.keyLen, rd.dataBytes, rd.count, 0, Pass::end(w, rd.count), pos, run, st,
                                                        lds.stage, lds.wsum);
    if (p.owes() && threadIdx.x == 0) b.result[r] = (!good || pos != rd.dataBytes) ? E_STREAM : rd.count * 2u;
}
template <bool ZZ, bool I16ZZ, class Pass>
__global__ __launch_bounds__(WG, Pass::WAVES) void svb_pass_kernel(ReadBatch b, Pass p) { svb_pass_read<ZZ, I16ZZ>(b, p); }

// Where a segment of a large read begins in the read's data bytes (pos; total: the data bytes all its segments announce, SELF only) and
// where its delta chain stands (run), as svb_seg_decode_kernel's passes left them: the SELF sums of seg_val / seg_run in front of this
// segment, else the scan launches' seg_pos[] / seg_run[].  For the pass kernels only: svb_seg_decode_kernel states the same in its own
// text and is left as it is -- its instantiations' registers move with where its read is opened and its sums are taken
// (profiles/HISTORY.md, "svb stage: one statement of how a read is opened").
struct SegAt
{
    uint64_t pos = 0, total = 0;
    uint32_t run = 0;
};
template <bool ZZ, bool SELF>
__device__ __forceinline__ SegAt seg_positions(const uint32_t* seg_first, const uint32_t* seg_val, const uint64_t* seg_pos, const uint32_t* seg_run,
                                               uint32_t r, uint64_t* sums_s)
{
    SegAt at;
    if (SELF) {
        seg_sums(seg_val, seg_first[r], blockIdx.x, seg_first[r + 1], sums_s, at.pos, at.total);
        if (ZZ) {
            uint64_t run = 0, all;
            seg_sums(seg_run, seg_first[r], blockIdx.x, seg_first[r + 1], sums_s, run, all);
            at.run = (uint32_t)run;
        }
    } else {
        at.pos = seg_pos[blockIdx.x];
        at.run = ZZ ? seg_run[blockIdx.x] : 0u;
    }
    return at;
}

// One segment of a large read: svb_seg_decode_kernel's MODE 0 at the positions its passes left, every segment that begins in front of
// the walk's end (the trim: most segments of a long read lie behind the prefix and return at once; the others add their words to the
// read's slab).
template <bool ZZ, bool I16ZZ, bool SELF, class Pass>
__device__ __forceinline__ void svb_pass_segment(const ReadBatch& b, const uint32_t* seg_first, const uint32_t* seg_val, const uint64_t* seg_pos,
                                                 const uint32_t* seg_run, const Pass& p)
{
    constexpr uint32_t SEG = WG * Vpl<2>::value * SEG_TILES;
    const SvbDecLds<2, I16ZZ> lds;
    __shared__ uint64_t sums_s[8];
    uint32_t r, sg;
    if (!seg_locate(seg_first, b.n_reads, blockIdx.x, r, sg)) return;
    SvbRead rd;
    uint32_t verdict;
    const bool open = svb_read_open<2, I16ZZ>(b, r, &rd, &verdict);
    SegAt at;
    if constexpr (Pass::SEG_VERDICT) at = seg_positions<ZZ, SELF>(seg_first, seg_val, seg_pos, seg_run, r, sums_s);   // (in front of every return: the read's verdict takes the total)
    typename Pass::Read w;
    if (!p.template admit_segment<SELF>(b, r, sg, open, rd, verdict, at.total, &w)) return;
    const uint32_t first = sg * SEG, lim = Pass::end(w, rd.count);
    if (first >= lim) return;
    if constexpr (!Pass::SEG_VERDICT) at = seg_positions<ZZ, SELF>(seg_first, seg_val, seg_pos, seg_run, r, sums_s);   // (behind them: no sums for a segment that walks nothing)
    const auto st = p.template sink<false>(b, r, w);
    (void)svb_decode_range<2, ZZ, I16ZZ, 0>(rd.in, rd.in + rd.keyLen, rd.dataBytes, rd.count, first, lim - first > SEG ? first + SEG : lim, at.pos,
                                            at.run, st, lds.stage, lds.wsum);
}
template <bool ZZ, bool I16ZZ, bool SELF, class Pass>
__global__ __launch_bounds__(WG) void svb_seg_pass_kernel(ReadBatch b, const uint32_t* seg_first, const uint32_t* seg_val, const uint64_t* seg_pos,
                                                          const uint32_t* seg_run, Pass p)
{
    svb_pass_segment<ZZ, I16ZZ, SELF>(b, seg_first, seg_val, seg_pos, seg_run, p);
}

// Read r of a trim launch's select, by the whole workgroup: false when there is nothing to scan -- the read is another launch group's
// (nothing is written), it has an error verdict (begin 0) or no window (begin min(t0, T)); else *k is its state.
__device__ __forceinline__ bool trim_read_open(const ReadBatch& b, const TrimOut& tr, uint32_t r, TrimK* k)
{
    const uint32_t g = read_gate(b, r, true);
    if (g == GATE_SKIP) return false;
    if (g || b.result[r] >= E_FIRST) {
        trim_zero(b, tr, r);
        return false;
    }
    return trim_windows(b, tr, r, b.dst_cap[r] >> 1, k);
}

// one workgroup per read of the large-read path: the words the segments added to the read's slab (zeroed again) -> the scan
__global__ __launch_bounds__(WG) void trim_select_kernel(ReadBatch b, TrimOut tr)
{
    const uint32_t r = blockIdx.x;
    TrimK k;
    if (!trim_read_open(b, tr, r, &k)) return;
    NormLds* L = norm_lds();
    uint32_t* slab = b.sig.norm.slab + (size_t)r * NORM_SLAB;
    for (uint32_t i = threadIdx.x; i < k.nW; i += WG) {
        L->h[i] = slab[i];
        slab[i] = 0;
    }
    __syncthreads();
    if (threadIdx.x < 64) trim_scan(L->h, k);
}

// a POD5 row as a read of its own
template <class Pass>
__device__ __forceinline__ void svb16_pass_row(const ReadBatch& b, const Pass& p)
{
    const Svb16Lds lds;

    const uint32_t r = blockIdx.x;
    uint32_t in_size = 0, count = 0, verdict;
    if (!svb16_row_open(b, r, &in_size, &count, &verdict)) return p.closed(b, r, verdict);
    typename Pass::Read w;
    if (!p.admit(b, r, count, &w)) return;
    const auto st = p.template sink<false>(b, r, w);
    const bool good = svb16_decode_row<Pass::PREFIX>(b.src + b.src_off[r], in_size, count, st, lds.stage, lds.wsum, Pass::end(w, count));
    st.done();
    if (p.owes() && threadIdx.x == 0) b.result[r] = good ? count * 2u : E_STREAM;
}
template <class Pass>
__global__ __launch_bounds__(WG) void svb16_pass_kernel(ReadBatch b, Pass p) { svb16_pass_row(b, p); }

// POD5 reads of several rows: one workgroup per READ walks its rows in turn, as svb16_count_reads does (and writes their verdicts where
// the pass owes them).  A bad first_row leaves everything alone.
template <class Pass>
__device__ __forceinline__ void svb16_pass_reads(const ReadBatch& b, const Pod5Reads& pr, const Pass& p)
{
    const Svb16Lds lds;

    if (*pr.bad) return;
    const uint32_t k = blockIdx.x;
    const uint32_t first = pr.first_row[k], end = pr.first_row[k + 1];
    const Pod5Read rd = pr.reads[k];
    typename Pass::Read w;
    if (!p.admit_rows(b, pr, k, first, end, rd, &w)) return;
    auto st = p.template sink<true>(b, k, w);
    if constexpr (Pass::ZEROED_MAP) p.zero_map(st, rd.T);
    svb16_walk_rows<Pass::PREFIX>(b, pr, first, end, st, lds, p.owes(), Pass::end(w, rd.T));
    st.done();
}
template <class Pass>
__global__ __launch_bounds__(WG) void svb16_pass_reads_kernel(ReadBatch b, Pod5Reads pr, Pass p) { svb16_pass_reads(b, pr, p); }

// read_result[k]: the code of the read's first failing row, else T * elem
__global__ __launch_bounds__(WG) void pod5_read_results_kernel(ReadBatch b, Pod5Reads pr, uint32_t elem)
{
    const uint32_t k = blockIdx.x * WG + threadIdx.x;
    if (k >= pr.n_reads || *pr.bad) return;
    uint32_t v = pr.reads[k].T * elem;
    for (uint32_t j = pr.first_row[k]; j < pr.first_row[k + 1]; ++j) {
        if (b.result[j] >= E_FIRST) {
            v = b.result[j];
            break;
        }
    }
    pr.read_result[k] = v;
}

hipError_t launch_norm_init(const ReadBatch& b, bool zigzag, hipStream_t s)
{
    hipLaunchKernelGGL(norm_init_kernel, dim3((b.n_reads + WG - 1) / WG), dim3(WG), 0, s, b, zigzag ? 1u : 0u);
    return hipGetLastError();
}

// one workgroup per read of the batch (more: the kernel's arguments behind it, a pass policy)
template <typename K, typename... More>
hipError_t launch1(K kernel, const ReadBatch& b, hipStream_t s, const More&... more)
{
    if (b.n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3(b.n_reads), dim3(WG), 0, s, b, more...);
    return hipGetLastError();
}

// ---- the launchers' two dispatches: the element kind and the decoder's store --------------------------------------------------------
template <int V> using Int = std::integral_constant<int, V>;
template <bool V> using Bool = std::integral_constant<bool, V>;

// (integer_size, zigzag) -> f(ELEM, ZZ, I16ZZ) as compile-time tags; SMALL: sizes 1 and 4 exist (the typed and chunk stores: int16 only)
template <bool SMALL = true, class F>
hipError_t svb_dispatch_elem(int integer_size, bool zigzag, F&& f)
{
    if (integer_size == 2) return zigzag ? f(Int<2>{}, Bool<true>{}, Bool<true>{}) : f(Int<2>{}, Bool<false>{}, Bool<false>{});
    if constexpr (SMALL) {
        if (integer_size == 4) return zigzag ? f(Int<4>{}, Bool<true>{}, Bool<false>{}) : f(Int<4>{}, Bool<false>{}, Bool<false>{});
        if (integer_size == 1) return zigzag ? f(Int<1>{}, Bool<true>{}, Bool<false>{}) : f(Int<1>{}, Bool<false>{}, Bool<false>{});
    }
    return hipErrorInvalidValue;
}

// b.sig's store -> f(OUT): OUT = b.sig.type, | SIG_CHUNK with chunk rows, | SIG_CHUNK | SIG_WINDOW with window rows, | SIG_RANGE with range
// tables (DecStore; chunk and window stores only); an event call: SIG_EVENT [| SIG_RANGE], whatever the type
template <class F>
hipError_t svb_dispatch_store(const ReadBatch& b, F&& f)
{
    constexpr uint32_t WIN = SIG_CHUNK | SIG_WINDOW;
    if (b.sig.events) return b.sig.ranged() ? f(Int<SIG_EVENT | SIG_RANGE>{}) : f(Int<SIG_EVENT>{});   // (an event call: no sample is stored)
    switch (b.sig.type == SIG_NONE ? SIG_NONE : b.sig.type | (b.sig.row ? SIG_CHUNK : 0u) | (b.sig.wfirst ? WIN : 0u) | (b.sig.ranged() ? SIG_RANGE : 0u)) {
    case SIG_F32 | WIN: return f(Int<SIG_F32 | WIN>{});
    case SIG_F16 | WIN: return f(Int<SIG_F16 | WIN>{});
    case SIG_BF16 | WIN: return f(Int<SIG_BF16 | WIN>{});
    case SIG_F32 | WIN | SIG_RANGE: return f(Int<SIG_F32 | WIN | SIG_RANGE>{});
    case SIG_F16 | WIN | SIG_RANGE: return f(Int<SIG_F16 | WIN | SIG_RANGE>{});
    case SIG_BF16 | WIN | SIG_RANGE: return f(Int<SIG_BF16 | WIN | SIG_RANGE>{});
    case SIG_F32 | SIG_CHUNK | SIG_RANGE: return f(Int<SIG_F32 | SIG_CHUNK | SIG_RANGE>{});
    case SIG_F16 | SIG_CHUNK | SIG_RANGE: return f(Int<SIG_F16 | SIG_CHUNK | SIG_RANGE>{});
    case SIG_BF16 | SIG_CHUNK | SIG_RANGE: return f(Int<SIG_BF16 | SIG_CHUNK | SIG_RANGE>{});
    case SIG_NONE: return f(Int<SIG_NONE>{});
    case SIG_F32: return f(Int<SIG_F32>{});
    case SIG_F16: return f(Int<SIG_F16>{});
    case SIG_BF16: return f(Int<SIG_BF16>{});
    case SIG_F32 | SIG_CHUNK: return f(Int<SIG_F32 | SIG_CHUNK>{});
    case SIG_F16 | SIG_CHUNK: return f(Int<SIG_F16 | SIG_CHUNK>{});
    case SIG_BF16 | SIG_CHUNK: return f(Int<SIG_BF16 | SIG_CHUNK>{});
    default: return hipErrorInvalidValue;
    }
}

// the one-workgroup decoder with the store OUT
template <int OUT>
hipError_t svb_decode_launch(const ReadBatch& b, int integer_size, bool zigzag, hipStream_t s)
{
    return svb_dispatch_elem<OUT == SIG_NONE>(integer_size, zigzag, [&](auto e, auto z, auto i) {
        return launch1(svb_decode_kernel<e(), z(), i(), OUT>, b, s);
    });
}

// the counting pass's store -> f(OUT): the range's values alone when the statistics are the range's
template <class F>
hipError_t svb_dispatch_count(const ReadBatch& b, F&& f)
{
    return b.sig.ranged_stats() ? f(Int<SIG_COUNT | SIG_RANGE>{}) : f(Int<SIG_COUNT>{});
}

// ---- the signal pass of a decode launch: the span pass, else the trim pass, else none ---------------------------------------------------
// what every decode launcher refuses of them: a trim without statistics, a span call with a typed output, both together
bool pass_refused(const ReadBatch& b, const TrimOut* trim, const SpanOut* span)
{
    return (trim && !b.sig.norm.st) || (span && (b.sig.type != SIG_NONE || trim));
}

// launch(policy) launches the stream form's pass kernel.  verdicts: the span pass runs alone and owes them (SpanPass)
template <class Launch>
hipError_t launch_pass(const TrimOut* trim, const SpanOut* span, uint32_t verdicts, Launch&& launch)
{
    if (span) return launch(SpanPass{ {}, *span, verdicts });
    if (trim) return launch(TrimPass{ *trim });
    return hipSuccess;
}
// a form's pass kernel with the policy p: one workgroup per int16 read, per POD5 row (svb16_pass_kernel through launch1), per POD5 read
template <class P>
hipError_t svb_pass_launch(const ReadBatch& b, bool zigzag, const P& p, hipStream_t s)
{
    return zigzag ? launch1(svb_pass_kernel<true, true, P>, b, s, p) : launch1(svb_pass_kernel<false, false, P>, b, s, p);
}
template <class P>
hipError_t svb16_pass_reads_launch(const ReadBatch& b, const Pod5Reads& pr, const P& p, hipStream_t s)
{
    if (pr.n_reads) hipLaunchKernelGGL(svb16_pass_reads_kernel<P>, dim3(pr.n_reads), dim3(WG), 0, s, b, pr, p);
    return hipGetLastError();
}

// The launches of a decode in front of its store.  With a normalisation (b.sig.norm.st; int16 samples only): init(), `lead` (launches
// the counting passes need behind the init: the segmented decoder's position passes), then norm_passes() x count(), every pass ending in
// its select, and behind the last one the call's signal pass (launch_pass through `pass`).  Without: lead(), and behind it the span pass
// of a call that brings its own constants -- all that runs for such a call, verdicts included.
// *store: whether the store pass follows -- not for the statistics alone (b.sig.type == SIG_NONE), and not for a span call.
// slab: b.sig.norm.slab must be set (the segments add their counts there) or must not be (one workgroup per read counts in LDS).
template <class Init, class Lead, class Count, class Pass>
hipError_t norm_prepasses(const ReadBatch& b, int integer_size, bool slab, const TrimOut* trim, const SpanOut* span, Init init, Lead lead, Count count,
                          Pass pass, bool* store)
{
    *store = !span;
    if (!b.sig.norm.st) {
        const hipError_t e = lead();
        return e == hipSuccess ? launch_pass(nullptr, span, 1u, pass) : e;
    }
    if (integer_size != 2 || slab != (b.sig.norm.slab != nullptr)) return hipErrorInvalidValue;
    *store = !span && b.sig.type != SIG_NONE && b.n_reads != 0;
    if (b.n_reads == 0) return hipSuccess;
    hipError_t e = init();
    if (e == hipSuccess) e = lead();
    for (uint32_t p = 0; e == hipSuccess && p < norm_passes(b.sig.norm.method); ++p) e = count();
    if (e == hipSuccess) e = launch_pass(trim, span, 0u, pass);
    return e;
}

// the segmented decode: MODE 1, then (SELF) MODE 2 and MODE 0, or the verdict scan, MODE 2 and its scan, and MODE 0; only MODE 0 stores
template <int E, bool Z, bool I, int OUT>
hipError_t svb_decode_seg_sequence(const ReadBatch& b, const uint32_t* seg_first, uint32_t max_segs, uint32_t* seg_val, uint64_t* seg_pos,
                                   uint32_t* seg_run, uint32_t self_max, hipStream_t s, const TrimOut* trim, const SpanOut* span)
{
    const dim3 segs(max_segs), reads(b.n_reads), t(WG);
    const bool self = max_segs <= self_max;
    auto mode0 = [&](auto o) {
        if (self) hipLaunchKernelGGL((svb_seg_decode_kernel<E, Z, I, 0, true, o()>), segs, t, 0, s, b, seg_first, seg_val, seg_pos, seg_run);
        else hipLaunchKernelGGL((svb_seg_decode_kernel<E, Z, I, 0, false, o()>), segs, t, 0, s, b, seg_first, seg_val, seg_pos, seg_run);
        return hipGetLastError();
    };
    bool store;
    const hipError_t e = norm_prepasses(
        b, E, true, trim, span,
        [&] {
            (void)hipMemsetAsync(b.sig.norm.slab, 0, 4ull * NORM_SLAB * b.n_reads, s);
            return launch_norm_init(b, Z, s);
        },
        [&] {
            hipLaunchKernelGGL((svb_seg_decode_kernel<E, Z, I, 1>), segs, t, 0, s, b, seg_first, seg_val, seg_pos, seg_run);
            if (self) {
                if (Z) hipLaunchKernelGGL((svb_seg_decode_kernel<E, Z, I, 2, true>), segs, t, 0, s, b, seg_first, seg_val, seg_pos, seg_run);
            } else {
                hipLaunchKernelGGL((svb_seg_decode_scan_kernel<E, I, true, DecStore<E, OUT>::BYTES>), reads, t, 0, s, b, seg_first, seg_val, seg_pos, seg_run);
                if (Z) {
                    hipLaunchKernelGGL((svb_seg_decode_kernel<E, Z, I, 2>), segs, t, 0, s, b, seg_first, seg_val, seg_pos, seg_run);
                    hipLaunchKernelGGL((svb_seg_decode_scan_kernel<E, I, false>), reads, t, 0, s, b, seg_first, seg_val, seg_pos, seg_run);
                }
            }
            return hipGetLastError();
        },
        [&] {   // a counting pass at the storing pass's positions, behind it a select launch
            if constexpr (E == 2) {
                const hipError_t ec = svb_dispatch_count(b, mode0);
                if (ec != hipSuccess) return ec;
                if (b.sig.ranged_stats()) hipLaunchKernelGGL(norm_select_range_kernel, reads, t, 0, s, b);
                else hipLaunchKernelGGL(norm_select_kernel, reads, t, 0, s, b);
            }
            return hipGetLastError();
        },
        [&](auto p) {   // the pass at the same positions (E == 2, OUT == SIG_NONE: launch_svb_decode_seg has looked); behind a trim's segments its scan launch
            using P = decltype(p);
            if constexpr (E == 2) {
                if (self) hipLaunchKernelGGL((svb_seg_pass_kernel<Z, I, true, P>), segs, t, 0, s, b, seg_first, seg_val, seg_pos, seg_run, p);
                else hipLaunchKernelGGL((svb_seg_pass_kernel<Z, I, false, P>), segs, t, 0, s, b, seg_first, seg_val, seg_pos, seg_run, p);
                if constexpr (std::is_same<P, TrimPass>::value) hipLaunchKernelGGL(trim_select_kernel, reads, t, 0, s, b, p.out);
            }
            return hipGetLastError();
        },
        &store);
    return e == hipSuccess && store ? mode0(Int<OUT>{}) : e;   // (no store: the statistics only, or a span call)
}


}  // namespace

bool svb_encode_fills_plans(int integer_size, bool zigzag, bool half) { return integer_size == 2 && zigzag && !half; }

hipError_t launch_svb_encode(const ReadBatch& b, int integer_size, bool zigzag, uint32_t hdr, bool strict_cap, bool half, uint32_t* period_hint,
                             void* plans, hipStream_t s)
{
    if (b.n_reads == 0) return hipSuccess;
    dim3 g(b.n_reads), t(WG);
    if (half) {  // v1, 1-byte integers: the nibble codec
        if (integer_size != 1) return hipErrorInvalidValue;
        if (period_hint) (void)hipMemsetAsync(period_hint, 0, 4ull * b.n_reads, s);   // (the nibble stream is not probed)
        if (zigzag) hipLaunchKernelGGL((svb_half_encode_kernel<true>), g, t, 0, s, b, hdr);
        else hipLaunchKernelGGL((svb_half_encode_kernel<false>), g, t, 0, s, b, hdr);
        return hipGetLastError();
    }
    const uint32_t sc = strict_cap ? 1u : 0u;
    EncPlan* pre = zstd_encode_plans(plans);
    if (pre && svb_encode_fills_plans(integer_size, zigzag, half) && hdr == 0 && !strict_cap) {
        // the int16 zig-zag stream of a read on its way to the entropy stage: its data bytes' sample counted on the way
        if (period_hint) hipLaunchKernelGGL((svb_encode_kernel<2, true, true, true, true>), g, t, 0, s, b, hdr, sc, period_hint, pre);
        else hipLaunchKernelGGL((svb_encode_kernel<2, true, true, false, true>), g, t, 0, s, b, hdr, sc, period_hint, pre);
        return hipGetLastError();
    }
    pre = nullptr;
    return svb_dispatch_elem(integer_size, zigzag, [&](auto e, auto z, auto i) {
        if (period_hint) hipLaunchKernelGGL((svb_encode_kernel<e(), z(), i(), true>), g, t, 0, s, b, hdr, sc, period_hint, pre);
        else hipLaunchKernelGGL((svb_encode_kernel<e(), z(), i(), false>), g, t, 0, s, b, hdr, sc, period_hint, pre);
        return hipGetLastError();
    });
}

hipError_t launch_svb_decode(const ReadBatch& b, int integer_size, bool zigzag, bool half, hipStream_t s, const TrimOut* trim, const SpanOut* span)
{
    if (pass_refused(b, trim, span) || ((trim || span) && half) || (span && integer_size != 2)) return hipErrorInvalidValue;
    if (span && b.n_reads == 0) return hipSuccess;
    if (half) {
        if (integer_size != 1 || b.sig.type != SIG_NONE) return hipErrorInvalidValue;
        return zigzag ? launch1(svb_half_decode_kernel<true>, b, s) : launch1(svb_half_decode_kernel<false>, b, s);
    }
    bool store;   // the counting passes (each selects at its end) and the signal pass, then the store -- none for the statistics alone
    const hipError_t e = norm_prepasses(
        b, integer_size, false, trim, span, [&] { return launch_norm_init(b, zigzag, s); }, [] { return hipSuccess; },
        [&] { return svb_dispatch_count(b, [&](auto out) { return svb_decode_launch<out()>(b, 2, zigzag, s); }); },
        [&](auto p) { return svb_pass_launch(b, zigzag, p, s); }, &store);
    if (e != hipSuccess || !store) return e;
    return svb_dispatch_store(b, [&](auto out) { return svb_decode_launch<out()>(b, integer_size, zigzag, s); });
}

// ---- svb16 (POD5) ---------------------------------------------------------------------------------------------------
hipError_t launch_svb16_encode(const ReadBatch& b, uint32_t* period_hint, hipStream_t s)
{
    if (b.n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(svb16_encode_kernel, dim3(b.n_reads), dim3(WG), 0, s, b, period_hint);
    return hipGetLastError();
}

hipError_t launch_svb16_decode(const ReadBatch& b, hipStream_t s, const TrimOut* trim, const SpanOut* span)
{
    if (b.n_reads == 0) return hipSuccess;
    if (pass_refused(b, trim, span)) return hipErrorInvalidValue;
    bool store;   // the counting passes (each selects at its end: one workgroup per read) and the signal pass, then the store
    const hipError_t e = norm_prepasses(
        b, 2, false, trim, span,
        [&] {
            hipLaunchKernelGGL(norm_init16_kernel, dim3((b.n_reads + WG - 1) / WG), dim3(WG), 0, s, b);
            return hipGetLastError();
        },
        [] { return hipSuccess; }, [&] { return svb_dispatch_count(b, [&](auto out) { return launch1(svb16_decode_kernel<out()>, b, s); }); },
        [&](auto p) { return launch1(svb16_pass_kernel<decltype(p)>, b, s, p); }, &store);
    if (e != hipSuccess || !store) return e;
    return svb_dispatch_store(b, [&](auto out) { return launch1(svb16_decode_kernel<out()>, b, s); });
}

// ---- POD5 reads of several rows -----------------------------------------------------------------------------------------
hipError_t launch_pod5_reads_check(uint32_t n_rows, const Pod5Reads& pr, uint32_t* out, hipStream_t s)
{
    (void)hipMemsetAsync(pr.bad, 0, 4, s);
    hipLaunchKernelGGL(pod5_reads_check_kernel, dim3(pr.n_reads / WG + 1), dim3(WG), 0, s, n_rows, pr);
    if (out && pr.n_reads) hipLaunchKernelGGL(pod5_reads_bad_kernel, dim3((pr.n_reads + WG - 1) / WG), dim3(WG), 0, s, pr, out);
    return hipGetLastError();
}

hipError_t launch_pod5_read_samples(const Pod5Reads& pr, const uint32_t* row_samples, uint32_t* read_samples, hipStream_t s)
{
    if (pr.n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(pod5_read_samples_kernel, dim3((pr.n_reads + WG - 1) / WG), dim3(WG), 0, s, pr, row_samples, read_samples);
    return hipGetLastError();
}

hipError_t launch_window_pad(const ReadBatch& b, const Pod5Reads& pr, const WindowScratch& w, hipStream_t s)
{
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    if (n == 0 || b.sig.wrows == 0) return hipSuccess;
    const uint64_t wgs = (b.sig.wrows + WG / 64 - 1) / (WG / 64);
    hipLaunchKernelGGL(window_pad_kernel, dim3((uint32_t)(wgs < 16384u ? wgs : 16384u)), dim3(WG), 0, s, b, pr, w.scan);
    return hipGetLastError();
}

static uint32_t event_grid(uint64_t rows)
{
    const uint64_t wgs = (rows + WG - 1) / WG;
    return (uint32_t)(wgs < 16384u ? wgs : 16384u);
}
hipError_t launch_event_zero(const ReadBatch& b, const Pod5Reads& pr, const WindowScratch& w, hipStream_t s)
{
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    if (n == 0 || b.sig.wrows == 0) return hipSuccess;
    hipLaunchKernelGGL(event_zero_kernel, dim3(event_grid(b.sig.wrows)), dim3(WG), 0, s, b, pr, w.scan);
    return hipGetLastError();
}
hipError_t launch_event_finish(const ReadBatch& b, const Pod5Reads& pr, const float* offset, const float* scale, const WindowScratch& w, void* out,
                               hipStream_t s)
{
    const uint32_t n = pr.reads ? pr.n_reads : b.n_reads;
    if (n == 0 || b.sig.wrows == 0) return hipSuccess;
    hipLaunchKernelGGL(event_finish_kernel, dim3(event_grid(b.sig.wrows)), dim3(WG), 0, s, b, pr, offset, scale, w.scan, reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

hipError_t launch_svb16_decode_reads(const ReadBatch& b, const Pod5Reads& pr, const float* offset, const float* scale, uint64_t chunk_rows,
                                     hipStream_t s, const TrimOut* trim, const WindowScratch* win, void* event_out, const SpanOut* span,
                                     const SegmentScratch* spsc)
{
    const uint32_t most = std::max(b.n_reads, pr.n_reads);
    if (most == 0) return hipSuccess;
    if ((b.n_reads && !b.gate) || (b.sig.type == SIG_NONE && !b.sig.norm.st && !span) || b.sig.norm.slab || pass_refused(b, trim, span)) return hipErrorInvalidValue;
    if (span && (!spsc || b.sig.wfirst || b.sig.row)) return hipErrorInvalidValue;
    const dim3 rows(b.n_reads), reads(pr.n_reads), t(WG);
    if (b.sig.ranged() && !pr.range) return hipErrorInvalidValue;
    if (b.sig.wfirst) {   // the plan with the first half of the window check, the second half, the pad
        if (!win || b.sig.row) return hipErrorInvalidValue;
        if (b.sig.ranged()) hipLaunchKernelGGL(pod5_reads_plan_window_range_kernel, dim3((most + WG - 1) / WG), t, 0, s, b, pr, offset, scale);
        else hipLaunchKernelGGL(pod5_reads_plan_window_kernel, dim3((most + WG - 1) / WG), t, 0, s, b, pr, offset, scale);
        hipError_t ew = launch_window_check(b, pr, nullptr, nullptr, *win, s);
        if (ew == hipSuccess) ew = b.sig.events ? launch_event_zero(b, pr, *win, s) : launch_window_pad(b, pr, *win, s);
        if (ew != hipSuccess) return ew;
    } else if (b.sig.ranged()) hipLaunchKernelGGL(pod5_reads_plan_range_kernel, dim3((most + WG - 1) / WG), t, 0, s, b, pr, offset, scale, chunk_rows);
    else hipLaunchKernelGGL(pod5_reads_plan_kernel, dim3((most + WG - 1) / WG), t, 0, s, b, pr, offset, scale, chunk_rows);
    if (span) {   // (the maps' layout: from the reads' sample counts the plan has left)
        const hipError_t el = launch_segment_layout(b, pr, *spsc, s);
        if (el != hipSuccess) return el;
    }
    const bool store = b.sig.type != SIG_NONE;
    if (b.sig.norm.st && pr.n_reads)
        for (uint32_t p = 0; p < norm_passes(b.sig.norm.method); ++p) {
            if (b.sig.ranged_stats()) hipLaunchKernelGGL(svb16_count_reads_range_kernel, reads, t, 0, s, b, pr, !store && p == 0 ? 1u : 0u);
            else hipLaunchKernelGGL(svb16_count_reads_kernel, reads, t, 0, s, b, pr, !store && p == 0 ? 1u : 0u);
        }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_pass(trim, span, b.sig.norm.st ? 0u : 1u, [&](auto p) { return svb16_pass_reads_launch(b, pr, p, s); });
    if (e != hipSuccess) return e;
    if (b.n_reads) {
        if (store) {
            e = svb_dispatch_store(b, [&](auto out) {
                if constexpr (out() != SIG_NONE) hipLaunchKernelGGL(svb16_decode_rows_kernel<out()>, rows, t, 0, s, b, pr);
                return hipGetLastError();
            });
            if (e != hipSuccess) return e;
        }
    }
    if (b.sig.events) {   // the records, behind the event pass and the counting passes
        e = launch_event_finish(b, pr, offset, scale, *win, event_out, s);
        if (e != hipSuccess) return e;
    }
    if (pr.read_result && pr.n_reads) {
        const uint32_t elem = b.sig.type == SIG_F32 && !b.sig.events ? 4u : 2u;   // (an event call: the int16 decode's verdicts)
        hipLaunchKernelGGL(pod5_read_results_kernel, dim3((pr.n_reads + WG - 1) / WG), t, 0, s, b, pr, elem);
    }
    return hipGetLastError();
}

// ---- signal segmentation --------------------------------------------------------------------------------------------------------------
hipError_t launch_svb_segment(const ReadBatch& b, bool zigzag, const SegmentOut& so, hipStream_t s)
{
    return svb_pass_launch(b, zigzag, SegmentPass{ {}, so }, s);
}

hipError_t launch_svb16_segment(const ReadBatch& b, const SegmentOut& so, hipStream_t s)
{
    return launch1(svb16_pass_kernel<SegmentPass>, b, s, SegmentPass{ {}, so });
}

hipError_t launch_svb16_segment_reads(const ReadBatch& b, const Pod5Reads& pr, const SegmentOut& so, const SegmentScratch& sc, hipStream_t s)
{
    const uint32_t most = std::max(b.n_reads, pr.n_reads);
    if (most == 0) return hipSuccess;
    if ((b.n_reads && !b.gate) || b.sig.norm.st || b.sig.row || b.sig.wfirst || (b.sig.ranged() && !pr.range)) return hipErrorInvalidValue;
    const dim3 t(WG);
    if (b.sig.ranged()) hipLaunchKernelGGL(pod5_reads_plan_range_kernel, dim3((most + WG - 1) / WG), t, 0, s, b, pr, nullptr, nullptr, 0ull);
    else hipLaunchKernelGGL(pod5_reads_plan_kernel, dim3((most + WG - 1) / WG), t, 0, s, b, pr, nullptr, nullptr, 0ull);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_segment_layout(b, pr, sc, s);
    if (e == hipSuccess) e = svb16_pass_reads_launch(b, pr, SegmentPass{ {}, so }, s);
    if (e != hipSuccess) return e;
    if (pr.read_result && pr.n_reads) hipLaunchKernelGGL(pod5_read_results_kernel, dim3((pr.n_reads + WG - 1) / WG), t, 0, s, b, pr, 2u);
    return hipGetLastError();
}

hipError_t launch_svb16_key_raw(uint32_t n, const uint32_t* raw_size, uint32_t* key_raw, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(svb16_key_raw_kernel, dim3((n + WG - 1) / WG), dim3(WG), 0, s, n, raw_size, key_raw);
    return hipGetLastError();
}

// ---- segmented launches (few, large reads) --------------------------------------------------------------------------
uint32_t svb_seg_unit_bytes(int integer_size)
{
    return (uint32_t)(WG * (integer_size == 4 ? 4 : 8) * SEG_TILES * integer_size);  // raw bytes of one segment
}

hipError_t launch_svb_encode_seg(const ReadBatch& b, int integer_size, bool zigzag, uint32_t hdr, bool strict_cap, const uint32_t* seg_first,
                                 uint32_t max_segs, uint32_t* seg_bytes, uint64_t* seg_off, uint32_t self_max, hipStream_t s)
{
    if (b.n_reads == 0) return hipSuccess;
    const uint32_t sc = strict_cap ? 1u : 0u;
    const bool self = max_segs <= self_max;
    const dim3 segs(max_segs), reads(b.n_reads), t(WG);
    return svb_dispatch_elem(integer_size, zigzag, [&](auto e, auto z, auto i) {
        constexpr int E = e();
        constexpr bool Z = z(), I = i();
        hipLaunchKernelGGL((svb_seg_encode_kernel<E, Z, I, true>), segs, t, 0, s, b, hdr, sc, seg_first, seg_bytes, seg_off);
        if (self) {
            hipLaunchKernelGGL((svb_seg_encode_kernel<E, Z, I, false, true>), segs, t, 0, s, b, hdr, sc, seg_first, seg_bytes, seg_off);
        } else {
            hipLaunchKernelGGL((svb_seg_encode_scan_kernel<E, I>), reads, t, 0, s, b, hdr, sc, seg_first, seg_bytes, seg_off);
            hipLaunchKernelGGL((svb_seg_encode_kernel<E, Z, I, false>), segs, t, 0, s, b, hdr, sc, seg_first, seg_bytes, seg_off);
        }
        return hipGetLastError();
    });
}

hipError_t launch_svb_decode_seg(const ReadBatch& b, int integer_size, bool zigzag, const uint32_t* seg_first, uint32_t max_segs,
                                 uint32_t* seg_val, uint64_t* seg_pos, uint32_t* seg_run, uint32_t self_max, hipStream_t s, const TrimOut* trim,
                                 const SpanOut* span)
{
    if (b.n_reads == 0) return hipSuccess;
    if (pass_refused(b, trim, span) || (span && (integer_size != 2 || b.sig.events))) return hipErrorInvalidValue;
    return svb_dispatch_store(b, [&](auto out) {
        return svb_dispatch_elem<out() == SIG_NONE>(integer_size, zigzag, [&](auto e, auto z, auto i) {
            return svb_decode_seg_sequence<e(), z(), i(), out()>(b, seg_first, max_segs, seg_val, seg_pos, seg_run, self_max, s, trim, span);
        });
    });
}

}  // namespace vbzhip
