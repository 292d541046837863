// zstd_tables.h -- serial statements of the table descriptions the zstd-format decoders read (RFC 8878).
//
// The decoder-side counterpart of zstd_entropy.h: plain integer functions, compiled for gfx950 and under g++ (the CPU unit tests:
// tests/test_zstd_tables_host.py, against the oracle's restatement oracle/zstd_restate.c).  The three decoders instantiate them with
// policies of their own for where the bytes, the counts and the tables live:
//   zstd_decode.hip       lane 0 of the frame's wavefront, LDS arrays (read_ncount, seq_table, huf_read_weights)
//   zstd_decode_ref.hip   one lane per frame, LDS columns [index][lane], tables in LDS or in memory (ref_seq_table)
//   zstd_decode_fast.hip  one lane per tree description, LDS columns (fast_weights_kernel)
// The wave-parallel tree reader of zstd_decode.hip (huf_read_tree) must give the same verdicts; it ends in huf_weights_close.
//
//   fse_read_ncount      FSE table description (4.1.1): normalised counts, accuracy log
//   fse_build            FSE decoding table (4.1.1): the spread, the "less than one" cells, the state numbers
//   seq_table            one table of the sequences section (3.1.1.3.2.2): predefined, RLE, FSE-described or repeat
//   huf_read_weights     Huffman tree description (4.2.1.1): direct or FSE-coded weights
//   huf_weights_close    the implied last weight and libzstd's HUF_readStats rules
//   huf_fill_wave        the Huffman decoding table (4.2.1) from the weights, across a wavefront (device only)
//
// A table policy `t` of fse_build / seq_table / huf_read_weights holds:
//   t.norm(s), t.set_norm(s, c)    normalised count of symbol s
//   t.next(s)                      a uint16_t& the build numbers symbol s's states with
//   t.cell(u)                      a reference to the storage of cell u: its symbol while the table is spread (any type that holds 0..255)
//   t.entry(u, sym, nb, base)      writes the finished cell u; it is called after cell u was last read.  huf_read_weights reads the
//                                  entries back through t.cell(u) and so needs them packed: fse_entry().
#pragma once

#include <stdint.h>

// VBZ_HD as zstd_entropy.h defines it (the same tokens, so either header may come first).  That header is not included here: its
// out-of-line functions are defined for the one translation unit that includes it, the encoder's.
#ifndef VBZ_HD
#if defined(__HIPCC__)
#define VBZ_HD __host__ __device__ __forceinline__
#else
#define VBZ_HD inline
#endif
#endif

namespace vbzhip {

constexpr int HUF_LOG_LIMIT = 12;  // the widest Huffman table of a zstd decoder (libzstd's HUF_TABLELOG_MAX)

VBZ_HD int tab_hbit(uint32_t v) { return 31 - __builtin_clz(v); }  // index of the highest set bit, v != 0

// k <= 17 bits at bit position pos of the little-endian bytes p[0 .. n), bytes from n on reading as zero
VBZ_HD uint32_t le_bits(const uint8_t* p, int n, uint32_t pos, int k)
{
    uint32_t v = 0;
    const uint32_t by = pos >> 3;
    for (int i = 0; i < 3; ++i) {
        const uint32_t idx = by + (uint32_t)i;
        v |= (idx < (uint32_t)n ? (uint32_t)p[idx] : 0u) << (8 * i);
    }
    return (v >> (pos & 7u)) & ((1u << k) - 1u);
}

// a decoding table cell in one word: symbol | nbBits << 8 | new-state base << 16
VBZ_HD uint32_t fse_entry(uint32_t sym, uint32_t nb, uint32_t base) { return sym | (nb << 8) | ((base & 0xFFFFu) << 16); }

// FSE table description (RFC 8878 4.1.1) of n bytes: bits(pos, k) gives k <= 16 bits at bit position pos of the description, zero
// from byte n on; put(s, c) takes the normalised count of symbol s (-1: "less than one").  Returns the bytes used, or -1; sets the
// accuracy log and the number of symbols.
// The one guard against reading far past the description: a description is accepted only if its bits end inside its n bytes, and the
// bit position only grows, so once it is beyond 8 n every way out of the loop is -1 -- leaving there changes no verdict.
template <class Bits, class Put>
VBZ_HD int fse_read_ncount(const Bits& bits, int n, int max_symbol, int max_log, Put put, int* out_log, int* out_nsym)
{
    if (n < 1) return -1;
    const int log = (int)(bits(0u, 4) & 0xF) + 5;
    if (log > max_log) return -1;
    uint32_t bitpos = 4;
    int remaining = (1 << log) + 1, threshold = 1 << log, nbits = log + 1, sym = 0;
    bool prev0 = false;
    while (remaining > 1 && sym <= max_symbol) {
        if (bitpos > 8u * (uint32_t)n) return -1;
        if (prev0) {  // repeat flags: 2 bits each, 3 = three more zeros and another flag
            for (;;) {
                const uint32_t rr = bits(bitpos, 2);
                bitpos += 2;
                for (uint32_t k = 0; k < rr; ++k) {
                    if (sym > max_symbol) return -1;
                    put(sym++, 0);
                }
                if (rr != 3) break;
            }
            prev0 = false;
            if (sym > max_symbol) break;
            continue;
        }
        const int max = (2 * threshold - 1) - remaining;
        const uint32_t v = bits(bitpos, nbits);
        int count;
        if ((int)(v & (uint32_t)(threshold - 1)) < max) {
            count = (int)(v & (uint32_t)(threshold - 1));
            bitpos += (uint32_t)(nbits - 1);
        } else {
            count = (int)(v & (uint32_t)(2 * threshold - 1));
            if (count >= threshold) count -= max;
            bitpos += (uint32_t)nbits;
        }
        count--;  // value 0 is probability "-1"
        remaining -= count < 0 ? -count : count;
        put(sym++, count);
        prev0 = (count == 0);
        while (remaining < threshold) {
            nbits--;
            threshold >>= 1;
        }
    }
    if (remaining != 1) return -1;
    if (sym > max_symbol + 1) return -1;
    const int used = (int)((bitpos + 7) >> 3);
    if (used > n) return -1;
    *out_log = log;
    *out_nsym = sym;
    return used;
}

// FSE decoding table (RFC 8878 4.1.1) from t.norm(0 .. nsym): symbols of count -1 take the cells from the top down, the others are
// spread with the step (5/8 size + 3), and a cell's state number is its symbol's count plus the cell's rank among that symbol's cells.
// false: the counts do not spread over the table.
template <class Tab>
VBZ_HD bool fse_build(Tab& t, int nsym, int log)
{
    const int size = 1 << log;
    int high = size - 1;
    for (int s = 0; s < nsym; ++s) {
        const int c = t.norm(s);
        if (c == -1) {
            t.cell(high--) = s;
            t.next(s) = 1;
        } else {
            t.next(s) = (uint16_t)c;
        }
    }
    const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    int pos = 0;
    for (int s = 0; s < nsym; ++s) {
        const int c = t.norm(s);
        for (int i = 0; i < c; ++i) {
            t.cell(pos) = s;
            do {
                pos = (pos + step) & mask;
            } while (pos > high);
        }
    }
    if (pos != 0) return false;
    for (int u = 0; u < size; ++u) {
        const uint32_t s = (uint32_t)t.cell(u) & 0xFFu;
        const uint32_t ns = t.next((int)s)++;
        const uint32_t nb = (uint32_t)(log - tab_hbit(ns));
        t.entry(u, s, nb, (ns << nb) - (uint32_t)size);
    }
    return true;
}

// One table of a sequences section (RFC 8878 3.1.1.3.2.2), mode 0 predefined (def[0 .. def_n), accuracy log def_log), 1 RLE, 2 FSE,
// 3 repeat; its description is n bytes read through bits(pos, k) as for fse_read_ncount.  Returns the bytes used, or -1.
template <class Tab, class Bits>
VBZ_HD int seq_table(Tab& t, const Bits& bits, int mode, int n, const int16_t* def, int def_n, int def_log, int max_sym, int max_log,
                     int* log_io, bool* have)
{
    if (mode == 0) {
        for (int i = 0; i < def_n; ++i) t.set_norm(i, def[i]);
        if (!fse_build(t, def_n, def_log)) return -1;
        *log_io = def_log;
        *have = true;
        return 0;
    }
    if (mode == 1) {
        if (n < 1) return -1;
        const uint32_t sym = bits(0u, 8);
        if (sym > (uint32_t)max_sym) return -1;
        t.entry(0, sym, 0u, 0u);
        *log_io = 0;
        *have = true;
        return 1;
    }
    if (mode == 2) {
        int log, nsym;
        const int used = fse_read_ncount(bits, n, max_sym, max_log, [&](int s, int c) { t.set_norm(s, c); }, &log, &nsym);
        if (used < 0) return -1;
        if (!fse_build(t, nsym, log)) return -1;
        *log_io = log;
        *have = true;
        return used;
    }
    return *have ? 0 : -1;
}

// The rules of libzstd's HUF_readStats on the weights but the last (total = sum of 2^(w-1) over the non-zero weights, ones = how many
// are 1): the table log is the smallest that leaves room, and the room must be one power of two -- the implied last weight, *lastw --
// and the weight-1 symbols must come in an even number, at least two.  Returns the table log, -1 for a refused description, or -2 for a
// legal one whose table log is beyond max_log (a decoder that keeps no table that wide leaves the tree to one that does).
VBZ_HD int huf_weights_close(uint32_t total, uint32_t ones, int max_log, uint32_t* lastw)
{
    if (total == 0) return -1;
    const int log = tab_hbit(total) + 1;
    if (log > max_log) return log > HUF_LOG_LIMIT ? -1 : -2;
    const uint32_t rest = (1u << log) - total;
    if (rest & (rest - 1)) return -1;
    *lastw = (uint32_t)tab_hbit(rest) + 1;
    ones += *lastw == 1 ? 1u : 0u;
    if (ones < 2 || (ones & 1)) return -1;
    return log;
}

// Huffman tree description (RFC 8878 4.2.1.1) of n bytes -> every weight, the implied last one included, through put(i, w) as it is
// produced.  src.byte(i) is byte i of the description; src.bits(pos, k) k <= 16 bits at bit position pos of the part behind the header
// byte, zero beyond that part (for FSE-coded weights: from byte 1 + header byte on).  t: table policy for the weights' FSE table of at
// most 64 cells with packed entries (fse_entry).  Returns the bytes used, -1, or -2 (huf_weights_close); sets the number of weights and
// the table log.
template <class Src, class Tab, class Put>
VBZ_HD int huf_read_weights(const Src& src, int n, int max_log, Tab& t, Put put, int* out_nw, int* out_log)
{
    if (n < 1) return -1;
    const int hb = (int)src.byte(0);
    int nw = 0, used;
    uint32_t total = 0, ones = 0;
    bool wide = false;
    auto take = [&](uint32_t wt) {
        put(nw++, wt);
        wide |= wt >= 12u;
        total += (wt != 0u && wt < 12u) ? (1u << (wt - 1u)) : 0u;
        ones += wt == 1u ? 1u : 0u;
    };
    if (hb >= 128) {  // direct representation: 4 bits per weight
        const int cnt = hb - 127;
        used = 1 + (cnt + 1) / 2;
        if (used > n) return -1;
        for (int i = 0; i < cnt; ++i) {
            const uint32_t by = src.byte(1 + i / 2);
            take((i & 1) ? (by & 0xFu) : (by >> 4));
        }
    } else {
        used = 1 + hb;
        if (hb == 0 || used > n) return -1;
        int log, nsym;
        // (the weights' alphabet ends at 11 = HUF_TABLELOG_MAX - 1: libzstd >= 1.4.7 refuses a description that lists a symbol beyond it)
        const int hdr = fse_read_ncount([&](uint32_t pos, int k) { return src.bits(pos, k); }, hb, 11, 6,
                                        [&](int s, int c) { t.set_norm(s, c); }, &log, &nsym);
        if (hdr < 0) return -1;
        if (!fse_build(t, nsym, log)) return -1;
        // two interleaved FSE states over the backward bit stream in bytes [1 + hdr, 1 + hb)
        const int q0 = 1 + hdr, qn = hb - hdr;
        if (qn < 1) return -1;
        const uint32_t last = src.byte(hb);
        if (last == 0) return -1;
        const int top = tab_hbit(last);
        int left = (qn - 1) * 8 + top;  // unread bits of the stream
        uint64_t buf = top ? ((uint64_t)(last & ((1u << top) - 1u)) << (64 - top)) : 0ull;
        int avail = top, nextb = qn - 1;
        auto rd = [&](int nb) -> uint32_t {  // bits below the stream read as zero
            while (avail <= 56 && nextb > 0) {
                --nextb;
                buf |= (uint64_t)src.byte(q0 + nextb) << (56 - avail);
                avail += 8;
            }
            const uint32_t v = nb ? (uint32_t)(buf >> (64 - nb)) : 0u;
            buf <<= nb;
            avail = avail > nb ? avail - nb : 0;
            left -= nb;
            return v;
        };
        uint32_t s1 = rd(log), s2 = rd(log);
        if (left < 0) return -1;
        for (;;) {
            if (nw > 253) return -1;
            uint32_t e = t.cell((int)s1);
            take(e & 0xFFu);
            s1 = (e >> 16) + rd((int)((e >> 8) & 0xFF));
            if (left < 0) {
                take(t.cell((int)s2) & 0xFFu);
                break;
            }
            if (nw > 253) return -1;
            e = t.cell((int)s2);
            take(e & 0xFFu);
            s2 = (e >> 16) + rd((int)((e >> 8) & 0xFF));
            if (left < 0) {
                take(t.cell((int)s1) & 0xFFu);
                break;
            }
        }
    }
    if (wide) return -1;
    uint32_t lastw = 0;
    const int log = huf_weights_close(total, ones, max_log, &lastw);
    if (log < 0) return log;
    put(nw++, lastw);
    *out_nw = nw;
    *out_log = log;
    return used;
}

#if defined(__HIPCC__)
// All 64 lanes of a wavefront: the Huffman decoding table T (symbol | nbBits << 8, 2^tlog cells) from the weights W[0 .. nw) (RFC 8878
// 4.2.1: cells by increasing weight, then increasing symbol value).  Lane l holds symbols l, l + 64, l + 128, l + 192; a symbol's first
// cell = the cells of all lighter symbols + those of the equally heavy symbols before it, both counted with ballots.  Short runs are
// written by the owning lane, long ones by the whole wave.  The caller orders the writes before the table's readers.
__device__ __forceinline__ void huf_fill_wave(uint16_t* T, const uint8_t* W, uint32_t nw, uint32_t tlog, int lane)
{
    uint32_t wt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t s = (uint32_t)lane + 64u * j;
        wt[j] = s < nw ? W[s] : 0u;
    }
    uint32_t base[13];
    {
        uint32_t acc = 0;
#pragma unroll
        for (int v = 1; v <= 12; ++v) {
            uint32_t c = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) c += (uint32_t)__popcll(__ballot(wt[j] == (uint32_t)v));
            base[v] = acc;
            acc += c << (v - 1);
        }
        base[0] = 0;
    }
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t st[4], len[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        st[j] = 0;
        len[j] = wt[j] ? 1u << (wt[j] - 1) : 0u;
#pragma unroll
        for (int v = 1; v <= 12; ++v) {
            const uint64_t m = __ballot(wt[j] == (uint32_t)v);
            if (wt[j] == (uint32_t)v) st[j] = base[v] + ((uint32_t)__popcll(m & below) << (v - 1));
            base[v] += (uint32_t)__popcll(m) << (v - 1);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t s = (uint32_t)lane + 64u * j;
        const uint16_t ent = (uint16_t)(s | ((tlog + 1 - wt[j]) << 8));
        if (len[j] && len[j] < 64)
            for (uint32_t i = 0; i < len[j]; ++i) T[st[j] + i] = ent;
        uint64_t big = __ballot(len[j] >= 64);
        while (big) {
            const int src_lane = __ffsll((long long)big) - 1;
            big &= big - 1;
            const uint32_t bst = (uint32_t)__builtin_amdgcn_readlane((int)st[j], src_lane);
            const uint32_t blen = (uint32_t)__builtin_amdgcn_readlane((int)len[j], src_lane);
            const uint32_t bent = (uint32_t)__builtin_amdgcn_readlane((int)ent, src_lane);
            for (uint32_t i = lane; i < blen; i += 64u) T[bst + i] = (uint16_t)bent;
        }
    }
}
#endif

}  // namespace vbzhip
