// zstd_frame.h -- serial statements of the headers the zstd-format decoders read (RFC 8878) and of the library's own trailers.
//
// The layer above zstd_tables.h: pure readers over bytes or 64-bit windows the caller already holds, compiled for gfx950 and under g++
// (the CPU unit tests: tests/test_zstd_frame_host.py, against libzstd and the oracle's restatement oracle/zstd_restate.c).  A byte
// accessor at(i) gives byte i of the frame (or of the section) as a uint32_t, ld32(o) the little-endian word at offset o; where those
// bytes live is the caller's business.  The readers decode; what a decoder refuses stays at its call site, in its own order.
//
//   zstd_frame_header   frame header (3.1.1.1): magic, FHD, window, Dictionary_ID, content size
//   zstd_block_header   block header (3.1.1.2): last, type, size, the bytes up to the next block
//   zstd_lit_header     literals section header (3.1.1.3.1.1): type, size format, header bytes, sizes, streams
//   zstd_nseq           Number_of_Sequences (3.1.1.3.2.1)
//   huf_desc_size       bytes of a Huffman tree description (4.2.1) from its header byte
//   zstd_checkpoints    the encoder's checkpoint trailer (CP_MAGIC), with or without the span index trailer (IDX_MAGIC) behind it
//   zstd_skip_frames    skippable frames (3.1.2) behind a frame
#pragma once

#include <stdint.h>

// VBZ_HD as zstd_entropy.h and zstd_tables.h define it
#ifndef VBZ_HD
#if defined(__HIPCC__)
#define VBZ_HD __host__ __device__ __forceinline__
#else
#define VBZ_HD inline
#endif
#endif

namespace vbzhip {

constexpr uint32_t ZSTD_MAGIC = 0xFD2FB528u;
constexpr uint32_t SKIP_MAGIC = 0x184D2A50u, SKIP_MASK = 0xFFFFFFF0u;  // skippable frames: magic & SKIP_MASK == SKIP_MAGIC
constexpr uint32_t CP_MAGIC = 0x184D2A5Bu;    // zstd_encode.hip: the decoder checkpoints of the first sequences section
constexpr uint32_t IDX_MAGIC = 0x184D2A5Cu;   // zstd_encode.hip: the span index
constexpr uint32_t NSEQ_LONG_BASE = 0x7F00u;  // Number_of_Sequences in three bytes: byte1 + (byte2 << 8) + this

struct ZFrameHeader
{
    uint32_t magic, fhd;
    uint32_t len;         // header bytes, the magic number included
    uint32_t wlog;        // Window_Descriptor: 10 + exponent (0: single segment, no descriptor)
    uint32_t did_bytes;   // size of the Dictionary_ID field: 0, 1, 2 or 4
    uint32_t did;
    uint32_t fcs_bytes;   // size of the Frame_Content_Size field (0: the header gives no content size)
    uint32_t checksum;    // Content_Checksum_flag
    uint64_t fcs;         // the content size (+ 256 for the two-byte field)
    uint64_t window;      // the window size; single segment: the content size
};

// The frame header of the n bytes at(0 .. n): false if it does not end inside them (h->len says where it would end; the fields behind
// the FHD byte are then not read).  at(0 .. 4) are always read.
template <class At>
VBZ_HD bool zstd_frame_header(const At& at, uint32_t n, ZFrameHeader* h)
{
    h->magic = at(0) | (at(1) << 8) | (at(2) << 16) | (at(3) << 24);
    const uint32_t fhd = at(4) & 0xFF, single = (fhd >> 5) & 1, fcs_flag = fhd >> 6, did_flag = fhd & 3;
    h->fhd = fhd;
    h->checksum = (fhd >> 2) & 1;
    h->did_bytes = did_flag == 3 ? 4u : did_flag;
    h->fcs_bytes = fcs_flag == 0 ? single : 1u << fcs_flag;
    h->len = 5 + (single ^ 1u) + h->did_bytes + h->fcs_bytes;
    h->wlog = 0;
    h->did = 0;
    h->fcs = 0;
    h->window = 0;
    if (h->len > n) return false;
    uint32_t pos = 5;
    if (!single) {
        const uint32_t wd = at(pos++);
        h->wlog = 10 + (wd >> 3);
        h->window = (1ull << h->wlog) + ((1ull << h->wlog) >> 3) * (wd & 7);
    }
    for (uint32_t i = 0; i < h->did_bytes; ++i) h->did |= at(pos + i) << (8 * i);
    pos += h->did_bytes;
    for (uint32_t i = 0; i < h->fcs_bytes; ++i) h->fcs |= (uint64_t)at(pos + i) << (8 * i);
    if (h->fcs_bytes == 2) h->fcs += 256;
    if (single) h->window = h->fcs;
    return true;
}

struct ZBlockHeader
{
    uint32_t last, type, size;
    uint32_t src;    // bytes behind the header in the source: the next block header is 3 + src bytes on (an RLE block holds one byte)
};

// the block header of the three bytes bh (little-endian, higher bits ignored)
VBZ_HD ZBlockHeader zstd_block_header(uint32_t bh)
{
    ZBlockHeader k;
    k.last = bh & 1;
    k.type = (bh >> 1) & 3;
    k.size = (bh >> 3) & 0x1FFFFF;
    k.src = k.type == 1 ? 1u : k.size;
    return k;
}

struct ZLitHeader
{
    uint32_t type, fmt;   // Literals_Block_Type (0 raw, 1 RLE, 2 compressed, 3 treeless), Size_Format
    uint32_t hsize;       // header bytes
    uint32_t regen;       // Regenerated_Size
    uint32_t csize;       // bytes of the literals behind the header: Compressed_Size, the regenerated size (raw) or 1 (RLE)
    uint32_t streams;     // Huffman streams: 1 or 4 (raw / RLE: 1)
};

// The literals section header over the eight bytes v at the section's start (little-endian; bytes past the block are the caller's to
// rule out: hsize and csize against the block size).  The RFC's rule for compressed literals -- a block of 5 bytes or more and non-zero
// sizes -- is the caller's to apply.
VBZ_HD ZLitHeader zstd_lit_header(uint64_t v)
{
    ZLitHeader l;
    const uint32_t h0 = (uint32_t)v & 0xFF;
    l.type = h0 & 3;
    l.fmt = (h0 >> 2) & 3;
    if (l.type < 2) {  // Size_Format 0 / 2: 5 bits of size, 1: 12, 3: 20
        l.hsize = (l.fmt & 1) ? l.fmt - (l.fmt >> 1) + 1 : 1;
        l.regen = (l.fmt & 1) ? ((uint32_t)v & (0xFFFFFFu >> (8 * (3 - l.hsize)))) >> 4 : h0 >> 3;
        l.csize = l.type == 0 ? l.regen : 1;
        l.streams = 1;
    } else {  // Size_Format 0 / 1: two sizes of 10 bits, 2: 14, 3: 18
        const uint32_t bits = l.fmt < 2 ? 10 : 4 * l.fmt + 6;
        l.hsize = l.fmt < 2 ? 3 : l.fmt + 2;
        l.regen = (uint32_t)(v >> 4) & ((1u << bits) - 1);
        l.csize = (uint32_t)(v >> (4 + bits)) & ((1u << bits) - 1);
        l.streams = l.fmt == 0 ? 1 : 4;
    }
    return l;
}

// Number_of_Sequences from the n >= 1 bytes at(0 .. n) of the sequences section: *used = the bytes of the field (0: it needs more than
// n bytes; the bytes behind at(0) are then not read)
template <class At>
VBZ_HD uint32_t zstd_nseq(const At& at, uint32_t n, uint32_t* used)
{
    const uint32_t b0 = at(0);
    if (b0 < 128) {
        *used = 1;
        return b0;
    }
    if (b0 == 255) {
        if (n < 3) { *used = 0; return 0; }
        *used = 3;
        return at(1) + (at(2) << 8) + NSEQ_LONG_BASE;
    }
    if (n < 2) { *used = 0; return 0; }
    *used = 2;
    return ((b0 - 128) << 8) + at(1);
}

// bytes of a Huffman tree description whose header byte is hb: 1 + the FSE-coded weights, or 1 + the 4-bit weights packed in bytes;
// 0 for hb == 0 (no description is that short)
VBZ_HD uint32_t huf_desc_size(uint32_t hb)
{
    if (hb >= 128) return 1 + ((hb - 127) + 1) / 2;
    return hb == 0 ? 0u : 1 + hb;
}

struct ZCheckpoints
{
    uint32_t off, count, spacing;   // the checkpoint words at offset off; count 0: no trailer
};

// The encoder's checkpoint trailer (a skippable frame that ends the buffer of n bytes, or stands right in front of a span index trailer
// that ends it): magic, size, { u16 spacing, u16 count }, count checkpoint words.  Looked for in buffers of 64 bytes or more.
template <class Ld32>
VBZ_HD ZCheckpoints zstd_checkpoints(const Ld32& ld32, uint32_t n)
{
    ZCheckpoints c = { 0u, 0u, 0u };
    if (n < 64) return c;
    uint32_t tb = ld32(n - 4), ne = n;  // ne: where the checkpoint trailer would end
    if (tb >= 24 && tb <= n - 16 && (tb & 7u) == 0) {  // (n >= 64; no sum that could wrap: these are arbitrary bytes)
        if (ld32(n - tb) == IDX_MAGIC && ld32(n - tb + 4) == tb - 8) {
            ne = n - tb;
            tb = ld32(ne - 4);
        }
    }
    if (tb >= 20 && tb <= 8 + 4 + 4 * 63 + 4 && tb + 16 <= ne) {
        const uint32_t m0 = ld32(ne - tb), m1 = ld32(ne - tb + 4), m2 = ld32(ne - tb + 8);
        const uint32_t cnt = m2 >> 16;
        if (m0 == CP_MAGIC && m1 == tb - 8 && tb == 16 + 4 * cnt && cnt >= 1) {
            c.off = ne - tb + 12;
            c.count = cnt;
            c.spacing = m2 & 0xFFFFu;
        }
    }
    return c;
}

// where the skippable frames that follow offset pos of a buffer of n bytes end (pos itself if none does)
template <class Ld32>
VBZ_HD uint32_t zstd_skip_frames(const Ld32& ld32, uint32_t pos, uint32_t n)
{
    while (n - pos >= 8) {
        const uint32_t m0 = ld32(pos), m1 = ld32(pos + 4);
        if ((m0 & SKIP_MASK) != SKIP_MAGIC || (uint64_t)pos + 8 + m1 > n) break;
        pos += 8 + m1;
    }
    return pos;
}

}  // namespace vbzhip
