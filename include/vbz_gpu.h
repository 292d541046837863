/*
 * vbz_gpu.h -- batched, device-resident extension of the VBZ C ABI (MI355X / gfx950).
 *
 * The reference API (vbz.h) handles one host buffer per call, which cannot feed a GPU
 * (SURVEY.md section 8b "needed extension").  This header adds the entry points a caller that
 * already holds many reads in HBM binds instead: one call encodes or decodes a whole batch of
 * independent reads, each with exactly the semantics of the corresponding single-buffer call
 *
 *   vbz_gpu_compress_batch   == n x vbz_compress[_sized]    (reference vbz/vbz.cpp:116-208,302-330)
 *   vbz_gpu_decompress_batch == n x vbz_decompress[_sized]  (reference vbz/vbz.cpp:210-300,332-366)
 *
 * Plain C: pointers and sizes only, no torch / HIP types in the signatures (the stream is passed
 * as an opaque void* that is a hipStream_t).  All pointers in vbz_gpu_batch are DEVICE pointers.
 * Calls are asynchronous on the context's stream; results (per-read sizes or vbz error codes) land
 * in batch->result in stream order.
 *
 * How a batch is laid onto the device is the library's business and never changes the DECODED data.  The compressed bytes
 * (and so result[i] of a compress call) may depend on it: reads on the large-read path are coded as spans (unless they
 * repeat at one distance, below), a batch too small to fill the device is coded as spans too, and the matcher is used only
 * where dst_cap[i] leaves room for its workspace above the worst-case frame.  The library may write anywhere inside a read's
 * destination slot [dst_off[i], dst_off[i] + dst_cap[i]) (workspace, staging), not only the result[i] bytes it reports.
 *   - the shape rule: a batch whose average read is half a megabyte or more (a 10 M-element buffer), or which is too
 *     small to fill the device with one wavefront per read (up to 96 MB of reads of 64 KB and more: one HDF5 chunk per
 *     call), runs on the large-read path, many workgroups per read;
 *   - per-read routing: in any other batch the reads of 512 KB and more (at most 16 of them, 64 MB in all;
 *     the first in batch order; none if the batch holds more than 1024 such reads) are coded on that path beside the rest of the batch, on a second stream of the
 *     context that is forked from and joined to the context's stream inside the call -- to the caller the
 *     call is still one unit of work in stream order;
 *   - a read whose bytes repeat at one distance (a cycled template) gets that distance coded as zstd matches
 *     at every zstd_compression_level (the reference passes its level to libzstd, whose matcher is on at all
 *     of them), whatever its length: a long read that has such a distance is coded by one wavefront with the matcher
 *     instead of as spans (15-60 x smaller, at one wavefront's speed);
 *   - decompress: frames of this library's shape are decoded by a batched decoder, any other conforming zstd frame by the
 *     general one in the same call; in calls of 2 560 reads and more the sequence chains of frames libzstd wrote (the
 *     reference's files) are walked ahead of the general decoder, one lane per frame, on a second stream of the context
 *     that is forked from and joined to the context's stream inside the call.  Bytes and verdicts never depend on it
 *     (vbz_gpu_decode_paths tells which frames went which way).
 * Descriptor tables are untrusted like the data: before any other kernel runs, one thread per read checks
 * src_off + src_size <= src_bytes and dst_off + dst_cap <= dst_bytes (64-bit arithmetic); a read that fails gets
 * VBZ_INPUT_SIZE_ERROR or VBZ_DESTINATION_SIZE_ERROR and none of its addresses is ever formed
 * (vbz_gpu_compress_batch / vbz_gpu_decompress_batch; the stage-level entry points below trust their tables).
 */
#ifndef VBZ_GPU_H_MI355X
#define VBZ_GPU_H_MI355X

#include <stddef.h>
#include <stdint.h>

#include "vbz.h"

#if defined(__cplusplus)
extern "C" {
#endif

typedef struct vbz_gpu_ctx vbz_gpu_ctx;

typedef struct vbz_gpu_batch
{
    uint32_t n_reads;
    uint32_t reserved;
    /* inputs: read i occupies src[src_off[i] .. src_off[i]+src_size[i]).  Offsets must not overlap,
     * should be 16-byte aligned (a slower path handles other alignments), and the arena must be
     * readable for 16 bytes past the last input (the same slack streamvbyte asks for).
     * Decompression additionally reads whole ALIGNED 128-byte lines: device memory must be readable
     * from the 128-byte line that holds the first input byte to the end of the line that holds the
     * last one (+ 16).  Any arena that is an allocation of its own (hipMalloc: 256-byte aligned,
     * page granular) satisfies this; an arena carved out of a larger buffer does as long as the
     * enclosing buffer covers those lines. */
    const void* src;
    const uint64_t* src_off;
    const uint32_t* src_size;
    uint64_t src_bytes; /* extent of the src arena covering every read (sizes the scratch) */
    /* outputs: read i may use dst[dst_off[i] .. dst_off[i]+dst_cap[i]).
     *   compress:   dst_cap[i] >= vbz_max_compressed_size(src_size[i]) (as for vbz_compress)
     *   decompress: dst_cap[i] == the exact original byte count      (as for vbz_decompress);
     *               for the sized variant it is the capacity and the size comes from the header */
    void* dst;
    const uint64_t* dst_off;
    const uint32_t* dst_cap;
    uint64_t dst_bytes; /* extent of the dst arena covering every slot */
    /* per read: number of bytes produced, or a vbz error code (vbz_is_error) */
    uint32_t* result;
} vbz_gpu_batch;

/* Create a context on HIP device `device`.  `stream` is a hipStream_t to launch on (NULL: the
 * context creates its own non-blocking stream).  Returns NULL (message on stderr) if no gfx950
 * device or kernel image is usable. */
VBZ_EXPORT vbz_gpu_ctx* vbz_gpu_create(int device, void* stream);
VBZ_EXPORT void vbz_gpu_destroy(vbz_gpu_ctx* ctx);
VBZ_EXPORT void* vbz_gpu_stream(vbz_gpu_ctx* ctx);
VBZ_EXPORT const char* vbz_gpu_last_error(vbz_gpu_ctx* ctx);
/* Decoder hints behind the zstd frame.  By default a compressed buffer may end in zstd SKIPPABLE frames (RFC 8878 3.1.2;
 * libzstd, hence the reference's vbz_decompress, ignores them): checkpoints of the sequences section (magic 0x184D2A5B,
 * <= 272 bytes) and, for reads of half a megabyte or more (and for every read of a small batch), an index of the frame's spans (magic
 * 0x184D2A5C, 8 bytes per span of 4 - 32 KB of content, 256 KB in very large frames; bit 31 of its span count says that the data bytes share one Huffman table: spans that
 * begin with a treeless block).  This library's decoder uses them to decode one frame on many lanes / wavefronts and verifies
 * them; without them it decodes the same frames, more slowly.  enable = 0 writes plain single zstd frames (for consumers
 * that insist on consumed == source size after ONE frame); the compression itself (run sequences included) is unchanged.
 * The single-buffer API of vbz.h follows the environment variable VBZ_HIP_TRAILERS (0 / 1, default 1). */
VBZ_EXPORT void vbz_gpu_set_trailers(vbz_gpu_ctx* ctx, int enable);
/* Canonical encoding.  The reference's output for a buffer is a function of (input, options, libzstd version) alone
 * (vbz/vbz.cpp:116-208).  Every frame this library writes is standard zstd that the reference decodes, but by default WHICH kernels code
 * a read -- hence its bytes -- follows from the shape of the call it arrives in (few large reads, a handful of reads, thousands): the
 * same read may come out differently from the HDF5 filter, the bulk re-packer and a large batch.  enable = 1: a read's bytes depend on
 * the read, the options, the trailer setting and the library version only -- reads of 512 KiB of raw data and more are coded as spans
 * with a table each, all others by one wavefront, whatever else is in the call.  Destination slots must have the reference's capacity
 * (vbz_max_compressed_size), as the reference requires anyway.  Costs one stream synchronisation per compress call (the number of large
 * reads comes back to the host), nothing at thousands of ordinary reads per call, and the small-call latency of the default (a call
 * with one 100 k-sample read: ~0.4 ms instead of ~0.14).  Decoding is unaffected.  The single-buffer API of vbz.h, the HDF5 plugin and
 * the re-packer follow the environment variable VBZ_HIP_CANONICAL (0 / 1, default 0). */
VBZ_EXPORT void vbz_gpu_set_canonical(vbz_gpu_ctx* ctx, int enable);
/* Content checksums (RFC 8878 3.1.1).  Decoding: a frame whose header carries Content_Checksum_flag is held to the low 32 bits of
 * XXH64 (seed 0) of its content -- the svb stream, or the raw bytes at integer_size 0 -- stored behind its last block; a mismatch is
 * VBZ_ZSTD_ERROR for that read, the verdict libzstd (checksum_wrong), hence the reference's vbz_decompress, gives.  Always on: one short
 * launch per decode that reads one byte of each frame without the flag.
 * Encoding: enable = 1 writes every zstd frame with the flag and the checksum (between the last block and the skippable trailers; a frame
 * whose trailers would then not fit vbz_max_compressed_size loses the trailers, which are hints only).  Every decoder of zstd frames checks
 * it: damaged data is an error at read time instead of a silent change.  The frames are otherwise the same bytes; enable = 0 (the default)
 * writes exactly what this library wrote before.  Level 0 writes no zstd frame: the knob does nothing there.  Cost: every read's svb
 * stream is hashed once more (in front of the entropy stage) and its trailers moved (behind it).  Measured on one MI355X, 65 536 reads of
 * ~100 k int16 samples: 1.70 ms per encode call, 1.64 ms per decode call of checksummed frames (the hash runs at ~5 TB/s over the svb
 * streams); bench.py 587 -> 508 GB/s.  ONE large read is hashed by one quad of lanes, bound by the latency of its serial chain
 * (57 cycles a round of 32 bytes: ~1.35 GB/s at best) and partly by load latency: ~1 GB/s measured, a 40 MB buffer ~41 ms, so a
 * 10 M-element uint32 buffer costs ~16 ms per direction instead of ~0.2 ms (profiles/HISTORY.md).  The single-buffer API of
 * vbz.h, the HDF5 plugin and the re-packer follow the environment variable VBZ_HIP_CHECKSUM (0 / 1, default 0). */
VBZ_EXPORT void vbz_gpu_set_checksum(vbz_gpu_ctx* ctx, int enable);
/* wait for everything queued on the context's stream; returns 0 or a negative HIP error */
VBZ_EXPORT int vbz_gpu_synchronize(vbz_gpu_ctx* ctx);

/* Both return 0 when the batch was queued, negative on a launch/allocation failure (see
 * vbz_gpu_last_error; -2: options this library does not know, or declared arena extents beyond 2^46 bytes, refused before
 * anything is sized by them).  Per-read failures are reported in batch->result, not here. */
VBZ_EXPORT int vbz_gpu_compress_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch,
                                      const struct CompressionOptions* options, int sized);
VBZ_EXPORT int vbz_gpu_decompress_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch,
                                        const struct CompressionOptions* options, int sized);

/* Calibrated signal.  vbz_gpu_decompress_signal_batch decodes int16 signal (options->integer_size must be 2; any zig-zag setting, version 0
 * or 1, any level, sized or not) straight into float32, float16 or bfloat16: sample x of read i becomes
 *     y = ((float)x + offset[i]) * scale[i]
 * in float32 arithmetic, each operation rounded to nearest even, the add before the multiply, no fused multiply-add; for F16 / BF16 the
 * float32 y is rounded once (to nearest even) to the output type.  Float32 output is therefore bit for bit numpy's
 * (x.astype(np.float32) + np.float32(o)) * np.float32(s).  Overflow gives +-inf; a NaN among the constants gives NaN (its bits unspecified).
 * fast5: offset = the channel's offset, scale = range / digitisation; POD5: offset and scale as stored.
 * The src side of the batch is as for vbz_gpu_decompress_batch.  The dst side describes the TYPED arena, E = 4 (F32) or 2 bytes per
 * sample: unsized, dst_cap[i] = samples * E exactly; sized, dst_cap[i] is the capacity and the header gives the sample count.
 * result[i] = samples * E, or the error code vbz_gpu_decompress_batch gives for the same source with the int16 capacity dst_cap[i] / E * 2;
 * a slot whose dst_off[i] or dst_cap[i] is not a multiple of E gets VBZ_DESTINATION_SIZE_ERROR and is never written.  Nothing outside the
 * slots is written; what a slot holds after an error is unspecified.  Returns 0 when queued, -1 for a NULL context or batch or a launch
 * failure, -2 (nothing launched) for options other than those above, a NULL format, an unknown out_type, is_signed not 0 / 1, a NULL table
 * of the batch or a declared extent beyond 2^46 bytes.
 * The conversion is the svb decode stage's store (there is no second pass over the samples): every decode path of the int16 call
 * (split batches, routed long reads, the large-read path, level 0, frames libzstd wrote) carries it.  Slots 16-byte aligned take the
 * wide stores; E-aligned slots that are not decode correctly on a slower path.  Measured on one MI355X, 65 536 reads of ~100 k samples
 * (tools/time_signal.py, profiles/HISTORY.md "Calibrated signal"): int16 call 11.2 ms; float16 11.4 ms, bfloat16 11.3 ms, float32
 * 14.2 ms; the int16 call followed by torch's (x.float() + o) * s 46.5 ms. */
#define VBZ_GPU_SIGNAL_F32 1
#define VBZ_GPU_SIGNAL_F16 2
#define VBZ_GPU_SIGNAL_BF16 3
typedef struct vbz_gpu_signal_format
{
    uint32_t out_type;   /* VBZ_GPU_SIGNAL_* */
    uint32_t is_signed;  /* 1: the 16-bit samples are int16, 0: uint16 (the format does not say which) */
    const float* offset; /* device, n_reads floats; NULL: 0 for every read */
    const float* scale;  /* device, n_reads floats; NULL: 1 for every read */
} vbz_gpu_signal_format;
VBZ_EXPORT int vbz_gpu_decompress_signal_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                               int sized, const vbz_gpu_signal_format* format);

/* Model-input chunks.  A model takes a dense [chunks, L] tensor of fixed-length windows, not ragged reads.  The chunking of a read of T
 * samples (L = chunk_len, S = step):
 *   T == 0: no chunk.  0 < T <= L: one chunk, starting at 0.  T > L: K = k* + 1 chunks, k* = ceil((T - L) / S); chunk k < k* starts at
 *   k * S, the last one at k* * S (PAD) or at min(k* * S, e), e = ceil((T - L) / end_align) * end_align (END: pulled back to end at most
 *   end_align - 1 samples past the read's end).  Position p of a chunk starting at s holds sample s + p when s + p < T, else `pad`.
 * Starts increase strictly.  L and S are multiples of 8, 8 <= S <= L <= 2^20; end_align is 1 ... 4096 for END and 0 for PAD; `pad` is
 * rounded (to nearest even) to the output type; reserved must be 0.
 * vbz_gpu_chunk_layout_batch: chunk_first[i] = the exclusive scan of the reads' chunk counts (chunk_first[n] = the total; samples[i] of
 * 2^31 or more -- an error code of vbz_gpu_decompressed_size_batch -- counts 0).  chunk_info (nullable; written only when the total is at
 * most info_cap, otherwise untouched): chunk_info[2c] = the read of row c, chunk_info[2c + 1] = its start sample.  A first call with NULL
 * sizes the table (one synchronisation).  Returns 0 when queued, -1 for a NULL context or a launch failure, -2 (nothing launched) for a
 * chunking outside the rules, a NULL chunk_first, or a NULL samples when n > 0.
 * vbz_gpu_decompress_chunks_batch: decodes int16 signal as vbz_gpu_decompress_signal_batch does (the same options and format) and stores
 * chunk k of read i as row chunk_first[i] + k of `chunks`, a row-major [chunk_rows, L] arena of the output type, 16-byte aligned.  The
 * dst side of the batch (dst_off, dst_cap, dst_bytes) is the int16 layout vbz_gpu_decompress_batch would take for the same reads
 * (unsized: dst_cap[i] = 2 * T; sized: the capacity); batch->dst is neither read nor written and may be NULL.  Per read, in this order:
 * the descriptor checks; sized, the header verdicts; then the chunk check -- chunk_first is untrusted: chunk_first[i + 1] - chunk_first[i]
 * != K(T), chunk_first[i] > chunk_first[i + 1] or chunk_first[i + 1] > chunk_rows gives VBZ_DESTINATION_SIZE_ERROR and not one byte of
 * chunks is written for the read; otherwise the signal call's verdict.  result[i] = T * E (E = 4 or 2 bytes per sample) on success, when
 * every position of the read's K rows has been written.  Rows of a read that fails after the chunk check hold unspecified contents; rows
 * chunk_first[n] ... chunk_rows - 1 are never written.  Returns 0 when queued, -1 for a NULL context or batch or a launch failure, -2
 * (nothing launched) for everything the signal call refuses, a chunking outside the rules, a NULL chunk_first or chunks when n > 0, a
 * chunks arena not 16-byte aligned, or chunk_rows * L * E beyond 2^46 bytes.
 * The placement is the svb decode stage's store (no per-read intermediate, no second pass): each sample is converted once and stored in
 * every chunk that holds it, as whole 16-byte stores, the END chunk's unaligned start included; the padding is written in the same launch.
 * Measured on one MI355X, 65 536 reads of ~100 k samples, L = 10 000, S = 9 504, float16 (tools/time_chunks.py, profiles/HISTORY.md
 * "Model-input chunks"): signal call 10.9 ms; chunks PAD 11.6 ms, END 11.9 ms; the signal call followed by a torch gather 30.5 ms. */
#define VBZ_GPU_CHUNK_PAD 0 /* chunk k starts at k * step; the last one is padded past the read's end */
#define VBZ_GPU_CHUNK_END 1 /* the last chunk is pulled back to end at the read's end */
typedef struct vbz_gpu_chunking
{
    uint32_t chunk_len; /* L: samples per chunk, a multiple of 8, 8 <= L <= 2^20 */
    uint32_t step;      /* S: samples between consecutive chunk starts, a multiple of 8, 8 <= S <= L (overlap L - S) */
    uint32_t mode;      /* VBZ_GPU_CHUNK_PAD or VBZ_GPU_CHUNK_END */
    uint32_t end_align; /* END only: the last chunk's start is rounded UP to a multiple of this, 1 ... 4096 (PAD: must be 0) */
    float pad;          /* the value of positions past the read's end, rounded (RNE) to the output type */
    uint32_t reserved;  /* must be 0 */
} vbz_gpu_chunking;     /* 24 bytes */
VBZ_EXPORT int vbz_gpu_chunk_layout_batch(vbz_gpu_ctx* ctx, uint32_t n_reads, const uint32_t* samples, const vbz_gpu_chunking* chunking,
                                          uint64_t* chunk_first, uint32_t* chunk_info, uint64_t info_cap);
VBZ_EXPORT int vbz_gpu_decompress_chunks_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                               const vbz_gpu_signal_format* format, const vbz_gpu_chunking* chunking,
                                               const uint64_t* chunk_first, void* chunks, uint64_t chunk_rows);

/* Per-read normalisation.  A model wants each read normalised by statistics of its own signal, which exist only once the read is decoded.
 * These calls derive them on the device, from the svb streams the decode leaves in its scratch, by extra passes of the svb stage that store
 * nothing; the zstd stage still runs once.  The statistics are order statistics of the read's T raw 16-bit values (int16 or uint16 per
 * is_signed), x_(0) <= ... <= x_(T-1), in float64 arithmetic, each operation rounded to nearest even, no fused multiply-add:
 *   MED_MAD:  c = the median (x_(floor((T-1)/2)) + x_(ceil((T-1)/2))) / 2, w = the median of the T values |x_j - c| by the same rule
 *             (both bit for bit numpy's np.median on float64);
 *   QUANTILE: Q(q) is numpy's np.quantile(x.astype(float64), float64(q)) (method "linear"): h = float64(q) * (T - 1), j = floor(h),
 *             t = h - j, a = x_(j), b = x_(min(j + 1, T - 1)), d = b - a, Q = t < 0.5 ? a + d * t : b - d * (1 - t);
 *             c = Q(quantile_a) + Q(quantile_b), w = Q(quantile_b) - Q(quantile_a);
 *   T == 0:   c = w = 0.
 * shift = float32(max(float64(shift_min), float64(shift_mul) * c)), scale = float32(max(float64(scale_min), float64(scale_mul) * w)).
 * Bonito / Remora: MED_MAD, shift_mul 1, scale_mul 1.4826, shift_min -INFINITY, scale_min FLT_MIN: (x - med) / (1.4826 MAD).  Dorado:
 * QUANTILE 0.2 / 0.9, shift_mul 0.51, scale_mul 0.53, shift_min 10, scale_min 1.
 * The decode calls then store ((float)x - shift) * scale' with scale' = float32(1.0 / float64(scale)) -- a MULTIPLY BY A ROUNDED
 * RECIPROCAL, not a division by scale: exactly the signal call's formula with offset = -shift and scale = scale' (its rounding rules,
 * F16 / BF16 rounded once from the float32 value).
 * shift_scale (device, n_reads x {float shift, float scale}; nullable for the two decode calls, required for the statistics alone) gets
 * every read's shift and scale; for a read whose result[i] is an error code the entry is unspecified.
 * vbz_gpu_decompress_signal_norm_batch and vbz_gpu_decompress_chunks_norm_batch behave exactly like vbz_gpu_decompress_signal_batch and
 * vbz_gpu_decompress_chunks_batch (options, format, chunking, descriptor checks, sized headers, verdicts, result[i], what is and is not
 * written), except that read i's constants come from its statistics: format->offset and format->scale must be NULL.
 * vbz_gpu_signal_norm_batch computes the statistics alone: the dst side of the batch is the int16 layout (as for the chunk call), batch->dst
 * may be NULL and is never written, result[i] is what vbz_gpu_decompress_batch gives for the read.
 * All three return 0 when queued, -1 for a NULL context or batch or a launch failure, -2 (nothing launched) for everything their
 * counterparts refuse, and: a NULL norm, an unknown method, reserved != 0, quantile fields outside their rules, NaN or +-inf where the struct
 * says finite, a scale_min that is not a normal positive float, format->offset or format->scale not NULL, a NULL shift_scale (statistics
 * call).
 * How: a counting pass of the svb decoder histograms the read's values into 4 x 1024 bins of LDS around its first sample, and the ranks
 * are read off the counts at the pass's end (on the large-read path the segments add their counts up in scratch, and a launch of its own
 * selects); a rank outside those bins costs two more passes (the bracket shrinks 1024-fold a pass), a MAD outside them two more.  A call
 * launches every pass a read may need (MED_MAD 5, QUANTILE 3); reads already finished leave a pass at once.  Measured on one MI355X, 65 536
 * reads of ~100 k samples, L = 10 000, S = 9 504, PAD, float16 (tools/time_norm.py, profiles/HISTORY.md "Normalised chunks"): chunk call
 * with given constants 11.7 ms; normalised chunks MED_MAD 16.9 ms, QUANTILE 16.7 ms; statistics alone 11.8 ms; int16 decode + torch
 * per-read median / MAD + chunk call 708 ms.  The first counting pass costs about what the store pass costs (LDS atomics on crowded bins). */
#define VBZ_GPU_NORM_MED_MAD 1
#define VBZ_GPU_NORM_QUANTILE 2
typedef struct vbz_gpu_normalization
{
    uint32_t method;            /* VBZ_GPU_NORM_* */
    uint32_t reserved;          /* must be 0 */
    float quantile_a;           /* QUANTILE: 0 <= quantile_a <= quantile_b <= 1; MED_MAD: both must be 0 */
    float quantile_b;
    float shift_mul, scale_mul; /* finite */
    float shift_min;            /* finite, or -INFINITY (no floor) */
    float scale_min;            /* finite, normal, > 0 */
} vbz_gpu_normalization;        /* 32 bytes */
VBZ_EXPORT int vbz_gpu_signal_norm_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                         uint32_t is_signed, const vbz_gpu_normalization* norm, float* shift_scale);
VBZ_EXPORT int vbz_gpu_decompress_signal_norm_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                    int sized, const vbz_gpu_signal_format* format, const vbz_gpu_normalization* norm,
                                                    float* shift_scale);
VBZ_EXPORT int vbz_gpu_decompress_chunks_norm_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                    int sized, const vbz_gpu_signal_format* format, const vbz_gpu_chunking* chunking,
                                                    const uint64_t* chunk_first, void* chunks, uint64_t chunk_rows,
                                                    const vbz_gpu_normalization* norm, float* shift_scale);

/* POD5 signal rows.  options->vbz_version = VBZ_GPU_VERSION_POD5 (the bytes "POD5") with integer_size 2 and perform_delta_zig_zag 1
 * selects the codec of the POD5 format's signal table: a row of n int16 samples x_j is one zstd frame (RFC 8878; pod5 writes libzstd level 1,
 * content size present, no checksum) whose content is the svb16 stream of
 *     d_j = (x_j - x_{j-1}) mod 2^16 (x_{-1} = 0: every row starts from 0),  z_j = ((d_j << 1) ^ (int16(d_j) >> 15)) & 0xFFFF:
 * K = ceil(n / 8) key bytes -- bit j % 8 (LSB first) of byte j / 8 is 1 when z_j takes two data bytes; unused bits are written 0 and
 * ignored -- then, for j = 0 ... n - 1, z_j as one byte (z_j < 256) or two, little-endian.  svb16_max(n) = K + 2n; n = 0 is an empty stream.
 * The value exists in this batched API only: vbz.h's calls, the HDF5 filter and vbz.py give VBZ_VERSION_ERROR for it, as the reference does.
 * Accepted with sized = 0 and zstd_compression_level >= 1 (levels above 1 write level-1 frames, as for v0); sized = 1, level 0, zig-zag 0 or
 * integer_size != 2 return -2 before anything is launched, and vbz_gpu_decompressed_size_batch refuses the options (a row has no header;
 * its sample count is the file's `samples` column).  Calls that take them, with the semantics they document, one batch entry per row:
 * vbz_gpu_compress_batch / vbz_gpu_decompress_batch, vbz_gpu_decompress_signal_batch, vbz_gpu_decompress_chunks_batch, the three
 * normalising calls (a row counts as a read: its chunks and statistics are the row's; reads of several rows: the vbz_gpu_pod5_* calls below), and the svb stage entry points with
 * version = VBZ_GPU_VERSION_POD5 (the svb16 stream alone).  Compress slots need dst_cap[i] >= vbz_gpu_pod5_max_compressed_size(samples)
 * = ZSTD_COMPRESSBOUND(svb16_max(n)), pod5's compressed_signal_max_size.  Decode verdicts per row: a zstd failure or frame content longer
 * than svb16_max(n) is VBZ_ZSTD_ERROR; a stream whose length is not K + n + popcount(the first n key bits) is VBZ_STREAMVBYTE_STREAM_ERROR;
 * descriptor, capacity and alignment failures are the v0 int16 call's.  Trailers, checksums and canonical mode act on POD5 frames as on
 * v0's; libzstd decodes them.  The rows of one read decode into one contiguous signal when their slots are adjacent
 * (batch.pod5_read_layout).  The svb16 stage runs one workgroup per row on every path. */
#define VBZ_GPU_VERSION_POD5 0x35444F50u
VBZ_EXPORT uint64_t vbz_gpu_pod5_max_compressed_size(uint32_t samples);

/* POD5 reads of several rows.  A pod5 file cuts a read into signal rows (102 400 samples by default); the four calls below take the rows
 * as the batch's entries -- one zstd frame each, dst_cap[i] = 2 x the row's samples in the int16 layout, exactly as above -- and a table
 * that says which rows form a read.  The read's signal is the concatenation of its rows, T = the sum of their samples; its chunks are
 * vbz_gpu_chunking's for T samples and its statistics those of its T values.  POD5 options only (anything else: -2, nothing launched); all
 * are asynchronous on the context's stream.
 * Bit-exactness: a read's chunks and its {shift, scale} are, bit for bit, what vbz_gpu_decompress_chunks[_norm]_batch and
 * vbz_gpu_signal_norm_batch give for the concatenated signal passed as ONE read (the chunking rules and the statistics above, the multiply
 * by the rounded reciprocal included); a read of one row is the row-wise call's.
 * result[i] stays per ROW: the verdict the row-wise call gives (descriptor checks, zstd and stream verdicts; the row's samples x E on
 * success), except that the chunk check is per READ -- chunk_first[r + 1] - chunk_first[r] != K(T), chunk_first[r] > chunk_first[r + 1]
 * or chunk_first[r + 1] > chunk_rows, and likewise a read of 2^31 samples or more, gives VBZ_DESTINATION_SIZE_ERROR to EVERY row of the
 * read, and not one byte of chunks is written for it.  read_result[k] = T x E (E = bytes per stored sample; 2 for the statistics call), or
 * the error code of the read's first failing row in row order.  A failing row inside a read leaves the read's chunk rows and its
 * shift_scale entry unspecified; its other rows keep their own verdicts, and other reads are untouched and exact.
 * first_row is untrusted and fails whole: first_row[0] != 0, a decreasing pair or first_row[n_reads] != batch->n_reads makes every
 * result[i] and read_result[k] VBZ_INPUT_SIZE_ERROR; no address is formed from the table and nothing in chunks / dst / shift_scale is
 * written (one launch checks it before any other kernel reads it).
 * A read without rows, or of empty rows only, has T = 0: no chunk, c = w = 0.  Empty rows anywhere in a read are legal, and row sample
 * counts need not be multiples of 8.  Nothing outside a read's chunk rows, the rows' slots and the shift_scale entries is written.
 * -2 (nothing launched): everything the row-wise counterparts refuse, a NULL reads, reserved != 0, a NULL first_row, n_reads > 0 with a
 * NULL table the call needs (chunk_first, chunks, read_samples, shift_scale of the statistics call), norm with format->offset or
 * format->scale.
 * vbz_gpu_pod5_read_samples_batch: read_samples[k] = the sum of the read's row_samples (device, n_rows words); 2^31 or more gives
 * VBZ_DESTINATION_SIZE_ERROR and a bad first_row VBZ_INPUT_SIZE_ERROR in every entry, both of which vbz_gpu_chunk_layout_batch counts as 0
 * chunks: its output feeds that call unchanged (chunk_first has n_reads + 1 entries, chunk_info names reads).
 * vbz_gpu_pod5_decompress_chunks_batch: chunk k of read r is row chunk_first[r] + k of chunks.  norm == NULL: format->offset / scale are
 * per READ (n_reads floats, nullable); norm != NULL: the read's own statistics, format->offset and format->scale must be NULL, and
 * shift_scale (nullable) has n_reads entries.
 * vbz_gpu_pod5_signal_norm_batch: the statistics alone, per read; result[i] is the int16 decode's for the row.
 * vbz_gpu_pod5_decompress_signal_norm_batch: every row is decoded into its own typed slot as vbz_gpu_decompress_signal_batch does (adjacent
 * slots under batch.pod5_read_layout make the read contiguous), normalised by its READ's statistics.
 * How: the rows pass the entropy stage as any batch's (rows are not routed to the large-read path); one launch then
 * gives every row its place in its read, and the svb16 store -- still one workgroup per row -- places its samples by read position: whole
 * 16-byte lines for a row that begins at a multiple of 8 samples of its read (every row behind full default-size rows), element by
 * element otherwise and wherever a line holds samples of two rows.  The counting passes run one workgroup per READ, walking its rows. */
typedef struct vbz_gpu_pod5_reads
{
    uint32_t n_reads;          /* reads the batch's rows form */
    uint32_t reserved;         /* must be 0 */
    const uint32_t* first_row; /* device, n_reads + 1 words: read k owns rows first_row[k] ... first_row[k + 1] - 1, in signal order;
                                  first_row[0] == 0, non-decreasing, first_row[n_reads] == batch->n_reads.  A read may own no row. */
    uint32_t* read_result;     /* device, n_reads words, nullable: per read, T * E on success, else the error code of its first failing row */
} vbz_gpu_pod5_reads;          /* 24 bytes */
VBZ_EXPORT int vbz_gpu_pod5_read_samples_batch(vbz_gpu_ctx* ctx, uint32_t n_rows, const uint32_t* row_samples, const vbz_gpu_pod5_reads* reads,
                                               uint32_t* read_samples);
VBZ_EXPORT int vbz_gpu_pod5_decompress_chunks_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                    const vbz_gpu_signal_format* format, const vbz_gpu_chunking* chunking,
                                                    const vbz_gpu_pod5_reads* reads, const uint64_t* chunk_first, void* chunks, uint64_t chunk_rows,
                                                    const vbz_gpu_normalization* norm, float* shift_scale);
VBZ_EXPORT int vbz_gpu_pod5_signal_norm_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                              uint32_t is_signed, const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm,
                                              float* shift_scale);
VBZ_EXPORT int vbz_gpu_pod5_decompress_signal_norm_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                         const vbz_gpu_signal_format* format, const vbz_gpu_pod5_reads* reads,
                                                         const vbz_gpu_normalization* norm, float* shift_scale);

/* Sample ranges.  No caller of the chunk and normalising calls wants the whole read: Bonito trims the start of the signal, then normalises
 * and chunks signal[trim:]; Dorado normalises over the whole read and drops signal[:trim] before it chunks; Remora and re-squiggle
 * workflows slice by the ts / ns of an earlier basecall; training loaders cut windows.  The *_range_batch calls below are the chunk and
 * statistics calls with one more argument, a per-read [begin, end) in samples.
 * The range: for a read of T samples, e = min(end[i], T), b = min(begin[i], e), T' = e - b.  The tables are untrusted and are clamped,
 * never refused: begin > end or begin >= T is an empty range, end = 0xFFFFFFFF means "to the end"; no address is formed from a table
 * value before it is clamped.  A NULL begin is 0 for every read, a NULL end the read's sample count.
 * Bit-exactness: the read's chunks, and under VBZ_GPU_RANGE_STATS_RANGE its {shift, scale}, are bit for bit what
 * vbz_gpu_decompress_chunks[_norm]_batch and vbz_gpu_signal_norm_batch give for the signal x[b:e] passed as ONE read of T' samples: the
 * chunking rules for T' (PAD, and END with end_align), the pad value, the float64 order statistics, the multiply by the rounded
 * reciprocal; T' == 0: no chunk, c = w = 0.  Under VBZ_GPU_RANGE_STATS_READ the constants are the whole read's (all T values) and only the
 * chunking sees the range.  Without norm, format->offset and format->scale apply as in the chunk call.
 * Verdicts do not change: result[i] is what the un-ranged call gives (descriptor checks, sized headers, the zstd and stream verdicts; on
 * success T x E with T the read's FULL count), and every stream is still walked to its end, so damage behind `end` keeps its verdict.  The
 * one exception is the chunk check, which is against K(T'): chunk_first entries that are not exactly the range's chunks give
 * VBZ_DESTINATION_SIZE_ERROR and not one byte of chunks is written for the read.  Nothing outside a read's K(T') chunk rows and its
 * shift_scale entry is written.
 * ranges == NULL, or begin and end both NULL, is the un-ranged call (the same kernels).  -2 (nothing launched): everything the
 * counterpart refuses, reserved != 0, an unknown stats.
 * vbz_gpu_range_samples_batch: range_samples[i] = T' for samples[i] = T (device tables of n_reads words); a samples[i] of 2^31 or more (an
 * error code) passes through unchanged, so the output feeds vbz_gpu_chunk_layout_batch as it is, and chunk_info's start samples are then
 * relative to b.
 * vbz_gpu_decompress_chunks_range_batch: the arguments of vbz_gpu_decompress_chunks_norm_batch with norm and shift_scale nullable as in
 * the POD5 chunk call (norm == NULL: the given constants), plus ranges.  vbz_gpu_signal_norm_range_batch: the statistics alone, over the
 * range (under VBZ_GPU_RANGE_STATS_READ: the un-ranged call).  The two vbz_gpu_pod5_*_range_batch calls are the same over POD5 reads of
 * several rows: the tables are per READ, in positions of the concatenated signal; result[] stays per row and read_result[] per read, both
 * as in the un-ranged calls (read_result[k] = T x E with the full T); the chunk check is per read, against K(T').
 * How: samples outside the range are decoded, because the delta chain needs them, and are neither converted, stored nor
 * counted.  With b a multiple of 8 a lane's eight samples are still one aligned 16-byte line of the range's signal and the whole-line
 * stores of the chunk call are kept; any other b stores sample by sample.  Measured on one MI355X, 65 536 reads of ~100 k samples,
 * L = 10 000, S = 9 504, PAD, float16 (tools/time_ranges.py, profiles/HISTORY.md "Sample ranges"): chunk call 11.7 ms; range call with
 * [0, T) 12.3 ms, begin = 2 000 12.2 ms, begin = 2 003 16.5 ms; [2 000, T - 2 000) with MED_MAD 18.1 ms (statistics of the range) and
 * 17.4 ms (of the read) against 16.7 ms un-ranged; int16 decode + torch slice statistics + signal decode + gather 700 ms. */
#define VBZ_GPU_RANGE_STATS_RANGE 0 /* statistics of the range's samples (Bonito: trim, then normalise) */
#define VBZ_GPU_RANGE_STATS_READ 1  /* statistics of the whole read (Dorado: normalise, then trim) */
typedef struct vbz_gpu_sample_ranges
{
    const uint32_t* begin; /* device, one word per read, nullable: 0 */
    const uint32_t* end;   /* device, one word per read, nullable: the read's sample count */
    uint32_t stats;        /* VBZ_GPU_RANGE_STATS_*; ignored without norm */
    uint32_t reserved;     /* must be 0 */
} vbz_gpu_sample_ranges;   /* 24 bytes */
VBZ_EXPORT int vbz_gpu_range_samples_batch(vbz_gpu_ctx* ctx, uint32_t n_reads, const uint32_t* samples, const vbz_gpu_sample_ranges* ranges,
                                           uint32_t* range_samples);
VBZ_EXPORT int vbz_gpu_decompress_chunks_range_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                     int sized, const vbz_gpu_signal_format* format, const vbz_gpu_chunking* chunking,
                                                     const uint64_t* chunk_first, void* chunks, uint64_t chunk_rows,
                                                     const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges);
VBZ_EXPORT int vbz_gpu_signal_norm_range_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                               uint32_t is_signed, const vbz_gpu_normalization* norm, float* shift_scale,
                                               const vbz_gpu_sample_ranges* ranges);
VBZ_EXPORT int vbz_gpu_pod5_decompress_chunks_range_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                          const vbz_gpu_signal_format* format, const vbz_gpu_chunking* chunking,
                                                          const vbz_gpu_pod5_reads* reads, const uint64_t* chunk_first, void* chunks,
                                                          uint64_t chunk_rows, const vbz_gpu_normalization* norm, float* shift_scale,
                                                          const vbz_gpu_sample_ranges* ranges);
VBZ_EXPORT int vbz_gpu_pod5_signal_norm_range_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                    uint32_t is_signed, const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm,
                                                    float* shift_scale, const vbz_gpu_sample_ranges* ranges);

/* Signal trim.  The two calls below find, on the device, the sample at which each read's signal proper begins -- the trim point the
 * basecallers cut at -- and write it to a per-read table begin[] that is, as it stands, the vbz_gpu_sample_ranges.begin of the *_range_batch
 * calls above: no host round trip lies between finding the trim and chunking signal[trim:].  They are the statistics-alone calls
 * (vbz_gpu_signal_norm_range_batch, vbz_gpu_pod5_signal_norm_range_batch) with one more pass of the svb decoder behind the counting passes;
 * the zstd stage still runs once per call.
 * The rule.  A read has T raw 16-bit values x_j (int16 or uint16 per is_signed).  {shift, scale} is the float32 pair the statistics call
 * gives for the same norm and ranges (ranges applies to the statistics only -- NULL: the whole read; either `stats` value is accepted, with
 * the meaning it has there).  With W = window, m = min_elements, t0 = min_trim, M = max_samples, f = threshold_factor:
 *   threshold   thr = float64(shift) + float64(f) * float64(scale): one multiply, then one add, each rounded to nearest even (no fused
 *               multiply-add).
 *   high        sample j is high when float64(x_j) > thr; a sample equal to thr is not.
 *   windows     N = min(M, T); nW = N > t0 ? (N - t0) / W : 0 (integer division); window k covers positions [t0 + k W, t0 + (k + 1) W) and
 *               ends at e_k = t0 + (k + 1) W.
 *   scan        walk k = 0 ... nW - 1 with seen = false.  A window that holds MORE than m high samples sets seen.  While seen is not set
 *               the walk goes on to the next window.  Once it is set (the window that set it included): a window whose last sample
 *               x[e_k - 1] is high -- whatever its count -- goes on to the next window; the first whose last sample is not high stops the walk.
 *   verdict     on the stopping window: min(t0, T) when VBZ_GPU_TRIM_REJECT_AT_END is set and e_k >= N; min(t0, T) when
 *               float64(e_k) > float64(max_fraction) * float64(T); otherwise e_k.  A walk that ends without stopping -- no peak, or a peak that
 *               never comes down -- gives min(t0, T).
 * begin[i] (device, one word per read) is the answer for read i, and 0 for a read whose result[i] is an error code.  result[i] is what the
 * statistics call gives; the pod5 call also writes read_result[k] as that call does.  shift_scale (nullable here) is written when given.
 * Nothing else is written; batch->dst may be NULL.  POD5 reads of several rows: everything is per READ, over the concatenated signal; begin
 * has n_reads entries; a read with a failing row gets 0; a bad first_row fails whole as in the statistics call, and begin is not written.
 * Both return 0 when queued, -1 for a NULL context or batch or a launch failure, and -2 (nothing launched) for everything the statistics call
 * refuses, a NULL trim or begin, a field outside its rule, reserved != 0, unknown flags, and (M - min(t0, M)) / W > 4096: a read's windows
 * must fit the counting passes' bins.
 * The tools.  With VBZ_GPU_NORM_MED_MAD or VBZ_GPU_NORM_QUANTILE as norm, W = 40, m = 3, t0 = 10, M = 8000 and f = 2.4 this is the shape of
 * the trim Bonito and Dorado apply; they differ in which samples the statistics are taken over (the range table says that) and in the two
 * rejection rules (max_fraction and VBZ_GPU_TRIM_REJECT_AT_END say those).  This library was written without either tool's source: the
 * rule above is the contract, not "what Bonito does".
 * The hand-over.  begin[] goes straight into vbz_gpu_range_samples_batch (as ranges.begin), its output into vbz_gpu_chunk_layout_batch, and
 * both into vbz_gpu_decompress_chunks_range_batch, all on the context's stream.  A caller that normalises by the whole read can hand the
 * chunk call format->offset = -shift and format->scale = float32(1 / float64(scale)) from shift_scale as given constants (norm = NULL): that
 * saves its counting passes, and the chunks are bit for bit those of VBZ_GPU_RANGE_STATS_READ.
 * How: the trim pass is one more store of the svb decoder.  It turns thr into the smallest high key once per read, counts
 * the high samples of the prefix [t0, t0 + nW W) per window in the LDS bins of the counting passes (most samples are not high and cost no
 * LDS operation), leaves the tile loop behind the prefix, and one wavefront scans the window words by ballot; on the large-read path the
 * segments add their words up in scratch and a launch of its own scans.  Measured on one MI355X, 65 536 reads of ~100 k samples, the
 * defaults above (tools/time_trim.py, profiles/HISTORY.md "Signal trim"): statistics alone 11.7 ms (MED_MAD) / 11.6 ms (QUANTILE), the trim
 * call 12.3 / 12.1 ms -- the trim pass costs about 0.5 ms, its kernel 5 - 6 % of the first counting pass's time; trim call + range_samples +
 * layout + ranged normalised chunk call 34.7 ms; int16 decode + torch median / MAD + the window walk in torch + the same chunk call 735 ms.
 * One 20 M-sample read: statistics 0.435 ms, trim call 0.439 ms. */
#define VBZ_GPU_TRIM_REJECT_AT_END 1u
typedef struct vbz_gpu_trim
{
    uint32_t window;        /* W: samples per window, 1 ... 65536 */
    uint32_t min_elements;  /* m: a window opens the peak when MORE than m of its samples are high */
    uint32_t min_trim;      /* t0: samples in front of the first window; also the answer when no trim is found */
    uint32_t max_samples;   /* M >= 1: only the first min(M, T) samples are looked at */
    float threshold_factor; /* f, finite */
    float max_fraction;     /* finite, 0 < max_fraction <= 1: a trim beyond this share of the read is rejected (1: never) */
    uint32_t flags;         /* VBZ_GPU_TRIM_* */
    uint32_t reserved;      /* must be 0 */
} vbz_gpu_trim;             /* 32 bytes */
VBZ_EXPORT int vbz_gpu_signal_trim_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                         uint32_t is_signed, const vbz_gpu_normalization* norm, const vbz_gpu_sample_ranges* ranges,
                                         const vbz_gpu_trim* trim, float* shift_scale, uint32_t* begin);
VBZ_EXPORT int vbz_gpu_pod5_signal_trim_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                              uint32_t is_signed, const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm,
                                              const vbz_gpu_sample_ranges* ranges, const vbz_gpu_trim* trim, float* shift_scale, uint32_t* begin);

/* Signal windows.  The chunk calls cut every read on the regular grid k * step.  A modification caller wants a fixed-length context around
 * every candidate site of a read, a training loader windows at recorded or random offsets: many windows per read, at positions only the
 * caller knows.  The two calls below are the ranged chunk calls with the chunking replaced by a list of windows per read.
 * The arena: `out` is a row-major [window_rows, L] arena of format->out_type (L = window_len), 16-byte aligned.  Read i owns rows
 * window_first[i] ... window_first[i + 1] - 1, and start[c] says where row c's window begins in the read's signal.
 * The rule for one position: the signal is the read's samples x[b:e) of T' = e - b samples, ranges clamped exactly as in the *_range_batch
 * calls above (ranges NULL, or both tables NULL: the whole read).  Position p of row c holds the converted sample start[c] + p of that
 * signal when 0 <= start[c] + p < T' (64-bit arithmetic), and `pad` otherwise.  So a window may hang over the front of the signal (a
 * negative start) or over its end, or lie wholly outside (all pad); windows may overlap to any degree and may repeat; T' == 0 gives rows
 * of pad.  The conversion is the signal call's, with its rounding: ((float)x + offset) * scale, the constants format->offset / scale when
 * norm is NULL, else the read's own statistics as in the *_norm calls (format->offset and scale must then be NULL, shift_scale is nullable,
 * ranges->stats has its meaning).  `pad` is rounded (to nearest even) to the output type and otherwise taken as it is.
 * The tables are untrusted.  Per read, in this order: the descriptor checks; sized, the header verdicts; then the window check, which
 * refuses window_first[i] > window_first[i + 1], window_first[i + 1] > window_rows, more than 2^31 - 1 rows of one read, and a pair
 * start[c] > start[c + 1] inside the read's rows (the starts of a read must be sorted: a lane then finds a position's windows by a walk,
 * not a search).  A read refused by it gets VBZ_DESTINATION_SIZE_ERROR and not one byte of out is written for it.  No start[] entry of a
 * read is read before its two window_first entries have passed, and no address is formed from an unchecked value.  Reads need not tile the
 * arena and are checked one by one: rows that two reads both list are written by both.
 * Verdicts otherwise are the chunk call's: result[i] = T x E with the read's FULL sample count on success, when every position of the
 * read's rows has been written; rows of a read that fails after the window check hold unspecified contents; nothing outside the rows owned
 * by reads is ever written.
 * vbz_gpu_pod5_decompress_windows_batch: the same over POD5 reads of several rows.  The constants, window_first, shift_scale and the range
 * tables are per READ, positions are those of the concatenated signal; result[] stays per row and read_result[] per read as in the POD5
 * chunk calls; the window check is per READ and gives VBZ_DESTINATION_SIZE_ERROR to every row of the read; a bad first_row fails whole.
 * Both return 0 when queued, -1 for a NULL context or batch or a launch failure, -2 (nothing launched) for everything
 * vbz_gpu_decompress_chunks_range_batch / its POD5 twin refuse, a NULL windows, window_len outside its rule, flags or reserved != 0, a NULL
 * window_first, start (when window_rows > 0) or out while the call has reads, out not 16-byte aligned, window_rows * L * E beyond 2^46 bytes.
 * How: one more store of the svb decoder, on every decode path.  A lane holds eight consecutive samples; the windows that
 * hold them are consecutive in the read's sorted list; the workgroup brackets the candidates of each tile of 2 048 samples with two
 * cursors that only advance, and a lane walks that bracket alone.  A window whose start is congruent to the
 * lane's position modulo 8 takes whole 16-byte stores; any other is stored sample by sample.  The pad positions are written by one launch
 * of its own behind the window check, a wavefront per row.  Measured on one MI355X: 65 536 reads of ~100 k samples, float16 (tools/time_windows.py, profiles/HISTORY.md
 * "Signal windows"; the parent of the commit that adds these calls is 922424a): the PAD grid L = 10 000, S = 9 504 given as windows 14.4 ms
 * against 11.2 ms for the chunk call itself and 30.0 ms for the signal call (10.6 ms) followed by a torch gather; as many windows at random
 * starts 16.8 ms against 29.5 ms unfused; L = 512 every 64 samples (coverage 8) over 8 192 reads 18.2 ms against 23.1 ms unfused -- the stores
 * dominate and the saving shrinks from 2.1 x to 1.27 x.  One 20 M-sample read: 0.354 / 0.367 / 0.487 ms against 0.424 / 0.393 / 0.748 ms. */
typedef struct vbz_gpu_windows
{
    uint32_t window_len;          /* L: samples per window, a multiple of 8, 8 <= L <= 2^20 */
    float pad;                    /* the value of positions outside the signal, rounded (RNE) to the output type */
    uint64_t window_rows;         /* rows of the arena = entries of start[] */
    const uint64_t* window_first; /* device, n_reads + 1: read i owns rows window_first[i] ... window_first[i + 1] - 1 */
    const int32_t* start;         /* device, window_rows: the first sample of each row's window, in positions of the read's signal */
    uint32_t flags;               /* must be 0 */
    uint32_t reserved;            /* must be 0 */
} vbz_gpu_windows;                /* 40 bytes */
VBZ_EXPORT int vbz_gpu_decompress_windows_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                                const vbz_gpu_signal_format* format, const vbz_gpu_windows* windows, void* out,
                                                const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges);
VBZ_EXPORT int vbz_gpu_pod5_decompress_windows_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                     const vbz_gpu_signal_format* format, const vbz_gpu_pod5_reads* reads,
                                                     const vbz_gpu_windows* windows, void* out, const vbz_gpu_normalization* norm,
                                                     float* shift_scale, const vbz_gpu_sample_ranges* ranges);

/* Signal events.  Every call above gives samples.  A modification caller that reduces a read to one signal level per base along the
 * basecaller's move table, a re-squiggle or event-align tool, per-k-mer level QC want one record {mean, sd, length} per EVENT, the caller
 * saying where each event begins.  The two calls below decode and reduce in one pass of the svb decoder: no sample is stored anywhere.
 * The signal is the read's samples x[b:e) of T' = e - b samples, ranges clamped exactly as in the *_range_batch calls (ranges NULL, or both
 * tables NULL: the whole read).
 * The rows: read i owns rows c0 = event_first[i] ... c1 - 1 = event_first[i + 1] - 1 of `out` (and of `moments`).  Row c covers the
 * positions [a, z) of the signal, a = min(start[c], T'), z = min(start[c + 1], T') when c + 1 < c1 and z = T' for the read's last row.
 * Samples in front of the read's first start belong to no event; equal starts give an empty event; a start at or behind T' (0xFFFFFFFF
 * included) gives an empty event.
 * The moments are exact integers: n = z - a, S1 = sum x_j, S2 = sum x_j^2 over the row's positions, x_j the raw 16-bit value (int16, or
 * uint16 with format->is_signed == 0).  n < 2^31 keeps |S1| < 2^47 and S2 <= 2^63: nothing wraps.  moments[c] = {S1, S2} when `moments`
 * is given (NULL: they live in scratch of the context).
 * The record, in float64, every operation rounded to nearest even and none fused: m = float64(S1) / float64(n);
 * v = float64(S2) / float64(n) - m * m, 0 when negative; r = sqrt(v), correctly rounded; with the read's constants o and s,
 * mean = float32((m + float64(o)) * float64(s)) and sd = float32(r * fabs(float64(s))).  o and s are format->offset[i] / scale[i] (NULL:
 * 0 and 1) when norm is NULL; otherwise o = -shift and s = float32(1 / float64(scale)) from the read's own statistics as in the *_norm
 * calls (format->offset and scale must then be NULL, shift_scale is nullable, ranges->stats has its meaning).  n == 0 gives
 * mean = sd = +0; `zero` is written 0.  format->out_type must be VBZ_GPU_SIGNAL_F32.  Integer sums do not depend on the order of the
 * additions: the records are numpy's bit for bit (tests/events_ref.py).
 * Verdicts: result[i] is what the statistics-alone call gives -- the int16 decode's verdict, T x 2 with the read's FULL sample count on
 * success.  The tables are untrusted.  Per read, in this order: the descriptor checks; sized, the header verdicts; then the event check,
 * which is the window check's rule: event_first[i] > event_first[i + 1], event_first[i + 1] > event_rows, more than 2^31 - 1 rows of one
 * read, or a pair start[c] > start[c + 1] (unsigned) inside the read's rows.  A read refused by it gets VBZ_DESTINATION_SIZE_ERROR and not
 * one byte of out or moments is written for it.  No start[] entry of a read is read before its two event_first entries have passed, and
 * no address is formed from an unchecked value.  Rows of a read that fails after the event check hold unspecified contents; nothing
 * outside the rows owned by reads, and the shift_scale entries, is ever written; batch->dst may be NULL.
 * vbz_gpu_pod5_signal_events_batch: the same over POD5 reads of several rows.  event_first, the constants, shift_scale and the range
 * tables are per READ, positions are those of the concatenated signal; result[] stays per row and read_result[] per read as in the POD5
 * statistics call; the event check is per READ and reaches every row of the read; a bad first_row fails the whole call.
 * Both return 0 when queued, -1 for a NULL context or batch or a launch failure, -2 (nothing launched) for everything
 * vbz_gpu_signal_norm_range_batch / its POD5 twin refuse (a NULL norm is allowed here), a NULL events, flags or reserved != 0, an out_type
 * other than F32, a NULL event_first, start (when event_rows > 0) or out while the call has reads, out or moments not 16-byte aligned,
 * event_rows * 16 beyond 2^46 bytes.
 * How: one more sink of the svb decoder, on every decode path.  A lane holds eight consecutive samples; they lie in
 * consecutive events of the read's sorted list; the workgroup brackets the starts inside each tile of 2 048 samples with two cursors that
 * only advance, a lane bisects that bracket for its first sample's event and adds up each run of samples that share an event, sum x in
 * 32 bits and sum x^2 in 64, and adds the run to the row's two 64-bit words with global integer adds.  The words are zeroed by a launch
 * behind the event check; one thread per row derives n from the starts, applies the formulas and writes one 16-byte record behind the
 * pass.  Measured on one MI355X (tools/time_events.py, profiles/HISTORY.md "Signal events"; the parent of the commit that adds these
 * calls is 7d0484f): 8 192 reads of ~100 k samples cut into 51.2 M events of random dwell 2 ... 30, records and moments: 13.75 ms with
 * given constants against 1.66 ms for the int16 decode alone and 30.72 ms for the int16 decode followed by a torch reduction (integer
 * cumulative sums, float64 arithmetic); 14.41 ms with MED_MAD against 2.03 ms for the statistics alone and 32.62 ms unfused.  One
 * 20 M-sample read: 0.689 / 0.337 / 1.090 ms.  Fusing wins 2.2 x over the unfused route and stays 8 x above the decode: the event pass,
 * with its global adds, is 10.4 of the 13.75 ms (DESIGN.md 4.19 says what comes next). */
typedef struct vbz_gpu_events
{
    uint64_t event_rows;         /* entries of start[] = rows of out / moments */
    const uint64_t* event_first; /* device, n_reads + 1: read i owns rows event_first[i] ... event_first[i + 1] - 1 */
    const uint32_t* start;       /* device, event_rows: first sample of each event, in positions of the read's signal */
    uint32_t flags;              /* must be 0 */
    uint32_t reserved;           /* must be 0 */
} vbz_gpu_events;                /* 32 bytes */
typedef struct vbz_gpu_event
{
    float mean;    /* ((S1 / n) + o) * s */
    float sd;      /* sqrt(S2 / n - (S1 / n)^2) * |s|: the population standard deviation */
    uint32_t n;    /* samples of the event */
    uint32_t zero; /* written 0 */
} vbz_gpu_event;   /* 16 bytes */
typedef struct vbz_gpu_event_moments
{
    int64_t sum;    /* S1 */
    uint64_t sumsq; /* S2 */
} vbz_gpu_event_moments; /* 16 bytes */
VBZ_EXPORT int vbz_gpu_signal_events_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                           const vbz_gpu_signal_format* format, const vbz_gpu_events* events, vbz_gpu_event* out,
                                           vbz_gpu_event_moments* moments, const vbz_gpu_normalization* norm, float* shift_scale,
                                           const vbz_gpu_sample_ranges* ranges);
VBZ_EXPORT int vbz_gpu_pod5_signal_events_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                const vbz_gpu_signal_format* format, const vbz_gpu_pod5_reads* reads,
                                                const vbz_gpu_events* events, vbz_gpu_event* out, vbz_gpu_event_moments* moments,
                                                const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges);

/* Signal segmentation.  The event calls above take the events' starts from the caller.  A re-squiggle or event-align tool has no move
 * table to take them from: it segments the raw signal itself.  The two calls below find every read's event starts on the device and
 * write them in the layout vbz_gpu_events reads as it stands: decode -> segment -> per-event records stays on the context's stream, and
 * no sample is stored anywhere.  This library was written without the source of any segmentation tool: the rule below is the contract.
 * It is the familiar two-window t-statistic with a local non-maximum suppression as the picker, so every position's verdict is a function
 * of a bounded neighbourhood and the result is reproducible bit for bit (tests/segment_ref.py).
 * The signal is the read's samples x[b:e) of T' = e - b raw 16-bit values (int16, or uint16 with is_signed == 0), ranges clamped exactly
 * as in the *_range_batch calls (ranges NULL, or both tables NULL: the whole read; ranges->stats is ignored).  Positions q are positions
 * in this signal, the convention of vbz_gpu_events.start.
 * Parameters: the short detector has window w1 = short_window, 1 ... 32, and threshold t1 = short_threshold; the long one w2 =
 * long_window, 0 ... 32 (0: there is no second detector, long_threshold is ignored) and t2 = long_threshold; thresholds are finite
 * float32 > 0; the radius r = radius is 1 ... 32.
 * Detector d (window w, threshold t): s_d[q] = 0 unless w <= q <= T' - w.  For such a q, in exact integers: A = sum x[q - w : q),
 * B = sum x[q : q + w), A2 and B2 the sums of squares over the same two windows, N = w (A - B)^2, D = max(w (A2 + B2) - A^2 - B^2, 1).
 * With w <= 32, N < 2^47 and D < 2^43: both fit int64 and are exact in float64.  s_d[q] = (float64(N) / float64(D)) / (float64(t) *
 * float64(t)): one multiply and two divisions, each rounded to nearest even, none fused.  N / D is the squared t-statistic
 * w dmean^2 / (var_a + var_b); it does not change under offset and scale, so the call takes no format and no normalisation.  D = 0 (both
 * windows constant) is taken as 1: a step between two plateaus scores as high as the integers allow, a flat stretch scores 0.
 * The score is s[q] = max(s_1[q], s_2[q]).
 * Boundary: q in 1 ... T' - 1 is a boundary when s[q] >= 1, s[q] > s[j] for every j in [max(q - r, 0), q), and s[q] >= s[j] for every j
 * in (q, min(q + r, T')].  Of equal scores the first wins: a later equal score within r of an earlier one is suppressed, whether or not
 * the earlier one is itself a boundary.  Two boundaries are therefore more than r apart.
 * The rows of a read: none when T' == 0; otherwise row 0 starts at 0 and one row follows per boundary, ascending.  Hence
 * rows <= 2 + T' / (r + 1) (integer division): a caller sizes start[] from that bound -- and from vbz_gpu_range_samples_batch's output
 * when ranges are used -- without a synchronisation.
 * event_first[0] = 0 and event_first[i + 1] - event_first[i] is read i's row count: 0 for a read whose decode verdict is an error and for
 * a POD5 read with a failing row.  The table is always complete and holds the true counts, whatever start_cap is.  Read i's starts are
 * written to start[event_first[i] ... event_first[i + 1]) when event_first[i + 1] <= start_cap; a read that does not fit gets
 * VBZ_DESTINATION_SIZE_ERROR (on every row of a POD5 read, and its read_result) and not one word of start is written for it; nothing
 * beyond start_cap and no entry owned by no fitting read is ever written.  start == NULL with start_cap == 0 is the count-only call: it
 * writes event_first alone and leaves the verdicts alone.  result[i] is otherwise what the statistics-alone call gives: the int16
 * decode's verdict, T x 2 with the read's FULL sample count on success; the POD5 twin writes read_result[] as that call does, its tables
 * (event_first, ranges) are per READ, positions those of the concatenated signal, and a bad first_row fails the whole call with nothing
 * written.  A read whose bit map (below) finds no room in the call's scratch -- possible only when the int16 layout's slots overlap --
 * gets VBZ_OUT_OF_MEMORY_ERROR.  batch->dst may be NULL.
 * Both return 0 when queued, -1 for a NULL context or batch or a launch failure, -2 (nothing launched) for everything
 * vbz_gpu_signal_norm_range_batch / its POD5 twin refuse about the batch, the options, `reads` and `ranges`, a NULL segmentation or
 * event_first, start == NULL with start_cap != 0, a window, the radius or a threshold outside its rule (NaN and infinities included),
 * flags != 0, start_cap * 4 beyond 2^46 bytes.
 * The hand-over: event_first and start go as they are into a vbz_gpu_events of the event calls, event_rows being start_cap (or the total
 * when the caller has read it), with the same ranges, on the same stream.
 * How: kernels of their own around the svb decoder's shared walks, with the first sink that needs a neighbourhood of
 * each sample.  One workgroup walks a read's whole signal in order -- on every path: the long reads of the large-read path and POD5 reads
 * of several rows included, which is what is built; spreading one long read over workgroups with seams between them is not -- and stages
 * each tile of 2 048 samples in an LDS ring indexed by signal position.  Behind a barrier a lane scores eight consecutive positions,
 * sliding the four window sums, into a second ring of float64 scores; the two divisions are made only where N >= 0.99 D t^2.  Behind a
 * second barrier a lane applies the boundary test to a group of eight positions and writes one byte of the read's bit map in scratch (one
 * bit a position, 1/16 of the int16 arena).  A count launch that reads result[] first, the scan and an emit launch (one workgroup per
 * read, rank by rank) follow behind everything the call has queued.  Measured on one MI355X (tools/time_segment.py, profiles/HISTORY.md
 * "Signal segmentation"; the parent of the commit that adds these calls is d26a89f; median of 20, every table checked bit for bit against
 * the unfused route): 8 192 step-signal reads of ~100 k samples, w = (3, 6), t = (4, 9), r = 2, 66.0 M rows: 12.77 ms against 5.18 ms for
 * the int16 decode alone and 278.8 ms for the int16 decode followed by torch (integer cumulative sums, float64 scores, max_pool1d,
 * nonzero); followed by the event call on its tables 30.36 ms.  One 20 M-sample read: 99.99 ms against 0.648 ms and 7.77 ms -- one
 * workgroup walks it, and there fusing loses 12.9 x to the unfused route. */
typedef struct vbz_gpu_segmentation
{
    uint32_t short_window;   /* w1: 1 ... 32 */
    uint32_t long_window;    /* w2: 0 (no second detector) or 1 ... 32 */
    float short_threshold;   /* t1: finite, > 0 */
    float long_threshold;    /* t2: finite, > 0; ignored when long_window == 0 */
    uint32_t radius;         /* r: 1 ... 32 */
    uint32_t flags;          /* must be 0 */
    uint64_t start_cap;      /* entries of start[] */
} vbz_gpu_segmentation;      /* 32 bytes */
VBZ_EXPORT int vbz_gpu_signal_segment_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                            uint32_t is_signed, const vbz_gpu_sample_ranges* ranges, const vbz_gpu_segmentation* segmentation,
                                            uint64_t* event_first, uint32_t* start);
VBZ_EXPORT int vbz_gpu_pod5_signal_segment_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                 uint32_t is_signed, const vbz_gpu_pod5_reads* reads, const vbz_gpu_sample_ranges* ranges,
                                                 const vbz_gpu_segmentation* segmentation, uint64_t* event_first, uint32_t* start);

/* Signal spans.  Where a read's signal leaves its working band: open-pore spikes between molecules (read splitting), stalls and adapter
 * plateaus (stretches below a level for at least so many samples), saturation at the ADC rails.  All are one primitive -- take the
 * positions whose raw value lies above or below a per-read threshold, merge hits that are at most a gap apart, drop runs that are too
 * short -- and the two calls below do it on the device with no sample stored.  The trim call above is a prefix-only, one-answer form of
 * it.  This library was written without the source of any read splitter: the rule below is the contract (tests/spans_ref.py).
 * The signal is the read's samples x[b:e) of T' = e - b raw 16-bit values (int16, or uint16 with is_signed == 0), ranges clamped exactly
 * as in the *_range_batch calls (ranges NULL, or both tables NULL: the whole read).  Positions q are positions in this signal.
 * The threshold: thr = float64(a) + float64(f) * float64(w), f = threshold_factor: one multiply, then one add, each rounded to nearest
 * even, none fused (the trim call's expression).  With `norm`, {a, w} is the read's {shift, scale} exactly as the statistics-alone call
 * gives it (vbz_gpu_signal_norm_range_batch with the same norm and ranges: ranges->stats has its usual meaning), shift_scale is written
 * when given, and spans->level must be NULL.  Without `norm` (NULL), {a, w} = level[i] is given in raw counts, no counting pass runs,
 * shift_scale is ignored and level must not be NULL: a shift_scale table from an earlier statistics call is a valid level, and a caller
 * with calibrated units passes a = pA / scale - offset, w = 0.  A NaN thr makes nothing in; +inf and -inf behave as the comparison says.
 * In: in(q) holds when q >= p0 = ignore_prefix and float64(x[q]) > thr (VBZ_GPU_SPAN_ABOVE) or float64(x[q]) < thr (VBZ_GPU_SPAN_BELOW).
 * The comparison is strict: a sample equal to thr is not in.
 * Spans: walk the in-positions in ascending order.  Two consecutive in-positions q < q' belong to one span when q' - q - 1 <= D,
 * D = merge_gap, 0 ... 65535.  A span is [first, last + 1).  Spans with last + 1 - first < m, m = min_length, 1 ... 2^31 - 1, are
 * dropped: the length test comes after the merge.  Equivalently a span opens at an in-position with no in-position in the D + 1
 * positions before it and closes behind an in-position with none in the D + 1 positions after it.  Hence
 * spans <= (T' + D + 1) / (m + D + 1) by integer division: a caller sizes edge[] -- two entries a span -- from that bound (and from
 * vbz_gpu_range_samples_batch's output when ranges are used) without a synchronisation.
 * The rows: span k of read i is the pair edge[edge_first[i] + 2k] = begin, edge[edge_first[i] + 2k + 1] = end; rows ascend and
 * end <= T'.  edge_first[0] = 0 and edge_first[i + 1] - edge_first[i] is twice the read's span count: 0 for a read whose decode verdict
 * is an error and for a POD5 read with a failing row.  The table is always complete and holds the true counts, whatever edge_cap is.
 * Read i's pairs are written when edge_first[i + 1] <= edge_cap; a read whose rows end beyond edge_cap gets VBZ_DESTINATION_SIZE_ERROR
 * (on every row of a POD5 read, and its read_result) and not one word of edge is written for it; nothing beyond edge_cap and no entry
 * owned by no fitting read is ever written.  edge == NULL with edge_cap == 0 is the count-only call: it writes edge_first alone and
 * leaves the verdicts alone.  result[i] is otherwise what the statistics-alone call gives: the int16 decode's verdict, T x 2 with the
 * read's FULL sample count on success; the POD5 twin writes read_result[] as the POD5 statistics call does, its tables (edge_first,
 * level, shift_scale, ranges) are per READ, positions those of the concatenated signal, and a bad first_row fails the whole call with
 * nothing written.  A read whose bit map (below) finds no room in the call's scratch -- possible only when the int16 layout's slots
 * overlap -- gets VBZ_OUT_OF_MEMORY_ERROR.  batch->dst may be NULL.
 * Both return 0 when queued, -1 for a NULL context or batch or a launch failure, -2 (nothing launched) for everything
 * vbz_gpu_signal_norm_range_batch / its POD5 twin refuse about the batch, the options, `reads` and `ranges` (a NULL norm is allowed
 * here; a norm that is given must pass its rules), a NULL spans or edge_first, an unknown direction, merge_gap > 65535, min_length 0 or
 * above 2^31 - 1, a threshold_factor that is not finite, flags != 0, level NULL without norm or not NULL with it, edge == NULL with
 * edge_cap != 0, edge_cap * 4 beyond 2^46 bytes.
 * The hand-over: edge_first and edge are a vbz_gpu_events as they stand -- event_first, start, event_rows = edge_cap (or the total when
 * the caller has read it) -- with the same ranges, on the same stream.  Even rows of a read are then the spans' records (mean, sd,
 * dwell), odd rows the stretches between spans, the last odd row running to T': for a split read those stretches are its sub-reads,
 * and window starts for the windows call are built from them.  (The samples in front of the first span belong to no row.)
 * How: one more sink of the svb decoder, and the cheap one: a position's bit depends on that sample alone, so there is
 * no neighbourhood, no LDS and no seam.  Once per read the threshold becomes an integer bound on the 16-bit key; a lane turns its eight
 * samples into eight bits with integer compares and stores one byte of the read's bit map in scratch (one bit per position of the READ,
 * 1/16 of the int16 arena).  The pass runs on the one-workgroup path, on every SEGMENT of the large-read path (a 20 M-sample read is
 * spread over ~1 200 workgroups) and over POD5 rows and reads; with `norm` it runs behind the last counting pass.  A count launch that
 * reads result[] first (one workgroup per read walks the map a word a thread, carrying the last in-position and the open span's begin
 * with two running maxima), the scan, and an emit launch that makes the same walk follow behind everything the call has queued.
 * Measured on one MI355X (tools/time_spans.py, profiles/HISTORY.md "Signal spans"; the parent of the commit that adds these calls is bf9fbf2;
 * median of 20, calls alternating in one process, every table checked bit for bit against the unfused route): 65 536 synthetic reads of
 * ~100 k samples with three planted plateaus each, ABOVE, MED_MAD, f = 6, D = 50, m = 5, 196 608 spans: 19.77 ms with the normalisation
 * against 11.44 ms for the statistics-alone call and 11.65 ms for the trim call; 14.94 ms with given constants against 10.25 ms for the
 * int16 decode; 194.3 ms for the unfused route (statistics, int16 decode, torch compare, nonzero, diff, merge and filter).  The span pass
 * costs what the int16 store pass costs (7.4 - 7.6 ms against 7.4 - 8.4 ms by the library's labels: the decode bounds both, not the
 * store); count + scan + emit cost 5.1 ms.  One 20 M-sample read: 3.68 ms against 0.44 ms for the statistics alone and 9.50 ms unfused --
 * the pass itself adds 0.02 ms there (it is spread over 1 221 segments); the rest is the two one-workgroup walks of count and emit. */
#define VBZ_GPU_SPAN_ABOVE 0u   /* a sample is "in" when float64(x) >  thr */
#define VBZ_GPU_SPAN_BELOW 1u   /* a sample is "in" when float64(x) <  thr */
typedef struct vbz_gpu_spans
{
    uint32_t direction;      /* VBZ_GPU_SPAN_* */
    uint32_t merge_gap;      /* D: 0 ... 65535 */
    uint32_t min_length;     /* m: 1 ... 2^31 - 1 */
    uint32_t ignore_prefix;  /* p0: positions q < p0 of the signal are never in */
    float threshold_factor;  /* f, finite */
    uint32_t flags;          /* must be 0 */
    const float* level;      /* device, n_reads x {float a, float w}; required when norm is NULL, must be NULL otherwise */
    uint64_t edge_cap;       /* entries of edge[] */
} vbz_gpu_spans;             /* 40 bytes */
VBZ_EXPORT int vbz_gpu_signal_spans_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                          uint32_t is_signed, const vbz_gpu_normalization* norm, float* shift_scale,
                                          const vbz_gpu_sample_ranges* ranges, const vbz_gpu_spans* spans, uint64_t* edge_first, uint32_t* edge);
VBZ_EXPORT int vbz_gpu_pod5_signal_spans_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                               uint32_t is_signed, const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm,
                                               float* shift_scale, const vbz_gpu_sample_ranges* ranges, const vbz_gpu_spans* spans,
                                               uint64_t* edge_first, uint32_t* edge);

/* Signal match.  Finding a known squiggle inside the start of every read: signal-space barcode demultiplexing, adapter location and target
 * filtering all reduce to it.  The calls below run a subsequence DTW of every read's quantised, normalised prefix against every row of a
 * matrix of reference squiggles, on the device.  This library was written without the source of any demultiplexer or squiggle filter: the
 * rule below is the contract (tests/match_ref.py).
 * Query.  The signal is the read's samples x[b:e) of T' = e - b values, ranges clamped exactly as in the *_range_batch calls.  The query
 * is its first n = min(T', N) samples, N = query_len.  Sample j is converted as the windows call converts it: z_j = ((float)x_j + o) * s in
 * float32, each operation rounded to nearest even, none fused; o and s are format->offset / scale when norm is NULL, otherwise the read's
 * own statistics exactly as in the *_norm calls (o = -shift, s = float32(1 / float64(scale)); ranges->stats has its meaning).  It is then
 * quantised: v = z_j * quant (one float32 multiply, RNE); k_j = 0 when v is NaN, otherwise clamp(rint(v), -127, 127), rint to nearest
 * even, +-inf giving +-127.  quant is a finite float32 > 0 (levels per unit; 32 suits MAD-normalised signal).
 * References.  R = n_refs rows of int8 in a device matrix ref[R][ref_stride]; row r has M_r = ref_len[r] valid entries, values taken as
 * they are (-128 is legal).  ref_len is an untrusted device table: M_r == 0 or M_r > ref_stride makes column r of the output
 * {0xFFFFFFFF, 0} for every read, and no address is formed from it.
 * Cost.  For reference r_0 ... r_{M-1} and query k_0 ... k_{n-1}, c(i, j) = |r_i - k_j|, in integers:
 *   D[0][j] = c(0, j)                                             (the alignment may start anywhere in the query)
 *   D[i][0] = c(i, 0) + D[i-1][0]
 *   D[i][j] = c(i, j) + min(D[i-1][j-1], D[i-1][j], D[i][j-1])
 *   cost = min_j D[M-1][j]                                        (it may end anywhere)
 *   end = 1 + the SMALLEST j that attains it
 * The whole reference is aligned to a stretch of the query that ends at `end` (exclusive).  D[i][j] <= 255 (i + 1) < 2^20, so nothing
 * wraps; integer minima do not depend on evaluation order, so the answer is reproducible bit for bit.  n == 0 gives {0xFFFFFFFF, 0}; so
 * does an empty range, and so does a read whose verdict is an error.
 * Output.  out is a row-major [n_reads, R] arena of vbz_gpu_match_hit (8 bytes), 16-byte aligned.  EVERY entry is written by every call
 * that launches; nothing else is written, apart from query and shift_scale.
 * vbz_gpu_match_batch is the stage-level entry: query is a row-major [n_reads, N] float32 arena, 16-byte aligned -- exactly what the
 * windows call writes for one window per read -- and valid[i] (device, untrusted) is clamped to N; 0 gives the empty verdict.
 * vbz_gpu_signal_match_batch and its POD5 twin are the windows call (one row per read, start 0, L = N, pad +0, under window tables of the
 * library's own, so the window check cannot fail) followed by the match launch on the context's stream.  valid[i] is derived on the device
 * from the verdicts and the range tables; an error gives 0.  query is REQUIRED and caller-owned (n_reads x N x 4 bytes): the hand-over
 * between the two stages and an output the caller may keep; positions at and behind T' hold +0, rows of failing reads are unspecified.
 * format->out_type must be F32.  result[] / read_result[] are exactly the windows call's, shift_scale is as there.  The POD5 tables are per
 * READ over the concatenated signal, and a bad first_row fails the whole call: out still gets the empty verdict everywhere and query is
 * not written.
 * All return 0 when queued, -1 for a NULL context or batch or a launch failure, -2 (nothing launched, nothing written) for everything the
 * windows call / its POD5 twin refuse about batch, options, format, norm, ranges and reads; a NULL match, ref, ref_len, query or out (the
 * stage entry: valid) while the call has reads; query_len, n_refs, ref_stride or quant outside their rule (NaN and infinities included);
 * flags or reserved != 0; ref, query or out not 16-byte aligned; n_reads * R * 8 or n_reads * N * 4 beyond 2^46 bytes; an out_type other
 * than F32.
 * How: no new sink of the svb decoder -- the prefix costs N x 4 bytes a read against a DP of N x M x R cells.  One
 * wavefront per (read, reference) pair, the four wavefronts of a workgroup sharing a read.  The lanes are the reference: lane l owns
 * rows l c ... l c + c - 1, c = 1, 2, 4, 8, 16 or 32 by M.  The schedule is systolic: at step t lane l takes sample t - l; a step is two
 * wave_shr:1 DPP moves (the lane below's last row, and the sample) and c cells in registers, each a v_min3_u32 and a v_msad_u8.  Rows
 * behind the reference's end cost nothing, so the last row of the lane that holds row M - 1 is the running minimum and the answer is
 * tracked on one register with a strict <.  No LDS, no barrier.
 * Measured on one MI355X (tools/time_match.py, profiles/HISTORY.md "Signal match"; the parent of the commit that adds these calls is
 * 0465232; median of 20, calls alternating in one process, every hit checked bit for bit against the unfused route): 8 192 synthetic
 * reads of ~100 k samples, MED_MAD, N = 2 048 behind the trim call's begin[], quant 32.  R = 24 references of M = 400: 18.00 ms
 * against 2.64 ms for the windows call alone, 15.39 ms for the stage entry alone and 2 080 ms for the unfused route (the windows call,
 * then a torch DTW over all pairs, one step per anti-diagonal); R = 96: 64.00 / 2.66 / 61.38 / 7 693 ms; R = 4 of M = 2 048: 10.74 /
 * 2.74 / 8.15 / 2 854 ms.  That is 10.5 T cells/s at M = 400 and 16.9 T at M = 2 048, against an issue bound -- the kernel's own 9 + 2 c
 * VALU instructions a step at 4.1 cycles each -- of 9.6 T and 16.8 T: the kernel stands at its bound (a little above it at c = 8,
 * where three of the 25 instructions are moves that cost 2.2 cycles).  One 20 M-sample read: 0.63 / 0.49 / 0.16 / 168 ms at R = 24 --
 * 24 wavefronts cannot fill 1 024 SIMDs; the stage entry is then the latency of one wavefront's 2 447 steps. */
typedef struct vbz_gpu_match
{
    uint32_t query_len;      /* N: a multiple of 8, 8 ... 65536 */
    uint32_t n_refs;         /* R: 1 ... 4096 */
    uint32_t ref_stride;     /* bytes per row of ref: a multiple of 16, 16 ... 2048 */
    uint32_t flags;          /* must be 0 */
    float quant;             /* finite, > 0 */
    uint32_t reserved;       /* must be 0 */
    const int8_t* ref;       /* device, 16-byte aligned, n_refs x ref_stride */
    const uint32_t* ref_len; /* device, n_refs words */
} vbz_gpu_match;             /* 40 bytes */
typedef struct vbz_gpu_match_hit
{
    uint32_t cost; /* min_j D[M-1][j]; 0xFFFFFFFF: the empty verdict */
    uint32_t end;  /* 1 + the smallest j that attains it; 0: the empty verdict */
} vbz_gpu_match_hit; /* 8 bytes */
VBZ_EXPORT int vbz_gpu_match_batch(vbz_gpu_ctx* ctx, uint32_t n_reads, const float* query, const uint32_t* valid, const vbz_gpu_match* match,
                                   vbz_gpu_match_hit* out);
VBZ_EXPORT int vbz_gpu_signal_match_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                          const vbz_gpu_signal_format* format, const vbz_gpu_normalization* norm, float* shift_scale,
                                          const vbz_gpu_sample_ranges* ranges, const vbz_gpu_match* match, float* query, vbz_gpu_match_hit* out);
VBZ_EXPORT int vbz_gpu_pod5_signal_match_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                               const vbz_gpu_signal_format* format, const vbz_gpu_pod5_reads* reads,
                                               const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges,
                                               const vbz_gpu_match* match, float* query, vbz_gpu_match_hit* out);

/* Signal match with the start of the aligned stretch.  The three calls below are the three above with one more answer per pair: where the
 * stretch that `end` closes begins.  Query, quantisation, references, cost and `end` are exactly those of vbz_gpu_match; the arguments,
 * the refusals and the return codes are those of their twins (vbz_gpu_match is the same 40 bytes, flags and reserved 0).  The rule
 * (tests/match_span_ref.py):
 *   A warping path of a pair runs from (0, s) to (M - 1, e - 1) in steps (i+1, j), (i, j+1), (i+1, j+1); horizontal steps inside row 0
 *   count: a path may sit on row 0 for several samples.  start = the SMALLEST s over all paths of cost `cost` that end at column end - 1.
 *   The reference is aligned to the query's samples [start, end); start < end always.
 * As a DP over pairs P = (cost, start) ordered lexicographically, cost first and then start:
 *   P[0][j] = (c(0, j), j)                   if j == 0 or P[0][j-1].cost > 0
 *           = (c(0, j), P[0][j-1].start)     if P[0][j-1].cost == 0                 (equal cost, smaller start)
 *   P[i][j] = c(i, j) + lexmin(P[i-1][j-1], P[i-1][j], P[i][j-1])                   (the cost is added to the first component)
 * Adding one cell's cost to all three candidates keeps their order, so this DP is the minimum over all paths.  The first column that
 * attains the minimum cost also holds the smallest start of all columns that attain it (a path that starts left of another and ends right
 * of it shares a cell with it, and swapping tails there gives two paths of the minimum cost), so (end, start) is the lexicographic minimum
 * of the last row's pairs at its first column.  This holds for the smallest start only, which is why the rule is the smallest.
 * The empty verdict is {0xFFFFFFFF, 0, 0, 0}, under the conditions of the calls above: n == 0, an empty range, a read whose verdict is an
 * error, M_r == 0 or M_r > ref_stride.
 * Output.  out is a row-major [n_reads, R] arena of vbz_gpu_match_span (16 bytes), 16-byte aligned; EVERY entry is written by every call
 * that launches, by one 16-byte store, `zero` as 0.  -2 as for the twins, the size rule being n_reads * R * 16 beyond 2^46 bytes.
 * How ("The start").  A cell is the key cost << sb | start in one 32-bit word, sb = ceil(log2 N): v_min3_u32 over keys is
 * the lexicographic minimum, and schedule, lanes and registers are those of the kernel above.  Lane 0's incoming pair is the key (0, j);
 * a cell is v_min3_u32 and v_sad_u32 over levels shifted into the cost field, and the row that holds the answer is chosen once, by a
 * scalar switch, not selected every step.  That packed kernel runs when 255 ref_stride < 2^(31 - sb) (ref_stride 2 048 up to
 * N = 4 096, 400 up to 16 384, 128 up to 65 536); every other call inside the limits runs a second kernel that keeps the pair in a 64-bit
 * key.  The host chooses between them from query_len and ref_stride alone; no call is refused for its size.
 * Measured on one MI355X (tools/time_match.py, profiles/match_span_time.json; workload and shapes of the calls above, median of 20, the
 * calls alternating in one process, every (cost, end) checked bit for bit against the cost-only call of the same run): the span stage
 * entry 15.79 ms against 15.34 ms at R = 24, M = 400 (1.03 x), 62.92 against 61.13 ms at R = 96 (1.03 x), 8.11 against 8.03 ms at R = 4,
 * M = 2 048 (1.01 x); the fused span call 18.46 / 65.70 / 10.83 ms.  That is the ratio of the kernels' instruction counts, 10 + 2 c against
 * 9 + 2 c VALU instructions a step, and 1.00 - 1.05 of the packed kernel's own issue bound; running the cost-only kernel forward and
 * reversed, the only other way to a start, costs 1.94 - 1.98 times as much. */
typedef struct vbz_gpu_match_span
{
    uint32_t cost;  /* as vbz_gpu_match_hit; 0xFFFFFFFF: the empty verdict */
    uint32_t end;   /* as vbz_gpu_match_hit; 0: the empty verdict */
    uint32_t start; /* the smallest start of a path of that cost to end - 1; start < end */
    uint32_t zero;  /* written 0 */
} vbz_gpu_match_span; /* 16 bytes */
VBZ_EXPORT int vbz_gpu_match_span_batch(vbz_gpu_ctx* ctx, uint32_t n_reads, const float* query, const uint32_t* valid, const vbz_gpu_match* match,
                                        vbz_gpu_match_span* out);
VBZ_EXPORT int vbz_gpu_signal_match_span_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                               const vbz_gpu_signal_format* format, const vbz_gpu_normalization* norm, float* shift_scale,
                                               const vbz_gpu_sample_ranges* ranges, const vbz_gpu_match* match, float* query,
                                               vbz_gpu_match_span* out);
VBZ_EXPORT int vbz_gpu_pod5_signal_match_span_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                    const vbz_gpu_signal_format* format, const vbz_gpu_pod5_reads* reads,
                                                    const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges,
                                                    const vbz_gpu_match* match, float* query, vbz_gpu_match_span* out);

/* Signal match: the warping path of chosen pairs.  The span calls say which reference a read carries and where; these two stage-level
 * calls say which samples belong to which reference level, for the pairs the caller lists -- typically the one winner per read -- without
 * the arena or the query crossing to the host: span -> best -> path are three queued calls on one stream.
 * The rule (tests/match_path_ref.py).  A pair names a read, a reference and a window [a, b) of the read's query, 0 <= a < b <= n,
 * n = min(valid[read], N).  Query, quantisation, references and c(i, j) are exactly vbz_gpu_match's.  Over the window's columns alone run the
 * span rule's DP of pairs P = (cost, start), ordered lexicographically: row 0 at column a is (c(0, a), a), a path may sit on row 0, and
 * nothing left of a exists.  The path is the backtrace from cell (M - 1, b - 1):
 *   at (i, j) with i > 0, j > a: step to the FIRST of diagonal (i-1, j-1), up (i-1, j), left (i, j-1) whose P equals the lexicographic
 *                                minimum of the three;
 *   at j == a, i > 0:            step up;
 *   in row 0:                    step left while j > a and P[0][j-1].cost == 0; otherwise stop: that column is the path's start.
 * The answer per pair is a hit {cost, end, start, rows} -- cost = P[M-1][b-1].cost, end = b, start = the column where the backtrace stops,
 * rows = M -- and one {begin, end} per reference row: row i is aligned to the query's samples [begin_i, end_i).  begin_0 == start ==
 * P[M-1][b-1].start, end_{M-1} == b, begin_i < end_i, and begin_{i+1} is end_i - 1 (a vertical step) or end_i (a diagonal step); the sum of
 * c(i, j) over the path's cells is cost.  When (a, b) is a span call's (start, end) for that pair, or any a' <= start with the same b, the
 * hit's cost and start are the span call's.  The hit reuses vbz_gpu_match_span: its fourth word, `zero`, carries rows HERE; the span calls
 * still write 0 there.  The empty verdict is the hit {0xFFFFFFFF, 0, 0, 0} with every row {0, 0}.
 * vbz_gpu_match_best_batch: the winners' table, made on the device.  spans is a span call's [n_reads, n_refs] arena; pairs[i] is read i with
 * the reference of least cost among row i, ties to the smallest reference index; empty verdicts and costs above max_cost are skipped;
 * begin and end are that hit's start and end.  If no reference qualifies, ref = 0xFFFFFFFF and begin = end = 0.  One wavefront per read.
 * Returns 0 when queued, -1 for a NULL context or a launch failure, -2 (nothing launched) for NULL or not 16-byte aligned tables while
 * the call has reads, n_refs outside 1 ... 4096, n_reads * n_refs * 16 beyond 2^46 bytes.
 * vbz_gpu_match_path_batch: query is the [n_reads, N] arena the fused span calls leave with the caller; valid may be NULL, meaning every
 * row has N samples (the fused calls do not hand their valid[] out; positions behind a read's end hold +0 there, and b bounds every
 * access).  path->max_width is the largest b - a the call accepts, a multiple of 8 from 8 to 65536; it sizes the scratch.  rows is a
 * row-major [n_pairs, ref_stride] arena of vbz_gpu_match_row (8 bytes), 16-byte aligned; entries at i >= M are written {0, 0}.  hit is
 * [n_pairs], written by 16-byte stores.  pairs is an untrusted device table, 16-byte aligned: a pair gets the empty verdict, with no
 * address formed from it, when read >= n_reads or ref >= R (the "none" of the best call included), begin >= end, end > min(valid, N),
 * end - begin > max_width, M_r == 0 or M_r > ref_stride.  EVERY entry of hit and rows is written by every call that launches.
 * Returns 0 when queued, -1 for a NULL context or a launch failure, -2, with nothing launched and nothing written, for NULL tables while
 * the call has pairs (valid apart), misalignment, path flags or reserved != 0, max_width outside its rule, everything vbz_gpu_match is
 * refused for, and n_pairs * ref_stride * 8 beyond 2^46 bytes.
 * How ("The path").  A forward launch, one wavefront per pair, runs the span kernel's schedule over the window's W columns
 * (W + la steps; the packed or the wide key by the span calls' rule with max_width in N's place, starts relative to a) and stores two
 * direction bits a cell into a bit-matrix in the context's scratch: about 16 c max_width bytes a pair, c the rows per lane of ref_stride.
 * A second launch, one wavefront per pair again, walks the bits back in scalar registers (at most W + M steps; 64 words of bits are
 * fetched by one load) and writes rows and hit.  The host runs the pairs in groups so that the bit-matrix stays under a cap (4 GiB;
 * VBZ_HIP_MATCH_PATH_CAP=<bytes> or vbz_gpu_set_match_path_cap; a pair larger than the cap runs alone): the answers do not depend on
 * it.  The context keeps the bit-matrix of its largest call -- the bits of one group, at most the cap and a quarter -- until it is
 * destroyed, like every scratch buffer of a context. */
typedef struct vbz_gpu_match_pair
{
    uint32_t read;  /* < n_reads */
    uint32_t ref;   /* < n_refs; 0xFFFFFFFF: none */
    uint32_t begin; /* a */
    uint32_t end;   /* b */
} vbz_gpu_match_pair; /* 16 bytes */
typedef struct vbz_gpu_match_path
{
    uint32_t max_width; /* the largest end - begin: a multiple of 8, 8 ... 65536 */
    uint32_t flags;     /* must be 0 */
    uint64_t reserved;  /* must be 0 */
} vbz_gpu_match_path; /* 16 bytes */
typedef struct vbz_gpu_match_row
{
    uint32_t begin; /* the first sample aligned to this reference row */
    uint32_t end;   /* one behind the last; {0, 0}: no such row */
} vbz_gpu_match_row; /* 8 bytes */
VBZ_EXPORT int vbz_gpu_match_best_batch(vbz_gpu_ctx* ctx, uint32_t n_reads, const vbz_gpu_match_span* spans, uint32_t n_refs, uint32_t max_cost,
                                        vbz_gpu_match_pair* pairs);
VBZ_EXPORT int vbz_gpu_match_path_batch(vbz_gpu_ctx* ctx, uint32_t n_pairs, uint32_t n_reads, const float* query, const uint32_t* valid,
                                        const vbz_gpu_match* match, const vbz_gpu_match_pair* pairs, const vbz_gpu_match_path* path,
                                        vbz_gpu_match_span* hit, vbz_gpu_match_row* rows);
/* The bytes of direction bits one group of a path call may take (0: the default). */
VBZ_EXPORT void vbz_gpu_set_match_path_cap(vbz_gpu_ctx* ctx, uint64_t bytes);

/* Signal locate.  The other orientation of the match calls, the one target filtering needs: the read's prefix is the sequence that is
 * matched WHOLE, against a stretch of a long expected squiggle of a target -- an amplicon, a plasmid, a viral genome on both strands, tens
 * of thousands to millions of levels.  The rule (tests/locate_ref.py):
 * Query.  Exactly the match calls' query: n = min(T', N) samples of the read's range, converted as the windows call converts them and
 * quantised with quant by the match rule (NaN -> 0, clamp to +-127, rint to nearest even).  N = query_len <= 2048.
 * Targets.  G = n_targets rows of int8 in a device matrix target[G][target_stride]; row g has L_g = target_len[g] valid entries, taken as
 * they are (-128 is legal).  target_len is an untrusted device table: L_g == 0 or L_g > target_stride gives column g the empty verdict for
 * every read, and no address is formed from it.
 * Cost.  c(i, j) = |k_i - g_j| in integers, rows the query, columns the target:
 *   D[0][j] = c(0, j)                                             (the alignment may start anywhere in the target)
 *   D[i][0] = c(i, 0) + D[i-1][0]
 *   D[i][j] = c(i, j) + min(D[i-1][j-1], D[i-1][j], D[i][j-1])
 *   cost = min_j D[n-1][j]          end = 1 + the SMALLEST j that attains it
 * The whole query is aligned to a stretch of the target that ends at `end` (exclusive, in target coordinates).  D <= 255 n < 2^20 whatever
 * L is, and end <= 2^30.  This is the match rule with its arguments exchanged: tests/match_ref.py's dtw_batch(levels of the read,
 * target[None, :L], [L]).  The empty verdict {0xFFFFFFFF, 0}: n == 0, an empty range, a read whose verdict is an error, or a refused
 * target_len.
 * Output.  out is a row-major [n_reads, G] arena of vbz_gpu_match_hit (8 bytes), 16-byte aligned.  Every entry is written by every call
 * that launches; nothing else is written, apart from query and shift_scale.
 * The three calls have the argument lists of their match twins with vbz_gpu_locate in vbz_gpu_match's place.  vbz_gpu_locate_batch is the
 * stage entry: query is a row-major [n_reads, N] float32 arena, 16-byte aligned, valid[i] (device, untrusted) is clamped to N.
 * vbz_gpu_signal_locate_batch and its POD5 twin behave as the fused match calls do: the windows call into the caller's REQUIRED query
 * arena under the library's own tables, valid[] from the verdicts and the range tables, then the locate launch on the context's stream; a
 * bad first_row fails the whole call as there.  Return codes and refusals (-2, nothing launched, nothing written) are those of the match
 * twins, with the rules of the struct below; the size rules are n_reads * G * 8, G * target_stride and n_reads * N * 4 beyond 2^46 bytes.
 * How: match.hip's systolic schedule with the operands exchanged (csrc/locate.hip).  One wavefront per (read, target)
 * pair; the lanes hold the read's quantised prefix, c = 1 ... 32 rows a lane by n; the target streams through as int8, a dword a lane for
 * 256 steps, one level a step.  The four wavefronts of a workgroup take four reads against one target row.  A step is 8.25 + 2 c VALU
 * instructions in the disassembly (match_kernel: 9 + 2 c).  No LDS, no barrier.
 * Not here: the path of a located read and the start of its stretch, which these three calls do not give (the span calls and
 * vbz_gpu_locate_path_batch below do); cutting one target across
 * wavefronts (a stretch has no bound in DTW, so a cut with overlap is not exact: a caller who wants more parallelism for a small batch
 * passes overlapping tiles as target rows and reads one hit per tile).
 * Measured on one MI355X (tools/time_locate.py, profiles/locate_time.json; the parent of the commit that adds these calls is b74e1b0; median
 * of 20, calls alternating in one process): synthetic reads of ~100 k samples, MED_MAD, N = 2 048 behind the trim call's begin[], quant 32,
 * G = 2 targets.  8 192 reads against L = 30 000: 58.59 ms fused, 2.65 ms for the windows call alone, 55.97 ms for the stage entry, and
 * 58.21 ms for the parent's only route over the same cells -- vbz_gpu_match_batch with the roles swapped, the target written out as float32
 * and the reads quantised by the caller -- whose hits equal these bit for bit; L = 48 000: 92.12 / 2.67 / 89.48 / 93.22 ms.  That is 18.0 T
 * cells/s and 279 cycles a step, against an issue bound of 290 (72.25 VALU instructions at 4.1 cycles, the twelve plain moves of a turn at
 * 2.2) and the swapped match's 17.3 T.  512 reads are one wavefront a SIMD, which issues an instruction every 5.1 cycles, not 4.1: 5.36 /
 * 0.77 / 4.59 / 4.62 ms at L = 30 000 and 8.13 / 0.78 / 7.34 / 7.33 ms at L = 48 000 (13.7 T cells/s, 366 cycles a step, the swapped
 * match's time to within its spread).  One target of L = 1 048 576 against 512 reads, which no match call can express: 160.99 / 0.81 /
 * 160.31 ms -- 512 wavefronts on 1 024 SIMDs, each walking its 1 048 639 steps alone. */
typedef struct vbz_gpu_locate
{
    uint32_t query_len;         /* N: a multiple of 8, 8 ... 2048 (64 lanes x 32 rows) */
    uint32_t n_targets;         /* G: 1 ... 4096 */
    uint32_t target_stride;     /* bytes per row of target: a multiple of 16, 16 ... 2^30 */
    uint32_t flags;             /* must be 0 */
    float quant;                /* finite, > 0 */
    uint32_t reserved;          /* must be 0 */
    const int8_t* target;       /* device, 16-byte aligned, n_targets x target_stride */
    const uint32_t* target_len; /* device, n_targets words */
} vbz_gpu_locate;               /* 40 bytes */
VBZ_EXPORT int vbz_gpu_locate_batch(vbz_gpu_ctx* ctx, uint32_t n_reads, const float* query, const uint32_t* valid, const vbz_gpu_locate* locate,
                                    vbz_gpu_match_hit* out);
VBZ_EXPORT int vbz_gpu_signal_locate_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                           const vbz_gpu_signal_format* format, const vbz_gpu_normalization* norm, float* shift_scale,
                                           const vbz_gpu_sample_ranges* ranges, const vbz_gpu_locate* locate, float* query, vbz_gpu_match_hit* out);
VBZ_EXPORT int vbz_gpu_pod5_signal_locate_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                const vbz_gpu_signal_format* format, const vbz_gpu_pod5_reads* reads,
                                                const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges,
                                                const vbz_gpu_locate* locate, float* query, vbz_gpu_match_hit* out);

/* Signal locate with the start of the aligned stretch: the interval [start, end) of the target that the read's prefix is aligned to -- what
 * tells two amplicons apart, rejects a "hit" that smears over half a genome, and hands the stretch to a second stage.
 * The rule (tests/locate_span_ref.py).  Query, quantisation, targets, c(i, j) = |k_i - g_j|, cost, end and the empty verdict are exactly
 * vbz_gpu_locate's; rows the query, columns the target.  The start is the match-span rule with its arguments exchanged --
 * tests/match_span_ref.py's span_brute(levels of the read, target[:L]): a warping path runs from (0, s) to (n - 1, e - 1) in steps (i+1, j),
 * (i, j+1), (i+1, j+1); horizontal steps inside row 0 count (a path may sit on the query's first level over several target levels); start
 * is the SMALLEST s over all paths of cost `cost` that end at column end - 1.  start < end always; both are in target coordinates,
 * start <= 2^30 - 1.
 * Output.  out is a row-major [n_reads, G] arena of vbz_gpu_match_span (16 bytes: {cost, end, start, 0}), 16-byte aligned, every entry
 * written by one 16-byte store by every call that launches.  The empty verdict is {0xFFFFFFFF, 0, 0, 0}, under the locate calls'
 * conditions: n == 0, an empty range, a read whose verdict is an error, target_len 0 or above target_stride.
 * The three calls have the argument lists of their locate twins with vbz_gpu_match_span* out, the same vbz_gpu_locate (flags and reserved
 * 0), the same refusals and the same return codes; the arena's size rule is n_reads * G * 16 beyond 2^46 bytes.
 * The winners' table.  vbz_gpu_match_best_batch(ctx, n_reads, spans, G, max_cost, pairs) over a locate span arena (G <= 4096 in both) gives
 * each read's best target -- least cost, ties to the smallest target index, empty verdicts and costs above max_cost skipped -- and its
 * [begin, end) in TARGET coordinates: span -> best are two queued calls on one stream, nothing crosses to the host.  That kernel copies
 * start and end as 32-bit words and assumes nothing about their range.
 * How ("The start").  Phase 1 is the locate kernel's loop as it stands: (cost, end).  Phase 2, in the same wavefront, walks
 * BACK from (cost, end) with an anchored DP in reversed coordinates -- the lanes hold the query reversed, the target streams backwards
 * from level end - 1 -- whose row n - 1 holds `cost` exactly at the columns a path of that cost can start at; the last such column is the
 * start.  The walk stops as soon as every live cell of the wavefront's fronts of two consecutive steps exceeds `cost` (tested once a block
 * of 256 steps), or at the target's first level: it covers about the width of the stretch, not L.  A step of phase 2 is 6.25 + 3 c VALU
 * instructions against phase 1's 8.25 + 2 c (c - 1 of them the selects that pick row n - 1 out of the lane's rows; 86.5 or 101.5 at c = 32).  No LDS, no barrier, no atomics, no scratch; 128
 * VGPRs, four wavefronts a SIMD; locate_kernel is untouched.
 * Measured on one MI355X (tools/time_locate.py, profiles/locate_span_time.json; workload and shapes of the locate calls above, median of 20,
 * the legs alternating in one process, every (cost, end) checked bit for bit against the cost-only leg of the same run, six reads a case
 * held to numpy): the span stage entry 59.13 ms against 55.87 ms at 8 192 reads, L = 30 000 (1.058 x) and 91.91 against 89.05 ms at
 * L = 48 000 (1.032 x); the fused span call 61.77 / 94.69 ms.  That is the expectation 1 + (width + 63 + up to 256 steps at phase 2's count)
 * / (L + 63 at phase 1's): 1.056 and 1.032, the stretch's width 788 and 482 levels in the median, 895 and 768 steps walked back by the
 * numpy model of the rule.  The cost-only stage entry, timed before and after in the same loop, did not move (55.87 / 55.91, 89.05 /
 * 89.09 ms).  With 512 reads -- one wavefront a SIMD -- the span stage took 4.69 against 4.63 ms, 7.19 against 7.38 ms and, at
 * L = 1 048 576, 146.79 against 159.76 ms: there the span kernel's phase 1, the same instructions under another register allocation, runs
 * faster than locate_kernel's own loop, which is not explained. */
VBZ_EXPORT int vbz_gpu_locate_span_batch(vbz_gpu_ctx* ctx, uint32_t n_reads, const float* query, const uint32_t* valid, const vbz_gpu_locate* locate,
                                         vbz_gpu_match_span* out);
VBZ_EXPORT int vbz_gpu_signal_locate_span_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options, int sized,
                                                const vbz_gpu_signal_format* format, const vbz_gpu_normalization* norm, float* shift_scale,
                                                const vbz_gpu_sample_ranges* ranges, const vbz_gpu_locate* locate, float* query,
                                                vbz_gpu_match_span* out);
VBZ_EXPORT int vbz_gpu_pod5_signal_locate_span_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                                     const vbz_gpu_signal_format* format, const vbz_gpu_pod5_reads* reads,
                                                     const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges,
                                                     const vbz_gpu_locate* locate, float* query, vbz_gpu_match_span* out);

/* Signal locate: the warping path of chosen pairs, in target coordinates.  The span calls say which target a read sits on and on which
 * levels [start, end) of it; this stage-level call says which of those levels each sample of the read's prefix belongs to -- what
 * adaptive sampling, methylation calling and resquiggling do with a located read -- for the pairs the caller lists, typically the one
 * winner per read, without the arena or the query crossing to the host: span -> best -> path are three queued calls on one stream.
 * The rule (tests/locate_path_ref.py).  It is the match-path rule with its arguments exchanged: tests/match_path_ref.py's
 * path_pair(levels of the read[:n], target[:L], a, b).  A pair is a vbz_gpu_match_pair {read, ref = target index, begin = a, end = b} with
 * [a, b) in TARGET coordinates -- exactly what vbz_gpu_match_best_batch writes over a locate span arena.  Rows are the query's
 * n = min(valid[read], N) levels, quantised by the match rule; columns are the target levels a ... b - 1; c(i, j) = |k_i - g_j|.  Over the
 * window's columns alone runs the DP of pairs P = (cost, start), ordered lexicographically: row 0 at column a is (c(0, a), a), nothing left
 * of a exists, and a path may sit on row 0 while that costs 0.  The backtrace starts at (n - 1, b - 1):
 *   at i > 0, j > a:  the FIRST of diagonal, up, left that equals the lexicographic minimum of the three;
 *   at j == a:        up;
 *   in row 0:         left while j > a and P[0][j-1].cost == 0, otherwise it stops.
 * Answers.  hit = {cost, end = b, start, rows = n} (vbz_gpu_match_span; its fourth word carries rows here, as in the match path).  rows is
 * a row-major [n_pairs, query_len] arena of vbz_gpu_match_row, 16-byte aligned: sample i of the prefix is aligned to target levels
 * [begin_i, end_i); entries at i >= n are {0, 0}.  begin_0 == start, end_{n-1} == b, begin_i < end_i, begin_{i+1} is end_i - 1 or end_i,
 * and the sum of c over the named cells is cost.  With (a, b) a locate span call's (start, end) for that pair, or any a' <= start with the
 * same b, cost and start are the span call's.
 * Untrusted tables.  pairs, valid and target_len are untrusted device tables.  A pair gets the hit {0xFFFFFFFF, 0, 0, 0} and every row
 * {0, 0} when read >= n_reads or ref >= G (the best call's "none" included), begin >= end, n == 0, L_g == 0 or L_g > target_stride,
 * end > L_g, or end - begin > max_width; no address is formed from such a pair beyond valid[read] and target_len[ref] of indices inside
 * the call.  EVERY entry of hit and rows is written by every call that launches, hit by 16-byte stores; nothing else is written.
 * path->max_width is the largest b - a the call accepts, a multiple of 8 from 8 to 65536; it sizes the scratch.
 * Returns 0 when queued, -1 for a NULL context or a launch failure, -2, with nothing launched and nothing written, for everything
 * vbz_gpu_locate_batch refuses about locate; query or hit not 16-byte aligned; path NULL, with flags or reserved != 0, or with max_width
 * outside its rule; a NULL query, valid, target, target_len, pairs, hit or rows while the call has pairs (valid is REQUIRED here, unlike
 * the match path: the whole query is aligned, so zero padding behind a short read would be aligned as signal); pairs or rows not 16-byte
 * aligned; n_pairs * N * 8, n_reads * N * 4 or G * target_stride beyond 2^46 bytes.  n_pairs == 0 with good arguments returns 0 and
 * launches nothing.
 * vbz_gpu_query_valid_batch writes the valid[] that the fused match and locate calls derive internally and do not hand out: min(T', N),
 * or 0 for an error verdict, from result[] -- what such a call leaves, T x 4 bytes or an error code; for the POD5 twins read_result[] -- and
 * the range tables (ranges may be NULL; begin and end clamped as everywhere).  -2 for NULL tables while the call has reads, or for
 * query_len outside 8 ... 65536 in multiples of 8.  With it the whole fused chain is queued on one stream with no host copy:
 * vbz_gpu_signal_locate_span_batch -> vbz_gpu_query_valid_batch -> vbz_gpu_match_best_batch -> vbz_gpu_locate_path_batch.
 * How ("The path").  Two launches per group of pairs, one wavefront per pair, as the match path.  The forward launch runs
 * the locate kernel's schedule -- the query in the lanes, c = 1 ... 32 rows a lane by the pair's own n, the window streamed as int8, a dword
 * a lane per 256 steps -- over the span kernels' keys cost << sb | start (starts relative to a; packed or wide by csrc/match_select.h with
 * max_width in N's place and query_len in ref_stride's) and stores the match path's two direction bits a cell in the match path's layout.
 * The window starts and ends at arbitrary bytes: aligned dwords are loaded and shifted by a % 4 bytes, and nothing at or behind dword
 * (L_g + 3) / 4 of a row is read.  The traceback is the match path's, stated once (csrc/match_path.h).  The scratch is the context's
 * match-path carve, match_path_pair_words(max_width, query_len) words a pair, grouped under VBZ_HIP_MATCH_PATH_CAP /
 * vbz_gpu_set_match_path_cap; the answers do not depend on the cap.  No LDS, no barrier, no atomics.
 * Measured on one MI355X (tools/time_locate.py, profiles/locate_path_time.json; workload and shapes of the locate calls above, median of 20,
 * the legs alternating in one process, every winner's (cost, start) equal to its span's): span -> best -> path 66.63 ms against the span
 * stage's 59.28 ms at 8 192 reads, L = 30 000, and 99.10 against 92.09 ms at L = 48 000; the path call alone 7.40 / 7.21 ms there and
 * 1.29 ms at 512 reads whatever L is -- with one wavefront per pair a small call lasts as long as its widest pair -- which is what
 * vbz_gpu_match_path_batch with the roles swapped takes where it can express the pairs (1.30 ms, the same bytes). */
VBZ_EXPORT int vbz_gpu_locate_path_batch(vbz_gpu_ctx* ctx, uint32_t n_pairs, uint32_t n_reads, const float* query, const uint32_t* valid,
                                         const vbz_gpu_locate* locate, const vbz_gpu_match_pair* pairs, const vbz_gpu_match_path* path,
                                         vbz_gpu_match_span* hit, vbz_gpu_match_row* rows);
VBZ_EXPORT int vbz_gpu_query_valid_batch(vbz_gpu_ctx* ctx, uint32_t n_reads, const uint32_t* result, const vbz_gpu_sample_ranges* ranges,
                                         uint32_t query_len, uint32_t* valid);

/* Event-space alignment.  The alignment calls above take samples: at about ten samples a base, the 2 048 entries of a locate query reach
 * some 200 target levels.  Squiggle mappers align EVENTS, one value a base, and an event-align or re-squiggle tool wants the answer as a
 * table per target level.  The two stage-level calls below are those two links, so that
 *   segment -> events -> events_query -> locate_span -> match_best -> locate_path -> locate_levels
 * is a run of queued calls on one stream with no host copy.  No other call changes; the locate limit of 2 048 entries stands.
 * vbz_gpu_events_query_batch: the event records as a query arena.  The rule (tests/eventalign_ref.py).  Read i owns rows
 * c0 = event_first[i] ... c1 - 1 of `records` (a vbz_gpu_events, as the event calls read it; events->start is not read and may be NULL).
 * Walk them in order and keep the rows with records[c].n >= min_n (0 keeps all).  The k-th kept row, k < N = query_len, gives
 * query[i][k] = records[c].mean, the 32 bits copied (NaN payloads, -0), and index[i][k] = c - c0; the walk stops behind N kept rows.
 * valid[i] is the number kept, at most N; positions at and behind it hold +0 in query and 0 in index.  index may be NULL.  result may be
 * NULL, meaning every read is good; otherwise a read whose result[i] is an error verdict gets valid[i] = 0, by exactly the test of
 * vbz_gpu_query_valid_batch.  event_first is untrusted: a read gets valid[i] = 0, and no address is formed from its rows, when
 * event_first[i] > event_first[i + 1], event_first[i + 1] > event_rows, or it has more than 2^31 - 1 rows.  query and index are row-major
 * [n_reads, N] arenas, 16-byte aligned.  EVERY entry of query, valid and index is written by every call that launches; nothing else is.
 * Returns 0 when queued, -1 for a NULL context or a launch failure, -2, with nothing launched and nothing written, for a NULL events or
 * q, flags or reserved != 0 in either, query_len outside its rule, a NULL event_first, records (when event_rows > 0), query or valid while
 * the call has reads, query, records or index not 16-byte aligned, n_reads * N * 4 or event_rows * 16 beyond 2^46 bytes.
 * vbz_gpu_locate_levels_batch: the path, transposed.  pairs, hit and rows ([n_pairs, query_len]) are what vbz_gpu_locate_path_batch took
 * and wrote; of a pair only `read` is used.  index is the first call's [n_reads, query_len] table (NULL: entry k is row k); events -- with
 * start REQUIRED here -- records and moments are the event call's tables.  The rule.  For pair p with hit {cost, end, start, n}: levels
 * is a row-major [n_pairs, max_width] arena of vbz_gpu_level, 16-byte aligned, and row t of pair p is target level start + t, t < end -
 * start.  The entries of level j are E_j = {k < n : begin_k <= j < end_k}: the path is monotone, so that is a range [k0, k1), never empty
 * inside [start, end).  Entry k is event row c_k = event_first[read] + index[read][k].  first_sample = start[c_k0]; end_sample =
 * start[c] + records[c].n of c = c_(k1-1); n_samples, sum and sumsq are the sums of records[c_k].n, moments[c_k].sum and
 * moments[c_k].sumsq over k0 <= k < k1, modulo 2^32 and 2^64 -- the tables are inputs, and the rule is the same whether the sums are
 * added up or taken as differences of prefix sums; n_entries = k1 - k0.  An entry aligned to several levels counts in each.
 * n_levels[p] = end - start; rows at and behind it are 32 zero bytes.  Floating-point mean and sd of a level are the event call's
 * formulas over its exact moments, the caller's to apply.
 * Every table is untrusted.  A pair gets n_levels = 0 and every row zero, with no address formed from an unchecked value, when
 * read >= n_reads; n == 0 (the empty verdict and the best call's "none" are that) or n > query_len; start >= end or end - start >
 * max_width; a row breaks the path's invariants -- begin_0 == start, end_(n-1) == end, begin_k < end_k, begin_(k+1) one of end_k - 1 and
 * end_k; an index[read][k], k < n, at or beyond the read's row count; or a bad event_first as above.  EVERY entry of n_levels and levels
 * is written by every call that launches, the latter by 16-byte stores; nothing else is.
 * Returns 0 / -1 as above; -2 for a NULL events or flags or reserved != 0 in it; query_len or max_width outside 8 ... 65536 in multiples
 * of 8; a NULL pairs, hit, rows, event_first, n_levels or levels while the call has pairs -- and start, records or moments when
 * event_rows > 0; pairs, hit, rows, records, moments or levels not 16-byte aligned; n_pairs * query_len * 8, n_pairs * max_width * 32,
 * n_reads * query_len * 4 or event_rows * 16 beyond 2^46 bytes.
 * How (csrc/eventalign.hip).  Both: one wavefront per read / pair, four to a workgroup; no LDS, no barrier, no atomics,
 * no scratch.  The query is a stream compaction: 64 rows a turn, the keep mask by a ballot, the rank by mbcnt, and the wavefront leaves
 * as soon as N are kept; it writes the zero tail itself, by 16-byte stores.  The levels are differences of prefix values with no prefix
 * array: a pass over the path checks it; a second pass takes 64 entries a turn, scans n, S1 and S2 across the lanes with a carried total,
 * and the LAST entry of a level writes its record -- the exclusive sums of the level's first entry come by one shuffle from the lane a
 * running maximum names, or from a carry when a stall began in an earlier turn.  A turn costs the same whatever the path looks like; an
 * entry spanning many levels is written by the whole wavefront: O(n + width) a pair.
 * Measured on one MI355X (tools/time_eventalign.py, profiles/eventalign_time.json; the parent of the commit that adds these calls is f62cf9c
 * and can run neither, so the comparison is the unfused route in the same run; median of 20, the legs alternating in one process, every
 * table checked bit for bit against the stopped chains, the stage calls and the unfused routes, six reads held to numpy): 8 192 step-signal
 * reads of ~100 k samples, 66.0 M events, N = 2 048, min_n = 4, G = 2 targets of 30 000 levels, winners 1 857 levels wide in the median,
 * max_width 2 256.  events_query alone 0.109 ms against 5.80 ms for torch (repeat_interleave, cumsum ranks, one scatter: 53 x);
 * locate_levels alone 0.462 ms against 6.14 ms for torch (cumsum over entries, two searchsorted, gathers: 13 x).  The chain 103.73 ms:
 * segment -> events 30.52, stopped before locate_levels 103.36; the locate legs they stand beside are 63.27 ms (span) and 9.24 ms (path).
 * Both calls move their tables about once -- some 0.4 GB and 1.5 GB, 3 - 4 TB/s -- and wait for memory. */
typedef struct vbz_gpu_events_query
{
    uint32_t query_len; /* N: a multiple of 8, 8 ... 65536 */
    uint32_t min_n;     /* events with n < min_n are dropped; 0 keeps all */
    uint32_t flags;     /* must be 0 */
    uint32_t reserved;  /* must be 0 */
} vbz_gpu_events_query; /* 16 bytes */
typedef struct vbz_gpu_level
{
    uint32_t first_sample; /* start[] of the first entry's event */
    uint32_t end_sample;   /* start + n of the last entry's event */
    uint32_t n_samples;    /* sum of n over the level's entries */
    uint32_t n_entries;    /* query entries aligned to this level, >= 1 */
    int64_t sum;           /* sum of S1, modulo 2^64 */
    uint64_t sumsq;        /* sum of S2, modulo 2^64 */
} vbz_gpu_level;           /* 32 bytes */
VBZ_EXPORT int vbz_gpu_events_query_batch(vbz_gpu_ctx* ctx, uint32_t n_reads, const uint32_t* result, const vbz_gpu_events* events,
                                          const vbz_gpu_event* records, const vbz_gpu_events_query* q, float* query, uint32_t* valid,
                                          uint32_t* index);
VBZ_EXPORT int vbz_gpu_locate_levels_batch(vbz_gpu_ctx* ctx, uint32_t n_pairs, uint32_t n_reads, uint32_t query_len, uint32_t max_width,
                                           const vbz_gpu_match_pair* pairs, const vbz_gpu_match_span* hit, const vbz_gpu_match_row* rows,
                                           const uint32_t* index, const vbz_gpu_events* events, const vbz_gpu_event* records,
                                           const vbz_gpu_event_moments* moments, uint32_t* n_levels, vbz_gpu_level* levels);

/* Pore model on the device: the two ends of the event-space chain above.  In front of it, vbz_gpu_locate.target is an int8 matrix of
 * expected levels that a caller had to make on the host, k-mer by k-mer, with a quantisation that matches the library's bit for bit;
 * behind it, the exact moments per level that vbz_gpu_locate_levels_batch leaves exist so that each read's shift and scale can be
 * re-estimated against the model.  vbz_gpu_squiggle_batch writes the target arena from bases and a k-mer table; vbz_gpu_levels_fit_batch
 * turns a vbz_gpu_level arena into per-read {offset, scale} tables in the layout vbz_gpu_signal_format.offset / .scale take, so that a
 * second round of the chain runs under the refined constants with nothing crossing to the host.  No other call changes.
 * vbz_gpu_squiggle_batch: target levels from bases.  The rule (tests/squiggle_ref.py).  Rows = S = n_seqs, or 2 S with BOTH: row 2s is
 * sequence s as given, row 2s + 1 its reverse complement.  Base codes are A/a = 0, C/c = 1, G/g = 2, T/t/U/u = 3; every other byte is
 * invalid.  Sequence s has n = seq_len[s] bases b_0 ... b_(n-1), the first n bytes of row s of seq; n > seq_stride gives the row or rows
 * of s length 0, and no address is formed from it.  The reverse complement strand is b'_i = 3 - b_(n-1-i); invalid stays invalid.
 * L = n - k + 1 when k <= n, else 0; L > target_stride also gives 0.  The k-mer at j has index sum_(i<k) b_(j+i) 4^(k-1-i), the first
 * base most significant, and its level is m = model[index].  Output position j < L holds the k-mer at j, or at L - 1 - j with REVERSED;
 * with BOTH as well the order is strand first, then reversed.  The quantisation is exactly the query's of the match calls: v = m * quant
 * (one float32 multiply), 0 when v is NaN, otherwise clamp(rint(v), -127, 127), rint to nearest even, +-inf giving +-127.  A k-mer that
 * holds an invalid base gives int8 0 and float +0, and is counted in masked[row].  target[row][0 ... target_stride) is written whole, by
 * 16-byte stores, with zeros at and behind L; level (nullable: [rows][target_stride] float32) holds the 32 bits of m, +0 where masked or
 * behind L; target_len[row] = L.  EVERY entry of all four tables is written by every call that launches; nothing else is.
 * Returns 0 when queued, -1 for a NULL context or a launch failure, -2, with nothing launched and nothing written, for a NULL struct;
 * k, n_seqs, either stride or quant outside its rule (NaN and infinities included); unknown flag bits; a NULL seq, seq_len, model,
 * target, target_len or masked; seq, target or level not 16-byte aligned; rows * target_stride * 4 or S * seq_stride beyond 2^46 bytes.
 * vbz_gpu_levels_fit_batch: new constants per pair, from exact integers.  The rule.  pairs, hit, n_levels and levels ([n_pairs,
 * max_width]) are what vbz_gpu_locate_levels_batch took and wrote, locate is the chain's own.  Pair p has hit {cost, end, start, n} and
 * W = n_levels[p]; row t < W of its levels is target level start + t of row g = pairs[p].ref, and g_t is the int8 there.  The level's
 * value is m_t = float64(sum_t) / float64(n_samples_t); the level is left out when n_samples_t < max(min_samples, 1), when n_entries_t >
 * max_entries and max_entries != 0, and when |m_t| <= 32768 does not hold.  q_t = int64(rint(m_t * 64)), rint to nearest even.  Over the
 * K kept levels, in exact integers: Sg = sum g_t, Sgg = sum g_t^2, Sq = sum q_t, Sgq = sum g_t q_t; num = K Sgq - Sg Sq, den = K Sgg -
 * Sg^2.  With K <= 2^16, |g| <= 2^7 and |q| <= 2^21, |num| < 2^62 and den < 2^47: everything is int64, nothing wraps, and integer sums do
 * not depend on their order, so the answer is reproducible bit for bit.  sums[p] = {Sg, Sgg, Sq, Sgq} when given.  In float64, each
 * operation rounded to nearest even and none fused: A = float64(num) / float64(den), B = (float64(Sq) - A * float64(Sg)) / float64(K),
 * a = A / 64, b = B / 64.  A read sample x on model level g is x ~ a g + b, and the constants under which ((float)x + o) * s * quant ~ g
 * are scale = float32(1.0 / (a * float64(quant))) and offset = float32(-b).  ok = 1 when the pair is valid, K >= 2, den > 0, num > 0 and
 * both float32 results are finite with scale > 0; otherwise ok = 0 and offset and scale are the prior's: offset = -shift, scale =
 * float32(1 / float64(scale)) of prior_shift_scale[read], or 0 and 1 when the prior is NULL or read >= n_reads.  used = K, or 0 for an
 * invalid pair.  offset[p] / scale[p] repeat the record's two floats: vbz_gpu_match_best_batch writes pair i for read i, so in the chain
 * they are per-read tables.
 * Every table is untrusted.  A pair is invalid, and no address is formed from an unchecked value, when read >= n_reads; ref >= G; W == 0
 * or W > max_width; end - start != W; L_g == 0 or L_g > target_stride; end > L_g.  EVERY entry of out, offset, scale and sums, when given,
 * is written by every call that launches; nothing else is.
 * Returns 0 / -1 as above; -2 for everything vbz_gpu_locate_batch refuses about locate; a NULL fit, or flags != 0; max_width outside its
 * rule; a NULL pairs, hit, n_levels, levels, out, offset or scale while the call has pairs; pairs, hit, levels or out not 16-byte aligned;
 * n_pairs * max_width * 32 beyond 2^46 bytes.  n_pairs == 0 with good arguments returns 0 and launches nothing.
 * How (csrc/squiggle.hip).  No LDS, no barrier, no atomics, no scratch memory in either.  The squiggle: one lane makes 16
 * consecutive levels, so one 16-byte store of int8 and four of float32; it loads the seven aligned dwords that cover its 16 + k - 1
 * bases, shifts them into place, rolls the index (shift by 2, mask, add) beside a bit mask of the last k bases' validity, and gathers the
 * model from global memory; the reverse strand reads the same bytes from the other end.  masked is exact with no zeroing launch: a
 * wavefront adds its lanes' counts by shuffles and stores one word of the context's scratch, and a second tiny launch, one wavefront a
 * row, adds the words up.  The fit: one wavefront a pair, four to a workgroup, 64 levels a turn; a lane loads its 32-byte record by two
 * 16-byte loads and its int8 level from the aligned dword that holds it; the five sums stay in registers, are added across the
 * wavefront once, and one lane does the float64 arithmetic and the stores.
 * Measured on one MI355X (tools/time_refit.py, profiles/refit_time.json; the parent of the commit that adds these calls is 43d0dce and can
 * run neither, so the comparison is the unfused torch route in the same run; median of 20, the legs alternating in one process, every
 * table checked bit for bit): squiggle of 4 rows (S = 2, BOTH) with levels, 30 000 bases 0.0225 ms, 1 048 576 bases 0.034 ms (k = 6) and
 * 0.045 ms (k = 9), against 1.0 - 1.3 ms for torch: two launches, about 0.022 ms whatever they do, so 0.6 - 0.75 TB/s at the large shape
 * and not a copy's rate.  levels_fit over 8 192 pairs, max_width 2 256, 15.2 M levels: 0.158 ms against 2.30 ms for torch, 3.2 TB/s
 * over the records it reads, beside locate_levels at 0.459 ms and the span leg at 62.95 ms. */
#define VBZ_GPU_SQUIGGLE_BOTH 1u     /* row 2s: sequence s as given; row 2s + 1: its reverse complement */
#define VBZ_GPU_SQUIGGLE_REVERSED 2u /* levels in 3'->5' order (direct RNA) */
typedef struct vbz_gpu_squiggle
{
    uint32_t k;              /* 1 ... 9 */
    uint32_t n_seqs;         /* S: 1 ... 4096; 1 ... 2048 with BOTH (rows <= 4096 = the locate calls' G) */
    uint32_t seq_stride;     /* bytes per row of seq: a multiple of 16, 16 ... 2^30 */
    uint32_t target_stride;  /* entries per output row: a multiple of 16, 16 ... 2^30 */
    uint32_t flags;          /* BOTH | REVERSED; other bits must be 0 */
    float quant;             /* finite, > 0: the locate calls' quant */
    const uint8_t* seq;      /* device, 16-byte aligned, S x seq_stride ASCII bytes */
    const uint32_t* seq_len; /* device, S words, untrusted */
    const float* model;      /* device, 4^k float32: the expected level of each k-mer in the query's units */
} vbz_gpu_squiggle;          /* 48 bytes */
typedef struct vbz_gpu_levels_fit
{
    uint32_t max_width;   /* of the levels arena: a multiple of 8, 8 ... 65536 */
    uint32_t min_samples; /* levels with n_samples < max(min_samples, 1) are left out */
    uint32_t max_entries; /* levels with n_entries > max_entries are left out (stalls); 0: no cap */
    uint32_t flags;       /* must be 0 */
} vbz_gpu_levels_fit;     /* 16 bytes */
typedef struct vbz_gpu_level_fit
{
    float offset;  /* what format->offset takes: -b, or the prior's -shift */
    float scale;   /* what format->scale takes: 1 / (a quant), or the prior's 1 / scale */
    uint32_t used; /* K, the levels kept; 0 for an invalid pair */
    uint32_t ok;   /* 1: a good fit; 0: offset and scale are the prior's */
} vbz_gpu_level_fit; /* 16 bytes */
VBZ_EXPORT int vbz_gpu_squiggle_batch(vbz_gpu_ctx* ctx, const vbz_gpu_squiggle* squiggle, int8_t* target, uint32_t* target_len, uint32_t* masked,
                                      float* level);
VBZ_EXPORT int vbz_gpu_levels_fit_batch(vbz_gpu_ctx* ctx, uint32_t n_pairs, uint32_t n_reads, const vbz_gpu_locate* locate,
                                        const vbz_gpu_match_pair* pairs, const vbz_gpu_match_span* hit, const uint32_t* n_levels,
                                        const vbz_gpu_level* levels, const vbz_gpu_levels_fit* fit, const float* prior_shift_scale,
                                        vbz_gpu_level_fit* out, float* offset, float* scale, int64_t* sums);

/* Stage-level entry points (the two halves of the path, used by tests and stage benchmarks).
 *   svb:  reference vbz_delta_zig_zag_streamvbyte_{compress,decompress}_v{0,1}
 *         (vbz/v0/vbz_streamvbyte.cpp:20-108, vbz/v1/vbz_streamvbyte.cpp:22-113)
 *   zstd: the reference's ZSTD_compress / ZSTD_decompress call sites (vbz/vbz.cpp:194-207,236-273)
 * For zstd decompress, dst_cap[i] is the capacity and result[i] the frame content size. */
VBZ_EXPORT int vbz_gpu_svb_compress_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, int integer_size,
                                          int zigzag, int version);
VBZ_EXPORT int vbz_gpu_svb_decompress_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, int integer_size,
                                            int zigzag, int version);
/* key_bytes (device, nullable): length of the control-byte section of each svb stream, which the
 * encoder codes with its own Huffman table; NULL codes the whole stream as one region. */
/* With vbz_gpu_set_checksum on, a read whose frame and checksum do not fit dst_cap[i] gets VBZ_DESTINATION_SIZE_ERROR (a slot of
 * ZSTD_COMPRESSBOUND(src_size[i]) + 4 bytes always fits). */
VBZ_EXPORT int vbz_gpu_zstd_compress_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const uint32_t* key_bytes);
VBZ_EXPORT int vbz_gpu_zstd_decompress_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch);
/* XXH64 (seed 0) of every read's src bytes into out[i] (device, n_reads x u64); dst fields unused.  One quad of lanes per read, one
 * accumulator each (the four are independent, the rounds within one a serial chain): many reads at memory speed (65 536 reads of
 * ~100 KB: 1.3 ms, ~5 TB/s), one read near the speed of its chain (one 40 MB buffer: ~41 ms, ~1 GB/s). */
VBZ_EXPORT int vbz_gpu_xxh64_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, uint64_t* out);

/* Dense arenas.  A compress call leaves every read in a slot of vbz_max_compressed_size(raw) bytes; these two calls lay a batch out
 * contiguously instead, each byte count rounded up to `align` (a power of two, 1 ... 4096), error entries taking no bytes:
 * off[i] = the exclusive scan of the rounded counts, off[n] = the total (device tables of n + 1 and n words).  Both are asynchronous
 * on the context's stream and return 0 when queued, -1 for a NULL context or batch or a launch failure, -2 for bad arguments,
 * refused on the host before anything is launched: `align`, unknown options, a NULL pointer among the fields the call uses, a declared
 * extent beyond 2^46 bytes.
 *
 * vbz_gpu_pack_batch: the dense arena of a finished compress (or decompress) call.  Uses n_reads, dst, dst_off, dst_cap, dst_bytes and
 * result; the src fields are not looked at.  result[] is untrusted like the descriptor tables: a read takes space only when result[i]
 * is a byte count (!vbz_is_error) that fits dst_cap[i] and its slot lies inside [0, dst_bytes); packed_size[i] = that count,
 * result[i] unchanged when it is an error code, VBZ_INPUT_SIZE_ERROR for a count that does not fit its slot (whose bytes are then
 * never read).  The bytes -- and zeros in the padding between reads -- are written to packed only when packed != NULL and
 * packed_off[n] <= packed_cap; otherwise nothing in packed is touched (packed = NULL: the tables alone, one synchronisation away from
 * sizing the arena; an arena too small fails whole, it never holds some of the reads).  packed must not overlap the dst arena (-2).
 * With align >= 16, (packed, packed_off, packed_size) are directly the src tables of a vbz_gpu_decompress_batch on the decoders'
 * aligned path; like every src arena, the packed one must then stay readable for 16 bytes behind packed_off[n].
 * Measured on one MI355X: profiles/HISTORY.md (dense arenas). */
VBZ_EXPORT int vbz_gpu_pack_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, uint32_t align, void* packed, uint64_t packed_cap,
                                  uint64_t* packed_off /* n + 1 */, uint32_t* packed_size /* n */);
/* vbz_gpu_decompressed_size_batch: n x vbz_decompressed_size over sized buffers (vbz_compress_sized, the HDF5 filter's chunks), and the
 * layout of their decoded output.  Uses n_reads, src, src_off, src_size and src_bytes; the dst fields are not looked at.  raw_size[i] =
 * the buffer's 4-byte little-endian header, VBZ_INPUT_SIZE_ERROR for a buffer shorter than 4 bytes or outside [0, src_bytes).  Header
 * values are taken as they are: a damaged one can ask for up to 4 GB, which the caller sees in raw_off[n] before allocating. */
VBZ_EXPORT int vbz_gpu_decompressed_size_batch(vbz_gpu_ctx* ctx, const vbz_gpu_batch* batch, const struct CompressionOptions* options,
                                               uint32_t align, uint32_t* raw_size /* n */, uint64_t* raw_off /* n + 1 */);

/* Synthetic workload of SURVEY.md section 8(d), generated on the device (no host data needed).
 *   lengths:  out_len[i] = samples of read first_read+i (90 000 + mix(..) % 20 001), i < n_reads
 *   signal:   int16 samples of read first_read+i written at dst + off[i] (bytes), len[i] samples
 *   u32:      config-4 values, len[i] elements */
VBZ_EXPORT int vbz_gpu_synth_lengths(vbz_gpu_ctx* ctx, uint64_t seed, uint64_t first_read, uint32_t n_reads,
                                     uint32_t* out_len);
VBZ_EXPORT int vbz_gpu_synth_signal(vbz_gpu_ctx* ctx, uint64_t seed, uint64_t first_read, uint32_t n_reads,
                                    void* dst, const uint64_t* off, const uint32_t* len);
VBZ_EXPORT int vbz_gpu_synth_u32(vbz_gpu_ctx* ctx, uint64_t seed, uint64_t first_read, uint32_t n_reads,
                                 void* dst, const uint64_t* off, const uint32_t* len);

/* Per-kernel timing with HIP events recorded on the context's stream around every launch.
 * enable=1 starts collecting; vbz_gpu_profile_read synchronizes, copies up to `cap` entries
 * (kernel name, launches, total milliseconds) and returns the number of distinct kernels. */
VBZ_EXPORT void vbz_gpu_profile_enable(vbz_gpu_ctx* ctx, int enable);
VBZ_EXPORT int vbz_gpu_profile_read(vbz_gpu_ctx* ctx, const char** names, uint32_t* launches, double* total_ms, int cap);
VBZ_EXPORT void vbz_gpu_profile_reset(vbz_gpu_ctx* ctx);

/* How the frames of the context's last decompress launch group were decoded (a diagnostic; synchronizes): *batched = frames decoded by
 * the batched decoder for frames this library wrote, *walked = frames whose sequence chains were walked one lane per frame ahead of the
 * general decoder (frames the reference wrote with libzstd).  Returns the number of frames of that group, 0 when it did not run on these
 * paths (the large-read path, VBZ_HIP_FAST_DECODE=0), < 0 on a device error.  The bytes and verdicts never depend on the path. */
VBZ_EXPORT int vbz_gpu_decode_paths(vbz_gpu_ctx* ctx, uint32_t* batched, uint32_t* walked);
/* ... and for how many of the walked frames the literals of the first block were decoded beside the walk (64 pieces of the four Huffman
 * streams, one lane each, ahead of the general decoder; VBZ_HIP_REF_LITERALS=0: never).  Counted over the frames of a call that walked: a
 * frame of literals alone has no chain to walk and is counted here all the same.  A diagnostic like the above; < 0 on a device error. */
VBZ_EXPORT int vbz_gpu_decode_literals_ahead(vbz_gpu_ctx* ctx);
/* The same for the large-read path (few, large reads; synchronizes): *by_spans = frames of the last decompress launch group that were
 * decoded span by span as their index says (or, without an index, by one wavefront at once) -- the others needed the second, gated
 * launch of the one-wavefront decoder.  Returns the frames of that group, 0 when it did not run on the large-read path. */
VBZ_EXPORT int vbz_gpu_decode_span_paths(vbz_gpu_ctx* ctx, uint32_t* by_spans);

/* Version string of the library: "vbz_hip <semver> gfx950". */
VBZ_EXPORT const char* vbz_gpu_version(void);

#if defined(__cplusplus)
}
#endif
#endif
