/*
 * vbz_oracle.h -- CPU ORACLE for the VBZ int16 hot path.  TEST INFRASTRUCTURE ONLY.
 *
 * This is a plain-C restatement of the reference algorithm (nanoporetech/vbz_compression)
 * used as the checker for the HIP product path.  Only tests/, __graft_entry__.smoke() and
 * bench.py's cpu_baseline leg may load it.  The product library (libvbz_hip.so) never
 * links, loads or calls anything in oracle/.
 *
 * Parity pinning (see DESIGN.md "Oracle"):
 *   - the reference itself is UNBUILDABLE in this image without stand-ins (its
 *     third_party/streamvbyte submodule is empty and vbz/vbz_export.h is cmake-generated),
 *     so there is no oracle/_ref;
 *   - the restatement is pinned against every known-answer vector the reference's own
 *     tests hold for this path (tests/golden/kat.json, each entry cites file:line) and
 *     against the decode pins in the three shipped fast5 files (tests/golden/fast5_*.bin);
 *   - the zstd stage of the oracle is the pinned third-party dependency itself
 *     (facebook/zstd, conan pin zstd/1.4.8, reference CMakeLists.txt:92-93), loaded at run
 *     time with dlopen("libzstd.so.1"); vbo_zstd_version() reports what was loaded.
 *   - streamvbyte (lemire/streamvbyte, un-vendored submodule, unpinned) is restated from
 *     its published format; uint32 values needing 3-4 bytes have no KAT in the reference:
 *     "parity unpinned" for those beyond round trips.
 */
#ifndef VBZ_ORACLE_H
#define VBZ_ORACLE_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint32_t vbo_size_t;

/* reference vbz/vbz.h:15-22 */
#define VBO_ZSTD_ERROR ((vbo_size_t)-1)
#define VBO_INPUT_SIZE_ERROR ((vbo_size_t)-2)
#define VBO_INTEGER_SIZE_ERROR ((vbo_size_t)-3)
#define VBO_DESTINATION_SIZE_ERROR ((vbo_size_t)-4)
#define VBO_STREAM_ERROR ((vbo_size_t)-5)
#define VBO_VERSION_ERROR ((vbo_size_t)-6)
#define VBO_OUT_OF_MEMORY_ERROR ((vbo_size_t)-7)
#define VBO_FIRST_ERROR VBO_OUT_OF_MEMORY_ERROR

/* reference vbz/vbz.h:29-53 (sizeof == 16: bool@0, u32@4,8,12) */
typedef struct VboOptions {
    bool perform_delta_zig_zag;
    unsigned int integer_size;
    unsigned int zstd_compression_level;
    unsigned int vbz_version;
} VboOptions;

/* ---- L1: integer codec (reference vbz/v0/vbz_streamvbyte.cpp, vbz/v1/vbz_streamvbyte.cpp) */
/* vbz_oracle_simd.c: an SSSE3 form of the int16 zig-zag stage, byte-identical to the scalar one, for the CPU baseline leg
 * only.  vbo_use_simd_svb(1) makes vbo_streamvbyte_compress / _decompress (hence vbo_compress / vbo_decompress) take it
 * for integer_size 2 with zig-zag; the default is the scalar restatement. */
#define VBO_SIMD_DECLINED ((vbo_size_t)-100)
int vbo_simd_available(void);
void vbo_use_simd_svb(int on);
vbo_size_t vbo_i16zz_compress_simd(const uint8_t* src, vbo_size_t src_size, uint8_t* dst);
vbo_size_t vbo_i16zz_decompress_simd(const uint8_t* src, vbo_size_t src_size, uint8_t* dst, vbo_size_t dst_size);
vbo_size_t vbo_max_streamvbyte_size(size_t integer_size, vbo_size_t source_size);
vbo_size_t vbo_streamvbyte_compress(const void* src, vbo_size_t src_size, void* dst, vbo_size_t dst_cap,
                                    int integer_size, bool zigzag, unsigned version);
vbo_size_t vbo_streamvbyte_decompress(const void* src, vbo_size_t src_size, void* dst, vbo_size_t dst_size,
                                      int integer_size, bool zigzag, unsigned version);

/* ---- L2: C API (reference vbz/vbz.cpp) */
bool vbo_is_error(vbo_size_t v);
const char* vbo_error_string(vbo_size_t v);
vbo_size_t vbo_max_compressed_size(vbo_size_t source_size, const VboOptions* o);
vbo_size_t vbo_compress(const void* src, vbo_size_t src_size, void* dst, vbo_size_t dst_cap, const VboOptions* o);
vbo_size_t vbo_decompress(const void* src, vbo_size_t src_size, void* dst, vbo_size_t dst_size, const VboOptions* o);
vbo_size_t vbo_compress_sized(const void* src, vbo_size_t src_size, void* dst, vbo_size_t dst_cap, const VboOptions* o);
vbo_size_t vbo_decompress_sized(const void* src, vbo_size_t src_size, void* dst, vbo_size_t dst_cap, const VboOptions* o);
vbo_size_t vbo_decompressed_size(const void* src, vbo_size_t src_size, const VboOptions* o);

/* ---- L3: HDF5 filter 32020 calling convention (reference vbz_plugin/vbz_plugin.cpp:97-229) */
size_t vbo_filter(unsigned flags, size_t cd_nelmts, const unsigned cd_values[], size_t nbytes,
                  size_t* buf_size, void** buf);

/* ---- zstd dependency (dlopen'd) */
const char* vbo_zstd_version(void);          /* NULL if libzstd.so.1 could not be loaded */
size_t vbo_zstd_compress(void* dst, size_t cap, const void* src, size_t n, int level);     /* (size_t)-1 on error */
size_t vbo_zstd_decompress(void* dst, size_t cap, const void* src, size_t n);              /* (size_t)-1 on error */
size_t vbo_zstd_bound(size_t n);
unsigned long long vbo_zstd_content_size(const void* src, size_t n);                       /* >= (u64)-2 on error/unknown */

/* ---- synthetic signal generator of SURVEY.md section 8(d) (integer-only, counter based) */
uint64_t vbo_mix64(uint64_t x);
uint32_t vbo_synth_read_length(uint64_t seed, uint64_t read_index);     /* config 2/5 length rule */
void vbo_synth_signal(uint64_t seed, uint64_t read_index, int16_t* out, size_t n);
void vbo_synth_u32(uint64_t seed, uint64_t read_index, uint32_t* out, size_t n);  /* config 4 values */

/* ---- restated zstd frame decoder (oracle/zstd_restate.c), the CPU mirror of the HIP decoder.
 * Returns decoded size, or (size_t)-1 on any format error. Writes at most cap bytes. */
size_t vbo_zstd_restate_decompress(void* dst, size_t cap, const void* src, size_t n);

/* ---- census of a zstd buffer (oracle/zstd_restate.c): which RFC 8878 features its frames hold.  The one list of the counters: id, name,
 * kind ('c' a count, 'm' a maximum, 's' a sum of bytes).  Counts are per frame, block, literals section, tree, table or sequence as the
 * name says.  The order inside a group is relied on (type + format, table + mode). */
#define VBO_CENSUS(X)                                                                                                                 \
    /* frame header (RFC 8878 3.1.1.1) */                                                                                             \
    X(FRAMES, "frames", 'c')                                                                                                          \
    X(FRAME_SINGLE_SEGMENT, "frame_single_segment", 'c')                                                                              \
    X(FRAME_WINDOW_DESCRIPTOR, "frame_window_descriptor", 'c')                                                                        \
    X(FRAME_CONTENT_SIZE_0_BYTES, "frame_content_size_0_bytes", 'c')                                                                  \
    X(FRAME_CONTENT_SIZE_1_BYTE, "frame_content_size_1_byte", 'c')                                                                    \
    X(FRAME_CONTENT_SIZE_2_BYTES, "frame_content_size_2_bytes", 'c')                                                                  \
    X(FRAME_CONTENT_SIZE_4_BYTES, "frame_content_size_4_bytes", 'c')                                                                  \
    X(FRAME_CONTENT_SIZE_8_BYTES, "frame_content_size_8_bytes", 'c')                                                                  \
    X(FRAME_CHECKSUM, "frame_checksum", 'c')                                                                                          \
    X(FRAME_WINDOW_LOG_UP_TO_16, "frame_window_log_up_to_16", 'c')                                                                    \
    X(FRAME_WINDOW_LOG_17_TO_19, "frame_window_log_17_to_19", 'c')                                                                    \
    X(FRAME_WINDOW_LOG_FROM_20, "frame_window_log_from_20", 'c')                                                                       \
    /* blocks (3.1.1.2) */                                                                                                            \
    X(BLOCK_RAW, "block_raw", 'c')                                                                                                    \
    X(BLOCK_RLE, "block_rle", 'c')                                                                                                    \
    X(BLOCK_COMPRESSED, "block_compressed", 'c')                                                                                      \
    X(BLOCK_LAST, "block_last", 'c')                                                                                                  \
    X(BLOCK_NOT_LAST, "block_not_last", 'c')                                                                                          \
    X(BLOCK_RAW_EMPTY, "block_raw_empty", 'c')                                                                                        \
    /* literals sections (3.1.1.3.1): raw and RLE by the header's bytes, compressed and treeless by the size format */                \
    X(LIT_RAW_1, "lit_raw_header_1_byte", 'c')                                                                                        \
    X(LIT_RAW_2, "lit_raw_header_2_bytes", 'c')                                                                                       \
    X(LIT_RAW_3, "lit_raw_header_3_bytes", 'c')                                                                                       \
    X(LIT_RLE_1, "lit_rle_header_1_byte", 'c')                                                                                        \
    X(LIT_RLE_2, "lit_rle_header_2_bytes", 'c')                                                                                       \
    X(LIT_RLE_3, "lit_rle_header_3_bytes", 'c')                                                                                       \
    X(LIT_HUF_FMT_0, "lit_compressed_format_0", 'c')                                                                                  \
    X(LIT_HUF_FMT_1, "lit_compressed_format_1", 'c')                                                                                  \
    X(LIT_HUF_FMT_2, "lit_compressed_format_2", 'c')                                                                                  \
    X(LIT_HUF_FMT_3, "lit_compressed_format_3", 'c')                                                                                  \
    X(LIT_TREELESS_FMT_0, "lit_treeless_format_0", 'c')                                                                               \
    X(LIT_TREELESS_FMT_1, "lit_treeless_format_1", 'c')                                                                               \
    X(LIT_TREELESS_FMT_2, "lit_treeless_format_2", 'c')                                                                               \
    X(LIT_TREELESS_FMT_3, "lit_treeless_format_3", 'c')                                                                               \
    X(LIT_STREAMS_1, "lit_streams_1", 'c')                                                                                            \
    X(LIT_STREAMS_4, "lit_streams_4", 'c')                                                                                            \
    X(LIT_TREELESS_TREE_OF_PREVIOUS_BLOCK, "lit_treeless_tree_of_previous_block", 'c')                                                \
    X(LIT_TREELESS_TREE_OF_EARLIER_BLOCK, "lit_treeless_tree_of_earlier_block", 'c')                                                  \
    /* Huffman tree descriptions (4.2.1), per tree */                                                                                 \
    X(HUF_DESC_DIRECT, "huf_description_direct", 'c')                                                                                 \
    X(HUF_DESC_FSE, "huf_description_fse", 'c')                                                                                       \
    X(HUF_WEIGHTS_LOG_5, "huf_weights_log_5", 'c')                                                                                    \
    X(HUF_WEIGHTS_LOG_6, "huf_weights_log_6", 'c')                                                                                    \
    X(HUF_MAX_BITS, "huf_max_bits", 'm')                                                                                              \
    X(HUF_TREES_11_BITS, "huf_trees_11_bits", 'c')                                                                                    \
    X(HUF_TREES_UP_TO_6_BITS, "huf_trees_up_to_6_bits", 'c')                                                                          \
    X(HUF_SYMBOLS_MAX, "huf_symbols_max", 'm')                                                                                        \
    X(HUF_SYMBOLS_UP_TO_16, "huf_symbols_up_to_16", 'c')                                                                              \
    X(HUF_SYMBOLS_ABOVE_128, "huf_symbols_above_128", 'c')                                                                            \
    /* sequences sections (3.1.1.3.2.1), per block; modes, logs and "less than 1" probabilities per table */                          \
    X(SEQ_NONE, "seq_none", 'c')                                                                                                      \
    X(SEQ_COUNT_1_BYTE, "seq_count_1_byte", 'c')                                                                                      \
    X(SEQ_COUNT_2_BYTES, "seq_count_2_bytes", 'c')                                                                                    \
    X(SEQ_COUNT_3_BYTES, "seq_count_3_bytes", 'c')                                                                                    \
    X(SEQ_LL_PREDEFINED, "seq_ll_predefined", 'c')                                                                                    \
    X(SEQ_LL_RLE, "seq_ll_rle", 'c')                                                                                                  \
    X(SEQ_LL_FSE, "seq_ll_fse", 'c')                                                                                                  \
    X(SEQ_LL_REPEAT, "seq_ll_repeat", 'c')                                                                                            \
    X(SEQ_OF_PREDEFINED, "seq_of_predefined", 'c')                                                                                    \
    X(SEQ_OF_RLE, "seq_of_rle", 'c')                                                                                                  \
    X(SEQ_OF_FSE, "seq_of_fse", 'c')                                                                                                  \
    X(SEQ_OF_REPEAT, "seq_of_repeat", 'c')                                                                                            \
    X(SEQ_ML_PREDEFINED, "seq_ml_predefined", 'c')                                                                                    \
    X(SEQ_ML_RLE, "seq_ml_rle", 'c')                                                                                                  \
    X(SEQ_ML_FSE, "seq_ml_fse", 'c')                                                                                                  \
    X(SEQ_ML_REPEAT, "seq_ml_repeat", 'c')                                                                                            \
    X(SEQ_LL_LOG_MAX, "seq_ll_log_max", 'm')                                                                                          \
    X(SEQ_OF_LOG_MAX, "seq_of_log_max", 'm')                                                                                          \
    X(SEQ_ML_LOG_MAX, "seq_ml_log_max", 'm')                                                                                          \
    X(SEQ_LL_LOG_5, "seq_ll_log_5", 'c')                                                                                              \
    X(SEQ_OF_LOG_5, "seq_of_log_5", 'c')                                                                                              \
    X(SEQ_ML_LOG_5, "seq_ml_log_5", 'c')                                                                                              \
    X(SEQ_LL_LOG_LIMIT, "seq_ll_log_9", 'c')                                                                                          \
    X(SEQ_OF_LOG_LIMIT, "seq_of_log_8", 'c')                                                                                          \
    X(SEQ_ML_LOG_LIMIT, "seq_ml_log_9", 'c')                                                                                          \
    X(SEQ_LL_LESS_THAN_1, "seq_ll_less_than_1", 'c')                                                                                  \
    X(SEQ_OF_LESS_THAN_1, "seq_of_less_than_1", 'c')                                                                                  \
    X(SEQ_ML_LESS_THAN_1, "seq_ml_less_than_1", 'c')                                                                                  \
    /* sequences (3.1.1.3.2.1.1, 3.1.1.5) */                                                                                          \
    X(OFF_NEW, "off_new", 'c')                                                                                                        \
    X(OFF_REP0, "off_rep0", 'c')                                                                                                      \
    X(OFF_REP1, "off_rep1", 'c')                                                                                                      \
    X(OFF_REP2, "off_rep2", 'c')                                                                                                      \
    X(OFF_LL0_REP1, "off_ll0_rep1", 'c')                                                                                              \
    X(OFF_LL0_REP2, "off_ll0_rep2", 'c')                                                                                              \
    X(OFF_LL0_REP0_MINUS_1, "off_ll0_rep0_minus_1", 'c')                                                                              \
    X(SEQ_LITERAL_LENGTH_0, "seq_literal_length_0", 'c')                                                                              \
    X(MAX_LL_CODE, "max_ll_code", 'm')                                                                                                \
    X(MAX_OF_CODE, "max_of_code", 'm')                                                                                                \
    X(MAX_ML_CODE, "max_ml_code", 'm')                                                                                                \
    X(LL_CODE_35, "ll_code_35", 'c')                                                                                                  \
    X(ML_CODE_52, "ml_code_52", 'c')                                                                                                  \
    X(MATCH_OVERLAPS_ITSELF, "match_overlaps_itself", 'c')                                                                            \
    X(MATCH_OFFSET_1, "match_offset_1", 'c')                                                                                          \
    X(MATCH_FROM_BEFORE_THE_BLOCK, "match_from_before_the_block", 'c')                                                                \
    X(OFF_ABOVE_64K, "off_above_64k", 'c')                                                                                            \
    X(OFF_ABOVE_128K, "off_above_128k", 'c')                                                                                          \
    X(OFF_ABOVE_1M, "off_above_1m", 'c')                                                                                              \
    X(TAIL_LITERALS_NONE, "tail_literals_none", 'c')                                                                                  \
    X(TAIL_LITERALS_SOME, "tail_literals_some", 'c')                                                                                  \
    /* content: literals (those of raw and RLE blocks included) and match bytes; their sum is the content size */                    \
    X(LITERAL_BYTES, "literal_bytes", 's')                                                                                            \
    X(MATCH_BYTES, "match_bytes", 's')
enum {
#define X(id, name, kind) VBO_CEN_##id,
    VBO_CENSUS(X)
#undef X
    VBO_CEN_COUNT
};
/* Decodes as vbo_zstd_restate_decompress does (every frame of the buffer, nothing stored) and adds to counters[0 .. VBO_CEN_COUNT) what it
 * meets; ncounters >= VBO_CEN_COUNT.  Returns the content size, or (size_t)-1 for a buffer the decoder refuses (the counters then hold
 * what was met up to there) */
size_t vbo_zstd_restate_census(const void* src, size_t n, uint64_t* counters, size_t ncounters);
int vbo_zstd_census_count(void);
const char* vbo_zstd_census_name(int k);  /* NULL beyond the list */
int vbo_zstd_census_is_max(int k);        /* a maximum: merged over frames with max, the others with + */

/* ---- the listing: every block and every sequence of a buffer's frames, as the restated decoder meets them.  Content positions count
 * from the start of the buffer's content (over all its frames); a block's ordinal counts inside its frame. */
typedef struct {
    uint64_t begin, end; /* the block's content range [begin, end) */
    uint32_t ordinal;
    uint32_t type;       /* Block_Type: 0 raw, 1 RLE, 2 compressed */
    uint32_t literals;   /* regenerated size of the literals section; of a raw or RLE block: its content */
    uint32_t nseq;
} VboSeqBlock;
typedef struct {
    uint64_t pos;        /* content position where the sequence's literals begin */
    int64_t unread;      /* bits of the sequences bit stream still unread at the head of the loop, before the sequence's extra bits */
    uint32_t block;      /* ordinal of its block */
    uint32_t ll, ml;     /* literal length, match length */
    uint32_t offset;     /* the resolved offset */
    uint32_t ofv;        /* the raw Offset_Value: 1 .. 3 a repeat offset, else offset + 3 */
    uint16_t ll_state, ml_state; /* the FSE states at the head of the loop */
    uint8_t ll_code, of_code, ml_code, reserved0;
    uint32_t reserved1;
} VboSeq;
/* Decodes as vbo_zstd_restate_census does and fills blocks[0 .. block_cap) and seqs[0 .. seq_cap) (either may be NULL); *nblocks (if not
 * NULL) gets the number of blocks and the return value is the number of sequences -- of the whole buffer, also where they exceed the
 * room given, so a call without room sizes the next.  (size_t)-1 for a buffer the decoder refuses (the arrays then hold what was met). */
size_t vbo_zstd_restate_sequences(const void* src, size_t n, VboSeqBlock* blocks, size_t block_cap, size_t* nblocks, VboSeq* seqs, size_t seq_cap);

/* ---- replay of the reference's fuzz target (oracle/vbz_oracle_fuzz.c; reference vbz/fuzzing/vbz_fuzz.cpp:138-161) */
uint32_t vbo_fuzz_max_destination(uint32_t size, const VboOptions* o);
int vbo_fuzz_decompress_sweep(const void* data, uint32_t size, const VboOptions* o, uint32_t max_destination, uint32_t* results);

#ifdef __cplusplus
}
#endif
#endif
