// vbz_kernels.h -- internal interface between the C ABI (vbz_api.hip) and the HIP kernels.
// Not installed; the public surface is include/vbz.h and include/vbz_gpu.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vbzhip {

// vbz error codes (include/vbz.h), usable in device code
constexpr uint32_t E_ZSTD = 0xFFFFFFFFu;
constexpr uint32_t E_INPUT_SIZE = 0xFFFFFFFEu;
constexpr uint32_t E_INTEGER_SIZE = 0xFFFFFFFDu;
constexpr uint32_t E_DESTINATION_SIZE = 0xFFFFFFFCu;
constexpr uint32_t E_STREAM = 0xFFFFFFFBu;
constexpr uint32_t E_VERSION = 0xFFFFFFFAu;
constexpr uint32_t E_OOM = 0xFFFFFFF9u;
constexpr uint32_t E_DEVICE = 0xFFFFFFF8u;
constexpr uint32_t E_FIRST = E_DEVICE;
constexpr uint32_t GATE_SKIP = E_FIRST - 1u;   // gate value "not in this launch group"; gate >= GATE_SKIP: no work here
constexpr int PHASE_SLOTS = 12;  // per-read cycle counters of the timed kernel builds (debug aid)

// Typed decode (vbz_gpu_decompress_signal_batch): the svb decoder of int16 streams stores sample x of read i as
// ((float)x + cal[i].x) * cal[i].y in the output type (SIG_*: the VBZ_GPU_SIGNAL_* values), x being int16 (bias 0) or uint16
// (bias 0x8000).  dst_off / dst_cap of the batch then count int16 bytes: the read's typed slot starts at dst + dst_off[i] / 2 * E
// (E = 4 or 2 bytes per sample) and result[i] is samples * E.  type == SIG_NONE: the int16 samples themselves.
// Chunk store (vbz_gpu_decompress_chunks_batch; row != NULL): the typed samples go to fixed-length chunks instead of a slot -- chunk k of
// read i is row row[i] + k of a row-major [rows, chunk_len] arena at dst (see chunk_count / chunk_last_start); dst_off is not used.
constexpr uint32_t SIG_NONE = 0, SIG_F32 = 1, SIG_F16 = 2, SIG_BF16 = 3;
constexpr uint32_t SIG_CHUNK = 4;   // (or-ed into the chunk store's type: the svb decoder's OUT, the store DecStore<ELEM, OUT> of its kernels)
constexpr uint32_t SIG_COUNT = 8;   // the svb decoder's counting pass of a normalising decode (OUT only: it stores nothing)
constexpr uint32_t SIG_RANGE = 16;  // (or-ed into a chunk store's or the counting pass's OUT: only the samples of SignalOut's per-read range)
constexpr uint32_t SIG_TRIM = 32;   // the svb decoder's trim pass behind the counting passes (OUT only: it stores nothing; TrimOut below)
constexpr uint32_t SIG_WINDOW = 64; // (or-ed into a chunk store's OUT: the rows are caller-listed windows of the signal -- SignalOut::wfirst / wstart)
constexpr uint32_t SIG_EVENT = 128; // the svb decoder's event pass (OUT only, | SIG_RANGE: it stores no sample; SignalOut::events)
constexpr uint32_t RANGE_STATS_RANGE = 0, RANGE_STATS_READ = 1;   // (= VBZ_GPU_RANGE_STATS_*)
constexpr uint32_t CHUNK_PAD = 0, CHUNK_END = 1;

// Normalising decode (vbz_gpu_*_norm_batch): every read's {-shift, 1 / scale} are derived on the device from order statistics of its own
// 16-bit values, written to SignalOut::cal, and the store pass reads them there.  The statistics are found by counting passes of the svb
// decoder (OUT = SIG_COUNT) over keys: the value's key u = the 16-bit value made monotone (int16: x + 32768; uint16: x), or, for the MAD,
// d = |2u - c2| (c2 = twice the median in keys).  A pass counts up to NORM_WINDOWS windows of NORM_BINS bins, window w holding the keys
// [lo[w], lo[w] + NORM_BINS << sh[w]) and a count of the keys below it; after it, the select narrows every wanted rank's bracket [a, z].
// The first pass's windows are four adjacent ones of width 1 around the read's first sample (NormRead::anchored); every later window
// covers one unresolved bracket whole, so a bracket shrinks NORM_BINS-fold per pass.
constexpr uint32_t NORM_MED_MAD = 1, NORM_QUANTILE = 2;   // (= VBZ_GPU_NORM_*)
constexpr uint32_t NORM_VALUE = 0, NORM_DEV = 1, NORM_DONE = 2;   // NormRead::phase: keys u, keys d, finished
constexpr uint32_t NORM_WINDOWS = 4, NORM_BINS = 1024, NORM_OFF = 0xFFu;   // sh[w] == NORM_OFF: window w is not counted
constexpr uint32_t NORM_SLAB = NORM_WINDOWS * NORM_BINS + 8;   // words per read of the large-read path's counts (bins, then below[4])
struct NormRead
{
    uint32_t phase, c2, anchored, pad;
    uint32_t lo[NORM_WINDOWS], sh[NORM_WINDOWS];   // the next pass's windows
    uint32_t a[NORM_WINDOWS], z[NORM_WINDOWS];     // target t's key lies in [a[t], z[t]] (a == z: found)
};
struct NormOut
{
    NormRead* st = nullptr;          // per read, in the batch's read order; non-null: a normalising decode
    float2* ss = nullptr;            // the caller's shift_scale ({shift, scale}) at map ? map[r] : r
    const uint32_t* map = nullptr;   // (routed reads: their index in the call's batch)
    uint32_t* slab = nullptr;        // large-read path: NORM_SLAB words per read the segments add their counts into (zero between passes)
    uint32_t method = 0;
    float qa = 0.0f, qb = 0.0f, shift_mul = 0.0f, scale_mul = 0.0f, shift_min = 0.0f, scale_min = 0.0f;
};
// counting passes a method may need (the first pass, then <= 2 per stage of keys): every read is finished after them
inline uint32_t norm_passes(uint32_t method) { return method == NORM_MED_MAD ? 5u : 3u; }

struct SignalOut
{
    const float2* cal = nullptr;   // per read {offset, scale}, in the batch's read order (a normalising decode: its select writes them)
    uint32_t type = SIG_NONE;      // (a normalising decode with SIG_NONE: the statistics only, no store)
    uint32_t bias = 0;
    const uint64_t* row = nullptr;   // chunk store: per read, its first row (chunk_first), in the batch's read order
    uint32_t chunk_len = 0, step = 0, mode = 0, end_align = 0;
    float pad = 0.0f;
    NormOut norm;
    // Sample ranges (vbz_gpu_*_range_batch): read i's chunks (and, with rstats == RANGE_STATS_RANGE, its statistics) are those of its
    // samples [b, e) -- e = min(rend[i], T), b = min(rbegin[i], e); a NULL table: 0 / T -- taken as a read of e - b samples.  The tables
    // are the caller's (untrusted); entry rmap ? rmap[r] : r is read r's (routed reads: their index in the call's batch; POD5: per READ).
    const uint32_t* rbegin = nullptr;
    const uint32_t* rend = nullptr;
    const uint32_t* rmap = nullptr;
    uint32_t rstats = RANGE_STATS_RANGE;
    uint32_t events = 0;   // != 0: an event call (below; the word fills the struct's padding: no kernel's arguments move)
    __host__ __device__ bool ranged() const { return rbegin || rend; }
    __host__ __device__ bool ranged_stats() const { return ranged() && rstats == RANGE_STATS_RANGE; }
    // Signal windows (vbz_gpu_*_windows_batch; `row` stays NULL): read i owns rows wfirst[i] ... wfirst[i + 1] - 1 of the [wrows, chunk_len]
    // arena at dst, row c holding the samples wstart[c] ... wstart[c] + chunk_len - 1 of the read's signal (its range, when ranged) and
    // `pad` outside it.  The tables are the caller's (untrusted: the window check closes the gate of a read whose entries are not rows of
    // the arena or whose starts decrease); entry wmap ? wmap[r] : r of wfirst is read r's (routed reads; POD5: per READ).
    const uint64_t* wfirst = nullptr;
    const int32_t* wstart = nullptr;
    const uint32_t* wmap = nullptr;
    uint64_t wrows = 0;
    // Signal events (vbz_gpu_*_signal_events_batch; `events` != 0).  The tables are the windows' -- read i owns rows wfirst[i] ...
    // wfirst[i + 1] - 1 of wrows, wstart[c] (taken as uint32) is where event c begins in the read's signal, the window check is the event
    // check -- and the arena at dst holds the rows' exact moments: {sum x, sum x^2} of row c are the two 64-bit words at dst + 16 c, zeroed
    // by launch_event_zero, added to by the event pass (OUT = SIG_EVENT), read by launch_event_finish, which writes the records.
    __host__ __device__ unsigned long long* event_moments(uint8_t* dst) const { return reinterpret_cast<unsigned long long*>(dst); }
};
constexpr uint32_t WINDOW_READ_ROWS_MAX = 0x7FFFFFFFu;   // rows one read may own (the window check refuses more)

// Signal trim (vbz_gpu_*_signal_trim_batch; the rule: include/vbz_gpu.h): behind the counting passes of a statistics call one more pass of
// the svb decoder (OUT = SIG_TRIM) counts, window by window, the samples above thr = shift + f * scale in the first
// t0 + nW * W <= min(M, T) positions of every read, and the scan of those counts writes the read's trim point to begin[].  The trim is an
// argument of its own of the kernels that take it, beside their ReadBatch -- no other kernel's arguments change -- and the host keeps it there
// too (DecodeJob).  begin: the caller's table, entry norm.map ? norm.map[r] : r (POD5 reads of several rows: per READ); nullptr: no trim pass.
constexpr uint32_t TRIM_REJECT_AT_END = 1;   // (= VBZ_GPU_TRIM_REJECT_AT_END)
constexpr uint32_t TRIM_MAX_WINDOWS = NORM_WINDOWS * NORM_BINS;   // a read's window counts live in the counting passes' bins (NormLds::h, NormOut::slab)
struct TrimOut
{
    uint32_t* begin = nullptr;
    uint32_t W = 0, m = 0, t0 = 0, M = 0, flags = 0;
    float f = 0.0f, max_fraction = 1.0f;
};
struct SpanOut;   // (signal spans: below, beside SegmentOut)

// the clamped range of read r of T samples: *rb <= *re <= T (no address is formed from a table value before this)
__device__ inline void sample_range(const SignalOut& sg, uint32_t r, uint32_t T, uint32_t* rb, uint32_t* re)
{
    const uint32_t i = sg.rmap ? sg.rmap[r] : r;
    const uint32_t e0 = sg.rend ? sg.rend[i] : T, e = e0 < T ? e0 : T;
    const uint32_t b0 = sg.rbegin ? sg.rbegin[i] : 0u;
    *re = e;
    *rb = b0 < e ? b0 : e;
}

// the chunking of a read of T samples (include/vbz_gpu.h, vbz_gpu_chunking): K chunks, the last one starting at chunk_last_start
__host__ __device__ inline uint32_t chunk_count(uint32_t T, uint32_t L, uint32_t S)
{
    if (T == 0) return 0;
    if (T <= L) return 1;
    return (T - L + S - 1) / S + 1;
}
__host__ __device__ inline uint32_t chunk_last_start(uint32_t T, uint32_t K, uint32_t L, uint32_t S, uint32_t mode, uint32_t end_align)
{
    if (K <= 1) return 0;
    const uint32_t g = (K - 1) * S;
    if (mode != CHUNK_END) return g;
    const uint32_t e = (T - L + end_align - 1) / end_align * end_align;
    return e < g ? e : g;
}

// Arrays carved out of one buffer of device scratch, each 16-byte aligned (host only).  base == nullptr measures: the same take<>() calls
// carve nothing, and bytes() behind them is what to allocate -- the arrays and a quarter more + 512 bytes of headroom (allocations are
// not sized to the byte: a kernel that reads a vector past the end of its array stays inside the buffer).
struct MetaCarver
{
    uint8_t* p;
    size_t off = 0;
    explicit MetaCarver(void* base) : p((uint8_t*)base) {}
    template <typename T>
    T* take(size_t n)
    {
        off = (off + 15) & ~(size_t)15;
        T* r = p ? (T*)(p + off) : nullptr;
        off += n * sizeof(T);
        return r;
    }
    size_t bytes() const { return off + off / 4 + 512; }
};

// One batch of independent reads ("reads" in the reference's vocabulary: one HDF5 chunk each).
// All pointers are device pointers.  `result[i]` receives the bytes produced or an error code.
// If `gate` is non-null, reads whose gate[i] is an error code are skipped and the error is kept; reads whose gate[i] is
// GATE_SKIP belong to another launch group of the same call (per-read routing: vbz_api.hip): nothing of theirs is touched.
struct ReadBatch
{
    uint32_t n_reads;
    const uint8_t* src;
    const uint64_t* src_off;
    const uint32_t* src_size;
    uint8_t* dst;
    const uint64_t* dst_off;
    const uint32_t* dst_cap;
    uint32_t* result;
    const uint32_t* gate;
    SignalOut sig;   // decode only: what the svb stage stores (every other stage ignores it)
};

// The gate protocol of read r, the first thing every kernel over a ReadBatch decides: 0 = go on; GATE_SKIP = the read is another launch
// group's (nothing of it is written); else the verdict the read keeps -- the gate's error, else (inherits: src_size can carry one, which
// is so for every decoder and for no encoder) the previous stage's, left in src_size[r].  The order is part of the ABI: it decides which
// verdict a read that is bad in two ways gets.
// The passes of a normalising decode that stand around its counting passes (norm_init_read, norm_select_read, trim_read_open) ask no
// more than this and an even dst_cap: the counting pass opens every read in full (svb_read_open / svb16_row_open) and writes its verdict,
// the trim behind it tests result[], the select NormRead::phase and then touches only the read's own state and slab (no address comes
// from the stream), and the init in front of it forms no address but the stream's first bytes, whose presence it checks itself.
__device__ __forceinline__ uint32_t read_gate(const ReadBatch& b, uint32_t r, bool inherits)
{
    if (b.gate && b.gate[r] >= GATE_SKIP) return b.gate[r];
    if (inherits && b.src_size[r] >= E_FIRST) return b.src_size[r];
    return 0;
}
// a read that was not opened: thread 0 of the workgroup leaves its verdict (read_gate's, or an open function's), if one is to be written
__device__ __forceinline__ void read_closed(const ReadBatch& b, uint32_t r, uint32_t verdict)
{
    if (threadIdx.x == 0 && verdict != GATE_SKIP) b.result[r] = verdict;
}

// ---- the per-read plans of the staged encoder (zstd_encode.hip), and what the svb encoder leaves in them ---------------------------
// The entropy stage turns every run of >= RMIN equal control bytes into a zstd sequence and Huffman-codes what is left, each region from
// its own byte histogram.  The one-wavefront path does that in stages that hand a read on through its EncPlan: the svb encoder counts
// the data bytes' sample on the way (int16 zig-zag reads: svb_kernels.hip CNT), zstd_plan_kernel tokenises the control bytes, codes their
// sequences section and builds both regions' tables (two wavefronts per read), zstd_pack_kernel packs.
#ifndef VBZ_RMIN
#define VBZ_RMIN 12
#endif
constexpr uint32_t RMIN = VBZ_RMIN;  // shortest run of equal bytes that becomes a match (break-even is ~13 bytes); >= 8, <= 24
struct EncRegionPlan
{
    uint32_t S, nblk, nrec, seqmode, Sh, treeSize, huffLog, pad;
    uint32_t ctable[256];   // code | length << 16.  (reg[1], before zstd_plan_kernel: the histogram the svb encoder left: EncPlan::hist_mode)
    uint32_t tree[34];      // the tree description (136 bytes)
};
struct EncPlan
{
    EncRegionPlan reg[2];
    uint32_t seqBytes, seqOff;      // the sequences section of region 0, coded by zstd_plan_kernel at the top of the destination slot
    uint32_t cpCount, cpSpacing;    // its decoder checkpoints (CP_MAGIC trailer)
    uint32_t cp[64];
    // the control bytes are tokenised IN PLACE (their literals compacted to the front of the region, the run records at the tail of the
    // scratch slot): whoever codes the read afterwards takes the result from here
    uint32_t tok_done, tok_nrec, tok_lit;
    // histogram of the data bytes the svb encoder left: 0 none; 1: reg[1].ctable = the data bytes region_histogram's sample counts (one
    // kilobyte in four + the unaligned ends); 2: and histB = the data bytes the sample leaves out (reads so short that the region may be
    // counted exactly)
    uint32_t hist_mode;
    uint32_t pad[8];
    uint32_t histB[256];
};
constexpr uint32_t PLAN_OPEN = 1, PLAN_REG0 = 2, PLAN_REG1 = 4, PLAN_READY = 7;
constexpr uint32_t ENC_TRAILERS = 1, ENC_PRE_FILLED = 2;   // bits of the entropy stage's `trailers` argument
inline EncPlan* zstd_encode_plans(void* plan_meta) { return reinterpret_cast<EncPlan*>(plan_meta); }   // the plans inside plan_meta

// ---- streamvbyte stage (svb_kernels.hip) -------------------------------------------------------
// integer_size in {1,2,4}; zigzag.
// hdr: 0, or 4 to prepend / skip the sized header (u32 LE original size) in front of the svb stream.
// strict_cap: apply the reference's worst-case capacity rule (keys + 4 bytes per value) to dst_cap.
// half: the v1 nibble codec for 1-byte integers (vbz/v1/vbz_streamvbyte_impl.h)
// period_hint (nullable, n_reads words): the encoder also looks for ONE long repeat distance in the data bytes it writes
// (svb_kernels.hip: PeriodProbe) and leaves it there (0: none) for the entropy stage's long-repeat coder.
// plans (nullable: the plan_meta of launch_zstd_encode; int16 zig-zag reads into library scratch only): every read's data bytes are
// counted on the way and the histogram left in its plan (EncPlan::hist_mode, written for EVERY read of the launch).
hipError_t launch_svb_encode(const ReadBatch& b, int integer_size, bool zigzag, uint32_t hdr, bool strict_cap, bool half, uint32_t* period_hint,
                             void* plans, hipStream_t s);
bool svb_encode_fills_plans(int integer_size, bool zigzag, bool half);   // does launch_svb_encode(plans) write every read's hist_mode?
// Decode: b.sig.type != SIG_NONE (integer_size 2 only; launch_svb_decode_seg too) stores the typed samples of SignalOut (OUT = b.sig.type,
// | SIG_CHUNK with b.sig.row).  b.sig.norm.st (integer_size 2 only; both launchers): the counting passes and their selects run in front of
// the store and leave every read's constants in b.sig.cal (and b.sig.norm.ss); with b.sig.type == SIG_NONE they are all that runs (the
// results are the int16 decode's; launch_svb_decode_seg: b.sig.norm.slab must be set).
// b.sig.rbegin / rend (the chunk stores and the counting passes only; launch_svb16_decode and launch_svb_decode_seg too): the ranged
// instantiations (OUT | SIG_RANGE) store the chunks of every read's clamped range, and with rstats == RANGE_STATS_RANGE count its values alone.
// trim (nullable; with b.sig.norm.st only; every decode launcher below too): the trim pass behind the last counting pass.
// span (nullable; int16 samples, b.sig.type == SIG_NONE; every decode launcher below too): the span pass -- behind the last counting pass with
// b.sig.norm.st, where result[] is the counting passes'; else it is all that runs and writes the int16 decode's verdicts itself.
hipError_t launch_svb_decode(const ReadBatch& b, int integer_size, bool zigzag, bool half, hipStream_t s, const TrimOut* trim = nullptr,
                             const SpanOut* span = nullptr);
// svb16, the svb stage of POD5 signal rows (int16 samples, delta + zig-zag; one key bit per sample): one workgroup per read, on every
// path.  Encode: the worst case ceil(n / 8) + 2n must fit dst_cap (else E_DESTINATION_SIZE); period_hint (nullable) is zeroed (no
// matcher).  Decode: the stores of launch_svb_decode(2, zigzag) (b.sig; b.sig.norm.slab must be NULL); a stream longer than
// ceil(n / 8) + 2n is E_ZSTD, one whose length the key bits do not announce E_STREAM.
hipError_t launch_svb16_encode(const ReadBatch& b, uint32_t* period_hint, hipStream_t s);
hipError_t launch_svb16_decode(const ReadBatch& b, hipStream_t s, const TrimOut* trim = nullptr, const SpanOut* span = nullptr);
// key_raw[i]: the raw size whose key region at key_elem = 4 is svb16's ceil(n / 8) bytes (the entropy stage's orig_size for POD5, hdr 0)
hipError_t launch_svb16_key_raw(uint32_t n, const uint32_t* raw_size, uint32_t* key_raw, hipStream_t s);
constexpr uint32_t SVB16_KEY_ELEM = 4;
// POD5 reads of several rows (vbz_gpu_pod5_* of include/vbz_gpu.h): the batch's entries are rows, first_row (untrusted) says which rows
// form a read, and the chunk store and the counting passes see a read's rows as one signal.  The tables are the call's scratch, filled by
// the plan launch: row i lies s0 samples into read `read`; the read has T samples, its chunks start at chunk row `row`.
constexpr uint32_t POD5_ROW_PAD = 1;     // Pod5Row::flags: this row's workgroup writes the read's pad lines (the read's last row)
constexpr uint32_t POD5_READ_FAIL = 1;   // Pod5Read::flags: the read failed its check (chunk_first, or 2^31 samples and more): nothing of it is stored
constexpr uint32_t POD5_READ_PAD_ELEMS = 2;   // the line that holds the read's last sample was stored element by element: its pad positions are the pad writer's
struct Pod5Row
{
    uint32_t s0, read, flags, pad;
};
struct Pod5Read
{
    uint32_t T, flags;
    uint64_t row;
};
struct Pod5Reads
{
    uint32_t n_reads = 0;
    const uint32_t* first_row = nullptr;   // the caller's, n_reads + 1 words; no kernel but the check reads it while *bad is not known to be 0
    uint32_t* read_result = nullptr;       // the caller's (nullable)
    Pod5Row* rows = nullptr;               // per row of the batch
    Pod5Read* reads = nullptr;             // per read
    uint32_t* bad = nullptr;               // one word: != 0 when first_row is not a partition of the batch's rows
    uint2* range = nullptr;                // per read, a ranged call only: the clamped {b, e} of SignalOut's range (the plan writes them)
};
// Signal windows (SignalOut::wfirst), the launches in front of the decode.  b: the call's reads, or with pr.reads (a call over POD5 reads)
// its rows, the tables of b.sig being per READ of pr.  w: scratch of the call, n words and n + 1 offsets for n reads.
// launch_window_check (pack.hip): the window check.  Reads of a batch (pr.reads == NULL): cal[i] = {offset[i], scale[i]} as in
// launch_chunk_slots, and a read whose gate is open and whose two wfirst entries are not rows of the arena (first > next, next > wrows,
// more than WINDOW_READ_ROWS_MAX rows) gets gate[i] = E_DESTINATION_SIZE; POD5 reads: the plan has done that (POD5_READ_FAIL).  Then
// w.scan = the exclusive scan of the passing reads' row counts, and a grid-stride pass over those rows closes every read that has a pair
// start[c] > start[c + 1] among its rows (POD5: POD5_READ_FAIL, its rows' gates, its statistics finished).  No start is read before its
// read's pair has passed.
// launch_window_pad (svb_kernels.hip), behind it: the pad positions of every passing read's rows.
struct WindowScratch
{
    uint32_t* count = nullptr;   // [n]
    uint64_t* scan = nullptr;    // [n + 1]
    size_t carve(void* base, uint32_t n)   // (host only; base == nullptr measures: scratch_tables.h)
    {
        MetaCarver mc(base);
        scan = mc.take<uint64_t>((size_t)n + 1);
        count = mc.take<uint32_t>(n);
        return mc.bytes();
    }
};
hipError_t launch_window_check(const ReadBatch& b, const Pod5Reads& pr, const float* offset, const float* scale, const WindowScratch& w, hipStream_t s);
hipError_t launch_window_pad(const ReadBatch& b, const Pod5Reads& pr, const WindowScratch& w, hipStream_t s);
// Signal events (SignalOut::events), the launches around the event pass (svb_kernels.hip), both one thread per row counted in w.scan and both
// passing over the rows of a read the event check has closed.  launch_event_zero, behind launch_window_check: the rows' moments = 0.
// launch_event_finish, behind the event pass (and the counting passes of a normalising call): the rows' records (include/vbz_gpu.h:
// vbz_gpu_event) from their moments, into `out` -- the read's constants are {offset[i], scale[i]} (NULL: 0 / 1), or with b.sig.norm.st the
// read's {-shift, float32(1 / scale)} of b.sig.norm.ss.
hipError_t launch_event_zero(const ReadBatch& b, const Pod5Reads& pr, const WindowScratch& w, hipStream_t s);
hipError_t launch_event_finish(const ReadBatch& b, const Pod5Reads& pr, const float* offset, const float* scale, const WindowScratch& w, void* out,
                               hipStream_t s);
// Signal segmentation (vbz_gpu_*_signal_segment_batch; the rule: include/vbz_gpu.h): a pass of the svb decoder of its own kernels
// (svb_kernels.hip: SegmentStore) scores every position of a read's signal with the two-window t-statistic, picks the boundaries and
// leaves them as one bit per position in the read's map -- bytes [map_off[i], map_off[i] + ceil(T' / 8)) of `map`, every byte written by
// one lane, no sample stored -- and the read's row count (boundaries + 1; 0 for an empty signal) in rows[i].  Like the trim, the call's
// state is an argument of its own of the kernels that take it (the host: DecodeJob).  i: the read's entry of the call's tables (rmap: a routed read's; the
// upper half of a split call gets the tables offset).  A read whose map does not end inside map_cap gets E_OOM.
constexpr uint32_t SEGMENT_WINDOW_MAX = 32, SEGMENT_RADIUS_MAX = 32;
// the maps of a segmentation or a span call: one bit per position, read i's in bytes [map_off[i], map_off[i + 1]) of the call's scratch
struct ReadMaps
{
    uint8_t* map = nullptr;              // nullptr: not such a call
    const uint64_t* map_off = nullptr;   // [n + 1], multiples of 4 (launch_segment_layout)
    uint64_t map_cap = 0;
    const uint32_t* rmap = nullptr;
    // read r's entry of the call's tables
    __device__ uint32_t entry(uint32_t r) const { return rmap ? rmap[r] : r; }
    // whether read i's map of ceil(T / 8) bytes lies inside the call's scratch: no byte of a map is written before this has passed
    __device__ bool fits(uint32_t i, uint32_t T) const
    {
        const uint64_t a = map_off[i], z = map_off[i + 1];
        return z <= map_cap && a <= z && (uint64_t)((T + 7u) >> 3) <= z - a;
    }
};
struct SegmentOut : ReadMaps
{
    uint32_t* rows = nullptr;            // [n]
    uint32_t w1 = 1, w2 = 0, r = 1;      // the two windows (w2 0: one detector) and the radius
    double k1 = 1.0, k2 = 1.0;           // float64(t) * float64(t) of the two thresholds (exact: 48 bits)
};
// Signal spans (vbz_gpu_*_signal_spans_batch; the rule: include/vbz_gpu.h): a pass of the svb decoder (svb_store.h: SpanStore) compares every
// sample of a read with the read's threshold thr = a + f w and leaves the verdicts as one bit per position OF THE READ in the read's map --
// launch_segment_layout's, bytes [map_off[i], map_off[i] + ceil(T / 8)) of `map`; bit p is set when p lies in [b + p0, e) and sample p is in
// -- and launch_span_emit (pack.hip) merges, filters and writes the pairs.  {a, w}: level[i], or with level == nullptr the read's
// {shift, scale} of b.sig.norm.ss, behind the last counting pass.  i, rmap and the cut of a split call: as for SegmentOut.
constexpr uint32_t SPAN_ABOVE = 0, SPAN_BELOW = 1;   // (= VBZ_GPU_SPAN_*)
constexpr uint32_t SPAN_GAP_MAX = 65535, SPAN_LENGTH_MAX = 0x7FFFFFFFu;
struct SpanOut : ReadMaps
{
    const float2* level = nullptr;       // the caller's {a, w} per read, or nullptr: the statistics'
    uint32_t below = 0, D = 0, m = 1, p0 = 0;
    float f = 0.0f;
};
// One launch group of a decompress call on the host (no kernel sees it).  What cuts a call into groups cuts the job (vbz_api.hip: upper_half, route).
struct DecodeJob { ReadBatch rb; TrimOut trim; SegmentOut seg; SpanOut span; };   // trim.begin == nullptr / seg.map == nullptr / span.map == nullptr: none
// The tables of a segmentation call, per read of the call (POD5 reads of several rows: per READ): the maps' sizes and offsets, the sinks'
// row counts, the counts of the reads that passed and their scan.
struct SegmentScratch
{
    uint64_t* map_off = nullptr;   // [n + 1]
    uint64_t* scan = nullptr;      // [n + 1]
    uint32_t* size = nullptr;      // [n]
    uint32_t* rows = nullptr;      // [n]
    uint32_t* count = nullptr;     // [n]
    size_t carve(void* base, uint32_t n)   // (host only; base == nullptr measures: scratch_tables.h)
    {
        MetaCarver mc(base);
        map_off = mc.take<uint64_t>((size_t)n + 1);
        scan = mc.take<uint64_t>((size_t)n + 1);
        size = mc.take<uint32_t>(n);
        rows = mc.take<uint32_t>(n);
        count = mc.take<uint32_t>(n);
        return mc.bytes();
    }
};
// launch_segment_layout (pack.hip), in front of the pass: map_off = the scan of the maps' sizes, ceil(T / 8) rounded up to 4 bytes, T the
// read's samples (b.dst_cap; pr.reads, behind the plan: the reads').  launch_segment_emit (pack.hip), behind everything the call has
// queued: count[i] = rows[i] of a read whose result (POD5: every row's) is no error and has samples, else 0; their scan; then one
// workgroup per read writes event_first[i] (the last one event_first[n] too) and, where the read's rows end at or in front of start_cap,
// its starts -- 0 and the positions of its map's bits, in order -- else E_DESTINATION_SIZE to its result (POD5: its rows' and
// read_result).  start == nullptr: event_first alone.  A bad first_row (*pr.bad): nothing is written.
hipError_t launch_segment_layout(const ReadBatch& b, const Pod5Reads& pr, const SegmentScratch& sc, hipStream_t s);
hipError_t launch_segment_emit(const ReadBatch& b, const Pod5Reads& pr, const SegmentOut& so, const SegmentScratch& sc, uint64_t* event_first,
                               uint32_t* start, uint64_t start_cap, hipStream_t s);
// The pass itself (svb_kernels.hip), one workgroup per read on every path: launch_svb_segment (the svb codec, int16), launch_svb16_segment
// (POD5 rows as reads) and launch_svb16_segment_reads (POD5 reads of several rows, behind launch_pod5_reads_check: the plan, the layout,
// the pass -- a read's workgroup walks its rows in turn and writes their verdicts --, the read results).  result[] is the int16 decode's.
hipError_t launch_svb_segment(const ReadBatch& b, bool zigzag, const SegmentOut& so, hipStream_t s);
hipError_t launch_svb16_segment(const ReadBatch& b, const SegmentOut& so, hipStream_t s);
hipError_t launch_svb16_segment_reads(const ReadBatch& b, const Pod5Reads& pr, const SegmentOut& so, const SegmentScratch& sc, hipStream_t s);
// launch_span_emit (pack.hip), behind everything a span call has queued: one workgroup per read walks the read's map (the bits of its
// range [b, e)), merging in-positions at most so.D apart and dropping spans shorter than so.m -- sc.rows[i] = twice the spans of a read
// whose result (POD5: every row's) is no error, else 0; their scan; then the same walk writes edge_first[i] (the last one edge_first[n]
// too) and, where the read's pairs end at or in front of edge_cap, its {begin, end} pairs in positions of the signal -- else
// E_DESTINATION_SIZE to its result (POD5: its rows' and read_result).  edge == nullptr: edge_first alone.  A bad first_row: nothing.
hipError_t launch_span_emit(const ReadBatch& b, const Pod5Reads& pr, const SpanOut& so, const SegmentScratch& sc, uint64_t* edge_first, uint32_t* edge,
                            uint64_t edge_cap, hipStream_t s);
// row j of the rows counted in scan (n + 1 offsets, scan[0] = 0 <= j < scan[n]) -> its read: the last k with scan[k] <= j
__device__ inline uint32_t scan_find(const uint64_t* scan, uint32_t n, uint64_t j)
{
    uint32_t lo = 0, hi = n;   // scan[lo] <= j; scan[hi] > j or hi == n
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (scan[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// *bad = whether first_row is bad (first entry not 0, a decreasing pair, last entry not n_rows); when it is and out != NULL (n_reads words:
// read_result or read_samples), every out[k] = E_INPUT_SIZE
hipError_t launch_pod5_reads_check(uint32_t n_rows, const Pod5Reads& pr, uint32_t* out, hipStream_t s);
// read_samples[k] = the sum of the read's row_samples (2^31 and more: E_DESTINATION_SIZE); behind launch_pod5_reads_check
hipError_t launch_pod5_read_samples(const Pod5Reads& pr, const uint32_t* row_samples, uint32_t* read_samples, hipStream_t s);
// The svb16 stage of a call over reads, behind launch_pod5_reads_check.  b: the rows (src: their svb16 streams; gate: the rows' gate,
// WRITABLE -- a bad table closes every row's with E_INPUT_SIZE, a read that fails its check its rows' with E_DESTINATION_SIZE), while
// b.sig.cal, b.sig.row (the caller's chunk_first) and b.sig.norm.st / ss are per READ.  offset / scale (nullable): the reads' given
// constants (without b.sig.norm.st).  Launches: the plan (tables, checks, constants or the reads' starting windows), the counting passes
// (one workgroup per read, its rows in turn), the store (one workgroup per row; none for the statistics alone, whose first counting
// pass gives the rows' verdicts), the read results.  b.sig.rbegin / rend: per READ; pr.range must then be set (the plan fills it).
// b.sig.wfirst (a window call; b.sig.row must be NULL): win must be set; the window check and the pad launch follow the plan.
// b.sig.events (an event call): the same with the zero launch in the pad's place, and the finish launch into event_out behind the passes.
// span (a span call; spsc must be set): the maps' layout behind the plan, the span pass over reads behind the counting passes.
hipError_t launch_svb16_decode_reads(const ReadBatch& b, const Pod5Reads& pr, const float* offset, const float* scale, uint64_t chunk_rows,
                                     hipStream_t s, const TrimOut* trim = nullptr, const WindowScratch* win = nullptr, void* event_out = nullptr,
                                     const SpanOut* span = nullptr, const SegmentScratch* spsc = nullptr);
// The same stage with one read spread over many workgroups ("segments" of svb_seg_unit_bytes raw bytes), for batches of few,
// large reads (one 10 M-element buffer, one 400 k-sample read): seg_first[n_reads + 1] from launch_seg_plan; max_segs
// bounds the total segment count (the grid); seg_* are scratch arrays of max_segs entries.  Not for the nibble codec.
// self_max: calls of at most that many segments have no scan launch between the passes (svb_kernels.hip: SELF); 0: every call has them.
constexpr uint32_t SVB_SEG_SELF_MAX = 1024;
uint32_t svb_seg_unit_bytes(int integer_size);
hipError_t launch_svb_encode_seg(const ReadBatch& b, int integer_size, bool zigzag, uint32_t hdr, bool strict_cap, const uint32_t* seg_first,
                                 uint32_t max_segs, uint32_t* seg_bytes, uint64_t* seg_off, uint32_t self_max, hipStream_t s);
hipError_t launch_svb_decode_seg(const ReadBatch& b, int integer_size, bool zigzag, const uint32_t* seg_first, uint32_t max_segs,
                                 uint32_t* seg_val, uint64_t* seg_pos, uint32_t* seg_run, uint32_t self_max, hipStream_t s, const TrimOut* trim = nullptr,
                                 const SpanOut* span = nullptr);

// ---- zstd-format entropy stage (zstd_encode.hip / zstd_decode.hip) -----------------------------
// encode: frame content = src read.  The launchers' arguments are host-side aggregates, filled field by field; what is not set is not used.
// The key region: key_elem = integer size whose key section (ceil(n/4) bytes, n derived from `orig_size[i] / key_elem`) is split into
// its own blocks; 0 = no split.  key_bytes (nullable) gives the key-section length per read directly and overrides key_elem.
struct KeyRegion
{
    const uint32_t* orig_size = nullptr;
    uint32_t key_elem = 0;
    const uint32_t* key_bytes = nullptr;
};
// src_cap + seq_tables (both or neither): the source streams live in library-owned scratch slots of that
// capacity, which lets the encoder rewrite the control-byte region as literals + zero-run sequences.
struct ZeroRuns
{
    const uint32_t* src_cap = nullptr;
    const void* seq_tables = nullptr;
};
// 8 x u64 per read, shader-clock cycles spent per phase (debug aid, VBZ_HIP_PHASE_TIMING): of the whole frame in one launch (= 1), of
// the staged encoder's planning launch (= 2: two per read, one per role) or of its packing launch (= 3)
struct EncDebug
{
    unsigned long long *frame = nullptr, *plan = nullptr, *pack = nullptr;
};
struct ZstdEncodeArgs
{
    KeyRegion key;
    uint32_t hdr = 0;        // 0 or 4 (sized header carrying orig_size[i] in front of the frame)
    ZeroRuns runs;
    bool trailers = false;   // append the decoder-checkpoint skippable frame when a sequences section was written (see zstd_encode.hip);
                             // (spans: checkpoints and span index behind the frame)
    // deep_d (n_reads words): the repeat distance launch_svb_encode's probe proposes for every read (0: none).  Reads
    // whose proposal holds are coded by a second launch with the long-repeat matcher (what libzstd's match finder gets out of
    // template-cycling signal, at every level); deep_d[r] is rewritten with the verdict.  The matcher's workspace is the top of
    // the destination slot (reads whose slot is too small for frame and workspace are coded without it).
    uint32_t* deep_d = nullptr;
    // plan_meta (zstd_encode_plan_bytes(n_reads) bytes of device scratch): the per-read plans.  staged: the ordinary read is
    // coded by the staged launches (tokeniser + sequences section, tables, packing -- each at the occupancy its own footprint allows) and
    // only what they leave over by the one-launch kernel; same frames either way.  pre_filled: launch_svb_encode(plans) has left every
    // read's hist_mode (and histogram) in the plans.  (launch_zstd_encode only)
    void* plan_meta = nullptr;
    bool staged = false, pre_filled = false;
    EncDebug dbg;
};
hipError_t launch_zstd_encode(const ReadBatch& b, const ZstdEncodeArgs& a, hipStream_t s);
size_t zstd_encode_plan_bytes(uint32_t n_reads);
size_t seq_tables_bytes();
void seq_tables_build(void* host_buffer);
// A second stream and two events for launches that run beside the main chain (the chain walk beside the launches for own frames, the
// shared-table spans beside the control-byte spans); stream == nullptr: none
struct SideStream
{
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
typedef SideStream FastSide;
// The same stage for batches of few, large reads: one wavefront per SPAN of a read's stream (see zstd_encode.hip).  a: key, hdr, runs,
// trailers.  stream_bytes bounds the total of the source streams; meta / tmp: zstd_span_meta_bytes / zstd_span_tmp_bytes of device
// scratch for the same stream_bytes, n_reads and shared_span_bytes (meta 16-byte aligned; the launcher carves its tables from it).
// shared_span_bytes: zstd_span_shared_bytes(the call's stream bytes), or 0 -- not 0: the data bytes of a read with a control-byte region
// get ONE table (counted and built by extra wavefronts of the launch that codes the control-byte spans) and are packed one wavefront
// per 8 KB span by the launch behind it; 0: a batch of large buffers, a matter of throughput, where every span builds its own table in
// one launch.
struct SpanEncodeWork
{
    uint64_t stream_bytes = 0;
    void* meta = nullptr;
    uint8_t* tmp = nullptr;
    uint32_t shared_span_bytes = 0;
};
size_t zstd_span_meta_bytes(uint64_t stream_bytes, uint32_t n_reads, uint32_t shared_span_bytes);  // 0: too large
uint64_t zstd_span_tmp_bytes(uint64_t stream_bytes, uint32_t n_reads);
uint32_t zstd_span_shared_bytes(uint64_t stream_bytes);
hipError_t launch_zstd_encode_spans(const ReadBatch& b, const ZstdEncodeArgs& a, const SpanEncodeWork& w, hipStream_t s);
// The long-repeat matcher in front of the span launches (batches too small to fill the device run as spans): a probe over
// every read below max_raw bytes, the check of launch_zstd_encode's first launch, and its matcher instantiation for the reads
// whose distance holds.  a: key, hdr, runs, trailers, and deep_d[n_reads] as scratch; gate_out[i] = GATE_SKIP for the reads coded here
// (the spans skip them), gate_in[i] otherwise.  b: as for launch_zstd_encode (source streams in library-owned slots of src_cap[i] bytes).
hipError_t launch_zstd_encode_matcher(const ReadBatch& b, const ZstdEncodeArgs& a, uint32_t max_raw, const uint32_t* gate_in, uint32_t* gate_out,
                                      hipStream_t s);
// decode: result[i] = frame content size, E_ZSTD for a malformed frame, or `toosmall_code` when the
// frame's content size exceeds dst_cap[i].
// seq_dtables (device, from seq_dtables_build): decoding tables of the predefined LL / ML distributions.
hipError_t launch_zstd_decode(const ReadBatch& b, uint32_t toosmall_code, unsigned long long* dbg, const void* seq_dtables,
                              hipStream_t s);
// Frames the reference wrote (libzstd: blocks of general sequences): the sequence chains of the reads with redo[i] != 0 walked one
// lane per frame ahead of the one-wavefront decoder (zstd_decode_ref.hip), which takes a frame's records when RefPre.ok says so.
constexpr uint32_t REF_MAXBLK = 4;
struct RefBlock
{
    uint32_t pos;             // where the block's header stands in the frame
    uint32_t nseq;
    uint32_t rec_lo, rec_hi;  // its first record in the workspace ({literal length, match length, offset, 0})
    uint32_t rep[3];          // the repeat offsets behind the block
    uint32_t end;             // the output position behind the block
};
struct RefPre
{
    uint32_t ok, nblk;
    uint32_t why;                                // BAIL: why the frame was left alone (diagnostics, VBZ_HIP_TRACE)
    uint32_t tab_cycles, chain_cycles, nseq_last;   // the frame's last block: cycles of its tables and of its chain, its sequences
    uint32_t pad[2];
    RefBlock blk[REF_MAXBLK];
};
// The literals of a reference-written frame's first block, decoded ahead of the one-wavefront decoder BESIDE the chain walk (the walk is a
// few hundred wavefronts bound by latency; the literals are seven tenths of such a frame's cycles and need nothing of the chains):
// blk = where the block header sits in the frame (0: not done), regen / csize as its literals header says, at = where in the
// destination slot the literals stand.  The decoder takes them when its own reading of the block says the same four numbers.
struct RefLits
{
    uint32_t blk, regen, csize, at;
    uint32_t tb, pcap;           // the literals stand in 64 stripes of pcap bytes from offset tb of the slot; lits_pos[64 r + q]: the first literal of stripe q
    uint32_t tail, pad;          // tail != 0: literal x also stands at tail - regen + x of the slot -- where the literals behind the last sequence
                                 // belong if the block's content ends at `tail` (the frame's content size for a last block, else a full block)
};
struct RefChains  // what launch_zstd_decode_only needs of them (pre == nullptr: none)
{
    const RefPre* pre = nullptr;
    const void* recs = nullptr;
    const RefLits* lits = nullptr;   // (nullable; only looked at for frames whose chains are walked) record k of read r at k * n_reads + r, k < REF_MAXBLK ...
    const uint32_t* lits_pos = nullptr;   // ... and 64 words per record
    uint32_t lits_units = 0;              // records per read this call has filled (k < lits_units)
};

size_t zstd_ref_pre_bytes(uint32_t n_reads);
const RefPre* zstd_ref_pre(const void* pre_meta);  // the per-frame hand-overs inside pre_meta
size_t zstd_ref_table_bytes(uint32_t n_reads);     // 0: a batch of this size keeps its tables in LDS
// pre_meta: zstd_ref_pre_bytes(n_reads); tables: zstd_ref_table_bytes(n_reads); recs: recs_cap records of 16 bytes.  *out: for the decoder.
hipError_t launch_zstd_ref_chain(const ReadBatch& b, const uint32_t* redo, void* pre_meta, void* tables, void* recs, uint64_t recs_cap, RefChains* out,
                                 hipStream_t s);
// The one-wavefront decoder for the reads with only[i] != 0 (the others are left alone); dbg: phase cycle counters (nullable).
hipError_t launch_zstd_decode_only(const ReadBatch& b, uint32_t toosmall_code, const void* seq_dtables, const uint32_t* only, RefChains chains,
                                   unsigned long long* dbg, hipStream_t s);
// Batched decoder for frames of the shape zstd_encode.hip writes (zstd_decode_fast.hip: one lane per frame for the headers, one lane
// per tree description, one wavefront per frame for nothing but the streams, one for the zero-run block); every frame that is not of
// that shape or fails a check, and every error verdict, goes through launch_zstd_decode_only at the end.  Same results as
// launch_zstd_decode.
size_t zstd_fast_meta_bytes(uint32_t n_reads);
const RefLits* zstd_ref_lits(const void* lit_meta, uint32_t n_reads);   // (diagnostics: zstd_ref_lit_units() records per read; blk != 0 = that block's literals were decoded ahead)
bool zstd_ref_literals_enabled();                                   // VBZ_HIP_REF_LITERALS
const uint32_t* zstd_fast_redo(const void* meta, uint32_t n_reads);  // after the call: redo[i] == 0 <=> frame i was decoded by the batched decoder
// The batched decoder's arguments.  meta: zstd_fast_meta_bytes(n_reads) bytes of device scratch.
// ref.*: scratch of launch_zstd_ref_chain (ref.pre == nullptr: frames of other writers go to the one-wavefront decoder as they are);
// ref.lits (nullable): zstd_ref_lit_meta_bytes(n_reads) bytes for the literals decoded beside the walk (zstd_ref_lit_units() records per
// read; ref.lit_units: how many of them this call fills -- blocks per frame that get a workgroup).
// dbg (nullable): phase cycle counters of the one-wavefront decoder, which then decodes EVERY frame (walked chains included).
struct RefWork
{
    void *pre = nullptr, *tables = nullptr, *recs = nullptr;
    uint64_t recs_cap = 0;   // records of 16 bytes
    void* lits = nullptr;
    uint32_t lit_units = 0;
};
struct FastDecodeArgs
{
    uint32_t toosmall_code = 0;
    const void* seq_dtables = nullptr;
    void* meta = nullptr;
    RefWork ref;
    unsigned long long* dbg = nullptr;
    FastSide side;
};
hipError_t launch_zstd_decode_fast(const ReadBatch& b, const FastDecodeArgs& a, hipStream_t s);
#ifdef VBZ_EXPERIMENTS
hipError_t zstd_fast_runs_counts(unsigned long long out[4], bool reset);   // fast_runs_kernel's path counters (zstd_decode_fast.hip)
hipError_t zstd_fast_streams_counts(unsigned long long out[3], bool reset);   // fast_streams_kernel's refill counters (zstd_decode_fast.hip)
#endif
size_t zstd_ref_lit_meta_bytes(uint32_t n_reads);
uint32_t zstd_ref_lit_units();
const uint32_t* zstd_ref_lit_skip(const void* lit_meta, uint32_t n_reads);   // (diagnostics: 0 = the scan made the block a unit)
size_t seq_dtables_bytes();
void seq_dtables_build(void* host_buffer);
// The same for batches of few, large reads: frames that carry the encoder's span index are decoded one span per wavefront
// (verified; anything else, and every error verdict, comes from the ordinary decoder in a second launch gated by redo[]).
// content_bytes bounds the total frame content; meta: zstd_dspan_meta_bytes(content_bytes, n_reads) bytes of device scratch, 16-byte
// aligned (the launcher carves its tables from it).  redo (out): n_reads words inside meta, after the call redo[i] == 0 <=> frame i was
// decoded as spans.
struct SpanDecodeArgs
{
    uint32_t toosmall_code = 0;
    const void* seq_dtables = nullptr;
    uint64_t content_bytes = 0;
    void* meta = nullptr;
    const uint32_t* redo = nullptr;
};
size_t zstd_dspan_meta_bytes(uint64_t content_bytes, uint32_t n_reads);  // 0: too large
hipError_t launch_zstd_decode_spans(const ReadBatch& b, SpanDecodeArgs* a, hipStream_t s);

// ---- the zstd content checksum (xxh64.hip) ------------------------------------------------------
// out[i] = XXH64 (seed 0) of src[off[i] .. off[i] + len[i]); reads with len[i] or skip[i] >= E_FIRST, gate[i] >= GATE_SKIP are left alone (gate, skip
// nullable).  One quad of lanes per buffer.
hipError_t launch_xxh64_batch(const uint8_t* src, const uint64_t* off, const uint32_t* len, const uint32_t* gate, const uint32_t* skip, uint32_t n,
                              uint64_t* out, hipStream_t s);
// After the zstd stage of a decode (b: the frames, their decoded content at dst + dst_off[i], result[i] its size): a frame with
// Content_Checksum_flag whose content does not hash to the stored value gets result[i] = E_ZSTD.  Frames without the flag: one byte read.
hipError_t launch_xxh64_verify(const ReadBatch& b, hipStream_t s);
// After the entropy stage of an encode (b: the frames written, result[i] bytes at dst + dst_off[i] including `hdr` bytes of sized header;
// hash[i] = XXH64 of the frame's content): Content_Checksum_flag and the checksum behind the last block, the trailers moved behind it.
// raw_size (nullable) + integer_size: the raw read sizes whose vbz_max_compressed_size the result must not exceed.
hipError_t launch_checksum_insert(const ReadBatch& b, const uint64_t* hash, uint32_t hdr, const uint32_t* raw_size, uint32_t integer_size, hipStream_t s);

// ---- dense arenas (pack.hip) ----------------------------------------------------------------------
// Layout of a batch's byte counts, each rounded up to `align` (a power of two): size[i] = the count or an error code (error entries
// occupy no bytes), off[i] = the exclusive scan, off[n] = the total.  Three launches (tile sums, their scan, the tiles' scans).
//   pack:  the count is result[i] when that is no error code, fits dst_cap[i] and the slot lies inside [0, dst_bytes); a count that
//          does not fit gets E_INPUT_SIZE, an error code stays as it is (vbz_gpu_pack_batch)
//   sized: the little-endian u32 header of every buffer, E_INPUT_SIZE for a buffer under 4 bytes or outside [0, src_bytes)
hipError_t launch_pack_layout(uint32_t n, const uint32_t* result, const uint64_t* dst_off, const uint32_t* dst_cap, uint64_t dst_bytes, uint32_t align,
                              uint64_t* packed_off, uint32_t* packed_size, hipStream_t s);
hipError_t launch_sized_layout(uint32_t n, const uint8_t* src, const uint64_t* src_off, const uint32_t* src_size, uint64_t src_bytes, uint32_t align,
                               uint32_t* raw_size, uint64_t* raw_off, hipStream_t s);
// After launch_pack_layout: every read's packed_size[i] bytes (if no error code) from dst + dst_off[i] to packed + packed_off[i], the
// padding between them zero; nothing at all when packed_off[n] > packed_cap.  packed must not overlap the slots.
hipError_t launch_pack_gather(uint32_t n, const uint8_t* dst, const uint64_t* dst_off, const uint64_t* packed_off, const uint32_t* packed_size,
                              uint8_t* packed, uint64_t packed_cap, hipStream_t s);

// ---- helpers (helpers.hip) ---------------------------------------------------------------------
// scratch slots for the intermediate svb streams: slot(i) = align16(ceil(raw_size[i]*num/den)+8)+48,
// off[i] = exclusive scan + 16, cap[i] = slot - 32; gate[i] = E_OOM if the slot exceeds `limit` bytes.
// gate_is_input: gate[] already holds per-read errors; those reads keep their error and get an empty slot.
hipError_t launch_plan_scratch(uint32_t n, const uint32_t* raw_size, uint32_t mul_num, uint32_t mul_den, uint64_t limit,
                               uint64_t* off, uint32_t* cap, uint32_t* gate, bool gate_is_input, hipStream_t s);
// seg_first[i] = number of segments of reads 0..i-1, a read of `size` bytes having max(1, ceil(size / unit_bytes)) of them
// (seg_first[n] = total); reads whose gate is an error get one segment.  max_segs = the size of the caller's segment tables
// (and grids): reads whose segments would not fit them (sources that alias each other can add up to more than the arena)
// keep one segment and get gate_out[i] = E_OOM; gate_out[i] = gate[i] (or 0) otherwise.  gate_out may be gate.
// scratch (nullable; used when n <= 1024): the scratch plan of launch_plan_scratch for the same reads in the same launch -- off / cap as
// there, gate[i] = gate_out[i] or E_OOM for a read whose slot does not fit.
struct ScratchPlan
{
    uint32_t num, den;
    uint64_t limit;
    uint64_t* off;
    uint32_t* cap;
    uint32_t* gate;
};
hipError_t launch_seg_plan(uint32_t n, const uint32_t* size, uint32_t unit_bytes, const uint32_t* gate, uint32_t max_segs, uint32_t* seg_first,
                           uint32_t* gate_out, const ScratchPlan* scratch, hipStream_t s);
hipError_t launch_count_nonzero(const uint32_t* a, uint32_t n, uint32_t* out, hipStream_t s);   // *out = the words of a[0..n) that are not zero
// canonical mode: see canon_classify_kernel (helpers.hip).  counts: two words of device memory.
hipError_t launch_canon_classify(uint32_t n, const uint32_t* raw_size, const uint32_t* gate, uint32_t min_bytes, uint32_t* gate_small, uint32_t* gate_large,
                                 uint32_t* counts, hipStream_t s);
// per-read routing: see route_reads_kernel (helpers.hip).  raw_size[i] = the read's raw (decoded) byte count.
// large: the routed reads' table, max_reads entries each (cal / row: their b.sig.cal / b.sig.row entries, not written when those are NULL);
// map[k] = routed read k's index in b, count: how many there are.  cand: route_cand_words() words of scratch.
struct RoutedTable
{
    uint64_t* src_off = nullptr;
    uint32_t* src_size = nullptr;
    uint64_t* dst_off = nullptr;
    uint32_t *dst_cap = nullptr, *gate = nullptr, *map = nullptr;
    float2* cal = nullptr;
    uint64_t* row = nullptr;
    uint32_t* count = nullptr;
};
struct RouteArgs
{
    const uint32_t* raw_size = nullptr;
    uint32_t min_bytes = 0, max_reads = 0;
    uint64_t max_bytes = 0;
    uint32_t* gate_small = nullptr;
    RoutedTable large;
    uint32_t* cand = nullptr;
};
hipError_t launch_route_reads(const ReadBatch& b, const RouteArgs& a, hipStream_t s);
size_t route_cand_words();
hipError_t launch_route_results(const uint32_t* l_result, const uint32_t* l_map, const uint32_t* l_count, uint32_t max_reads, uint32_t* result, hipStream_t s);
// sized decode: read the 4-byte headers -> payload offsets/sizes, original sizes, gate errors (gate_in, nullable: reads that
// already carry an error keep it and are not looked at)
hipError_t launch_parse_sized(uint32_t n, const uint8_t* src, const uint64_t* src_off, const uint32_t* src_size,
                              const uint32_t* dst_cap, const uint32_t* gate_in, uint64_t* pay_off, uint32_t* pay_size, uint32_t* orig_size,
                              uint32_t* gate, hipStream_t s);
// descriptor table against the declared arenas: gate[i] = 0, E_INPUT_SIZE (source slot outside [0, src_bytes)) or
// E_DESTINATION_SIZE (destination slot outside [0, dst_bytes)); 64-bit arithmetic
// The single-buffer API's hand-back: `*result` bytes at `src` (if no error code and <= host_cap) into pinned host memory at host + 16
// words, the result word to host[0], the bytes copied to host[1], then host[2] = seq (system-scope release): what the host polls.
// ticket: one zeroed word of device memory the launch's workgroups count themselves on (left at zero).
hipError_t launch_hand_back(const uint32_t* result, const uint8_t* src, uint32_t* host, uint32_t host_cap, uint32_t seq, uint32_t* ticket, hipStream_t s);
hipError_t launch_validate_batch(uint32_t n, const uint64_t* src_off, const uint32_t* src_size, uint64_t src_bytes, const uint64_t* dst_off,
                                 const uint32_t* dst_cap, uint64_t dst_bytes, uint32_t* gate, hipStream_t s);
// typed decode (SignalOut): the caller's typed slot table -> the int16 one every decode launch plans with, off16[i] = dst_off[i] / elem * 2
// and cap16[i] = dst_cap[i] / elem * 2; cal[i] = {offset ? offset[i] : 0, scale ? scale[i] : 1}.  A slot whose offset or capacity is not a
// multiple of elem gets gate[i] = E_DESTINATION_SIZE (gate: launch_validate_batch's verdicts on the typed table, updated in place).
hipError_t launch_signal_slots(uint32_t n, const uint64_t* dst_off, const uint32_t* dst_cap, uint32_t elem, const float* offset, const float* scale,
                               uint64_t* off16, uint32_t* cap16, float2* cal, uint32_t* gate, hipStream_t s);
// chunk decode (SignalOut::row): the per-read table and the chunk check, once the int16 capacities are final (unsized: the caller's; sized:
// the headers' sizes).  cal[i] as in launch_signal_slots; a read whose gate is no error and whose chunk_first entries are not exactly
// its chunks (chunk_first[i] <= chunk_first[i + 1] <= chunk_rows, the difference chunk_count(cap16[i] / 2, L, S)) gets
// gate[i] = E_DESTINATION_SIZE: nothing of it is decoded or stored.
// sig (nullable): a ranged call's tables (SignalOut::rbegin / rend) -- the chunk check is then against the range's sample count.
hipError_t launch_chunk_slots(uint32_t n, const uint32_t* cap16, const float* offset, const float* scale, uint32_t L, uint32_t S,
                              const uint64_t* chunk_first, uint64_t chunk_rows, float2* cal, uint32_t* gate, const SignalOut* sig, hipStream_t s);
// range_samples[i] = the sample count of read i's clamped range (samples[i] of 2^31 or more, an error code, passes through)
hipError_t launch_range_samples(uint32_t n, const uint32_t* samples, const uint32_t* begin, const uint32_t* end, uint32_t* range_samples, hipStream_t s);
// chunk layout (pack.hip): chunk_first[i] = the exclusive scan of chunk_count(samples[i]) (samples of 2^31 or more: 0 chunks), chunk_first[n]
// the total; count: n words of scratch.  launch_chunk_info: when chunk_first[n] <= info_cap, info[2c] / info[2c + 1] = the read / start
// sample of row c (a grid-stride launch; nothing when the total is larger).
hipError_t launch_chunk_layout(uint32_t n, const uint32_t* samples, uint32_t L, uint32_t S, uint32_t* count, uint64_t* chunk_first, hipStream_t s);
hipError_t launch_chunk_info(uint32_t n, const uint32_t* samples, uint32_t L, uint32_t S, uint32_t mode, uint32_t end_align, const uint64_t* chunk_first,
                             uint32_t* info, uint64_t info_cap, hipStream_t s);
// integer_size == 0 && level == 0: per-read copy (reference vbz/vbz.cpp:130-133)
hipError_t launch_copy_bytes(const ReadBatch& b, uint32_t hdr, hipStream_t s);
hipError_t launch_synth_lengths(uint64_t seed, uint64_t first, uint32_t n, uint32_t* out_len, hipStream_t s);
hipError_t launch_synth_signal(uint64_t seed, uint64_t first, uint32_t n, uint8_t* dst, const uint64_t* off,
                               const uint32_t* len, hipStream_t s);
hipError_t launch_synth_u32(uint64_t seed, uint64_t first, uint32_t n, uint8_t* dst, const uint64_t* off,
                            const uint32_t* len, hipStream_t s);
// Signal match (match.hip; the rule: include/vbz_gpu.h, vbz_gpu_match): out[i R + r] = {cost, end} of the subsequence DTW of reference row
// r (ref + r ref_stride, ref_len[r] levels: untrusted, 0 or > ref_stride gives the empty verdict) against the first min(valid[i], N)
// samples of query row i (N floats a row), quantised by `quant`.  Every entry of out is written.
hipError_t launch_match(uint32_t n_reads, const float* query, const uint32_t* valid, uint32_t N, float quant, const int8_t* ref, const uint32_t* ref_len,
                        uint32_t R, uint32_t ref_stride, void* out, hipStream_t s);
// ... with the start of the aligned stretch (vbz_gpu_match_span): out[i R + r] = {cost, end, start, 0}, 16 bytes an entry.  The packed kernel
// or the wide one, by match_select.h from N and ref_stride alone.
hipError_t launch_match_span(uint32_t n_reads, const float* query, const uint32_t* valid, uint32_t N, float quant, const int8_t* ref,
                             const uint32_t* ref_len, uint32_t R, uint32_t ref_stride, void* out, hipStream_t s);
// The path calls (vbz_gpu_match_best_batch, vbz_gpu_match_path_batch).  launch_match_best: pairs[i] = {i, the reference of least cost
// <= max_cost among spans[i R ... i R + R), its start, its end} or {i, 0xFFFFFFFF, 0, 0}; 16-byte entries both.
hipError_t launch_match_best(uint32_t n_reads, const void* spans, uint32_t R, uint32_t max_cost, void* pairs, hipStream_t s);
// One group of a path call (vbz_gpu_match_path_batch, vbz_gpu_locate_path_batch): pairs first ... first + count - 1 of the caller's table,
// slot w = pair - first of the scratch.  `levels` is the int8 matrix: the references of a match, which sit in the lanes, or the targets of
// a locate, which are streamed -- a pair's window [begin, end) is in query samples in the one and in TARGET levels in the other.  The rows
// of the cost matrix are the lanes' operand, so a pair owns levels_stride entries of `rows` in a match and N in a locate.
struct AlignPathArgs
{
    const float* query;          // [n_reads, N]
    const uint32_t* valid;       // [n_reads], untrusted; a match: or nullptr, N samples a row
    uint32_t n_reads, N;
    float quant;
    const int8_t* levels;        // [n_levels, levels_stride]
    const uint32_t* levels_len;  // [n_levels], untrusted
    uint32_t n_levels, levels_stride;
    const uint4* pairs;          // {read, ref or target, begin, end}, untrusted
    uint32_t max_width;
    uint32_t first, count;
    uint64_t pair_words;         // match_path_pair_words(max_width, the rows' stride)
    uint32_t* bits;              // [count x pair_words]: the direction bits (MatchPathScratch)
    uint32_t* cost;              // [count]: the forward pass's cost
    uint4* hit;                  // [n_pairs]
    uint2* rows;                 // [n_pairs, the rows' stride]
};
// The forward launch (the packed kernel or the wide one, by match_select.h with max_width in N's place and, in a locate, N in ref_stride's)
// and the traceback behind it.  Between them every hit and every row of the group's pairs is written.
hipError_t launch_match_path_forward(const AlignPathArgs& a, hipStream_t s);
hipError_t launch_match_path_trace(const AlignPathArgs& a, hipStream_t s);
hipError_t launch_locate_path_forward(const AlignPathArgs& a, hipStream_t s);
hipError_t launch_locate_path_trace(const AlignPathArgs& a, hipStream_t s);
// ... the fused calls' tables.  launch_match_windows: the window tables of "one row per read at start 0" (first: n + 1 entries, start: n).
// launch_match_valid, behind the decode: valid[i] = min(T', N) from the verdict result[i] (T x 4 bytes; an error: 0) and the range tables
// (nullable), clamped as sample_range clamps them.
hipError_t launch_match_windows(uint32_t n, uint64_t* first, int32_t* start, hipStream_t s);
hipError_t launch_match_valid(uint32_t n, const uint32_t* result, const uint32_t* rbegin, const uint32_t* rend, uint32_t N, uint32_t* valid, hipStream_t s);
// Signal locate (locate.hip; the rule: include/vbz_gpu.h, vbz_gpu_locate): out[i G + g] = {cost, end} of the subsequence DTW of the first
// min(valid[i], N) samples of query row i (N <= 2048 floats a row), quantised by `quant` and aligned WHOLE, against target row g (target +
// g target_stride, target_len[g] int8 levels: untrusted, 0 or > target_stride gives the empty verdict; the row is read in dwords, so
// target is 4-byte aligned and target_stride a multiple of 4).  Every entry of out is written.
hipError_t launch_locate(uint32_t n_reads, const float* query, const uint32_t* valid, uint32_t N, float quant, const int8_t* target,
                         const uint32_t* target_len, uint32_t G, uint32_t target_stride, void* out, hipStream_t s);
// ... with the start of the aligned stretch: out[i G + g] = {cost, end, start, 0} (vbz_gpu_match_span, 16 bytes an entry), start in target
// coordinates, found by a bounded walk back from (cost, end) in the same wavefront.
hipError_t launch_locate_span(uint32_t n_reads, const float* query, const uint32_t* valid, uint32_t N, float quant, const int8_t* target,
                              const uint32_t* target_len, uint32_t G, uint32_t target_stride, void* out, hipStream_t s);
// Event-space alignment (eventalign.hip; the rules: include/vbz_gpu.h, vbz_gpu_events_query and vbz_gpu_level).  launch_events_query: row i
// of query / index ([n_reads, N]) = the means / the row numbers of read i's first N events with n >= min_n, zeros behind them, valid[i]
// their count; result (nullable) gates a read as launch_match_valid does, event_first is untrusted, index is nullable.
hipError_t launch_events_query(uint32_t n_reads, const uint32_t* result, const uint64_t* event_first, uint64_t event_rows, const void* records, uint32_t min_n,
                               uint32_t N, float* query, uint32_t* valid, uint32_t* index, hipStream_t s);
// launch_locate_levels: the path rows of pair p ([n_pairs, N] of {begin, end}, n = hit[p].w of them) inverted into one 32-byte record per
// target level of [hit[p].z, hit[p].y) in levels ([n_pairs, max_width]), zeros behind them, n_levels[p] their count; every table is
// untrusted, index is nullable.
hipError_t launch_locate_levels(uint32_t n_pairs, uint32_t n_reads, uint32_t N, uint32_t max_width, const void* pairs, const void* hit, const void* rows,
                                const uint32_t* index, const uint64_t* event_first, uint64_t event_rows, const uint32_t* start, const void* records,
                                const void* moments, uint32_t* n_levels, void* levels, hipStream_t s);
// The two ends of the event-space chain (squiggle.hip; the rules: include/vbz_gpu.h, vbz_gpu_squiggle and vbz_gpu_levels_fit).
// launch_squiggle: row r of target / level ([rows, target_stride]) = the quantised / the float32 model levels of the k-mers of sequence r
// (flags: VBZ_GPU_SQUIGGLE_*), zeros behind target_len[r]; masked[r] the k-mers that hold an invalid base, added up by a second launch
// over part, squiggle_part_words(rows, target_stride) words of scratch that the first launch writes whole.  seq_len is untrusted, level
// is nullable.
uint32_t squiggle_part_words(uint32_t rows, uint32_t target_stride);
hipError_t launch_squiggle(uint32_t k, uint32_t rows, uint32_t seq_stride, uint32_t target_stride, uint32_t flags, float quant, const uint8_t* seq,
                           const uint32_t* seq_len, const float* model, int8_t* target, uint32_t* target_len, uint32_t* masked, float* level, uint32_t* part,
                           hipStream_t s);
// launch_levels_fit: pair p's {offset, scale, used, ok} in out and its two floats again in offset / scale, from the least-squares line
// through (target level, mean of the level's record) over the rows of levels ([n_pairs, max_width]) that min_samples and max_entries keep;
// sums ([n_pairs, 4] int64: Sg, Sgg, Sq, Sgq) and prior ([n_reads] {shift, scale}) are nullable; every table is untrusted.
hipError_t launch_levels_fit(uint32_t n_pairs, uint32_t n_reads, uint32_t G, uint32_t target_stride, float quant, const int8_t* target,
                             const uint32_t* target_len, const void* pairs, const void* hit, const uint32_t* n_levels, const void* levels, uint32_t max_width,
                             uint32_t min_samples, uint32_t max_entries, const float* prior, void* out, float* offset, float* scale, int64_t* sums,
                             hipStream_t s);
// The pile-up across reads (pile.hip; the rules: include/vbz_gpu_pile.h).  A pile is four planes of n_cells 64-bit words: count word,
// n_samples, sum, sumsq.
// launch_levels_pile: every kept level of every valid pair (levels_fit's test) added into cell ref * target_stride + start + t of pile
// (G * target_stride cells), its value ((mean + offset) * scale) * fix in float64 rounded to an integer; fit ([n_pairs] {offset, scale,
// used, ok}) is nullable; clear zeroes the arena in front, also with no pairs.
hipError_t launch_levels_pile(uint32_t n_pairs, uint32_t n_reads, uint32_t G, uint32_t target_stride, const uint32_t* target_len, const void* pairs,
                              const void* hit, const uint32_t* n_levels, const void* levels, uint32_t max_width, uint32_t min_samples, uint32_t max_entries,
                              bool require_ok, bool clear, float fix, const void* fit, uint64_t* pile, hipStream_t s);
// launch_squiggle_kmers: row r of kmer ([rows, target_stride] words) = the index of the k-mer launch_squiggle would look up there,
// 0xFFFFFFFF where it would count a masked one and at and behind target_len[r], which is written too.
hipError_t launch_squiggle_kmers(uint32_t k, uint32_t rows, uint32_t seq_stride, uint32_t target_stride, uint32_t flags, const uint8_t* seq,
                                 const uint32_t* seq_len, uint32_t* kmer, uint32_t* target_len, hipStream_t s);
// launch_pile_kmers: the four words of position cell (g, j), j < target_len[g] (untrusted), added to cell kmer[g][j] < 4^k of kmer_pile;
// tables of k <= PILE_KMERS_LDS_KMAX are summed per workgroup in LDS first unless direct.
constexpr uint32_t PILE_KMERS_LDS_KMAX = 6;
hipError_t launch_pile_kmers(uint32_t k, uint32_t rows, uint32_t target_stride, bool clear, bool direct, const uint32_t* target_len, const uint32_t* kmer,
                             const uint64_t* pile, uint64_t* kmer_pile, hipStream_t s);
// launch_model_update: model[i] / sd[i] = mean / sd of k-mer cell i over fix when its count reaches max(min_obs, 1), else prior[i] / +0;
// prior may be model, sd is nullable.
hipError_t launch_model_update(uint32_t k, uint32_t min_obs, float fix, const uint64_t* kmer_pile, const float* prior, float* model, float* sd, hipStream_t s);

// ---- wave / workgroup primitives ---------------------------------------------------------------
// For single-wave workgroups.  The LDS operations of one wave execute in issue order, so lanes of the same
// wave can hand data to each other through LDS without an s_barrier -- and, unlike __syncthreads(), without
// waiting for the wave's outstanding global stores.  This only pins the program order for the compiler.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the wave's outstanding global
// loads AND stores (s_waitcnt vmcnt(0)), which serialises a tile loop on memory latency; the streaming kernels
// only ever exchange data through LDS, so they wait for LDS alone and keep their global accesses in flight.
__device__ __forceinline__ void wg_lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The value of the lane below (lane 0 gets 0): one DPP move (wave_shr:1) instead of an LDS-crossbar shuffle.
__device__ __forceinline__ uint32_t wave_prev_lane_u32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, false);
}

// The value of the lane above (lane 63 gets 0): wave_shl:1.
__device__ __forceinline__ uint32_t wave_next_lane_u32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, false);
}

// Inclusive prefix sum over the 64 lanes of a wave with DPP row shifts and row broadcasts (gfx9: no LDS crossbar
// traffic, six additions): after the four row_shr steps every 16-lane row holds its own scan, row_bcast:15 adds the
// last lane of rows 0 and 2 into rows 1 and 3, row_bcast:31 adds lane 31 into the upper half.
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v)
{
#define VBZ_DPP_ADD(ctrl, rowmask) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rowmask, 0xF, false)
    VBZ_DPP_ADD(0x111, 0xF);  // row_shr:1
    VBZ_DPP_ADD(0x112, 0xF);  // row_shr:2
    VBZ_DPP_ADD(0x114, 0xF);  // row_shr:4
    VBZ_DPP_ADD(0x118, 0xF);  // row_shr:8
    VBZ_DPP_ADD(0x142, 0xA);  // row_bcast:15 -> rows 1, 3
    VBZ_DPP_ADD(0x143, 0xC);  // row_bcast:31 -> rows 2, 3
#undef VBZ_DPP_ADD
    return v;
}

// exclusive scan over a 256-thread workgroup; wsum = 4 words of LDS; returns the exclusive prefix,
// `total` gets the workgroup sum.  Contains two (LDS-only) barriers.
__device__ __forceinline__ uint32_t block_excl_scan_u32(uint32_t v, uint32_t* wsum, uint32_t& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = wave_incl_scan_u32(v);
    if (lane == 63) wsum[w] = inc;
    wg_lds_barrier();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t s = wsum[k];
        base += (k < w) ? s : 0u;
        tot += s;
    }
    wg_lds_barrier();
    total = tot;
    return base + inc - v;
}

}  // namespace vbzhip
