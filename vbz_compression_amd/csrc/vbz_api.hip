// vbz_api.hip -- the C ABI of libvbz_hip.so (include/vbz.h, include/vbz_gpu.h).
//
// Host side of the drop-in boundary.  It mirrors the control flow of the reference's vbz/vbz.cpp
// (option validation, size rules, stage chaining, error codes -- cited per function) and drives the
// HIP kernels; there is no CPU implementation of either stage in this library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <optional>
#include <string>
#include <map>
#include <vector>

#include "../../include/vbz.h"
#include "../../include/vbz_gpu.h"
#include "../../include/vbz_gpu_pile.h"
#include "vbz_kernels.h"
#include "scratch_tables.h"
#include "match_path_groups.h"

using namespace vbzhip;


// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
struct ProfEntry
{
    const char* name;
    uint32_t launches;
    double ms;
};

struct PendingEvent
{
    const char* name;
    hipEvent_t start, stop;
};

// ---- what a context holds: every object is freed by its owner's destructor and never copied (vbz_gpu_destroy deletes the context;
// nothing is released from a list) ---------------------------------------------------------------------------------------------------
template <class H, hipError_t (*Free)(H)>
struct Owned
{
    H p = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { release(); }
    void release()
    {
        if (p) (void)Free(p);
        p = nullptr;
    }
};
typedef Owned<hipStream_t, hipStreamDestroy> OwnedStream;
typedef Owned<hipEvent_t, hipEventDestroy> Event;   // (made without timing: make_event)
static bool make_event(Event& e) { return e.p || hipEventCreateWithFlags(&e.p, hipEventDisableTiming) == hipSuccess; }

template <hipError_t (*Free)(void*)>
struct OwnedBytes : Owned<void*, Free>   // ... of cap bytes
{
    size_t cap = 0;
    void release()
    {
        Owned<void*, Free>::release();
        cap = 0;
    }
};
typedef OwnedBytes<hipFree> DevBuf;   // a device allocation that only grows (ensure)

struct PinnedBuf : OwnedBytes<hipHostFree>   // a block of pinned host memory
{
    bool grow(size_t bytes, unsigned flags)   // (what it held is not kept)
    {
        if (bytes <= cap) return true;
        release();
        if (hipHostMalloc(&p, bytes, flags) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return false;
        }
        cap = bytes;
        return true;
    }
    uint32_t* words() const { return (uint32_t*)p; }
};

struct TimingEvents   // the events of Timed: every one made, and those not in use
{
    std::deque<Event> all;   // (a deque: an owner is not moved)
    std::vector<hipEvent_t> idle;
    hipEvent_t get()
    {
        if (idle.empty()) {
            all.emplace_back();
            (void)hipEventCreate(&all.back().p);
            return all.back().p;
        }
        hipEvent_t e = idle.back();
        idle.pop_back();
        return e;
    }
};

// A second stream with its fork / join events: all three objects or none -- a context never keeps a stream without its events.
// (FastSide is the plain view of them that the launchers take)
struct OwnedSide
{
    OwnedStream stream;
    Event fork, join;
    bool create()
    {
        if (stream.p) return true;
        if (hipStreamCreateWithFlags(&stream.p, hipStreamNonBlocking) == hipSuccess && make_event(fork) && make_event(join)) return true;
        join.release(), fork.release(), stream.release();
        return false;
    }
    FastSide view() const { return { stream.p, fork.p, join.p }; }
};

// A child context (its own stream and buffers, for a launch group that runs beside the parent's) with the events that fork it from the
// parent's stream and join it again: the three are made together or the child is not kept
static hipError_t destroy_child(vbz_gpu_ctx* c)
{
    vbz_gpu_destroy(c);
    return hipSuccess;
}
struct Child
{
    Owned<vbz_gpu_ctx*, destroy_child> ctx;
    Event fork, join;
    bool create(int device)
    {
        if (ctx.p) return true;
        ctx.p = vbz_gpu_create(device, nullptr);
        if (ctx.p && make_event(fork) && make_event(join)) return true;
        join.release(), fork.release(), ctx.release();
        return false;
    }
    operator vbz_gpu_ctx*() const { return ctx.p; }
    vbz_gpu_ctx* operator->() const { return ctx.p; }
};

// The settings of a context: read from the environment by vbz_gpu_create (README.md), three of them set by vbz_gpu_set_trailers /
// _canonical / _checksum.  A child context gets its parent's by assignment before every call it takes part in (inherit_large,
// inherit_half), so a setter reaches the routed reads and the upper halves by being a field here.
struct Knobs
{
    bool routing = true;          // VBZ_HIP_ROUTING=0: by batch shape only
    uint32_t split_min = 16384;   // VBZ_HIP_SPLIT_MIN: batches of this many reads and more are split (0: never)
    // Canonical encoding (vbz_gpu_set_canonical / VBZ_HIP_CANONICAL=1): a read's compressed bytes are a function of the read, the options
    // and the library version -- not of the batch it arrives in (see compress_canonical)
    bool canonical = false;
    bool staged_encode = true;    // VBZ_HIP_STAGED_ENCODE=0: the fused encoder kernel for every read
    bool shared_tables = true;    // VBZ_HIP_SHARED_TABLES=0: large-read path, every span of the data bytes with a table of its own (round 4's frames)
    bool fast_decode = true;      // VBZ_HIP_FAST_DECODE=0: every frame through the one-wavefront decoder
    int ref_chains = 1;           // VBZ_HIP_REF_CHAINS: 0 their sequence chains are walked by the one-wavefront decoder itself, 1 walked ahead of
                                  // it in calls of REF_MIN_READS reads and more, 2 in every call
    bool trailers = true;         // decoder hints (checkpoints, span index) in skippable frames behind the zstd frame
    bool checksum = false;        // vbz_gpu_set_checksum / VBZ_HIP_CHECKSUM=1: frames written with the content checksum (xxh64.hip)
    int segmented = -1;           // -1: by batch shape; 0 / 1: forced (VBZ_HIP_SEGMENTED, for tests)
    uint32_t seg_self_max = SVB_SEG_SELF_MAX;   // VBZ_HIP_SEG_SELF_MAX: large-read path, calls of more segments get scan launches between the svb passes (0: every call)
    bool zero_run_sequences = true;
    bool long_repeats = true;     // VBZ_HIP_LONG_REPEATS=0: no search for a repeat distance
    int phase_timing = 0;         // VBZ_HIP_PHASE_TIMING: 1 phase counters of the entropy kernels (one launch per frame), 2 / 3 of the encoder's planning / packing launch (staged, under load)
    uint64_t match_path_cap = MATCH_PATH_CAP_DEFAULT;   // vbz_gpu_set_match_path_cap / VBZ_HIP_MATCH_PATH_CAP: bytes of direction bits a group of a path call may take
    bool trace = false;           // VBZ_HIP_TRACE=1: synchronise after every launch group and name it on stderr (to find a faulting kernel)
};

// Members are destroyed last to first: the context's own stream is declared first, so everything that may be queued on it goes before it.
struct vbz_gpu_ctx
{
    OwnedStream own_stream;
    hipStream_t stream = nullptr;   // own_stream's, or the caller's (which is left alone)
    int device = 0;
    std::string error;
    Knobs knobs;
    DevBuf scratch;   // intermediate svb streams of a batch
    DevBuf meta;      // the sized headers' tables (SizedTables)
    DevBuf gmeta;     // per-read bookkeeping arrays of one launch group (StageSlots)
    DevBuf route;     // per-read routing: the first group's gates, the second group's compact descriptors (RouteTables; CanonGates)
    Child large;      // per-read routing: the second group's own stream and buffers (it runs beside the first group)
    // A large batch on the one-workgroup path is coded as TWO HALVES on two streams (split_batch): the upper half on this child context
    Child half;
    DevBuf splitmeta;          // the scratch plan of the whole batch (slot offsets, capacities, gates), shared by the two halves (SplitTables)
    bool last_split = false;      // vbz_gpu_decode_paths: the last decompress call ran as halves
    // Frames of OTHER writers (every vbz file in existence: the reference's libzstd frames) decode on one wavefront each behind a chain walk
    // of fixed latency, and two halves of such a call do not run beside each other (482 GB/s as one group, 420 as halves); the host
    // does not know whose frames a call holds.  Every decompress call leaves the number of frames the batched decoder did not take in
    // pinned memory (a counting launch and a 4-byte copy behind the call, no wait); the NEXT call looks at it if it has arrived and runs
    // as one group when most frames were foreign.  A matter of speed only: the decoded bytes do not depend on it.
    PinnedBuf foreign_host;   // [frames left to the one-wavefront decoder, frames looked at]
    DevBuf foreign_dev;
    Event ev_foreign;
    bool foreign_pending = false, mostly_foreign = false;
    int foreign_state = -1;   // what the last call that was looked at held: -1 not known, 0 no foreign frame at all, 1 some
    PinnedBuf canon_host;     // canonical encoding: the classification's count comes back here
    // single-buffer API staging
    DevBuf one_in, one_out;
    DevBuf dbg;       // per-read phase timers (VBZ_HIP_PHASE_TIMING=1)
    DevBuf seqtab;    // encoding tables of the predefined sequence distributions
    DevBuf seqdtab;   // decoding tables of the same distributions
    DevBuf segmeta;   // segment / span tables of the large-read path (SegTables)
    DevBuf spanmeta, spantmp;  // span tables and temporary slots of the entropy stage in the large-read path
    DevBuf vgate;     // verdicts on the caller's descriptor table (one word per read)
    DevBuf encplan;   // per-read plans of the staged encoder (tables of both regions: zstd_encode.hip STAGE 1 / 2)
    DevBuf fastmeta;  // per-frame descriptors, stream tasks and weights of the batched own-frame decoder (zstd_decode_fast.hip)
    DevBuf refpre, reftab, refrecs;  // frames the reference wrote: per-frame hand-over, tables (large batches), records (zstd_decode_ref.hip)
    DevBuf reflits;                  // ... their literals decoded beside the walk (zstd_decode_fast.hip: ref_pieces_kernel)
    uint32_t last_lit_units = 0;     // (records per read the last call filled)
    OwnedSide side;            // the walk's own stream (beside the launches for this library's frames)
    bool last_walked = false;
    uint32_t last_frames = 0;  // vbz_gpu_decode_paths: the frames of the last zstd_frames call (0: none, or not on the batched path)
    uint32_t last_span_frames = 0;          // ... of the last call on the large-read path, and its redo[] (in spanmeta)
    const uint32_t* last_span_redo = nullptr;
    DevBuf cksum;              // the hashes of a compress launch group (8 bytes per read)
    DevBuf sigmeta;            // typed decode: the int16 slot table and the per-read constants (TypedSlots), or the constants alone
    DevBuf chunkmeta;          // chunk layout: the per-read chunk counts
    DevBuf winmeta;            // signal windows: the per-read row counts and their scan (WindowScratch)
    DevBuf evmeta;             // signal events: the rows' moments of a call whose caller takes none (two 64-bit words a row)
    DevBuf segmtab;            // signal segmentation: the per-read tables of a call (SegmentScratch)
    DevBuf segmap;             // ... and the reads' boundary maps, one bit a sample (1/16 of the int16 arena the call never writes)
    DevBuf normmeta;           // normalising decode: the per-read NormRead states of a call (NormTables)
    DevBuf normslab;           // ... and, on the large-read path, the counts of a launch group (NORM_SLAB words per read)
    DevBuf pod5meta;           // a call over POD5 reads: the rows' and the reads' tables, the reads' constants (Pod5Tables)
    DevBuf matchmeta;          // signal match: the fused calls' own window tables, valid[] and, for a caller that takes none, read_result (MatchTables)
    DevBuf matchpath;          // the path call: one group's direction bits and costs (MatchPathScratch)
    DevBuf squigpart;          // the squiggle call: the masked counts of one call's wavefronts (squiggle_part_words)
    bool profiling = false;    // (not a setting: outside Knobs; the upper half of a split call gets the call's)
    PinnedBuf pinned;          // the single-buffer API's pinned area (run_one)
    uint32_t one_seq = 0;      // the single-buffer API's hand-back flag: a number per call (run_one)
    std::vector<PendingEvent> pending;
    std::vector<ProfEntry> prof;
    TimingEvents events;
};

namespace {

void set_error(vbz_gpu_ctx* c, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->error = buf;
    fprintf(stderr, "vbz_hip: %s\n", buf);
}

bool ensure(vbz_gpu_ctx* c, DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return true;
    if (b.p) {
        (void)hipStreamSynchronize(c->stream);  // earlier work may still use the old buffer
        b.release();
    }
    size_t want = bytes + bytes / 8 + 4096;
    hipError_t e = bytes > ((size_t)1 << 60) ? hipErrorOutOfMemory : hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        set_error(c, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        (void)hipGetLastError();   // (the runtime keeps the failure as the thread's last error: the caller's next HIP call must not trip over it)
        b.p = nullptr;
        return false;
    }
    b.cap = want;
    return true;
}

// A table of scratch_tables.h in a buffer: the table's carve measures, the buffer grows to that, the same carve places the arrays
template <class T, class... D>
bool ensure_carved(vbz_gpu_ctx* c, DevBuf& b, T& t, D... dims)
{
    if (!ensure(c, b, t.carve(nullptr, dims...))) return false;
    t.carve(b.p, dims...);
    return true;
}
// ... and one array of n elements (nullptr: no memory)
template <class T>
T* ensure_array(vbz_gpu_ctx* c, DevBuf& b, size_t n)
{
    return ensure(c, b, array_bytes<T>(n)) ? reinterpret_cast<T*>(b.p) : nullptr;
}

struct Timed  // records a pair of events around one kernel launch when profiling is on
{
    vbz_gpu_ctx* c;
    const char* name;
    hipEvent_t start = nullptr;
    Timed(vbz_gpu_ctx* ctx, const char* n) : c(ctx), name(n)
    {
        if (c->profiling) {
            start = c->events.get();
            (void)hipEventRecord(start, c->stream);
        }
    }
    ~Timed()
    {
        if (c->knobs.trace) {
            const hipError_t e = hipStreamSynchronize(c->stream);
            fprintf(stderr, "vbz_hip trace: %s %s\n", name, e == hipSuccess ? "ok" : hipGetErrorString(e));
        }
        if (start) {
            hipEvent_t stop = c->events.get();
            (void)hipEventRecord(stop, c->stream);
            c->pending.push_back({ name, start, stop });
        }
    }
};

void drain_profile(vbz_gpu_ctx* c)
{
    if (c->pending.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    for (auto& p : c->pending) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, p.start, p.stop);
        bool found = false;
        for (auto& e : c->prof)
            if (e.name == p.name || strcmp(e.name, p.name) == 0) {
                e.launches++;
                e.ms += ms;
                found = true;
                break;
            }
        if (!found) c->prof.push_back({ p.name, 1, (double)ms });
        c->events.idle.push_back(p.start);
        c->events.idle.push_back(p.stop);
    }
    c->pending.clear();
}

// debug aid: per-phase shader-clock cycles of the entropy kernels, averaged over the batch, on stderr
// per_role: the counters of the encoder's planning launch (VBZ_HIP_PHASE_TIMING=2), two wavefronts per read
unsigned long long* dbg_begin(vbz_gpu_ctx* c, uint32_t n, bool per_role = false)
{
    if (!c->knobs.phase_timing) return nullptr;
    if (per_role) n *= 2;
    unsigned long long* d = ensure_array<unsigned long long>(c, c->dbg, (size_t)n * PHASE_SLOTS);
    if (d) (void)hipMemsetAsync(d, 0, (size_t)n * PHASE_SLOTS * 8, c->stream);
    return d;
}

// VBZ_HIP_PHASE_TIMING=2: the planning launch's counters, two per read (one per role), averaged per role over the wavefronts that planned
void dbg_end_roles(vbz_gpu_ctx* c, uint32_t n, const char* what, unsigned long long* d)
{
    std::vector<unsigned long long> h((size_t)n * PHASE_SLOTS);
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(h.data(), d, (size_t)n * PHASE_SLOTS * 8, hipMemcpyDeviceToHost);
    for (uint32_t role = 0; role < 2; ++role) {
        double sum[PHASE_SLOTS] = {};
        uint32_t m = 0;
        for (uint32_t i = role; i < n; i += 2) {
            unsigned long long t = 0;
            for (int k = 0; k < PHASE_SLOTS; ++k) t += h[(size_t)i * PHASE_SLOTS + k];
            if (!t) continue;
            ++m;
            for (int k = 0; k < PHASE_SLOTS; ++k) sum[k] += (double)h[(size_t)i * PHASE_SLOTS + k];
        }
        fprintf(stderr, "vbz_hip phase cycles/read (%s, role %u, n=%u):", what, role, m);
        for (int k = 0; k < PHASE_SLOTS; ++k) fprintf(stderr, " p%d=%.0f", k, m ? sum[k] / m : 0.0);
        fprintf(stderr, "\n");
    }
}

void dbg_end(vbz_gpu_ctx* c, uint32_t n, const char* what, unsigned long long* d, bool per_role = false)
{
    if (!d) return;
    if (per_role) return dbg_end_roles(c, 2 * n, what, d);
    std::vector<unsigned long long> h((size_t)n * PHASE_SLOTS);
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(h.data(), d, (size_t)n * PHASE_SLOTS * 8, hipMemcpyDeviceToHost);
    double sum[PHASE_SLOTS] = {};
    for (uint32_t i = 0; i < n; ++i)
        for (int k = 0; k < PHASE_SLOTS; ++k) sum[k] += (double)h[(size_t)i * PHASE_SLOTS + k];
    fprintf(stderr, "vbz_hip phase cycles/read (%s, n=%u):", what, n);
    for (int k = 0; k < PHASE_SLOTS; ++k) fprintf(stderr, " p%d=%.0f", k, sum[k] / n);
    fprintf(stderr, "\n");
}

// v1 codes 1-byte integers with the nibble codec (vbz/v1/vbz_streamvbyte.cpp:22-113)
bool half_codec(const CompressionOptions* o) { return o->vbz_version == 1 && o->integer_size == 1; }

// POD5 signal rows (VBZ_GPU_VERSION_POD5): svb16 + one zstd frame, int16 zig-zag samples, no sized header, level >= 1
bool pod5_codec(const CompressionOptions* o) { return o->vbz_version == VBZ_GPU_VERSION_POD5; }

bool valid_int_size(const CompressionOptions* o)  // vbz/vbz.cpp:44-50
{
    return o->integer_size == 0 || o->integer_size == 1 || o->integer_size == 2 || o->integer_size == 4;
}

// the options of the batched calls: the reference's (versions 0 and 1), or POD5 rows with their one layout
bool batch_options_ok(const CompressionOptions* o, int sized)
{
    if (pod5_codec(o)) return o->integer_size == 2 && o->perform_delta_zig_zag && o->zstd_compression_level >= 1 && sized == 0;
    return valid_int_size(o) && (o->integer_size == 0 || o->vbz_version <= 1);
}

// worst-case svb bytes per raw byte as a fraction, for what the device encoder can really emit
void svb_factor(unsigned integer_size, bool zigzag, uint32_t* num, uint32_t* den)
{
    if (integer_size == 2 && zigzag) { *num = 9; *den = 8; }     // keys n/4 + 2 bytes per value
    else if (integer_size == 1) { *num = 17; *den = 4; }         // keys n/4 + 4 bytes per value
    else if (integer_size == 2) { *num = 17; *den = 8; }
    else { *num = 17; *den = 16; }
}

size_t zstd_bound(size_t n)  // published ZSTD_COMPRESSBOUND (zstd.h), what vbz/vbz.cpp:109 calls
{
    return n + (n >> 8) + (n < (128u << 10) ? (((128u << 10) - n) >> 11) : 0);
}

// The entry points run on the context's device and leave the caller's current device as they found it (a process
// that drives several GPUs from one thread must not have its later allocations land on another device).
struct DeviceGuard
{
    int saved = -1;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&saved) != hipSuccess) saved = -1;
        if (saved != device) (void)hipSetDevice(device);
        else saved = -1;
    }
    ~DeviceGuard()
    {
        if (saved >= 0) (void)hipSetDevice(saved);
    }
};

#define HIPCHK(c, expr, what)                                                      \
    do {                                                                           \
        hipError_t e__ = (expr);                                                   \
        if (e__ != hipSuccess) {                                                   \
            set_error((c), "%s failed: %s", (what), hipGetErrorString(e__));      \
            (void)hipGetLastError(); /* reported here: not left for the caller's next HIP call to trip over */ \
            return -1;                                                             \
        }                                                                          \
    } while (0)

// One read per workgroup (svb) / per wavefront (entropy stage) fills the GPU when a batch has thousands of reads.  A batch of
// few, large reads (BASELINE configs[0] and [3]: one 400 k-sample read, one 10 M-element buffer; the HDF5 filter's one chunk
// per call) takes the segmented kernels instead: every read is spread over many workgroups.  The rule looks at the batch
// shape only (the sizes themselves live on the device): average read of half a megabyte or more.
constexpr uint64_t SEGMENTED_MIN_AVG = 512u << 10;
// ... and batches too small to fill the device with one wavefront per read: a call with one read of 100 k samples (the
// single-buffer API, the HDF5 filter) takes 0.39 / 0.25 ms on one wavefront and 0.16 / 0.16 ms as spans (tools/time_one_read.py),
// whatever the read's length; the one-wavefront kernels win from a few thousand reads per call on, or when the reads are
// so short that a read is hardly more than one span.
constexpr uint64_t SMALL_BATCH_MIN_AVG = 64u << 10, SMALL_BATCH_MAX_BYTES = 96u << 20;
// Decoding a handful of short reads -- a chunk per call through the HDF5 filter -- is a chain of nine launches on the one-wavefront
// path (scan, weights, streams, runs, the gated second attempt, ...: 0.17 - 0.23 ms for 1 - 64 reads of 5 - 10 k samples) and six with
// spans (0.13 - 0.19 ms, tools/time_small_batch.py); encoding such reads is faster on one wavefront each (0.11 - 0.13 against 0.12 - 0.20 ms).
constexpr uint64_t TINY_DECODE_MIN_AVG = 8u << 10;
constexpr uint32_t TINY_DECODE_MAX_READS = 64;

// The context's second stream (the chain walk beside the launches for own frames; the shared-table spans beside the control-byte spans)
bool ensure_side(vbz_gpu_ctx* c)
{
    if (c->side.create()) return true;
    set_error(c, "second stream: %s", hipGetErrorString(hipGetLastError()));
    return false;
}

bool use_segments(const vbz_gpu_ctx* c, uint64_t raw_arena_bytes, uint32_t n, bool decode)
{
    if (c->knobs.segmented >= 0) return c->knobs.segmented != 0;
    const uint64_t avg = raw_arena_bytes / n;
    return avg >= SEGMENTED_MIN_AVG || (avg >= SMALL_BATCH_MIN_AVG && raw_arena_bytes <= SMALL_BATCH_MAX_BYTES) ||
           (decode && n <= TINY_DECODE_MAX_READS && avg >= TINY_DECODE_MIN_AVG);
}

// segment tables for a batch whose raw bytes span `raw_arena_bytes`; sizes (device) are the reads' raw byte counts
// scratch (nullable): the group's scratch plan in the same launch (calls of up to 1024 reads: *scratch_done says whether it was)
int plan_segments(vbz_gpu_ctx* c, uint32_t n, const uint32_t* raw_size, const uint32_t* gate, uint64_t raw_arena_bytes, uint32_t unit, SegTables* t,
                  const ScratchPlan* scratch = nullptr, bool* scratch_done = nullptr)
{
    const uint64_t segs = raw_arena_bytes / unit + n + 1;
    if (segs > 0x7FFFFFFFull) {
        set_error(c, "batch too large for the segmented path");
        return -1;
    }
    if (!ensure_carved(c, c->segmeta, *t, n, (uint32_t)segs)) return -1;
    Timed tm(c, "seg_plan");
    HIPCHK(c, launch_seg_plan(n, raw_size, unit, gate, t->max_segs, t->first, t->gate, scratch, c->stream), "seg_plan launch");
    if (scratch_done) *scratch_done = scratch != nullptr && n <= 1024;
    return 0;
}

ReadBatch to_rb(const vbz_gpu_batch* bt)
{
    ReadBatch rb;
    rb.n_reads = bt->n_reads;
    rb.src = (const uint8_t*)bt->src;
    rb.src_off = bt->src_off;
    rb.src_size = bt->src_size;
    rb.dst = (uint8_t*)bt->dst;
    rb.dst_off = bt->dst_off;
    rb.dst_cap = bt->dst_cap;
    rb.result = bt->result;
    rb.gate = nullptr;
    return rb;
}

// The scratch plan of a batch made ONCE for both halves of a split call (split_batch): the group then takes its slots from here
// instead of planning its own, and its scratch is the planning context's.
struct Preplanned
{
    void* scratch = nullptr;
    uint64_t* svb_off = nullptr;
    uint32_t *svb_cap = nullptr, *gate = nullptr;
    uint32_t* svb_size = nullptr;   // (nullable) where the halves leave their streams' sizes: one table for a stage behind the join
};

// The content checksum of the frames of an entropy stage (vbz_gpu_set_checksum), in two launches of its own around the stage, whatever
// path writes the frames.  z = that stage's batch (src: the frames' content, dst / result: the frames), gate: the group's (nullable).
// checksum_content runs IN FRONT of the stage: the staged encoder rewrites the control bytes of an svb stream in its scratch slot in place.
int checksum_content(vbz_gpu_ctx* c, const ReadBatch& z, const uint32_t* gate)
{
    if (!c->knobs.checksum || z.n_reads == 0) return 0;
    uint64_t* const hashes = ensure_array<uint64_t>(c, c->cksum, z.n_reads);
    if (!hashes) return -1;
    Timed t(c, "checksum");
    HIPCHK(c, launch_xxh64_batch(z.src, z.src_off, z.src_size, gate, nullptr, z.n_reads, hashes, c->stream), "xxh64 launch");
    return 0;
}
// ... and behind it: the frames get the flag and the checksum.  raw_size (nullable) + integer_size: what bounds the result.
int checksum_frames(vbz_gpu_ctx* c, const ReadBatch& z, const uint32_t* gate, uint32_t hdr, const uint32_t* raw_size, uint32_t integer_size)
{
    if (!c->knobs.checksum || z.n_reads == 0) return 0;
    Timed t(c, "checksum");
    ReadBatch w = z;
    w.gate = gate;
    HIPCHK(c, launch_checksum_insert(w, reinterpret_cast<const uint64_t*>(c->cksum.p), hdr, raw_size, integer_size, c->stream), "checksum insert launch");
    return 0;
}

// A decode's zstd stage is done (z: frames, their content and its sizes): frames that carry a content checksum are held to it.  One short
// launch that looks at one byte of every frame without the flag.
int verify_checksums(vbz_gpu_ctx* c, const ReadBatch& z)
{
    Timed t(c, "checksum_verify");
    HIPCHK(c, launch_xxh64_verify(z, c->stream), "checksum verify launch");
    return 0;
}

// What both kinds of launch group start with: the per-read arrays, on the large-read path the segment tables, and for both stages the
// scratch that holds the svb streams between them -- its slots planned with the segments when they can be (two launches less for a call
// of few reads), adopted from a split call's Preplanned, or left to launch_stage_plan.
struct StagePlan
{
    StageSlots m;
    SegTables seg;
    bool both_stages = false, planned = false;
    uint32_t num = 1, den = 1;   // svb_factor
    size_t scratch_need = 0;
    void* scratch_base = nullptr;
};
// sizes / arena_bytes: the reads' raw byte counts and their extent -- src_size / src_bytes of a compress group, dst_cap / dst_bytes of a
// decompress group.  zigzag: whether svb_factor may count on it (a decode passes false: any code length may appear in a foreign stream).
int plan_stage_scratch(vbz_gpu_ctx* c, const ReadBatch& rb, const uint32_t* sizes, uint64_t arena_bytes, const CompressionOptions* o, bool zigzag,
                       bool segmented, const Preplanned* pre, StagePlan* p)
{
    const uint32_t n = rb.n_reads;
    // svb into scratch, then the entropy stage into dst (vbz.cpp:163-207), or the entropy stage into scratch (sized for the largest svb
    // stream the expected output can have), then svb decode into dst (vbz.cpp:234-299)
    p->both_stages = o->integer_size != 0 && o->zstd_compression_level != 0;
    if (p->both_stages) {
        svb_factor(o->integer_size, zigzag, &p->num, &p->den);
        p->scratch_need = (size_t)(((unsigned __int128)arena_bytes * p->num + p->den - 1) / p->den) + (size_t)n * 96 + 256;
        if (!pre && !ensure(c, c->scratch, p->scratch_need)) return -1;
    }
    if (!ensure_carved(c, c->gmeta, p->m, n)) return -1;
    p->scratch_base = pre ? pre->scratch : c->scratch.p;
    if (pre) {   // (both stages, one-workgroup path: what split_batch asks for) -- slots and gates planned once for the whole batch
        p->m.svb_off = pre->svb_off;
        p->m.svb_cap = pre->svb_cap;
        p->m.gate = pre->gate;
        if (pre->svb_size) p->m.svb_size = pre->svb_size;
        p->planned = true;
    }
    const ScratchPlan splan = { p->num, p->den, c->scratch.cap, p->m.svb_off, p->m.svb_cap, p->m.gate };
    if (segmented && plan_segments(c, n, sizes, pre ? pre->gate : rb.gate, arena_bytes, svb_seg_unit_bytes((int)o->integer_size), &p->seg,
                                   p->both_stages ? &splan : nullptr, &p->planned) != 0)
        return -1;
    return 0;
}

// Both stages, slots not planned yet: the plan's own launch.  gate_src (nullable): the gate the reads come with (the caller's; on the
// large-read path the segments', E_OOM for a read whose segments do not fit the tables) -- copied, the plan adds its own E_OOM.
int launch_stage_plan(vbz_gpu_ctx* c, uint32_t n, const uint32_t* sizes, const uint32_t* gate_src, const StagePlan& p)
{
    if (p.planned) return 0;
    if (gate_src) HIPCHK(c, hipMemcpyAsync(p.m.gate, gate_src, 4ull * n, hipMemcpyDeviceToDevice, c->stream), "gate copy");
    Timed t(c, "plan_scratch");
    HIPCHK(c, launch_plan_scratch(n, sizes, p.num, p.den, c->scratch.cap, p.m.svb_off, p.m.svb_cap, p.m.gate, gate_src != nullptr, c->stream), "plan launch");
    return 0;
}

// VBZ_HIP_PHASE_TIMING on the one-wavefront encoder: whose launch gets the phase counters, whether the encoder is staged under them, and
// what dbg_end prints.  1: the whole frame in one launch (never staged); 2: the planning launch's counters (two per read, one per role),
// 3: the packing launch's -- both under load, the other launches as they are.  The large-read path has no counters.
struct EncodeTiming
{
    bool staged = false, per_role = false;
    unsigned long long* counters = nullptr;
    EncDebug dbg;
    const char* label = "";
};
EncodeTiming encode_timing(vbz_gpu_ctx* c, uint32_t n, bool segmented)
{
    EncodeTiming t;
    const int pt = segmented ? 0 : c->knobs.phase_timing;
    t.per_role = pt == 2;
    t.counters = pt ? dbg_begin(c, n, t.per_role) : nullptr;
    t.staged = !segmented && c->knobs.staged_encode && (!t.counters || pt == 2 || pt == 3) && c->knobs.zero_run_sequences;
    (pt == 2 ? t.dbg.plan : pt == 3 ? t.dbg.pack : t.dbg.frame) = t.counters;
    t.label = pt == 3   ? "zstd_pack: setup region lookups+scan bits quads ends+headers sequences trailer"
              : pt == 2 ? "zstd_plan: setup tokeniser sequences hist store rest | sort merge leaves lengths codes+weights tree"
                        : "zstd_encode: setup hist plan size hdr encode";
    return t;
}

// The entropy stage of a compress group on the large-read path (few, large reads): one wavefront per span of a stream, then compaction.
// z: the svb streams in scratch -> the frames; a: key, hdr (runs and trailers are the context's).
int entropy_encode_spans(vbz_gpu_ctx* c, ReadBatch z, ZstdEncodeArgs a, const CompressionOptions* o, const StagePlan& p)
{
    const uint32_t n = z.n_reads;
    hipStream_t s = c->stream;
    SpanEncodeWork w;
    w.stream_bytes = p.scratch_need;
    // Shared tables (zstd_encode.hip, SpanRegion): the data bytes of a read get ONE table, built beside the control-byte spans, and are
    // packed in spans of 8 KB by a launch of their own.  For calls that are a matter of latency (zstd_span_shared_bytes) and for 8 / 16-bit
    // elements, whose control bytes are mostly zero and cheap to code: 0.176 -> 0.140 ms per call for a 100 k-sample read.  The
    // control-byte spans of 32-bit elements take as long as the table construction itself (a 40 MB buffer: 100 us in the first launch,
    // + 15 us counting + 34 us packing against 125 us for everything in one launch) -- they keep a table per span.
    // (canonical mode: whether the data bytes share a table must not follow from the call's size -- every span its own table)
    w.shared_span_bytes = (c->knobs.shared_tables && !c->knobs.canonical && (o->integer_size == 1 || o->integer_size == 2)) ? zstd_span_shared_bytes(p.scratch_need) : 0u;
    const size_t meta_bytes = zstd_span_meta_bytes(p.scratch_need, n, w.shared_span_bytes);
    if (!meta_bytes) {
        set_error(c, "batch too large for the span path");
        return -1;
    }
    if (!ensure(c, c->spantmp, zstd_span_tmp_bytes(p.scratch_need, n)) || !ensure(c, c->spanmeta, meta_bytes)) return -1;
    w.meta = c->spanmeta.p;
    w.tmp = (uint8_t*)c->spantmp.p;
    a.runs = { p.m.svb_cap, c->seqtab.p };
    a.trailers = c->knobs.trailers;
    z.gate = p.m.gate;
    if (c->knobs.zero_run_sequences && c->knobs.long_repeats && o->integer_size != 0) {
        // reads that repeat at one distance go to the one-wavefront matcher after all, whatever their length: a read that
        // cycles a template (the reference's own perf generator: vbz/perf/test_data_generator.h:61-67) is 15-30 x smaller as
        // matches than as spans of Huffman blocks, which is worth one wavefront's time on it (libzstd, the reference's
        // coder, finds those matches at every level and every length: vbz/vbz.cpp:194-207).  The probe looks at the head of
        // a long read's data bytes only (PROBE_WINDOW in zstd_encode.hip): two short launches for a read that has no period.
        a.deep_d = p.m.deep_d;
        Timed t(c, "zstd_encode_matcher");
        HIPCHK(c, launch_zstd_encode_matcher(z, a, 0xFFFFFFFFu, p.m.gate, p.m.gate2, s), "zstd_encode (matcher) launch");
        z.gate = p.m.gate2;
    }
    if (!c->knobs.zero_run_sequences) a.runs = ZeroRuns();
    Timed t(c, "zstd_encode");
    HIPCHK(c, launch_zstd_encode_spans(z, a, w, s), "zstd_encode (spans) launch");
    return 0;
}

// ... and on the one-workgroup path: one wavefront per read, staged (the per-read plans, in which the svb encoder has left the data
// bytes' histogram of int16 zig-zag reads when pre_filled: svb_kernels.hip CNT) or in one launch; the long-repeat matcher behind it.
int entropy_encode_reads(vbz_gpu_ctx* c, const ReadBatch& z, ZstdEncodeArgs a, const StagePlan& p, const EncodeTiming& tm, bool matcher)
{
    {
        Timed t(c, "zstd_encode");
        if (c->knobs.zero_run_sequences) a.runs = { p.m.svb_cap, c->seqtab.p };
        a.trailers = c->knobs.trailers;
        a.deep_d = (matcher && !tm.counters) ? p.m.deep_d : nullptr;
        a.staged = tm.staged;
        a.dbg = tm.dbg;
        HIPCHK(c, launch_zstd_encode(z, a, c->stream), "zstd_encode launch");
    }
    dbg_end(c, z.n_reads, tm.label, tm.counters, tm.per_role);
    return 0;
}

// One launch group of a compress call: the reads of rb_in (those whose gate is closed left alone), on the one-workgroup path or
// on the large-read path.  src_bytes: extent of the raw bytes of the group's reads.
int compress_group(vbz_gpu_ctx* c, const ReadBatch& rb_in, uint64_t src_bytes, const CompressionOptions* o, int sized, bool segmented,
                   const Preplanned* pre = nullptr)
{
    const uint32_t n = rb_in.n_reads;
    if (n == 0) return 0;
    const uint32_t hdr = sized ? 4u : 0u;
    hipStream_t s = c->stream;
    ReadBatch rb = rb_in;
    if (o->integer_size == 0 && o->zstd_compression_level == 0) {  // vbz.cpp:130-133
        Timed t(c, "copy_bytes");
        HIPCHK(c, launch_copy_bytes(rb, hdr, s), "copy launch");
        return 0;
    }
    StagePlan p;
    if (plan_stage_scratch(c, rb, rb.src_size, src_bytes, o, o->perform_delta_zig_zag, segmented, pre, &p) != 0) return -1;
    const SegTables& seg = p.seg;
    if (segmented) rb.gate = seg.gate;   // (E_OOM for a read whose segments do not fit the tables)
    if (o->zstd_compression_level == 0) {  // vbz.cpp:171-192: svb straight into dst
        Timed t(c, "svb_encode");
        if (segmented)
            HIPCHK(c, launch_svb_encode_seg(rb, (int)o->integer_size, o->perform_delta_zig_zag, hdr, true, seg.first, seg.max_segs, seg.val, seg.off, c->knobs.seg_self_max, s),
                   "svb_encode (segmented) launch");
        else
            HIPCHK(c, launch_svb_encode(rb, (int)o->integer_size, o->perform_delta_zig_zag, hdr, true, half_codec(o), nullptr, nullptr, s), "svb_encode launch");
        return 0;
    }
    ZstdEncodeArgs za;
    za.key.orig_size = rb.src_size;
    za.hdr = hdr;
    if (o->integer_size == 0) {  // zstd only
        if (checksum_content(c, rb, rb.gate) != 0) return -1;
        {
            Timed t(c, "zstd_encode");
            za.trailers = c->knobs.trailers;
            HIPCHK(c, launch_zstd_encode(rb, za, s), "zstd_encode launch");
        }
        return checksum_frames(c, rb, rb.gate, hdr, rb.src_size, 0);
    }
    // the long-repeat matcher (every level: the reference's libzstd matches at every level; its workspace is the top of the
    // destination slots)
    const bool matcher = !segmented && c->knobs.zero_run_sequences && c->knobs.long_repeats;
    if (launch_stage_plan(c, n, rb.src_size, pre ? nullptr : rb.gate, p) != 0) return -1;
    const EncodeTiming tm = encode_timing(c, n, segmented);
    const bool pod5 = pod5_codec(o);
    za.pre_filled = tm.staged && !pod5 && svb_encode_fills_plans((int)o->integer_size, o->perform_delta_zig_zag, half_codec(o));
    if (tm.staged) {
        if (!ensure(c, c->encplan, zstd_encode_plan_bytes(n))) return -1;
        za.plan_meta = c->encplan.p;
    }
    // the entropy stage's key region: ceil(n / 4) bytes of the raw size at integer_size, or svb16's ceil(n / 8) through key_raw (POD5)
    za.key.key_elem = o->integer_size;
    if (pod5) {
        HIPCHK(c, launch_svb16_key_raw(n, rb.src_size, p.m.key_raw, s), "svb16 key launch");
        za.key.orig_size = p.m.key_raw;
        za.key.key_elem = SVB16_KEY_ELEM;
    }
    ReadBatch a = rb;   // the svb stage: the reads -> their streams in scratch
    a.dst = (uint8_t*)p.scratch_base;
    a.dst_off = p.m.svb_off;
    a.dst_cap = p.m.svb_cap;
    a.result = p.m.svb_size;
    a.gate = p.m.gate;
    {
        Timed t(c, "svb_encode");
        if (pod5)   // (one workgroup per read on every path: DESIGN.md 4.13)
            HIPCHK(c, launch_svb16_encode(a, matcher ? p.m.deep_d : nullptr, s), "svb16_encode launch");
        else if (segmented)
            HIPCHK(c, launch_svb_encode_seg(a, (int)o->integer_size, o->perform_delta_zig_zag, 0, false, seg.first, seg.max_segs, seg.val, seg.off, c->knobs.seg_self_max, s),
                   "svb_encode (segmented) launch");
        else
            HIPCHK(c, launch_svb_encode(a, (int)o->integer_size, o->perform_delta_zig_zag, 0, false, half_codec(o), matcher ? p.m.deep_d : nullptr,
                                        za.pre_filled ? za.plan_meta : nullptr, s),
                   "svb_encode launch");
    }
    ReadBatch z = rb;   // the entropy stage: the streams -> the frames
    z.src = (const uint8_t*)p.scratch_base;
    z.src_off = p.m.svb_off;
    z.src_size = p.m.svb_size;
    if (checksum_content(c, z, p.m.gate) != 0) return -1;
    if ((segmented ? entropy_encode_spans(c, z, za, o, p) : entropy_encode_reads(c, z, za, p, tm, matcher)) != 0) return -1;
    return checksum_frames(c, z, p.m.gate, hdr, pod5 ? nullptr : rb.src_size, o->integer_size);
}

constexpr uint32_t REF_MIN_READS = 2560;   // calls of fewer reads: the one-wavefront decoder walks reference-written chains itself

// The frames of a launch group on the one-workgroup path (not the large-read path): frames of this library's shape on the batched
// decoder, the sequence chains of frames the reference wrote walked one lane per frame, everything else -- and every error verdict --
// from the one-wavefront decoder.  content_bytes bounds the frames' content in all.
// (decompress_split passes the WHOLE call's dst_bytes for each half: avg_content doubles and refrecs is sized for the call twice -- ADVICE.md)
int zstd_frames(vbz_gpu_ctx* c, const ReadBatch& z, uint32_t toosmall_code, uint64_t content_bytes, unsigned long long* dbg)
{
    const uint32_t n = z.n_reads;
    hipStream_t s = c->stream;
    Timed t(c, "zstd_decode");
    c->last_frames = 0;
    if (!c->knobs.fast_decode) {
        HIPCHK(c, launch_zstd_decode(z, toosmall_code, dbg, c->seqdtab.p, s), "zstd_decode launch");
        return 0;
    }
    if (!ensure(c, c->fastmeta, zstd_fast_meta_bytes(n))) return -1;
    // Frames the reference wrote: their chains are walked ahead of the one-wavefront decoder when the call is large enough for that to
    // pay (the walk is a launch of its own whose duration is one chain's latency, ~0.7 ms: measured break-even 2 500 such frames).
    // Records of walked chains: 16 bytes per sequence, claimed from one workspace of the call as the lanes go (an atomic counter; a frame
    // that finds no room is decoded as before).  libzstd on nanopore signal writes ~1 100 sequences per 126 KB of content -- records of
    // 14 % of the content's size --: the workspace is a quarter of the declared content + 1 MiB, at most 1 GiB (the declared size
    // is the caller's word, and the buffer stays with the context: ADVICE round 4; 16 384 reads of 100 k samples need 290 MB).
    // (a workload that has shown no foreign frame does not launch the walk at all: the -- empty -- launch sits on a side stream, gets its
    // few wavefronts late when the device is full, and the launches behind the join wait for it; should foreign frames appear after all,
    // the one-wavefront decoder walks their chains itself for one call and the next call knows)
    const bool walk = (c->knobs.ref_chains >= 2 || (c->knobs.ref_chains == 1 && n >= REF_MIN_READS)) && (c->foreign_state != 0 || c->knobs.ref_chains >= 2);
    const uint64_t recs_bytes = walk ? std::min<uint64_t>(((content_bytes >> 2) + (1ull << 20)) & ~15ull, 1ull << 30) : 0;
    if (walk && (!ensure(c, c->refpre, zstd_ref_pre_bytes(n)) || !ensure(c, c->reftab, zstd_ref_table_bytes(n)) || !ensure(c, c->refrecs, recs_bytes)))
        return -1;
    if (walk && !dbg && !ensure_side(c)) return -1;
    const bool lits = walk && zstd_ref_literals_enabled();
    if (lits && !ensure(c, c->reflits, zstd_ref_lit_meta_bytes(n))) return -1;
    // (blocks per frame that get a record and a workgroup of the pieces' kernel: a call of short reads has one block a frame -- three of four
    // workgroups of a grid for four would start only to end, 0.3 ms per 16 384 frames --, a call of long reads two or three of 128 KB and a rest)
    const uint64_t avg_content = content_bytes / n;
    // (content_bytes is the caller's bound: the decoded bytes of the call, 1.6 x the frames' content where an svb stage follows)
    const uint32_t lit_units = avg_content <= (96u << 10) ? 1u : (uint32_t)std::min<uint64_t>(avg_content / (256u << 10) + 2u, zstd_ref_lit_units());
    c->last_lit_units = lits ? lit_units : 0;
    FastDecodeArgs a;
    a.toosmall_code = toosmall_code;
    a.seq_dtables = c->seqdtab.p;
    a.meta = c->fastmeta.p;
    a.ref.pre = walk ? c->refpre.p : nullptr;
    a.ref.tables = c->reftab.p;
    a.ref.recs = c->refrecs.p;
    a.ref.recs_cap = recs_bytes / 16;
    a.ref.lits = lits ? c->reflits.p : nullptr;
    a.ref.lit_units = lit_units;
    a.dbg = dbg;
    a.side = c->side.view();
    HIPCHK(c, launch_zstd_decode_fast(z, a, s), "zstd_decode (batched) launch");
    c->last_walked = walk;
    c->last_frames = dbg ? 0 : n;
    if (c->knobs.split_min != 0 && n >= c->knobs.split_min / 2 && !dbg) {   // (the context of a call that may be split: see foreign_host)
        if (!c->foreign_host.p && !(c->foreign_host.grow(16, hipHostMallocDefault) && make_event(c->ev_foreign))) {   // (the words and their event, or neither)
            (void)hipGetLastError();
            c->foreign_host.release();
        }
        uint32_t* const d = (c->foreign_host.p && !c->foreign_pending) ? ensure_array<uint32_t>(c, c->foreign_dev, 4) : nullptr;
        if (d) {
            if (launch_count_nonzero(zstd_fast_redo(c->fastmeta.p, n), n, d, s) == hipSuccess &&
                hipMemcpyAsync(c->foreign_host.p, d, 4, hipMemcpyDeviceToHost, s) == hipSuccess && hipEventRecord(c->ev_foreign.p, s) == hipSuccess) {
                c->foreign_host.words()[1] = n;
                c->foreign_pending = true;
            } else {
                (void)hipGetLastError();
            }
        }
    }
    return 0;
}

// The entropy stage of a decompress group on the large-read path (few, large reads): frames with a span index are decoded one span per
// wavefront.  z: the frames -> their content in scratch.
int entropy_decode_spans(vbz_gpu_ctx* c, const ReadBatch& z, uint32_t toosmall_code, const StagePlan& p)
{
    SpanDecodeArgs a;
    a.toosmall_code = toosmall_code;
    a.seq_dtables = c->seqdtab.p;
    a.content_bytes = p.scratch_need;
    const size_t meta_bytes = zstd_dspan_meta_bytes(p.scratch_need, z.n_reads);
    if (!meta_bytes) {
        set_error(c, "batch too large for the span path");
        return -1;
    }
    if (!ensure(c, c->spanmeta, meta_bytes)) return -1;
    a.meta = c->spanmeta.p;
    Timed t(c, "zstd_decode");
    HIPCHK(c, launch_zstd_decode_spans(z, &a, c->stream), "zstd_decode (spans) launch");
    c->last_frames = 0;
    c->last_span_frames = z.n_reads;
    c->last_span_redo = a.redo;
    return 0;
}

// The svb stage of a decompress group (j.rb: the streams -> the reads, with the store and the normalising passes of its sig)
int svb_decode_stage(vbz_gpu_ctx* c, const DecodeJob& j, const CompressionOptions* o, bool segmented, const SegTables& seg)
{
    Timed t(c, "svb_decode");
    const TrimOut* const trim = j.trim.begin ? &j.trim : nullptr;
    const SpanOut* const span = j.span.map ? &j.span : nullptr;   // (a span call: the span pass, on the segments of the large-read path too -- DESIGN.md 4.21)
    if (j.seg.map) {   // (a segmentation call: kernels of their own, one workgroup per read on every path -- DESIGN.md 4.20)
        if (pod5_codec(o)) HIPCHK(c, launch_svb16_segment(j.rb, j.seg, c->stream), "svb16 segment launch");
        else HIPCHK(c, launch_svb_segment(j.rb, o->perform_delta_zig_zag, j.seg, c->stream), "svb segment launch");
        return 0;
    }
    if (pod5_codec(o))   // (one workgroup per read on every path: DESIGN.md 4.13)
        HIPCHK(c, launch_svb16_decode(j.rb, c->stream, trim, span), "svb16_decode launch");
    else if (segmented)
        HIPCHK(c, launch_svb_decode_seg(j.rb, (int)o->integer_size, o->perform_delta_zig_zag, seg.first, seg.max_segs, seg.val, seg.off, seg.run, c->knobs.seg_self_max, c->stream, trim, span),
               "svb_decode (segmented) launch");
    else
        HIPCHK(c, launch_svb_decode(j.rb, (int)o->integer_size, o->perform_delta_zig_zag, half_codec(o), c->stream, trim, span), "svb_decode launch");
    return 0;
}

// One launch group of a decompress call: the reads of j.rb (dst_cap = the exact decoded byte counts; those whose gate is closed
// left alone), on the one-workgroup path or on the large-read path.  dst_bytes: extent of the decoded bytes of the group.
// streams (nullable; both stages only): the svb stage is the caller's -- *streams is what it decodes (the streams, the group's gate)
int decompress_group(vbz_gpu_ctx* c, DecodeJob j, uint64_t dst_bytes, const CompressionOptions* o, bool segmented,
                     const Preplanned* pre = nullptr, ReadBatch* streams = nullptr)
{
    const uint32_t n = j.rb.n_reads;
    if (n == 0) return 0;
    hipStream_t s = c->stream;
    ReadBatch& rb = j.rb;
    if (o->integer_size == 0 && o->zstd_compression_level == 0) {
        Timed t(c, "copy_bytes");
        HIPCHK(c, launch_copy_bytes(rb, 0, s), "copy launch");
        return 0;
    }
    const bool pod5 = pod5_codec(o);
    if (rb.sig.norm.st && segmented && !pod5) {   // (a normalising decode on the large-read path: the segments' counts add up here)
        if (!(rb.sig.norm.slab = ensure_array<uint32_t>(c, c->normslab, (size_t)n * NORM_SLAB))) return -1;
    }
    StagePlan p;
    if (plan_stage_scratch(c, rb, rb.dst_cap, dst_bytes, o, false, segmented, pre, &p) != 0) return -1;
    // the gate the reads come with: a split call's (planned), the segments' (E_OOM for a read whose segments do not fit the tables) or
    // the caller's; every stage runs under the group's copy of it
    const uint32_t* const gate_src = pre ? nullptr : segmented ? p.seg.gate : rb.gate;
    if (!p.both_stages && gate_src) HIPCHK(c, hipMemcpyAsync(p.m.gate, gate_src, 4ull * n, hipMemcpyDeviceToDevice, s), "gate copy");
    if (pre || gate_src) rb.gate = p.m.gate;
    if (o->zstd_compression_level == 0) return svb_decode_stage(c, j, o, segmented, p.seg);
    if (o->integer_size == 0) {  // vbz.cpp:259-262: content larger than the destination -> DESTINATION_SIZE
        if (segmented) {
            Timed t(c, "zstd_decode");
            HIPCHK(c, launch_zstd_decode(rb, E_DESTINATION_SIZE, nullptr, c->seqdtab.p, s), "zstd_decode launch");
        } else if (zstd_frames(c, rb, E_DESTINATION_SIZE, dst_bytes, nullptr) != 0) {
            return -1;
        }
        return verify_checksums(c, rb);
    }
    if (launch_stage_plan(c, n, rb.dst_cap, gate_src, p) != 0) return -1;
    ReadBatch z = rb;   // the entropy stage: the frames -> their content in scratch
    z.dst = (uint8_t*)p.scratch_base;
    z.dst_off = p.m.svb_off;
    z.dst_cap = p.m.svb_cap;
    z.result = p.m.svb_size;
    z.gate = p.m.gate;
    // a frame whose content cannot be a valid svb stream of the expected size: the reference would
    // decode it and then fail in the svb stage with a stream error (POD5: content beyond svb16_max(n) is the zstd stage's error)
    const uint32_t toosmall_code = pod5 ? E_ZSTD : E_STREAM;
    unsigned long long* dbg = segmented ? nullptr : dbg_begin(c, n);
    if (segmented) {
        if (entropy_decode_spans(c, z, toosmall_code, p) != 0) return -1;
    } else {
        c->last_span_frames = 0;
        if (zstd_frames(c, z, toosmall_code, dst_bytes, dbg) != 0) return -1;
    }
    dbg_end(c, n, "zstd_decode: parse flush seqtables chain place huftable header queue | general sequences: flush tables records literals matches", dbg);
    if (verify_checksums(c, z) != 0) return -1;
    rb.src = (const uint8_t*)p.scratch_base;   // the svb stage: the streams -> the reads
    rb.src_off = p.m.svb_off;
    rb.src_size = p.m.svb_size;
    rb.gate = p.m.gate;
    if (streams) {
        *streams = rb;
        return 0;
    }
    return svb_decode_stage(c, j, o, segmented, p.seg);
}

// ---- per-read routing ----------------------------------------------------------------------------------------------------
// The one-workgroup / one-wavefront kernels fill the GPU with thousands of reads, but ONE very long read among them (ultra-long
// nanopore reads exist: millions of samples) would run on one wavefront of 1024 for tens of milliseconds -- the reference
// treats every buffer alike (vbz/vbz.cpp:116-208), a batch must too.  The host does not know the sizes (they live on the
// device), so every call whose arena could hold a long read routes on the device: route_reads picks the reads of
// ROUTE_MIN_BYTES and more (at most ROUTE_MAX_READS of them, ROUTE_MAX_BYTES in all: more than that and the batch shape rule
// above has already sent the whole batch down the large-read path) into a compact second group that takes the large-read
// path with small grids; in the first group their gate says GATE_SKIP.  Without long reads the second group's launches
// find nothing to do (a few empty grids per call).
constexpr uint32_t ROUTE_MIN_BYTES = (uint32_t)SEGMENTED_MIN_AVG, ROUTE_MAX_READS = 16;
constexpr uint64_t ROUTE_MAX_BYTES = 64ull << 20;

struct Routed
{
    uint32_t* gate_small = nullptr;   // [n]
    DecodeJob large;                  // ROUTE_MAX_READS compact entries (gate: GATE_SKIP behind the routed ones); compress: large.rb alone
    uint32_t* large_orig = nullptr;   // compress: raw sizes of the routed reads (= large.src_size); decompress: unused
    uint32_t* map = nullptr;          // [ROUTE_MAX_READS] index of each routed read in the batch
    uint32_t* count = nullptr;        // [1]
};

bool routing_applies(const vbz_gpu_ctx* c, const CompressionOptions* o, uint64_t raw_arena_bytes, uint32_t n)
{
    return c->knobs.routing && c->knobs.segmented < 0 && n > 1 && o->integer_size != 0 && !half_codec(o) && raw_arena_bytes >= ROUTE_MIN_BYTES;
}

// One launch group beside the context's own, on a child's stream: the child's stream waits for what the context has queued so far ...
int fork(vbz_gpu_ctx* c, const Child& k)
{
    HIPCHK(c, hipEventRecord(k.fork.p, c->stream), "event record");
    HIPCHK(c, hipStreamWaitEvent(k->stream, k.fork.p, 0), "stream wait");
    return 0;
}
// ... and the context's stream for what the child has queued: the child is done before anything enqueued behind the call runs
int join(vbz_gpu_ctx* c, const Child& k)
{
    HIPCHK(c, hipEventRecord(k.join.p, k->stream), "event record");
    HIPCHK(c, hipStreamWaitEvent(c->stream, k.join.p, 0), "stream wait");
    return 0;
}

// What a child context works with: the parent's settings, whole (Knobs), with the few that make it the child it is -- copied field by
// field, those left out (staged_encode, fast_decode, ref_chains, phase_timing, trace) were what the child had read from the environment
// for itself when it was made.  What a decompress call asks of a child is no context's state: it rides on the child's DecodeJob.
// large: the routed reads, and canonical mode's large ones -- the large-read path, nothing routed or split again.
int inherit_large(vbz_gpu_ctx* c)
{
    if (!c->large.create(c->device)) {
        set_error(c, "could not create the context of the routed reads");
        return -1;
    }
    vbz_gpu_ctx* k = c->large;
    k->knobs = c->knobs;
    k->knobs.routing = false;
    k->knobs.split_min = 0;
    k->knobs.segmented = 1;
    return 0;
}
// half: the upper half [n / 2, n) of a split call -- the one-workgroup path; it gets the call's profiling switch (its launches count under
// the parent's labels: vbz_gpu_profile_read) and what is known of foreign frames.
int inherit_half(vbz_gpu_ctx* c)
{
    if (!c->half.create(c->device)) {
        set_error(c, "could not create the context of a batch's upper half");
        return -1;
    }
    vbz_gpu_ctx* k = c->half;
    k->knobs = c->knobs;
    k->knobs.routing = false;
    k->knobs.split_min = 0;
    k->knobs.segmented = 0;
    k->profiling = c->profiling;
    k->foreign_state = c->foreign_state;
    return 0;
}

int route(vbz_gpu_ctx* c, const ReadBatch& rb, const uint32_t* raw_size, Routed* r, const TrimOut& trim = {}, const SegmentOut& seg = {},
          const SpanOut& span = {})
{
    const uint32_t n = rb.n_reads;
    if (inherit_large(c) != 0) return -1;
    RouteTables tab;
    if (!ensure_carved(c, c->route, tab, n, ROUTE_MAX_READS, route_cand_words())) return -1;
    RouteArgs a;
    a.large = tab.large;
    a.cand = tab.cand;
    const RoutedTable& l = a.large;
    r->gate_small = tab.gate_small;
    r->map = l.map;
    r->count = l.count;
    ReadBatch& g = r->large.rb = rb;
    g.n_reads = ROUTE_MAX_READS;
    g.src_off = l.src_off;
    g.src_size = l.src_size;
    g.dst_off = l.dst_off;
    g.dst_cap = l.dst_cap;
    g.gate = l.gate;
    g.result = tab.result;
    if (rb.sig.cal) g.sig.cal = l.cal;   // (the routed reads' constants, gathered through the map)
    if (rb.sig.row) g.sig.row = l.row;   // (and their first chunk rows)
    if (rb.sig.norm.st) {   // (a normalising decode: states of their own; shift_scale, and a trim's begin, written back through the map)
        g.sig.norm.st = tab.norm;
        g.sig.norm.map = r->map;
    }
    if (rb.sig.ranged()) g.sig.rmap = r->map;   // (their ranges: the call's tables, through the map)
    if (rb.sig.wfirst) g.sig.wmap = r->map;     // (and their windows)
    r->large.trim = trim, r->large.seg = seg;   // (a decompress call's trim and segmentation: the routed reads share them)
    if (seg.map) r->large.seg.rmap = r->map;    // (their boundary maps and row counts: through the map too)
    r->large.span = span;                       // (a span call's rule and tables, likewise)
    if (span.map) r->large.span.rmap = r->map;
    Timed t(c, "route");
    a.raw_size = raw_size;
    a.min_bytes = ROUTE_MIN_BYTES;
    a.max_reads = ROUTE_MAX_READS;
    a.max_bytes = ROUTE_MAX_BYTES;
    a.gate_small = r->gate_small;
    HIPCHK(c, launch_route_reads(rb, a, c->stream), "route launch");
    return fork(c, c->large);
}

// the second group is done before anything enqueued behind the call runs
int route_join(vbz_gpu_ctx* c, const Routed& r, uint32_t* result)
{
    HIPCHK(c, launch_route_results(r.large.rb.result, r.map, r.count, ROUTE_MAX_READS, result, c->large->stream), "route results launch");
    return join(c, c->large);
}


// ---- two halves of a batch in flight -------------------------------------------------------------------------------------
// One launch sequence per batch leaves the device to ONE kind of kernel at a time: instruction-bound launches (svb, packing) and
// latency-bound ones (planning, the stream decoder) each run alone, and every launch ends in a tail of partly idle CUs.  Two contexts
// coding alternate batches on streams of their own measured 572 GB/s where one reaches 545 (profiles/r05r_two_in_flight.txt).  The
// same inside ONE call: descriptors are validated, the sized headers parsed, long reads routed and the scratch slots of ALL reads
// planned once on the context's stream; then the reads are cut at the midpoint of the table, the lower half goes on on this
// stream, the upper half on a child context's stream (its own per-read tables; the scratch arena and its plan are shared -- every
// per-read table is an array, so a half is a pointer offset), and the child's stream is joined before the call returns.  A read's
// bytes do not depend on its neighbours, so the output is what the unsplit call writes (tests/test_gpu_split.py: sha256).
bool split_applies(const vbz_gpu_ctx* c, const CompressionOptions* o, uint32_t n)
{
    return c->knobs.split_min != 0 && n >= c->knobs.split_min && o->integer_size != 0 && o->zstd_compression_level != 0 && !half_codec(o) && !c->knobs.phase_timing && !c->knobs.trace;
}

struct Split
{
    uint32_t h = 0;              // reads [0, h) stay on the context, [h, n) go to the child
    Preplanned lo, hi;
};

// raw_size: the reads' raw (decoded) byte counts; num / den as the group would have chosen them
// one_sizes: the halves leave their streams' sizes in one table (Preplanned::svb_size)
int split_plan(vbz_gpu_ctx* c, const ReadBatch& rb, const uint32_t* raw_size, uint64_t raw_bytes, uint32_t num, uint32_t den, Split* sp,
               bool one_sizes = false)
{
    const uint32_t n = rb.n_reads;
    if (inherit_half(c) != 0) return -1;
    const size_t scratch_need = (size_t)(((unsigned __int128)raw_bytes * num + den - 1) / den) + (size_t)n * 96 + 256;
    SplitTables tab;
    if (!ensure(c, c->scratch, scratch_need) || !ensure_carved(c, c->splitmeta, tab, n)) return -1;
    hipStream_t s = c->stream;
    if (rb.gate) HIPCHK(c, hipMemcpyAsync(tab.gate, rb.gate, 4ull * n, hipMemcpyDeviceToDevice, s), "gate copy");
    {
        Timed t(c, "plan_scratch");
        HIPCHK(c, launch_plan_scratch(n, raw_size, num, den, c->scratch.cap, tab.svb_off, tab.svb_cap, tab.gate, rb.gate != nullptr, s), "plan launch");
    }
    sp->h = n / 2;
    sp->lo.scratch = sp->hi.scratch = c->scratch.p;
    sp->lo.svb_off = tab.svb_off;
    sp->lo.svb_cap = tab.svb_cap;
    sp->lo.gate = tab.gate;
    sp->hi.svb_off = tab.svb_off + sp->h;
    sp->hi.svb_cap = tab.svb_cap + sp->h;
    sp->hi.gate = tab.gate + sp->h;
    if (one_sizes) {
        sp->lo.svb_size = tab.svb_size;
        sp->hi.svb_size = tab.svb_size + sp->h;
    }
    return fork(c, c->half);
}

ReadBatch upper_half(const ReadBatch& rb, uint32_t h)
{
    ReadBatch u = rb;
    u.n_reads = rb.n_reads - h;
    u.src_off += h;
    u.src_size += h;
    u.dst_off += h;
    u.dst_cap += h;
    u.result += h;
    if (u.gate) u.gate += h;
    if (u.sig.cal) u.sig.cal += h;
    if (u.sig.row) u.sig.row += h;
    if (u.sig.norm.st) {
        u.sig.norm.st += h;
        u.sig.norm.ss += h;
    }
    if (u.sig.rbegin) u.sig.rbegin += h;
    if (u.sig.rend) u.sig.rend += h;
    if (u.sig.wfirst) u.sig.wfirst += h;
    return u;
}
DecodeJob upper_half(const DecodeJob& job, uint32_t h)   // (the same cut of a decompress job: its own per-read tables move with the batch's)
{
    DecodeJob u{ upper_half(job.rb, h), job.trim, job.seg, job.span };
    if (u.trim.begin) u.trim.begin += h;
    if (u.seg.map) u.seg.map_off += h, u.seg.rows += h;
    if (u.span.map) u.span.map_off += h;
    if (u.span.level) u.span.level += h;
    return u;
}

// the upper half's stream is joined whatever happened in between (it may still be writing the caller's arenas)
int split_join(vbz_gpu_ctx* c)
{
    if (join(c, c->half) != 0) return -1;
    if (c->error.empty() && !c->half->error.empty()) c->error = c->half->error;
    return 0;
}

int compress_split(vbz_gpu_ctx* c, const ReadBatch& rb, uint64_t src_bytes, const CompressionOptions* o, int sized)
{
    uint32_t num, den;
    svb_factor(o->integer_size, o->perform_delta_zig_zag, &num, &den);
    Split sp;
    if (split_plan(c, rb, rb.src_size, src_bytes, num, den, &sp) != 0) return -1;
    ReadBatch lo = rb;
    lo.n_reads = sp.h;
    int rc = compress_group(c, lo, src_bytes, o, sized, false, &sp.lo);
    if (rc == 0) rc = compress_group(c->half, upper_half(rb, sp.h), src_bytes, o, sized, false, &sp.hi);
    if (split_join(c) != 0) rc = -1;
    return rc;
}

// streams (nullable): as for decompress_group -- the halves run the entropy stage, *streams is the whole batch's behind the join
int decompress_split(vbz_gpu_ctx* c, const DecodeJob& job, uint64_t dst_bytes, const CompressionOptions* o, ReadBatch* streams = nullptr)
{
    uint32_t num, den;
    svb_factor(o->integer_size, false, &num, &den);
    Split sp;
    if (split_plan(c, job.rb, job.rb.dst_cap, dst_bytes, num, den, &sp, streams != nullptr) != 0) return -1;
    DecodeJob lo = job;
    ReadBatch hi_streams;
    lo.rb.n_reads = sp.h;
    int rc = decompress_group(c, lo, dst_bytes, o, false, &sp.lo, streams);
    if (rc == 0) rc = decompress_group(c->half, upper_half(job, sp.h), dst_bytes, o, false, &sp.hi, streams ? &hi_streams : nullptr);
    if (split_join(c) != 0) rc = -1;
    if (streams) streams->n_reads = job.rb.n_reads;   // (the lower half's tables are the whole batch's, cut at h)
    c->last_split = rc == 0;
    return rc;
}


// ---- canonical encoding ----------------------------------------------------------------------------------------------------------------
// The reference is a pure function of (input, options, libzstd version) per buffer (vbz/vbz.cpp:116-208).  This library's frames are
// standard zstd whatever path wrote them, but WHICH path a read takes follows, by default, from the shape of the call it arrives in
// (a batch of few large reads, a handful of reads, per-read routing with its limits, shared tables while the call is small): the same
// read can come out as different -- equally valid -- bytes from the HDF5 filter, the bulk re-packer and a batch of thousands.  In
// canonical mode the rule looks at the READ alone: a read of CANON_LARGE_BYTES raw bytes and more is coded as spans (every span its own
// table), every other read by one wavefront -- one kernel classifies the reads by their sizes on the device, the count of large ones
// comes back to the host (the one synchronisation of the call), and the two kinds run as two launch groups beside each other like
// per-read routing's.  Destination slots are taken to have the reference's capacity contract (vbz_max_compressed_size): the long-repeat
// coder's workspace is what a slot has above the worst-case frame.  Decoding needs no such mode.  tests/test_gpu_canonical.py holds
// vbz_compress, batches of 1 and of 4096, the HDF5 filter and the bulk re-packer to one sha256 per read.
constexpr uint32_t CANON_LARGE_BYTES = (uint32_t)SEGMENTED_MIN_AVG;

int compress_canonical(vbz_gpu_ctx* c, const ReadBatch& rb, uint64_t src_bytes, const CompressionOptions* o, int sized)
{
    const uint32_t n = rb.n_reads;
    hipStream_t s = c->stream;
    if (!c->canon_host.grow(16, hipHostMallocDefault)) {
        set_error(c, "pinned word for the canonical classification");
        return -1;
    }
    CanonGates g;
    if (!ensure_carved(c, c->route, g, n)) return -1;
    HIPCHK(c, launch_canon_classify(n, rb.src_size, rb.gate, CANON_LARGE_BYTES, g.gate_small, g.gate_large, g.counts, s), "classify launch");
    HIPCHK(c, hipMemcpyAsync(c->canon_host.p, g.counts, 8, hipMemcpyDeviceToHost, s), "count copy");
    HIPCHK(c, hipStreamSynchronize(s), "stream synchronize");
    const uint32_t nbig = c->canon_host.words()[0];
    const bool split = split_applies(c, o, n);
    if (nbig == 0) return split ? compress_split(c, rb, src_bytes, o, sized) : compress_group(c, rb, src_bytes, o, sized, false);
    if (nbig == n) return compress_group(c, rb, src_bytes, o, sized, true);
    if (inherit_large(c) != 0 || fork(c, c->large) != 0) return -1;
    ReadBatch small = rb, large = rb;
    small.gate = g.gate_small;
    large.gate = g.gate_large;
    int rc = 0;   // (as in compress_batch_impl: the second stream is joined whatever happens)
    if (compress_group(c->large, large, src_bytes, o, sized, true) != 0) rc = -1;
    if (rc == 0 && (split ? compress_split(c, small, src_bytes, o, sized) : compress_group(c, small, src_bytes, o, sized, false)) != 0) rc = -1;
    if (rc != 0 && c->error.empty() && !c->large->error.empty()) c->error = c->large->error;
    if (join(c, c->large) != 0) rc = -1;
    return rc;
}

// The caller's descriptor table is untrusted (vbz_gpu.h): one thread per read checks its slots against the declared arenas before any
// other kernel forms an address from them; the verdicts are the gate every launch group of the call starts from.
int validate_descriptors(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, ReadBatch* rb)
{
    uint32_t* g = ensure_array<uint32_t>(c, c->vgate, bt->n_reads);
    if (!g) return -1;
    HIPCHK(c, launch_validate_batch(bt->n_reads, bt->src_off, bt->src_size, bt->src_bytes, bt->dst_off, bt->dst_cap, bt->dst_bytes, g, c->stream), "validate launch");
    rb->gate = g;
    return 0;
}

// The arena extents a caller declares size the scratch: a value no device could hold is refused before any arithmetic is done with it
// (scratch bounds are a few times the extent: 2^46 bytes keeps every product inside 64 bits).
constexpr uint64_t EXTENT_MAX = 1ull << 46;
bool plausible_extents(vbz_gpu_ctx* c, const vbz_gpu_batch* bt)
{
    if (bt->n_reads != 0 && (!bt->src_off || !bt->src_size || !bt->dst_off || !bt->dst_cap || !bt->result || (!bt->src && bt->src_bytes != 0) ||
                             (!bt->dst && bt->dst_bytes != 0))) {
        set_error(c, "a table or arena pointer of the batch is NULL");
        return false;
    }
    if (bt->src_bytes <= EXTENT_MAX && bt->dst_bytes <= EXTENT_MAX) return true;
    set_error(c, "declared arena extents are not plausible (src_bytes %llu, dst_bytes %llu)", (unsigned long long)bt->src_bytes, (unsigned long long)bt->dst_bytes);
    return false;
}

// own_descriptors: the table is the library's own (the single-buffer API: one read, slots it has just allocated) -- nothing to validate
int compress_batch_impl(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, bool own_descriptors = false)
{
    const uint32_t n = bt->n_reads;
    c->last_span_frames = 0;   // (vbz_gpu_decode_span_paths: its redo[] lives in spanmeta, which a span-mode compress call carves anew)
    if (n == 0) return 0;
    ReadBatch rb = to_rb(bt);
    if (!own_descriptors && validate_descriptors(c, bt, &rb) != 0) return -1;
    if (c->knobs.canonical && c->knobs.segmented < 0 && o->integer_size != 0 && o->zstd_compression_level != 0 && !half_codec(o))
        return compress_canonical(c, rb, bt->src_bytes, o, sized);
    const bool by_shape = o->integer_size != 0 && !half_codec(o) && use_segments(c, bt->src_bytes, n, false);
    const bool split = !by_shape && split_applies(c, o, n);
    if (by_shape || !routing_applies(c, o, bt->src_bytes, n))
        return split ? compress_split(c, rb, bt->src_bytes, o, sized) : compress_group(c, rb, bt->src_bytes, o, sized, by_shape);
    Routed r;
    if (route(c, rb, bt->src_size, &r) != 0) return -1;
    ReadBatch small = rb;
    small.gate = r.gate_small;
    // (the second group first: its launches are short.)  Whatever fails from here on, the second stream is joined before the call
    // returns -- it may still be writing the caller's arenas -- and its error message becomes the context's
    int rc = 0;
    if (compress_group(c->large, r.large.rb, ROUTE_MAX_BYTES, o, sized, true) != 0) rc = -1;
    if (rc == 0 && (split ? compress_split(c, small, bt->src_bytes, o, sized) : compress_group(c, small, bt->src_bytes, o, sized, false)) != 0) rc = -1;
    if (rc != 0 && c->error.empty() && !c->large->error.empty()) c->error = c->large->error;
    if (route_join(c, r, bt->result) != 0) rc = -1;
    return rc;
}

// ---- typed decodes: the checks of the ABI's structs, the request (TypedCall), the decode, the one way in (typed_decode) ---------------
// the options of a typed decode and what it stores (`what`: which decode, for the error text).  type_ok: the format is there and its
// out_type known (the statistics alone store nothing and have no format: true)
bool typed_args_ok(vbz_gpu_ctx* c, const CompressionOptions* o, int sized, const char* what, bool type_ok, uint32_t is_signed)
{
    if (!o || o->integer_size != 2 || !batch_options_ok(o, sized)) {
        set_error(c, "unsupported options for a %s decode (integer_size must be 2, version 0, 1 or POD5)", what);
        return false;
    }
    if (!type_ok || is_signed > 1) {
        set_error(c, "signal format: NULL, unknown out_type or is_signed not 0 / 1");
        return false;
    }
    return true;
}

static_assert(CHUNK_PAD == VBZ_GPU_CHUNK_PAD && CHUNK_END == VBZ_GPU_CHUNK_END, "the ABI's chunk modes");
static_assert(sizeof(vbz_gpu_chunking) == 24, "vbz_gpu_chunking is 24 bytes");
bool chunking_ok(vbz_gpu_ctx* c, const vbz_gpu_chunking* ch)
{
    if (!ch) {
        set_error(c, "chunking is NULL");
        return false;
    }
    const uint32_t L = ch->chunk_len, S = ch->step;
    const bool align_ok = ch->mode == VBZ_GPU_CHUNK_PAD ? ch->end_align == 0 : (ch->end_align >= 1 && ch->end_align <= 4096);
    if (L < 8 || L > (1u << 20) || L % 8 != 0 || S < 8 || S > L || S % 8 != 0 || ch->mode > VBZ_GPU_CHUNK_END || !align_ok || ch->reserved != 0) {
        set_error(c, "chunking outside the rules (chunk_len %u, step %u, mode %u, end_align %u, reserved %u)", L, S, ch->mode, ch->end_align, ch->reserved);
        return false;
    }
    return true;
}
// the chunk part of SignalOut, and the arena the svb stage stores into (rb->dst: the caller's dst side only describes the reads)
void chunk_out(const vbz_gpu_chunking* ch, const uint64_t* chunk_first, void* chunks, ReadBatch* rb)
{
    rb->dst = (uint8_t*)chunks;
    rb->sig.row = chunk_first;
    rb->sig.chunk_len = ch->chunk_len;
    rb->sig.step = ch->step;
    rb->sig.mode = ch->mode;
    rb->sig.end_align = ch->end_align;
    rb->sig.pad = ch->pad;
}

// the windows of a *_windows_batch call: the struct's rules, the tables and the arena a call with reads needs (n_out: the reads the tables
// have entries for), the arena's alignment and extent
static_assert(sizeof(vbz_gpu_windows) == 40, "vbz_gpu_windows is 40 bytes");
static_assert(offsetof(vbz_gpu_windows, window_len) == 0 && offsetof(vbz_gpu_windows, pad) == 4 && offsetof(vbz_gpu_windows, window_rows) == 8 &&
                  offsetof(vbz_gpu_windows, window_first) == 16 && offsetof(vbz_gpu_windows, start) == 24 && offsetof(vbz_gpu_windows, flags) == 32 &&
                  offsetof(vbz_gpu_windows, reserved) == 36,
              "the fields of vbz_gpu_windows");
bool windows_ok(vbz_gpu_ctx* c, const vbz_gpu_windows* w, const void* out, uint32_t n_out, uint32_t elem)
{
    if (!w) {
        set_error(c, "windows is NULL");
        return false;
    }
    const uint32_t L = w->window_len;
    if (L < 8 || L > (1u << 20) || L % 8 != 0 || w->flags != 0 || w->reserved != 0) {
        set_error(c, "windows outside the rules (window_len %u, flags %u, reserved %u)", L, w->flags, w->reserved);
        return false;
    }
    if (n_out != 0 && (!w->window_first || (!w->start && w->window_rows != 0) || !out)) {
        set_error(c, "window_first, start or the window arena is NULL");
        return false;
    }
    if (((uintptr_t)out & 15u) != 0) {
        set_error(c, "the window arena is not 16-byte aligned");
        return false;
    }
    const uint64_t row_bytes = (uint64_t)L * elem;
    if (w->window_rows > EXTENT_MAX / row_bytes) {
        set_error(c, "declared window arena is not plausible (%llu rows of %llu bytes)", (unsigned long long)w->window_rows, (unsigned long long)row_bytes);
        return false;
    }
    return true;
}
// the window part of SignalOut, and the arena the svb stage stores into
void window_out(const vbz_gpu_windows* w, void* out, ReadBatch* rb)
{
    rb->dst = (uint8_t*)out;
    rb->sig.wfirst = w->window_first;
    rb->sig.wstart = w->start;
    rb->sig.wrows = w->window_rows;
    rb->sig.chunk_len = w->window_len;
    rb->sig.pad = w->pad;
}

// the match of a *_match_batch call: the struct's rules, the tables and the arenas a call with reads needs, their alignment and extent
static_assert(sizeof(vbz_gpu_match) == 40, "vbz_gpu_match is 40 bytes");
static_assert(offsetof(vbz_gpu_match, query_len) == 0 && offsetof(vbz_gpu_match, n_refs) == 4 && offsetof(vbz_gpu_match, ref_stride) == 8 &&
                  offsetof(vbz_gpu_match, flags) == 12 && offsetof(vbz_gpu_match, quant) == 16 && offsetof(vbz_gpu_match, reserved) == 20 &&
                  offsetof(vbz_gpu_match, ref) == 24 && offsetof(vbz_gpu_match, ref_len) == 32,
              "the fields of vbz_gpu_match");
static_assert(sizeof(vbz_gpu_match_hit) == 8 && offsetof(vbz_gpu_match_hit, cost) == 0 && offsetof(vbz_gpu_match_hit, end) == 4,
              "vbz_gpu_match_hit is 8 bytes: cost, end");
static_assert(sizeof(vbz_gpu_match_span) == 16 && offsetof(vbz_gpu_match_span, cost) == 0 && offsetof(vbz_gpu_match_span, end) == 4 &&
                  offsetof(vbz_gpu_match_span, start) == 8 && offsetof(vbz_gpu_match_span, zero) == 12,
              "vbz_gpu_match_span is 16 bytes: cost, end, start, zero");
// the locate of a *_locate_batch call, likewise
static_assert(sizeof(vbz_gpu_locate) == 40, "vbz_gpu_locate is 40 bytes");
static_assert(offsetof(vbz_gpu_locate, query_len) == 0 && offsetof(vbz_gpu_locate, n_targets) == 4 && offsetof(vbz_gpu_locate, target_stride) == 8 &&
                  offsetof(vbz_gpu_locate, flags) == 12 && offsetof(vbz_gpu_locate, quant) == 16 && offsetof(vbz_gpu_locate, reserved) == 20 &&
                  offsetof(vbz_gpu_locate, target) == 24 && offsetof(vbz_gpu_locate, target_len) == 32,
              "the fields of vbz_gpu_locate");
// What the two structs share, field for field: the view every check and launch below takes.  `levels` is the int8 matrix -- the references
// of a match, the targets of a locate -- n_levels rows of levels_stride bytes.
struct AlignView
{
    bool null;   // the caller's struct is NULL
    uint32_t query_len, n_levels, levels_stride, flags;
    float quant;
    uint32_t reserved;
    const int8_t* levels;
    const uint32_t* levels_len;
};
AlignView align_view(const vbz_gpu_match* m)
{
    return m ? AlignView{ false, m->query_len, m->n_refs, m->ref_stride, m->flags, m->quant, m->reserved, m->ref, m->ref_len } : AlignView{ true };
}
AlignView align_view(const vbz_gpu_locate* l)
{
    return l ? AlignView{ false, l->query_len, l->n_targets, l->target_stride, l->flags, l->quant, l->reserved, l->target, l->target_len } : AlignView{ true };
}
// The two kinds: the nouns of their messages, the profile entries and launches of their calls, and their limits.  A match's references
// sit in the lanes (32 rows a lane: 2048) and its query is streamed; a locate's query sits in the lanes (query_in_lanes) and its targets
// are streamed, so they alone can be implausibly large, a path's rows are the query's, and its valid[] is never NULL.
struct AlignKind
{
    const char *name, *level, *levels;   // "match", "ref", "refs"
    uint32_t query_max, stride_max;
    bool query_in_lanes;
    const char *forward_entry, *trace_entry, *forward_launch, *trace_launch, *hit_launch, *span_launch;
    hipError_t (*hit)(uint32_t, const float*, const uint32_t*, uint32_t, float, const int8_t*, const uint32_t*, uint32_t, uint32_t, void*, hipStream_t);
    hipError_t (*span)(uint32_t, const float*, const uint32_t*, uint32_t, float, const int8_t*, const uint32_t*, uint32_t, uint32_t, void*, hipStream_t);
    hipError_t (*path_forward)(const AlignPathArgs&, hipStream_t);
    hipError_t (*path_trace)(const AlignPathArgs&, hipStream_t);
};
const AlignKind MATCH = { "match", "ref", "refs", 65536u, 2048u, false, "match_path_forward", "match_path_trace", "match path forward launch",
                          "match path traceback launch", "match launch", "match span launch", launch_match, launch_match_span,
                          launch_match_path_forward, launch_match_path_trace };
const AlignKind LOCATE = { "locate", "target", "targets", 2048u, 1u << 30, true, "locate_path_forward", "locate_path_trace",
                           "locate path forward launch", "locate path traceback launch", "locate launch", "locate span launch", launch_locate,
                           launch_locate_span, launch_locate_path_forward, launch_locate_path_trace };
// (out: n_out x n_levels entries of hit_bytes each -- vbz_gpu_match_hit, or vbz_gpu_match_span of the span calls)
bool align_ok(vbz_gpu_ctx* c, const AlignKind& k, const AlignView& m, const float* query, const void* out, size_t hit_bytes, uint32_t n_out)
{
    if (m.null) {
        set_error(c, "%s is NULL", k.name);
        return false;
    }
    const uint32_t N = m.query_len, R = m.n_levels, S = m.levels_stride;
    if (N < 8 || N > k.query_max || N % 8 != 0 || R < 1 || R > 4096 || S < 16 || S > k.stride_max || S % 16 != 0 || !(m.quant > 0.0f) ||
        !std::isfinite(m.quant) || m.flags != 0 || m.reserved != 0) {
        set_error(c, "%s outside the rules (query_len %u, n_%s %u, %s_stride %u, quant %g, flags %u, reserved %u)", k.name, N, k.levels, R, k.level, S,
                  (double)m.quant, m.flags, m.reserved);
        return false;
    }
    if (n_out != 0 && (!m.levels || !m.levels_len || !query || !out)) {
        set_error(c, "%s, %s_len, the query arena or the hit arena is NULL", k.level, k.level);
        return false;
    }
    if ((((uintptr_t)m.levels | (uintptr_t)query | (uintptr_t)out) & 15u) != 0) {
        set_error(c, "%s, the query arena or the hit arena is not 16-byte aligned", k.level);
        return false;
    }
    if ((uint64_t)n_out * R > EXTENT_MAX / hit_bytes || (k.query_in_lanes && (uint64_t)R * S > EXTENT_MAX) || (uint64_t)n_out * N > EXTENT_MAX / sizeof(float)) {
        if (k.query_in_lanes) set_error(c, "declared locate arenas are not plausible (%u reads, %u targets of %u bytes, %u samples)", n_out, R, S, N);
        else set_error(c, "declared match arenas are not plausible (%u reads, %u references, %u samples)", n_out, R, N);
        return false;
    }
    return true;
}
// The fused calls' scratch: the window tables of "one row per read, start 0" (the library's own, so the window check cannot fail), valid[],
// and a read_result for a POD5 caller that passed none (the verdicts are where valid[] comes from)
struct MatchTables
{
    uint64_t* first = nullptr;      // [n + 1]
    int32_t* start = nullptr;       // [n]
    uint32_t* valid = nullptr;      // [n]
    uint32_t* read_result = nullptr;   // [n]
    size_t carve(void* base, uint32_t n)
    {
        MetaCarver mc(base);
        first = mc.take<uint64_t>((size_t)n + 1);
        start = mc.take<int32_t>(n);
        valid = mc.take<uint32_t>(n);
        read_result = mc.take<uint32_t>(n);
        return mc.bytes();
    }
};

// the events of a *_signal_events_batch call: the struct's rules, the output type (records are float32), the tables and the arenas a call
// with reads needs (n_out: the reads the tables have entries for), the arenas' alignment and extent
static_assert(sizeof(vbz_gpu_events) == 32, "vbz_gpu_events is 32 bytes");
static_assert(offsetof(vbz_gpu_events, event_rows) == 0 && offsetof(vbz_gpu_events, event_first) == 8 && offsetof(vbz_gpu_events, start) == 16 &&
                  offsetof(vbz_gpu_events, flags) == 24 && offsetof(vbz_gpu_events, reserved) == 28,
              "the fields of vbz_gpu_events");
static_assert(sizeof(vbz_gpu_event) == 16 && offsetof(vbz_gpu_event, mean) == 0 && offsetof(vbz_gpu_event, sd) == 4 && offsetof(vbz_gpu_event, n) == 8 &&
                  offsetof(vbz_gpu_event, zero) == 12,
              "vbz_gpu_event is 16 bytes: mean, sd, n, zero");
static_assert(sizeof(vbz_gpu_event_moments) == 16 && offsetof(vbz_gpu_event_moments, sum) == 0 && offsetof(vbz_gpu_event_moments, sumsq) == 8,
              "vbz_gpu_event_moments is 16 bytes: sum, sumsq");
bool events_ok(vbz_gpu_ctx* c, const vbz_gpu_events* ev, const vbz_gpu_signal_format* f, const vbz_gpu_event* out, const vbz_gpu_event_moments* moments,
               uint32_t n_out)
{
    if (!ev) {
        set_error(c, "events is NULL");
        return false;
    }
    if (ev->flags != 0 || ev->reserved != 0) {
        set_error(c, "events outside the rules (flags %u, reserved %u)", ev->flags, ev->reserved);
        return false;
    }
    if (f->out_type != VBZ_GPU_SIGNAL_F32) {
        set_error(c, "event records are float32 (out_type %u)", f->out_type);
        return false;
    }
    if (n_out != 0 && (!ev->event_first || (!ev->start && ev->event_rows != 0) || !out)) {
        set_error(c, "event_first, start or the event arena is NULL");
        return false;
    }
    if ((((uintptr_t)out | (uintptr_t)moments) & 15u) != 0) {
        set_error(c, "the event arena or the moments are not 16-byte aligned");
        return false;
    }
    if (ev->event_rows > EXTENT_MAX / sizeof(vbz_gpu_event)) {
        set_error(c, "declared event arena is not plausible (%llu rows of 16 bytes)", (unsigned long long)ev->event_rows);
        return false;
    }
    return true;
}
// the event part of SignalOut (the windows' tables), and the arena the svb stage adds into: the rows' moments (the caller's, or the call's
// scratch).  The records' arena is the finish launch's argument.
void event_out(const vbz_gpu_events* ev, void* moments, ReadBatch* rb)
{
    rb->dst = (uint8_t*)moments;
    rb->sig.wfirst = ev->event_first;
    rb->sig.wstart = reinterpret_cast<const int32_t*>(ev->start);
    rb->sig.wrows = ev->event_rows;
    rb->sig.events = 1;
}

// the ranges of a *_range_batch call (nullable: the un-ranged call)
static_assert(RANGE_STATS_RANGE == VBZ_GPU_RANGE_STATS_RANGE && RANGE_STATS_READ == VBZ_GPU_RANGE_STATS_READ, "the ABI's stats modes");
static_assert(sizeof(vbz_gpu_sample_ranges) == 24, "vbz_gpu_sample_ranges is 24 bytes");
bool ranges_ok(vbz_gpu_ctx* c, const vbz_gpu_sample_ranges* g)
{
    if (g && (g->reserved != 0 || g->stats > VBZ_GPU_RANGE_STATS_READ)) {
        set_error(c, "sample ranges outside their rules (stats %u, reserved %u)", g->stats, g->reserved);
        return false;
    }
    return true;
}

static_assert(NORM_MED_MAD == VBZ_GPU_NORM_MED_MAD && NORM_QUANTILE == VBZ_GPU_NORM_QUANTILE, "the ABI's methods");
static_assert(sizeof(vbz_gpu_normalization) == 32, "vbz_gpu_normalization is 32 bytes");
// the normalisation's fields (include/vbz_gpu.h), and a format whose constants the call would ignore
bool norm_ok(vbz_gpu_ctx* c, const vbz_gpu_normalization* m, const vbz_gpu_signal_format* f)
{
    if (!m) {
        set_error(c, "normalization is NULL");
        return false;
    }
    const bool fin = std::isfinite(m->shift_mul) && std::isfinite(m->scale_mul) && (std::isfinite(m->shift_min) || m->shift_min == -INFINITY);
    const bool q = m->method == VBZ_GPU_NORM_MED_MAD ? m->quantile_a == 0.0f && m->quantile_b == 0.0f
                                                      : 0.0f <= m->quantile_a && m->quantile_a <= m->quantile_b && m->quantile_b <= 1.0f;
    const bool known = m->method == VBZ_GPU_NORM_MED_MAD || m->method == VBZ_GPU_NORM_QUANTILE;
    if (!known || m->reserved != 0 || !q || !fin || !std::isnormal(m->scale_min) || !(m->scale_min > 0.0f)) {
        set_error(c, "normalization outside its rules (method %u, reserved %u, quantiles %g / %g, shift_mul %g, scale_mul %g, shift_min %g, scale_min %g)",
                  m->method, m->reserved, (double)m->quantile_a, (double)m->quantile_b, (double)m->shift_mul, (double)m->scale_mul,
                  (double)m->shift_min, (double)m->scale_min);
        return false;
    }
    if (f && (f->offset || f->scale)) {
        set_error(c, "a normalising decode takes no offset or scale table (the statistics give them)");
        return false;
    }
    return true;
}
// st: the call's per-read state; ss: where the reads' {shift, scale} go
NormOut norm_out(const vbz_gpu_normalization* m, NormRead* st, float2* ss)
{
    NormOut no;
    no.st = st;
    no.ss = ss;
    no.method = m->method;
    no.qa = m->quantile_a;
    no.qb = m->quantile_b;
    no.shift_mul = m->shift_mul;
    no.scale_mul = m->scale_mul;
    no.shift_min = m->shift_min;
    no.scale_min = m->scale_min;
    return no;
}

// the trim's fields (include/vbz_gpu.h) and its table; a read's windows must fit the counting passes' bins
static_assert(TRIM_REJECT_AT_END == VBZ_GPU_TRIM_REJECT_AT_END, "the ABI's trim flags");
static_assert(sizeof(vbz_gpu_trim) == 32, "vbz_gpu_trim is 32 bytes");
bool trim_ok(vbz_gpu_ctx* c, const vbz_gpu_trim* t, const uint32_t* begin)
{
    if (!t || !begin) {
        set_error(c, "trim or begin is NULL");
        return false;
    }
    const bool fields = t->window >= 1 && t->window <= 65536 && t->max_samples >= 1 && std::isfinite(t->threshold_factor) &&
                        std::isfinite(t->max_fraction) && t->max_fraction > 0.0f && t->max_fraction <= 1.0f &&
                        (t->flags & ~(uint32_t)VBZ_GPU_TRIM_REJECT_AT_END) == 0 && t->reserved == 0;
    if (!fields || (t->max_samples - std::min(t->min_trim, t->max_samples)) / t->window > TRIM_MAX_WINDOWS) {
        set_error(c, "trim outside its rules (window %u, min_elements %u, min_trim %u, max_samples %u, threshold_factor %g, max_fraction %g, flags %u, "
                     "reserved %u; at most %u windows)",
                  t->window, t->min_elements, t->min_trim, t->max_samples, (double)t->threshold_factor, (double)t->max_fraction, t->flags, t->reserved,
                  TRIM_MAX_WINDOWS);
        return false;
    }
    return true;
}
TrimOut trim_out(const vbz_gpu_trim* t, uint32_t* begin)
{
    TrimOut to;
    to.begin = begin;
    to.W = t->window;
    to.m = t->min_elements;
    to.t0 = t->min_trim;
    to.M = t->max_samples;
    to.flags = t->flags;
    to.f = t->threshold_factor;
    to.max_fraction = t->max_fraction;
    return to;
}

// the segmentation's fields (include/vbz_gpu.h) and its two tables
static_assert(sizeof(vbz_gpu_segmentation) == 32, "vbz_gpu_segmentation is 32 bytes");
static_assert(offsetof(vbz_gpu_segmentation, short_window) == 0 && offsetof(vbz_gpu_segmentation, long_window) == 4 &&
                  offsetof(vbz_gpu_segmentation, short_threshold) == 8 && offsetof(vbz_gpu_segmentation, long_threshold) == 12 &&
                  offsetof(vbz_gpu_segmentation, radius) == 16 && offsetof(vbz_gpu_segmentation, flags) == 20 &&
                  offsetof(vbz_gpu_segmentation, start_cap) == 24,
              "the fields of vbz_gpu_segmentation");
bool segmentation_ok(vbz_gpu_ctx* c, const vbz_gpu_segmentation* g, const uint64_t* event_first, const uint32_t* start)
{
    if (!g || !event_first) {
        set_error(c, "segmentation or event_first is NULL");
        return false;
    }
    if (!start && g->start_cap != 0) {
        set_error(c, "start is NULL with start_cap %llu (the count-only call: NULL and 0)", (unsigned long long)g->start_cap);
        return false;
    }
    auto threshold_ok = [](float t) { return std::isfinite(t) && t > 0.0f; };
    const bool fields = g->short_window >= 1 && g->short_window <= SEGMENT_WINDOW_MAX && g->long_window <= SEGMENT_WINDOW_MAX && g->radius >= 1 &&
                        g->radius <= SEGMENT_RADIUS_MAX && threshold_ok(g->short_threshold) && (g->long_window == 0 || threshold_ok(g->long_threshold)) &&
                        g->flags == 0;
    if (!fields) {
        set_error(c, "segmentation outside its rules (short_window %u, long_window %u, short_threshold %g, long_threshold %g, radius %u, flags %u)",
                  g->short_window, g->long_window, (double)g->short_threshold, (double)g->long_threshold, g->radius, g->flags);
        return false;
    }
    if (g->start_cap > EXTENT_MAX / sizeof(uint32_t)) {
        set_error(c, "declared start table is not plausible (%llu entries of 4 bytes)", (unsigned long long)g->start_cap);
        return false;
    }
    return true;
}
// the rule's part of SegmentOut (the tables and the map: the call's scratch, decompress_batch_impl)
SegmentOut segment_out(const vbz_gpu_segmentation* g)
{
    SegmentOut so;
    so.w1 = g->short_window;
    so.w2 = g->long_window;
    so.r = g->radius;
    so.k1 = (double)g->short_threshold * (double)g->short_threshold;
    so.k2 = so.w2 ? (double)g->long_threshold * (double)g->long_threshold : 1.0;
    return so;
}

// the spans' fields (include/vbz_gpu.h) and their two tables; level: given exactly when there is no normalisation
static_assert(SPAN_ABOVE == VBZ_GPU_SPAN_ABOVE && SPAN_BELOW == VBZ_GPU_SPAN_BELOW, "the ABI's span directions");
static_assert(sizeof(vbz_gpu_spans) == 40, "vbz_gpu_spans is 40 bytes");
static_assert(offsetof(vbz_gpu_spans, direction) == 0 && offsetof(vbz_gpu_spans, merge_gap) == 4 && offsetof(vbz_gpu_spans, min_length) == 8 &&
                  offsetof(vbz_gpu_spans, ignore_prefix) == 12 && offsetof(vbz_gpu_spans, threshold_factor) == 16 && offsetof(vbz_gpu_spans, flags) == 20 &&
                  offsetof(vbz_gpu_spans, level) == 24 && offsetof(vbz_gpu_spans, edge_cap) == 32,
              "the fields of vbz_gpu_spans");
bool spans_ok(vbz_gpu_ctx* c, const vbz_gpu_spans* g, const uint64_t* edge_first, const uint32_t* edge, bool with_norm)
{
    if (!g || !edge_first) {
        set_error(c, "spans or edge_first is NULL");
        return false;
    }
    if (!edge && g->edge_cap != 0) {
        set_error(c, "edge is NULL with edge_cap %llu (the count-only call: NULL and 0)", (unsigned long long)g->edge_cap);
        return false;
    }
    const bool fields = g->direction <= VBZ_GPU_SPAN_BELOW && g->merge_gap <= SPAN_GAP_MAX && g->min_length >= 1 && g->min_length <= SPAN_LENGTH_MAX &&
                        std::isfinite(g->threshold_factor) && g->flags == 0;
    if (!fields) {
        set_error(c, "spans outside their rules (direction %u, merge_gap %u, min_length %u, threshold_factor %g, flags %u)", g->direction, g->merge_gap,
                  g->min_length, (double)g->threshold_factor, g->flags);
        return false;
    }
    if ((g->level != nullptr) == with_norm) {
        set_error(c, with_norm ? "spans: level must be NULL with a normalisation (the statistics give the constants)"
                               : "spans: level is NULL and there is no normalisation");
        return false;
    }
    if (g->edge_cap > EXTENT_MAX / sizeof(uint32_t)) {
        set_error(c, "declared edge table is not plausible (%llu entries of 4 bytes)", (unsigned long long)g->edge_cap);
        return false;
    }
    return true;
}
// the rule's part of SpanOut (the map and its offsets: the call's scratch, typed_outputs)
SpanOut span_out(const vbz_gpu_spans* g)
{
    SpanOut so;
    so.level = reinterpret_cast<const float2*>(g->level);
    so.below = g->direction == VBZ_GPU_SPAN_BELOW ? 1u : 0u;
    so.D = g->merge_gap;
    so.m = g->min_length;
    so.p0 = g->ignore_prefix;
    so.f = g->threshold_factor;
    return so;
}

// POD5 reads of several rows (o nullable: a call without options)
static_assert(sizeof(vbz_gpu_pod5_reads) == 24, "vbz_gpu_pod5_reads is 24 bytes");
bool pod5_reads_ok(vbz_gpu_ctx* c, const CompressionOptions* o, const vbz_gpu_pod5_reads* reads)
{
    if (o && !pod5_codec(o)) {
        set_error(c, "the calls over POD5 reads take POD5 options only");
        return false;
    }
    if (!reads || reads->reserved != 0 || !reads->first_row) {
        set_error(c, "reads: NULL, reserved not 0 or a NULL first_row");
        return false;
    }
    return true;
}

// TypedCall: one typed decode as its entry point states it (the table of entries: in front of them, below).  A part the entry does not
// have keeps its default.  Where the entries' rules for a NULL differ, the entry says which one holds (Null); it is not inferred.
enum class Typed { SIGNAL, CHUNKS, STATISTICS, EVENTS, SEGMENT, SPANS };   // what is stored: typed samples in the reads' slots; in chunks; nothing (the
                                                                    // constants alone); one record per caller-listed event; nothing in the
                                                                    // reads' slots either -- every read's event starts, found on the device;
                                                                    // the same for every read's spans above or below its level
enum class Null { ALLOWED, REFUSED, REFUSED_WITH_READS };   // REFUSED_WITH_READS: refused unless the call has no read to write an entry for
struct TypedCall
{
    Typed kind;
    int sized;
    const vbz_gpu_signal_format* f = nullptr;   // SIGNAL, CHUNKS: the caller's.  STATISTICS: none, is_signed alone (typed_decode gives
    uint32_t is_signed = 0;                     // ... the decode {SIG_NONE, is_signed} here)
    const vbz_gpu_chunking* ch = nullptr;       // CHUNKS: rb.dst becomes the chunk arena and the svb stage stores the typed samples into
    const uint64_t* chunk_first = nullptr;      // ... the reads' chunks (untrusted: chunk_slots gates every read whose entries are not
    void* chunks = nullptr;                     // ... exactly its chunks before anything of it is decoded)
    uint64_t chunk_rows = 0;
    bool with_windows = false;                  // CHUNKS, in place of a chunking (never both): rb.dst becomes the window arena and the svb
    const vbz_gpu_windows* win = nullptr;       // ... stage stores the typed samples into the reads' windows (untrusted: the window check
    void* win_out = nullptr;                    // ... gates every read whose rows or starts are not in order before anything of it is stored)
    const vbz_gpu_events* ev = nullptr;         // EVENTS: rb.dst becomes the rows' moments; the svb stage adds them up and a launch behind
    vbz_gpu_event* ev_out = nullptr;            // ... it writes the records to ev_out (untrusted tables: the event check is the window
    vbz_gpu_event_moments* ev_moments = nullptr;   // ... check, unsigned).  ev_moments NULL: the moments live in the call's scratch
    const vbz_gpu_normalization* norm = nullptr;   // non-null: a normalising decode (the constants from the reads' statistics, into cal
    Null norm_null = Null::ALLOWED;                // ... and shift_scale)
    float* shift_scale = nullptr;
    Null shift_scale_null = Null::ALLOWED;
    const vbz_gpu_sample_ranges* ranges = nullptr;   // nullable in every entry that has it (per READ with `reads`)
    bool pod5 = false;                               // the entry is over POD5 reads of several rows: `reads` must be there, and the
    const vbz_gpu_pod5_reads* reads = nullptr;       // ... constants, chunk_first, shift_scale, ranges and begin are per READ
    bool with_trim = false;                          // a trim call (the statistics, then the trim pass): the rule, and the table it fills
    const vbz_gpu_trim* trim = nullptr;
    uint32_t* begin = nullptr;
    const vbz_gpu_segmentation* seg = nullptr;       // SEGMENT (is_signed as for STATISTICS): the rule, and the two tables the call fills --
    uint64_t* seg_first = nullptr;                   // ... event_first and start, the layout a vbz_gpu_events reads
    uint32_t* seg_start = nullptr;
    const vbz_gpu_spans* spans = nullptr;            // SPANS (is_signed as for STATISTICS; norm nullable: the constants are then spans->level): the
    uint64_t* edge_first = nullptr;                  // ... rule, and the two tables the call fills -- edge_first and edge, which a vbz_gpu_events
    uint32_t* edge = nullptr;                        // ... reads as event_first and start
    bool with_match = false;                         // CHUNKS, in place of a chunking or windows: the window call of one row per read at start 0
    const AlignKind* align = nullptr;                // ... into match_query (the library's own window tables), then the launch of a match or of a
    AlignView match = { true };                      // ... locate (untrusted like every struct: NULL is refused) on the context's stream: every
    float* match_query = nullptr;                    // ... pair's hit into match_out -- vbz_gpu_match_hit, or with match_span vbz_gpu_match_span
    void* match_out = nullptr;                       // ... (the span launch in the other's place)
    bool match_span = false;

    TypedCall(Typed k, int s) : kind(k), sized(s) {}
    TypedCall& format(const vbz_gpu_signal_format* f_) { f = f_; return *this; }
    TypedCall& statistics(uint32_t is_signed_) { is_signed = is_signed_; return *this; }
    TypedCall& chunking(const vbz_gpu_chunking* ch_, const uint64_t* first, void* arena, uint64_t rows)
    {
        ch = ch_, chunk_first = first, chunks = arena, chunk_rows = rows;
        return *this;
    }
    TypedCall& windows(const vbz_gpu_windows* w, void* arena)
    {
        with_windows = true, win = w, win_out = arena;
        return *this;
    }
    TypedCall& events(const vbz_gpu_events* e, vbz_gpu_event* arena, vbz_gpu_event_moments* moments)
    {
        ev = e, ev_out = arena, ev_moments = moments;
        return *this;
    }
    TypedCall& normalise(const vbz_gpu_normalization* m, Null m_null, float* ss, Null ss_null)
    {
        norm = m, norm_null = m_null, shift_scale = ss, shift_scale_null = ss_null;
        return *this;
    }
    TypedCall& range(const vbz_gpu_sample_ranges* g) { ranges = g; return *this; }
    TypedCall& pod5_reads(const vbz_gpu_pod5_reads* r) { pod5 = true, reads = r; return *this; }
    TypedCall& trimmed(const vbz_gpu_trim* t, uint32_t* b) { with_trim = true, trim = t, begin = b; return *this; }
    TypedCall& segmented(const vbz_gpu_segmentation* g, uint64_t* first, uint32_t* start) { seg = g, seg_first = first, seg_start = start; return *this; }
    TypedCall& spanned(const vbz_gpu_spans* g, uint64_t* first, uint32_t* e) { spans = g, edge_first = first, edge = e; return *this; }
    TypedCall& aligned(const AlignKind& k, const AlignView& m, float* query, vbz_gpu_match_hit* out) { with_match = true, align = &k, match = m, match_query = query, match_out = out; return *this; }
    TypedCall& aligned(const AlignKind& k, const AlignView& m, float* query, vbz_gpu_match_span* out) { aligned(k, m, query, (vbz_gpu_match_hit*)nullptr); match_out = out, match_span = true; return *this; }
};

// Typed decode (vbz_gpu_decompress_signal_batch): the caller's dst side describes the typed arena, E bytes per sample.  The call decodes
// through the int16 slot table made from it here -- offsets and capacities / E * 2, the extent likewise -- so that the descriptor checks,
// the sized headers, the scratch plan, routing and the split see exactly what an int16 call with those capacities sees; the svb stage
// alone stores the typed samples (rb.sig).  A slot whose offset or capacity is not a multiple of E gets VBZ_DESTINATION_SIZE_ERROR.
// The typed slots lie inside [0, dst_bytes) iff the int16 ones lie inside [0, dst_bytes / E * 2): validate_descriptors looked at the former.
static_assert(SIG_F32 == VBZ_GPU_SIGNAL_F32 && SIG_F16 == VBZ_GPU_SIGNAL_F16 && SIG_BF16 == VBZ_GPU_SIGNAL_BF16, "the ABI's output types");
// *cal: the per-read constants, for rb->sig.cal
int signal_slots(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const vbz_gpu_signal_format* f, ReadBatch* rb, uint64_t* dst_bytes, float2** cal)
{
    const uint32_t n = bt->n_reads, elem = f->out_type == VBZ_GPU_SIGNAL_F32 ? 4u : 2u;
    TypedSlots m;
    if (!ensure_carved(c, c->sigmeta, m, n)) return -1;
    *cal = m.cal;
    Timed t(c, "signal_slots");
    HIPCHK(c, launch_signal_slots(n, bt->dst_off, bt->dst_cap, elem, f->offset, f->scale, m.off16, m.cap16, m.cal, reinterpret_cast<uint32_t*>(c->vgate.p),
                                  c->stream),
           "signal slots launch");
    rb->dst_off = m.off16;
    rb->dst_cap = m.cap16;
    *dst_bytes = bt->dst_bytes / elem * 2u;
    return 0;
}

// The call's tables over POD5 reads (Pod5Reads) and the reads' constants, from ctx->pod5meta; the check of first_row is queued here, before
// any other launch of the call (out: read_result or read_samples, nullable -- E_INPUT_SIZE in every entry when the table is bad)
int pod5_reads_begin(vbz_gpu_ctx* c, uint32_t n_rows, const vbz_gpu_pod5_reads* reads, uint32_t* out, Pod5Reads* pr, float2** cal)
{
    Pod5Tables tab;
    if (!ensure_carved(c, c->pod5meta, tab, n_rows, reads->n_reads)) return -1;
    *pr = tab.pr;
    *cal = tab.cal;
    pr->n_reads = reads->n_reads;
    pr->first_row = reads->first_row;
    pr->read_result = reads->read_result;
    Timed t(c, "pod5_reads_check");
    HIPCHK(c, launch_pod5_reads_check(n_rows, *pr, out, c->stream), "pod5 reads check launch");
    return 0;
}

struct CallScratch { WindowScratch win; SegmentScratch seg; float2* cal = nullptr; };   // a window or an event call's (scan == nullptr: neither); a segmentation's; the per-read constants

// The tables and the maps of a segmentation or a span call over n reads: one bit a sample of the int16 layout of dst_bytes, every read's
// map rounded up to 4 bytes (launch_segment_layout lays them out, the carve sizes the tables)
bool read_maps(vbz_gpu_ctx* c, uint64_t dst_bytes, uint32_t n, CallScratch* sc, ReadMaps* m)
{
    m->map_cap = dst_bytes / 16 + 4ull * n + 64;
    m->map = ensure_carved(c, c->segmtab, sc->seg, n) ? ensure_array<uint8_t>(c, c->segmap, m->map_cap) : nullptr;
    m->map_off = sc->seg.map_off;
    return m->map != nullptr;
}

// Outputs: what the call stores and where.  j->rb (the caller's batch so far) gets its sig and the arena the svb stage writes, j->trim /
// j->seg a trim's or a segmentation's rule and tables; *dst_bytes: the extent of the int16 layout the call decodes through (every kind
// but SIGNAL: the caller's dst side as it is).  sc->cal comes in as the constants' table of a call over POD5 reads (pod5_reads_begin).
int typed_outputs(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const TypedCall& t, DecodeJob* j, uint64_t* dst_bytes, CallScratch* sc)
{
    ReadBatch& rb = j->rb;
    const uint32_t n = bt->n_reads, n_const = t.reads ? t.reads->n_reads : n;   // n_const: how many reads have constants and statistics
    float2* cal = nullptr;   // the per-read constants
    switch (t.kind) {
    case Typed::SIGNAL:   // typed slots (of POD5 rows too)
        if (signal_slots(c, bt, t.f, &rb, dst_bytes, &cal) != 0) return -1;
        break;
    case Typed::CHUNKS:
        if (t.with_windows) window_out(t.win, t.win_out, &rb);
        else chunk_out(t.ch, t.chunk_first, t.chunks, &rb);
        if (t.with_windows && !ensure_carved(c, c->winmeta, sc->win, n_const)) return -1;
        break;
    case Typed::EVENTS: {   // (an event call takes the window call's way: its tables are the windows')
        void* const moments = t.ev_moments ? (void*)t.ev_moments : (void*)ensure_array<vbz_gpu_event_moments>(c, c->evmeta, std::max<uint64_t>(t.ev->event_rows, 1));
        if (!moments || !ensure_carved(c, c->winmeta, sc->win, n_const)) return -1;
        event_out(t.ev, moments, &rb);
        break;
    }
    case Typed::STATISTICS: break;
    case Typed::SEGMENT:
        j->seg = segment_out(t.seg);
        if (!read_maps(c, *dst_bytes, n_const, sc, &j->seg)) return -1;
        j->seg.rows = sc->seg.rows;
        break;
    case Typed::SPANS:   // (segmentation's tables and maps)
        j->span = span_out(t.spans);
        if (!read_maps(c, *dst_bytes, n_const, sc, &j->span)) return -1;
        break;
    }
    if (t.reads) cal = sc->cal;   // (else, but for SIGNAL: the constants' table is chunk_slots' or the selects' to fill)
    else if (t.kind != Typed::SIGNAL && !(cal = ensure_array<float2>(c, c->sigmeta, n))) return -1;
    rb.sig.cal = sc->cal = cal, rb.sig.type = t.f->out_type, rb.sig.bias = t.f->is_signed ? 0u : 0x8000u;
    if (t.ranges) rb.sig.rbegin = t.ranges->begin, rb.sig.rend = t.ranges->end, rb.sig.rstats = t.ranges->stats;   // (both tables NULL: un-ranged)
    NormTables nt;   // (ss: for a caller that passed no shift_scale)
    if (t.norm && !ensure_carved(c, c->normmeta, nt, n_const)) return -1;
    if (t.norm) rb.sig.norm = norm_out(t.norm, nt.st, t.shift_scale ? reinterpret_cast<float2*>(t.shift_scale) : nt.ss);
    if (t.with_trim) j->trim = trim_out(t.trim, t.begin);
    return 0;
}

// Front: the launch a batch call owes in front of its groups, each from the final int16 capacities (the headers' sizes when sized)
int typed_front(vbz_gpu_ctx* c, const TypedCall& t, const ReadBatch& rb, const CallScratch& sc)
{
    if (t.kind == Typed::EVENTS || (t.kind == Typed::CHUNKS && t.with_windows)) {   // (the window check, then the pad or the moments' zero)
        Timed tm(c, "window_slots");
        HIPCHK(c, launch_window_check(rb, Pod5Reads(), t.f->offset, t.f->scale, sc.win, c->stream), "window check launch");
        if (t.kind == Typed::EVENTS) HIPCHK(c, launch_event_zero(rb, Pod5Reads(), sc.win, c->stream), "event zero launch");
        else HIPCHK(c, launch_window_pad(rb, Pod5Reads(), sc.win, c->stream), "window pad launch");
    } else if (t.kind == Typed::CHUNKS) {   // (the chunk check)
        Timed tm(c, "chunk_slots");
        HIPCHK(c, launch_chunk_slots(rb.n_reads, rb.dst_cap, t.f->offset, t.f->scale, rb.sig.chunk_len, rb.sig.step, t.chunk_first, t.chunk_rows,
                                     sc.cal, const_cast<uint32_t*>(rb.gate), &rb.sig, c->stream), "chunk slots launch");
    } else if (t.kind == Typed::SEGMENT || t.kind == Typed::SPANS) {   // (the maps' layout)
        Timed tm(c, "segment_layout");
        HIPCHK(c, launch_segment_layout(rb, Pod5Reads(), sc.seg, c->stream), "segment layout launch");
    }
    return 0;
}

// Finish: the launch a call (t, nullable) owes behind everything it has queued, the halves and the routed reads joined; rc: what that returned
// (not 0: nothing owed).  j.rb: its reads, or with pr.reads the rows' streams (inside svb_decode's label; the event finish is the launcher's own)
int typed_finish(vbz_gpu_ctx* c, const TypedCall* t, const DecodeJob& j, const Pod5Reads& pr, const CallScratch& sc, int rc)
{
    if (rc != 0 || !t) return rc;
    std::optional<Timed> tm;
    if (t->kind == Typed::SEGMENT) {   // (count, scan and emit)
        if (!pr.reads) tm.emplace(c, "segment_emit");
        HIPCHK(c, launch_segment_emit(j.rb, pr, j.seg, sc.seg, t->seg_first, t->seg_start, t->seg->start_cap, c->stream), "segment emit launch");
    } else if (t->kind == Typed::SPANS) {   // (count, scan and emit)
        if (!pr.reads) tm.emplace(c, "span_emit");
        HIPCHK(c, launch_span_emit(j.rb, pr, j.span, sc.seg, t->edge_first, t->edge, t->spans->edge_cap, c->stream), "span emit launch");
    } else if (t->kind == Typed::EVENTS) {   // (the records)
        tm.emplace(c, "event_finish");
        HIPCHK(c, launch_event_finish(j.rb, pr, t->f->offset, t->f->scale, sc.win, t->ev_out, c->stream), "event finish launch");
    }
    return 0;
}

// out (nullable): a typed decode that typed_decode has checked (out->f is set)
int decompress_batch_impl(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, bool own_descriptors = false,
                          const TypedCall* out = nullptr)
{
    const uint32_t n = bt->n_reads;
    c->last_frames = 0;
    c->last_span_frames = 0;
    const vbz_gpu_pod5_reads* const reads = out ? out->reads : nullptr;
    hipStream_t s = c->stream;
    if (out && out->kind == Typed::SEGMENT && (reads ? reads->n_reads : n) == 0) HIPCHK(c, hipMemsetAsync(out->seg_first, 0, 8, s), "event_first of no reads");
    if (out && out->kind == Typed::SPANS && (reads ? reads->n_reads : n) == 0) HIPCHK(c, hipMemsetAsync(out->edge_first, 0, 8, s), "edge_first of no reads");
    if (n == 0 && !(reads && reads->n_reads)) return 0;
    DecodeJob job{ to_rb(bt) };
    ReadBatch& rb = job.rb;
    Pod5Reads pr;
    CallScratch sc;
    if (reads && pod5_reads_begin(c, n, reads, reads->read_result, &pr, &sc.cal) != 0) return -1;
    if (n != 0 && !own_descriptors && validate_descriptors(c, bt, &rb) != 0) return -1;
    uint64_t dst_bytes = bt->dst_bytes;
    if (out && typed_outputs(c, bt, *out, &job, &dst_bytes, &sc) != 0) return -1;
    if (sized) {  // vbz.cpp:332-366: strip the header, the original size becomes the exact destination size
        SizedTables h;
        if (!ensure_carved(c, c->meta, h, n)) return -1;
        Timed t(c, "parse_sized");
        HIPCHK(c, launch_parse_sized(n, rb.src, bt->src_off, bt->src_size, rb.dst_cap, rb.gate, h.pay_off, h.pay_size, h.orig_size, h.gate, s),
               "parse_sized launch");
        rb.src_off = h.pay_off;
        rb.src_size = h.pay_size;
        rb.dst_cap = h.orig_size;
        rb.gate = h.gate;
    }
    if (out && !reads && typed_front(c, *out, rb, sc) != 0) return -1;   // (a call over POD5 reads: its plan, in the svb stage)
    const bool by_shape = n != 0 && o->integer_size != 0 && !half_codec(o) && use_segments(c, dst_bytes, n, true);
    if (c->foreign_pending && hipEventQuery(c->ev_foreign.p) == hipSuccess) {   // what the call before this one found (see foreign_host)
        const uint32_t* const found = c->foreign_host.words();
        c->mostly_foreign = 2ull * found[0] > found[1];
        c->foreign_state = found[0] != 0 ? 1 : 0;
        c->foreign_pending = false;
    } else if (c->foreign_pending) {
        (void)hipGetLastError();   // (hipErrorNotReady is not an error to leave behind)
    }
    const bool split = !by_shape && split_applies(c, o, n) && !c->mostly_foreign;
    c->last_split = false;
    if (reads) {
        // The rows go through the entropy stage as any batch's (a split call's halves included; rows are not routed: a read's rows meet
        // again in ONE svb stage behind the join, where the plan, the counting passes over reads and the store see all of them).
        DecodeJob streams = job;   // (what the svb stage over reads decodes: the rows' streams under the call's sig, trim and seg)
        if (n != 0) {
            DecodeJob e{ rb };   // (the entropy stage alone stores nothing and owes no trim or segmentation)
            e.rb.sig = SignalOut();
            const int rc = split ? decompress_split(c, e, dst_bytes, o, &streams.rb) : decompress_group(c, e, dst_bytes, o, by_shape, nullptr, &streams.rb);
            if (rc != 0) return rc;
            streams.rb.sig = rb.sig;
        }
        Timed t(c, "svb_decode");
        if (streams.seg.map) {   // (the pass over reads, then count, scan and emit)
            HIPCHK(c, launch_svb16_segment_reads(streams.rb, pr, streams.seg, sc.seg, s), "svb16 segment (reads) launch");
            return typed_finish(c, out, streams, pr, sc, 0);
        }
        HIPCHK(c, launch_svb16_decode_reads(streams.rb, pr, out->f->offset, out->f->scale, out->chunk_rows, s, streams.trim.begin ? &streams.trim : nullptr,
                                            sc.win.scan ? &sc.win : nullptr, out->ev_out, streams.span.map ? &streams.span : nullptr, &sc.seg),
               "svb16_decode (reads) launch");
        return streams.span.map ? typed_finish(c, out, streams, pr, sc, 0) : 0;   // (a span call: count, scan and emit behind the pass over reads)
    }
    if (by_shape || !routing_applies(c, o, dst_bytes, n))
        return typed_finish(c, out, job, pr, sc, split ? decompress_split(c, job, dst_bytes, o) : decompress_group(c, job, dst_bytes, o, by_shape));
    Routed r;
    if (route(c, rb, rb.dst_cap, &r, job.trim, job.seg, job.span) != 0) return -1;   // by the decoded size
    DecodeJob small = job;
    small.rb.gate = r.gate_small;
    int rc = 0;   // (as in compress_batch_impl: the second stream is joined whatever happens)
    if (decompress_group(c->large, r.large, ROUTE_MAX_BYTES, o, true) != 0) rc = -1;
    if (rc == 0 && (split ? decompress_split(c, small, dst_bytes, o) : decompress_group(c, small, dst_bytes, o, false)) != 0) rc = -1;
    if (rc != 0 && c->error.empty() && !c->large->error.empty()) c->error = c->large->error;
    if (route_join(c, r, bt->result) != 0) rc = -1;
    return typed_finish(c, out, job, pr, sc, rc);
}

// A fused match call that has passed every check: the window call of one row per read at start 0 (L = N, pad +0) into the caller's query
// arena, under the library's own tables; valid[] from the verdicts it leaves and the range tables; the match launch.  Over POD5 reads the
// verdicts are read_result's (the call's own table when the caller takes none): a bad first_row leaves an error in every entry, the window
// call writes nothing, and every hit is the empty verdict.
int match_decode(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, TypedCall& t, uint32_t n_out)
{
    const AlignView& m = t.match;
    const uint32_t N = m.query_len;
    MatchTables tab;
    if (!ensure_carved(c, c->matchmeta, tab, n_out)) return -1;
    {
        Timed tm(c, "match_tables");
        HIPCHK(c, launch_match_windows(n_out, tab.first, tab.start, c->stream), "match tables launch");
    }
    const vbz_gpu_windows win = { N, 0.0f, n_out, tab.first, tab.start, 0, 0 };
    vbz_gpu_pod5_reads reads;
    if (t.pod5) {
        reads = *t.reads;
        if (!reads.read_result) reads.read_result = tab.read_result;
        t.reads = &reads;
    }
    t.windows(&win, t.match_query);
    const int rc = decompress_batch_impl(c, bt, o, t.sized, false, &t);
    if (rc != 0) return rc;
    Timed tm(c, "match");
    HIPCHK(c, launch_match_valid(n_out, t.pod5 ? reads.read_result : bt->result, t.ranges ? t.ranges->begin : nullptr, t.ranges ? t.ranges->end : nullptr,
                                 N, tab.valid, c->stream), "match valid launch");
    HIPCHK(c, (t.match_span ? t.align->span : t.align->hit)(n_out, t.match_query, tab.valid, N, m.quant, m.levels, m.levels_len, m.n_levels, m.levels_stride,
                                                             t.match_out, c->stream),
           t.align->hit_launch);
    return 0;
}

// The one way into a typed decode: every check of every entry, in this order, then the decode.  A call with one fault gets that fault's
// message; with several, the first in this order.
int typed_decode(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, const TypedCall& call)
{
    static const char* const WHAT[] = { "signal", "chunk", "statistics", "event", "segmentation", "span" };
    if (!c || !bt) return -1;                                                                                        // 1
    DeviceGuard dg(c->device);                                                                                       // 2
    TypedCall t = call;
    const bool stats = t.kind == Typed::STATISTICS || t.kind == Typed::SEGMENT || t.kind == Typed::SPANS;   // (no format: is_signed alone)
    const bool type_ok = stats || (t.f && t.f->out_type >= VBZ_GPU_SIGNAL_F32 && t.f->out_type <= VBZ_GPU_SIGNAL_BF16);
    if (!typed_args_ok(c, o, t.sized, WHAT[(int)t.kind], type_ok, stats ? t.is_signed : t.f ? t.f->is_signed : 0u)) return -2;   // 3
    if (t.pod5 && !pod5_reads_ok(c, o, t.reads)) return -2;                                                         // 4
    if ((t.norm || t.norm_null != Null::ALLOWED) && !norm_ok(c, t.norm, t.f)) return -2;                            // 5
    if (!ranges_ok(c, t.ranges)) return -2;                                                                          // 6
    const uint32_t n_out = t.pod5 ? t.reads->n_reads : bt->n_reads;   // the reads the per-read tables have an entry for
    if (t.with_trim && !trim_ok(c, t.trim, t.begin)) return -2;                                                      // 7
    if (t.kind == Typed::SEGMENT && !segmentation_ok(c, t.seg, t.seg_first, t.seg_start)) return -2;                 // 7 (a segmentation in the trim's place)
    if (t.kind == Typed::SPANS && !spans_ok(c, t.spans, t.edge_first, t.edge, t.norm != nullptr)) return -2;         // 7 (spans, likewise)
    if (!t.shift_scale && (t.shift_scale_null == Null::REFUSED || (t.shift_scale_null == Null::REFUSED_WITH_READS && n_out != 0))) {
        set_error(c, "shift_scale is NULL");
        return -2;
    }
    if (t.kind == Typed::EVENTS) {                                                                                   // 8 (events)
        if (!events_ok(c, t.ev, t.f, t.ev_out, t.ev_moments, n_out)) return -2;
    } else if (t.kind == Typed::CHUNKS && t.with_match) {                                                            // 8 (a match in place of a chunking)
        const size_t hit_bytes = t.match_span ? sizeof(vbz_gpu_match_span) : sizeof(vbz_gpu_match_hit);
        if (!align_ok(c, *t.align, t.match, t.match_query, t.match_out, hit_bytes, n_out)) return -2;
        if (t.f->out_type != VBZ_GPU_SIGNAL_F32) {
            set_error(c, "the query of a match is float32 (out_type %u)", t.f->out_type);
            return -2;
        }
    } else if (t.kind == Typed::CHUNKS && t.with_windows) {                                                          // 8 (windows in place of a chunking)
        if (!windows_ok(c, t.win, t.win_out, n_out, t.f->out_type == VBZ_GPU_SIGNAL_F32 ? 4u : 2u)) return -2;
    } else if (t.kind == Typed::CHUNKS) {
        if (!chunking_ok(c, t.ch)) return -2;
        if (n_out != 0 && (!t.chunk_first || !t.chunks)) {
            set_error(c, "chunk_first or the chunk arena is NULL");
            return -2;
        }
        if (((uintptr_t)t.chunks & 15u) != 0) {
            set_error(c, "the chunk arena is not 16-byte aligned");
            return -2;
        }
        const uint64_t row_bytes = (uint64_t)t.ch->chunk_len * (t.f->out_type == VBZ_GPU_SIGNAL_F32 ? 4u : 2u);
        if (t.chunk_rows > EXTENT_MAX / row_bytes) {
            set_error(c, "declared chunk arena is not plausible (%llu rows of %llu bytes)", (unsigned long long)t.chunk_rows, (unsigned long long)row_bytes);
            return -2;
        }
    }
    // 9. batch->dst is an arena of a SIGNAL decode alone: a chunk decode stores into `chunks` and the statistics store nothing, so their
    // callers may leave it NULL beside the dst_bytes of the int16 layout that describes the reads.  plausible_extents, which refuses a
    // NULL arena of a declared size, therefore sees a batch whose dst is not NULL; the decode gets the caller's batch and reads no dst.
    vbz_gpu_batch b = *bt;
    if (t.kind != Typed::SIGNAL) b.dst = &b;
    if (!plausible_extents(c, &b)) return -2;                                                                        // 10
    const vbz_gpu_signal_format none = { SIG_NONE, t.is_signed, nullptr, nullptr };
    if (stats) t.f = &none;
    if (t.with_match) return match_decode(c, bt, o, t, n_out);                                                       // 11 (the window call, then the match)
    return decompress_batch_impl(c, bt, o, t.sized, false, &t);                                                      // 11
}

// A stage call on a query arena the caller filled (vbz_gpu_*_match_batch, ..._locate_batch and their span forms): the checks, then the launch
int align_stage(vbz_gpu_ctx* c, const AlignKind& k, const AlignView& m, uint32_t n_reads, const float* query, const uint32_t* valid, void* out, bool span)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (!align_ok(c, k, m, query, out, span ? sizeof(vbz_gpu_match_span) : sizeof(vbz_gpu_match_hit), n_reads)) return -2;
    if (n_reads != 0 && !valid) {
        set_error(c, "valid is NULL");
        return -2;
    }
    Timed t(c, k.name);
    HIPCHK(c, (span ? k.span : k.hit)(n_reads, query, valid, m.query_len, m.quant, m.levels, m.levels_len, m.n_levels, m.levels_stride, out, c->stream),
           span ? k.span_launch : k.hit_launch);
    return 0;
}

// The path call of a match or a locate: the view's and the path struct's rules, the tables a call with pairs needs, the extents, then the
// groups -- forward launch and traceback -- over the context's scratch.  The rows of the cost matrix are the operand in the lanes: a pair
// owns ref_stride rows of a match and query_len of a locate.  A match takes valid == NULL (every row has N samples); a locate refuses it.
int path_call(vbz_gpu_ctx* c, const AlignKind& k, const AlignView& m, uint32_t n_pairs, uint32_t n_reads, const float* query, const uint32_t* valid,
              const vbz_gpu_match_pair* pairs, const vbz_gpu_match_path* path, vbz_gpu_match_span* hit, vbz_gpu_match_row* rows)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    // (the view's own rules, the levels' extent and the alignment of the levels, query and hit; the tables a call with pairs needs: below)
    if (!align_ok(c, k, m, query, hit, sizeof(vbz_gpu_match_span), 0)) return -2;
    if (!path || path->flags != 0 || path->reserved != 0 || path->max_width < 8 || path->max_width > 65536 || path->max_width % 8 != 0) {
        set_error(c, "path is NULL or outside the rules (max_width %u, flags %u)", path ? path->max_width : 0u, path ? path->flags : 0u);
        return -2;
    }
    if (n_pairs != 0 && (!m.levels || !m.levels_len || !query || (!valid && k.query_in_lanes) || !pairs || !hit || !rows)) {
        set_error(c, "%s, %s_len, the query arena, %sthe pair table, the hit table or the row arena is NULL", k.level, k.level, k.query_in_lanes ? "valid, " : "");
        return -2;
    }
    if ((((uintptr_t)pairs | (uintptr_t)rows) & 15u) != 0) {
        set_error(c, "the pair table or the row arena is not 16-byte aligned");
        return -2;
    }
    const uint32_t rows_stride = k.query_in_lanes ? m.query_len : m.levels_stride;
    if ((uint64_t)n_pairs * rows_stride > EXTENT_MAX / sizeof(vbz_gpu_match_row) || (uint64_t)n_reads * m.query_len > EXTENT_MAX / sizeof(float)) {
        set_error(c, "declared path arenas are not plausible (%u pairs, %u reads)", n_pairs, n_reads);
        return -2;
    }
    if (n_pairs == 0) return 0;
    AlignPathArgs a{};
    a.query = query, a.valid = valid, a.n_reads = n_reads, a.N = m.query_len, a.quant = m.quant;
    a.levels = m.levels, a.levels_len = m.levels_len, a.n_levels = m.n_levels, a.levels_stride = m.levels_stride;
    a.pairs = reinterpret_cast<const uint4*>(pairs), a.max_width = path->max_width;
    a.pair_words = match_path_pair_words(a.max_width, rows_stride);
    a.hit = reinterpret_cast<uint4*>(hit), a.rows = reinterpret_cast<uint2*>(rows);
    const uint32_t group = match_path_group_pairs(n_pairs, a.max_width, rows_stride, c->knobs.match_path_cap);
    MatchPathScratch sc;
    if (!ensure_carved(c, c->matchpath, sc, group, a.pair_words)) return -1;
    a.bits = sc.bits, a.cost = sc.cost;
    for (uint32_t first = 0; first < n_pairs; first += group) {   // (the groups share the scratch: the stream orders them)
        a.first = first, a.count = n_pairs - first < group ? n_pairs - first : group;
        {
            Timed t(c, k.forward_entry);
            HIPCHK(c, k.path_forward(a, c->stream), k.forward_launch);
        }
        Timed t(c, k.trace_entry);
        HIPCHK(c, k.path_trace(a, c->stream), k.trace_launch);
    }
    return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// vbz_gpu.h
// ------------------------------------------------------------------------------------------------
extern "C" {

#ifdef VBZ_EXPERIMENTS
const char* vbz_gpu_version(void) { return "vbz_hip 0.6.0 gfx950 +experiments"; }
#else
const char* vbz_gpu_version(void) { return "vbz_hip 0.6.0 gfx950"; }
#endif

vbz_gpu_ctx* vbz_gpu_create(int device, void* stream)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error(nullptr, "no HIP device available (%s); this library has no CPU path", hipGetErrorString(e));
        return nullptr;
    }
    if (device < 0 || device >= count) {
        set_error(nullptr, "device %d out of range (%d devices)", device, count);
        return nullptr;
    }
    DeviceGuard dg(device);
    {
        int now = -1;
        if (hipGetDevice(&now) != hipSuccess || now != device) {
            set_error(nullptr, "hipSetDevice(%d) failed", device);
            return nullptr;
        }
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            set_error(nullptr, "device %d is %s; this library carries gfx950 (MI355X) code objects only", device, prop.gcnArchName);
            return nullptr;
        }
    }
    vbz_gpu_ctx* c = new vbz_gpu_ctx();
    c->device = device;
    // The knobs of the shipped library (README.md): every one selects between paths the suites run.  The timed kernel
    // instantiations are compiled into the experiments build only (-DVBZ_EXPERIMENTS: lib/libvbz_hip_x.so, for tools/);
    // here VBZ_HIP_PHASE_TIMING does nothing.
    if (const char* e = getenv("VBZ_HIP_TRACE")) c->knobs.trace = atoi(e) != 0;
    if (const char* e = getenv("VBZ_HIP_ZERO_RUN_SEQUENCES")) c->knobs.zero_run_sequences = atoi(e) != 0;
    if (const char* e = getenv("VBZ_HIP_LONG_REPEATS")) c->knobs.long_repeats = atoi(e) != 0;
    if (const char* e = getenv("VBZ_HIP_FAST_DECODE")) c->knobs.fast_decode = atoi(e) != 0;
    if (const char* e = getenv("VBZ_HIP_REF_CHAINS")) c->knobs.ref_chains = atoi(e);
    if (const char* e = getenv("VBZ_HIP_STAGED_ENCODE")) c->knobs.staged_encode = atoi(e) != 0;
    if (const char* e = getenv("VBZ_HIP_SHARED_TABLES")) c->knobs.shared_tables = atoi(e) != 0;
    if (const char* e = getenv("VBZ_HIP_ROUTING")) c->knobs.routing = atoi(e) != 0;
    if (const char* e = getenv("VBZ_HIP_SEGMENTED")) c->knobs.segmented = atoi(e) != 0;
    if (const char* e = getenv("VBZ_HIP_SEG_SELF_MAX")) c->knobs.seg_self_max = (uint32_t)strtoul(e, nullptr, 10);
    if (const char* e = getenv("VBZ_HIP_TRAILERS")) c->knobs.trailers = atoi(e) != 0;
    if (const char* e = getenv("VBZ_HIP_CANONICAL")) c->knobs.canonical = atoi(e) != 0;
    if (const char* e = getenv("VBZ_HIP_CHECKSUM")) c->knobs.checksum = atoi(e) != 0;
    if (const char* e = getenv("VBZ_HIP_MATCH_PATH_CAP")) vbz_gpu_set_match_path_cap(c, strtoull(e, nullptr, 10));
    if (const char* e = getenv("VBZ_HIP_SPLIT_MIN")) c->knobs.split_min = (uint32_t)strtoul(e, nullptr, 10);   // 0: a batch is never coded as two halves
#ifdef VBZ_EXPERIMENTS
    if (const char* e = getenv("VBZ_HIP_PHASE_TIMING")) c->knobs.phase_timing = atoi(e);   // timed instantiations of the entropy kernels
#endif
    {
        std::vector<uint8_t> host(seq_tables_bytes());
        seq_tables_build(host.data());
        if (!ensure(c, c->seqtab, host.size()) ||
            hipMemcpy(c->seqtab.p, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
            set_error(nullptr, "could not upload the sequence tables");
            vbz_gpu_destroy(c);
            return nullptr;
        }
        std::vector<uint8_t> hostd(seq_dtables_bytes());
        seq_dtables_build(hostd.data());
        if (!ensure(c, c->seqdtab, hostd.size()) ||
            hipMemcpy(c->seqdtab.p, hostd.data(), hostd.size(), hipMemcpyHostToDevice) != hipSuccess) {
            set_error(nullptr, "could not upload the sequence decoding tables");
            vbz_gpu_destroy(c);
            return nullptr;
        }
    }
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        if (hipStreamCreateWithFlags(&c->own_stream.p, hipStreamNonBlocking) != hipSuccess) {
            set_error(nullptr, "hipStreamCreate failed");
            c->own_stream.p = nullptr;
            vbz_gpu_destroy(c);  // frees the uploaded tables as well
            return nullptr;
        }
        c->stream = c->own_stream.p;
    }
    return c;
}

void vbz_gpu_destroy(vbz_gpu_ctx* c)
{
    if (!c) return;
    DeviceGuard dg(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;   // (every member frees what it holds, the children and then the stream last: see vbz_gpu_ctx)
}

void* vbz_gpu_stream(vbz_gpu_ctx* c) { return c ? (void*)c->stream : nullptr; }

void vbz_gpu_set_trailers(vbz_gpu_ctx* c, int enable)
{
    if (c) c->knobs.trailers = enable != 0;
}
void vbz_gpu_set_canonical(vbz_gpu_ctx* c, int enable)
{
    if (c) c->knobs.canonical = enable != 0;
}
void vbz_gpu_set_checksum(vbz_gpu_ctx* c, int enable)
{
    if (c) c->knobs.checksum = enable != 0;
}
void vbz_gpu_set_match_path_cap(vbz_gpu_ctx* c, uint64_t bytes)
{
    if (c) c->knobs.match_path_cap = bytes != 0 ? bytes : MATCH_PATH_CAP_DEFAULT;
}
const char* vbz_gpu_last_error(vbz_gpu_ctx* c) { return c ? c->error.c_str() : "no context"; }

int vbz_gpu_synchronize(vbz_gpu_ctx* c)
{
    if (!c) return -1;
    HIPCHK(c, hipStreamSynchronize(c->stream), "stream synchronize");
    return 0;
}

int vbz_gpu_compress_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized)
{
    if (!c || !bt || !o) return -1;
    DeviceGuard dg(c->device);
    if (!batch_options_ok(o, sized)) {
        set_error(c, "unsupported options (integer_size=%u version=%u sized=%d level=%d zigzag=%d)", o->integer_size, o->vbz_version, sized,
                  o->zstd_compression_level, (int)o->perform_delta_zig_zag);
        return -2;
    }
    if (!plausible_extents(c, bt)) return -2;
    return compress_batch_impl(c, bt, o, sized);
}

int vbz_gpu_decompress_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized)
{
    if (!c || !bt || !o) return -1;
    DeviceGuard dg(c->device);
    if (!batch_options_ok(o, sized)) {
        set_error(c, "unsupported options (integer_size=%u version=%u sized=%d level=%d zigzag=%d)", o->integer_size, o->vbz_version, sized,
                  o->zstd_compression_level, (int)o->perform_delta_zig_zag);
        return -2;
    }
    if (!plausible_extents(c, bt)) return -2;
    return decompress_batch_impl(c, bt, o, sized);
}

int vbz_gpu_chunk_layout_batch(vbz_gpu_ctx* c, uint32_t n, const uint32_t* samples, const vbz_gpu_chunking* ch, uint64_t* chunk_first,
                               uint32_t* chunk_info, uint64_t info_cap)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (!chunking_ok(c, ch)) return -2;
    if (!chunk_first || (n != 0 && !samples)) {
        set_error(c, "a table of the chunk layout call is NULL");
        return -2;
    }
    uint32_t* const counts = ensure_array<uint32_t>(c, c->chunkmeta, n);
    if (!counts) return -1;
    Timed t(c, "chunk_layout");
    HIPCHK(c, launch_chunk_layout(n, samples, ch->chunk_len, ch->step, counts, chunk_first, c->stream),
           "chunk layout launch");
    HIPCHK(c, launch_chunk_info(n, samples, ch->chunk_len, ch->step, ch->mode, ch->end_align, chunk_first, chunk_info, info_cap, c->stream),
           "chunk info launch");
    return 0;
}

int vbz_gpu_range_samples_batch(vbz_gpu_ctx* c, uint32_t n, const uint32_t* samples, const vbz_gpu_sample_ranges* ranges, uint32_t* range_samples)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (!ranges_ok(c, ranges)) return -2;
    if (n != 0 && (!samples || !range_samples)) {
        set_error(c, "a table of the range samples call is NULL");
        return -2;
    }
    Timed t(c, "range_samples");
    HIPCHK(c, launch_range_samples(n, samples, ranges ? ranges->begin : nullptr, ranges ? ranges->end : nullptr, range_samples, c->stream),
           "range samples launch");
    return 0;
}

int vbz_gpu_pod5_read_samples_batch(vbz_gpu_ctx* c, uint32_t n_rows, const uint32_t* row_samples, const vbz_gpu_pod5_reads* reads, uint32_t* read_samples)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (!pod5_reads_ok(c, nullptr, reads)) return -2;
    if ((n_rows != 0 && !row_samples) || (reads->n_reads != 0 && !read_samples)) {
        set_error(c, "row_samples or read_samples is NULL");
        return -2;
    }
    Pod5Reads pr;
    float2* cal;
    if (pod5_reads_begin(c, n_rows, reads, read_samples, &pr, &cal) != 0) return -1;
    HIPCHK(c, launch_pod5_read_samples(pr, row_samples, read_samples, c->stream), "pod5 read samples launch");
    return 0;
}

// The twenty-four typed decodes.  Every entry fills a TypedCall and returns typed_decode's verdict; none has a check of its own.
//
//   vbz_gpu_..._batch             kind        sized  chunking  norm      shift_scale          ranges    reads  trim   (chunking "windows": a
//                                                                                                                   vbz_gpu_windows in its place;
//                                                                                                                   "events": a vbz_gpu_events)
//   decompress_signal             SIGNAL      arg    -         -         -                    -         -      -
//   decompress_signal_norm        SIGNAL      arg    -         required  nullable             -         -      -
//   decompress_chunks             CHUNKS      arg    yes       -         -                    -         -      -
//   decompress_chunks_norm        CHUNKS      arg    yes       required  nullable             -         -      -
//   decompress_chunks_range       CHUNKS      arg    yes       nullable  nullable             nullable  -      -
//   decompress_windows            CHUNKS      arg    windows   nullable  nullable             nullable  -      -
//   signal_events                 EVENTS      arg    events    nullable  nullable             nullable  -      -
//   signal_norm                   STATISTICS  arg    -         required  required             -         -      -
//   signal_norm_range             STATISTICS  arg    -         required  required             nullable  -      -
//   signal_trim                   STATISTICS  arg    -         required  nullable             nullable  -      yes
//   signal_segment                SEGMENT     arg    -         -         -                    nullable  -      segmentation (in the trim's place)
//   pod5_decompress_signal_norm   SIGNAL      0      -         required  nullable             -         yes    -
//   pod5_decompress_chunks        CHUNKS      0      yes       nullable  nullable             -         yes    -
//   pod5_decompress_chunks_range  CHUNKS      0      yes       nullable  nullable             nullable  yes    -
//   pod5_decompress_windows       CHUNKS      0      windows   nullable  nullable             nullable  yes    -
//   pod5_signal_events            EVENTS      0      events    nullable  nullable             nullable  yes    -
//   pod5_signal_norm              STATISTICS  0      -         required  required with reads  -         yes    -
//   pod5_signal_norm_range        STATISTICS  0      -         required  required with reads  nullable  yes    -
//   pod5_signal_trim              STATISTICS  0      -         required  nullable             nullable  yes    yes
//   pod5_signal_segment           SEGMENT     0      -         -         -                    nullable  yes    segmentation
//   signal_spans                  SPANS       arg    -         nullable  nullable             nullable  -      spans (in the trim's place)
//   pod5_signal_spans             SPANS       0      -         nullable  nullable             nullable  yes    spans
//   signal_match                  CHUNKS      arg    match     nullable  nullable             nullable  -      -      (match: the library's own
//   pod5_signal_match             CHUNKS      0      match     nullable  nullable             nullable  yes    -       windows, then match.hip)
//   signal_match_span             CHUNKS      arg    match     nullable  nullable             nullable  -      -      (as signal_match: 16-byte hits,
//   pod5_signal_match_span        CHUNKS      0      match     nullable  nullable             nullable  yes    -       the span launch in its place)
//   signal_locate                 CHUNKS      arg    locate    nullable  nullable             nullable  -      -      (as signal_match: a vbz_gpu_locate,
//   pod5_signal_locate            CHUNKS      0      locate    nullable  nullable             nullable  yes    -       the locate launch in its place)
//   signal_locate_span            CHUNKS      arg    locate    nullable  nullable             nullable  -      -      (as signal_locate: 16-byte hits,
//   pod5_signal_locate_span       CHUNKS      0      locate    nullable  nullable             nullable  yes    -       the locate span launch in its place)
//
// The NULL rules that differ between entries, kept as they were when the entries were written one by one:
// - shift_scale of the statistics alone: `required` refuses a NULL in a call of no reads too; `required with reads` (the POD5 twins)
//   only when reads->n_reads != 0.
// - norm: NULL is a chunk decode without normalisation in decompress_chunks_range, the POD5 chunk entries and the two window entries,
//   records under the format's constants in the two event entries, and a fault everywhere else.
// - chunk_first and the chunk arena may be NULL when there is no read to store: batch->n_reads == 0, or, over POD5 reads,
//   reads->n_reads == 0 (whatever the number of rows).  The window entries: window_first, start (with window_rows != 0) and the arena, likewise;
//   the event entries: event_first, start (with event_rows != 0) and the event arena.
// - the segmentation entries: event_first is never NULL (a call of no reads writes event_first[0]); start is NULL exactly in the
//   count-only call (start_cap == 0).
// - the span entries: edge_first and edge, likewise; norm NULL means the constants are the caller's (spans->level, which must then be
//   there and must not be otherwise); a shift_scale without a norm is ignored.
int vbz_gpu_decompress_signal_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, const vbz_gpu_signal_format* f)
{
    return typed_decode(c, bt, o, TypedCall(Typed::SIGNAL, sized).format(f));
}

int vbz_gpu_decompress_signal_norm_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, const vbz_gpu_signal_format* f,
                                         const vbz_gpu_normalization* norm, float* shift_scale)
{
    return typed_decode(c, bt, o, TypedCall(Typed::SIGNAL, sized).format(f).normalise(norm, Null::REFUSED, shift_scale, Null::ALLOWED));
}

int vbz_gpu_decompress_chunks_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, const vbz_gpu_signal_format* f,
                                    const vbz_gpu_chunking* ch, const uint64_t* chunk_first, void* chunks, uint64_t chunk_rows)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, sized).format(f).chunking(ch, chunk_first, chunks, chunk_rows));
}

int vbz_gpu_decompress_chunks_norm_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, const vbz_gpu_signal_format* f,
                                         const vbz_gpu_chunking* ch, const uint64_t* chunk_first, void* chunks, uint64_t chunk_rows,
                                         const vbz_gpu_normalization* norm, float* shift_scale)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, sized).format(f).chunking(ch, chunk_first, chunks, chunk_rows)
                                      .normalise(norm, Null::REFUSED, shift_scale, Null::ALLOWED));
}

int vbz_gpu_decompress_chunks_range_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, const vbz_gpu_signal_format* f,
                                          const vbz_gpu_chunking* ch, const uint64_t* chunk_first, void* chunks, uint64_t chunk_rows,
                                          const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, sized).format(f).chunking(ch, chunk_first, chunks, chunk_rows)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_decompress_windows_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, const vbz_gpu_signal_format* f,
                                     const vbz_gpu_windows* windows, void* out, const vbz_gpu_normalization* norm, float* shift_scale,
                                     const vbz_gpu_sample_ranges* ranges)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, sized).format(f).windows(windows, out)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_signal_events_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, const vbz_gpu_signal_format* f,
                                const vbz_gpu_events* events, vbz_gpu_event* out, vbz_gpu_event_moments* moments, const vbz_gpu_normalization* norm,
                                float* shift_scale, const vbz_gpu_sample_ranges* ranges)
{
    return typed_decode(c, bt, o, TypedCall(Typed::EVENTS, sized).format(f).events(events, out, moments)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_signal_norm_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, uint32_t is_signed,
                              const vbz_gpu_normalization* norm, float* shift_scale)
{
    return typed_decode(c, bt, o, TypedCall(Typed::STATISTICS, sized).statistics(is_signed).normalise(norm, Null::REFUSED, shift_scale, Null::REFUSED));
}

int vbz_gpu_signal_norm_range_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, uint32_t is_signed,
                                    const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges)
{
    return typed_decode(c, bt, o, TypedCall(Typed::STATISTICS, sized).statistics(is_signed).normalise(norm, Null::REFUSED, shift_scale, Null::REFUSED)
                                      .range(ranges));
}

int vbz_gpu_signal_trim_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, uint32_t is_signed,
                              const vbz_gpu_normalization* norm, const vbz_gpu_sample_ranges* ranges, const vbz_gpu_trim* trim, float* shift_scale,
                              uint32_t* begin)
{
    return typed_decode(c, bt, o, TypedCall(Typed::STATISTICS, sized).statistics(is_signed).normalise(norm, Null::REFUSED, shift_scale, Null::ALLOWED)
                                      .range(ranges).trimmed(trim, begin));
}

// ---- POD5 reads of several rows ------------------------------------------------------------------------------------------------------
int vbz_gpu_pod5_decompress_signal_norm_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, const vbz_gpu_signal_format* f,
                                              const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm, float* shift_scale)
{
    return typed_decode(c, bt, o, TypedCall(Typed::SIGNAL, 0).format(f).pod5_reads(reads).normalise(norm, Null::REFUSED, shift_scale, Null::ALLOWED));
}

int vbz_gpu_pod5_decompress_chunks_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, const vbz_gpu_signal_format* f,
                                         const vbz_gpu_chunking* ch, const vbz_gpu_pod5_reads* reads, const uint64_t* chunk_first, void* chunks,
                                         uint64_t chunk_rows, const vbz_gpu_normalization* norm, float* shift_scale)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, 0).format(f).pod5_reads(reads).chunking(ch, chunk_first, chunks, chunk_rows)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED));
}

int vbz_gpu_pod5_decompress_chunks_range_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, const vbz_gpu_signal_format* f,
                                               const vbz_gpu_chunking* ch, const vbz_gpu_pod5_reads* reads, const uint64_t* chunk_first, void* chunks,
                                               uint64_t chunk_rows, const vbz_gpu_normalization* norm, float* shift_scale,
                                               const vbz_gpu_sample_ranges* ranges)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, 0).format(f).pod5_reads(reads).chunking(ch, chunk_first, chunks, chunk_rows)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_pod5_decompress_windows_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, const vbz_gpu_signal_format* f,
                                          const vbz_gpu_pod5_reads* reads, const vbz_gpu_windows* windows, void* out,
                                          const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, 0).format(f).pod5_reads(reads).windows(windows, out)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_pod5_signal_events_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, const vbz_gpu_signal_format* f,
                                     const vbz_gpu_pod5_reads* reads, const vbz_gpu_events* events, vbz_gpu_event* out, vbz_gpu_event_moments* moments,
                                     const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges)
{
    return typed_decode(c, bt, o, TypedCall(Typed::EVENTS, 0).format(f).pod5_reads(reads).events(events, out, moments)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_pod5_signal_norm_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, uint32_t is_signed,
                                   const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm, float* shift_scale)
{
    return typed_decode(c, bt, o, TypedCall(Typed::STATISTICS, 0).statistics(is_signed).pod5_reads(reads)
                                      .normalise(norm, Null::REFUSED, shift_scale, Null::REFUSED_WITH_READS));
}

int vbz_gpu_pod5_signal_norm_range_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, uint32_t is_signed,
                                         const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm, float* shift_scale,
                                         const vbz_gpu_sample_ranges* ranges)
{
    return typed_decode(c, bt, o, TypedCall(Typed::STATISTICS, 0).statistics(is_signed).pod5_reads(reads)
                                      .normalise(norm, Null::REFUSED, shift_scale, Null::REFUSED_WITH_READS).range(ranges));
}

int vbz_gpu_pod5_signal_trim_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, uint32_t is_signed,
                                   const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm, const vbz_gpu_sample_ranges* ranges,
                                   const vbz_gpu_trim* trim, float* shift_scale, uint32_t* begin)
{
    return typed_decode(c, bt, o, TypedCall(Typed::STATISTICS, 0).statistics(is_signed).pod5_reads(reads)
                                      .normalise(norm, Null::REFUSED, shift_scale, Null::ALLOWED).range(ranges).trimmed(trim, begin));
}

int vbz_gpu_signal_segment_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, uint32_t is_signed,
                                 const vbz_gpu_sample_ranges* ranges, const vbz_gpu_segmentation* segmentation, uint64_t* event_first, uint32_t* start)
{
    return typed_decode(c, bt, o, TypedCall(Typed::SEGMENT, sized).statistics(is_signed).range(ranges).segmented(segmentation, event_first, start));
}

int vbz_gpu_pod5_signal_segment_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, uint32_t is_signed,
                                      const vbz_gpu_pod5_reads* reads, const vbz_gpu_sample_ranges* ranges, const vbz_gpu_segmentation* segmentation,
                                      uint64_t* event_first, uint32_t* start)
{
    return typed_decode(c, bt, o, TypedCall(Typed::SEGMENT, 0).statistics(is_signed).pod5_reads(reads).range(ranges)
                                      .segmented(segmentation, event_first, start));
}

int vbz_gpu_signal_spans_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, uint32_t is_signed,
                               const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges, const vbz_gpu_spans* spans,
                               uint64_t* edge_first, uint32_t* edge)
{
    return typed_decode(c, bt, o, TypedCall(Typed::SPANS, sized).statistics(is_signed).normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED)
                                      .range(ranges).spanned(spans, edge_first, edge));
}

int vbz_gpu_pod5_signal_spans_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, uint32_t is_signed,
                                    const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm, float* shift_scale,
                                    const vbz_gpu_sample_ranges* ranges, const vbz_gpu_spans* spans, uint64_t* edge_first, uint32_t* edge)
{
    return typed_decode(c, bt, o, TypedCall(Typed::SPANS, 0).statistics(is_signed).pod5_reads(reads).normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED)
                                      .range(ranges).spanned(spans, edge_first, edge));
}

int vbz_gpu_match_batch(vbz_gpu_ctx* c, uint32_t n_reads, const float* query, const uint32_t* valid, const vbz_gpu_match* match, vbz_gpu_match_hit* out)
{
    return align_stage(c, MATCH, align_view(match), n_reads, query, valid, out, false);
}

int vbz_gpu_signal_match_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, const vbz_gpu_signal_format* f,
                               const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges, const vbz_gpu_match* match,
                               float* query, vbz_gpu_match_hit* out)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, sized).format(f).aligned(MATCH, align_view(match), query, out)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_pod5_signal_match_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, const vbz_gpu_signal_format* f,
                                    const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm, float* shift_scale,
                                    const vbz_gpu_sample_ranges* ranges, const vbz_gpu_match* match, float* query, vbz_gpu_match_hit* out)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, 0).format(f).pod5_reads(reads).aligned(MATCH, align_view(match), query, out)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_match_span_batch(vbz_gpu_ctx* c, uint32_t n_reads, const float* query, const uint32_t* valid, const vbz_gpu_match* match, vbz_gpu_match_span* out)
{
    return align_stage(c, MATCH, align_view(match), n_reads, query, valid, out, true);
}

int vbz_gpu_signal_match_span_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, const vbz_gpu_signal_format* f,
                                    const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges, const vbz_gpu_match* match,
                                    float* query, vbz_gpu_match_span* out)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, sized).format(f).aligned(MATCH, align_view(match), query, out)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_pod5_signal_match_span_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, const vbz_gpu_signal_format* f,
                                         const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm, float* shift_scale,
                                         const vbz_gpu_sample_ranges* ranges, const vbz_gpu_match* match, float* query, vbz_gpu_match_span* out)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, 0).format(f).pod5_reads(reads).aligned(MATCH, align_view(match), query, out)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_locate_batch(vbz_gpu_ctx* c, uint32_t n_reads, const float* query, const uint32_t* valid, const vbz_gpu_locate* locate, vbz_gpu_match_hit* out)
{
    return align_stage(c, LOCATE, align_view(locate), n_reads, query, valid, out, false);
}

int vbz_gpu_signal_locate_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, const vbz_gpu_signal_format* f,
                                const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges, const vbz_gpu_locate* locate,
                                float* query, vbz_gpu_match_hit* out)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, sized).format(f).aligned(LOCATE, align_view(locate), query, out)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_pod5_signal_locate_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, const vbz_gpu_signal_format* f,
                                     const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm, float* shift_scale,
                                     const vbz_gpu_sample_ranges* ranges, const vbz_gpu_locate* locate, float* query, vbz_gpu_match_hit* out)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, 0).format(f).pod5_reads(reads).aligned(LOCATE, align_view(locate), query, out)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_locate_span_batch(vbz_gpu_ctx* c, uint32_t n_reads, const float* query, const uint32_t* valid, const vbz_gpu_locate* locate,
                              vbz_gpu_match_span* out)
{
    return align_stage(c, LOCATE, align_view(locate), n_reads, query, valid, out, true);
}

int vbz_gpu_signal_locate_span_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, int sized, const vbz_gpu_signal_format* f,
                                     const vbz_gpu_normalization* norm, float* shift_scale, const vbz_gpu_sample_ranges* ranges,
                                     const vbz_gpu_locate* locate, float* query, vbz_gpu_match_span* out)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, sized).format(f).aligned(LOCATE, align_view(locate), query, out)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

int vbz_gpu_pod5_signal_locate_span_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, const vbz_gpu_signal_format* f,
                                          const vbz_gpu_pod5_reads* reads, const vbz_gpu_normalization* norm, float* shift_scale,
                                          const vbz_gpu_sample_ranges* ranges, const vbz_gpu_locate* locate, float* query, vbz_gpu_match_span* out)
{
    return typed_decode(c, bt, o, TypedCall(Typed::CHUNKS, 0).format(f).pod5_reads(reads).aligned(LOCATE, align_view(locate), query, out)
                                      .normalise(norm, Null::ALLOWED, shift_scale, Null::ALLOWED).range(ranges));
}

static_assert(sizeof(vbz_gpu_match_pair) == 16 && offsetof(vbz_gpu_match_pair, read) == 0 && offsetof(vbz_gpu_match_pair, ref) == 4 &&
                  offsetof(vbz_gpu_match_pair, begin) == 8 && offsetof(vbz_gpu_match_pair, end) == 12,
              "vbz_gpu_match_pair is 16 bytes: read, ref, begin, end");
static_assert(sizeof(vbz_gpu_match_path) == 16 && offsetof(vbz_gpu_match_path, max_width) == 0 && offsetof(vbz_gpu_match_path, flags) == 4 &&
                  offsetof(vbz_gpu_match_path, reserved) == 8,
              "vbz_gpu_match_path is 16 bytes: max_width, flags, reserved");
static_assert(sizeof(vbz_gpu_match_row) == 8 && offsetof(vbz_gpu_match_row, begin) == 0 && offsetof(vbz_gpu_match_row, end) == 4,
              "vbz_gpu_match_row is 8 bytes: begin, end");

int vbz_gpu_match_best_batch(vbz_gpu_ctx* c, uint32_t n_reads, const vbz_gpu_match_span* spans, uint32_t n_refs, uint32_t max_cost, vbz_gpu_match_pair* pairs)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (n_refs < 1 || n_refs > 4096 || (uint64_t)n_reads * n_refs > EXTENT_MAX / sizeof(vbz_gpu_match_span)) {
        set_error(c, "match best outside the rules (%u reads, n_refs %u)", n_reads, n_refs);
        return -2;
    }
    if ((n_reads != 0 && (!spans || !pairs)) || (((uintptr_t)spans | (uintptr_t)pairs) & 15u) != 0) {
        set_error(c, "the span arena or the pair table is NULL or not 16-byte aligned");
        return -2;
    }
    Timed t(c, "match_best");
    HIPCHK(c, launch_match_best(n_reads, spans, n_refs, max_cost, pairs, c->stream), "match best launch");
    return 0;
}

int vbz_gpu_match_path_batch(vbz_gpu_ctx* c, uint32_t n_pairs, uint32_t n_reads, const float* query, const uint32_t* valid, const vbz_gpu_match* match,
                             const vbz_gpu_match_pair* pairs, const vbz_gpu_match_path* path, vbz_gpu_match_span* hit, vbz_gpu_match_row* rows)
{
    return path_call(c, MATCH, align_view(match), n_pairs, n_reads, query, valid, pairs, path, hit, rows);
}

int vbz_gpu_locate_path_batch(vbz_gpu_ctx* c, uint32_t n_pairs, uint32_t n_reads, const float* query, const uint32_t* valid, const vbz_gpu_locate* locate,
                              const vbz_gpu_match_pair* pairs, const vbz_gpu_match_path* path, vbz_gpu_match_span* hit, vbz_gpu_match_row* rows)
{
    return path_call(c, LOCATE, align_view(locate), n_pairs, n_reads, query, valid, pairs, path, hit, rows);
}

int vbz_gpu_query_valid_batch(vbz_gpu_ctx* c, uint32_t n_reads, const uint32_t* result, const vbz_gpu_sample_ranges* ranges, uint32_t query_len,
                              uint32_t* valid)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (query_len < 8 || query_len > 65536 || query_len % 8 != 0) {
        set_error(c, "query_len %u outside 8 ... 65536 in multiples of 8", query_len);
        return -2;
    }
    if (n_reads != 0 && (!result || !valid)) {
        set_error(c, "result or valid is NULL");
        return -2;
    }
    Timed t(c, "query_valid");
    HIPCHK(c, launch_match_valid(n_reads, result, ranges ? ranges->begin : nullptr, ranges ? ranges->end : nullptr, query_len, valid, c->stream),
           "query valid launch");
    return 0;
}

static_assert(sizeof(vbz_gpu_events_query) == 16 && offsetof(vbz_gpu_events_query, query_len) == 0 && offsetof(vbz_gpu_events_query, min_n) == 4 &&
                  offsetof(vbz_gpu_events_query, flags) == 8 && offsetof(vbz_gpu_events_query, reserved) == 12,
              "vbz_gpu_events_query is 16 bytes: query_len, min_n, flags, reserved");
static_assert(sizeof(vbz_gpu_level) == 32 && offsetof(vbz_gpu_level, first_sample) == 0 && offsetof(vbz_gpu_level, end_sample) == 4 &&
                  offsetof(vbz_gpu_level, n_samples) == 8 && offsetof(vbz_gpu_level, n_entries) == 12 && offsetof(vbz_gpu_level, sum) == 16 &&
                  offsetof(vbz_gpu_level, sumsq) == 24,
              "vbz_gpu_level is 32 bytes: first_sample, end_sample, n_samples, n_entries, sum, sumsq");

static bool entries_len_ok(uint32_t n) { return n >= 8 && n <= 65536 && n % 8 == 0; }

// what the two event-space calls share about the event tables: the struct's own rule, and the rows' extent
static bool eventalign_events_ok(vbz_gpu_ctx* c, const vbz_gpu_events* ev)
{
    if (!ev) {
        set_error(c, "events is NULL");
        return false;
    }
    if (ev->flags != 0 || ev->reserved != 0) {
        set_error(c, "events outside the rules (flags %u, reserved %u)", ev->flags, ev->reserved);
        return false;
    }
    if (ev->event_rows > EXTENT_MAX / sizeof(vbz_gpu_event)) {
        set_error(c, "declared event arena is not plausible (%llu rows of 16 bytes)", (unsigned long long)ev->event_rows);
        return false;
    }
    return true;
}

int vbz_gpu_events_query_batch(vbz_gpu_ctx* c, uint32_t n_reads, const uint32_t* result, const vbz_gpu_events* ev, const vbz_gpu_event* records,
                               const vbz_gpu_events_query* q, float* query, uint32_t* valid, uint32_t* index)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (!eventalign_events_ok(c, ev)) return -2;
    if (!q || !entries_len_ok(q->query_len) || q->flags != 0 || q->reserved != 0) {
        set_error(c, "events query is NULL or outside the rules (query_len %u, flags %u, reserved %u)", q ? q->query_len : 0u, q ? q->flags : 0u,
                  q ? q->reserved : 0u);
        return -2;
    }
    if (n_reads != 0 && (!ev->event_first || (!records && ev->event_rows != 0) || !query || !valid)) {
        set_error(c, "event_first, the event arena, the query arena or valid is NULL");
        return -2;
    }
    if ((((uintptr_t)query | (uintptr_t)records | (uintptr_t)index) & 15u) != 0) {
        set_error(c, "the query arena, the event arena or the index arena is not 16-byte aligned");
        return -2;
    }
    if ((uint64_t)n_reads * q->query_len > EXTENT_MAX / sizeof(float)) {
        set_error(c, "declared query arena is not plausible (%u reads of %u entries)", n_reads, q->query_len);
        return -2;
    }
    Timed t(c, "events_query");
    HIPCHK(c, launch_events_query(n_reads, result, ev->event_first, ev->event_rows, records, q->min_n, q->query_len, query, valid, index, c->stream),
           "events query launch");
    return 0;
}

int vbz_gpu_locate_levels_batch(vbz_gpu_ctx* c, uint32_t n_pairs, uint32_t n_reads, uint32_t query_len, uint32_t max_width, const vbz_gpu_match_pair* pairs,
                                const vbz_gpu_match_span* hit, const vbz_gpu_match_row* rows, const uint32_t* index, const vbz_gpu_events* ev,
                                const vbz_gpu_event* records, const vbz_gpu_event_moments* moments, uint32_t* n_levels, vbz_gpu_level* levels)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (!eventalign_events_ok(c, ev)) return -2;
    if (!entries_len_ok(query_len) || !entries_len_ok(max_width)) {
        set_error(c, "locate levels outside the rules (query_len %u, max_width %u: multiples of 8, 8 ... 65536)", query_len, max_width);
        return -2;
    }
    if (n_pairs != 0 && (!pairs || !hit || !rows || !ev->event_first || ((!ev->start || !records || !moments) && ev->event_rows != 0) || !n_levels || !levels)) {
        set_error(c, "the pair table, the hit table, the row arena, event_first, start, the event arena, the moments, n_levels or the level arena is NULL");
        return -2;
    }
    if ((((uintptr_t)pairs | (uintptr_t)hit | (uintptr_t)rows | (uintptr_t)records | (uintptr_t)moments | (uintptr_t)levels) & 15u) != 0) {
        set_error(c, "the pair table, the hit table, the row arena, the event arena, the moments or the level arena is not 16-byte aligned");
        return -2;
    }
    if ((uint64_t)n_pairs * query_len > EXTENT_MAX / sizeof(vbz_gpu_match_row) || (uint64_t)n_pairs * max_width > EXTENT_MAX / sizeof(vbz_gpu_level) ||
        (uint64_t)n_reads * query_len > EXTENT_MAX / sizeof(uint32_t)) {
        set_error(c, "declared level arenas are not plausible (%u pairs, %u reads, %u entries, %u levels)", n_pairs, n_reads, query_len, max_width);
        return -2;
    }
    Timed t(c, "locate_levels");
    HIPCHK(c, launch_locate_levels(n_pairs, n_reads, query_len, max_width, pairs, hit, rows, index, ev->event_first, ev->event_rows, ev->start, records,
                                   moments, n_levels, levels, c->stream),
           "locate levels launch");
    return 0;
}

static_assert(sizeof(vbz_gpu_squiggle) == 48 && offsetof(vbz_gpu_squiggle, k) == 0 && offsetof(vbz_gpu_squiggle, n_seqs) == 4 &&
                  offsetof(vbz_gpu_squiggle, seq_stride) == 8 && offsetof(vbz_gpu_squiggle, target_stride) == 12 && offsetof(vbz_gpu_squiggle, flags) == 16 &&
                  offsetof(vbz_gpu_squiggle, quant) == 20 && offsetof(vbz_gpu_squiggle, seq) == 24 && offsetof(vbz_gpu_squiggle, seq_len) == 32 &&
                  offsetof(vbz_gpu_squiggle, model) == 40,
              "vbz_gpu_squiggle is 48 bytes: k, n_seqs, seq_stride, target_stride, flags, quant, seq, seq_len, model");
static_assert(sizeof(vbz_gpu_levels_fit) == 16 && offsetof(vbz_gpu_levels_fit, max_width) == 0 && offsetof(vbz_gpu_levels_fit, min_samples) == 4 &&
                  offsetof(vbz_gpu_levels_fit, max_entries) == 8 && offsetof(vbz_gpu_levels_fit, flags) == 12,
              "vbz_gpu_levels_fit is 16 bytes: max_width, min_samples, max_entries, flags");
static_assert(sizeof(vbz_gpu_level_fit) == 16 && offsetof(vbz_gpu_level_fit, offset) == 0 && offsetof(vbz_gpu_level_fit, scale) == 4 &&
                  offsetof(vbz_gpu_level_fit, used) == 8 && offsetof(vbz_gpu_level_fit, ok) == 12,
              "vbz_gpu_level_fit is 16 bytes: offset, scale, used, ok");

// What the two calls over a vbz_gpu_squiggle share: the struct's own rules and the arenas' extent.  `tables`: the call's own pointers are
// all there; `arenas`: those that must be 16-byte aligned, or-ed.
static bool squiggle_ok(vbz_gpu_ctx* c, const vbz_gpu_squiggle* sq, bool tables, uintptr_t arenas, const char* null_msg, const char* align_msg)
{
    if (!sq) {
        set_error(c, "squiggle is NULL");
        return false;
    }
    const bool both = (sq->flags & VBZ_GPU_SQUIGGLE_BOTH) != 0;
    const auto stride_ok = [](uint32_t s) { return s >= 16 && s <= (1u << 30) && s % 16 == 0; };
    if (sq->k < 1 || sq->k > 9 || sq->n_seqs < 1 || sq->n_seqs > (both ? 2048u : 4096u) || !stride_ok(sq->seq_stride) || !stride_ok(sq->target_stride) ||
        (sq->flags & ~(VBZ_GPU_SQUIGGLE_BOTH | VBZ_GPU_SQUIGGLE_REVERSED)) != 0 || !(sq->quant > 0.0f) || !std::isfinite(sq->quant)) {
        set_error(c, "squiggle outside the rules (k %u, n_seqs %u, seq_stride %u, target_stride %u, flags %u, quant %g)", sq->k, sq->n_seqs, sq->seq_stride,
                  sq->target_stride, sq->flags, (double)sq->quant);
        return false;
    }
    if (!sq->seq || !sq->seq_len || !tables) {
        set_error(c, "%s", null_msg);
        return false;
    }
    if ((((uintptr_t)sq->seq | arenas) & 15u) != 0) {
        set_error(c, "%s", align_msg);
        return false;
    }
    const uint32_t rows = both ? 2u * sq->n_seqs : sq->n_seqs;
    if ((uint64_t)rows * sq->target_stride > EXTENT_MAX / sizeof(float) || (uint64_t)sq->n_seqs * sq->seq_stride > EXTENT_MAX) {
        set_error(c, "declared squiggle arenas are not plausible (%u sequences of %u bytes, %u rows of %u levels)", sq->n_seqs, sq->seq_stride, rows,
                  sq->target_stride);
        return false;
    }
    return true;
}

int vbz_gpu_squiggle_batch(vbz_gpu_ctx* c, const vbz_gpu_squiggle* sq, int8_t* target, uint32_t* target_len, uint32_t* masked, float* level)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (!squiggle_ok(c, sq, sq && sq->model && target && target_len && masked, (uintptr_t)target | (uintptr_t)level,
                     "seq, seq_len, the model, the target arena, target_len or masked is NULL", "seq, the target arena or the level arena is not 16-byte aligned"))
        return -2;
    const uint32_t rows = (sq->flags & VBZ_GPU_SQUIGGLE_BOTH) != 0 ? 2u * sq->n_seqs : sq->n_seqs;
    uint32_t* const part = ensure_array<uint32_t>(c, c->squigpart, squiggle_part_words(rows, sq->target_stride));
    if (!part) return -1;
    Timed t(c, "squiggle");
    HIPCHK(c, launch_squiggle(sq->k, rows, sq->seq_stride, sq->target_stride, sq->flags, sq->quant, sq->seq, sq->seq_len, sq->model, target, target_len, masked,
                              level, part, c->stream),
           "squiggle launch");
    return 0;
}

int vbz_gpu_levels_fit_batch(vbz_gpu_ctx* c, uint32_t n_pairs, uint32_t n_reads, const vbz_gpu_locate* locate, const vbz_gpu_match_pair* pairs,
                             const vbz_gpu_match_span* hit, const uint32_t* n_levels, const vbz_gpu_level* levels, const vbz_gpu_levels_fit* fit,
                             const float* prior_shift_scale, vbz_gpu_level_fit* out, float* offset, float* scale, int64_t* sums)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    // (the locate's own rules, the targets' extent and alignment: what vbz_gpu_locate_batch refuses about it; the tables a call with pairs needs: below)
    const AlignView m = align_view(locate);
    if (!align_ok(c, LOCATE, m, nullptr, nullptr, sizeof(vbz_gpu_match_span), 0)) return -2;
    if (!fit || fit->flags != 0 || !entries_len_ok(fit->max_width)) {
        set_error(c, "levels fit is NULL or outside the rules (max_width %u: a multiple of 8, 8 ... 65536; flags %u)", fit ? fit->max_width : 0u,
                  fit ? fit->flags : 0u);
        return -2;
    }
    if (n_pairs != 0 && (!m.levels || !m.levels_len || !pairs || !hit || !n_levels || !levels || !out || !offset || !scale)) {
        set_error(c, "target, target_len, the pair table, the hit table, n_levels, the level arena, the fit table, offset or scale is NULL");
        return -2;
    }
    if ((((uintptr_t)pairs | (uintptr_t)hit | (uintptr_t)levels | (uintptr_t)out) & 15u) != 0) {
        set_error(c, "the pair table, the hit table, the level arena or the fit table is not 16-byte aligned");
        return -2;
    }
    if ((uint64_t)n_pairs * fit->max_width > EXTENT_MAX / sizeof(vbz_gpu_level)) {
        set_error(c, "declared level arena is not plausible (%u pairs of %u levels)", n_pairs, fit->max_width);
        return -2;
    }
    Timed t(c, "levels_fit");
    HIPCHK(c, launch_levels_fit(n_pairs, n_reads, m.n_levels, m.levels_stride, m.quant, m.levels, m.levels_len, pairs, hit, n_levels, levels, fit->max_width,
                                fit->min_samples, fit->max_entries, prior_shift_scale, out, offset, scale, sums, c->stream),
           "levels fit launch");
    return 0;
}

// ---- the pile-up across reads (include/vbz_gpu_pile.h) ----
static_assert(sizeof(vbz_gpu_levels_pile) == 32 && offsetof(vbz_gpu_levels_pile, max_width) == 0 && offsetof(vbz_gpu_levels_pile, min_samples) == 4 &&
                  offsetof(vbz_gpu_levels_pile, max_entries) == 8 && offsetof(vbz_gpu_levels_pile, flags) == 12 && offsetof(vbz_gpu_levels_pile, fix) == 16 &&
                  offsetof(vbz_gpu_levels_pile, reserved0) == 20,
              "vbz_gpu_levels_pile is 32 bytes: max_width, min_samples, max_entries, flags, fix, three reserved words");
static_assert(sizeof(vbz_gpu_pile_kmers) == 16 && offsetof(vbz_gpu_pile_kmers, k) == 0 && offsetof(vbz_gpu_pile_kmers, rows) == 4 &&
                  offsetof(vbz_gpu_pile_kmers, target_stride) == 8 && offsetof(vbz_gpu_pile_kmers, flags) == 12,
              "vbz_gpu_pile_kmers is 16 bytes: k, rows, target_stride, flags");
static_assert(sizeof(vbz_gpu_model_update) == 16 && offsetof(vbz_gpu_model_update, k) == 0 && offsetof(vbz_gpu_model_update, min_obs) == 4 &&
                  offsetof(vbz_gpu_model_update, flags) == 8 && offsetof(vbz_gpu_model_update, fix) == 12,
              "vbz_gpu_model_update is 16 bytes: k, min_obs, flags, fix");

int vbz_gpu_levels_pile_batch(vbz_gpu_ctx* c, uint32_t n_pairs, uint32_t n_reads, const vbz_gpu_locate* locate, const vbz_gpu_match_pair* pairs,
                              const vbz_gpu_match_span* hit, const uint32_t* n_levels, const vbz_gpu_level* levels, const vbz_gpu_levels_pile* params,
                              const vbz_gpu_level_fit* fit, uint64_t* pile)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    // (the checks of vbz_gpu_levels_fit_batch, in its order, with the pile in the place of its outputs)
    const AlignView m = align_view(locate);
    if (!align_ok(c, LOCATE, m, nullptr, nullptr, sizeof(vbz_gpu_match_span), 0)) return -2;
    if (!params || (params->flags & ~(VBZ_GPU_PILE_CLEAR | VBZ_GPU_PILE_REQUIRE_OK)) != 0 || (params->reserved0 | params->reserved1 | params->reserved2) != 0 ||
        !entries_len_ok(params->max_width) || !(params->fix > 0.0f) || !std::isfinite(params->fix)) {
        set_error(c, "levels pile is NULL or outside the rules (max_width %u: a multiple of 8, 8 ... 65536; flags %u; fix %g: finite, > 0; reserved words 0)",
                  params ? params->max_width : 0u, params ? params->flags : 0u, params ? (double)params->fix : 0.0);
        return -2;
    }
    if (!pile || (n_pairs != 0 && (!m.levels || !m.levels_len || !pairs || !hit || !n_levels || !levels))) {
        set_error(c, "the pile, target, target_len, the pair table, the hit table, n_levels or the level arena is NULL");
        return -2;
    }
    if ((((uintptr_t)pairs | (uintptr_t)hit | (uintptr_t)levels | (uintptr_t)fit | (uintptr_t)pile) & 15u) != 0) {
        set_error(c, "the pair table, the hit table, the level arena, the fit table or the pile is not 16-byte aligned");
        return -2;
    }
    if ((uint64_t)n_pairs * params->max_width > EXTENT_MAX / sizeof(vbz_gpu_level) || (uint64_t)m.n_levels * m.levels_stride > EXTENT_MAX / 32u) {
        set_error(c, "declared level arena or pile is not plausible (%u pairs of %u levels, %u targets of %u cells)", n_pairs, params->max_width, m.n_levels,
                  m.levels_stride);
        return -2;
    }
    Timed t(c, "levels_pile");
    HIPCHK(c, launch_levels_pile(n_pairs, n_reads, m.n_levels, m.levels_stride, m.levels_len, pairs, hit, n_levels, levels, params->max_width, params->min_samples,
                                 params->max_entries, (params->flags & VBZ_GPU_PILE_REQUIRE_OK) != 0, (params->flags & VBZ_GPU_PILE_CLEAR) != 0, params->fix, fit,
                                 pile, c->stream),
           "levels pile launch");
    return 0;
}

int vbz_gpu_squiggle_kmers_batch(vbz_gpu_ctx* c, const vbz_gpu_squiggle* sq, uint32_t* kmer, uint32_t* target_len)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (!squiggle_ok(c, sq, kmer && target_len, (uintptr_t)kmer, "seq, seq_len, the kmer arena or target_len is NULL",
                     "seq or the kmer arena is not 16-byte aligned"))
        return -2;
    const uint32_t rows = (sq->flags & VBZ_GPU_SQUIGGLE_BOTH) != 0 ? 2u * sq->n_seqs : sq->n_seqs;
    Timed t(c, "squiggle_kmers");
    HIPCHK(c, launch_squiggle_kmers(sq->k, rows, sq->seq_stride, sq->target_stride, sq->flags, sq->seq, sq->seq_len, kmer, target_len, c->stream),
           "squiggle kmers launch");
    return 0;
}

int vbz_gpu_pile_kmers_batch(vbz_gpu_ctx* c, const vbz_gpu_pile_kmers* params, const uint32_t* target_len, const uint32_t* kmer, const uint64_t* pile,
                             uint64_t* kmer_pile)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (!params || params->k < 1 || params->k > 9 || params->rows < 1 || params->rows > 4096 || params->target_stride < 16 ||
        params->target_stride > (1u << 30) || params->target_stride % 16 != 0 || (params->flags & ~(VBZ_GPU_PILE_CLEAR | VBZ_GPU_PILE_DIRECT)) != 0) {
        set_error(c, "pile kmers is NULL or outside the rules (k %u, rows %u, target_stride %u, flags %u)", params ? params->k : 0u, params ? params->rows : 0u,
                  params ? params->target_stride : 0u, params ? params->flags : 0u);
        return -2;
    }
    if (!target_len || !kmer || !pile || !kmer_pile) {
        set_error(c, "target_len, the kmer arena, the pile or the k-mer pile is NULL");
        return -2;
    }
    if ((((uintptr_t)kmer | (uintptr_t)pile | (uintptr_t)kmer_pile) & 15u) != 0) {
        set_error(c, "the kmer arena, the pile or the k-mer pile is not 16-byte aligned");
        return -2;
    }
    if ((uint64_t)params->rows * params->target_stride > EXTENT_MAX / 32u) {
        set_error(c, "declared pile is not plausible (%u rows of %u cells)", params->rows, params->target_stride);
        return -2;
    }
    Timed t(c, "pile_kmers");
    HIPCHK(c, launch_pile_kmers(params->k, params->rows, params->target_stride, (params->flags & VBZ_GPU_PILE_CLEAR) != 0,
                                (params->flags & VBZ_GPU_PILE_DIRECT) != 0, target_len, kmer, pile, kmer_pile, c->stream),
           "pile kmers launch");
    return 0;
}

int vbz_gpu_model_update_batch(vbz_gpu_ctx* c, const vbz_gpu_model_update* params, const uint64_t* kmer_pile, const float* prior, float* model, float* sd)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    if (!params || params->k < 1 || params->k > 9 || params->flags != 0 || !(params->fix > 0.0f) || !std::isfinite(params->fix)) {
        set_error(c, "model update is NULL or outside the rules (k %u, flags %u, fix %g)", params ? params->k : 0u, params ? params->flags : 0u,
                  params ? (double)params->fix : 0.0);
        return -2;
    }
    if (!kmer_pile || !prior || !model || ((uintptr_t)kmer_pile & 15u) != 0) {
        set_error(c, "the k-mer pile, the prior or the model is NULL, or the k-mer pile is not 16-byte aligned");
        return -2;
    }
    Timed t(c, "model_update");
    HIPCHK(c, launch_model_update(params->k, params->min_obs, params->fix, kmer_pile, prior, model, sd, c->stream), "model update launch");
    return 0;
}

int vbz_gpu_svb_compress_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, int integer_size, int zigzag, int version)
{
    if (!c || !bt) return -1;
    DeviceGuard dg(c->device);
    if ((unsigned)version == VBZ_GPU_VERSION_POD5) {
        if (integer_size != 2 || !zigzag) return -2;
        Timed t(c, "svb_encode");
        HIPCHK(c, launch_svb16_encode(to_rb(bt), nullptr, c->stream), "svb16_encode launch");
        return 0;
    }
    if ((integer_size != 1 && integer_size != 2 && integer_size != 4) || version > 1 || version < 0) return -2;
    Timed t(c, "svb_encode");
    HIPCHK(c, launch_svb_encode(to_rb(bt), integer_size, zigzag != 0, 0, true, version == 1 && integer_size == 1, nullptr, nullptr, c->stream), "svb_encode launch");
    return 0;
}

int vbz_gpu_svb_decompress_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, int integer_size, int zigzag, int version)
{
    if (!c || !bt) return -1;
    DeviceGuard dg(c->device);
    if ((unsigned)version == VBZ_GPU_VERSION_POD5) {
        if (integer_size != 2 || !zigzag) return -2;
        Timed t(c, "svb_decode");
        HIPCHK(c, launch_svb16_decode(to_rb(bt), c->stream), "svb16_decode launch");
        return 0;
    }
    if ((integer_size != 1 && integer_size != 2 && integer_size != 4) || version > 1 || version < 0) return -2;
    Timed t(c, "svb_decode");
    HIPCHK(c, launch_svb_decode(to_rb(bt), integer_size, zigzag != 0, version == 1 && integer_size == 1, c->stream), "svb_decode launch");
    return 0;
}

uint64_t vbz_gpu_pod5_max_compressed_size(uint32_t samples)
{
    const uint64_t n = samples, svb = (n + 7) / 8 + 2 * n;   // svb16_max(n)
    return svb + (svb >> 8) + (svb < (128u << 10) ? (((128u << 10) - svb) >> 11) : 0);   // ZSTD_COMPRESSBOUND
}

int vbz_gpu_zstd_compress_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const uint32_t* key_bytes)
{
    if (!c || !bt) return -1;
    DeviceGuard dg(c->device);
    if (checksum_content(c, to_rb(bt), nullptr) != 0) return -1;
    Timed t(c, "zstd_encode");
    ZstdEncodeArgs a;
    a.key.orig_size = bt->src_size;
    a.key.key_bytes = key_bytes;
    a.trailers = c->knobs.trailers;
    HIPCHK(c, launch_zstd_encode(to_rb(bt), a, c->stream), "zstd_encode launch");
    return checksum_frames(c, to_rb(bt), nullptr, 0, nullptr, 0);
}

int vbz_gpu_zstd_decompress_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt)
{
    if (!c || !bt) return -1;
    DeviceGuard dg(c->device);
    if (!plausible_extents(c, bt)) return -2;
    if (zstd_frames(c, to_rb(bt), E_ZSTD, bt->dst_bytes, nullptr) != 0) return -1;
    return verify_checksums(c, to_rb(bt));
}

int vbz_gpu_xxh64_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, uint64_t* out)
{
    if (!c || !bt || !out) return -1;
    DeviceGuard dg(c->device);
    Timed t(c, "xxh64");
    HIPCHK(c, launch_xxh64_batch((const uint8_t*)bt->src, bt->src_off, bt->src_size, nullptr, nullptr, bt->n_reads, out, c->stream), "xxh64 launch");
    return 0;
}

// Dense arenas (pack.hip).  Arguments are checked here, before anything is launched; each call looks only at the side of the batch
// it reads (plausible_extents' rules for those fields).
static bool pack_align_ok(vbz_gpu_ctx* c, uint32_t align)
{
    if (align >= 1 && align <= 4096 && (align & (align - 1)) == 0) return true;
    set_error(c, "align %u is not a power of two in 1 ... 4096", align);
    return false;
}

int vbz_gpu_pack_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, uint32_t align, void* packed, uint64_t packed_cap, uint64_t* packed_off,
                       uint32_t* packed_size)
{
    if (!c || !bt) return -1;
    DeviceGuard dg(c->device);
    if (!pack_align_ok(c, align)) return -2;
    const uint32_t n = bt->n_reads;
    if (!packed_off || (n != 0 && (!bt->dst_off || !bt->dst_cap || !bt->result || !packed_size || (!bt->dst && bt->dst_bytes != 0)))) {
        set_error(c, "a table or arena pointer of the pack call is NULL");
        return -2;
    }
    if (bt->dst_bytes > EXTENT_MAX || (packed && packed_cap > EXTENT_MAX)) {
        set_error(c, "declared arena extents are not plausible (dst_bytes %llu, packed_cap %llu)", (unsigned long long)bt->dst_bytes,
                  (unsigned long long)packed_cap);
        return -2;
    }
    const uintptr_t d0 = (uintptr_t)bt->dst, p0 = (uintptr_t)packed;
    if (packed && packed_cap && bt->dst_bytes && p0 < d0 + bt->dst_bytes && d0 < p0 + packed_cap) {
        set_error(c, "the packed arena overlaps the dst arena");
        return -2;
    }
    {
        Timed t(c, "pack_layout");
        HIPCHK(c, launch_pack_layout(n, bt->result, bt->dst_off, bt->dst_cap, bt->dst_bytes, align, packed_off, packed_size, c->stream), "pack layout launch");
    }
    if (!packed) return 0;
    Timed t(c, "pack_gather");
    HIPCHK(c, launch_pack_gather(n, (const uint8_t*)bt->dst, bt->dst_off, packed_off, packed_size, (uint8_t*)packed, packed_cap, c->stream),
           "pack gather launch");
    return 0;
}

int vbz_gpu_decompressed_size_batch(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, const CompressionOptions* o, uint32_t align, uint32_t* raw_size,
                                    uint64_t* raw_off)
{
    if (!c || !bt) return -1;
    DeviceGuard dg(c->device);
    if (!o || !valid_int_size(o) || pod5_codec(o)) {   // (POD5 rows carry no size header)
        set_error(c, "unsupported options");
        return -2;
    }
    if (!pack_align_ok(c, align)) return -2;
    const uint32_t n = bt->n_reads;
    if (!raw_off || (n != 0 && (!bt->src_off || !bt->src_size || !raw_size || (!bt->src && bt->src_bytes != 0)))) {
        set_error(c, "a table or arena pointer of the size query is NULL");
        return -2;
    }
    if (bt->src_bytes > EXTENT_MAX) {
        set_error(c, "declared arena extent is not plausible (src_bytes %llu)", (unsigned long long)bt->src_bytes);
        return -2;
    }
    Timed t(c, "sized_layout");
    HIPCHK(c, launch_sized_layout(n, (const uint8_t*)bt->src, bt->src_off, bt->src_size, bt->src_bytes, align, raw_size, raw_off, c->stream),
           "sized layout launch");
    return 0;
}

int vbz_gpu_synth_lengths(vbz_gpu_ctx* c, uint64_t seed, uint64_t first, uint32_t n, uint32_t* out_len)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    HIPCHK(c, launch_synth_lengths(seed, first, n, out_len, c->stream), "synth_lengths launch");
    return 0;
}

int vbz_gpu_synth_signal(vbz_gpu_ctx* c, uint64_t seed, uint64_t first, uint32_t n, void* dst, const uint64_t* off,
                         const uint32_t* len)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    HIPCHK(c, launch_synth_signal(seed, first, n, (uint8_t*)dst, off, len, c->stream), "synth_signal launch");
    return 0;
}

int vbz_gpu_synth_u32(vbz_gpu_ctx* c, uint64_t seed, uint64_t first, uint32_t n, void* dst, const uint64_t* off, const uint32_t* len)
{
    if (!c) return -1;
    DeviceGuard dg(c->device);
    HIPCHK(c, launch_synth_u32(seed, first, n, (uint8_t*)dst, off, len, c->stream), "synth_u32 launch");
    return 0;
}

#ifdef VBZ_EXPERIMENTS
// Test aid (experiments build only): the first half of vbz_gpu_compress_batch for int16 zig-zag reads at level != 0 on the one-workgroup
// path -- scratch slots, svb_encode with its hand-over to the entropy stage (svb_kernels.hip CNT) -- and nothing of the entropy stage.
// Afterwards read i's svb stream stands at the bottom of its destination slot, result[i] = the stream's size, and plans_out (device,
// n_reads * vbz_gpu_x_plan_bytes() bytes) holds the per-read plans.  tests/test_gpu_handover.py holds them to a numpy statement of
// region_histogram's sample.
VBZ_EXPORT size_t vbz_gpu_x_plan_bytes(void) { return sizeof(EncPlan); }
VBZ_EXPORT int vbz_gpu_x_svb_handover(vbz_gpu_ctx* c, const vbz_gpu_batch* bt, void* plans_out)
{
    if (!c || !bt || !plans_out) return -1;
    DeviceGuard dg(c->device);
    const uint32_t n = bt->n_reads;
    if (n == 0) return 0;
    hipStream_t s = c->stream;
    ReadBatch rb = to_rb(bt);
    uint32_t num, den;
    svb_factor(2, true, &num, &den);
    const size_t scratch_need = (size_t)(((unsigned __int128)bt->src_bytes * num + den - 1) / den) + (size_t)n * 96 + 256;
    StageSlots m;
    if (!ensure(c, c->scratch, scratch_need) || !ensure_carved(c, c->meta, m, n) || !ensure(c, c->encplan, zstd_encode_plan_bytes(n))) return -1;
    uint64_t* const svb_off = m.svb_off;
    uint32_t *const svb_cap = m.svb_cap, *const svb_size = m.svb_size, *const gate = m.gate;
    HIPCHK(c, launch_plan_scratch(n, bt->src_size, num, den, c->scratch.cap, svb_off, svb_cap, gate, false, s), "plan launch");
    ReadBatch a = rb;
    a.dst = (uint8_t*)c->scratch.p;
    a.dst_off = svb_off;
    a.dst_cap = svb_cap;
    a.result = svb_size;
    a.gate = gate;
    HIPCHK(c, launch_svb_encode(a, 2, true, 0, false, false, nullptr, c->encplan.p, s), "svb_encode launch");
    ReadBatch cp = rb;   // scratch slot -> bottom of the destination slot
    cp.src = (const uint8_t*)c->scratch.p;
    cp.src_off = svb_off;
    cp.src_size = svb_size;
    cp.gate = gate;
    HIPCHK(c, launch_copy_bytes(cp, 0, s), "copy launch");
    HIPCHK(c, hipMemcpyAsync(plans_out, c->encplan.p, (size_t)n * sizeof(EncPlan), hipMemcpyDeviceToDevice, s), "plan copy");
    return 0;
}
// Measuring aid (experiments build only): which way fast_runs_kernel's zero-run blocks went since the last reset -- chunks of 64
// sequences, those built in LDS, sequences sections with checkpoints, those staged in LDS (profiles/occ_experiments.md).
VBZ_EXPORT int vbz_gpu_x_runs_counts(vbz_gpu_ctx* c, unsigned long long* out4, int reset)
{
    if (!c || !out4) return -1;
    DeviceGuard dg(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream), "runs counts sync");
    HIPCHK(c, zstd_fast_runs_counts(out4, reset != 0), "runs counts");
    return 0;
}
// Measuring aid (experiments build only, VBZ_HIP_FS_COUNT=1): what fast_streams_kernel's refill path did since the last reset -- periods
// walked, periods in which the wavefront took the path, lanes that issued (profiles/stream_refill.md).
VBZ_EXPORT int vbz_gpu_x_streams_counts(vbz_gpu_ctx* c, unsigned long long* out3, int reset)
{
    if (!c || !out3) return -1;
    DeviceGuard dg(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream), "streams counts sync");
    HIPCHK(c, zstd_fast_streams_counts(out3, reset != 0), "streams counts");
    return 0;
}
#endif

void vbz_gpu_profile_enable(vbz_gpu_ctx* c, int enable)
{
    if (!c) return;
    if (!enable) drain_profile(c);
    c->profiling = enable != 0;
    if (c->half) vbz_gpu_profile_enable(c->half, enable);
}

int vbz_gpu_decode_span_paths(vbz_gpu_ctx* c, uint32_t* by_spans)
{
    if (!c) return -1;
    DeviceGuard guard(c->device);
    if (by_spans) *by_spans = 0;
    if (c->last_span_frames == 0) return 0;
    std::vector<uint32_t> redo(c->last_span_frames);
    if (hipMemcpyAsync(redo.data(), c->last_span_redo, 4ull * redo.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    uint32_t nb = 0;
    for (uint32_t v : redo) nb += v == 0;
    if (by_spans) *by_spans = nb;
    return (int)c->last_span_frames;
}

static int decode_paths_one(vbz_gpu_ctx* c, uint32_t* batched, uint32_t* walked);

int vbz_gpu_decode_paths(vbz_gpu_ctx* c, uint32_t* batched, uint32_t* walked)
{
    if (!c) return -1;
    uint32_t b0 = 0, w0 = 0, b1 = 0, w1 = 0;
    const int n0 = decode_paths_one(c, &b0, &w0);
    const int n1 = (n0 >= 0 && c->last_split && c->half) ? decode_paths_one(c->half, &b1, &w1) : 0;   // (the upper half of a split call)
    if (batched) *batched = b0 + b1;
    if (walked) *walked = w0 + w1;
    return (n0 < 0 || n1 < 0) ? -1 : n0 + n1;
}

int vbz_gpu_decode_literals_ahead(vbz_gpu_ctx* c)
{
    if (!c) return -1;
    int total = 0;
    for (vbz_gpu_ctx* k : { c, (c->last_split && c->half) ? c->half : (vbz_gpu_ctx*)nullptr }) {
        if (!k || !k->last_frames || !k->last_walked || !zstd_ref_literals_enabled() || !k->reflits.p) continue;
        DeviceGuard guard(k->device);
        const uint32_t per = k->last_lit_units;
        if (per == 0) continue;
        std::vector<RefLits> lits((size_t)k->last_frames * per);
        if (hipMemcpyAsync(lits.data(), zstd_ref_lits(k->reflits.p, k->last_frames), sizeof(RefLits) * lits.size(), hipMemcpyDeviceToHost, k->stream) != hipSuccess ||
            hipStreamSynchronize(k->stream) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
        if (k->knobs.trace) {   // per block ordinal: units the scan made, units whose literals stand
            std::vector<uint32_t> sk((size_t)k->last_frames * per);
            if (hipMemcpy(sk.data(), zstd_ref_lit_skip(k->reflits.p, k->last_frames), 4 * sk.size(), hipMemcpyDeviceToHost) == hipSuccess)
                for (uint32_t u = 0; u < per; ++u) {
                    uint32_t made = 0, done = 0;
                    for (uint32_t i = 0; i < k->last_frames; ++i) {
                        made += sk[(size_t)u * k->last_frames + i] == 0;
                        done += lits[(size_t)u * k->last_frames + i].blk != 0;
                    }
                    fprintf(stderr, "vbz_hip: literals beside the walk, unit %u: %u made by the scan, %u done\n", u, made, done);
                }
        }
        for (uint32_t i = 0; i < k->last_frames; ++i) {   // (frames with at least one block's literals ahead)
            bool any = false;
            for (uint32_t u = 0; u < per; ++u) any = any || lits[(size_t)u * k->last_frames + i].blk != 0;   // (record u of read i)
            total += any;
        }
    }
    return total;
}

static int decode_paths_one(vbz_gpu_ctx* c, uint32_t* batched, uint32_t* walked)
{
    DeviceGuard guard(c->device);
    if (batched) *batched = 0;
    if (walked) *walked = 0;
    const uint32_t n = c->last_frames;
    if (n == 0) return 0;
    std::vector<uint32_t> redo(n);
    std::vector<RefPre> pre(c->last_walked ? n : 0);
    if (hipMemcpyAsync(redo.data(), zstd_fast_redo(c->fastmeta.p, n), 4ull * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
    if (!pre.empty() && hipMemcpyAsync(pre.data(), zstd_ref_pre(c->refpre.p), sizeof(RefPre) * (size_t)n, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        return -1;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    uint32_t nb = 0, nw = 0;
    for (uint32_t i = 0; i < n; ++i) {
        nb += redo[i] == 0;
        if (!pre.empty()) nw += pre[i].ok != 0;
    }
    if (c->knobs.trace && !pre.empty()) {  // why frames of other writers were left to the one-wavefront decoder (zstd_decode_ref.hip: BAIL)
        std::map<uint32_t, uint32_t> why;
        for (uint32_t i = 0; i < n; ++i)
            if (redo[i] && !pre[i].ok) ++why[pre[i].why];
        for (auto& e : why) fprintf(stderr, "vbz_hip: chains not walked: reason %u, %u frame(s)\n", e.first, e.second);
        double tb = 0, ch = 0, ns = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (pre[i].ok) tb += pre[i].tab_cycles, ch += pre[i].chain_cycles, ns += pre[i].nseq_last;
        if (nw) fprintf(stderr, "vbz_hip: walked chains: %u frames, last block: %.0f cycles for the tables, %.0f for the chain, %.0f sequences\n", nw, tb / nw, ch / nw, ns / nw);
    }
    if (batched) *batched = nb;
    if (walked) *walked = nw;
    return (int)n;
}

void vbz_gpu_profile_reset(vbz_gpu_ctx* c)
{
    if (!c) return;
    drain_profile(c);
    c->prof.clear();
    if (c->half) vbz_gpu_profile_reset(c->half);
}

int vbz_gpu_profile_read(vbz_gpu_ctx* c, const char** names, uint32_t* launches, double* total_ms, int cap)
{
    if (!c) return 0;
    drain_profile(c);
    if (c->half) {   // the upper halves of split calls: their launches count under the same labels
        drain_profile(c->half);
        for (auto& h : c->half->prof) {
            bool found = false;
            for (auto& e : c->prof)
                if (strcmp(e.name, h.name) == 0) {
                    e.launches += h.launches;
                    e.ms += h.ms;
                    found = true;
                    break;
                }
            if (!found) c->prof.push_back(h);
        }
        c->half->prof.clear();
    }
    int k = 0;
    for (auto& e : c->prof) {
        if (k < cap) {
            if (names) names[k] = e.name;
            if (launches) launches[k] = e.launches;
            if (total_ms) total_ms[k] = e.ms;
        }
        ++k;
    }
    return k;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// vbz.h : the reference's single-buffer API over host pointers
// ------------------------------------------------------------------------------------------------
namespace {

// The reference's calls are re-entrant and callers parallelise by calling from many threads (vbz.cpp has no
// statics).  A call here needs a context (stream, device buffers), so there is a pool of them: a caller takes an idle
// context or creates one -- up to VBZ_HIP_CONTEXTS (default 16) -- and calls from different threads overlap on the
// GPU, each on its own stream.  Beyond the limit callers wait for a context to come back.
std::mutex g_mutex;
std::condition_variable g_idle_cv;
std::vector<vbz_gpu_ctx*> g_idle;
unsigned g_created = 0;
unsigned g_limit = 0;        // 0: pool_limit(); lowered to the number of live contexts once a creation fails
bool g_ctx_failed = false;

unsigned pool_limit()
{
    unsigned n = 16;
    if (const char* e = getenv("VBZ_HIP_CONTEXTS")) n = (unsigned)atoi(e);
    return n < 1 ? 1 : (n > 256 ? 256 : n);
}

vbz_gpu_ctx* take_ctx()
{
    std::unique_lock<std::mutex> lock(g_mutex);
    for (;;) {
        if (!g_idle.empty()) {
            vbz_gpu_ctx* c = g_idle.back();
            g_idle.pop_back();
            return c;
        }
        if (g_ctx_failed) return nullptr;
        if (g_created < (g_limit ? g_limit : pool_limit())) {
            ++g_created;
            lock.unlock();
            int dev = 0;
            if (const char* e = getenv("VBZ_HIP_DEVICE")) dev = atoi(e);
            vbz_gpu_ctx* c = vbz_gpu_create(dev, nullptr);
            lock.lock();
            if (c) return c;
            --g_created;
            if (g_created == 0) {
                g_ctx_failed = true;  // no usable device: every call reports a device failure
                g_idle_cv.notify_all();
                return nullptr;
            }
            // creation failed while other contexts live (e.g. hipMalloc under memory pressure): stop growing the pool
            // and wait for one of them to come back instead of retrying at once
            g_limit = g_created;
        }
        g_idle_cv.wait(lock);
    }
}

void give_ctx(vbz_gpu_ctx* c)
{
    {
        std::lock_guard<std::mutex> lock(g_mutex);
        g_idle.push_back(c);
    }
    g_idle_cv.notify_one();
}

struct CtxLease
{
    vbz_gpu_ctx* c;
    CtxLease() : c(take_ctx()) {}
    ~CtxLease()
    {
        if (c) give_ctx(c);
    }
};

// vbz.h callers may be binaries compiled against the REFERENCE header and only re-linked: they test
// `ret >= VBZ_FIRST_ERROR` with the reference's value (-7).  A device failure is therefore reported with the
// reference's own VBZ_OUT_OF_MEMORY_ERROR ("the device or its memory is not available") plus a line on stderr;
// the detailed cause is in vbz_gpu_last_error / on stderr.  VBZ_DEVICE_ERROR (-8) only appears in vbz_gpu.h results.
vbz_size_t device_failure()
{
    fprintf(stderr, "vbz_hip: no usable gfx950 device (or a device operation failed); this library has no CPU path\n");
    return VBZ_OUT_OF_MEMORY_ERROR;
}

constexpr uint32_t ONE_PINNED_MAX = 1u << 20;   // reads / results up to this size go through pinned memory (run_one)

struct OneMeta  // device-side descriptors of a one-read batch
{
    uint64_t src_off, dst_off;
    uint32_t src_size, dst_cap, result, pad;
};

// run one read through the batch path: host src -> device -> kernels -> host dst
vbz_size_t run_one(bool compress, const void* src, vbz_size_t src_size, void* dst, vbz_size_t dst_cap, vbz_size_t dev_cap,
                   const CompressionOptions* o, int sized)
{
    CtxLease lease;
    vbz_gpu_ctx* c = lease.c;
    if (!c) return device_failure();
    DeviceGuard dg(c->device);
    // Device buffers: one_in = [OneMeta | 64 bytes | the read], one_out = the result.  Pinned host memory: [OneMeta | pad to 256 | the
    // read on its way in | 16 words of hand-back header + the result on its way out] -- reads and results of up to ONE_PINNED_MAX go
    // through it: ONE host-to-device copy from pinned memory (descriptors and read together), and on the way back no copy call and no
    // stream synchronisation at all: hand_back_kernel writes the result into the pinned area and raises a flag this thread polls
    // (a synchronisation costs 10-20 us, the two copies of a pageable call as much again; 100 KB over the link 2 us).  Larger calls
    // keep the plain copies (a host memcpy of megabytes costs more than it saves: DESIGN 4.7).
    const bool small_in = src_size <= ONE_PINNED_MAX, small_out = (compress ? dev_cap : dst_cap) <= ONE_PINNED_MAX;
    const size_t in_off = 256, out_off = in_off + (small_in ? (((size_t)src_size + 63) & ~(size_t)63) : 0);
    const uint32_t out_cap = small_out ? (compress ? dev_cap : dst_cap) : 0u;
    const size_t pin_need = out_off + 64 + out_cap + 64;
    if (!ensure(c, c->one_in, (size_t)src_size + 512) || !ensure(c, c->one_out, (size_t)dev_cap + 64)) return VBZ_OUT_OF_MEMORY_ERROR;
    // (host-coherent: the hand-back flag is polled while the kernel that raises it may still be running)
    if (c->pinned.cap < pin_need && !c->pinned.grow(std::max<size_t>(pin_need, 1u << 20), hipHostMallocCoherent | hipHostMallocMapped))
        return VBZ_OUT_OF_MEMORY_ERROR;
    uint8_t* pin = (uint8_t*)c->pinned.p;
    OneMeta* hm = (OneMeta*)pin;
    hm->src_off = 0;
    hm->dst_off = 0;
    hm->src_size = src_size;
    hm->dst_cap = dev_cap;
    hm->result = VBZ_DEVICE_ERROR;
    hm->pad = 0;
    hipStream_t s = c->stream;
    uint8_t* din = (uint8_t*)c->one_in.p;       // device: the descriptors, then the read at + 256
    bool ok = true;
    if (small_in) {
        if (src_size) memcpy(pin + in_off, src, src_size);
        ok &= hipMemcpyAsync(din, pin, in_off + src_size, hipMemcpyHostToDevice, s) == hipSuccess;
    } else {
        ok &= hipMemcpyAsync(din, pin, sizeof(OneMeta), hipMemcpyHostToDevice, s) == hipSuccess;
        ok &= hipMemcpyAsync(din + in_off, src, src_size, hipMemcpyHostToDevice, s) == hipSuccess;
    }
    if (!ok) {
        set_error(c, "host to device copy failed");
        return device_failure();
    }
    OneMeta* dm = (OneMeta*)din;
    vbz_gpu_batch bt;
    memset(&bt, 0, sizeof bt);
    bt.n_reads = 1;
    bt.src = din + in_off;
    bt.src_off = &dm->src_off;
    bt.src_size = &dm->src_size;
    bt.src_bytes = src_size;
    bt.dst = c->one_out.p;
    bt.dst_off = &dm->dst_off;
    bt.dst_cap = &dm->dst_cap;
    bt.dst_bytes = dev_cap;
    bt.result = &dm->result;
    int rc = compress ? compress_batch_impl(c, &bt, o, sized, true) : decompress_batch_impl(c, &bt, o, sized, true);
    if (rc != 0) {
        (void)hipStreamSynchronize(s);   // (the copy out of the pinned area may still be in flight: the next call rewrites it)
        return device_failure();
    }
    uint32_t result = VBZ_DEVICE_ERROR;
    uint32_t have = 0;   // bytes of the result that have arrived in pinned memory
    volatile uint32_t* hb = (volatile uint32_t*)(pin + out_off);
    if (small_out) {
        const uint32_t seq = ++c->one_seq ? c->one_seq : ++c->one_seq;   // (never 0: what the flag holds between calls)
        hb[2] = 0;
        if (launch_hand_back(&dm->result, (const uint8_t*)c->one_out.p, (uint32_t*)(pin + out_off), out_cap, seq, &dm->pad, s) != hipSuccess) {
            set_error(c, "hand-back launch failed: %s", hipGetErrorString(hipGetLastError()));
            (void)hipStreamSynchronize(s);
            return device_failure();
        }
        // poll the flag; now and then ask the stream whether it is still alive (a faulting kernel never raises the flag)
        bool done = false;
        for (uint64_t spin = 0; !done; ++spin) {
            if (__atomic_load_n((const uint32_t*)&hb[2], __ATOMIC_ACQUIRE) == seq) {
                done = true;
                break;
            }
            if ((spin & 0xFFFu) == 0xFFFu) {
                const hipError_t q = hipStreamQuery(s);
                if (q == hipSuccess) {   // the stream has drained: the flag is there, or the launch chain failed
                    done = __atomic_load_n((const uint32_t*)&hb[2], __ATOMIC_ACQUIRE) == seq;
                    break;
                }
                if (q != hipErrorNotReady) break;
            }
        }
        if (!done) {
            (void)hipStreamSynchronize(s);
            set_error(c, "kernel execution failed: %s", hipGetErrorString(hipGetLastError()));
            return device_failure();
        }
        result = hb[0];
        have = hb[1];
    } else {
        if (hipMemcpyAsync(&hm->result, &dm->result, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            set_error(c, "kernel execution failed: %s", hipGetErrorString(hipGetLastError()));
            return device_failure();
        }
        result = hm->result;
    }
    if (result == VBZ_DEVICE_ERROR) return device_failure();
    if (result >= VBZ_FIRST_ERROR) return result;
    if (result > dst_cap) return VBZ_DESTINATION_SIZE_ERROR;
    if (have) memcpy(dst, pin + out_off + 64, have);
    if (result > have && (hipMemcpyAsync((uint8_t*)dst + have, (const uint8_t*)c->one_out.p + have, result - have, hipMemcpyDeviceToHost, s) != hipSuccess ||
                          hipStreamSynchronize(s) != hipSuccess)) {
        set_error(c, "device to host copy failed");
        return device_failure();
    }
    return result;
}

vbz_size_t max_svb_size(unsigned integer_size, vbz_size_t source_size)
{
    // vbz/v0/vbz_streamvbyte.cpp:7-18 == vbz/v1/vbz_streamvbyte.cpp:9-20
    if (source_size % integer_size != 0) return VBZ_INPUT_SIZE_ERROR;
    const uint32_t count = source_size / integer_size;
    return (vbz_size_t)((uint64_t)(count + 3) / 4 + 4ull * count);  // truncation to 32 bits as in the reference
}

}  // namespace

extern "C" {

bool vbz_is_error(vbz_size_t v) { return v >= VBZ_DEVICE_ERROR; }  // the reference's seven codes and the vbz_gpu.h extension

char const* vbz_error_string(vbz_size_t v)
{
    switch (v) {
    case VBZ_ZSTD_ERROR: return "VBZ_ZSTD_ERROR";
    case VBZ_INPUT_SIZE_ERROR: return "VBZ_INPUT_SIZE_ERROR";
    case VBZ_INTEGER_SIZE_ERROR: return "VBZ_INTEGER_SIZE_ERROR";
    case VBZ_DESTINATION_SIZE_ERROR: return "VBZ_DESTINATION_SIZE_ERROR";
    case VBZ_STREAMVBYTE_STREAM_ERROR: return "VBZ_STREAMVBYTE_STREAM_ERROR";
    case VBZ_VERSION_ERROR: return "VBZ_VERSION_ERROR";
    case VBZ_OUT_OF_MEMORY_ERROR: return "VBZ_OUT_OF_MEMORY_ERROR";
    case VBZ_DEVICE_ERROR: return "VBZ_DEVICE_ERROR";
    default: return "VBZ_UNKNOWN_ERROR";
    }
}

vbz_size_t vbz_max_compressed_size(vbz_size_t source_size, CompressionOptions const* o)
{
    if (!valid_int_size(o)) return VBZ_INTEGER_SIZE_ERROR;
    vbz_size_t max_size = source_size;
    if (o->integer_size != 0) {
        if (o->vbz_version > 1) return VBZ_VERSION_ERROR;
        max_size = max_svb_size(o->integer_size, max_size);
        if (vbz_is_error(max_size)) return max_size;
    }
    if (o->zstd_compression_level != 0) max_size = (vbz_size_t)zstd_bound(max_size);
    return max_size + 4;  // always room for the sized header (vbz.cpp:112-113)
}

vbz_size_t vbz_compress(void const* source, vbz_size_t source_size, void* destination, vbz_size_t destination_capacity,
                        CompressionOptions const* o)
{
    if (!valid_int_size(o)) return VBZ_INTEGER_SIZE_ERROR;
    if (o->integer_size != 0) {
        if (o->vbz_version > 1) return VBZ_VERSION_ERROR;
        const vbz_size_t max_svb = max_svb_size(o->integer_size, source_size);
        if (vbz_is_error(max_svb)) return max_svb;  // vbz.cpp:153-160
        if (o->zstd_compression_level == 0 && max_svb > destination_capacity) return VBZ_DESTINATION_SIZE_ERROR;
    } else if (o->zstd_compression_level == 0 && source_size > destination_capacity) {
        return VBZ_DESTINATION_SIZE_ERROR;
    }
    const vbz_size_t bound = vbz_max_compressed_size(source_size, o);
    const vbz_size_t dev_cap = destination_capacity < bound ? destination_capacity : bound;
    return run_one(true, source, source_size, destination, destination_capacity, dev_cap, o, 0);
}

vbz_size_t vbz_decompress(void const* source, vbz_size_t source_size, void* destination, vbz_size_t destination_size,
                          CompressionOptions const* o)
{
    if (!valid_int_size(o)) return VBZ_INTEGER_SIZE_ERROR;
    // the reference checks the version only after the zstd stage (vbz.cpp:282-290); an invalid version
    // can never succeed, so it is reported up front
    if (o->integer_size != 0 && o->vbz_version > 1) return VBZ_VERSION_ERROR;
    return run_one(false, source, source_size, destination, destination_size, destination_size, o, 0);
}

vbz_size_t vbz_compress_sized(void const* source, vbz_size_t source_size, void* destination, vbz_size_t destination_capacity,
                              CompressionOptions const* o)
{
    if (!valid_int_size(o)) return VBZ_INTEGER_SIZE_ERROR;
    if (destination_capacity < 4) return VBZ_DESTINATION_SIZE_ERROR;
    if (o->integer_size != 0) {
        if (o->vbz_version > 1) return VBZ_VERSION_ERROR;
        const vbz_size_t max_svb = max_svb_size(o->integer_size, source_size);
        if (vbz_is_error(max_svb)) return max_svb;  // NOTE: the reference returns this error + 4 (vbz.cpp:321-329)
        if (o->zstd_compression_level == 0 && max_svb > destination_capacity - 4) return VBZ_DESTINATION_SIZE_ERROR;
    } else if (o->zstd_compression_level == 0 && source_size > destination_capacity - 4) {
        return VBZ_DESTINATION_SIZE_ERROR;
    }
    const vbz_size_t bound = vbz_max_compressed_size(source_size, o);
    const vbz_size_t dev_cap = destination_capacity < bound ? destination_capacity : bound;
    return run_one(true, source, source_size, destination, destination_capacity, dev_cap, o, 1);
}

vbz_size_t vbz_decompress_sized(void const* source, vbz_size_t source_size, void* destination, vbz_size_t destination_capacity,
                                CompressionOptions const* o)
{
    if (!valid_int_size(o)) return VBZ_INTEGER_SIZE_ERROR;
    if (source_size < 4) return VBZ_INPUT_SIZE_ERROR;
    uint32_t original;
    memcpy(&original, source, 4);
    if (destination_capacity < original) return VBZ_DESTINATION_SIZE_ERROR;
    if (o->integer_size != 0 && o->vbz_version > 1) return VBZ_VERSION_ERROR;
    return run_one(false, source, source_size, destination, destination_capacity, destination_capacity, o, 1);
}

vbz_size_t vbz_decompressed_size(void const* source, vbz_size_t source_size, CompressionOptions const* o)
{
    if (!valid_int_size(o)) return VBZ_INTEGER_SIZE_ERROR;
    if (source_size < 4) return VBZ_INPUT_SIZE_ERROR;
    uint32_t original;
    memcpy(&original, source, 4);
    return original;
}

}  // extern "C"
