// eventalign.hip -- the two links between the event calls and the alignment calls (the rules: include/vbz_gpu.h).
//   vbz_gpu_events_query_batch:  the ragged table of event records -> the dense [n_reads, N] query arena the locate calls take, events
//                                with n < min_n dropped: a stream compaction per read.
//   vbz_gpu_locate_levels_batch: the path of a located pair, one {begin, end} per query entry -> one record per TARGET level with the
//                                samples that belong to it and their exact moments: the inversion of the path and the segmented sum.
// Both are one wavefront per read / pair, four to a workgroup of 256: very short reads dominate a real batch, and a wavefront that has
// nothing to do leaves at once.  No LDS, no barrier, no atomics, no scratch: lanes talk through ballots and shuffles alone.
#include "vbz_kernels.h"

namespace vbzhip {
namespace {

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The rows of read `read` under an untrusted event_first: false, with nothing formed from the two entries, for a descending pair, a pair
// behind event_rows, or more than 2^31 - 1 rows.
__device__ __forceinline__ bool event_rows_of(const uint64_t* __restrict__ event_first, uint64_t event_rows, uint32_t read, uint64_t& c0, uint32_t& rows)
{
    c0 = event_first[read];
    const uint64_t c1 = event_first[read + 1];
    if (c0 > c1 || c1 > event_rows || c1 - c0 > 0x7FFFFFFFull) return false;
    rows = (uint32_t)(c1 - c0);
    return true;
}

// Zero the dwords [from, N) of a 16-byte aligned row of N % 4 == 0 dwords: single dwords up to the next multiple of 4, 16-byte stores
// behind it.
__device__ __forceinline__ void zero_tail(uint32_t* __restrict__ row, uint32_t from, uint32_t N, uint32_t lane)
{
    const uint32_t up = (from + 3u) & ~3u;   // (<= N, N being a multiple of 4)
    if (from + lane < up) row[from + lane] = 0u;
    uint4* const row4 = reinterpret_cast<uint4*>(row);
    for (uint32_t k = up / 4u + lane; k < N / 4u; k += 64u) row4[k] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- vbz_gpu_events_query_batch ---------------------------------------------------------------------------------------------------------
// A turn is 64 rows of the read: one 16-byte load a lane, the keep mask by a ballot, a lane's rank among the kept by mbcnt, one store (two
// with the index) per survivor.  The count is wave-uniform, so the wavefront leaves as soon as N are kept and reads nothing behind that
// turn; the same wavefront writes the zero tail.
__global__ __launch_bounds__(256) void events_query_kernel(uint32_t n_reads, const uint32_t* __restrict__ result, const uint64_t* __restrict__ event_first,
                                                           uint64_t event_rows, const uint4* __restrict__ records, uint32_t min_n, uint32_t N,
                                                           uint32_t* __restrict__ query, uint32_t* __restrict__ valid, uint32_t* __restrict__ index)
{
    const uint32_t read = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (read >= n_reads) return;
    uint64_t c0 = 0;
    uint32_t rows = 0;
    if (!event_rows_of(event_first, event_rows, read, c0, rows) || (result && result[read] >= E_FIRST)) rows = 0;
    uint32_t* const q = query + (size_t)read * N;
    uint32_t* const ix = index ? index + (size_t)read * N : nullptr;
    uint32_t kept = 0;
    for (uint32_t base = 0; base < rows && kept < N; base += 64u) {
        const uint32_t r = base + lane;   // (rows < 2^31: no wrap)
        bool keep = false;
        uint32_t mean = 0;
        if (r < rows) {
            const uint4 rec = records[c0 + r];
            keep = rec.z >= min_n;
            mean = rec.x;
        }
        const uint64_t mask = __ballot(keep);
        const uint32_t pos = kept + lanes_below(mask);
        if (keep && pos < N) {
            q[pos] = mean;
            if (ix) ix[pos] = r;
        }
        kept += (uint32_t)__popcll(mask);
    }
    kept = kept < N ? kept : N;
    zero_tail(q, kept, N, lane);
    if (ix) zero_tail(ix, kept, N, lane);
    if (lane == 0) valid[read] = kept;
}

// ---- vbz_gpu_locate_levels_batch --------------------------------------------------------------------------------------------------------
struct LevelsArgs
{
    uint32_t n_pairs, n_reads, N, max_width;
    const uint4* pairs;           // {read, target, begin, end}: read alone is used
    const uint4* hit;             // {cost, end, start, n}
    const uint2* rows;            // [n_pairs, N] {begin, end}
    const uint32_t* index;        // [n_reads, N] or nullptr: entry k is row k
    const uint64_t* event_first;  // [n_reads + 1]
    uint64_t event_rows;
    const uint32_t* start;        // [event_rows]
    const uint4* records;         // [event_rows] {mean, sd, n, 0}
    const uint4* moments;         // [event_rows] {S1 lo, S1 hi, S2 lo, S2 hi}
    uint32_t* n_levels;           // [n_pairs]
    uint4* levels;                // [n_pairs, max_width] of two 16-byte halves
};

template <typename T>
__device__ __forceinline__ T wave_inclusive_sum(T v, uint32_t lane)
{
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const T below = __shfl_up(v, o);
        if (lane >= o) v += below;
    }
    return v;
}

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return (uint64_t)hi << 32 | lo; }

__device__ __forceinline__ void store_level(uint4* __restrict__ lv, uint32_t t, uint32_t first, uint32_t end, uint32_t ns, uint32_t ne, uint64_t s1, uint64_t s2)
{
    lv[2u * (size_t)t] = make_uint4(first, end, ns, ne);
    lv[2u * (size_t)t + 1u] = make_uint4((uint32_t)s1, (uint32_t)(s1 >> 32), (uint32_t)s2, (uint32_t)(s2 >> 32));
}

// The form built is the difference of two prefix values, with no prefix array anywhere.  A level j holds the entries [k0, k1).  Its LAST
// entry k1 - 1 is the one entry k with begin_k <= j < min(end_k, begin_{k+1}) -- every level has exactly one -- and that lane writes the
// record.  It holds the inclusive sums up to itself (a wave scan of n, S1, S2 with a carried total: 64 entries a turn); what it lacks is the
// exclusive sums and the start of the level's FIRST entry k0.  Of the levels an entry is last for, all but the first, begin_k, hold that
// entry alone.  For begin_k: k0 = k when the step into k was diagonal (begin_k == end_{k-1}); otherwise it is the first entry of the last
// level of entry k - 1, F(k - 1), where F(k) = k when end_k > end_{k-1} (the entry opens its last level) and F(k - 1) otherwise -- a stall
// of any length passes one value along.  F is a running maximum: one more wave scan, and the values of entry F come by one shuffle, or
// from the carry when the stall began in an earlier turn.  So a turn costs the same whatever the path looks like, a level holding 2 048
// entries included; an entry that spans many levels writes the first eight behind begin_k itself and the wavefront writes the rest
// together, 64 levels a step: O(n + width) a pair.
// Pass 1 reads the whole path and the index before anything is written: a pair that breaks a rule anywhere gets zeros everywhere, and
// pass 2 forms addresses from checked values alone.
constexpr uint32_t LEVELS_OWN = 8;   // levels behind begin_k that a lane writes alone

__global__ __launch_bounds__(256) void locate_levels_kernel(LevelsArgs a)
{
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (p >= a.n_pairs) return;
    const uint4 pr = a.pairs[p], h = a.hit[p];
    const uint32_t read = pr.x, end = h.y, start = h.z, n = h.w;
    bool ok = read < a.n_reads && n >= 1u && n <= a.N && start < end && end - start <= a.max_width;
    uint64_t c0 = 0;
    uint32_t nrows = 0;
    if (ok) ok = event_rows_of(a.event_first, a.event_rows, read, c0, nrows);
    const uint2* const prow = a.rows + (size_t)p * a.N;
    const uint32_t* const pidx = (ok && a.index) ? a.index + (size_t)read * a.N : nullptr;

    for (uint32_t base = 0; ok && base < n; base += 64u) {   // pass 1: the invariants of the path, the index
        const uint32_t k = base + lane;
        bool good = true;
        if (k < n) {
            const uint2 r = prow[k];
            good = r.x < r.y;
            if (k == 0u) good = good && r.x == start;
            else {
                const uint32_t pe = prow[k - 1u].y;
                good = good && (r.x == pe || r.x + 1u == pe);   // (pe == 0 fails entry k - 1 itself)
            }
            if (k == n - 1u) good = good && r.y == end;
            const uint32_t idx = pidx ? pidx[k] : k;
            good = good && idx < nrows;
        }
        ok = __ballot(!good) == 0;
    }

    uint4* const lv = a.levels + 2u * (size_t)p * a.max_width;
    const uint32_t width = ok ? end - start : 0u;
    if (ok) {   // pass 2
        uint32_t tot_n = 0;            // the inclusive sums of every earlier turn
        uint64_t tot_s1 = 0, tot_s2 = 0;
        uint32_t car_k = 0, car_first = 0, car_n = 0;   // entry F of the last entry of the earlier turns: its number, its event's start,
        uint64_t car_s1 = 0, car_s2 = 0;                // its exclusive sums
        for (uint32_t base = 0; base < n; base += 64u) {
            const uint32_t k = base + lane;
            const bool in = k < n;
            uint2 r = make_uint2(0u, 0u);
            uint32_t pe = 0, nb = 0, ev_start = 0, ev_n = 0;
            uint64_t s1 = 0, s2 = 0;
            if (in) {
                r = prow[k];
                pe = k != 0u ? prow[k - 1u].y : 0u;
                nb = k + 1u < n ? prow[k + 1u].x : end;
                const uint64_t c = c0 + (pidx ? pidx[k] : k);
                ev_start = a.start[c];
                ev_n = a.records[c].z;
                const uint4 m = a.moments[c];
                s1 = u64_of(m.x, m.y);
                s2 = u64_of(m.z, m.w);
            }
            const uint32_t inc_n = tot_n + wave_inclusive_sum(ev_n, lane);
            const uint64_t inc_s1 = tot_s1 + wave_inclusive_sum(s1, lane), inc_s2 = tot_s2 + wave_inclusive_sum(s2, lane);
            const bool opens = in && (k == 0u || r.y > pe);   // F(k) == k
            uint32_t f = opens ? k + 1u : 0u;                 // F(k) + 1 as a running maximum; 0: in an earlier turn
#pragma unroll
            for (uint32_t o = 1; o < 64u; o <<= 1) {
                const uint32_t below = __shfl_up(f, o);
                if (lane >= o && below > f) f = below;
            }
            // the first entry of level begin_k: itself behind a diagonal step, F(k - 1) behind a vertical one
            const uint32_t fprev = __shfl_up(f, 1u);
            const bool diag = k == 0u || r.x == pe;
            const uint32_t want = diag ? k + 1u : (lane == 0u ? 0u : fprev);
            const uint32_t src = want != 0u ? want - 1u - base : lane;   // (want - 1 >= base: it was set in this turn)
            const uint32_t g_first = __shfl(ev_start, src), g_n = __shfl(inc_n - ev_n, src);
            const uint64_t g_s1 = __shfl(inc_s1 - s1, src), g_s2 = __shfl(inc_s2 - s2, src);
            const bool own = want != 0u;
            const uint32_t k0 = own ? want - 1u : car_k, first = own ? g_first : car_first, ex_n = own ? g_n : car_n;
            const uint64_t ex_s1 = own ? g_s1 : car_s1, ex_s2 = own ? g_s2 : car_s2;

            const uint32_t top = r.y < nb ? r.y : nb;           // the entry is the last of levels [begin_k, top)
            const uint32_t span = in && top > r.x ? top - r.x : 0u;
            const uint32_t t0 = r.x - start, ev_end = ev_start + ev_n;
            if (span != 0u) {
                store_level(lv, t0, first, ev_end, inc_n - ex_n, k + 1u - k0, inc_s1 - ex_s1, inc_s2 - ex_s2);
                const uint32_t mine = span - 1u < LEVELS_OWN ? span - 1u : LEVELS_OWN;
                for (uint32_t e = 1; e <= mine; ++e) store_level(lv, t0 + e, ev_start, ev_end, ev_n, 1u, s1, s2);
            }
            for (uint64_t wide = __ballot(span > LEVELS_OWN + 1u); wide != 0; wide &= wide - 1u) {   // a long skip: the wavefront together
                const uint32_t w = (uint32_t)__builtin_ctzll(wide);
                const uint32_t w_t0 = __shfl(t0, w), w_span = __shfl(span, w), w_start = __shfl(ev_start, w), w_end = __shfl(ev_end, w),
                               w_n = __shfl(ev_n, w);
                const uint64_t w_s1 = __shfl(s1, w), w_s2 = __shfl(s2, w);
                for (uint32_t e = LEVELS_OWN + 1u + lane; e < w_span; e += 64u) store_level(lv, w_t0 + e, w_start, w_end, w_n, 1u, w_s1, w_s2);
            }

            const uint32_t f_last = __shfl(f, 63u);
            if (f_last != 0u) {   // an entry of this turn opened a level: it is what a stall into the next turn refers to
                const uint32_t s = f_last - 1u - base;
                car_k = f_last - 1u;
                car_first = __shfl(ev_start, s);
                car_n = __shfl(inc_n - ev_n, s);
                car_s1 = __shfl(inc_s1 - s1, s);
                car_s2 = __shfl(inc_s2 - s2, s);
            }
            tot_n = __shfl(inc_n, 63u);
            tot_s1 = __shfl(inc_s1, 63u);
            tot_s2 = __shfl(inc_s2, 63u);
        }
    }
    for (size_t k = 2u * (size_t)width + lane; k < 2u * (size_t)a.max_width; k += 64u) lv[k] = make_uint4(0u, 0u, 0u, 0u);
    if (lane == 0) a.n_levels[p] = width;
}

}  // namespace

hipError_t launch_events_query(uint32_t n_reads, const uint32_t* result, const uint64_t* event_first, uint64_t event_rows, const void* records, uint32_t min_n,
                               uint32_t N, float* query, uint32_t* valid, uint32_t* index, hipStream_t s)
{
    if (n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(events_query_kernel, dim3((n_reads + 3u) / 4u), dim3(256), 0, s, n_reads, result, event_first, event_rows,
                       reinterpret_cast<const uint4*>(records), min_n, N, reinterpret_cast<uint32_t*>(query), valid, index);
    return hipGetLastError();
}

hipError_t launch_locate_levels(uint32_t n_pairs, uint32_t n_reads, uint32_t N, uint32_t max_width, const void* pairs, const void* hit, const void* rows,
                                const uint32_t* index, const uint64_t* event_first, uint64_t event_rows, const uint32_t* start, const void* records,
                                const void* moments, uint32_t* n_levels, void* levels, hipStream_t s)
{
    if (n_pairs == 0) return hipSuccess;
    LevelsArgs a;
    a.n_pairs = n_pairs;
    a.n_reads = n_reads;
    a.N = N;
    a.max_width = max_width;
    a.pairs = reinterpret_cast<const uint4*>(pairs);
    a.hit = reinterpret_cast<const uint4*>(hit);
    a.rows = reinterpret_cast<const uint2*>(rows);
    a.index = index;
    a.event_first = event_first;
    a.event_rows = event_rows;
    a.start = start;
    a.records = reinterpret_cast<const uint4*>(records);
    a.moments = reinterpret_cast<const uint4*>(moments);
    a.n_levels = n_levels;
    a.levels = reinterpret_cast<uint4*>(levels);
    hipLaunchKernelGGL(locate_levels_kernel, dim3((n_pairs + 3u) / 4u), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace vbzhip
