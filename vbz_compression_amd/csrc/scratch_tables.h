// scratch_tables.h -- the multi-array layouts of the host's device scratch (host only; vbz_api.hip).
//
// Every table is a set of arrays carved out of ONE device buffer by its carve(): with base == nullptr the carve measures (every pointer
// stays null), with the buffer's base the SAME take<>() calls place the arrays, and both return what to allocate (MetaCarver::bytes(): the
// arrays, each 16-byte aligned, and a quarter more + 512 bytes of headroom).  A buffer is sized by the carve that fills it and by nothing
// else (ensure_carved in vbz_api.hip): an array added to a carve is an array allocated.  The counts are in elements, [n] per read of the
// call unless stated; a count is widened to size_t before it is added to (n + 1 of 2^32 - 1 reads does not wrap).
// tests/test_scratch_tables_host.py holds every table to its documented counts (tests/host/scratch_tables_harness.cpp).
#pragma once

#include <stddef.h>

#include "vbz_kernels.h"

namespace vbzhip {

// n elements for each of the arrays, in the order given
template <class... T>
size_t carve_each(void* base, size_t n, T*&... arrays)
{
    MetaCarver mc(base);
    ((arrays = mc.take<T>(n)), ...);
    return mc.bytes();
}

// The segment tables of a launch group on the large-read path (launch_seg_plan)
struct SegTables
{
    uint32_t* first = nullptr;  // [n + 1]
    uint32_t* gate = nullptr;   // [n]: the input gate, plus E_OOM for reads whose segments do not fit the tables
    uint32_t* val = nullptr;    // [max_segs]
    uint64_t* off = nullptr;    // [max_segs]
    uint32_t* run = nullptr;    // [max_segs]
    uint32_t max_segs = 0;
    size_t carve(void* base, uint32_t n, uint32_t segs)
    {
        MetaCarver mc(base);
        max_segs = segs;
        first = mc.take<uint32_t>((size_t)n + 1);
        gate = mc.take<uint32_t>(n);
        val = mc.take<uint32_t>(segs);
        off = mc.take<uint64_t>(segs);
        run = mc.take<uint32_t>(segs);
        return mc.bytes();
    }
};

// The per-read arrays of a launch group's intermediate svb streams
struct StageSlots
{
    uint64_t* svb_off = nullptr;
    uint32_t *svb_cap = nullptr, *svb_size = nullptr, *gate = nullptr;
    uint32_t *deep_d = nullptr, *key_raw = nullptr, *gate2 = nullptr;   // encode: the matcher's distances, POD5's key sizes, the spans' gate
    size_t carve(void* base, uint32_t n) { return carve_each(base, n, svb_off, svb_cap, svb_size, gate, deep_d, key_raw, gate2); }
};

// Per-read routing (launch_route_reads): the first group's gate, the compact table of the routed reads (max_reads entries each), the
// candidates' scratch (cand_words = route_cand_words())
struct RouteTables
{
    uint32_t* gate_small = nullptr;   // [n]
    RoutedTable large;                // [max_reads] each; count: [4]
    uint32_t* result = nullptr;       // [max_reads]: the routed reads' results (launch_route_results scatters them)
    NormRead* norm = nullptr;         // [max_reads]: their states of a normalising decode
    uint32_t* cand = nullptr;         // [cand_words]
    size_t carve(void* base, uint32_t n, uint32_t max_reads, size_t cand_words)
    {
        MetaCarver mc(base);
        gate_small = mc.take<uint32_t>(n);
        large.src_off = mc.take<uint64_t>(max_reads);
        large.dst_off = mc.take<uint64_t>(max_reads);
        large.src_size = mc.take<uint32_t>(max_reads);
        large.dst_cap = mc.take<uint32_t>(max_reads);
        large.gate = mc.take<uint32_t>(max_reads);
        result = mc.take<uint32_t>(max_reads);
        large.map = mc.take<uint32_t>(max_reads);
        large.cal = mc.take<float2>(max_reads);
        large.row = mc.take<uint64_t>(max_reads);
        norm = mc.take<NormRead>(max_reads);
        large.count = mc.take<uint32_t>(4);
        cand = mc.take<uint32_t>(cand_words);
        return mc.bytes();
    }
};

// The scratch plan of a whole batch that is coded as two halves (split_plan)
struct SplitTables
{
    uint64_t* svb_off = nullptr;
    uint32_t *svb_cap = nullptr, *gate = nullptr, *svb_size = nullptr;
    size_t carve(void* base, uint32_t n) { return carve_each(base, n, svb_off, svb_cap, gate, svb_size); }
};

// Canonical encoding: the classification's counts and the two groups' gates (launch_canon_classify)
struct CanonGates
{
    uint32_t* counts = nullptr;   // [4]
    uint32_t *gate_small = nullptr, *gate_large = nullptr;
    size_t carve(void* base, uint32_t n)
    {
        MetaCarver mc(base);
        counts = mc.take<uint32_t>(4);
        gate_small = mc.take<uint32_t>(n);
        gate_large = mc.take<uint32_t>(n);
        return mc.bytes();
    }
};

// Typed decode: the int16 slot table made from the caller's typed one, and the per-read constants (launch_signal_slots)
struct TypedSlots
{
    uint64_t* off16 = nullptr;
    uint32_t* cap16 = nullptr;
    float2* cal = nullptr;
    size_t carve(void* base, uint32_t n) { return carve_each(base, n, off16, cap16, cal); }
};

// Normalising decode: the reads' states, and a shift_scale table of the call's own for a caller that passed none
struct NormTables
{
    NormRead* st = nullptr;
    float2* ss = nullptr;
    size_t carve(void* base, uint32_t n) { return carve_each(base, n, st, ss); }
};

// Sized decode: what the 4-byte headers say (launch_parse_sized)
struct SizedTables
{
    uint64_t* pay_off = nullptr;
    uint32_t *pay_size = nullptr, *orig_size = nullptr, *gate = nullptr;
    size_t carve(void* base, uint32_t n) { return carve_each(base, n, pay_off, pay_size, orig_size, gate); }
};

// A call over POD5 reads of several rows: the carved part of Pod5Reads (the caller's tables are filled in by pod5_reads_begin) and the
// reads' constants
struct Pod5Tables
{
    Pod5Reads pr;          // bad: [4], rows: [n_rows], reads / range: [n_reads]
    float2* cal = nullptr; // [n_reads]
    size_t carve(void* base, uint32_t n_rows, uint32_t n_reads)
    {
        MetaCarver mc(base);
        pr.bad = mc.take<uint32_t>(4);
        pr.rows = mc.take<Pod5Row>(n_rows);
        pr.reads = mc.take<Pod5Read>(n_reads);
        cal = mc.take<float2>(n_reads);
        pr.range = mc.take<uint2>(n_reads);
        return mc.bytes();
    }
};

// One group of a path call (launch_match_path_forward, launch_match_path_trace): the pairs' direction bits, pair_words words a pair
// (match_path_groups.h), and the forward pass's costs
struct MatchPathScratch
{
    uint32_t* bits = nullptr;   // [pairs x pair_words]
    uint32_t* cost = nullptr;   // [pairs]
    size_t carve(void* base, uint32_t pairs, uint64_t pair_words)
    {
        MetaCarver mc(base);
        bits = mc.take<uint32_t>((size_t)pairs * (size_t)pair_words);
        cost = mc.take<uint32_t>(pairs);
        return mc.bytes();
    }
};

// One array of n elements in a buffer of its own: what to allocate for it
template <typename T>
size_t array_bytes(size_t n)
{
    T* a;
    return carve_each(nullptr, n, a);
}

}  // namespace vbzhip
