// scratch_tables_harness.cpp -- runs the carves of csrc/scratch_tables.h on the host, for tests/test_scratch_tables_host.py.
//
//   scratch_tables_harness CASE...      CASE = Table:d0[,d1[,d2]][:m]
//
// Per case: the measuring pass (base == nullptr), then -- unless the case ends in :m -- the carving pass into a malloc of exactly the
// measured size and a second one into another block, and a write to every element of every array.  Printed per case:
//   case <CASE> measured <bytes> [carved <bytes> null_when_measuring <0|1>]
//   array <name> <elem bytes> <count> <offset in the first block> <offset in the second>      (after a carving pass)
// The counts are the ones the structs document, written out here once more; the test holds them to its own statement of them.
// No HIP call is made: the program runs without a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scratch_tables.h"

using namespace vbzhip;

namespace {

struct Array
{
    const char* name;
    const void* p;
    size_t elem, count;
};
#define ARR(ptr, count) Array{ #ptr, (ptr), sizeof(*(ptr)), (size_t)(count) }

// every table: its carve over the case's dimensions, and its arrays with their documented counts
template <class T>
size_t carve(T& t, void* base, const std::vector<uint64_t>& d);
template <class T>
std::vector<Array> arrays(const T& t, const std::vector<uint64_t>& d);

#define PER_READ(T, ...)                                                                                                 \
    template <> size_t carve(T& t, void* base, const std::vector<uint64_t>& d) { return t.carve(base, (uint32_t)d[0]); } \
    template <> std::vector<Array> arrays(const T& t, const std::vector<uint64_t>& d)                                    \
    {                                                                                                                    \
        const size_t n = d[0];                                                                                           \
        (void)n;                                                                                                         \
        return { __VA_ARGS__ };                                                                                          \
    }
PER_READ(StageSlots, ARR(t.svb_off, n), ARR(t.svb_cap, n), ARR(t.svb_size, n), ARR(t.gate, n), ARR(t.deep_d, n), ARR(t.key_raw, n), ARR(t.gate2, n))
PER_READ(SplitTables, ARR(t.svb_off, n), ARR(t.svb_cap, n), ARR(t.gate, n), ARR(t.svb_size, n))
PER_READ(CanonGates, ARR(t.counts, 4), ARR(t.gate_small, n), ARR(t.gate_large, n))
PER_READ(TypedSlots, ARR(t.off16, n), ARR(t.cap16, n), ARR(t.cal, n))
PER_READ(NormTables, ARR(t.st, n), ARR(t.ss, n))
PER_READ(SizedTables, ARR(t.pay_off, n), ARR(t.pay_size, n), ARR(t.orig_size, n), ARR(t.gate, n))
PER_READ(WindowScratch, ARR(t.scan, n + 1), ARR(t.count, n))

template <> size_t carve(SegTables& t, void* base, const std::vector<uint64_t>& d) { return t.carve(base, (uint32_t)d[0], (uint32_t)d[1]); }
template <> std::vector<Array> arrays(const SegTables& t, const std::vector<uint64_t>& d)
{
    const size_t n = d[0], segs = d[1];
    return { ARR(t.first, n + 1), ARR(t.gate, n), ARR(t.val, segs), ARR(t.off, segs), ARR(t.run, segs) };
}

template <> size_t carve(RouteTables& t, void* base, const std::vector<uint64_t>& d) { return t.carve(base, (uint32_t)d[0], (uint32_t)d[1], (size_t)d[2]); }
template <> std::vector<Array> arrays(const RouteTables& t, const std::vector<uint64_t>& d)
{
    const size_t n = d[0], m = d[1], cand = d[2];
    return { ARR(t.gate_small, n),  ARR(t.large.src_off, m), ARR(t.large.dst_off, m), ARR(t.large.src_size, m), ARR(t.large.dst_cap, m),
             ARR(t.large.gate, m),  ARR(t.result, m),        ARR(t.large.map, m),     ARR(t.large.cal, m),      ARR(t.large.row, m),
             ARR(t.norm, m),        ARR(t.large.count, 4),   ARR(t.cand, cand) };
}

template <> size_t carve(Pod5Tables& t, void* base, const std::vector<uint64_t>& d) { return t.carve(base, (uint32_t)d[0], (uint32_t)d[1]); }
template <> std::vector<Array> arrays(const Pod5Tables& t, const std::vector<uint64_t>& d)
{
    const size_t rows = d[0], R = d[1];
    return { ARR(t.pr.bad, 4), ARR(t.pr.rows, rows), ARR(t.pr.reads, R), ARR(t.cal, R), ARR(t.pr.range, R) };
}

template <class T>
int run(const std::string& name, const std::vector<uint64_t>& d, bool measure_only)
{
    T t;
    const size_t measured = carve(t, nullptr, d);
    bool all_null = true;
    for (const Array& a : arrays(t, d)) all_null = all_null && a.p == nullptr;
    if (measure_only) {
        printf("case %s measured %zu null_when_measuring %d\n", name.c_str(), measured, (int)all_null);
        return 0;
    }
    uint8_t* b0 = (uint8_t*)malloc(measured);
    uint8_t* b1 = (uint8_t*)malloc(measured + 4096);   // (another size: another place)
    if (!b0 || !b1) return 1;
    T u;
    const size_t carved = carve(t, b0, d);
    carve(u, b1, d);
    printf("case %s measured %zu carved %zu null_when_measuring %d\n", name.c_str(), measured, carved, (int)all_null);
    const std::vector<Array> a0 = arrays(t, d), a1 = arrays(u, d);
    for (size_t i = 0; i < a0.size(); ++i) {
        printf("array %s %zu %zu %td %td\n", a0[i].name, a0[i].elem, a0[i].count, (const uint8_t*)a0[i].p - b0, (const uint8_t*)a1[i].p - b1);
        memset(const_cast<void*>(a0[i].p), 0xA5, a0[i].elem * a0[i].count);   // every element of the array, inside a block of exactly the measured size
    }
    free(b0);
    free(b1);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; ++i) {
        const std::string c = argv[i];
        const size_t c1 = c.find(':'), c2 = c.find(':', c1 + 1);
        if (c1 == std::string::npos) return 2;
        const std::string table = c.substr(0, c1), dims = c.substr(c1 + 1, c2 == std::string::npos ? std::string::npos : c2 - c1 - 1);
        const bool m = c2 != std::string::npos;
        std::vector<uint64_t> d;
        for (size_t p = 0; p <= dims.size();) {
            const size_t q = std::min(dims.find(',', p), dims.size());
            d.push_back(strtoull(dims.substr(p, q - p).c_str(), nullptr, 0));
            p = q + 1;
        }
        d.resize(3, 0);
        int rc = 2;
#define TABLE(T) if (table == #T) rc = run<T>(c, d, m);
        TABLE(SegTables) TABLE(StageSlots) TABLE(RouteTables) TABLE(SplitTables) TABLE(CanonGates) TABLE(TypedSlots) TABLE(NormTables)
        TABLE(SizedTables) TABLE(WindowScratch) TABLE(Pod5Tables)
        if (rc != 0) {
            fprintf(stderr, "scratch_tables_harness: case %s failed (%d)\n", c.c_str(), rc);
            return rc;
        }
    }
    return 0;
}
