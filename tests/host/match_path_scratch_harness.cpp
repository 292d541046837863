// match_path_scratch_harness.cpp -- runs the carve of MatchPathScratch (csrc/scratch_tables.h) on the host, for
// tests/test_match_path_scratch_host.py, in the format of scratch_tables_harness.cpp:
//
//   match_path_scratch_harness CASE...      CASE = MatchPathScratch:pairs,max_width,ref_stride[:m]
//
// Per case: the measuring pass (base == nullptr), then -- unless the case ends in :m -- the carving pass into a malloc of exactly the
// measured size and a second one into another block, and a write to every element of every array.  Printed per case:
//   case <CASE> measured <bytes> [carved <bytes>] null_when_measuring <0|1>
//   array <name> <elem bytes> <count> <offset in the first block> <offset in the second>      (after a carving pass)
// The words a pair takes are match_path_groups.h's, from max_width and ref_stride.  No HIP call is made: the program runs without a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "match_path_groups.h"
#include "scratch_tables.h"

using namespace vbzhip;

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; ++i) {
        const std::string c = argv[i];
        unsigned long long pairs = 0, width = 0, stride = 0;
        char tail[4] = "";
        const int got = sscanf(c.c_str(), "MatchPathScratch:%llu,%llu,%llu%3s", &pairs, &width, &stride, tail);
        if (got < 3) return 2;
        const bool measure_only = strcmp(tail, ":m") == 0;
        const uint64_t words = match_path_pair_words((uint32_t)width, (uint32_t)stride);
        MatchPathScratch t, u;
        const size_t measured = t.carve(nullptr, (uint32_t)pairs, words);
        const bool all_null = t.bits == nullptr && t.cost == nullptr;
        if (measure_only) {
            printf("case %s measured %zu null_when_measuring %d\n", c.c_str(), measured, (int)all_null);
            continue;
        }
        uint8_t* b0 = (uint8_t*)malloc(measured);
        uint8_t* b1 = (uint8_t*)malloc(measured + 4096);   // (another size: another place)
        if (!b0 || !b1) return 1;
        const size_t carved = t.carve(b0, (uint32_t)pairs, words);
        u.carve(b1, (uint32_t)pairs, words);
        printf("case %s measured %zu carved %zu null_when_measuring %d\n", c.c_str(), measured, carved, (int)all_null);
        const size_t n_bits = (size_t)pairs * (size_t)words;
        printf("array t.bits %zu %zu %td %td\n", sizeof(*t.bits), n_bits, (uint8_t*)t.bits - b0, (uint8_t*)u.bits - b1);
        printf("array t.cost %zu %zu %td %td\n", sizeof(*t.cost), (size_t)pairs, (uint8_t*)t.cost - b0, (uint8_t*)u.cost - b1);
        memset(t.bits, 0xA5, n_bits * sizeof(*t.bits));   // every element, inside a block of exactly the measured size
        memset(t.cost, 0xA5, (size_t)pairs * sizeof(*t.cost));
        free(b0);
        free(b1);
    }
    return 0;
}
