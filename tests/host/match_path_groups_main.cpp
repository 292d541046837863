// Stand-alone sweep of vbz_compression_amd/csrc/match_path_groups.h (tests only; built by tests/test_match_path_groups_host.py with the
// address and undefined-behaviour sanitizers): over every (max_width, ref_stride) inside the header's limits and caps from tiny to huge,
// a group has at least one pair and no more than the call, its direction bits stay within the cap whenever one pair fits, the words of a
// pair cover every word the forward kernel stores for any reference length up to ref_stride, nothing wraps in 32 bits, and the packed / wide
// choice for max_width is the no-wrap inequality recomputed in 64 bits.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "match_path_groups.h"
#include "match_select.h"

using namespace vbzhip;

static void fail(const char* what, uint64_t W, uint64_t S, uint64_t cap)
{
    std::printf("FAIL %s max_width %llu stride %llu cap %llu\n", what, (unsigned long long)W, (unsigned long long)S, (unsigned long long)cap);
    std::exit(1);
}

int main()
{
    const uint64_t caps[] = { 0, 1, 255, 4096, 1u << 20, UINT64_C(1) << 30, UINT64_C(1) << 34, UINT64_C(1) << 46, ~UINT64_C(0) };
    const uint32_t counts[] = { 1u, 2u, 8192u, 0xFFFFFFFFu };
    uint64_t cases = 0, packed = 0, wide = 0;
    for (uint64_t S = 16; S <= 2048; S += 16) {
        const uint32_t c = match_rows_per_lane((uint32_t)S);
        if ((c & (c - 1)) != 0 || c > 32 || UINT64_C(64) * c < S || (c > 1 && UINT64_C(64) * (c / 2) >= S)) fail("rows per lane", 0, S, 0);
        for (uint32_t M = 1; M <= S; M += (M < 130 ? 1 : 61))
            if (match_rows_per_lane(M) > c) fail("a shorter reference with more rows a lane", M, S, 0);
        for (uint64_t W = 8; W <= 65536; W += 8) {
            const uint64_t words = match_path_pair_words((uint32_t)W, (uint32_t)S);
            // the last word any lane stores: steps <= W + 63, c cells a step, 16 cells a word, word g of lane l at g * 64 + l
            const uint64_t last = ((W + 63) * c - 1) / 16 * 64 + 63;
            if (words <= last || words % 64 != 0 || words * 4 > UINT64_C(16) * c * (W + 63) + 256) fail("pair words", W, S, 0);
            if ((uint64_t)(uint32_t)last != last) fail("a word index beyond 32 bits", W, S, 0);
            // the packed / wide choice with max_width in N's place, recomputed from the fields' definitions
            const uint32_t sb = match_span_start_bits((uint32_t)W);
            const bool sound = W - 1 < (UINT64_C(1) << sb) && ((UINT64_C(255) * S << sb) | (W - 1)) < (UINT64_C(1) << 31) &&
                               (UINT64_C(1) << 31) + 63 * 255 * (UINT64_C(1) << sb) < (UINT64_C(1) << 32);
            if (match_span_packed((uint32_t)W, (uint32_t)S)) {
                ++packed;
                if (!sound) fail("packed where the key can wrap", W, S, 0);
            } else {
                ++wide;
                if (UINT64_C(255) * S < (UINT64_C(1) << (31 - sb))) fail("wide inside the packed rule", W, S, 0);
            }
            if (W % 64 != 8 && W != 65536) continue;   // (the group rule: a sixth of the widths and the last)
            for (uint64_t cap : caps)
                for (uint32_t n : counts) {
                    const uint32_t g = match_path_group_pairs(n, (uint32_t)W, (uint32_t)S, cap);
                    ++cases;
                    if (g < 1 || g > n) fail("group outside 1 ... n_pairs", W, S, cap);
                    const uint64_t bytes = (uint64_t)g * words * 4;
                    if (bytes / 4 / words != g) fail("group bytes wrap", W, S, cap);
                    if (words * 4 <= cap && bytes > cap) fail("group beyond the cap", W, S, cap);
                    if (words * 4 > cap && g != 1) fail("a pair larger than the cap does not run alone", W, S, cap);
                    if (g < n && (uint64_t)(g + UINT64_C(1)) * words * 4 <= cap) fail("group smaller than the cap allows", W, S, cap);
                }
        }
    }
    // arguments outside every limit: the functions are total
    const uint32_t odd[] = { 0u, 1u, 7u, 65537u, 1u << 31, 0xFFFFFFFFu };
    for (uint32_t W : odd)
        for (uint32_t S : odd)
            for (uint64_t cap : caps) {
                const uint32_t g = match_path_group_pairs(W, W, S, cap);
                if (g < 1 || match_rows_per_lane(S) > 32 || match_path_pair_words(W, S) == 0) fail("outside the limits", W, S, cap);
            }
    std::printf("ok cases %llu packed %llu wide %llu\n", (unsigned long long)cases, (unsigned long long)packed, (unsigned long long)wide);
    return 0;
}
