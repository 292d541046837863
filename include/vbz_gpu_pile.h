/* vbz_gpu_pile.h -- the pile-up across reads: per-position and per-k-mer sums, a model update.  The entry points of include/vbz_gpu.h are
 * a closed, recorded set (tests/golden/prototypes.json is a yardstick no change edits), so these four are declared here, in a header of
 * their own that includes that one; they live in the same library and take the same context.
 *
 * Every table of the event-space chain of vbz_gpu.h belongs to one read.  These calls add reads up, on the device, and close the outer
 * loop with nothing crossing to the host:
 *   squiggle(model) -> [segment ... locate_levels] -> levels_fit -> levels_pile -> pile_kmers -> model_update -> squiggle(new model) -> ...
 * The pile arena.  A pile is four planes of 64-bit words over cells: plane q of cell c is pile[q * n_cells + c], the arena 16-byte
 * aligned.  Plane 0 is the count word n + 2^32 * skipped, added to as ONE 64-bit number; plane 1 n_samples; plane 2 sum, an int64 in
 * two's complement; plane 3 sumsq.  Every add is modulo 2^64.  The position pile has n_cells = G * target_stride and cell g *
 * target_stride + j; the k-mer pile has n_cells = 4^k.  Planes, not 32-byte records: 64 lanes on consecutive cells make one contiguous
 * 512-byte atomic instruction per plane.
 * vbz_gpu_levels_pile_batch: the levels of every pair added into their target positions.  The rule (tests/pile_ref.py).  locate, pairs, hit,
 * n_levels and levels ([n_pairs, max_width]) are exactly what vbz_gpu_levels_fit_batch takes, fit the vbz_gpu_level_fit table it wrote, or
 * NULL.  A pair is valid by exactly that call's test -- invalid when read >= n_reads; ref >= G; W == 0 or W > max_width; end - start != W;
 * L_g == 0 or L_g > target_stride; end > L_g -- and the kernels share the function.  The pair's constants are o = fit[p].offset and s =
 * fit[p].scale, or 0 and 1 when fit is NULL; with REQUIRE_OK a pair whose fit[p].ok == 0 contributes nothing.  Row t < W of a contributing
 * pair goes to cell (g = pairs[p].ref, j = start + t).  In float64, each operation rounded to nearest even and none fused:
 * m = float64(sum) / float64(n_samples), v = (m + float64(o)) * float64(s), w = v * float64(fix).  The level is SKIPPED -- count word +=
 * 2^32, nothing else -- when n_samples < max(min_samples, 1), when n_entries > max_entries and max_entries != 0, and when |w| <= 2^24
 * does not hold (NaN included).  Otherwise it is kept: u = int64(rint(w)), rint to nearest even; count word += 1, n_samples +=
 * n_samples, sum += u, sumsq += u * u.  With |u| <= 2^24, u * u <= 2^48: sumsq cannot wrap below 2^15 observations of a cell, and sum
 * never wraps in practice (2^39 observations); the low half of the count word carries into the high half at 2^32 observations.  Integer
 * adds do not depend on their order, so the arena is reproducible bit for bit whatever the schedule: that is why a fixed-point u is
 * summed and not a float.  fix is the fixed point's scale: 256 keeps 1/256 of the model's unit.
 * Flags.  With VBZ_GPU_PILE_CLEAR the whole arena is zeroed on the context's stream before the adds; without it the call adds to what is
 * there -- batch after batch of reads on one reference is the point.  Nothing outside cells [g][start, end) of contributing pairs is
 * touched.  Returns 0 when queued, -1 for a NULL context or a launch failure, -2, with nothing launched and nothing written, for
 * everything vbz_gpu_levels_fit_batch refuses about locate, max_width, alignment and sizes; a NULL params; fix not finite or <= 0; unknown
 * flags or a reserved word != 0; a NULL pile; pile or fit not 16-byte aligned; G * target_stride * 32 beyond 2^46 bytes.  n_pairs == 0
 * with good arguments returns 0; with CLEAR it clears.
 * vbz_gpu_squiggle_kmers_batch: the key of every position.  kmer is a row-major uint32 [rows][target_stride] arena, 16-byte aligned;
 * rows, strands, BOTH and REVERSED are vbz_gpu_squiggle_batch's, and target_len[row] is its L.  Position j < L holds the index of the
 * k-mer that call would look up there; the mark 0xFFFFFFFF stands where that call would count a masked k-mer, and at and behind L.  EVERY
 * entry of kmer and target_len is written, kmer by 16-byte stores.  squiggle->model is not read and may be NULL, quant is checked and not
 * used; everything else the squiggle call refuses is refused here (-2), kmer or target_len NULL and kmer not 16-byte aligned too.
 * vbz_gpu_pile_kmers_batch: positions added into k-mers.  For row g < rows and j < target_len[g] with idx = kmer[g][j] < 4^k, all four
 * words of position cell (g, j) of pile (rows * target_stride cells) are added to cell idx of kmer_pile (4^k cells), plane by plane,
 * modulo 2^64.  target_len is untrusted: with target_len[g] > target_stride the row contributes nothing and no address is formed from it.
 * Cells whose four words are all zero are skipped.  Sums are additive, so reads piled per position first and positions per k-mer second
 * give what a direct per-k-mer pile of the levels would, and position cells (G x L) are far fewer than levels (n_pairs x W).  CLEAR zeroes
 * kmer_pile first; DIRECT makes global adds whatever k is (the other side of the measurement below).  -2 for a NULL params; k outside 1
 * ... 9; rows outside 1 ... 4096; target_stride outside 16 ... 2^30 in multiples of 16; unknown flags; a NULL target_len, kmer, pile or
 * kmer_pile; kmer, pile or kmer_pile not 16-byte aligned; rows * target_stride * 32 beyond 2^46 bytes.
 * vbz_gpu_model_update_batch: the new table.  For k-mer i < 4^k let n be the low 32 bits of the count word.  When n >= max(min_obs, 1),
 * in float64, each operation rounded, none fused: mean = float64(int64 sum) / float64(n); model[i] = float32(mean / float64(fix)); var =
 * float64(sumsq) / float64(n) - mean * mean; sd[i] = float32(sqrt(max(var, 0)) / float64(fix)), the square root correctly rounded as the
 * event call's sd has it.  Otherwise model[i] takes the 32 bits of prior[i] and sd[i] = +0.  sd may be NULL; prior may not, and may be the
 * same pointer as model.  EVERY entry of model and sd is written.  -2 for a NULL params; k outside 1 ... 9; flags != 0; fix not finite or
 * <= 0; a NULL kmer_pile, prior or model; kmer_pile not 16-byte aligned.
 * How (csrc/pile.hip).  levels_pile has levels_fit's shape: one wavefront a pair, four to a workgroup, 64 levels a turn; a
 * lane loads its 32-byte record by two 16-byte loads, does the float64 arithmetic and issues four no-return 64-bit adds at agent scope, a
 * skipped level one.  Lanes of a turn hit consecutive cells, so a wavefront never collides with itself; pairs collide with each other at
 * the coverage depth.  No LDS, no scratch, no barrier.  squiggle_kmers is the squiggle kernel's base loading and index roll
 * (csrc/squiggle_bases.h) with the gather left out.  pile_kmers: a workgroup takes 4 096 positions of a row; for k <= 6 (4^k * 32
 * bytes of LDS: 128 KB at k = 6, where the measurement below puts the threshold) it keeps a private table in LDS, adds into it with
 * LDS 64-bit adds and adds its non-zero words into global memory at its end; above that it makes global adds directly.  model_update:
 * one thread a k-mer.
 * Measured on one MI355X (tools/time_pile.py, profiles/pile_time.json; the parent of the commit that adds these calls is 3d1b100 and can
 * run none of them, so the yardstick is the unfused torch route -- float64 arithmetic, index_add_ on int64 -- in the same run; median of
 * 20, the legs alternating in one process, every arena checked bit for bit against that route): levels_pile over 8 192 pairs,
 * max_width 2 256, 15.2 M levels, CLEAR included: 0.640 ms on G = 2 targets of 30 000 levels (depth 274) and 0.412 ms with the same pairs
 * dealt over G = 64 (depth 10), against 3.41 and 3.14 ms for torch; the CLEAR alone 0.035 ms.  That is 0.80 and 1.30 TB/s of added bytes
 * (32 a kept level) beside the 1.3 TB/s measured for float32 adds on this chip -- 64-bit integer adds run at the same byte rate when
 * spread, and lose 38 % piled 274 deep -- and 4.6 times vbz_gpu_levels_fit_batch's 0.141 ms over the same arena: the adds are the bound.
 * pile_kmers, table in LDS / global adds (DIRECT): 2 rows 0.0228 / 0.690 ms (k = 1), 0.0246 / 0.0376 (k = 5), 0.0298 / 0.0444 (k = 6),
 * 64 rows 0.0427 / 0.2303 (k = 5), 0.0855 / 0.3159 (k = 6); k = 9, global adds, 0.05 - 0.06 ms; torch 0.35 - 1.52 ms.  squiggle_kmers
 * 0.017 - 0.022 ms (torch 0.14 - 11 ms), model_update 0.017 - 0.019 ms (torch 0.13 - 0.14 ms). */
#ifndef VBZ_GPU_PILE_H
#define VBZ_GPU_PILE_H

#include "vbz_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VBZ_GPU_PILE_CLEAR 1u      /* zero the arena the call adds into, on the context's stream, before the adds */
#define VBZ_GPU_PILE_REQUIRE_OK 2u /* levels_pile: a pair whose fit[p].ok == 0 contributes nothing */
#define VBZ_GPU_PILE_DIRECT 4u     /* pile_kmers: global adds whatever k is, no table in LDS */
typedef struct vbz_gpu_levels_pile
{
    uint32_t max_width;   /* of the levels arena: a multiple of 8, 8 ... 65536 */
    uint32_t min_samples; /* levels with n_samples < max(min_samples, 1) are skipped */
    uint32_t max_entries; /* levels with n_entries > max_entries are skipped (stalls); 0: no cap */
    uint32_t flags;       /* CLEAR | REQUIRE_OK; other bits must be 0 */
    float fix;            /* finite, > 0: the fixed point's scale, u = rint(v * fix) */
    uint32_t reserved0;   /* must be 0 */
    uint32_t reserved1;   /* must be 0 */
    uint32_t reserved2;   /* must be 0 */
} vbz_gpu_levels_pile;    /* 32 bytes */
typedef struct vbz_gpu_pile_kmers
{
    uint32_t k;             /* 1 ... 9 */
    uint32_t rows;          /* G: 1 ... 4096 */
    uint32_t target_stride; /* entries per row of kmer and of the position pile: a multiple of 16, 16 ... 2^30 */
    uint32_t flags;         /* CLEAR | DIRECT; other bits must be 0 */
} vbz_gpu_pile_kmers;       /* 16 bytes */
typedef struct vbz_gpu_model_update
{
    uint32_t k;       /* 1 ... 9 */
    uint32_t min_obs; /* k-mers with fewer than max(min_obs, 1) kept observations keep the prior */
    uint32_t flags;   /* must be 0 */
    float fix;        /* finite, > 0: the pile's */
} vbz_gpu_model_update; /* 16 bytes */
VBZ_EXPORT int vbz_gpu_levels_pile_batch(vbz_gpu_ctx* ctx, uint32_t n_pairs, uint32_t n_reads, const vbz_gpu_locate* locate,
                                         const vbz_gpu_match_pair* pairs, const vbz_gpu_match_span* hit, const uint32_t* n_levels,
                                         const vbz_gpu_level* levels, const vbz_gpu_levels_pile* params, const vbz_gpu_level_fit* fit,
                                         uint64_t* pile);
VBZ_EXPORT int vbz_gpu_squiggle_kmers_batch(vbz_gpu_ctx* ctx, const vbz_gpu_squiggle* squiggle, uint32_t* kmer, uint32_t* target_len);
VBZ_EXPORT int vbz_gpu_pile_kmers_batch(vbz_gpu_ctx* ctx, const vbz_gpu_pile_kmers* params, const uint32_t* target_len, const uint32_t* kmer,
                                        const uint64_t* pile, uint64_t* kmer_pile);
VBZ_EXPORT int vbz_gpu_model_update_batch(vbz_gpu_ctx* ctx, const vbz_gpu_model_update* params, const uint64_t* kmer_pile, const float* prior,
                                          float* model, float* sd);

#ifdef __cplusplus
}
#endif

#endif
