#!/usr/bin/env python3
"""Cost of the locate calls (vbz_gpu_locate_batch, vbz_gpu_signal_locate_batch) against the windows call alone and against the only route
the parent has for the same cells, vbz_gpu_match_batch with the roles swapped; the calls alternate in one process.

Workload: --reads reads of ~100 k int16 samples of the synthetic signal (the lengths of SURVEY.md 8d, rounded down to 32), synthesised on
the device and compressed once; the trim call's begin[] (its defaults, MED_MAD) is the range's begin; the query is the first N = 2 048
samples behind it, MED_MAD-normalised, quant 32.  The targets are synthetic squiggles -- plateaus of 6 levels under noise, inside +-127 --
with the whole quantised query of a few reads planted in them, so some pairs cost nothing and most do not.  Cases (reads x G x L): 512 and
8 192 reads against G = 2 targets of L = 30 000 and of L = 48 000, and 512 reads against one target of L = 1 048 576.  Each leg behind
untimed warm-up calls and timed with HIP events on the codec's stream (median of --reps calls):
  windows   the windows call alone (one row per read at start 0, L = N, float32): the fused call's floor
  locate    the stage entry alone, on the query the windows call left
  fused     the fused call: query, hits and shift_scale
  span      the span stage entry (vbz_gpu_locate_span_batch) on the same query: (cost, end) and the start of the stretch, found by the walk
            back.  Every (cost, end) must equal the cost-only leg's bit for bit in the same run
  fused_span  the fused span call (vbz_gpu_signal_locate_span_batch)
  locate_after  the cost-only stage entry once more, behind the span legs: against `locate` it shows whether the cost-only kernel moved
  span_best_path  span -> best -> path (vbz_gpu_locate_span_batch, vbz_gpu_match_best_batch, vbz_gpu_locate_path_batch), queued on one stream with
            no host copy; max_width is the smallest multiple of 8 that covers the widest winner (found by one untimed run).  `path` is the
            path call alone on that winners' table.  Every winner's (cost, start) must equal its span's, the sampled reads' hits and rows
            tests/locate_path_ref.py's
  swapped_path  at 512 reads and L <= 65 536: the parent's only route to the same paths, vbz_gpu_match_path_batch with the roles swapped over
            the same winners' table (the targets as float32 "queries", the reads' levels as int8 "references").  Its hits and rows must
            equal the path leg's bit for bit in the same run
  span_after  the span stage entry once more, behind the path legs: against `span` it shows whether the span kernel moved
  swapped   wherever L <= 65 536: vbz_gpu_match_batch over the same cells -- the targets written out as float32 level / quant "queries" of
            query_len = the target's stride, the reads' levels, quantised here with torch, as int8 "references" of M = 2 048 (4 096 of them a
            call, the rule's most).  Its hits must equal the locate call's bit for bit in the same run.
Six reads are checked against tests/locate_ref.py and tests/locate_span_ref.py on the host where the target is short enough for numpy
(L <= 65 536).  For those reads' pairs the steps the walk back takes are counted by the numpy model of the kernel's rule (the fronts of a
block's last two steps, a block 256 virtual steps); for every pair the arena gives the least it can take, end - start + la.

Next to the measured cells per second and cycles a step stands the kernel's issue bound: VALU instructions a wavefront issues per step of
locate_pair<C>'s four-step turn, counted in the disassembly of locate.hip (8.25 + 2 c: per turn eight DPP moves, one v_readlane, four
v_min_u32 / v_cmp / v_cndmask of the running minimum and twelve v_mov_b32, and v_min3_u32 + v_msad_u8 per row and step), at 4.1 cycles an
instruction and 2.2 for the plain moves (profiles/r06_valu_rate.txt), on 256 CUs x 4 SIMDs at 2.4 GHz.  Phase 2 (locate_back<C>): 6.25 + 3 c
-- per turn eight DPP moves, one v_readlane, four v_cmp_eq / v_cndmask of the last hit, twelve v_mov_b32, per row and step the cell's two and
(c - 1 of c) a select; at c = 32 the compiler branches over half of the selects: 346 or 406 a turn, 86.5 or 101.5 a step.  The path's forward
pass (locate_path_forward<32>, packed key): 790 a turn, 197.5 a step -- per cell v_min3_u32, v_sad_u32, two subtractions and two
v_alignbit_b32 (eight of the 256 folded away), and per turn eight DPP moves, eight plain moves and one v_readlane -- and eight 256-byte
stores of direction bits a turn.  The expectation for the path of the winners: the span stage's time x (W + 63) / (L + 63) x 197.5 / 72.25
per pair a read, W the median winner's width -- one wavefront per read where the span stage has G.

    python tools/time_locate.py [--reps 20] [--sample 6] [--cases 512x2x30000,...]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import locate_path_ref as LP  # noqa: E402
import locate_ref as LR  # noqa: E402
import locate_span_ref as LS  # noqa: E402
from vbz_compression_amd import batch  # noqa: E402

N = 2048
QUANT = 32.0
TURN = 4                 # steps a turn of the inner loop
TURN_VALU = 33           # VALU instructions a turn besides the cells
TURN_MOVES = 12          # ... of which plain v_mov_b32
CYCLES_PER_VALU = 4.1
CYCLES_PER_MOVE = 2.2
SIMDS, HZ = 256 * 4, 2.4e9
MATCH_REFS = 4096        # vbz_gpu_match.n_refs at most
BACK_TURN_VALU = {32: (346, 406)}   # phase 2, VALU instructions a turn: otherwise 25 + 12 c
PATH_TURN_VALU = 790     # locate_path_forward<32>, packed key: VALU instructions a turn of four steps


def progress(*what):
    print("#", *what, file=sys.stderr, flush=True)


def timed(c, fns, reps, warm=2):
    """(median, lowest, highest) milliseconds of every fn, the fns alternating call by call"""
    ms = {k: [] for k in fns}
    with torch.cuda.stream(c.stream):
        for _ in range(warm):
            for f in fns.values():
                f()
        for _ in range(reps):
            for k, f in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
    return {k: (round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)) for k, v in ms.items()}


def torch_quantize(z):
    v = z * QUANT
    return torch.where(torch.isnan(v), torch.zeros_like(v), torch.clamp(torch.round(v), -127.0, 127.0)).to(torch.int8)


def step_cycles(C):
    """(VALU instructions a step, its cycles at 4.1 an instruction, its cycles with the plain moves at 2.2)"""
    valu = TURN_VALU / TURN + 2 * C
    return valu, valu * CYCLES_PER_VALU, valu * CYCLES_PER_VALU - TURN_MOVES / TURN * (CYCLES_PER_VALU - CYCLES_PER_MOVE)


def back_cycles(C):
    """phase 2: (VALU instructions a step, least and most; the issue bound in cycles a step, the plain moves at 2.2, least and most)"""
    turn = BACK_TURN_VALU.get(C, (25 + 12 * C,) * 2)
    valu = [v / TURN for v in turn]
    return valu, [v * CYCLES_PER_VALU - TURN_MOVES / TURN * (CYCLES_PER_VALU - CYCLES_PER_MOVE) for v in valu]


class Reads:
    """--reads compressed reads, their trim points, and the query the windows call leaves"""

    def __init__(self, c, n, seed=5):
        self.c, self.n = c, n
        dev = c.device
        lens = (c.synth_lengths(seed, 0, n) // 32 * 32).to(torch.int32)
        self.opts = opts = c.options(True, 2, 1, 1)
        lens64 = lens.to(torch.int64)
        sizes = lens64 * 2
        self.off = off = torch.cumsum(sizes, 0) - sizes
        with torch.cuda.stream(c.stream):
            raw = torch.empty(int(lens64.sum()) * 2, dtype=torch.uint8, device=dev)
            c.synth_signal(seed, 0, raw, off, lens)
            caps = torch.tensor([c.L.vbz_max_compressed_size(int(s), ctypes.byref(opts)) for s in sizes.cpu().tolist()], dtype=torch.int64)
            coff, ctotal = batch.layout(caps, 64)
            self.comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
            self.coff = coff.to(dev)
            self.csize = torch.zeros(n, dtype=torch.int32, device=dev)
            c.compress(raw, off, sizes.to(torch.int32), self.comp, self.coff, caps.to(torch.int32).to(dev), self.csize, opts)
        torch.cuda.synchronize()
        del raw
        self.lens, self.lens64, self.size32 = lens, lens64, sizes.to(torch.int32)
        self.res = torch.zeros(n, dtype=torch.int32, device=dev)
        self.begin = torch.zeros(n, dtype=torch.int32, device=dev)
        c.signal_trim(self.comp, self.coff, self.csize, off, self.size32, self.res, opts, batch.MED_MAD, out=self.begin)
        torch.cuda.synchronize()
        self.valid = torch.clamp(lens64 - torch.minimum(self.begin.to(torch.int64), lens64), max=N).to(torch.int32)
        self.wfirst = torch.arange(n + 1, dtype=torch.int64, device=dev)
        self.wstart = torch.zeros(n, dtype=torch.int32, device=dev)
        self.ss_w = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        self.q = None
        with torch.cuda.stream(c.stream):
            self.windows()
        torch.cuda.synchronize()
        self.levels = torch_quantize(self.q)
        progress("compressed", n, "reads")

    def windows(self):
        self.q, _ = self.c.decompress_windows(self.comp, self.coff, self.csize, self.lens.clone(), self.res, self.opts, self.wfirst, self.wstart, N, 0.0,
                                              torch.float32, norm=batch.MED_MAD, norm_out=self.ss_w, begin=self.begin)


def targets(r, G, L, seed):
    """G synthetic squiggles of L levels (int8 [G, stride], stride the next multiple of 16), a few reads' whole queries planted in them"""
    dev = r.c.device
    gen = torch.Generator(device="cpu").manual_seed(seed)
    stride = (L + 15) // 16 * 16
    plateaus = torch.randint(-70, 71, (G, stride // 6 + 1), generator=gen).repeat_interleave(6, dim=1)[:, :stride]
    t = torch.clamp(plateaus + torch.randint(-6, 7, (G, stride), generator=gen), -127, 127).to(torch.int8).to(dev)
    full = torch.nonzero(r.valid == N).flatten().tolist()
    for k, i in enumerate(full[:: max(1, len(full) // 6)][:6]):
        at = (k * 7919 * 13) % (L - N + 1)
        t[k % G, at : at + N] = r.levels[i]
    return t, stride


def case(c, r, G, L, reps, sample, seed):
    dev, n = c.device, r.n
    t, stride = targets(r, G, L, seed)
    t_len = torch.full((G,), L, dtype=torch.int32, device=dev)
    lc = batch.Locate(N, QUANT)
    hits_s = torch.empty((n, G, 2), dtype=torch.int32, device=dev)
    hits_f = torch.empty((n, G, 2), dtype=torch.int32, device=dev)
    query = torch.zeros((n, N), dtype=torch.float32, device=dev)
    ss_f = torch.zeros((n, 2), dtype=torch.float32, device=dev)

    def stage():
        c.locate(r.q, r.valid, t, t_len, lc, out=hits_s)

    def fused():
        c.signal_locate(r.comp, r.coff, r.csize, r.off, r.size32, r.res, r.opts, t, t_len, lc, norm=batch.MED_MAD, norm_out=ss_f, begin=r.begin,
                        query=query, out=hits_f)

    spans_s = torch.empty((n, G, 4), dtype=torch.int32, device=dev)
    spans_f = torch.empty((n, G, 4), dtype=torch.int32, device=dev)
    query_sp = torch.zeros((n, N), dtype=torch.float32, device=dev)
    ss_sp = torch.zeros((n, 2), dtype=torch.float32, device=dev)

    def span():
        c.locate_span(r.q, r.valid, t, t_len, lc, out=spans_s)

    def fused_span():
        c.signal_locate_span(r.comp, r.coff, r.csize, r.off, r.size32, r.res, r.opts, t, t_len, lc, norm=batch.MED_MAD, norm_out=ss_sp, begin=r.begin,
                             query=query_sp, out=spans_f)

    # the path of the winners: max_width from one untimed run of span -> best
    with torch.cuda.stream(c.stream):
        span()
        table = c.match_best(spans_s)
    torch.cuda.synchronize()
    tb = table.cpu().numpy().view(np.uint32)
    won = tb[:, 1] != 0xFFFFFFFF
    widest = int((tb[:, 3] - tb[:, 2])[won].max()) if won.any() else 8
    max_width = max(8, (widest + 7) // 8 * 8)
    pairs_d = torch.empty((n, 4), dtype=torch.int32, device=dev)
    phit = torch.empty((n, 4), dtype=torch.int32, device=dev)
    prows = torch.empty((n, N, 2), dtype=torch.int32, device=dev)

    def span_best_path():
        c.locate_span(r.q, r.valid, t, t_len, lc, out=spans_s)
        c.match_best(spans_s, out=pairs_d)
        c.locate_path(r.q, r.valid, t, t_len, pairs_d, max_width, lc, hit=phit, rows=prows)

    def path():
        c.locate_path(r.q, r.valid, t, t_len, table, max_width, lc, hit=phit, rows=prows)

    legs = {"windows": r.windows, "locate": stage, "fused": fused, "span": span, "fused_span": fused_span, "locate_after": stage,
            "span_best_path": span_best_path, "path": path, "span_after": span}
    swap_path = L <= 65536 and n <= MATCH_REFS and n <= 512
    if swap_path:
        sw_pairs = table[:, [1, 0, 2, 3]].contiguous()
        sw_hit = torch.empty((n, 4), dtype=torch.int32, device=dev)
        sw_rows = torch.empty((n, N, 2), dtype=torch.int32, device=dev)
        sw_q = t.to(torch.float32) / QUANT
        sw_mt = batch.Match(stride, QUANT)
        sw_ref = r.levels.contiguous()

        def swapped_path():
            c.match_path(sw_q, t_len, sw_ref, r.valid, sw_pairs, max_width, sw_mt, hit=sw_hit, rows=sw_rows)

        legs["swapped_path"] = swapped_path
    swap = L <= 65536
    if swap:
        tq = t.to(torch.float32) / QUANT   # (level / 32 * 32 is exact)
        mt = batch.Match(stride, QUANT)
        parts = [(a, min(n, a + MATCH_REFS)) for a in range(0, n, MATCH_REFS)]
        swapped_hits = [torch.empty((G, b - a, 2), dtype=torch.int32, device=dev) for a, b in parts]
        refs = [r.levels[a:b].contiguous() for a, b in parts]
        ref_len = [r.valid[a:b].contiguous() for a, b in parts]

        def swapped():
            for k in range(len(parts)):
                c.match(tq, t_len, refs[k], ref_len[k], mt, out=swapped_hits[k])

        legs["swapped"] = swapped
    progress("case", n, G, L)
    spread = timed(c, legs, reps)
    ms = {k: v[0] for k, v in spread.items()}
    progress("timed", ms)
    torch.cuda.synchronize()
    assert torch.equal(r.res.to(torch.int64), r.lens64 * 4), "verdicts"
    assert torch.equal(query, r.q) and torch.equal(ss_f, r.ss_w), "the fused call's query or shift_scale != the windows call's"
    assert torch.equal(hits_f, hits_s), "fused hits != the stage entry's, bit for bit"
    if swap:
        assert torch.equal(torch.cat(swapped_hits, dim=1).transpose(0, 1).contiguous(), hits_s), "swapped match hits != the locate call's, bit for bit"
    assert torch.equal(spans_s[:, :, :2], hits_s), "the span call's (cost, end) != the cost-only call's, bit for bit"
    assert torch.equal(spans_f, spans_s) and torch.equal(query_sp, r.q) and torch.equal(ss_sp, r.ss_w), "fused span call != the span stage entry"
    got_sp = spans_s.cpu().numpy().view(np.uint32)
    assert torch.equal(pairs_d, table), "the winners' table moved between runs"
    hit_h, rows_h = phit.cpu().numpy().view(np.uint32), prows.cpu().numpy().view(np.uint32)
    valid_h = r.valid.cpu().numpy()
    for i in np.flatnonzero(won):
        assert hit_h[i][:3].tolist() == got_sp[i][tb[i][1]][:3].tolist() and hit_h[i][3] == valid_h[i], ("the winner's (cost, start)", int(i))
    assert (hit_h[~won] == np.array(LP.EMPTY, np.uint32)).all()
    if swap_path:
        assert torch.equal(sw_hit, phit) and torch.equal(sw_rows, prows), "swapped match path != the locate path, bit for bit"
    live = got_sp[:, :, 0] != 0xFFFFFFFF
    assert (got_sp[:, :, 2][live] < got_sp[:, :, 1][live]).all() and (got_sp[:, :, 3] == 0).all()
    pick = np.linspace(0, n - 1, min(sample, n)).astype(int) if swap else []
    walked = []
    if len(pick):
        q_h, v_h, t_h = r.q.cpu().numpy()[pick], r.valid.cpu().numpy()[pick], t.cpu().numpy()
        want = LR.hits(q_h, v_h, QUANT, t_h, [L] * G)
        assert (hits_s.cpu().numpy().view(np.uint32)[pick] == want).all(), "locate_ref"
        assert (got_sp[pick] == LS.spans(q_h, v_h, QUANT, t_h, [L] * G)).all(), "locate_span_ref"
        sub = [(k, int(tb[i][1]), int(tb[i][2]), int(tb[i][3])) for k, i in enumerate(pick)]
        whit, wrows = LP.paths(q_h, v_h, QUANT, t_h, [L] * G, sub, max_width)
        assert (hit_h[pick] == whit).all() and (rows_h[pick] == wrows).all(), "locate_path_ref"
        K = LR.M.quantize(q_h, QUANT)
        for k, i in enumerate(pick):
            for g in range(G):
                cost, end, start, _ = (int(x) for x in got_sp[i][g])
                if cost != 0xFFFFFFFF:
                    nv = int(v_h[k])
                    walked.append(LS.steps_back(K[k, :nv], t_h[g, :L].astype(np.int64), cost, end, start, LR.rows_per_lane(nv)))
    v64 = r.valid.to(torch.int64)
    cells = int(v64.sum()) * G * L
    C = 32
    valu, bound_all, bound_moves = step_cycles(C)
    pairs = n * G
    la = (N - 1) // C
    per_simd = max(1.0, pairs / SIMDS)        # wavefronts a SIMD issues for, when the pairs are spread evenly
    cyc = ms["locate"] * 1e-3 * HZ / ((L + la) * per_simd)
    bound_cells = N / bound_moves * HZ * SIMDS
    # phase 2 from the arena: a pair walks at least to its start, end - start + la steps; the kernel tests its rule at block ends
    width = (got_sp[:, :, 1].astype(np.int64) - got_sp[:, :, 2].astype(np.int64))[live]
    least = width + la
    back_ms = ms["span"] - ms["locate"]
    back_valu, back_bound = back_cycles(C)
    back_steps = float(np.minimum(least + 256 + 63, got_sp[:, :, 1].astype(np.int64)[live] + la).mean())   # (the expectation: width + 63 + up to 256)
    span_out = {"span_over_locate": round(ms["span"] / ms["locate"], 4), "span_minus_locate_ms": round(back_ms, 4),
                "fused_span_over_fused": round(ms["fused_span"] / ms["fused"], 4),
                "locate_after_over_locate": round(ms["locate_after"] / ms["locate"], 4),
                "locate_spread_ms": round(spread["locate"][2] - spread["locate"][1], 4),
                "locate_after_minus_locate_ms": round(ms["locate_after"] - ms["locate"], 4),
                "stretch_width_median_max": [float(np.median(width)), int(width.max())] if width.size else None,
                "steps_back_at_least_median_max": [float(np.median(least)), int(least.max())] if width.size else None,
                "steps_back_modelled_pairs": len(walked),
                "steps_back_modelled_median_max": [float(np.median(walked)), int(max(walked))] if walked else None,
                "expected_span_over_locate": round(1 + back_steps * back_valu[1] / ((L + la) * valu), 4),
                "back_valu_per_step": back_valu, "back_bound_cycles_per_step": [round(b, 1) for b in back_bound],
                # (means something only where span - locate is above the cost-only leg's own spread: not with one wavefront a SIMD)
                "back_cycles_per_step_if_width_plus_319": round(back_ms * 1e-3 * HZ / (back_steps * per_simd), 1) if back_steps else None,
                "cost_end_equal_cost_only": True, "reads_checked_against_locate_span_ref": len(pick)}
    wwin = (tb[:, 3].astype(np.int64) - tb[:, 2].astype(np.int64))[won]
    path_valu = PATH_TURN_VALU / TURN
    path_bound = path_valu * CYCLES_PER_VALU - 8 / TURN * (CYCLES_PER_VALU - CYCLES_PER_MOVE)
    path_steps = float((wwin + la).mean()) if wwin.size else 0.0
    path_simd = max(1.0, n / SIMDS)
    path_out = {"max_width": max_width, "winners": int(won.sum()), "winner_width_median_max": [float(np.median(wwin)), int(wwin.max())] if wwin.size else None,
                "path_ms": ms["path"], "span_best_path_minus_span_ms": round(ms["span_best_path"] - ms["span"], 4),
                "path_over_span": round(ms["path"] / ms["span"], 4),
                "expected_path_over_span": round((float(np.median(wwin)) + 63) / (L + 63) * path_valu / valu / G, 4) if wwin.size else None,
                "forward_valu_per_step": path_valu, "forward_bound_cycles_per_step": round(path_bound, 1),
                "path_cycles_per_step_both_launches": round(ms["path"] * 1e-3 * HZ / (path_steps * path_simd), 1) if path_steps else None,
                "span_after_over_span": round(ms["span_after"] / ms["span"], 4), "span_spread_ms": round(spread["span"][2] - spread["span"][1], 4),
                "span_after_minus_span_ms": round(ms["span_after"] - ms["span"], 4),
                "winners_equal_their_spans": True, "reads_checked_against_locate_path_ref": len(pick)}
    if swap_path:
        path_out["swapped_path_ms"] = ms["swapped_path"]
        path_out["path_over_swapped_path"] = round(ms["path"] / ms["swapped_path"], 4)
        path_out["paths_equal_swapped_match_path"] = True
    out = {"reads": n, "G": G, "L": L, "target_stride": stride, "rows_per_lane": C, "cells": cells, "path": path_out,
           "ms": ms, "lowest_highest_ms": {k: v[1:] for k, v in spread.items()}, "pairs_at_cost_0": int((hits_s[:, :, 0] == 0).sum()),
           "locate_tcells_per_s": round(cells / ms["locate"] / 1e9, 2), "fused_minus_windows_tcells_per_s": round(cells / (ms["fused"] - ms["windows"]) / 1e9, 2),
           "valu_per_step": valu, "bound_cycles_per_step_all_at_4.1": round(bound_all, 1), "bound_cycles_per_step_moves_at_2.2": round(bound_moves, 1),
           "locate_cycles_per_step": round(cyc, 1), "issue_bound_tcells_per_s": round(bound_cells / 1e12, 2),
           "share_of_bound": round(cells / (ms["locate"] * 1e-3) / bound_cells, 3), "wavefronts_per_simd": round(pairs / SIMDS, 2),
           "hits_equal_swapped_match": True if swap else None, "reads_checked_against_locate_ref": len(pick), "span": span_out}
    if swap:
        s = spread["swapped"]
        out["swapped_tcells_per_s"] = round(cells / ms["swapped"] / 1e9, 2)
        out["locate_over_swapped"] = round(ms["locate"] / ms["swapped"], 4)
        out["swapped_spread_ms"] = round(s[2] - s[1], 4)
        out["locate_minus_swapped_ms"] = round(ms["locate"] - ms["swapped"], 4)
        out["target_bytes"] = {"locate": G * stride, "swapped": G * stride * 4}
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sample", type=int, default=6)
    ap.add_argument("--cases", default="512x2x30000,512x2x48000,8192x2x30000,8192x2x48000,512x1x1048576", help="reads x G x L, comma separated")
    args = ap.parse_args()
    cases = [tuple(int(v) for v in s.split("x")) for s in args.cases.split(",")]
    c = batch.GpuCodec(0)
    out = {"norm": "med_mad", "N": N, "quant": QUANT, "reps": args.reps, "cases": []}
    reads = {}
    for k, (n, G, L) in enumerate(cases):
        if n not in reads:
            reads[n] = Reads(c, n)
        out["cases"].append(case(c, reads[n], G, L, args.reps, args.sample, 100 + k))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
