#!/usr/bin/env python3
"""Cost of the fused match call (vbz_gpu_signal_match_batch) against its floor, the stage entry and the unfused route, alternating in
one process.

Workload: --reads reads of ~100 k int16 samples (the lengths of SURVEY.md 8d, rounded down to 32) of the synthetic signal, synthesised on
the device and compressed once; the trim call's begin[] (its defaults, MED_MAD) is the range's begin; the query is the first N = 2 048
samples behind it, MED_MAD-normalised, quant 32.  The references are stretches of the reads' own quantised queries (read r gives row r),
so some pairs cost nothing and most do not.  Cases: R = 24 and R = 96 rows of M = 400, and R = 4 rows of M = 2 048.  Each behind untimed
warm-up calls and timed with HIP events on the codec's stream (median of --reps calls, the calls alternating):
  windows   the windows call alone (one row per read at start 0, L = N, float32): the fused call's floor
  match     the stage entry alone, on the query the windows call left
  fused     the fused call: query, hits and shift_scale
  unfused   the windows call, then a torch DTW over all pairs on the device, one step per anti-diagonal (int32; blocks of pairs below
            2^27 cells a diagonal); --unfused-reps calls, it being two orders slower
Every hit of the fused call and of the stage entry is checked bit for bit against the unfused route in the same run, and --sample reads
against tests/match_ref.py on the host.  Then one 20 M-sample read, the same.

Next to the measured cells per second stands the issue bound: VALU instructions a wavefront issues per step of the committed kernel
(VALU_PER_STEP, counted in the disassembly of match.hip's inner loops: the two DPP moves, v_readlane and the v_mov behind it, the
compare and two selects of the running minimum, three copies, and v_min3_u32 + v_msad_u8 per row: 9 + 2 c) times
4.1 cycles an instruction (profiles/r06_valu_rate.txt: v_min3 / VOP3 / DPP at 4 and 8 wavefronts per SIMD), on 256 CUs x 4 SIMDs at 2.4 GHz.

The span calls (vbz_gpu_match_span_batch, vbz_gpu_signal_match_span_batch) are two more legs of the same alternating loop:
  span        the span stage entry alone, on the same query
  fused_span  the fused span call
Every (cost, end) they write is checked bit for bit against the cost-only call of the same run, and --sample reads against
tests/match_span_ref.py on the host.  The packed kernel's inner loop is 10 + 2 c VALU instructions a step (SPAN_VALU_PER_STEP: v_min3_u32
and v_sad_u32 per row; the cost-only step's nine, and the v_or that keeps lane 0's diagonal far -- the step number as the DPP move's
`old` takes the place of the cost-only step's zero); three of them are plain v_mov, which issue in 2.2 cycles (SPAN_MOVES).

The path calls (vbz_gpu_match_best_batch, vbz_gpu_match_path_batch) are two more legs, on the winners of the span call of the same run:
  best        the winners' table from the span stage entry's arena
  path        the path stage: forward launch and traceback of every winner, max_width = N
Every hit is checked against the span call of the same run (cost, end, start of the winner), and --sample reads against
tests/match_path_ref.py on the host.  The forward kernel's inner loop is 6 + 6 c VALU instructions a step (PATH_VALU_PER_STEP, counted in
the disassembly: per row v_min3_u32, v_sad_u32 and a subtraction and a v_alignbit_b32 for each of the two direction bits; the
subtractions issue in 2.4 cycles, the rest in 4.1).  The
traceback's share of the stage is read from the library's per-launch timers in one more call; --path-caps times the stage under other
scratch caps (bytes).  The unfused path route -- the span arena and the query copied to the host, then match_path_ref's backtrace over
the winners -- is timed on the --sample reads and SCALED to the batch.  --unfused-reps 0 leaves the torch DTW out (and the checks against
it).

    python tools/time_match.py [--reads 8192] [--reps 20] [--unfused-reps 2] [--sample 6] [--long 20000000] [--path-caps a,b,c]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import match_path_ref as PR  # noqa: E402
import match_ref as MR  # noqa: E402
import match_span_ref as SR  # noqa: E402
from vbz_compression_amd import batch  # noqa: E402

N = 2048
QUANT = 32.0
FAR = 1 << 30
DIAGONAL_CELLS = 1 << 27
# rows per lane -> VALU instructions per step of match_pair<C>'s inner loop (see the module text)
VALU_PER_STEP = {1: 11, 2: 13, 4: 17, 8: 25, 16: 41, 32: 73}
SPAN_VALU_PER_STEP = {c: 10 + 2 * c for c in (1, 2, 4, 8, 16, 32)}
SPAN_MOVES = 3
PATH_VALU_PER_STEP = {c: 6 + 6 * c for c in (1, 2, 4, 8, 16, 32)}
PATH_SUBS_PER_ROW = 2    # v_sub_u32, which issues in CYCLES_PER_SUB (profiles/r06_valu_rate.txt: v_add_u32 at two wavefronts a SIMD and more)
CYCLES_PER_SUB = 2.4
CYCLES_PER_VALU = 4.1
CYCLES_PER_MOVE = 2.2
SIMDS, HZ = 256 * 4, 2.4e9


def progress(*what):
    print("#", *what, file=sys.stderr, flush=True)


def timed(c, fns, reps, warm=2):
    """median milliseconds of every fn, the fns alternating call by call"""
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
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def torch_quantize(z):
    v = z * QUANT
    return torch.where(torch.isnan(v), torch.zeros_like(v), torch.clamp(torch.round(v), -127.0, 127.0)).to(torch.int32)


def torch_dtw(K, valid, ref, ref_len):
    """hits int32 [reads, R, 2] of every pair, one step per anti-diagonal.  K int32 [reads, N]; ref int32 [R, M]; every ref_len == M"""
    n, dev = K.shape[0], K.device
    R, M = ref.shape
    out = torch.empty((n, R, 2), dtype=torch.int32, device=dev)
    Kp = torch.nn.functional.pad(torch.flip(K, dims=[1]), (M, M))   # k[d - i] = Kp[N - 1 - d + M + i]
    rows = torch.arange(M, device=dev)
    step = max(1, DIAGONAL_CELLS // (R * M))
    ref3 = ref[None, :, :]
    for a in range(0, n, step):
        b = min(n, a + step)
        nb = b - a
        P = [torch.full((nb, R, M + 1), FAR, dtype=torch.int32, device=dev) for _ in range(3)]
        for p in P:
            p[:, :, 0] = 0   # (the row above row 0: the free start)
        tmp = torch.empty((nb, R, M), dtype=torch.int32, device=dev)
        best = torch.full((nb, R), 0x7FFFFFFF, dtype=torch.int32, device=dev)
        best_j = torch.zeros((nb, R), dtype=torch.int32, device=dev)
        nv = valid[a:b, None].to(torch.int32)
        for d in range(N + M - 1):
            p0, p1, p2 = P[d % 3], P[(d - 1) % 3], P[(d - 2) % 3]
            s = N - 1 - d + M
            c = (ref3 - Kp[a:b, None, s : s + M]).abs_()
            torch.minimum(p1[:, :, :-1], p2[:, :, :-1], out=tmp)
            torch.minimum(tmp, p1[:, :, 1:], out=tmp)
            torch.add(c, tmp, out=p0[:, :, 1:])
            if d < M - 1:
                p0[:, :, 1:].masked_fill_(rows > d, FAR)   # (cells in front of sample 0)
            j = d - (M - 1)
            if j >= 0:
                v = p0[:, :, M]
                upd = (v < best) & (nv > j)
                best = torch.where(upd, v, best)
                best_j = torch.where(upd, torch.full_like(best_j, j), best_j)
        empty = (nv <= 0).expand(nb, R)
        out[a:b, :, 0] = torch.where(empty, torch.full_like(best, -1), best)
        out[a:b, :, 1] = torch.where(empty, torch.zeros_like(best_j), best_j + 1)
    return out


def bound_cells_per_second(M):
    C = next(c for c in (1, 2, 4, 8, 16, 32) if 64 * c >= M)
    return M / (VALU_PER_STEP[C] * CYCLES_PER_VALU) * HZ * SIMDS, C


def span_bound_cells_per_second(M):
    C = next(c for c in (1, 2, 4, 8, 16, 32) if 64 * c >= M)
    cycles = (SPAN_VALU_PER_STEP[C] - SPAN_MOVES) * CYCLES_PER_VALU + SPAN_MOVES * CYCLES_PER_MOVE
    return M / cycles * HZ * SIMDS


def path_leg(c, ms, q, valid, ref, ref_len, mt, span_s, pairs, path_hit, path_rows, M, C, sample, caps):
    """the checks and the figures of the best and path legs (ms: the alternating loop's medians)"""
    n, R = span_s.shape[0], span_s.shape[1]
    torch.cuda.synchronize()
    sp, pr, hit = (t.cpu().numpy().view(np.uint32) for t in (span_s, pairs, path_hit))
    assert (pr == PR.best(sp)).all(), "match_best != match_path_ref.best"
    won = pr[:, 1] != PR.NONE
    rows_i = np.arange(n)[won]
    assert (hit[won, :3] == sp[rows_i, pr[won, 1], :3]).all() and (hit[won, 3] == M).all(), "path hits != the span call's winners"
    assert (hit[~won] == np.array(PR.EMPTY, np.uint32)).all()
    pick = np.linspace(0, n - 1, min(sample, n)).astype(int)
    q_h, v_h, ref_h = q.cpu().numpy(), valid.cpu().numpy(), ref.cpu().numpy()
    t0 = time.perf_counter()   # the unfused route on the sampled reads: arena and query are on the host, the backtrace over the winners
    winners = PR.best(sp[pick])
    winners[:, 0] = pick
    want_hit, want_rows = PR.paths(q_h, v_h, QUANT, ref_h, [M] * R, winners, N)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert (hit[pick] == want_hit).all() and (path_rows.cpu().numpy().view(np.uint32)[pick] == want_rows).all(), "match_path_ref"
    # the traceback's share, from the library's per-launch timers over one more call
    c.profile_reset()
    c.profile(True)
    with torch.cuda.stream(c.stream):
        c.match_path(q, valid, ref, ref_len, pairs, N, mt, hit=path_hit, rows=path_rows)
    prof = c.profile_read()
    c.profile(False)
    fwd, trace = prof["match_path_forward"], prof["match_path_trace"]
    steps = int((hit[won, 1].astype(np.int64) - hit[won, 2] + (M - 1) // C).sum())
    waves = -(-int(won.sum()) // SIMDS)   # wavefronts a SIMD runs one after another when the pairs are spread evenly
    step_cycles = (PATH_VALU_PER_STEP[C] - PATH_SUBS_PER_ROW * C) * CYCLES_PER_VALU + PATH_SUBS_PER_ROW * C * CYCLES_PER_SUB
    bound_ms = steps / max(1, int(won.sum())) * waves * step_cycles / HZ * 1e3
    out = {"best_ms": ms["best"], "path_ms": ms["path"], "path_over_span": round(ms["path"] / ms["span"], 4), "winners": int(won.sum()),
           "mean_width": round(float((hit[won, 1].astype(np.int64) - hit[won, 2]).mean()), 1), "groups": fwd[0],
           "forward_ms": round(fwd[1], 4), "trace_ms": round(trace[1], 4), "trace_share": round(trace[1] / (fwd[1] + trace[1]), 3),
           "valu_per_step": PATH_VALU_PER_STEP[C], "forward_issue_bound_ms": round(bound_ms, 4),
           "forward_cycles_per_step": round(fwd[1] * 1e-3 * HZ / (steps / max(1, int(won.sum())) * waves), 1),
           "bound_cycles_per_step": round(step_cycles, 1),
           "unfused_host_ms_scaled": round(host_ms * n / len(pick), 1), "unfused_is_scaled_from_reads": len(pick),
           "hits_equal_span_winners": True, "reads_checked_against_match_path_ref": len(pick), "caps": {}}
    for cap in caps:
        progress("cap", cap)
        c.L.vbz_gpu_set_match_path_cap(c.ctx, cap)
        out["caps"][str(cap)] = timed(c, {"path": lambda: c.match_path(q, valid, ref, ref_len, pairs, N, mt, hit=path_hit, rows=path_rows)}, 10)["path"]
    c.L.vbz_gpu_set_match_path_cap(c.ctx, 0)
    return out


def case(c, lens, reps, unfused_reps, seed, shapes, sample, path_caps=()):
    dev = c.device
    n = int(lens.numel())
    opts = c.options(True, 2, 1, 1)
    lens64 = lens.to(torch.int64)
    total = int(lens64.sum())
    sizes = lens64 * 2
    off = torch.cumsum(sizes, 0) - sizes
    with torch.cuda.stream(c.stream):
        raw = torch.empty(total * 2, dtype=torch.uint8, device=dev)
        c.synth_signal(seed, 0, raw, off, lens)
        caps = torch.tensor([c.L.vbz_max_compressed_size(int(s), ctypes.byref(opts)) for s in sizes.cpu().tolist()], dtype=torch.int64)
        coff, ctotal = batch.layout(caps, 64)
        comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
        coff = coff.to(dev)
        csize = torch.zeros(n, dtype=torch.int32, device=dev)
        c.compress(raw, off, sizes.to(torch.int32), comp, coff, caps.to(torch.int32).to(dev), csize, opts)
    torch.cuda.synchronize()
    progress("compressed", n, "reads")
    del raw
    size32 = sizes.to(torch.int32)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    begin = torch.zeros(n, dtype=torch.int32, device=dev)
    c.signal_trim(comp, coff, csize, off, size32, res, opts, batch.MED_MAD, out=begin)
    torch.cuda.synchronize()
    valid = torch.clamp(lens64 - torch.minimum(begin.to(torch.int64), lens64), max=N).to(torch.int32)
    wfirst = torch.arange(n + 1, dtype=torch.int64, device=dev)
    wstart = torch.zeros(n, dtype=torch.int32, device=dev)
    samples = lens.clone()
    ss_w = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    ss_f = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    query = torch.zeros((n, N), dtype=torch.float32, device=dev)
    mt = batch.Match(N, QUANT)
    w = {}

    def windows():
        w["q"], _ = c.decompress_windows(comp, coff, csize, samples, res, opts, wfirst, wstart, N, 0.0, torch.float32, norm=batch.MED_MAD,
                                         norm_out=ss_w, begin=begin)

    with torch.cuda.stream(c.stream):
        windows()
    torch.cuda.synchronize()
    K = torch_quantize(w["q"])
    out = {"reads": n, "samples": total, "N": N, "quant": QUANT, "cases": []}
    for R, M in shapes:
        stride = (M + 15) // 16 * 16
        ref = torch.zeros((R, stride), dtype=torch.int8, device=dev)
        for r in range(R):
            src = K[r % n]
            at = (37 * r) % (N - M + 1)
            ref[r, :M] = src[at : at + M].to(torch.int8)
        ref_len = torch.full((R,), M, dtype=torch.int32, device=dev)
        hits_f = torch.empty((n, R, 2), dtype=torch.int32, device=dev)
        hits_s = torch.empty((n, R, 2), dtype=torch.int32, device=dev)
        span_f = torch.empty((n, R, 4), dtype=torch.int32, device=dev)
        span_s = torch.empty((n, R, 4), dtype=torch.int32, device=dev)
        query_span = torch.zeros((n, N), dtype=torch.float32, device=dev)
        pairs = torch.empty((n, 4), dtype=torch.int32, device=dev)
        path_hit = torch.empty((n, 4), dtype=torch.int32, device=dev)
        path_rows = torch.empty((n, stride, 2), dtype=torch.int32, device=dev)
        u = {}

        def stage():
            c.match(w["q"], valid, ref, ref_len, mt, out=hits_s)

        def fused():
            c.signal_match(comp, coff, csize, off, size32, res, opts, ref, ref_len, mt, norm=batch.MED_MAD, norm_out=ss_f, begin=begin, query=query,
                           out=hits_f)

        def span():
            c.match_span(w["q"], valid, ref, ref_len, mt, out=span_s)

        def fused_span():
            c.signal_match_span(comp, coff, csize, off, size32, res, opts, ref, ref_len, mt, norm=batch.MED_MAD, norm_out=ss_f, begin=begin,
                                query=query_span, out=span_f)

        def best():
            c.match_best(span_s, out=pairs)

        def path():
            c.match_path(w["q"], valid, ref, ref_len, pairs, N, mt, hit=path_hit, rows=path_rows)

        def unfused():
            windows()
            u["hits"] = torch_dtw(torch_quantize(w["q"]), valid, ref[:, :M].to(torch.int32), ref_len)

        legs = {"windows": windows, "match": stage, "span": span, "best": best, "path": path, "fused": fused, "fused_span": fused_span}
        progress("case", R, M)
        ms = timed(c, legs, reps)
        progress("timed", ms)
        if unfused_reps:
            ms.update(timed(c, {"unfused": unfused}, unfused_reps, warm=0))
        torch.cuda.synchronize()
        assert torch.equal(res.to(torch.int64), lens64 * 4), "verdicts"
        assert torch.equal(query, w["q"]) and torch.equal(ss_f, ss_w), "the fused call's query or shift_scale != the windows call's"
        assert torch.equal(hits_f, hits_s), "fused hits != the stage entry's, bit for bit"
        if unfused_reps:
            assert torch.equal(hits_f, u["hits"]), "fused hits != the unfused route, bit for bit"
        q_h, v_h, ref_h = w["q"].cpu().numpy(), valid.cpu().numpy(), ref.cpu().numpy()
        pick = np.linspace(0, n - 1, min(sample, n)).astype(int)
        want = MR.hits(q_h[pick], v_h[pick], QUANT, ref_h, [M] * R)
        assert (hits_f.cpu().numpy().view(np.uint32)[pick] == want).all(), "match_ref"
        assert torch.equal(span_s[:, :, :2], hits_s) and torch.equal(span_f[:, :, :2], hits_f), "span (cost, end) != the cost-only call, bit for bit"
        assert torch.equal(span_s, span_f) and torch.equal(query_span, query), "the fused span call != the span stage entry"
        want = SR.spans(q_h[pick], v_h[pick], QUANT, ref_h, [M] * R)
        assert (span_s.cpu().numpy().view(np.uint32)[pick] == want).all(), "match_span_ref"
        cells = int(valid.to(torch.int64).sum()) * R * M
        span_bound = span_bound_cells_per_second(M)
        bound, C = bound_cells_per_second(M)
        dp_ms = ms["fused"] - ms["windows"]
        zero = int((hits_f[:, :, 0] == 0).sum())
        out["cases"].append({"R": R, "M": M, "rows_per_lane": C, "cells": cells, "ms": ms, "pairs_at_cost_0": zero,
                             "match_gcells_per_s": round(cells / ms["match"] / 1e6, 1), "fused_minus_windows_gcells_per_s": round(cells / dp_ms / 1e6, 1),
                             "issue_bound_gcells_per_s": round(bound / 1e9, 1), "share_of_bound": round(cells / (ms["match"] * 1e-3) / bound, 3),
                             "unfused_over_fused": round(ms["unfused"] / ms["fused"], 1) if unfused_reps else None, "checked_against_unfused": bool(unfused_reps),
                             "path": path_leg(c, ms, w["q"], valid, ref, ref_len, mt, span_s, pairs, path_hit, path_rows, M, C, sample, path_caps),
                             "reads_checked_against_match_ref": len(pick),
                             "span": {"over_match": round(ms["span"] / ms["match"], 3), "fused_span_over_fused": round(ms["fused_span"] / ms["fused"], 3),
                                      "gcells_per_s": round(cells / ms["span"] / 1e6, 1), "valu_per_step": SPAN_VALU_PER_STEP[C], "moves_per_step": SPAN_MOVES,
                                      "issue_bound_gcells_per_s": round(span_bound / 1e9, 1),
                                      "share_of_bound": round(cells / (ms["span"] * 1e-3) / span_bound, 3),
                                      "over_twice_the_cost_only_call": round(ms["span"] / (2 * ms["match"]), 3),
                                      "cost_end_equal_cost_only": True, "reads_checked_against_match_span_ref": len(pick)}})
        print(json.dumps(out["cases"][-1]), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--unfused-reps", type=int, default=2)
    ap.add_argument("--sample", type=int, default=6)
    ap.add_argument("--long", type=int, default=20_000_000, help="samples of the one long read (0: none)")
    ap.add_argument("--shapes", default="24x400,96x400,4x2048", help="R x M, comma separated")
    ap.add_argument("--path-caps", default="", help="scratch caps (bytes) to time the path stage under, comma separated")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    c = batch.GpuCodec(0)
    lens = (c.synth_lengths(5, 0, args.reads) // 32 * 32).to(torch.int32)
    caps = [int(v) for v in args.path_caps.split(",") if v]
    out = {"norm": "med_mad", "headline": case(c, lens, args.reps, args.unfused_reps, 5, shapes, args.sample, caps)}
    print(json.dumps(out), flush=True)
    if args.long:
        torch.cuda.empty_cache()
        out["one_long_read"] = case(c, torch.tensor([args.long // 32 * 32], dtype=torch.int32, device=c.device), args.reps, args.unfused_reps, 7, shapes, 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
