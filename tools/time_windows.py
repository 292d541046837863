#!/usr/bin/env python3
"""Cost of decoding straight into caller-listed windows (vbz_gpu_decompress_windows_batch) against the chunk call and the unfused route,
alternating in one process.

Headline: 65 536 synthetic reads (~100 k int16 samples each) compressed once, float16 output; then, each behind untimed
warm-up calls and timed with HIP events on the codec's stream (median of --reps calls), three window lists:
  grid     the PAD grid of L = 10 000, S = 9 504 given as windows (every start a multiple of 8: whole-line stores), against
           vbz_gpu_decompress_chunks_batch itself (chunks_pad) -- the two arenas are compared bit for bit
  random   the same number of windows per read, L = 10 000, at random starts in [0, T - L] (coverage ~ 1, seven in eight unaligned:
           element stores)
  dense    L = 512 every 64 samples (coverage 8), over an eighth of the reads: the stores dominate
Each list is also timed on the cheapest unfused route: the float16 signal decode (f16), then a torch gather (index_select) of the
float16 arena through a precomputed flat int64 index of every window position (a position outside the signal indexes the pad value
stored right behind its read's samples), issued in blocks of whole reads below 2^30 elements of source and output each.  Every fused
arena is checked bit for bit against the unfused one of the same list in the same run.  A case whose arenas and index would not fit the
device's free memory is cut in reads (the cut is reported).  Then one 20 M-sample read (the large-read path), the same lists.

    python tools/time_windows.py [--reads 65536] [--reps 20]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vbz_compression_amd import _lib, batch  # noqa: E402

L_, S_ = 10000, 9504
DENSE_L, DENSE_S = 512, 64
PAD = -1.0


def timed(c, fns, reps, warm=3):
    """median milliseconds of every fn, the fns alternating call by call"""
    ms = {k: [] for k in fns}
    c.stream.wait_stream(torch.cuda.current_stream(c.device))   # (the caller's tensors -- the unfused route's index -- were made on that stream)
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


def gather_plan(c, start, lens, sig_off, first, L, limit=1 << 30):
    """The unfused route's index, in blocks of whole reads that keep every gather below 2^30 elements of source and of output:
    [(source lo, source hi, row lo, row hi, int64 index relative to lo)].  A position outside a read's signal indexes the read's pad
    element (the arena element right behind its samples)."""
    dev = c.device
    lens_h, off_h, first_h = lens.cpu().tolist(), sig_off.cpu().tolist(), first.cpu().tolist()
    ar = torch.arange(L, dtype=torch.int64, device=dev)[None, :]
    lens64 = lens.to(torch.int64)
    counts = first[1:] - first[:-1]
    rd_all = torch.repeat_interleave(torch.arange(len(lens_h), dtype=torch.int64, device=dev), counts)
    plan, n, a = [], len(lens_h), 0
    while a < n:
        b = a + 1
        while b < n and off_h[b] + lens_h[b] + 1 - off_h[a] < limit and (first_h[b + 1] - first_h[a]) * L < limit:
            b += 1
        lo, hi, r0, r1 = off_h[a], off_h[b - 1] + lens_h[b - 1] + 1, first_h[a], first_h[b]
        if r1 > r0:
            rd = rd_all[r0:r1]
            pos = start[r0:r1].to(torch.int64)[:, None] + ar
            T = lens64[rd][:, None]
            base = sig_off[rd][:, None] - lo
            plan.append((lo, hi, r0, r1, (base + torch.where((pos >= 0) & (pos < T), pos, T)).reshape(-1)))
        a = b
    return plan


def window_lists(c, lens, which, seed):
    """(window_first int64 [n + 1], start int32 [rows], L) of one of the three lists over reads of `lens` samples"""
    dev = c.device
    n = int(lens.numel())
    if which == "dense":
        L = DENSE_L
        counts = torch.clamp((lens.to(torch.int64) - L) // DENSE_S + 1, min=1)
    else:
        L = L_
        first, info = c.chunk_layout(lens, L_, S_, mode="pad", end_align=0)
        if which == "grid":
            return first, info[:, 1].contiguous(), L
        counts = first[1:] - first[:-1]
    first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    first[1:] = torch.cumsum(counts, 0)
    rows = int(first[-1])
    rd = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), counts)
    k = torch.arange(rows, dtype=torch.int64, device=dev) - first[rd]
    if which == "dense":
        return first, (k * DENSE_S).to(torch.int32), L
    g = torch.Generator(device=dev).manual_seed(seed)
    span = torch.clamp(lens.to(torch.int64)[rd] - L + 1, min=1)
    st = (torch.rand(rows, generator=g, device=dev, dtype=torch.float64) * span).to(torch.int64)
    order = torch.argsort(rd * (1 << 32) + st)   # sorted within every read
    return first, st[order].to(torch.int32), L


def case(c, lens, reps, only, seed, dense_div):
    dev = c.device
    n = int(lens.numel())
    opts = c.options(True, 2, 1, 1)
    with torch.cuda.stream(c.stream):
        sizes = lens.to(torch.int64) * 2
        off, total = batch.layout(sizes.cpu() + 2, 64)   # (one element behind every slot: the unfused route's pad)
        off = off.to(dev)
        raw = torch.empty(total, dtype=torch.uint8, device=dev)
        c.synth_signal(seed, 0, raw, off, lens)
        caps = torch.tensor([c.L.vbz_max_compressed_size(int(s), ctypes.byref(opts)) for s in sizes.cpu().tolist()], dtype=torch.int64)
        coff, ctotal = batch.layout(caps, 64)
        comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
        coff = coff.to(dev)
        csize = torch.zeros(n, dtype=torch.int32, device=dev)
        c.compress(raw, off, sizes.to(torch.int32).to(dev), comp, coff, caps.to(torch.int32).to(dev), csize, opts)
    torch.cuda.synchronize()
    del raw
    size32 = sizes.to(torch.int32).to(dev)
    g = torch.Generator().manual_seed(seed)
    o_t = (torch.rand(n, generator=g) * 400 - 200).to(dev)
    s_t = (torch.rand(n, generator=g) * 0.3 + 0.05).to(dev)
    sig = torch.empty(total // 2, dtype=torch.float16, device=dev)
    sig_off = off // 2
    sig[sig_off + lens.to(torch.int64)] = PAD
    sres = torch.zeros(n, dtype=torch.int32, device=dev)
    f = _lib.GpuSignalFormat()
    f.out_type, f.is_signed, f.offset, f.scale = _lib.VBZ_GPU_SIGNAL_F16, 1, o_t.data_ptr(), s_t.data_ptr()
    row = {"reads": n, "samples": int(lens.to(torch.int64).sum()), "ms": {}}
    for which in ("grid", "random", "dense"):
        if only and which not in only:
            continue
        m = n if which != "dense" else max(n // dense_div, 1)   # the reads this list runs over (a prefix of the batch)
        first, start, L = window_lists(c, lens[:m], which, seed)
        rows = int(first[-1])
        free = torch.cuda.mem_get_info()[0]
        while m > 1 and rows * L * (2 + 2 + 8) + (1 << 30) > free:   # the fused arena, the gathered one and the index
            m //= 2
            first, start, L = window_lists(c, lens[:m], which, seed)
            rows = int(first[-1])
        out = torch.empty((rows, L), dtype=torch.float16, device=dev)
        wres = torch.zeros(m, dtype=torch.int32, device=dev)
        b = c._batch(comp, coff[:m], csize[:m], torch.empty(0, dtype=torch.uint8, device=dev), off[:m], size32[:m], wres)
        b.dst, b.dst_bytes = None, total
        fm = _lib.GpuSignalFormat()
        fm.out_type, fm.is_signed, fm.offset, fm.scale = f.out_type, 1, o_t.data_ptr(), s_t.data_ptr()
        w = _lib.GpuWindows()
        w.window_len, w.pad, w.window_rows, w.window_first, w.start = L, PAD, rows, first.data_ptr(), start.data_ptr()
        fres = torch.zeros(m, dtype=torch.int32, device=dev)

        def f16(m=m, fres=fres):
            c.decompress_signal(comp, coff[:m], csize[:m], sig, off[:m], size32[:m], fres, opts, scale=s_t, offset=o_t)

        def fused(b=b, fm=fm, w=w, out=out):
            rc = c.L.vbz_gpu_decompress_windows_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 0, ctypes.byref(fm), ctypes.byref(w), out.data_ptr(), None,
                                                      None, None)
            assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)

        plan = gather_plan(c, start, lens[:m], sig_off[:m], first, L)
        gathered = torch.empty(rows * L, dtype=torch.float16, device=dev)

        def unfused(plan=plan, gathered=gathered, L=L):
            f16()
            for lo, hi, r0, r1, idx in plan:
                torch.index_select(sig[lo:hi], 0, idx, out=gathered[r0 * L : r1 * L])

        fns = {"f16": f16, "windows": fused, "f16+gather": unfused}
        chunks = None
        if which == "grid":
            ch = c._chunking(L_, S_, "pad", 0, PAD)
            chunks = torch.empty((rows, L), dtype=torch.float16, device=dev)
            cres = torch.zeros(m, dtype=torch.int32, device=dev)
            bc = c._batch(comp, coff[:m], csize[:m], torch.empty(0, dtype=torch.uint8, device=dev), off[:m], size32[:m], cres)
            bc.dst, bc.dst_bytes = None, total

            def chunk_call(bc=bc, ch=ch, first=first, chunks=chunks, rows=rows):
                rc = c.L.vbz_gpu_decompress_chunks_batch(c.ctx, ctypes.byref(bc), ctypes.byref(opts), 0, ctypes.byref(fm), ctypes.byref(ch), first.data_ptr(),
                                                         chunks.data_ptr(), rows)
                assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)

            fns["chunks_pad"] = chunk_call
        ms = timed(c, fns, reps)
        torch.cuda.synchronize()
        assert torch.equal(wres.to(torch.int64), lens[:m].to(torch.int64) * 2), which
        assert torch.equal(out.view(-1).view(torch.int16), gathered.view(torch.int16)), "%s != the unfused gather" % which
        if chunks is not None:
            assert torch.equal(out.view(torch.int16), chunks.view(torch.int16)), "the grid's windows != the chunk call"
        row[which] = {"reads": m, "rows": rows, "window_len": L, "coverage": round(rows * L / max(int(lens[:m].to(torch.int64).sum()), 1), 3), "ms": ms,
                      "gather_over_windows": round(ms["f16+gather"] / ms["windows"], 3), "windows_over_f16": round(ms["windows"] / ms["f16"], 3),
                      "checked": True}
        del out, gathered, plan, fns, chunks
        torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", action="append", default=[], help="time only these lists (grid, random, dense)")
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    out = {"headline": case(c, c.synth_lengths(5, 0, args.reads), args.reps, args.only, 5, 8)}
    torch.cuda.empty_cache()
    out["one_20M_read"] = case(c, torch.tensor([20_000_000], dtype=torch.int32, device=c.device), args.reps, args.only, 7, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
