#!/usr/bin/env python3
"""Cost of decoding straight into model-input chunks (vbz_gpu_decompress_chunks_batch) against the signal decode and the unfused route,
alternating in one process.

Headline: 65 536 synthetic reads (~100 k int16 samples each) compressed once; chunks of L = 10 000 samples every S = 9 504 (S / L = 0.95; S is a multiple of 8)
(float16); then, each behind untimed warm-up calls and timed with HIP events on the codec's stream (median of --reps calls):
  int16            vbz_gpu_decompress_batch into an int16 arena
  f16              vbz_gpu_decompress_signal_batch into a float16 arena (random per-read offset and scale)
  chunks_pad       the fused chunk decode, PAD (the last chunk padded past the read's end)
  chunks_end       the fused chunk decode, END with end_align 1 (the last chunk pulled back: its start is mostly not a multiple of 8)
  f16+gather_pad / f16+gather_end   the cheapest unfused route: the f16 decode, then a torch gather (index_select) of the float16 arena
                   through a precomputed flat int64 index of every chunk position (a pad position indexes the pad value stored right behind
                   its read's samples), issued in blocks of whole reads below 2^30 elements of source and output each (~7 at the headline)
Then one 20 M-sample read (the large-read path), the same calls.  The schemes are timed one after the other (the unfused route's index
is 8 bytes per chunk position), int16 and f16 alternating with each.  Every fused chunk arena is checked bit for bit against the unfused
one of the same scheme in the same run.  The layout (vbz_gpu_chunk_layout_batch) is made once per scheme, outside the timed calls.

    python tools/time_chunks.py [--reads 65536] [--reps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_chunks.py --reps 3 --only chunks_end"""
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


def gather_plan(c, info, lens, sig_off, first, L, limit=1 << 30):
    """The unfused route's index, in blocks of whole reads that keep every gather below 2^30 elements of source and of output:
    [(source lo, source hi, row lo, row hi, int64 index relative to lo)].  A position past a read's end indexes the read's pad element
    (the arena element right behind its samples)."""
    dev = c.device
    lens_h, off_h, first_h = lens.cpu().tolist(), sig_off.cpu().tolist(), first.cpu().tolist()
    ar = torch.arange(L, dtype=torch.int64, device=dev)[None, :]
    lens64 = lens.to(torch.int64)
    plan, n, a = [], len(lens_h), 0
    while a < n:
        b = a + 1
        while b < n and off_h[b] + lens_h[b] + 1 - off_h[a] < limit and (first_h[b + 1] - first_h[a]) * L < limit:
            b += 1
        lo, hi, r0, r1 = off_h[a], off_h[b - 1] + lens_h[b - 1] + 1, first_h[a], first_h[b]
        if r1 > r0:
            rd = info[r0:r1, 0].to(torch.int64)
            pos = info[r0:r1, 1].to(torch.int64)[:, None] + ar
            T = lens64[rd][:, None]
            base = sig_off[rd][:, None] - lo
            plan.append((lo, hi, r0, r1, (base + torch.where(pos < T, pos, T)).reshape(-1)))
        a = b
    return plan


def case(c, lens, reps, only, seed):
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
    samples = int(lens.to(torch.int64).sum())
    size32 = sizes.to(torch.int32).to(dev)
    back = torch.empty(total, dtype=torch.uint8, device=dev)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(seed)
    o_t = (torch.rand(n, generator=g) * 400 - 200).to(dev)
    s_t = (torch.rand(n, generator=g) * 0.3 + 0.05).to(dev)
    # the float16 arena: the int16 layout at 2 bytes per sample, the pad value right behind every read's samples (the unfused gather's)
    sig = torch.empty(total // 2, dtype=torch.float16, device=dev)
    sig_off = off // 2
    sig[sig_off + lens.to(torch.int64)] = PAD
    sres = torch.zeros(n, dtype=torch.int32, device=dev)

    def int16():
        c.decompress(comp, coff, csize, back, off, size32, res, opts)

    def f16():
        c.decompress_signal(comp, coff, csize, sig, off, size32, sres, opts, scale=s_t, offset=o_t)

    f = _lib.GpuSignalFormat()
    f.out_type, f.is_signed, f.offset, f.scale = _lib.VBZ_GPU_SIGNAL_F16, 1, o_t.data_ptr(), s_t.data_ptr()
    row = {"reads": n, "samples": samples, "chunk_len": L_, "step": S_, "ms": {}}
    # one scheme at a time (the flat index of the unfused route is 8 bytes per chunk position): int16, f16, the fused chunk decode and the
    # unfused route alternating
    for mode in ("pad", "end"):
        ck, gk = "chunks_" + mode, "f16+gather_" + mode
        if only and ck not in only and gk not in only:
            continue
        ch = c._chunking(L_, S_, mode, 1, PAD)
        first, info = c.chunk_layout(lens, L_, S_, mode=mode, end_align=1)
        rows = int(first[-1])
        chunks = torch.empty((rows, L_), dtype=torch.float16, device=dev)
        cres = torch.zeros(n, dtype=torch.int32, device=dev)
        b = c._batch(comp, coff, csize, back, off, size32, cres)
        b.dst, b.dst_bytes = None, total

        def fused(b=b, ch=ch, first=first, chunks=chunks, rows=rows):
            rc = c.L.vbz_gpu_decompress_chunks_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(ch), first.data_ptr(),
                                                     chunks.data_ptr(), rows)
            assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)

        fns = {"int16": int16, "f16": f16, ck: fused}
        gathered = plan = None
        if not only or gk in only:
            plan = gather_plan(c, info, lens, sig_off, first, L_)
            gathered = torch.empty(rows * L_, dtype=torch.float16, device=dev)

            def unfused(plan=plan, gathered=gathered):
                f16()
                for lo, hi, r0, r1, idx in plan:
                    torch.index_select(sig[lo:hi], 0, idx, out=gathered[r0 * L_ : r1 * L_])

            fns[gk] = unfused
        del info
        if only:
            fns = {k: fn for k, fn in fns.items() if k in only}
        ms = timed(c, fns, reps)
        torch.cuda.synchronize()
        for k, v in ms.items():
            row["ms"][k if k in (ck, gk) else k + "_" + mode + "_run"] = v
        if ck in ms and "f16" in ms:
            row[ck + "_over_f16"] = round(ms[ck] / ms["f16"], 3)
        if ck in ms and gk in ms:
            row[gk + "_over_" + ck] = round(ms[gk] / ms[ck], 3)
        row[ck + "_rows"] = rows
        if ck in fns:   # every fused call reported samples * 2
            assert torch.equal(cres.to(torch.int64), lens.to(dev).to(torch.int64) * 2), ck
        if ck in fns and gk in fns:   # fused == unfused, bit for bit
            assert torch.equal(chunks.view(-1).view(torch.int16), gathered.view(torch.int16)), "%s != the unfused gather" % ck
            row["checked_" + mode] = True
        del chunks, gathered, plan, fns
        torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", action="append", default=[],
                    help="time only these calls (int16, f16, chunks_pad, chunks_end, f16+gather_pad, f16+gather_end)")
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    out = {"headline": case(c, c.synth_lengths(5, 0, args.reads), args.reps, args.only, 5)}
    torch.cuda.empty_cache()
    out["one_20M_read"] = case(c, torch.tensor([20_000_000], dtype=torch.int32, device=c.device), args.reps, args.only, 7)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
