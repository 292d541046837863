#!/usr/bin/env python3
"""Cost of decoding straight to calibrated samples (vbz_gpu_decompress_signal_batch) against the int16 decode, alternating in one process.

Headline: 65 536 synthetic reads (~100 k int16 samples each) compressed once; then, each behind untimed warm-up calls and
timed with HIP events on the codec's stream (median of --reps calls):
  int16          vbz_gpu_decompress_batch into an int16 arena
  int16+convert  the same, then the cheapest unfused conversion, (x.float() + o) * s with scalar o and s (a lower bound for any
                 unfused route: per-read constants cost a gather on top)
  f32 / f16 / bf16   the fused decode, random per-read offset and scale
Then one 20 M-sample read (the large-read path): int16, int16+convert and f32.  The fused outputs are checked against the unfused ones
(float32: bit for bit; the scalar constants of the unfused route are those of read 0 of the fused call, applied to every read).

    python tools/time_signal.py [--reads 65536] [--reps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_signal.py --reps 3 --only f32"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vbz_compression_amd import batch  # noqa: E402


def timed(c, fns, reps, warm=3):
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


def case(c, lens, reps, only, seed):
    dev = c.device
    n = int(lens.numel())
    opts = c.options(True, 2, 1, 1)
    with torch.cuda.stream(c.stream):
        sizes = lens.to(torch.int64) * 2
        off, total = batch.layout(sizes.cpu(), 64)
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
    o0, s0 = float(o_t[0]), float(s_t[0])
    conv = {}

    def int16():
        c.decompress(comp, coff, csize, back, off, size32, res, opts)

    def int16_convert():
        int16()
        conv["y"] = (back.view(torch.int16).float() + o0) * s0

    fused_out, fused_res = {}, {}
    fns = {"int16": int16, "int16+convert": int16_convert}
    for name, dt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
        if only and name not in only:
            continue
        E = torch.empty(0, dtype=dt).element_size()
        out = torch.empty(total // 2, dtype=dt, device=dev)
        r = torch.zeros(n, dtype=torch.int32, device=dev)
        fused_out[name], fused_res[name] = out, r
        fns[name] = (lambda out=out, r=r, E=E: c.decompress_signal(comp, coff, csize, out, off // 2 * E, size32 // 2 * E, r, opts, scale=s_t,
                                                                     offset=o_t))
    if only:
        fns = {k: f for k, f in fns.items() if k in only}
    ms = timed(c, fns, reps)
    torch.cuda.synchronize()
    row = {"reads": n, "samples": samples, "ms": ms}
    if "int16" in ms and "int16+convert" in ms:
        row["conversion_ms"] = round(ms["int16+convert"] - ms["int16"], 4)
        for k in ("f32", "f16", "bf16"):
            if k in ms:
                row[k + "_over_int16"] = round(ms[k] / ms["int16"], 3)
        if "f32" in ms:
            row["f32_added_share_of_conversion"] = round((ms["f32"] - ms["int16"]) / max(row["conversion_ms"], 1e-9), 3)
    # every fused call reported samples * E; float32 agrees bit for bit with the unfused route where the constants are read 0's
    for k, r in fused_res.items():
        E = 4 if k == "f32" else 2
        assert torch.equal(r.to(torch.int64), lens.to(dev).to(torch.int64) * E), k
    if "f32" in fused_out and "y" in conv:
        k0 = int(lens[0])
        assert torch.equal(fused_out["f32"][:k0].view(torch.int32), conv["y"][:k0].view(torch.int32)), "f32 != unfused"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", action="append", default=[], help="time only these calls (int16, int16+convert, f32, f16, bf16)")
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    out = {"headline": case(c, c.synth_lengths(5, 0, args.reads), args.reps, args.only, 5)}
    torch.cuda.empty_cache()
    only_large = [k for k in args.only if k in ("int16", "int16+convert", "f32")] or ["int16", "int16+convert", "f32"]
    out["one_20M_read"] = case(c, torch.tensor([20_000_000], dtype=torch.int32, device=c.device), args.reps, only_large, 7)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
