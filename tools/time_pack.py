#!/usr/bin/env python3
"""Rates of the dense-arena pack (vbz_gpu_pack_batch, pack.hip) against what a caller had before it, alternating in one process.

Headline: 65 536 synthetic reads (~100 k int16 samples each) compressed once; then, each behind untimed warm-up calls
and timed with HIP events on the codec's stream (median of --reps calls):
  pack_a1 / pack_a16   vbz_gpu_pack_batch at align 1 and 16, into a preallocated arena (no synchronisation)
  workaround           what tools/pcie_pipeline.py does: offsets from a torch cumsum, then a level-0 integer_size-0 compress call as a copier
  copy                 a plain device copy of the same byte count (torch's vectorised uint8 copy_, 16 bytes a lane)
Rates are bytes moved (each packed byte read once and written once: 2 x the packed total) per second, and the share of the copy's rate.
Then one 40 MB buffer and 2^20 reads of 1 - 64 bytes (fabricated slots), pack against copy.

    python tools/time_pack.py [--reads 65536] [--reps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_pack.py --reps 3"""
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
    return {k: statistics.median(v) for k, v in ms.items()}


def report(name, ms, moved, out):
    copy = ms["copy"]
    rows = {}
    for k, t in ms.items():
        rows[k] = {"ms": round(t, 4), "GB_per_s": round(moved / t / 1e6, 1), "share_of_copy": round(copy / t, 3)}
    out[name] = {"bytes_moved": moved, **rows}


def case_fabricated(c, sizes, reps, out, name):
    dev = c.device
    sizes = sizes.to(torch.int64)
    cap = sizes + 7
    off = torch.zeros_like(cap)
    off[1:] = torch.cumsum(cap, 0)[:-1]
    off += torch.arange(len(sizes), dtype=torch.int64) % 16   # every skew
    dst = torch.randint(0, 256, (int(off[-1] + cap[-1]) + 64,), dtype=torch.uint8, device=dev)
    o, k, r = off.to(dev), cap.to(torch.int32).to(dev), sizes.to(torch.int32).to(dev)
    total = int(sizes.sum())
    packed = torch.empty(total + 16 * len(sizes) + 64, dtype=torch.uint8, device=dev)
    a, b = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(total, dtype=torch.uint8, device=dev)
    ms = timed(c, {"pack_a1": lambda: c.pack(dst, o, k, r, 1, out=packed), "copy": lambda: b.copy_(a)}, reps)
    report(name, ms, 2 * total, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    dev = c.device
    n = args.reads
    opts = c.options(True, 2, 1, 1)
    copy_opts = c.options(False, 0, 0, 0)
    with torch.cuda.stream(c.stream):
        lens = c.synth_lengths(5, 0, n)
        sizes = lens.to(torch.int64) * 2
        off, total = batch.layout(sizes.cpu(), 64)
        raw = torch.empty(total, dtype=torch.uint8, device=dev)
        c.synth_signal(5, 0, raw, off.to(dev), lens)
        caps = torch.tensor([c.L.vbz_max_compressed_size(int(s), ctypes.byref(opts)) for s in sizes.cpu().tolist()], dtype=torch.int64)
        coff, ctotal = batch.layout(caps, 64)
        comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
        coff, cap32 = coff.to(dev), caps.to(torch.int32).to(dev)
        res = torch.zeros(n, dtype=torch.int32, device=dev)
        c.compress(raw, off.to(dev), sizes.to(torch.int32).to(dev), comp, coff, cap32, res, opts)
        packed, poff, psize = c.pack(comp, coff, cap32, res, 16)
    torch.cuda.synchronize()
    packed_bytes = int(res.to(torch.int64).sum())
    out = {"reads": n, "raw_bytes": int(sizes.sum()), "compressed_bytes": packed_bytes}
    arena1 = torch.empty(packed_bytes + 64, dtype=torch.uint8, device=dev)
    arena16 = torch.empty(int(poff[-1]) + 64, dtype=torch.uint8, device=dev)
    dense = torch.empty(packed_bytes + 64, dtype=torch.uint8, device=dev)
    doff = torch.zeros(n, dtype=torch.int64, device=dev)
    dres = torch.zeros(n, dtype=torch.int32, device=dev)
    ca, cb = torch.empty(packed_bytes, dtype=torch.uint8, device=dev), torch.empty(packed_bytes, dtype=torch.uint8, device=dev)

    def workaround():
        sz = res.to(torch.int64)
        doff.copy_(torch.cumsum(sz, 0) - sz)
        c.compress(comp, coff, res, dense, doff, res, dres, copy_opts)

    fns = {
        "pack_a1": lambda: c.pack(comp, coff, cap32, res, 1, out=arena1),
        "pack_a16": lambda: c.pack(comp, coff, cap32, res, 16, out=arena16),
        "workaround": workaround,
        "copy": lambda: cb.copy_(ca),
    }
    ms = timed(c, fns, args.reps)
    torch.cuda.synchronize()
    # the three arenas hold the same bytes
    assert torch.equal(arena1[:packed_bytes], dense[:packed_bytes])
    report("headline", ms, 2 * packed_bytes, out)
    del raw, comp, arena1, arena16, dense, ca, cb
    case_fabricated(c, torch.tensor([40 << 20]), args.reps, out, "one_40MB")
    g = torch.Generator().manual_seed(3)
    case_fabricated(c, torch.randint(1, 65, (1 << 20,), generator=g), args.reps, out, "tiny_2^20")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
