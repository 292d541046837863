#!/usr/bin/env python3
"""Rates of the content checksum's hash (vbz_gpu_xxh64_batch, xxh64.hip): one 40 MB buffer -- one quad of lanes, the serial chain --
and 65 536 reads of 90 - 110 KB, median of 10 calls behind 3 untimed ones (HIP events on the codec's stream); then, for a kernel trace,
one encode + decode of 16 384 bench-shaped reads with the checksum writer on.

    python tools/time_xxh64.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_xxh64.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from vbz_compression_amd import _lib, batch  # noqa: E402


def rate(c, sizes, reps=10):
    sizes = torch.tensor(sizes, dtype=torch.int64)
    off = torch.zeros_like(sizes)
    off[1:] = torch.cumsum(sizes, 0)[:-1]
    total = int(sizes.sum())
    src = torch.randint(0, 256, (total + 256,), dtype=torch.uint8, device=c.device)
    o, s = off.to(c.device), sizes.to(torch.int32).to(c.device)
    out = torch.zeros(len(sizes), dtype=torch.int64, device=c.device)
    with torch.cuda.stream(c.stream):
        for _ in range(3):
            c.xxh64(src, o, s, out)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(reps):
            a.record(c.stream)
            c.xxh64(src, o, s, out)
            b.record(c.stream)
            b.synchronize()
            ts.append(a.elapsed_time(b))
    ts.sort()
    return total, ts[len(ts) // 2], ts[0], ts[-1]


def main():
    c = batch.GpuCodec(0)
    for name, sizes in (("one 40 MB buffer", [40_000_000]), ("65536 reads of 90-110 KB", [90_000 + (i * 7919) % 20001 for i in range(65536)])):
        total, med, lo, hi = rate(c, sizes)
        print("%s: %.3f ms median (min %.3f, max %.3f), %.2f GB/s" % (name, med, lo, hi, total / med / 1e6), flush=True)
    # the writer and the check at the bench's shape (for the kernel trace)
    n = 16384
    ln = c.synth_lengths(5, 0, n)
    lens = ln.cpu().tolist()
    off, total = batch.layout([2 * x for x in lens], 64, c.device)
    raw = torch.zeros(total, dtype=torch.uint8, device=c.device)
    c.synth_signal(5, 0, raw, off, ln)
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    L = _lib.load()
    import ctypes

    caps = [L.vbz_max_compressed_size(2 * x, ctypes.byref(opts)) for x in lens]
    coff, ctotal = batch.layout(caps, 64, c.device)
    comp = torch.zeros(ctotal, dtype=torch.uint8, device=c.device)
    res = torch.zeros(n, dtype=torch.int32, device=c.device)
    nbytes = torch.tensor([2 * x for x in lens], dtype=torch.int32, device=c.device)
    capt = torch.tensor(caps, dtype=torch.int64).to(torch.int32).to(c.device)
    back = torch.zeros_like(raw)
    res2 = torch.zeros(n, dtype=torch.int32, device=c.device)
    c.set_checksum(1)
    for _ in range(3):
        c.compress(raw, off, nbytes, comp, coff, capt, res, opts)
        c.decompress(comp, coff, res, back, off, nbytes, res2, opts)
    torch.cuda.synchronize()
    assert torch.equal(res2, nbytes) and torch.equal(back, raw)
    print("16384 reads: encode + decode with checksums x 3, round trip verified", flush=True)


if __name__ == "__main__":
    main()
