#!/usr/bin/env python3
"""One call of every typed decode entry, batch and POD5, for comparing what two builds of libvbz_hip.so queue: after every call the
library's launch labels and their counts (vbz_gpu_profile_read) go to stdout.  Under a kernel trace the ordered kernel names come out too:

    VBZ_HIP_LIB=<lib> [VBZ_HIP_SPLIT_MIN=64] rocprofv3 --kernel-trace -f csv -d <dir> -- python profiles/job_typed_launches.py [--long]
    python profiles/job_typed_launches.py --names <dir>      # the trace's kernel names in the order they were queued

--long puts one read of 300 000 samples among the 200 short ones (per-read routing).  Every call runs on a context of its own that has seen
no frames: a context whose last call left most of its frames to the one-wavefront decoder runs the next call as one group (foreign_host in
vbz_api.hip), and these synthetic reads do that -- so with VBZ_HIP_SPLIT_MIN=64 every call really is a split one (zstd_decode 2)."""
import argparse
import csv
import glob
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--long", action="store_true")
ap.add_argument("--names", metavar="DIR")
args = ap.parse_args()
if args.names:
    rows = []
    for path in glob.glob(os.path.join(args.names, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    for r in sorted(rows, key=lambda r: int(r["Dispatch_Id"])):
        print(r["Kernel_Name"])
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes

import torch
from vbz_compression_amd import batch

c = batch.GpuCodec(0)
torch.cuda.set_stream(c.stream)
dev = c.device
N = 200


def frames(lens, opts, cap_of):
    """device-synthesised reads of `lens` samples, compressed: (src, src_off, src_size)"""
    sizes = [2 * t for t in lens]
    off, total = batch.layout(sizes, 64)
    raw = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    c.synth_signal(5, 0, raw, off.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev))
    caps = [cap_of(t) for t in lens]
    coff, ctotal = batch.layout(caps, 64)
    comp = torch.zeros(ctotal + 64, dtype=torch.uint8, device=dev)
    res = torch.zeros(len(lens), dtype=torch.int32, device=dev)
    c.compress(raw, off.to(dev), torch.tensor(sizes, dtype=torch.int32, device=dev), comp, coff.to(dev), torch.tensor(caps, dtype=torch.int32, device=dev), res, opts)
    c.synchronize()
    return comp, coff.to(dev), res


def tables(lens, per_read=3):
    """window_first / event_first and ascending starts, `per_read` rows per read"""
    first = torch.arange(0, per_read * len(lens) + 1, per_read, dtype=torch.int64, device=dev)
    start = torch.tensor([k * max(t // per_read, 1) for t in lens for k in range(per_read)], dtype=torch.int32, device=dev)
    return first, start


used = []   # (the contexts stay until the process ends)


def one(name, fn):
    global c
    torch.cuda.synchronize()
    used.append(c)
    c = batch.GpuCodec(0)   # (it has seen no frames: nothing but the knobs decides the call's shape)
    torch.cuda.set_stream(c.stream)
    c.profile_reset()
    c.profile(True)
    fn()
    c.synchronize()
    torch.cuda.synchronize()
    c.profile(False)
    print("== " + name)
    for label, (launches, _) in c.profile_read().items():
        print("%-24s %d" % (label, launches))


lens = [3000 + 25 * i for i in range(N)]
if args.long:
    lens[N // 2 + 17] = 300_000
opts = c.options(True, 2, 1, 1)
src, off, size = frames(lens, opts, lambda t: c.L.vbz_max_compressed_size(2 * t, ctypes.byref(opts)))
samples = torch.tensor(lens, dtype=torch.int32, device=dev)
doff, dcap = c._row_layout(samples)
doff = doff[:N].contiguous()
res = torch.zeros(N, dtype=torch.int32, device=dev)
out = torch.empty(sum(lens) + 64, dtype=torch.float32, device=dev)
first, start = tables(lens)
norm = batch.MED_MAD
bg, en = [7] * N, [t - 100 for t in lens]
one("signal", lambda: c.decompress_signal(src, off, size, out, doff * 2, dcap * 2, res, opts))
one("signal_norm", lambda: c.decompress_signal(src, off, size, out, doff * 2, dcap * 2, res, opts, norm=norm))
one("chunks", lambda: c.decompress_chunks(src, off, size, samples, res, opts, 512, 256))
one("chunks_norm", lambda: c.decompress_chunks(src, off, size, samples, res, opts, 512, 256, norm=norm))
one("chunks_range", lambda: c.decompress_chunks(src, off, size, samples, res, opts, 512, 256, norm=norm, begin=bg, end=en))
one("windows", lambda: c.decompress_windows(src, off, size, samples, res, opts, first, start, 256, begin=bg, end=en))
one("signal_events", lambda: c.signal_events(src, off, size, doff, dcap, res, opts, first, start, norm=norm))
one("statistics", lambda: c.signal_norm(src, off, size, doff, dcap, res, opts, norm))
one("statistics_range", lambda: c.signal_norm(src, off, size, doff, dcap, res, opts, norm, begin=bg, end=en))
one("signal_trim", lambda: c.signal_trim(src, off, size, doff, dcap, res, opts, norm, shift_scale=True))
one("signal_segment", lambda: c.signal_segment(src, off, size, doff, dcap, res, opts, begin=bg, end=en))

# POD5: two rows a read
rows = [t // 2 for t in lens for _ in range(2)]
popts = batch.pod5_options(1)
psrc, poff, psize = frames(rows, popts, batch.pod5_max_compressed_size)
row_samples = torch.tensor(rows, dtype=torch.int32, device=dev)
read_first = list(range(0, 2 * N, 2))
pres = torch.zeros(2 * N, dtype=torch.int32, device=dev)
rlens = [2 * (t // 2) for t in lens]
pfirst, pstart = tables(rlens)
pbg, pen = [7] * N, [t - 100 for t in rlens]
one("pod5_signal_norm", lambda: c.pod5_decompress_signal_norm(psrc, poff, psize, rows, read_first, pres, norm))
one("pod5_chunks", lambda: c.pod5_decompress_chunks(psrc, poff, psize, row_samples, read_first, pres, 512, 256))
one("pod5_chunks_norm", lambda: c.pod5_decompress_chunks(psrc, poff, psize, row_samples, read_first, pres, 512, 256, norm=norm))
one("pod5_chunks_range", lambda: c.pod5_decompress_chunks(psrc, poff, psize, row_samples, read_first, pres, 512, 256, norm=norm, begin=pbg, end=pen))
one("pod5_windows", lambda: c.pod5_decompress_windows(psrc, poff, psize, row_samples, read_first, pres, pfirst, pstart, 256))
one("pod5_signal_events", lambda: c.pod5_signal_events(psrc, poff, psize, row_samples, read_first, pres, pfirst, pstart, norm=norm))
one("pod5_statistics", lambda: c.pod5_signal_norm(psrc, poff, psize, row_samples, read_first, pres, norm))
one("pod5_statistics_range", lambda: c.pod5_signal_norm(psrc, poff, psize, row_samples, read_first, pres, norm, begin=pbg, end=pen))
one("pod5_signal_trim", lambda: c.pod5_signal_trim(psrc, poff, psize, row_samples, read_first, pres, norm))
one("pod5_signal_segment", lambda: c.pod5_signal_segment(psrc, poff, psize, row_samples, read_first, pres, begin=pbg, end=pen))
bad = [hex(v & 0xFFFFFFFF) for v in res.tolist() + pres.tolist() if (v & 0xFFFFFFFF) >= 0xFFFFFFF0]
print("== error verdicts of the last calls:", bad[:4] or "none")
