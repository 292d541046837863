#!/usr/bin/env python3
"""Which way fast_runs_kernel's zero-run blocks go on the bench workload: the share of chunks of 64 sequences that are built in LDS
(zstd_runs.h, place_zero_runs) and the share of sequences sections with checkpoints that are staged in LDS for the parallel walk
(zero_run_chain_segments).  Counted by the experiments build of the library (lib/libvbz_hip_x.so, vbz_gpu_x_runs_counts):

    VBZ_HIP_LIB=vbz_compression_amd/lib/libvbz_hip_x.so python tools/zero_run_paths.py [reads]
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vbz_compression_amd import batch

codec = batch.GpuCodec(0)
torch.cuda.set_stream(codec.stream)
L = codec.L
L.vbz_gpu_x_runs_counts.restype = ctypes.c_int
L.vbz_gpu_x_runs_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
opts = codec.options(True, 2, 1, 1)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
lens = codec.synth_lengths(5, 0, n)
sizes = lens.to(torch.int64) * 2
off, total = batch.layout(sizes.cpu(), 64)
raw = torch.empty(total, dtype=torch.uint8, device="cuda")
off = off.cuda()
codec.synth_signal(5, 0, raw, off, lens)
s32 = sizes.to(torch.int32)
caps = torch.tensor([L.vbz_max_compressed_size(int(s), ctypes.byref(opts)) for s in sizes.cpu().tolist()], dtype=torch.int64)
coff, ctotal = batch.layout(caps, 64)
comp = torch.empty(ctotal, dtype=torch.uint8, device="cuda")
coff = coff.cuda()
cap32 = caps.to(torch.int32).cuda()
cs = torch.zeros(n, dtype=torch.int32, device="cuda")
back = torch.empty_like(raw)
res = torch.zeros(n, dtype=torch.int32, device="cuda")
codec.compress(raw, off, s32, comp, coff, cap32, cs, opts)
out = (ctypes.c_ulonglong * 4)()
assert L.vbz_gpu_x_runs_counts(codec.ctx, out, 1) == 0
codec.decompress(comp, coff, cs, back, off, s32, res, opts)
assert L.vbz_gpu_x_runs_counts(codec.ctx, out, 1) == 0
assert torch.equal(raw, back)
chunks, in_lds, sections, staged = (int(x) for x in out)
print("reads %d  decode_paths %s  chunks %d in LDS %d (%.4f)  sections with checkpoints %d staged %d (%.4f)" % (
    n, codec.decode_paths(), chunks, in_lds, in_lds / max(chunks, 1), sections, staged, staged / max(sections, 1)))
