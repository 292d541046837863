#!/usr/bin/env python3
"""What fast_streams_kernel's refill path does on the bench workload: periods walked, periods in which the wavefront took the path, lanes
that issued (tools/stream_refill_model.py is the CPU model of the same three).  Counted by the counting twin of a variant in the
experiments build of the library (lib/libvbz_hip_x.so, vbz_gpu_x_streams_counts):

    VBZ_HIP_LIB=vbz_compression_amd/lib/libvbz_hip_x.so VBZ_HIP_FS_COUNT=1 VBZ_HIP_FS_VARIANT=8,7 python tools/stream_refill_counts.py [reads]
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
L.vbz_gpu_x_streams_counts.restype = ctypes.c_int
L.vbz_gpu_x_streams_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
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
out = (ctypes.c_ulonglong * 3)()
assert L.vbz_gpu_x_streams_counts(codec.ctx, out, 1) == 0
codec.decompress(comp, coff, cs, back, off, s32, res, opts)
assert L.vbz_gpu_x_streams_counts(codec.ctx, out, 1) == 0
assert torch.equal(raw, back)
periods, refills, issued = (int(x) for x in out)
assert periods > 0, "no counting kernel ran: VBZ_HIP_FS_COUNT=1 and the experiments build are needed"
print("variant %s  reads %d  decode_paths %s  periods %d  with refill %d (%.4f)  lanes issued %d (%.2f per refill)" % (
    os.environ.get("VBZ_HIP_FS_VARIANT", "shipped"), n, codec.decode_paths(), periods, refills, refills / periods, issued, issued / max(refills, 1)))
