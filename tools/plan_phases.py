#!/usr/bin/env python3
"""Per-phase shader-clock cycles of the staged encoder's planning launch (zstd_plan_kernel) UNDER LOAD, per role, on the bench workload:

    python tools/plan_phases.py [--reads 65536] [--calls 3] [--lib path/to/libvbz_hip_x.so]

The timed instantiation lives in the experiments build of the library (lib/libvbz_hip_x.so, -DVBZ_EXPERIMENTS); this tool selects it
(VBZ_HIP_LIB) and sets VBZ_HIP_PHASE_TIMING=2.  The library prints two lines per encode call on stderr (dbg_end_roles in vbz_api.hip):
role 0 (control bytes: tokeniser, sequences section, the literals' table) and role 1 (the data bytes' table), each the average over the
wavefronts of that role that planned their read, slots as listed in the line.  The timers cost registers of their own, so the timed
launch may run at another occupancy than the product's: compare builds with each other, not with kernel times."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=65536)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--lib", default=os.path.join(ROOT, "vbz_compression_amd", "lib", "libvbz_hip_x.so"))
args = ap.parse_args()
os.environ["VBZ_HIP_LIB"] = os.path.abspath(args.lib)
os.environ["VBZ_HIP_PHASE_TIMING"] = "2"
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from vbz_compression_amd import batch  # noqa: E402

codec = batch.GpuCodec(0)
torch.cuda.set_stream(codec.stream)
opts = codec.options(True, 2, 1, 1)
L = codec.L
n = args.reads
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
print("library", L.vbz_gpu_version().decode(), "reads", n, flush=True)
for i in range(args.calls):
    print("call", i, flush=True)
    sys.stderr.flush()
    codec.compress(raw, off, s32, comp, coff, cap32, cs, opts)
    torch.cuda.synchronize()
    sys.stderr.flush()
codec.decompress(comp, coff, cs, back, off, s32, res, opts)
torch.cuda.synchronize()
assert torch.equal(raw, back), "round trip"
print("round trip ok", flush=True)
