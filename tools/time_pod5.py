#!/usr/bin/env python3
"""Cost of the POD5 codec (svb16 + zstd, include/vbz_gpu.h: VBZ_GPU_VERSION_POD5) next to v0 on the same signal, alternating in one process.

Headline: 65 536 synthetic reads (~100 k int16 samples each), each coded once as a POD5 row and once as a v0 read; then,
each behind untimed warm-up calls and timed with HIP events on the codec's stream (median of --reps calls, the calls alternating):
  compress   vbz_gpu_compress_batch, POD5 against v0
  int16      vbz_gpu_decompress_batch into an int16 arena
  chunks     vbz_gpu_decompress_chunks_batch, float16, L = 10 000, S = 9 504, PAD, random per-read offset and scale
and the compressed bytes of both.  Then 2 048 rows libzstd wrote (as pod5 does; the v0 frames of the same signal by the reference's
path, as tools/time_foreign_decode.py decodes them), and one 20 M-sample row (compress, int16 decode).  Every decode is checked against
the signal it came from.

    python tools/time_pod5.py [--reads 65536] [--reps 20]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
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


OPTS = {"pod5": batch.pod5_options(), "v0": batch.GpuCodec.options(True, 2, 1, 0)}


def cap_of(c, name, nbytes):
    if name == "pod5":
        return batch.pod5_max_compressed_size(nbytes // 2)
    return c.L.vbz_max_compressed_size(int(nbytes), ctypes.byref(OPTS[name]))


def device_case(c, lens, reps, seed, chunks=True):
    """both codecs on device-synthesised signal of reads of `lens` samples"""
    dev = c.device
    n = int(lens.numel())
    sizes = lens.to(torch.int64).cpu() * 2
    off, total = batch.layout(sizes, 64)
    off = off.to(dev)
    size32 = sizes.to(torch.int32).to(dev)
    raw = torch.empty(total, dtype=torch.uint8, device=dev)
    c.synth_signal(seed, 0, raw, off, lens)
    comp = {}
    for name in OPTS:
        caps = torch.tensor([cap_of(c, name, int(s)) for s in sizes.tolist()], dtype=torch.int64)
        coff, ctotal = batch.layout(caps, 64)
        arena = torch.empty(ctotal, dtype=torch.uint8, device=dev)
        res = torch.zeros(n, dtype=torch.int32, device=dev)
        comp[name] = (arena, coff.to(dev), caps.to(torch.int32).to(dev), res)
    fns = {}
    for name, (arena, coff, cap, res) in comp.items():
        fns["compress_" + name] = lambda name=name, arena=arena, coff=coff, cap=cap, res=res: c.compress(raw, off, size32, arena, coff, cap, res,
                                                                                                          OPTS[name])
    ms = timed(c, fns, reps)
    torch.cuda.synchronize()
    row = {"reads": n, "samples": int(lens.to(torch.int64).sum()), "ms": ms, "bytes": {}}
    for name, (_, _, _, res) in comp.items():
        assert int(res.min()) >= 0, name
        row["bytes"][name] = int(res.to(torch.int64).sum())
    row["bytes"]["pod5_over_v0"] = round(row["bytes"]["pod5"] / row["bytes"]["v0"], 4)
    back = {k: torch.empty(total, dtype=torch.uint8, device=dev) for k in OPTS}
    dres = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in OPTS}
    fns = {}
    for name, (arena, coff, _, res) in comp.items():
        fns["int16_" + name] = lambda name=name, arena=arena, coff=coff, res=res: c.decompress(arena, coff, res, back[name], off, size32, dres[name],
                                                                                               OPTS[name])
    if chunks:
        L, S = 10_000, 9_504
        ch = c._chunking(L, S, "pad", 1)
        chunk_first, _ = c.chunk_layout(lens, L, S, "pad", info=False)
        rows = int(chunk_first[-1])
        g = torch.Generator().manual_seed(seed)
        o_t = (torch.rand(n, generator=g) * 400 - 200).to(dev)
        s_t = (torch.rand(n, generator=g) * 0.3 + 0.05).to(dev)
        outs = {k: torch.empty((rows, L), dtype=torch.float16, device=dev) for k in OPTS}
        cres = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in OPTS}
        for name, (arena, coff, _, res) in comp.items():
            fns["chunks_f16_" + name] = lambda name=name, arena=arena, coff=coff, res=res: c._decode_chunks(
                arena, coff, res, off, size32, total, cres[name], OPTS[name], False, ch, chunk_first, outs[name], torch.float16, s_t, o_t, True)
    ms = timed(c, fns, reps)
    torch.cuda.synchronize()
    row["ms"].update(ms)
    for name in OPTS:
        assert torch.equal(dres[name], size32), name
        assert torch.equal(back[name], raw), name
        if chunks:
            assert torch.equal(cres[name], size32), name
    if chunks:
        assert torch.equal(outs["pod5"], outs["v0"]), "chunks differ"
    for k in ("compress", "int16", "chunks_f16"):
        if k + "_pod5" in row["ms"]:
            row[k + "_pod5_over_v0"] = round(row["ms"][k + "_pod5"] / row["ms"][k + "_v0"], 3)
    return row


def foreign_case(c, n, reps, seed):
    """rows libzstd wrote (pod5's compress_signal) and the v0 frames the reference's path writes, of the same signal"""
    import oracle_lib as O
    import pod5_ref as P

    dev = c.device
    reads = [O.synth_signal(seed, i, O.synth_read_length(seed, i)) for i in range(n)]
    frames = {"pod5": [P.compress_row(x) for x in reads], "v0": [O.compress(x, O.options(True, 2, 1, 0)) for x in reads]}
    sizes = [2 * len(x) for x in reads]
    off, total = batch.layout(sizes, 64)
    off = off.to(dev)
    size32 = torch.tensor(sizes, dtype=torch.int32, device=dev)
    want = np.zeros(total, np.uint8)
    for x, o in zip(reads, off.tolist()):
        want[o : o + x.nbytes] = x.view(np.uint8)
    fns, outs = {}, {}
    for name, fr in frames.items():
        fsz = [len(f) for f in fr]
        foff, ftotal = batch.layout(fsz, 16)
        a = np.zeros(ftotal + 64, np.uint8)
        for f, o in zip(fr, foff.tolist()):
            a[o : o + len(f)] = f
        src = torch.from_numpy(a).to(dev)
        foff = foff.to(dev)
        fs = torch.tensor(fsz, dtype=torch.int32, device=dev)
        out = torch.zeros(total, dtype=torch.uint8, device=dev)
        res = torch.zeros(n, dtype=torch.int32, device=dev)
        outs[name] = (out, res)
        fns["int16_" + name] = lambda name=name, src=src, foff=foff, fs=fs, out=out, res=res: c.decompress(src, foff, fs, out, off, size32, res,
                                                                                                          OPTS[name])
    ms = timed(c, fns, reps)
    torch.cuda.synchronize()
    for name, (out, res) in outs.items():
        assert torch.equal(res, size32), name
        assert (out.cpu().numpy() == want).all(), name
    return {"reads": n, "samples": int(sum(sizes) // 2), "ms": ms, "pod5_over_v0": round(ms["int16_pod5"] / ms["int16_v0"], 3),
            "frame_bytes": {k: int(sum(len(f) for f in v)) for k, v in frames.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--foreign", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    out = {"headline": device_case(c, c.synth_lengths(5, 0, args.reads), args.reps, 5)}
    torch.cuda.empty_cache()
    out["libzstd_rows"] = foreign_case(c, args.foreign, args.reps, 5)
    torch.cuda.empty_cache()
    out["one_20M_row"] = device_case(c, torch.tensor([20_000_000], dtype=torch.int32, device=c.device), args.reps, 7, chunks=False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
