#!/usr/bin/env python3
"""Cost of decoding straight into per-read normalised chunks (vbz_gpu_decompress_chunks_norm_batch) against the chunk call with given
constants and the unfused route, alternating in one process.

Headline: 65 536 synthetic reads (~100 k int16 samples each) compressed once; chunks of L = 10 000 samples every S = 9 504,
PAD, float16; then, each behind untimed warm-up calls and timed with HIP events on the codec's stream (median of --reps calls):
  chunks          vbz_gpu_decompress_chunks_batch with per-read constants given (random offset and scale)
  chunks_med_mad  vbz_gpu_decompress_chunks_norm_batch, MED_MAD (Bonito: (x - med) / (1.4826 MAD))
  chunks_quantile vbz_gpu_decompress_chunks_norm_batch, QUANTILE (Dorado: q20 / q90)
  stats_med_mad   vbz_gpu_signal_norm_batch, MED_MAD: the statistics alone
  unfused_med_mad the route without the feature: the int16 decode, a torch per-read median and MAD (rows of reads padded with the int16
                  maximum, sorted; blocks of 4 096 reads), then the chunk call with the constants they give
Then one 20 M-sample read (the large-read path), the same calls.  The normalised chunk arena is checked bit for bit against the chunk call
fed the constants the call reports, and against the unfused route's constants.

    python tools/time_norm.py [--reads 65536] [--reps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_norm.py --reps 3 --only chunks_med_mad"""
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
PAD = 0.0
BLOCK = 4096


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


def torch_med_mad(back16, off16, lens, maxT):
    """per-read median and MAD of the int16 arena in torch (float64 results): rows padded with 32767 sort behind every sample, so rank
    k < T of a sorted row is the read's; the deviations' pads are +inf"""
    n = int(lens.numel())
    dev = back16.device
    med = torch.empty(n, dtype=torch.float64, device=dev)
    mad = torch.empty(n, dtype=torch.float64, device=dev)
    ar = torch.arange(maxT, dtype=torch.int64, device=dev)[None, :]
    T = lens.to(torch.int64)
    for a in range(0, n, BLOCK):
        b = min(n, a + BLOCK)
        t = T[a:b][:, None]
        inside = ar < t
        idx = torch.where(inside, off16[a:b][:, None] + ar, 0)
        rows = torch.where(inside, back16[idx], torch.tensor(32767, dtype=torch.int16, device=dev))
        s, _ = torch.sort(rows, dim=1)
        j0, j1 = (t - 1).clamp(min=0) // 2, t // 2
        c = (s.gather(1, j0).double() + s.gather(1, j1).double()) / 2.0
        d = torch.where(inside, (rows.float() - c.float()).abs(), torch.tensor(float("inf"), device=dev))   # (exact: half-integers)
        d, _ = torch.sort(d, dim=1)
        med[a:b] = c[:, 0]
        mad[a:b] = ((d.gather(1, j0).double() + d.gather(1, j1).double()) / 2.0)[:, 0]
    return med, mad


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
    first, _ = c.chunk_layout(lens, L_, S_, mode="pad", info=False)
    rows = int(first[-1])
    ch = c._chunking(L_, S_, "pad", 1, PAD)

    def arena():
        return torch.empty((rows, L_), dtype=torch.float16, device=dev)

    outs = {k: arena() for k in ("chunks", "chunks_med_mad", "chunks_quantile", "unfused_med_mad")}
    ress = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in list(outs) + ["stats_med_mad"]}
    sss = {k: torch.zeros((n, 2), dtype=torch.float32, device=dev) for k in ("chunks_med_mad", "chunks_quantile", "stats_med_mad")}
    u_off = torch.empty(n, dtype=torch.float32, device=dev)
    u_scale = torch.empty(n, dtype=torch.float32, device=dev)
    off16, maxT = off // 2, int(lens.max())

    def chunk_call(key, f, m=None, ss=None):
        b = c._batch(comp, coff, csize, back, off, size32, ress[key])
        b.dst, b.dst_bytes = None, total
        if m is None:
            rc = c.L.vbz_gpu_decompress_chunks_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(ch), first.data_ptr(),
                                                     outs[key].data_ptr(), rows)
        else:
            rc = c.L.vbz_gpu_decompress_chunks_norm_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(ch),
                                                          first.data_ptr(), outs[key].data_ptr(), rows, ctypes.byref(m), ss.data_ptr())
        assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)

    def fmt(o=None, s=None):
        f = _lib.GpuSignalFormat()
        f.out_type, f.is_signed = _lib.VBZ_GPU_SIGNAL_F16, 1
        f.offset, f.scale = (o.data_ptr() if o is not None else None), (s.data_ptr() if s is not None else None)
        return f

    f_given, f_none, f_unf = fmt(o_t, s_t), fmt(), fmt(u_off, u_scale)
    mm, qq = batch.MED_MAD.c_struct(), batch.DORADO_QUANTILE.c_struct()

    def stats():
        b = c._batch(comp, coff, csize, back, off, size32, ress["stats_med_mad"])
        b.dst, b.dst_bytes = None, total
        rc = c.L.vbz_gpu_signal_norm_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 0, 1, ctypes.byref(mm), sss["stats_med_mad"].data_ptr())
        assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)

    def unfused():
        c.decompress(comp, coff, csize, back, off, size32, res, opts)
        med, mad = torch_med_mad(back.view(torch.int16), off16, lens, maxT)
        k = torch.tensor(1.4826, dtype=torch.float32).double().item()
        scale = torch.clamp(k * mad, min=batch.FLT_MIN).float()   # (the Bonito constants, rounded as the call rounds them)
        u_off.copy_(-med.float())
        u_scale.copy_((1.0 / scale.double()).float())
        chunk_call("unfused_med_mad", f_unf)

    fns = {"chunks": lambda: chunk_call("chunks", f_given), "chunks_med_mad": lambda: chunk_call("chunks_med_mad", f_none, mm, sss["chunks_med_mad"]),
           "chunks_quantile": lambda: chunk_call("chunks_quantile", f_none, qq, sss["chunks_quantile"]), "stats_med_mad": stats,
           "unfused_med_mad": unfused}
    if only:
        fns = {k: fn for k, fn in fns.items() if k in only}
    ms = timed(c, fns, reps)
    torch.cuda.synchronize()
    row = {"reads": n, "samples": samples, "chunk_len": L_, "step": S_, "rows": rows, "ms": ms}
    if "chunks" in ms:
        for k in ("chunks_med_mad", "chunks_quantile", "stats_med_mad", "unfused_med_mad"):
            if k in ms:
                row[k + "_over_chunks"] = round(ms[k] / ms["chunks"], 3)
    for k in fns:
        assert torch.equal(ress[k].to(torch.int64), lens.to(dev).to(torch.int64) * 2), k   # (float16 and int16: 2 bytes a sample)
    with torch.cuda.stream(c.stream):   # (the checks' torch work in the codec's stream order, as in the timed calls)
        for k in ("chunks_med_mad", "chunks_quantile"):   # == the chunk call fed the constants the normalising call reported
            if k not in fns:
                continue
            ss = sss[k]
            u_off.copy_(-ss[:, 0])
            u_scale.copy_((1.0 / ss[:, 1].double()).float())
            chunk_call("unfused_med_mad", f_unf)
            torch.cuda.synchronize()
            assert torch.equal(outs[k].view(torch.int16), outs["unfused_med_mad"].view(torch.int16)), k
            row["checked_" + k] = True
        if "unfused_med_mad" in fns and "chunks_med_mad" in fns:   # the torch route's constants are the call's
            unfused()
            torch.cuda.synchronize()
            row["unfused_matches"] = bool(torch.equal(outs["chunks_med_mad"].view(torch.int16), outs["unfused_med_mad"].view(torch.int16)))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", action="append", default=[],
                    help="time only these calls (chunks, chunks_med_mad, chunks_quantile, stats_med_mad, unfused_med_mad)")
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    out = {"headline": case(c, c.synth_lengths(5, 0, args.reads), args.reps, args.only, 5)}
    torch.cuda.empty_cache()
    out["one_20M_read"] = case(c, torch.tensor([20_000_000], dtype=torch.int32, device=c.device), args.reps, args.only, 7)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
